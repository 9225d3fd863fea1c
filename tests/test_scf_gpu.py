"""Device restricted Hartree-Fock (auto_oo_amd/scf.py, csrc/scf.hip) against the host ``gaussian.rhf`` and numpy.

Where the bounds come from
- Fock contraction: per element 4 n^2 2^-52 sum|g||D| over that element's terms, the worst-case summation error of two
  orders of an n^2-term sum, computed by the test from the inputs.
- Eigensolver: 1e-12 ||A||_2 for eigenvalues and residuals, 1e-12 for orthonormality: cyclic Jacobi is accurate to a
  small multiple of n 2^-52 ||A|| = 1.4e-14 at n = 64, which leaves a factor of about 70.
- Molecules: |dE| <= 1e-10 Ha (second order in the converged commutator), density matrix 1e-7 (both solvers stop at
  max|e| < 1e-9 with gaps >= 0.467 Ha: a few 1e-9 of rotation on each side, times 10), orbital energies 1e-8,
  C^T S C = I to 1e-12, commutator < 1e-9, iterations within +-3 of the host's count.
Orbitals are never compared column by column (H-F has an exactly degenerate pi pair).
"""
import copy
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import auto_oo_amd as aoo                                   # noqa: E402
from auto_oo_amd import _lib, gaussian, gto, scf            # noqa: E402
from auto_oo_amd.gaussian import Moldata_sto3g              # noqa: E402
from auto_oo_amd.moldata import get_formal_geo              # noqa: E402
from auto_oo_amd.synthetic import synthetic_problem         # noqa: E402
from tests._scf_scope import host_rhf_counted               # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "notebook_runs.json")) as fh:
    BERRY = json.load(fh)["tutorial_berry_phase"]

E_RHF = -92.66372193556138
SIZES = (1, 2, 7, 13, 16, 17, 43, 64)
STACKS = (1, 3, 37)
FORMAL_POINTS = ((140.0, 80.0), (100.0, 0.0), (180.0, 90.0), (125.0, 45.0))
HF = "H 0 0 0; F 0 0 1.1"
WATER = "O 0 0 0; H 0 0.757 0.587; H 0 -0.757 0.587"
WATER_STRETCHED = "O 0 0 0; H 0 1.2 0.9; H 0 -1.2 0.9"


def ring(n=16):
    """n points around the loop of the Berry-phase notebook (the ring of tests/test_gto_gpu.py)."""
    phase = np.pi / BERRY["phase_pi_over"]
    return [(BERRY["origin"][0] + BERRY["radius"][0] * np.cos(2 * np.pi * k / n + phase),
             BERRY["origin"][1] + BERRY["radius"][1] * np.sin(2 * np.pi * k / n + phase)) for k in range(n)]


def formal(p):
    return get_formal_geo(*p)


@functools.lru_cache(maxsize=None)
def formal_basis():
    return gto.GTOBasis(["N", "C", "H", "H", "H"])


def cuda(x):
    return torch.as_tensor(np.array(x, dtype=np.float64)).cuda()


@functools.lru_cache(maxsize=None)
def host_solution(geometry):
    """A molecule on the integrals the device makes for ``geometry`` and its host ``gaussian.rhf`` solution on those
    same integrals, computed once and shared by the tests (the host integral code takes 0.4 s per formaldimine)."""
    symbols, _ = gaussian.zmatrix_to_cartesian(geometry)
    basis = gto.GTOBasis(symbols)
    I = gto.integrals_batch(basis, [geometry])
    mol = aoo.Moldata(I.int1e_ao[0].cpu().numpy(), I.int2e_ao[0].cpu().numpy(), I.overlap[0].cpu().numpy(),
                      I.nuc[0].item(), basis.nelectron)
    n_occ = mol.nelectron // 2
    C, e, e_elec = gaussian.rhf(mol.int1e_ao, mol.int2e_ao, mol.overlap, n_occ)
    C2, e2, e_elec2, count, last, converged = host_rhf_counted(mol.int1e_ao, mol.int2e_ao, mol.overlap, n_occ)
    assert np.array_equal(C, C2) and np.array_equal(e, e2) and e_elec == e_elec2 and converged
    for a in (C, e, mol.int1e_ao, mol.int2e_ao, mol.overlap):
        a.setflags(write=False)
    return dict(mol=mol, n_occ=n_occ, C=C, e=e, e_elec=e_elec, e_tot=e_elec + mol.nuc, iterations=count)


def fock_host(mol, D):
    J = np.einsum("pqrs,rs->pq", mol.int2e_ao, D)
    K = np.einsum("prqs,rs->pq", mol.int2e_ao, D)
    return mol.int1e_ao + J - 0.5 * K


# ---- 1. Fock contraction ------------------------------------------------------------------------------------------
def _random_g_d(n, G, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    g = torch.randn((G, n, n, n, n), generator=gen, dtype=torch.float64, device="cuda")
    D = torch.randn((G, n, n), generator=gen, dtype=torch.float64, device="cuda")
    return g, D


@pytest.mark.parametrize("G", STACKS)
@pytest.mark.parametrize("n", SIZES)
def test_fock_jk_against_einsum(n, G):
    g, D = _random_g_d(n, G, 100 * n + G)          # deliberately without any symmetry
    J, K = scf.fock_jk(g, D)
    J, K = J.cpu().numpy(), K.cpu().numpy()
    worst = 0.0
    for b in range(G):
        gb, Db = g[b].cpu().numpy(), D[b].cpu().numpy()
        Jr = np.einsum("pqrs,rs->pq", gb, Db, optimize=True)
        Kr = np.einsum("prqs,rs->pq", gb, Db, optimize=True)
        ga, Da = np.abs(gb), np.abs(Db)
        scale = 4.0 * n * n * 2.0 ** -52
        Jb = scale * np.einsum("pqrs,rs->pq", ga, Da, optimize=True)
        Kb = scale * np.einsum("prqs,rs->pq", ga, Da, optimize=True)
        worst = max(worst, (np.abs(J[b] - Jr) / Jb).max(), (np.abs(K[b] - Kr) / Kb).max())
        assert (np.abs(J[b] - Jr) <= Jb).all(), f"J of geometry {b}: {np.abs(J[b] - Jr).max()}"
        assert (np.abs(K[b] - Kr) <= Kb).all(), f"K of geometry {b}: {np.abs(K[b] - Kr).max()}"
    print(f"n = {n}, G = {G}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("n,G", [(13, 37), (17, 5), (43, 3), (64, 3)])
def test_fock_jk_of_a_stack_equals_its_geometries_one_by_one_and_permutes(n, G):
    g, D = _random_g_d(n, G, 7 + n)
    J, K = scf.fock_jk(g, D)
    for b in range(G):
        Jb, Kb = scf.fock_jk(g[b], D[b])
        assert torch.equal(Jb, J[b]) and torch.equal(Kb, K[b])
    perm = torch.as_tensor(np.random.default_rng(n).permutation(G)).cuda()
    Jp, Kp = scf.fock_jk(g[perm].contiguous(), D[perm].contiguous())
    assert torch.equal(Jp, J[perm]) and torch.equal(Kp, K[perm])


# ---- 2. eigensolver -----------------------------------------------------------------------------------------------
def _check_eig(A, w, V, label):
    n = A.shape[0]
    norm = max(np.abs(np.linalg.eigvalsh(A)).max(), 1e-300)
    w_ref = np.linalg.eigh(A)[0]
    d_w = np.abs(w - w_ref).max() / norm
    d_r = np.abs(A @ V - V * w[None, :]).max() / norm
    d_o = np.abs(V.T @ V - np.eye(n)).max()
    print(f"{label}: eigenvalues {d_w:.2e}, residual {d_r:.2e}, orthonormality {d_o:.2e}")
    assert d_w <= 1e-12 and d_r <= 1e-12 and d_o <= 1e-12
    assert (np.diff(w) >= 0).all()
    for j in range(n):                     # the component of largest magnitude is positive, the first one on ties
        assert V[np.argmax(np.abs(V[:, j])), j] > 0


@pytest.mark.parametrize("n", SIZES)
def test_sym_eigh_against_numpy(n):
    rng = np.random.default_rng(n)
    mats = []
    for _ in range(3):
        a = rng.standard_normal((n, n))
        mats.append(0.5 * (a + a.T))
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = rng.uniform(-2.0, 2.0, n)
    if n > 2:
        lam[1] = lam[n - 1] = lam[0]       # a repeated eigenvalue
    rep = (q * lam) @ q.T
    mats.append(0.5 * (rep + rep.T))
    mats.append(np.diag(rng.uniform(-3.0, 3.0, n)))        # already diagonal
    w, V, info = scf.sym_eigh_batch(cuda(np.stack(mats)))
    assert info.cpu().tolist() == [0] * len(mats)
    w, V = w.cpu().numpy(), V.cpu().numpy()
    for k, A in enumerate(mats):
        _check_eig(A, w[k], V[k], f"n = {n}, matrix {k}")
    w1, V1, _ = scf.sym_eigh_batch(cuda(mats[0]))
    assert np.array_equal(w1.cpu().numpy(), w[0]) and np.array_equal(V1.cpu().numpy(), V[0])


def test_sym_eigh_flags_a_matrix_that_is_not_finite():
    a = np.stack([np.eye(5), np.eye(5), np.eye(5)])
    a[1, 3, 2] = np.nan
    w, V, info = scf.sym_eigh_batch(cuda(a))
    assert info.cpu().tolist() == [0, -3, 0]
    assert torch.isnan(w[1]).all() and torch.isnan(V[1]).all()
    assert torch.equal(w[0], torch.ones(5, dtype=torch.float64).cuda()) and torch.equal(w[2], w[0])


# ---- 3. molecules against the host solver -------------------------------------------------------------------------
def _compare_with_host(res, k, sol, label):
    mol, n_occ = sol["mol"], sol["n_occ"]
    pick = (lambda t: t.cpu().numpy()) if k is None else (lambda t: t[k].cpu().numpy())
    C, c, eps = pick(res.mo_coeff), pick(res.oao_mo_coeff), pick(res.mo_energy)
    e_elec, iters = float(pick(res.e_elec)), int(pick(res.iterations))
    S = mol.overlap
    D = 2.0 * C[:, :n_occ] @ C[:, :n_occ].T
    D_ref = 2.0 * sol["C"][:, :n_occ] @ sol["C"][:, :n_occ].T
    F = fock_host(mol, D)
    comm = np.abs(F @ D @ S - S @ D @ F).max()
    d_e, d_d, d_eps = abs(e_elec - sol["e_elec"]), np.abs(D - D_ref).max(), np.abs(eps - sol["e"]).max()
    d_o = np.abs(C.T @ S @ C - np.eye(mol.nao)).max()
    print(f"{label}: |dE| {d_e:.2e}, |dD| {d_d:.2e}, |deps| {d_eps:.2e}, |C^T S C - 1| {d_o:.2e}, commutator "
          f"{comm:.2e}, iterations {iters} (host {sol['iterations']})")
    assert bool(pick(res.converged)) and int(pick(res.info)) == 0
    assert d_e <= 1e-10
    assert d_d <= 1e-7
    assert d_eps <= 1e-8
    assert d_o <= 1e-12
    assert comm < 1e-9
    assert abs(iters - sol["iterations"]) <= 3
    assert float(pick(res.diis_error)) < 1e-9
    # oao_mo_coeff is the eigenvector matrix itself: orthogonal, and S^-1/2 times it gives mo_coeff
    assert np.abs(c.T @ c - np.eye(mol.nao)).max() <= 1e-12
    assert np.abs(mol.oao_coeff @ c - C).max() <= 1e-10


def _solve_stack(geometries):
    sols = [host_solution(g) for g in geometries]
    mols = [s["mol"] for s in sols]
    res = scf.rhf_batch(cuda(np.stack([m.int1e_ao for m in mols])), cuda(np.stack([m.int2e_ao for m in mols])),
                        cuda(np.stack([m.overlap for m in mols])), sols[0]["n_occ"])
    return res, sols


def test_formaldimine_stack_against_the_host_solver():
    geos = [formal(p) for p in FORMAL_POINTS]
    res, sols = _solve_stack(geos)
    for k, sol in enumerate(sols):
        _compare_with_host(res, k, sol, f"formaldimine {FORMAL_POINTS[k]}")
    e_tot = res.e_elec[0].item() + sols[0]["mol"].nuc
    print("E_tot (140, 80)", e_tot, "literal", E_RHF)
    assert abs(e_tot - E_RHF) <= 1e-9


def test_ring_stack_against_the_host_solver():
    geos = [formal(p) for p in ring()]
    res, sols = _solve_stack(geos)
    for k, sol in enumerate(sols):
        _compare_with_host(res, k, sol, f"ring point {k}")


@pytest.mark.parametrize("geometry", [HF, WATER, WATER_STRETCHED], ids=["HF", "water", "water-stretched"])
def test_single_molecules_against_the_host_solver(geometry):
    sol = host_solution(geometry)
    mol = sol["mol"]
    res = scf.rhf_batch(cuda(mol.int1e_ao), cuda(mol.int2e_ao), cuda(mol.overlap), sol["n_occ"])
    assert res.mo_coeff.shape == (mol.nao, mol.nao) and res.e_elec.dim() == 0
    _compare_with_host(res, None, sol, geometry)
    # S^-1/2 handed in instead of made by the call: the same solution
    res2 = scf.rhf_batch(cuda(mol.int1e_ao), cuda(mol.int2e_ao), cuda(mol.overlap), sol["n_occ"],
                         oao_coeff=cuda(mol.oao_coeff))
    _compare_with_host(res2, None, sol, geometry + " (S^-1/2 given)")


# ---- 4. self-consistency at N = 43 --------------------------------------------------------------------------------
SYN_SEEDS = tuple(range(1000, 1006))


@functools.lru_cache(maxsize=None)
def synthetic_stack():
    P = [synthetic_problem(43, s) for s in SYN_SEEDS]
    h, g, S = (cuda(np.stack([p[k] for p in P])) for k in ("int1e_ao", "int2e_ao", "overlap"))
    return P, h, g, S


def _host_commutator(p, C, n_occ):
    D = 2.0 * C[:, :n_occ] @ C[:, :n_occ].T
    J = np.einsum("pqrs,rs->pq", p["int2e_ao"], D, optimize=True)
    K = np.einsum("prqs,rs->pq", p["int2e_ao"], D, optimize=True)
    F = p["int1e_ao"] + J - 0.5 * K
    return np.abs(F @ D @ p["overlap"] - p["overlap"] @ D @ F).max(), D, F


def test_synthetic_n43_solutions_are_self_consistent():
    """These problems are not physical and may have several solutions, so nothing is compared with the host's
    energies.  The commutator that must be below ``err_tol`` is the one the convergence test saw, i.e. that of the
    density that entered the last iteration: the solver (like ``gaussian.rhf``) returns the orbitals of one more DIIS
    step, and for these slowly converging problems (67-114 iterations) that step can leave the commutator slightly
    above the threshold -- the host routine's own orbitals for seed 1003 have 2.66e-9, the device's 2.66e-9.  So the
    density of the last iteration is obtained from a run stopped one iteration earlier, its commutator is recomputed
    on the host, and must be below ``err_tol`` and equal to the reported ``diis_error``; the commutator of the final
    orbitals is printed and held to 10 x ``err_tol``."""
    P, h, g, S = synthetic_stack()
    n_occ = 8
    res = scf.rhf_batch(h, g, S, n_occ)
    iters = res.iterations.cpu().tolist()
    print("iterations", iters, "diis_error", res.diis_error.cpu().tolist())
    assert res.converged.cpu().tolist() == [True] * len(P)
    assert (res.diis_error < 1e-9).all().item()
    for k, p in enumerate(P):
        C, eps, E = res.mo_coeff[k].cpu().numpy(), res.mo_energy[k].cpu().numpy(), res.e_elec[k].item()
        before = scf.rhf_batch(h[k], g[k], S[k], n_occ, max_cycle=iters[k] - 1)
        assert before.info.item() == 1 and before.iterations.item() == iters[k] - 1
        seen, D_seen, F_seen = _host_commutator(p, before.mo_coeff.cpu().numpy(), n_occ)
        comm, D, F = _host_commutator(p, C, n_occ)
        d_o = np.abs(C.T @ p["overlap"] @ C - np.eye(43)).max()
        e_host = 0.5 * np.sum(D_seen * (p["int1e_ao"] + F_seen))
        print(f"seed {SYN_SEEDS[k]}: commutator at the convergence test {seen:.3e} (reported "
              f"{res.diis_error[k].item():.3e}), of the returned orbitals {comm:.2e}, orthonormality {d_o:.2e}, "
              f"|E - E(D)| {abs(E - e_host):.2e}")
        assert seen < 1e-9 and abs(seen - res.diis_error[k].item()) <= 1e-12
        assert comm < 1e-8
        assert d_o <= 1e-12
        assert (np.diff(eps) >= 0).all()                                   # aufbau: the occupied ones are the lowest
        assert abs(E - e_host) <= 1e-10 * abs(E)                           # E = 1/2 sum D (h + F) of that density


def test_synthetic_n43_stack_equals_its_geometries_one_by_one():
    P, h, g, S = synthetic_stack()
    res = scf.rhf_batch(h, g, S, 8)
    for k in range(len(P)):
        one = scf.rhf_batch(h[k], g[k], S[k], 8)
        for name in scf._RHF_FIELDS:
            assert torch.equal(getattr(one, name), getattr(res, name)[k]), f"{name} of seed {SYN_SEEDS[k]}"


# ---- 5. failures are reported -------------------------------------------------------------------------------------
def test_max_cycle_is_reported_and_the_neighbour_is_unaffected():
    P = [synthetic_problem(20, s) for s in (1000, 1001)]
    h, g, S = (cuda(np.stack([p[k] for p in P])) for k in ("int1e_ao", "int2e_ao", "overlap"))
    res = scf.rhf_batch(h, g, S, 5, max_cycle=30)
    print("info", res.info.cpu().tolist(), "iterations", res.iterations.cpu().tolist())
    assert res.info[0].item() == 1 and not res.converged[0].item() and res.iterations[0].item() == 30
    solo = scf.rhf_batch(h[1], g[1], S[1], 5, max_cycle=30)
    for name in scf._RHF_FIELDS:
        assert torch.equal(getattr(solo, name), getattr(res, name)[1]), name


def test_a_nan_in_one_core_hamiltonian_is_reported_for_that_geometry_only():
    geos = [formal(p) for p in FORMAL_POINTS[:3]]
    sols = [host_solution(g) for g in geos]
    mols = [s["mol"] for s in sols]
    h = np.stack([m.int1e_ao for m in mols])
    h[1, 2, 5] = np.nan
    g, S = cuda(np.stack([m.int2e_ao for m in mols])), cuda(np.stack([m.overlap for m in mols]))
    res = scf.rhf_batch(cuda(h), g, S, 8)
    assert res.info.cpu().tolist() == [0, -3, 0] and res.converged.cpu().tolist() == [True, False, True]
    assert torch.isnan(res.mo_coeff[1]).all() and torch.isnan(res.e_elec[1])
    for k in (0, 2):
        _compare_with_host(res, k, sols[k], f"neighbour {k} of the NaN")
    # ... and in the two-electron integrals
    gn = g.clone()
    gn[2, 1, 1, 4, 0] = float("inf")
    res = scf.rhf_batch(cuda(np.stack([m.int1e_ao for m in mols])), gn, S, 8)
    assert res.info.cpu().tolist() == [0, 0, -3]
    _compare_with_host(res, 0, sols[0], "neighbour 0 of the Inf")


def test_two_atoms_on_top_of_each_other_are_reported():
    basis = formal_basis()
    xyz = basis.coordinates([formal(FORMAL_POINTS[0]), formal(FORMAL_POINTS[0])])
    xyz[1, 3] = xyz[1, 2]                                  # the two hydrogens of the carbon coincide
    I = gto.integrals_batch(basis, xyz, check_overlap=False)
    res = scf.rhf_batch(I.int1e_ao, I.int2e_ao, I.overlap, 8)
    assert res.info.cpu().tolist() == [0, -1] and res.converged.cpu().tolist() == [True, False]
    assert torch.isnan(res.mo_coeff[1]).all()
    assert abs(res.e_elec[0].item() + I.nuc[0].item() - E_RHF) <= 1e-9


def test_what_is_out_of_scope_raises_before_any_launch():
    z = lambda *s: torch.zeros(s, dtype=torch.float64).cuda()          # noqa: E731
    with pytest.raises(ValueError, match="N = 65"):
        scf.rhf_batch(z(65, 65), z(1, 1, 1, 1), z(65, 65), 3)
    with pytest.raises(ValueError, match="n_occ"):
        scf.rhf_batch(z(4, 4), z(4, 4, 4, 4), z(4, 4), 4)
    with pytest.raises(ValueError, match="n_occ"):
        scf.rhf_batch(z(4, 4), z(4, 4, 4, 4), z(4, 4), 0)
    mol = host_solution(HF)["mol"]
    odd = aoo.Moldata(mol.int1e_ao, mol.int2e_ao, mol.overlap, mol.nuc, mol.nelectron - 1)
    with pytest.raises(ValueError, match="even electron count"):
        odd.run_rhf(device=True)
    lib = _lib.load()
    assert lib.oovqe_rhf_work_size(65, 1) < 0 and lib.oovqe_rhf_work_size(13, 0) < 0


# ---- 6. wiring ----------------------------------------------------------------------------------------------------
def np_fabric():
    return aoo.Parameterized_circuit(2, 2, None, ansatz="np_fabric", n_layers=1)


def _host_orbitals(geometry):
    sol = host_solution(geometry)
    return aoo.mo_ao_to_mo_oao(sol["C"], sol["mol"].overlap)


def _forbid_host_rhf(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the host gaussian.rhf was called")
    monkeypatch.setattr(aoo.batch, "rhf", refuse)


def _check_batch_against_host(batch, geos, rows, label):
    zeros = torch.zeros((batch.G, batch.n_theta), dtype=torch.float64)
    E0 = batch.energy(zeros).cpu().numpy()
    e_ci = batch.casci()[0].cpu().numpy()[:, 0]
    ref = aoo.OO_pqc_batch.from_geometries(np_fabric(), formal_basis(), geos, 2, 2,
                                           oao_mo_coeffs=[_host_orbitals(g) for g in geos], freeze_active=True)
    e_ci_ref = ref.casci()[0].cpu().numpy()[:, 0]
    for k, (r, geo) in enumerate(zip(rows, geos)):
        d0, d1 = abs(E0[r] - host_solution(geo)["e_tot"]), abs(e_ci[r] - e_ci_ref[k])
        print(f"{label} row {r}: |E(theta = 0) - E_RHF| {d0:.2e}, |dE_CASCI| {d1:.2e}")
        assert d0 <= 1e-9 and d1 <= 1e-9


def test_from_geometries_and_set_geometries_with_device_rhf_orbitals(monkeypatch):
    _forbid_host_rhf(monkeypatch)
    pts = ring()
    geos = [formal(p) for p in pts]
    batch = aoo.OO_pqc_batch.from_geometries(np_fabric(), formal_basis(), geos, 2, 2, oao_mo_coeffs="rhf",
                                             freeze_active=True)
    _check_batch_against_host(batch, geos, range(16), "from_geometries")
    r = batch.rhf()
    assert r.converged.all().item()
    assert np.abs(r.e_tot.cpu().numpy() - np.array([host_solution(g)["e_tot"] for g in geos])).max() <= 1e-9
    # every row moves on to the next point of the ring
    nxt = geos[1:] + geos[:1]
    batch.set_geometries(nxt, oao_mo_coeffs="rhf")
    _check_batch_against_host(batch, nxt, range(16), "set_geometries")
    # with an index the other rows keep their bits
    before = {k: getattr(batch, k).clone() for k in ("oao_mo_coeff", "mo_coeff", "int1e_ao", "oao_coeff")}
    batch.set_geometries([geos[3], geos[9]], index=[3, 9], oao_mo_coeffs="rhf")
    others = [k for k in range(16) if k not in (3, 9)]
    for name, old in before.items():
        assert torch.equal(getattr(batch, name)[others], old[others]), name
    mixed = [geos[k] if k in (3, 9) else nxt[k] for k in range(16)]
    _check_batch_against_host(batch, [mixed[3], mixed[9]], [3, 9], "set_geometries(index)")
    with pytest.raises(ValueError):
        batch.set_geometries(nxt, oao_mo_coeffs="uhf")


def test_a_geometry_that_does_not_converge_is_named(monkeypatch):
    batch = aoo.OO_pqc_batch.from_geometries(np_fabric(), formal_basis(), [formal(p) for p in FORMAL_POINTS[:2]], 2, 2,
                                             oao_mo_coeffs="rhf", freeze_active=True)
    r = batch.rhf(index=[1], max_cycle=2)
    assert r.info.cpu().tolist() == [1] and r.iterations.cpu().tolist() == [2]
    monkeypatch.setattr(scf, "rhf_batch", functools.partial(scf.rhf_batch, max_cycle=2))
    with pytest.raises(_lib.OovqeError, match=r"geometries 0 .*1 "):
        batch.set_geometries([formal(p) for p in FORMAL_POINTS[2:]], oao_mo_coeffs="rhf")


def test_run_rhf_on_the_device():
    geo = formal(FORMAL_POINTS[0])
    m = Moldata_sto3g(geo)
    m2 = copy.copy(m)
    m2.run_rhf()                                            # the default of Moldata_sto3g is still the host solver
    C, e, e_elec = gaussian.rhf(m.int1e_ao, m.int2e_ao, m.overlap, 8)
    assert np.array_equal(m2.hf.mo_coeff, C) and m2.hf.e_tot == e_elec + m.nuc
    m.run_rhf(device=True)
    print("Moldata_sto3g device RHF", m.hf.e_tot, "host", m2.hf.e_tot)
    assert abs(m.hf.e_tot - m2.hf.e_tot) <= 1e-10 and m.hf.converged
    assert np.abs(m.hf.mo_energy - e).max() <= 1e-8
    plain = aoo.Moldata(m.int1e_ao, m.int2e_ao, m.overlap, m.nuc, m.nelectron)
    with pytest.raises(RuntimeError):
        plain.run_rhf()
    plain.run_rhf(device=True)
    assert plain.hf.e_tot == m.hf.e_tot and np.array_equal(plain.hf.mo_coeff, m.hf.mo_coeff)
    assert np.array_equal(plain.hf.mo_energy, m.hf.mo_energy) and plain.hf.converged
