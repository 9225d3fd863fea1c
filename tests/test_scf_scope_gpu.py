"""The iterative solvers over their whole scope, n = 2 .. 64 and 1 <= n_occ < n: ``scf.sym_eigh_batch``,
``scf.rhf_batch`` (csrc/scf.hip, csrc/jacobi.h), ``nucgrad.zvector`` and ``nucgrad.response_d2`` (csrc/zvector.hip)
against numpy, the host twin ``gaussian.rhf`` and the dense solve of the virt-occ Hessian on the gapped family of
tests/_scf_scope.py, which says where the problems and the references come from; tests/test_scf_scope_cpu.py holds the
references against each other and asserts the conditions every problem used here must meet.

Bounds (nothing in one comes from the device's output):
  * eigensolver: those of ``_check_eig`` in tests/test_scf_gpu.py, 1e-12 ||A||_2 for eigenvalues and residuals, 1e-12
    for orthonormality; the cluster 1 + j 1e-13 by residual and orthonormality only.
  * RHF: those of ``_compare_with_host`` in tests/test_scf_gpu.py, with |dE| relative to max(1, |E|), the commutator of
    the returned orbitals below 10 err_tol, and the density bound ``_scf_scope.density_bound`` per problem in place of
    the molecules' 1e-7.  Orbital energies are printed, not asserted, on the grid (they are first order in the density
    error); the g = 0 tests hold them to 1e-10 at every n.
  * Z-vector: ``_scf_scope.z_error_bound`` in the 2-norm per set, residual <= tol, iterations within +-3 of
    ``_scf_scope.host_pcg`` on the host matrix.
  * response_d2: 10 x 8 x 2^-52 x (max |d2| + 3 max |Z| max |D0|): six products and one subtraction per element.

No defect was found: every test passed on its first run, and the thresholds of ``sym_jacobi_wave`` stay as they are (the
matrices scaled by 1e-100 and 1e+100 are solved like those of norm 1).  Measured on an MI355X (one run):

  eigensolver, largest of (eigenvalues, residual, orthonormality) over the nine matrices: n = 2 3.3e-16, n = 3 8.5e-16,
    n = 16 7.1e-15, n = 17 7.6e-15, n = 62 .. 64 at most 4.7e-14 (bound 1e-12); the scaled matrices as the others.
  RHF grid, 33 problems: the iteration count is the host's in 30, 7 / 6 at (2, 1) seed 2, 16 / 17 at (3, 2) seed 2 and
    17 / 14 at (2, 1) seed 3 (its commutator has one independent element, so the eight-vector DIIS system has rank 1);
    |dE| at most 5.8e-12 at E = -284 (bound 2.8e-8), |dD| at most 5.6e-14 for n >= 13 and 4.1e-9 at (2, 1) seed 3
    (bounds 2e-8 .. 5e-7), |deps| at most 1.2e-13 for n >= 13 and 2.5e-8 at (2, 1) seed 3, C^T S C - 1 at most 2.6e-14,
    commutator of the returned orbitals at most 1.01e-9 ((33, 16) hard seed 2).
  g = 0: 2 iterations at every n, E within 1.8e-14 relative, mo_energy within 6.7e-14; diagonal h: commutator exactly 0.
  max_cycle at (13, 6) hard: 16 iterations, as the host; easy / hard / easy at (33, 16): 9, 30, 9.
  Z-vector grid, largest error / bound per problem 0.04 .. 0.60, the iteration count within 1 of ``host_pcg``, every
    residual <= 1e-10 (largest 9.8e-11); LDS of the step kernel 113.6 KB at (64, 32), 102.2 KB at (64, 5), 98.5 KB at
    (64, 63); the ten scaled sets finish after 6, 8, 11, 13, 0, 14, 16, 17, 18, 20 iterations.
  response_d2: error 3.6e-15 (n = 22, 23), 7.1e-15 (n = 33, 64); bounds 1.4e-12 .. 1.8e-12.
  slowest cases 5 s (the RHF grid at n = 64: two host solutions of 2 s each), the file 38 s.

(23, 12) has 11 x 12 = 132 virt-occ unknowns; the first shape at which a thread of the step kernel takes a second one
is (33, 16) with 272, which the grid, the hard case and the sets test run.

Mutation check (scratch copies of the kernels, one edit each, this file against each library):
  * ``k < min(nvo, ZV_NT)`` in the update loop of ``zvector_step_kernel``: red in the Z-vector grid at (33, 16) firm
    and hard, (64, 32), (64, 5) and in the sets test.
  * ``break`` in place of ``rs += ZV_NT`` in ``response_d2_kernel``: red at n = 23, 33, 64 (green at 22: 253 pairs).
  * ``slot = (it + 1) % SCF_HIST`` in ``scf_step_kernel``: red in all 39 RHF tests.
  * ``ld = n`` in ``zvector_step_kernel``: green, and no test can tell: ``ld`` is only the row pitch of the kernel's own
    LDS matrices, used consistently, and the launch reserves the larger ``n | 1`` pitch; the edit changes bank
    conflicts, not values.
  * the pivot test of the DIIS solve removed: green, and no test can tell: a zero pivot then divides by zero, every
    row below it (or the last unknown) becomes Inf or NaN, and the back substitution's ``isfinite`` test rejects the
    weights, which is what the pivot test did.  ``test_diis_exactly_singular_keeps_the_plain_fock_matrix`` runs that path.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.linalg
import torch

pytestmark = pytest.mark.gpu

from auto_oo_amd import _lib, nucgrad, scf                  # noqa: E402
from auto_oo_amd._lib import check, dptr, stream_ptr        # noqa: E402
from tests import _response_scope as R                      # noqa: E402
from tests import _scf_scope as V                           # noqa: E402

F64 = torch.float64


def dev():
    return torch.device("cuda", 0)


def cuda(x):
    return torch.as_tensor(np.array(x, dtype=np.float64)).to(dev())


def stack_id(s):
    return "{}-{}-{}".format(*s[:3])


def same_bits(a, b):
    """Bit equality of two tensors, NaN equal to NaN."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.nan_to_num(a.to(F64), nan=-7.25e300),
                                                                     torch.nan_to_num(b.to(F64), nan=-7.25e300))


# ---- 1. eigensolver ----------------------------------------------------------------------------------------------------
EIG_SIZES = (1, 2, 3, 16, 17, 62, 63, 64)
EIG_NAMES = ("graded", "cluster", "ones", "projector", "zero", "tau = 0 blocks", "ties", "1e-100", "1e+100")


def eig_matrices(n):
    rng = np.random.default_rng(4000 + n)
    sym = lambda a: 0.5 * (a + a.T)                                                     # noqa: E731
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    d = 10.0 ** (-12.0 * np.arange(n) / max(n - 1, 1))
    graded = d[:, None] * sym(q) * d[None, :]
    cluster = sym((q * (1.0 + 1e-13 * np.arange(n))) @ q.T)
    ones = np.ones((n, n))
    projector = sym(q[:, :n // 2] @ q[:, :n // 2].T)
    blocks = np.zeros((n, n))
    m = n - (n & 1)
    blocks[:m, :m] = np.kron(np.eye(m // 2), np.array([[0.0, 1.0], [1.0, 0.0]]))
    ties = np.diag(np.array([1.0, 1.0] + [0.0] * n)[:n])
    small = 1e-100 * sym(rng.standard_normal((n, n)))
    large = 1e+100 * sym(rng.standard_normal((n, n)))
    return [graded, cluster, ones, projector, np.zeros((n, n)), blocks, ties, small, large]


def check_eig(A, w, V_, label, eigenvalues=True):
    """``_check_eig`` of tests/test_scf_gpu.py; ``eigenvalues=False`` leaves the eigenvalue comparison out."""
    n = A.shape[0]
    norm = max(np.abs(np.linalg.eigvalsh(A)).max(), 1e-300)
    w_ref = np.linalg.eigh(A)[0]
    d_w = np.abs(w - w_ref).max() / norm
    d_r = np.abs(A @ V_ - V_ * w[None, :]).max() / norm
    d_o = np.abs(V_.T @ V_ - np.eye(n)).max()
    print(f"{label}: eigenvalues {d_w:.2e}, residual {d_r:.2e}, orthonormality {d_o:.2e}")
    assert (d_w <= 1e-12 or not eigenvalues) and d_r <= 1e-12 and d_o <= 1e-12
    assert (np.diff(w) >= 0).all()
    for j in range(n):                     # the component of largest magnitude is positive, the first one on ties
        assert V_[np.argmax(np.abs(V_[:, j])), j] > 0


@pytest.mark.parametrize("n", EIG_SIZES)
def test_sym_eigh_on_graded_clustered_low_rank_zero_and_scaled_matrices_in_one_stack(n):
    mats = eig_matrices(n)
    w, U, info = scf.sym_eigh_batch(cuda(np.stack(mats)))
    assert info.cpu().tolist() == [0] * len(mats)
    wh, Uh = w.cpu().numpy(), U.cpu().numpy()
    for k, (name, A) in enumerate(zip(EIG_NAMES, mats)):
        check_eig(A, wh[k], Uh[k], f"n = {n}, {name}", eigenvalues=name != "cluster")
    # exact ties: ascending, equal eigenvalues in the order of their columns, unit vectors with positive sign
    k = EIG_NAMES.index("ties")
    order = list(range(2, n)) + list(range(min(2, n)))
    assert np.array_equal(wh[k], np.diag(mats[k])[order])
    assert np.array_equal(Uh[k], np.eye(n)[:, order])
    assert np.array_equal(wh[EIG_NAMES.index("zero")], np.zeros(n))
    assert np.array_equal(Uh[EIG_NAMES.index("zero")], np.eye(n))
    # a matrix does not depend on its neighbours
    for k, A in enumerate(mats):
        w1, U1, i1 = scf.sym_eigh_batch(cuda(A))
        assert torch.equal(w1, w[k]) and torch.equal(U1, U[k]) and i1.item() == 0, EIG_NAMES[k]


# ---- 2. RHF: the scope grid against the host twin --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rhf_inputs(n, n_occ, setting, seeds):
    """(h, g, S) of a stack on the device, made once."""
    P = [V.problem(n, n_occ, s, setting) for s in seeds]
    return tuple(cuda(np.stack([p[k] for p in P])) for k in ("int1e_ao", "int2e_ao", "overlap"))


@functools.lru_cache(maxsize=None)
def rhf_stack(n, n_occ, setting, seeds):
    h, g, S = rhf_inputs(n, n_occ, setting, seeds)
    return scf.rhf_batch(h, g, S, n_occ)


def assert_same_result(one, res, k, label):
    for name in scf._RHF_FIELDS:
        want = getattr(res, name) if k is None else getattr(res, name)[k]
        assert same_bits(getattr(one, name), want), f"{name} of {label}"


def compare_with_host(res, k, sol, g, label, err_tol=V.ERR_TOL):
    """``_compare_with_host`` of tests/test_scf_gpu.py for a problem of the family: the density bound is computed
    from the host solution, the energy bound is relative above 1, and the commutator of the returned orbitals is held
    to 10 err_tol (they are those of one more DIIS step than the convergence test saw)."""
    mol, n_occ = sol["mol"], sol["n_occ"]
    pick = lambda t: t[k].cpu().numpy()                                                 # noqa: E731
    C, c, eps = pick(res.mo_coeff), pick(res.oao_mo_coeff), pick(res.mo_energy)
    e_elec, iters = float(pick(res.e_elec)), int(pick(res.iterations))
    S = mol.overlap
    D = 2.0 * C[:, :n_occ] @ C[:, :n_occ].T
    D_ref = 2.0 * sol["C"][:, :n_occ] @ sol["C"][:, :n_occ].T
    F = V.fock_host(mol.int1e_ao, g, D)
    comm = np.abs(F @ D @ S - S @ D @ F).max()
    d_e, d_d, d_eps = abs(e_elec - sol["e_elec"]), np.abs(D - D_ref).max(), np.abs(eps - sol["e"]).max()
    d_o = np.abs(C.T @ S @ C - np.eye(mol.nao)).max()
    bound_d = V.density_bound(sol, err_tol)
    print(f"{label}: |dE| {d_e:.2e} (E {sol['e_elec']:.3f}), |dD| {d_d:.2e} (bound {bound_d:.2e}: lambda_min(A) "
          f"{sol['lam_min']:.3f}, lambda_min(S) {sol['lam_s']:.3f}), |deps| {d_eps:.2e}, |C^T S C - 1| {d_o:.2e}, "
          f"commutator {comm:.2e}, iterations {iters} (host {sol['iterations']})")
    assert bool(pick(res.converged)) and int(pick(res.info)) == 0
    assert d_e <= 1e-10 * max(1.0, abs(sol["e_elec"]))
    assert d_d <= bound_d
    assert d_o <= 1e-12
    assert comm < 10.0 * err_tol
    assert abs(iters - sol["iterations"]) <= 3
    assert float(pick(res.diis_error)) < err_tol
    assert (np.diff(eps) >= 0).all()
    # oao_mo_coeff is the eigenvector matrix itself: orthogonal, and S^-1/2 times it gives mo_coeff
    assert np.abs(c.T @ c - np.eye(mol.nao)).max() <= 1e-12
    assert np.abs(mol.oao_coeff @ c - C).max() <= 1e-10


@pytest.mark.parametrize("stack", V.rhf_stacks(), ids=stack_id)
def test_rhf_scope_grid_against_the_host_twin(stack):
    n, n_occ, setting, seeds = stack
    res = rhf_stack(*stack)
    g = rhf_inputs(*stack)[1]
    for k, seed in enumerate(seeds):
        sol = V.host_solution(n, n_occ, seed, setting)
        compare_with_host(res, k, sol, g[k].cpu().numpy(), f"({n}, {n_occ}) {setting} seed {seed}")


@pytest.mark.parametrize("stack", V.rhf_stacks(), ids=stack_id)
def test_rhf_every_geometry_alone_and_the_stack_permuted_have_the_bits_of_the_stack(stack):
    n, n_occ, setting, seeds = stack
    h, g, S = rhf_inputs(*stack)
    res = rhf_stack(*stack)
    for k, seed in enumerate(seeds):
        assert_same_result(scf.rhf_batch(h[k], g[k], S[k], n_occ), res, k, f"seed {seed} alone")
    perm = list(range(1, len(seeds))) + [0]
    rp = scf.rhf_batch(h[perm].contiguous(), g[perm].contiguous(), S[perm].contiguous(), n_occ)
    for j, k in enumerate(perm):
        assert_same_result(scf.RHFResult(*(getattr(rp, name)[j] for name in scf._RHF_FIELDS)), res, k,
                           f"seed {seeds[k]} at place {j}")
    print(f"({n}, {n_occ}) {setting}: iterations {res.iterations.cpu().tolist()}")


# ---- 3. RHF: the DIIS system at its limits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_occ", [(13, 6), (64, 32)])
def test_diis_exactly_singular_keeps_the_plain_fock_matrix(n, n_occ):
    """h diagonal with distinct levels, S = 1, g = 0: every commutator is exactly zero, B = 0, the bordered system is
    singular and the plain F must be kept."""
    levels = np.random.default_rng(n).permutation(np.concatenate([np.linspace(-3.0, -1.0, n_occ),
                                                                  np.linspace(-0.4, 2.6, n - n_occ)]))
    zero = torch.zeros((n, n, n, n), dtype=F64, device=dev())
    res = scf.rhf_batch(cuda(np.diag(levels)), zero, cuda(np.eye(n)), n_occ)
    order = np.argsort(levels)
    want = 2.0 * np.sort(levels)[:n_occ].sum()
    E = res.e_elec.item()
    print(f"n = {n}: info {res.info.item()}, iterations {res.iterations.item()}, commutator {res.diis_error.item():.1e}, "
          f"E relative {abs(E - want) / abs(want):.1e}")
    assert res.info.item() == 0 and res.iterations.item() == 2 and res.diis_error.item() == 0.0
    assert abs(E - want) <= 1e-14 * abs(want)
    assert np.array_equal(res.mo_coeff.cpu().numpy(), np.eye(n)[:, order])
    assert np.array_equal(res.mo_energy.cpu().numpy(), levels[order])


@pytest.mark.parametrize("n,n_occ", V.NEARLY_SINGULAR_PAIRS)
def test_diis_nearly_singular_returns_the_generalised_eigenvalues(n, n_occ):
    """g = 0 with h and S of the family: the second commutator is rounding noise, B has size 1e-29 and the device
    solves the bordered system with its own elimination; weights that do not sum to 1 would rescale F."""
    P = V.problem(n, n_occ, 1, "firm")
    h, S = P["int1e_ao"], P["overlap"]
    zero = torch.zeros((n, n, n, n), dtype=F64, device=dev())
    res = scf.rhf_batch(cuda(h), zero, cuda(S), n_occ)
    ref = scipy.linalg.eigh(h, S, eigvals_only=True)
    want = 2.0 * ref[:n_occ].sum()
    d_e = abs(res.e_elec.item() - want) / abs(want)
    d_eps = np.abs(res.mo_energy.cpu().numpy() - ref).max()
    print(f"n = {n}: info {res.info.item()}, iterations {res.iterations.item()}, commutator {res.diis_error.item():.1e}, "
          f"E relative {d_e:.1e}, mo_energy {d_eps:.1e}")
    assert res.info.item() == 0 and res.iterations.item() == 2
    assert d_e <= 1e-12 and d_eps <= 1e-10


# ---- 4. RHF: max_cycle, frozen geometries, the synchronous driver -----------------------------------------------------------
HARD = (13, 6, "hard", (1,))


def test_max_cycle_on_either_side_of_the_check_interval_and_of_convergence():
    n, n_occ = HARD[:2]
    h, g, S = (t[0] for t in rhf_inputs(*HARD))
    full = scf.rhf_batch(h, g, S, n_occ)
    k = full.iterations.item()
    print(f"the device needs {k} iterations (host {V.host_solution(n, n_occ, 1, 'hard')['iterations']})")
    assert full.info.item() == 0 and k > 6
    for mc in (1, 3, 4, 5, k - 1):
        r = scf.rhf_batch(h, g, S, n_occ, max_cycle=mc)
        assert r.info.item() == 1 and r.iterations.item() == mc and not r.converged.item(), mc
        assert torch.isfinite(r.mo_coeff).all() and torch.isfinite(r.e_elec)
    for mc in (k, k + 1, k + 4):
        assert_same_result(scf.rhf_batch(h, g, S, n_occ, max_cycle=mc), full, None, f"max_cycle = {mc}")


def test_an_easy_problem_stays_frozen_beside_a_hard_one():
    n, n_occ = 33, 16
    easy, hard = (n, n_occ, "easy", (1,)), (n, n_occ, "hard", (1,))
    he, ge, Se = rhf_inputs(*easy)
    hh, gh, Sh = rhf_inputs(*hard)
    res = scf.rhf_batch(torch.cat([he, hh, he]), torch.cat([ge, gh, ge]), torch.cat([Se, Sh, Se]), n_occ)
    its = res.iterations.cpu().tolist()
    print("iterations", its, "host", [V.host_solution(n, n_occ, 1, s)["iterations"] for s in ("easy", "hard", "easy")])
    assert res.info.cpu().tolist() == [0, 0, 0] and its[1] - its[0] > 2 * 4     # (frozen for more than two check blocks)
    assert_same_result(scf.rhf_batch(he[0], ge[0], Se[0], n_occ), res, 0, "the easy problem first")
    assert_same_result(scf.rhf_batch(hh[0], gh[0], Sh[0], n_occ), res, 1, "the hard problem")
    assert_same_result(scf.rhf_batch(he[0], ge[0], Se[0], n_occ), res, 2, "the easy problem last")
    for k, s in enumerate(("easy", "hard", "easy")):
        compare_with_host(res, k, V.host_solution(n, n_occ, 1, s), (ge, gh, ge)[k][0].cpu().numpy(), f"{s} at {k}")


def test_the_driver_without_the_pinned_verdict_words_gives_the_same_bits():
    stack = (17, 1, "firm", V.seeds_of(17, 1, "firm"))
    n, n_occ = stack[:2]
    h, g, S = rhf_inputs(*stack)
    res = rhf_stack(*stack)
    G = int(h.shape[0])
    lib = _lib.load()
    work = torch.empty(int(lib.oovqe_rhf_work_size(n, G)), dtype=F64, device=dev())
    mo, oao_mo = torch.empty((G, n, n), dtype=F64, device=dev()), torch.empty((G, n, n), dtype=F64, device=dev())
    eps = torch.empty((G, n), dtype=F64, device=dev())
    e_elec, err = torch.empty(G, dtype=F64, device=dev()), torch.empty(G, dtype=F64, device=dev())
    iters = torch.empty(G, dtype=torch.int32, device=dev())
    info = torch.empty(G, dtype=torch.int32, device=dev())
    check(lib.oovqe_rhf_batch(dptr(h), dptr(g), dptr(S), None, n, n_occ, G, V.CONV_TOL, V.ERR_TOL, 200, dptr(mo),
                              dptr(oao_mo), dptr(eps), dptr(e_elec), dptr(err), dptr(iters, torch.int32),
                              dptr(info, torch.int32), dptr(work), ctypes.c_void_p(None), stream_ptr()),
          "oovqe_rhf_batch")
    raw = scf.RHFResult(mo, oao_mo, eps, e_elec, info == 0, iters, err, info)
    print("iterations", iters.cpu().tolist())
    assert info.cpu().tolist() == [0] * G
    assert_same_result(raw, res, slice(None), "the synchronous driver")


# ---- 5. Z-vector: the bare solver on the scope grid -----------------------------------------------------------------------
def z_nset(n):
    return 10 if n <= 33 else 3


@functools.lru_cache(maxsize=None)
def z_inputs(n, n_occ, setting, seeds):
    """(g, C, eps) on the device: the integrals of the stack and the host's converged canonical orbitals."""
    sols = [V.host_solution(n, n_occ, s, setting) for s in seeds]
    g = cuda(np.stack([V.problem(n, n_occ, s, setting)["int2e_ao"] for s in seeds]))
    return g, cuda(np.stack([s["C"] for s in sols])), cuda(np.stack([s["e"] for s in sols]))


def solve_bare(g, C, eps, n_occ, w, tol=V.Z_TOL, max_iter=100):
    """``nucgrad.zvector`` with n_core = 0, ncas = n: nothing is eliminated and w[n_occ:, :n_occ] goes to the solver
    as it is."""
    n = int(C.shape[-1])
    return nucgrad.zvector(g, C, eps, 0, n, n_occ, w, tol, max_iter)


def check_sets(res, k, sol, ws, label, tol=V.Z_TOL):
    n, n_occ = sol["mol"].nao, sol["n_occ"]
    A = sol["A"]
    d = (sol["e"][n_occ:, None] - sol["e"][None, :n_occ]).reshape(-1)
    z = res.z[k].cpu().numpy()
    vo, _ = nucgrad.response_pairs(n, 0, n, n_occ)
    worst = 0.0
    for s, w in enumerate(ws):
        b = w[n_occ:, :n_occ].reshape(-1)
        ref = np.linalg.solve(A, b)
        _, host_its = V.host_pcg(A, b, d, tol)
        err = np.linalg.norm(z[s][n_occ:, :n_occ].reshape(-1) - ref)
        bound = V.z_error_bound(sol, ref, tol)
        its, resid = int(res.iterations[k, s]), res.residual[k, s].item()
        print(f"{label} set {s}: ||z|| {np.linalg.norm(ref):.2e}, error {err:.2e}, bound {bound:.2e}, residual "
              f"{resid:.2e}, iterations {its} (host {host_its})")
        assert int(res.info[k, s]) == 0 and resid <= tol
        assert err <= bound
        assert abs(its - host_its) <= 3
        assert not z[s][~vo].any()
        worst = max(worst, err / bound)
    return worst


@pytest.mark.parametrize("stack", V.z_stacks(), ids=stack_id)
def test_zvector_scope_grid_against_the_dense_solve(stack):
    n, n_occ, setting, seeds = stack
    g, C, eps = z_inputs(*stack)
    K = z_nset(n)
    ws = [V.z_rhs(n, n_occ, K, s) for s in seeds]
    res = solve_bare(g, C, eps, n_occ, cuda(np.stack(ws)))
    lds = R.step_lds_bytes(n, n_occ) / 1024.0
    for k, seed in enumerate(seeds):
        sol = V.host_solution(n, n_occ, seed, setting)
        worst = check_sets(res, k, sol, ws[k], f"({n}, {n_occ}) {setting} seed {seed}")
        print(f"({n}, {n_occ}) {setting} seed {seed}: {n_occ * (n - n_occ)} unknowns, LDS {lds:.1f} KB, lambda_min(A) "
              f"{sol['lam_min']:.3f}, cond(A) {sol['cond']:.1f}, largest error / bound {worst:.3f}")


def test_zvector_elimination_path_above_the_molecules():
    """n = 17, three core, six active, eleven external orbitals against the full dense L of ``zvector_host``; the bound
    of ``test_zvector_against_the_dense_host_solve``: Z_TOL times max(eps_a - eps_i) / lambda_min(A)."""
    e = V.ELIMINATION_CASE
    n, n_core, ncas, n_occ = e["n"], e["n_core"], e["ncas"], e["n_occ"]
    stack = (n, n_occ, e["setting"], (e["seed"],))
    g, C, eps = z_inputs(*stack)
    sol = V.host_solution(n, n_occ, e["seed"], e["setting"])
    ws = R.masked_rhs(n, n_core, ncas, n_occ, 2, 1717)
    res = nucgrad.zvector(g, C, eps, n_core, ncas, n_occ, cuda(ws[None]), V.Z_TOL, 100)
    assert res.info.tolist() == [[0, 0]]
    gh = V.problem(n, n_occ, e["seed"], e["setting"])["int2e_ao"]
    bound = V.Z_TOL * (sol["e"][n_occ:].max() - sol["e"][:n_occ].min()) / sol["lam_min"]
    for s in range(2):
        want = nucgrad.zvector_host(gh, sol["C"], sol["e"], n_core, ncas, n_occ, ws[s])
        err = np.abs(res.z[0, s].cpu().numpy() - want).max()
        print(f"set {s}: max |z| {np.abs(want).max():.3e}, {int(res.iterations[0, s])} iterations, residual "
              f"{res.residual[0, s].item():.2e}, lambda_min {sol['lam_min']:.3f}, error {err:.2e}, bound {bound:.2e}")
        assert res.residual[0, s].item() <= V.Z_TOL
        assert err <= bound


# ---- 6. Z-vector: sets that finish at different iterations -------------------------------------------------------------------
SETS_STACK = (33, 16, "firm", (1,))
SCALES = tuple(10.0 ** np.linspace(-8.0, 4.0, 9))


def scaled_rhs():
    """Ten right-hand sides of very different size, and with them different iteration counts to the absolute ``tol``;
    set 4 is exactly zero."""
    n, n_occ = SETS_STACK[:2]
    w = V.z_rhs(n, n_occ, 10, 99)
    scales = list(SCALES[:4]) + [0.0] + list(SCALES[4:])
    return w * np.array(scales)[:, None, None]


def test_zvector_sets_finish_at_different_iterations_with_the_bits_they_have_alone():
    n, n_occ, setting, seeds = SETS_STACK
    g, C, eps = z_inputs(*SETS_STACK)
    sol = V.host_solution(n, n_occ, seeds[0], setting)
    ws = scaled_rhs()
    w = cuda(ws[None])
    res = solve_bare(g, C, eps, n_occ, w)
    its = res.iterations[0].cpu().tolist()
    print("iterations", its)
    check_sets(res, 0, sol, ws, "scaled")
    assert its[4] == 0 and res.info[0, 4].item() == 0 and not res.z[0, 4].any().item()
    assert res.residual[0, 4].item() == 0.0
    assert len(set(its)) >= 5
    fields = ("z", "info", "iterations", "residual")
    for s in range(10):                                                 # alone
        one = solve_bare(g, C, eps, n_occ, w[:, s:s + 1].contiguous())
        for f in fields:
            assert same_bits(getattr(one, f)[:, 0], getattr(res, f)[:, s]), (f, s)
    for order in ([9, 8, 7, 6, 5, 4, 3, 2, 1, 0], [7, 3, 4, 9, 1], [9, 0, 8, 4, 6, 5]):     # another place; 5 and 6 sets
        sub = solve_bare(g, C, eps, n_occ, w[:, order].contiguous())
        for f in fields:
            assert same_bits(getattr(sub, f), getattr(res, f)[:, order]), (f, order)
    for mi in (1, 3, 4, 5):                                             # either side of the check interval
        cut = solve_bare(g, C, eps, n_occ, w, max_iter=mi)
        for s in range(10):
            if its[s] <= mi:
                for f in fields:
                    assert same_bits(getattr(cut, f)[:, s], getattr(res, f)[:, s]), (f, s, mi)
            else:
                assert cut.info[0, s].item() == 1 and cut.iterations[0, s].item() == mi, (s, mi)
                assert torch.isfinite(cut.z[0, s]).all() and cut.residual[0, s].item() > V.Z_TOL


# ---- 7. Z-vector: info = -2 both ways ------------------------------------------------------------------------------------------
NEG_STACK = (23, 12, "firm", (1,))


def test_zvector_reports_an_occupied_level_above_a_virtual_one_at_the_start():
    n, n_occ, setting, seeds = NEG_STACK
    g, C, eps = z_inputs(*NEG_STACK)
    w = cuda(V.z_rhs(n, n_occ, 3, 5)[None])
    alone = solve_bare(g, C, eps, n_occ, w)
    bad = eps.clone()
    bad[0, n_occ - 1] = bad[0, n_occ] + 0.125
    res = solve_bare(torch.cat([g, g]), torch.cat([C, C]), torch.cat([bad, eps]), n_occ, torch.cat([w, w]))
    print("info", res.info.tolist(), "iterations", res.iterations.tolist())
    assert res.info[0].tolist() == [-2] * 3 and res.iterations[0].tolist() == [0] * 3
    assert torch.isnan(res.z[0]).all() and torch.isnan(res.residual[0]).all()
    for f in ("z", "info", "iterations", "residual"):
        assert same_bits(getattr(res, f)[1], getattr(alone, f)[0]), f


def test_zvector_reports_a_negative_curvature_in_the_first_step():
    """g replaced by -c g with c from the host matrix so that lambda_min(A) < 0, and w = (eps_a - eps_i) v with v that
    eigenvector: p_0 = v and p^T A p = lambda_min |v|^2 < 0 in iteration 1."""
    n, n_occ, setting, seeds = NEG_STACK
    g, C, eps = z_inputs(*NEG_STACK)
    sol = V.host_solution(n, n_occ, seeds[0], setting)
    d = (sol["e"][n_occ:, None] - sol["e"][None, :n_occ]).reshape(-1)
    two = sol["A"] - np.diag(d)                              # the two-electron part, linear in g
    top = np.linalg.eigvalsh(0.5 * (two + two.T))[-1]
    assert top > 0.0
    c = 2.0 * d.max() / top
    lam, vec = np.linalg.eigh(np.diag(d) - c * 0.5 * (two + two.T))
    print(f"c = {c:.3f}, lambda_min of the host matrix {lam[0]:.3f}")
    assert lam[0] < -0.5 * d.max()
    w = np.zeros((1, n, n))
    w[0, n_occ:, :n_occ] = (d * vec[:, 0]).reshape(n - n_occ, n_occ)
    w = cuda(w[None])
    alone = solve_bare(g, C, eps, n_occ, w)
    assert alone.info.tolist() == [[0]]
    res = solve_bare(torch.cat([g, -c * g, g]), torch.cat([C] * 3), torch.cat([eps] * 3), n_occ, torch.cat([w] * 3))
    print("info", res.info.tolist(), "iterations", res.iterations.tolist())
    assert res.info[1].tolist() == [-2] and res.iterations[1].tolist() == [1]
    assert torch.isnan(res.z[1]).all() and torch.isnan(res.residual[1]).all()
    for k in (0, 2):
        for f in ("z", "info", "iterations", "residual"):
            assert same_bits(getattr(res, f)[k], getattr(alone, f)[0]), (f, k)


# ---- 8. response_d2 beyond 256 pairs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [22, 23, 33, 64])
def test_response_d2_beyond_256_pairs(n):
    """n (n + 1) / 2 = 253, 276, 561, 2080 pairs rs for the 256 threads of a workgroup."""
    rows, K = (2, 2) if n <= 33 else (1, 1)
    rng = np.random.default_rng(500 + n)
    sym = lambda t: t + t.transpose(0, 2, 1)                                            # noqa: E731
    Z, D0 = sym(rng.standard_normal((rows, n, n))), sym(rng.standard_normal((rows, n, n)))
    base = cuda(rng.standard_normal((rows, K) + (n,) * 4))
    base = base + base.transpose(2, 3)
    base = base + base.transpose(4, 5)
    base = (base + base.permute(0, 1, 4, 5, 2, 3)).contiguous()
    before = base.clone()
    view = base[:, K - 1]
    out = nucgrad.response_d2(cuda(Z), cuda(D0), view)
    assert out.data_ptr() == view.data_ptr()
    if K > 1:
        assert torch.equal(base[:, 0], before[:, 0])
    for perm in ((0, 2, 1, 3, 4), (0, 1, 2, 4, 3), (0, 3, 4, 1, 2)):
        assert torch.equal(view, view.permute(perm))
    got, old = view.cpu().numpy(), before[:, K - 1].cpu().numpy()
    for r in range(rows):
        want = old[r] - nucgrad.response_d2_host(Z[r], D0[r])
        bound = 10.0 * 8.0 * V.EPS * (np.abs(old[r]).max() + 3.0 * np.abs(Z[r]).max() * np.abs(D0[r]).max())
        err = np.abs(got[r] - want).max()
        print(f"n = {n}, row {r}: {n * (n + 1) // 2} pairs, error {err:.2e}, bound {bound:.2e}")
        assert err <= bound
