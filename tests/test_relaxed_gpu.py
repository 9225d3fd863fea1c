"""Orbital-relaxed CASCI gradients on the device: the multi-set Fock kernel, the Z-vector solve, the response part of the
two-particle density, and ``OO_pqc_batch.casci_relaxed_gradients`` against finite differences of CASCI energies whose
orbitals are RE-SOLVED by RHF at every displaced geometry.

References and bounds (nothing in a bound comes from the code under test):
  * ``fock_jk_sets``: ``fock_jk`` per set.  The two kernels sum in different orders, so the bound is 10 x the difference
    between ``fock_jk`` and a sum in extended precision on the n = 13 case, taken relative to the scale of such a sum,
    ``sum |g| |D|`` (which is what a rounding error is proportional to), and applied to every n with that n's own scale.
  * ``zvector``: the dense solve of ``nucgrad.zvector_host`` on the same inputs; bound ``z_tol`` times the condition
    estimate ``max(eps_a - eps_i) / lambda_min(A)`` of the host matrix.
  * the method: the 4th-order stencil of tests/_casci_gradients.py at h = 1e-3 Bohr; bound 10 x its disagreement with
    h = 2e-3, per case.

The figures in the docstrings of the tests were measured on an MI355X."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import auto_oo_amd as aoo                                   # noqa: E402
from auto_oo_amd import _lib, nucgrad, scf                  # noqa: E402
from auto_oo_amd.gaussian import BOHR                       # noqa: E402
from auto_oo_amd.moldata import get_formal_geo              # noqa: E402
from tests import _casci_gradients as C                     # noqa: E402
from tests import _charges as Q                             # noqa: E402
from tests import _gto_d as D                               # noqa: E402
from tests import _relaxed as R                             # noqa: E402

F64 = torch.float64
H1, H2 = C.H1, C.H2
Z_TOL = 1e-10


def _randn(shape, seed):
    gen = torch.Generator(device=C.dev())
    gen.manual_seed(seed)
    return torch.randn(shape, dtype=F64, device=C.dev(), generator=gen)


# ---- 1. fock_jk_sets ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def summation_figure():
    """max |fock_jk - extended-precision sum| / max sum |g| |D| on the seeded n = 13 case."""
    n = 13
    g, d = _randn((1, n, n, n, n), 1300), _randn((1, n, n), 1301)
    J, K = scf.fock_jk(g, d)
    gl, dl = g[0].cpu().numpy().astype(np.longdouble), d[0].cpu().numpy().astype(np.longdouble)
    Jx, Kx = np.einsum("pqrs,rs->pq", gl, dl), np.einsum("prqs,rs->pq", gl, dl)
    unit = max(np.einsum("pqrs,rs->pq", np.abs(gl), np.abs(dl)).max(), np.einsum("prqs,rs->pq", np.abs(gl), np.abs(dl)).max())
    err = max(np.abs(J[0].cpu().numpy() - Jx).max(), np.abs(K[0].cpu().numpy() - Kx).max())
    return float(err), float(err / unit)


@pytest.mark.parametrize("n,nset", [(1, 1), (1, 10), (7, 5), (7, 6), (13, 1), (13, 5), (13, 6), (13, 10), (63, 6),
                                    (64, 1), (64, 10)])
def test_fock_jk_sets_against_fock_jk_per_set(n, nset):
    """Seeded non-symmetric g and D, two geometries.  Measured: fock_jk differs from the extended-precision sum at
    n = 13 by 5.3e-15, 4.3e-17 of sum |g| |D|; the bounds are 8.7e-17 (n = 1, one set) .. 2.7e-12 (n = 64, ten sets) and
    the two kernels differ by 0 (n = 1), 3.6e-15 .. 7.1e-15 (n = 7), 1.1e-14 .. 1.4e-14 (n = 13), 3.8e-13 .. 4.3e-13
    (n = 63, 64): at most a third of the bound."""
    G = 2
    g, d = _randn((G, n, n, n, n), 10 * n + nset), _randn((G, nset, n, n), 10 * n + nset + 1)
    J, K = scf.fock_jk_sets(g, d)
    assert tuple(J.shape) == tuple(K.shape) == (G, nset, n, n)
    err13, rel = summation_figure()
    Ja, Ka = scf.fock_jk(g.abs(), d.abs().amax(dim=1))
    bound = 10.0 * rel * max(Ja.max().item(), Ka.max().item())
    worst = 0.0
    for s in range(nset):
        Js, Ks = scf.fock_jk(g, d[:, s].contiguous())
        worst = max(worst, (J[:, s] - Js).abs().max().item(), (K[:, s] - Ks).abs().max().item())
    print(f"n = {n}, nset = {nset}: fock_jk_sets - fock_jk {worst:.2e}, bound {bound:.2e} (fock_jk against the extended "
          f"sum at n = 13: {err13:.2e}, relative to sum |g||D| {rel:.2e})")
    assert worst <= bound


def test_a_set_has_the_same_bits_for_every_nset_and_place_and_a_geometry_alone():
    n, G = 13, 3
    g, d = _randn((G, n, n, n, n), 77), _randn((G, 10, n, n), 78)
    J, K = scf.fock_jk_sets(g, d)
    for order in ([3], [7, 3, 0, 9, 1], [9, 8, 7, 6, 5, 4], [2, 0, 1, 3, 4, 5, 6, 7, 8, 9]):
        Jo, Ko = scf.fock_jk_sets(g, d[:, order].contiguous())
        assert torch.equal(Jo, J[:, order]) and torch.equal(Ko, K[:, order]), order
    J1, K1 = scf.fock_jk_sets(g[1], d[1])
    assert torch.equal(J1, J[1]) and torch.equal(K1, K[1])
    perm = [2, 0, 1]
    Jp, Kp = scf.fock_jk_sets(g[perm].contiguous(), d[perm].contiguous())
    assert torch.equal(Jp, J[perm]) and torch.equal(Kp, K[perm])


# ---- batches on canonical RHF orbitals ----------------------------------------------------------------------------------
def tighten(b):
    """RHF orbitals converged well beyond the default, installed in the batch"""
    res = b.rhf(conv_tol=1e-14, err_tol=1e-12, max_cycle=100)
    assert res.diis_error.max().item() < 1e-10
    b.oao_mo_coeff.copy_(res.oao_mo_coeff)
    b.refresh_mo_coeff()
    return b


def geometry(name):
    basis, xyz = C.case(name)
    return basis, xyz[:1]


@functools.lru_cache(maxsize=None)
def rhf_batch(name, ncas, nelecas, charges=0):
    basis, xyz = geometry(name)
    pc = None if not charges else Q.cloud(xyz[0] * BOHR, charges, on_nucleus=False)
    return tighten(aoo.OO_pqc_batch.from_geometries(C.circuit(ncas, nelecas), basis, xyz * BOHR, ncas, nelecas,
                                                    oao_mo_coeffs="rhf", point_charges=pc))


def host_inputs(b, R_):
    """Per state of geometry 0 of a batch: the orbital gradient from the host twins on the batch's own integrals and
    orbitals -> (g, C, eps, n_core, n_occ, [w])"""
    S, h, g = (t[0].cpu().numpy() for t in (b.overlap, b.int1e_ao, b.int2e_ao))
    Cm = b.mo_coeff[0].cpu().numpy()
    n_occ = b.nelectron // 2
    f = Cm.T @ (h + nucgrad._g_host(g, 2.0 * Cm[:, :n_occ] @ Cm[:, :n_occ].T)) @ Cm
    sol = R.host_casci(S, h, g, b.nuc[0].item(), b.nelectron, b.ncas, b.nelecas, R_, Cm, np.diag(f).copy())
    ws = [nucgrad.orbital_gradient_host(R.host_state_quantities(S, h, g, sol, b.ncas, r)[2]) for r in range(R_)]
    return g, Cm, sol["eps"], sol["n_core"], n_occ, ws


ZCASES = [("h2", 2, 2), ("water", 2, 2), ("formaldimine", 2, 2), ("formaldimine", 3, 4)]


# ---- 2. zvector -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ncas,nelecas", ZCASES)
def test_zvector_against_the_dense_host_solve(name, ncas, nelecas):
    """Two states per geometry.  Measured (error / bound; iterations): h2 1.4e-16 / 5.7e-10 (1 iteration for its three
    unknowns); water 7.8e-12 / 4.0e-09 (7 - 8); formaldimine CAS(2e,2o)
    1.4e-11 / 2.4e-08 (16 - 17); CAS(4e,3o) 1.5e-11 / 2.4e-08 (16); lambda_min(A) = 1.02, 0.52, 0.067."""
    b = rhf_batch(name, ncas, nelecas)
    g, Cm, eps, n_core, n_occ, ws = host_inputs(b, 2)
    dev = C.dev()
    w = torch.as_tensor(np.stack(ws)[None]).to(dev)
    res = nucgrad.zvector(b.int2e_ao, b.mo_coeff, torch.as_tensor(eps[None]).to(dev), n_core, ncas, n_occ, w, Z_TOL, 100)
    assert res.info.tolist() == [[0, 0]]
    for s in range(2):
        want = nucgrad.zvector_host(g, Cm, eps, n_core, ncas, n_occ, ws[s])
        _, A, _ = nucgrad.zvector_host(g, Cm, eps, n_core, ncas, n_occ, ws[s], eliminate=True)
        lam = np.linalg.eigvalsh(0.5 * (A + A.T)).min()
        bound = Z_TOL * (eps[n_occ:].max() - eps[:n_occ].min()) / lam
        err = np.abs(res.z[0, s].cpu().numpy() - want).max()
        print(f"{name} CAS({nelecas}e,{ncas}o) state {s}: max |z| {np.abs(want).max():.3e}, {int(res.iterations[0, s])} "
              f"iterations, residual {res.residual[0, s].item():.2e}, lambda_min {lam:.3f}, error {err:.2e}, bound "
              f"{bound:.2e}")
        assert res.residual[0, s].item() <= Z_TOL
        assert err <= bound


def test_zvector_reports_per_set_and_freezes_what_has_finished():
    """max_iter = 1: info 1 for the set that needs more, 0 for the set whose right-hand side is zero; a stack with one
    NaN geometry: -3 there, NaN outputs, and the same bits for its neighbours as alone."""
    b = rhf_batch("water", 2, 2)
    g, Cm, eps, n_core, n_occ, ws = host_inputs(b, 2)
    dev = C.dev()
    e = torch.as_tensor(eps[None]).to(dev)
    w = torch.as_tensor(np.stack([ws[1], np.zeros_like(ws[1])])[None]).to(dev)
    one = nucgrad.zvector(b.int2e_ao, b.mo_coeff, e, n_core, 2, n_occ, w, Z_TOL, 1)
    assert one.info.tolist() == [[1, 0]] and one.iterations.tolist() == [[1, 0]]
    assert torch.isfinite(one.z).all() and one.z[0, 1].abs().max().item() == 0.0
    w = torch.as_tensor(np.stack(ws)[None]).to(dev)
    alone = nucgrad.zvector(b.int2e_ao, b.mo_coeff, e, n_core, 2, n_occ, w, Z_TOL, 100)
    g3 = b.int2e_ao.expand(3, -1, -1, -1, -1).clone()
    g3[1, 2, 3, 1, 0] = float("nan")
    rep = lambda t: t.expand((3,) + tuple(t.shape[1:])).contiguous()
    res = nucgrad.zvector(g3, rep(b.mo_coeff), rep(e), n_core, 2, n_occ, rep(w), Z_TOL, 100)
    assert res.info.tolist() == [[0, 0], [-3, -3], [0, 0]]
    assert torch.isnan(res.z[1]).all() and torch.isnan(res.residual[1]).all()
    for k in (0, 2):
        assert torch.equal(res.z[k], alone.z[0]) and torch.equal(res.iterations[k], alone.iterations[0])
    # NaN in the orbital energies of another geometry, found at the start
    e3 = rep(e).clone()
    e3[2, 1] = float("nan")
    res = nucgrad.zvector(rep(b.int2e_ao), rep(b.mo_coeff), e3, n_core, 2, n_occ, rep(w), Z_TOL, 100)
    assert res.info.tolist() == [[0, 0], [0, 0], [-3, -3]]
    assert torch.equal(res.z[0], alone.z[0]) and torch.equal(res.z[1], alone.z[0])


# ---- 3. response_d2 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 13])
def test_response_d2_against_numpy_and_exact_symmetry(n):
    """rows of a strided view; bound 1e-13 on numbers of order 10 (a handful of products per element)."""
    rows, K = 3, 2
    sym = lambda t: t + t.transpose(1, 2)
    Z, D0 = sym(_randn((rows, n, n), 5)), sym(_randn((rows, n, n), 6))
    base = _randn((rows, K) + (n,) * 4, 7)
    base = base + base.transpose(2, 3)
    base = base + base.transpose(4, 5)
    base = (base + base.permute(0, 1, 4, 5, 2, 3)).contiguous()
    before = base.clone()
    out = nucgrad.response_d2(Z, D0, base[:, 1])
    assert out.data_ptr() == base[:, 1].data_ptr() and torch.equal(base[:, 0], before[:, 0])
    got = base[:, 1].cpu().numpy()
    for r in range(rows):
        want = before[r, 1].cpu().numpy() - nucgrad.response_d2_host(Z[r].cpu().numpy(), D0[r].cpu().numpy())
        assert np.abs(got[r] - want).max() < 1e-13
        for perm in ((1, 0, 2, 3), (0, 1, 3, 2), (2, 3, 0, 1)):
            assert np.array_equal(got[r], got[r].transpose(perm))


# ---- 4. - 6. the method against the total finite difference -----------------------------------------------------------------
def total_reference(name, ncas, nelecas, nroots, charges=0, move="atoms"):
    """Finite differences of the CASCI energies with every displaced copy re-solved by RHF, tightly -> ([R, natm or M,
    3] at h = 1e-3, its disagreement with h = 2e-3)"""
    basis, xyz = geometry(name)
    pc = None
    if charges:
        q, r = Q.cloud(xyz[0] * BOHR, charges, on_nucleus=False)
    if move == "atoms":
        stack = np.concatenate([C.fd_stack(xyz[0], h) for h in (H1, H2)])
        if charges:
            pc = (q, r)
    else:
        rs = np.concatenate([C.fd_stack(r / BOHR, h) for h in (H1, H2)])
        stack = np.repeat(xyz, len(rs), axis=0)
        pc = (np.repeat(q[None], len(rs), axis=0), rs * BOHR)
    bd = tighten(aoo.OO_pqc_batch.from_geometries(C.circuit(ncas, nelecas), basis, stack * BOHR, ncas, nelecas,
                                                  oao_mo_coeffs="rhf", point_charges=pc))
    e = bd.casci(nroots)[0].cpu().numpy().T
    n = bd.G // 2
    a, b_ = C.fd_combine(e[:, :n], H1), C.fd_combine(e[:, n:], H2)
    return a, np.abs(a - b_).max()


@pytest.mark.parametrize("name,ncas,nelecas", [("water", 2, 2), ("formaldimine", 2, 2), ("formaldimine", 3, 4),
                                               ("h2", 2, 2)])
def test_relaxed_gradients_against_the_total_finite_difference(name, ncas, nelecas):
    """R = 2.  The relaxed gradient within 10 x the reference's own disagreement, the fixed-orbital one outside it and
    equal to the diagonal of ``casci_nuclear_gradients`` bit for bit; no net force.  Measured (reference disagreement
    -> bound; relaxed - reference; fixed-orbital - reference; net force): water 1.7e-09 -> 1.7e-08; 1.3e-10; 2.7e-02;
    9.4e-16.  formaldimine CAS(2e,2o) 8.6e-09 -> 8.6e-08; 5.6e-10; 2.0e-01; 1.3e-15.  CAS(4e,3o) 1.1e-10 -> 1.1e-09;
    9.8e-11; 8.4e-02; 1.6e-15.  h2 1.09e-09 -> 1.09e-08; 1.09e-09; 1.7e-03; 1.1e-16."""
    b = rhf_batch(name, ncas, nelecas)
    res = b.casci_relaxed_gradients(nroots=2)
    natm = b.basis.natm
    assert tuple(res.gradients.shape) == tuple(res.fixed_orbital.shape) == (1, 2, natm, 3)
    assert res.z_info.tolist() == [[0, 0]] and res.charge_gradients is None
    fixed = b.casci_nuclear_gradients(nroots=2)
    k = torch.arange(2, device=b.device)
    assert torch.equal(res.fixed_orbital, fixed.gradients[:, k, k])
    assert torch.equal(res.energies, fixed.energies) and torch.equal(res.ci, fixed.ci)
    want, dis = total_reference(name, ncas, nelecas, 2)
    err = np.abs(res.gradients[0].cpu().numpy() - want).max()
    miss = np.abs(res.fixed_orbital[0].cpu().numpy() - want).max()
    net = res.gradients.sum(dim=2).abs().max().item()
    print(f"{name} CAS({nelecas}e,{ncas}o): gradients up to {np.abs(want).max():.3g}, reference disagreement {dis:.2e}, "
          f"bound {10 * dis:.2e}, relaxed - reference {err:.2e}, fixed-orbital - reference {miss:.2e}, net force "
          f"{net:.2e}")
    assert err < 10 * dis
    assert miss > 10 * dis
    assert net < 1e-10 * natm


def test_embedded_water_atoms_and_charges_against_the_total_finite_difference():
    """Water in 4 charges of tests/_charges.cloud (none on a nucleus): the atoms' gradients and ``charge_gradients``
    against the same finite difference, the latter with the charges displaced.  Measured: gradients up to 87 Ha / Bohr
    (one charge sits 0.2 Bohr from the oxygen nucleus), reference disagreement 1.5e-06 -> bound 1.5e-05, relaxed -
    reference 1.0e-07 for the atoms and for the charges."""
    M = 4
    b = rhf_batch("water", 2, 2, M)
    res = b.casci_relaxed_gradients(nroots=2)
    assert tuple(res.charge_gradients.shape) == (1, 2, M, 3)
    fixed = b.casci_nuclear_gradients(nroots=2)
    k = torch.arange(2, device=b.device)
    assert torch.equal(res.fixed_orbital, fixed.gradients[:, k, k])
    for what, got in (("atoms", res.gradients), ("charges", res.charge_gradients)):
        want, dis = total_reference("water", 2, 2, 2, M, what)
        err = np.abs(got[0].cpu().numpy() - want).max()
        print(f"embedded water, {what}: gradients up to {np.abs(want).max():.3g}, reference disagreement {dis:.2e}, bound "
              f"{10 * dis:.2e}, relaxed - reference {err:.2e}")
        assert err < 10 * dis
    miss = np.abs(res.fixed_orbital[0].cpu().numpy() - total_reference("water", 2, 2, 2, M, "atoms")[0]).max()
    assert miss > 10 * total_reference("water", 2, 2, 2, M, "atoms")[1]


# ---- 5., 7. translation invariance and bits over a stack ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def formaldimine_stack(order=(0, 1, 2)):
    basis, xyz = C.case("formaldimine")
    return tighten(aoo.OO_pqc_batch.from_geometries(C.circuit(2, 2), basis, xyz[list(order)] * BOHR, 2, 2,
                                                    oao_mo_coeffs="rhf"))


def test_no_net_force_and_the_same_bits_for_index_chunk_and_a_permuted_stack():
    """Measured: net force 2.2e-15 for a bound of 5e-10 (1e-10 times 5 atoms)."""
    b = formaldimine_stack()
    full = b.casci_relaxed_gradients(nroots=2)
    natm = b.basis.natm
    net = full.gradients.sum(dim=2).abs().max().item()
    print(f"formaldimine, three geometries: net force {net:.2e} (bound {1e-10 * natm:.0e})")
    assert net < 1e-10 * natm
    by_one = b.casci_relaxed_gradients(nroots=2, chunk=1)
    for x, y in zip(by_one[:5], full[:5]):
        assert torch.equal(x, y)
    part = b.casci_relaxed_gradients(nroots=2, index=[2, 0])
    for x, y in zip(part[:5], full[:5]):
        assert torch.equal(x, y[[2, 0]])
    one = b.casci_relaxed_gradients(nroots=2, index=1)
    assert torch.equal(one.gradients, full.gradients[1:2])
    perm = (2, 0, 1)
    p = formaldimine_stack(perm)
    assert torch.equal(p.mo_coeff, b.mo_coeff[list(perm)])
    other = p.casci_relaxed_gradients(nroots=2)
    assert torch.equal(other.gradients, full.gradients[list(perm)])
    assert torch.equal(other.fixed_orbital, full.fixed_orbital[list(perm)])


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    pqc = C.circuit(2, 2)
    # linear H-F, CAS(2e,2o): the degenerate pi pair is split between core and active space
    basis, xyz = C.case("hf")
    hf = aoo.OO_pqc_batch.from_geometries(pqc, basis, xyz * BOHR, 2, 2, oao_mo_coeffs="rhf")
    with pytest.raises(ValueError, match=r"\|eps_p - eps_q\| <"):
        hf.casci_relaxed_gradients(nroots=2)
    res = hf.casci_relaxed_gradients(nroots=2, small_gap="nan")
    assert torch.isnan(res.gradients).all() and torch.isfinite(res.fixed_orbital).all()
    assert res.z_info.tolist() == [[-4, -4]]
    with pytest.raises(ValueError, match="small_gap"):
        hf.casci_relaxed_gradients(small_gap="ignore")
    # orbitals that are not RHF orbitals
    with pytest.raises(ValueError, match="not canonical RHF orbitals"):
        C.batch("water", 2, 2).casci_relaxed_gradients()
    # a Z-vector solve that does not converge names geometry, state and code
    w = rhf_batch("water", 2, 2)
    with pytest.raises(_lib.OovqeError, match=r"\(0, 1: 1 max_iter reached\)"):
        w.casci_relaxed_gradients(nroots=2, z_max_iter=1)
    # the refusals of casci_nuclear_gradients
    dbatch = aoo.OO_pqc_batch.from_geometries(pqc, D.m2_basis(), D.WATER[None], 2, 2, oao_mo_coeffs="rhf",
                                              freeze_active=True)
    with pytest.raises(NotImplementedError, match="d shells"):
        dbatch.casci_relaxed_gradients()
    from auto_oo_amd.gaussian import Moldata_sto3g
    mol = Moldata_sto3g(get_formal_geo(*C.POINTS[0]))
    host = aoo.OO_pqc_batch(pqc, [mol], 2, 2, oao_mo_coeffs=[np.eye(13)])
    with pytest.raises(RuntimeError, match="from_geometries"):
        host.casci_relaxed_gradients()
    big = copy.copy(w)
    big.ncas = nucgrad.MAX_NCAS + 1
    with pytest.raises(NotImplementedError, match="ncas"):
        big.casci_relaxed_gradients()
    with pytest.raises(ValueError):
        w.casci_relaxed_gradients(index=[3])
    with pytest.raises(ValueError, match="nroots"):
        w.casci_relaxed_gradients(nroots=0)
