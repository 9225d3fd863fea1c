"""The orbital-orbital Hessian kernels (auto_oo_amd/csrc/hessian.hip: ``hess_ab_kernel``, ``t2k_tri_kernel<4|8|12|16>``,
``hess_matrix_kernel``, ``hess_full_kernel`` and the contraction chains between them) and ``oovqe_fock_core_active`` over
their whole scope, against the numpy twin of tests/_hessian_scope.py, which tests/test_hessian_scope_cpu.py holds against
the dense oracle.  tests/_hessian_scope.py says where the bound comes from; nothing in it comes from the device's output.

Level A: ``oovqe_orbital_hessian`` with the Fock matrix of the twin, RDMs WITHOUT index symmetry, 8-fold symmetric and
non-symmetric integrals (a transposed index anywhere in gamma2_full, At / Bt or Vk -> T2K -> W -> Kint moves the result by
many orders of magnitude more than the bound).  Level B: ``oovqe_orbital_hessian_batch`` for stacks of three, on the
``t2k_tri_kernel`` route (flags of ``ops.eri_flags``) and on the contraction route (flags 0).  Level C: ``OO_energy`` and
``OO_pqc_batch.energy_gradient_hessian`` with the Fock matrix of the device's own CAS path and RDMs with the symmetry of a
real state.

No defect was found: every case passed on its first run.  Measured on an MI355X (one run; "share" is the largest error /
bound over the elements; DESIGN.md has the figures case by case): Level A shares 7.4e-05 .. 0.026 (the largest at
(2, 0, 1)), 7.9e-06 at (64, 24, 8); Level B 3.3e-05 .. 0.026, the same on both routes wherever ``t2k_tri_kernel`` serves
the shape; Level C 7.9e-06 .. 0.00044 and 0.0024 for the one-call batch; ``fock_core`` / ``fock_active`` up to 0.088 /
0.37.  With ``gam`` transposed in the (occ, act, act, occ) branch of ``gamma2_full`` (a scratch build) every Level A
case with a core and ``ncas`` > 1 fails, (6, 2, 2) first, by 3.7e11 bounds.  The file takes 16.5 s, its slowest cases
(Level A at (64, 24, 8), the twin on the host) 3.1 - 3.4 s; kernel times were not measured.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import auto_oo_amd as aoo                                   # noqa: E402
from auto_oo_amd import _lib, ops                           # noqa: E402
from oracle import cpu_ref as R                             # noqa: E402
from tests import _hessian_scope as V                       # noqa: E402

F64 = torch.float64
to_dev = V.to_dev


def host(t):
    return t.detach().cpu().numpy()


def case_id(c):
    return "-".join(str(int(x)) if not isinstance(x, bool) else ("frozen" if x else "free") for x in c)


def geometry(N, n_occ, ncas, k, kind, integrals):
    """(h, g, C, gam, Gam) of geometry k of a case."""
    seed = V.seed_of(N, n_occ, ncas, k)
    h, g, S, U, C = V.problem(N, seed)
    if integrals == "nonsymmetric":
        g = V.nonsymmetric(g, seed)
    gam, Gam = V.rdms(ncas, seed, kind)
    return h, g, C, gam, Gam


def tables(N, n_occ, ncas, freeze):
    rows, cols = V.kappa_tables(N, n_occ, ncas, freeze)
    return rows, cols, to_dev(rows, torch.int32), to_dev(cols, torch.int32)


def held(what, got, ref, bound):
    """Print "largest error / bound" of a result and return it."""
    err = np.abs(got - ref)
    s = V.share(err, bound)
    print(f"{what}: max |H| {np.abs(ref).max():.3g}, largest error {err.max():.2e}, largest error / bound {s:.2g}")
    return s


# ---- Level A: oovqe_orbital_hessian ------------------------------------------------------------------------------------------
A_CASES = [c + (True, True) for c in V.A_BOTH] + [c + (True, False) for c in V.A_MATRIX] + [c + (False, True) for c in V.A_FULL]


@pytest.mark.parametrize("integrals", ["symmetric", "nonsymmetric"])
@pytest.mark.parametrize("N,n_occ,ncas,freeze,want_matrix,want_full", A_CASES, ids=[case_id(c[:4]) for c in A_CASES])
def test_level_a_single_geometry_against_the_twin(N, n_occ, ncas, freeze, want_matrix, want_full, integrals):
    """``ops.orbital_hessian`` with the twin's Fock matrix and RDMs without symmetry.  Where both are asked for, the
    matrix and ``full_hessian_to_matrix`` of the full tensor agree under ``torch.equal``: ``hess_matrix_kernel`` and
    ``hess_full_kernel`` evaluate the same expression ``hess_x(pqrs) - hess_x(pqsr) - hess_x(qprs) + hess_x(qpsr)`` on the
    same intermediates of the one call."""
    h, g, C, gam, Gam = geometry(N, n_occ, ncas, 0, "plain", integrals)
    args = (h, g, C, gam, Gam, n_occ, ncas)
    rows, cols, drows, dcols = tables(N, n_occ, ncas, freeze)
    fock = V.fock_twin(*args)
    Hm, Hf = ops.orbital_hessian(to_dev(g), to_dev(h), to_dev(C), to_dev(gam), to_dev(Gam), to_dev(fock), n_occ, ncas,
                                 drows, dcols, want_matrix=want_matrix, want_full=want_full)
    torch.cuda.synchronize()
    what = f"A ({N}, {n_occ}, {ncas}) {'frozen' if freeze else 'free'}, {integrals}, n_kappa {len(rows)}"
    shares = []
    if want_full:
        assert tuple(Hf.shape) == (N,) * 4 and bool(torch.isfinite(Hf).all())
        shares.append(held(what + ", full", host(Hf), V.hessian_twin(*args), V.hessian_bound(*args)))
    if want_matrix:
        assert tuple(Hm.shape) == (len(rows),) * 2 and bool(torch.isfinite(Hm).all())
        shares.append(held(what + ", matrix", host(Hm), V.hessian_twin(*args, rows, cols),
                           V.hessian_bound(*args, rows, cols)))
    if want_full and want_matrix:
        r, c = drows.long(), dcols.long()
        gathered = Hf[r, c, :, :][:, r, c]
        print(f"{what}: matrix against the gather of the full tensor, largest difference "
              f"{(gathered - Hm).abs().max().item():.1e}")
        assert torch.equal(gathered, Hm)
    assert max(shares) <= 1.0


# ---- Level B: oovqe_orbital_hessian_batch ------------------------------------------------------------------------------------
G_B = 3


def stack_of(N, n_occ, ncas, integrals, rows=None, cols=None, G=G_B):
    """Device stacks (g, h, C, gam, Gam, fock) of G geometries with different integrals, orbitals and RDMs, the Fock
    matrices being the twin's; with ``rows``, ``cols`` also (twin, bound) of every geometry."""
    geo, focks, refs = [], [], []
    for k in range(G):
        x = geometry(N, n_occ, ncas, k, "plain", integrals)
        geo.append(x)
        focks.append(V.fock_twin(*x, n_occ, ncas))
        if rows is not None:
            refs.append((V.hessian_twin(*x, n_occ, ncas, rows, cols), V.hessian_bound(*x, n_occ, ncas, rows, cols)))
    dev = [to_dev(np.stack([x[i] for x in geo])) for i in (1, 0, 2, 3, 4)] + [to_dev(np.stack(focks))]
    return dev, refs


def batch_share(what, H, refs):
    """Largest error / bound over the geometries of a stack."""
    Hh = host(H)
    assert np.isfinite(Hh).all()
    worst = max(V.share(np.abs(Hh[k] - ref), bound) for k, (ref, bound) in enumerate(refs))
    err = max(np.abs(Hh[k] - ref).max() for k, (ref, _) in enumerate(refs))
    print(f"{what}: largest error {err:.2e}, largest error / bound {worst:.2g}")
    return worst


@pytest.mark.parametrize("N,n_occ,ncas", V.B_CASES, ids=[case_id(c) for c in V.B_CASES])
def test_level_b_stack_on_both_routes_against_the_twin(N, n_occ, ncas):
    """A stack of three with symmetric integrals, with the flags of ``ops.eri_flags`` (the quarter transform comes from
    stage 1 and ``t2k_tri_kernel`` where N <= 48 and M <= 16) and again with flags 0 (the contraction route): both
    against the twin."""
    M = n_occ + ncas
    rows, cols, drows, dcols = tables(N, n_occ, ncas, False)
    dev, refs = stack_of(N, n_occ, ncas, "symmetric", rows, cols)
    flags = ops.eri_flags(dev[0])
    assert flags & ops.ERI_PQ_SYMMETRIC
    route = V.t2k_route(N, M)
    lds = f"t2k_tri_kernel<{4 * ((M + 3) // 4)}>, LDS {V.t2k_lds_bytes(N, M) / 1024:.1f} KB, N M = {N * M}" if route \
        else "off t2k_tri_kernel"
    what = f"B ({N}, {n_occ}, {ncas}), M = {M}, {lds}"
    H1 = V.hessian_batch(*dev, n_occ, ncas, drows, dcols, flags)
    s1 = batch_share(what + "; flags set", H1, refs)
    H0 = V.hessian_batch(*dev, n_occ, ncas, drows, dcols, 0)
    s0 = batch_share(what + "; flags 0", H0, refs)
    assert s1 <= 1.0 and s0 <= 1.0


@pytest.mark.parametrize("N,n_occ,ncas", V.B_NONSYMMETRIC, ids=[case_id(c) for c in V.B_NONSYMMETRIC])
def test_level_b_stack_with_nonsymmetric_integrals(N, n_occ, ncas):
    """Integrals without any index symmetry and flags 0: the index order of Vk -> T2K -> W -> Kint and of the J chain."""
    rows, cols, drows, dcols = tables(N, n_occ, ncas, False)
    dev, refs = stack_of(N, n_occ, ncas, "nonsymmetric", rows, cols)
    assert ops.eri_flags(dev[0]) == 0
    H = V.hessian_batch(*dev, n_occ, ncas, drows, dcols, 0)
    s = batch_share(f"B ({N}, {n_occ}, {ncas}), nonsymmetric integrals, flags 0", H, refs)
    assert s <= 1.0


def test_level_b_geometry_alone_in_the_stack_and_permuted():
    """(33, 8, 8), the ``t2k_tri_kernel`` route with the LDS opt-in: a geometry has the same bits alone and in the stack,
    and the permuted stack gives the permuted result, under ``torch.equal``.  (Beside the matrix against the gather of
    the full tensor in Level A, the only comparisons of the library with itself in this file.)"""
    N, n_occ, ncas = 33, 8, 8
    rows, cols, drows, dcols = tables(N, n_occ, ncas, False)
    dev, _ = stack_of(N, n_occ, ncas, "symmetric")
    flags = ops.eri_flags(dev[0])
    assert flags & ops.ERI_PQ_SYMMETRIC
    for fl in (flags, 0):
        H = V.hessian_batch(*dev, n_occ, ncas, drows, dcols, fl)
        for k in range(G_B):
            alone = V.hessian_batch(*[t[k:k + 1].contiguous() for t in dev], n_occ, ncas, drows, dcols, fl)
            assert torch.equal(alone[0], H[k]), (fl, k)
        perm = torch.tensor([2, 0, 1], device=H.device)
        Hp = V.hessian_batch(*[t[perm].contiguous() for t in dev], n_occ, ncas, drows, dcols, fl)
        assert torch.equal(Hp, H[perm]), fl


# ---- Level C: OO_energy and OO_pqc_batch -------------------------------------------------------------------------------------
@pytest.mark.parametrize("want", ["matrix", "full"])
@pytest.mark.parametrize("N,n_occ,ncas", V.C_CASES, ids=[case_id(c) for c in V.C_CASES])
def test_level_c_oo_energy_against_the_twin(N, n_occ, ncas, want):
    """``OO_energy.analytic_hessian_matrix`` and ``analytic_hessian``: the Fock matrix comes from the device's CAS path
    (``cas_eval``), the RDMs have the symmetry of a real state."""
    seed = V.seed_of(N, n_occ, ncas)
    h, g, S, U, C = V.problem(N, seed)
    gam, Gam = V.rdms(ncas, seed, "state")
    mol = aoo.Moldata(h, g, S, 31.0, 2 * n_occ + ncas)
    oo = aoo.OO_energy(mol, ncas, ncas, oao_mo_coeff=U)
    rows, cols = V.kappa_tables(N, n_occ, ncas, False)
    assert oo._n_occ == n_occ and np.array_equal(host(oo._kap_row), rows) and np.array_equal(host(oo._kap_col), cols)
    args = (h, g, C, gam, Gam, n_occ, ncas)
    what = f"C ({N}, {n_occ}, {ncas}), {want}"
    if want == "matrix":
        H = oo.analytic_hessian_matrix(gam, Gam, mo_coeff=C)
        s = held(what, host(H), V.hessian_twin(*args, rows, cols), V.hessian_bound(*args, rows, cols))
    else:
        H = oo.analytic_hessian(gam, Gam, mo_coeff=C)
        s = held(what, host(H), V.hessian_twin(*args), V.hessian_bound(*args))
    assert s <= 1.0


def test_level_c_one_call_batch_kappa_block_against_the_twin():
    """``OO_pqc_batch.energy_gradient_hessian`` (``oovqe_oo_hessian_batch``) at N = 33 with 30 electrons (M = 16,
    N M = 528), two geometries: the kappa-kappa block is a block of a larger matrix (ldh > n_kappa), its chains run on
    the forked stream and share stage 1 with the evaluation.  Held to the twin with the oracle's RDMs of each geometry's
    circuit at its theta and the orbitals the batch itself holds."""
    from tests.test_newton_gpu import _batch_of
    N, n_occ, ncas = V.C_BATCH
    G = 2
    pqc, batch, objs, probs = _batch_of(N, G, nelec=30)
    assert batch._n_occ == n_occ and batch.ncas == ncas and (batch.eri_flags & ops.ERI_PQ_SYMMETRIC)
    assert V.t2k_route(N, n_occ + ncas) and pqc.n_qubits <= 10
    thetas = torch.tensor(np.random.default_rng(17).uniform(0, 2 * np.pi, (G, pqc.theta_shape)))
    E, grad, H = batch.energy_gradient_hessian(thetas.cuda())
    torch.cuda.synchronize()
    nt, nk = batch.n_theta, batch.n_kappa
    assert tuple(H.shape) == (G, nt + nk, nt + nk) and nt > 0
    rows, cols = host(batch._kap_row), host(batch._kap_col)
    assert np.array_equal(rows, V.kappa_tables(N, n_occ, ncas, False)[0])
    opqc = R.OraclePQC(3, 4, "ucc")
    worst = 0.0
    for k in range(G):
        g1, g2 = opqc.get_rdms(thetas[k])
        args = (probs[k]["int1e_ao"], probs[k]["int2e_ao"], host(batch.mo_coeff[k]), g1.numpy(), g2.numpy(), n_occ, ncas)
        worst = max(worst, held(f"C one-call batch ({N}, {n_occ}, {ncas}), geometry {k}", host(H[k, nt:, nt:]),
                                V.hessian_twin(*args, rows, cols), V.hessian_bound(*args, rows, cols)))
    assert worst <= 1.0


# ---- oovqe_fock_core_active ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,n_occ,ncas", V.FOCK_CASES, ids=[case_id(c) for c in V.FOCK_CASES])
def test_fock_core_and_active_against_the_oracles_formulas(N, n_occ, ncas):
    """``fock_core`` and ``fock_active`` for MO integrals and a 1-RDM without any index symmetry against the oracle's two
    formulas in numpy; without a core ``fock_core`` is ``h_mo`` bit for bit."""
    seed = V.seed_of(N, n_occ, ncas)
    h, g, S, U, C = V.problem(N, seed)
    g = V.nonsymmetric(g, seed)
    h = h + 0.1 * np.random.default_rng(seed + 4).standard_normal(h.shape)
    gam, _ = V.rdms(ncas, seed, "plain")
    dh, dg, dgam = to_dev(h), to_dev(g), to_dev(gam)
    FI = torch.empty((N, N), dtype=F64, device=dg.device)
    FA = torch.empty((N, N), dtype=F64, device=dg.device)
    _lib.check(_lib.load().oovqe_fock_core_active(_lib.dptr(dh), _lib.dptr(dg), _lib.dptr(dgam), N, n_occ, ncas,
                                                  _lib.dptr(FI), _lib.dptr(FA), _lib.stream_ptr()), "oovqe_fock_core_active")
    torch.cuda.synchronize()
    core, active = V.fock_core_active_host(h, g, gam, n_occ, ncas)
    b_core, b_active = V.fock_core_active_bounds(h, g, gam, n_occ, ncas)
    s_core = V.share(np.abs(host(FI) - core), b_core)
    s_active = V.share(np.abs(host(FA) - active), b_active)
    print(f"fock_core_active ({N}, {n_occ}, {ncas}): largest error core {np.abs(host(FI) - core).max():.2e}, active "
          f"{np.abs(host(FA) - active).max():.2e}; largest error / bound: core {s_core:.2g}, active {s_active:.2g}")
    assert s_core <= 1.0 and s_active <= 1.0
    if n_occ == 0:
        assert torch.equal(FI, dh)


# ---- refusals before any launch ----------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    """``ncas`` = 0, ``n_occ + ncas > N``, ``batch`` = 0 and 65536, no output requested, and ``n_kappa`` = 0 with the
    matrix requested: an error code (the wrapper raises), and neither the output nor the workspace is written."""
    N, n_occ, ncas = 6, 2, 2
    h, g, C, gam, Gam = geometry(N, n_occ, ncas, 0, "plain", "symmetric")
    rows, cols, drows, dcols = tables(N, n_occ, ncas, False)
    nk = len(rows)
    fock = V.fock_twin(h, g, C, gam, Gam, n_occ, ncas)
    d = [to_dev(x) for x in (g, h, C, gam, Gam, fock)]
    lib = _lib.load()
    wsz = int(lib.oovqe_orbital_hessian_work_size(N, N, N))           # enough for any n_occ + ncas <= N
    work = torch.full((wsz,), 7.0, dtype=F64, device=d[0].device)
    Hm = torch.full((nk, nk), 7.0, dtype=F64, device=d[0].device)
    Hf = torch.full((N,) * 4, 7.0, dtype=F64, device=d[0].device)
    p, ip = _lib.dptr, lambda t: _lib.dptr(t, torch.int32)

    def single(n_occ_, ncas_, n_kappa_, Hm_, Hf_):
        return lib.oovqe_orbital_hessian(*[p(x) for x in d], N, n_occ_, ncas_, ip(drows), ip(dcols), n_kappa_, p(work),
                                         p(Hm_), p(Hf_), _lib.stream_ptr())

    def stack(batch_):
        return V.hessian_batch_rc(*d, N, n_occ, ncas, drows, dcols, nk, batch_, work, Hm, 0)

    refused = {"ncas = 0": single(n_occ, 0, nk, Hm, Hf), "n_occ + ncas > N": single(N - 1, 2, nk, Hm, Hf),
               "no output requested": single(n_occ, ncas, nk, None, None), "n_kappa = 0": single(n_occ, ncas, 0, Hm, None),
               "batch = 0": stack(0), "batch = 65536": stack(65536)}
    torch.cuda.synchronize()
    print("refusals:", refused)
    assert all(rc != 0 for rc in refused.values()), refused
    assert bool((work == 7.0).all()) and bool((Hm == 7.0).all()) and bool((Hf == 7.0).all())
    with pytest.raises(_lib.OovqeError):
        ops.orbital_hessian(*d, n_occ, ncas, drows, dcols, want_matrix=False, want_full=False)
    with pytest.raises(_lib.OovqeError):
        ops.orbital_hessian(*d, n_occ, 0, drows, dcols)
    # the same arguments are served when nothing is wrong with them
    assert single(n_occ, ncas, nk, Hm, Hf) == 0 and stack(1) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(Hm).all()) and not bool((Hf == 7.0).all())
