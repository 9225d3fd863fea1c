"""The host twin of the orbital-orbital Hessian (tests/_hessian_scope.py) against the dense, untouched oracle
(oracle/cpu_ref.py: ``analytic_hessian``, ``analytic_hessian_from_integrals``, ``fock_generalized``,
``full_hessian_to_matrix``) at the shapes where the oracle's N^6 einsums take under a second, with RDMs with and without
the symmetry of a real state and with 8-fold symmetric and non-symmetric integrals; the twin against the same
contractions in ``np.longdouble``; and the case table of tests/test_hessian_scope_gpu.py.  The bounds are those of the
device tests (tests/_hessian_scope.py says where they come from)."""
import functools

import numpy as np
import pytest
import torch

from oracle import cpu_ref as R
from tests import _hessian_scope as V

IDS = [f"{n}-{o}-{a}-{'frozen' if f else 'free'}" for n, o, a, f in V.CPU_CASES]


@functools.lru_cache(maxsize=None)
def oracle_of(N, n_occ, ncas, freeze):
    """The oracle's object for a case: ``nelecas = ncas`` and ``nelectron = 2 n_occ + ncas`` put n_occ orbitals in the
    core."""
    h, g, S, U, C = V.problem(N, V.seed_of(N, n_occ, ncas))
    mol = R.OracleMol(h, g, S, 31.0, 2 * n_occ + ncas)
    ooo = R.OracleOOEnergy(mol, ncas, ncas, U, freeze_active=freeze)
    assert len(ooo.occ_idx) == n_occ and (len(ooo.act_idx), len(ooo.virt_idx)) == (ncas, N - n_occ - ncas)
    return ooo


def inputs(N, n_occ, ncas, kind, integrals):
    seed = V.seed_of(N, n_occ, ncas)
    h, g, S, U, C = V.problem(N, seed)
    if integrals == "nonsymmetric":
        g = V.nonsymmetric(g, seed)
        assert np.abs(g - g.transpose(1, 0, 2, 3)).max() > 1e-3 and np.abs(g - g.transpose(2, 3, 0, 1)).max() > 1e-3
    gam, Gam = V.rdms(ncas, seed, kind)
    return h, g, C, gam, Gam


def test_inputs_have_the_symmetry_they_are_named_for():
    gam, Gam = V.rdms(3, 5, "state")
    assert np.array_equal(gam, gam.T)
    assert np.allclose(Gam, Gam.transpose(1, 0, 3, 2), atol=1e-15) and np.allclose(Gam, Gam.transpose(2, 3, 0, 1), atol=1e-15)
    gam, Gam = V.rdms(3, 5, "plain")
    assert np.abs(gam - gam.T).max() > 0.1
    assert np.abs(Gam - Gam.transpose(1, 0, 3, 2)).max() > 0.1 and np.abs(Gam - Gam.transpose(2, 3, 0, 1)).max() > 0.1
    h, g, S, U, C = V.problem(6, 11)
    assert np.abs(C.T @ S @ C - np.eye(6)).max() < 1e-13 and np.abs(U.T @ U - np.eye(6)).max() < 1e-14
    assert np.array_equal(g, g.transpose(1, 0, 2, 3)) and np.array_equal(g, g.transpose(0, 1, 3, 2))


@pytest.mark.parametrize("integrals", ["symmetric", "nonsymmetric"])
@pytest.mark.parametrize("kind", ["plain", "state"])
@pytest.mark.parametrize("N,n_occ,ncas,freeze", V.CPU_CASES, ids=IDS)
def test_twin_against_the_oracle(N, n_occ, ncas, freeze, kind, integrals):
    """Full tensor, gathered matrix and generalized Fock matrix of the twin against the oracle, within the bound of the
    device tests.  Symmetric integrals go through ``analytic_hessian`` (the oracle transforms them itself),
    non-symmetric ones through ``analytic_hessian_from_integrals`` behind the oracle's own general transform."""
    ooo = oracle_of(N, n_occ, ncas, freeze)
    h, g, C, gam, Gam = inputs(N, n_occ, ncas, kind, integrals)
    t = torch.as_tensor
    assert np.abs(ooo.mo_coeff.numpy() - C).max() < 1e-13
    h_mo, g_mo = R.int1e_transform(t(h), t(C)), R.int2e_transform(t(g), t(C))
    if integrals == "symmetric":
        ref = ooo.analytic_hessian(t(gam), t(Gam), mo_coeff=t(C))
    else:
        ref = ooo.analytic_hessian_from_integrals(h_mo, g_mo, t(gam), t(Gam))
    rows, cols = V.kappa_tables(N, n_occ, ncas, freeze)
    tril = np.tril_indices(N, -1)
    assert np.array_equal(rows, tril[0][ooo.params_idx]) and np.array_equal(cols, tril[1][ooo.params_idx])
    assert len(rows) == ooo.n_kappa > 0
    args = (h, g, C, gam, Gam, n_occ, ncas)
    full, bound = V.hessian_twin(*args), V.hessian_bound(*args)
    s_full = V.share(np.abs(full - ref.numpy()), bound)
    mat = V.hessian_twin(*args, rows, cols)
    assert np.array_equal(mat, full[rows, cols][:, rows, cols])
    s_mat = V.share(np.abs(mat - ooo.full_hessian_to_matrix(ref).numpy()), V.hessian_bound(*args, rows, cols))
    F = ooo.fock_generalized(h_mo, g_mo, t(gam), t(Gam)).numpy()
    Ft = V.fock_twin(*args)
    s_fock = V.share(np.abs(Ft - F), V.fock_bound(*args))
    assert not Ft[n_occ + ncas:].any()
    print(f"({N}, {n_occ}, {ncas}) {kind}, {integrals}: max |H| {np.abs(full).max():.3g}, error {np.abs(full - ref.numpy()).max():.2e}; "
          f"largest error / bound: full {s_full:.4f}, matrix {s_mat:.4f}, Fock {s_fock:.4f}")
    assert s_full <= 1.0 and s_mat <= 1.0 and s_fock <= 1.0
    # a wrong or missing term is an error of order one, far above the bound
    assert bound.max() < 1e-9 * np.abs(full).max()


@pytest.mark.parametrize("N,n_occ,ncas,freeze", [c for c in V.CPU_CASES if not c[3]], ids=[i for i in IDS if "free" in i])
def test_twin_within_half_its_bound_of_extended_precision(N, n_occ, ncas, freeze):
    """The fp64 twin against the same contractions in ``np.longdouble``: within half of the two-sided bound."""
    if np.finfo(np.longdouble).eps >= 2.0 ** -60:
        pytest.skip("np.longdouble is no wider than fp64 on this platform")
    worst = 0.0
    for integrals in ("symmetric", "nonsymmetric"):
        args = inputs(N, n_occ, ncas, "plain", integrals) + (n_occ, ncas)
        wide = V.hessian_twin(*args, dtype=np.longdouble)
        assert wide.dtype == np.longdouble
        err = np.abs((V.hessian_twin(*args) - wide).astype(np.float64))
        worst = max(worst, V.share(err, 0.5 * V.hessian_bound(*args)))
        errf = np.abs((V.fock_twin(*args) - V.fock_twin(*args, dtype=np.longdouble)).astype(np.float64))
        worst = max(worst, V.share(errf, 0.5 * V.fock_bound(*args)))
    print(f"({N}, {n_occ}, {ncas}): fp64 twin against np.longdouble, largest error / half bound {worst:.4f}")
    assert worst <= 1.0


def test_a_transposed_index_is_far_outside_the_bound():
    """What the device tests rely on: with RDMs without symmetry, gam -> gam^T moves the Hessian by far more than the
    bound (with the RDMs of a real state it would not move at all)."""
    N, n_occ, ncas = 6, 2, 2
    h, g, C, gam, Gam = inputs(N, n_occ, ncas, "plain", "symmetric")
    H = V.hessian_twin(h, g, C, gam, Gam, n_occ, ncas)
    bound = V.hessian_bound(h, g, C, gam, Gam, n_occ, ncas)
    assert V.share(np.abs(V.hessian_twin(h, g, C, gam.T, Gam, n_occ, ncas) - H), bound) > 1e6
    assert V.share(np.abs(V.hessian_twin(h, g, C, gam, Gam.transpose(2, 3, 0, 1), n_occ, ncas) - H), bound) > 1e6
    gn = V.nonsymmetric(g, 1)
    Hn = V.hessian_twin(h, gn, C, gam, Gam, n_occ, ncas)
    assert V.share(np.abs(V.hessian_twin(h, gn.transpose(1, 0, 3, 2), C, gam, Gam, n_occ, ncas) - Hn), bound) > 1e6


def test_device_case_table():
    """Every case of the device tests has rotations to differentiate (a frozen active space with no core and no virtual
    orbital would have none), and reaches the edge it is listed for."""
    for N, n_occ, ncas, freeze in V.device_cases():
        assert ncas >= 1 and n_occ + ncas <= N
        assert len(V.kappa_tables(N, n_occ, ncas, freeze)[0]) > 0, (N, n_occ, ncas, freeze)
    nk = {c: len(V.kappa_tables(*c)[0]) for c in V.A_BOTH + V.A_MATRIX}
    assert [nk[c] for c in V.A_BOTH] == [1, 10, 13, 79, 60, 108, 80] and nk[V.A_MATRIX[0]] == 1244
    assert 1244 ** 2 > 4096 * 256 and 11 ** 4 <= 64 * 256 < 12 ** 4                       # second trips: matrix, hess_ab
    assert 38 ** 4 <= 8192 * 256 < 39 ** 4                                     # hess_full_kernel: one trip | two
    route = {c: V.t2k_route(c[0], c[1] + c[2]) for c in V.B_CASES}
    assert [c for c in V.B_CASES if not route[c]] == [(49, 8, 8), (24, 9, 8)]
    assert {c[1] + c[2] for c in V.B_CASES if route[c]} >= {1, 2, 4, 5, 8, 9, 12, 13, 16}
    assert V.t2k_lds_bytes(32, 16) == 65536 and V.t2k_lds_bytes(33, 16) > 65536 > V.t2k_lds_bytes(48, 11)
    assert 32 * 16 == 512 and 33 * 16 == 528 == 48 * 11 and V.t2k_lds_bytes(48, 16) == 96 * 1024
    N, n_occ, ncas = V.C_BATCH
    assert N * (n_occ + ncas) == 528 and n_occ + ncas == 16 and 2 * n_occ + 4 == 30
