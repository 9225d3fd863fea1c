"""Host-side checks of the ADAPT-VQE feature (no device): the new symbols, the operator pools and their refusals, the
host twin of tests/_adapt.py against the CPU oracle's RDMs, and the non-vacuity of the molecule case the device tests
compare on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import auto_oo_amd as aoo
from auto_oo_amd import _lib, adapt, excitations as X
from oracle import cpu_ref as R
from tests import _adapt as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("oovqe_pool_gradients_batch", "oovqe_pool_gradients_from_coefficients_batch",
       "oovqe_pool_gradients_from_coefficients_work_size")
SPACES = [(2, 2), (3, 4), (4, 3), (4, 4), (6, 6)]         # (ncas, nelecas)


def test_new_symbols_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "oovqe.h")) as fh:
        header = fh.read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    for name in ("adapt", "OperatorPool", "adapt_vqe", "AdaptResult"):
        assert hasattr(aoo, name) and name in aoo.__all__
    assert hasattr(aoo.OO_pqc, "pool_gradients")
    assert hasattr(aoo.OO_pqc_batch, "pool_gradients") and hasattr(aoo.OO_pqc_batch, "set_circuit")


def test_work_size_answers_without_a_device():
    lib = _lib.load()
    for ncas, na, nb, batch in ((3, 3, 3, 1), (4, 6, 6, 3), (8, 70, 70, 256)):
        assert (lib.oovqe_pool_gradients_from_coefficients_work_size(ncas, na, nb, batch)
                >= lib.oovqe_sector_work_size(ncas, na, nb, batch) + batch * na * nb)
    assert lib.oovqe_pool_gradients_from_coefficients_work_size(3, 3, 3, 0) == 0


@pytest.mark.parametrize("ncas,nelecas", SPACES)
def test_pool_sizes(ncas, nelecas):
    n = 2 * ncas
    singles, doubles = X.excitations(nelecas, n)
    sd = aoo.OperatorPool(ncas, nelecas, "sd")
    assert len(sd) == len(singles) + len(doubles) == X.uccd_gates(ncas, nelecas, add_singles=True)[1]
    assert len(aoo.OperatorPool(ncas, nelecas, "pair")) == len(X.generalized_pair_doubles(range(n)))
    assert len(aoo.OperatorPool(ncas, nelecas, "gsd")) == A.gsd_count(n)


def test_sd_pool_is_the_gate_table_of_uccsd_and_gsd_doubles_agree_with_fde_gate():
    ncas, nelecas = 3, 4
    n = 2 * ncas
    gates, n_theta = X.uccd_gates(ncas, nelecas, add_singles=True)
    pool = aoo.OperatorPool(ncas, nelecas, "sd")
    fields = lambda g: (g.mask_hi, g.mask_lo, g.mask_par, g.sign)                        # noqa: E731
    for k in range(n_theta):
        assert [fields(g) for g in pool.operators[k]] == [fields(g) for g in gates if g.theta_idx == k]
    _, doubles = X.excitations(nelecas, n)
    for s, r, q, p in doubles:
        mine = adapt.gsd_double_gate([s, r], [q, p], n, 0)
        assert fields(mine) == fields(X.fde_gate(range(s, r + 1), range(q, p + 1), n, 0))


@pytest.mark.parametrize("kind", ["sd", "gsd", "pair"])
@pytest.mark.parametrize("ncas,nelecas", SPACES)
def test_every_operator_conserves_the_sector(kind, ncas, nelecas):
    n = 2 * ncas
    pool = aoo.OperatorPool(ncas, nelecas, kind)
    alpha = sum(1 << (n - 1 - w) for w in range(0, n, 2))
    beta = sum(1 << (n - 1 - w) for w in range(1, n, 2))
    assert pool.op_first[0] == 0 and pool.op_first[-1] == pool.n_gates == len(pool.gate_sign)
    for k, op in enumerate(pool.operators):
        assert 1 <= len(op) <= 4
        for g in op:
            assert g.theta_idx == k and g.mask_hi & g.mask_lo == 0
            for spin in (alpha, beta):
                assert bin(g.mask_hi & spin).count("1") == bin(g.mask_lo & spin).count("1")


def test_custom_pools_and_refusals():
    ncas, nelecas, n = 3, 4, 6
    rot = X.orbital_rotation_gates([0, 1, 2, 3], n, 7)             # two gates on one parameter
    pool = aoo.OperatorPool(ncas, nelecas, [rot, [X.fse_gate(range(0, 3), n, 0)]])
    assert len(pool) == 2 and pool.n_gates == 3 and list(pool.op_first) == [0, 2, 3]
    assert [g.theta_idx for g in pool.gates] == [0, 0, 1]
    assert [g.theta_idx for g in pool.operator_gates(0, 5)] == [5, 5]
    with pytest.raises(ValueError, match="conserve"):              # alpha -> beta: leaves (N_alpha, N_beta)
        aoo.OperatorPool(ncas, nelecas, [[X.fse_gate(range(0, 2), n, 0)]])
    with pytest.raises(ValueError, match="conserve"):              # two alphas -> one alpha, one beta
        aoo.OperatorPool(ncas, nelecas, [[X.double_excitation_gate([0, 2, 4, 5], n, 0)]])
    with pytest.raises(ValueError):
        aoo.OperatorPool(ncas, nelecas, [])
    with pytest.raises(ValueError):
        aoo.OperatorPool(ncas, nelecas, [[X.fse_gate(range(0, 3), n, 0)] * 5])
    with pytest.raises(ValueError):
        aoo.OperatorPool(ncas, nelecas, "qubit")


def test_twin_quadratic_form_equals_the_rdm_contraction():
    """v^T Hop v == c1 . gamma(v) + c2 . Gamma(v) with the oracle's RDMs, random v and coefficients, CAS(4e,3o)."""
    tw = A.Twin(3, 2, 2)
    rng = np.random.default_rng(7)
    v = rng.standard_normal(tw.Dc)
    c1, c2 = rng.standard_normal((3, 3)), rng.standard_normal((3, 3, 3, 3))
    g1, g2 = R.rdms_from_state(torch.as_tensor(tw.embed(v)), R.RdmOperators(3))
    ref = float((c1 * g1.numpy()).sum() + (c2 * g2.numpy()).sum())
    mine = float(v @ tw.hop(c1, c2) @ v)
    scale = float(np.abs(v) @ tw.hop(c1, c2, absolute=True) @ np.abs(v))
    print(f"v^T Hop v = {mine!r}, c1 . gamma + c2 . Gamma = {ref!r}, scale {scale:.3e}")
    assert abs(mine - ref) <= (3 ** 4 + 3 ** 2 + tw.Dc) * A.EPS * scale


def test_twin_gradient_is_the_derivative_of_the_appended_gate():
    """g of the twin == d/dt of Q(U(t) psi) by central differences of the closed-form rotation."""
    tw = A.Twin(3, 2, 2)
    psi, c1, c2 = A.random_case(tw, 1, 11)
    pool = aoo.OperatorPool(3, 4, "gsd")
    g, _, _ = A.pool_gradients(tw, pool, psi[0], c1[0], c2[0])
    H = np.asarray(tw.hop(c1[0], c2[0]), dtype=float)
    h = 1e-5
    for k in (0, 5, 11, 23):
        G = np.asarray(tw.generator(pool.operators[k])[0], dtype=float)
        from scipy.linalg import expm
        q = [float((expm(t * G) @ psi[0]) @ H @ (expm(t * G) @ psi[0])) for t in (h, -h)]
        assert abs((q[0] - q[1]) / (2 * h) - g[k]) < 1e-8


def test_molecule_case_is_not_vacuous():
    """The seeds of tests/_adapt.formaldimine_case: with the CPU oracle's circuit state and active-space coefficients
    the twin finds 0 of the 8 "sd" gradients and 4 of the 24 "gsd" gradients below 1e-8 -- at most a quarter."""
    mol, C, theta = A.formaldimine_case()
    omol = R.OracleMol(mol.int1e_ao, mol.int2e_ao, mol.overlap, mol.nuc, mol.nelectron)
    opqc = R.OraclePQC(3, 4, "ucc")
    oo = R.OracleOOPQC(opqc, omol, 3, 4, torch.as_tensor(C))
    _, c1, c2 = oo.get_active_integrals(oo.mo_coeff)
    tw = A.Twin(3, 2, 2)
    psi = tw.restrict(opqc.qnode(torch.as_tensor(theta)).real.numpy())
    for kind, small in (("sd", 0), ("gsd", 4)):
        g, _, _ = A.pool_gradients(tw, aoo.OperatorPool(3, 4, kind), psi, np.asarray(c1), np.asarray(c2))
        n = int((np.abs(g) < 1e-8).sum())
        print(kind, len(g), "operators,", n, "below 1e-8, largest", np.abs(g).max())
        assert n == small and 4 * n <= len(g)
