"""Point-charge embedding, the parts that need no device: the host twin ``gaussian.point_charge_integrals_from_table``
against the nuclear attraction of ``gaussian.one_electron_integrals`` (the same recursions, the charges an axis of
the arrays instead of a loop: agreement to the rounding of a different order of summation, 1e-13 of the largest
element), its linearity in the charges, and the argument checks of the new ``gto`` functions and of
``OO_pqc_batch.from_geometries(point_charges=...)`` that run before the device is touched."""
import numpy as np
import pytest
import torch

import auto_oo_amd as aoo
from auto_oo_amd import gaussian, gto
from auto_oo_amd.batch import OO_pqc_batch
from tests import _charges as C
from tests import _gto_d as D


@pytest.mark.parametrize("name", ["water", "m1-spherical", "m1-cartesian"])
def test_twin_with_the_nuclei_as_charges_is_the_nuclear_attraction(name):
    basis, xyz = C.case(name)
    R = C.bohr(xyz)
    shells = gaussian.shells_from_table(basis.table, R)
    V = gaussian.one_electron_integrals(shells, basis.charges, R)[2]
    U = gaussian.basis_transform(basis.table, basis.d_functions or "spherical")
    ref = U @ V @ U.T
    got = gaussian.point_charge_integrals_from_table(basis.table, R, basis.charges, R, basis.d_functions or "spherical")
    assert got.shape == (basis.nao, basis.nao) and np.array_equal(got, got.T)
    assert np.abs(got - ref).max() < 1e-13 * np.abs(ref).max()


def test_twin_is_linear_in_the_charges():
    basis, xyz = C.case("m1-spherical")
    q, r = C.cloud(xyz, 12)
    q2 = np.random.default_rng(5).uniform(-1, 1, q.size)
    Va, Vb = C.host_operator(basis, xyz, q, r), C.host_operator(basis, xyz, q2, r)
    Vc = C.host_operator(basis, xyz, 0.3 * q - 1.7 * q2, r)
    assert np.abs(Vc - (0.3 * Va - 1.7 * Vb)).max() < 1e-13 * max(np.abs(Va).max(), np.abs(Vb).max())
    # a charge of zero contributes nothing, and the cloud is the sum of its charges
    parts = sum(C.host_operator(basis, xyz, q[k:k + 1], r[k:k + 1]) for k in range(q.size))
    assert np.abs(parts - Va).max() < 1e-13 * np.abs(Va).max()
    assert not C.host_operator(basis, xyz, [0.0], r[3:4]).any()


def test_fixture_cloud_holds_the_hard_cases():
    q, r = C.cloud(C.WATER)
    R, rb = C.bohr(C.WATER), C.bohr(r)
    assert q.size == C.M_MAX and np.abs(q).max() <= 1.0 and (q > 0).any() and (q < 0).any() and q[3] == 0.0
    assert np.linalg.norm(rb[0] - R[0]) == pytest.approx(C.NEAR, rel=1e-12)
    assert np.array_equal(rb[1], R[1])
    assert np.linalg.norm(rb[2] - R[0]) == pytest.approx(50.0, rel=1e-12)
    q2, r2 = C.cloud(C.WATER, on_nucleus=False)
    assert np.linalg.norm(C.bohr(r2)[:, None] - R[None], axis=2).min() > 0.19


def test_point_charge_energy():
    Z, R = np.array([8.0, 1.0]), np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 2.0]])
    e = gaussian.point_charge_energy(Z, R, [0.5, -1.0], [[0.0, 0.0, -1.0], [0.0, 3.0, 2.0]])
    assert e == pytest.approx(8 * 0.5 / 1 + 1 * 0.5 / 3 - 8 / np.sqrt(13) - 1 / 3, rel=1e-15)
    with pytest.raises(ValueError):
        gaussian.point_charge_energy(Z, R, [0.5], [[0, 0, 1.0], [0, 0, 2.0]])


def test_exports():
    assert aoo.point_charge_integrals_batch is gto.point_charge_integrals_batch
    assert aoo.point_charge_gradient_batch is gto.point_charge_gradient_batch


BAD = [
    ("no charges", np.zeros(0), np.zeros((0, 3))),
    ("too many", np.zeros(65536), np.zeros((65536, 3))),
    ("mismatched M", np.zeros(4), np.zeros((5, 3))),
    ("mismatched G", np.zeros((2, 4)), np.zeros((4, 3))),
    ("no xyz", np.zeros(4), np.zeros((4, 2))),
    ("NaN position", np.ones(2), np.array([[0.0, np.nan, 1.0], [1.0, 1.0, 1.0]])),
    ("infinite charge", np.array([1.0, np.inf]), np.ones((2, 3))),
]


@pytest.mark.parametrize("what,q,r", BAD, ids=[b[0] for b in BAD])
def test_bad_charges_are_refused_on_the_host(what, q, r):
    basis = C.water_basis()
    with pytest.raises(ValueError):
        gto.point_charge_integrals_batch(basis, C.WATER, q, r)
    with pytest.raises(ValueError):
        gto.point_charge_gradient_batch(basis, C.WATER, q, r, torch.zeros((1, 7, 7), dtype=torch.float64))
    with pytest.raises(ValueError):
        OO_pqc_batch.from_geometries(None, basis, C.WATER[None], 2, 2, point_charges=(q, r))


def test_bad_shapes_of_the_device_level_functions():
    basis = C.water_basis()
    xyz = torch.zeros((2, 3, 3), dtype=torch.float64)
    q, r = torch.zeros((2, 4), dtype=torch.float64), torch.zeros((2, 4, 3), dtype=torch.float64)
    for args in ((xyz[:, :2], q, r), (xyz, q[:1], r), (xyz, q, r[:, :3]), (xyz, q[0], r), (xyz, q[:, :0], r[:, :0])):
        with pytest.raises(ValueError):
            gto.point_charge_integrals_into(basis, *args)
        with pytest.raises(ValueError):
            gto.point_charge_gradient_into(basis, *args, torch.zeros((2, 7, 7), dtype=torch.float64))
    with pytest.raises(ValueError, match="dm1"):
        gto.point_charge_gradient_batch(basis, C.WATER, np.ones(3), np.ones((3, 3)),
                                        torch.zeros((1, 7, 6), dtype=torch.float64))
    with pytest.raises(ValueError, match="pair"):
        OO_pqc_batch.from_geometries(None, basis, C.WATER[None], 2, 2, point_charges=np.ones(3))


def test_d_shells_are_refused_by_the_gradient_before_anything_else():
    basis = D.m2_basis()
    with pytest.raises(NotImplementedError, match="d shells"):
        gto.point_charge_gradient_batch(basis, C.WATER, np.ones(3), np.ones((3, 3)), None)
    with pytest.raises(NotImplementedError, match="d shells"):
        gto.point_charge_gradient_into(basis, None, None, None, None)


def test_charges_for_a_batch_built_without_them():
    batch = OO_pqc_batch.__new__(OO_pqc_batch)
    batch.basis, batch.charge_q, batch.charge_xyz_bohr = C.water_basis(), None, None
    with pytest.raises(ValueError, match="without point charges"):
        batch.set_geometries(C.WATER[None], point_charges=(np.ones(3), np.ones((3, 3))))


def test_work_size_answers_without_a_device():
    lib = aoo._lib.load()
    base = int(lib.oovqe_gto_work_size(5, 3, 3))
    assert int(lib.oovqe_gto_point_charge_gradient_work_size(5, 3, 3, 3, 130)) == base + 3 * 3 * 3 * 3
    assert int(lib.oovqe_gto_point_charge_gradient_work_size(5, 3, 3, 3, 10000)) == base + 3 * 157 * 3 * 3
    for M in (0, 65536):
        assert int(lib.oovqe_gto_point_charge_gradient_work_size(5, 3, 3, 3, M)) < 0
    assert int(lib.oovqe_gto_point_charge_gradient_work_size(5, 3, 3, 65536, 4)) < 0
