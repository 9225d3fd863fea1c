"""Dipole and second-moment integrals on the host side: the host twin ``gaussian.moment_integrals_from_table`` against
quadrature and its identities, the kernel bodies of csrc/gto_moments.hip run on the CPU against the host twin, and the
interface (header, bindings, refusals).  No GPU.

Bounds: quadrature 1e-12 (measured 4.3e-14 on a 181^3 grid over [-9, 9]^3 Bohr, values up to 4.8); origin shift 1e-13
(measured 4.4e-16 ... 1.8e-15); the kernel bodies against the host twin ``TOL_M`` of tests/_moments.py (measured
2.7e-15)."""
import os
import re

import numpy as np
import pytest

from tests import _gto_d as D
from tests import _moments as M
from auto_oo_amd import _lib, gaussian, gto

BOHR = gaussian.BOHR
ORIGIN_BOHR = M.ORIGIN / BOHR


# ---- 1. host twin ---------------------------------------------------------------------------------------------------------
def test_host_twin_against_quadrature():
    """M1 over its 17 Cartesian functions (A: s 0, d 1..6; B: p 7..9, d 10..15; C: s 16): element pairs of all six pair
    classes, a d-d pair on one shell and d-d pairs across centres, all 9 components and the overlap, at a non-zero
    origin, against the trapezoid rule."""
    basis = D.m1_basis("cartesian")
    xyz = D.M1_XYZ / BOHR
    shells = gaussian.shells_from_table(basis.table, xyz)
    twin = M.host_moments(basis, D.M1_XYZ, 2, M.ORIGIN)
    S = M.host_overlap(basis, D.M1_XYZ)
    pairs = [(16, 0), (8, 0), (9, 7), (3, 16), (5, 8), (2, 1), (6, 6), (14, 4), (10, 1)]
    worst = worst_s = 0.0
    for mu, nu in pairs:
        quad, s = M.quadrature_moments(shells[mu], shells[nu], ORIGIN_BOHR)
        worst = max(worst, np.abs(quad - twin[:, mu, nu]).max())
        worst_s = max(worst_s, abs(s - S[mu, nu]))
    print(f"host twin against quadrature: moments {worst:.2e}, overlap {worst_s:.2e}, largest value "
          f"{np.abs(twin).max():.3g}")
    assert np.abs(twin).max() > 1.0
    assert worst < 1e-12 and worst_s < 1e-12


@pytest.mark.parametrize("form", ["spherical", "cartesian"])
def test_host_twin_identities(form):
    basis = D.m1_basis(form)
    S = M.host_overlap(basis, D.M1_XYZ)
    m0 = M.host_moments(basis, D.M1_XYZ, 2)
    mo = M.host_moments(basis, D.M1_XYZ, 2, M.ORIGIN)
    O = ORIGIN_BOHR
    assert m0.shape == (9, basis.nao, basis.nao)
    # order 1 is the head of order 2 (the twin itself, not the cache of tests/_moments.py); symmetric in (mu, nu)
    hf = M.hf_basis()
    two = gaussian.moment_integrals_from_table(hf.table, M.HF_XYZ / BOHR, "spherical", 2, O)
    assert np.array_equal(gaussian.moment_integrals_from_table(hf.table, M.HF_XYZ / BOHR, "spherical", 1, O), two[:3])
    assert np.abs(two - M.host_moments(hf, M.HF_XYZ, 2, M.ORIGIN)).max() == 0.0
    assert np.array_equal(mo, mo.transpose(0, 2, 1))
    # the shift of the origin is exact: r - O, (r_i - O_i)(r_j - O_j)
    err = max(np.abs(mo[d] - (m0[d] - O[d] * S)).max() for d in range(3))
    k = 3
    for i in range(3):
        for j in range(i, 3):
            want = m0[k] - O[i] * m0[j] - O[j] * m0[i] + O[i] * O[j] * S
            err = max(err, np.abs(mo[k] - want).max())
            k += 1
    print(f"{form}: origin shift identity {err:.2e}")
    assert err < 1e-13
    # the spherical form is the transform of the Cartesian one
    U = gaussian.basis_transform(D.m1_basis("cartesian").table, form)
    cart = gaussian.moment_integrals_from_table(basis.table, D.M1_XYZ / BOHR, "cartesian", 2, O)
    assert np.abs(mo - U @ cart @ U.T).max() < 1e-14


def test_host_twin_refuses_other_orders():
    basis = M.hf_basis()
    for order in (0, 3):
        with pytest.raises(ValueError, match=f"order = {order}"):
            gaussian.moment_integrals_from_table(basis.table, M.HF_XYZ / BOHR, "spherical", order)


# ---- 2. the kernel bodies as host functions -----------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["spherical", "cartesian"])
def test_kernel_bodies_on_the_cpu_against_the_host_twin(form):
    """ds, dp, dd (workgroup bodies, one lane) and ss, ps, pp (register bodies, SPLIT = 1) of M1: every element
    written, plain M1 within TOL_M of the host twin; the stack plain, shifted, moved exactly symmetric, order 1 = head
    of order 2, and a geometry alone with the bits it has in the stack."""
    basis = D.m1_basis(form)
    got = M.run_host_bodies(basis, M.M1_STACK, 2, M.ORIGIN)
    assert not np.isnan(got).any()
    worst = np.abs(got[0] - M.host_moments(basis, D.M1_XYZ, 2, M.ORIGIN)).max()
    print(f"{form}: kernel bodies on the CPU against the host twin {worst:.2e} (TOL_M {M.TOL_M:.2e})")
    assert worst < M.TOL_M
    assert np.array_equal(got, got.transpose(0, 1, 3, 2))
    assert np.array_equal(M.run_host_bodies(basis, M.M1_STACK, 1, M.ORIGIN), got[:, :3])
    # a geometry alone has the bits it has in the stack
    assert np.array_equal(M.run_host_bodies(basis, M.M1_STACK[2:], 2, M.ORIGIN)[0], got[2])


def test_kernel_bodies_on_the_cpu_s_and_p_classes():
    for basis, xyz in ((M.h2_basis(), M.H2_XYZ), (M.hf_basis(), M.HF_XYZ)):
        got = M.run_host_bodies(basis, xyz[None], 2)[0]
        err = np.abs(got - M.host_moments(basis, xyz, 2)).max()
        print(f"{basis.symbols}: kernel bodies on the CPU against the host twin {err:.2e}")
        assert err < M.TOL_M


def test_tolerance_is_the_measured_one():
    assert M.TOL_M == 10 * max(M.HOST_TWIN_ERROR, M.HOST_BODY_ERROR) and M.TOL_M >= 4.3e-13


# ---- 3. interface -----------------------------------------------------------------------------------------------------------
def test_header_bindings_and_exports():
    with open(os.path.join(M.ROOT, "include", "oovqe.h")) as fh:
        hdr = fh.read()
    assert int(re.search(r"#define OOVQE_GTO_MAX_MOMENT (\S+)", hdr).group(1), 0) == gto.MAX_MOMENT == 2
    lib = _lib.load()
    for name in ("oovqe_gto_moments_batch", "oovqe_gto_moments_expect_batch"):
        assert re.search(rf"\bint {name}\(", hdr)
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES["oovqe_gto_moments_batch"][1]) == 15
    assert len(_lib.SIGNATURES["oovqe_gto_moments_expect_batch"][1]) == 13
    import auto_oo_amd as aoo
    from auto_oo_amd import properties
    assert aoo.DEBYE == properties.DEBYE == 2.541746473
    assert aoo.multipole_moments is properties.multipole_moments
    assert aoo.traceless_quadrupole is properties.traceless_quadrupole
    assert aoo.moment_integrals_batch is gto.moment_integrals_batch and aoo.properties is properties
    for name in ("dipole_moment", "multipole_moments", "rhf_dipole_moment", "casci_dipole_matrix"):
        assert callable(getattr(aoo.OO_pqc_batch, name))
    assert gaussian.MOMENT_COMPONENTS[3:] == gaussian.CARTESIAN_D


@pytest.mark.parametrize("order", [0, 3])
def test_an_order_outside_1_and_2_is_refused_with_a_text_that_names_it(order):
    """By the C entry point before anything is launched (no device is needed to be refused), and in Python."""
    lib = _lib.load()
    rc = lib.oovqe_gto_moments_batch(1, None, 1, None, None, 1, None, 1, None, 1, order, None, None, None, None)
    assert rc < 0
    assert f"order = {order}".encode() in lib.oovqe_last_error()
    with pytest.raises(ValueError, match=f"order = {order}"):
        gto.moment_integrals_batch(M.hf_basis(), M.HF_XYZ[None], order=order)
    with pytest.raises(ValueError, match=f"order = {order}"):
        gto.moment_components(order)
    assert (gto.moment_components(1), gto.moment_components(2)) == (3, 9)


def test_the_contraction_refuses_other_component_counts():
    lib = _lib.load()
    assert lib.oovqe_gto_moments_expect_batch(None, 6, 4, 1, None, 1, 1, None, None, None, None, None, None) < 0
    assert b"ncomp = 6" in lib.oovqe_last_error()


def test_traceless_quadrupole():
    """A charge q at height z: Q_zz = q z^2, Theta_zz = q z^2, Theta_xx = Theta_yy = -q z^2 / 2; trace zero always."""
    from auto_oo_amd import properties
    Q = np.zeros((3, 3))
    Q[2, 2] = 0.7 * 1.3 ** 2
    T = properties.traceless_quadrupole(Q)
    assert np.allclose(np.diag(T), [-0.5 * Q[2, 2], -0.5 * Q[2, 2], Q[2, 2]], atol=1e-15)
    R = np.random.default_rng(3).standard_normal((4, 3, 3))
    R = R + R.transpose(0, 2, 1)
    T = properties.traceless_quadrupole(R)
    assert np.abs(np.trace(T, axis1=1, axis2=2)).max() < 1e-14 and np.allclose(T, T.transpose(0, 2, 1))
    import torch
    assert np.allclose(properties.traceless_quadrupole(torch.as_tensor(R)).numpy(), T, atol=1e-15)
