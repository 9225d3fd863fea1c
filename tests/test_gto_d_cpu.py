"""d shells on the host side: the tables of ``GTOBasis(..., d_functions=...)``, the limits of the C ABI, the host twin
of the device kernels (``gaussian.integrals_from_table``) and, independently of any l = 2 code path, the host d
integrals against finite differences of the pinned s-type integrals.  No GPU.

Bounds: the overlap diagonal 1e-14 (measured 6.7e-16); the RHF energy under a rigid motion 1e-9 Ha (the project's
energy tolerance); the finite-difference comparison 10 x the disagreement between the step sizes 0.02 and 0.01 Bohr,
computed in the test from the s-type integrals alone (measured for xx / zz / xy / yz at h = 0.01: one-electron error
9.8e-10 / 7.6e-10 / 4.2e-9 / 5.2e-9 against bounds of 1.5e-7 / 1.1e-7 / 6.3e-7 / 7.7e-7, two-electron 7.3e-11 /
8.5e-11 / 2.9e-10 / 3.8e-10 against 1.1e-8 / 1.3e-8 / 4.3e-8 / 5.6e-8)."""
import os
import re

import numpy as np
import pytest

from tests import _gto_d as D
from auto_oo_amd import _lib, gaussian, gto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. tables ------------------------------------------------------------------------------------------------------
def test_both_forms_build_with_the_documented_sizes_and_fields():
    sph, cart = D.m1_basis("spherical"), D.m1_basis("cartesian")
    assert (sph.nao, cart.nao) == (15, 17) and sph.nshell == cart.nshell == 5
    assert sph.max_l == cart.max_l == 2 and sph.max_nprim == 2 and sph.nelectron == 14
    assert sph.shells[:, 1].tolist() == [0, 2, 1, 2, 0]
    assert cart.shells[:, 1].tolist() == [0, 2 | gto.CARTESIAN, 1, 2 | gto.CARTESIAN, 0]
    assert np.array_equal(sph.exps, cart.exps) and np.array_equal(sph.coefs, cart.coefs)
    assert D.m2_basis().nao == 18
    # the coefficients of a d shell are those that normalise xx: a single primitive x^2 exp(-a r^2)
    a = 0.8
    c = sph.coefs[sph.shells[3, 3]]
    assert c * c * 3.0 * (np.pi / (2 * a)) ** 1.5 / (4 * a) ** 2 == pytest.approx(1.0, abs=1e-14)


def test_component_order_is_the_documented_one():
    """Cartesian: xx, xy, xz, yy, yz, zz; spherical: xy, yz, 3z^2 - r^2, xz, x^2 - y^2 with the signs of these
    polynomials -- the rows of the transform applied to the (normalised) monomials, at random points."""
    assert gaussian.CARTESIAN_D == ((2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2))
    table = [(0, 2, np.array([0.7]), np.array([1.0]))]
    assert [s.lmn for s in gaussian.shells_from_table(table, np.zeros((1, 3)))] == list(gaussian.CARTESIAN_D)
    assert np.array_equal(gaussian.basis_transform(table, "cartesian"), np.eye(6))
    U = gaussian.basis_transform(table, "spherical")
    assert U.shape == (5, 6)
    x, y, z = np.random.default_rng(5).standard_normal((3, 40))
    mono = np.stack([x ** l * y ** m * z ** n * gaussian.component_norm((l, m, n)) for l, m, n in gaussian.CARTESIAN_D])
    want = np.stack([x * y, y * z, 3 * z * z - (x * x + y * y + z * z), x * z, x * x - y * y])
    ratio = (U @ mono) / want
    assert (ratio > 0).all()
    for m in range(5):
        assert np.allclose(ratio[m], ratio[m, 0], rtol=1e-12)


def test_what_stays_out_of_scope_raises():
    d = {"H": [(0, [1.0], [1.0]), ("d", [0.8], [1.0])]}
    with pytest.raises(ValueError, match="l = 2") as err:
        gto.GTOBasis(["H"], d)
    assert "spherical" in str(err.value) and "cartesian" in str(err.value)
    with pytest.raises(ValueError, match="d_functions"):
        gto.GTOBasis(["H"], d, d_functions="5d")
    for form in ("spherical", "cartesian"):
        with pytest.raises(ValueError, match="l = 3"):
            gto.GTOBasis(["H"], {"H": [("f", [0.8], [1.0])]}, d_functions=form)
        with pytest.raises(ValueError, match="primitives"):
            gto.GTOBasis(["H"], {"H": [(2, np.ones(gto.MAX_PRIM + 1), np.ones(gto.MAX_PRIM + 1))]}, d_functions=form)
    ok = gto.GTOBasis(["H"], {"H": [(2, np.linspace(0.3, 3.0, gto.MAX_PRIM), np.ones(gto.MAX_PRIM))]},
                      d_functions="spherical")
    assert ok.max_nprim == gto.MAX_PRIM == 10 and ok.nao == 5


def test_header_macros_and_size_functions():
    with open(os.path.join(ROOT, "include", "oovqe.h")) as fh:
        hdr = fh.read()
    for macro, value in (("OOVQE_GTO_MAX_L", gto.MAX_L), ("OOVQE_GTO_MAX_PRIM", gto.MAX_PRIM),
                         ("OOVQE_GTO_CARTESIAN", gto.CARTESIAN)):
        assert int(re.search(rf"#define {macro} (\S+)", hdr).group(1), 0) == value
    assert (gto.MAX_L, gto.MAX_PRIM) == (2, 10)
    lib = _lib.load()
    for nshell, nprim, G in ((5, 2, 3), (21, 10, 2), (1, 1, 1)):
        npair = nshell * (nshell + 1) // 2
        ints = nshell + 6 * npair * 2                      # AO offsets and the lists of six pair classes
        want = (((ints + 1) // 2 + 1) & ~1) + G * npair * nprim * nprim * 8
        assert lib.oovqe_gto_work_size(nshell, nprim, G) == want
        # the gradient buffer holds the same tables and pair data in front of its records
        extra = [lib.oovqe_gto_gradient_work_size(nshell, k, 3, G) - lib.oovqe_gto_work_size(nshell, k, G)
                 for k in (1, nprim)]
        assert extra[0] == extra[1] > 0
    assert lib.oovqe_gto_work_size(5, gto.MAX_PRIM + 1, 1) < 0
    assert b"11 primitives" in lib.oovqe_last_error()
    assert lib.oovqe_gto_gradient_work_size(5, gto.MAX_PRIM + 1, 3, 1) < 0


def test_gradients_of_a_d_basis_are_refused_on_the_host():
    basis = D.m1_basis("spherical")
    with pytest.raises(NotImplementedError, match="d shells"):
        gto.gradient_batch(basis, D.M1_XYZ[None])
    gto.refuse_d_gradient(gto.GTOBasis(["H", "F"]))          # s and p: nothing to refuse


# ---- 2. host twin -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["spherical", "cartesian"])
def test_host_functions_are_normalised(form):
    S = D.m1_host(form)[0]
    print(form, "max |S_ii - 1| =", np.abs(np.diag(S) - 1).max(), "smallest eigenvalue", np.linalg.eigvalsh(S).min())
    assert S.shape[0] == (15 if form == "spherical" else 17)
    assert np.abs(np.diag(S) - 1).max() < 1e-14
    assert np.linalg.eigvalsh(S).min() > 0.1


def test_host_rhf_energy_is_invariant_under_a_rigid_motion():
    """Rotation about a generic axis and a translation: the energy moves by less than 1e-9 Ha in both forms (a wrong
    spherical transform or a wrong component norm breaks the rotation invariance of the space a d shell spans)."""
    for form in ("spherical", "cartesian"):
        e = []
        for which in ("plain", "moved"):
            S, h, g, nuc = D.m1_host(form, which)
            e.append(gaussian.rhf(h, g, S, 7)[2] + nuc)
        print(form, "RHF", e, "difference", e[0] - e[1])
        assert abs(e[0] - e[1]) < 1e-9


# ---- 3. host d integrals against finite differences of s-type integrals ---------------------------------------------
A, B, C = D.M1_XYZ / gaussian.BOHR
EXP_A = 0.9
CHARGES = [6.0, 7.0, 1.0]
_D1 = {2: -1.0 / 12, 1: 8.0 / 12, -1: -8.0 / 12, -2: 1.0 / 12}             # first derivative, 4th order
_D2 = {2: -1.0 / 12, 1: 16.0 / 12, 0: -30.0 / 12, -1: 16.0 / 12, -2: -1.0 / 12}    # second derivative, 4th order


def _others():
    return [gaussian._Shell(B, (0, 0, 0), [1.3, 0.4], [0.5, 0.6]), gaussian._Shell(B, (0, 1, 0), [0.9], [1.0]),
            gaussian._Shell(C, (0, 0, 0), [0.6], [1.0])]


def _elements(first):
    """The elements in which the first function occurs once: S, T, V against the three others, and (0 j | k l)."""
    shells = [first] + _others()
    S, T, V = gaussian.one_electron_integrals(shells, CHARGES, [A, B, C])
    g = gaussian.electron_repulsion_integrals(shells)[0, 1:, 1:, 1:].ravel()
    return np.concatenate([S[0, 1:], T[0, 1:], V[0, 1:]]), g


def _s_at(delta):
    return _elements(gaussian._Shell(A + np.asarray(delta, dtype=float), (0, 0, 0), [EXP_A], [1.0]))


def _from_differences(lmn, h):
    """x^2 s = (d^2 s / dA_x^2 + 2 a s) / 4 a^2 and x y s = (d^2 s / dA_x dA_y) / 4 a^2 for an unnormalised primitive
    on A, from central differences of 4th order of the s-type integrals; scaled to the normalised d function."""
    axes = [d for d in range(3) for _ in range(lmn[d])]
    one, two = 0.0, 0.0
    if axes[0] == axes[1]:
        for k, w in _D2.items():
            step = np.zeros(3)
            step[axes[0]] = k * h
            a, b = _s_at(step)
            one, two = one + w * a / h ** 2, two + w * b / h ** 2
        a, b = _s_at(np.zeros(3))
        one, two = one + 2 * EXP_A * a, two + 2 * EXP_A * b
    else:
        for k, wk in _D1.items():
            for m, wm in _D1.items():
                step = np.zeros(3)
                step[axes[0]], step[axes[1]] = k * h, m * h
                a, b = _s_at(step)
                one, two = one + wk * wm * a / h ** 2, two + wk * wm * b / h ** 2
    c_s = gaussian._Shell(A, (0, 0, 0), [EXP_A], [1.0]).coefs[0]
    c_d = gaussian.normalised_shell(A, lmn, [EXP_A], [1.0]).coefs[0]
    f = c_d / c_s / (4 * EXP_A ** 2)
    return f * one, f * two


@pytest.mark.parametrize("lmn", [(2, 0, 0), (0, 0, 2), (1, 1, 0), (0, 1, 1)], ids=["xx", "zz", "xy", "yz"])
def test_host_d_integrals_against_differences_of_s_integrals(lmn):
    one, two = _elements(gaussian.normalised_shell(A, lmn, [EXP_A], [1.0]))
    c1, c2 = _from_differences(lmn, 0.02)
    f1, f2 = _from_differences(lmn, 0.01)
    bound1, bound2 = 10 * np.abs(c1 - f1).max(), 10 * np.abs(c2 - f2).max()
    err1, err2 = np.abs(one - f1).max(), np.abs(two - f2).max()
    print(f"{lmn}: one-electron error {err1:.2e} (bound {bound1:.2e}), two-electron {err2:.2e} (bound {bound2:.2e})")
    assert np.abs(one).max() > 1e-2 and np.abs(two).max() > 1e-3        # (the elements compared are not all tiny)
    assert err1 < bound1 and err2 < bound2
