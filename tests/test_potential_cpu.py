"""Electrostatic potential and field on the host side: the host twin ``gaussian.potential_from_table`` against a closed
form that shares nothing with the McMurchie-Davidson code, the bounds of tests/_potential.py re-measured, the kernel
bodies of csrc/gto_potential.hip run on the CPU against the host twin and against differences of it, the interface
(header, bindings, refusals) and ``properties.fit_esp_charges``.  No GPU.

Measured here (``python -m pytest tests/test_potential_cpu.py -s``; every test prints its figures before it asserts):
host twin against the closed form 1.2e-15 relative, the kernel bodies 4.4e-16 (potential) and 7.9e-16 (field); kernel
bodies against the host twin at most 3.6e-15 of values up to 5.8 (bounds 3.8e-14 .. 7.2e-13); their field against the
difference reference at most 0.7 % of its bound; lanes as 8 host threads: the bits of one lane."""
import os
import re

import numpy as np
import pytest
import torch

from auto_oo_amd import _lib, gaussian, gto, properties
from tests import _charges as C
from tests import _gto_d as D
from tests import _potential as P

BOHR = gaussian.BOHR
# the anchor: 10 x the error of the host Boys function of the orders it uses (0 for the potential, 0 and 1 for the field)
ANCHOR_RTOL = 10 * max(D.HOST_BOYS_ERROR[:2])


# ---- 1. host twin against the closed form ---------------------------------------------------------------------------------
def anchor_points():
    rng = np.random.default_rng(1)
    u = rng.normal(size=(40, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    r = np.concatenate(([0.0, 1e-6, 1e-3], np.geomspace(1e-2, 200.0, 37)))
    return u * r[:, None]


@pytest.mark.parametrize("a", [0.15, 1.3, 5277.0])
def test_host_twin_against_the_closed_form_of_one_s_primitive(a):
    """One normalised s primitive of exponent a with D = 1: phi_el(r) = -erf(sqrt(2a) r) / r, -2 sqrt(2a / pi) at r = 0;
    distances 0 .. 200 Bohr and a centre off the origin.  Bound: ANCHOR_RTOL of the value."""
    A = np.array([0.3, -0.2, 0.5])
    table = [(0, 0, np.array([a]), np.array([1.0]))]
    pts = (A + anchor_points()) - A                  # (the distances the twin sees, to the bit)
    phi = gaussian.potential_from_table(table, [1.0], A[None], A + pts, np.ones((1, 1)), "spherical", nuc=False)
    want = P.s_primitive_potential(a, np.linalg.norm(pts, axis=1))
    rel = np.abs(phi / want - 1.0).max()
    print(f"a = {a}: host twin against -erf(sqrt(2a) r) / r: {rel:.2e} relative (bound {ANCHOR_RTOL:.2e}), phi(0) = "
          f"{phi[0]:.15g}")
    assert phi.shape == (40,) and rel < ANCHOR_RTOL
    assert phi[0] == pytest.approx(-2.0 * np.sqrt(2.0 * a / np.pi), rel=ANCHOR_RTOL)
    # the nuclear term, one flag per set, and the point on the nucleus
    both = gaussian.potential_from_table(table, [3.0], A[None], A + pts, np.ones((2, 1, 1)), "spherical", nuc=[True, False])
    assert both.shape == (2, 40) and np.array_equal(both[1], phi) and np.isinf(both[0, 0])
    pn = 3.0 / np.linalg.norm(pts[1:], axis=1)
    assert np.abs((both[0, 1:] - phi[1:]) / pn - 1.0).max() < 1e-14


@pytest.mark.parametrize("a", [0.15, 1.3, 5277.0])
def test_kernel_bodies_against_the_closed_form_of_one_s_primitive(a):
    """The analytic field of the kernel bodies against the analytic derivative of the closed form (the host twin has no
    field of its own), and the difference reference of tests/_potential.py against the same: the reference alone stays
    inside its bound."""
    A = np.array([0.3, -0.2, 0.5])
    basis = gto.GTOBasis(["H"], {"H": [("s", [a], [1.0])]})
    pts = (A + anchor_points()) - A
    phi, F = P.run_host_bodies(basis, A[None, None], (A + pts)[None], np.ones((1, 1, 1, 1)))
    want = P.s_primitive_potential(a, np.linalg.norm(pts, axis=1))
    wantF = P.s_primitive_field(a, pts)
    rel = np.abs(phi[0, 0] / want - 1.0).max()
    scale = np.linalg.norm(wantF, axis=1)
    scale[0] = 1.0
    relF = (np.abs(F[0, 0] - wantF).max(axis=1) / scale).max()
    print(f"a = {a}: kernel bodies against the closed form: potential {rel:.2e}, field {relF:.2e} relative (bound "
          f"{ANCHOR_RTOL:.2e})")
    assert rel < ANCHOR_RTOL and relF < ANCHOR_RTOL and np.abs(F[0, 0, 0]).max() < 1e-15
    fd, bound = P.difference_field(lambda p: P.s_primitive_potential(a, np.linalg.norm(p - A, axis=1)), (A + pts)[3:])
    ratio = (np.abs(fd - wantF[3:]) / bound).max()
    print(f"a = {a}: difference reference against the analytic field: worst error / bound {ratio:.3f}")
    assert ratio < 1.0


# ---- 2. bounds ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.MOL_CASES + P.L_CASES)
def test_bounds_are_the_measured_ones(name):
    got = P.measured_potential_bound(name)
    print(f"{name}: 10 x (perturbed - plain host twin) = {got:.3e}, recorded {P.POTENTIAL_BOUND[name]:.3e}")
    assert got == pytest.approx(P.POTENTIAL_BOUND[name], rel=5e-3)


# ---- 3. the kernel bodies as host functions ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.MOL_CASES + P.L_CASES)
def test_kernel_bodies_on_the_cpu_against_the_host_twin(name):
    """One lane per workgroup, a chunk = one point: every element written; the potential within the bound of the case; the
    electronic field within the bound of the difference reference at the points kept; the potential has the same bits with
    and without the field."""
    basis, xyz, pts, dm = P.basis_of(name), P.xyz_of(name), P.points_of(name), P.density_of(name)
    phi, F = P.run_host_bodies(basis, xyz[None], pts[None], dm[None])
    assert not np.isnan(phi).any() and not np.isnan(F).any()
    err = np.abs(phi[0] - P.host_phi(name)).max()
    Fr, Fb, kept = P.host_field(name)
    ratio = (np.abs(F[0][:, kept] - Fr) / Fb).max()
    print(f"{name}: kernel bodies on the CPU against the host twin {err:.2e} (bound {P.POTENTIAL_BOUND[name]:.2e}); field "
          f"against the difference reference: worst error / bound {ratio:.3f}, {int((~kept).sum())} of {kept.size} points "
          f"left out")
    assert err < P.POTENTIAL_BOUND[name] and ratio < 1.0 and int((~kept).sum()) <= P.FD_EXCLUDE_CAP
    off, none = P.run_host_bodies(basis, xyz[None], pts[None], dm[None], field=False)
    assert none is None and np.array_equal(off, phi)


def test_kernel_bodies_with_the_lanes_as_host_threads():
    """8 lanes per workgroup as host threads with a real barrier, chunks of 8 points, 19 points (two chunks and a rest),
    a stack of two geometries, nuclei on for set 0 and 2: the bits of the one-lane run, and a geometry alone has the
    bits it has in the stack."""
    name = "m1-cartesian"
    basis = P.basis_of(name)
    X = np.stack([P.xyz_of(name), D.M1_MOVED / BOHR])
    pts = np.stack([P.points_of(name)[:19], C.bohr(C.cloud(D.M1_MOVED, 19, seed=3)[1])])
    dm = np.stack([P.densities(name), P.densities(name, P.K, 12)])
    one = P.run_host_bodies(basis, X, pts, dm, nuc_mask=5)
    thr = P.run_host_bodies(basis, X, pts, dm, nuc_mask=5, exe=P.host_program(8))
    for a, b in zip(one, thr):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.isinf(one[0][0, 0, 1]) and np.isinf(one[0][0, 2, 1]) and np.isfinite(one[0][0, 1]).all()
    alone = P.run_host_bodies(basis, X[1:], pts[1:], dm[1:], nuc_mask=5, exe=P.host_program(8))
    assert np.array_equal(alone[0][0], one[0][1]) and np.array_equal(alone[1][0], one[1][1], equal_nan=True)


# ---- 4. interface --------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_exports():
    with open(os.path.join(P.ROOT, "include", "oovqe.h")) as fh:
        hdr = fh.read()
    assert int(re.search(r"#define OOVQE_GTO_GRAD_MAX_SETS (\S+)", hdr).group(1), 0) == gto.MAX_GRAD_SETS
    lib = _lib.load()
    assert re.search(r"\bint64_t oovqe_gto_potential_work_size\(", hdr)
    assert re.search(r"\bint oovqe_gto_potential_batch\(", hdr)
    for name, nargs in (("oovqe_gto_potential_work_size", 5), ("oovqe_gto_potential_batch", 19)):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert len(_lib.SIGNATURES[name][1]) == nargs
    import auto_oo_amd as aoo
    assert aoo.potential_batch is gto.potential_batch and aoo.potential_into is gto.potential_into
    assert "potential_batch" in aoo.__all__ and "potential_into" in aoo.__all__
    assert gto.MAX_POINTS == gto.MAX_POINT_CHARGES == 65535
    for name in ("electrostatic_potential", "rhf_electrostatic_potential", "casci_electrostatic_potential"):
        assert callable(getattr(aoo.OO_pqc_batch, name))
    assert callable(properties.fit_esp_charges) and callable(gaussian.potential_from_table)


def test_work_size_answers_without_a_device():
    lib = _lib.load()
    basis = P.basis_of("m2-spherical")
    base = lib.oovqe_gto_work_size(basis.nshell, basis.max_nprim, 7)
    assert lib.oovqe_gto_potential_work_size(basis.nshell, basis.max_nprim, basis.natm, 7, 3) == base > 0
    # it does not grow with the sets (nor, having no such argument, with the points)
    assert lib.oovqe_gto_potential_work_size(basis.nshell, basis.max_nprim, basis.natm, 7, 10) == base
    for args, text in (((0, 3, 3, 1, 1), "nshell = 0"), ((4, 11, 3, 1, 1), "11 primitives"), ((4, 3, 0, 1, 1), "natm = 0"),
                       ((4, 3, 3, -1, 1), "batch = -1"), ((4, 3, 3, 65536, 1), "batch = 65536"),
                       ((4, 3, 3, 1, 0), "nset = 0"), ((4, 3, 3, 1, 11), "nset = 11")):
        assert lib.oovqe_gto_potential_work_size(*args) < 0
        assert text.encode() in lib.oovqe_last_error(), (args, lib.oovqe_last_error())


def test_the_entry_refuses_before_anything_is_launched():
    """No device is needed to be refused."""
    lib = _lib.load()
    for (nset, npoint, mask), text in (((0, 4, 0), "nset = 0"), ((11, 4, 0), "nset = 11"), ((2, 0, 0), "npoint = 0"),
                                       ((2, 65536, 0), "npoint = 65536"), ((2, 4, 4), "nuc_mask"),
                                       ((2, 4, 3), "null pointer")):
        rc = lib.oovqe_gto_potential_batch(1, None, 1, None, None, 1, None, 1, None, 1, nset, None, npoint, None, mask,
                                           None, None, None, None)
        assert rc < 0 and text.encode() in lib.oovqe_last_error(), (text, lib.oovqe_last_error())


def test_python_refusals():
    basis, xyz = C.case("water")
    N = basis.nao
    dm = torch.zeros((1, N, N), dtype=torch.float64)
    pts = np.zeros((4, 3))
    for bad in (np.zeros(3), np.zeros((4, 2)), np.zeros((2, 4, 3)), np.zeros((1, 4, 3, 1))):
        with pytest.raises(ValueError, match="points of shape"):
            gto.potential_batch(basis, xyz[None], bad, dm)
    for M in (0, 65536):
        with pytest.raises(ValueError, match=f"{M} points per geometry"):
            gto.potential_batch(basis, xyz[None], np.zeros((M, 3)), dm)
    with pytest.raises(ValueError, match="finite"):
        gto.potential_batch(basis, xyz[None], np.full((4, 3), np.inf), dm)
    with pytest.raises(ValueError, match="finite"):
        gto.potential_batch(basis, xyz[None], pts, dm * float("nan"))
    for bad in (np.zeros((1, N, N)), torch.zeros((N, N)), torch.zeros((1, N, N + 1)), torch.zeros((2, N, N)),
                torch.zeros((1, 2, N, N + 1))):
        with pytest.raises(ValueError, match="dm has shape"):
            gto.potential_batch(basis, xyz[None], pts, bad)
    for K in (0, 11):
        with pytest.raises(ValueError, match=f"{K} density sets"):
            gto.potential_batch(basis, xyz[None], pts, torch.zeros((1, K, N, N), dtype=torch.float64))
    with pytest.raises(ValueError, match="3 flags for 2 sets"):
        gto.potential_batch(basis, xyz[None], pts, torch.zeros((1, 2, N, N), dtype=torch.float64), nuc=[True, False, True])
    # potential_into: the same for tensors in Bohr (host tensors are enough to be refused)
    X = torch.as_tensor(xyz[None] / BOHR)
    r = torch.zeros((1, 4, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match="coordinates of shape"):
        gto.potential_into(basis, X[0], r, dm[:, None])
    with pytest.raises(ValueError, match="points of shape"):
        gto.potential_into(basis, X, r[0], dm[:, None])
    with pytest.raises(ValueError, match="dm has shape"):
        gto.potential_into(basis, X, r, dm)
    with pytest.raises(ValueError, match="points per geometry"):
        gto.potential_into(basis, X, torch.zeros((1, 0, 3), dtype=torch.float64), dm[:, None])
    # no geometries: empty tensors, nothing launched (no library call: this passes without a device)
    phi, F = gto.potential_into(basis, X[:0], r[:0], dm[:0, None], field=True)
    assert tuple(phi.shape) == (0, 1, 4) and tuple(F.shape) == (0, 1, 4, 3)
    with pytest.raises(ValueError, match="nuclear charges"):
        gaussian.potential_from_table(basis.table, [1.0], xyz / BOHR, pts, np.zeros((N, N)), "spherical")
    with pytest.raises(ValueError, match="dm of shape"):
        gaussian.potential_from_table(basis.table, basis.charges, xyz / BOHR, pts + 1.0, np.zeros((N, N + 1)), "spherical")


# ---- 5. charges fitted to a potential ----------------------------------------------------------------------------------------
def esp_case():
    R = C.bohr(C.WATER)
    pts = C.bohr(C.cloud(C.WATER, on_nucleus=False)[1])
    A = 1.0 / np.linalg.norm(pts[:, None, :] - R[None, :, :], axis=2)
    return R, pts, A


def test_fit_esp_charges_recovers_the_charges_that_made_the_potential():
    R, pts, A = esp_case()
    q = np.array([-0.82, 0.47, 0.41])
    got = properties.fit_esp_charges(A @ q, pts, R, q.sum())
    err = np.abs(got.numpy() - q).max()
    print(f"fit_esp_charges: recovered to {err:.2e}, constraint {abs(got.sum().item() - q.sum()):.2e}")
    assert tuple(got.shape) == (3,) and err < 1e-10
    assert abs(got.sum().item() - q.sum()) < 1e-12
    # batched over leading axes, one total charge per entry, tensors or arrays
    qs = np.array([[q, [0.3, -0.1, -0.2]], [[1.0, 0.0, 0.0], [-0.5, 0.25, 0.25]]])
    phi = torch.as_tensor(qs @ A.T)
    got = properties.fit_esp_charges(phi, torch.as_tensor(pts), torch.as_tensor(R), qs.sum(axis=-1))
    assert tuple(got.shape) == (2, 2, 3) and np.abs(got.numpy() - qs).max() < 1e-10
    assert np.abs(got.sum(-1).numpy() - qs.sum(-1)).max() < 1e-12


def test_fit_esp_charges_follows_the_normal_equations():
    """A potential no three charges reproduce; the fit is the solution of [[A^T A, 1], [1^T, 0]] (q, lambda) = (A^T phi,
    Q), and another Q shifts it by (Q' - Q) (A^T A)^-1 1 / (1^T (A^T A)^-1 1)."""
    R, pts, A = esp_case()
    phi = A @ np.array([-0.7, 0.3, 0.4]) + 0.01 * np.random.default_rng(2).standard_normal(len(pts))
    n = 3
    kkt = np.zeros((n + 1, n + 1))
    kkt[:n, :n], kkt[:n, n], kkt[n, :n] = A.T @ A, 1.0, 1.0
    worst = 0.0
    fits = {}
    for Q in (0.0, 1.0, -0.35):
        want = np.linalg.solve(kkt, np.concatenate((A.T @ phi, [Q])))[:n]
        fits[Q] = properties.fit_esp_charges(phi, pts, R, Q).numpy()
        worst = max(worst, np.abs(fits[Q] - want).max())
        assert abs(fits[Q].sum() - Q) < 1e-12
    w = np.linalg.solve(A.T @ A, np.ones(n))
    shift = np.abs((fits[1.0] - fits[0.0]) - w / w.sum()).max()
    # cond(A^T A) = 1.2e3 here: the normal equations themselves are good to 1e-16 x 1.2e3 x |q| ~ 1e-13
    print(f"fit against the normal equations {worst:.2e}, shift with the constraint {shift:.2e}, cond(A^T A) = "
          f"{np.linalg.cond(A.T @ A):.3g}")
    assert worst < 1e-10 and shift < 1e-10


def test_fit_esp_charges_refusals():
    R, pts, A = esp_case()
    with pytest.raises(ValueError, match="values of phi"):
        properties.fit_esp_charges(np.zeros(5), pts, R, 0.0)
    with pytest.raises(ValueError, match="values of phi"):
        properties.fit_esp_charges(np.zeros(2), pts[:2], R, 0.0)
    with pytest.raises(ValueError, match="on an atom"):
        properties.fit_esp_charges(np.zeros(len(pts)), np.concatenate((R[:1], pts[1:])), R, 0.0)
    with pytest.raises(ValueError, match="expected"):
        properties.fit_esp_charges(np.zeros(len(pts)), pts[:, :2], R, 0.0)
    one = properties.fit_esp_charges(np.ones(4), pts[:4], R[:1], 0.7)
    assert one.tolist() == [0.7]
