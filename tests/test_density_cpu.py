"""Electron density, its gradient and orbital values on the host side: the host twins ``gaussian.density_from_table`` and
``gaussian.orbital_values_from_table`` against things that share no code with them (a closed form, the Poisson equation
with the validated ``gaussian.potential_from_table``, differences, quadrature against the host overlap), the bound of
tests/_density.py shown valid (40-digit arithmetic) and not lax (planted defects), the kernel bodies of
csrc/gto_density.hip run on the CPU, the interface (header, bindings, refusals) and the grid helpers of
``properties``.  No GPU.

Measured here (``python -m pytest tests/test_density_cpu.py -s``; every test prints its figures before it asserts): twin
against the closed form 4e-16 relative; twin against 40-digit arithmetic at most 0.05 bounds; every planted defect at least
4e10 bounds; Poisson check at h = 1e-3 Bohr: error at most 0.8 % of its bound (stencil disagreement up to 3.3e-3 for the
s shells of exponent 5.3e3 of Lss, 1e-8 .. 7e-6 elsewhere); gradient against differences at most 0.7 % of its bound; quadrature
of the overlap on the 49^3 grid 4.3e-11 (spherical) and 5.9e-11 (Cartesian); kernel bodies against the twin at most 0.06
bounds; lanes as 8 host threads: the bits of one lane."""
import os
import re

import numpy as np
import pytest

from auto_oo_amd import _lib, gaussian, gto, properties
from tests import _charges as C
from tests import _gto_d as D
from tests import _density as Dn
from tests import _potential as P

BOHR = gaussian.BOHR
ROOT = P.ROOT
ALL_CASES = P.MOL_CASES + P.L_CASES
NEW_SYMBOLS = ("oovqe_gto_density_batch", "oovqe_gto_orbital_values_batch")
# the closed form against the twin: the few roundings of (2a/pi)^(3/2) e^(-2 a r^2) and the argument error 6 x u of the
# twin's two exponentials (tests/_density.py), x <= X_MAX
ANCHOR_C = 16 + 2 * Dn.ARG_ERR * Dn.X_MAX


# ---- 1. interface ------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "oovqe.h")) as fh:
        hdr = fh.read()
    declared = set(re.findall(r"\b(oovqe_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    # no work buffer: no *_work_size of these entries exists
    assert "oovqe_gto_density_work_size" not in declared and "oovqe_gto_orbital_values_work_size" not in declared
    # the LDS columns of the density kernel as gto.py counts them: (65536 - sizeof(gto_den_lds_t)) / 512
    with open(os.path.join(ROOT, "auto_oo_amd", "csrc", "gto_density.hip")) as fh:
        src = fh.read()
    lds_max = int(re.search(r"#define DEN_LDS_MAX (\d+)", src).group(1))
    static = 8 * gto.MAX_GRAD_SETS * 36 + 4 * int(re.search(r"#define OOVQE_GTO_MAX_SHELL (\d+)", hdr).group(1))
    assert gto.DENSITY_LDS_COLUMNS == (lds_max - static) // 512
    few, many = P.basis_of("m1-spherical"), gto.GTOBasis(["H"], {"H": [("s", [1.0 + k], [1.0]) for k in range(59)]})
    assert gto.density_max_sets(few) == gto.density_max_sets(few, True) == gto.MAX_GRAD_SETS
    assert gto.density_max_sets(many) == gto.MAX_GRAD_SETS and gto.density_max_sets(many, True) == 0
    import auto_oo_amd as aoo
    for name in ("density_batch", "density_into", "orbital_values_batch"):
        assert getattr(aoo, name) is getattr(gto, name) and name in aoo.__all__
    for name in ("electron_density", "rhf_electron_density", "casci_electron_density", "orbital_values", "_density_of"):
        assert callable(getattr(aoo.OO_pqc_batch, name))


def test_refusals_of_the_entries_need_no_device():
    """sizes out of scope return a negative code with a message before anything touches a device"""
    lib = _lib.load()
    for entry in (lib.oovqe_gto_density_batch, lib.oovqe_gto_orbital_values_batch):
        def call(nshell=2, batch=1, nset=1, npoint=5):
            return entry(nshell, None, 2, None, None, 2, batch, None, 2, nset, None, npoint, None, None, None, None)
        for kwargs, word in (({"batch": 65536}, b"65535 geometries"), ({"npoint": 0}, b"npoint"),
                             ({"npoint": 65536}, b"npoint"), ({"nset": 0}, b"per geometry"),
                             ({"nset": gto.MAX_GRAD_SETS + 1}, b"per geometry"), ({"nshell": 0}, b"nshell"),
                             ({}, b"null pointer")):
            assert call(**kwargs) < 0
            assert word in lib.oovqe_last_error(), (kwargs, lib.oovqe_last_error())


# ---- 2. host twin against the closed form ------------------------------------------------------------------------------------
def anchor_points():
    rng = np.random.default_rng(1)
    u = rng.normal(size=(40, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    r = np.concatenate(([0.0, 1e-6, 1e-3], np.geomspace(1e-2, 200.0, 37)))
    return u * r[:, None]


@pytest.mark.parametrize("a", [0.15, 1.3, 5277.0])
def test_host_twin_against_the_closed_form_of_one_s_primitive(a):
    """One normalised s primitive with D = 1: rho = (2a/pi)^(3/2) e^(-2 a r^2), d rho / d r = -4 a (r - A) rho; distances
    0 .. 200 Bohr (exact zeros beyond the underflow) and a centre off the origin."""
    A = np.array([0.3, -0.2, 0.5])
    table = [(0, 0, np.array([a]), np.array([1.0]))]
    d = (A + anchor_points()) - A                    # (the distances the twin sees, to the bit)
    rho, drho, _, _ = gaussian.density_from_table(table, A[None], A + d, np.ones((1, 1)), "spherical", True)
    r2 = np.sum(d * d, axis=1)
    want = (2.0 * a / np.pi) ** 1.5 * np.exp(-2.0 * a * r2)
    wantg = -4.0 * a * d * want[:, None]
    tol = Dn.U * ANCHOR_C
    # (relative to the value; 1e-290 keeps the subnormal values before the underflow out of the ratio)
    err = np.abs(rho - want) / (want + 1e-290)
    errg = np.abs(drho - wantg).max(axis=1) / (4.0 * a * np.sqrt(r2) * want + 1e-290)
    print(f"a = {a}: twin against the closed form: rho {err.max():.2e}, gradient {errg.max():.2e} relative (bound "
          f"{tol:.2e}); rho(0) = {rho[0]:.15g}, zeros beyond {np.sqrt(r2[want == 0].min()) if (want == 0).any() else None}")
    assert rho.shape == (40,) and drho.shape == (40, 3)
    assert err.max() < tol and errg.max() < tol
    assert np.all(drho[0] == 0.0) and np.all(rho[want == 0] == 0.0) and np.all(drho[want == 0] == 0.0)
    psi, dpsi, _, _ = gaussian.orbital_values_from_table(table, A[None], A + d, np.ones((1, 1)), "spherical", True)
    assert np.abs(psi[0] ** 2 - rho).max() <= 4 * Dn.U * rho.max()


# ---- 3. the bound: valid and not lax ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_twin_against_the_same_formula_in_40_digits(name):
    hd, ho = Dn.host_density(name), Dn.host_orbitals(name)
    err = Dn.multiprecision_errors(name)
    r = [float((e / Dn.bound_of(name, a)).max()) for e, a in zip(err, (hd[2], hd[3], ho[2], ho[3]))]
    print(f"{name}: c = {Dn.bound_constant(P.basis_of(name)):.0f}; fp64 twin against 40-digit arithmetic, worst error / bound: "
          f"rho {r[0]:.3f}, drho {r[1]:.3f}, psi {r[2]:.3f}, dpsi {r[3]:.3f}")
    assert max(r) < 1.0
    # the point ON atom 1 and the point 50 Bohr away
    assert np.isfinite(hd[0][:, 1]).all() and np.isfinite(hd[1][:, 1]).all()
    if name in P.MOL_CASES:
        assert np.all(hd[0][:, 2] == 0.0) and np.all(hd[1][:, 2] == 0.0) and np.all(hd[2][:, 2] == 0.0)


@pytest.mark.parametrize("defect", Dn.DEFECTS)
def test_planted_defects_move_a_value_by_more_than_1000_bounds(defect):
    seen = 0
    for name in ALL_CASES:
        if not Dn.defect_applies(name, defect):
            continue
        r = Dn.defect_ratio(name, defect)
        print(f"{defect} on {name}: {r:.3g} bounds")
        assert r > Dn.LAX
        seen += 1
    assert seen >= 4


# ---- 4. the twin against references that share no code with it ----------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_poisson_equation_with_the_host_potential(name):
    """The 4th-order central-difference Laplacian of ``gaussian.potential_from_table`` (electronic part) is 4 pi rho; bound
    per point: max(what the potential's own error makes of the stencil, 10 x the disagreement of h and 2h)."""
    h = 1e-3 * Dn.FD_K
    rho = Dn.host_density(name)[0]
    dm = P.density_of(name)
    L, dis = Dn.difference_laplacian(lambda p: P.host_potential(name, p, dm), P.points_of(name), h)
    floor = Dn.poisson_floor(name, h)
    err = np.abs(L - 4.0 * np.pi * rho)
    ratio = err / np.maximum(floor, 10.0 * dis)
    print(f"{name}: |4 pi rho| up to {np.abs(4 * np.pi * rho).max():.3g}; stencil at h against 2h up to {dis.max():.2e}, "
          f"floor {floor:.2e}; |Laplacian - 4 pi rho| up to {err.max():.2e}, worst error / bound {ratio.max():.4f}")
    assert ratio.max() < 1.0


@pytest.mark.parametrize("name", ALL_CASES)
def test_gradient_against_differences_of_the_twin(name):
    rho, drho, _, _ = Dn.host_density(name)
    F, bound = P.difference_field(lambda p: Dn.twin_density(name, p)[0], P.points_of(name))
    ratio = np.abs(drho + F) / bound
    psi, dpsi, _, _ = Dn.host_orbitals(name)
    Fo, bo = P.difference_field(lambda p: Dn.twin_orbitals(name, p)[0], P.points_of(name))
    ro = np.abs(dpsi + Fo) / bo
    print(f"{name}: analytic gradient against the 4th-order difference of the twin: drho worst error / bound "
          f"{ratio.max():.4f} (bounds {bound.min():.1e} .. {bound.max():.1e}), dpsi {ro.max():.4f}")
    assert ratio.max() < 1.0 and ro.max() < 1.0


@pytest.mark.parametrize("name", ["m1-spherical", "m1-cartesian"])
def test_quadrature_reproduces_the_overlap(name):
    """sum chi_mu chi_nu h^3 on the 49^3 grid of spacing 0.3 Bohr around the centroid against the host overlap"""
    e = Dn.quadrature_errors(name)
    print(f"{name}: |sum chi chi h^3 - S| {e[0].max():.2e} (recorded {Dn.QUAD_MEASURED[name]:.1e}), |sum d(chi chi) h^3| "
          f"{e[1].max():.2e}, |sum r chi chi h^3 - <r>| {e[2].max():.2e}")
    assert e[0].max() < 10.0 * Dn.QUAD_MEASURED[name]


# ---- 5. the kernel bodies as host functions ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_kernel_bodies_on_the_cpu_against_the_host_twin(name):
    """One lane per workgroup, a chunk = one point: every element written, every value within its bound, the same bits
    with and without the gradient."""
    basis, xyz, pts = P.basis_of(name), P.xyz_of(name), P.points_of(name)
    rho, drho = Dn.run_host_bodies(basis, xyz[None], pts[None], P.density_of(name)[None])
    psi, dpsi = Dn.run_host_bodies(basis, xyz[None], pts[None], Dn.coefficients(name)[None], orbitals=True)
    for x in (rho, drho, psi, dpsi):
        assert not np.isnan(x).any()
    rd, ro = Dn.ratios(name, (rho[0], drho[0])), Dn.ratios(name, (psi[0], dpsi[0]), kind="orbitals")
    print(f"{name}: kernel bodies on the CPU against the host twin, worst error / bound: rho {rd[0]:.3f}, drho {rd[1]:.3f}, "
          f"psi {ro[0]:.3f}, dpsi {ro[1]:.3f}")
    assert max(rd + ro) < 1.0
    off, none = Dn.run_host_bodies(basis, xyz[None], pts[None], P.density_of(name)[None], gradient=False)
    assert none is None and np.array_equal(off, rho)
    off, none = Dn.run_host_bodies(basis, xyz[None], pts[None], Dn.coefficients(name)[None], orbitals=True, gradient=False)
    assert none is None and np.array_equal(off, psi)
    if name in P.MOL_CASES:          # ON atom 1: finite; 50 Bohr away: exact zeros (psi of 1e-177 is still a number there,
        assert np.isfinite(rho[0, :, 1]).all() and np.isfinite(drho[0, :, 1]).all()      # its square is not)
        assert np.all(rho[0, :, 2] == 0.0) and np.all(drho[0, :, 2] == 0.0)


def test_kernel_bodies_far_away_and_on_a_centre_in_one_component():
    """points at 1e3, 1e80 and 1e300 Bohr: exact zeros, no NaN; a point that shares one and two coordinates with the d
    centre: finite and within bound"""
    name = "m1-cartesian"
    basis, xyz = P.basis_of(name), P.xyz_of(name)
    A = xyz[0]
    pts = np.array([[1e3, 0.0, 0.0], [1e80, -1e80, 3.0], [1e300, 1e300, -1e300], [A[0], A[1] + 0.4, A[2] - 0.3],
                    [A[0], A[1], A[2] + 0.5], A])
    dm = P.densities(name)
    rho, drho = Dn.run_host_bodies(basis, xyz[None], pts[None], dm[None])
    psi, dpsi = Dn.run_host_bodies(basis, xyz[None], pts[None], Dn.coefficients(name)[None], orbitals=True)
    for x in (rho, drho, psi, dpsi):
        assert np.isfinite(x).all() and np.all(x[0, :, :3] == 0.0)
    want = Dn.twin_density(name, pts)
    wanto = Dn.twin_orbitals(name, pts)
    r = Dn.ratios(name, (rho[0], drho[0]), want) + Dn.ratios(name, (psi[0], dpsi[0]), wanto)
    print(f"far points and points on a centre: worst error / bound {max(r):.3f}; rho at the centre {rho[0, :, 5]}")
    assert max(r) < 1.0 and np.all(want[0][:, :3] == 0.0)


def test_kernel_bodies_with_the_lanes_as_host_threads():
    """8 lanes per workgroup as host threads with a real barrier, chunks of 8 points, 19 points (two chunks and a rest),
    a stack of two geometries: the bits of the one-lane run, and a geometry alone has the bits it has in the stack."""
    name = "m1-cartesian"
    basis = P.basis_of(name)
    X = np.stack([P.xyz_of(name), D.M1_MOVED / BOHR])
    pts = np.stack([P.points_of(name)[:19], C.bohr(C.cloud(D.M1_MOVED, 19, seed=3)[1])])
    dm = np.stack([P.densities(name), P.densities(name, P.K, 12)])
    cm = np.stack([Dn.coefficients(name), Dn.coefficients(name)[::-1]])
    for x, orbitals in ((dm, False), (cm, True)):
        one = Dn.run_host_bodies(basis, X, pts, x, orbitals)
        thr = Dn.run_host_bodies(basis, X, pts, x, orbitals, exe=Dn.host_program(8))
        for a, b in zip(one, thr):
            assert not np.isnan(a).any() and np.array_equal(a, b)
        alone = Dn.run_host_bodies(basis, X[1:], pts[1:], x[1:], orbitals)
        assert np.array_equal(alone[0][0], one[0][1]) and np.array_equal(alone[1][0], one[1][1])


# ---- 6. grids and cube files ----------------------------------------------------------------------------------------------------
def test_cube_grid_integrate_grid_and_write_cube(tmp_path):
    xyz = D.M1_XYZ
    origin, shape, pts = properties.cube_grid(xyz, 0.4, 4.0)
    assert pts.shape == (shape[0] * shape[1] * shape[2], 3) and np.allclose(pts[0], origin)
    assert np.all(pts.min(axis=0) <= xyz.min(axis=0) - 4.0 + 1e-12) and np.all(pts.max(axis=0) >= xyz.max(axis=0) + 4.0 - 1e-12)
    assert np.allclose(pts[1] - pts[0], [0.0, 0.0, 0.4]) and np.allclose(pts[shape[2]] - pts[0], [0.0, 0.4, 0.0])
    # a normalised s Gaussian integrates to 1 (spacing in Angstrom, values in atomic units).  The rule is the trapezoidal
    # one: its error for e^(-2 a r^2) is 6 e^(-pi^2 / (2 a h^2)) = 3e-9 at a = 0.4, h = 0.4 / BOHR, and the box cuts off
    # less than e^(-2 a (4 / BOHR)^2) = 1e-20
    a = 0.4
    centre = xyz.mean(axis=0)
    val = (2 * a / np.pi) ** 1.5 * np.exp(-2 * a * np.sum(((pts - centre) / BOHR) ** 2, axis=1))
    total = properties.integrate_grid(val, 0.4)
    print(f"grid {shape}: a normalised Gaussian integrates to {total:.12f}")
    assert abs(total - 1.0) < 1e-8
    path = tmp_path / "rho.cube"
    properties.write_cube(path, P.basis_of("m1-spherical").symbols, xyz, origin, shape, 0.4, val)
    lines = path.read_text().splitlines()
    natm = len(xyz)
    assert int(lines[2].split()[0]) == natm and [int(lines[3 + d].split()[0]) for d in range(3)] == list(shape)
    assert np.allclose([float(x) for x in lines[2].split()[1:]], origin / BOHR, atol=1e-6)
    body = np.array([float(x) for line in lines[6 + natm:] for x in line.split()])
    assert body.size == val.size and np.allclose(body, val, rtol=2e-5, atol=1e-12)
    with pytest.raises(ValueError):
        properties.write_cube(path, ["H"] * natm, xyz, origin, shape, 0.4, val[:-1])
    with pytest.raises(ValueError):
        properties.cube_grid(xyz, 0.0, 1.0)
