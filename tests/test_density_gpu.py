"""Electron density, its gradient and orbital values on the device (csrc/gto_density.hip, gto.density_*,
gto.orbital_values_*, the ``*electron_density`` and ``orbital_values`` methods of OO_pqc_batch) against the host twins
``gaussian.density_from_table`` / ``gaussian.orbital_values_from_table``, bit for bit against itself, and by quadrature
against the electron count and the dipole moment of the same density.

Bounds: tests/_density.py (none taken from what the device code gives).  Every comparison prints its figures before it
asserts.  Measured on an MI355X: device against the twins at most 0.021 (rho), 0.020 (drho), 0.057 (psi, dpsi) bounds;
rho of 2 C C^T against 2 sum psi^2 0.0002 of the sum of both bounds; quadrature of the RHF density of M1: 13.999999999972
electrons (bound 3.8e-10), integral of the gradient at most 2.4e-10 (bounds from 6.8e-10), dipole against
``rhf_dipole_moment`` at most 1.9e-10 (bounds from 3.4e-10); the whole file runs in 4 s.
"""
from unittest import mock

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import auto_oo_amd as aoo                                   # noqa: E402
from auto_oo_amd import gaussian, gto, nucgrad, properties     # noqa: E402
from auto_oo_amd.gto import density_batch, density_into, orbital_values_batch, orbital_values_into   # noqa: E402
from tests import _charges as C                             # noqa: E402
from tests import _gto_d as D                               # noqa: E402
from tests import _density as Dn                            # noqa: E402
from tests import _potential as P                           # noqa: E402
from tests.test_moments_gpu import cas_batch, seeded_thetas, formal_coords, POINTS, _circuit   # noqa: E402

F64 = torch.float64
BOHR = gaussian.BOHR


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def to_dev(x):
    return torch.as_tensor(np.array(x, dtype=np.float64, order="C")).to(dev())


def device_density(name, dm=None, points_angstrom=None, gradient=True):
    """``gto.density_batch`` of one geometry of a case -> numpy (rho [K, M], drho [K, M, 3])"""
    pts = P.points_angstrom(name) if points_angstrom is None else points_angstrom
    dm = P.density_of(name) if dm is None else dm
    out = density_batch(P.basis_of(name), P.angstrom_of(name)[None], pts, to_dev(dm)[None], gradient=gradient)
    return (out[0][0].cpu().numpy(), out[1][0].cpu().numpy()) if gradient else (out[0].cpu().numpy(), None)


def device_orbitals(name, points_angstrom=None, gradient=True):
    pts = P.points_angstrom(name) if points_angstrom is None else points_angstrom
    out = orbital_values_batch(P.basis_of(name), P.angstrom_of(name)[None], pts, to_dev(Dn.coefficients(name))[None],
                               gradient=gradient)
    return (out[0][0].cpu().numpy(), out[1][0].cpu().numpy()) if gradient else (out[0].cpu().numpy(), None)


# ---- 1. every case against the host twins --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.L_CASES + P.MOL_CASES)
def test_density_and_orbitals_against_the_host_twins(name):
    """L-cases: two centres, one shell each, the density in the block of the two shells and its transpose, M = 65.
    Molecules: K = 3 random non-symmetric densities at the 130-point cloud.  C = a seeded random [N, 3].  No point is left
    out."""
    rho, drho = device_density(name)
    psi, dpsi = device_orbitals(name)
    M = P.points_of(name).shape[0]
    assert rho.shape == (P.density_of(name).shape[0], M) and drho.shape == rho.shape + (3,)
    assert psi.shape == (Dn.NCOL, M) and dpsi.shape == psi.shape + (3,)
    rd, ro = Dn.ratios(name, (rho, drho)), Dn.ratios(name, (psi, dpsi), kind="orbitals")
    print(f"{name}: device against the host twin, worst error / bound: rho {rd[0]:.4f}, drho {rd[1]:.4f}, psi {ro[0]:.4f}, "
          f"dpsi {ro[1]:.4f} (|rho| up to {np.abs(rho).max():.3g})")
    for x in (rho, drho, psi, dpsi):
        assert np.isfinite(x).all()
    assert max(rd + ro) < 1.0
    if name in P.MOL_CASES:
        # point 1 is ON atom 1: finite (above) and within bound like every point; point 2 is 50 Bohr away: exact zeros
        assert np.all(rho[:, 2] == 0.0) and np.all(drho[:, 2] == 0.0)
        print(f"{name}: ON atom 1 rho = {rho[:, 1]}, drho = {drho[0, 1]}")


def test_far_points_are_exact_zeros_and_points_on_a_centre_are_finite():
    name = "m1-cartesian"
    A = P.xyz_of(name)[0]
    pts = np.array([[1e3, 0.0, 0.0], [1e80, -1e80, 3.0], [1e300, 1e300, -1e300], [A[0], A[1] + 0.4, A[2] - 0.3],
                    [A[0], A[1], A[2] + 0.5], A])
    rho, drho = device_density(name, points_angstrom=pts * BOHR)
    psi, dpsi = device_orbitals(name, points_angstrom=pts * BOHR)
    seen = (pts * BOHR) / BOHR
    r = Dn.ratios(name, (rho, drho), Dn.twin_density(name, seen)) + Dn.ratios(name, (psi, dpsi), Dn.twin_orbitals(name, seen))
    print(f"far points and points on a centre: worst error / bound {max(r):.4f}; rho at the centre {rho[:, 5]}")
    for x in (rho, drho, psi, dpsi):
        assert np.isfinite(x).all() and np.all(x[:, :3] == 0.0)
    assert max(r) < 1.0


# ---- 2. chunk edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 63, 64, 65, 130])
def test_chunk_edges(M):
    name = "m1-spherical"
    pts = P.points_angstrom(name)[:M]
    rho, drho = device_density(name, points_angstrom=pts)
    psi, dpsi = device_orbitals(name, points_angstrom=pts)
    hd, ho = Dn.host_density(name), Dn.host_orbitals(name)
    want = tuple(x[:, :M] for x in hd)
    wanto = tuple(x[:, :M] for x in ho)
    r = Dn.ratios(name, (rho, drho), want) + Dn.ratios(name, (psi, dpsi), wanto)
    print(f"M = {M}: worst error / bound {max(r):.4f}")
    assert rho.shape == (P.K, M) and max(r) < 1.0


# ---- 3. the same bits -------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_stack_the_points_the_sets_the_stream_or_the_gradient():
    name = "m1-spherical"
    basis = P.basis_of(name)
    X = np.stack([P.angstrom_of(name), D.M1_MOVED, P.angstrom_of(name) + 0.1])
    pts = np.stack([P.points_angstrom(name), C.cloud(D.M1_MOVED, C.M_MAX, seed=3)[1], P.points_angstrom(name) + 0.1])
    dm = to_dev(np.stack([P.densities(name, 5, 20 + g) for g in range(3)]))
    cm = to_dev(np.stack([np.random.default_rng(30 + g).uniform(-1, 1, (basis.nao, 5)) for g in range(3)]))
    rho, drho = density_batch(basis, X, pts, dm, gradient=True)
    psi, dpsi = orbital_values_batch(basis, X, pts, cm, gradient=True)
    # with and without the gradient
    assert torch.equal(density_batch(basis, X, pts, dm), rho) and torch.equal(orbital_values_batch(basis, X, pts, cm), psi)
    # a geometry alone against inside a stack of 3 permuted geometries
    perm = [2, 0, 1]
    prho, pdrho = density_batch(basis, X[perm], pts[perm], dm[perm], gradient=True)
    assert torch.equal(prho, rho[perm]) and torch.equal(pdrho, drho[perm])
    ppsi, pdpsi = orbital_values_batch(basis, X[perm], pts[perm], cm[perm], gradient=True)
    assert torch.equal(ppsi, psi[perm]) and torch.equal(pdpsi, dpsi[perm])
    for g in range(3):
        a, b = density_batch(basis, X[g:g + 1], pts[g:g + 1], dm[g:g + 1], gradient=True)
        assert torch.equal(a[0], rho[g]) and torch.equal(b[0], drho[g])
    # a point alone, first in a chunk, and last in a partial chunk
    for m, sl in ((77, slice(77, 78)), (77, slice(77, 130)), (77, slice(64, 78)), (129, slice(100, 130))):
        a, b = density_batch(basis, X[:1], pts[:1, sl], dm[:1], gradient=True)
        k = m - sl.start
        assert torch.equal(a[0, :, k], rho[0, :, m]) and torch.equal(b[0, :, k], drho[0, :, m])
        a, b = orbital_values_batch(basis, X[:1], pts[:1, sl], cm[:1], gradient=True)
        assert torch.equal(a[0, :, k], psi[0, :, m]) and torch.equal(b[0, :, k], dpsi[0, :, m])
    # a set alone against among K = 5, at each place
    for k in range(5):
        a, b = density_batch(basis, X, pts, dm[:, k], gradient=True)
        assert torch.equal(a, rho[:, k]) and torch.equal(b, drho[:, k])
        a, b = orbital_values_batch(basis, X, pts, cm[:, :, k:k + 1].contiguous(), gradient=True)
        assert torch.equal(a[:, 0], psi[:, k]) and torch.equal(b[:, 0], dpsi[:, k])
    order = [3, 1, 4, 0, 2]
    a = density_batch(basis, X, pts, dm[:, order])
    assert torch.equal(a, rho[:, order])
    # on a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a, b = density_batch(basis, X, pts, dm, gradient=True)
        c, d = orbital_values_batch(basis, X, pts, cm, gradient=True)
    side.synchronize()
    assert torch.equal(a, rho) and torch.equal(b, drho) and torch.equal(c, psi) and torch.equal(d, dpsi)
    # [M, 3] shared points against the same points given per geometry
    shared = density_batch(basis, X, pts[0], dm, gradient=True)
    tiled = density_batch(basis, X, np.tile(pts[0], (3, 1, 1)), dm, gradient=True)
    assert torch.equal(shared[0], tiled[0]) and torch.equal(shared[1], tiled[1]) and torch.equal(shared[0][0], rho[0])
    # the device-tensor entry in atomic units
    a, b = density_into(basis, to_dev(X / BOHR), to_dev(pts / BOHR), dm, True)
    assert torch.equal(a, rho) and torch.equal(b, drho)


# ---- 4. density of doubly occupied orbitals -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["water", "m1-spherical", "m1-cartesian"])
def test_density_of_occupied_orbitals_is_twice_the_sum_of_their_squares(name):
    Cm = Dn.coefficients(name)
    dm = 2.0 * Cm @ Cm.T
    rho, _ = device_density(name, dm[None])
    psi, _ = device_orbitals(name)
    basis = P.basis_of(name)
    A = gaussian.density_from_table(basis.table, P.xyz_of(name), P.points_of(name), dm, P.form_of(name))[1]
    ho = Dn.host_orbitals(name)
    # the bound of rho, and of 2 sum psi^2: 2 |psi| times the bound of psi, twice, and the roundings of the few products
    b = Dn.bound_of(name, A) + np.sum(4.0 * np.abs(ho[0]) * Dn.bound_of(name, ho[2]) + 8 * Dn.U * 2.0 * ho[0] ** 2, axis=0)
    ratio = np.abs(rho[0] - 2.0 * np.sum(psi ** 2, axis=0)) / b
    print(f"{name}: rho of D = 2 C C^T against 2 sum psi^2: worst difference / bound {ratio.max():.4f}")
    assert ratio.max() < 1.0


# ---- 5. quadrature on the device ------------------------------------------------------------------------------------------------
def test_quadrature_of_the_rhf_density_gives_the_electrons_and_the_dipole():
    """M1 (spherical) twice in the stack, the 49^3 grid of spacing 0.3 Bohr as two slabs of 27 planes (64827 points; they
    share 5 planes, counted once), different points per row.  Bounds from the host twin (tests/_density.py:
    ``quadrature_errors``): sum |D| (quadrature error of the products + u (c + M) sum of their absolute values)."""
    name = "m1-spherical"
    basis, xyz = P.basis_of(name), P.angstrom_of(name)
    pqc, ncas, nelecas = _circuit()
    b = aoo.OO_pqc_batch.from_geometries(pqc, basis, np.stack([xyz, xyz]), ncas, nelecas, oao_mo_coeffs="rhf")
    res = b.rhf(conv_tol=1e-12, err_tol=1e-10)
    assert bool(res.converged.all())
    grid = Dn.quadrature_points(P.xyz_of(name))                          # Bohr
    n2 = Dn.QUAD_N ** 2
    slabs = np.stack([grid[:27 * n2], grid[-27 * n2:]]) * BOHR
    rho, drho = b.rhf_electron_density(slabs, result=res, gradient=True)
    assert tuple(rho.shape) == (2, 27 * n2) and tuple(drho.shape) == (2, 27 * n2, 3)
    skip = (2 * 27 - Dn.QUAD_N) * n2
    full = torch.cat([rho[0], rho[1, skip:]])
    dfull = torch.cat([drho[0], drho[1, skip:]])
    pts = to_dev(grid)
    h = Dn.QUAD_H * BOHR
    nel = properties.integrate_grid(full, h).item()
    dint = properties.integrate_grid(dfull.T, h).cpu().numpy()
    R, Z = P.xyz_of(name), basis.charges
    dip = (to_dev(Z @ R) - properties.integrate_grid((pts * full[:, None]).T, h)).cpu().numpy()
    want = b.rhf_dipole_moment(result=res)[0].cpu().numpy()
    # bounds
    n_occ = basis.nelectron // 2
    Co = res.mo_coeff[0, :, :n_occ].cpu().numpy()
    Dabs = np.abs(2.0 * Co @ Co.T)
    eS, eD, eR, aS, aD, aR = Dn.quadrature_errors(name)
    uc = Dn.U * (Dn.bound_constant(basis) + full.numel())
    bN = float(np.sum(Dabs * (eS + uc * aS)))
    bD = np.sum(Dabs[None] * (eD + uc * aD), axis=(1, 2))
    mom = np.abs(gaussian.moment_integrals_from_table(basis.table, R, "spherical", order=1)[:3])
    bR = np.sum(Dabs[None] * (eR + uc * aR), axis=(1, 2)) + P.CLASSICAL_RTOL * (
        np.abs(Z[:, None] * R).sum(axis=0) + np.sum(Dabs[None] * mom, axis=(1, 2)))
    print(f"electrons {nel:.12f} (bound {bN:.2e}); integral of the gradient {dint} (bounds {bD}); dipole from the grid "
          f"{dip}, rhf_dipole_moment {want}, difference {np.abs(dip - want)} (bounds {bR})")
    assert basis.nelectron == 14 and abs(nel - 14.0) < bN
    assert np.all(np.abs(dint) < bD)
    assert np.all(np.abs(dip - want) < bR)


# ---- 6. the batch methods --------------------------------------------------------------------------------------------------------
def batch_points(G=3, M=5):
    return np.stack([C.cloud(formal_coords(POINTS)[g], M, on_nucleus=False, seed=50 + g)[1] for g in range(G)])


def test_electron_density_of_a_circuit_state_is_the_raw_call_on_its_density():
    b = cas_batch("ucc")
    th = seeded_thetas(b)
    pts = batch_points()
    rows = list(range(b.G))
    d1 = b._state_density(th, rows)
    rho, drho = b.electron_density(th, pts, gradient=True)
    raw, draw = density_batch(b.basis, formal_coords(POINTS), pts, d1, gradient=True)
    assert tuple(rho.shape) == (3, 5) and torch.equal(rho, raw) and torch.equal(drho, draw)
    assert torch.equal(b.electron_density(th, pts), rho)
    # index=: the same bits
    a, g = b.electron_density(th, pts[[2, 0]], index=[2, 0], gradient=True)
    assert torch.equal(a, rho[[2, 0]]) and torch.equal(g, drho[[2, 0]])
    assert torch.equal(b.electron_density(th, pts[1], index=1), rho[1:2])
    # against the host twin with the device density of geometry 0
    ref = gaussian.density_from_table(b.basis.table, formal_coords(POINTS)[0] / BOHR, pts[0] / BOHR, d1[0].cpu().numpy(),
                                      "spherical")
    ratio = np.abs(rho[0].cpu().numpy() - ref[0]) / (Dn.U * Dn.bound_constant(b.basis) * ref[1] + Dn.FLOOR)
    print(f"circuit state: rho {rho[0].tolist()}, against the host twin {ratio.max():.4f} bounds")
    assert ratio.max() < 1.0
    # RHF
    res = b.rhf(conv_tol=1e-12, err_tol=1e-10)
    r2, g2 = b.rhf_electron_density(pts, result=res, gradient=True)
    w2, wg2 = density_batch(b.basis, formal_coords(POINTS), pts, b._rhf_density(res, None, rows)[1], gradient=True)
    assert torch.equal(r2, w2) and torch.equal(g2, wg2)
    # and that density is 2 C_o C_o^T: the twin on the host product of geometry 0, within the bound
    Co = res.mo_coeff[0, :, :b.nelectron // 2].cpu().numpy()
    ref = gaussian.density_from_table(b.basis.table, formal_coords(POINTS)[0] / BOHR, pts[0] / BOHR, 2.0 * Co @ Co.T,
                                      "spherical", True)
    bc = Dn.U * Dn.bound_constant(b.basis)
    rr = max((np.abs(r2[0].cpu().numpy() - ref[0]) / (bc * ref[2] + Dn.FLOOR)).max(),
             (np.abs(g2[0].cpu().numpy() - ref[1]) / (bc * ref[3] + Dn.FLOOR)).max())
    print(f"RHF: the raw call on the density of _rhf_density to the bit; against the twin on 2 C_o C_o^T {rr:.4f} bounds")
    assert rr < 1.0
    assert torch.equal(b.rhf_electron_density(pts[[1]], index=[1]), b.rhf_electron_density(pts)[1:2])


@pytest.mark.parametrize("R", [1, 2, 4])
def test_casci_electron_density(R):
    """The matrix over the roots is ``density_into`` of the sets of ``_casci_densities`` bit for bit, cut into calls of
    ``MAX_GRAD_SETS`` sets as ``_density_of`` cuts them; exactly symmetric; R = 1 works.  R = 4, the most roots the CI
    solver takes (``ci.MAX_ROOTS``), makes 4 states and 6 pairs: 10 sets, one call filled to its limit.  The cut into
    several calls on this path is run with the limit lowered to 4 sets per call (10 = 4 + 4 + 2): the same bits."""
    b = cas_batch("ucc", 2)
    pts = batch_points(2)
    e, rho, drho = b.casci_electron_density(pts, nroots=R, gradient=True)
    assert tuple(rho.shape) == (2, R, R, 5) and tuple(drho.shape) == (2, R, R, 5, 3)
    assert torch.equal(rho, rho.transpose(1, 2)) and torch.equal(drho, drho.transpose(1, 2))
    e0, dens, _ = b._casci_densities("test", R, True, 1e-9, 200)
    assert torch.equal(e, e0)
    assert int(dens.shape[1]) == R + R * (R - 1) // 2
    outs = [density_into(b.basis, b.coords_bohr, to_dev(pts / BOHR), dens[:, a:a + gto.MAX_GRAD_SETS].contiguous(), True)
            for a in range(0, int(dens.shape[1]), gto.MAX_GRAD_SETS)]
    raw = torch.cat([o[0] for o in outs], dim=1)
    draw = torch.cat([o[1] for o in outs], dim=1)
    from auto_oo_amd.batch import pair_matrix
    assert torch.equal(rho, pair_matrix(raw, R)) and torch.equal(drho, pair_matrix(draw, R))
    assert torch.equal(b.casci_electron_density(pts, nroots=R)[1], rho)
    if R == 4:
        from auto_oo_amd import ci
        assert ci.MAX_ROOTS == 4
        calls = []
        real = gto.density_into
        with mock.patch.object(gto, "MAX_GRAD_SETS", 4), mock.patch.object(
                gto, "density_into", lambda *a, **k: calls.append(int(a[3].shape[1])) or real(*a, **k)):
            _, crho, cdrho = b.casci_electron_density(pts, nroots=R, gradient=True)
        assert calls == [4, 4, 2] and torch.equal(crho, rho) and torch.equal(cdrho, drho)
    print(f"R = {R}: {int(dens.shape[1])} densities; rho of the ground state {rho[0, 0, 0].tolist()}")


def test_more_sets_than_one_call_takes_and_orbital_values():
    b = cas_batch("ucc", 2)
    pts = batch_points(2)
    dens = to_dev(np.random.default_rng(3).uniform(-1, 1, (2, gto.MAX_GRAD_SETS + 3, b.nao, b.nao)))
    rho, drho = b._density_of([0, 1], dens, pts, True)
    assert tuple(rho.shape) == (2, gto.MAX_GRAD_SETS + 3, 5)
    for k in (0, gto.MAX_GRAD_SETS - 1, gto.MAX_GRAD_SETS, gto.MAX_GRAD_SETS + 2):
        a, g = density_batch(b.basis, formal_coords(POINTS[:2]), pts, dens[:, k], gradient=True)
        assert torch.equal(a, rho[:, k]) and torch.equal(g, drho[:, k])
    # orbital values: the default columns, all 13 (two calls), a choice, index=
    n_def = b._n_occ + b.ncas
    psi, dpsi = b.orbital_values(pts, gradient=True)
    assert tuple(psi.shape) == (2, n_def, 5) and tuple(dpsi.shape) == (2, n_def, 5, 3)
    allc = b.orbital_values(pts, columns=range(b.nao))
    assert tuple(allc.shape) == (2, b.nao, 5) and b.nao > gto.MAX_GRAD_SETS and torch.equal(allc[:, :n_def], psi)
    raw = orbital_values_batch(b.basis, formal_coords(POINTS[:2]), pts, b.mo_coeff[:, :, [12, 3]].contiguous())
    assert torch.equal(b.orbital_values(pts, columns=[12, 3]), raw) and torch.equal(raw, allc[:, [12, 3]])
    assert torch.equal(b.orbital_values(pts[1], index=1), psi[1:2])
    with pytest.raises(ValueError, match="columns"):
        b.orbital_values(pts, columns=[13])


def many_shell_basis(n):
    """one atom with n s shells of one primitive each"""
    return gto.GTOBasis(["H"], {"H": [("s", [a], [1.0]) for a in np.geomspace(0.05, 40.0, n)]})


def raw_density_call(basis, xyz_bohr, pts_bohr, dm, gradient):
    """the return code of ``oovqe_gto_density_batch`` itself (``density_into`` cuts the sets before it is reached)"""
    from auto_oo_amd._lib import dptr, load, stream_ptr
    G, K, M = int(dm.shape[0]), int(dm.shape[1]), int(pts_bohr.shape[1])
    rho = torch.empty((G, K, M), dtype=F64, device=dev())
    drho = torch.empty((G, K, M, 3), dtype=F64, device=dev()) if gradient else None
    return load().oovqe_gto_density_batch(*gto._head(basis, dev())[:-1], G, dptr(xyz_bohr), basis.nao, K, dptr(dm), M,
                                          dptr(pts_bohr), dptr(rho), dptr(drho), stream_ptr())


def test_tables_with_many_shells():
    """The density kernel holds K + nshell LDS columns (4 K + 2 nshell with the gradient) of 121.  45 shells: 7 sets per
    launch with the gradient; the entry takes 7 and refuses 8 with a message, ``density_into`` cuts 10 sets into 7 + 3
    with the bits of each set alone, within the bound of the twin.  115 shells: 6 sets without the gradient, none with it:
    refused."""
    from auto_oo_amd._lib import OovqeError, load
    rng = np.random.default_rng(9)
    pts = rng.uniform(-1.5, 1.5, (1, 70, 3))
    xyz = np.zeros((1, 1, 3))
    for n, grad, most in ((45, True, 7), (45, False, 10), (115, False, 6), (115, True, 0)):
        basis = many_shell_basis(n)
        assert basis.nshell == n and gto.density_max_sets(basis, grad) == most
        dm = to_dev(rng.uniform(-1.0, 1.0, (1, gto.MAX_GRAD_SETS, n, n)))
        if most:
            assert raw_density_call(basis, to_dev(xyz), to_dev(pts), dm[:, :most].contiguous(), grad) == 0
        if most < gto.MAX_GRAD_SETS:
            assert raw_density_call(basis, to_dev(xyz), to_dev(pts), dm[:, :most + 1].contiguous(), grad) < 0
            assert b"LDS" in load().oovqe_last_error()
        if not most:
            with pytest.raises(OovqeError, match="LDS"):
                density_batch(basis, xyz * BOHR, pts * BOHR, dm, gradient=grad)
            continue
        out = density_into(basis, to_dev(xyz), to_dev(pts), dm, grad)
        rho = out[0] if grad else out
        for k in (0, most - 1, most % gto.MAX_GRAD_SETS, gto.MAX_GRAD_SETS - 1):
            one = density_into(basis, to_dev(xyz), to_dev(pts), dm[:, k:k + 1].contiguous(), grad)
            assert torch.equal((one[0] if grad else one)[:, 0], rho[:, k])
            if grad:
                assert torch.equal(one[1][:, 0], out[1][:, k])
        ref = gaussian.density_from_table(basis.table, xyz[0], pts[0], dm[0].cpu().numpy(), "spherical", True)
        bc = Dn.U * Dn.bound_constant(basis)
        r = (np.abs(rho[0].cpu().numpy() - ref[0]) / (bc * ref[2] + Dn.FLOOR)).max()
        if grad:
            r = max(r, (np.abs(out[1][0].cpu().numpy() - ref[1]) / (bc * ref[3] + Dn.FLOOR)).max())
        print(f"{n} shells, gradient {grad}: {most} sets per launch; against the twin {r:.4f} bounds")
        assert r < 1.0


def test_embedded_batch():
    pqc, ncas, nelecas = _circuit()
    xyz = formal_coords(POINTS[:2])
    q, r = C.cloud(xyz[0], 4, on_nucleus=False)
    from tests.test_moments_gpu import formal_basis
    b = aoo.OO_pqc_batch.from_geometries(pqc, formal_basis(), xyz, ncas, nelecas, oao_mo_coeffs="rhf",
                                         point_charges=(np.tile(q, (2, 1)), np.tile(r, (2, 1, 1))))
    pts = batch_points(2)
    res = b.rhf(conv_tol=1e-12, err_tol=1e-10)
    rho, drho = b.rhf_electron_density(pts, result=res, gradient=True)
    th = seeded_thetas(b)
    rs = b.electron_density(th, pts)
    assert tuple(rho.shape) == (2, 5) and bool(torch.isfinite(rho).all()) and bool(torch.isfinite(drho).all())
    # (a density of positive occupations is nowhere negative; far out it underflows to an exact zero)
    assert tuple(rs.shape) == (2, 5) and bool((rho >= 0).all()) and bool((rs >= 0).all()) and rho[:, 0].min().item() > 1.0
    free = cas_batch("np_fabric", 2)
    assert not torch.equal(free.rhf_electron_density(pts), rho)          # the charges polarise the density


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_raw_calls():
    name = "water"
    basis, xyz = P.basis_of(name), P.angstrom_of(name)[None]
    N = basis.nao
    pts = P.points_angstrom(name)[:5]
    dm = to_dev(P.densities(name))[None]
    cm = to_dev(Dn.coefficients(name))[None]
    for bad in (np.zeros(3), np.zeros((2, 5, 3)), np.zeros((5, 2)), np.zeros((0, 3)), np.zeros((gto.MAX_POINTS + 1, 3))):
        with pytest.raises(ValueError, match="points"):
            density_batch(basis, xyz, bad, dm)
        with pytest.raises(ValueError, match="points"):
            orbital_values_batch(basis, xyz, bad, cm)
    nan = pts.copy()
    nan[2, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        density_batch(basis, xyz, nan, dm)
    with pytest.raises(ValueError, match="finite"):
        density_batch(basis, xyz, pts, dm * float("inf"))
    with pytest.raises(ValueError, match="finite"):
        orbital_values_batch(basis, xyz, pts, cm * float("nan"))
    for bad in (dm[0, 0], dm[:, :, :-1], to_dev(np.zeros((1, 0, N, N))), to_dev(np.zeros((1, gto.MAX_GRAD_SETS + 1, N, N))),
                to_dev(np.zeros((2, 1, N, N)))):
        with pytest.raises(ValueError):
            density_batch(basis, xyz, pts, bad)
    for bad in (cm[0], cm[:, :-1], to_dev(np.zeros((1, N, 0))), to_dev(np.zeros((1, N, gto.MAX_GRAD_SETS + 1))),
                to_dev(np.zeros((2, N, 1)))):
        with pytest.raises(ValueError):
            orbital_values_batch(basis, xyz, pts, bad)
    for call in (lambda: density_into(basis, to_dev(xyz), to_dev(pts)[None, :, :2], dm),
                 lambda: density_into(basis, to_dev(xyz), to_dev(np.zeros((1, gto.MAX_POINTS + 1, 3))), dm),
                 lambda: orbital_values_into(basis, to_dev(xyz), to_dev(pts), cm)):
        with pytest.raises(ValueError, match="points"):
            call()


def test_refusals_of_the_batch_methods():
    pqc, ncas, nelecas = _circuit()
    from auto_oo_amd.gaussian import Moldata_sto3g
    from auto_oo_amd import get_formal_geo
    host = aoo.OO_pqc_batch(pqc, [Moldata_sto3g(get_formal_geo(*POINTS[0]))], ncas, nelecas, oao_mo_coeffs=[np.eye(13)])
    th = torch.zeros((1, host.n_theta), dtype=F64)
    pts = batch_points()
    for call in (lambda: host.electron_density(th, pts[0]), lambda: host.rhf_electron_density(pts[0]),
                 lambda: host.casci_electron_density(pts[0]), lambda: host.orbital_values(pts[0])):
        with pytest.raises(RuntimeError, match="from_geometries"):
            call()
    b = cas_batch("ucc")
    th = seeded_thetas(b)
    for bad in (np.zeros(3), np.zeros((2, 5, 3)), np.zeros((5, 2)), np.zeros((3, 0, 3)), np.full((3, 3), np.nan)):
        with pytest.raises(ValueError, match="points"):
            b.electron_density(th, bad)
        with pytest.raises(ValueError, match="points"):
            b.casci_electron_density(bad)
    # oversized ncas: what the potential methods do
    with mock.patch.object(nucgrad, "MAX_NCAS", b.ncas - 1):
        for meth, pot in (("electron_density", "electrostatic_potential"),):
            with pytest.raises(NotImplementedError) as want:
                getattr(b, pot)(th, pts)
            with pytest.raises(NotImplementedError) as got:
                getattr(b, meth)(th, pts)
            assert str(got.value) == str(want.value)
        with pytest.raises(NotImplementedError, match="ncas"):
            b.casci_electron_density(pts)
        with pytest.raises(NotImplementedError, match="ncas"):
            b.casci_electrostatic_potential(pts)


def test_a_sector_engine_circuit_is_refused():
    """kUpCCD CAS(6e,6o) (12 qubits: the sector engine).  The potential methods serve such a circuit (they take its RDMs
    from the engine); its density is not part of this feature: ``electron_density`` raises before anything is launched,
    also with the gradient and with ``index``.  The methods that do not run the circuit still work on that batch."""
    b = cas_batch("kupccd", 2)
    assert b.pqc._use_sector
    th = seeded_thetas(b)
    pts = batch_points(2)
    launched = []
    with mock.patch.object(gto, "density_into", lambda *a, **k: launched.append(a)), mock.patch.object(
            type(b), "_state_density", lambda *a, **k: launched.append(a)):
        for kwargs in ({}, {"gradient": True}, {"index": [1]}):
            with pytest.raises(NotImplementedError, match="sector engine"):
                b.electron_density(th, pts[kwargs.get("index", slice(None))], **kwargs)
    assert not launched
    assert tuple(b.electrostatic_potential(th, pts).shape) == (2, 5)
    psi = b.orbital_values(pts, columns=[0, 1])
    assert tuple(psi.shape) == (2, 2, 5) and bool(torch.isfinite(psi).all())
