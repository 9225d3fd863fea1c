"""Electrostatic potential and field on the device (csrc/gto_potential.hip, gto.potential_*, the
``*electrostatic_potential`` methods of OO_pqc_batch) against the host twin ``gaussian.potential_from_table``, against
differences of the host twin, against the embedding kernels that already exist on the device, and against the
derivative of the embedded RHF energy in a charge.

Bounds: tests/_potential.py (none taken from what the device code gives).  Every comparison prints its figures before
it asserts.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import auto_oo_amd as aoo                                   # noqa: E402
from auto_oo_amd import ci, gaussian, gto, nucgrad, ops     # noqa: E402
from tests import _ci_dense                                 # noqa: E402
from tests import _charges as C                             # noqa: E402
from tests import _gto_d as D                               # noqa: E402
from tests import _potential as P                           # noqa: E402
from tests.test_moments_gpu import cas_batch, seeded_thetas, formal_coords, POINTS, _circuit   # noqa: E402

F64 = torch.float64
BOHR = gaussian.BOHR


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def to_dev(x):
    return torch.as_tensor(np.array(x, dtype=np.float64, order="C")).to(dev())


def device_potential(name, dm, points_angstrom=None, nuc=False, field=True):
    """``gto.potential_batch`` of one geometry of a case -> numpy (phi [K, M], F [K, M, 3])"""
    pts = P.points_angstrom(name) if points_angstrom is None else points_angstrom
    out = gto.potential_batch(P.basis_of(name), P.angstrom_of(name)[None], pts, to_dev(dm)[None], nuc=nuc, field=field)
    if not field:
        return out[0].cpu().numpy(), None
    return out[0][0].cpu().numpy(), out[1][0].cpu().numpy()


def check_against_host(name, phi, F, label):
    """phi against the host twin, F against the differences of the host twin at the kept points"""
    ref, bound = P.host_phi(name), P.POTENTIAL_BOUND[name]
    err = np.abs(phi - ref).max()
    Fr, Fb, kept = P.host_field(name)
    ratio = np.abs(F[:, kept] - Fr) / Fb
    print(f"{label}: |phi| up to {np.abs(ref).max():.3g}, |device - host| {err:.2e} (bound {bound:.2e}); field up to "
          f"{np.abs(Fr).max():.3g}, worst |device - difference| / bound {ratio.max():.3f} (bounds {Fb.min():.1e} .. "
          f"{Fb.max():.1e}), {int((~kept).sum())} of {kept.size} points left out of the difference reference")
    assert np.isfinite(phi).all() and np.isfinite(F).all()
    assert int((~kept).sum()) <= P.FD_EXCLUDE_CAP
    assert err < bound
    assert ratio.max() < 1.0


# ---- 1. pair classes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.L_CASES)
def test_one_pair_class_against_the_host_twin(name):
    """Two centres, one shell each, 10-primitive contractions; the density lives in the block of the two shells and its
    transpose alone, K = 1, M = 65 (one wave and one point), both d forms."""
    dm = P.class_density(name)
    phi, F = device_potential(name, dm)
    assert phi.shape == (1, P.M_CLASS) and F.shape == (1, P.M_CLASS, 3)
    check_against_host(name, phi, F, name)


# ---- 2. whole molecules ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.MOL_CASES)
def test_whole_molecules_against_the_host_twin(name):
    """K = 3 random non-symmetric densities at the 130-point cloud (0.2 Bohr from a nucleus, ON a nucleus, 50 Bohr away),
    without the nuclei: finite everywhere and within bound; the symmetrised densities give the same to the bound."""
    dm = P.densities(name)
    phi, F = device_potential(name, dm)
    assert phi.shape == (P.K, C.M_MAX)
    check_against_host(name, phi, F, name)
    sphi, sF = device_potential(name, 0.5 * (dm + dm.transpose(0, 2, 1)))
    Fb = P.host_field(name)[1].max()
    print(f"{name}: symmetrised densities: phi {np.abs(sphi - phi).max():.2e}, field {np.abs(sF - F).max():.2e}")
    assert np.abs(sphi - phi).max() < P.POTENTIAL_BOUND[name]
    assert np.abs(sF - F).max() < Fb


@pytest.mark.parametrize("name", P.MOL_CASES)
def test_nuclear_term_and_the_point_on_a_nucleus(name):
    """With the nuclei the entries of the point ON atom 1 are not finite, and no other entry notices that point: the same
    bits as with that point moved away.  The nuclear part is the closed form to CLASSICAL_RTOL of the absolute terms."""
    dm = P.densities(name)
    pts = P.points_angstrom(name)
    phi0, F0 = device_potential(name, dm, pts, nuc=False)
    phi1, F1 = device_potential(name, dm, pts, nuc=True)
    assert not np.isfinite(phi1[:, 1]).any() and not np.isfinite(F1[:, 1]).any()
    others = np.arange(C.M_MAX) != 1
    assert np.isfinite(phi1[:, others]).all() and np.isfinite(F1[:, others]).all()
    away = C.cloud(P.angstrom_of(name), on_nucleus=False)[1]
    phi2, F2 = device_potential(name, dm, away, nuc=True)
    assert np.array_equal(phi2[:, others], phi1[:, others]) and np.array_equal(F2[:, others], F1[:, others])
    assert np.isfinite(phi2).all() and np.isfinite(F2).all()
    pn, fn, fabs = P.nuclear_potential(name, pts[others] / BOHR)
    ep = np.abs((phi1 - phi0)[:, others] - pn) / (pn + np.abs(phi0[:, others]))
    ef = np.abs((F1 - F0)[:, others] - fn) / (fabs + np.abs(F0[:, others]))
    print(f"{name}: nuclear potential {ep.max():.2e}, nuclear field {ef.max():.2e} of the absolute terms (bound "
          f"{P.CLASSICAL_RTOL:.0e})")
    assert ep.max() < P.CLASSICAL_RTOL and ef.max() < P.CLASSICAL_RTOL
    # one flag per set
    mix = gto.potential_batch(P.basis_of(name), P.angstrom_of(name)[None], away, to_dev(dm)[None], nuc=[True, False, True])
    phi3, _ = device_potential(name, dm, away, nuc=False)
    assert np.array_equal(mix[0].cpu().numpy()[[0, 2]], phi2[[0, 2]]) and np.array_equal(mix[0, 1].cpu().numpy(), phi3[1])


# ---- 3. Boys arguments -------------------------------------------------------------------------------------------------
def test_boys_arguments():
    """Lss (10-primitive s shells): a point ON the atom (T = 0 for its one-centre pairs), T just below and just above the
    switch of the Boys function for the tightest and the loosest primitive pair, 60 and 2000 Bohr away; and the same
    distances around the d shell of Ldd."""
    for name in ("Lss", "Ldd"):
        pts = P.boys_points(name)
        dm = P.densities(name, 1, 5)
        phi, F = device_potential(name, dm, pts * BOHR)
        # (pts * BOHR / BOHR need not be pts to the bit: the host gets what the device gets)
        ref, bound = P.measured_bound_at(name, (pts * BOHR) / BOHR, dm)
        err = np.abs(phi - ref)
        print(f"{name}: distances 0, switch -+ (tight), switch -+ (loose), 60, 2000 Bohr: phi {ref[0]}, |device - host| "
              f"{err[0]} (bound {bound:.2e})")
        assert np.isfinite(phi).all() and np.isfinite(F).all()
        assert err.max() < bound
        # far away every term is D_ab S_ab / r and the bound above says nothing about values of 1e-3: there, two
        # analytic evaluations in different order, CLASSICAL_RTOL of the sum of the absolute terms
        shells = gaussian.shells_from_table(P.basis_of(name).table, P.xyz_of(name))
        U = gaussian.basis_transform(P.basis_of(name).table, P.form_of(name))
        S = U @ gaussian.one_electron_integrals(shells, (), ())[0] @ U.T
        scale = np.abs(dm[0] * S).sum() / np.array([60.0, 2000.0])
        print(f"{name}: far points {phi[0, 5:]}, |device - host| / sum of absolute terms {err[0, 5:] / scale}")
        assert (err[0, 5:] < P.CLASSICAL_RTOL * scale).all()


# ---- 4. same bits ------------------------------------------------------------------------------------------------------
SAME = "m1-spherical"           # all six pair classes


def raw(basis, xyz_a, pts_a, dm, **kw):
    return gto.potential_batch(basis, xyz_a, pts_a, dm, **kw)


def test_a_point_has_the_same_bits_alone_and_anywhere_in_a_cloud():
    basis, xyz = P.basis_of(SAME), P.angstrom_of(SAME)
    dm = to_dev(P.densities(SAME))[None]
    cloud = P.points_angstrom(SAME)
    for k in (0, 1, 2, 7):
        phi1, F1 = raw(basis, xyz[None], cloud[k:k + 1], dm, nuc=False, field=True)
        for M in C.M_SIZES[1:]:
            for place in (0, M // 2, M - 1):
                others = [i for i in range(M) if i != k][:M - 1]
                order = others[:place] + [k] + others[place:]
                phi, F = raw(basis, xyz[None], cloud[order], dm, nuc=False, field=True)
                assert torch.equal(phi[:, :, place], phi1[:, :, 0]) and torch.equal(F[:, :, place], F1[:, :, 0]), (k, M, place)


def stack_of_three():
    basis, xyz = P.basis_of(SAME), P.angstrom_of(SAME)
    X = np.stack([xyz, xyz + 0.05 * np.array([0.3, -0.2, 0.5]), D.M1_MOVED])
    pts = np.stack([C.cloud(X[g], on_nucleus=False, seed=40 + g)[1] for g in range(3)])
    dm = to_dev(np.stack([P.densities(SAME, P.K, 20 + g) for g in range(3)]))
    return basis, X, pts, dm


def test_a_geometry_has_the_same_bits_alone_permuted_and_on_another_stream():
    basis, X, pts, dm = stack_of_three()
    phi, F = raw(basis, X, pts, dm, field=True)
    assert tuple(phi.shape) == (3, P.K, C.M_MAX) and tuple(F.shape) == (3, P.K, C.M_MAX, 3)
    perm = [2, 0, 1]
    pphi, pF = raw(basis, X[perm], pts[perm], dm[perm].contiguous(), field=True)
    assert torch.equal(pphi, phi[perm]) and torch.equal(pF, F[perm])
    for g in range(3):
        aphi, aF = raw(basis, X[g:g + 1], pts[g:g + 1], dm[g:g + 1], field=True)
        assert torch.equal(aphi[0], phi[g]) and torch.equal(aF[0], F[g])
    assert not torch.equal(phi[0], phi[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sphi, sF = raw(basis, X, pts, dm, field=True)
    side.synchronize()
    assert torch.equal(sphi, phi) and torch.equal(sF, F)
    # field on against field off
    assert torch.equal(raw(basis, X, pts, dm, field=False), phi)
    # points shared by all geometries
    shared = raw(basis, X, pts[0], dm)
    assert torch.equal(shared[0], phi[0]) and tuple(shared.shape) == (3, P.K, C.M_MAX)


def test_a_set_has_the_same_bits_alone_and_among_ten():
    basis, xyz = P.basis_of(SAME), P.angstrom_of(SAME)
    pts = C.cloud(xyz, on_nucleus=False)[1]
    ten = to_dev(P.densities(SAME, gto.MAX_GRAD_SETS, 31))[None]
    one = to_dev(P.densities(SAME, 1, 32))
    phi1, F1 = raw(basis, xyz[None], pts, one, field=True)                 # [1, N, N]: the K axis is dropped
    assert tuple(phi1.shape) == (1, C.M_MAX) and tuple(F1.shape) == (1, C.M_MAX, 3)
    for place in (0, 9):
        dm = ten.clone()
        dm[0, place] = one[0]
        phi, F = raw(basis, xyz[None], pts, dm, field=True)
        assert torch.equal(phi[0, place], phi1[0]) and torch.equal(F[0, place], F1[0])
        assert not torch.equal(phi[0, 4], phi1[0])
    # the order of the other sets
    flipped = raw(basis, xyz[None], pts, ten.flip(1).contiguous())
    assert torch.equal(flipped.flip(1), raw(basis, xyz[None], pts, ten))


def test_no_geometries():
    basis = P.basis_of("water")
    phi, F = gto.potential_batch(basis, np.zeros((0, 3, 3)), np.zeros((4, 3)),
                                 torch.zeros((0, 2, basis.nao, basis.nao), dtype=F64, device=dev()), field=True)
    assert tuple(phi.shape) == (0, 2, 4) and tuple(F.shape) == (0, 2, 4, 3) and phi.is_cuda


# ---- 5. against the embedding kernels ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.CASES)
def test_potential_weighted_with_charges_is_the_trace_with_the_embedding_operator(name):
    """sum_m q_m phi_el[m] = tr(D V_ext): two analytic evaluations in different order of summation"""
    basis, xyz = C.case(name)
    q, r = C.cloud(xyz)
    dm = np.random.default_rng(3).uniform(-1.0, 1.0, (basis.nao, basis.nao))
    V = gto.point_charge_integrals_batch(basis, xyz, q, r)[0].cpu().numpy()
    phi = gto.potential_batch(basis, xyz[None], r, to_dev(dm)[None], nuc=False)[0].cpu().numpy()
    lhs, rhs = float(np.sum(q * phi)), float(np.sum(dm * V))
    scale = max(np.abs(q * phi).sum(), np.abs(dm * V).sum())
    print(f"{name}: sum q phi = {lhs:.15g}, tr(D V_ext) = {rhs:.15g}, difference {abs(lhs - rhs):.2e} of {scale:.3g}")
    assert abs(lhs - rhs) < P.CLASSICAL_RTOL * scale


def test_field_times_charge_is_minus_the_force_kernel_of_the_charges():
    """gQ[m] = -q_m F[m], nuclear terms on in both (s and p shells: the scope of the gradient kernel).  The sum of the
    absolute terms of a component is bounded by the nuclear ones plus the field of sum |D S| electrons at the distance
    of the nearest nucleus."""
    basis, xyz = C.case("water")
    q, r = C.cloud(xyz, on_nucleus=False)
    dm = C.random_symmetric(basis.nao, 11)
    gQ = gto.point_charge_gradient_batch(basis, xyz, q, r, to_dev(dm)[None], nuc=True)[1][0].cpu().numpy()
    F = gto.potential_batch(basis, xyz[None], r, to_dev(dm)[None], nuc=True, field=True)[1][0].cpu().numpy()
    S = gto.integrals_batch(basis, xyz[None]).overlap[0].cpu().numpy()
    dist = np.linalg.norm(C.bohr(r)[:, None, :] - C.bohr(xyz)[None, :, :], axis=2)
    scale = np.abs(q) * ((basis.charges / dist ** 2).sum(axis=1) + np.abs(dm * S).sum() / dist.min(axis=1) ** 2)
    live = q != 0.0
    err = np.abs(gQ + q[:, None] * F).max(axis=1)
    print(f"gQ + q F: worst {err.max():.2e}, worst relative to the absolute terms {(err[live] / scale[live]).max():.2e}")
    assert (err[live] < P.CLASSICAL_RTOL * scale[live]).all() and err[~live].max() == 0.0


# ---- 6. end to end: d E_RHF / d q_k = phi(r_k) --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["water", "m2-spherical"])
def test_rhf_potential_is_the_charge_derivative_of_the_embedded_energy(name):
    """RHF is variational, so Hellmann-Feynman holds: the central difference of the embedded RHF energy in one charge
    q_k, at the steps 1e-3 and 2e-3 e, all 16 displaced copies and the undisplaced one in ONE stack; bound max(1e-9, 10 x
    the disagreement of the two steps)."""
    basis, xyz = C.case(name)
    q, r = C.cloud(xyz, 4, on_nucleus=False)
    steps = (1e-3, -1e-3, 2e-3, -2e-3)
    Q = np.tile(q, (17, 1))
    for k in range(4):
        for s, h in enumerate(steps):
            Q[1 + 4 * k + s, k] += h
    pqc, ncas, nelecas = _circuit()
    b = aoo.OO_pqc_batch.from_geometries(pqc, basis, np.tile(xyz, (17, 1, 1)), ncas, nelecas, oao_mo_coeffs="rhf",
                                         point_charges=(Q, np.tile(r, (17, 1, 1))))
    res = b.rhf(conv_tol=1e-13, err_tol=1e-11)
    assert bool(res.converged.all())
    e = res.e_tot.cpu().numpy()[1:].reshape(4, 4)
    d1 = (e[:, 0] - e[:, 1]) / 2e-3
    d2 = (e[:, 2] - e[:, 3]) / 4e-3
    bound = np.maximum(1e-9, 10.0 * np.abs(d1 - d2))
    one = res._replace(**{f: getattr(res, f)[:1] for f in res._fields if getattr(res, f) is not None})
    phi, F = b.rhf_electrostatic_potential(r, result=one, index=0, field=True)
    assert tuple(phi.shape) == (1, 4) and tuple(F.shape) == (1, 4, 3)
    err = np.abs(phi[0].cpu().numpy() - d1)
    print(f"{name}: phi(r_k) = {phi[0].tolist()}, dE/dq_k = {d1.tolist()}, |difference| {err} (bounds {bound})")
    assert (err < bound).all()


# ---- 7. the batch methods ----------------------------------------------------------------------------------------------
def batch_points(G=3, M=5):
    return np.stack([C.cloud(formal_coords(POINTS)[g], M, on_nucleus=False, seed=50 + g)[1] for g in range(G)])


def test_rhf_electrostatic_potential_is_the_raw_call_on_the_rhf_density():
    b = cas_batch("ucc")
    pts = batch_points()
    res = b.rhf(conv_tol=1e-12, err_tol=1e-10)
    phi, F = b.rhf_electrostatic_potential(pts, result=res, field=True)
    n_occ = b.nelectron // 2
    Co = res.mo_coeff[:, :, :n_occ]
    dm = 2.0 * Co @ Co.transpose(1, 2)
    rphi, rF = gto.potential_batch(b.basis, formal_coords(POINTS), pts, dm, field=True)
    err = max((phi - rphi).abs().max().item(), (F - rF).abs().max().item())
    print(f"RHF: against the raw call on 2 C_o C_o^T {err:.2e}")
    assert tuple(phi.shape) == (3, 5) and tuple(F.shape) == (3, 5, 3) and err < 1e-12
    assert torch.equal(b.rhf_electrostatic_potential(pts, result=res), phi)
    sub = res._replace(**{f: getattr(res, f)[[2, 0]] for f in res._fields if getattr(res, f) is not None})
    assert torch.equal(b.rhf_electrostatic_potential(pts[[2, 0]], result=sub, index=[2, 0]), phi[[2, 0]])
    with pytest.raises(ValueError, match="rows asked"):
        b.rhf_electrostatic_potential(pts, result=sub)


@pytest.mark.parametrize("kind", ["ucc", "np_fabric"])
def test_electrostatic_potential_of_a_circuit_state_is_the_raw_call_on_its_density(kind):
    b = cas_batch(kind)
    th = seeded_thetas(b)
    pts = batch_points()
    pqc = b.pqc
    gamma, Gamma = ops.circuit_rdms(th, pqc._gates_dev, pqc._n_gates, pqc.n_qubits, b.ncas, pqc._init_index,
                                    tangents=False)
    d1 = nucgrad.cas_ao_densities(b.mo_coeff, b._n_occ, b.ncas, gamma[:, 0], Gamma[:, 0], want_d2=False)[0]
    phi, F = b.electrostatic_potential(th, pts, field=True)
    rphi, rF = gto.potential_batch(b.basis, formal_coords(POINTS), pts, d1, field=True)
    assert tuple(phi.shape) == (3, 5) and torch.equal(phi, rphi) and torch.equal(F, rF)
    # against the host twin with the host density of geometry 0
    hd, _ = nucgrad.cas_ao_densities_host(b.mo_coeff[0].cpu().numpy(), b._n_occ, b.ncas, gamma[0, 0].cpu().numpy(),
                                          Gamma[0, 0].cpu().numpy())
    ref = gaussian.potential_from_table(b.basis.table, b.basis.charges, formal_coords(POINTS)[0] / BOHR, pts[0] / BOHR,
                                        hd, "spherical")
    err = np.abs(phi[0].cpu().numpy() - ref).max()
    print(f"{kind}: phi {phi[0].tolist()}, against host D1 and the host twin {err:.2e}")
    assert err < 1e-10
    # the same bits whatever index
    assert torch.equal(b.electrostatic_potential(th, pts[[2, 0]], index=[2, 0]), phi[[2, 0]])
    assert torch.equal(b.electrostatic_potential(th, pts[1], index=1), phi[1:2])
    assert torch.equal(b.electrostatic_potential(th, pts), phi)


def test_casci_electrostatic_potential():
    b = cas_batch("ucc", 2)
    a, ne, R = b.ncas, b.nelecas, 3
    pts = batch_points(2)
    e, phi, F = b.casci_electrostatic_potential(pts, nroots=R, field=True)
    e0, vecs = b.casci(nroots=R)
    assert tuple(phi.shape) == (2, R, R, 5) and tuple(F.shape) == (2, R, R, 5, 3)
    assert (e - e0).abs().max().item() < 1e-12
    assert torch.equal(phi, phi.transpose(1, 2)) and torch.equal(F, F.transpose(1, 2))
    e1, phi1 = b.casci_electrostatic_potential(pts, nroots=R)
    assert torch.equal(phi1, phi)
    # the diagonal: each root's own D1 through the raw call, nuclear term included
    g1, g2 = ci.sector_rdms(vecs.reshape(2 * R, -1), a, ne)
    Cm = b.mo_coeff[:, None].expand(2, R, b.nao, b.nao).reshape(2 * R, b.nao, b.nao)
    d1 = nucgrad.cas_ao_densities(Cm, b._n_occ, a, g1, g2, want_d2=False)[0].reshape(2, R, b.nao, b.nao)
    diag = gto.potential_batch(b.basis, formal_coords(POINTS[:2]), pts, d1)
    k = torch.arange(R, device=dev())
    err = (phi[:, k, k] - diag).abs().max().item()
    print(f"state potentials against the raw call on each root's D1: {err:.2e}")
    assert err < 1e-12
    # the off-diagonal against the transition density of the two CI vectors
    Ex = _ci_dense.excitation_matrices(a, ne)
    c = vecs.cpu().numpy()
    worst = 0.0
    for g in range(2):
        Ca = b.mo_coeff[g].cpu().numpy()[:, b._n_occ:b._n_occ + a]
        for i in range(R):
            for j in range(i):
                gam = np.einsum("x,pqxy,y->pq", c[g, i], Ex, c[g, j])          # (not symmetrised: tr(D V) does that)
                want = gaussian.potential_from_table(b.basis.table, b.basis.charges, formal_coords(POINTS)[g] / BOHR,
                                                     pts[g] / BOHR, Ca @ gam @ Ca.T, "spherical", nuc=False)
                worst = max(worst, np.abs(phi[g, i, j].cpu().numpy() - want).max())
    print(f"transition potentials against the dense excitation matrices and the host twin: {worst:.2e}, largest "
          f"{phi[:, 1, 0].abs().max().item():.3g}")
    assert worst < 1e-10
    assert phi[:, 1, 0].abs().max().item() > 1e-5 or phi[:, 2, 0].abs().max().item() > 1e-5
    # apply_tracking permutes and signs the matrix like any other [G, R, R, ...] quantity
    from auto_oo_amd import overlaps
    perm = torch.tensor([[1, 0, 2], [0, 1, 2]], device=dev())
    sign = torch.tensor([[1.0, -1.0, 1.0], [1.0, 1.0, -1.0]], dtype=F64, device=dev())
    tracked = overlaps.apply_tracking(phi, perm, sign)
    assert tuple(tracked.shape) == tuple(phi.shape) and torch.equal(tracked, tracked.transpose(1, 2))


def test_casci_electrostatic_potential_of_one_root():
    """``nroots=1``: no pair, the matrices are the one root's potential and field -- the same library call on the same
    ``D1``, so the same bits."""
    b = cas_batch("ucc", 2)
    pts = batch_points(2, 3)
    e, phi, F = b.casci_electrostatic_potential(pts, nroots=1, field=True)
    e0, vecs = b.casci(nroots=1)
    assert tuple(e.shape) == (2, 1) and tuple(phi.shape) == (2, 1, 1, 3) and tuple(F.shape) == (2, 1, 1, 3, 3)
    assert torch.equal(e, e0)
    g1, g2 = ci.sector_rdms(vecs.reshape(2, -1), b.ncas, b.nelecas)
    d1 = nucgrad.cas_ao_densities(b.mo_coeff, b._n_occ, b.ncas, g1, g2, want_d2=False)[0].reshape(2, 1, b.nao, b.nao)
    wphi, wF = gto.potential_into(b.basis, b.coords_bohr, to_dev(pts / BOHR), d1, True, True)
    print("potential of the one root", phi[:, 0, 0].tolist(), "potential_into of its D1", wphi[:, 0].tolist())
    assert torch.equal(phi[:, 0, 0], wphi[:, 0]) and torch.equal(F[:, 0, 0], wF[:, 0])
    assert torch.equal(b.casci_electrostatic_potential(pts, nroots=1)[1], phi)


def test_errors_of_the_batch_methods():
    pqc, ncas, nelecas = _circuit()
    from auto_oo_amd.gaussian import Moldata_sto3g
    from auto_oo_amd import get_formal_geo
    host = aoo.OO_pqc_batch(pqc, [Moldata_sto3g(get_formal_geo(*POINTS[0]))], ncas, nelecas, oao_mo_coeffs=[np.eye(13)])
    th = torch.zeros((1, host.n_theta), dtype=F64)
    pts = batch_points()
    for call in (lambda: host.electrostatic_potential(th, pts[0]), lambda: host.rhf_electrostatic_potential(pts[0]),
                 lambda: host.casci_electrostatic_potential(pts[0])):
        with pytest.raises(RuntimeError, match="from_geometries"):
            call()
    b = cas_batch("ucc")
    th = seeded_thetas(b)
    for bad in (np.zeros(3), np.zeros((2, 5, 3)), np.zeros((5, 2)), np.zeros((3, 0, 3))):
        with pytest.raises(ValueError, match="points"):
            b.electrostatic_potential(th, bad)
    with pytest.raises(ValueError, match="finite"):
        b.electrostatic_potential(th, np.full((5, 3), np.nan))
    with pytest.raises(ValueError):
        b.electrostatic_potential(th, pts, index=[3])
    with pytest.raises(ValueError):
        b.rhf_electrostatic_potential(pts, result=b.rhf(), index=[0])


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    basis, xyz = C.case("water")
    X = to_dev(C.bohr(xyz))[None]
    r = to_dev(C.bohr(C.cloud(xyz, 4)[1]))[None]
    Dm = to_dev(P.densities("water", 2))[None]
    bad = r.clone()
    bad[0, 2, 1] = float("nan")
    for args in ((X, bad, Dm), (X * float("nan"), r, Dm), (X, r, Dm * float("inf"))):
        with pytest.raises(ValueError, match="finite"):
            gto.potential_into(basis, *args)
    with pytest.raises(ValueError, match="density sets"):
        gto.potential_into(basis, X, r, torch.zeros((1, 11, basis.nao, basis.nao), dtype=F64, device=dev()))
    with pytest.raises(ValueError, match="flags"):
        gto.potential_into(basis, X, r, Dm, nuc=[True])
    # the C entry itself: a negative code and a message, nothing launched, the outputs untouched
    lib = aoo._lib.load()
    t = basis.device_tables(dev())
    work = gto.potential_work(basis, dev(), 1, 2)
    phi = torch.zeros((1, 2, 4), dtype=F64, device=dev())
    F = torch.zeros((1, 2, 4, 3), dtype=F64, device=dev())
    p = aoo._lib.dptr

    def call(batch=1, nset=2, npoint=4, mask=3, dm=Dm, pts=r, out=phi, nshell=basis.nshell):
        return lib.oovqe_gto_potential_batch(nshell, p(t.shells, torch.int32), int(basis.exps.size), p(t.exps), p(t.coefs),
                                             basis.natm, p(t.charges), batch, p(X), basis.nao, nset, p(dm), npoint,
                                             p(pts), ctypes.c_uint(mask), p(out), p(F), p(work), aoo._lib.stream_ptr())
    for kw, text in ((dict(npoint=0), "npoint = 0"), (dict(npoint=65536), "npoint = 65536"), (dict(nset=0), "nset = 0"),
                     (dict(nset=11), "nset = 11"), (dict(batch=65536), "batch = 65536"), (dict(batch=-1), "batch = -1"),
                     (dict(mask=4), "nuc_mask"), (dict(dm=None), "null pointer"), (dict(pts=None), "null pointer"),
                     (dict(out=None), "null pointer"), (dict(nshell=0), "nshell = 0")):
        rc = call(**kw)
        torch.cuda.synchronize()
        assert rc < 0 and text.encode() in lib.oovqe_last_error(), (kw, lib.oovqe_last_error())
        assert not phi.any() and not F.any()
    assert call() == 0
    torch.cuda.synchronize()
    assert phi.abs().min().item() > 0.0
