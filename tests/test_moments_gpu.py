"""Dipole and second-moment integrals and moments on the device (csrc/gto_moments.hip, gto.moment_integrals_batch,
auto_oo_amd/properties.py, OO_pqc_batch.dipole_moment / multipole_moments / rhf_dipole_moment / casci_dipole_matrix).

Bounds, none of them taken from the device: the integrals against the host twin ``TOL_M`` of tests/_moments.py
(measured on the CPU); the contraction ``N^2 max|D| max|M| 4e-16 x 10``; the Hellmann-Feynman check 10 x the
disagreement of the finite difference at h = 1e-3 with itself at h = 2e-3 (floor 1e-9), computed in the test; pinned
RHF dipoles and RHF covariance 1e-8 (first order in the RHF residual of 1e-9); origin independence 1e-12; state and
transition dipoles against host densities contracted with the host twin 1e-10.  Every test prints its figures before it
asserts."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import auto_oo_amd as aoo                                   # noqa: E402
from auto_oo_amd import ci, gto, nucgrad, ops, properties, scf   # noqa: E402
from auto_oo_amd.gaussian import BOHR                       # noqa: E402
from auto_oo_amd.moldata import get_formal_geo              # noqa: E402
from tests import _ci_dense                                 # noqa: E402
from tests import _gto_d as D                               # noqa: E402
from tests import _moments as M                             # noqa: E402

F64 = torch.float64
POINTS = [(140.0, 80.0), (100.0, 0.0), (180.0, 90.0)]       # tests/test_nucgrad_gpu.py
WATER_DIPOLE = (0.05773163, 0.01307932, 0.67102423)         # RHF, atomic units, measured with the host twin and host RHF
M2_DIPOLE = (0.04271543, 0.01091516, 0.49104202)


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def to_dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dev())


def cases(name):
    """(basis, one geometry [natm, 3] in Angstrom)"""
    if name == "h2":
        return M.h2_basis(), M.H2_XYZ
    if name == "hf":
        return M.hf_basis(), M.HF_XYZ
    return D.m1_basis(name.split("-")[1]), D.M1_XYZ


# ---- 1. the integrals element by element ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["h2", "hf", "m1-spherical", "m1-cartesian"])
def test_integrals_against_the_host_twin(name):
    """h2: class ss with a 6-primitive contraction (36 primitive pairs on 8 lanes); hf: ps, pp on two centres; M1: ds, dp,
    dd with repeated shells, both d forms.  Order 2 at the origin of the coordinates and at a non-zero origin; order 1 is
    the head of order 2 bit for bit; every matrix equals its transpose exactly."""
    basis, xyz = cases(name)
    for origin in (None, M.ORIGIN):
        got = gto.moment_integrals_batch(basis, xyz[None], order=2, origin=origin)
        assert tuple(got.shape) == (1, 9, basis.nao, basis.nao)
        want = M.host_moments(basis, xyz, 2, origin)
        err = np.abs(got[0].cpu().numpy() - want).max()
        print(f"{name}, origin {origin is not None}: device against host twin {err:.2e} (TOL_M {M.TOL_M:.2e}), "
              f"largest value {np.abs(want).max():.3g}")
        assert err < M.TOL_M
        assert torch.equal(got, got.transpose(2, 3))
        one = gto.moment_integrals_batch(basis, xyz[None], order=1, origin=origin)
        assert tuple(one.shape) == (1, 3, basis.nao, basis.nao)
        assert torch.equal(one, got[:, :3])


def test_an_origin_per_geometry():
    basis, xyz = cases("m1-spherical")
    stack = np.stack([xyz, D.M1_SHIFTED])
    origins = np.stack([M.ORIGIN, -2.0 * M.ORIGIN])
    got = gto.moment_integrals_batch(basis, stack, order=2, origin=origins).cpu().numpy()
    for g in range(2):
        err = np.abs(got[g] - M.host_moments(basis, stack[g], 2, origins[g])).max()
        print(f"geometry {g} with its own origin: {err:.2e}")
        assert err < M.TOL_M
    # a device tensor [G, 3] and one origin for all are the same thing
    same = gto.moment_integrals_batch(basis, stack, order=2, origin=to_dev(np.stack([M.ORIGIN, M.ORIGIN])))
    assert torch.equal(same, gto.moment_integrals_batch(basis, stack, order=2, origin=M.ORIGIN))


# ---- 2. bits ----------------------------------------------------------------------------------------------------------------
def seeded_densities(N, G=1, nd=3, seed=11):
    d = np.random.default_rng(seed).standard_normal((G, nd, N, N))
    return d + d.transpose(0, 1, 3, 2)


@pytest.mark.parametrize("form", ["spherical", "cartesian"])
def test_a_geometry_has_the_same_bits_alone_permuted_and_on_another_stream(form):
    basis = D.m1_basis(form)
    xyz = to_dev(M.M1_STACK / BOHR)
    dens = to_dev(seeded_densities(basis.nao, 3))
    origin = M.ORIGIN / BOHR

    def both(rows):
        sel = torch.as_tensor(rows, device=dev())
        x, d = xyz[sel].contiguous(), dens[sel].contiguous()
        ints = torch.empty((len(rows), 9, basis.nao, basis.nao), dtype=F64, device=dev())
        gto.moment_integrals_into(basis, x, ints, 2, gto.origin_to_device(origin, len(rows), dev()))
        return ints, properties.multipole_moments(basis, x, d, order=2, origin=origin)

    full_i, full_m = both([0, 1, 2])
    assert not torch.equal(full_i[0], full_i[1]) and not torch.equal(full_m[0], full_m[2])
    for k in range(3):
        i, m = both([k])
        assert torch.equal(i[0], full_i[k]) and torch.equal(m[0], full_m[k]), k
    perm = [2, 0, 1]
    i, m = both(perm)
    assert torch.equal(i, full_i[perm]) and torch.equal(m, full_m[perm])
    side = ops.side_streams(dev())[0]
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        i, m = both([0, 1, 2])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(i, full_i) and torch.equal(m, full_m)


# ---- 3. the contraction ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hf", "m1-cartesian"])
def test_contraction_against_numpy_on_the_integrals_read_back(name):
    basis, xyz = cases(name)
    N = basis.nao
    stack = np.stack([xyz, xyz + D.SHIFT])
    dens = seeded_densities(N, 2)
    o = M.ORIGIN / BOHR
    ints = gto.moment_integrals_batch(basis, stack, order=2, origin=M.ORIGIN).cpu().numpy()
    x = to_dev(stack / BOHR)
    got = properties.multipole_moments(basis, x, to_dev(dens), order=2, origin=o).cpu().numpy()
    assert got.shape == (2, 3, 9)
    nuc = np.stack([M.nuclear_moments(basis.charges, stack[g] / BOHR, 2, o) for g in range(2)])
    want = nuc[:, None, :] - np.einsum("gkpq,gcpq->gkc", dens, ints)
    bound = N * N * np.abs(dens).max() * np.abs(ints).max() * 4e-16 * 10
    err = np.abs(got - want).max()
    print(f"{name}: contraction against numpy {err:.2e} (bound {bound:.2e}), largest moment {np.abs(want).max():.3g}")
    assert err < bound
    # per-density nuclear flags, one density [G, N, N], order 1 = head of order 2
    flags = properties.multipole_moments(basis, x, to_dev(dens), order=2, origin=o, nuclear=[True, False, True])
    assert np.abs(flags.cpu().numpy() - (want - nuc[:, None, :] * np.array([0.0, 1.0, 0.0])[None, :, None])).max() < bound
    single = properties.multipole_moments(basis, x, to_dev(dens[:, 1]), order=1, origin=o)
    assert tuple(single.shape) == (2, 3) and torch.equal(single, to_dev(got)[:, 1, :3])
    # the nuclear part alone: natm terms of magnitude max |Z (R - O)^c| each, added in the order of the atoms
    zero = torch.zeros((2, N, N), dtype=F64, device=dev())
    only = properties.multipole_moments(basis, x, zero, order=2, origin=o).cpu().numpy()
    terms = max(np.abs(M.nuclear_terms(basis.charges, stack[g] / BOHR, 2, o)).max() for g in range(2))
    nbound = basis.natm * terms * 2.3e-16 * 10
    print(f"{name}: nuclear part alone {np.abs(only - nuc).max():.2e} (bound {nbound:.2e})")
    assert np.abs(only - nuc).max() < nbound
    dip, second = properties.split_moments(to_dev(got))
    assert tuple(dip.shape) == (2, 3, 3) and tuple(second.shape) == (2, 3, 3, 3)
    assert torch.equal(second, second.transpose(-1, -2)) and torch.equal(second[..., 1, 2], to_dev(got)[..., 7])


# ---- 4. dipole = -dE/dF (Hellmann-Feynman, RHF): independent of the host twin ---------------------------------------------
def _circuit(kind="np_fabric"):
    if kind == "np_fabric":
        return aoo.Parameterized_circuit(2, 2, None, ansatz="np_fabric", n_layers=1), 2, 2
    if kind == "kupccd":
        return aoo.Parameterized_circuit(6, 6, None, ansatz="kupccd", k=1), 6, 6
    return aoo.Parameterized_circuit(3, 4, None, ansatz="ucc"), 3, 4


def _field_case(name):
    return (gto.GTOBasis(["O", "H", "H"]) if name == "water" else D.m2_basis()), D.WATER


@pytest.mark.parametrize("name", ["water", "m2"])
def test_rhf_dipole_is_minus_the_field_derivative_of_the_energy(name):
    """The test adds F . r (the device moment integrals) to int1e_ao and runs ``scf.rhf_batch`` on all displaced fields
    in one stack: 3 directions x (+-1e-3, +-2e-3, +-4e-3) a.u.  Reference: the 4th-order central difference of
    E_RHF(F) - F . sum Z R at h = 1e-3; bound: 10 x its disagreement with h = 2e-3, at least 1e-9.
    (m2 runs through the d integral kernels of csrc/gto_d.hip.)"""
    basis, xyz = _field_case(name)
    n_occ = basis.nelectron // 2
    ints = gto.integrals_batch(basis, xyz[None])
    r = gto.moment_integrals_batch(basis, xyz[None], order=1)[0]                       # [3, N, N]
    steps = torch.tensor([1e-3, -1e-3, 2e-3, -2e-3, 4e-3, -4e-3], dtype=F64, device=dev())
    h = ints.int1e_ao[0][None, None] + steps[None, :, None, None] * r[:, None]        # [3, 6, N, N]
    K = 18
    N = basis.nao
    res = scf.rhf_batch(h.reshape(K, N, N).contiguous(), ints.int2e_ao.expand(K, N, N, N, N).contiguous(),
                        ints.overlap.expand(K, N, N).contiguous(), n_occ, conv_tol=1e-13, err_tol=1e-10)
    assert bool(res.converged.all())
    e = res.e_elec.reshape(3, 6).cpu().numpy()
    d1 = (8.0 * (e[:, 0] - e[:, 1]) - (e[:, 2] - e[:, 3])) / (12.0 * 1e-3)
    d2 = (8.0 * (e[:, 2] - e[:, 3]) - (e[:, 4] - e[:, 5])) / (12.0 * 2e-3)
    nuc = M.nuclear_moments(basis.charges, xyz / BOHR, 1)
    ref = nuc - d1                       # -d/dF [E_elec(F) - F . sum Z R]
    dis = np.abs(d1 - d2).max()
    bound = max(10 * dis, 1e-9)
    zero = scf.rhf_batch(ints.int1e_ao, ints.int2e_ao, ints.overlap, n_occ, conv_tol=1e-13, err_tol=1e-11)
    assert bool(zero.converged.all())
    dens = nucgrad.cas_ao_densities(zero.mo_coeff, n_occ, 0, want_d2=False)[0]
    mu = properties.multipole_moments(basis, to_dev(xyz[None] / BOHR), dens, order=1)[0].cpu().numpy()
    err = np.abs(mu - ref).max()
    print(f"{name}: mu = {mu} a.u., |mu| = {np.linalg.norm(mu) * properties.DEBYE:.4f} D; -dE/dF {ref}; reference "
          f"disagreement {dis:.2e}, bound {bound:.2e}, error {err:.2e}")
    assert err < bound


@pytest.mark.parametrize("name", ["water", "m2"])
def test_rhf_dipole_moment_reproduces_the_pinned_dipoles(name):
    basis, xyz = _field_case(name)
    pqc, ncas, nelecas = _circuit()
    b = aoo.OO_pqc_batch.from_geometries(pqc, basis, xyz[None], ncas, nelecas, oao_mo_coeffs="rhf")
    mu = b.rhf_dipole_moment()
    want = np.array(WATER_DIPOLE if name == "water" else M2_DIPOLE)
    err = np.abs(mu[0].cpu().numpy() - want).max()
    print(f"{name}: rhf_dipole_moment {mu[0].tolist()}, |mu| = {mu[0].norm().item() * properties.DEBYE:.4f} D, "
          f"against the pinned value {err:.2e}")
    assert tuple(mu.shape) == (1, 3)
    assert err < 1e-8


# ---- 5. physics of the public calls -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def formal_basis():
    return gto.GTOBasis(["N", "C", "H", "H", "H"])


def formal_coords(points):
    return formal_basis().coordinates([get_formal_geo(*p) for p in points])          # Angstrom


@functools.lru_cache(maxsize=None)
def rotated_orbitals():
    """RHF orbitals of the three POINTS times expm of a seeded skew matrix of norm 0.1 (tests/test_nucgrad_gpu.py)"""
    pqc, ncas, nelecas = _circuit()
    b = aoo.OO_pqc_batch.from_geometries(pqc, formal_basis(), formal_coords(POINTS), ncas, nelecas, oao_mo_coeffs="rhf")
    rng = np.random.default_rng(17)
    out = []
    for U in b.oao_mo_coeff.cpu().numpy():
        K = rng.standard_normal(U.shape)
        K = K - K.T
        K *= 0.1 / np.linalg.norm(K)
        out.append(U @ torch.linalg.matrix_exp(torch.as_tensor(K)).numpy())
    return out


@functools.lru_cache(maxsize=None)
def cas_batch(kind, G=3):
    pqc, ncas, nelecas = _circuit(kind)
    return aoo.OO_pqc_batch.from_geometries(pqc, formal_basis(), formal_coords(POINTS[:G]), ncas, nelecas,
                                            oao_mo_coeffs=rotated_orbitals()[:G])


def seeded_thetas(batch, seed=5):
    return to_dev(np.random.default_rng(seed).uniform(-0.6, 0.6, (batch.G, batch.n_theta)))


@functools.lru_cache(maxsize=None)
def formal_twin(g, order=1):
    return M.host_moments(formal_basis(), formal_coords(POINTS)[g], order)


def host_dipole(g, d1):
    xyz = formal_coords(POINTS)[g] / BOHR
    return M.nuclear_moments(formal_basis().charges, xyz, 1) - np.einsum("pq,cpq->c", d1, formal_twin(g))


@pytest.mark.parametrize("form", ["spherical", "cartesian"])
def test_rhf_dipole_turns_with_the_molecule(form):
    """Converged RHF is covariant: the dipole of M1 rotated and translated is the rotated dipole of M1 (a neutral
    molecule: the translation drops out)."""
    pqc, ncas, nelecas = _circuit()
    b = aoo.OO_pqc_batch.from_geometries(pqc, D.m1_basis(form), np.stack([D.M1_XYZ, D.M1_MOVED]), ncas, nelecas,
                                         oao_mo_coeffs="rhf")
    mu = b.rhf_dipole_moment(b.rhf(conv_tol=1e-13, err_tol=1e-11)).cpu().numpy()
    err = np.abs(mu[1] - D.ROTATION @ mu[0]).max()
    print(f"M1 {form}: mu = {mu[0]}, moved {mu[1]}, |moved - R mu| = {err:.2e}")
    assert np.abs(mu[0]).max() > 0.1
    assert err < 1e-8
    one = b.rhf_dipole_moment(index=1)
    assert tuple(one.shape) == (1, 3) and np.abs(one[0].cpu().numpy() - mu[1]).max() < 1e-8


def test_origin_independence_and_the_shift_of_the_second_moments():
    b = cas_batch("ucc")
    th = seeded_thetas(b)
    mu = b.dipole_moment(th)
    O = M.ORIGIN
    err = (b.dipole_moment(th, origin=O) - mu).abs().max().item()
    print(f"dipole of a neutral molecule at another origin: {err:.2e}")
    assert err < 1e-12
    per = np.stack([O, -O, 3.0 * O])
    assert (b.dipole_moment(th, origin=per) - mu).abs().max().item() < 1e-12
    dip0, q0 = b.multipole_moments(th, order=2)
    dipo, qo = b.multipole_moments(th, order=2, origin=O)
    assert tuple(dip0.shape) == (3, 3) and tuple(q0.shape) == (3, 3, 3) and torch.equal(dip0, mu)
    ob = to_dev(O / BOHR)
    # Q(O)_ij = Q(0)_ij - O_i mu_j - O_j mu_i + O_i O_j (total charge = 0).  Nuclear and electronic parts of up to 1e2
    # cancel; each is a sum of N^2 = 169 products rounded to 1.1e-16 relative: 1e2 x 169 x 1.1e-16 x 10 = 1.9e-11
    want = q0 - ob[None, :, None] * mu[:, None, :] - ob[None, None, :] * mu[:, :, None]
    err = (qo - want).abs().max().item()
    print(f"shift identity of the second moments: {err:.2e}, largest second moment {q0.abs().max().item():.3g}")
    assert err < 1.9e-11
    theta_q = properties.traceless_quadrupole(q0)
    assert theta_q.diagonal(dim1=-2, dim2=-1).sum(-1).abs().max().item() < 1e-12
    assert torch.equal(b.dipole_moment(th, index=[2, 0]), mu[[2, 0]])


@pytest.mark.parametrize("kind", ["ucc", "np_fabric"])
def test_dipole_moment_of_a_circuit_state_against_host_densities(kind):
    b = cas_batch(kind)
    th = seeded_thetas(b)
    pqc = b.pqc
    gamma, Gamma = ops.circuit_rdms(th, pqc._gates_dev, pqc._n_gates, pqc.n_qubits, b.ncas, pqc._init_index,
                                    tangents=False)
    mu = b.dipole_moment(th).cpu().numpy()
    assert mu.shape == (3, 3)
    for g in range(3):
        d1, _ = nucgrad.cas_ao_densities_host(b.mo_coeff[g].cpu().numpy(), b._n_occ, b.ncas, gamma[g, 0].cpu().numpy(),
                                              Gamma[g, 0].cpu().numpy())
        err = np.abs(mu[g] - host_dipole(g, d1)).max()
        print(f"{kind}, geometry {g}: mu = {mu[g]}, against host D1 and host integrals {err:.2e}")
        assert err < 1e-10


def test_dipole_moment_of_a_sector_engine_circuit():
    """kUpCCD CAS(6e,6o) (12 qubits: the sector engine) on formaldimine at G = 2, the RDMs read back from the circuit
    object."""
    b = cas_batch("kupccd", 2)
    assert b.pqc._use_sector
    th = seeded_thetas(b)
    mu = b.dipole_moment(th).cpu().numpy()
    g1, g2 = b.pqc._sector.rdms(b.pqc._sector.state(th))
    for g in range(2):
        d1, _ = nucgrad.cas_ao_densities_host(b.mo_coeff[g].cpu().numpy(), b._n_occ, b.ncas, g1[g].cpu().numpy(),
                                              g2[g].cpu().numpy())
        err = np.abs(mu[g] - host_dipole(g, d1)).max()
        print(f"kUpCCD, geometry {g}: mu = {mu[g]}, against host D1 and host integrals {err:.2e}")
        assert err < 1e-10


# ---- 6. state and transition dipoles of CASCI ---------------------------------------------------------------------------
def test_casci_dipole_matrix():
    b = cas_batch("ucc", 2)
    a, ne, R = b.ncas, b.nelecas, 3
    e, dip = b.casci_dipole_matrix(nroots=R)
    e0, vecs = b.casci(nroots=R)
    assert tuple(dip.shape) == (2, R, R, 3)
    print("CASCI energies", e.tolist(), "difference to casci()", (e - e0).abs().max().item())
    assert (e - e0).abs().max().item() < 1e-12
    assert torch.equal(dip, dip.transpose(1, 2))
    # the diagonal: each root's own D1
    g1, g2 = ci.sector_rdms(vecs.reshape(2 * R, -1), a, ne)
    C = b.mo_coeff[:, None].expand(2, R, b.nao, b.nao).reshape(2 * R, b.nao, b.nao)
    d1 = nucgrad.cas_ao_densities(C, b._n_occ, a, g1, g2, want_d2=False)[0].reshape(2, R, b.nao, b.nao)
    diag = properties.multipole_moments(b.basis, b.coords_bohr, d1, order=1)
    k = torch.arange(R, device=dev())
    err = (dip[:, k, k] - diag).abs().max().item()
    print(f"state dipoles against multipole_moments of each root's D1: {err:.2e}")
    assert err < 1e-12
    # the off-diagonal: -tr(C_a gamma^IJ C_a^T r), gamma^IJ = c_I^T E_pq c_J symmetrised, from the dense E_pq
    E = _ci_dense.excitation_matrices(a, ne)
    c = vecs.cpu().numpy()
    worst = 0.0
    for g in range(2):
        Ca = b.mo_coeff[g].cpu().numpy()[:, b._n_occ:b._n_occ + a]
        for i in range(R):
            for j in range(i):
                gam = np.einsum("x,pqxy,y->pq", c[g, i], E, c[g, j])
                gam = 0.5 * (gam + gam.T)
                want = -np.einsum("pq,cpq->c", Ca @ gam @ Ca.T, formal_twin(g))
                worst = max(worst, np.abs(dip[g, i, j].cpu().numpy() - want).max())
    print(f"transition dipoles against the dense excitation matrices: {worst:.2e}, largest "
          f"{dip[:, 1, 0].abs().max().item():.3g}")
    assert worst < 1e-10
    assert dip[:, 1, 0].abs().max().item() > 1e-3 or dip[:, 2, 0].abs().max().item() > 1e-3


def test_casci_dipole_matrix_of_one_root():
    """``nroots=1``: no pair, the matrix is the one root's dipole -- the same library call on the same ``D1``, so the same
    bits."""
    b = cas_batch("ucc", 2)
    e, dip = b.casci_dipole_matrix(nroots=1)
    e0, vecs = b.casci(nroots=1)
    assert tuple(e.shape) == (2, 1) and tuple(dip.shape) == (2, 1, 1, 3)
    assert torch.equal(e, e0)
    g1, g2 = ci.sector_rdms(vecs.reshape(2, -1), b.ncas, b.nelecas)
    d1 = nucgrad.cas_ao_densities(b.mo_coeff, b._n_occ, b.ncas, g1, g2, want_d2=False)[0].reshape(2, 1, b.nao, b.nao)
    want = properties.multipole_moments(b.basis, b.coords_bohr, d1, order=1)
    print("dipole of the one root", dip[:, 0, 0].tolist(), "multipole_moments of its D1", want[:, 0].tolist())
    assert torch.equal(dip[:, 0, 0], want[:, 0])


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------
def test_errors():
    pqc, ncas, nelecas = _circuit()
    from auto_oo_amd.gaussian import Moldata_sto3g
    host = aoo.OO_pqc_batch(pqc, [Moldata_sto3g(get_formal_geo(*POINTS[0]))], ncas, nelecas, oao_mo_coeffs=[np.eye(13)])
    th = torch.zeros((1, host.n_theta), dtype=F64)
    for call in (lambda: host.dipole_moment(th), lambda: host.multipole_moments(th), host.rhf_dipole_moment,
                 host.casci_dipole_matrix):
        with pytest.raises(RuntimeError, match="from_geometries"):
            call()
    b = cas_batch("ucc")
    th = seeded_thetas(b)
    for origin in (np.zeros(2), np.zeros((2, 3)), np.zeros((3, 3, 1))):
        with pytest.raises(ValueError, match="origin"):
            b.dipole_moment(th, origin=origin)
        with pytest.raises(ValueError, match="origin"):
            gto.moment_integrals_batch(formal_basis(), formal_coords(POINTS), origin=origin)
    with pytest.raises(ValueError, match="order = 3"):
        b.multipole_moments(th, order=3)
    with pytest.raises(ValueError, match="order = 3"):
        gto.moment_integrals_batch(formal_basis(), formal_coords(POINTS), order=3)
    with pytest.raises(ValueError, match="order = 3"):
        properties.multipole_moments(formal_basis(), b.coords_bohr, b.mo_coeff, order=3)
    with pytest.raises(ValueError):
        b.dipole_moment(th, index=[3])
    with pytest.raises(ValueError):
        properties.multipole_moments(formal_basis(), b.coords_bohr, b.mo_coeff[:2])
