"""Analytic nuclear gradients on the device (csrc/gto_grad.hip, auto_oo_amd/nucgrad.py, gto.gradient_batch,
OO_pqc_batch.nuclear_gradient / rhf_nuclear_gradient) against finite differences of the entry points that existed
before them (gto.integrals_into, OO_pqc_batch.from_geometries + energy, OO_pqc_batch.rhf).

The reference everywhere is the 4th-order central difference (8 (f(+h) - f(-h)) - (f(+2h) - f(-2h))) / 12h with
h = 1e-3 Bohr, all 4 * 3 * natm displaced copies in one stack.  The same difference is made with h = 2e-3; the largest
disagreement of the two is what the reference can be trusted to, and every bound below is 10 x that figure of the
very case and term under test (the factor covers the order of summation, as in tests/test_gto_gpu.py).  Nothing in a
bound comes from the analytic code.  The figures are printed by every test before it asserts.

Measured on an MI355X: disagreement of the reference at h = 2e-3 with itself at h = 1e-3 (the bound is 10 x that) and,
after the slash, the largest error of the analytic gradient against the reference at h = 1e-3:

    raw contraction   D1 . dh            WQ . dS            1/2 D2 . dg        nuclear            all together
    H2 (6 prim.)      3.3e-12 / 9.8e-14  1.7e-12 / 7.2e-13  2.1e-11 / 3.5e-12  7.6e-13 / 5.2e-14  1.7e-11 / 3.5e-12
    H-F               1.0e-11 / 6.7e-12  1.8e-12 / 7.0e-13  3.0e-11 / 7.9e-12  6.6e-12 / 7.9e-13  4.1e-11 / 7.8e-12
    water             5.5e-11 / 1.3e-11  2.5e-12 / 9.7e-13  5.7e-11 / 1.1e-11  6.1e-12 / 1.4e-12  6.8e-11 / 2.2e-11
    formaldimine      4.0e-11 / 2.0e-11  4.8e-12 / 1.9e-12  7.6e-11 / 8.7e-12  1.3e-11 / 4.3e-12  1.0e-10 / 2.2e-11

(largest gradient components 2.4 ... 35; the water row reproduces the host figures 5.9e-11, 2.5e-12, 5.7e-11, 6.1e-12 the
feature was specified with.)  The whole differs from the sum of its parts by at most 7.1e-15.

    energy gradients (formaldimine, three points)        disagreement / error
    nuclear_gradient, np_fabric CAS(2,2), rotated U      1.0e-10 / 7.5e-11     torque - dE/dphi: 1.0e-10 / 1.1e-10
    nuclear_gradient, ucc CAS(4e,3o), rotated U          1.3e-10 / 8.3e-11     torque - dE/dphi: 9.8e-11 / 9.1e-11
    rhf_nuclear_gradient, water                          1.1e-10 / 7.8e-11
    rhf_nuclear_gradient, formaldimine (140, 80)         6.6e-11 / 1.0e-10     (2.6e-10 with orbitals converged to 1e-9 only)
    nuclear_gradient(theta = 0) - rhf_nuclear_gradient   9.9e-11               torque there 3.7e-10; 3.6e-2 at the rotated U

Every figure is below the thresholds (1e-9 raw, 1e-8 energies) beyond which the step would have to be reconsidered.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import auto_oo_amd as aoo                                   # noqa: E402
from auto_oo_amd import gto, nucgrad, ops                   # noqa: E402
from auto_oo_amd.gaussian import BOHR                       # noqa: E402
from auto_oo_amd.moldata import get_formal_geo              # noqa: E402

F64 = torch.float64
H1, H2 = 1e-3, 2e-3
POINTS = [(140.0, 80.0), (100.0, 0.0), (180.0, 90.0)]       # tests/test_gto_gpu.py
WATER = np.array([[0.0, 0.01, 0.02], [0.3, 0.75, 0.55], [-0.2, -0.70, 0.62]])
TERMS = ("dm1", "wq", "dm2", "nuc")


def dev():
    return torch.device("cuda", torch.cuda.current_device())


@functools.lru_cache(maxsize=None)
def case(name):
    """(basis, coordinates [natm, 3] in Bohr as a host array)"""
    if name == "h2":
        # one 1-primitive and one 6-primitive s shell per atom (36 primitive pairs are no multiple of 8; MAX_PRIM = 10
        # is reached in tests/test_gto_edges_gpu.py)
        table = {"H": [(0, [0.6], [1.0]),
                       (0, [30.0, 8.0, 2.5, 0.9, 0.35, 0.12], [0.02, 0.08, 0.25, 0.4, 0.3, 0.1])]}
        basis = gto.GTOBasis(["H", "H"], table)
        xyz = np.array([[0.1, 0.2, 0.3], [0.55, -0.35, 0.8]])
    elif name == "hf":
        basis = gto.GTOBasis(["H", "F"])
        xyz = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.1]])
    elif name == "water":
        basis = gto.GTOBasis(["O", "H", "H"])
        xyz = WATER
    else:
        basis = formal_basis()
        xyz = basis.coordinates([get_formal_geo(*POINTS[0])])[0]
    return basis, xyz / BOHR


@functools.lru_cache(maxsize=None)
def formal_basis():
    return gto.GTOBasis(["N", "C", "H", "H", "H"])


def fd_stack(xyz, h):
    """[natm, 3] (Bohr, host) -> [4 * 3 * natm, natm, 3]: per coordinate +h, -h, +2h, -2h."""
    natm = xyz.shape[0]
    out = np.repeat(xyz[None], 12 * natm, axis=0)
    for a in range(natm):
        for d in range(3):
            for k, s in enumerate((1.0, -1.0, 2.0, -2.0)):
                out[(a * 3 + d) * 4 + k, a, d] += s * h
    return out


def fd_combine(f, h):
    """f [..., 4 * 3 * natm] of the stack above -> [..., natm, 3]"""
    f = f.reshape(f.shape[:-1] + (-1, 3, 4))
    return (8.0 * (f[..., 0] - f[..., 1]) - (f[..., 2] - f[..., 3])) / (12.0 * h)


@functools.lru_cache(maxsize=None)
def densities(name):
    """seeded standard-normal D1, WQ, D2, symmetrised by adding their transposes"""
    basis, _ = case(name)
    N = basis.nao
    rng = np.random.default_rng(0)
    d1, wq, d2 = rng.standard_normal((N, N)), rng.standard_normal((N, N)), rng.standard_normal((N,) * 4)
    d1, wq = d1 + d1.T, wq + wq.T
    d2 = d2 + d2.transpose(1, 0, 2, 3)
    d2 = d2 + d2.transpose(0, 1, 3, 2)
    d2 = d2 + d2.transpose(2, 3, 0, 1)
    return tuple(torch.as_tensor(x).to(dev())[None].contiguous() for x in (d1, wq, d2))


def term_values(name, coords_bohr):
    """The four contractions D1 . h, WQ . S, 1/2 D2 . g, E_nuc of every geometry of a stack -> [4, G] (device)."""
    basis, _ = case(name)
    d1, wq, d2 = densities(name)
    xyz = torch.as_tensor(coords_bohr).to(dev()).contiguous()
    G, N = int(xyz.shape[0]), basis.nao
    S = torch.empty((G, N, N), dtype=F64, device=dev())
    h = torch.empty_like(S)
    g = torch.empty((G,) + (N,) * 4, dtype=F64, device=dev())
    nuc = torch.empty(G, dtype=F64, device=dev())
    gto.integrals_into(basis, xyz, S, h, g, nuc)
    return torch.stack(((h * d1).sum(dim=(1, 2)), (S * wq).sum(dim=(1, 2)), 0.5 * (g * d2).sum(dim=(1, 2, 3, 4)), nuc))


@functools.lru_cache(maxsize=None)
def raw_reference(name):
    """-> (finite-difference gradients of the four terms [4, natm, 3] at h = 1e-3, their disagreement with h = 2e-3 per
    term [4], the same for the sum) as host arrays"""
    _, xyz = case(name)
    a = fd_combine(term_values(name, fd_stack(xyz, H1)), H1).cpu().numpy()
    b = fd_combine(term_values(name, fd_stack(xyz, H2)), H2).cpu().numpy()
    return a, np.abs(a - b).reshape(4, -1).max(axis=1), np.abs(a.sum(axis=0) - b.sum(axis=0)).max()


def analytic(name, which, coords_bohr=None):
    basis, xyz = case(name)
    d1, wq, d2 = densities(name)
    x = torch.as_tensor(xyz if coords_bohr is None else coords_bohr).to(dev())
    x = x[None] if x.dim() == 2 else x
    G = int(x.shape[0])
    ex = lambda t: t.expand((G,) + tuple(t.shape[1:])).contiguous()            # noqa: E731
    return gto.gradient_into(basis, x.contiguous(), ex(d1) if "dm1" in which else None,
                             ex(wq) if "wq" in which else None, ex(d2) if "dm2" in which else None, "nuc" in which)


# ---- 1. the raw contraction ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["h2", "hf", "water", "formaldimine"])
def test_raw_contraction_term_by_term_and_together(name):
    """Every term alone (the others null) and all together against the finite-difference reference, each within 10 x
    the disagreement of the reference's two step sizes for that term; the parts add up to the whole to 1e-12.
    h2: 6 primitives, 36 primitive pairs on 8 lanes; hf: every pair and quartet class on two centres; water:
    three centres; formaldimine: four."""
    ref, dis, dis_all = raw_reference(name)
    parts = []
    for k, term in enumerate(TERMS):
        got = analytic(name, (term,))[0].cpu().numpy()
        parts.append(got)
        err = np.abs(got - ref[k]).max()
        print(f"{name} {term}: max |grad| {np.abs(ref[k]).max():.3g}, reference disagreement {dis[k]:.2e}, "
              f"bound {10 * dis[k]:.2e}, error {err:.2e}")
        assert err < 10 * dis[k], (name, term, err, dis[k])
    whole = analytic(name, TERMS)[0].cpu().numpy()
    err = np.abs(whole - ref.sum(axis=0)).max()
    split = np.abs(whole - sum(parts)).max()
    print(f"{name} all: reference disagreement {dis_all:.2e}, bound {10 * dis_all:.2e}, error {err:.2e}; "
          f"whole - sum of parts {split:.2e}")
    assert err < 10 * dis_all
    assert split < 1e-12


# ---- 2. structure -------------------------------------------------------------------------------------------------------
def five_geometries():
    basis = formal_basis()
    pts = POINTS + [(120.0, 40.0), (160.0, 60.0)]
    return basis.coordinates([get_formal_geo(*p) for p in pts]) / BOHR


def test_translation_sum_vanishes():
    g = analytic("formaldimine", TERMS)[0]
    s = g.sum(dim=0).abs().max().item()
    print("sum over atoms of the formaldimine gradient:", s, "largest component", g.abs().max().item())
    assert s < 1e-10


def test_a_permuted_stack_gives_the_permuted_result_and_a_geometry_alone_the_same_bits():
    xyz = five_geometries()
    full = analytic("formaldimine", TERMS, xyz)
    perm = [3, 0, 4, 2, 1]
    assert torch.equal(analytic("formaldimine", TERMS, xyz[perm]), full[perm])
    for k in range(5):
        assert torch.equal(analytic("formaldimine", TERMS, xyz[k:k + 1])[0], full[k]), k
    assert not torch.equal(full[0], full[1])


def test_a_call_on_another_stream_gives_the_same_bits():
    xyz = five_geometries()
    full = analytic("formaldimine", TERMS, xyz)
    side = ops.side_streams(dev())[0]
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = analytic("formaldimine", TERMS, xyz)          # (the basis keeps one work buffer per stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    basis = formal_basis()
    assert len([k for k in basis._work if k[0] == "gradient"]) >= 2
    assert torch.equal(full, other)


# ---- 3. AO densities ----------------------------------------------------------------------------------------------------
def circuit(kind):
    if kind == "np_fabric":
        return aoo.Parameterized_circuit(2, 2, None, ansatz="np_fabric", n_layers=1), 2, 2
    return aoo.Parameterized_circuit(3, 4, None, ansatz="ucc"), 3, 4


def formal_coords(points):
    return formal_basis().coordinates([get_formal_geo(*p) for p in points])          # Angstrom


@functools.lru_cache(maxsize=None)
def rhf_oao_orbitals():
    """OAO -> MO coefficients of device RHF at the three POINTS (host array [3, N, N])"""
    pqc, ncas, nelecas = circuit("np_fabric")
    b = aoo.OO_pqc_batch.from_geometries(pqc, formal_basis(), formal_coords(POINTS), ncas, nelecas,
                                         oao_mo_coeffs="rhf")
    return b.oao_mo_coeff.cpu().numpy()


@functools.lru_cache(maxsize=None)
def rotated_orbitals():
    """the RHF orbitals of each point times expm of a seeded skew matrix of norm 0.1: far from stationary"""
    rng = np.random.default_rng(17)
    out = []
    for U in rhf_oao_orbitals():
        K = rng.standard_normal(U.shape)
        K = K - K.T
        K *= 0.1 / np.linalg.norm(K)
        out.append(U @ torch.linalg.matrix_exp(torch.as_tensor(K)).numpy())
    return out


def seeded_thetas(batch, G, seed=5):
    return torch.as_tensor(np.random.default_rng(seed).uniform(-0.6, 0.6, (G, batch.n_theta))).to(dev())


@functools.lru_cache(maxsize=None)
def cas_batch(kind):
    pqc, ncas, nelecas = circuit(kind)
    return aoo.OO_pqc_batch.from_geometries(pqc, formal_basis(), formal_coords(POINTS), ncas, nelecas,
                                            oao_mo_coeffs=rotated_orbitals())


def _assert_sym8(d2):
    assert torch.equal(d2, d2.permute(0, 2, 1, 3, 4)) and torch.equal(d2, d2.permute(0, 1, 2, 4, 3))
    assert torch.equal(d2, d2.permute(0, 3, 4, 1, 2))


@pytest.mark.parametrize("kind", ["np_fabric", "ucc"])
def test_ao_densities_reproduce_the_energy_of_the_batch(kind):
    b = cas_batch(kind)
    th = seeded_thetas(b, b.G)
    pqc = b.pqc
    gamma, Gamma = ops.circuit_rdms(th, pqc._gates_dev, pqc._n_gates, pqc.n_qubits, b.ncas, pqc._init_index,
                                    tangents=False)
    d1, d2 = nucgrad.cas_ao_densities(b.mo_coeff, b._n_occ, b.ncas, gamma[:, 0], Gamma[:, 0])
    e = (d1 * b.int1e_ao).sum(dim=(1, 2)) + 0.5 * (d2 * b.int2e_ao).sum(dim=(1, 2, 3, 4)) + b.nuc
    err = (e - b.energy(th)).abs().max().item()
    print(f"{kind}: |D1 . h + 1/2 D2 . g + nuc - E| = {err:.2e}")
    assert err < 1e-10
    _assert_sym8(d2)
    assert torch.equal(d1, d1.transpose(1, 2))
    # against the numpy twin written from the definition
    t1, t2 = nucgrad.cas_ao_densities_host(b.mo_coeff[1].cpu().numpy(), b._n_occ, b.ncas, gamma[1, 0].cpu().numpy(),
                                           Gamma[1, 0].cpu().numpy())
    assert np.abs(d1[1].cpu().numpy() - t1).max() < 1e-12 and np.abs(d2[1].cpu().numpy() - t2).max() < 1e-12


def test_ao_densities_closed_shell():
    b = cas_batch("np_fabric")
    n_occ = b.nelectron // 2
    d1, d2 = nucgrad.cas_ao_densities(b.mo_coeff, n_occ, 0)
    Co = b.mo_coeff[:, :, :n_occ]
    D = 2.0 * Co @ Co.transpose(1, 2)
    ref = torch.einsum("gpq,grs->gpqrs", D, D) - 0.5 * torch.einsum("gpr,gqs->gpqrs", D, D)
    ref = 0.5 * (ref + ref.permute(0, 2, 1, 3, 4))
    ref = 0.5 * (ref + ref.permute(0, 1, 2, 4, 3))
    ref = 0.5 * (ref + ref.permute(0, 3, 4, 1, 2))
    print("closed shell:", (d1 - D).abs().max().item(), (d2 - ref).abs().max().item())
    assert (d1 - D).abs().max().item() < 1e-13 and (d2 - ref).abs().max().item() < 1e-12
    _assert_sym8(d2)


# ---- 4. the energy gradient away from any stationary point ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def energy_reference(kind):
    """finite differences of the batch energy at fixed theta and fixed U -> ([3, natm, 3] at h = 1e-3, disagreement
    with h = 2e-3)"""
    pqc, ncas, nelecas = circuit(kind)
    b0 = cas_batch(kind)
    th = seeded_thetas(b0, 3)
    xyz = formal_coords(POINTS) / BOHR
    natm = xyz.shape[1]
    res = []
    for h in (H1, H2):
        stack = np.concatenate([fd_stack(xyz[k], h) for k in range(3)])
        U = [rotated_orbitals()[k] for k in range(3) for _ in range(12 * natm)]
        b = aoo.OO_pqc_batch.from_geometries(pqc, formal_basis(), stack * BOHR, ncas, nelecas, oao_mo_coeffs=U)
        e = b.energy(th.repeat_interleave(12 * natm, dim=0))
        res.append(fd_combine(e.reshape(3, -1), h).cpu().numpy())
    return res[0], np.abs(res[0] - res[1]).max()


def rotation_stack(xyz, h):
    """[natm, 3] -> [12, natm, 3]: the molecule turned about x, y, z by +h, -h, +2h, -2h (radians)"""
    out = []
    for k in range(3):
        i, j = (k + 1) % 3, (k + 2) % 3
        for s in (1.0, -1.0, 2.0, -2.0):
            R = np.eye(3)
            c, sn = np.cos(s * h), np.sin(s * h)
            R[i, i], R[i, j], R[j, i], R[j, j] = c, -sn, sn, c
            out.append(xyz @ R.T)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def rotation_reference(kind):
    """dE/dphi about the three axes through the origin at fixed theta and fixed U, by the same finite difference in
    the angle -> ([3 points, 3 axes], disagreement of the two steps)"""
    pqc, ncas, nelecas = circuit(kind)
    th = seeded_thetas(cas_batch(kind), 3)
    xyz = formal_coords(POINTS) / BOHR
    res = []
    for h in (H1, H2):
        stack = np.concatenate([rotation_stack(xyz[k], h) for k in range(3)])
        U = [rotated_orbitals()[k] for k in range(3) for _ in range(12)]
        b = aoo.OO_pqc_batch.from_geometries(pqc, formal_basis(), stack * BOHR, ncas, nelecas, oao_mo_coeffs=U)
        e = b.energy(th.repeat_interleave(12, dim=0)).reshape(3, 3, 4)
        res.append(((8.0 * (e[..., 0] - e[..., 1]) - (e[..., 2] - e[..., 3])) / (12.0 * h)).cpu().numpy())
    return res[0], np.abs(res[0] - res[1]).max()


@pytest.mark.parametrize("kind", ["np_fabric", "ucc"])
def test_nuclear_gradient_away_from_stationary_points(kind):
    """formaldimine at the three POINTS, seeded thetas, orbitals rotated away from RHF (the pull-back through S^-1/2
    is exercised): against the finite difference of the energy with the same U and theta in every displaced copy;
    index= and chunk=1 give the same bits; the net force vanishes.

    Rotations: at FIXED OAO-to-MO coefficients U the energy is not invariant under a rigid rotation of the nuclei
    unless the orbital gradient vanishes -- the p functions keep the axes of the laboratory, so turning the molecule
    under a fixed U is an orbital rotation by the p-block of the rotation matrix.  The torque sum_A R_A x grad_A of
    the true energy gradient is therefore compared with what it must equal, dE/dphi of a rigid rotation about each
    axis (the same finite difference, in the angle), instead of with zero; where the orbital gradient vanishes it is
    compared with zero (test_general_route_reduces_to_the_rhf_route_at_the_hartree_fock_determinant)."""
    b = cas_batch(kind)
    th = seeded_thetas(b, 3)
    ref, dis = energy_reference(kind)
    grad = b.nuclear_gradient(th)
    err = np.abs(grad.cpu().numpy() - ref).max()
    print(f"{kind}: max |grad| {np.abs(ref).max():.3g}, reference disagreement {dis:.2e}, bound {10 * dis:.2e}, "
          f"error {err:.2e}")
    assert tuple(grad.shape) == (3, 5, 3)
    assert err < 10 * dis
    assert torch.equal(b.nuclear_gradient(th, chunk=1), grad)
    assert torch.equal(b.nuclear_gradient(th, index=[2, 0]), grad[[2, 0]])
    assert torch.equal(b.nuclear_gradient(th, index=1), grad[1:2])
    net = grad.sum(dim=1).abs().max().item()
    xyz = torch.as_tensor(formal_coords(POINTS) / BOHR).to(dev())
    torque = torch.cross(xyz, grad, dim=2).sum(dim=1).cpu().numpy()
    rot, rdis = rotation_reference(kind)
    terr = np.abs(torque - rot).max()
    print(f"{kind}: net force {net:.2e}; torque up to {np.abs(torque).max():.2e}, dE/dphi by finite differences "
          f"disagrees with itself by {rdis:.2e}, bound {10 * rdis:.2e}, torque - dE/dphi {terr:.2e}")
    assert net < 10 * dis
    assert terr < 10 * rdis


# ---- 5. the stationary case and the two public routes ------------------------------------------------------------------------
def rhf_case(name):
    if name == "water":
        basis, xyz = case("water")
    else:
        basis, xyz = case("formaldimine")
    return basis, xyz


@pytest.mark.parametrize("name", ["water", "formaldimine"])
def test_rhf_nuclear_gradient_against_converged_rhf_energies(name):
    basis, xyz = rhf_case(name)
    pqc, ncas, nelecas = circuit("np_fabric")
    eye = np.eye(basis.nao)
    natm = xyz.shape[0]
    res = []
    for h in (H1, H2):
        stack = fd_stack(xyz, h)
        b = aoo.OO_pqc_batch.from_geometries(pqc, basis, stack * BOHR, ncas, nelecas, oao_mo_coeffs=[eye] * len(stack))
        r = b.rhf(conv_tol=1e-13)
        assert bool(r.converged.all())
        res.append(fd_combine(r.e_tot, h).cpu().numpy())
    dis = np.abs(res[0] - res[1]).max()
    b = aoo.OO_pqc_batch.from_geometries(pqc, basis, xyz[None] * BOHR, ncas, nelecas, oao_mo_coeffs="rhf")
    # (the analytic formula takes the orbitals as stationary, so its error is of FIRST order in what is left of the
    # commutator F D S - S D F, where the energies above are of second order: converged to 1e-11 here, not the default 1e-9)
    r = b.rhf(conv_tol=1e-13, err_tol=1e-11)
    assert bool(r.converged.all())
    grad = b.rhf_nuclear_gradient(r)
    err = np.abs(grad[0].cpu().numpy() - res[0]).max()
    print(f"RHF {name}: max |grad| {np.abs(res[0]).max():.3g}, reference disagreement {dis:.2e}, "
          f"bound {10 * dis:.2e}, error {err:.2e}")
    assert tuple(grad.shape) == (1, natm, 3)
    assert err < 10 * dis
    assert (b.rhf_nuclear_gradient() - grad).abs().max().item() < 1e-9        # (its own RHF run, default tolerances)


@pytest.mark.parametrize("kind", ["np_fabric", "ucc"])
def test_general_route_reduces_to_the_rhf_route_at_the_hartree_fock_determinant(kind):
    """theta = 0 with RHF orbitals: the pull-back through S^-1/2 must reduce to the energy-weighted density."""
    pqc, ncas, nelecas = circuit(kind)
    b = aoo.OO_pqc_batch.from_geometries(pqc, formal_basis(), formal_coords(POINTS), ncas, nelecas, oao_mo_coeffs="rhf")
    a = b.nuclear_gradient(torch.zeros((3, b.n_theta), dtype=F64, device=dev()))
    r = b.rhf_nuclear_gradient(b.rhf(conv_tol=1e-13))
    d = (a - r).abs().max().item()
    xyz = torch.as_tensor(formal_coords(POINTS) / BOHR).to(dev())
    torque = torch.cross(xyz, a, dim=2).sum(dim=1).abs().max().item()
    print(f"{kind}: nuclear_gradient(theta = 0) - rhf_nuclear_gradient = {d:.2e}; torque at the stationary point "
          f"{torque:.2e}")
    assert d < 1e-9
    # rotational invariance holds where the orbital gradient vanishes.  The "rhf" orbitals are converged to max |F D S -
    # S D F| < 1e-9 (err_tol of the solver), the orbital gradient is 4 times that per rotation pair at most, and a
    # rigid rotation's generator has elements of at most 1 on the N (N - 1) / 2 = 78 pairs: 78 * 4e-9.  Away from
    # stationarity the torque of these molecules is 3.6e-2 (the test above).
    assert torque < 78 * 4e-9


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------
def test_errors():
    pqc, ncas, nelecas = circuit("np_fabric")
    basis = formal_basis()
    from auto_oo_amd.gaussian import Moldata_sto3g
    mol = Moldata_sto3g(get_formal_geo(*POINTS[0]))
    host = aoo.OO_pqc_batch(pqc, [mol], ncas, nelecas, oao_mo_coeffs=[np.eye(13)])
    with pytest.raises(RuntimeError):
        host.nuclear_gradient(torch.zeros((1, host.n_theta), dtype=F64))
    with pytest.raises(RuntimeError):
        host.rhf_nuclear_gradient()
    xyz = formal_coords(POINTS[:2])
    N = basis.nao
    z = torch.zeros((2, N, N), dtype=F64, device=dev())
    with pytest.raises(ValueError):
        gto.gradient_batch(basis, xyz, dm1=z[:1])
    with pytest.raises(ValueError):
        gto.gradient_batch(basis, xyz, wq=torch.zeros((2, N, N + 1), dtype=F64, device=dev()))
    with pytest.raises(ValueError):
        gto.gradient_batch(basis, xyz, dm2=torch.zeros((2, N, N, N), dtype=F64, device=dev()))
    with pytest.raises(ValueError):
        gto.gradient_batch(basis, xyz[:, :4], dm1=z)
    b = cas_batch("np_fabric")
    with pytest.raises(ValueError):
        b.nuclear_gradient(seeded_thetas(b, 3), index=[3])
    # everything null: the zero gradient; the nuclear term alone is the repulsion's derivative in Angstrom input
    assert gto.gradient_batch(basis, xyz, nuc=False).abs().max().item() == 0.0
    g = gto.gradient_batch(basis, xyz)
    assert torch.equal(g, gto.gradient_into(basis, torch.as_tensor(xyz / BOHR).to(dev())))
