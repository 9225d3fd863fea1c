"""Point-charge embedding on the device (csrc/gto_charges.hip, gto.point_charge_*, OO_pqc_batch with point_charges=)
against the host twin ``gaussian.point_charge_integrals_from_table`` and against finite differences.

Bounds (none taken from what the device code gives):

* operator against the host twin: the bounds of ``int1e_ao`` against its host twin, ``TOL_H`` of tests/test_gto_gpu.py
  (9.4e-12, STO-3G) and of tests/test_gto_d_gpu.py (4.1e-12, the d tables M1 and M2);
* additivity in the batch: 1e-13 relative for ``int1e_ao``, 1e-12 relative for ``nuc`` (sums of a handful of doubles);
* energies 1e-9 Ha (the project's bound);
* gradients against central differences: per component ``max(1e-9, 10 |FD(h) - FD(h/2)|)``, the device compared with
  FD(h/2).  Raw gradients: h = 1e-5 Bohr, chosen on the CPU so that the two steps of the host twin agree to 6.0e-9
  (gQ, the charge 0.2 Bohr from the oxygen) and 6.1e-9 (gA) -- better than 1e-8 for every component of the fixture;
  without that charge 6e-11.  Batch energies (-56 Ha; a kernel's energy is good to 1e-12, so a central difference
  carries a noise of 1e-12 / h): h = 1e-3 Bohr for a generic coordinate (noise 1e-9, the step error of water's
  gradients at this h is 1e-7), h = 3e-5 Bohr for the stiff ones -- the charge 0.2 Bohr from the oxygen and the oxygen
  itself, whose third derivatives are 1e4 times larger (noise 3e-8, step error 1e-6 of gradients of 80 Ha/Bohr);
* whole-system invariance: 1e-10 Ha/Bohr times the number of summed terms.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import auto_oo_amd as aoo                                   # noqa: E402
from auto_oo_amd import gaussian, gto                       # noqa: E402
from tests import _charges as C                             # noqa: E402
from tests import _gto_d as D                               # noqa: E402
from tests.test_gto_gpu import TOL_H as TOL_H_SP            # noqa: E402
from tests.test_gto_d_gpu import TOL_H as TOL_H_D           # noqa: E402

F64 = torch.float64
BOHR = gaussian.BOHR
H_RAW = 1e-5            # Bohr (see above)
H_STIFF, H_SOFT = 3e-5, 1e-3
M_BATCH = 70            # charges of the embedded batches: one chunk of 64 and a rest


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def to_dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=F64).to(dev())


# ---- 1. the operator against the host twin ----------------------------------------------------------------------------
@pytest.mark.parametrize("M", C.M_SIZES)
@pytest.mark.parametrize("name", C.CASES)
def test_operator_against_the_host_twin(name, M):
    """Measured worst |device - host twin| over the sizes M: water 1.3e-15, M1 1.4e-15 (both forms), M2 2.4e-15 (both
    forms), of elements up to 4.6 ("Point-charge embedding"); printed per case."""
    basis, xyz = C.case(name)
    q, r = C.cloud(xyz, M)
    V = gto.point_charge_integrals_batch(basis, xyz, q, r)
    ref = C.host_operator_of(name, M)
    tol = TOL_H_SP if name == "water" else TOL_H_D
    err = np.abs(V[0].cpu().numpy() - ref).max()
    print(f"{name} M = {M}: max |V_ext| {np.abs(ref).max():.3g}, |device - host| {err:.2e} (bound {tol:.1e})")
    assert tuple(V.shape) == (1, basis.nao, basis.nao)
    assert torch.equal(V, V.transpose(1, 2))
    assert err < tol


def test_operator_with_the_nuclei_as_charges_is_the_nuclear_attraction_of_the_device():
    """V_ext of (Z_A, R_A) against int1e_ao minus the kinetic energy of the host: the bound of int1e_ao"""
    basis, xyz = C.case("water")
    R = C.bohr(xyz)
    V = gto.point_charge_integrals_batch(basis, xyz, basis.charges, xyz)[0].cpu().numpy()
    T = gaussian.one_electron_integrals(gaussian.shells_from_table(basis.table, R), (), ())[1]
    h = gto.integrals_batch(basis, xyz).int1e_ao[0].cpu().numpy()
    assert np.abs(V - (h - T)).max() < TOL_H_SP


# ---- 2. a geometry has the same bits wherever it stands ------------------------------------------------------------------
def stack_of_three(name, place):
    """geometry and cloud of the case at ``place`` of a stack of 3, the neighbours differ with the place"""
    basis, xyz = C.case(name)
    others = [(xyz + 0.05 * (k + 1) * np.array([0.3, -0.2, 0.5]), C.cloud(xyz, seed=100 + k + 7 * place)) for k in range(2)]
    mine = (xyz, C.cloud(xyz))
    items = others[:place] + [mine] + others[place:] if place < 2 else others + [mine]
    return (basis, np.stack([i[0] for i in items]), np.stack([i[1][0] for i in items]),
            np.stack([i[1][1] for i in items]))


@pytest.mark.parametrize("name", ["water", "m1-cartesian", "m2-spherical"])
def test_operator_does_not_depend_on_the_stack(name):
    basis, xyz = C.case(name)
    q, r = C.cloud(xyz)
    alone = gto.point_charge_integrals_batch(basis, xyz, q, r)[0]
    for place in (0, 2):
        b, X, Q, Rr = stack_of_three(name, place)
        V = gto.point_charge_integrals_batch(b, X, Q, Rr)
        assert torch.equal(V[place], alone)
        assert not torch.equal(V[1], alone)


def test_gradients_do_not_depend_on_the_stack():
    basis, xyz = C.case("water")
    q, r = C.cloud(xyz)
    Dm = to_dev(C.random_symmetric(basis.nao, 3))
    gA, gQ = gto.point_charge_gradient_batch(basis, xyz, q, r, Dm[None], nuc=False)
    for place in (0, 2):
        b, X, Q, Rr = stack_of_three("water", place)
        dm = torch.stack([Dm if k == place else to_dev(C.random_symmetric(basis.nao, 20 + k)) for k in range(3)])
        A, Qg = gto.point_charge_gradient_batch(b, X, Q, Rr, dm, nuc=False)
        assert torch.equal(A[place], gA[0]) and torch.equal(Qg[place], gQ[0])
        assert not torch.equal(A[1], gA[0])


# ---- 3. additivity in the batch --------------------------------------------------------------------------------------------
def circuit():
    return aoo.Parameterized_circuit(2, 2, None, ansatz="np_fabric", n_layers=1), 2, 2


def water_stack():
    """3 water geometries in Angstrom with one cloud each (no charge on a nucleus: the classical term exists)"""
    X = np.stack([C.WATER, D.WATER_2, C.WATER + np.array([0.02, -0.01, 0.03])])
    clouds = [C.cloud(X[k], M_BATCH, on_nucleus=False, seed=31 + k) for k in range(3)]
    return X, np.stack([c[0] for c in clouds]), np.stack([c[1] for c in clouds])


def test_embedded_batch_is_the_vacuum_batch_plus_the_operator():
    basis = C.water_basis()
    pqc, ncas, nelecas = circuit()
    X, Q, Rr = water_stack()
    eye = [np.eye(basis.nao)] * 3
    vac = aoo.OO_pqc_batch.from_geometries(pqc, basis, X, ncas, nelecas, oao_mo_coeffs=eye)
    emb = aoo.OO_pqc_batch.from_geometries(pqc, basis, X, ncas, nelecas, oao_mo_coeffs=eye, point_charges=(Q, Rr))
    I = gto.integrals_batch(basis, X)
    for name in ("int1e_ao", "nuc", "overlap", "int2e_ao", "oao_coeff"):
        assert torch.equal(getattr(vac, name), getattr(I, name)), name
    assert vac.charge_q is None and torch.equal(emb.overlap, vac.overlap) and torch.equal(emb.int2e_ao, vac.int2e_ao)
    V = gto.point_charge_integrals_batch(basis, X, Q, Rr)
    dh = (emb.int1e_ao - (vac.int1e_ao + V)).abs().max().item() / emb.int1e_ao.abs().max().item()
    e_pc = np.array([gaussian.point_charge_energy(basis.charges, C.bohr(X[k]), Q[k], C.bohr(Rr[k])) for k in range(3)])
    ref = vac.nuc.cpu().numpy() + e_pc
    dn = np.abs((emb.nuc.cpu().numpy() - ref) / ref).max()
    print(f"int1e_ao: relative {dh:.2e} (bound 1e-13); nuc: relative {dn:.2e} (bound 1e-12), classical term {e_pc}")
    assert dh < 1e-13 and dn < 1e-12
    assert torch.equal(emb.charge_q, to_dev(Q)) and torch.equal(emb.charge_xyz_bohr, to_dev(Rr / BOHR))
    # a frozen environment: moving a row without charges keeps its cloud; new charges replace it; M is fixed
    emb.set_geometries(X[2:3], index=[0])
    one = aoo.OO_pqc_batch.from_geometries(pqc, basis, X[2:3], ncas, nelecas, oao_mo_coeffs=eye[:1],
                                           point_charges=(Q[0], Rr[0]))
    assert torch.equal(emb.int1e_ao[0], one.int1e_ao[0]) and torch.equal(emb.nuc[0], one.nuc[0])
    emb.set_geometries(X[0:1], index=[0], point_charges=(Q[1], Rr[1]))
    one = aoo.OO_pqc_batch.from_geometries(pqc, basis, X[0:1], ncas, nelecas, oao_mo_coeffs=eye[:1],
                                           point_charges=(Q[1], Rr[1]))
    assert torch.equal(emb.int1e_ao[0], one.int1e_ao[0]) and torch.equal(emb.charge_q[0], to_dev(Q[1]))
    with pytest.raises(ValueError):
        emb.set_geometries(X[0:1], index=[0], point_charges=(Q[1][:5], Rr[1][:5]))
    with pytest.raises(ValueError, match="without point charges"):
        vac.set_geometries(X[0:1], index=[0], point_charges=(Q[1], Rr[1]))


# ---- 4. energy ---------------------------------------------------------------------------------------------------------------
def test_rhf_energy_of_embedded_water():
    basis = C.water_basis()
    pqc, ncas, nelecas = circuit()
    q, r = C.cloud(C.WATER, M_BATCH, on_nucleus=False)
    b = aoo.OO_pqc_batch.from_geometries(pqc, basis, C.WATER[None], ncas, nelecas, oao_mo_coeffs="rhf",
                                         point_charges=(q, r))
    R = C.bohr(C.WATER)
    S, h, g, nuc = gaussian.integrals_from_table(basis.table, basis.charges, R)
    h = h + C.host_operator(basis, C.WATER, q, r)
    e = gaussian.rhf(h, g, S, basis.nelectron // 2)[2] + nuc + gaussian.point_charge_energy(basis.charges, R, q, C.bohr(r))
    vac = gaussian.rhf(h - C.host_operator(basis, C.WATER, q, r), g, S, basis.nelectron // 2)[2] + nuc
    got = b.rhf().e_tot.item()
    print(f"embedded RHF {got:.10f}, host {e:.10f}, difference {abs(got - e):.2e}; vacuum {vac:.10f}")
    assert abs(got - e) < 1e-9
    assert abs(e - vac) > 1e-3                     # (the environment does something)


# ---- 5. raw gradients against the host twin ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def raw_reference():
    """central differences of sum D . V_ext(host twin) in every atom and charge coordinate at h and h / 2 ->
    (FD(h/2) of gA [3, 3], of gQ [M, 3], |FD(h) - FD(h/2)| of each)"""
    basis, xyz = C.case("water")
    q, r = C.cloud(xyz)
    R, rb = C.bohr(xyz), C.bohr(r)
    Dm = C.random_symmetric(basis.nao, 11)

    def per_charge(R_, r_):
        return np.einsum("kmn,mn->k", gaussian.point_charge_integrals_from_table(basis.table, R_, q, r_, per_charge=True),
                         Dm)
    fa, fq = [], []
    for h in (H_RAW, 0.5 * H_RAW):
        a, c = np.zeros((3, 3)), np.zeros((q.size, 3))
        for d in range(3):
            s = np.zeros(3)
            s[d] = h
            c[:, d] = (per_charge(R, rb + s) - per_charge(R, rb - s)) / (2 * h)        # (each charge feels only itself)
            for at in range(3):
                Rp, Rm = R.copy(), R.copy()
                Rp[at, d] += h
                Rm[at, d] -= h
                a[at, d] = (per_charge(Rp, rb).sum() - per_charge(Rm, rb).sum()) / (2 * h)
        fa.append(a)
        fq.append(c)
    return fa[1], fq[1], np.abs(fa[0] - fa[1]), np.abs(fq[0] - fq[1])


def test_raw_gradients_against_differences_of_the_host_twin():
    """water STO-3G, the whole fixture cloud (130 charges: one 0.2 Bohr from O, one ON a hydrogen, one 50 Bohr away),
    a random symmetric D, no classical term.  Measured on the CPU: |FD(h) - FD(h/2)| of the host twin up to 6.0e-9
    (gQ) and 6.1e-9 (gA) at h = 1e-5.  Device against FD(h/2): 2.2e-9 (gA) and 2.4e-9 (gQ, the charge 0.2 Bohr from O
    -- a third of the disagreement, the step error of FD(h/2) itself); the charge on the nucleus 3.7e-11, the other
    128 charges 4.5e-11; net force of atoms and charges together 2.7e-15."""
    basis, xyz = C.case("water")
    q, r = C.cloud(xyz)
    Dm = to_dev(C.random_symmetric(basis.nao, 11))
    ra, rq, da, dq = raw_reference()
    gA, gQ = gto.point_charge_gradient_batch(basis, xyz, q, r, Dm[None], nuc=False)
    ea, eq = np.abs(gA[0].cpu().numpy() - ra), np.abs(gQ[0].cpu().numpy() - rq)
    print(f"gA: max {np.abs(ra).max():.3g}, FD disagreement {da.max():.2e}, device - FD(h/2) {ea.max():.2e}; "
          f"gQ: max {np.abs(rq).max():.3g}, FD disagreement {dq.max():.2e}, device - FD(h/2) {eq.max():.2e} "
          f"(charge 0: {eq[0].max():.2e}, on the nucleus: {eq[1].max():.2e}, the others {eq[2:].max():.2e})")
    assert tuple(gA.shape) == (1, 3, 3) and tuple(gQ.shape) == (1, q.size, 3)
    assert da.max() < 1e-8 and dq.max() < 1e-8
    assert (ea < np.maximum(1e-9, 10 * da)).all()
    assert (eq < np.maximum(1e-9, 10 * dq)).all()
    assert not gQ[0, 3].any()                                         # q = 0
    # the operator alone is translationally invariant: atoms and charges together feel no net force
    net = (gA.sum(dim=1) + gQ.sum(dim=1)).abs().max().item()
    print(f"net {net:.2e}")
    assert net < 1e-10 * (3 + q.size)


def test_classical_term_of_the_raw_gradients():
    basis, xyz = C.case("water")
    q, r = C.cloud(xyz, on_nucleus=False)
    Dm = to_dev(C.random_symmetric(basis.nao, 11))[None]
    a0, q0 = gto.point_charge_gradient_batch(basis, xyz, q, r, Dm, nuc=False)
    a1, q1 = gto.point_charge_gradient_batch(basis, xyz, q, r, Dm, nuc=True)
    R, rb = C.bohr(xyz), C.bohr(r)
    d = R[:, None, :] - rb[None, :, :]
    f = basis.charges[:, None, None] * q[None, :, None] * d / np.linalg.norm(d, axis=2)[..., None] ** 3
    ea = np.abs((a1 - a0)[0].cpu().numpy() + f.sum(axis=1)).max()
    eq = np.abs((q1 - q0)[0].cpu().numpy() - f.sum(axis=0)).max()
    print(f"classical term: atoms {ea:.2e} of {np.abs(f.sum(axis=1)).max():.3g}, charges {eq:.2e} of "
          f"{np.abs(f.sum(axis=0)).max():.3g}")
    assert ea < 1e-12 * np.abs(f).sum(axis=1).max() and eq < 1e-12 * np.abs(f.sum(axis=0)).max()


# ---- 6. whole-system invariance ----------------------------------------------------------------------------------------------
def net_and_torque(xyz_bohr, gA, r_bohr, gQ):
    net = gA.sum(dim=1) + gQ.sum(dim=1)
    tq = torch.cross(xyz_bohr, gA, dim=2).sum(dim=1) + torch.cross(r_bohr, gQ, dim=2).sum(dim=1)
    return net.abs().max().item(), tq.abs().max().item()


@functools.lru_cache(maxsize=None)
def embedded_water(orbitals="rhf"):
    basis = C.water_basis()
    pqc, ncas, nelecas = circuit()
    q, r = C.cloud(C.WATER, M_BATCH, on_nucleus=False)
    return aoo.OO_pqc_batch.from_geometries(pqc, basis, C.WATER[None], ncas, nelecas, oao_mo_coeffs=orbitals,
                                            point_charges=(q, r))


def test_rhf_pair_feels_no_net_force_and_no_torque():
    b = embedded_water()
    gA, gQ = b.rhf_nuclear_gradient(), b.rhf_point_charge_gradient()
    net, tq = net_and_torque(b.coords_bohr, gA, b.charge_xyz_bohr, gQ)
    bound = 1e-10 * (3 + M_BATCH)
    print(f"RHF: net force {net:.2e}, torque {tq:.2e} (bound {bound:.1e}); max |gA| {gA.abs().max().item():.3g}, "
          f"max |gQ| {gQ.abs().max().item():.3g}")
    assert tuple(gQ.shape) == (1, M_BATCH, 3)
    assert net < bound and tq < bound


def test_cas_pair_feels_no_net_force_and_no_torque():
    """CAS(2,2) of embedded water.  The net force vanishes at ANY parameters and orbitals.  The torque of a gradient at
    fixed OAO-to-MO coefficients is dE/dphi of a rigid rotation at fixed coefficients, which vanishes only where the
    orbital gradient does (tests/test_nucgrad_gpu.py): it is therefore checked at the stationary point the Newton
    steps of the batch reach from non-zero thetas -- thetas stay non-zero there, the state is correlated."""
    basis = C.water_basis()
    pqc, ncas, nelecas = circuit()
    q, r = C.cloud(C.WATER, M_BATCH, on_nucleus=False)
    b = aoo.OO_pqc_batch.from_geometries(pqc, basis, C.WATER[None], ncas, nelecas, oao_mo_coeffs="rhf",
                                         point_charges=(q, r))
    bound = 1e-10 * (3 + M_BATCH)
    th = torch.full((1, b.n_theta), 0.3, dtype=F64, device=dev())
    net, tq = net_and_torque(b.coords_bohr, b.nuclear_gradient(th), b.charge_xyz_bohr, b.point_charge_gradient(th))
    print(f"CAS away from the stationary point: net force {net:.2e} (bound {bound:.1e}), torque {tq:.2e}")
    assert net < bound
    for it in range(30):
        g = b.energy_gradient_hessian(th)[1].abs().max().item()
        if g < 1e-12:
            break
        th = b.damped_newton_step(th)[0]
    net, tq = net_and_torque(b.coords_bohr, b.nuclear_gradient(th), b.charge_xyz_bohr, b.point_charge_gradient(th))
    print(f"CAS after {it} Newton steps: thetas {th.cpu().numpy().ravel()}, |gradient| {g:.2e}, net force {net:.2e}, "
          f"torque {tq:.2e} (bound {bound:.1e})")
    assert th.abs().max().item() > 1e-3
    assert net < bound and tq < bound


# ---- 7. batch gradients against differences of batch energies ----------------------------------------------------------------
# (what moves, its index, the component, the step); charge 0 sits 0.2 Bohr from atom 0
MOVES = (("atom", 0, 1, H_STIFF), ("atom", 2, 0, H_SOFT), ("charge", 0, 2, H_STIFF), ("charge", 0, 0, H_STIFF),
         ("charge", 5, 1, H_SOFT))


@functools.lru_cache(maxsize=None)
def fixed_orbitals():
    """the RHF orbitals of embedded water times expm of a seeded skew matrix of norm 0.05 (the pull-back through S^-1/2
    is exercised)"""
    U = embedded_water().oao_mo_coeff[0].cpu().numpy()
    K = np.random.default_rng(17).standard_normal(U.shape)
    K = K - K.T
    K *= 0.05 / np.linalg.norm(K)
    return U @ torch.linalg.matrix_exp(torch.as_tensor(K)).numpy()


@functools.lru_cache(maxsize=None)
def displaced_batch():
    """the embedded water of ``embedded_water`` re-made at +h, -h, +h/2, -h/2 along every move of MOVES, same orbital
    coefficients everywhere: [4 * len(MOVES)] geometries in one batch"""
    basis = C.water_basis()
    pqc, ncas, nelecas = circuit()
    q, r = C.cloud(C.WATER, M_BATCH, on_nucleus=False)
    X, Rr = [], []
    for kind, k, d, h in MOVES:
        for s in (1.0, -1.0, 0.5, -0.5):
            x, rr = C.bohr(C.WATER), C.bohr(r)
            (x if kind == "atom" else rr)[k, d] += s * h
            X.append(x * BOHR)
            Rr.append(rr * BOHR)
    n = len(X)
    return aoo.OO_pqc_batch.from_geometries(pqc, basis, np.stack(X), ncas, nelecas, oao_mo_coeffs=[fixed_orbitals()] * n,
                                            point_charges=(np.repeat(q[None], n, axis=0), np.stack(Rr)))


def differences(e):
    """energies [4 * len(MOVES), ...] of ``displaced_batch`` -> (FD(h/2), |FD(h) - FD(h/2)|), each [len(MOVES), ...]"""
    e = e.reshape((len(MOVES), 4) + e.shape[1:])
    h = np.array([m[3] for m in MOVES]).reshape((-1,) + (1,) * (e.ndim - 2))
    f1, f2 = (e[:, 0] - e[:, 1]) / (2 * h), (e[:, 2] - e[:, 3]) / h
    return f2, np.abs(f1 - f2)


def picked(gA, gQ):
    return np.array([(gA if kind == "atom" else gQ)[k, d] for kind, k, d, _ in MOVES])


def test_batch_gradients_against_differences_of_the_energy():
    basis = C.water_basis()
    pqc, ncas, nelecas = circuit()
    q, r = C.cloud(C.WATER, M_BATCH, on_nucleus=False)
    b = aoo.OO_pqc_batch.from_geometries(pqc, basis, C.WATER[None], ncas, nelecas, oao_mo_coeffs=[fixed_orbitals()],
                                         point_charges=(q, r))
    th = torch.as_tensor(np.random.default_rng(5).uniform(-0.6, 0.6, (1, b.n_theta))).to(dev())
    fd = displaced_batch()
    ref, dis = differences(fd.energy(th.repeat(fd.G, 1)).cpu().numpy())
    got = picked(b.nuclear_gradient(th)[0].cpu().numpy(), b.point_charge_gradient(th)[0].cpu().numpy())
    for m, g_, r_, d_ in zip(MOVES, got, ref, dis):
        print(f"{m}: analytic {g_:+.10f}, FD(h/2) {r_:+.10f}, error {abs(g_ - r_):.2e}, FD disagreement {d_:.2e}")
    assert (np.abs(got - ref) < np.maximum(1e-9, 10 * dis)).all()
    assert torch.equal(b.point_charge_gradient(th, index=[0]), b.point_charge_gradient(th))


def test_casci_state_gradients_against_differences_of_the_casci_energies():
    basis = C.water_basis()
    pqc, ncas, nelecas = circuit()
    q, r = C.cloud(C.WATER, M_BATCH, on_nucleus=False)
    b = aoo.OO_pqc_batch.from_geometries(pqc, basis, C.WATER[None], ncas, nelecas, oao_mo_coeffs=[fixed_orbitals()],
                                         point_charges=(q, r))
    res = b.casci_nuclear_gradients(nroots=2)
    ref, dis = differences(displaced_batch().casci(2)[0].cpu().numpy())
    atoms = [i for i, m in enumerate(MOVES) if m[0] == "atom"]
    for I in range(2):
        g = res.gradients[0, I, I].cpu().numpy()
        for i in atoms:
            _, k, d, _ = MOVES[i]
            print(f"root {I}, atom {k} component {d}: analytic {g[k, d]:+.10f}, FD(h/2) {ref[i, I]:+.10f}, error "
                  f"{abs(g[k, d] - ref[i, I]):.2e}, FD disagreement {dis[i, I]:.2e}")
            assert abs(g[k, d] - ref[i, I]) < max(1e-9, 10 * dis[i, I])
    cpl = b.casci_derivative_couplings(nroots=2)
    assert torch.equal(cpl.gradients, res.gradients)
    assert torch.equal(res.gradients[0, 0, 1], res.gradients[0, 1, 0])


def test_vacuum_batch_is_untouched():
    basis = C.water_basis()
    pqc, ncas, nelecas = circuit()
    make = lambda: aoo.OO_pqc_batch.from_geometries(pqc, basis, C.WATER[None], ncas, nelecas, oao_mo_coeffs="rhf")   # noqa: E731
    a, b = make(), make()
    th = torch.full((1, a.n_theta), 0.2, dtype=F64, device=dev())
    assert torch.equal(a.nuclear_gradient(th), b.nuclear_gradient(th))
    assert torch.equal(a.rhf_nuclear_gradient(), b.rhf_nuclear_gradient())
    assert torch.equal(a.casci_nuclear_gradients(2).gradients, b.casci_nuclear_gradients(2).gradients)
    ref = gto.gradient_into(basis, a.coords_bohr, *_rhf_sets(a))
    assert torch.equal(a.rhf_nuclear_gradient(), ref)
    for f in (lambda: a.point_charge_gradient(th), a.rhf_point_charge_gradient):
        with pytest.raises(RuntimeError, match="point_charges"):
            f()


def _rhf_sets(b):
    from auto_oo_amd import nucgrad
    res = b.rhf()
    d1, d2 = nucgrad.cas_ao_densities(res.mo_coeff, b.nelectron // 2, 0)
    return d1, nucgrad.energy_weighted_pullback(res.mo_coeff, res.mo_energy, b.nelectron // 2), d2, True


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    basis, xyz = C.case("water")
    X = to_dev(C.bohr(xyz))[None]
    q, r = C.cloud(xyz, 4)
    qd, rd = to_dev(q)[None], to_dev(C.bohr(r))[None]
    Dm = to_dev(C.random_symmetric(basis.nao, 1))[None]
    with pytest.raises(NotImplementedError, match="d shells"):
        gto.point_charge_gradient_into(D.m2_basis(), X, qd, rd, Dm)
    bad = rd.clone()
    bad[0, 2, 1] = float("nan")
    for args in ((X, qd, bad), (X, qd * float("inf"), rd), (X * float("nan"), qd, rd)):
        with pytest.raises(ValueError, match="finite"):
            gto.point_charge_integrals_into(basis, *args)
        with pytest.raises(ValueError, match="finite"):
            gto.point_charge_gradient_into(basis, *args, Dm)
    # the C entries themselves: a negative code and a message, nothing launched
    lib = aoo._lib.load()
    t = basis.device_tables(dev())
    work = basis.work(dev(), 1)
    out = torch.zeros((1, basis.nao, basis.nao), dtype=F64, device=dev())
    p = aoo._lib.dptr
    for M in (0, 65536):
        rc = lib.oovqe_gto_point_charge_batch(basis.nshell, p(t.shells, torch.int32), int(basis.exps.size), p(t.exps),
                                              p(t.coefs), basis.natm, p(t.charges), 1, p(X), basis.nao, M, p(qd), p(rd),
                                              p(out), p(work), aoo._lib.stream_ptr())
        assert rc < 0 and not out.any()
    d = D.m2_basis()
    td = d.device_tables(dev())
    gA, gQ = torch.zeros((1, 3, 3), dtype=F64, device=dev()), torch.zeros((1, 4, 3), dtype=F64, device=dev())
    wd = gto.point_charge_gradient_work(d, dev(), 1, 4)
    Dd = torch.zeros((1, d.nao, d.nao), dtype=F64, device=dev())
    rc = lib.oovqe_gto_point_charge_gradient_batch(d.nshell, p(td.shells, torch.int32), int(d.exps.size), p(td.exps),
                                                   p(td.coefs), d.natm, p(td.charges), 1, p(X), d.nao, 4, p(qd), p(rd),
                                                   p(Dd), 1, p(gA), p(gQ), p(wd), aoo._lib.stream_ptr())
    assert rc < 0 and not gA.any() and not gQ.any()
    with pytest.raises(aoo._lib.OovqeError, match="d shells"):
        aoo._lib.check(rc, "oovqe_gto_point_charge_gradient_batch")
