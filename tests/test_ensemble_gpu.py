"""State-averaged OO-VQE on the device (csrc/ensemble.hip, auto_oo_amd/ensemble.py).

1. the three kernels against the longdouble host twin (tests/_ensemble.py) within the bounds derived there (no figure
   of a bound comes from device output); 2. their bitwise properties; 3. E_SA, gradient and full Hessian against torch
autograd through the oracle's superposed statevectors; 4. S = 1 against the existing engine; 5. invariance of the
equi-ensemble under a rotation of its initial states; 6. / 7. the ensemble variational principle on H4 end to end;
8. the nuclear gradient of E_SA against finite differences; 9. refusals.

Every comparison prints its figures before it asserts.  Measured on an MI355X, largest error against the derived
bounds over the eight kernel cases: vectors (2-norm) 2.5e-16 against 3.8e-15 .. 4.3e-14 (at most 0.087 of the bound),
RDM and transition sets 1.1e-15 against 1.9e-14 .. 1.8e-12 (0.032), H 4.6e-15 against 1.5e-12 .. 5.1e-11 (0.001);
against the oracle |dE| 2.7e-13, |dgrad| 1.1e-13, |dH| 2.0e-13; S = 1 against the existing engine 0, 0, 8.9e-16; under
a rotation of the equi-ensemble 3.6e-15 against 9.6e-12; H4: 3 Newton steps, 4.4e-16 from the mean of the roots, the
full optimisation 5 steps to max |grad| 9.3e-11; nuclear gradient 5.3e-13 against a bound of 3.5e-11.  (The figures
that pass through the RDM sets were printed while that kernel still summed an element in one thread; with one wave per
element every test passes within the same bounds, its figures were not printed again.)
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.linalg
import torch

pytestmark = pytest.mark.gpu

import auto_oo_amd as aoo                                   # noqa: E402
from auto_oo_amd import _lib, gto                           # noqa: E402
from auto_oo_amd._lib import check, dptr, stream_ptr        # noqa: E402
from auto_oo_amd.gaussian import BOHR                       # noqa: E402
from oracle import cpu_ref as R                             # noqa: E402
from tests import _circuit_scope as C                       # noqa: E402
from tests import _ensemble as T                            # noqa: E402
from tests.test_nucgrad_gpu import fd_combine, fd_stack     # noqa: E402

F64 = torch.float64
U = C.U


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def to_dev(x, dtype=F64):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(dev()).contiguous()


@functools.lru_cache(maxsize=None)
def circuit(name):
    ncas, nelecas, ansatz, kw = T.CIRCUITS[name]
    return aoo.Parameterized_circuit(ncas, nelecas, None, ansatz=ansatz, **kw)


# ---- 1. the kernels against the twin --------------------------------------------------------------------------------
def run_kernels(name, theta, psi0, w, pairs, c1=None, c2=None, transition=True):
    """The three library calls on host inputs -> (vecs [G, S, nv, D], gamma_sa, Gamma_sa, gamma_st, Gamma_st, H) as
    device tensors (H None without pairs)."""
    lib, pqc = _lib.load(), circuit(name)
    a, n = pqc.ncas, pqc.n_qubits
    G, nt = theta.shape
    nS, npairs = psi0.shape[0], len(pairs)
    th, p0, wd = to_dev(theta), to_dev(psi0), to_dev(w)
    pd = to_dev(np.array(pairs, dtype=np.int32).reshape(-1, 2), torch.int32) if npairs else None
    size = lib.oovqe_ensemble_work_size(nt, n, nS, npairs, G)
    assert size == G * nS * (1 + nt + npairs) * (1 << n)
    vecs = torch.empty(size, dtype=F64, device=dev())
    check(lib.oovqe_ensemble_states(dptr(th), nt, dptr(pqc._gates_dev, torch.uint8), pqc._n_gates, n, dptr(p0), nS,
                                    None if pd is None else dptr(pd, torch.int32), npairs, G, dptr(vecs),
                                    stream_ptr()), "oovqe_ensemble_states")
    g1 = torch.empty((G, 1 + nt, a, a), dtype=F64, device=dev())
    g2 = torch.empty((G, 1 + nt) + (a,) * 4, dtype=F64, device=dev())
    t1 = torch.empty((G, nS, nS, a, a), dtype=F64, device=dev()) if transition else None
    t2 = torch.empty((G, nS, nS) + (a,) * 4, dtype=F64, device=dev()) if transition else None
    check(lib.oovqe_ensemble_rdms(dptr(vecs), 1 + nt + npairs, dptr(wd), n, a, nS, nt, G, dptr(g1), dptr(g2),
                                  dptr(t1), dptr(t2), stream_ptr()), "oovqe_ensemble_rdms")
    H = None
    if npairs:
        # c1 | c2 of every row in one packed array with a stride, as the CAS evaluation leaves them
        stride = a * a + a ** 4 + 3
        c12 = torch.zeros((G, stride), dtype=F64, device=dev())
        c12[:, :a * a] = to_dev(c1).reshape(1, -1)
        c12[:, a * a:a * a + a ** 4] = to_dev(c2).reshape(1, -1)
        H = torch.full((G, nt, nt), float("nan"), dtype=F64, device=dev())
        check(lib.oovqe_ensemble_circuit_hessian_batch(
            dptr(vecs), dptr(wd), n, a, nS, nt, dptr(pd, torch.int32), npairs, G, dptr(c12),
            ctypes.c_void_p(c12.data_ptr() + 8 * a * a), stride, dptr(H), stream_ptr()),
            "oovqe_ensemble_circuit_hessian_batch")
    torch.cuda.synchronize()
    return vecs.view(G, nS, 1 + nt + npairs, 1 << n), g1, g2, t1, t2, H


def worst(err, bound):
    """largest error, and the largest ratio error / bound (inf where an error exceeds a zero bound)"""
    err, bound = np.asarray(err), np.asarray(bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > bound, np.where(bound > 0, err / bound, np.inf), np.where(bound > 0, err / bound, 0.0))
    return float(err.max()), float(ratio.max())


@pytest.mark.parametrize("case", T.KERNEL_CASES, ids=T.case_id)
def test_kernels_against_the_twin(case):
    ref = T.reference(case)
    with_h = case[4]
    vecs, g1, g2, t1, t2, H = run_kernels(case[0], ref["theta"], ref["psi0"], ref["w"], ref["pairs"],
                                          ref.get("c1"), ref.get("c2"))
    ev = np.linalg.norm(vecs.cpu().numpy() - ref["vecs"], axis=3)
    rows = [("vectors (2-norm)", ev, ref["vb"]),
            ("gamma_sa", np.abs(g1.cpu().numpy() - ref["g1"]), ref["b1"]),
            ("Gamma_sa", np.abs(g2.cpu().numpy() - ref["g2"]), ref["b2"]),
            ("gamma_st", np.abs(t1.cpu().numpy() - ref["t1"]), ref["tb1"]),
            ("Gamma_st", np.abs(t2.cpu().numpy() - ref["t2"]), ref["tb2"])]
    if with_h:
        Hh = H.cpu().numpy()
        assert np.array_equal(Hh, Hh.transpose(0, 2, 1))
        rows.append(("H", np.abs(Hh - ref["H"]), ref["HB"]))
    res = [(name,) + worst(e, b) + (float(np.max(b)),) for name, e, b in rows]
    for name, emax, ratio, bmax in res:
        print(f"{T.case_id(case)}: {name}: largest error {emax:.2e}, largest bound {bmax:.2e}, "
              f"largest error / bound {ratio:.3f}")
    for name, emax, ratio, _ in res:
        assert ratio <= 1.0, name
    # a parameter that drives no gate, and the skipped gates: exact zeros where the twin has them
    zero = np.all(ref["vecs"] == 0.0, axis=3)
    assert np.all(vecs.cpu().numpy()[zero] == 0.0)


# ---- 2. bitwise properties ------------------------------------------------------------------------------------------
def test_a_row_has_the_same_bits_wherever_it_stands():
    case = ("cas43_ucc", "singlet2", "w73", 5, True)
    ref = T.reference(case)
    args = (ref["psi0"], ref["w"], ref["pairs"], ref["c1"], ref["c2"])
    full = run_kernels(case[0], ref["theta"], *args)
    alone = run_kernels(case[0], ref["theta"][2:3], *args)
    moved = run_kernels(case[0], ref["theta"][[4, 2, 0]], *args)
    for a, b, c in zip(full, alone, moved):
        assert torch.equal(a[2], b[0]) and torch.equal(a[2], c[1]) and torch.equal(a[4], c[0])


def test_a_state_of_weight_zero_changes_nothing():
    case = ("cas22_fabric1", "singlet3", "zero3", 5, True)
    ref = T.reference(case)
    three = run_kernels(case[0], ref["theta"], ref["psi0"], ref["w"], ref["pairs"], ref["c1"], ref["c2"])
    two = run_kernels(case[0], ref["theta"], ref["psi0"][[0, 2]], ref["w"][[0, 2]], ref["pairs"], ref["c1"], ref["c2"])
    assert ref["w"][1] == 0.0
    assert torch.equal(three[1], two[1]) and torch.equal(three[2], two[2]) and torch.equal(three[5], two[5])
    assert torch.equal(three[0][:, [0, 2]], two[0])


@pytest.mark.parametrize("case", [T.KERNEL_CASES[1], T.KERNEL_CASES[4]], ids=T.case_id)
def test_weighted_state_sets_sum_to_set_zero(case):
    ref = T.reference(case)
    _, g1, g2, t1, t2, _ = run_kernels(case[0], ref["theta"], ref["psi0"], ref["w"], [])
    w = to_dev(ref["w"])
    nS = len(ref["w"])
    d1 = torch.diagonal(t1, dim1=1, dim2=2).movedim(-1, 1)          # [G, S, a, a]
    d2 = torch.diagonal(t2, dim1=1, dim2=2).movedim(-1, 1)
    s1 = (d1 * w[None, :, None, None]).sum(dim=1)
    s2 = (d2 * w[None, :, None, None, None, None]).sum(dim=1)
    idx = np.arange(nS)
    # each side is within its bound of the same exact number; the sum over S terms adds (S + 1) u of the sum of the
    # absolute terms, which the bound of set 0 (2 (D + 13 + S) u of it) contains
    b1 = ref["b1"][:, 0] + np.einsum("s,gsab->gab", ref["w"], ref["tb1"][:, idx, idx]) + ref["b1"][:, 0]
    b2 = ref["b2"][:, 0] + np.einsum("s,gsabcd->gabcd", ref["w"], ref["tb2"][:, idx, idx]) + ref["b2"][:, 0]
    e1, e2 = (s1 - g1[:, 0]).abs().cpu().numpy(), (s2 - g2[:, 0]).abs().cpu().numpy()
    print(f"{T.case_id(case)}: sum_I w_I gamma_st[I][I] - gamma_sa[0]: {e1.max():.2e} (bound {b1.max():.2e}), Gamma: "
          f"{e2.max():.2e} (bound {b2.max():.2e})")
    assert np.all(e1 <= b1) and np.all(e2 <= b2)


# ---- 3. / 4. / 5. energies, gradients, Hessians on a synthetic problem ----------------------------------------------
SYNTH = {"cas22_fabric1": 6, "cas43_ucc": 8}                  # circuit -> electrons of the N = 8 problem
N_SYNTH = 8


@functools.lru_cache(maxsize=None)
def synthetic_batch(name, G=2):
    ncas, nelecas = T.CIRCUITS[name][:2]
    probs = [R.synthetic_problem(N_SYNTH, 20300 + g) for g in range(G)]
    mols = [aoo.Moldata(P["int1e_ao"], P["int2e_ao"], P["overlap"], P["nuc"] + 0.01 * g, SYNTH[name])
            for g, P in enumerate(probs)]
    batch = aoo.OO_pqc_batch(circuit(name), mols, ncas, nelecas, oao_mo_coeffs=[P["oao_mo_coeff"] for P in probs])
    return batch, probs


def synthetic_thetas(name, G=2):
    return C.thetas("synthetic_" + name, G, T.gate_table(name)[1])


def oracle_energy(name, P, nelec, psi0, w, oao_mo_coeff=None):
    """x = (theta, kappa) -> sum_I w_I E_I(theta, kappa) through the oracle's superposed statevectors and
    OracleOOEnergy.energy_from_kappa"""
    ncas, nelecas = T.CIRCUITS[name][:2]
    nt = T.gate_table(name)[1]
    omol = R.OracleMol(P["int1e_ao"], P["int2e_ao"], P["overlap"], P["nuc"], nelec)
    oo = R.OracleOOEnergy(omol, ncas, nelecas, P["oao_mo_coeff"] if oao_mo_coeff is None else oao_mo_coeff)
    rops = R.RdmOperators(ncas)

    def energy(x):
        g1, g2 = 0.0, 0.0
        for I in range(psi0.shape[0]):
            r1, r2 = R.rdms_from_state(T.oracle_state(name, x[:nt], psi0[I]), rops)
            g1, g2 = g1 + w[I] * r1, g2 + w[I] * r2
        return oo.energy_from_kappa(x[nt:], g1, g2)

    return energy, oo.n_kappa


# rows of the synthetic stack the oracle differentiates: its autograd Hessian of CAS(4e,3o) takes seconds per geometry
# on the host, so that case compares the second row alone (the row whose outputs lie behind another row's)
ORACLE_ROWS = {"cas22_fabric1": (0, 1), "cas43_ucc": (1,)}


@functools.lru_cache(maxsize=None)
def oracle_egh(name, kind, wname):
    """(E [R], gradient [R, n], Hessian [R, n, n]) of the oracle at kappa = 0 for the rows ORACLE_ROWS of the synthetic
    stack (computed once)"""
    _, probs = synthetic_batch(name)
    th = synthetic_thetas(name)
    psi0, w = T.initial_states(name, kind), T.WEIGHTS[wname]
    out = []
    for g in ORACLE_ROWS[name]:
        Pg = dict(probs[g], nuc=probs[g]["nuc"] + 0.01 * g)
        f, nk = oracle_energy(name, Pg, SYNTH[name], psi0, w)
        x = torch.cat((torch.as_tensor(th[g]), torch.zeros(nk, dtype=F64)))
        out.append((f(x).item(), torch.autograd.functional.jacobian(f, x).numpy(),
                    torch.autograd.functional.hessian(f, x).numpy()))
    return tuple(np.stack(z) for z in zip(*out))


@pytest.mark.parametrize("name,kind,wname", [("cas22_fabric1", "singlet2", "w73"), ("cas43_ucc", "singlet2", "equal2")])
def test_energy_gradient_hessian_against_the_oracle(name, kind, wname):
    batch, probs = synthetic_batch(name)
    ens = aoo.StateEnsemble(circuit(name), T.initial_states(name, kind), T.WEIGHTS[wname])
    sa = aoo.SA_OO_pqc_batch(batch, ens)
    th = to_dev(synthetic_thetas(name))
    rows = list(ORACLE_ROWS[name])
    E, grad, H = sa.energy_gradient_hessian(th)
    Er, gr, Hr = oracle_egh(name, kind, wname)
    eg = sa.energy_and_gradient(th).cpu().numpy()[rows]
    de = np.abs(E.cpu().numpy()[rows] - Er).max()
    dg = np.abs(grad.cpu().numpy()[rows] - gr).max()
    dh = np.abs(H.cpu().numpy()[rows] - Hr).max()
    sym = (H - H.transpose(1, 2)).abs().max().item()
    print(f"{name} {kind} {wname}: |dE| {de:.2e}, |dgrad| {dg:.2e}, |dH| {dh:.2e}, asymmetry {sym:.2e}")
    assert de < 1e-9 and dg < 1e-8 and dh < 1e-8 and sym < 1e-8
    assert np.abs(eg[:, 0] - Er).max() < 1e-9 and np.abs(eg[:, 1:] - gr).max() < 1e-8
    assert np.abs(sa.energy(th).cpu().numpy()[rows] - Er).max() < 1e-9
    # the state energies and the energy at rotated orbitals, against the oracle
    w = np.array(T.WEIGHTS[wname])
    assert np.abs((sa.state_energies(th).cpu().numpy() * w).sum(axis=1)[rows] - Er).max() < 1e-9
    kap = 0.05 * np.random.default_rng(4).standard_normal((batch.G, batch.n_kappa))
    ek = sa.energy(th, to_dev(kap)).cpu().numpy()
    for g, P in enumerate(probs):
        f, _ = oracle_energy(name, dict(P, nuc=P["nuc"] + 0.01 * g), SYNTH[name], T.initial_states(name, kind), w)
        x = torch.cat((torch.as_tensor(synthetic_thetas(name)[g]), torch.as_tensor(kap[g])))
        assert abs(ek[g] - f(x).item()) < 1e-9


@pytest.mark.parametrize("name", ["cas22_fabric1", "cas43_ucc"])
def test_one_state_reduces_to_the_existing_engine(name):
    batch, _ = synthetic_batch(name)
    sa = aoo.SA_OO_pqc_batch(batch, aoo.StateEnsemble(circuit(name), T.initial_states(name, "hf"), (1.0,)))
    th = to_dev(synthetic_thetas(name))
    E, g, H = sa.energy_gradient_hessian(th)
    Er, gr, Hr = batch.energy_gradient_hessian(th)
    de, dg, dh = (E - Er).abs().max().item(), (g - gr).abs().max().item(), (H - Hr).abs().max().item()
    print(f"{name}: S = 1 against OO_pqc_batch: |dE| {de:.2e}, |dgrad| {dg:.2e}, |dH| {dh:.2e}")
    assert de < 1e-9 and dg < 1e-8 and dh < 1e-8
    assert (sa.energy_and_gradient(th) - batch.energy_and_gradient(th)).abs().max().item() < 1e-8


def kappa_response(batch):
    """(M [G, a^2 + a^4, n_kappa], g0 [G, n_kappa]): the orbital gradient of the existing CAS evaluation is affine in
    the RDMs, g_kappa = g0 + sum_e M[e] r_e; row k >= 1 of its kappa-theta output is M applied to derivative set k, so
    unit sets read M off (the CAS path is not under test here: it is the parent's)."""
    a, G = batch.ncas, batch.G
    ne = a * a + a ** 4
    g1 = torch.zeros((G, 1 + ne, a * a), dtype=F64, device=dev())
    g2 = torch.zeros((G, 1 + ne, a ** 4), dtype=F64, device=dev())
    for e in range(ne):
        (g1 if e < a * a else g2)[:, 1 + e, e if e < a * a else e - a * a] = 1.0
    out, _, _ = batch._cas_batch(g1.reshape(G, 1 + ne, a, a), g2.reshape((G, 1 + ne) + (a,) * 4), G)
    gv = out[:, 2 + ne:2 + ne + (1 + ne) * batch.n_kappa].reshape(G, 1 + ne, batch.n_kappa)
    return gv[:, 1:].cpu().numpy(), gv[:, 0].cpu().numpy()


@pytest.mark.parametrize("name,kind", [("cas22_fabric1", "singlet2"), ("cas43_ucc", "singlet3")])
def test_the_equi_ensemble_is_invariant_under_a_rotation_of_its_states(name, kind):
    """Equal weights, psi0 -> R psi0 with a seeded random orthogonal R: E_SA and its gradient stay the same within twice
    the bound of test 1 carried through the contraction with the CAS coefficients (each side is within one bound of the
    same exact number), state_energies change, the resolved energies do not.

    The bound: E = c0 + c1 . gamma + c2 . Gamma and dE/dtheta_k = c1 . gamma_k + c2 . Gamma_k, with the coefficients of
    the batch (the same bits on both sides): |c1| . B_gamma + |c2| . B_Gamma, plus (a^4 + a^2 + 4) u of the sum of the
    absolute terms for the contraction.  dE/dkappa = g0 + M r (``kappa_response``): sum_e |M_e| B_e, plus
    (4 N + a^4 + a^2 + 8) u (|g0| + sum_e |M_e| |r_e|) for the four index transformations of length N and the RDM
    contraction the evaluation is made of.  The resolved energies are eigenvalues of H_IJ, which move by at most the
    2-norm of its perturbation <= S max |delta H_IJ|, delta H_IJ bounded like E from the transition-set bounds."""
    batch, _ = synthetic_batch(name)
    pqc = circuit(name)
    ncas = pqc.ncas
    a2, a4 = ncas ** 2, ncas ** 4
    psi0 = T.initial_states(name, kind)
    nS = psi0.shape[0]
    Rm = T.random_orthogonal(nS, 11)
    rot = Rm @ psi0
    w = np.full(nS, 1.0 / nS)
    theta = synthetic_thetas(name)
    th = to_dev(theta)
    gates, nt = T.gate_table(name)
    reg = C.register(ncas)
    sides = []
    for states in (psi0, rot):
        sa = aoo.SA_OO_pqc_batch(batch, aoo.StateEnsemble(pqc, states, None))
        bounds = []
        for g in range(batch.G):
            v = T.vectors(gates, nt, theta[g], 2 * ncas, states, (), T.LD)
            vb = T.vector_bounds(gates, nt, [], v)
            bounds.append(T.rdm_bounds(reg, v, w, nt, vb) + T.transition_bounds(reg, v, vb)
                          + T.ensemble_rdms(reg, np.asarray(v, dtype=np.float64), w, nt, absolute=True))
        sides.append((sa.energy_and_gradient(th).cpu().numpy(), sa.state_energies(th).cpu().numpy(),
                      sa.resolve(th)[0], [np.stack(x) for x in zip(*bounds)]))
    out, _, _ = batch._cas_batch(*[x.contiguous() for x in aoo.SA_OO_pqc_batch(
        batch, aoo.StateEnsemble(pqc, psi0, None)).rdms(th)], batch.G)
    out = out.cpu().numpy()
    c0 = np.abs(out[:, 0])
    c1 = np.abs(out[:, 3 + batch.n_kappa:3 + batch.n_kappa + a2])
    c2 = np.abs(out[:, 3 + batch.n_kappa + a2:])
    M, g0 = kappa_response(batch)
    bound = np.zeros_like(sides[0][0])
    hb = 0.0
    for _, _, _, (b1, b2, tb1, tb2, s1, s2) in sides:
        b1f, b2f = b1.reshape(batch.G, 1 + nt, a2), b2.reshape(batch.G, 1 + nt, a4)
        s1f, s2f = s1.reshape(batch.G, 1 + nt, a2), s2.reshape(batch.G, 1 + nt, a4)
        lin = np.einsum("ge,gke->gk", c1, b1f) + np.einsum("ge,gke->gk", c2, b2f)
        mag = np.einsum("ge,gke->gk", c1, s1f) + np.einsum("ge,gke->gk", c2, s2f)
        mag[:, 0] += c0
        bound[:, :1 + nt] += lin + (a4 + a2 + 4) * U * mag
        be = np.concatenate((b1f[:, 0], b2f[:, 0]), axis=1)
        re = np.concatenate((s1f[:, 0], s2f[:, 0]), axis=1)
        bound[:, 1 + nt:] += np.einsum("gek,ge->gk", np.abs(M), be) \
            + (4 * N_SYNTH + a4 + a2 + 8) * U * (np.abs(g0) + np.einsum("gek,ge->gk", np.abs(M), re))
        dH = np.einsum("ge,gije->gij", c1, tb1.reshape(batch.G, nS, nS, a2)) \
            + np.einsum("ge,gije->gij", c2, tb2.reshape(batch.G, nS, nS, a4))
        hb = hb + nS * (dH.max(axis=(1, 2)) + (a4 + a2 + 4) * U * (c0 + c1.sum(axis=1) * 2 + c2.sum(axis=1) * 6))
    err = np.abs(sides[0][0] - sides[1][0])
    emax, ratio = worst(err, bound)
    res = np.abs(sides[0][2] - sides[1][2]).max(axis=1)
    moved = np.abs(sides[0][1] - sides[1][1]).max()
    print(f"{name} {kind}: E_SA and gradient under R: largest difference {emax:.2e}, largest bound {bound.max():.2e}, "
          f"largest difference / bound {ratio:.3f}; resolved energies {res.max():.2e} (bound {np.max(hb):.2e}); "
          f"state energies moved by {moved:.2e}")
    assert ratio <= 1.0
    assert np.all(res <= hb)
    assert moved > 1e-3


# ---- 6. / 7. the ensemble variational principle on H4 ---------------------------------------------------------------
def h4_coords():
    """three slightly different, unsymmetric H4 chains [3, 4, 3] in Angstrom"""
    out = np.zeros((3, 4, 3))
    for g, s in enumerate((0.0, 0.03, -0.02)):
        out[g, :, 0] = [0.0, 0.95 + s, 2.05 + 2 * s, 2.95 + s]
    return out


def h4_stack():
    basis = gto.GTOBasis(["H"] * 4)
    pqc = circuit("cas22_fabric1")
    # (active-active rotations frozen, as in the optimisation test of tests/test_api_gpu.py: in CAS(2e,2o) the one
    # active-active rotation does what the circuit's OrbitalRotation parameter does)
    batch = aoo.OO_pqc_batch.from_geometries(pqc, basis, h4_coords(), 2, 2, oao_mo_coeffs="rhf", freeze_active=True)
    return batch, aoo.SA_OO_pqc_batch(batch, aoo.StateEnsemble(pqc, nstates=2))


def theta_only_minimum(sa):
    nt = sa.n_theta
    th = torch.zeros((sa.G, nt), dtype=F64, device=dev())
    for it in range(30):
        E, g, H = sa.energy_gradient_hessian(th)
        if g[:, :nt].abs().max().item() < 1e-7:
            return th, E, it
        th = th - torch.linalg.solve(H[:, :nt, :nt].cpu(), g[:, :nt].cpu()).to(dev())
    raise AssertionError("the theta-only Newton iteration did not reach max |dE/dtheta| < 1e-7 in 30 steps")


def test_theta_only_minimum_is_the_mean_of_the_two_singlet_roots():
    """H4 / STO-3G, CAS(2e,2o), singlet_states(nstates=2) with equal weights, np_fabric with n_layers = 1 -- the
    smallest that reaches the mean: on the host, with the oracle's integrals and the twin, plain Newton steps from
    theta = 0 reach max |dE/dtheta| < 1e-7 in 3 steps at every one of the three chains and end within 5e-16 of the
    mean of the two lowest singlet roots (the 2-planes of the 3-dimensional singlet space are a 2-parameter family,
    and the circuit has 2 parameters)."""
    batch, sa = h4_stack()
    th, E, it = theta_only_minimum(sa)
    roots, _ = batch.casci(nroots=2, fix_singlet=True)
    res, Umat = sa.resolve(th)
    d_mean = (E - roots.mean(dim=1)).abs().max().item()
    d_res = np.abs(res - roots.cpu().numpy()).max()
    print(f"H4: {it} Newton steps; |E_SA - mean of the roots| {d_mean:.2e}; |resolved - roots| {d_res:.2e}")
    assert d_mean < 1e-9 and d_res < 1e-9
    # the sign convention: the largest component of every eigenvector is positive
    assert np.all(np.take_along_axis(Umat, np.abs(Umat).argmax(axis=1)[:, None, :], axis=1) > 0)


def test_full_optimization_over_theta_and_kappa():
    batch, sa = h4_stack()
    th0, E0, _ = theta_only_minimum(sa)
    energies, th = sa.full_optimization(torch.zeros_like(th0), max_iterations=50, conv_tol=1e-10)
    assert energies.shape[1] == 3 and 2 <= energies.shape[0] <= 51
    assert np.all(energies[1:] <= energies[:-1] + 1e-10)
    assert np.abs(energies[-1] - energies[-2]).max() < 1e-10
    E, g, H = sa.energy_gradient_hessian(th)
    low = torch.linalg.eigvalsh(H.cpu())[:, 0]
    # the oracle's ensemble energy at the final parameters and orbitals
    psi0, w = sa.ensemble.states_host, sa.ensemble.weights_host
    S_, h_, g_ = batch.overlap.cpu().numpy(), batch.int1e_ao.cpu().numpy(), batch.int2e_ao.cpu().numpy()
    ref = []
    for k in range(3):
        P = dict(int1e_ao=h_[k], int2e_ao=g_[k], overlap=S_[k], nuc=float(batch.nuc[k].item()))
        f, nk = oracle_energy("cas22_fabric1", P, 4, psi0, w, oao_mo_coeff=batch.oao_mo_coeff[k].cpu().numpy())
        ref.append(f(torch.cat((th[k].cpu(), torch.zeros(nk, dtype=F64)))).item())
    d = np.abs(E.cpu().numpy() - np.array(ref)).max()
    print(f"H4 full optimisation: {energies.shape[0] - 1} steps, max |grad| {g.abs().max().item():.2e}, lowest Hessian "
          f"eigenvalue {low.min().item():.2e}, |E_SA - oracle| {d:.2e}, E_SA - theta-only minimum "
          f"{(E - E0).max().item():.2e}")
    assert g.abs().max().item() < 1e-6 and low.min().item() > -1e-8
    assert d < 1e-9
    assert np.abs(E.cpu().numpy() - energies[-1]).max() < 1e-9
    assert bool((E <= E0 + 1e-10).all())


# ---- 8. nuclear gradient ---------------------------------------------------------------------------------------------
def test_nuclear_gradient_against_finite_differences():
    """dE_SA/dR of the first H4 chain at seeded theta and orbitals rotated away from RHF, against the 4th-order central
    difference of SA_OO_pqc_batch.energy over displaced stacks with the same theta and oao_mo_coeff in every copy;
    h = 1e-3 and 2e-3 Bohr, the bound 10 x the disagreement of the two (tests/test_nucgrad_gpu.py)."""
    basis = gto.GTOBasis(["H"] * 4)
    pqc = circuit("cas22_fabric1")
    xyz = h4_coords()[0] / BOHR
    b0 = aoo.OO_pqc_batch.from_geometries(pqc, basis, xyz[None] * BOHR, 2, 2, oao_mo_coeffs="rhf")
    rng = np.random.default_rng(23)
    K = rng.standard_normal((4, 4))
    K = 0.1 * (K - K.T) / np.linalg.norm(K - K.T)
    Uo = b0.oao_mo_coeff[0].cpu().numpy() @ scipy.linalg.expm(K)
    theta = rng.uniform(-1.0, 1.0, (1, 2))
    ens = aoo.StateEnsemble(pqc, nstates=2, weights=(0.7, 0.3))
    res = []
    for h in (1e-3, 2e-3):
        stack = fd_stack(xyz, h)
        b = aoo.OO_pqc_batch.from_geometries(pqc, basis, stack * BOHR, 2, 2, oao_mo_coeffs=[Uo] * len(stack))
        e = aoo.SA_OO_pqc_batch(b, ens).energy(to_dev(np.repeat(theta, len(stack), axis=0)))
        res.append(fd_combine(e.reshape(1, -1), h).cpu().numpy()[0])
    dis = np.abs(res[0] - res[1]).max()
    b = aoo.OO_pqc_batch.from_geometries(pqc, basis, xyz[None] * BOHR, 2, 2, oao_mo_coeffs=[Uo])
    sa = aoo.SA_OO_pqc_batch(b, ens)
    grad = sa.nuclear_gradient(to_dev(theta))
    err = np.abs(grad[0].cpu().numpy() - res[0]).max()
    print(f"H4 ensemble nuclear gradient: max |grad| {np.abs(res[0]).max():.3g}, reference disagreement {dis:.2e}, "
          f"bound {10 * dis:.2e}, error {err:.2e}")
    assert tuple(grad.shape) == (1, 4, 3)
    assert err < 10 * dis
    assert torch.equal(sa.nuclear_gradient(to_dev(theta), index=[0], chunk=1), grad)


# ---- 9. refusals -----------------------------------------------------------------------------------------------------
def test_refusals():
    big = aoo.Parameterized_circuit(8, 8, None, ansatz="kupccd", k=1)
    with pytest.raises(NotImplementedError, match="10 qubits"):
        aoo.StateEnsemble(big)
    batch, _ = synthetic_batch("cas22_fabric1")
    sa = aoo.SA_OO_pqc_batch(batch, aoo.StateEnsemble(circuit("cas22_fabric1")))
    bad = torch.zeros((batch.G + 1, batch.n_theta), dtype=F64, device=dev())
    for call in (sa.energy, sa.energy_and_gradient, sa.energy_gradient_hessian, sa.rdms, sa.hamiltonian,
                 sa.damped_newton_step, sa.full_optimization, sa.resolve):
        with pytest.raises(ValueError, match="thetas of shape"):
            call(bad)
    with pytest.raises(ValueError, match="another circuit"):
        aoo.SA_OO_pqc_batch(batch, aoo.StateEnsemble(circuit("cas43_ucc")))
    lib = _lib.load()
    assert lib.oovqe_ensemble_states(None, 1, None, 1, 12, None, 2, None, 0, 1, None, None) != 0
    assert "OOVQE_ENSEMBLE_MAX_QUBITS = 10" in lib.oovqe_last_error().decode()
