"""The host twin of the dense-register kernels (tests/_circuit_scope.py) earns its trust here, without a device:
  * its fp64 arithmetic against its own longdouble arithmetic, within half of every bound the device tests use (the
    factor 2 of the bounds leaves one share for the twin);
  * against independent host code: the gate-level simulator and the Jordan-Wigner matrices of oracle.cpu_ref at 4 to
    8 qubits, and the sector twin of tests/_sector_scope.py scattered into the register;
  * identities: Gamma symmetries, traces to the electron number, spin-summed spin RDMs = restricted RDMs;
  * its tangents and second tangents against central differences of the longdouble twin, the tolerance being the
    truncation plus the rounding term of the quotient, both computed here;
  * sensitivity: on the cases of the device tables every planted defect moves a compared quantity by more than 1000
    bounds.  A defect is planted where its operation exists: the first-gate-only tangent in lists with a parameter
    that drives several gates, the Jordan-Wigner sign and the p/q swap from two orbitals on (one orbital has E_00
    alone: no sign, nothing to swap), the batch defects from two elements on."""
import itertools

import numpy as np
import pytest
import torch

from oracle import cpu_ref as R
from tests import _circuit_scope as C
from tests import _sector_scope as S

LD = C.LD
EPS_LD = float(np.finfo(LD).eps)
FACTOR = 1000.0


def f64(x):
    return np.asarray(x, dtype=np.float64)


def norm(x):
    return float(np.linalg.norm(f64(x)))


def within_half(what, got, ref, bound):
    err = np.abs(f64(np.asarray(got, dtype=LD) - ref))
    assert (err <= 0.5 * np.asarray(bound)).all(), \
        f"{what}: fp64 twin off its longdouble twin by {err.max():.3e}, half bound {0.5 * float(np.max(bound)):.3e}"


def shared_lists(case_kind, n):
    gates, n_theta, _ = C.gate_list(case_kind, n)
    return [k for k, own in enumerate(S.param_gates(gates, n_theta)) if len(own) > 1]


# ---- fp64 twin against longdouble twin -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.STATE_CASES, ids=C.state_id)
def test_states_fp64_against_longdouble(case):
    th, psi, dpsi = C.state_reference(case)
    _, psi_l, dpsi_l = C.state_reference(case, dtype=LD)
    es, tb = C.state_bounds(case, dpsi)
    for b in range(psi.shape[0]):
        assert norm(np.asarray(psi[b], dtype=LD) - psi_l[b]) <= 0.5 * es
        for k in range(dpsi.shape[1]):
            assert norm(np.asarray(dpsi[b, k], dtype=LD) - dpsi_l[b, k]) <= 0.5 * tb[b, k], (b, k)
    gates, n_theta, _ = C.gate_list(case[1], case[0])
    for k, own in enumerate(S.param_gates(gates, n_theta)):
        if not own:
            assert not dpsi[:, k].any() and not dpsi_l[:, k].any()      # a parameter with no gate: exactly zero


@pytest.mark.parametrize("ncas", range(1, 8))
@pytest.mark.parametrize("same", [True, False])
def test_rdms_fp64_against_longdouble(ncas, same):
    for i in range(3):                       # the three kinds of vectors; further pairs are dense again
        _, _, g1, g2, b1, b2 = C.rdm_reference(ncas, i, same)
        _, _, l1, l2, _, _ = C.rdm_reference(ncas, i, same, LD)
        within_half(f"gamma[{i}]", g1, l1, b1)
        within_half(f"Gamma[{i}]", g2, l2, b2)


@pytest.mark.parametrize("ncas", range(1, 8))
def test_rdm_tangent_sets_fp64_against_longdouble(ncas):
    for b in range(2):
        g1, g2, b1, b2 = C.rdm_tangent_reference(ncas, b, 5)
        l1, l2, _, _ = C.rdm_tangent_reference(ncas, b, 5, LD)
        within_half("d gamma", g1, l1, b1)
        within_half("d Gamma", g2, l2, b2)


@pytest.mark.parametrize("n,batch", [c for c in C.SPIN_CASES if c[1] == 3])
def test_spin_rdms_fp64_against_longdouble(n, batch):
    for i in range(batch):
        _, _, g1, g2, b1, b2 = C.spin_reference(n, i)
        _, _, l1, l2, _, _ = C.spin_reference(n, i, LD)
        within_half("spin gamma", g1, l1, b1)
        within_half("spin Gamma", g2, l2, b2)


@pytest.mark.parametrize("ncas,kind", C.HESSIAN_CASES)
def test_hessian_fp64_against_longdouble(ncas, kind):
    _, _, _, H, B = C.hessian_reference(ncas, kind)
    _, _, _, Hl, _ = C.hessian_reference(ncas, kind, LD)
    assert np.array_equal(H, H.T)
    within_half("H", H, Hl, B)


# ---- against independent host code -----------------------------------------------------------------------------------
ORACLE_TOL = 1e-12      # the gate-level simulator multiplies ~150 complex 2 x 2 gates per excitation: ~1e-14 of error


@pytest.mark.parametrize("ncas", [2, 3, 4])
@pytest.mark.parametrize("kind", ["kupccd", "uccsd", "fabric"])
def test_states_and_rdms_against_the_oracle(ncas, kind):
    n = 2 * ncas
    gates, n_theta, init = C.gate_list(kind, n)
    theta = C.thetas(f"oracle{ncas}{kind}", 1, n_theta)[0]
    tt = torch.tensor(theta)
    if kind == "kupccd":
        ref = R.kupccd_state(tt, ncas, 2 * (ncas // 2))
    elif kind == "uccsd":
        ref = R.uccd_state(tt, ncas, C.UCCSD_ELECTRONS[n], add_singles=True)
    else:
        ref = R.gatefabric_state(tt, ncas, C.FABRIC_ELECTRONS[n], 2)
    ref = np.asarray(ref)
    assert np.abs(ref.imag).max() <= ORACLE_TOL
    psi = C.apply_gates(gates, theta, n, init)
    assert np.abs(psi - ref.real).max() <= ORACLE_TOL
    g1, g2 = C.register(ncas).rdms(psi, psi)
    o1, o2 = R.rdms_from_state(torch.tensor(psi), R.RdmOperators(ncas))
    assert np.abs(g1 - o1.numpy()).max() <= ORACLE_TOL and np.abs(g2 - o2.numpy()).max() <= ORACLE_TOL
    s1, s2 = C.spin_rdms(psi, psi, n)
    p1, p2 = R.spin_rdms_from_state(torch.tensor(psi), ncas)
    assert np.abs(s1 - p1.numpy()).max() <= ORACLE_TOL and np.abs(s2 - p2.numpy()).max() <= ORACLE_TOL


@pytest.mark.parametrize("ncas,na,nb,kind", [(2, 1, 1, "ladder"), (3, 2, 1, "uccsd"), (4, 2, 2, "kupccd"),
                                             (5, 2, 2, "uccsd"), (6, 3, 3, "fabric"), (7, 3, 3, "ladder")])
def test_against_the_sector_twin(ncas, na, nb, kind):
    """states, tangents and RDMs of a number-conserving list: the sector twin scattered into the register."""
    sec = S.Sector(ncas, na, nb)
    gates, n_theta = S.circuit(kind, ncas, na, nb)
    init = C.X.basis_index(sec.occupation())
    theta = C.thetas(f"sector{ncas}{kind}", 1, n_theta)[0]
    n, reg = 2 * ncas, C.register(ncas)

    def scatter(v):
        out = np.zeros(1 << n)
        out[sec.x] = v
        return out

    es = C.state_bound(gates)
    psi = C.apply_gates(gates, theta, n, init)
    assert norm(psi - scatter(S.apply_gates(gates, theta, sec, init)[0])) <= es
    own = S.param_gates(gates, n_theta)
    for k in range(0, n_theta, max(1, n_theta // 6)):
        tau = C.tangent(gates, theta, n, init, k, n_theta)
        assert norm(tau - scatter(S.tangent(gates, theta, sec, init, k, n_theta))) <= C.tangent_bound(gates, len(own[k]), tau)
    for seed in (1, 2):
        v = S.make_vectors(sec, seed, 3)[seed]
        g1, g2 = reg.rdms(scatter(v), scatter(v))
        r1, r2 = sec.rdms(v)
        b1, b2 = C.rdm_bounds(reg, scatter(v), scatter(v))
        assert (np.abs(g1 - r1) <= b1).all() and (np.abs(g2 - r2) <= b2).all()


# ---- identities ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncas,kind", [(2, "fabric"), (3, "uccsd"), (4, "kupccd"), (5, "fabric"), (6, "ladder")])
def test_rdm_identities_of_number_conserving_states(ncas, kind):
    n = 2 * ncas
    gates, n_theta, init = C.gate_list(kind, n)
    psi = C.apply_gates(gates, C.thetas(f"id{ncas}{kind}", 1, n_theta)[0], n, init)
    nel = bin(init).count("1")
    reg = C.register(ncas)
    g1, g2 = reg.rdms(psi, psi)
    b1, b2 = C.rdm_bounds(reg, psi, psi)
    assert (np.abs(g2 - g2.transpose(2, 3, 0, 1)) <= b2 + b2.transpose(2, 3, 0, 1)).all()      # (pq) <-> (rs)
    assert (np.abs(g2 - g2.transpose(1, 0, 3, 2)) <= b2 + b2.transpose(1, 0, 3, 2)).all()      # real bra = ket
    assert (np.abs(g1 - g1.T) <= b1 + b1.T).all()
    assert abs(np.trace(g1) - nel) <= np.trace(b1) + 16 * C.state_bound(gates)
    assert abs(np.einsum("pprr->", g2) - nel * (nel - 1)) <= np.einsum("pprr->", b2) + 16 * nel * C.state_bound(gates)


@pytest.mark.parametrize("ncas", [1, 2, 3, 4])
def test_spin_summed_spin_rdms_are_the_restricted_rdms(ncas):
    n = 2 * ncas
    bra, ket = C.make_pairs(1 << n, 77 + ncas, 3, False)
    for i in range(3):
        g1, g2 = C.spin_summed(*C.spin_rdms(bra[i], ket[i], n))
        r1, r2 = C.register(ncas).rdms(bra[i], ket[i])
        b1, b2 = C.rdm_bounds(C.register(ncas), bra[i], ket[i])
        assert (np.abs(g1 - r1) <= b1).all() and (np.abs(g2 - r2) <= b2).all()


# ---- tangents against central differences of the longdouble twin -----------------------------------------------------
FD_CASES = [c for c in C.STATE_CASES if c[0] <= 8 and c[3] == 1] + [(14, "hand", "hf", 1)]


def _quotient(f, theta, k, m3, e_r):
    """central difference of f along theta_k in longdouble: step h balancing the truncation h^2 M3 / 6 (M3 bounds the
    third derivative) against the rounding e_r / h (e_r bounds the error of one value of f); -> (quotient, tolerance)."""
    h = (3.0 * e_r / m3) ** (1.0 / 3.0)
    tp, tm = np.asarray(theta, dtype=LD).copy(), np.asarray(theta, dtype=LD).copy()
    tp[k] += LD(h)
    tm[k] -= LD(h)
    step = tp[k] - tm[k]
    return (f(tp) - f(tm)) / step, h * h * m3 / 6.0 + e_r / h


@pytest.mark.parametrize("case", FD_CASES, ids=C.state_id)
def test_tangents_against_central_differences(case):
    n, kind = case[0], case[1]
    gates, n_theta, _ = C.gate_list(kind, n)
    init = C.start_index(case)
    th = C.state_reference(case)[0][0]
    own = S.param_gates(gates, n_theta)
    e_state = 8.0 * S.n_rotations(gates) * EPS_LD          # the state bound at the longdouble unit
    for k in range(n_theta):
        m = max(len(own[k]), 1)
        # each theta_k-derivative of psi is a sum of m terms of norm <= 1/2
        q, tol = _quotient(lambda t: C.apply_gates(gates, t, n, init, (), LD), th, k, (0.5 * m) ** 3, e_state)
        tau = C.tangent(gates, th, n, init, k, n_theta, LD)
        assert norm(tau - q) <= tol, (k, norm(tau - q), tol)
        assert tol < 1e-9
    for j, k in itertools.islice(itertools.combinations_with_replacement(range(n_theta), 2), 0, None, 3):
        mj, mk = max(len(own[j]), 1), max(len(own[k]), 1)
        q, tol = _quotient(lambda t: C.tangent(gates, t, n, init, j, n_theta, LD), th, k,
                           0.5 * mj * (0.5 * mk) ** 3, mj * e_state)
        t2 = C.second_tangent(gates, th, n, init, j, k, n_theta, LD)
        assert norm(t2 - q) <= tol, (j, k, norm(t2 - q), tol)


# ---- sensitivity -------------------------------------------------------------------------------------------------------
def moved(ref, mutated, bound):
    """does any compared quantity move by more than FACTOR bounds?  (2-norms against a scalar bound, or elementwise)"""
    d = np.abs(f64(ref) - f64(mutated))
    return bool((d > FACTOR * np.asarray(bound)).any())


def norms(d):
    return np.linalg.norm(d, axis=-1)


# Cases that cannot see a defect by their structure.  Each is a shape the scope names (kUpCCD and the singles ladders
# exist at 4 qubits only in this form) and stays as an extra next to a case of the same register that does see the
# defect (asserted below); every other case must see every defect planted in it.
#   4 qubits, two electrons: the sector has four determinants; every single touches all four and the one double is
#   the first gate, applied to the start determinant alone -- no differentiated gate ever has an untouched amplitude.
BLIND_STATES = {"q4_kupccd_hf_b1": {"annihilate"}, "q4_uccsd_hf_b3": {"annihilate"}, "q4_ladder_hf_b1": {"annihilate"},
                "q4_ladder_shared_hf_b3": {"annihilate"}}


def state_defects_seen(case):
    n, kind, _, batch = case
    th, psi, dpsi = C.state_reference(case)
    es, tb = C.state_bounds(case, dpsi)
    seen = {}
    _, _, no_kill = C.state_reference(case, annihilate=False)
    seen["annihilate"] = bool((norms(dpsi - no_kill) > FACTOR * tb).any())
    if shared_lists(kind, n):
        _, _, first = C.state_reference(case, first_only=True)
        seen["first_only"] = bool((norms(dpsi - first) > FACTOR * tb).any())
    if batch > 1:
        seen["batch"] = bool((norms(psi[1:] - psi[0]) > FACTOR * es).all()
                             and all((norms(dpsi[b] - dpsi[0]) > FACTOR * tb[b]).any() for b in range(1, batch)))
    return seen


@pytest.mark.parametrize("case", C.STATE_CASES, ids=C.state_id)
def test_state_cases_detect_the_planted_defects(case):
    seen = state_defects_seen(case)
    assert {d for d, hit in seen.items() if not hit} == BLIND_STATES.get(C.state_id(case), set()), seen


def test_blind_state_cases_stand_next_to_seeing_ones():
    for cid, defects in BLIND_STATES.items():
        case = next(c for c in C.STATE_CASES if C.state_id(c) == cid)
        for d in defects:
            assert any(state_defects_seen(c).get(d) for c in C.STATE_CASES if c[0] == case[0]), (cid, d)


@pytest.mark.parametrize("route", ["small", "lds", "global"])
def test_every_route_has_a_shared_parameter_that_matters(route):
    """a parameter that drives several gates whose first-gate-only tangent is at least 0.1 away in 2-norm: in the
    one-workgroup kernel (CIRCUIT_RDMS_CASES), the LDS-resident and the global-memory register (STATE_CASES)."""
    worst = 0.0
    if route == "small":
        for ncas, kind, small in C.CIRCUIT_RDMS_CASES:
            if small and shared_lists(kind, 2 * ncas):
                full = C.circuit_rdms_reference(ncas, kind, 0)[1]
                first = C.circuit_rdms_reference(ncas, kind, 0, first_only=True)[1]
                worst = max(worst, norms(full - first).max())
    else:
        for case in C.STATE_CASES:
            if C.route(case[0]) == route and shared_lists(case[1], case[0]):
                worst = max(worst, norms(C.state_reference(case)[2] - C.state_reference(case, first_only=True)[2]).max())
    assert worst >= 0.1, worst


def test_the_named_case_has_eleven_shared_parameters_that_matter():
    case = next(c for c in C.STATE_CASES if c[:2] == (14, "fabric"))
    full, first = C.state_reference(case)[2][0], C.state_reference(case, first_only=True)[2][0]
    d = norms(full - first)
    shared = shared_lists("fabric", 14)
    far = [k for k in shared if d[k] >= 0.1]
    # nine of the eleven: the other two rotate orbital pairs that are both empty when their block acts (first layer,
    # wires 8 to 13 of the six-electron start), so both of their gates meet zero amplitudes and the tangent is zero
    assert len(shared) == 11 and len(far) == 9 and all(not full[k].any() for k in shared if k not in far), d


RDM_DEFECTS = [{"jw": False}, {"swap": True}, {"delta": False}]


def rdm_defects(ncas):
    return RDM_DEFECTS if ncas >= 2 else [{"delta": False}]


@pytest.mark.parametrize("ncas,batch,same", C.RDM_CASES)
def test_rdm_cases_detect_the_planted_defects(ncas, batch, same):
    reg = C.register(ncas)
    refs = [C.rdm_reference(ncas, i, same) for i in range(batch)]
    for defect in rdm_defects(ncas):
        hit = False
        for bra, ket, g1, g2, b1, b2 in refs[:3]:
            m1, m2 = reg.rdms(bra, ket, **defect)
            hit = hit or moved(g1, m1, b1) or moved(g2, m2, b2)
        assert hit, defect
    for i in range(1, batch):               # element i reading the vectors of element 0
        assert moved(refs[i][2], refs[0][2], refs[i][4]) or moved(refs[i][3], refs[0][3], refs[i][5]), i


@pytest.mark.parametrize("ncas,n_tan,batch", C.RDM_TANGENT_CASES)
def test_rdm_tangent_cases_detect_the_planted_defects(ncas, n_tan, batch):
    reg = C.register(ncas)
    refs = [C.rdm_tangent_reference(ncas, b, n_tan) for b in range(batch)]
    for defect in rdm_defects(ncas):
        hit = False
        for b in range(batch):
            psi, dpsi = C.tangent_vectors(ncas, b)
            m1, m2 = reg.rdms_tangent(psi, dpsi[:n_tan], **defect)
            hit = hit or moved(refs[b][0], m1, refs[b][2]) or moved(refs[b][1], m2, refs[b][3])
        assert hit, defect
    if batch > 1:
        assert moved(refs[1][0], refs[0][0], refs[1][2]) or moved(refs[1][1], refs[0][1], refs[1][3])


# 4 qubits, two electrons, singles only: see BLIND_STATES; the GateFabric case of the same size sees the defect.
BLIND_CIRCUIT_RDMS = {(2, "ladder_shared"): {"annihilate"}}
# kUpCCD states and all their tangents hold doubly occupied determinants only; between two of them every surviving
# term of gamma and Gamma moves a whole pair or none, and the Jordan-Wigner signs of the two spins cancel.  The
# UCCSD and GateFabric cases see the sign.
BLIND_HESSIANS = {(4, "kupccd"): {"jw"}}


def name(defect):
    return next(iter(defect))


@pytest.mark.parametrize("ncas,kind,small", C.CIRCUIT_RDMS_CASES)
def test_circuit_rdms_cases_detect_the_planted_defects(ncas, kind, small):
    """compared there: psi, the tangents, the RDM sets."""
    reg = C.register(ncas)
    psi, dpsi, g1, g2, b1, b2, es, tb = C.circuit_rdms_reference(ncas, kind, 0)
    seen = {}
    for defect in rdm_defects(ncas):
        m1, m2 = reg.rdms_tangent(psi, dpsi, **defect)
        seen[name(defect)] = moved(g1, m1, b1) or moved(g2, m2, b2)
    tangent_defects = [{"annihilate": False}] + ([{"first_only": True}] if shared_lists(kind, 2 * ncas) else [])
    for defect in tangent_defects:
        m = C.circuit_rdms_reference(ncas, kind, 0, **defect)
        seen[name(defect)] = bool((norms(dpsi - m[1]) > FACTOR * tb).any()) or moved(g1, m[2], b1) or moved(g2, m[3], b2)
        if ncas >= 2 and seen[name(defect)]:        # ... and then in the derivative sets as well
            assert moved(g1, m[2], b1) or moved(g2, m[3], b2), defect
    other = C.circuit_rdms_reference(ncas, kind, 1)
    seen["batch"] = norm(other[0] - psi) > FACTOR * es and (moved(other[2], g1, other[4]) or moved(other[3], g2, other[5]))
    assert {d for d, hit in seen.items() if not hit} == BLIND_CIRCUIT_RDMS.get((ncas, kind), set()), seen
    for d in BLIND_CIRCUIT_RDMS.get((ncas, kind), set()):
        assert any(c[0] == ncas and c[1] != kind for c in C.CIRCUIT_RDMS_CASES)


@pytest.mark.parametrize("ncas,kind", C.HESSIAN_CASES)
def test_hessian_cases_detect_the_planted_defects(ncas, kind):
    th, c1, c2, H, B = C.hessian_reference(ncas, kind)
    gates, n_theta, init, _ = C.circuit_case(ncas, kind, 1)
    defects = [{"rdm_defect": d} for d in rdm_defects(ncas)] + [{"tangent_defect": {"annihilate": False}}]
    if shared_lists(kind, 2 * ncas):
        defects.append({"tangent_defect": {"first_only": True}})
    seen = {name(planted): moved(H, C.hessian(gates, th, ncas, init, c1, c2, n_theta, **{which: planted}), B)
            for defect in defects for which, planted in defect.items()}
    assert {d for d, hit in seen.items() if not hit} == BLIND_HESSIANS.get((ncas, kind), set()), seen


@pytest.mark.parametrize("n,batch", C.SPIN_CASES)
def test_spin_cases_detect_the_planted_defects(n, batch):
    refs = [C.spin_reference(n, i) for i in range(batch)]
    if n >= 2:          # one spin orbital has no Jordan-Wigner sign
        hit = False
        for bra, ket, g1, g2, b1, b2 in refs:
            m1, m2 = C.spin_rdms(bra, ket, n, jw=False)
            hit = hit or moved(g1, m1, b1) or moved(g2, m2, b2)
        assert hit
    for i in range(1, batch):
        assert moved(refs[i][2], refs[0][2], refs[i][4]) or moved(refs[i][3], refs[0][3], refs[i][5])


# ---- the case tables ---------------------------------------------------------------------------------------------------
def test_the_tables_cover_what_they_claim():
    qubits = {c[0] for c in C.STATE_CASES}
    assert qubits == {2, 3, 4, 5, 6, 8, 10, 12, 13, 14, 15}
    assert {C.route(n) for n in qubits} == {"lds", "global"} and C.route(13) == "lds" and C.route(14) == "global"
    assert {c[2] for c in C.STATE_CASES} == {"hf", "0", "D-1"}
    assert {c[3] for c in C.STATE_CASES if c[0] <= 8} >= {1, 3, 33} and (14, "fabric", "hf", 2) in C.STATE_CASES
    for n in qubits:
        gates, n_theta = C.hand_gates(n)
        own = S.param_gates(gates, n_theta)
        assert len(own[0]) == 3 and all(b - a > 1 for a, b in zip(own[0], own[0][1:])) and own[2] == []
        assert {int(g.sign) for g in gates} == {1, -1} and any(g.theta_idx < 0 for g in gates)
        assert {int(g.nfix) for g in gates} == ({2, 4} if n >= 4 else {2})
        fixed = [int(g.mask_hi | g.mask_lo) for g in gates]
        assert any(f & 1 for f in fixed) and any(f >> (n - 1) & 1 for f in fixed)
        if n >= 3:
            assert any(int(g.mask_par) == ((1 << (n - 1)) - 2) for g in gates)
    for case in C.STATE_CASES:
        th = C.state_reference(case)[0]
        assert (np.abs(th) <= C.TWO_PI).all() and (th.size < 3 or ((th == 0.0).any() and (th == np.pi).any()))
        assert len({tuple(t) for t in th}) == len(th)
    gates, n_theta, _ = C.gate_list("fabric", 14)
    assert (len(gates), n_theta) == (36, 22) and any(g.theta_idx < 0 for g in C.gate_list("fabric", 8)[0])
