"""The host twin of the sector engine (tests/_sector_scope.py) against everything independent of it: the oracle's
circuits and RDM operators (oracle/cpu_ref.py) at ncas <= 4, the full-register gate emulation (tests/_emulate.py) up
to 16 qubits including unequal sectors, the dense E_pq of tests/_ci_dense.py where N_alpha = N_beta, a brute-force
Fock-space a^+_P a_Q over occupation tuples for unequal and empty sectors, central differences of the twin's own
energy for the adjoint and Hessian formulas, and its np.longdouble versions (the fp64 twin stays within HALF of each
device bound).  Then the device case tables of tests/test_sector_scope_gpu.py: a replica of the entry points'
dispatch arithmetic (MT / NT, the LDS formulas, mp = ceil(max_pairs / 512), nit = ceil(Dc / 1024), the batch
thresholds; 256 CUs assumed where the count matters) shows that every case reaches the instance it names and that
every reachable instance is named."""
import itertools

import numpy as np
import pytest
import torch

from auto_oo_amd import excitations as X
from oracle import cpu_ref as R
from tests import _ci_dense, _emulate
from tests import _sector_scope as S


def _oracle(ncas, nelecas, kind):
    if kind == "kupccd":
        return R.OraclePQC(ncas, nelecas, "kupccd", k=1), X.kupccd_gates(ncas, 1)
    if kind == "np_fabric":
        return R.OraclePQC(ncas, nelecas, "np_fabric", n_layers=2), X.gatefabric_gates(ncas, nelecas, 2)
    return (R.OraclePQC(ncas, nelecas, "ucc", add_singles=kind == "uccsd"),
            X.uccd_gates(ncas, nelecas, kind == "uccsd"))


@pytest.mark.parametrize("ncas,nelecas,kind", [(2, 2, "ucc"), (3, 4, "ucc"), (3, 3, "uccsd"), (3, 4, "uccsd"),
                                               (4, 4, "kupccd"), (4, 3, "uccsd"), (3, 2, "np_fabric"),
                                               (4, 4, "np_fabric"), (4, 5, "np_fabric")])
def test_twin_states_and_rdms_equal_the_oracle(ncas, nelecas, kind):
    pqc, (gates, n_theta) = _oracle(ncas, nelecas, kind)
    hf = X.hf_state(nelecas, 2 * ncas)
    sec = S.Sector(ncas, int(hf[0::2].sum()), int(hf[1::2].sum()))
    theta = np.random.default_rng(ncas + nelecas).uniform(0, 2 * np.pi, n_theta)
    psi, _ = S.apply_gates(gates, theta, sec, X.basis_index(hf))
    ref = pqc.qnode(torch.tensor(theta)).real.numpy()
    assert np.abs(ref[sec.x] - psi).max() < 1e-13 and abs(np.linalg.norm(ref) - np.linalg.norm(psi)) < 1e-13
    g1, g2 = sec.rdms(psi)
    r1, r2 = pqc.get_rdms(torch.tensor(theta))
    assert np.abs(g1 - r1.numpy()).max() < 1e-12 and np.abs(g2 - r2.numpy()).max() < 1e-12   # (the oracle's own error)


@pytest.mark.parametrize("ncas,na,nb,kind", [(3, 2, 1, "uccsd"), (4, 1, 3, "ladder"), (4, 0, 2, "ladder"),
                                             (5, 2, 1, "uccsd"), (6, 3, 2, "uccsd"), (6, 3, 3, "fabric"),
                                             (7, 2, 3, "ladder"), (8, 4, 4, "kupccd"), (8, 3, 5, "ladder"),
                                             (8, 8, 1, "ladder")])
def test_twin_states_equal_the_full_register_emulation(ncas, na, nb, kind):
    sec = S.Sector(ncas, na, nb)
    gates, n_theta = S.circuit(kind, ncas, na, nb)
    init = X.basis_index(sec.occupation())
    theta = np.random.default_rng(7 * ncas + na).uniform(0, 2 * np.pi, n_theta)
    psi, counts = S.apply_gates(gates, theta, sec, init)
    ref = _emulate.apply_gate_table(gates, theta, 2 * ncas, init)
    assert np.array_equal(ref[sec.x], psi)                    # the same arithmetic on the same pairs
    assert np.count_nonzero(ref) == np.count_nonzero(psi)     # nothing outside the sector
    x = np.arange(1 << (2 * ncas))
    inside = np.zeros(len(x), dtype=bool)
    inside[sec.x] = True
    for g, n in zip(gates, counts):
        sel = (x & (g.mask_hi | g.mask_lo)) == g.mask_hi
        assert n == (np.count_nonzero(sel & inside) if g.theta_idx >= 0 else 0)


@pytest.mark.parametrize("ncas,nelecas", [(2, 2), (4, 4), (5, 4), (6, 6)])
def test_twin_epq_equals_the_dense_excitation_matrices(ncas, nelecas):
    sec = S.Sector(ncas, nelecas // 2, nelecas // 2)
    E = _ci_dense.excitation_matrices(ncas, nelecas)
    v = S.dense_vector(sec, 3)
    V = sec.apply_epq(v).reshape(ncas, ncas, -1)
    assert np.abs(V - np.einsum("pqij,j->pqi", E, v)).max() < 1e-14


def _fock_epq(ncas, na, nb):
    """E_pq by brute force over occupation tuples of the whole Fock space: a_Q then a^+_P, each with the sign of the
    occupied spin orbitals in front of it."""
    n = 2 * ncas
    sec = S.Sector(ncas, na, nb)
    dets = {tuple(int(b) for b in format(int(x), f"0{n}b")): c for c, x in enumerate(sec.x)}
    E = np.zeros((ncas, ncas, sec.Dc, sec.Dc))
    for occ, c in dets.items():
        for p, q, sp in itertools.product(range(ncas), range(ncas), (0, 1)):
            P, Q = 2 * p + sp, 2 * q + sp
            o = list(occ)
            if not o[Q]:
                continue
            sgn = (-1) ** sum(o[:Q])
            o[Q] = 0
            if o[P]:
                continue
            sgn *= (-1) ** sum(o[:P])
            o[P] = 1
            E[p, q, dets[tuple(o)], c] += sgn
    return sec, E


@pytest.mark.parametrize("ncas,na,nb", [(3, 2, 1), (4, 1, 3), (4, 0, 2), (4, 2, 1), (5, 2, 1), (5, 0, 0), (5, 5, 2),
                                        (3, 0, 3)])
def test_twin_operators_equal_brute_force_fock_space(ncas, na, nb):
    sec, E = _fock_epq(ncas, na, nb)
    v = S.dense_vector(sec, 5)
    c1, c2 = S.coefficients(ncas, 9)
    V = np.einsum("pqij,j->pqi", E, v)
    assert np.abs(sec.apply_epq(v).reshape(ncas, ncas, -1) - V).max() < 1e-14
    g1, g2 = sec.rdms(v)
    G2 = np.einsum("qpi,rsi->pqrs", V, V) - np.einsum("qr,ps->pqrs", np.eye(ncas), np.einsum("i,psi->ps", v, V))
    assert np.abs(g1 - np.einsum("i,pqi->pq", v, V)).max() < 1e-12 and np.abs(g2 - G2).max() < 1e-12
    H = np.einsum("pq,pqij->ij", c1, E) + np.einsum("pqrs,pqik,rskj->ij", c2, E, E) \
        - np.einsum("pqqs,psij->ij", c2, E)
    lam = sec.lam(v, c1, c2)
    assert np.abs(lam - (H + H.T) @ v).max() < 1e-11 * max(1.0, np.abs(lam).max())
    assert abs(sec.energy(v, c1, c2) - v @ H @ v) < 1e-11 * max(1.0, abs(v @ H @ v))
    # the |.| companions dominate, and the norm bound holds
    Ha = np.einsum("pq,pqij->ij", np.abs(c1), np.abs(E)) + np.einsum("pqrs,pqik,rskj->ij", np.abs(c2), np.abs(E),
                                                                     np.abs(E)) \
        + np.einsum("pqqs,psij->ij", np.abs(c2), np.abs(E))
    assert np.abs(sec.lam(v, c1, c2, absolute=True) - (Ha + Ha.T) @ np.abs(v)).max() <= 1e-10 * np.abs(Ha).sum()
    assert np.linalg.norm(H + H.T, 2) <= sec.lam_norm(c1, c2) * (1 + 1e-12)


@pytest.mark.parametrize("ncas,na,nb,kind", [(3, 2, 1, "uccsd"), (4, 2, 1, "uccsd"), (4, 2, 2, "fabric"),
                                             (4, 1, 3, "ladder")])
def test_adjoint_and_hessian_formulas_equal_central_differences(ncas, na, nb, kind):
    sec = S.Sector(ncas, na, nb)
    gates, n_theta = S.circuit(kind, ncas, na, nb)
    init = X.basis_index(sec.occupation())
    c1, c2 = S.coefficients(ncas, 21)
    theta = np.random.default_rng(ncas).uniform(0, 2 * np.pi, n_theta)

    def energy(t):
        return sec.energy(S.apply_gates(gates, t, sec, init)[0], c1, c2)

    grad, _ = S.adjoint(gates, theta, sec, init, c1, c2, n_theta)
    H = S.hessian(gates, theta, sec, init, c1, c2, n_theta)
    assert np.abs(H - H.T).max() < 1e-11 * np.abs(H).max()
    h = 1e-4
    scale = max(1.0, np.abs(grad).max())
    for k in range(min(n_theta, 6)):
        e = np.zeros(n_theta)
        e[k] = h
        assert abs((energy(theta + e) - energy(theta - e)) / (2 * h) - grad[k]) < 1e-6 * scale
        gp = S.adjoint(gates, theta + e, sec, init, c1, c2, n_theta)[0]
        gm = S.adjoint(gates, theta - e, sec, init, c1, c2, n_theta)[0]
        assert np.abs((gp - gm) / (2 * h) - H[:, k]).max() < 1e-6 * max(1.0, np.abs(H).max())


@pytest.mark.parametrize("ncas,na,nb", [(3, 2, 1), (4, 2, 2), (4, 0, 2), (5, 2, 1), (6, 3, 2), (7, 2, 3), (8, 2, 1)])
def test_fp64_twin_within_half_of_each_bound_of_its_longdouble_version(ncas, na, nb):
    if np.finfo(np.longdouble).eps >= 2.0 ** -60:
        pytest.fail("np.longdouble is no wider than double here: the twin's own error cannot be measured")
    sec = S.Sector(ncas, na, nb)
    c1, c2 = S.coefficients(ncas, 2)
    worst = 0.0
    for v in S.make_vectors(sec, 40 + ncas, 4):
        g1, g2 = sec.rdms(v)
        l1, l2 = sec.rdms(v, dtype=np.longdouble)
        b1, b2 = S.rdm_bounds(sec, v)
        for got, ref, b in ((g1, l1, b1), (g2, l2, b2), (sec.lam(v, c1, c2), sec.lam(v, c1, c2, dtype=np.longdouble),
                                                        S.lam_bound(sec, v, c1, c2))):
            err = np.abs(got - ref).astype(np.float64)
            assert (err <= 0.5 * b).all()
            worst = max(worst, float((err[b > 0] / b[b > 0]).max()))
    print(f"fp64 twin against longdouble, ncas {ncas} ({na},{nb}): largest error / bound {worst:.3f} (limit 0.5)")


# ---- the device case tables ----------------------------------------------------------------------------------------
def _max_pairs(s):
    ncas, na, nb, kind = s[:4]
    sec = S.Sector(ncas, na, nb)
    gates, n_theta = S.circuit(kind, ncas, na, nb)
    counts = S.apply_gates(gates, np.zeros(n_theta), sec, X.basis_index(sec.occupation()))[1]
    return sec, len(gates), n_theta, int(counts.max())


def test_every_sector_of_the_table_is_there_for_the_shape_it_names():
    got = {}
    for s in S.SECTORS + S.STATE_ONLY:
        sec = S.Sector(*s[:3])
        got[s[:3]] = (sec.na, sec.nb)
    want = {(2, 1, 1): (2, 2), (3, 2, 1): (3, 3), (4, 2, 2): (6, 6), (4, 2, 1): (6, 4), (4, 1, 3): (4, 4),
            (4, 0, 2): (1, 6), (5, 2, 2): (10, 10), (5, 1, 1): (5, 5), (5, 2, 1): (10, 5), (6, 3, 3): (20, 20),
            (6, 2, 2): (15, 15), (6, 3, 2): (20, 15), (7, 3, 3): (35, 35), (7, 4, 3): (35, 35), (7, 2, 3): (21, 35),
            (8, 4, 4): (70, 70), (8, 3, 5): (56, 56), (8, 4, 3): (70, 56), (8, 4, 1): (70, 8), (8, 1, 4): (8, 70),
            (8, 2, 1): (28, 8), (8, 0, 4): (1, 70), (9, 1, 1): (9, 9), (9, 3, 3): (84, 84), (9, 4, 4): (126, 126),
            (9, 4, 3): (126, 84), (10, 2, 4): (45, 210), (12, 1, 1): (12, 12), (13, 1, 1): (13, 13),
            (13, 2, 1): (78, 13), (13, 1, 2): (13, 78)}
    assert got == want


def test_sweep_cases_reach_every_instance_a_shape_can_reach():
    """MAXP of the pair-list sweeps, MAXIT of the plain ones.  What no accepted shape reaches (DESIGN.md lists them):
    adjoint_pl<16> -- a gate of more than 4 096 pairs in a sector whose two vectors fit 160 KB (8 193 ... 10 200
    determinants) would have to rotate 80 % of it; an excitation rotates at most 27 % of any sector of that size."""
    seen = set()
    for s in S.SECTORS + S.STATE_ONLY:
        sec, ng, nt, mp = _max_pairs(s)
        for kind in ("state", "deriv", "adjoint"):
            for pl in (True, False):
                seen.add(S.sweep_route(s[0], sec.na, sec.nb, ng, nt, mp, pl, kind))
    named = {(9, 4, 4): ("state_pl<16>", "deriv_pl<16>"), (9, 4, 3): ("state_pl<8>", "deriv_pl<8>"),
             (10, 2, 4): ("adjoint_pl<8>",), (9, 3, 3): ("state_pl<4>", "adjoint_pl<4>", "state<8>", "adjoint<8>")}
    for key, names in named.items():
        s = next(t for t in S.SECTORS + S.STATE_ONLY if t[:3] == key)
        sec, ng, nt, mp = _max_pairs(s)
        for name in names:
            kind, pl = name.split("<")[0].replace("_pl", ""), "_pl" in name
            assert S.sweep_route(s[0], sec.na, sec.nb, ng, nt, mp, pl, kind) == name, (key, name)
    want = {f"{k}_pl<{m}>" for k in ("state", "deriv") for m in (1, 2, 4, 8, 16)} \
        | {f"adjoint_pl<{m}>" for m in (1, 2, 4, 8)} \
        | {f"{k}<{m}>" for k in ("state", "deriv", "adjoint") for m in (1, 2, 5, 8)} | {"refused"}
    assert seen == want, (sorted(want - seen), sorted(seen - want))
    # adjoint_pl<16>: every sector of more than 8 192 determinants whose reverse sweep fits 160 KB, and the largest
    # share of it a single excitation rotates (a double excitation fixes four occupations and rotates less)
    from math import comb
    share = 0.0
    for a in range(2, 14):
        for n_a in range(a + 1):
            for n_b in range(a + 1):
                Dc = comb(a, n_a) * comb(a, n_b)
                if Dc > 8192 and S.sweep_route(a, comb(a, n_a), comb(a, n_b), 1, 1, 1, True, "adjoint") != "refused":
                    share = max([share] + [comb(a - 2, n - 1) / comb(a, n) for n in (n_a, n_b) if 1 <= n < a])
    assert 0 < share < 0.27 and share * 10240 < 4096
    assert S.sweep_route(9, 126, 126, 32, 32, 4410, True, "adjoint") == "refused"


def _rdm_cases():
    for (ncas, na, nb) in S.RDM_WALK_GENERIC:
        for batch in S.RDM_BATCHES_GENERIC:
            yield ncas, na, nb, batch, {}
    for (ncas, na, nb) in S.RDM_WALK_FUSED:
        for batch in S.RDM_BATCHES_FUSED:
            for opt in S.RDM_OPTIONS:
                yield ncas, na, nb, batch, opt
    for s in S.SECTORS:
        for batch in S.RDM_BATCHES_EACH:
            yield s[0], s[1], s[2], batch, {}


def test_rdm_cases_reach_every_instance():
    seen = set()
    for ncas, na, nb, batch, opt in _rdm_cases():
        sec = S.Sector(ncas, na, nb)
        seen.update(S.rdm_route(ncas, sec.na, sec.nb, batch, 256, opt.get("sector_unfused", 0),
                                opt.get("sector_rdm_r3", 0)))
    want = {"epq", "epq_rows"}
    # row chunks: nsplit = min(8, CUs / batch, chunks); 16 orbital pairs have one chunk (18 rows of 8 columns)
    want |= {"rdm_rows<1>:nsplit=1"} | {f"rdm_rows<4>:nsplit={n}" for n in (1, 2, 4, 7, 8)}
    # chunks of 128 determinants: nsplit 8 / 4 / 2 / 1 by batch; 36 determinants at most for 16 orbital pairs
    want |= {"rdm_fused<1>:nsplit=1"} | {f"rdm_fused<4>:nsplit={n}" for n in (1, 2, 4, 8)}
    # the Gram from V in memory: every template instance at every nsplit, both load branches where both exist
    # (the binomials of 7 are all odd: gram_rows<4,4,false> only ever sees an odd Dc)
    rows = ("2,2,false", "3,3,false", "4,4,false", "4,4,true", "1,1,true")
    for t in rows:
        for n in (1, 2, 8):
            assert {f"gram_rows<{t}>:nsplit={n}", f"gram_rows<{t}>:nsplit={n}:odd"} & seen, (t, n)
    for t in ("2,2,false", "3,3,false", "4,4,false"):
        assert any(x.startswith(f"gram_rows<{t}>") and x.endswith(":odd") for x in seen), t
    for t in ("2,2,false", "3,3,false", "4,4,true", "1,1,true"):
        assert any(x.startswith(f"gram_rows<{t}>") and not x.endswith(":odd") for x in seen), t
    # the tile-per-workgroup Gram: every tile count of ncas 2 ... 13 in the table, and every nsplit
    for m, n in ((1, 1), (2, 1), (2, 2), (3, 3), (4, 4), (5, 4), (6, 6), (7, 7), (10, 9), (11, 11)):
        assert any(x.startswith(f"gram<MT={m},NT={n}>") for x in seen), (m, n)
    for k in (1, 2, 8):
        assert any(x.startswith("gram<") and x.endswith(f"nsplit={k}") for x in seen), k
    assert not want - seen, sorted(want - seen)
    # the thresholds of the generic route: batches 1-3 and 8-15 on one kernel, 4-7 and >= 16 on the other
    kinds = [S.rdm_route(6, 20, 15, b)[1].split(":")[0].split("<")[0] for b in S.RDM_BATCHES_GENERIC]
    assert kinds == ["gram", "gram", "gram_rows", "gram_rows", "gram", "gram", "gram_rows", "gram_rows", "gram_rows"]
    assert [S.rdm_route(6, 20, 15, b)[0] for b in (7, 8)] == ["epq", "epq_rows"]
    # 84 x 84 is the last size of the E_pq rows variant; 45 x 210 is past it
    assert S.rdm_route(9, 84, 84, 8)[0] == "epq_rows" and S.rdm_route(10, 45, 210, 8)[0] == "epq"
    assert S.rdm_route(12, 12, 12, 16)[0] == "epq_rows" and "fused" not in "".join(S.rdm_route(12, 12, 12, 16))
    # the rows route from 16 states on, the chunks of 128 below
    assert [S.rdm_route(8, 70, 56, b)[0].split("<")[0] for b in (15, 16)] == ["rdm_fused", "rdm_rows"]


def _lam_cases():
    for s in S.SECTORS:
        for batch in S.LAM_BATCHES + (S.LAM_BATCHES_FUSED_EXTRA if s[:3] in S.RDM_WALK_FUSED else []):
            for opt in (S.LAM_OPTIONS if s[0] in (4, 8) else [{}]):
                yield s[0], s[1], s[2], batch, opt


def test_lam_cases_reach_every_instance():
    seen = set()
    for ncas, na, nb, batch, opt in _lam_cases():
        sec = S.Sector(ncas, na, nb)
        seen.update(S.lam_route(ncas, sec.na, sec.nb, batch, 256, opt.get("sector_unfused", 0),
                                opt.get("sector_lambda_w", 0)))
    want = {"gmat", "lambda_dense", "epq", "epq_rows", "mode_contract", "lambda_tab", "w_fused<1>:nsplit=1",
            "lambda:lds=67584", "lambda:lds=34816", "lambda:lds=2304", "lambda_fused<1>:nsplit=1"}
    want |= {f"w_fused<4>:nsplit={n}" for n in (1, 2, 4, 8)}
    want |= {f"lambda_fused<4>:nsplit={n}" for n in (1, 2, 4, 7, 8)}
    assert not want - seen, sorted(want - seen)
    assert [S.lam_route(8, 70, 56, b)[0].split("<")[0] for b in (31, 32)] == ["w_fused", "gmat"]
    # a^2 = 144 is a multiple of 16 and takes no fused route; ncas 13 is the one launch past 64 KB of dynamic LDS
    assert S.lam_route(12, 12, 12, 32) == ["epq_rows", "mode_contract", "lambda:lds=34816"]
    assert S.lam_route(13, 78, 13, 1)[-1] == "lambda:lds=67584" and 67584 > 64 * 1024


def test_case_tables_take_the_smallest_shapes():
    assert max(S.Sector(*s[:3]).Dc for s in S.SECTORS) == 45 * 210
    assert max(S.Sector(*s[:3]).Dc for s in S.STATE_ONLY) * 8 <= 127 * 1024
