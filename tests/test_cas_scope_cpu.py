"""tests/_cas_scope.py without a device: the case list reaches every class the plan can choose, the new reference
agrees with the oracle the project trusts and with itself in two precisions, the inputs meet their condition, and the
comparison reports a wrong geometry."""
import re

import numpy as np
import pytest
import torch

from auto_oo_amd import _lib

from tests import _cas_scope as S

# long double has no BLAS: the geometries of N > CPU_N_MAX are held against it where they run (test_cas_scope_gpu.py)
CPU_N_MAX = 49


def test_case_list_reaches_every_class():
    """The sweep of the plan space, repeated here: CASES has exactly one case per class (path, stage-1 kernel, tail
    build, circuit placement, W), every knob and every edge is taken by a case, and every further case is the first to
    take a knob or an edge (its reason to exist).  A class added to cas.hip later fails here until it gets a case."""
    found = S.enumerate_classes()
    assert len(found) > 200 and {c[0] for c in found} == {"packed_tail", "packed_split", "fused", "column", "staged"}
    listed = [S.class_of(S.case_plan(s, None if s[7] else S.GIVEN_N_THETA)) for s in S.CASES]
    assert len(set(listed)) == len(listed), "two cases of one class"
    missing = sorted(set(found) - set(listed))
    assert not missing, f"classes without a case: {missing}"
    assert not set(listed) - set(found), "a case of a class outside the sweep"

    taken_knobs, taken_edges = set(), set()
    for i, (shape, n_given) in enumerate(S.all_cases()):
        plan, nrdm = S.case_plan(shape, n_given), S.case_nrdm(shape, n_given)
        knobs = {k for k, f in S.KNOBS.items() if f(shape, plan, nrdm)}
        edges = {e for e, f in S.EDGES.items() if f(shape, plan)}
        if i >= len(S.CASES):
            assert (knobs - taken_knobs) or (edges - taken_edges), f"case {shape} takes nothing new"
        taken_knobs |= knobs
        taken_edges |= edges
    assert taken_knobs == set(S.KNOBS), set(S.KNOBS) - taken_knobs
    assert taken_edges == set(S.EDGES), set(S.EDGES) - taken_edges


def test_refused_shapes():
    for shape, words in S.REFUSED:
        with pytest.raises(_lib.OovqeError, match=re.escape(words)):
            S.case_plan(shape, S.GIVEN_N_THETA)


def test_option_cases_take_their_realisation():
    assert {o[0] for o in S.OPTION_CASES} == {"sym_two_step", "sym_simple", "sym_mirror", "sym_no_rs", "panel_no_w",
                                              "no_ride", "tail_split", "cas_unfused", "fused_chunks", "gm_plain_grid",
                                              "panel_rows"}
    for option, value, shape, n_given, cls, fields in S.OPTION_CASES:
        default = S.case_plan(shape, n_given)
        with _lib.debug_options(**{option: value}):
            plan = S.case_plan(shape, n_given)
        assert S.class_of(plan) == cls, (option, S.class_of(plan))
        assert {k: plan[k] for k in fields} == fields, (option, plan)
        assert S.class_of(default) != cls or any(default.get(k) != v for k, v in fields.items()), option
        assert S.case_plan(shape, n_given) == default


def test_describe_reports_the_launch_choices():
    """The fields oovqe_oo_eval_plan_describe appends, against the arithmetic written out here for three shapes"""
    p = S.plan_of(6, 0, 6, 1, 0, False, False, n_theta=40)             # column: 160 KB of LDS, sets of 8 (36 + 1296) B
    base = (6 * 36 + 6 * 6 + 216 + 6 + 6 + 6 + 6 + 4 * 6) * 8
    chunk = (160 * 1024 - base) // ((36 + 1296) * 8)
    assert (p["rdm_chunk"], p["zsplit"]) == (str(chunk), str(min(-(-41 // chunk), 2 * 256 // 6, 64)))
    p = S.plan_of(21, 12, 8, 1, 0, False, False, n_theta=40)
    assert p["path"] == "staged" and p["staged_rows"] == "0"
    p = S.plan_of(6, 2, 2, 385, 1, False, True, nelecas=2)             # panel with W: npan = ceil(6 * 385 / 384)
    assert (p["panel_w"], p["npan"], p["xcd_grid"], p["rdm_chunk"]) == ("1", "7", "1", "2")


ORACLE_SHAPES = ((9, 0, 2, 3), (10, 3, 2, 0), (12, 2, 3, 1))


@pytest.mark.parametrize("N, n_occ, ncas, flags", ORACLE_SHAPES)
def test_reference_agrees_with_the_oracle(N, n_occ, ncas, flags):
    from oracle import cpu_ref as R
    g = S.integral_tensors(N, flags, 3, 11)[-1]
    assert S.has_symmetry(g) == flags
    C, gamma, Gamma, nuc, h = S.geometry_inputs(N, ncas, 3, 2, 11)
    rows, cols = S.kappa_tables(N, n_occ, ncas)
    args = (h[1], g, C[1], gamma[1], Gamma[1], nuc[1], n_occ, ncas, rows, cols)
    ref, mag = S.evaluate(*args, dtype=S.LD), S.evaluate(*args, mag=True)
    occ, act = np.arange(n_occ), np.arange(n_occ, n_occ + ncas)
    Ct = torch.tensor(C[1])
    h1, g2 = R.int1e_transform(torch.tensor(h[1]), Ct), R.int2e_transform(torch.tensor(g), Ct)
    c0, c1, c2 = R.molecular_hamiltonian_coefficients(nuc[1], h1, g2, occ, act)
    oo = object.__new__(R.OracleOOEnergy)
    oo.occ_idx, oo.act_idx, M = occ, act, n_occ + ncas
    g1, G2 = torch.tensor(gamma[1]), torch.tensor(Gamma[1])
    F = [oo.fock_generalized(h1, g2, g1[k], G2[k]) for k in range(3)]
    got = dict(c0=np.array([float(c0)]), c1=c1.numpy(), c2=c2.numpy(), fock=F[0].numpy(), gmat=(2 * (F[0] - F[0].T)).numpy(),
               E=np.array([float(c0 + (c1 * g1[0]).sum() + (c2 * G2[0]).sum())]),
               dE=np.array([float((c1 * g1[k]).sum() + (c2 * G2[k]).sum()) for k in (1, 2)]),
               gvec=(2 * (F[0] - F[0].T)).numpy()[rows, cols][None], Gm=g2[:, :M, :M, :M].numpy(), hmo=h1[:, :M].numpy())
    ref0 = dict(ref, gvec=ref["gvec"][:1])
    mag0 = dict(mag, gvec=mag["gvec"][:1])
    ratios, failures = S.compare(got, ref0, mag0, S.chain_lengths(N, n_occ, ncas), factor=2)
    print({q: round(r, 2) for q, r in ratios.items()})
    assert not failures, failures
    assert np.array_equal(rows, np.tril_indices(N, -1)[0][R.non_redundant_indices(list(occ), list(act), list(range(M, N)), False)])


def _keys(n_max):
    seen = {}
    for shape, n_given in S.all_cases():
        if shape[0] <= n_max:
            seen.setdefault(S.input_key(shape), (shape, S.case_nrdm(shape, n_given)))
    return list(seen.values())


def test_float64_reference_and_input_condition():
    """Per input key with N <= CPU_N_MAX: the float64 reference agrees with the long-double one within the bound (every
    geometry at N <= 24, one middle geometry above), and the bound of every quantity is below 1e-9 max(1, its largest
    element) on the geometries the long-double reference is run for."""
    worst = {}
    for shape, nrdm in _keys(CPU_N_MAX):
        inp = S.case_inputs(shape, nrdm)
        ref = S.Reference(shape, inp)
        G = shape[4]
        picks = S.long_double_geometries(G)
        both = range(G) if shape[0] <= 24 and G <= 31 else picks if shape[0] <= 24 else picks[1:2] or picks[:1]
        for g in sorted(set(picks) | set(both)):
            f64 = ref.evaluate(g, inp["gamma"][g], inp["Gamma"][g], "f64")
            mag = ref.evaluate(g, inp["gamma"][g], inp["Gamma"][g], "mag")
            assert not S.input_condition(f64, mag, ref.k), (shape, g, S.input_condition(f64, mag, ref.k))
            if g in both:
                ld = ref.evaluate(g, inp["gamma"][g], inp["Gamma"][g], "ld")
                ratios, failures = S.check_geometry(g, f64, ld, mag, ref.k, 1)
                assert not failures, (shape, failures)
                for q, r in ratios.items():
                    worst[q] = max(worst.get(q, 0), r / ref.k[q])
    print("float64 against long double, worst error / bound:", {q: f"{r:.3f}" for q, r in worst.items()})


FAIL_CASES = ((20, 1, 2, 2, 31, 3, False, False), (17, 15, 2, 2, 1, 0, False, False), (6, 2, 2, 2, 385, 1, False, False))


@pytest.mark.parametrize("shape", FAIL_CASES, ids=str)
def test_the_comparison_can_fail(shape):
    """The float64 evaluation stands in for the device.  Clean, it passes against the long-double reference; with one
    element of C of a middle geometry changed by 1e-6 relative, with two RDM sets of a geometry swapped, or with the
    last row of the last partly filled 16-wide tile dropped from the contractions, the comparison reports that
    geometry and the quantities it reaches."""
    nrdm, G = 3, shape[4]
    inp = S.case_inputs(shape, nrdm)
    ref = S.Reference(shape, inp)
    mid = S.long_double_geometries(G)[len(S.long_double_geometries(G)) // 2]
    N, M = shape[0], shape[1] + shape[2]
    assert N % 16 != 0

    def run(g, C=None, gamma=None, Gamma=None):
        w = inp["which"][g]
        got = S.evaluate(inp["h"][w], inp["g"][w], inp["C"][g] if C is None else C, inp["gamma"][g] if gamma is None else gamma,
                         inp["Gamma"][g] if Gamma is None else Gamma, inp["nuc"][g], shape[1], shape[2], inp["rows"], inp["cols"])
        ld = ref.evaluate(g, inp["gamma"][g], inp["Gamma"][g], "ld")
        mag = ref.evaluate(g, inp["gamma"][g], inp["Gamma"][g], "mag")
        return S.check_geometry(g, got, ld, mag, ref.k, 1)[1]

    for g in S.long_double_geometries(G):
        assert not run(g)
    C = inp["C"][mid].copy()
    C[N // 2, M - 1] *= 1 + 1e-6
    bad = run(mid, C=C)
    assert bad and all(f[0] == mid for f in bad) and {"Gm", "E", "gvec"} <= {f[1] for f in bad}, bad
    swapped = inp["gamma"][mid][[0, 2, 1]], inp["Gamma"][mid][[0, 2, 1]]
    bad = run(mid, gamma=swapped[0], Gamma=swapped[1])
    assert {f[1] for f in bad} == {"dE", "gvec"} and all(f[0] == mid for f in bad), bad
    C = inp["C"][mid].copy()
    C[N - 1, :] = 0.0                      # row N - 1 of every contraction: the last row of the partly filled tile
    bad = run(mid, C=C)
    assert {"Gm", "hmo", "c1", "c2", "E", "fock"} <= {f[1] for f in bad}, bad
