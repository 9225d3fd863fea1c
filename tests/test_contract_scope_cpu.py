"""The case table and the references of the contraction kernels' whole-scope tests (tests/_contract_scope.py), without
a device: the table reaches every one of the 91 builds of K1 / K1P, every edge row lands where it says, the integer
inputs are exact in fp64, the longdouble reference is what it claims to be, and the describe call behind all of it
reports the launch arithmetic.  A change of contract_plan() in csrc/contract.hip has to come with a new table here."""
import math

import numpy as np
import pytest

from auto_oo_amd import _lib, ops
from tests import _contract_scope as S


def test_the_enumeration_has_91_builds():
    """The explicit list, written out family by family, against S.BUILDS"""
    want = set()
    for nt in range(1, 14):
        want |= {("deep", True, False, nt), ("deep", True, True, nt)}           # 26: 20-row chunks, INNER and LAST
        want |= {("shallow", False, False, nt), ("shallow", False, True, nt)}   # 26: 12-row chunks
        want |= {("wide", False, False, nt)}                                    # 13: long stride, INNER only
    for nt in range(1, 5):
        want |= {("short", False, False, nt), ("short", False, True, nt)}       # 8: single chunk
    for nt in range(5, 14):
        want |= {("pair", True, False, nt), ("pair", False, False, nt)}         # 18: two strips per wave
    assert len(want) == 91 and set(S.BUILDS) == want and len(S.BUILDS) == 91


def test_case_table_lands_on_all_91_builds():
    got = {S.build_of(c): c.name for c in S.BUILD_CASES}
    missing = set(S.BUILDS) - set(got)
    print(f"{len(set(got) & set(S.BUILDS))} of {len(S.BUILDS)} builds covered by the table")
    assert not missing, sorted(S.build_id(b) for b in missing)
    assert len(S.BUILD_CASES) == 91 and set(got) == set(S.BUILDS)
    for c, b in zip(S.BUILD_CASES, S.BUILDS):
        assert S.build_of(c) == b and c.name == S.build_id(b)


@pytest.mark.parametrize("c", S.BUILD_CASES + S.EDGE_CASES, ids=lambda c: c.name)
def test_every_case_lands_where_it_says(c):
    p = S.plan_of(c)
    assert c.expect, "a case has to say where it lands"
    for key, want in c.expect.items():
        assert p[key] == want, (c.name, key, want, p)
    # the launch arithmetic the fields share
    assert p["rounds"] == -(-(-(-p["strips"] // p["waves"])) // p["grid_x"])
    assert p["n_items"] == (-(-c.A // 16) if c.last else c.A * -(-c.B // 16)) and p["nbt"] == (1 if c.last else -(-c.B // 16))
    assert p["ngroups"] == -(-(-(-c.J // 16)) // p["nt"]) and 1 <= p["nt"] <= 13
    assert (p["waves"], p["strips"]) == ((4, c.A * -(-c.B // 32)) if p["family"] == "pair" else (8, p["n_items"]))
    # the largest case: 35 MB of T and 115 MB of results
    assert (c.A * c.K * c.B + c.A * c.J * c.B) * 8 * c.batch <= 160e6


def test_edge_rows_cover_what_the_kernels_branch_on():
    E = S.EDGE_CASES
    plans = {c.name: S.plan_of(c) for c in E}
    assert len({c.name for c in E + S.BUILD_CASES}) == len(E) + len(S.BUILD_CASES)
    for KC in (12, 20, 48):
        assert {KC - 1, KC, KC + 1, 2 * KC} <= {c.K for c in E}
    assert {1, 48, 49} <= {c.K for c in E}
    assert {1, 15, 16, 17, 31, 32, 33} <= {c.B for c in E if not c.last}
    assert {1, 15, 16, 17} <= {c.A for c in E if c.last} and any(c.last and c.A % 128 for c in E)
    assert all({16 * n - 15, 16 * n - 1, 16 * n} <= {c.J for c in E} for n in (1, 2, 3))
    assert {1, 2} <= {p["rounds"] for p in plans.values()}
    assert any(p["rounds"] == 2 and -(-p["strips"] // p["waves"]) % p["grid_x"] for p in plans.values())   # ragged
    assert any(c.ldc > c.J for c in E) and any(c.t_odd for c in E) and any(c.out_odd for c in E)
    assert {1, 2, 7} <= {c.batch for c in E} and any(c.batch > 1 and c.c_bs == 0 for c in E)
    assert any(c.batch > 1 and c.t_bs > c.A * c.K * c.B and c.o_bs > c.A * c.J * c.B for c in E)
    for fam in ("short", "deep", "shallow", "wide", "pair"):
        assert any(c.batch > 1 and not c.last and plans[c.name]["family"] == fam for c in E), fam
    assert any(c.batch > 1 and c.last for c in E)
    # what keeps a shape out of the pair family, one reason at a time: the twin that differs in nothing else is in it
    assert plans["pair-taken"]["family"] == "pair" and plans["pair-padding-none"]["family"] == "pair"
    for name in ("pair-odd-B", "pair-padding-rule", "pair-T-misaligned", "pair-out-misaligned", "pair-no-pair",
                 "batch2-pair-odd-t_bs", "batch2-pair-odd-o_bs"):
        assert plans[name]["family"] == "deep" and plans[name]["nt"] == 5, name


def test_describe_follows_the_debug_options_and_refuses_what_the_launch_refuses():
    free = ops.contract_plan(3, 49, 205, 23467, False)
    assert (free["family"], free["nt"]) == ("deep", 13)
    for nt in range(1, 14):
        with _lib.debug_options(k1_force_nt=nt):
            p = ops.contract_plan(3, 49, 205, 23467, False)
        assert p["nt"] == -(-13 // -(-13 // nt)) and p["ngroups"] == -(-13 // nt), (nt, p)
    with _lib.debug_options(k1_force_wide=1):
        assert ops.contract_plan(3, 49, 205, 23467, False)["family"] == "wide"
    assert ops.contract_plan(3, 49, 205, 23467, False) == free               # the options were restored
    # a stride that no 32-bit step offset spans: the long-stride family without being forced
    assert ops.contract_plan(1, 49, 16, 34_000_000, False)["family"] == "wide"
    for args, msg in (((1, 5, 5, 2, True), "last-mode needs B == 1"), ((0, 5, 5, 1, False), "bad dims"),
                      ((1, 0, 5, 1, False), "bad dims"), ((1, 5, 0, 1, False), "bad dims"),
                      ((2_000_000_000, 5, 5, 16, False), "too many strips"),
                      ((1, 5, 5, 1, False, 0), "batch=0"), ((1, 5, 5, 1, False, 65536), "batch=65536")):
        with pytest.raises(_lib.OovqeError, match=msg):
            ops.contract_plan(*args)


def test_integer_inputs_are_exact_in_fp64():
    """|T|, |Cm| <= 8: the sum of magnitudes stays below 64 K < 2^53 for every K of the tables, the inputs have no
    structure to hide an index swap, and the fp64 product of the host equals the int64 one."""
    assert max(c.K for c in S.BUILD_CASES + S.EDGE_CASES) * S.VMAX * S.VMAX < 2 ** 53
    for c in (S.EDGE_CASES[0], S.EDGE_CASES[23], S.case("x", 3, 61, 45, 333), S.case("y", 200, 49, 45, last=True),
              S.case("z", 2, 30, 37, 50, batch=3)):
        T, Cm = S.integer_inputs(c)
        assert np.abs(T).max() <= S.VMAX and np.abs(Cm).max() <= S.VMAX and (T == np.rint(T)).all()
        assert float((np.abs(Cm[0]).T @ np.abs(T[0, 0])).max()) <= 64 * c.K
        ref = S.exact_reference(c, T, Cm)
        truth = S.product(T, Cm, np.int64)
        assert ref.dtype == np.float64 and np.array_equal(ref.astype(np.int64), truth) and np.array_equal(ref, truth)
        # against the definition, element by element, on a few entries
        for b, a, j, col in ((0, 0, 0, 0), (c.batch - 1, c.A - 1, c.J - 1, c.B - 1), (0, c.A // 2, c.J // 3, c.B // 2)):
            want = sum(int(Cm[b if Cm.shape[0] > 1 else 0, k, j]) * int(T[b, a, k, col]) for k in range(c.K))
            assert truth[b, a, j, col] == want
        if c.K == c.J:
            assert not np.array_equal(Cm[0], Cm[0].T)
        for axis in range(1, 4):                                # no two slabs, rows or columns of T alike
            if T.shape[axis] > 1 and T.size // T.shape[axis] >= 30:
                flat = np.moveaxis(T[0], axis - 1, 0).reshape(T.shape[axis], -1)
                assert len({row.tobytes() for row in flat}) == T.shape[axis]


def test_longdouble_reference_against_fsum():
    assert np.finfo(S.LD).nmant >= 63, "the rounded reference needs a 64-bit significand"
    for c, scaled in ((S.case("x", 3, 61, 45, 333), False), (S.case("x", 3, 61, 45, 333), True),
                      (S.case("y", 200, 49, 45, last=True), True)):
        T, Cm = S.real_inputs(c, scaled)
        if scaled:
            assert np.abs(Cm).max() > 2.0 ** 290 and np.abs(Cm).min() < 2.0 ** -290
        n = c.A if c.last else c.B
        idx = S.sample(n)
        assert set(range(33)) <= set(idx) and set(range(n - 33, n)) <= set(idx)
        assert all({e - 1, e} <= set(idx) for e in range(16, n, 16))
        ref, bound = S.rounded_reference(c, T, Cm, idx)
        for i, a, j in ((0, 0, 0), (len(idx) - 1, c.A - 1, c.J - 1), (len(idx) // 2, 1, 7), (5, 2, 44)):
            if c.last:
                terms = [Cm[0, k, j] * T[0, idx[i], k, 0] for k in range(c.K)]     # (each product: one rounding)
                got, bnd = ref[0, i, j, 0], bound[0, i, j, 0]
            else:
                terms = [Cm[0, k, j] * T[0, a, k, idx[i]] for k in range(c.K)]
                got, bnd = ref[0, a, j, i], bound[0, a, j, i]
            mag = math.fsum(abs(t) for t in terms)
            assert abs(float(got) - math.fsum(terms)) <= 2 * S.U * mag        # fsum is exact on fp64-rounded products
            assert abs(bnd - (c.K + 2) * S.U * mag) <= 1e-12 * bnd
