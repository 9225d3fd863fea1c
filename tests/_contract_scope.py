"""Cases and host references of the whole-scope tests of the contraction kernels (csrc/contract.hip, K1, and
csrc/contract_pair.hip, K1P); numpy only, no device.

    INNER:  out[a, j, b] = sum_k Cm[k, j] T[a, k, b]          LAST:  out[a, j] = sum_k T[a, k] Cm[k, j]

K1 is 91 template builds (BUILDS below).  Which one serves a call is decided by contract_plan() in contract.hip from the
shape, the alignment of T and out, the batch strides and three debug options; ``plan_of`` asks the library itself
(ops.contract_plan -> oovqe_mode_contract_plan_describe), nothing here restates the rule.  BUILD_CASES gives every
build one shape that the rule places there; EDGE_CASES are small shapes on the values the kernels branch on; both say
where they expect to land and tests/test_contract_scope_cpu.py holds them to it, so a change of the planning rule has to
come with a new table.

Two references ("The contraction kernels over their whole scope"):
  * exact -- integer inputs with |T|, |Cm| <= 8: every product and every partial sum is an integer below 64 K < 2^53,
    so fp64 arithmetic in any order, fused or not, returns the integer result itself.  The int64 product is the truth;
    the fp64 product of the host BLAS is the same numbers (the CPU test checks that) and serves the large cases.
  * rounded -- real inputs against np.longdouble, within (K + 2) 2^-53 sum_k |Cm[k, j]| |T[a, k, b]| per element."""
import collections

import numpy as np

from auto_oo_amd import _lib, ops

U = 2.0 ** -53
LD = np.longdouble
VMAX = 8                        # |integer input| <= VMAX

# ---- the builds ----------------------------------------------------------------------------------------------------
# (family, deep, last, nt); deep: 20-row K-chunks, which only the pair family keeps apart from its name
BUILDS = tuple(
    [("deep", True, last, nt) for last in (False, True) for nt in range(1, 14)] +
    [("shallow", False, last, nt) for last in (False, True) for nt in range(1, 14)] +
    [("wide", False, False, nt) for nt in range(1, 14)] +
    [("short", False, last, nt) for last in (False, True) for nt in range(1, 5)] +
    [("pair", deep, False, nt) for deep in (True, False) for nt in range(5, 14)])

Case = collections.namedtuple(
    "Case", "name A K J B last batch ldc t_bs c_bs o_bs t_odd out_odd opts expect")


def case(name, A, K, J, B=1, last=False, batch=1, ldc=None, t_bs=None, c_bs=None, o_bs=None, t_odd=False,
         out_odd=False, opts=None, **expect):
    """One call of the library.  ldc: row pitch of Cm (default J); t_bs / c_bs / o_bs: batch strides in doubles (default:
    the tensors back to back); t_odd / out_odd: T / out begins 8 bytes past a 16-byte boundary; opts: debug options;
    expect: the fields of ops.contract_plan the case is meant to land on."""
    ldc = J if ldc is None else ldc
    t_bs = A * K * B if t_bs is None else t_bs
    c_bs = K * ldc if c_bs is None else c_bs
    o_bs = A * J * B if o_bs is None else o_bs
    return Case(name, A, K, J, B, bool(last), batch, ldc, t_bs, c_bs, o_bs, t_odd, out_odd, dict(opts or {}), expect)


def plan_of(c):
    """The launch the library would make for the case (no device needed)."""
    with _lib.debug_options(**c.opts):
        return ops.contract_plan(c.A, c.K, c.J, c.B, c.last, c.batch, not c.t_odd, not c.out_odd,
                                 c.t_bs if c.batch > 1 else 0, c.o_bs if c.batch > 1 else 0)


def build_of(c):
    p = plan_of(c)
    return (p["family"], p["deep"] if p["family"] == "pair" else p["family"] == "deep", c.last, p["nt"])


def build_id(b):
    family, deep, last, nt = b
    if family == "pair":
        family = "pair20" if deep else "pair12"
    return f"{family}-{'last' if last else 'inner'}-nt{nt}"


# The planning rule halves nt while the launch has fewer than 512 workgroups, so a build with nt tiles only runs from
# 2049 strips on (257 workgroups of 8 waves: halving would pass 512), and a workgroup only walks a second strip group
# -- the cross-strip prefetch under the last chunk, an inactive Strip in the ragged final round -- from 4097 strips on.
# The table takes 4401 (551 groups on 512 workgroups: 39 workgroups walk two, the last group has one live wave), in
# three slabs of odd length for INNER, J = 16 nt - 3 (a ragged last tile), K = 49 for 20-row chunks (3 chunks, 9 live
# rows in the last), K = 61 for 12-row chunks (6 chunks, 1 live row in the last: 20-row chunks would waste 31 %), and
# K = 47 / 13 for the single-chunk builds.  The largest case (nt = 13) moves 115 MB of results.
_INNER = dict(A=3, B=1467 * 16 - 5)           # 3 x 1467 = 4401 strips of 16 columns
_LAST = dict(A=4401 * 16 - 13, B=1, last=True)
_PAIR = dict(A=3, B=734 * 32 - 6)             # 3 x 734 = 2202 strips of 32 columns (>= 2048), even B, no padding loss


def _build_cases():
    out = []
    for family, deep, last, nt in BUILDS:
        J = 16 * nt - 3
        shape = dict(_LAST if last else _PAIR if family == "pair" else _INNER)
        opts = {}
        if family == "short":
            K = 13 if last else 47
        elif family == "deep" or (family == "pair" and deep):
            K = 49
        else:
            K = 61
        if family == "wide":
            opts["k1_force_wide"] = 1
        expect = dict(family=family, nt=nt, ngroups=1, rounds=2)
        if family == "pair":
            expect.update(deep=deep, rounds=3)
        out.append(case(build_id((family, deep, last, nt)), K=K, J=J, opts=opts, **shape, **expect))
    return tuple(out)


BUILD_CASES = _build_cases()

# ---- edge rows -----------------------------------------------------------------------------------------------------
# Small shapes: the rule halves them down to nt = 1 unless the comment says otherwise, so these walk the branches on
# K, J, B, A, the strides and the alignment, not the tile counts (the table above does that).
def _edge_cases():
    E = []
    # K around the chunk depths 12 (shallow), 20 (deep), 48 (short): one short of a chunk, a full chunk, one over, two
    # chunks; K = 1; 48 / 49 is where the single-chunk family ends.
    for K in (1, 11, 12, 13, 19, 20, 21, 24, 40, 47, 48):
        E.append(case(f"short-inner-K{K}", 2, K, 37, 50, family="short", nt=1))
        E.append(case(f"short-last-K{K}", 37, K, 21, last=True, family="short", nt=1))
    for K, fam in ((49, "deep"), (60, "deep"), (61, "shallow"), (95, "shallow"), (96, "deep"), (97, "deep")):
        E.append(case(f"{fam}-inner-K{K}", 2, K, 37, 50, family=fam, nt=1))
        E.append(case(f"{fam}-last-K{K}", 37, K, 21, last=True, family=fam, nt=1))
    # K <= 48 outside the single-chunk family: more than 4 tiles per wave (forced chunked kernels at K = 11 .. 48)
    for K, fam in ((11, "shallow"), (12, "shallow"), (13, "deep"), (19, "deep"), (20, "deep"), (21, "shallow"),
                   (24, "shallow"), (40, "deep"), (48, "shallow")):
        E.append(case(f"{fam}-inner-K{K}-nt5", 3, K, 77, 10923, family=fam, nt=5, rounds=1))
    # J on both sides of a tile edge
    for J in (1, 15, 16, 17, 31, 32, 33, 47, 48, 49):
        E.append(case(f"inner-J{J}", 2, 23, J, 50, family="short"))
        E.append(case(f"last-J{J}", 50, 23, J, last=True, family="short"))
        E.append(case(f"wide-J{J}", 2, 23, J, 50, opts=dict(k1_force_wide=1), family="wide"))
    # B on both sides of a strip edge
    for B in (1, 15, 16, 17, 31, 32, 33):
        E.append(case(f"inner-B{B}", 3, 30, 20, B, family="short", nbt=(B + 15) // 16))
        E.append(case(f"deep-B{B}", 3, 50, 20, B, family="deep", nbt=(B + 15) // 16))
        E.append(case(f"wide-B{B}", 3, 50, 20, B, opts=dict(k1_force_wide=1), family="wide"))
    # LAST: rows on both sides of a strip edge, a partial group of 8 waves (A no multiple of 128)
    for A in (1, 15, 16, 17, 127, 129, 200):
        E.append(case(f"last-A{A}", A, 30, 20, last=True, family="short", n_items=(A + 15) // 16))
        E.append(case(f"shallow-last-A{A}", A, 61, 20, last=True, family="shallow", n_items=(A + 15) // 16))
    # rounds of a workgroup at nt = 1: exactly one, exactly two, a ragged second one (512 workgroups)
    E.append(case("rounds-1", 1, 50, 16, 512 * 8 * 16, family="deep", nt=1, grid_x=512, rounds=1, strips=4096))
    E.append(case("rounds-2", 1, 50, 16, 1024 * 8 * 16, family="deep", nt=1, grid_x=512, rounds=2, strips=8192))
    E.append(case("rounds-ragged", 1, 50, 16, 700 * 8 * 16 - 100, family="deep", nt=1, grid_x=512, rounds=2, strips=5594))
    E.append(case("rounds-ragged-last", 700 * 128 - 100, 50, 16, last=True, family="deep", nt=1, grid_x=512, rounds=2))
    E.append(case("rounds-5-two-j-groups", 2, 61, 29, 1100 * 8 * 8 + 3, opts=dict(k1_force_nt=1), family="shallow", nt=1,
                  ngroups=2, grid_x=256, rounds=5))
    # the pair family and what keeps a shape out of it: odd B, an even B that 32-wide strips pad by more than 2 %
    # (200 -> 224 against 208), T or out 8 bytes off a 16-byte boundary, odd batch strides
    pair = dict(A=12, K=50, J=77, B=5498)
    E.append(case("pair-taken", **pair, family="pair", nt=5, deep=True))
    E.append(case("pair-odd-B", 12, 50, 77, 5499, family="deep", nt=5))
    E.append(case("pair-padding-rule", 320, 50, 77, 200, family="deep", nt=5))
    E.append(case("pair-padding-none", 320, 50, 77, 224, family="pair", nt=5))
    E.append(case("pair-T-misaligned", **pair, t_odd=True, family="deep", nt=5))
    E.append(case("pair-out-misaligned", **pair, out_odd=True, family="deep", nt=5))
    E.append(case("pair-no-pair", **pair, opts=dict(k1_no_pair=1), family="deep", nt=5))
    E.append(case("pair-mostly-empty-last-block", 12, 61, 77, 5442, family="pair", nt=5, deep=False))
    # Cm a block of a wider matrix
    E.append(case("ldc-inner", 2, 30, 37, 50, ldc=41, family="short"))
    E.append(case("ldc-last", 50, 30, 37, ldc=64, last=True, family="short"))
    E.append(case("ldc-deep", 2, 50, 37, 50, ldc=38, family="deep"))
    E.append(case("ldc-pair", **pair, ldc=91, family="pair"))
    E.append(case("ldc-wide", 2, 50, 37, 50, ldc=39, opts=dict(k1_force_wide=1), family="wide"))
    # batched calls: 1, 2, 7 elements; Cm shared (c_bs = 0) or one each; gaps between the elements; odd strides
    sh = dict(A=2, K=30, J=37, B=50)
    n_t, n_c, n_o = 2 * 30 * 50, 30 * 37, 2 * 37 * 50
    for batch in (1, 2, 7):
        E.append(case(f"batch{batch}-short", **sh, batch=batch, family="short"))
        E.append(case(f"batch{batch}-short-shared-Cm", **sh, batch=batch, c_bs=0, family="short"))
        E.append(case(f"batch{batch}-short-gaps", **sh, batch=batch, t_bs=n_t + 6, c_bs=n_c + 3, o_bs=n_o + 10,
                      family="short"))
        E.append(case(f"batch{batch}-short-odd-strides", **sh, batch=batch, t_bs=n_t + 7, o_bs=n_o + 5, family="short"))
    E.append(case("batch3-last-nn", 50, 37, 21, last=True, batch=3, family="short"))          # matmul_nn_batch (3,50,37,21)
    E.append(case("batch3-last-shared-Cm", 50, 61, 21, last=True, batch=3, c_bs=0, family="shallow"))
    E.append(case("batch2-deep", 2, 50, 37, 50, batch=2, t_bs=5003, o_bs=3711, family="deep"))
    E.append(case("batch2-shallow", 2, 61, 37, 50, batch=2, c_bs=0, family="shallow"))
    E.append(case("batch2-wide", 2, 61, 37, 50, batch=2, c_bs=0, o_bs=3800, opts=dict(k1_force_wide=1), family="wide"))
    pb = dict(A=6, K=50, J=77, B=5498)
    n_pt, n_po = 6 * 50 * 5498, 6 * 77 * 5498
    E.append(case("batch2-pair", **pb, batch=2, family="pair", nt=5))
    E.append(case("batch2-pair-gaps-shared-Cm", **pb, batch=2, t_bs=n_pt + 4, c_bs=0, o_bs=n_po + 2, family="pair", nt=5))
    E.append(case("batch2-pair-odd-t_bs", **pb, batch=2, t_bs=n_pt + 1, family="deep", nt=5))
    E.append(case("batch2-pair-odd-o_bs", **pb, batch=2, o_bs=n_po + 3, family="deep", nt=5))
    return tuple(E)


EDGE_CASES = _edge_cases()


# ---- inputs --------------------------------------------------------------------------------------------------------
def _seed(c):
    return [c.A % 65521, c.K, c.J, c.B % 65521, int(c.last), c.batch, c.ldc]


def integer_inputs(c):
    """T [batch, A, K, B] and Cm [batch or 1, K, J] as fp64 arrays of integers in [-VMAX, VMAX], drawn independently
    for every element: no symmetry, no repeated slab, row or column for a swapped index to hide behind."""
    rng = np.random.default_rng(_seed(c))
    T = rng.integers(-VMAX, VMAX + 1, (c.batch, c.A, c.K, c.B)).astype(np.float64)
    Cm = rng.integers(-VMAX, VMAX + 1, (1 if c.c_bs == 0 else c.batch, c.K, c.J)).astype(np.float64)
    return T, Cm


def real_inputs(c, scaled=False):
    """Standard normal T and Cm; ``scaled``: row k of Cm times 2^+300 or 2^-300 (drawn per row)."""
    rng = np.random.default_rng(_seed(c) + [1])
    T = rng.standard_normal((c.batch, c.A, c.K, c.B))
    Cm = rng.standard_normal((1 if c.c_bs == 0 else c.batch, c.K, c.J))
    if scaled:
        Cm = Cm * np.ldexp(1.0, 300 * rng.choice((-1, 1), c.K))[None, :, None]
    return T, Cm


def product(T, Cm, dtype=np.float64):
    """out [batch, A, J, B] = sum_k Cm[., k, j] T[., a, k, b] in ``dtype`` (np.int64: the truth of the integer inputs)"""
    T, Cm = T.astype(dtype), Cm.astype(dtype)
    out = np.empty((T.shape[0], T.shape[1], Cm.shape[2], T.shape[3]), dtype=dtype)
    for b in range(T.shape[0]):
        Ct = np.ascontiguousarray(Cm[b if Cm.shape[0] > 1 else 0].T)
        for a in range(T.shape[1]):
            np.matmul(Ct, T[b, a], out=out[b, a])
    return out


def exact_reference(c, T, Cm):
    """The integer result as fp64.  LAST cases come as T [batch, A, K, 1]: one product T Cm per element."""
    if c.last:
        return np.stack([T[b, :, :, 0] @ Cm[b if Cm.shape[0] > 1 else 0] for b in range(c.batch)])[..., None]
    return product(T, Cm)


def sample(n):
    """Indices along the streamed dimension (b for INNER, rows a for LAST) for the rounded cases: the first and the
    last 33 and both sides of every 16-element boundary (hence of every 32-element one)."""
    idx = set(range(min(33, n))) | set(range(max(0, n - 33), n))
    for edge in range(16, n, 16):
        idx.update((edge - 1, edge))
    return np.array(sorted(idx))


def rounded_reference(c, T, Cm, idx):
    """(reference in longdouble, bound) on the sample idx of the streamed dimension.  The bound of a length-K dot
    product summed in fp64 in any order, with or without fused multiply-adds: each of at most K products and K - 1
    sums rounds once, (1 + u)^K - 1 <= (K + 2) u for K u < 0.01; the longdouble reference's own error is 2^-11 of it."""
    if c.last:
        Ts = T[:, idx, :, :]
        ref = np.stack([Ts[b, :, :, 0].astype(LD) @ Cm[b if Cm.shape[0] > 1 else 0].astype(LD)
                        for b in range(c.batch)])[..., None]
        mag = np.stack([np.abs(Ts[b, :, :, 0]) @ np.abs(Cm[b if Cm.shape[0] > 1 else 0])
                        for b in range(c.batch)])[..., None]
    else:
        Ts = np.ascontiguousarray(T[:, :, :, idx])
        ref = product(Ts, Cm, LD)
        mag = product(np.abs(Ts), np.abs(Cm))
    return ref, (c.K + 2) * U * mag * (1 + 4 * U)      # (the fp64 sum of magnitudes may itself round down)


# the builds the rounded cases and the isolation / identity tests visit: every family and mode at its widest build,
# at an even and an odd tile count in between, and at nt = 1
def builds_with_nt(nts):
    return tuple(c for c, b in zip(BUILD_CASES, BUILDS) if b[3] in nts)
