"""The plan of a batched evaluation (csrc/plan.h: oovqe_eval_plan, seen through oovqe_oo_eval_plan_describe) on the
CPU: which of the six paths a shape takes, which stage-1 kernel, where the circuit goes, how many launches, and
where the workspace blocks lie.  Without a device the library plans for 256 CUs, the MI355X's own count.

Expected values: tests/golden/eval_plan_parent.json holds the launches (kernel, grid, workgroup, LDS bytes) that the
commit BEFORE the plan existed made for each shape, recorded from a build of it whose HIP launch entry points were
replaced by a recorder (tools/launch_recorder: record.py's docstring is the recipe); path, circuit placement, W and
launch count are read off those launches here."""
import json
import os

import pytest

from auto_oo_amd import _lib, excitations as X, ops

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "eval_plan_parent.json")) as _fh:
    RECORDED = json.load(_fh)

PATH_OF_KERNEL = (("cas_tail_kernel", "packed_tail"), ("sym_gm_kernel", "packed_split"),
                  ("sym_q_contract_kernel", "packed_two_step"), ("half_transform_fused_kernel", "fused"),
                  ("cas_column_kernel", "column"), ("fock_rows_kernel", "staged"), ("fock_kernel", "staged"))
CIRCUIT_KERNELS = ("circuit_rdm_small_kernel", "circuit_kernel")


def _circuit(ncas, nelecas):
    gates, n_theta = X.uccd_gates(ncas, nelecas, False)
    return n_theta, len(gates)


def _n_kappa(N, n_occ, ncas):
    return len(X.non_redundant_indices(list(range(n_occ)), list(range(n_occ, n_occ + ncas)),
                                       list(range(n_occ + ncas, N)), False))


def _plan(N, n_occ, ncas, nelecas, batch, flags, packed, derivatives=True, circuit=True):
    n_theta, n_gates = _circuit(ncas, nelecas)
    return ops.eval_plan(N, n_occ, ncas, _n_kappa(N, n_occ, ncas), batch, flags, packed, n_theta, n_gates,
                         derivatives, circuit)


def _read_off(row):
    """(path, circuit placement, w, launches) of a recorded launch sequence"""
    names = [ln.split(" grid=")[0].split("<")[0] for ln in row["log"]]
    path = next(p for k, p in PATH_OF_KERNEL if k in names)
    own = [ln for ln in row["log"] if ln.split(" grid=")[0] in CIRCUIT_KERNELS]
    circuit = "none" if not row["circuit"] else "own" if own else "rides"
    w = bool(own) and own[0].split(" grid=")[1].split(",")[0] == str(2 * row["batch"])
    return path, circuit, w, len(row["log"])


# The table of the issue that introduced the plan: a small UCC circuit, derivatives on, a packed copy held when both
# flags are set.  (N, n_occ, ncas, batch, flags) -> path, stage-1 kernel, circuit, w, kernel launches
TABLE = [
    ((43, 6, 3, 6, 3), "column", "half_transform_kernel<1,11,3> (slabs p <= q)", "rides", False, 4),
    ((43, 6, 3, 7, 3), "packed_split", "half_tri_reg_kernel<11,3,8,3>", "rides", False, 4),
    ((43, 6, 3, 192, 3), "packed_split", "half_tri_reg_kernel<11,3,8,3>", "rides", False, 4),
    ((43, 6, 3, 193, 3), "packed_tail", "half_tri_reg_kernel<11,3,8,3>", "own", True, 3),
    ((43, 6, 3, 256, 3), "packed_tail", "half_tri_reg_kernel<11,3,8,3>", "own", True, 3),
    ((43, 6, 3, 129, 1), "packed_split", "half_tri_kernel<11,3,0>", "own", True, 5),
    ((43, 6, 3, 256, 1), "packed_split", "half_tri_kernel<11,3,0>", "own", True, 5),
    ((43, 6, 3, 7, 0), "fused", "half_transform_fused_kernel<11,3>", "rides", False, 4),
    ((43, 6, 3, 256, 0), "fused", "half_transform_fused_kernel<11,3>", "rides", False, 4),
    ((20, 6, 3, 30, 3), "column", "half_transform_kernel<1,8,2> (slabs p <= q)", "rides", False, 4),
    ((20, 6, 3, 31, 3), "packed_split", "half_tri_reg_kernel<8,2,5,3>", "rides", False, 4),
    ((20, 6, 3, 193, 3), "packed_tail", "half_tri_reg_kernel<8,2,5,3>", "own", True, 3),
    ((13, 6, 3, 72, 3), "column", "half_transform_kernel<1,4,1> (slabs p <= q)", "rides", False, 4),
    ((13, 6, 3, 73, 3), "fused", "half_transform_fused_kernel<4,1>", "rides", False, 4),      # the packed workspace bound fails
    ((13, 6, 3, 193, 3), "fused", "half_transform_fused_kernel<4,1>", "own", False, 5),       # at this shape
    ((48, 12, 4, 40, 3), "column", "half_transform_kernel<1,12,3> (slabs p <= q)", "own", False, 7),   # general circuit path: 3 launches
    ((24, 18, 3, 2, 3), "staged", "half_transform_kernel<2,8,2> (slabs p <= q)", "own", False, 14),    # 1 + 1 + 2 * 6
    ((56, 6, 3, 4, 3), "column", "half_tiles_kernel<1,8>", "own", False, 5),
]


@pytest.mark.parametrize("shape, path, stage1, circuit, w, launches", TABLE, ids=lambda v: str(v) if isinstance(v, tuple) else None)
def test_plan_table(shape, path, stage1, circuit, w, launches):
    N, n_occ, ncas, batch, flags = shape
    # the literal row against the parent's recorded launches ...
    row = next(r for r in RECORDED if r["table"] and (r["N"], r["n_occ"], r["ncas"], r["batch"], r["flags"]) == shape)
    assert _read_off(row) == (path, circuit, w, launches) and row["stage1"] == stage1
    # ... and against the plan
    p = _plan(N, n_occ, ncas, 4, batch, flags, flags == 3)
    assert (p["path"], p["stage1"], p["circuit"], p["w"], p["launches"]) == (path, stage1, circuit, w, launches)


def test_plan_equals_what_the_parent_launched():
    """Every recorded shape (the table, a spread of the N / batch / flags sweep with and without a packed copy,
    energy-only and RDM-given calls): the plan names the path, circuit placement, W, stage-1 kernel and launch count
    of the launches the parent made."""
    assert len(RECORDED) > 300 and sum(r["table"] for r in RECORDED) == len(TABLE)
    seen = set()
    for row in RECORDED:
        p = ops.eval_plan(row["N"], row["n_occ"], row["ncas"], _n_kappa(row["N"], row["n_occ"], row["ncas"]), row["batch"],
                          row["flags"], row["packed"], row["n_theta"], row["n_gates"], row["derivatives"], row["circuit"])
        got = (p["path"], p["circuit"], p["w"], p["launches"], p["stage1"])
        assert got == _read_off(row) + (row["stage1"],), row
        seen.add(p["path"])
    assert seen == {"packed_tail", "packed_split", "fused", "column", "staged"}    # (two-step: options only)


def _assert_structure(p, N, n_occ, ncas, nrdm, batch, flags, packed):
    work = batch * _lib.load().oovqe_cas_eval_work_size(N, n_occ, ncas, nrdm)
    spans = sorted(p["blocks"].values())
    assert spans and spans[0][0] >= 0 and spans[-1][0] + spans[-1][1] <= work
    for (o0, l0), (o1, _) in zip(spans, spans[1:]):
        assert o0 + l0 <= o1, p["blocks"]
    if p["w"]:
        assert p["path"] in ("packed_tail", "packed_split") and p["circuit"] == "own"
        assert p["blocks"]["T3"][1] == batch * N * N
    if p["path"] == "packed_tail":
        assert p["w"] and flags == 3 and packed
    if p["circuit"] == "rides":
        # the contraction dispatcher's own answer for the K1 launch this path makes (sym_gm_kernel, the host on the
        # one-step packed path, is built with the circuit workgroups for every shape it serves)
        assert p["path"] == "packed_split" or p["k1_hosts"], p
    assert p["launches"] >= sum(p["labels"].values())


def test_plan_properties():
    """Structure of every plan over N = 1..64, several active spaces, batches on both sides of every threshold and
    all flag combinations: the blocks a path uses lie inside the workspace and apart from each other, W only on a
    packed path with the circuit in its own launch, the one-launch tail only with W, both flags and a packed copy, a
    riding circuit only where oovqe_contract_hosts_circuit accepts the K1 launch that hosts it (k1_hosts)."""
    n = rides = 0
    for n_occ, ncas, nelecas in ((0, 1, 2), (0, 2, 2), (1, 2, 2), (6, 3, 4), (2, 4, 4), (12, 4, 4), (18, 3, 4), (30, 3, 4)):
        # (one active orbital has no excitation to build a UCC circuit from: the plan only sees the sizes)
        n_theta, n_gates = _circuit(ncas, nelecas) if ncas > 1 else (1, 1)
        for N in range(n_occ + ncas, 65):
            n_kappa = _n_kappa(N, n_occ, ncas)
            for batch in (1, 7, 64, 129, 256, 300, 385, 40000):
                for flags, packed in ((0, False), (1, False), (3, False), (3, True)):
                    for circuit in (True, False):
                        try:
                            p = ops.eval_plan(N, n_occ, ncas, n_kappa, batch, flags, packed, n_theta, n_gates, True, circuit)
                        except _lib.OovqeError as err:
                            # the one shape nothing serves: large N * M^2 without a virtual orbital
                            assert "at least one virtual orbital" in str(err) and N == n_occ + ncas
                            continue
                        assert (p["circuit"] == "none") == (not circuit)
                        _assert_structure(p, N, n_occ, ncas, 1 + n_theta, batch, flags, packed)
                        n += 1
                        rides += p["circuit"] == "rides" and p["path"] != "packed_split"
    assert n > 15000 and rides > 1000


def test_w_stays_out_of_g_mo():
    """n_occ + ncas = 3: W [N][N] is larger than the T3 block [N][27] once N > 27, and g_mo lies behind that block.
    The circuit's launch then leaves no W (the panel kernel forms its rows of C^T h itself) -- unless the one-launch
    tail runs, which forms no g_mo in memory."""
    for N, w in ((27, True), (28, False), (43, False)):
        p = _plan(N, 1, 2, 2, 400, 1, False)
        assert p["path"] == "packed_split" and p["circuit"] == "own" and p["w"] == w
    p = _plan(43, 1, 2, 2, 400, 3, True)
    assert p["path"] == "packed_tail" and p["w"]
