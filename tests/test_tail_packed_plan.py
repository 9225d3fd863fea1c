"""cas_tail_kernel with p -> n over the packed columns only (the entries of g_mo[n] that stage 3 reads): the plan
still takes the one-launch tail wherever the commit before it did, within 160 KB of LDS, and the index maps of the
kernel -- position table, packed column of every accumulator row of q -> x, column tiles of p -> n -- emulated on the
host.  No device needed.

tests/golden/tail_plan_parent.json: path, tail build and LDS bytes that ops.eval_plan of the parent commit reports for
N = 17..48 with 6 core + 3 active orbitals at 256 geometries and for CAS(2e,2o) at N = 43 with 3 core orbitals (385
geometries) and with 6 (193)."""
import json
import os

import pytest

from auto_oo_amd import excitations as X, ops

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "tail_plan_parent.json")) as _fh:
    PARENT = json.load(_fh)


def _plan(N, n_occ, ncas, nelecas, batch):
    gates, n_theta = X.uccd_gates(ncas, nelecas, False)
    n_kappa = len(X.non_redundant_indices(list(range(n_occ)), list(range(n_occ, n_occ + ncas)),
                                          list(range(n_occ + ncas, N)), False))
    return ops.eval_plan(N, n_occ, ncas, n_kappa, batch, 3, True, n_theta, len(gates), True, True)


def test_fixture_covers_the_shapes():
    shapes = [(r["N"], r["n_occ"], r["ncas"], r["batch"]) for r in PARENT]
    assert shapes == [(N, 6, 3, 256) for N in range(17, 49)] + [(43, 3, 2, 385), (43, 6, 2, 193)]
    assert all(r["path"] == "packed_tail" for r in PARENT if r["N"] >= 33)


@pytest.mark.parametrize("row", PARENT, ids=lambda r: f"N{r['N']}-{r['n_occ']}+{r['ncas']}")
def test_plan_keeps_the_tail(row):
    p = _plan(row["N"], row["n_occ"], row["ncas"], row["nelecas"], row["batch"])
    if row["path"] != "packed_tail":
        return
    assert p["path"] == "packed_tail"
    assert p["tail"] == row["tail"]
    assert 0 < int(p["tail_lds"]) <= 160 * 1024


# ---- the kernel's index maps in plain Python ----------------------------------------------------------------------
def _needed(x, y, z, no):
    lo, hi = min(y, z), max(y, z)
    if lo >= no:
        return True
    if hi < no:
        return lo == hi or x == lo or x == hi
    return x >= no or x == lo


def _tables(M, no):
    """tab[(x, y, z)] and tabp[x * ncol + yz] as the kernel's prefix count over (x, y <= z) in order leaves them"""
    pairs = [(y, z) for y in range(M) for z in range(y, M)]
    tab, tabp, nc = {}, [], 0
    for x in range(M):
        for y, z in pairs:
            v = -1
            if _needed(x, y, z, no):
                v, nc = nc, nc + 1
            tab[(x, y, z)] = tab[(x, z, y)] = v
            tabp.append(v)
    return pairs, tab, tabp, nc


@pytest.mark.parametrize("M, no", [(9, 6), (5, 3), (8, 6)])
def test_index_maps(M, no):
    pairs, tab, tabp, nc = _tables(M, no)
    ncol, nty, nct = len(pairs), (len(pairs) + 15) // 16, (nc + 15) // 16
    pitch = 16 * (nct | 1)
    assert nc == sum(_needed(x, y, z, no) for x in range(M) for y, z in pairs)
    assert nc == {(9, 6): 210, (5, 3): 54, (8, 6): 138}[(M, no)]
    # the kept entries: distinct columns 0..NC-1 in the order (x, y <= z); (x, y, z) and (x, z, y) share one
    kept = [tab[(x, y, z)] for x in range(M) for y, z in pairs if _needed(x, y, z, no)]
    assert kept == list(range(nc))
    assert all(tab[(x, y, z)] == tab[(x, z, y)] for x in range(M) for y in range(M) for z in range(M))
    assert all((tab[(x, y, z)] >= 0) == _needed(x, y, z, no) for x in range(M) for y in range(M) for z in range(M))
    # q -> x: the accumulator rows of lane (lq, lr) in tile ty are (x = lq + 4 j, yz = 16 ty + lr); every kept column
    # is stored exactly once per row p, and nothing else
    stored = []
    for ty in range(nty):
        for lq in range(4):
            for lr in range(16):
                for j in range(4):
                    x, yz = lq + 4 * j, 16 * ty + lr
                    col = tabp[x * ncol + yz] if x < M and yz < ncol else -1
                    if col >= 0:
                        assert col == tab[(x,) + pairs[yz]]
                        stored.append(col)
    assert sorted(stored) == list(range(nc))
    # p -> n: the column tiles cover the kept columns inside the pitch; the operand reads of a group of 32 lanes
    # (two values of lq, sixteen of lr) fall on 64 distinct 4-byte banks
    tiles = {16 * ct + lr for ct in range(nct) for lr in range(16)}
    assert set(range(nc)) <= tiles and max(tiles) < pitch
    for half in (0, 2):
        banks = {(2 * ((half + dq) * pitch + lr) + w) % 64 for dq in range(2) for lr in range(16) for w in range(2)}
        assert len(banks) == 64
