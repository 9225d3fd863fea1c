"""Probe: one ``gto.gradient_sets_into`` call for K density sets per geometry against K calls of ``gto.gradient_into``
on the same densities -- the way to the same numbers without the sets entry.

Stack: G = 64 points of the formaldimine ring (STO-3G, N = 13, 5 atoms), K = 3 (two states and their coupling) and
K = 10 (four states), seeded symmetric D1, WQ and 8-fold symmetric D2 per set, all terms and the nuclear term.  The two
routes are timed alternately, ``reps`` times each after ``warmup`` calls of both (host clock around a stream
synchronise); per route the median, the smallest and the largest time are reported, and the ratio of the medians.  The
sets call counts as faster only when its largest time is below the smallest time of the K calls.  The results of the two
routes are compared (largest absolute difference) so that faster does not mean different.

One JSON line per K.  Not part of bench.py.

  python tools/time_gradient_sets.py [--geometries 64] [--sets 3 10] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from auto_oo_amd import _lib, gto                                   # noqa: E402
from auto_oo_amd.moldata import get_formal_geo                      # noqa: E402

F64 = torch.float64


def ring(G):
    return [get_formal_geo(130.0 + 10.0 * np.cos(2 * np.pi * k / G + np.pi / 20),
                           89.9 + 10.0 * np.sin(2 * np.pi * k / G + np.pi / 20)) for k in range(G)]


def seeded_sets(G, K, N, device):
    rng = np.random.default_rng(7)
    d1, wq = rng.standard_normal((2, G, K, N, N))
    d2 = rng.standard_normal((G, K) + (N,) * 4)
    d1, wq = d1 + d1.transpose(0, 1, 3, 2), wq + wq.transpose(0, 1, 3, 2)
    d2 = d2 + d2.transpose(0, 1, 3, 2, 4, 5)
    d2 = d2 + d2.transpose(0, 1, 2, 3, 5, 4)
    d2 = d2 + d2.transpose(0, 1, 4, 5, 2, 3)
    return tuple(torch.as_tensor(x).to(device).contiguous() for x in (d1, wq, d2))


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--geometries", type=int, default=64)
    ap.add_argument("--sets", type=int, nargs="+", default=[3, 10])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    device = _lib.require_device()
    G = a.geometries
    basis = gto.GTOBasis(["N", "C", "H", "H", "H"])
    xyz = gto.coords_to_device(basis, ring(G), device)
    N = basis.nao
    for K in a.sets:
        d1, wq, d2 = seeded_sets(G, K, N, device)
        singles = [tuple(t[:, k].contiguous() for t in (d1, wq, d2)) for k in range(K)]
        one_call = lambda: gto.gradient_sets_into(basis, xyz, d1, wq, d2, True)                      # noqa: E731
        k_calls = lambda: torch.stack([gto.gradient_into(basis, xyz, *s, True) for s in singles], dim=1)   # noqa: E731
        for _ in range(a.warmup):
            one_call()
            k_calls()
        torch.cuda.synchronize()
        t_sets, t_single = [], []
        for _ in range(a.reps):
            t, got = timed(one_call)
            t_sets.append(t)
            t, want = timed(k_calls)
            t_single.append(t)
        stats = lambda t: {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t))}  # noqa: E731
        print(json.dumps({
            "G": G, "N": N, "natm": basis.natm, "K": K, "tile": gto.GRAD_SETS_TILE, "reps": a.reps,
            "sets_call_ms": stats(t_sets), "k_single_calls_ms": stats(t_single),
            "k_calls_over_sets_call": float(np.median(t_single) / np.median(t_sets)),
            "faster_beyond_the_spread": bool(np.max(t_sets) < np.min(t_single)),
            "max_abs_difference_of_the_two": float((got - want).abs().max().item()),
            "max_abs_gradient": float(want.abs().max().item())}), flush=True)


if __name__ == "__main__":
    main()
