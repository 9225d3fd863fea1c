"""Probe: timing of the device Hartree-Fock solver (scf.rhf_batch) against the host route it replaces.

Stacks: the formaldimine ring (STO-3G, N = 13, n_occ = 8) at G = 1, 16, 64, 256 and synthetic N = 43 problems
(n_occ = 8) at G = 1, 16, 64.  Two alternating passes over all stacks; in each pass a stack is solved `reps` times after
warm-up and the median wall time of a call (stream synchronised) is reported beside the iteration counts.  The host route
is what ``from_geometries(oao_mo_coeffs=None)`` does: the three integral tensors copied to the host, then
``gaussian.rhf`` geometry by geometry (at N = 43 it is timed for at most --host-max geometries).  One JSON line per
stack and pass.

  python tools/rhf_bench.py                      the timings
  python tools/rhf_bench.py --trace N G          four iterations of one stack and nothing else, to be run under
                                                 ``rocprofv3 --kernel-trace --stats`` (no geometry converges in four
                                                 iterations, so every launch works on the whole stack)
  python tools/rhf_bench.py --stats FILE N G     per-iteration split of such a run's kernel_stats.csv: Fock contraction
                                                 and step kernel, and the contraction's fraction of 8 TB/s over its
                                                 algorithmic 8 N^4 G bytes
Not part of bench.py."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from auto_oo_amd import gaussian, gto, scf                          # noqa: E402
from auto_oo_amd.moldata import get_formal_geo                      # noqa: E402
from auto_oo_amd.synthetic import synthetic_problem_device          # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def ring_stack(G):
    """G points of the Berry-phase notebook's loop (origin (130, 89.9), radii (10, 10) degrees, phase pi / 20)."""
    basis = gto.GTOBasis(["N", "C", "H", "H", "H"])
    geos = [get_formal_geo(130.0 + 10.0 * np.cos(2 * np.pi * k / G + np.pi / 20),
                           89.9 + 10.0 * np.sin(2 * np.pi * k / G + np.pi / 20)) for k in range(G)]
    I = gto.integrals_batch(basis, geos)
    return I.int1e_ao, I.int2e_ao, I.overlap, basis.nelectron // 2


def synthetic_stack(G, n=43):
    dev = torch.device("cuda", 0)
    P = [synthetic_problem_device(n, 1000 + k, dev) for k in range(G)]
    return (torch.stack([p["int1e_ao"] for p in P]), torch.stack([p["int2e_ao"] for p in P]),
            torch.stack([p["overlap"] for p in P]).contiguous(), 8)


def stack(n, G):
    return ring_stack(G) if n == 13 else synthetic_stack(G, n)


def time_device(h, g, S, n_occ, reps, warm):
    for _ in range(warm):
        res = scf.rhf_batch(h, g, S, n_occ)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = scf.rhf_batch(h, g, S, n_occ)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), res


def time_host(h, g, S, n_occ, count):
    t0 = time.perf_counter()
    hh, gh, Sh = h[:count].cpu().numpy(), g[:count].cpu().numpy(), S[:count].cpu().numpy()
    t1 = time.perf_counter()
    for k in range(count):
        gaussian.rhf(hh[k], gh[k], Sh[k], n_occ)
    return t1 - t0, time.perf_counter() - t1


def run(reps, warm, host_max):
    shapes = [(13, G) for G in (1, 16, 64, 256)] + [(43, G) for G in (1, 16, 64)]
    for p in range(2):
        for n, G in shapes:
            h, g, S, n_occ = stack(n, G)
            t, res = time_device(h, g, S, n_occ, reps, warm)
            it = res.iterations.cpu().numpy()
            row = {"pass": p, "N": n, "G": G, "device_ms_per_stack": 1e3 * t, "device_ms_per_geometry": 1e3 * t / G,
                   "iterations_min": int(it.min()), "iterations_max": int(it.max()),
                   "converged": int(res.converged.sum().item())}
            if p == 0:
                count = G if n == 13 else min(G, host_max)
                t_copy, t_rhf = time_host(h, g, S, n_occ, count)
                row.update({"host_geometries_timed": count, "host_copy_ms": 1e3 * t_copy, "host_rhf_ms": 1e3 * t_rhf,
                            "host_ms_per_stack": 1e3 * (t_copy + t_rhf) * G / count})
            print(json.dumps(row), flush=True)
            del h, g, S, res
            torch.cuda.empty_cache()


def trace(n, G):
    h, g, S, n_occ = stack(n, G)
    torch.cuda.synchronize()
    res = scf.rhf_batch(h, g, S, n_occ, max_cycle=4)
    torch.cuda.synchronize()
    print(json.dumps({"N": n, "G": G, "iterations": res.iterations.cpu().tolist()[:4], "fock_launches": 4,
                      "step_launches": 5}))


def stats(path, n, G):
    rows = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            rows[r["Name"]] = r
    def pick(key):                                                  # noqa: E306
        hit = [v for k, v in rows.items() if key in k]
        return (float(hit[0]["TotalDurationNs"]), int(hit[0]["Calls"])) if hit else (float("nan"), 0)
    f_ns, f_calls = pick("scf_fock_jk_kernel")
    s_ns, s_calls = pick("scf_step_kernel")
    x_ns, x_calls = pick("sym_invsqrt_kernel")
    fock_us, step_us = 1e-3 * f_ns / max(f_calls, 1), 1e-3 * s_ns / max(s_calls, 1)
    nbytes = 8.0 * n ** 4 * G
    print(json.dumps({"N": n, "G": G, "fock_us_per_iteration": fock_us, "step_us_per_iteration": step_us,
                      "invsqrt_us": 1e-3 * x_ns / max(x_calls, 1), "fock_calls": f_calls, "step_calls": s_calls,
                      "fock_bytes": nbytes, "fock_fraction_of_8TBps": nbytes / (fock_us * 1e-6) / HBM_BYTES_PER_S}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-max", type=int, default=4, help="geometries of an N = 43 stack the host route is timed on")
    ap.add_argument("--trace", nargs=2, type=int, metavar=("N", "G"))
    ap.add_argument("--stats", nargs=3, metavar=("FILE", "N", "G"))
    a = ap.parse_args()
    if a.stats:
        stats(a.stats[0], int(a.stats[1]), int(a.stats[2]))
    elif a.trace:
        trace(*a.trace)
    else:
        run(a.reps, a.warmup, a.host_max)


if __name__ == "__main__":
    main()
