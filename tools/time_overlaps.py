"""Time the batched state overlaps against the per-pair host route of berry.py.

    python tools/time_overlaps.py [--reps 7]

Two sizes, each a closed loop of formaldimine geometries in STO-3G (``OO_pqc_batch.from_geometries``):

  ring64   64 points, ``ucc`` CAS(4e,3o), RHF orbitals of every point (dense-register engine)
  cas88    16 points, kUpCCD CAS(8e,8o), seeded orthogonal ``oao_mo_coeff`` (sector engine, 70 x 70 minors)

Routes, alternated after one warm-up round, each timed from the call to the values on the host:

  batched-oao  ``batch.state_overlaps(thetas, metric="oao")``: circuit states, U and all pairs in one kernel launch
  loop         per pair ``berry.bogoliubov_atob_cas`` + ``berry.state_overlap`` (the states are made once outside the
               timing: the loop is given that for free)
  batched-ao   ``batch.state_overlaps(thetas, metric="ao")``: the exact overlaps (cross overlap, core fold), for scale

Prints median / min / max per route in milliseconds and one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import auto_oo_amd as aoo                                            # noqa: E402
from auto_oo_amd import gto                                           # noqa: E402
from auto_oo_amd.berry import bogoliubov_atob_cas, state_overlap      # noqa: E402


def ring(n):
    return [aoo.get_formal_geo(130.0 + 10.0 * np.cos(2 * np.pi * k / n), 85.0 + 10.0 * np.sin(2 * np.pi * k / n))
            for k in range(n)]


def build(name):
    basis = gto.GTOBasis(["N", "C", "H", "H", "H"])
    if name == "ring64":
        pqc = aoo.Parameterized_circuit(3, 4, None, ansatz="ucc")
        batch = aoo.OO_pqc_batch.from_geometries(pqc, basis, basis.coordinates(ring(64)), 3, 4, oao_mo_coeffs="rhf")
    else:
        pqc = aoo.Parameterized_circuit(8, 8, None, ansatz="kupccd", k=1)
        rng = np.random.default_rng(11)
        base = np.linalg.qr(rng.standard_normal((13, 13)))[0]
        orbs = []
        for _ in range(16):          # neighbours differ by a small rotation, as along a tracked loop
            a = 0.05 * rng.standard_normal((13, 13))
            orbs.append(base @ np.linalg.qr(np.eye(13) + a - a.T)[0])
        batch = aoo.OO_pqc_batch.from_geometries(pqc, basis, basis.coordinates(ring(16)), 8, 8, oao_mo_coeffs=orbs)
    thetas = torch.as_tensor(np.random.default_rng(3).uniform(-0.3, 0.3, (batch.G, batch.n_theta))).to(batch.device)
    return pqc, batch, thetas


def routes(pqc, batch, thetas):
    G = batch.G
    states = [pqc.state_real(thetas[g]) for g in range(G)]
    orb = batch.oao_mo_coeff.cpu().numpy()

    def loop():
        out = []
        for a in range(G):
            b = (a + 1) % G
            rot = bogoliubov_atob_cas(orb[a].T @ orb[b], batch.act_idx, batch.nelecas)
            out.append(state_overlap(states[b], rot, states[a]).item())
        return np.array(out)

    return {"batched-oao": lambda: batch.state_overlaps(thetas, metric="oao").cpu().numpy(), "loop": loop,
            "batched-ao": lambda: batch.state_overlaps(thetas, metric="ao").cpu().numpy()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    result = {}
    for name in ("ring64", "cas88"):
        pqc, batch, thetas = build(name)
        fns = routes(pqc, batch, thetas)
        vals = {k: f() for k, f in fns.items()}                  # warm-up round
        diff = float(np.abs(vals["batched-oao"] - vals["loop"]).max())
        times = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, f in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                times[k].append(1e3 * (time.perf_counter() - t0))
        print(f"{name}: {batch.G} pairs, |batched-oao - loop| = {diff:.2e}, W(oao) = {np.prod(vals['batched-oao']):+.6f}, "
              f"W(ao) = {np.prod(vals['batched-ao']):+.6f}")
        result[name] = {"pairs": batch.G, "max_abs_diff": diff}
        for k, t in times.items():
            med, lo, hi = float(np.median(t)), float(min(t)), float(max(t))
            print(f"  {k:12s} median {med:10.3f} ms   min {lo:10.3f}   max {hi:10.3f}   ({args.reps} runs)")
            result[name][k] = {"median_ms": med, "min_ms": lo, "max_ms": hi}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
