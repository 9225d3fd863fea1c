"""Probe: the state-averaged evaluation (auto_oo_amd/ensemble.py, csrc/ensemble.hip) on a stack of the bench's headline
shape (N = 43, CAS(4e,3o), UCCD, 256 geometries), S = 2 singlet states with equal weights, next to the route it
replaces: S calls of ``OO_pqc_batch.energy_and_gradient`` (one per state; that path is untouched by the ensemble, so it
stands for the code as it was).

Timed with HIP events around one call each, after ``warmup`` calls of both, the two alternating call by call in the same
run (median, smallest, largest per call):
  ensemble   -- ``SA_OO_pqc_batch.energy_and_gradient``: oovqe_ensemble_states, oovqe_ensemble_rdms, one CAS evaluation
                of the stack (one N^4 sweep);
  front_end  -- the two ensemble launches alone (states + tangents, weighted RDM sets);
  per_state  -- ``S`` calls of ``OO_pqc_batch.energy_and_gradient`` back to back (``S`` N^4 sweeps);
  one_call   -- one such call.
``ratio_to_one_call`` = ensemble / one_call (the expectation: about 1, not S); ``ratio_to_per_state`` = ensemble /
per_state.  No threshold is asserted.  One JSON line.  Not part of bench.py.

  python tools/time_ensemble.py [--geoms 256] [--states 2] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import auto_oo_amd as aoo                                           # noqa: E402
import bench                                                        # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b)                                   # microseconds


def summary(x):
    return dict(median_us=float(np.median(x)), min_us=float(min(x)), max_us=float(max(x)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--geoms", type=int, default=bench.N_GEOM)
    ap.add_argument("--states", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    pqc, batch, _, thetas = bench.build_geometries(list(range(a.geoms)))
    S = a.states
    sa = aoo.SA_OO_pqc_batch(batch, aoo.StateEnsemble(pqc, nstates=S))
    thetas = thetas.contiguous()

    calls = dict(
        ensemble=lambda: sa.energy_and_gradient(thetas),
        front_end=lambda: sa._rdms(sa._states(thetas, None), sa.n_theta, False),
        per_state=lambda: [batch.energy_and_gradient(thetas) for _ in range(S)],
        one_call=lambda: batch.energy_and_gradient(thetas))
    for _ in range(a.warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, fn in calls.items():
            times[k].append(timed(fn))
    # the two routes agree where they must: with the HF determinant alone the ensemble is the single-state evaluation
    one = aoo.SA_OO_pqc_batch(batch, aoo.StateEnsemble(pqc, nstates=1))
    diff = float((one.energy_and_gradient(thetas) - batch.energy_and_gradient(thetas)).abs().max().item())
    res = dict(shape=dict(N=bench.NAO, cas=f"({bench.NELECAS}e,{bench.NCAS}o)", n_theta=sa.n_theta,
                          n_kappa=sa.n_kappa, geometries=a.geoms, states=S),
               reps=a.reps, warmup=a.warmup, **{k: summary(v) for k, v in times.items()},
               ratio_to_one_call=float(np.median(times["ensemble"]) / np.median(times["one_call"])),
               ratio_to_per_state=float(np.median(times["ensemble"]) / np.median(times["per_state"])),
               max_abs_diff_one_state_to_single_state_route=diff)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
