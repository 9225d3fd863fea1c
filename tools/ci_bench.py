"""Probe: timing of the batched determinant-CI solver (oovqe_ci_davidson_batch, one launch per call).

Random 8-fold-symmetric active-space coefficients, G in {1, 16, 256} problems x CAS(2e,2o), (4e,4o), (8e,8o), one
root, singlets; each call timed with HIP events after warm-up calls (median of the timed calls).  Prints one JSON line
per shape: us per stack, us per geometry.  Not part of bench.py."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from auto_oo_amd import ci as CI                   # noqa: E402
from tests import _ci_dense as D                   # noqa: E402


def main(reps=10, warm=3):
    rng = np.random.default_rng(0)
    dev = torch.device("cuda", 0)
    for a in (2, 4, 8):
        c0, c1, c2 = zip(*[D.random_coefficients(a, rng) for _ in range(8)])
        for G in (1, 16, 256):
            idx = np.arange(G) % 8
            coef = torch.as_tensor(np.concatenate([np.array(c0)[idx, None], np.stack(c1)[idx].reshape(G, -1),
                                                   np.stack(c2)[idx].reshape(G, -1)], axis=1), device=dev)
            for _ in range(warm):
                out = CI.casci_packed(coef, 1, a, a)
            torch.cuda.synchronize()
            times = []
            for _ in range(reps):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                out = CI.casci_packed(coef, 1, a, a)
                e.record()
                e.synchronize()
                times.append(s.elapsed_time(e) * 1e3)
            info = out[4].cpu()
            us = float(np.median(times))
            print(json.dumps({"ncas": a, "nelecas": a, "G": G, "Dc": CI.ci_dimension(a, a), "us_per_stack": us,
                              "us_per_geometry": us / G, "all_converged": bool((info == 0).all())}), flush=True)


if __name__ == "__main__":
    main()
