"""Probe: timing of the orbital-relaxed CASCI gradients (OO_pqc_batch.casci_relaxed_gradients) beside the fixed-orbital
ones (casci_nuclear_gradients) on the same batch.

Stacks: the formaldimine ring (STO-3G, N = 13, CAS(2e,2o), R = 2 roots, device RHF orbitals) at G = 1, 64, 256.  Per
stack, after warm-up, the two methods are called alternately `reps` times; the median wall time of a call (stream
synchronised) is reported.  A second pass wraps ``nucgrad.zvector`` and ``nucgrad.relaxed_densities`` in synchronised
clocks to split the extra time (the synchronisations make this pass slower than the first: only its shares are used),
and reads the iteration counts.  A third part times ``scf.fock_jk_sets`` with two densities against two ``scf.fock_jk``
calls on the batch's integrals.  One JSON line per stack and part.

  python tools/bench_relaxed_gradients.py                  the timings
  python tools/bench_relaxed_gradients.py --fixed-only     casci_nuclear_gradients alone (what another checkout has)
  python tools/bench_relaxed_gradients.py --root DIR       import auto_oo_amd from DIR instead of this checkout
  python tools/bench_relaxed_gradients.py --trace G        one relaxed call on a warm stack and nothing else timed, to be
                                                           run under ``rocprofv3 --kernel-trace --stats``
  python tools/bench_relaxed_gradients.py --stats FILE     the Fock and step kernels' time per launch from such a run's
                                                           kernel_stats.csv
Not part of bench.py."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np


def ring_batch(aoo, gto, get_formal_geo, G):
    """G points of the Berry-phase notebook's loop (origin (130, 89.9), radii (10, 10) degrees, phase pi / 20)."""
    basis = gto.GTOBasis(["N", "C", "H", "H", "H"])
    geos = [get_formal_geo(130.0 + 10.0 * np.cos(2 * np.pi * k / G + np.pi / 20),
                           89.9 + 10.0 * np.sin(2 * np.pi * k / G + np.pi / 20)) for k in range(G)]
    pqc = aoo.Parameterized_circuit(2, 2, None, ansatz="np_fabric", n_layers=1)
    return aoo.OO_pqc_batch.from_geometries(pqc, basis, basis.coordinates(geos), 2, 2, oao_mo_coeffs="rhf")


def clock(torch, f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def stats(path):
    rows = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            rows[r["Name"]] = r
    out = {}
    for key in ("fock_jk_sets_kernel", "zvector_step_kernel", "response_d2_kernel", "scf_fock_jk_kernel"):
        hit = [v for k, v in rows.items() if key in k]
        if hit:
            out[key] = {"calls": int(hit[0]["Calls"]),
                        "us_per_launch": 1e-3 * float(hit[0]["TotalDurationNs"]) / max(int(hit[0]["Calls"]), 1)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 64, 256])
    ap.add_argument("--fixed-only", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--trace", type=int, metavar="G")
    ap.add_argument("--stats", metavar="FILE")
    a = ap.parse_args()
    if a.stats:
        return stats(a.stats)
    sys.path.insert(0, a.root)
    import torch
    import auto_oo_amd as aoo
    from auto_oo_amd import gto, nucgrad, scf
    from auto_oo_amd.moldata import get_formal_geo

    if a.trace:
        b = ring_batch(aoo, gto, get_formal_geo, a.trace)
        b.casci_relaxed_gradients(nroots=2)
        torch.cuda.synchronize()
        res = b.casci_relaxed_gradients(nroots=2)
        torch.cuda.synchronize()
        print(json.dumps({"G": a.trace, "relaxed_calls": 2, "z_info_zero": bool((res.z_info == 0).all().item())}))
        return

    relaxed = not a.fixed_only and hasattr(aoo.OO_pqc_batch, "casci_relaxed_gradients")
    for G in a.sizes:
        b = ring_batch(aoo, gto, get_formal_geo, G)
        fixed_call = lambda: b.casci_nuclear_gradients(nroots=2)
        relaxed_call = lambda: b.casci_relaxed_gradients(nroots=2)
        for _ in range(a.warmup):
            fixed_call()
            if relaxed:
                relaxed_call()
        tf, tr = [], []
        for _ in range(a.reps):                                      # alternating
            tf.append(clock(torch, fixed_call)[0])
            if relaxed:
                tr.append(clock(torch, relaxed_call)[0])
        row = {"part": "calls", "G": G, "reps": a.reps, "casci_nuclear_gradients_ms": 1e3 * float(np.median(tf)),
               "casci_nuclear_gradients_ms_min_max": [1e3 * min(tf), 1e3 * max(tf)]}
        if relaxed:
            row.update({"casci_relaxed_gradients_ms": 1e3 * float(np.median(tr)),
                        "casci_relaxed_gradients_ms_min_max": [1e3 * min(tr), 1e3 * max(tr)]})
        print(json.dumps(row), flush=True)
        if not relaxed:
            continue

        # the split of the extra time, synchronised clocks around the two new stages
        spent = {"zvector": [], "relaxed_densities": []}
        last = {}
        originals = {k: getattr(nucgrad, k) for k in spent}

        def wrap(name):
            def timed(*args, **kw):
                t, out = clock(torch, lambda: originals[name](*args, **kw))
                spent[name].append(t)
                last[name] = out
                return out
            return timed
        for k in spent:
            setattr(nucgrad, k, wrap(k))
        try:
            total = [clock(torch, relaxed_call)[0] for _ in range(a.reps)]
        finally:
            for k, f in originals.items():
                setattr(nucgrad, k, f)
        it = last["zvector"].iterations.cpu().numpy()
        print(json.dumps({"part": "split", "G": G, "call_ms": 1e3 * float(np.median(total)),
                          "zvector_ms": 1e3 * float(np.median(spent["zvector"])),
                          "relaxed_densities_ms": 1e3 * float(np.median(spent["relaxed_densities"])),
                          "iterations_min": int(it.min()), "iterations_max": int(it.max()),
                          "iterations_mean": float(it.mean())}), flush=True)

        # one pass with two densities against two passes with one
        g = b.int2e_ao
        d = torch.randn((G, 2, b.nao, b.nao), dtype=torch.float64, device=g.device,
                        generator=torch.Generator(device=g.device).manual_seed(5))
        d0, d1 = d[:, 0].contiguous(), d[:, 1].contiguous()
        n_inner = 20
        one = lambda: [scf.fock_jk_sets(g, d) for _ in range(n_inner)]
        two = lambda: [(scf.fock_jk(g, d0), scf.fock_jk(g, d1)) for _ in range(n_inner)]
        one(), two()
        t1, t2 = [], []
        for _ in range(a.reps):
            t1.append(clock(torch, one)[0] / n_inner)
            t2.append(clock(torch, two)[0] / n_inner)
        print(json.dumps({"part": "fock", "G": G, "fock_jk_sets_2_us": 1e6 * float(np.median(t1)),
                          "two_fock_jk_us": 1e6 * float(np.median(t2))}), flush=True)
        del b, g, d
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
