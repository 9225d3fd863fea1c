"""Probe: the ADAPT-VQE pool gradients (csrc/pool.hip) at CAS(8e,8o) with the "gsd" pool (2 044 operators), for 1 and 256
states, next to the route they replace: one ``circuit_gradient`` evaluation per candidate with the gate appended.

Timed with HIP events around ``reps`` calls after ``warmup`` calls (median, smallest, largest per call):
  kernel   -- ``oovqe_pool_gradients_batch`` alone on resident psi and lam;
  call     -- ``oovqe_pool_gradients_from_coefficients_batch``: the operator on every state (per-state coefficients), then
              the kernel;
  replaced -- ``OO_pqc.circuit_gradient`` of the kUpCCD circuit with one pool operator appended at 0, for ``sample``
              operators spread over the pool (host clock around a synchronise, circuits built beforehand); the route
              needs P + 1 such evaluations per state, reported as mean x (P + 1) x states: an extrapolation, marked so.
The molecule is a seeded synthetic problem (N = 16); the states are kUpCCD states at seeded parameters.

One JSON line per batch size.  Not part of bench.py.

  python tools/time_pool_gradients.py [--batches 1 256] [--reps 20] [--warmup 3] [--sample 16]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import auto_oo_amd as aoo                                           # noqa: E402
from auto_oo_amd import _lib, adapt                                 # noqa: E402
from auto_oo_amd._lib import check, dptr, stream_ptr                # noqa: E402
from auto_oo_amd.synthetic import synthetic_problem                 # noqa: E402

F64 = torch.float64


def event_times(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(1e3 * a.elapsed_time(b))                          # microseconds
    return dict(median_us=float(np.median(out)), min_us=float(min(out)), max_us=float(max(out)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 256])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=16)
    a = ap.parse_args()
    lib = _lib.load()
    dev = _lib.require_device()
    N, ncas, nelecas, nelec = 16, 8, 8, 12
    P = synthetic_problem(N, 20261)
    mol = aoo.Moldata(P["int1e_ao"], P["int2e_ao"], P["overlap"], P["nuc"], nelec)
    pqc = aoo.Parameterized_circuit(ncas, nelecas, None, ansatz="kupccd", k=1)
    oo = aoo.OO_pqc(pqc, mol, ncas, nelecas, oao_mo_coeff=P["oao_mo_coeff"])
    eng = pqc._sector
    pool = aoo.OperatorPool(ncas, nelecas, "gsd")
    pairs, tabs, first, sign = pool.device_tables(eng)
    nt = int(pqc.theta_shape)
    rng = np.random.default_rng(5)
    _, c1, c2 = oo.get_active_integrals(oo.mo_coeff)
    i32 = torch.int32

    # the replaced route: circuits with one operator appended, built beforehand
    which = [int(k) for k in np.linspace(0, len(pool) - 1, a.sample)]
    theta1 = torch.as_tensor(0.3 * rng.standard_normal(nt), device=dev)
    ext = torch.cat((theta1, torch.zeros(1, dtype=F64, device=dev)))
    circuits = [aoo.Parameterized_circuit(ncas, nelecas, None, ansatz=list(pqc._gates) + pool.operator_gates(k, nt))
                for k in which]
    ref, per_eval = [], []
    for rep in range(2):                                             # (the first pass makes plans and pair lists)
        for c in circuits:
            adapt.swap_circuit(oo, c)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g = oo.circuit_gradient(ext)
            torch.cuda.synchronize()
            if rep:
                per_eval.append(1e6 * (time.perf_counter() - t0))
                ref.append(float(g[-1]))
    adapt.swap_circuit(oo, pqc)
    mine = oo.pool_gradients(theta1, pool)[which].cpu().numpy()
    diff = float(np.abs(mine - np.array(ref)).max())

    for B in a.batches:
        thetas = torch.as_tensor(0.3 * rng.standard_normal((B, nt)), device=dev)
        psi = eng.state(thetas)
        c12 = torch.cat((c1.reshape(-1), c2.reshape(-1)))[None].repeat(B, 1).contiguous()
        work = torch.empty(int(lib.oovqe_pool_gradients_from_coefficients_work_size(ncas, eng.na, eng.nb, B)),
                           dtype=F64, device=dev)
        out = torch.empty((B, len(pool)), dtype=F64, device=dev)
        lam = eng.lam_geometries(psi, 1, c12, c12.stride(0)) if eng.geometry_coefficients_ok() else eng.lam(psi, c1, c2)

        def kernel():
            check(lib.oovqe_pool_gradients_batch(dptr(psi), dptr(lam), eng.na, eng.nb, B, dptr(pairs, i32),
                                                 pool.n_gates, dptr(first, i32), dptr(sign, i32), len(pool), dptr(out),
                                                 stream_ptr()), "oovqe_pool_gradients_batch")

        def call():
            check(lib.oovqe_pool_gradients_from_coefficients_batch(
                dptr(psi), ncas, *eng._tabs(), B, dptr(c12), ctypes.c_void_p(c12.data_ptr() + 8 * ncas * ncas),
                int(c12.stride(0)), tabs, dptr(pairs, i32), pool.n_gates, dptr(first, i32), dptr(sign, i32),
                len(pool), dptr(work), dptr(out), stream_ptr()), "oovqe_pool_gradients_from_coefficients_batch")

        n_pairs = int(pairs[:pool.n_gates].sum().item())
        res = dict(cas="(8e,8o)", pool="gsd", operators=len(pool), states=B, determinants=eng.Dc,
                   pairs_per_state=n_pairs, kernel=event_times(kernel, a.reps, a.warmup),
                   call=event_times(call, a.reps, a.warmup),
                   replaced_per_evaluation_us=dict(mean=float(np.mean(per_eval)), min=float(min(per_eval)),
                                                   max=float(max(per_eval)), sampled=len(per_eval)),
                   replaced_extrapolated_ms=float(np.mean(per_eval)) * (len(pool) + 1) * B / 1e3,
                   max_abs_diff_to_replaced_route=diff)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
