"""Probe: timing of the point-charge embedding kernels (csrc/gto_charges.hip) on a ring of formaldimine geometries in
STO-3G, each in its own cloud of M point charges (default G = 64, M = 4096).

``gto.point_charge_integrals_into`` (the operator) and ``gto.point_charge_gradient_into`` (gA and gQ for a symmetric
density) are timed on device tensors: warm-up calls first, then ``--windows`` windows of ``--calls`` calls between two
HIP events each; the figure is the median over the windows of the time per call.  A call is what a user's call is: the
finiteness check of its arguments, the read-back of the shell table, the pair data of the stack and the kernels.

Next to the time: (charge, primitive pair) evaluations per second -- each is one Boys function and one table of
Hermite Coulomb integrals -- and the fp64 operations these evaluations issue, counted from the shell classes by
``flops_per_evaluation`` below (an exponential counted as 20, a square root or an error function as 20, the 36-term
series of the Boys function in full although half of the evaluations take the short branch), over the fp64 vector
peak of the device (78.6 TFLOP/s): a whole-call rate over peak, not a kernel's share of it.

Before anything is timed the results at the timed size are checked against calls on the two halves of every cloud:
the operator is the sum of the halves' operators (1e-12 of its largest element), gQ of a half has the bits of the
whole call's (a charge's derivative is made by one lane from that charge alone; M / 2 a multiple of 64), gA is the
sum of the halves' (1e-12).  Prints one JSON line.  Not part of bench.py."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import auto_oo_amd as aoo                                   # noqa: E402
from auto_oo_amd import gto                                 # noqa: E402
from auto_oo_amd.moldata import get_formal_geo              # noqa: E402

FP64_PEAK = 78.6e12
F64 = torch.float64


def ring(n):
    ph = np.pi / 20
    return [get_formal_geo(130 + 10 * np.cos(2 * np.pi * k / n + ph), 89.9 + 10 * np.sin(2 * np.pi * k / n + ph))
            for k in range(n)]


def cloud(G, M, seed=1):
    """q [G, M] in [-1, 1] and positions [G, M, 3] in Bohr, 4 .. 20 Bohr from the origin of the coordinates"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(G, M, 3))
    u /= np.linalg.norm(u, axis=2)[..., None]
    return rng.uniform(-1.0, 1.0, (G, M)), u * rng.uniform(4.0, 20.0, (G, M))[..., None]


def comps(l):
    return {0: [(0, 0, 0)], 1: [(1, 0, 0), (0, 1, 0), (0, 0, 1)]}[l]


def flops_per_evaluation(la, lb, gradient):
    """fp64 operations one (charge, primitive pair) evaluation issues in class (la, lb): Boys function of order L,
    its scaling, the R_tuv recursion (one multiply-add per node), and what meets R per charge -- for the operator
    only the sum into the lane's table, for the gradient the Hermite coefficients of the pair (rebuilt per charge)
    and the six sums over (t, u, v) per component pair."""
    L = la + lb + (1 if gradient else 0)
    boys = 20 + 3 * 36 + 4 + 3 * L
    scale = 2 * (L + 1)
    nodes = sum(1 for t in range(L + 1) for u in range(L + 1 - t) for v in range(L + 1 - t - u)
                for n in range(L + 1 - t - u - v) if t + u + v > 0)
    table = (L + 1) * (L + 2) * (L + 3) // 6
    if not gradient:
        return boys + scale + 2 * nodes + table
    herm = 3 * 6 * (la + 2) * (lb + 1) * (la + lb + 2) + 3 * 3 * (la + 1) * (lb + 1) * (la + lb + 2)
    sums = 0
    for a in comps(la):
        for b in comps(lb):
            n = [a[d] + b[d] for d in range(3)]
            plain = 2 * (n[0] + 1) * (n[1] + 1) * (n[2] + 1)
            sums += 3 * plain + 2 * 3                     # d/dP: the same sum on a shifted table
            for d in range(3):
                m = list(n)
                m[d] += 1
                sums += 2 * (m[0] + 1) * (m[1] + 1) * (m[2] + 1) + 2
    return boys + scale + 2 * nodes + herm + sums


def evaluations(basis):
    """-> {(la, lb): primitive pairs of the shell pairs of that class}"""
    out = {}
    ls, np_ = basis.shells[:, 1] & 255, basis.shells[:, 2]
    for i in range(basis.nshell):
        for j in range(i + 1):
            key = (int(max(ls[i], ls[j])), int(min(ls[i], ls[j])))
            out[key] = out.get(key, 0) + int(np_[i]) * int(np_[j])
    return out


def timed(f, calls, windows, warmup):
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            f()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometries", type=int, default=64)
    ap.add_argument("--charges", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    device = aoo._lib.require_device()
    G, M = args.geometries, args.charges
    basis = gto.GTOBasis(["N", "C", "H", "H", "H"])
    xyz = gto.coords_to_device(basis, ring(G), device)
    q, r = cloud(G, M)
    q, r = torch.as_tensor(q).to(device), torch.as_tensor(r).to(device)
    rng = np.random.default_rng(2)
    d1 = rng.uniform(-1, 1, (G, basis.nao, basis.nao))
    d1 = torch.as_tensor(0.5 * (d1 + d1.transpose(0, 2, 1))).to(device)
    out = torch.empty((G, basis.nao, basis.nao), dtype=F64, device=device)
    # the results at this size against the two halves of every cloud
    h = M // 2
    whole = gto.point_charge_integrals_into(basis, xyz, q, r)
    parts = (gto.point_charge_integrals_into(basis, xyz, q[:, :h].contiguous(), r[:, :h].contiguous())
             + gto.point_charge_integrals_into(basis, xyz, q[:, h:].contiguous(), r[:, h:].contiguous()))
    op_err = ((whole - parts).abs().max() / whole.abs().max()).item()
    gA, gQ = gto.point_charge_gradient_into(basis, xyz, q, r, d1, True)
    a0, q0 = gto.point_charge_gradient_into(basis, xyz, q[:, :h].contiguous(), r[:, :h].contiguous(), d1, True)
    a1, q1 = gto.point_charge_gradient_into(basis, xyz, q[:, h:].contiguous(), r[:, h:].contiguous(), d1, True)
    ga_err = ((gA - (a0 + a1)).abs().max() / gA.abs().max()).item()
    gq_same = bool(torch.equal(gQ, torch.cat((q0, q1), dim=1))) if h % 64 == 0 else None
    if not (op_err < 1e-12 and ga_err < 1e-12 and gq_same in (True, None)):
        raise SystemExit(f"results at the timed size disagree with their halves: operator {op_err:.2e}, gA {ga_err:.2e}, "
                         f"gQ same bits: {gq_same}")
    ev = evaluations(basis)
    line = {"tool": "bench_point_charges", "geometries": G, "charges": M, "nao": basis.nao,
            "primitive_pairs": sum(ev.values()), "calls": args.calls, "windows": args.windows,
            "fp64_peak_tflops": FP64_PEAK / 1e12,
            "check_against_halves": {"operator_rel": op_err, "gA_rel": ga_err, "gQ_same_bits": gq_same}}
    for name, gradient, f in (
            ("operator", False, lambda: gto.point_charge_integrals_into(basis, xyz, q, r, out)),
            ("gradient", True, lambda: gto.point_charge_gradient_into(basis, xyz, q, r, d1, True))):
        med, lo, hi = timed(f, args.calls, args.windows, args.warmup)
        n_eval = G * M * sum(ev.values())
        flops = G * M * sum(n * flops_per_evaluation(la, lb, gradient) for (la, lb), n in ev.items())
        line[name] = {"ms_per_stack": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                      "evaluations_per_s": n_eval / (med * 1e-3), "counted_gflop": flops / 1e9,
                      "counted_tflops": flops / (med * 1e-3) / 1e12,
                      "ratio_to_fp64_vector_peak": flops / (med * 1e-3) / FP64_PEAK}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
