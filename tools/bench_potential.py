"""Probe: timing of ``gto.potential_into`` (csrc/gto_potential.hip), the electrostatic potential and field of a stack of
geometries at M points per geometry for K densities per geometry.

Molecules: water in STO-3G (7 functions), water with a d shell on O and p shells on H (``water-pd`` of tools/gto_bench.py:
M2 of the tests, 18 functions) and formaldimine in the 43-function polarised table of tools/gto_bench.py.  The stack is the
equilibrium geometry with small seeded displacements, the points lie 4 .. 20 Bohr from the origin, the densities are
random and symmetric.  Sizes: ``--geometries`` x ``--points`` x ``--sets``, with and without the field.

A call is what a user's call is: the finiteness check of its arguments, the read-back of the shell table, the pair data
of the stack and the kernel.  Per size: warm-up calls, one timed call to choose how many calls fill ``--window`` seconds,
then ``--windows`` windows between two HIP events each; the figure is the median over the windows of the time per call.
Beside it ``sum_q_phi_ms``: the time of the only thing the library could do before, one
``gto.point_charge_integrals_into`` for charges on the points plus the trace with one density, which yields the single
number sum_m q_m phi_el[m] per geometry (K = 1 rows only).

Before a size is timed its first geometry is checked: the potential of the whole call against a call on that geometry and
the first 64 points alone (the same bits), and sum q phi against tr(D V_ext) of the operator kernel (1e-12 of the absolute
terms).  Prints one JSON line per size.  ``--one``: only run ``--calls`` calls of the one size given, for a kernel trace
(the split over gto_setup_kernel, gto_pair_kernel and gto_potential_kernel comes from rocprofv3 --kernel-trace --stats
around such a run).  Not part of bench.py."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import auto_oo_amd as aoo                                   # noqa: E402
from auto_oo_amd import gto                                 # noqa: E402
from auto_oo_amd.gaussian import BOHR                       # noqa: E402
import gto_bench                                            # noqa: E402

F64 = torch.float64


def molecule(name):
    if name == "water-sto3g":
        return gto.GTOBasis(["O", "H", "H"]), gto_bench.WATER
    basis, xyz, _ = gto_bench.polarised_basis(name)
    return basis, xyz


def problem(name, G, M, K, device, seed=1):
    basis, xyz0 = molecule(name)
    rng = np.random.default_rng(seed)
    xyz = xyz0[None] + rng.uniform(-0.02, 0.02, (G,) + xyz0.shape)
    u = rng.normal(size=(G, M, 3))
    u /= np.linalg.norm(u, axis=2)[..., None]
    pts = u * rng.uniform(4.0, 20.0, (G, M))[..., None]
    dm = rng.uniform(-1.0, 1.0, (G, K, basis.nao, basis.nao))
    dm = 0.5 * (dm + dm.transpose(0, 1, 3, 2))
    q = rng.uniform(-1.0, 1.0, (G, M))
    t = lambda a: torch.as_tensor(a).to(device)             # noqa: E731
    return basis, t(xyz / BOHR), t(pts), t(dm), t(q)


def check(basis, xyz, pts, dm, q, field):
    out = gto.potential_into(basis, xyz, pts, dm, True, field)
    phi = out[0] if field else out
    m = min(64, int(pts.shape[1]))
    alone = gto.potential_into(basis, xyz[:1], pts[:1, :m].contiguous(), dm[:1], True, False)
    if not torch.equal(alone[0], phi[0, :, :m]):
        raise SystemExit("a geometry and its first points alone do not have the bits they have in the whole call")
    el = gto.potential_into(basis, xyz[:1], pts[:1], dm[:1, :1], False, False)[0, 0]
    V = gto.point_charge_integrals_into(basis, xyz[:1], q[:1], pts[:1])[0]
    lhs, rhs = (q[0] * el).sum().item(), (dm[0, 0] * V).sum().item()
    scale = max((q[0] * el).abs().sum().item(), (dm[0, 0] * V).abs().sum().item())
    if not abs(lhs - rhs) < 1e-12 * scale:
        raise SystemExit(f"sum q phi = {lhs!r}, tr(D V_ext) = {rhs!r}")
    return abs(lhs - rhs) / scale


def timed(f, window, windows, warmup):
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    calls = int(min(200, max(1, window * 1e3 / max(a.elapsed_time(b), 1e-3))))
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            f()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    return float(np.median(ms)), float(min(ms)), float(max(ms)), calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", nargs="+", default=["water-sto3g", "water-pd", "polarised-43"])
    ap.add_argument("--geometries", type=int, nargs="+", default=[1, 64, 256])
    ap.add_argument("--points", type=int, nargs="+", default=[64, 4096, 65535])
    ap.add_argument("--sets", type=int, nargs="+", default=[1, 10])
    ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed window")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--one", action="store_true", help="run --calls calls of the first size with --field, untimed")
    ap.add_argument("--field", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    device = aoo._lib.require_device()
    if args.one:
        basis, xyz, pts, dm, q = problem(args.molecules[0], args.geometries[0], args.points[0], args.sets[0], device)
        for _ in range(args.calls):
            gto.potential_into(basis, xyz, pts, dm, True, bool(args.field))
        torch.cuda.synchronize()
        return
    for name in args.molecules:
        for G in args.geometries:
            for M in args.points:
                for K in args.sets:
                    basis, xyz, pts, dm, q = problem(name, G, M, K, device)
                    line = {"tool": "bench_potential", "molecule": name, "nao": basis.nao, "geometries": G, "points": M,
                            "sets": K}
                    for field in (False, True):
                        line["check_rel" if not field else "check_rel_field"] = check(basis, xyz, pts, dm, q, field)
                        med, lo, hi, calls = timed(lambda: gto.potential_into(basis, xyz, pts, dm, True, field),
                                                   args.window, args.windows, args.warmup)
                        line["field_ms" if field else "potential_ms"] = {"median": round(med, 4), "min": round(lo, 4),
                                                                         "max": round(hi, 4), "calls": calls}
                    if K == 1:
                        out = torch.empty((G, basis.nao, basis.nao), dtype=F64, device=device)
                        med, lo, hi, calls = timed(
                            lambda: (dm[:, 0] * gto.point_charge_integrals_into(basis, xyz, q, pts, out)).sum(dim=(1, 2)),
                            args.window, args.windows, args.warmup)
                        line["sum_q_phi_ms"] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4),
                                                "calls": calls}
                    print(json.dumps(line), flush=True)
                    del xyz, pts, dm, q


if __name__ == "__main__":
    main()
