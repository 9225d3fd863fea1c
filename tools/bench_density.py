"""Probe: timing of ``gto.density_into`` (csrc/gto_density.hip), the electron density and its gradient of a stack of
geometries at M points per geometry for K densities per geometry, in points per second (geometries x points / time).

Molecules: formaldimine in STO-3G on the ring of tools/gto_bench.py (13 functions) and in the 43-function polarised table
of tools/gto_bench.py (``polarised-43``; the equilibrium geometry with small seeded displacements).  The points lie up to
6 Bohr from the origin (inside the molecule's density), the densities are random and symmetric.  Default size: 64
geometries x 65535 points, K = 1 and 5, with and without the gradient.

A call is what a user's call is: the finiteness check of its arguments, the read-back of the shell table and the kernel.
Per size: warm-up calls, one timed call to choose how many calls fill ``--window`` seconds, then ``--windows`` windows
between two HIP events each; the figure is the median over the windows of the time per call.  Beside each figure
``torch_ms``: a plain-torch realisation of the same formula on the same device in the same run, which builds chi
[G, M, N] (and d chi [G, M, N, 3]) with torch operations and takes an ``einsum`` -- the only yardstick there is, the
library had no density before.  Before a size is timed, the two are compared (largest difference relative to the largest
value), and the first geometry with its first 64 points alone must have the bits it has in the whole call.

``--resources``: instead of timing, compile csrc/gto_density.hip for gfx950 with the compiler's resource report and print
it per kernel (registers, scratch, LDS, occupancy); needs no device.  Prints one JSON line per size.  Not part of
bench.py."""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "auto_oo_amd", "csrc", "gto_density.hip")
    out = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
                          os.devnull], capture_output=True, text=True, check=True).stderr
    line = None
    for text in out.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\S+)", text)
        if not m:
            continue
        if m.group(1) == "Function Name":
            if line:
                print(json.dumps(line), flush=True)
            line = {"tool": "bench_density", "kernel": m.group(2)}
        elif line is not None:
            line[m.group(1)] = int(m.group(2))
    if line:
        print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", nargs="+", default=["formaldimine-sto3g", "polarised-43"])
    ap.add_argument("--geometries", type=int, nargs="+", default=[64])
    ap.add_argument("--points", type=int, nargs="+", default=[65535])
    ap.add_argument("--sets", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed window")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--resources", action="store_true")
    args = ap.parse_args()
    if args.resources:
        return resources()

    import auto_oo_amd as aoo
    from auto_oo_amd import gaussian, gto
    import gto_bench
    from bench_potential import timed
    BOHR = gaussian.BOHR
    device = aoo._lib.require_device()

    def problem(name, G, M, K, seed=1):
        rng = np.random.default_rng(seed)
        if name == "formaldimine-sto3g":
            basis = gto.GTOBasis(["N", "C", "H", "H", "H"])
            xyz = basis.coordinates(gto_bench.ring(G))
        else:
            basis, xyz0, _ = gto_bench.polarised_basis(name)
            xyz = xyz0[None] + rng.uniform(-0.02, 0.02, (G,) + xyz0.shape)
        u = rng.normal(size=(G, M, 3))
        u /= np.linalg.norm(u, axis=2)[..., None]
        pts = u * rng.uniform(0.0, 6.0, (G, M))[..., None]
        dm = rng.uniform(-1.0, 1.0, (G, K, basis.nao, basis.nao))
        dm = 0.5 * (dm + dm.transpose(0, 1, 3, 2))
        t = lambda a: torch.as_tensor(a).to(device)         # noqa: E731
        return basis, t(xyz / BOHR), t(pts), t(dm)

    def torch_density(basis, xyz, pts, dm, gradient):
        """the same formula with torch operations: chi [G, M, ncart] shell by shell, the d form as a matrix, einsum"""
        T = torch.as_tensor(gaussian.basis_transform(basis.table, basis.d_functions or "spherical")).to(device)
        cols, dcols = [], []
        for atom, l, ex, co in basis.table:
            d = pts - xyz[:, atom, None, :]                                                   # [G, M, 3]
            r2 = (d * d).sum(-1)
            for lmn in gaussian._CARTESIAN[int(l)]:
                sh = gaussian.normalised_shell(np.zeros(3), lmn, ex, co)
                a, c = torch.as_tensor(sh.exps).to(device), torch.as_tensor(sh.coefs).to(device)
                e = torch.exp(-a * r2[..., None])
                r0 = (c * e).sum(-1)
                poly = d[..., 0] ** lmn[0] * d[..., 1] ** lmn[1] * d[..., 2] ** lmn[2]
                cols.append(poly * r0)
                if gradient:
                    r1 = (-2.0 * a * c * e).sum(-1)
                    g = []
                    for k in range(3):
                        t = d[..., k] * poly * r1
                        if lmn[k]:
                            low = list(lmn)
                            low[k] -= 1
                            t = t + lmn[k] * d[..., 0] ** low[0] * d[..., 1] ** low[1] * d[..., 2] ** low[2] * r0
                        g.append(t)
                    dcols.append(torch.stack(g, dim=-1))
        chi = torch.stack(cols, dim=-1) @ T.T                                                  # [G, M, N]
        sym = dm + dm.transpose(2, 3)
        half = torch.einsum("gkpq,gmq->gkmp", sym, chi)
        rho = 0.5 * torch.einsum("gkmp,gmp->gkm", half, chi)
        if not gradient:
            return rho
        dchi = torch.einsum("gmcx,pc->gmpx", torch.stack(dcols, dim=-2), T)
        return rho, torch.einsum("gkmp,gmpx->gkmx", half, dchi)

    for name in args.molecules:
        for G in args.geometries:
            for M in args.points:
                for K in args.sets:
                    basis, xyz, pts, dm = problem(name, G, M, K)
                    line = {"tool": "bench_density", "molecule": name, "nao": basis.nao, "nshell": basis.nshell,
                            "geometries": G, "points": M, "sets": K}
                    for grad in (False, True):
                        tag = "gradient" if grad else "density"
                        out = gto.density_into(basis, xyz, pts, dm, grad)
                        ref = torch_density(basis, xyz, pts, dm, grad)
                        m = min(64, M)
                        alone = gto.density_into(basis, xyz[:1], pts[:1, :m].contiguous(), dm[:1], False)
                        if not torch.equal(alone[0], (out[0] if grad else out)[0, :, :m]):
                            raise SystemExit("a geometry and its first points alone do not have the bits of the whole call")
                        pairs = list(zip(out, ref)) if grad else [(out, ref)]
                        line[tag + "_vs_torch"] = max(((a - b).abs().max() / b.abs().max()).item() for a, b in pairs)
                        del out, ref, pairs
                        med, lo, hi, calls = timed(lambda: gto.density_into(basis, xyz, pts, dm, grad), args.window,
                                                   args.windows, args.warmup)
                        line[tag + "_ms"] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4),
                                             "calls": calls}
                        line[tag + "_points_per_s"] = round(G * M / (med * 1e-3), 1)
                        tmed, tlo, thi, tcalls = timed(lambda: torch_density(basis, xyz, pts, dm, grad), args.window,
                                                       args.windows, 1)
                        line[tag + "_torch_ms"] = {"median": round(tmed, 4), "min": round(tlo, 4), "max": round(thi, 4),
                                                   "calls": tcalls}
                        line[tag + "_torch_over_kernel"] = round(tmed / med, 2)
                    print(json.dumps(line), flush=True)
                    del xyz, pts, dm


if __name__ == "__main__":
    main()
