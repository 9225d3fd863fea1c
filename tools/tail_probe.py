"""Phase table of cas_tail_kernel at the bench shape (N = 43, 6 core + 3 active, UCCD, 256 geometries).

Needs a probe build of the library (never the default one):

    tools/build_variant.sh tailprobe "-DOOVQE_TAIL_PROBE" cas.hip
    OOVQE_LIB_PATH=auto_oo_amd/lib/liboovqe_hip_tailprobe.so python tools/tail_probe.py [OUT.txt] [N] [G]

In that build every workgroup of the tail meets at a barrier at each phase boundary and thread 0 stores the
100 MHz wall clock there (csrc/cas.hip, TAIL_MARK).  The barriers serialise what the production kernel overlaps,
so the phases add up to somewhat more than the production kernel takes; the table orders the phases, it does not
time the kernel.  Prints, per phase, mean / min / max over the workgroups in microseconds."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

NCAS, NELECAS, NELEC = 3, 4, 16
WGS, MARKS = 512, 32
PHASES = [(0, 1, "input + first J loads issued, table"), (1, 2, "inputs: registers to LDS"), (2, 3, "h_mo"),
          (3, 4, "q->x, all tiles of (y <= z)"), (4, 5, "p->n over the packed columns"),
          (5, 6, "FI"), (6, 7, "gathers (Ga, Dc)"), (7, 8, "Cpart, c1, c2"), (8, 9, "Fock columns"),
          (9, 10, "energy parts"), (10, 11, "assembly"), (0, 11, "whole workgroup")]
LAST = PHASES[-1][1]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 43
    G = int(sys.argv[3]) if len(sys.argv) > 3 else 256
    import auto_oo_amd as aoo
    from auto_oo_amd import _lib
    from auto_oo_amd.synthetic import synthetic_problem
    lib = _lib.load()
    if not hasattr(lib, "oovqe_tail_probe_read"):
        raise SystemExit("not a probe build: build with -DOOVQE_TAIL_PROBE and select it with OOVQE_LIB_PATH")
    lib.oovqe_tail_probe_read.restype = ctypes.c_int
    lib.oovqe_tail_probe_read.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]
    pqc = aoo.Parameterized_circuit(NCAS, NELECAS, None, ansatz="ucc")
    base = [synthetic_problem(N, 20262 + 1000 * g) for g in range(4)]
    mols = [aoo.Moldata(base[g % 4]["int1e_ao"], base[g % 4]["int2e_ao"], base[g % 4]["overlap"],
                        base[g % 4]["nuc"] + 0.001 * g, NELEC) for g in range(G)]
    batch = aoo.OO_pqc_batch(pqc, mols, NCAS, NELECAS, oao_mo_coeffs=[base[g % 4]["oao_mo_coeff"] for g in range(G)])
    thetas = torch.tensor(np.random.default_rng(7).uniform(0, 2 * np.pi, (G, pqc.theta_shape)), device="cuda")
    for _ in range(5):
        batch.energy_and_gradient(thetas)
    torch.cuda.synchronize()
    buf = (ctypes.c_longlong * (WGS * MARKS))()
    if lib.oovqe_tail_probe_read(buf, WGS * MARKS):
        raise SystemExit("oovqe_tail_probe_read failed")
    t = np.frombuffer(buf, dtype=np.int64).reshape(WGS, MARKS)[:min(G, WGS)].astype(np.float64) * 0.01   # us
    lines = [f"cas_tail_kernel phase table, N={N}, {G} geometries, lib={os.path.basename(_lib.LIB_PATH)}",
             f"{'phase':40s} {'mean us':>8s} {'min':>7s} {'max':>7s}"]
    for a, b, name in PHASES:
        d = t[:, b] - t[:, a]
        lines.append(f"{name:40s} {d.mean():8.2f} {d.min():7.2f} {d.max():7.2f}")
    lines.append(f"first start to last end over the grid: {t[:, LAST].max() - t[:, 0].min():.2f} us")
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
