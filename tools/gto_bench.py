"""Probe: timing of the device integral engine (auto_oo_amd/gto.py) on rings of formaldimine geometries in STO-3G.

For G in {1, 8, 64, 256} points of the Berry-phase notebook's loop: ``gto.integrals_batch`` (integral kernels +
S^-1/2) and ``OO_pqc_batch.set_geometries`` (the same written into the batch, then the ingest pass and the orbital
refresh), each timed with HIP events after warm-up calls (median of the timed calls); next to them the parent's route
for the same ring -- host ``Moldata_sto3g`` per geometry + ``set_molecule`` -- timed with a host clock around a
device synchronise (``--host-geoms`` geometries are built, the rest extrapolated: 0.7 s each).  ``--profile G`` runs
only warm ``set_geometries`` calls of that size (for a kernel trace).  Prints one JSON line per shape.  Not part of
bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import auto_oo_amd as aoo                                   # noqa: E402
from auto_oo_amd import gto                                 # noqa: E402
from auto_oo_amd.moldata import get_formal_geo              # noqa: E402


def ring(n):
    ph = np.pi / 20
    return [get_formal_geo(130 + 10 * np.cos(2 * np.pi * k / n + ph), 89.9 + 10 * np.sin(2 * np.pi * k / n + ph))
            for k in range(n)]


def event_time(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e) * 1e3)
    return float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--host-geoms", type=int, default=8, help="geometries actually built on the host per shape")
    ap.add_argument("--profile", type=int, default=0, metavar="G")
    args = ap.parse_args()
    basis = gto.GTOBasis(["N", "C", "H", "H", "H"])
    pqc = aoo.Parameterized_circuit(2, 2, None, ansatz="np_fabric", n_layers=1)
    mol0 = aoo.Moldata_sto3g(ring(1)[0])
    mol0.run_rhf()
    c0 = aoo.mo_ao_to_mo_oao(mol0.hf.mo_coeff, mol0.overlap)
    for G in ((args.profile,) if args.profile else (1, 8, 64, 256)):
        geos = ring(G)
        xyz = torch.as_tensor(basis.coordinates(geos)).cuda()          # Angstrom, on the device
        batch = aoo.OO_pqc_batch.from_geometries(pqc, basis, xyz, 2, 2, oao_mo_coeffs=[c0] * G, freeze_active=True)
        if args.profile:
            for _ in range(args.warm + args.reps):
                batch.set_geometries(xyz)
            torch.cuda.synchronize()
            continue
        t_int = event_time(lambda: gto.integrals_batch(basis, xyz, check_overlap=False), args.reps, args.warm)
        t_set = event_time(lambda: batch.set_geometries(xyz), args.reps, args.warm)
        thetas = torch.zeros((G, batch.n_theta), dtype=torch.float64).cuda()
        t_step = event_time(lambda: batch.damped_newton_step(thetas), max(3, args.reps // 4), 2)
        # the parent's route: host integrals + set_molecule, geometry by geometry
        nh = min(G, args.host_geoms)
        t0 = time.perf_counter()
        mols = [aoo.Moldata_sto3g(g) for g in geos[:nh]]
        t_build = (time.perf_counter() - t0) / nh
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k, m in enumerate(mols):
            batch.set_molecule(k, m, c0)
        torch.cuda.synchronize()
        t_copy = (time.perf_counter() - t0) / nh
        print(json.dumps({
            "G": G, "integrals_batch_us": t_int[0], "integrals_batch_min_us": t_int[1],
            "set_geometries_us": t_set[0], "set_geometries_min_us": t_set[1],
            "set_geometries_us_per_geometry": t_set[0] / G, "lockstep_newton_step_us": t_step[0],
            "set_geometries_over_step": t_set[0] / t_step[0],
            "host_integrals_s_per_geometry": t_build, "set_molecule_us_per_geometry": t_copy * 1e6,
            "host_geometries_built": nh, "parent_route_s": G * (t_build + t_copy),
            "speedup_over_parent_route": G * (t_build + t_copy) / (t_set[0] * 1e-6)}), flush=True)


if __name__ == "__main__":
    main()
