"""Probe: timing of the device integral engine (auto_oo_amd/gto.py) on rings of formaldimine geometries in STO-3G.

For G in {1, 8, 64, 256} points of the Berry-phase notebook's loop: ``gto.integrals_batch`` (integral kernels +
S^-1/2) and ``OO_pqc_batch.set_geometries`` (the same written into the batch, then the ingest pass and the orbital
refresh), each timed with HIP events after warm-up calls (median of the timed calls); next to them the parent's route
for the same ring -- host ``Moldata_sto3g`` per geometry + ``set_molecule`` -- timed with a host clock around a
device synchronise (``--host-geoms`` geometries are built, the rest extrapolated: 0.7 s each).  ``--profile G`` runs
only warm ``set_geometries`` calls of that size (for a kernel trace).  Prints one JSON line per shape.  Not part of
bench.py.

``--basis water-pd``: water in STO-3G plus a d shell on O and a p shell on each H (18 spherical functions);
``--basis polarised-43``: formaldimine with a table of cc-pVDZ's shape -- 3s2p1d on C and N, 2s1p on H, 43 spherical
functions, two 8-primitive s shells per heavy atom; the exponents are even-tempered stand-ins, not a published basis.
For these two the stack is the equilibrium geometry with small random displacements, the starting orbitals are the
device RHF orbitals of the stack, and the host route is not timed (the host code takes seconds to minutes per
geometry with d shells).  ``--sizes`` chooses the stack sizes.

``--moments``: instead of the above, one line per stack size of the STO-3G ring with the medians of the dipole and
second-moment integrals (``gto.moment_integrals_batch``, order 2), of ``OO_pqc_batch.dipole_moment`` (circuit RDMs, AO
density, order-1 integrals, contraction) and ``rhf_dipole_moment`` from a given RHF result, next to the integral build
``oovqe_gto_integrals_batch`` of the same stack (``gto.integrals_into``, without S^-1/2), the yardstick."""
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


WATER = np.array([[0.0, 0.01, 0.02], [0.3, 0.75, 0.55], [-0.2, -0.70, 0.62]])


def _even_tempered(first, ratio, n):
    return [first / ratio ** k for k in range(n)]


def polarised_basis(name):
    """-> (GTOBasis, equilibrium coordinates [natm, 3] in Angstrom, CAS (ncas, nelecas))"""
    par = aoo.gaussian._STO3G
    g = aoo.gaussian
    if name == "water-pd":
        table = {"O": [("s", par["O"]["1s"], g._STO3G_1S_COEF), ("s", par["O"]["2sp"], g._STO3G_2S_COEF),
                       ("p", par["O"]["2sp"], g._STO3G_2P_COEF), ("d", [0.8], [1.0])],
                 "H": [("s", par["H"]["1s"], g._STO3G_1S_COEF), ("p", [1.1], [1.0])]}
        return gto.GTOBasis(["O", "H", "H"], table, d_functions="spherical"), WATER, (2, 2)
    table = {}
    for sym, z in (("C", 1.0), ("N", 1.35)):
        s8 = _even_tempered(6000.0 * z, 3.4, 8)
        table[sym] = [("s", s8, [0.001, 0.006, 0.03, 0.1, 0.25, 0.4, 0.3, 0.05]),
                      ("s", s8, [-0.0002, -0.0013, -0.007, -0.025, -0.07, -0.16, 0.1, 0.6]),
                      ("s", [0.16 * z], [1.0]),
                      ("p", _even_tempered(9.4 * z, 4.3, 3), [0.04, 0.21, 0.51]), ("p", [0.15 * z], [1.0]),
                      ("d", [0.55 * z], [1.0])]
    table["H"] = [("s", [13.0, 1.96, 0.44], [0.02, 0.14, 0.48]), ("s", [0.122], [1.0]), ("p", [0.73], [1.0])]
    basis = gto.GTOBasis(["N", "C", "H", "H", "H"], table, d_functions="spherical")
    return basis, basis.coordinates([get_formal_geo(130.0, 89.9)])[0], (3, 4)


def time_polarised(args):
    basis, xyz0, (ncas, nelecas) = polarised_basis(args.basis)
    pqc = aoo.Parameterized_circuit(ncas, nelecas, None, ansatz="np_fabric", n_layers=1)
    rng = np.random.default_rng(0)
    for G in ((args.profile,) if args.profile else args.sizes):
        xyz = torch.as_tensor(xyz0[None] + 0.02 * rng.standard_normal((G,) + xyz0.shape)).cuda()
        xyz[0] = torch.as_tensor(xyz0)
        batch = aoo.OO_pqc_batch.from_geometries(pqc, basis, xyz, ncas, nelecas, oao_mo_coeffs="rhf",
                                                 freeze_active=True)
        if args.profile:
            for _ in range(args.warm + args.reps):
                batch.set_geometries(xyz)
            torch.cuda.synchronize()
            continue
        t_int = event_time(lambda: gto.integrals_batch(basis, xyz, check_overlap=False), args.reps, args.warm)
        t_set = event_time(lambda: batch.set_geometries(xyz), args.reps, args.warm)
        print(json.dumps({"basis": args.basis, "nao": basis.nao, "G": G, "eri_flags": int(batch.eri_flags),
                          "integrals_batch_us": t_int[0], "integrals_batch_min_us": t_int[1],
                          "set_geometries_us": t_set[0], "set_geometries_min_us": t_set[1],
                          "set_geometries_us_per_geometry": t_set[0] / G}), flush=True)


def time_moments(args):
    basis = gto.GTOBasis(["N", "C", "H", "H", "H"])
    pqc = aoo.Parameterized_circuit(2, 2, None, ansatz="np_fabric", n_layers=1)
    for G in args.sizes:
        xyz = torch.as_tensor(basis.coordinates(ring(G))).cuda()
        batch = aoo.OO_pqc_batch.from_geometries(pqc, basis, xyz, 2, 2, oao_mo_coeffs="rhf")
        N = basis.nao
        S, h = torch.empty((G, N, N), dtype=torch.float64).cuda(), torch.empty((G, N, N), dtype=torch.float64).cuda()
        g, nuc = torch.empty((G, N, N, N, N), dtype=torch.float64).cuda(), torch.empty(G, dtype=torch.float64).cuda()
        thetas = torch.zeros((G, batch.n_theta), dtype=torch.float64).cuda()
        rhf = batch.rhf()
        t_int = event_time(lambda: gto.integrals_into(basis, batch.coords_bohr, S, h, g, nuc), args.reps, args.warm)
        t_mom = event_time(lambda: gto.moment_integrals_batch(basis, xyz, order=2), args.reps, args.warm)
        t_one = event_time(lambda: gto.moment_integrals_batch(basis, xyz, order=1), args.reps, args.warm)
        t_dip = event_time(lambda: batch.dipole_moment(thetas), args.reps, args.warm)
        t_rhf = event_time(lambda: batch.rhf_dipole_moment(rhf), args.reps, args.warm)
        print(json.dumps({"moments": True, "G": G, "nao": N, "gto_integrals_batch_us": t_int[0],
                          "gto_integrals_batch_min_us": t_int[1], "moment_integrals_order2_us": t_mom[0],
                          "moment_integrals_order2_min_us": t_mom[1], "moment_integrals_order1_us": t_one[0],
                          "dipole_moment_us": t_dip[0], "dipole_moment_min_us": t_dip[1],
                          "rhf_dipole_moment_us": t_rhf[0]}), flush=True)


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
    ap.add_argument("--basis", choices=("sto-3g", "water-pd", "polarised-43"), default="sto-3g")
    ap.add_argument("--sizes", type=int, nargs="+", default=None, metavar="G")
    ap.add_argument("--moments", action="store_true", help="time the moment integrals and dipole moments instead")
    args = ap.parse_args()
    if args.moments:
        args.sizes = args.sizes or [64]
        return time_moments(args)
    if args.basis != "sto-3g":
        args.sizes = args.sizes or [1, 64, 256]
        return time_polarised(args)
    args.sizes = args.sizes or [1, 8, 64, 256]
    basis = gto.GTOBasis(["N", "C", "H", "H", "H"])
    pqc = aoo.Parameterized_circuit(2, 2, None, ansatz="np_fabric", n_layers=1)
    mol0 = aoo.Moldata_sto3g(ring(1)[0])
    mol0.run_rhf()
    c0 = aoo.mo_ao_to_mo_oao(mol0.hf.mo_coeff, mol0.overlap)
    for G in ((args.profile,) if args.profile else args.sizes):
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
