"""Probe: timing of the analytic nuclear gradient of a geometry stack against the finite-difference route it replaces.

Stack: G = 64 points of the formaldimine ring (STO-3G, N = 13, 5 atoms), CAS(4e,3o) with the ``ucc`` circuit, RHF
orbitals of every point from the device solver, seeded circuit parameters.  After warm-up, the median wall time of
``reps`` calls (stream synchronised) of

  * ``OO_pqc_batch.nuclear_gradient`` (RDMs, generalised Fock matrix, AO densities, overlap pull-back, contraction),
  * its parts: the contraction ``gto.gradient_into`` alone on ready densities, and the integral build
    ``gto.integrals_into`` of the same stack as the yardstick ("one integral build"),
  * the same forces by two-point central differences: for each of the 3 * natm coordinates the whole stack displaced by
    +h and by -h, ``set_geometries`` + ``energy_and_gradient`` (2 * 3 * natm = 30 integral builds, ingests and
    evaluations), as a user had to do it before.

One JSON line.  Not part of bench.py.

  python tools/nuclear_gradient_bench.py [--geometries 64] [--reps 5] [--warmup 2] [--fd-reps 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import auto_oo_amd as aoo                                           # noqa: E402
from auto_oo_amd import gto, nucgrad, ops                           # noqa: E402
from auto_oo_amd.gaussian import BOHR                               # noqa: E402
from auto_oo_amd.moldata import get_formal_geo                      # noqa: E402

F64 = torch.float64


def ring(G):
    return [get_formal_geo(130.0 + 10.0 * np.cos(2 * np.pi * k / G + np.pi / 20),
                           89.9 + 10.0 * np.sin(2 * np.pi * k / G + np.pi / 20)) for k in range(G)]


def median_ms(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(times)), out


def finite_difference_forces(batch, thetas, xyz_bohr, h):
    """two-point central differences over set_geometries + energy_and_gradient; the batch ends where it started"""
    G, natm = xyz_bohr.shape[:2]
    U = batch.oao_mo_coeff.clone()
    keep = [U[g] for g in range(G)]
    out = torch.empty((G, natm, 3), dtype=F64, device=batch.device)
    for a in range(natm):
        for d in range(3):
            e = []
            for s in (1.0, -1.0):
                x = xyz_bohr.clone()
                x[:, a, d] += s * h
                batch.set_geometries(x * BOHR, oao_mo_coeffs=None)
                e.append(batch.energy_and_gradient(thetas)[:, 0].clone())
            out[:, a, d] = (e[0] - e[1]) / (2.0 * h)
    batch.set_geometries(xyz_bohr * BOHR, oao_mo_coeffs=keep)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--geometries", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fd-reps", type=int, default=2)
    ap.add_argument("--step", type=float, default=1e-3, help="finite-difference step in Bohr")
    a = ap.parse_args()
    G = a.geometries
    basis = gto.GTOBasis(["N", "C", "H", "H", "H"])
    pqc = aoo.Parameterized_circuit(3, 4, None, ansatz="ucc")
    batch = aoo.OO_pqc_batch.from_geometries(pqc, basis, ring(G), 3, 4, oao_mo_coeffs="rhf")
    thetas = torch.as_tensor(np.random.default_rng(5).uniform(-0.6, 0.6, (G, batch.n_theta))).to(batch.device)
    xyz = batch.coords_bohr.clone()

    t_grad, grad = median_ms(lambda: batch.nuclear_gradient(thetas), a.reps, a.warmup)

    # the parts: ready densities -> contraction alone; the integral build of the same stack
    gamma, Gamma = ops.circuit_rdms(thetas, pqc._gates_dev, pqc._n_gates, pqc.n_qubits, 3, pqc._init_index,
                                    tangents=False)
    _, _, fock = batch._cas_batch(gamma, Gamma, G, want_fock=True)
    t_dens, (d1, d2) = median_ms(lambda: nucgrad.cas_ao_densities(batch.mo_coeff, batch._n_occ, 3, gamma[:, 0],
                                                                  Gamma[:, 0]), a.reps, a.warmup)
    t_wq, wq = median_ms(lambda: nucgrad.overlap_pullback(batch.overlap, batch.oao_mo_coeff, fock), a.reps, a.warmup)
    t_con, _ = median_ms(lambda: gto.gradient_into(basis, xyz, d1, wq, d2, True), a.reps, a.warmup)
    N = basis.nao
    S = torch.empty((G, N, N), dtype=F64, device=batch.device)
    hh = torch.empty_like(S)
    gg = torch.empty((G,) + (N,) * 4, dtype=F64, device=batch.device)
    nuc = torch.empty(G, dtype=F64, device=batch.device)
    t_int, _ = median_ms(lambda: gto.integrals_into(basis, xyz, S, hh, gg, nuc), a.reps, a.warmup)

    t_fd, fd = median_ms(lambda: finite_difference_forces(batch, thetas, xyz, a.step), a.fd_reps, 1)
    print(json.dumps({
        "G": G, "N": N, "natm": basis.natm, "circuit": "ucc CAS(4e,3o)",
        "nuclear_gradient_ms": t_grad, "contraction_ms": t_con, "ao_densities_ms": t_dens,
        "overlap_pullback_ms": t_wq, "integral_build_ms": t_int,
        "contraction_over_integral_build": t_con / t_int,
        "finite_difference_ms": t_fd, "finite_difference_builds": 2 * 3 * basis.natm,
        "finite_difference_over_analytic": t_fd / t_grad,
        "max_abs_difference_of_the_two": float((fd - grad).abs().max().item()),
        "max_abs_force": float(grad.abs().max().item())}), flush=True)


if __name__ == "__main__":
    main()
