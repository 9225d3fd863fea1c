"""Writes tests/golden/gto_edges_<case>.npz, the recorded host-twin results of the edge tests of the Gaussian-integral
kernels (cases and readers: tests/_gto_edges.py).

    python tests/golden/make_gto_edges.py            # every case
    python tests/golden/make_gto_edges.py Lss G2     # some

Per case: S, h, the unique (pq|rs) packed (p >= q, r >= s, pq >= rs), nuc from ``gaussian.integrals_from_table``; mom
from ``moment_integrals_from_table`` (order 2, origin ``_gto_edges.origin_of``); cross from
``cross_overlap_from_table`` against the displaced copy; diff_h, diff_g: the largest elementwise change when every Boys
order n is multiplied by 1 + ``_gto_d.BOYS_RTOL[n]`` * (+-1 at random, seed 1).  G4 also holds its largest differences
from G1 (g4_S, g4_h, g4_g, g4_mom, g4_cross).  The files are reproduced bit for bit by a second run.

Run time (one core, both builds of a case): Lss, Lps, Lpp below 1 s, Lds 6 s, Ldp 6 s, Ldd 42 s, L3 43 s, G1 .. G5 12
to 17 s each; 3 minutes in all."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from auto_oo_amd import gaussian          # noqa: E402
from tests import _gto_edges as E         # noqa: E402


def host(name, boys=None):
    basis = E.basis_of(name)
    return gaussian.integrals_from_table(basis.table, basis.charges, E.xyz_of(name), E.form_of(name), boys)


def one_electron_extras(name):
    basis = E.basis_of(name)
    mom = gaussian.moment_integrals_from_table(basis.table, E.xyz_of(name), E.form_of(name), 2, E.origin_of(name))
    cross = gaussian.cross_overlap_from_table(basis.table, E.xyz_of(name), E.displaced(name), E.form_of(name))
    return mom, cross


def make(name):
    t0 = time.time()
    S, h, g, nuc = host(name)
    _, h2, g2, _ = host(name, E.perturbed_boys(1))
    mom, cross = one_electron_extras(name)
    out = dict(S=S, h=h, g_packed=E.pack_g(g), nuc=np.float64(nuc), mom=mom, cross=cross,
               diff_h=np.abs(h2 - h).max(), diff_g=np.abs(g2 - g).max())
    if name == "G4":
        S1, h1, g1, _ = host("G1")
        mom1, cross1 = one_electron_extras("G1")
        out.update(g4_S=np.abs(S - S1).max(), g4_h=np.abs(h - h1).max(), g4_g=np.abs(g - g1).max(),
                   g4_mom=np.abs(mom - mom1).max(), g4_cross=np.abs(cross - cross1).max())
    np.savez(E.fixture_path(name), **out)
    print(f"{name}: nao {S.shape[0]}, max |h| {np.abs(h).max():.3g}, max |g| {np.abs(g).max():.3g}, "
          f"diff_h {out['diff_h']:.2e}, diff_g {out['diff_g']:.2e}, "
          + (f"G4 - G1: S {out['g4_S']:.2e} h {out['g4_h']:.2e} g {out['g4_g']:.2e} mom {out['g4_mom']:.2e} "
             f"cross {out['g4_cross']:.2e}, " if name == "G4" else "")
          + f"{os.path.getsize(E.fixture_path(name))} bytes, {time.time() - t0:.0f} s", flush=True)


if __name__ == "__main__":
    for case in (sys.argv[1:] or E.FIXTURES):
        make(case)
