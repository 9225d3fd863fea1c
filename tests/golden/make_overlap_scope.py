"""Writes tests/golden/overlap_scope_<case>.npz, the recorded 40-digit results of the scope tests of the sector-overlap
kernel (cases, recipes and the mpmath reference: tests/_overlaps.py, ``SCOPE_CASES`` and ``make_scope_case``).

    python tests/golden/make_overlap_scope.py                        # every case
    python tests/golden/make_overlap_scope.py c5_32_core0 c6_42_q5   # some

Per case: the inputs themselves (s, bra, ket, index -- empty: no table --, ncas, n_alpha, n_beta, n_core, mode, signed),
``out`` and ``core_det`` from 40-digit arithmetic rounded once, ``host_err`` / ``host_core_err`` (the float64 host route
on the same inputs against them), ``cond_core`` = cond(s_cc) and ``cond_U`` = cond(U) per pair.  The files are
reproduced bit for bit by a second run.

Run time (one core): at most 8 s per case (c8_43_core40, c8_34_core40, c8_53_*), about one minute in all."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import _overlaps as V          # noqa: E402


def make(name):
    t0 = time.time()
    out = V.make_scope_case(name)
    np.savez(V.scope_fixture_path(name), **out)
    print(f"{name}: max |out| {np.abs(out['out']).max():.3g}, core_det {out['core_det'][0]:+.6g}, host error "
          f"{out['host_err']:.2e}, of core_det {out['host_core_err']:.2e}, cond(s_cc) {out['cond_core'].max():.3g}, "
          f"cond(U) {out['cond_U'].max():.3g}, {os.path.getsize(V.scope_fixture_path(name))} bytes, "
          f"{time.time() - t0:.0f} s", flush=True)


if __name__ == "__main__":
    for case in (sys.argv[1:] or V.SCOPE_CASES):
        make(case)
