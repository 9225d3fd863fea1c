"""Writes tests/golden/response_scope_z_<case>.npz, the canonical RHF orbitals of the Z-vector cases of the scope tests
of the density and orbital-response kernels (cases, recipes and references: tests/_response_scope.py, ``Z_CASES`` and
``make_z_case``).

    python tests/golden/make_response_scope.py                # every case
    python tests/golden/make_response_scope.py 2_1 64_32      # some

Per case, with one entry per geometry (seed): ``seeds``, ``mo_coeff`` and ``mo_energy`` of the host ``gaussian.rhf`` at
``conv_tol = 1e-12`` on ``synthetic_problem(n, seed)``; ``lam_min`` and ``lam_max`` of the virt-occ matrix A and
``cond_pre``, the condition number of A preconditioned with the orbital-energy differences; ``off_diagonal``, the
largest off-diagonal element of the Fock matrix in these orbitals; ``aufbau_gap``; ``class_gap``, the smallest orbital-
energy difference over the occ-occ and virt-virt pairs of the case's active window; ``g_sum`` and ``g_probes``, the sum
and four elements of g, against which a test checks the g it rebuilds from the seed.

A geometry is refused unless RHF converged, the aufbau gap is positive and lambda_min(A) > 0.  The figures above are
printed per geometry.  Run time (one core): up to 10 s per geometry at n = 64, about a minute in all."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import _response_scope as V          # noqa: E402


def make(name):
    t0 = time.time()
    out, lines = V.make_z_case(name)
    np.savez(V.fixture_path(name), **out)
    for line in lines:
        print(line)
    print(f"{name}: {os.path.getsize(V.fixture_path(name))} bytes, {time.time() - t0:.0f} s", flush=True)


if __name__ == "__main__":
    for case in (sys.argv[1:] or V.Z_CASES):
        make(case)
