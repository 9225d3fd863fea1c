"""Test molecules of the d-shell tests (tests/test_gto_d_cpu.py, tests/test_gto_d_gpu.py) and the bounds measured
for them on the CPU.

M1: three centres in general position (not collinear, no coordinate zero); A carries s (2 primitives) and d (2
primitives, contracted), B p and d, C s: 15 spherical / 17 Cartesian functions, all 6 pair classes and all 21 quartet
classes, a d-d pair on one shell, d-d pairs across centres, quartets with a repeated pair.  Smallest overlap
eigenvalue 0.57 (spherical) / 0.25 (Cartesian).  The element symbols only set the charges (14 electrons).

M2: water at the geometry of tests/test_nucgrad_gpu.py in STO-3G plus a d shell on O and a p shell on each H: 18
spherical functions.
"""
import functools

import numpy as np

from auto_oo_amd import gaussian, gto

M1_SYMBOLS = ["C", "N", "H"]
M1_TABLE = {"C": [("s", [1.9, 0.45], [0.4, 0.7]), ("d", [1.1, 0.35], [0.55, 0.6])],
            "N": [("p", [0.9], [1.0]), ("d", [0.8], [1.0])],
            "H": [("s", [0.6], [1.0])]}
M1_XYZ = np.array([[0.11, -0.23, 0.17], [0.95, 0.61, -0.42], [-0.53, 0.88, 0.71]])        # Angstrom
ROTATION = gaussian._rotation([0.3, -0.5, 0.8], 0.77)                                       # generic axis and angle
SHIFT = np.array([0.4, -0.3, 0.25])
M1_ROTATED = M1_XYZ @ ROTATION.T
M1_SHIFTED = M1_XYZ + SHIFT
M1_MOVED = M1_XYZ @ ROTATION.T + SHIFT

WATER = np.array([[0.0, 0.01, 0.02], [0.3, 0.75, 0.55], [-0.2, -0.70, 0.62]])             # tests/test_nucgrad_gpu.py
WATER_2 = np.array([[0.0, 0.01, 0.02], [0.33, 0.78, 0.52], [-0.2, -0.66, 0.66]])

# Relative error of the host Boys function gaussian._boys (scipy hyp1f1) against 40-digit arithmetic (mpmath), per
# order n = 0 .. 8, on the grid of the Boys tests (T = 0, 4001 points on [0, 40], 4001 on [40, 2000]); measured on
# the CPU ("d shells").  The device function is asked to agree with the host one to 10 x this.
HOST_BOYS_ERROR = (2.12e-15, 2.21e-15, 2.23e-15, 2.19e-15, 4.10e-15, 1.19e-14, 2.70e-14, 5.59e-14, 1.60e-13)
BOYS_RTOL = tuple(10 * e for e in HOST_BOYS_ERROR)


def m1_basis(d_functions):
    return gto.GTOBasis(M1_SYMBOLS, M1_TABLE, d_functions=d_functions)


@functools.lru_cache(maxsize=None)
def m2_basis():
    par = gaussian._STO3G
    table = {"O": [("s", par["O"]["1s"], gaussian._STO3G_1S_COEF), ("s", par["O"]["2sp"], gaussian._STO3G_2S_COEF),
                   ("p", par["O"]["2sp"], gaussian._STO3G_2P_COEF), ("d", [0.8], [1.0])],
             "H": [("s", par["H"]["1s"], gaussian._STO3G_1S_COEF), ("p", [1.1], [1.0])]}
    return gto.GTOBasis(["O", "H", "H"], table, d_functions="spherical")


@functools.lru_cache(maxsize=None)
def m1_host_cartesian(which="plain"):
    """Host integrals of M1 over its 17 normalised Cartesian functions (7 s): ``plain`` or ``moved`` (rotated and
    translated).  Both forms of the basis follow from them by ``gaussian.basis_transform``."""
    basis = m1_basis("cartesian")
    xyz = {"plain": M1_XYZ, "moved": M1_MOVED}[which]
    return gaussian.cartesian_integrals_from_table(basis.table, basis.charges, xyz / gaussian.BOHR)


def m1_host(d_functions, which="plain"):
    U = gaussian.basis_transform(m1_basis("cartesian").table, d_functions)
    return gaussian.transform_integrals(U, *m1_host_cartesian(which))
