"""Fixtures of the point-charge embedding tests (tests/test_charges_cpu.py, tests/test_charges_gpu.py): clouds of
classical charges around the test molecules, the bases, and host references made once per process.

A cloud has a fixed seed, |q| <= 1 and both signs.  Its first charges are the special ones, so that every prefix used
as a smaller cloud keeps the hard cases in front:

    0   ``NEAR`` Bohr from atom 0 (inside the tightest Gaussians of the basis)
    1   exactly ON atom 1 (T = 0 for that atom's one-centre pairs) -- or, ``on_nucleus=False``, at a generic place:
        the classical term Z q / |R - r| of the embedded energy and its derivative do not exist for such a charge
    2   50 Bohr away (the large-T branch of the Boys function)
    3   q = 0
    4.. random positions in a shell of 3 .. 12 Bohr around atom 0

Positions are handed out in Angstrom, as the ``*_batch`` functions take them; ``bohr`` converts exactly as the library
does, so the charge on a nucleus stays on it bit for bit.
"""
import functools

import numpy as np

from auto_oo_amd import gaussian, gto

from tests import _gto_d as D

BOHR = gaussian.BOHR
NEAR = 0.2                      # Bohr: distance of charge 0 from atom 0
M_MAX = 130
M_SIZES = (1, 63, 64, 65, 130)   # below, at and above one wave of 64 lanes; 130 = two chunks of the gradient and a rest

WATER = D.WATER
HF_XYZ = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.1]])


def cloud(xyz_angstrom, M=M_MAX, on_nucleus=True, seed=20240607, near=NEAR):
    """-> (q [M], positions [M, 3] in Angstrom) around the molecule ``xyz_angstrom`` [natm, 3]."""
    rng = np.random.default_rng(seed)
    R = np.asarray(xyz_angstrom, dtype=float) / BOHR
    q = rng.uniform(-1.0, 1.0, M_MAX)
    u = rng.normal(size=(M_MAX, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    r = R[0] + u * rng.uniform(3.0, 12.0, M_MAX)[:, None]
    q[0], r[0] = 0.8, R[0] + near * np.array([0.48, -0.6, 0.64])
    q[1] = -0.7
    q[2], r[2] = 0.9, R[0] + 50.0 * np.array([-0.6, 0.64, 0.48])
    q[3] = 0.0
    ang = r * BOHR
    if on_nucleus:
        ang[1] = np.asarray(xyz_angstrom, dtype=float)[1]
    assert q.min() < 0 < q.max() and np.abs(q).max() <= 1.0
    return q[:M].copy(), ang[:M].copy()


def bohr(x_angstrom):
    return np.asarray(x_angstrom, dtype=float) / BOHR


@functools.lru_cache(maxsize=None)
def water_basis():
    return gto.GTOBasis(["O", "H", "H"])


@functools.lru_cache(maxsize=None)
def hf_basis():
    return gto.GTOBasis(["H", "F"])


@functools.lru_cache(maxsize=None)
def m2_cartesian_basis():
    """M2 of tests/_gto_d.py with its d shell as 6 Cartesian functions."""
    par = gaussian._STO3G
    table = {"O": [("s", par["O"]["1s"], gaussian._STO3G_1S_COEF), ("s", par["O"]["2sp"], gaussian._STO3G_2S_COEF),
                   ("p", par["O"]["2sp"], gaussian._STO3G_2P_COEF), ("d", [0.8], [1.0])],
             "H": [("s", par["H"]["1s"], gaussian._STO3G_1S_COEF), ("p", [1.1], [1.0])]}
    return gto.GTOBasis(["O", "H", "H"], table, d_functions="cartesian")


def case(name):
    """-> (basis, geometry in Angstrom) of an operator case."""
    return {"water": (water_basis(), WATER), "m1-spherical": (D.m1_basis("spherical"), D.M1_XYZ),
            "m1-cartesian": (D.m1_basis("cartesian"), D.M1_XYZ), "m2-spherical": (D.m2_basis(), WATER),
            "m2-cartesian": (m2_cartesian_basis(), WATER)}[name]


CASES = ("water", "m1-spherical", "m1-cartesian", "m2-spherical", "m2-cartesian")


def host_operator(basis, xyz_angstrom, q, r_angstrom):
    return gaussian.point_charge_integrals_from_table(basis.table, bohr(xyz_angstrom), q, bohr(r_angstrom),
                                                      basis.d_functions or "spherical")


@functools.lru_cache(maxsize=None)
def host_operator_of(name, M):
    """The host twin's operator of a case with the first M charges of its cloud (made once, never modified)."""
    basis, xyz = case(name)
    q, r = cloud(xyz, M)
    V = host_operator(basis, xyz, q, r)
    V.setflags(write=False)
    return V


def random_symmetric(n, seed):
    a = np.random.default_rng(seed).uniform(-1.0, 1.0, (n, n))
    return 0.5 * (a + a.T)
