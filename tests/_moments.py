"""Shared helpers and measured bounds of the moment tests (tests/test_moments_cpu.py, tests/test_moments_gpu.py).

Molecules: M1 / M2 / WATER of tests/_gto_d.py, H2 with one 1-primitive and one 6-primitive s shell per atom, H-F and
formaldimine in STO-3G.

TOL_M, the bound of the device integrals against the host twin ``gaussian.moment_integrals_from_table``: the kernel
bodies of csrc/gto_moments.hip run on the CPU (tools/gto_moments_host.hip, one lane per workgroup) differ from the host
twin for M1 (plain, shifted, moved) at order 2, both d forms, two origins, by at most HOST_BODY_ERROR elementwise; the host
twin itself agrees with quadrature on a 181^3 grid to HOST_TWIN_ERROR.  The bound is 10 x the larger of the two: the
kernels evaluate the same formulae in another order, and the device contracts a * b + c into one rounding.
"""
import functools
import os
import subprocess
import tempfile

import numpy as np

from auto_oo_amd import gaussian, gto
from tests import _gto_d as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOHR = gaussian.BOHR

HOST_TWIN_ERROR = 4.3e-14         # host twin against quadrature (M1 Cartesian, 9 components), measured on the CPU
HOST_BODY_ERROR = 2.7e-15         # kernel bodies on the CPU against the host twin, measured (values up to 8.1)
TOL_M = 10 * max(HOST_TWIN_ERROR, HOST_BODY_ERROR)

ORIGIN = np.array([0.31, -0.17, 0.23])                                    # Angstrom, generic
M1_STACK = np.stack([D.M1_XYZ, D.M1_SHIFTED, D.M1_MOVED])                 # plain, shifted, moved

H2_TABLE = {"H": [("s", [0.8], [1.0]),
                  ("s", [18.73, 2.825, 0.6401, 0.1612, 0.05, 0.02], [0.03, 0.2, 0.5, 0.4, 0.1, 0.05])]}
H2_XYZ = np.array([[0.02, -0.01, -0.36], [0.05, 0.07, 0.39]])
HF_XYZ = np.array([[0.03, -0.02, 0.0], [-0.06, 0.04, 0.93]])


def h2_basis():
    return gto.GTOBasis(["H", "H"], H2_TABLE)


def hf_basis():
    return gto.GTOBasis(["H", "F"])


def form_of(basis):
    return basis.d_functions or "spherical"


_TWIN = {}


def host_moments(basis, xyz_angstrom, order=2, origin_angstrom=None):
    """The host twin for one geometry, [3 or 9, N, N] in atomic units.  The twin takes seconds for M1 (recursive ``_E``
    per function pair): its Cartesian order-2 result is kept per (table, geometry, origin), and the form and order asked
    for follow from it the way the twin itself makes them."""
    xyz = np.ascontiguousarray(np.asarray(xyz_angstrom, dtype=float) / BOHR)
    o = np.zeros(3) if origin_angstrom is None else np.asarray(origin_angstrom, dtype=float) / BOHR
    key = (repr(basis.table), xyz.tobytes(), o.tobytes())
    if key not in _TWIN:
        _TWIN[key] = gaussian.moment_integrals_from_table(basis.table, xyz, "cartesian", 2, o)
    U = gaussian.basis_transform(basis.table, form_of(basis))
    out = U @ _TWIN[key][:3 if order == 1 else 9] @ U.T
    return 0.5 * (out + out.transpose(0, 2, 1))


def host_overlap(basis, xyz_angstrom):
    """The host overlap [N, N] of one geometry (no two-electron integrals are made)."""
    xyz = np.asarray(xyz_angstrom, dtype=float) / BOHR
    S = gaussian.one_electron_integrals(gaussian.shells_from_table(basis.table, xyz), [], [])[0]
    U = gaussian.basis_transform(basis.table, form_of(basis))
    return U @ S @ U.T


def nuclear_terms(charges, xyz_bohr, order=2, origin_bohr=None):
    """Z_A (R_A - O)^c, [3 or 9, natm]."""
    r = np.asarray(xyz_bohr) - (0.0 if origin_bohr is None else np.asarray(origin_bohr))
    comps = gaussian.MOMENT_COMPONENTS[:3 if order == 1 else 9]
    return np.array([charges * r[:, 0] ** ex * r[:, 1] ** ey * r[:, 2] ** ez for ex, ey, ez in comps])


def nuclear_moments(charges, xyz_bohr, order=2, origin_bohr=None):
    """sum_A Z_A (R_A - O)^c, [3 or 9]."""
    return nuclear_terms(charges, xyz_bohr, order, origin_bohr).sum(axis=1)


# ---- quadrature ---------------------------------------------------------------------------------------------------------
def grid_values(shell, x, y, z):
    """A ``gaussian._Shell`` on the product grid x (x) y (x) z, as three 1-D factors (the function is their product)."""
    out = []
    for d, q in enumerate((x, y, z)):
        r = q - shell.center[d]
        out.append(r ** shell.lmn[d] * np.exp(-np.outer(shell.exps, r * r)))            # [nprim, n]
    return out


def quadrature_moments(A, B, origin_bohr, n=181, half=9.0):
    """<A| (r - O)^c |B> for the 9 components and the overlap by the trapezoid rule on an n^3 grid over [-half, half]^3
    (spectrally accurate for Gaussians that have decayed at the border).  The integrand is a sum over primitive pairs of
    products of three 1-D integrals, which is what the grid sum factorises into: no n^3 array is formed."""
    q = np.linspace(-half, half, n)
    h = q[1] - q[0]
    fa, fb = grid_values(A, q, q, q), grid_values(B, q, q, q)
    one = []                      # [d][e]: [na, nb] 1-D sums of (q - O_d)^e a_d b_d
    for d in range(3):
        w = q - origin_bohr[d]
        one.append([h * np.einsum("in,jn,n->ij", fa[d], fb[d], w ** e) for e in range(3)])
    cc = np.outer(A.coefs, B.coefs)
    vals = [np.sum(cc * one[0][ex] * one[1][ey] * one[2][ez]) for ex, ey, ez in gaussian.MOMENT_COMPONENTS]
    return np.array(vals), np.sum(cc * one[0][0] * one[1][0] * one[2][0])


# ---- the kernel bodies as a host program ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_program():
    """tools/gto_moments_host.hip compiled for the host alone (no device code, no HIP runtime call), once per session."""
    out = os.path.join(tempfile.mkdtemp(prefix="gto_moments_host_"), "gto_moments_host")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--cuda-host-only", "-O2", "-std=c++17", "-Wno-unused-function",
                    "-I", os.path.join(ROOT, "auto_oo_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "gto_moments_host.hip"), "-o", out, "-lpthread"], check=True)
    return out


def run_host_bodies(basis, xyz_angstrom, order=2, origin_angstrom=None, exe=None):
    """The moment integrals [G, 3 or 9, N, N] of the geometries ``xyz_angstrom`` [G, natm, 3] from the kernel bodies run
    on the CPU.  An element no body writes comes back NaN.  ``exe``: another build of the program (lanes as threads)."""
    xyz = np.asarray(xyz_angstrom, dtype=float) / BOHR
    G = xyz.shape[0]
    o = np.zeros((G, 3)) if origin_angstrom is None else np.broadcast_to(np.asarray(origin_angstrom) / BOHR, (G, 3))
    exe = exe or host_program()
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.txt"), os.path.join(tmp, "out.txt")
        with open(fin, "w") as fh:
            fh.write(f"{basis.nshell} {basis.natm} {G} {basis.nao} {order} {basis.exps.size}\n")
            fh.write(" ".join(str(int(v)) for v in basis.shells.ravel()) + "\n")
            for arr in (basis.exps, basis.coefs, xyz, o):
                fh.write(" ".join(repr(float(v)) for v in np.asarray(arr).ravel()) + "\n")
        subprocess.run([exe, fin, fout], check=True)
        vals = np.loadtxt(fout)
    return vals.reshape(G, 3 if order == 1 else 9, basis.nao, basis.nao)
