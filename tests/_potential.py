"""Cases, references and bounds of the electrostatic-potential tests (tests/test_potential_cpu.py,
tests/test_potential_gpu.py).  Everything here runs on the host; a reference is made once per process and never
modified.

Cases: the molecules of tests/_charges.py (water STO-3G, M1 in both d forms, M2) with the 130-point cloud of that module
as the points (point 0 is 0.2 Bohr from atom 0, point 1 ON atom 1, point 2 50 Bohr away), K = 3 random NON-symmetric
densities; and the two-centre one-class cases Lss .. Ldd of tests/_gto_edges.py (``"Lds"`` is the case in the d form of
its table, ``"Lds/cartesian"`` the same shells in the other form) with the first 65 points of their cloud and one density
whose only non-zero blocks are the pair class and its transpose.

Bounds ("Accuracy bounds": measured on the CPU, none taken from the device):

* potential, device (or kernel bodies on the CPU) against the host twin ``gaussian.potential_from_table``: the twin is
  evaluated twice, plain and with its Boys function of order n multiplied by 1 + 10 x HOST_BOYS_ERROR[n] x (+-1)
  (``_gto_edges.perturbed_boys``); ``POTENTIAL_BOUND[case]`` = 10 x their largest difference over sets and points
  (electronic part; measured by ``measured_potential_bound``, ``python -m pytest tests/test_potential_cpu.py -s -k
  bounds``).
* field: the reference of the ELECTRONIC field is the 4th-order central difference of the host potential (``nuc=False``)
  in the position of the point at h = 1e-3 Bohr; the bound, per set, point and component, is max(1e-9, 10 x its
  disagreement with h = 2e-3).  Points closer than ``FD_EXCLUDE`` = 0.05 Bohr to a nucleus are left out of this reference
  only (1 of 130: the point on the nucleus; the cap is 2).  The nuclear field has the closed form Z (r - R) / |r - R|^3 and
  is compared with that, to ``CLASSICAL_RTOL`` of the sum of the absolute terms.
* two analytic fp64 evaluations in different summation order (potential against the embedding operator, field against
  the forces on the charges): ``CLASSICAL_RTOL`` = 1e-12 relative to the sum of the absolute terms, the bound of
  ``test_classical_term_of_the_raw_gradients``.
"""
import functools
import os
import subprocess
import tempfile

import numpy as np

from auto_oo_amd import gaussian, gto
from tests import _charges as C
from tests import _gto_d as D
from tests import _gto_edges as E

BOHR = gaussian.BOHR
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 3
MOL_CASES = ("water", "m1-spherical", "m1-cartesian", "m2-spherical")
L_NAMES = ("Lss", "Lps", "Lpp", "Lds", "Ldp", "Ldd")
L_CASES = ("Lss", "Lps", "Lpp", "Lds", "Lds/cartesian", "Ldp", "Ldp/spherical", "Ldd", "Ldd/cartesian")
M_CLASS = 65
FD_H = 1e-3
FD_EXCLUDE = 0.05
FD_EXCLUDE_CAP = 2
CLASSICAL_RTOL = 1e-12
PERTURB_SEED = 7

# 10 x the largest change the perturbed Boys function makes to the host potential (electronic part), per case
POTENTIAL_BOUND = {
    "water": 5.24e-13, "m1-spherical": 7.18e-13, "m1-cartesian": 7.02e-13, "m2-spherical": 5.56e-13,
    "Lss": 5.66e-14, "Lps": 1.01e-13, "Lpp": 3.80e-14, "Lds": 6.61e-14, "Lds/cartesian": 7.74e-14, "Ldp": 1.29e-13,
    "Ldp/spherical": 1.81e-13, "Ldd": 3.28e-13, "Ldd/cartesian": 1.25e-13,
}


# ---- cases ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def basis_of(name):
    if name in C.CASES:
        return C.case(name)[0]
    base, _, form = name.partition("/")
    if not form:
        return E.basis_of(base)
    sym, table, _, _ = E.case(base)
    return gto.GTOBasis(sym, table, d_functions=form)


def angstrom_of(name):
    return C.case(name)[1] if name in C.CASES else E.angstrom_of(name.partition("/")[0])


def xyz_of(name):
    """[natm, 3] in Bohr, the bits the library makes of ``angstrom_of``"""
    return angstrom_of(name) / BOHR


def form_of(name):
    return basis_of(name).d_functions or "spherical"


def points_angstrom(name):
    """The cloud of tests/_charges.py around the case (charge ON atom 1 included): 130 points, 65 for an L-case."""
    return C.cloud(angstrom_of(name), C.M_MAX if name in C.CASES else M_CLASS)[1]


def points_of(name):
    return points_angstrom(name) / BOHR


def cloud_charges(name):
    return C.cloud(angstrom_of(name), C.M_MAX if name in C.CASES else M_CLASS)[0]


@functools.lru_cache(maxsize=None)
def densities(name, nset=K, seed=11):
    """[nset, N, N] random in (-1, 1), NOT symmetric"""
    N = basis_of(name).nao
    d = np.random.default_rng(seed).uniform(-1.0, 1.0, (nset, N, N))
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def class_density(name):
    """[1, N, N] of an L-case: random in the block (first shell, second shell) and, independently, in its transpose;
    zero in the two one-centre blocks."""
    basis = basis_of(name)
    f = int(basis.shells[0, 1])                 # (one shell per atom: shell 0 is the first block of functions)
    na = 6 if f == (2 | gto.CARTESIAN) else 2 * (f & 255) + 1
    d = np.random.default_rng(13).uniform(-1.0, 1.0, (1, basis.nao, basis.nao))
    d[:, :na, :na] = 0.0
    d[:, na:, na:] = 0.0
    d.setflags(write=False)
    return d


def density_of(name):
    return densities(name) if name in C.CASES else class_density(name)


# ---- host references ----------------------------------------------------------------------------------------------------
def host_potential(name, points_bohr, dm, nuc=False, boys=None):
    basis = basis_of(name)
    return gaussian.potential_from_table(basis.table, basis.charges, xyz_of(name), points_bohr, dm, form_of(name), nuc,
                                         boys)


@functools.lru_cache(maxsize=None)
def host_phi(name):
    """Electronic potential [K or 1, M] of the case at its points for its densities (host twin)."""
    phi = host_potential(name, points_of(name), density_of(name))
    phi.setflags(write=False)
    return phi


def nuclear_potential(name, points_bohr):
    """sum_A Z_A / |R_A - r| [M] and the field Z (r - R) / |r - R|^3 [M, 3] with the sums of their absolute terms"""
    Z, R = basis_of(name).charges, xyz_of(name)
    d = np.asarray(points_bohr)[:, None, :] - R[None, :, :]
    r = np.linalg.norm(d, axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = Z[None, :, None] * d / r[:, :, None] ** 3
        return np.sum(Z / r, axis=1), terms.sum(axis=1), np.abs(terms).sum(axis=1)


def measured_potential_bound(name):
    plain = host_phi(name)
    pert = host_potential(name, points_of(name), density_of(name), boys=E.perturbed_boys(PERTURB_SEED))
    return 10.0 * float(np.abs(pert - plain).max())


def boys_points(name="Lss"):
    """[7, 3] Bohr around atom 0 of the 10-primitive case: ON the atom (T = 0 for its one-centre pairs), at the distances
    that put T = p d^2 at 5 (1 -+ 1e-9) (GTO_BOYS_SWITCH) for the tightest and the loosest primitive pair of the atom's
    shell with itself (p = 2 a), 60 Bohr and 2000 Bohr away."""
    basis, A = basis_of(name), xyz_of(name)[0]
    ex = np.asarray(basis.table[0][2])
    u = np.array([0.48, -0.6, 0.64])
    d = [0.0] + [np.sqrt(5.0 * (1.0 + s * 1e-9) / (2.0 * a)) for a in (ex.max(), ex.min()) for s in (-1.0, 1.0)]
    return np.stack([A + x * u for x in d + [60.0, 2000.0]])


def measured_bound_at(name, points_bohr, dm):
    """10 x the largest change the perturbed Boys function makes to the host potential at other points"""
    plain = host_potential(name, points_bohr, dm)
    pert = host_potential(name, points_bohr, dm, boys=E.perturbed_boys(PERTURB_SEED))
    return plain, 10.0 * float(np.abs(pert - plain).max())


def kept_points(name, points_bohr=None):
    """mask [M] of the points at least FD_EXCLUDE from every nucleus"""
    pts = points_of(name) if points_bohr is None else points_bohr
    return np.linalg.norm(pts[:, None, :] - xyz_of(name)[None, :, :], axis=2).min(axis=1) >= FD_EXCLUDE


def difference_field(potential, points_bohr, h=FD_H):
    """(F [..., M, 3], bound [..., M, 3]): minus the 4th-order central difference of ``potential(points) -> [..., M]`` at
    the step h, and max(1e-9, 10 x its disagreement with the step 2h).  One call of ``potential`` for all 18 M displaced
    points."""
    pts = np.asarray(points_bohr, dtype=float)
    M = pts.shape[0]
    steps = (-4, -2, -1, 1, 2, 4)
    moved = np.stack([pts + s * h * np.eye(3)[d] for d in range(3) for s in steps])           # [18, M, 3]
    phi = potential(moved.reshape(-1, 3))
    phi = phi.reshape(phi.shape[:-1] + (3, len(steps), M))
    v = {s: phi[..., i, :] for i, s in enumerate(steps)}                                       # [..., 3, M]
    d1 = (8.0 * (v[1] - v[-1]) - (v[2] - v[-2])) / (12.0 * h)
    d2 = (8.0 * (v[2] - v[-2]) - (v[4] - v[-4])) / (24.0 * h)
    F = -np.moveaxis(d1, -2, -1)
    return F, np.maximum(1e-9, 10.0 * np.abs(np.moveaxis(d1 - d2, -2, -1)))


@functools.lru_cache(maxsize=None)
def host_field(name):
    """(F [K, M', 3], bound [K, M', 3], kept [M]) of the electronic field at the kept points of the case"""
    kept = kept_points(name)
    dm = density_of(name)
    F, bound = difference_field(lambda p: host_potential(name, p, dm), points_of(name)[kept])
    for a in (F, bound, kept):
        a.setflags(write=False)
    return F, bound, kept


# ---- the analytic anchor: one normalised s primitive ---------------------------------------------------------------------
def s_primitive_potential(a, r):
    """-erf(sqrt(2a) r) / r, -2 sqrt(2a / pi) at r = 0: the electronic potential of the density of one normalised s
    primitive of exponent a at the distance r (no McMurchie-Davidson code)."""
    from scipy.special import erf
    r = np.asarray(r, dtype=float)
    s = np.sqrt(2.0 * a)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(r == 0.0, -2.0 * s / np.sqrt(np.pi), -erf(s * r) / r)


def s_primitive_field(a, rvec):
    """minus the gradient of ``s_primitive_potential`` at the points rvec [M, 3] (zero at the centre): along r,
    -(erf(s r) / r^2 - 2 s exp(-s^2 r^2) / (sqrt(pi) r)), s = sqrt(2a).  The two terms cancel to r^3 at small r, so they
    are evaluated in 40-digit arithmetic and rounded."""
    import mpmath as mp
    rvec = np.asarray(rvec, dtype=float)
    out = np.zeros_like(rvec)
    with mp.workdps(40):
        s = mp.sqrt(2 * mp.mpf(float(a)))
        for i, v in enumerate(rvec):
            x = [mp.mpf(float(c)) for c in v]
            r = mp.sqrt(x[0] ** 2 + x[1] ** 2 + x[2] ** 2)
            if r == 0:
                continue
            dphi = mp.erf(s * r) / r ** 2 - 2 * s * mp.exp(-(s * r) ** 2) / (mp.sqrt(mp.pi) * r)
            out[i] = [float(-dphi * c / r) for c in x]
    return out


# ---- the kernel bodies as a host program ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_program(threads=0):
    """tools/gto_potential_host.hip compiled for the host alone (no device code, no HIP runtime call), once per session;
    ``threads``: that many lanes per workgroup as host threads with a real barrier."""
    out = os.path.join(tempfile.mkdtemp(prefix="gto_potential_host_"), "gto_potential_host")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    extra = [f"-DGTO_POT_THREADS={threads}"] if threads else []
    subprocess.run([hipcc, "--cuda-host-only", "-O2", "-std=c++17", "-Wno-unused-function", *extra,
                    "-I", os.path.join(ROOT, "auto_oo_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "gto_potential_host.hip"), "-o", out, "-lpthread"], check=True)
    return out


def run_host_bodies(basis, xyz_bohr, points_bohr, dm, nuc_mask=0, field=True, exe=None):
    """(phi [G, K, M], F [G, K, M, 3] or None) of the geometries ``xyz_bohr`` [G, natm, 3], points [G, M, 3] and
    densities [G, K, N, N] from the kernel bodies run on the CPU.  An element no body writes comes back NaN."""
    xyz, pts, dm = (np.asarray(x, dtype=float) for x in (xyz_bohr, points_bohr, dm))
    G, nset, M = xyz.shape[0], dm.shape[1], pts.shape[1]
    exe = exe or host_program()
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.txt"), os.path.join(tmp, "out.txt")
        with open(fin, "w") as fh:
            fh.write(f"{basis.nshell} {basis.natm} {G} {basis.nao} {nset} {M} {int(field)} {int(nuc_mask)} "
                     f"{basis.exps.size}\n")
            fh.write(" ".join(str(int(v)) for v in basis.shells.ravel()) + "\n")
            for arr in (basis.exps, basis.coefs, basis.charges, xyz, dm, pts):
                fh.write(" ".join(repr(float(v)) for v in np.asarray(arr).ravel()) + "\n")
        subprocess.run([exe, fin, fout], check=True)
        vals = np.loadtxt(fout)
    n = G * nset * M
    return vals[:n].reshape(G, nset, M), (vals[n:].reshape(G, nset, M, 3) if field else None)
