"""Cases, references and bounds of the electron-density tests (tests/test_density_cpu.py, tests/test_density_gpu.py).
Everything here runs on the host; a reference is made once per process and never modified.

Cases: those of tests/_potential.py (``MOL_CASES``: water STO-3G, M1 in both d forms, M2 with the 130-point cloud, point 0
0.2 Bohr from atom 0, point 1 ON atom 1, point 2 50 Bohr away, K = 3 random NON-symmetric densities; ``L_CASES``: the
one-class cases with ``class_density`` and 65 points).  The orbitals of a case are a seeded random C [N, 3].  No point is
left out of any comparison.

Bound of the device (or of the kernel bodies on the CPU) against the host twins ``gaussian.density_from_table`` and
``gaussian.orbital_values_from_table``, per value ("Electron density at points"; every figure comes from the
inputs and the number format, none from the device):

    |device - twin| <= u c A + FLOOR,      u = 2^-53,   c = chain + C_FACTOR + 2 ARG_ERR X_MAX

``A`` is the twin's sum of the absolute values of all the terms of that value.  ``chain``: the additions on the longest
chain of one value: the shell pairs (the sums of a lane's column), the 36 + 6 products of a dd pair, twice the primitives
of a shell (two radial sums meet in a term), 8 for the symmetrisation and the two d back-transforms.  ``C_FACTOR`` = 24:
the roundings of the factors of one term (two coordinate differences, two monomials of up to three factors each, two
contraction coefficients with -2a, the products with the radial sums, the two exponentials' own error of one ulp).
``X_MAX`` = 745.14 is the largest argument whose exponential is not zero in fp64, and an argument a r^2 is computed with a
relative error of at most ``ARG_ERR`` = 6 u (u from each difference, doubled by the square, u per square, 2 u from the two
additions, u from the product with a), so e^(-x) carries 6 x u; a term holds two exponentials.  ``FLOOR`` = 1e-300 stands
for products that underflow (absolute error below 2^-1022 per term).
"""
import functools
import os
import subprocess
import tempfile
from unittest import mock

import numpy as np

from auto_oo_amd import gaussian
from tests import _potential as P

BOHR = gaussian.BOHR
ROOT = P.ROOT
U = 2.0 ** -53
X_MAX = 745.14
ARG_ERR = 6
C_FACTOR = 24
FLOOR = 1e-300
NCOL = 3
LAX = 1000.0                   # a planted defect must move some compared value by more than this many bounds
FD_K = 1                       # the Poisson check differentiates at h = 1e-3 FD_K Bohr
QUAD_H = 0.3                   # Bohr: spacing of the quadrature grid
QUAD_N = 49                    # points per axis (half-width 7.2 Bohr around the centroid)
# |sum chi chi h^3 - S| on that grid, measured with the host code (test_quadrature_reproduces_the_overlap prints them)
QUAD_MEASURED = {"m1-spherical": 4.3e-11, "m1-cartesian": 5.9e-11}
DEFECTS = ("sqrt3", "m-swap", "no-transpose", "gradient-term", "coefficient", "last-chunk")


# ---- the bound -----------------------------------------------------------------------------------------------------------
def bound_constant(basis):
    chain = basis.nshell * (basis.nshell + 1) // 2 + 36 + 6 + 2 * basis.max_nprim + 8
    return chain + C_FACTOR + 2 * ARG_ERR * X_MAX


def bound_of(name, A):
    """the bound of every value whose absolute sum is ``A`` (array)"""
    return U * bound_constant(P.basis_of(name)) * np.asarray(A) + FLOOR


# ---- host references --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def coefficients(name):
    """[N, NCOL] random in (-1, 1)"""
    c = np.random.default_rng(17).uniform(-1.0, 1.0, (P.basis_of(name).nao, NCOL))
    c.setflags(write=False)
    return c


def twin_density(name, points_bohr=None, dm=None):
    basis = P.basis_of(name)
    return gaussian.density_from_table(basis.table, P.xyz_of(name), P.points_of(name) if points_bohr is None else
                                       points_bohr, P.density_of(name) if dm is None else dm, P.form_of(name), True)


def twin_orbitals(name, points_bohr=None):
    basis = P.basis_of(name)
    return gaussian.orbital_values_from_table(basis.table, P.xyz_of(name), P.points_of(name) if points_bohr is None else
                                              points_bohr, coefficients(name), P.form_of(name), True)


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def host_density(name):
    """(rho [K, M], drho [K, M, 3], A, dA) of the case at its points for its densities (host twin)"""
    return _frozen(twin_density(name))


@functools.lru_cache(maxsize=None)
def host_orbitals(name):
    """(psi [NCOL, M], dpsi [NCOL, M, 3], A, dA) of the case at its points for its coefficients (host twin)"""
    return _frozen(twin_orbitals(name))


def ratios(name, got, want=None, kind="density"):
    """largest |got - twin| / bound over all values, for the value and for its gradient; ``got`` = (value, gradient)"""
    ref = (host_density(name) if kind == "density" else host_orbitals(name)) if want is None else want
    out = []
    for g, r, a in ((got[0], ref[0], ref[2]), (got[1], ref[1], ref[3])):
        with np.errstate(invalid="ignore"):
            q = np.abs(np.asarray(g) - r) / bound_of(name, a)
        out.append(float(np.nan_to_num(q, nan=np.inf).max()))
    return tuple(out)


# ---- the same formulas in 40-digit arithmetic --------------------------------------------------------------------------------
def multiprecision_errors(name):
    """|fp64 twin - the same formula in 40-digit arithmetic| (floats) for rho, drho, psi, dpsi of the case: the inputs
    are the fp64 numbers the twin starts from (centres, points, exponents, normalised coefficients, the transform)."""
    import mpmath as mp
    basis = P.basis_of(name)
    R, pts = P.xyz_of(name), np.clip(P.points_of(name), -gaussian.POINT_CLAMP, gaussian.POINT_CLAMP)
    shells = gaussian.shells_from_table(basis.table, R)
    T = gaussian.basis_transform(basis.table, P.form_of(name))
    dm, C = P.density_of(name), coefficients(name)
    rho, drho, _, _ = host_density(name)
    psi, dpsi, _, _ = host_orbitals(name)
    M, N = pts.shape[0], T.shape[0]
    err = [np.zeros_like(x) for x in (rho, drho, psi, dpsi)]
    with mp.workdps(40):
        f = mp.mpf
        Tm = [[(c, f(float(T[p, c]))) for c in range(T.shape[1]) if T[p, c] != 0.0] for p in range(N)]
        Dm = [[[f(float(x)) for x in row] for row in d] for d in dm]
        Dt = [[[f(float(x)) for x in row] for row in d.T] for d in dm]
        Cm = [[f(float(x)) for x in col] for col in C.T]
        for m in range(M):
            cart, dcart = [], []
            for sh in shells:
                d = [f(float(pts[m, k])) - f(float(sh.center[k])) for k in range(3)]
                r2 = d[0] ** 2 + d[1] ** 2 + d[2] ** 2
                e = [mp.exp(-f(float(a)) * r2) for a in sh.exps]
                r0 = mp.fsum(f(float(c)) * x for c, x in zip(sh.coefs, e))
                r1 = mp.fsum(-2 * f(float(a)) * f(float(c)) * x for a, c, x in zip(sh.exps, sh.coefs, e))
                pw = [d[k] ** sh.lmn[k] for k in range(3)]
                poly = pw[0] * pw[1] * pw[2]
                cart.append(poly * r0)
                g = []
                for k in range(3):
                    low = f(0)
                    if sh.lmn[k] > 0:
                        low = sh.lmn[k] * d[k] ** (sh.lmn[k] - 1) * pw[(k + 1) % 3] * pw[(k + 2) % 3]
                    g.append(low * r0 + d[k] * poly * r1)
                dcart.append(g)
            chi = [mp.fsum(t * cart[c] for c, t in row) for row in Tm]
            dchi = [[mp.fsum(t * dcart[c][k] for c, t in row) for row in Tm] for k in range(3)]
            for ks in range(len(Dm)):
                t = [mp.fdot(Dm[ks][p], chi) for p in range(N)]
                tt = [mp.fdot(Dt[ks][p], chi) for p in range(N)]
                err[0][ks, m] = float(abs(f(float(rho[ks, m])) - mp.fdot(chi, t)))
                for k in range(3):
                    want = mp.fsum(dchi[k][p] * (t[p] + tt[p]) for p in range(N))
                    err[1][ks, m, k] = float(abs(f(float(drho[ks, m, k])) - want))
            for i in range(len(Cm)):
                err[2][i, m] = float(abs(f(float(psi[i, m])) - mp.fdot(Cm[i], chi)))
                for k in range(3):
                    err[3][i, m, k] = float(abs(f(float(dpsi[i, m, k])) - mp.fdot(Cm[i], dchi[k])))
    return err


# ---- planted defects ----------------------------------------------------------------------------------------------------
def defective(name, defect):
    """((rho, drho), (psi, dpsi)) of the host twins with one defect a kernel could have"""
    if defect == "sqrt3":            # the sqrt 3 of xy, xz, yz against xx: every d component scaled like xx
        keep = gaussian.component_norm
        patch = mock.patch.object(gaussian, "component_norm", lambda lmn: 3.0 ** -0.5 if sum(lmn) == 2 else keep(lmn))
    elif defect == "m-swap":         # m = -2 and m = -1 of the spherical d functions swapped
        patch = mock.patch.object(gaussian, "_SPHERICAL_D", gaussian._SPHERICAL_D[[1, 0, 2, 3, 4]])
    elif defect == "gradient-term":  # l x^(l-1) dropped
        patch = mock.patch.object(gaussian, "_monomial_derivative", lambda d, lmn, axis: np.zeros(d.shape[0]))
    elif defect == "coefficient":    # the second primitive's coefficient used for the first
        keep = gaussian._radial_sums

        def radial(shell, r2):
            sh = gaussian._Shell.__new__(gaussian._Shell)
            sh.exps, sh.coefs = shell.exps, shell.coefs.copy()
            if sh.coefs.size > 1:
                sh.coefs[0] = sh.coefs[1]
            return keep(sh, r2)
        patch = mock.patch.object(gaussian, "_radial_sums", radial)
    else:
        patch = mock.patch.object(gaussian, "POINT_CLAMP", gaussian.POINT_CLAMP)     # (nothing)
    dm = P.density_of(name)
    if defect == "no-transpose":     # D_ab of a shell pair used without D_ba
        dm = np.tril(dm)
    with patch:
        rho, drho = twin_density(name, dm=dm)[:2]
        psi, dpsi = twin_orbitals(name)[:2]
    if defect == "last-chunk":       # the last partial chunk of 64 points not written
        last = 64 * (rho.shape[-1] // 64)
        rho, drho, psi, dpsi = (x.copy() for x in (rho, drho, psi, dpsi))
        rho[:, last:], drho[:, last:], psi[:, last:], dpsi[:, last:] = 0.0, 0.0, 0.0, 0.0
    return (rho, drho), (psi, dpsi)


def defect_applies(name, defect):
    """a defect of the d functions needs a d shell (of the spherical form), one of l x^(l-1) a p or d shell"""
    basis = P.basis_of(name)
    if defect == "sqrt3":
        return basis.max_l == 2
    if defect == "m-swap":
        return basis.max_l == 2 and P.form_of(name) == "spherical"
    if defect == "coefficient":
        # Lds: the first (tightest, a > 1e3) primitives of its two shells reach no point of its cloud: e^-212 at the point
        # 0.2 Bohr from the s shell, and the d functions vanish at the point ON their centre
        return not name.startswith("Lds")
    return basis.max_l >= 1 if defect == "gradient-term" else True


def defect_ratio(name, defect):
    """the largest move of a compared value, in bounds"""
    den, orb = defective(name, defect)
    return max(ratios(name, den) + ratios(name, orb, kind="orbitals"))


# ---- the Poisson check ----------------------------------------------------------------------------------------------------
def difference_laplacian(potential, points_bohr, h):
    """(L [..., M], disagreement [..., M]): the 4th-order central-difference Laplacian of ``potential(points) -> [..., M]``
    at the step h and its difference from the one at 2h.  One call of ``potential`` for all 19 M points."""
    pts = np.asarray(points_bohr, dtype=float)
    M = pts.shape[0]
    steps = (-4, -2, -1, 1, 2, 4)
    moved = np.concatenate([pts[None]] + [(pts + s * h * np.eye(3)[d])[None] for d in range(3) for s in steps])
    phi = potential(moved.reshape(-1, 3))
    phi = phi.reshape(phi.shape[:-1] + (19, M))
    f0 = phi[..., 0, :]
    L1 = L2 = 0.0
    for d in range(3):
        v = {s: phi[..., 1 + 6 * d + i, :] for i, s in enumerate(steps)}
        L1 = L1 + (-(v[2] + v[-2]) + 16.0 * (v[1] + v[-1]) - 30.0 * f0) / (12.0 * h * h)
        L2 = L2 + (-(v[4] + v[-4]) + 16.0 * (v[2] + v[-2]) - 30.0 * f0) / (48.0 * h * h)
    return L1, np.abs(L1 - L2)


def poisson_floor(name, h):
    """What the error of the reference potential (``P.POTENTIAL_BOUND``) can make of the stencil: 3 axes x 64 / (12 h^2)"""
    return 3.0 * 64.0 / (12.0 * h * h) * P.POTENTIAL_BOUND[name]


# ---- the quadrature grid -----------------------------------------------------------------------------------------------------
def quadrature_points(xyz_bohr):
    """[QUAD_N^3, 3] Bohr: the uniform grid of spacing QUAD_H around the centroid, x slowest"""
    ax = QUAD_H * (np.arange(QUAD_N) - (QUAD_N - 1) / 2.0)
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)
    return g + np.asarray(xyz_bohr).mean(axis=0)[None, :]


@functools.lru_cache(maxsize=None)
def quadrature_errors(name):
    """The errors of the grid for the products of two functions of the case (M1), from the host twin and the host
    integrals: (|sum chi chi h^3 - S| [N, N], |sum d(chi chi) h^3| [3, N, N] (the integral is zero),
    |sum r chi chi h^3 - <r>| [3, N, N], and the sums of the absolute terms of the three: sum |chi chi| h^3 [N, N],
    sum |d chi chi| + |chi d chi| h^3 [3, N, N], sum |r| |chi chi| h^3 [3, N, N])"""
    basis, R = P.basis_of(name), P.xyz_of(name)
    pts = quadrature_points(R)
    T = gaussian.basis_transform(basis.table, P.form_of(name))
    N = T.shape[0]
    S = T @ gaussian.one_electron_integrals(gaussian.shells_from_table(basis.table, R), (), ())[0] @ T.T
    mom = gaussian.moment_integrals_from_table(basis.table, R, P.form_of(name), order=1)
    sq, sa = np.zeros((N, N)), np.zeros((N, N))
    dq, rq, da, ra = (np.zeros((3, N, N)) for _ in range(4))
    w = QUAD_H ** 3
    for a in range(0, pts.shape[0], QUAD_N * QUAD_N):
        p = pts[a:a + QUAD_N * QUAD_N]
        chi, _, dchi, _ = gaussian.functions_at_points(basis.table, R, p, P.form_of(name), True)
        sq += chi @ chi.T * w
        sa += np.abs(chi) @ np.abs(chi).T * w
        t = np.einsum("pmx,qm->xpq", dchi, chi) * w
        dq += t + t.transpose(0, 2, 1)
        t = np.einsum("pmx,qm->xpq", np.abs(dchi), np.abs(chi)) * w
        da += t + t.transpose(0, 2, 1)
        rq += np.einsum("pm,mx,qm->xpq", chi, p, chi) * w
        ra += np.einsum("pm,mx,qm->xpq", np.abs(chi), np.abs(p), np.abs(chi)) * w
    return _frozen((np.abs(sq - S), np.abs(dq), np.abs(rq - mom[:3]), sa, da, ra))


# ---- the kernel bodies as a host program ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_program(threads=0):
    """tools/gto_density_host.hip compiled for the host alone (no device code, no HIP runtime call), once per session;
    ``threads``: that many lanes per workgroup as host threads with a real barrier."""
    out = os.path.join(tempfile.mkdtemp(prefix="gto_density_host_"), "gto_density_host")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    extra = [f"-DGTO_DEN_THREADS={threads}"] if threads else []
    subprocess.run([hipcc, "--cuda-host-only", "-O2", "-std=c++17", "-Wno-unused-function", *extra,
                    "-I", os.path.join(ROOT, "auto_oo_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "gto_density_host.hip"), "-o", out, "-lpthread"], check=True)
    return out


def run_host_bodies(basis, xyz_bohr, points_bohr, x, orbitals=False, gradient=True, exe=None):
    """(value [G, K, M], gradient [G, K, M, 3] or None) of the geometries ``xyz_bohr`` [G, natm, 3], points [G, M, 3] and
    densities [G, K, N, N] (``orbitals``: coefficients [G, N, K]) from the kernel bodies run on the CPU.  An element no
    body writes comes back NaN."""
    xyz, pts, x = (np.asarray(a, dtype=float) for a in (xyz_bohr, points_bohr, x))
    G, M = xyz.shape[0], pts.shape[1]
    nset = x.shape[2] if orbitals else x.shape[1]
    exe = exe or host_program()
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.txt"), os.path.join(tmp, "out.txt")
        with open(fin, "w") as fh:
            fh.write(f"{basis.nshell} {basis.natm} {G} {basis.nao} {nset} {M} {int(gradient)} {int(orbitals)} "
                     f"{basis.exps.size}\n")
            fh.write(" ".join(str(int(v)) for v in basis.shells.ravel()) + "\n")
            for arr in (basis.exps, basis.coefs, xyz, x, pts):
                fh.write(" ".join(repr(float(v)) for v in np.asarray(arr).ravel()) + "\n")
        subprocess.run([exe, fin, fout], check=True)
        vals = np.loadtxt(fout, ndmin=1)
    n = G * nset * M
    return vals[:n].reshape(G, nset, M), (vals[n:].reshape(G, nset, M, 3) if gradient else None)
