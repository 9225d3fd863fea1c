"""AO integrals and RHF orbitals for s/p Gaussian basis sets (STO-3G), on the host (and, as a test oracle for the device
kernels only, of tables with d shells: ``integrals_from_table``).

SURVEY.md section 8(f) rank 3: the reference's ``Moldata_pyscf`` (src/auto_oo/moldata_pyscf.py:19-61)
gets its arrays from PySCF / libcint -- ``int1e_kin + int1e_nuc``, ``int2e``, ``int1e_ovlp``,
``energy_nuc()`` (:28-35), RHF orbitals (:58-61) -- which this container does not have.  For the
basis set of every STO-3G case in the reference's tests and notebooks (formaldimine: N, C, H) the
same quantities are computed here from scratch: contracted s/p Cartesian Gaussians, McMurchie-
Davidson Hermite expansion (overlap, kinetic, nuclear attraction, electron repulsion; Boys function
through the confluent hypergeometric function), a DIIS-accelerated RHF, and PySCF's Z-matrix ->
Cartesian convention.  Third-party algorithm restated: PySCF ``gto.mole.from_zmatrix`` and libcint
conventions (atoms in input order; per atom 1s, 2s, 2px, 2py, 2pz; contracted functions normalised;
1 Bohr = 0.52917721092 Angstrom).  Pinned by the reference's own literals: ``S^-1/2`` of
formaldimine at (alpha, phi) = (140, 80) (test/test_moldata_pyscf.py:21-85), the RHF energy
-92.66372193556138 (test/test_oo_energy.py:396) and the CAS(2,2) energy -92.74923236954386 at the
literal orbitals (test/test_oo_energy.py:298).

This is AO-integral preparation -- outside the hot path, once per geometry, numpy on the host like
the reference's libcint calls; the hot path starts at the arrays it returns.  cc-pVDZ (d shells,
general contractions) is out of scope.
"""
import itertools
from types import SimpleNamespace

import numpy as np
from scipy.special import hyp1f1

from .moldata import Moldata

BOHR = 0.52917721092        # Angstrom; the value PySCF converts with

# STO-3G (EMSL / Basis Set Exchange): exponents, s coefficients, p coefficients per shell
_STO3G_1S_COEF = (0.15432897, 0.53532814, 0.44463454)
_STO3G_2S_COEF = (-0.09996723, 0.39951283, 0.70011547)
_STO3G_2P_COEF = (0.15591627, 0.60768372, 0.39195739)
_STO3G = {
    "H": {"Z": 1, "1s": (3.42525091, 0.62391373, 0.16885540)},
    "C": {"Z": 6, "1s": (71.6168370, 13.0450960, 3.5305122), "2sp": (2.9412494, 0.6834831, 0.2222899)},
    "N": {"Z": 7, "1s": (99.1061690, 18.0523120, 4.8856602), "2sp": (3.7804559, 0.8784966, 0.2857144)},
    "O": {"Z": 8, "1s": (130.7093200, 23.8088610, 6.4436083), "2sp": (5.0331513, 1.1695961, 0.3803890)},
    # the shared STO-3G expansions scaled by Pople's standard exponents zeta(1s) = 8.65, zeta(2sp) = 2.55
    "F": {"Z": 9, "1s": (166.6791340, 30.36081233, 8.216820672), "2sp": (6.464803249, 1.502281245, 0.4885884864)},
}


# ---------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------
def _rotation(axis, angle):
    """Rotation matrix about `axis` by `angle` (Rodrigues)."""
    axis = np.asarray(axis, dtype=float)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def zmatrix_to_cartesian(zmat):
    """Z-matrix text (one atom per line: ``sym [ref dist [ref angle [ref dihedral]]]``, 1-based
    references, Angstrom / degrees) -> (symbols, coordinates [natm, 3] in Angstrom), laid out as
    PySCF does: first atom at the origin, second on +x, third rotated about z x (bond vector).
    A line of four tokens ``sym x y z`` (never a valid Z-matrix line) is a Cartesian position in
    Angstrom, as PySCF reads ``'H 0 0 0; F 0 0 1.1'``."""
    symbols, coord = [], []
    for line in zmat.replace(";", "\n").replace(",", " ").splitlines():
        tok = line.split()
        if not tok or tok[0].startswith("#"):
            continue
        symbols.append(tok[0])
        if len(tok) == 4:
            coord.append(np.array([float(t) for t in tok[1:]]))
        elif len(tok) < 3:
            coord.append(np.zeros(3))
        elif len(tok) == 3:
            coord.append(np.array([float(tok[2]), 0.0, 0.0]))
        else:
            bonda, bond = int(tok[1]) - 1, float(tok[2])
            anga, ang = int(tok[3]) - 1, float(tok[4]) / 180.0 * np.pi
            v1 = coord[anga] - coord[bonda]
            if len(tok) == 5:
                vecn = np.cross(v1, [0.0, 0.0, 1.0]) if not np.allclose(v1[:2], 0) else np.array([0.0, 0.0, 1.0])
                c = _rotation(vecn, ang) @ v1 * (bond / np.linalg.norm(v1))
            else:
                v1 = v1 / np.linalg.norm(v1)
                if ang < 1e-7:
                    c = v1 * bond
                elif np.pi - ang < 1e-7:
                    c = -v1 * bond
                else:
                    diha, dih = int(tok[5]) - 1, float(tok[6]) / 180.0 * np.pi
                    v2 = coord[diha] - coord[anga]
                    vecn = np.cross(v2, -v1)
                    norm = np.linalg.norm(vecn)
                    if norm < 1e-7:
                        vecn = (np.cross(v1, [0.0, 0.0, 1.0]) if not np.allclose(v1[:2], 0)
                                else np.array([0.0, 0.0, 1.0]))
                        c = _rotation(vecn, ang) @ v1 * bond
                    else:
                        vecn = _rotation(v1, -dih) @ vecn / norm
                        c = _rotation(vecn, ang) @ v1 * bond
            coord.append(coord[bonda] + c)
    return symbols, np.array(coord)


# ---------------------------------------------------------------------------------------------
# basis functions
# ---------------------------------------------------------------------------------------------
class _Shell:
    """One contracted Cartesian Gaussian x^l y^m z^n sum_k c_k exp(-a_k r^2) on a centre."""

    def __init__(self, center, lmn, exps, coefs):
        self.center = np.asarray(center, dtype=float)
        self.lmn = tuple(lmn)
        self.exps = np.asarray(exps, dtype=float)
        L = sum(lmn)
        prim_norm = (2 * self.exps / np.pi) ** 0.75 * (4 * self.exps) ** (L / 2.0)    # l, m, n <= 1
        self.coefs = np.asarray(coefs, dtype=float) * prim_norm
        # normalise the contraction
        a, b = self.exps[:, None], self.exps[None, :]
        s = (np.pi / (a + b)) ** 1.5 / (2 * (a + b)) ** L
        self.coefs = self.coefs / np.sqrt(self.coefs @ s @ self.coefs)


# ---- d shells (additions; nothing above or below calls them, and the device path never does) ------------------------
# ``_Shell`` normalises the radial part for a product of first powers: of the components of a d shell xy, xz, yz come
# out with norm 1 and xx, yy, zz with norm^2 = 3.  ``component_norm`` is the missing factor.
CARTESIAN_D = ((2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2))      # xx, xy, xz, yy, yz, zz
_CARTESIAN = {0: ((0, 0, 0),), 1: ((1, 0, 0), (0, 1, 0), (0, 0, 1)), 2: CARTESIAN_D}
# real solid harmonics m = -2 .. 2 (xy, yz, 3z^2 - r^2, xz, x^2 - y^2; PySCF's order and signs) in the six Cartesian
# functions, each of these normalised to 1
_SPHERICAL_D = np.array([[0.0, 1.0, 0.0, 0.0, 0.0, 0.0],
                         [0.0, 0.0, 0.0, 0.0, 1.0, 0.0],
                         [-0.5, 0.0, 0.0, -0.5, 0.0, 1.0],
                         [0.0, 0.0, 1.0, 0.0, 0.0, 0.0],
                         [0.75 ** 0.5, 0.0, 0.0, -(0.75 ** 0.5), 0.0, 0.0]])


def component_norm(lmn):
    """Factor that normalises the component x^l y^m z^n of a ``_Shell`` to 1: 1 / sqrt((2l-1)!! (2m-1)!! (2n-1)!!)."""
    f = 1.0
    for k in lmn:
        for odd in range(2 * k - 1, 1, -2):
            f *= odd
    return 1.0 / np.sqrt(f)


def normalised_shell(center, lmn, exps, coefs):
    """A ``_Shell`` whose component is normalised to 1 for every (l, m, n)."""
    sh = _Shell(center, lmn, exps, coefs)
    sh.coefs = sh.coefs * component_norm(lmn)
    return sh


def shells_from_table(table, coords_bohr):
    """Host shells of a ``GTOBasis``-style table ``[(atom, l, exponents, coefficients), ...]`` (``GTOBasis.table``) on
    the centres ``coords_bohr`` [natm, 3]: one normalised Cartesian function per component, per shell in the order
    s; x, y, z; xx, xy, xz, yy, yz, zz."""
    out = []
    for atom, l, ex, co in table:
        for lmn in _CARTESIAN[int(l)]:
            out.append(normalised_shell(coords_bohr[atom], lmn, ex, co))
    return out


def basis_transform(table, d_functions):
    """[nao, ncart]: the functions of the basis in the Cartesian functions of ``shells_from_table``.  The identity for
    ``d_functions="cartesian"``; for ``"spherical"`` every d shell becomes its 5 real solid harmonics."""
    if d_functions not in ("spherical", "cartesian"):
        raise ValueError(f"d_functions = {d_functions!r} ('spherical' or 'cartesian')")
    blocks = [_SPHERICAL_D if (int(l) == 2 and d_functions == "spherical") else np.eye(len(_CARTESIAN[int(l)]))
              for _, l, _, _ in table]
    U = np.zeros((sum(b.shape[0] for b in blocks), sum(b.shape[1] for b in blocks)))
    r = c = 0
    for b in blocks:
        U[r:r + b.shape[0], c:c + b.shape[1]] = b
        r, c = r + b.shape[0], c + b.shape[1]
    return U


def cartesian_integrals_from_table(table, charges, coords_bohr, boys=None):
    """(S, T + V, (pq|rs), nuclear repulsion) over the normalised Cartesian functions of ``shells_from_table``, on the
    host.  ``boys``: a replacement of ``_boys`` for the duration of the call (the accuracy bounds perturb it)."""
    global _boys
    keep = _boys
    if boys is not None:
        _boys = boys
    try:
        shells = shells_from_table(table, coords_bohr)
        S, T, V = one_electron_integrals(shells, charges, coords_bohr)
        g = electron_repulsion_integrals(shells)
    finally:
        _boys = keep
    nuc = sum(charges[i] * charges[j] / np.linalg.norm(coords_bohr[i] - coords_bohr[j])
              for i in range(len(charges)) for j in range(i))
    return S, T + V, g, nuc


def transform_integrals(U, S, h, g, nuc):
    """Integrals over Cartesian functions -> integrals over the functions ``U`` (``basis_transform``) stands for."""
    return U @ S @ U.T, U @ h @ U.T, np.einsum("ap,bq,cr,ds,pqrs->abcd", U, U, U, U, g, optimize=True), nuc


def integrals_from_table(table, charges, coords_bohr, d_functions="spherical", boys=None):
    """(S, T + V, (pq|rs), nuclear repulsion) of a table with s, p and d shells on the host, in the chosen form."""
    return transform_integrals(basis_transform(table, d_functions),
                               *cartesian_integrals_from_table(table, charges, coords_bohr, boys))


def cross_overlap_from_table(table, coords_a_bohr, coords_b_bohr, d_functions="spherical"):
    """``S_ab[mu, nu] = <chi_mu at R_a | chi_nu at R_b>`` [nao, nao] over the functions of ``integrals_from_table``, on
    the host: the twin of ``gto.cross_overlap_batch``.  The off-diagonal block of the overlap of the basis placed on
    both geometries at once; not symmetric."""
    A = np.asarray(coords_a_bohr, dtype=float)
    B = np.asarray(coords_b_bohr, dtype=float)
    shells = shells_from_table(table, A) + shells_from_table(table, B)
    n = len(shells) // 2
    S = one_electron_integrals(shells, (), ())[0]
    U = basis_transform(table, d_functions)
    return U @ S[:n, n:] @ U.T


def overlap_connection_from_table(table, coords_bohr, d_functions="spherical"):
    """``T[A, d, mu, nu] = <chi_mu | d chi_nu / dR_A,d>`` [natm, 3, nao, nao] over the functions of
    ``integrals_from_table``, on the host and analytic: the twin of ``gto.overlap_connection_batch`` (which contracts it
    with a matrix).  Non-zero only for ``nu`` on atom A, pairs of functions on ONE atom included.  The derivative of the
    ket with respect to its centre raises and lowers one power, ``2 b x^(j+1) - j x^(j-1)``, the contraction
    coefficients kept: every element is a combination of the overlaps of ``one_electron_integrals``.  ``T^A + T^A^T =
    dS / dR_A``."""
    R = np.asarray(coords_bohr, dtype=float)
    shells = shells_from_table(table, R)
    atoms = [int(atom) for atom, l, _, _ in table for _ in _CARTESIAN[int(l)]]
    n = len(shells)
    T = np.zeros((len(R), 3, n, n))
    for ia, A in enumerate(shells):
        for ib, B in enumerate(shells):
            a, b = A.exps[:, None], B.exps[None, :]
            Q = A.center - B.center
            cc = A.coefs[:, None] * B.coefs[None, :]
            s = [_overlap_1d(A.lmn[d], B.lmn[d], Q[d], a, b) for d in range(3)]
            for d in range(3):
                j = B.lmn[d]
                ds = 2.0 * b * _overlap_1d(A.lmn[d], j + 1, Q[d], a, b)
                if j:
                    ds = ds - j * _overlap_1d(A.lmn[d], j - 1, Q[d], a, b)
                T[atoms[ib], d, ia, ib] = np.sum(cc * ds * s[(d + 1) % 3] * s[(d + 2) % 3])
    U = basis_transform(table, d_functions)
    return U @ T @ U.T


def point_charge_integrals_from_table(table, coords_bohr, q, qxyz_bohr, d_functions="spherical", per_charge=False):
    """``V_ext[mu, nu] = - sum_k q_k <mu| 1 / |r - r_k| |nu>`` [nao, nao] over the functions of ``integrals_from_table``,
    on the host: the twin of ``gto.point_charge_integrals_batch``.  The ``V`` of ``one_electron_integrals`` with the
    charges ``q`` [M] on the centres ``qxyz_bohr`` [M, 3] in place of the nuclei (the same recursions; the charges are
    an axis of the arrays instead of a loop), followed by ``basis_transform``.  ``per_charge``: the contributions of the
    charges one by one, [M, nao, nao], instead of their sum."""
    q = np.asarray(q, dtype=float).reshape(-1)
    C = np.asarray(qxyz_bohr, dtype=float).reshape(-1, 3)
    if C.shape[0] != q.size:
        raise ValueError(f"{q.size} charges and {C.shape[0]} positions")
    shells = shells_from_table(table, np.asarray(coords_bohr, dtype=float))
    V = np.zeros((q.size if per_charge else 1, len(shells), len(shells)))
    for ia, A in enumerate(shells):
        for ib in range(ia + 1):
            pair = _Pair(A, shells[ib])
            p = pair.p[None]
            PC = [pair.P[None, ..., d] - C[:, d, None, None] for d in range(3)]            # [M, na, nb]
            Tt = p * (PC[0] ** 2 + PC[1] ** 2 + PC[2] ** 2)
            cache = {}
            term = 0.0
            for (t, u, v) in pair.tuv:
                term = term + pair.herm(t, u, v)[None] * _R(t, u, v, 0, p, PC, Tt, cache)
            x = q[:, None, None] * (pair.cc * 2.0 * np.pi / pair.p)[None] * term
            V[:, ia, ib] = V[:, ib, ia] = -(np.sum(x, axis=(1, 2)) if per_charge else np.sum(x))
    U = basis_transform(table, d_functions)
    V = U @ V @ U.T
    V = 0.5 * (V + V.transpose(0, 2, 1))               # (the products round the two halves differently)
    return V if per_charge else V[0]


def point_charge_energy(charges, coords_bohr, q, qxyz_bohr):
    """``sum_{A, k} Z_A q_k / |R_A - r_k|``: the classical energy of the nuclei in the field of the point charges (no
    charge-charge term: the self-energy of the environment is the caller's business)."""
    Z = np.asarray(charges, dtype=float).reshape(-1)
    R = np.asarray(coords_bohr, dtype=float).reshape(-1, 3)
    q = np.asarray(q, dtype=float).reshape(-1)
    C = np.asarray(qxyz_bohr, dtype=float).reshape(-1, 3)
    if R.shape[0] != Z.size or C.shape[0] != q.size:
        raise ValueError(f"{Z.size} nuclear charges for {R.shape[0]} atoms, {q.size} charges for {C.shape[0]} positions")
    d = np.linalg.norm(R[:, None, :] - C[None, :, :], axis=2)
    return float(np.sum(Z[:, None] * q[None, :] / d))


def potential_from_table(table, charges, coords_bohr, points_bohr, dm, d_functions, nuc=True, boys=None):
    """``phi[..., m] = (nuc) sum_A Z_A / |R_A - r_m| - sum_{mu nu} dm[..., mu, nu] <mu| 1 / |r - r_m| |nu>`` at the points
    ``points_bohr`` [M, 3], on the host: the twin of ``gto.potential_batch`` for one geometry.  ``dm`` is [N, N] or
    [K, N, N] over the functions of ``integrals_from_table`` and is not taken as symmetric; the operators are those of
    ``point_charge_integrals_from_table(..., per_charge=True)`` for unit charges on the points.  ``nuc``: a bool, or one
    bool per set; a point ON a nucleus then gives inf.  ``boys``: a replacement of ``_boys`` for the duration of the
    call (the accuracy bounds perturb it).  Returns [M] or [K, M] in Hartree / e; the field has no twin of its own (it is
    minus the derivative of this in the point)."""
    global _boys
    R = np.asarray(coords_bohr, dtype=float).reshape(-1, 3)
    Z = np.asarray(charges, dtype=float).reshape(-1)
    C = np.asarray(points_bohr, dtype=float).reshape(-1, 3)
    D = np.asarray(dm, dtype=float)
    if R.shape[0] != Z.size:
        raise ValueError(f"{Z.size} nuclear charges for {R.shape[0]} atoms")
    keep = _boys
    if boys is not None:
        _boys = boys
    try:
        V = point_charge_integrals_from_table(table, R, np.ones(C.shape[0]), C, d_functions, per_charge=True)
    finally:
        _boys = keep
    if D.ndim not in (2, 3) or D.shape[-2:] != V.shape[1:]:
        raise ValueError(f"dm of shape {D.shape}, expected [{V.shape[1]}, {V.shape[2]}] or [K, {V.shape[1]}, {V.shape[2]}]")
    phi = np.einsum("...pq,mpq->...m", D, V)
    flags = np.broadcast_to(np.asarray(nuc, dtype=bool), phi.shape[:-1])
    if flags.any():
        with np.errstate(divide="ignore"):
            pn = np.sum(Z[:, None] / np.linalg.norm(R[:, None, :] - C[None, :, :], axis=2), axis=0)
        phi = phi + np.where(flags[..., None], pn, 0.0) if phi.ndim > 1 else phi + pn
    return phi


# ---- basis functions, density and orbitals at points (the twins of gto.density_batch, gto.orbital_values_batch) ------------
POINT_CLAMP = 1e75             # Bohr: a coordinate of a point beyond +-POINT_CLAMP is taken as +-POINT_CLAMP (DEN_CLAMP)


def _radial_sums(shell, r2):
    """(sum_p c_p e^(-a_p r2), sum_p |c_p| e^(-a_p r2), sum_p -2 a_p c_p e^(-a_p r2), sum_p 2 a_p |c_p| e^(-a_p r2)) [M]
    of a ``_Shell``"""
    e = np.exp(-shell.exps[:, None] * r2[None, :])
    c = shell.coefs[:, None]
    a2 = 2.0 * shell.exps[:, None]
    return np.sum(c * e, axis=0), np.sum(np.abs(c) * e, axis=0), np.sum(-a2 * c * e, axis=0), np.sum(a2 * np.abs(c) * e, axis=0)


def _monomial(d, lmn):
    """x^l y^m z^n [M] at the displacements d [M, 3] (x^0 = 1 at x = 0 as everywhere)"""
    return d[:, 0] ** lmn[0] * d[:, 1] ** lmn[1] * d[:, 2] ** lmn[2]


def _monomial_derivative(d, lmn, axis):
    """d/dx_axis of ``_monomial``: l x^(l-1) y^m z^n, and 0 for l = 0"""
    if lmn[axis] == 0:
        return np.zeros(d.shape[0])
    low = list(lmn)
    low[axis] -= 1
    return lmn[axis] * _monomial(d, low)


def functions_at_points(table, coords_bohr, points_bohr, d_functions, gradient=False):
    """The functions of ``integrals_from_table`` at the points [M, 3] (Bohr), from their definition: chi [N, M] and the
    sum of the absolute values of the terms each is made of (primitives and Cartesian components), ``a`` [N, M]; with
    ``gradient`` also d chi / d r [N, M, 3] and its absolute sum.  Returns (chi, a) or (chi, a, dchi, da)."""
    R = np.asarray(coords_bohr, dtype=float).reshape(-1, 3)
    P = np.clip(np.asarray(points_bohr, dtype=float).reshape(-1, 3), -POINT_CLAMP, POINT_CLAMP)
    shells = shells_from_table(table, R)
    M = P.shape[0]
    chi, a = np.zeros((len(shells), M)), np.zeros((len(shells), M))
    dchi, da = np.zeros((len(shells), M, 3)), np.zeros((len(shells), M, 3))
    for i, sh in enumerate(shells):
        d = P - sh.center[None, :]
        r0, r0abs, r1, r1abs = _radial_sums(sh, np.sum(d * d, axis=1))
        poly = _monomial(d, sh.lmn)
        chi[i], a[i] = poly * r0, np.abs(poly) * r0abs
        if gradient:
            for ax in range(3):
                low = _monomial_derivative(d, sh.lmn, ax)
                dchi[i, :, ax] = low * r0 + d[:, ax] * poly * r1
                da[i, :, ax] = np.abs(low) * r0abs + np.abs(d[:, ax] * poly) * r1abs
    U = basis_transform(table, d_functions)
    if not gradient:
        return U @ chi, np.abs(U) @ a
    return U @ chi, np.abs(U) @ a, np.einsum("pc,cmx->pmx", U, dchi), np.einsum("pc,cmx->pmx", np.abs(U), da)


def density_from_table(table, coords_bohr, points_bohr, dm, d_functions, gradient=False):
    """``rho[..., m] = sum_{mu nu} dm[..., mu, nu] chi_mu(r_m) chi_nu(r_m)`` at the points ``points_bohr`` [M, 3], on the
    host and from the definition: the twin of ``gto.density_batch`` for one geometry.  ``dm`` is [N, N] or [K, N, N] over
    the functions of ``integrals_from_table`` and is not taken as symmetric.  Returns ``(rho, A)``, each [M] or [K, M] in
    e / Bohr^3, ``A`` the sum of the absolute values of all the terms of the value (the scale of its rounding error); with
    ``gradient`` ``(rho, drho, A, dA)``, ``drho`` [..., M, 3] = d rho / d r_m in e / Bohr^4."""
    D = np.asarray(dm, dtype=float)
    f = functions_at_points(table, coords_bohr, points_bohr, d_functions, gradient)
    N = f[0].shape[0]
    if D.ndim not in (2, 3) or D.shape[-2:] != (N, N):
        raise ValueError(f"dm of shape {D.shape}, expected [{N}, {N}] or [K, {N}, {N}]")
    rho = np.einsum("...pq,pm,qm->...m", D, f[0], f[0], optimize=True)
    A = np.einsum("...pq,pm,qm->...m", np.abs(D), f[1], f[1], optimize=True)
    if not gradient:
        return rho, A
    drho = (np.einsum("...pq,pmx,qm->...mx", D, f[2], f[0], optimize=True)
            + np.einsum("...pq,pm,qmx->...mx", D, f[0], f[2], optimize=True))
    dA = (np.einsum("...pq,pmx,qm->...mx", np.abs(D), f[3], f[1], optimize=True)
          + np.einsum("...pq,pm,qmx->...mx", np.abs(D), f[1], f[3], optimize=True))
    return rho, drho, A, dA


def orbital_values_from_table(table, coords_bohr, points_bohr, C, d_functions, gradient=False):
    """``psi[i, m] = sum_mu C[mu, i] chi_mu(r_m)`` at the points ``points_bohr`` [M, 3] for the columns of ``C``
    [N, ncol], on the host: the twin of ``gto.orbital_values_batch`` for one geometry.  Returns ``(psi [ncol, M], A)`` in
    Bohr^-3/2, ``A`` as for ``density_from_table``; with ``gradient`` ``(psi, dpsi [ncol, M, 3], A, dA)``."""
    C = np.asarray(C, dtype=float)
    f = functions_at_points(table, coords_bohr, points_bohr, d_functions, gradient)
    if C.ndim != 2 or C.shape[0] != f[0].shape[0]:
        raise ValueError(f"C of shape {C.shape}, expected [{f[0].shape[0]}, ncol]")
    psi, A = C.T @ f[0], np.abs(C).T @ f[1]
    if not gradient:
        return psi, A
    return psi, np.einsum("pi,pmx->imx", C, f[2]), A, np.einsum("pi,pmx->imx", np.abs(C), f[3])


# powers of (x - Ox, y - Oy, z - Oz) in the components of the moment integrals: x, y, z | xx, xy, xz, yy, yz, zz
MOMENT_COMPONENTS = ((1, 0, 0), (0, 1, 0), (0, 0, 1)) + CARTESIAN_D


def moment_integrals_from_table(table, coords_bohr, d_functions="spherical", order=1, origin=None):
    """``M[c, mu, nu] = <mu| (x - Ox)^ex (y - Oy)^ey (z - Oz)^ez |nu>`` [3 or 9, nao, nao] (``MOMENT_COMPONENTS``) over
    the functions of ``integrals_from_table``, on the host: the twin of ``gto.moment_integrals_batch``.  Per dimension
    ``sum_t E_t M^e_t`` with ``M^0 = (s)``, ``M^1 = (X s, s)``, ``M^2 = ((X^2 + 1/2p) s, 2 X s, 2 s)``, ``s = sqrt(pi /
    p)``, ``X = P - O``.  ``origin`` [3] in Bohr (default 0)."""
    if order not in (1, 2):
        raise ValueError(f"order = {order!r} (1 or 2)")
    O = np.zeros(3) if origin is None else np.asarray(origin, dtype=float).reshape(3)
    shells = shells_from_table(table, np.asarray(coords_bohr, dtype=float))
    comps = MOMENT_COMPONENTS[:3 if order == 1 else 9]
    M = np.zeros((len(comps), len(shells), len(shells)))
    for ia, A in enumerate(shells):
        for ib in range(ia + 1):
            B = shells[ib]
            a, b = A.exps[:, None], B.exps[None, :]
            p, Q = a + b, A.center - B.center
            m = []
            for d in range(3):
                X = (a * A.center[d] + b * B.center[d]) / p - O[d]
                e0, e1, e2 = (_E(A.lmn[d], B.lmn[d], t, Q[d], a, b) for t in range(3))
                m.append([e0, X * e0 + e1, (X * X + 0.5 / p) * e0 + 2 * X * e1 + 2 * e2])
            cc = A.coefs[:, None] * B.coefs[None, :] * (np.pi / p) ** 1.5
            for c, (ex, ey, ez) in enumerate(comps):
                M[c, ia, ib] = M[c, ib, ia] = np.sum(cc * m[0][ex] * m[1][ey] * m[2][ez])
    U = basis_transform(table, d_functions)
    M = U @ M @ U.T
    return 0.5 * (M + M.transpose(0, 2, 1))          # (the products round the two halves differently)


def sto3g_basis(symbols, coords_bohr):
    shells = []
    for sym, R in zip(symbols, coords_bohr):
        key = sym.capitalize()
        if key not in _STO3G:
            raise ValueError(f"no STO-3G parameters for element {sym!r} (H, C, N, O are built in)")
        par = _STO3G[key]
        shells.append(_Shell(R, (0, 0, 0), par["1s"], _STO3G_1S_COEF))
        if "2sp" in par:
            shells.append(_Shell(R, (0, 0, 0), par["2sp"], _STO3G_2S_COEF))
            for lmn in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
                shells.append(_Shell(R, lmn, par["2sp"], _STO3G_2P_COEF))
    return shells


# ---------------------------------------------------------------------------------------------
# McMurchie-Davidson machinery (arrays broadcast over primitives)
# ---------------------------------------------------------------------------------------------
def _E(i, j, t, Q, a, b):
    """Hermite expansion coefficient E_t^{ij} of the product of two 1-D Gaussians, Q = A - B."""
    p = a + b
    mu = a * b / p
    if t < 0 or t > i + j:
        return np.zeros(np.broadcast(Q, a, b).shape)
    if i == j == t == 0:
        return np.exp(-mu * Q * Q) * np.ones(np.broadcast(Q, a, b).shape)
    if j == 0:
        return (_E(i - 1, j, t - 1, Q, a, b) / (2 * p) - (mu * Q / a) * _E(i - 1, j, t, Q, a, b)
                + (t + 1) * _E(i - 1, j, t + 1, Q, a, b))
    return (_E(i, j - 1, t - 1, Q, a, b) / (2 * p) + (mu * Q / b) * _E(i, j - 1, t, Q, a, b)
            + (t + 1) * _E(i, j - 1, t + 1, Q, a, b))


def _boys(n, x):
    return hyp1f1(n + 0.5, n + 1.5, -x) / (2.0 * n + 1.0)


def _R(t, u, v, n, p, PC, T, cache):
    """Hermite Coulomb integral R^n_{tuv}(p, P - C), T = p |PC|^2."""
    key = (t, u, v, n)
    if key in cache:
        return cache[key]
    if t < 0 or u < 0 or v < 0:
        val = 0.0
    elif t == u == v == 0:
        val = (-2.0 * p) ** n * _boys(n, T)
    elif t == u == 0:
        val = PC[2] * _R(t, u, v - 1, n + 1, p, PC, T, cache)
        if v > 1:
            val = val + (v - 1) * _R(t, u, v - 2, n + 1, p, PC, T, cache)
    elif t == 0:
        val = PC[1] * _R(t, u - 1, v, n + 1, p, PC, T, cache)
        if u > 1:
            val = val + (u - 1) * _R(t, u - 2, v, n + 1, p, PC, T, cache)
    else:
        val = PC[0] * _R(t - 1, u, v, n + 1, p, PC, T, cache)
        if t > 1:
            val = val + (t - 1) * _R(t - 2, u, v, n + 1, p, PC, T, cache)
    cache[key] = val
    return val


class _Pair:
    """Primitive-pair data of two shells: exponent sums, product centres, Hermite coefficients."""

    def __init__(self, A, B):
        a, b = A.exps[:, None], B.exps[None, :]
        self.p = a + b
        self.P = (a[..., None] * A.center + b[..., None] * B.center) / self.p[..., None]   # [na, nb, 3]
        self.cc = A.coefs[:, None] * B.coefs[None, :]
        Q = A.center - B.center
        self.E = []          # per dimension: list over t of arrays [na, nb]
        for d in range(3):
            i, j = A.lmn[d], B.lmn[d]
            self.E.append([_E(i, j, t, Q[d], a, b) for t in range(i + j + 1)])
        self.tuv = [(t, u, v) for t in range(len(self.E[0])) for u in range(len(self.E[1]))
                    for v in range(len(self.E[2]))]

    def herm(self, t, u, v):
        return self.E[0][t] * self.E[1][u] * self.E[2][v]


def _overlap_1d(i, j, Q, a, b):
    return _E(i, j, 0, Q, a, b) * np.sqrt(np.pi / (a + b))


def one_electron_integrals(shells, charges, centers):
    """-> (S, T, V): overlap, kinetic energy, nuclear attraction, [nao, nao]."""
    n = len(shells)
    S, T, V = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
    for ia, A in enumerate(shells):
        for ib in range(ia + 1):
            B = shells[ib]
            a, b = A.exps[:, None], B.exps[None, :]
            cc = A.coefs[:, None] * B.coefs[None, :]
            Q = A.center - B.center
            s1 = [_overlap_1d(A.lmn[d], B.lmn[d], Q[d], a, b) for d in range(3)]
            S[ia, ib] = S[ib, ia] = np.sum(cc * s1[0] * s1[1] * s1[2])
            kin = 0.0
            for d in range(3):
                i, j = A.lmn[d], B.lmn[d]
                td = -2.0 * b * b * _overlap_1d(i, j + 2, Q[d], a, b) + b * (2 * j + 1) * s1[d]
                if j >= 2:
                    td = td - 0.5 * j * (j - 1) * _overlap_1d(i, j - 2, Q[d], a, b)
                others = [s1[e] for e in range(3) if e != d]
                kin = kin + td * others[0] * others[1]
            T[ia, ib] = T[ib, ia] = np.sum(cc * kin)
            pair = _Pair(A, B)
            acc = 0.0
            for Z, C in zip(charges, centers):
                PC = [pair.P[..., d] - C[d] for d in range(3)]
                Tt = pair.p * (PC[0] ** 2 + PC[1] ** 2 + PC[2] ** 2)
                cache = {}
                term = 0.0
                for (t, u, v) in pair.tuv:
                    term = term + pair.herm(t, u, v) * _R(t, u, v, 0, pair.p, PC, Tt, cache)
                acc = acc - Z * np.sum(pair.cc * term * 2.0 * np.pi / pair.p)
            V[ia, ib] = V[ib, ia] = acc
    return S, T, V


def electron_repulsion_integrals(shells):
    """(pq|rs) in chemist order, [nao]*4, 8-fold symmetry filled in exactly (bit-for-bit)."""
    n = len(shells)
    pairs = {(i, j): _Pair(shells[i], shells[j]) for i in range(n) for j in range(i + 1)}
    g = np.zeros((n, n, n, n))
    idx = [(i, j) for i in range(n) for j in range(i + 1)]
    for k1, (i, j) in enumerate(idx):
        ab = pairs[(i, j)]
        p = ab.p[:, :, None, None]
        for (k, l) in idx[:k1 + 1]:
            cd = pairs[(k, l)]
            q = cd.p[None, None, :, :]
            alpha = p * q / (p + q)
            PQ = [ab.P[:, :, None, None, d] - cd.P[None, None, :, :, d] for d in range(3)]
            Tt = alpha * (PQ[0] ** 2 + PQ[1] ** 2 + PQ[2] ** 2)
            cache = {}
            val = 0.0
            for (t, u, v) in ab.tuv:
                e1 = ab.herm(t, u, v)[:, :, None, None]
                for (tt, uu, vv) in cd.tuv:
                    e2 = cd.herm(tt, uu, vv)[None, None, :, :]
                    sign = -1.0 if (tt + uu + vv) % 2 else 1.0
                    val = val + sign * e1 * e2 * _R(t + tt, u + uu, v + vv, 0, alpha, PQ, Tt, cache)
            val = val * 2.0 * np.pi ** 2.5 / (p * q * np.sqrt(p + q))
            x = np.sum(ab.cc[:, :, None, None] * cd.cc[None, None, :, :] * val)
            for (a_, b_, c_, d_) in set(itertools.chain(
                    [(i, j, k, l), (j, i, k, l), (i, j, l, k), (j, i, l, k),
                     (k, l, i, j), (l, k, i, j), (k, l, j, i), (l, k, j, i)])):
                g[a_, b_, c_, d_] = x
    return g


# ---------------------------------------------------------------------------------------------
# molecule
# ---------------------------------------------------------------------------------------------
def rhf(int1e, int2e, overlap, n_occ, conv_tol=1e-12, max_cycle=200):
    """Restricted Hartree-Fock with DIIS from the core-Hamiltonian guess.
    -> (mo_coeff [nao, nao], mo_energy, electronic energy)."""
    s_val, s_vec = np.linalg.eigh(overlap)
    X = s_vec @ np.diag(s_val ** -0.5) @ s_vec.T

    def diag(F):
        e, c = np.linalg.eigh(X.T @ F @ X)
        return e, X @ c
    e, C = diag(int1e)
    D = 2.0 * C[:, :n_occ] @ C[:, :n_occ].T
    fs, errs = [], []
    energy = 0.0
    for _ in range(max_cycle):
        J = np.einsum("pqrs,rs->pq", int2e, D)
        K = np.einsum("prqs,rs->pq", int2e, D)
        F = int1e + J - 0.5 * K
        new_energy = 0.5 * np.sum(D * (int1e + F))
        err = F @ D @ overlap - overlap @ D @ F
        fs.append(F)
        errs.append(err)
        fs, errs = fs[-8:], errs[-8:]
        if len(fs) > 1:
            m = len(fs)
            B = -np.ones((m + 1, m + 1))
            B[m, m] = 0.0
            for a_ in range(m):
                for b_ in range(m):
                    B[a_, b_] = np.sum(errs[a_] * errs[b_])
            rhs = np.zeros(m + 1)
            rhs[m] = -1.0
            try:
                w = np.linalg.solve(B, rhs)[:m]
                F = sum(wi * fi for wi, fi in zip(w, fs))
            except np.linalg.LinAlgError:
                pass
        e, C = diag(F)
        D = 2.0 * C[:, :n_occ] @ C[:, :n_occ].T
        if abs(new_energy - energy) < conv_tol and np.abs(err).max() < 1e-9:
            energy = new_energy
            break
        energy = new_energy
    return C, e, energy


class Moldata_sto3g(Moldata):
    """Stand-in for ``Moldata_pyscf(geometry, 'sto-3g')`` (src/auto_oo/moldata_pyscf.py:19-61) for
    molecules of H, C, N, O, F: same attributes (``int1e_ao, int2e_ao, overlap, oao_coeff, nuc, nao``),
    ``run_rhf()`` -> ``hf.mo_coeff`` / ``hf.e_tot``.  ``geometry`` is a Z-matrix string (as
    ``get_formal_geo`` returns), a Cartesian string ``'H 0 0 0; F 0 0 1.1'`` or a list of
    ``(symbol, (x, y, z))`` in Angstrom."""

    def __init__(self, geometry, basis="sto-3g", charge=0):
        if str(basis).lower().replace("-", "") != "sto3g":
            raise ValueError("Moldata_sto3g only builds STO-3G integrals; import others with Moldata.from_npz")
        if isinstance(geometry, str):
            symbols, xyz = zmatrix_to_cartesian(geometry)
        else:
            symbols = [a[0] for a in geometry]
            xyz = np.array([a[1] for a in geometry], dtype=float)
        self.symbols = symbols
        self.coordinates = xyz
        R = xyz / BOHR
        charges = [_STO3G[s.capitalize()]["Z"] for s in symbols]
        shells = sto3g_basis(symbols, R)
        S, T, V = one_electron_integrals(shells, charges, R)
        g = electron_repulsion_integrals(shells)
        nuc = sum(charges[i] * charges[j] / np.linalg.norm(R[i] - R[j])
                  for i in range(len(charges)) for j in range(i))
        super().__init__(T + V, g, S, nuc, sum(charges) - charge)

    def run_rhf(self, verbose=0, device=False):
        """moldata_pyscf.py:58-61: the host ``rhf`` above; ``device=True`` takes the orbitals from the device solver
        (``scf.rhf_batch``) instead."""
        if device:
            return Moldata.run_rhf(self, verbose, device=True)
        if self.hf is None:
            C, e, e_elec = rhf(self.int1e_ao, self.int2e_ao, self.overlap, self.nelectron // 2)
            self.hf = SimpleNamespace(mo_coeff=C, mo_energy=e, e_tot=e_elec + self.nuc)
