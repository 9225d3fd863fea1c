"""Independent numpy reference of the overlap tests (tests/test_overlaps_cpu.py, tests/test_overlaps_gpu.py).

``brute_force``: the overlap of two determinant expansions over non-orthogonal orbitals from its definition -- for every
pair of determinants the determinant of the WHOLE occupied block (core + active occupied) of ``s`` per spin, with the
alpha-before-beta signs of ``berry.sector_tables``.  ``core_fold``: the same quantity through det(s_cc) and the Schur
complement.  The disagreement of the two host forms is the yardstick of the exact-metric bounds of the GPU tests.

``exact_reference``: the contract of the sector kernel in 40-digit mpmath arithmetic; ``SCOPE_CASES`` / ``scope_inputs``
/ ``make_scope_case``: the cases recorded as tests/golden/overlap_scope_*.npz by tests/golden/make_overlap_scope.py, and
``scope_bound`` the bound of a comparison with one (tests/test_overlap_scope_gpu.py).  ``run_overlap_host``: the
kernel's determinant and sign routines run on the CPU (tools/overlap_host.hip).
"""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from auto_oo_amd import gaussian
from auto_oo_amd.berry import ActiveSpaceRotation, _occupied, sector_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOHR = gaussian.BOHR
H2_XYZ = np.array([[0.0, 0.02, -0.37], [0.03, -0.01, 0.39]])                   # Angstrom
H2_XYZ_2 = np.array([[0.01, 0.02, -0.40], [0.03, 0.02, 0.41]])
H2_TABLE = {"H": [("s", [3.42525091, 0.62391373, 0.16885540], [0.15432897, 0.53532814, 0.44463454]),
                  ("s", [0.35], [1.0])]}


def _whole_minors(s, n_core, ncas, strings):
    """M[J, I] = det s[core + occ(J), core + occ(I)]: the whole occupied block of one spin."""
    core = list(range(n_core))
    occ = [core + [n_core + p for p in _occupied(m, ncas)] for m in strings]
    M = np.empty((len(occ), len(occ)))
    for j, oj in enumerate(occ):
        for i, oi in enumerate(occ):
            M[j, i] = np.linalg.det(s[np.ix_(oj, oi)]) if oj else 1.0
    return M


def contract(Ma, Mb, sign, bra, ket, signed):
    na, nb = Ma.shape[0], Mb.shape[0]
    bra = np.asarray(bra, dtype=float).reshape(-1, na, nb)
    ket = np.asarray(ket, dtype=float).reshape(-1, na, nb)
    if signed:
        bra, ket = bra * sign, ket * sign
    return np.einsum("iJK,JI,KL,jIL->ij", bra, Ma, Mb, ket, optimize=True)


def brute_force(s, n_core, ncas, n_alpha, n_beta, bra, ket, signed=True):
    """out[i, j] = <bra_i|ket_j>, all electrons, from whole-block determinants.  bra [Rb, na nb], ket [Rk, na nb]."""
    s = np.asarray(s, dtype=float)
    ua, ub, _, sign = sector_tables(ncas, n_alpha, n_beta)
    return contract(_whole_minors(s, n_core, ncas, ua), _whole_minors(s, n_core, ncas, ub), sign, bra, ket, signed)


def core_fold(s, n_core, ncas, n_alpha, n_beta, bra, ket, signed=True):
    """The same through the core fold: (out over U = s_aa - s_ac s_cc^-1 s_ca, det(s_cc)); the all-electron overlap is
    det(s_cc)^2 out."""
    s = np.asarray(s, dtype=float)
    c = n_core
    if c:
        U = s[c:, c:] - s[c:, :c] @ np.linalg.solve(s[:c, :c], s[:c, c:])
        det = np.linalg.det(s[:c, :c])
    else:
        U, det = s, 1.0
    ua, ub, _, sign = sector_tables(ncas, n_alpha, n_beta)
    return contract(_whole_minors(U, 0, ncas, ua), _whole_minors(U, 0, ncas, ub), sign, bra, ket, signed), det


def host_route(U, ncas, n_alpha, n_beta, bra, ket, orthogonalize=False, signed=True):
    """The host route of berry.py: ``ActiveSpaceRotation(U, ...)``'s M_alpha, M_beta and numpy."""
    rot = ActiveSpaceRotation(U, ncas, n_alpha, n_beta, orthogonalize=orthogonalize)
    return contract(rot.M_alpha, rot.M_beta, rot.sign, bra, ket, signed)


def host_s(basis, xyz_a, xyz_b, mo_a, mo_b, M):
    """s = C_a[:, :M]^T S_ab C_b[:, :M] from the host cross overlap (geometries in Angstrom)."""
    S_ab = gaussian.cross_overlap_from_table(basis.table, np.asarray(xyz_a) / BOHR, np.asarray(xyz_b) / BOHR,
                                             basis.d_functions or "spherical")
    return np.asarray(mo_a)[:, :M].T @ S_ab @ np.asarray(mo_b)[:, :M]


def random_orthogonal(n, rng, improper=False):
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    q = q * np.sign(np.diag(r))
    if (np.linalg.det(q) < 0) != improper:
        q[:, 0] = -q[:, 0]
    return q


def trial_matrices(ncas, seed):
    """{name: U}: generic orthogonal, improper (det = -1), non-orthogonal, and a permutation matrix whose leading
    minors vanish."""
    rng = np.random.default_rng(seed)
    perm = np.eye(ncas)[:, np.roll(np.arange(ncas), 1)]
    return {"orthogonal": random_orthogonal(ncas, rng), "improper": random_orthogonal(ncas, rng, True),
            "nonorthogonal": np.eye(ncas) + 0.3 * rng.standard_normal((ncas, ncas)), "permutation": perm}


# ---- the bodies of the cross-overlap kernels as a host program ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cross_host_program():
    """tools/gto_cross_host.hip compiled for the host alone (no device code, no HIP runtime call), once per session."""
    tmp = tempfile.mkdtemp(prefix="gto_cross_host_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    out = os.path.join(tmp, "gto_cross_host")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--cuda-host-only", "-O2", "-std=c++17", "-Wno-unused-function",
                    "-I", os.path.join(ROOT, "auto_oo_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "gto_cross_host.hip"), "-o", out], check=True)
    return out


def run_cross_bodies(basis, xyz_a, xyz_b):
    """S_ab [P, N, N] of the pairs (xyz_a[p], xyz_b[p]) (Angstrom) from the kernel bodies run on the CPU.  An element no
    body writes comes back NaN."""
    xa, xb = np.asarray(xyz_a, dtype=float) / BOHR, np.asarray(xyz_b, dtype=float) / BOHR
    P = xa.shape[0]
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.txt"), os.path.join(tmp, "out.txt")
        with open(fin, "w") as fh:
            fh.write(f"{basis.nshell} {basis.natm} {P} {basis.nao} {basis.exps.size}\n")
            fh.write(" ".join(str(int(v)) for v in basis.shells.ravel()) + "\n")
            for arr in (basis.exps, basis.coefs, xa, xb):
                fh.write(" ".join(repr(float(v)) for v in np.asarray(arr).ravel()) + "\n")
        subprocess.run([cross_host_program(), fin, fout], check=True)
        vals = np.loadtxt(fout)
    return vals.reshape(P, basis.nao, basis.nao)


# ---- the determinant and sign routines of the sector kernel as a host program -----------------------------------------
@functools.lru_cache(maxsize=None)
def overlap_host_program():
    """tools/overlap_host.hip compiled for the host alone (no device code, no HIP runtime call), once per session."""
    tmp = tempfile.mkdtemp(prefix="overlap_host_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    out = os.path.join(tmp, "overlap_host")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--cuda-host-only", "-O2", "-std=c++17", "-Wno-unused-function",
                    "-I", os.path.join(ROOT, "auto_oo_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "overlap_host.hip"), "-o", out], check=True)
    return out


def run_overlap_host(records):
    """records: (ncas, K, U [ncas, ncas], list1, list2).  Per record (minors [n1, n2] or None when K = -1, signs [n1, n2])
    from ``ovl_minor<K>`` (through the kernel's switch) and ``ovl_sign`` run on the CPU."""
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.txt"), os.path.join(tmp, "out.txt")
        with open(fin, "w") as fh:
            for ncas, K, U, l1, l2 in records:
                fh.write(f"{ncas} {K} {len(l1)} {len(l2)}\n")
                fh.write(" ".join(repr(float(v)) for v in np.asarray(U, dtype=float).reshape(ncas * ncas)) + "\n")
                fh.write(" ".join(str(int(v)) for v in l1) + "\n" + " ".join(str(int(v)) for v in l2) + "\n")
        subprocess.run([overlap_host_program(), fin, fout], check=True)
        vals = np.loadtxt(fout, ndmin=1)
    out, at = [], 0
    for ncas, K, U, l1, l2 in records:
        n = len(l1) * len(l2)
        minors = None
        if K >= 0:
            minors, at = vals[at:at + n].reshape(len(l1), len(l2)), at + n
        out.append((minors, vals[at:at + n].reshape(len(l1), len(l2))))
        at += n
    assert at == vals.size
    return out


# ---- matrices for the pivoting of ovl_minor ---------------------------------------------------------------------------
def hadamard8():
    """8 x 8 Hadamard matrix / sqrt(8) (orthogonal): every pivot search of every minor ties."""
    h = np.array([[1.0]])
    for _ in range(3):
        h = np.block([[h, h], [h, -h]])
    return h / np.sqrt(8.0)


def pivot_matrices(ncas=8, seed=808):
    """{name: U}: ``hadamard`` (ncas = 8), ``zero_column`` / ``zero_row`` (column / row 2 of a generic matrix vanishes: the
    minors through it are exactly 0), ``exchange`` (the largest element of every column of the whole matrix sits one row
    below the diagonal, cyclically: a row exchange at every column)."""
    rng = np.random.default_rng(seed)
    g = np.eye(ncas) + 0.3 * rng.standard_normal((ncas, ncas))
    zc, zr = g.copy(), g.T.copy()
    zc[:, 2 % ncas] = 0.0
    zr[2 % ncas, :] = 0.0
    ex = np.roll(np.eye(ncas), 1, axis=0) + 0.1 * rng.standard_normal((ncas, ncas))
    out = {"zero_column": zc, "zero_row": zr, "exchange": ex}
    if ncas == 8:
        out["hadamard"] = hadamard8()
    return out


# ---- the 40-digit reference of the sector kernel's contract -----------------------------------------------------------
DPS = 40


def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


def exact_U(s, n_core, ncas, mode):
    """(U as an mpmath matrix, core_det as mpf): det(s_cc), U = s_aa - s_ac s_cc^-1 s_ca, in mode 1 its Q factor with a
    positive diagonal of R (Gram-Schmidt with a second pass, 40 digits)."""
    mp = _mp()
    S = mp.matrix(np.asarray(s, dtype=float).tolist())
    c, m = n_core, n_core + ncas
    if c:
        U = S[c:m, c:m] - S[c:m, 0:c] * (mp.inverse(S[0:c, 0:c]) * S[0:c, c:m])
        det = mp.det(S[0:c, 0:c])
    else:
        U, det = S, mp.mpf(1)
    if mode == 1:
        Q = U.copy()
        for k in range(ncas):
            for _ in range(2):
                for j in range(k):
                    r = mp.fsum(Q[i, j] * Q[i, k] for i in range(ncas))
                    for i in range(ncas):
                        Q[i, k] -= r * Q[i, j]
            nrm = mp.sqrt(mp.fsum(Q[i, k] ** 2 for i in range(ncas)))
            for i in range(ncas):
                Q[i, k] /= nrm
        U = Q
    return U, det


def exact_det(rows):
    """mpmath.det of a square matrix given as rows (mpf or float), 40 digits.  An exactly zero pivot column makes the LU
    of mpmath 1.3.0 raise TypeError instead of reporting a singular matrix: the determinant is 0."""
    mp = _mp()
    try:
        return mp.det(mp.matrix(rows))
    except TypeError:
        return mp.mpf(0)


def _exact_minors(U, strings, ncas):
    """M[J][I] = det U[occ(J), occ(I)] by mpmath.det (lists of mpf)."""
    mp = _mp()
    occ = [_occupied(m, ncas) for m in strings]
    out = []
    for oj in occ:
        row = []
        for oi in occ:
            if not oj:
                row.append(mp.mpf(1))
            else:
                row.append(exact_det([[U[a, b] for b in oi] for a in oj]))
        out.append(row)
    return out


def exact_reference(s, n_core, ncas, n_alpha, n_beta, bra, ket, index=None, mode=0, signed=True):
    """The kernel's contract in 40-digit arithmetic, rounded to float64 once at the end: (out [Rb, Rk], core_det, U as
    float64).  bra [Rb, L], ket [Rk, L]; with ``index`` element (ia, ib) is read at index[ia nb + ib], zero outside
    0 .. L - 1."""
    mp = _mp()
    U, det = exact_U(s, n_core, ncas, mode)
    ua, ub, _, sign = sector_tables(ncas, n_alpha, n_beta)
    na, nb = len(ua), len(ub)
    Ma = _exact_minors(U, ua, ncas)
    Mb = Ma if n_alpha == n_beta else _exact_minors(U, ub, ncas)

    def gather(v):
        v = np.asarray(v, dtype=float)
        idx = np.arange(na * nb) if index is None else np.asarray(index).reshape(-1)
        w = [mp.mpf(float(v[x])) if 0 <= x < v.size else mp.mpf(0) for x in idx]
        if signed:
            w = [-x if sg < 0 else x for x, sg in zip(w, sign.reshape(-1))]
        return [w[i * nb:(i + 1) * nb] for i in range(na)]

    bras = [gather(v) for v in np.atleast_2d(bra)]
    out = np.empty((len(bras), len(np.atleast_2d(ket))))
    for j, kv in enumerate(np.atleast_2d(ket)):
        K = gather(kv)
        # T[Ja][Ib] = sum_Ia Ma[Ja][Ia] K[Ia][Ib];  W[Ja][Jb] = sum_Ib T[Ja][Ib] Mb[Jb][Ib]
        Kt = [[K[ia][ib] for ia in range(na)] for ib in range(nb)]
        T = [[mp.fdot(Ma[ja], Kt[ib]) for ib in range(nb)] for ja in range(na)]
        W = [[mp.fdot(T[ja], Mb[jb]) for jb in range(nb)] for ja in range(na)]
        for i, B in enumerate(bras):
            out[i, j] = float(mp.fsum(mp.fdot(B[ja], W[ja]) for ja in range(na)))
    Uf = np.array([[float(U[i, k]) for k in range(ncas)] for i in range(ncas)])
    return out, float(det), Uf


def host_reference(s, n_core, ncas, n_alpha, n_beta, bra, ket, index=None, mode=0, signed=True):
    """The float64 host route on the same inputs: ``core_fold`` (mode 0), or its U through ``berry.givens_orthogonal``
    and ``host_route`` (mode 1).  (out [Rb, Rk], core_det)."""
    s = np.asarray(s, dtype=float)
    bra, ket = np.atleast_2d(np.asarray(bra, dtype=float)), np.atleast_2d(np.asarray(ket, dtype=float))
    if index is not None:
        idx = np.asarray(index).reshape(-1)
        ok = (idx >= 0) & (idx < bra.shape[1])
        take = lambda v: np.where(ok, v[:, np.where(ok, idx, 0)], 0.0)               # noqa: E731
        bra, ket = take(bra), take(ket)
    c = n_core
    if mode == 0:
        return core_fold(s, c, ncas, n_alpha, n_beta, bra, ket, signed)
    if c:
        U = s[c:, c:] - s[c:, :c] @ np.linalg.solve(s[:c, :c], s[:c, c:])
        det = np.linalg.det(s[:c, :c])
    else:
        U, det = s, 1.0
    return host_route(U, ncas, n_alpha, n_beta, bra, ket, "givens", signed), det


# ---- the fixture cases of tests/test_overlap_scope_gpu.py (tests/golden/overlap_scope_*.npz) --------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generic_s(m, n_core, rng):
    """1 + (0.5 / sqrt(m)) randn, core rows 0 and n_core - 1 exchanged: the first pivot search must swap."""
    s = np.eye(m) + 0.5 / np.sqrt(m) * rng.standard_normal((m, m))
    if n_core > 1:
        s[[0, n_core - 1]] = s[[n_core - 1, 0]]
    return s


def _with_cond(n, cond, rng):
    """A matrix of the given 2-norm condition number and |det| = 1: seeded orthogonal factors, singular values
    sqrt(cond) .. 1 / sqrt(cond) spaced evenly in the logarithm."""
    u, v = random_orthogonal(n, rng), random_orthogonal(n, rng)
    h = 0.5 * np.log10(cond)
    return (u * np.logspace(h, -h, n)) @ v.T


def _signed_permutation_core(n, rng):
    """Row r has its one element (+-1) in column r + 1 (cyclically): a zero leading element at every step."""
    return np.roll(np.eye(n), 1, axis=1) * rng.choice([-1.0, 1.0], size=(n, 1))


# name: (ncas, n_alpha, n_beta, n_core, mode, P, rb, rk, recipe)
SCOPE_CASES = {
    "c5_32_core0": (5, 3, 2, 0, 0, 2, 2, 3, "generic"),
    "c5_05_core3": (5, 0, 5, 3, 0, 2, 2, 3, "generic"),
    "c7_43_core6": (7, 4, 3, 6, 0, 1, 2, 3, "generic"),
    "c7_76_core2": (7, 7, 6, 2, 0, 2, 2, 3, "generic"),
    "c8_87_core5": (8, 8, 7, 5, 0, 2, 2, 3, "generic"),
    "c6_51_core17": (6, 5, 1, 17, 0, 2, 2, 3, "generic"),
    "c1_10_core47": (1, 1, 0, 47, 0, 2, 2, 3, "generic"),
    "c8_43_core40": (8, 4, 3, 40, 0, 1, 1, 1, "generic"),
    "c8_34_core40": (8, 3, 4, 40, 0, 1, 1, 1, "mirror:c8_43_core40"),
    "c4_21_perm6": (4, 2, 1, 6, 0, 2, 2, 3, "permutation"),
    "c4_32_cond3": (4, 3, 2, 12, 0, 2, 2, 3, "cond:1e3"),
    "c4_32_cond6": (4, 3, 2, 12, 0, 2, 2, 3, "cond:1e6"),
    "c6_42_q2": (6, 4, 2, 0, 1, 2, 2, 3, "ucond:1e2"),
    "c6_42_q5": (6, 4, 2, 0, 1, 2, 2, 3, "ucond:1e5"),
    "c5_23_roots": (5, 2, 3, 4, 0, 1, 4, 4, "generic"),
}
for _sec, (_na, _nb) in (("53", (5, 3)), ("62", (6, 2)), ("88", (8, 8))):
    for _kind in ("hadamard", "zero_column", "zero_row", "exchange"):
        SCOPE_CASES[f"c8_{_sec}_{_kind}"] = (8, _na, _nb, 0, 0, 1, 1, 2, "pivot:" + _kind)
ROOTS_CASE = "c5_23_roots"                      # all 16 (rb, rk) combinations are slices of this one


def scope_fixture_path(name):
    return os.path.join(GOLDEN, f"overlap_scope_{name}.npz")


def scope_inputs(name):
    """The inputs of a fixture case, from its name alone: dict(s [P, m, m], bra [P, rb, D], ket [P, rk, D], ncas,
    n_alpha, n_beta, n_core, mode)."""
    import zlib
    from math import comb
    ncas, n_alpha, n_beta, n_core, mode, P, rb, rk, recipe = SCOPE_CASES[name]
    m, D = n_core + ncas, comb(ncas, n_alpha) * comb(ncas, n_beta)
    if recipe.startswith("mirror:"):
        src = scope_inputs(recipe[7:])
        na, nb = comb(ncas, n_beta), comb(ncas, n_alpha)               # of the source
        flip = lambda v: np.ascontiguousarray(v.reshape(v.shape[:2] + (na, nb)).transpose(0, 1, 3, 2)).reshape(v.shape)  # noqa: E731
        return dict(src, n_alpha=n_alpha, n_beta=n_beta, bra=flip(src["bra"]), ket=flip(src["ket"]))
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    s = np.empty((P, m, m))
    for p in range(P):
        if recipe == "generic":
            s[p] = _generic_s(m, n_core, rng)
        elif recipe == "permutation":
            s[p] = np.eye(m) + 0.3 * rng.standard_normal((m, m))
            s[p, :n_core, :n_core] = _signed_permutation_core(n_core, rng)
        elif recipe.startswith("cond:"):
            s[p] = np.eye(m) + 0.5 / np.sqrt(m) * rng.standard_normal((m, m))
            s[p, :n_core, :n_core] = _with_cond(n_core, float(recipe[5:]), rng)
        elif recipe.startswith("ucond:"):
            s[p] = _with_cond(ncas, float(recipe[6:]), rng)
        elif recipe.startswith("pivot:"):
            s[p] = pivot_matrices(ncas)[recipe[6:]]
        else:
            raise KeyError(recipe)
    bra = rng.standard_normal((P, rb, D)) / np.sqrt(D)
    ket = rng.standard_normal((P, rk, D)) / np.sqrt(D)
    return dict(s=s, bra=bra, ket=ket, ncas=ncas, n_alpha=n_alpha, n_beta=n_beta, n_core=n_core, mode=mode)


def make_scope_case(name):
    """Everything a fixture file holds: the inputs, the 40-digit ``out`` and ``core_det``, the errors of the float64 host
    route against them (``host_err``: of out, divided by max(1, |out|); ``host_core_err``: of core_det, divided by max(1,
    |core_det|)), cond(s_cc) and cond(U)."""
    a = scope_inputs(name)
    args = (a["n_core"], a["ncas"], a["n_alpha"], a["n_beta"])
    P = a["s"].shape[0]
    out = np.empty((P, a["bra"].shape[1], a["ket"].shape[1]))
    core, cond_core, cond_U = np.empty(P), np.ones(P), np.empty(P)
    host_err = host_core_err = 0.0
    for p in range(P):
        out[p], core[p], U = exact_reference(a["s"][p], *args, a["bra"][p], a["ket"][p], None, a["mode"], True)
        h, hdet = host_reference(a["s"][p], *args, a["bra"][p], a["ket"][p], None, a["mode"], True)
        host_err = max(host_err, np.abs(h - out[p]).max() / max(1.0, np.abs(out[p]).max()))
        host_core_err = max(host_core_err, abs(hdet - core[p]) / max(1.0, abs(core[p])))
        if a["n_core"]:
            cond_core[p] = np.linalg.cond(a["s"][p][:a["n_core"], :a["n_core"]])
        if a["mode"] == 1:                               # (of U before its Q factor is taken)
            U0 = exact_U(a["s"][p], a["n_core"], a["ncas"], 0)[0]
            U = np.array([[float(U0[i, k]) for k in range(a["ncas"])] for i in range(a["ncas"])])
        cond_U[p] = np.linalg.cond(U)
    return dict(s=a["s"], bra=a["bra"], ket=a["ket"], index=np.zeros(0, dtype=np.int32), ncas=np.int64(a["ncas"]),
                n_alpha=np.int64(a["n_alpha"]), n_beta=np.int64(a["n_beta"]), n_core=np.int64(a["n_core"]),
                mode=np.int64(a["mode"]), signed=np.int64(1), out=out, core_det=core, host_err=np.float64(host_err),
                host_core_err=np.float64(host_core_err), cond_core=cond_core, cond_U=cond_U)


@functools.lru_cache(maxsize=None)
def scope_fixture(name):
    with np.load(scope_fixture_path(name)) as f:
        return {k: f[k] for k in f.files}


def scope_bound(host_err):
    """max(1e-12, 10 x host error), to be multiplied with max(1, |reference|): the floor is the bound of the sector tests
    against the host route, the factor the project's habit.  Never taken from the device."""
    return max(1e-12, 10.0 * float(host_err))
