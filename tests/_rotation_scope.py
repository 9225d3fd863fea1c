"""Cases, host twins and references of the scope tests of the orbital-rotation kernels (csrc/expm.hip: ``oovqe_expm``,
``oovqe_expm_skew``, ``oovqe_rotate_orbitals_batch``) and of the line-search kernels (csrc/linesearch.hip:
``oovqe_linesearch_points``, ``oovqe_linesearch_update``).  Nothing here touches a device.

References
  * ``expm_ref``: np.longdouble (64-bit mantissa), scaling until the 1-norm is at most 2^-4, 24 Taylor terms (remainder
    2^-100 / 25!), then the squarings.  Neither its thresholds nor its degree are the kernel's.
    tests/test_rotation_scope_cpu.py holds it against 50-digit ``mpmath.expm`` and against ``scipy.linalg.expm``.
  * ``expm_twin``: the kernel's algorithm in numpy, in the precision asked for: s from the 1-norm with theta = 0.5 and
    s < 60, degree 8 / 12 / 16 at 0.06 and 0.3, A2, A3 = A2 A, A4 = A2 A2, Paterson-Stockmeyer with the kernel's grouping
    of the coefficients, s squarings.  In float64 it says what the algorithm itself loses at a matrix; the bound of a
    device result is ten times that (``expm_bound``; the factor covers the MFMA's order of summation).
  * ``planar``: a direct sum of planar rotation generators under a seeded permutation, optionally with one plane
    stretched by a diagonal similarity; its exponential is cos and sin in longdouble.
  * ``ls_points_twin``, ``ls_update_twin``: the rule of include/oovqe.h, one problem at a time, on Python floats.
"""
import math

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53

# ---- 1. the exponential ------------------------------------------------------------------------------------------------
THETA, THETA8, THETA12 = 0.5, 0.06, 0.3               # csrc/expm.hip
INV_FACT = [1.0 / math.factorial(k) for k in range(17)]     # (k! < 2^53: the kernel's 1.0 / k! exactly)


def norm1(X):
    return float(np.abs(np.asarray(X, dtype=np.float64)).sum(axis=0).max()) if np.size(X) else 0.0


def expm_ref(X):
    A = np.asarray(X, dtype=LD)
    n = A.shape[0]
    nrm = np.abs(A).sum(axis=0).max()
    s = 0
    while nrm > LD(2.0) ** -4:
        nrm = nrm / 2
        s += 1
    A = A * (LD(2.0) ** -s)
    eye = np.eye(n, dtype=LD)
    P = eye.copy()
    for k in range(24, 0, -1):                         # Horner: 1 + A/1 (1 + A/2 (1 + ... A/24))
        P = eye + (A @ P) / LD(k)
    for _ in range(s):
        P = P @ P
    return P


def expm_twin(X, dtype=np.float64):
    """-> (exp(X) as the kernel computes it, s, degree)"""
    A = np.asarray(X, dtype=dtype)
    n = A.shape[0]
    nrm = dtype(0.0)
    for c in range(n):
        cs = dtype(0.0)
        for r in range(n):
            cs = cs + abs(A[r, c])
        nrm = max(nrm, cs)
    nrm = float(nrm)
    s = 0
    while nrm > THETA and s < 60:
        nrm *= 0.5
        s += 1
    deg = 8 if nrm <= THETA8 else 12 if nrm <= THETA12 else 16
    A = A * dtype(math.ldexp(1.0, -s))
    A2 = A @ A
    A3 = A2 @ A
    A4 = A2 @ A2
    f = [dtype(v) for v in INV_FACT]
    eye = np.eye(n, dtype=dtype)

    def combine(T, alpha, c0, c1, c2, c3):
        v = c1 * A + c2 * A2 + c3 * A3 + c0 * eye
        return v + alpha * T

    P = combine(A4, f[deg], f[deg - 4], f[deg - 3], f[deg - 2], f[deg - 1])
    for b0 in range(deg - 8, -1, -4):
        P = combine(P @ A4, dtype(1.0), f[b0], f[b0 + 1], f[b0 + 2], f[b0 + 3])
    for _ in range(s):
        P = P @ P
    return P, s, deg


def expm_bound(X, ref=None):
    """-> (10 max |expm_twin(X, float64) - expm_ref(X)|, s, degree, max |exp|, ref)"""
    ref = expm_ref(X) if ref is None else ref
    tw, s, deg = expm_twin(X)
    return 10.0 * float(np.abs(tw.astype(LD) - ref).max()), s, deg, float(np.abs(ref).max()), ref


CAP = 1e-11


def cap(X, max_exp):
    """Every bound stays below this, so an inflated twin cannot hide a kernel error: 1e-11 max(1, max |exp|) -- or, where
    that is below what ANY float64 evaluation can keep, 40 ||X||_1 2^-53 max(1, max |exp|): rounding X alone moves exp(X)
    by ||X|| 2^-53 ||exp|| (the condition number of exp at a normal matrix is its norm), the s squarings of a scaled norm
    above 1/4 have 2^s <= 4 ||X||_1, and 10 is the factor of the bound itself.  The second figure takes over beyond
    ||X||_1 = 2252, i.e. for the norm 1e6 alone: there the twin's own error is 2e-11 .. 3e-11 at every size, N = 2
    included (measured on the CPU), which the plain 1e-11 cannot hold."""
    return max(CAP, 40.0 * norm1(X) * EPS) * max(1.0, max_exp)


def skew(n, norm, seed):
    """A seeded dense skew-symmetric matrix of the given 1-norm (to rounding; exactly 0 for norm 0 and for n = 1)."""
    r = np.random.default_rng(seed).standard_normal((n, n))
    k = r - r.T
    nk = norm1(k)
    return k * (norm / nk) if nk > 0 else k


def skew_with_exact_norm(n, norm, seed):
    """1-norm EXACTLY ``norm`` in any order of summation: the plane (0, 1) carries +-norm alone in its two columns, the
    rest is a dense skew block of 1-norm 0.6 norm."""
    k = np.zeros((n, n))
    k[1, 0], k[0, 1] = norm, -norm
    if n > 3:
        k[2:, 2:] = skew(n - 2, 0.6 * norm, seed)
    return k


SMALL_SIZES = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48)      # tile counts 1, 2, 3; every remainder of (N + 3) / 4
LARGE_SIZES = (49, 50, 63, 64, 65, 80, 96, 129)
NORMS = (0.0, 1e-8, 0.05, 0.2, 0.45, 3.0, 40.0, 1e3, 1e6)          # degree 8, 12, 16 at s = 0, then s up to 21
LARGE_NORMS = (0.0, 0.2, 3.0, 1e3, 1e6)                            # the list thinned to five per size
UP = lambda x: float(np.nextafter(x, np.inf))                      # noqa: E731
EDGE_NORMS = (THETA8, UP(THETA8), THETA12, UP(THETA12), THETA, UP(THETA))
EDGE_SIZES = (2, 5, 17, 48)
SCALARS = (0.0, 0.05, -0.2, 0.45, -3.0, 40.0, -700.0)              # N = 1 through ops.expm: exp of a number


def expm_cases(n):
    """[(label, X)] of one size: skew matrices over the norm list (and, on the small route, the threshold norms)."""
    norms = NORMS if n <= 48 else LARGE_NORMS
    out = [(f"norm {x:g}", skew(n, x, 100 * n + i)) for i, x in enumerate(norms)]
    if n in EDGE_SIZES:
        out += [(f"norm {x!r} exactly", skew_with_exact_norm(n, x, 7 * n + i)) for i, x in enumerate(EDGE_NORMS)]
    return out


def pair_tables(n, which):
    """(rows, cols) int32 of the kappa pairs: 'nonredundant' (occupied / active / virtual thirds), 'full' (all
    n (n - 1) / 2), 'last' (every pair of row n - 1: the scatter's row AND column n - 1)."""
    from auto_oo_amd import excitations as X
    if which == "full":
        r, c = np.tril_indices(n, -1)
    elif which == "last":
        r, c = np.full(n - 1, n - 1), np.arange(n - 1)
    else:
        no, na = max(n // 3, 1), max(n // 3, 1)
        occ, act, virt = list(range(no)), list(range(no, no + na)), list(range(no + na, n))
        pidx = X.non_redundant_indices(occ, act, virt, False)
        r, c = X.tril_tables(n, pidx)
    return np.asarray(r, dtype=np.int32), np.asarray(c, dtype=np.int32)


def scatter(n, rows, cols, kappa):
    k = np.zeros((n, n))
    k[rows, cols] = kappa
    k[cols, rows] = -np.asarray(kappa)
    return k


def kappa_of_norm(n, rows, cols, norm, seed):
    """A seeded kappa vector whose skew matrix has the given 1-norm (to rounding)."""
    v = np.random.default_rng(seed).standard_normal(len(rows))
    nk = norm1(scatter(n, rows, cols, v))
    return v * (norm / nk) if nk > 0 else v * 0.0


# ---- closed form -------------------------------------------------------------------------------------------------------
def planar(n, planes, seed=None, stretch=None):
    """K = sum over planes (p, q, angle) of angle (e_q e_p^T - e_p e_q^T), the planes disjoint; ``stretch`` = (plane
    index, d): that plane under the similarity diag(.., d at p, ..), which puts d angle into column q alone and angle / d
    into column p.  ``seed``: the planes are (2 i, 2 i + 1) of a seeded permutation with the angles given as a list.
    -> (K float64, exp(K) longdouble)."""
    if seed is not None:
        perm = np.random.default_rng(seed).permutation(n)
        planes = [(int(perm[2 * i]), int(perm[2 * i + 1]), a) for i, a in enumerate(planes)]
    K = np.zeros((n, n))
    U = np.eye(n, dtype=LD)
    for i, (p, q, a) in enumerate(planes):
        d = float(stretch[1]) if stretch is not None and stretch[0] == i else 1.0
        K[q, p], K[p, q] = a / d, -a * d
        c, s_ = np.cos(LD(a)), np.sin(LD(a))
        U[p, p] = U[q, q] = c
        U[q, p], U[p, q] = s_ / LD(d), -s_ * LD(d)
    return K, U


def one_column_cases(n):
    """[(label, K, exp K)]: the 1-norm sits in the two columns of ONE plane of angle 40 (a rotation generator), or in ONE
    column (a plane of angle 4 stretched by 16: 64 in column q, 0.25 in column p); every other column stays below 0.4.
    A norm reduction that drops such a column picks s = 0 and fails by orders of magnitude."""
    spots = list(dict.fromkeys((p, q) for p, q in ((0, 1), (63, 64), (n - 2, n - 1)) if q < n))
    # (row p, column q) of the heavy element: the columns 0, 63, 64 and n - 1, and one in the LAST ROW, which for
    # n = 1 mod 64 is the one row that the remainder loop of ``norm1_partial_kernel`` sums
    singles = list(dict.fromkeys((p, q) for p, q in ((5, 0), (58, 63), (59, 64), (n - 6, n - 1), (n - 1, n - 6))
                                 if max(p, q) < n))
    out = []
    for j, (p, q) in enumerate(spots):
        out.append((f"angle 40 in columns {p}, {q}", *_filled(n, (p, q, 40.0), None, 300 * n + j)))
    for j, (p, q) in enumerate(singles):
        out.append((f"64 in column {q} alone (row {p})", *_filled(n, (p, q, 4.0), (0, 16.0), 500 * n + j)))
    return out


def _filled(n, heavy, stretch, seed):
    rng = np.random.default_rng(seed)
    rest = [i for i in rng.permutation(n) if i not in heavy[:2]]
    planes = [heavy] + [(int(rest[2 * i]), int(rest[2 * i + 1]), float(rng.uniform(-0.39, 0.39)))
                        for i in range(len(rest) // 2)]
    return planar(n, planes, stretch=stretch)


# ---- non-normal input: the block matrices of the Frechet derivatives --------------------------------------------------------
BLOCK_SHAPES = ((2, 24), (2, 25), (3, 16), (3, 17))       # sizes 48 | 50 and 48 | 51: both sides of the one-workgroup limit
K_SCALES = (1e-4, 0.05, 0.5, 3.0)
OFF_MAGNITUDES = (1.0, 30.0, 100.0)


def block_parts(nb, n, k_scale, mag, seed=0):
    """(K, [off-diagonal blocks]): K skew of 1-norm ``k_scale``; dense blocks whose elements have magnitude ``mag``
    (uniform in +-mag, like the U (2 F^T) of ``kappa_gradient`` with Fock elements of tens of Hartree)."""
    rng = np.random.default_rng(9000 + 97 * n + 13 * nb + seed)
    K = skew(n, k_scale, int(rng.integers(1 << 30)))
    return K, [rng.uniform(-mag, mag, (n, n)) for _ in range(nb - 1)]


def block_matrix(K, offs):
    n, nb = K.shape[0], len(offs) + 1
    M = np.zeros((nb * n, nb * n))
    for i in range(nb):
        M[i * n:(i + 1) * n, i * n:(i + 1) * n] = K
    for i, A in enumerate(offs):
        M[i * n:(i + 1) * n, (i + 1) * n:(i + 2) * n] = A
    return M


def block_cases():
    return [(nb, n, ks, mag) for nb, n in BLOCK_SHAPES for ks in K_SCALES for mag in OFF_MAGNITUDES]


# The condition of the Frechet helpers (tests/test_rotation_scope_cpu.py measures both sides of it, on the CPU): the
# error of the float64 twin on the matrix a helper hands to ``ops.expm``, as a fraction of the largest element of the
# wanted block.
FRECHET_THRESHOLD = 1.5e-14


# ---- 2. orbital rotation ------------------------------------------------------------------------------------------------
def orbitals(n, seed):
    """A seeded orthogonal matrix times a well-conditioned column scaling (0.5 .. 2)."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return q * rng.uniform(0.5, 2.0, n)[None, :]


MIXED_NORMS = (0.0, 1e-8, 0.2, 3.0, 1e3)          # side by side in one batch: each workgroup picks its own s and degree


def rotation_reference(n, rows, cols, kappa, C):
    """-> (C expm(-K) longdouble, expm(-K) longdouble, bound of the product, bound of U, s, degree)."""
    K = scatter(n, rows, cols, kappa)
    b_u, s, deg, _, U = expm_bound(-K)
    ref = np.asarray(C, dtype=LD) @ U
    b_c = b_u + 10.0 * n * EPS * float(np.abs(C).max()) * n
    return ref, U, b_c, b_u, s, deg


# ---- 3. line search ----------------------------------------------------------------------------------------------------------
def dyadic(rng, shape, bits_below=20, below=2.0 ** 10):
    """Multiples of 2^-bits_below of magnitude below ``below``."""
    m = rng.integers(-int(below * 2 ** bits_below) + 1, int(below * 2 ** bits_below), shape)
    return m.astype(np.float64) * 2.0 ** -bits_below


def ls_points_twin(flat, dp, t, n_a):
    """points of ONE problem: ([first n_a], [rest]) of flat + t dp, the product rounded before the sum."""
    n = len(flat)
    n_a = n if n_a == 0 else n_a
    p = [float(t) * float(dp[i]) + float(flat[i]) for i in range(n)]
    return p[:n_a], p[n_a:]


def ls_update_twin(trial, energy, slope, info, beta, first, give_up, t, active, best):
    """The rule of include/oovqe.h over lists of Python floats (``trial`` / ``info`` may be None); t, active and best are
    changed in place.  -> flags."""
    batch = len(energy)
    any_act, any_nan, any_up = 0.0, 0.0, 0.0
    for b in range(batch):
        was = True if first else active[b] != 0.0
        act = False
        if was:
            if give_up:
                t[b] = 0.0
                best[b] = energy[b]
            else:
                tr = trial[b]
                if tr <= energy[b] + t[b] * slope[b]:              # (False for a NaN on either side)
                    best[b] = tr
                else:
                    act = True
                    t[b] = t[b] * beta
        active[b] = 1.0 if act else 0.0
        if act:
            any_act = 1.0
            if not slope[b] < 0.0:
                any_up = 1.0
        if slope[b] != slope[b]:
            any_nan = 1.0
    return [any_act, float(min(info)) if info is not None else 0.0, any_nan, any_up]


UPDATE_BATCHES = (1, 255, 256, 257, 1000)
ROUNDS = 6


def scripted_search(batch, beta=0.3, seed=0, nan_every=5, period=7, rounds=ROUNDS):
    """A search of ``rounds`` rounds and a give-up call for ``batch`` problems: problem b accepts in round b mod ``period``
    (a round that is not made: never).  Energies are dyadic and the slopes are -2^k, so energy + t slope is rounded once whether the product is
    fused into the sum or not, and the twin's threshold is the kernel's to the bit.  An accepting trial sits exactly on
    the threshold (even b) or 2^-12 below it; a rejected one is the next float above it, or a NaN (every ``nan_every``-th
    problem); a problem that has accepted is offered -1e9 afterwards, which it must ignore.
    -> dict: energy, slope [batch], trials [rounds][batch], and per round (and for the give-up call, last) the state
    the twin reaches: t, active, best, flags."""
    rng = np.random.default_rng(seed + batch)
    energy = dyadic(rng, batch, 12, 2.0 ** 8).tolist()
    slope = (-(2.0 ** rng.integers(-6, 3, batch))).tolist()
    t, active, best = [1.0] * batch, [7.0] * batch, [-5.0] * batch          # (stale active / best: first = 1 ignores them)
    trials, states = [], []
    for r in range(rounds):
        tr = []
        for b in range(batch):
            thr = energy[b] + t[b] * slope[b]
            if r > 0 and active[b] == 0.0:
                tr.append(-1e9)
            elif r == b % period:
                tr.append(thr if b % 2 == 0 else thr - 2.0 ** -12)
            else:
                tr.append(float("nan") if b % nan_every == 0 else float(np.nextafter(thr, np.inf)))
        flags = ls_update_twin(tr, energy, slope, None, beta, r == 0, 0, t, active, best)
        trials.append(tr)
        states.append((list(t), list(active), list(best), flags))
    flags = ls_update_twin(None, energy, slope, None, beta, 0, 1, t, active, best)
    states.append((list(t), list(active), list(best), flags))
    return dict(energy=energy, slope=slope, trials=trials, states=states)
