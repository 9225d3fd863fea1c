"""The CAS evaluation (csrc/cas.hip) over every realisation its plan can choose: cases, an independent reference and a
derived error bound.  Shared by tests/test_cas_scope_cpu.py and tests/test_cas_scope_gpu.py.

REFERENCE.  ``transform`` + ``assemble`` evaluate, in plain numpy and from the formulas of the reference project's
oo_energy.py / active_space.py, everything one evaluation writes: c0, c1, c2, E, dE, the orbital gradient vector of
every RDM set and, where asked, the generalized Fock and gradient matrices, g_mo[:, :M, :M, :M] and h_mo[:, :M].  It
shares no code with oracle/cpu_ref.py or the library.  ``np.longdouble`` is the truth; the float64 version is the same
routine on BLAS ``matmul`` and serves every geometry of a batch.

      g_mo[n,x,y,z] = sum_pqrs C[p,n] C[q,x] C[r,y] C[s,z] g[p,q,r,s]          h_mo[n,x] = sum_pq C[p,n] h[p,q] C[q,x]
      FI[n,x]  = h_mo[n,x] + sum_i (2 g_mo[n,x,i,i] - g_mo[n,i,i,x])
      c0 = nuc + sum_i (h_mo[i,i] + FI[i,i]);   c1 = FI[act,act];   c2 = g_mo[act,act,act,act] / 2
      per RDM set k:   FA[n,i] = sum_vw gam_k[v,w] (g_mo[n,i,V,W] - g_mo[n,W,V,i] / 2)
                       F_k[i,n] = 2 ([k == 0] FI[n,i] + FA[n,i])
                       F_k[V,n] = sum_w FI[n,W] gam_k[v,w] + sum_wxy Gam_k[v,w,x,y] g_mo[n,W,X,Y];   F_k[virtual, n] = 0
                       gvec_k[t] = 2 (F_k[r_t, c_t] - F_k[c_t, r_t]);   e_k = c1 . gam_k + c2 . Gam_k
      E = c0 + e_0;   dE[k-1] = e_k (k >= 1);   fock = F_0;   gmat = 2 (F_0 - F_0^T)

BOUND.  No tolerance is set by hand.  The same routine runs a second time on the absolute values of all inputs with
every subtraction turned into an addition (``sub = +1``): that gives, per output element, the sum A of the magnitudes
of its terms.  An element computed by ANY order of k rounded operations per term differs from the exact value by at
most k 2^-53 A (to first order; Higham, Accuracy and Stability, (3.5)), so the bound of an element is k 2^-53 A with k
the longest chain of rounded operations that forms it in the kernels (one fused multiply-add = one operation; the
multiplications by 2 and 1/2 are exact).  Against the float64 reference, which makes errors of the same kind, the
bound is doubled.  k per quantity (``chain_lengths``; N basis functions, o occupied, a active orbitals):

      g_mo, c2     4 N                        the four contractions r -> y, s -> z (stage 1), q -> x, p -> n, each a chain
                                              of N multiply-adds whatever kernel performs it
      h_mo         2 N
      c1 (FI)      4 N + 2 o + 1              g_mo, then 2 o additions and h_mo
      c0           4 N + 4 o + 2              FI[i,i], then 2 o additions and nuc
      fock (F_k)   4 N + 2 o + a^3 + a^2 + a + 4    the longer of the two rows: FI, its product with gam (a terms), then
                                              the a^3 products with Gam; the occupied rows (a^2 terms) are shorter
      gvec, gmat   k(fock) + 1                one subtraction
      E, dE        4 N + 4 o + a^4 + a^2 + 4  c0, then the a^2 + a^4 products with the RDMs (a tree in the kernels:
                                              shorter than the serial chain counted here)

An element whose A is zero (the virtual rows of fock, the virtual-virtual block of gmat) must be exactly zero.

INPUTS.  Every geometry of a batch has its own C, RDM sets and nuclear term; a batch cycles min(G, 4) integral
tensors.  The tensors carry exactly the symmetries the flags of the case claim: flags 3 -> g[pq][rs] from a
[tri][tri] table, flags 1 -> from a [tri][N][N] table (p <-> q only), flags 0 -> no symmetry; in a flags 0 / 1 case with
at least two tensors one of them is a fully symmetric tensor perturbed by one ulp in one element (flags 0) or in one
element and its p <-> q mirror (flags 1), as tests/test_eval_plan_gpu.py does.  All integrals are positive and C is
mostly positive, so that terms cancel little and A stays close to the values: ``input_condition`` asserts, per case,
that the bound of every quantity is below 1e-9 max(1, largest element of the quantity), the loosest tolerance the
older whole-evaluation tests use for E.  RDM sets are random and unphysical (the kernels are linear in them) except
in circuit cases, where the circuit kernel produces them and the test reads them back.

CASES.  ``enumerate_classes`` sweeps the plan on the CPU (``ops.eval_plan``) over RANGES -- N up to 100, so that the
k-chunk depths 11 and 12 of half_stream_kernel appear -- and keeps, per class (path, stage-1 kernel, tail build,
circuit placement, W), the shape with the smallest G N^4.  CASES holds the result as data; tests/test_cas_scope_cpu.py
repeats the sweep and asserts that CASES reaches every class, so a class added to cas.hip later fails there until it
gets a case.  KNOB_CASES, EDGE_CASES and OPTION_CASES add the launch-time choices, the edges of the orbital spaces and
the realisations behind the test options.
"""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
CONDITION = 1e-9

# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------
_POOL = None


def _threads():
    try:
        return max(1, min(16, len(os.sched_getaffinity(0))))
    except AttributeError:
        return max(1, min(16, os.cpu_count() or 1))


def _mm(a, b):
    """a @ b; long double has no BLAS, so its row blocks go to threads (numpy's loop releases the GIL)"""
    global _POOL
    if a.dtype != LD or a.shape[0] < 4096:
        return a @ b
    if _POOL is None:
        _POOL = ThreadPoolExecutor(_threads())
    parts = np.array_split(np.arange(a.shape[0]), 4 * _threads())
    out = np.empty((a.shape[0], b.shape[1]), dtype=LD)

    def work(idx):
        out[idx[0]:idx[-1] + 1] = a[idx[0]:idx[-1] + 1] @ b
    list(_POOL.map(work, [p for p in parts if len(p)]))
    return out


def transform(h, g, C, M, dtype=np.float64, mag=False):
    """-> g_mo [N, M, M, M], h_mo [N, M] in ``dtype``; mag: of the absolute values (no subtraction occurs here)"""
    N = C.shape[0]
    if mag:
        h, C = np.abs(h), np.abs(C)
        g = g if g.min() >= 0 else np.abs(g)
    h, C = h.astype(dtype), C.astype(dtype)
    Cm = np.ascontiguousarray(C[:, :M])
    t = _mm(np.asarray(g.reshape(N * N * N, N), dtype=dtype), Cm)                        # [p q r, z]
    t = np.ascontiguousarray(t.reshape(N * N, N, M).transpose(0, 2, 1)).reshape(N * N * M, N)
    t = _mm(t, Cm).reshape(N, N, M, M)                                                   # [p, q, z, y]
    t = np.ascontiguousarray(t.transpose(0, 3, 2, 1)).reshape(N * M * M, N)              # [p y z, q]
    t = _mm(t, Cm).reshape(N, M * M, M)                                                  # [p, y z, x]
    t = np.ascontiguousarray(t.transpose(2, 1, 0)).reshape(M * M * M, N)                 # [x y z, p]
    gm = np.ascontiguousarray(_mm(t, C).reshape(M, M, M, N).transpose(3, 0, 1, 2))       # [n, x, y, z]
    hmo = C.T @ (h @ Cm)
    return gm, hmo


def assemble(gm, hmo, gamma, Gamma, nuc, n_occ, ncas, rows, cols, mag=False):
    """Everything one evaluation writes, from g_mo, h_mo and the RDM sets gamma [nrdm, a, a], Gamma [nrdm, a, a, a, a]
    (see the module docstring).  mag: inputs are magnitudes, every subtraction becomes an addition."""
    dtype = gm.dtype
    sub = 1 if mag else -1
    N, M = hmo.shape
    o, a = n_occ, ncas
    gamma, Gamma = (np.abs(x).astype(dtype) if mag else x.astype(dtype) for x in (gamma, Gamma))
    nuc = dtype.type(abs(nuc) if mag else nuc)
    nrdm = gamma.shape[0]
    occ, act = np.arange(o), np.arange(o, M)
    two, half = dtype.type(2), dtype.type(0.5)
    FI = hmo.copy()
    for i in occ:
        FI = FI + two * gm[:, :, i, i] + sub * gm[:, i, i, :]
    c0 = nuc + sum((hmo[i, i] + FI[i, i] for i in occ), dtype.type(0))
    c1 = FI[np.ix_(act, act)]
    gact = gm[:, o:, o:, o:]                                            # [n, W, X, Y]
    c2 = half * gact[o:M]
    # J[n, i, v, w] = g_mo[n, i, V, W];  K[n, i, v, w] = g_mo[n, W, V, i]
    J = gm[:, :o, o:, o:]
    K = gm[:, o:, o:, :o].transpose(0, 3, 2, 1)
    JK = J + sub * half * K
    F = np.zeros((nrdm, N, N), dtype=dtype)
    e = np.zeros(nrdm, dtype=dtype)
    for k in range(nrdm):
        FA = np.tensordot(JK, gamma[k], axes=([2, 3], [0, 1]))         # [n, i]
        F[k, :o] = (two * ((FI[:, :o] if k == 0 else 0) + FA)).T
        F[k, o:M] = (FI[:, o:] @ gamma[k].T + gact.reshape(N, a ** 3) @ Gamma[k].reshape(a, a ** 3).T).T
        e[k] = (c1 * gamma[k]).sum() + (c2 * Gamma[k]).sum()
    gvec = two * (F[:, rows, cols] + sub * F[:, cols, rows])
    return dict(c0=np.array([c0]), c1=c1, c2=c2, E=np.array([c0 + e[0]]), dE=e[1:], gvec=gvec, fock=F[0],
                gmat=two * (F[0] + sub * F[0].T), Gm=gm, hmo=hmo)


def evaluate(h, g, C, gamma, Gamma, nuc, n_occ, ncas, rows, cols, dtype=np.float64, mag=False):
    gm, hmo = transform(h, g, C, n_occ + ncas, np.dtype(dtype), mag)
    return assemble(gm, hmo, gamma, Gamma, nuc, n_occ, ncas, rows, cols, mag)


def chain_lengths(N, n_occ, ncas):
    """k per quantity: the longest chain of rounded operations that forms one element (module docstring)"""
    o, a = n_occ, ncas
    fock = 4 * N + 2 * o + a ** 3 + a ** 2 + a + 4
    e = 4 * N + 4 * o + a ** 4 + a ** 2 + 4
    return dict(Gm=4 * N, c2=4 * N, hmo=2 * N, c1=4 * N + 2 * o + 1, c0=4 * N + 4 * o + 2, fock=fock, gvec=fock + 1,
                gmat=fock + 1, E=e, dE=e)


def compare(got, ref, mag, k, factor=1):
    """Every element of every quantity of ``got`` against ``ref`` with the bound factor k 2^-53 A (A from ``mag``).
    -> (ratios, failures): ratios {quantity: max |got - ref| / (2^-53 A)} (to be held against factor k), failures a
    list of (quantity, flat index of the worst element, ratio, allowed)."""
    ratios, failures = {}, []
    for q, x in got.items():
        if x is None:
            continue
        x = np.asarray(x, dtype=LD).reshape(-1)
        r = np.asarray(ref[q], dtype=LD).reshape(-1)
        A = np.asarray(mag[q], dtype=LD).reshape(-1)
        assert x.shape == r.shape == A.shape, (q, x.shape, r.shape, A.shape)
        err = np.abs(x - r)
        err[~np.isfinite(x)] = np.inf
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(A > 0, err / (LD(U) * A), np.where(err > 0, np.inf, 0))
        worst = int(np.argmax(ratio)) if ratio.size else 0
        ratios[q] = float(ratio[worst]) if ratio.size else 0.0
        if ratio.size and not ratio[worst] <= factor * k[q]:
            failures.append((q, worst, ratios[q], factor * k[q]))
    return ratios, failures


def input_condition(ref, mag, k):
    """-> list of (quantity, bound, limit) that break: max bound < 1e-9 max(1, largest element of the quantity)"""
    bad = []
    for q in k:
        if q not in ref or np.size(ref[q]) == 0:
            continue
        bound = float(k[q] * U * np.max(np.abs(np.asarray(mag[q], dtype=np.float64))))
        limit = CONDITION * max(1.0, float(np.max(np.abs(np.asarray(ref[q], dtype=np.float64)))))
        if not bound < limit:
            bad.append((q, bound, limit))
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def kappa_tables(N, n_occ, ncas):
    """(row, col), row > col in the order of the strict lower triangle, without occupied-occupied and virtual-virtual"""
    M = n_occ + ncas
    r, c = np.tril_indices(N, -1)
    keep = ~((r < n_occ) & (c < n_occ)) & ~((r >= M) & (c >= M))
    return r[keep].astype(np.int32), c[keep].astype(np.int32)


def _tri_index(N):
    idx = np.zeros((N, N), dtype=np.int64)
    iu = np.triu_indices(N)
    idx[iu] = np.arange(len(iu[0]))
    return np.maximum(idx, idx.T)


def integral_tensors(N, flags, count, seed):
    """``count`` <= 4 tensors [N, N, N, N] with exactly the symmetries of ``flags`` (1: p <-> q, 3: r <-> s as well)"""
    assert flags in (0, 1, 3) and 1 <= count <= 4
    rng = np.random.default_rng([seed, N, flags])
    tri, T = _tri_index(N), N * (N + 1) // 2
    ulp = min(2, count - 1) if (flags != 3 and count >= 2 and N >= 2) else -1
    out = []
    for j in range(count):
        if flags == 3 or j == ulp:
            g = rng.uniform(0.1, 1.0, (T, T))[tri[:, :, None, None], tri[None, None, :, :]]
        elif flags == 1:
            g = rng.uniform(0.1, 1.0, (T, N, N))[tri]
        else:
            g = rng.uniform(0.1, 1.0, (N, N, N, N))
        g = np.ascontiguousarray(g)
        if j == ulp:
            r, s = (2, 3) if N >= 4 else (0, 1)
            g[0, 1, r, s] = np.nextafter(g[0, 1, r, s], np.inf)
            if flags == 1:
                g[1, 0, r, s] = g[0, 1, r, s]
        out.append(g)
    return out


def has_symmetry(g):
    """flags the tensor carries, bit for bit"""
    pq = bool(np.array_equal(g, g.transpose(1, 0, 2, 3)))
    rs = bool(np.array_equal(g, g.transpose(0, 1, 3, 2)))
    return (1 if pq else 0) | (2 if rs else 0)


def geometry_inputs(N, ncas, nrdm, G, seed):
    """Per geometry: C [G, N, N], gamma [G, nrdm, a, a], Gamma [G, nrdm, a, a, a, a], nuc [G]; per tensor: h [4, N, N]"""
    rng = np.random.default_rng([seed, N, ncas, nrdm, G, 7])
    C = rng.uniform(-0.3, 1.0, (G, N, N)) / np.sqrt(N)
    gamma = rng.uniform(-1.0, 1.0, (G, nrdm) + (ncas,) * 2)
    Gamma = rng.uniform(-1.0, 1.0, (G, nrdm) + (ncas,) * 4)
    nuc = 10.0 + 0.37 * np.arange(G) + rng.uniform(0, 0.1, G)
    h = rng.uniform(-1.0, 1.0, (4, N, N))
    h = 0.5 * (h + h.transpose(0, 2, 1))
    return C, gamma, Gamma, nuc, h


def long_double_geometries(G):
    """The geometries held against the long-double reference: the first, the last and two in the middle whose index
    is no multiple of 8"""
    picks = {0, G - 1}
    for m in (G // 3, (2 * G) // 3):
        while m % 8 == 0 and m + 1 < G:
            m += 1
        if 0 <= m < G:
            picks.add(m)
    return sorted(picks)


# ---------------------------------------------------------------------------------------------------------------------
# the plan space
# ---------------------------------------------------------------------------------------------------------------------
# (ncas, nelecas, a UCCD circuit can be run for it in a test); without a circuit the evaluation is given 3 RDM sets
SPACES = ((2, 2, True), (3, 4, True), (4, 4, True), (1, 2, False), (6, 6, False), (8, 8, False))
RANGES = dict(N_max=100, spaces=SPACES, n_occ=(0, 1, 2, 5, 6, 8, 10, 12, 13, 14, 15, 18, 29, 30, 40),
              batch=(1, 2, 7, 31, 129, 193, 256, 385), flags_packed=((0, False), (1, False), (3, False), (3, True)))
GIVEN_N_THETA = 2


@functools.lru_cache(maxsize=None)
def circuit_sizes(ncas, nelecas):
    from auto_oo_amd import excitations as X
    gates, n_theta = X.uccd_gates(ncas, nelecas, False)
    return n_theta, len(gates)


def n_kappa(N, n_occ, ncas):
    nv = N - n_occ - ncas
    return n_occ * ncas + ncas * nv + n_occ * nv + ncas * (ncas - 1) // 2


def plan_of(N, n_occ, ncas, G, flags, packed, circuit, n_theta=None, nelecas=None):
    """ops.eval_plan of a case shape; circuit: the UCCD circuit of the space, else ``n_theta`` + 1 given RDM sets"""
    from auto_oo_amd import ops
    if circuit:
        nt, ng = circuit_sizes(ncas, nelecas)
    else:
        nt, ng = (GIVEN_N_THETA if n_theta is None else n_theta), 0
    return ops.eval_plan(N, n_occ, ncas, n_kappa(N, n_occ, ncas), G, flags, packed, nt, ng, True, circuit)


def class_of(plan):
    return (plan["path"], plan["stage1"], plan.get("tail", ""), plan["circuit"], plan["w"])


def enumerate_classes():
    """{class: (N, n_occ, ncas, nelecas, G, flags, packed, circuit)} with the smallest G N^4 per class, over RANGES"""
    from auto_oo_amd import _lib
    best = {}
    for ncas, nelecas, can_circuit in RANGES["spaces"]:
        for n_occ in RANGES["n_occ"]:
            for N in range(n_occ + ncas, RANGES["N_max"] + 1):
                for G in RANGES["batch"]:
                    for flags, packed in RANGES["flags_packed"]:
                        if flags != 3 and N < 2:
                            continue                      # a tensor of one orbital has both symmetries
                        for circuit in ((False, True) if can_circuit else (False,)):
                            try:
                                p = plan_of(N, n_occ, ncas, G, flags, packed, circuit, nelecas=nelecas)
                            except _lib.OovqeError:
                                continue
                            cls, size = class_of(p), G * N ** 4
                            if cls not in best or size < best[cls][0]:
                                best[cls] = (size, (N, n_occ, ncas, nelecas, G, flags, packed, circuit))
    return {cls: shape for cls, (_, shape) in best.items()}


# ---------------------------------------------------------------------------------------------------------------------
# the cases: (N, n_occ, ncas, nelecas, geometries, flags, packed copy, circuit)
# ---------------------------------------------------------------------------------------------------------------------
# one per class of enumerate_classes(), the shape with the smallest G N^4 that reaches it (written by that function)
CASES = (
    (1, 0, 1, 2, 1, 3, False, False), (2, 0, 2, 2, 1, 0, False, False), (2, 0, 2, 2, 1, 0, False, True),
    (2, 0, 2, 2, 1, 1, False, True), (4, 0, 4, 4, 1, 0, False, True), (4, 0, 4, 4, 1, 1, False, True),
    (6, 0, 2, 2, 385, 0, False, False), (6, 0, 2, 2, 385, 0, False, True), (6, 0, 2, 2, 385, 1, False, True),
    (6, 0, 4, 4, 385, 1, False, True), (6, 0, 4, 4, 385, 3, False, True), (6, 0, 4, 4, 385, 3, True, True),
    (6, 2, 2, 2, 385, 1, False, False), (6, 2, 2, 2, 385, 1, False, True), (6, 2, 2, 2, 385, 3, False, False),
    (6, 2, 2, 2, 385, 3, False, True), (6, 2, 2, 2, 385, 3, True, False), (6, 2, 2, 2, 385, 3, True, True),
    (7, 1, 2, 2, 256, 1, False, True), (7, 1, 2, 2, 256, 3, False, True), (7, 1, 2, 2, 256, 3, True, True),
    (17, 0, 2, 2, 1, 0, False, False), (17, 0, 2, 2, 1, 0, False, True), (17, 0, 2, 2, 1, 1, False, False),
    (17, 0, 2, 2, 1, 1, False, True), (17, 0, 4, 4, 1, 0, False, True), (17, 0, 4, 4, 1, 1, False, True),
    (17, 8, 2, 2, 129, 1, False, True), (17, 10, 2, 2, 129, 3, False, True), (17, 10, 2, 2, 129, 3, True, True),
    (17, 13, 4, 4, 1, 0, False, True), (17, 13, 4, 4, 1, 1, False, True), (17, 15, 2, 2, 1, 0, False, False),
    (17, 15, 2, 2, 1, 0, False, True), (17, 15, 2, 2, 1, 1, False, False), (17, 15, 2, 2, 1, 1, False, True),
    (20, 0, 2, 2, 31, 0, False, False), (20, 0, 2, 2, 31, 0, False, True), (20, 0, 4, 4, 31, 0, False, True),
    (20, 0, 4, 4, 31, 1, False, True), (20, 0, 4, 4, 31, 3, False, True), (20, 0, 4, 4, 31, 3, True, True),
    (20, 1, 2, 2, 31, 1, False, False), (20, 1, 2, 2, 31, 1, False, True), (20, 1, 2, 2, 31, 3, False, False),
    (20, 1, 2, 2, 31, 3, False, True), (20, 1, 2, 2, 31, 3, True, False), (20, 1, 2, 2, 31, 3, True, True),
    (21, 12, 8, 8, 1, 0, False, False), (21, 12, 8, 8, 1, 1, False, False), (21, 13, 2, 2, 129, 3, True, True),
    (23, 18, 4, 4, 1, 0, False, True), (23, 18, 4, 4, 1, 1, False, True), (33, 0, 2, 2, 1, 0, False, False),
    (33, 0, 2, 2, 1, 0, False, True), (33, 0, 2, 2, 1, 1, False, False), (33, 0, 2, 2, 1, 1, False, True),
    (33, 0, 4, 4, 1, 0, False, True), (33, 0, 4, 4, 1, 1, False, True), (33, 6, 2, 2, 193, 3, True, True),
    (33, 8, 2, 2, 129, 1, False, True), (33, 10, 2, 2, 129, 3, False, True), (33, 10, 2, 2, 129, 3, True, True),
    (33, 13, 4, 4, 1, 0, False, True), (33, 13, 4, 4, 1, 1, False, True), (33, 15, 2, 2, 1, 0, False, False),
    (33, 15, 2, 2, 1, 0, False, True), (33, 15, 2, 2, 1, 1, False, False), (33, 15, 2, 2, 1, 1, False, True),
    (33, 18, 2, 2, 1, 0, False, False), (33, 18, 2, 2, 1, 0, False, True), (33, 18, 2, 2, 1, 1, False, False),
    (33, 18, 2, 2, 1, 1, False, True), (34, 30, 3, 4, 1, 0, False, False), (34, 30, 3, 4, 1, 0, False, True),
    (34, 30, 3, 4, 1, 1, False, False), (34, 30, 3, 4, 1, 1, False, True), (41, 6, 2, 2, 193, 3, True, True),
    (42, 0, 2, 2, 7, 0, False, False), (42, 0, 2, 2, 7, 0, False, True), (42, 0, 4, 4, 7, 0, False, True),
    (42, 0, 4, 4, 7, 1, False, True), (42, 0, 4, 4, 7, 3, False, True), (42, 0, 4, 4, 7, 3, True, True),
    (42, 1, 2, 2, 7, 1, False, False), (42, 1, 2, 2, 7, 1, False, True), (42, 1, 2, 2, 7, 3, False, False),
    (42, 1, 2, 2, 7, 3, False, True), (42, 1, 2, 2, 7, 3, True, False), (42, 1, 2, 2, 7, 3, True, True),
    (44, 8, 8, 8, 1, 0, False, False), (44, 8, 8, 8, 1, 1, False, False), (45, 0, 2, 2, 1, 0, False, False),
    (45, 0, 2, 2, 1, 0, False, True), (45, 0, 2, 2, 1, 1, False, False), (45, 0, 2, 2, 1, 1, False, True),
    (45, 0, 2, 2, 7, 0, False, False), (45, 0, 2, 2, 7, 0, False, True), (45, 0, 4, 4, 1, 0, False, True),
    (45, 0, 4, 4, 1, 1, False, True), (45, 0, 4, 4, 7, 0, False, True), (45, 0, 4, 4, 7, 1, False, True),
    (45, 0, 4, 4, 7, 3, False, True), (45, 0, 4, 4, 7, 3, True, True), (45, 1, 2, 2, 7, 1, False, False),
    (45, 1, 2, 2, 7, 1, False, True), (45, 1, 2, 2, 7, 3, False, False), (45, 1, 2, 2, 7, 3, False, True),
    (45, 1, 2, 2, 7, 3, True, False), (45, 1, 2, 2, 7, 3, True, True), (45, 6, 2, 2, 193, 3, True, True),
    (45, 8, 2, 2, 129, 1, False, True), (45, 8, 8, 8, 1, 0, False, False), (45, 8, 8, 8, 1, 1, False, False),
    (45, 10, 2, 2, 129, 3, False, True), (45, 10, 2, 2, 129, 3, True, True), (45, 13, 4, 4, 1, 0, False, True),
    (45, 13, 4, 4, 1, 1, False, True), (45, 15, 2, 2, 1, 0, False, False), (45, 15, 2, 2, 1, 0, False, True),
    (45, 15, 2, 2, 1, 1, False, False), (45, 15, 2, 2, 1, 1, False, True), (45, 18, 2, 2, 1, 0, False, False),
    (45, 18, 2, 2, 1, 0, False, True), (45, 18, 2, 2, 1, 1, False, False), (45, 18, 2, 2, 1, 1, False, True),
    (45, 40, 2, 2, 1, 0, False, False), (45, 40, 2, 2, 1, 0, False, True), (45, 40, 2, 2, 1, 1, False, False),
    (45, 40, 2, 2, 1, 1, False, True), (49, 0, 2, 2, 1, 0, False, False), (49, 0, 2, 2, 1, 0, False, True),
    (49, 0, 2, 2, 1, 3, False, False), (49, 0, 2, 2, 1, 3, False, True), (49, 0, 2, 2, 1, 3, True, False),
    (49, 0, 2, 2, 1, 3, True, True), (49, 8, 8, 8, 1, 0, False, False), (49, 8, 8, 8, 1, 3, False, False),
    (49, 8, 8, 8, 1, 3, True, False), (49, 15, 2, 2, 1, 0, False, False), (49, 15, 2, 2, 1, 0, False, True),
    (49, 15, 2, 2, 1, 3, False, False), (49, 15, 2, 2, 1, 3, False, True), (49, 15, 2, 2, 1, 3, True, False),
    (49, 15, 2, 2, 1, 3, True, True), (49, 18, 2, 2, 1, 0, False, False), (49, 18, 2, 2, 1, 0, False, True),
    (49, 18, 2, 2, 1, 3, False, False), (49, 18, 2, 2, 1, 3, False, True), (49, 18, 2, 2, 1, 3, True, False),
    (49, 18, 2, 2, 1, 3, True, True), (49, 40, 2, 2, 1, 0, False, False), (49, 40, 2, 2, 1, 0, False, True),
    (49, 40, 2, 2, 1, 3, False, False), (49, 40, 2, 2, 1, 3, False, True), (49, 40, 2, 2, 1, 3, True, False),
    (49, 40, 2, 2, 1, 3, True, True), (53, 0, 2, 2, 1, 0, False, False), (53, 0, 2, 2, 1, 0, False, True),
    (53, 0, 2, 2, 1, 3, False, False), (53, 0, 2, 2, 1, 3, False, True), (53, 8, 8, 8, 1, 0, False, False),
    (53, 8, 8, 8, 1, 3, False, False), (53, 15, 2, 2, 1, 0, False, False), (53, 15, 2, 2, 1, 0, False, True),
    (53, 15, 2, 2, 1, 3, False, False), (53, 15, 2, 2, 1, 3, False, True), (53, 40, 2, 2, 1, 0, False, False),
    (53, 40, 2, 2, 1, 0, False, True), (53, 40, 2, 2, 1, 3, False, False), (53, 40, 2, 2, 1, 3, False, True),
    (57, 0, 2, 2, 1, 0, False, False), (57, 0, 2, 2, 1, 0, False, True), (57, 0, 2, 2, 1, 3, False, False),
    (57, 0, 2, 2, 1, 3, False, True), (57, 10, 6, 6, 1, 0, False, False), (57, 10, 6, 6, 1, 3, False, False),
    (57, 15, 2, 2, 1, 0, False, False), (57, 15, 2, 2, 1, 0, False, True), (57, 15, 2, 2, 1, 3, False, False),
    (57, 15, 2, 2, 1, 3, False, True), (57, 40, 2, 2, 1, 0, False, False), (57, 40, 2, 2, 1, 0, False, True),
    (57, 40, 2, 2, 1, 3, False, False), (57, 40, 2, 2, 1, 3, False, True), (58, 12, 4, 4, 1, 0, False, True),
    (58, 12, 4, 4, 1, 3, False, True), (58, 12, 4, 4, 1, 3, True, True), (61, 0, 2, 2, 1, 0, False, False),
    (61, 0, 2, 2, 1, 0, False, True), (61, 0, 2, 2, 1, 3, False, False), (61, 0, 2, 2, 1, 3, False, True),
    (61, 14, 2, 2, 1, 0, False, False), (61, 14, 2, 2, 1, 0, False, True), (61, 14, 2, 2, 1, 3, False, False),
    (61, 14, 2, 2, 1, 3, False, True), (61, 15, 2, 2, 1, 0, False, False), (61, 15, 2, 2, 1, 0, False, True),
    (61, 15, 2, 2, 1, 3, False, False), (61, 15, 2, 2, 1, 3, False, True), (61, 40, 2, 2, 1, 0, False, False),
    (61, 40, 2, 2, 1, 0, False, True), (61, 40, 2, 2, 1, 3, False, False), (61, 40, 2, 2, 1, 3, False, True),
    (65, 0, 2, 2, 1, 0, False, False), (65, 0, 2, 2, 1, 0, False, True), (65, 0, 2, 2, 1, 3, False, False),
    (65, 0, 2, 2, 1, 3, False, True), (65, 14, 2, 2, 1, 0, False, False), (65, 14, 2, 2, 1, 0, False, True),
    (65, 14, 2, 2, 1, 3, False, False), (65, 14, 2, 2, 1, 3, False, True), (65, 15, 2, 2, 1, 0, False, False),
    (65, 15, 2, 2, 1, 0, False, True), (65, 15, 2, 2, 1, 3, False, False), (65, 15, 2, 2, 1, 3, False, True),
    (65, 40, 2, 2, 1, 0, False, False), (65, 40, 2, 2, 1, 0, False, True), (65, 40, 2, 2, 1, 3, False, False),
    (65, 40, 2, 2, 1, 3, False, True), (81, 0, 2, 2, 1, 0, False, False), (81, 0, 2, 2, 1, 0, False, True),
    (81, 0, 2, 2, 1, 3, False, False), (81, 0, 2, 2, 1, 3, False, True), (81, 13, 2, 2, 1, 0, False, False),
    (81, 13, 2, 2, 1, 0, False, True), (81, 13, 2, 2, 1, 3, False, False), (81, 13, 2, 2, 1, 3, False, True),
    (81, 15, 2, 2, 1, 0, False, False), (81, 15, 2, 2, 1, 0, False, True), (81, 15, 2, 2, 1, 3, False, False),
    (81, 15, 2, 2, 1, 3, False, True), (81, 40, 2, 2, 1, 0, False, False), (81, 40, 2, 2, 1, 0, False, True),
    (81, 40, 2, 2, 1, 3, False, False), (81, 40, 2, 2, 1, 3, False, True), (89, 0, 2, 2, 1, 0, False, False),
    (89, 0, 2, 2, 1, 0, False, True), (89, 0, 2, 2, 1, 3, False, False), (89, 0, 2, 2, 1, 3, False, True),
    (89, 12, 2, 2, 1, 0, False, False), (89, 12, 2, 2, 1, 0, False, True), (89, 12, 2, 2, 1, 3, False, False),
    (89, 12, 2, 2, 1, 3, False, True), (89, 15, 2, 2, 1, 0, False, False), (89, 15, 2, 2, 1, 0, False, True),
    (89, 15, 2, 2, 1, 3, False, False), (89, 15, 2, 2, 1, 3, False, True), (89, 40, 2, 2, 1, 0, False, False),
    (89, 40, 2, 2, 1, 0, False, True), (89, 40, 2, 2, 1, 3, False, False), (89, 40, 2, 2, 1, 3, False, True),
    (97, 12, 2, 2, 1, 0, False, True), (97, 12, 2, 2, 1, 3, False, True),
)


def _i(plan, key):
    return int(plan.get(key, -1))


# The launch-time choices below the plan (oovqe_oo_eval_plan_describe reports them): every one is taken by a case.
# predicate(shape, plan, nrdm)
KNOBS = {
    "fused ring of 2 blocks": lambda s, p, n: p["path"] == "fused" and _i(p, "nbuf") == 2,
    "fused ring of 3 blocks": lambda s, p, n: p["path"] == "fused" and _i(p, "nbuf") == 3,
    "panel with W": lambda s, p, n: _i(p, "panel_w") == 1,
    "panel without W": lambda s, p, n: _i(p, "panel_w") == 0,
    "panel npan at its LDS limit": lambda s, p, n: _i(p, "npan") > 0 and _i(p, "npan") == _i(p, "npan_max"),
    "panel rdm_chunk < nrdm": lambda s, p, n: "npan" in p and 0 < _i(p, "rdm_chunk") < n,
    "column rdm_chunk < nrdm": lambda s, p, n: p["path"] == "column" and 0 < _i(p, "rdm_chunk") < n,
    "column zsplit > 1": lambda s, p, n: p["path"] == "column" and _i(p, "zsplit") > 1,
    "staged rows kernels": lambda s, p, n: _i(p, "staged_rows") == 1,
    "staged fock_kernel": lambda s, p, n: _i(p, "staged_rows") == 0,
    "remapped grid, batch no multiple of 8": lambda s, p, n: _i(p, "xcd_grid") == 1 and s[4] % 8 != 0,
    "batch of exactly 1": lambda s, p, n: s[4] == 1,
    # (fused with nchunk > 1 exists behind option fused_chunks only: a batch small enough for two chunks per CU is too
    # small for the fused path at N <= 48 -- OPTION_CASES has it)
}
# (shape, given RDM sets - 1): the smallest shape found for the knobs no class case takes
KNOB_CASES = (
    ((15, 8, 6, 6, 129, 0, False, False), 2),      # fused ring of 2 blocks; panel npan at its LDS limit, rdm_chunk < nrdm
    ((6, 0, 6, 6, 1, 0, False, False), 40),        # column rdm_chunk < nrdm, zsplit > 1; no virtual orbital
    ((21, 12, 8, 8, 1, 0, False, False), 40),      # staged fock_kernel
)

# The edges of the orbital spaces.  predicate(shape, plan)
def _m(s):
    return s[1] + s[2]


EDGES = {
    "n_occ = 0": lambda s, p: s[1] == 0,
    "ncas = 1 on a packed path": lambda s, p: s[2] == 1 and p["path"].startswith("packed"),
    "ncas = 1 on the staged path": lambda s, p: s[2] == 1 and p["path"] == "staged",
    "no virtual orbital (column, the one path that serves it)": lambda s, p: s[0] == _m(s) and s[0] > 1 and p["path"] == "column",
    "n_kappa = 0": lambda s, p: n_kappa(s[0], s[1], s[2]) == 0,
    **{f"M = {m}": (lambda s, p, m=m: _m(s) == m) for m in (16, 17, 32, 33, 48)},
    **{f"N = {n} in a batch": (lambda s, p, n=n: s[0] == n and s[4] > 1) for n in (16, 17, 32, 33, 40, 41, 44, 45, 48)},
    "N = 49": lambda s, p: s[0] == 49,
}
EDGE_CASES = (
    ((16, 6, 2, 2, 193, 3, True, True), None),     # N = 16: the one-launch tail on a full 16-wide tile
    ((32, 1, 2, 2, 31, 3, True, False), 2),        # N = 32
    ((40, 1, 2, 2, 31, 3, True, False), 2),        # N = 40
    ((44, 1, 2, 2, 7, 3, True, False), 2),         # N = 44
    ((48, 1, 2, 2, 7, 3, True, False), 2),         # N = 48
    ((20, 2, 1, 2, 31, 3, True, False), 2),        # ncas = 1 on a packed path
    ((33, 29, 1, 2, 1, 0, False, False), 2),       # ncas = 1 on the staged path
    ((45, 30, 2, 2, 1, 0, False, False), 2),       # M = 32
    ((53, 44, 4, 4, 1, 0, False, False), 2),       # M = 48
)
# shapes the plan refuses, with the words of the error
REFUSED = (
    ((53, 45, 4, 4, 1, 0, False, False), "n_occ+ncas = 49 > 48 not supported"),
    ((20, 12, 8, 8, 1, 0, False, False), "the staged path needs at least one virtual orbital"),
)

# Second tier: the realisations behind the test options, one case each at the smallest class shape that takes it.
# (option, value, shape, given RDM sets - 1, class under the option, further plan fields under the option)
OPTION_CASES = (
    ("sym_two_step", 1, (20, 1, 2, 2, 31, 3, False, False), 2,
     ("packed_two_step", "half_tri_kernel<8,2,0>", "", "none", False), {}),
    ("sym_simple", 1, (20, 1, 2, 2, 31, 3, False, False), 2,
     ("packed_two_step", "half_transform_kernel<1,8,2> (slabs p <= q)", "", "none", False), {}),
    ("sym_mirror", 1, (20, 1, 2, 2, 31, 3, False, False), 2,
     ("fused", "half_transform_fused_kernel<8,2>", "", "none", False), {}),
    ("sym_no_rs", 1, (20, 1, 2, 2, 31, 3, False, False), 2,
     ("packed_split", "half_tri_kernel<8,2,0>", "", "none", False), {}),
    ("panel_no_w", 1, (6, 2, 2, 2, 385, 1, False, True), None,
     ("packed_split", "half_tri_kernel<4,1,0>", "", "own", False), {"panel_w": "0"}),
    ("no_ride", 1, (7, 1, 2, 2, 256, 1, False, True), None,
     ("packed_split", "half_tri_kernel<4,1,0>", "", "own", True), {"panel_w": "1"}),
    ("tail_split", 1, (6, 2, 2, 2, 385, 3, True, True), None,
     ("packed_split", "half_tri_reg_kernel<4,1,2,3>", "", "own", True), {"panel_w": "1"}),
    ("cas_unfused", 1, (6, 0, 2, 2, 385, 0, False, False), 2,
     ("column", "half_transform_kernel<1,4,1>", "", "none", False), {}),
    ("fused_chunks", 2, (6, 0, 2, 2, 385, 0, False, False), 2,
     ("fused", "half_transform_fused_kernel<4,1>", "", "none", False), {"nchunk": "2", "qc": "4"}),
    ("gm_plain_grid", 1, (6, 2, 2, 2, 385, 3, False, False), 2,
     ("packed_split", "half_tri_kernel<4,1,1>", "", "none", False), {"xcd_grid": "0"}),
    ("panel_rows", 3, (6, 2, 2, 2, 385, 3, False, False), 2,
     ("packed_split", "half_tri_kernel<4,1,1>", "", "none", False), {"npan": "3"}),
)


def all_cases():
    """[(shape, given RDM sets - 1 or None for a circuit case)]: class, knob and edge cases"""
    out = [(s, None if s[7] else GIVEN_N_THETA) for s in CASES]
    return out + list(KNOB_CASES) + list(EDGE_CASES)


def case_plan(shape, n_given):
    N, n_occ, ncas, nelecas, G, flags, packed, circuit = shape
    return plan_of(N, n_occ, ncas, G, flags, packed, circuit, n_theta=n_given, nelecas=nelecas)


def case_nrdm(shape, n_given):
    return 1 + (circuit_sizes(shape[2], shape[3])[0] if shape[7] else n_given)


def input_key(shape):
    """cases with the same key share integrals, orbitals and references"""
    return shape[:6]


def case_inputs(shape, nrdm, seed=2026):
    """Host inputs of a case: dict(g = [tensors], which [G] -> tensor of geometry g, h [4, N, N], C, gamma, Gamma, nuc,
    rows, cols)"""
    N, n_occ, ncas, _, G, flags = shape[:6]
    g = integral_tensors(N, flags, min(G, 4), seed)
    C, gamma, Gamma, nuc, h = geometry_inputs(N, ncas, nrdm, G, seed)
    rows, cols = kappa_tables(N, n_occ, ncas)
    return dict(g=g, which=np.arange(G) % len(g), h=h, C=C, gamma=gamma, Gamma=Gamma, nuc=nuc, rows=rows, cols=cols)


class Reference:
    """g_mo and h_mo of the geometries of one input key, made once per precision and shared by its cases"""

    def __init__(self, shape, inp):
        self.shape, self.inp, self._t = shape, inp, {}
        self.k = chain_lengths(shape[0], shape[1], shape[2])

    def _transform(self, g, kind):
        if (g, kind) not in self._t:
            i, M = self.inp, self.shape[1] + self.shape[2]
            w = i["which"][g]
            self._t[(g, kind)] = transform(i["h"][w], i["g"][w], i["C"][g], M,
                                           np.dtype(LD if kind == "ld" else np.float64), mag=kind == "mag")
        return self._t[(g, kind)]

    def evaluate(self, g, gamma, Gamma, kind):
        """kind: 'f64', 'ld' (long double) or 'mag' (the magnitudes A)"""
        i = self.inp
        gm, hmo = self._transform(g, kind)
        return assemble(gm, hmo, gamma, Gamma, i["nuc"][g], self.shape[1], self.shape[2], i["rows"], i["cols"],
                        mag=kind == "mag")


def check_geometry(g, got, ref, mag, k, factor):
    """-> (ratios, [(geometry, quantity, element, ratio, allowed)])"""
    ratios, failures = compare(got, ref, mag, k, factor)
    return ratios, [(g,) + f for f in failures]


def unpack(out, nrdm, nk, ncas):
    """A packed output row [c0 | E | dE | gvec rows | c1 | c2] (include/oovqe.h) -> dict"""
    n_t = nrdm - 1 if nrdm > 1 else 1
    o = 2 + n_t
    d = dict(c0=out[0:1], E=out[1:2], dE=out[2:2 + nrdm - 1], gvec=out[o:o + nrdm * nk].reshape(nrdm, nk))
    o += nrdm * nk
    d["c1"] = out[o:o + ncas ** 2].reshape(ncas, ncas)
    d["c2"] = out[o + ncas ** 2:o + ncas ** 2 + ncas ** 4].reshape((ncas,) * 4)
    assert out.shape[-1] == o + ncas ** 2 + ncas ** 4
    return d
