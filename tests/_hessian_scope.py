"""Shared by tests/test_hessian_scope_cpu.py and tests/test_hessian_scope_gpu.py: the host twin of the orbital-orbital
Hessian (auto_oo_amd/csrc/hessian.hip), the inputs, the case tables and the bounds of its scope tests.

The twin.  ``hessian_twin`` follows the oracle term by term (oracle/cpu_ref.py: ``full_rdms``, ``fock_generalized``,
``y_matrix``, ``analytic_hessian_from_integrals``) in numpy fp64 and uses only what makes N = 64 affordable on a CPU:
the full-space 2-RDM lives on its (occ+act)^4 block (it is zero elsewhere), so Y_pqrs needs p, r < M = n_occ + ncas and
MO integrals with two general indices only, ``J[q,s,m,n] = g_mo[q,s,m,n]`` and ``K[q,m,n,s] = g_mo[q,m,n,s]`` (m, n < M).
No symmetry of g, gam or Gam is assumed anywhere.  tests/test_hessian_scope_cpu.py holds it against the dense, untouched
oracle before the device tests rely on it.

Inputs.  h, g, S are ``synthetic_problem(N, seed)``; ``C = S^-1/2 U`` with a seeded random orthogonal U;
``nonsymmetric(g, seed)`` adds a seeded standard-normal tensor of a tenth of the root mean square of g (for the routes that
promise no symmetry only); ``rdms(ncas, seed, kind)`` are seeded standard-normal, ``"plain"`` without any index symmetry,
``"state"`` symmetrised to what a real state has (gam symmetric, Gam_pqrs = Gam_qpsr = Gam_rspq).

Bounds.  u = 2^-53.  A sum of m products computed in any order differs from the exact sum by at most m u times the same
sum over absolute values (to first order).  The longest chain of the Hessian has 4 N + M^2 + 8 products: four transforms
of N terms, one M^2 contraction, and the antisymmetriser; the bound of an element is twice (the device and the twin once
each) that many u times the twin evaluated over |h|, |g|, |C|, |gam|, |Gam| with every sign positive (``positive=True``).
Nothing in a bound comes from the code under test."""
import ctypes
import functools

import numpy as np

from auto_oo_amd import excitations, synthetic

U53 = 2.0 ** -53

# ---- the device cases: (N, n_occ, ncas, freeze_active) -----------------------------------------------------------------
# Level A, matrix and full tensor: n_kappa = 1; no core and no virtual orbital; a plain shape; ncas = 1; no virtual orbital;
# M^4 = 20736 > 64 x 256 (second trip of hess_ab_kernel), free and frozen
A_BOTH = [(2, 0, 1, False), (5, 0, 5, False), (6, 2, 2, False), (17, 7, 1, False), (12, 4, 8, False), (16, 4, 8, False),
          (16, 4, 8, True)]
A_MATRIX = [(64, 24, 8, False)]                       # n_kappa = 1244: 1,547,536 elements, second trip of hess_matrix_kernel
A_FULL = [(38, 4, 3, False), (39, 4, 3, False)]       # N^4 = 2,085,136 (one trip of hess_full_kernel) | 2,313,441 (two)
# Level B (G = 3): MT = 4 > N | M = 4|5 | M = 8|9, a one-row tail | M = 12|13, no tail | N M = 512, 64 KB | N M = 528 above
# 64 KB | N M = 528 below it | the limit | the first shapes off t2k_tri_kernel by N and by M
B_CASES = [(2, 0, 1), (3, 1, 1), (6, 2, 2), (7, 2, 3), (17, 7, 1), (17, 6, 3), (16, 4, 8), (20, 5, 8), (32, 8, 8),
           (33, 8, 8), (48, 3, 8), (48, 8, 8), (49, 8, 8), (24, 9, 8)]
B_NONSYMMETRIC = [(17, 6, 3), (33, 8, 8)]
C_CASES = [(13, 6, 3), (20, 5, 8), (64, 24, 8)]
C_BATCH = (33, 13, 3)                                 # 30 electrons, four of them active: M = 16, N M = 528
FOCK_CASES = [(2, 0, 1), (5, 0, 5), (17, 7, 1), (64, 24, 8)]
# the shapes at which the dense N^6 einsums of the oracle take under a second
CPU_CASES = [(2, 0, 1, False), (5, 0, 5, False), (6, 2, 2, False), (9, 3, 3, False), (9, 3, 3, True), (12, 4, 8, False)]


def device_cases():
    """Every (N, n_occ, ncas, freeze_active) that a device test runs."""
    out = list(A_BOTH) + list(A_MATRIX) + list(A_FULL)
    out += [c + (False,) for c in B_CASES + C_CASES + [C_BATCH]]
    return out


def t2k_route(N, M):
    """Whether ``t2k_tri_kernel`` serves a stack with p <-> q symmetric integrals (hessian.hip: ``vk_tri``)."""
    return N <= 48 and M <= 16 and M * M * N * 8 <= 150 * 1024


def t2k_lds_bytes(N, M):
    return M * M * N * 8


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def seed_of(N, n_occ, ncas, k=0):
    return 70000 + 1000 * N + 31 * n_occ + 7 * ncas + 97 * k


@functools.lru_cache(maxsize=4)
def problem(N, seed):
    """(h, g, S, C) of ``synthetic_problem(N, seed)`` with ``C = S^-1/2 U``, U a seeded random orthogonal matrix."""
    P = synthetic.synthetic_problem(N, seed)
    S = 0.5 * (P["overlap"] + P["overlap"].T)
    s, V = np.linalg.eigh(S)
    U, _ = np.linalg.qr(np.random.default_rng(seed + 1).standard_normal((N, N)))
    C = (V * s ** -0.5) @ V.T @ U
    return P["int1e_ao"], P["int2e_ao"], S, U, C


def nonsymmetric(g, seed):
    """g plus a seeded standard-normal tensor of a tenth of the root mean square of g: no index symmetry left."""
    return g + 0.1 * np.sqrt(np.mean(g * g)) * np.random.default_rng(seed + 2).standard_normal(g.shape)


def rdms(ncas, seed, kind):
    """Seeded standard-normal (gam, Gam): ``"plain"`` without any index symmetry, ``"state"`` with gam symmetric and
    Gam_pqrs = Gam_qpsr = Gam_rspq."""
    rng = np.random.default_rng(seed + 3)
    gam = rng.standard_normal((ncas,) * 2)
    Gam = rng.standard_normal((ncas,) * 4)
    if kind == "state":
        gam = 0.5 * (gam + gam.T)
        Gam = 0.25 * (Gam + Gam.transpose(1, 0, 3, 2) + Gam.transpose(2, 3, 0, 1) + Gam.transpose(3, 2, 1, 0))
    else:
        assert kind == "plain"
    return gam, Gam


def kappa_tables(N, n_occ, ncas, freeze_active):
    """(rows, cols) int32 of the non-redundant rotations in the order of the kappa vector."""
    occ, act, virt = np.arange(n_occ), n_occ + np.arange(ncas), np.arange(n_occ + ncas, N)
    idx = excitations.non_redundant_indices(occ, act, virt, freeze_active)
    return excitations.tril_tables(N, idx)


# ---- the twin -------------------------------------------------------------------------------------------------------------
_MEMO = []          # the last two results of _parts: (key, the input arrays themselves, result)


def _parts(h_ao, g_ao, C, gam, Gam, n_occ, ncas, positive, dtype):
    """``_parts_of``, kept for the last two sets of arguments (the same array OBJECTS, which no caller writes into):
    ``fock_twin``, ``hessian_twin`` and the bounds of one case share the integral transforms."""
    arrays = (h_ao, g_ao, C, gam, Gam)
    key = (tuple(id(x) for x in arrays), n_occ, ncas, bool(positive), np.dtype(dtype).name)
    for k, _, value in _MEMO:
        if k == key:
            return value
    value = _parts_of(*arrays, n_occ, ncas, positive, dtype)
    _MEMO.append((key, arrays, value))
    del _MEMO[:-2]
    return value


def _parts_of(h_ao, g_ao, C, gam, Gam, n_occ, ncas, positive, dtype):
    """(h_mo [N,N], J [N,N,M,M], K [N,M,M,N], D1 [M,M], D [M,M,M,M], F [N,N]) of the twin.  ``positive``: every input by
    its absolute value and every sign positive."""
    sg = 1.0 if positive else -1.0
    cast = (lambda x: np.abs(np.asarray(x, dtype=dtype))) if positive else (lambda x: np.asarray(x, dtype=dtype))
    h, g, C, gam, Gam = (cast(x) for x in (h_ao, g_ao, C, gam, Gam))
    N, M = C.shape[0], n_occ + ncas
    o, a = slice(0, n_occ), slice(n_occ, M)
    Cm, td, e = C[:, :M], np.tensordot, np.einsum
    h_mo = C.T @ h @ C
    # J[q,s,m,n] = g_mo[q,s,m,n]: the two restricted indices first
    x = td(g, Cm, axes=([3], [0]))                          # p q r n
    x = td(x, Cm, axes=([2], [0]))                          # p q n m
    x = td(x, C, axes=([1], [0]))                           # p n m s
    x = td(x, C, axes=([0], [0]))                           # n m s q
    J = np.ascontiguousarray(x.transpose(3, 2, 1, 0))
    # K[q,m,n,s] = g_mo[q,m,n,s]
    x = td(g, Cm, axes=([1], [0]))                          # p r s m
    x = td(x, Cm, axes=([1], [0]))                          # p s m n
    x = td(x, C, axes=([1], [0]))                           # p m n s
    x = td(x, C, axes=([0], [0]))                           # m n s q
    K = np.ascontiguousarray(x.transpose(3, 0, 1, 2))
    # full_rdms on the (occ+act)^4 block
    eye = np.eye(n_occ, dtype=dtype)
    D1 = np.zeros((M, M), dtype=dtype)
    D1[o, o] = 2.0 * eye
    D1[a, a] = gam
    D = np.zeros((M,) * 4, dtype=dtype)
    D[o, o, o, o] = 4.0 * e("ij,kl->ijkl", eye, eye) + sg * 2.0 * e("il,jk->ijkl", eye, eye)
    D[o, o, a, a] = 2.0 * e("wv,ij->ijwv", gam, eye)
    D[a, a, o, o] = 2.0 * e("wv,ij->wvij", gam, eye)
    D[o, a, a, o] = sg * e("wv,ij->iwvj", gam, eye)
    D[a, o, o, a] = sg * e("wv,ij->vjiw", gam, eye)
    D[a, a, a, a] = Gam
    # fock_core, fock_active, fock_generalized
    FC = h_mo + 2.0 * e("qsii->qs", J[:, :, o, o]) + sg * e("qiis->qs", K[:, o, o, :])
    FA = e("vw,mnvw->mn", gam, J[:, :, a, a]) + sg * 0.5 * e("vw,mwvn->mn", gam, K[:, a, a, :])
    F = np.zeros((N, N), dtype=dtype)
    F[o, :] = 2.0 * (FC[:, o] + FA[:, o]).T
    F[a, :] = e("nw,vw->vn", FC[:, a], gam) + e("vwxy,nwxy->vn", Gam, K[:, a, a, a])
    return h_mo, J, K, D1, D, F


def fock_twin(h_ao, g_ao, C, gam, Gam, n_occ, ncas, positive=False, dtype=np.float64):
    """The generalized Fock matrix [N, N] (rows >= n_occ + ncas are zero), ``fock_generalized`` of the oracle."""
    return _parts(h_ao, g_ao, C, gam, Gam, n_occ, ncas, positive, dtype)[5]


def hessian_twin(h_ao, g_ao, C, gam, Gam, n_occ, ncas, rows=None, cols=None, positive=False, dtype=np.float64):
    """The orbital-orbital Hessian: the full [N,N,N,N] tensor, or with ``rows``, ``cols`` the gather
    ``H[rows[t1], cols[t1], rows[t2], cols[t2]]`` of it (``full_hessian_to_matrix``)."""
    sg = 1.0 if positive else -1.0
    h_mo, J, K, D1, D, F = _parts(h_ao, g_ao, C, gam, Gam, n_occ, ncas, positive, dtype)
    N, M = C.shape[0], n_occ + ncas
    m2, n2 = M * M, N * N
    # y_matrix: Y[p,r,q,s] = sum_mn [(D_pmrn + D_pmnr) K_qmns + D_prmn J_qsmn]
    A = (D.transpose(0, 2, 1, 3) + D.transpose(0, 3, 1, 2)).reshape(m2, m2)
    Y = A @ K.transpose(1, 2, 0, 3).reshape(m2, n2) + D.reshape(m2, m2) @ J.transpose(2, 3, 0, 1).reshape(m2, n2)
    Y = Y.reshape(M, M, N, N)
    D1f = np.zeros((N, N), dtype=dtype)
    D1f[:M, :M] = D1
    Fs = F + F.T

    def x(P, Q, R, S):
        # 2 gam_pr h_qs - (F_pr + F_rp) delta_qs + 2 Y_pqrs
        inside = (P < M) & (R < M)
        y = np.where(inside, Y[np.where(P < M, P, 0), np.where(R < M, R, 0), Q, S], 0.0)
        return 2.0 * D1f[P, R] * h_mo[Q, S] + sg * Fs[P, R] * (Q == S) + 2.0 * y

    if rows is None:
        # the dense tensor as the oracle forms it (the same sums in the same order as x, without index gathers)
        eye = np.eye(N, dtype=dtype)
        h0 = 2.0 * D1f[:, None, :, None] * h_mo[None, :, None, :] + sg * Fs[:, None, :, None] * eye[None, :, None, :]
        h0[:M, :, :M, :] += 2.0 * Y.transpose(0, 2, 1, 3)
        return h0 + sg * h0.transpose(0, 1, 3, 2) + sg * h0.transpose(1, 0, 2, 3) + h0.transpose(1, 0, 3, 2)
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    P, Q, R, S = rows[:, None], cols[:, None], rows[None, :], cols[None, :]
    return x(P, Q, R, S) + sg * x(P, Q, S, R) + sg * x(Q, P, R, S) + x(Q, P, S, R)


def products(N, M):
    """The number of products in the longest chain: four transforms, one M^2 contraction, the antisymmetriser."""
    return 4 * N + M * M + 8


def hessian_bound(h_ao, g_ao, C, gam, Gam, n_occ, ncas, rows=None, cols=None):
    """Per element: 2 (4 N + M^2 + 8) u times the twin over absolute values with every sign positive."""
    Habs = hessian_twin(h_ao, g_ao, C, gam, Gam, n_occ, ncas, rows, cols, positive=True)
    return 2.0 * products(C.shape[0], n_occ + ncas) * U53 * Habs


def fock_bound(h_ao, g_ao, C, gam, Gam, n_occ, ncas):
    """As ``hessian_bound`` for the generalized Fock matrix (its chains are shorter than the Hessian's)."""
    Fabs = fock_twin(h_ao, g_ao, C, gam, Gam, n_occ, ncas, positive=True)
    return 2.0 * products(C.shape[0], n_occ + ncas) * U53 * Fabs


def share(err, bound):
    """The largest share of its bound that an element's error takes (0 / 0 = 0)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0.0, 0.0, np.asarray(err) / np.asarray(bound))
    return float(np.max(r))


# ---- fock_core and fock_active of the oracle in numpy (MO integrals in, no symmetry assumed) ---------------------------
def fock_core_active_host(h_mo, g_mo, gam, n_occ, ncas, positive=False):
    """(fock_core, fock_active): ``h + sum_i (2 g_mnii - g_miin)`` and ``sum_vw gam_vw (g_mnvw - g_mwvn / 2)``."""
    sg = 1.0 if positive else -1.0
    if positive:
        h_mo, g_mo, gam = np.abs(h_mo), np.abs(g_mo), np.abs(gam)
    o, a = slice(0, n_occ), slice(n_occ, n_occ + ncas)
    core = h_mo + 2.0 * np.einsum("mnii->mn", g_mo[:, :, o, o]) + sg * np.einsum("miin->mn", g_mo[:, o, o, :])
    active = (np.einsum("vw,mnvw->mn", gam, g_mo[:, :, a, a])
              + sg * 0.5 * np.einsum("vw,mwvn->mn", gam, g_mo[:, a, a, :]))
    return core, active


def fock_core_active_bounds(h_mo, g_mo, gam, n_occ, ncas):
    """Per element 2 (2 n_occ + 2) u and 2 (2 ncas^2 + 1) u times the expressions over absolute values: the number of
    terms of each sum (the factors 2 and 1/2 are exact), the device and the host once each."""
    core, active = fock_core_active_host(h_mo, g_mo, gam, n_occ, ncas, positive=True)
    return 2.0 * (2 * n_occ + 2) * U53 * core, 2.0 * (2 * ncas * ncas + 1) * U53 * active


# ---- the device side (imported by the GPU tests only) ------------------------------------------------------------------
def to_dev(x, dtype=None):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


def hessian_batch_rc(g, h, C, gam, Gam, fock, N, n_occ, ncas, rows, cols, n_kappa, batch, work, H, eri_flags):
    """The return code of ``oovqe_orbital_hessian_batch``, called the way auto_oo_amd/batch.py calls it (device tensors,
    None = a null pointer)."""
    import torch
    from auto_oo_amd import _lib
    d = _lib.dptr
    return _lib.load().oovqe_orbital_hessian_batch(
        d(g), d(h), d(C), d(gam), d(Gam), d(fock), N, n_occ, ncas, d(rows, torch.int32), d(cols, torch.int32),
        n_kappa, batch, d(work), d(H), ctypes.c_uint(int(eri_flags)), _lib.stream_ptr())


def hessian_batch(g, h, C, gam, Gam, fock, n_occ, ncas, rows, cols, eri_flags):
    """[G, n_kappa, n_kappa] of ``oovqe_orbital_hessian_batch`` for stacks g [G,N,N,N,N], h, C, fock [G,N,N],
    gam [G,a,a], Gam [G,a,a,a,a] on the device."""
    import torch
    from auto_oo_amd import _lib
    G, N = C.shape[0], C.shape[-1]
    nk = rows.numel()
    wsz = _lib.load().oovqe_orbital_hessian_work_size(N, n_occ, ncas)
    work = torch.empty(G * wsz, dtype=torch.float64, device=C.device)
    H = torch.empty((G, nk, nk), dtype=torch.float64, device=C.device)
    _lib.check(hessian_batch_rc(g, h, C, gam, Gam, fock, N, n_occ, ncas, rows, cols, nk, G, work, H, eri_flags),
               "oovqe_orbital_hessian_batch")
    torch.cuda.synchronize()
    return H
