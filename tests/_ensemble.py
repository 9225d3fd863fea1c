"""Host twin of the ensemble kernels (csrc/ensemble.hip) and the case table the CPU and the GPU tests both walk.

The twin is built on tests/_circuit_scope.py and holds nothing of the kernels: by linearity the state from a
superposition psi0_I is sum_x psi0_I[x] * apply_gates(..., init=x), tangents and second tangents likewise (``tangent``,
``second_tangent`` of that file state the rules for shared parameters, annihilation and the -1/4 block); the RDM and
transition sets come from its ``Register``; the weighted sums are plain numpy.  fp64, and ``np.longdouble`` through the
``dtype`` argument: the device tests compare against the longdouble twin rounded to fp64.

Bounds of the device tests (u = 2^-53; no figure comes from device output):

  vectors   One circuit run on a vector of norm <= 1 is off by at most es = 8 n_rot u in 2-norm (_circuit_scope.
            state_bound: orthogonal passes carry earlier errors through, a differentiated block has norm 1/2).  A vector
            that is the sum of m runs: m (es + u) + u || v ||, the last term for the rounding of the longdouble
            reference to fp64.  m = 1 for the state, the number of gates of k for tangent k, (gates of j) x (gates of k)
            for a second tangent; a vector no gate contributes to is exactly zero (bound 0).
  RDM sets  One element of one transition set is a sum of D products of two operands that are themselves sums of two
            spin terms; whatever the order of the additions (a chain per lane, then a butterfly) no term passes through
            more than D of them: (D + 2) u of the same sum with every factor by its absolute value.
            Set k adds the two transition sets (1), multiplies with w_I (1), accumulates S states (S), subtracts the
            delta term (1); with the margin of 8 that file uses and the factor 2 for the twin's own share:
                | delta set | <= 2 (D + 13 + S) u sum_I w_I ABS_I  +  carried,
            ABS_I the set of state I from absolute values.  carried: the kernel reads the DEVICE's vectors, which are
            off by e_psi and e_tau: a bilinear form b . O k moves by at most || O || (|| b || dk + || k || db + db dk)
            with || E_pq || <= 2 and || E_pq E_rs - delta_qr E_ps || <= 6 (_circuit_scope.set_input_errors).
  Hessian   H_jk = sum_I w_I sum of four bilinear forms Q(b, k) = b . Hop k: each moves by f_h Qabs(b, k) + L (|| b || dk
            + || k || db + db dk), f_h = 2 (D + 17 + S) u (four sets added instead of two), L >= || Hop ||_2
            (Register.hop_norm), Qabs with every product by its absolute value; the contraction with the coefficients
            (a one-body coefficient is c1 minus a sum of a entries of c2) and the reduction over the a^4 + a^2 elements
            add (a^4 + a^2 + a + 16) u of the sum of the Qabs.
"""
import functools

import numpy as np
import torch

from auto_oo_amd import ensemble as ENS, excitations as X
from oracle import cpu_ref as R
from tests import _circuit_scope as C
from tests import _sector_scope as S

U = C.U
LD = np.longdouble


# ---- the twin -------------------------------------------------------------------------------------------------------
def pair_list(n_theta):
    return [(j, k) for j in range(n_theta) for k in range(j, n_theta)]


def vectors(gates, n_theta, theta, n, psi0, pairs=(), dtype=np.float64):
    """[S, 1 + n_theta + len(pairs), D]: per initial vector the state, its tangents and the second tangents of
    ``pairs``, by linearity from the basis states in the support of psi0."""
    psi0 = np.asarray(psi0, dtype=dtype)
    support = np.nonzero(np.abs(psi0).max(axis=0))[0]
    nv = 1 + n_theta + len(pairs)
    out = np.zeros((psi0.shape[0], nv, 1 << n), dtype=dtype)
    for x in support:
        x = int(x)
        col = [C.apply_gates(gates, theta, n, x, (), dtype)]
        col += [C.tangent(gates, theta, n, x, k, n_theta, dtype) for k in range(n_theta)]
        col += [C.second_tangent(gates, theta, n, x, j, k, n_theta, dtype) for j, k in pairs]
        out += psi0[:, x, None, None] * np.stack(col)[None]
    return out


def ensemble_rdms(reg, vecs, w, n_tan, dtype=np.float64, use_weights=True, cross=True, absolute=False):
    """gamma_sa [1 + n_tan, a, a], Gamma_sa [1 + n_tan, a, a, a, a]: set 0 = sum_I w_I RDM(psi_I), set k = sum_I w_I
    (T(tau_I,k, psi_I) + T(psi_I, tau_I,k)).  Planted defects: ``use_weights=False`` (every weight 1 / S),
    ``cross=False`` (the term T(psi_I, tau_I,k) dropped)."""
    nS = vecs.shape[0]
    w = np.asarray(w, dtype=dtype) if use_weights else np.full(nS, 1.0 / nS, dtype=dtype)
    a = reg.ncas
    g1 = np.zeros((1 + n_tan, a, a), dtype=dtype)
    g2 = np.zeros((1 + n_tan, a, a, a, a), dtype=dtype)
    for I in range(nS):
        psi = vecs[I, 0]
        for k in range(1 + n_tan):
            if k == 0:
                t1, t2 = reg.rdms(psi, psi, absolute, dtype)
            else:
                t1, t2 = reg.rdms(vecs[I, k], psi, absolute, dtype)
                if cross:
                    s1, s2 = reg.rdms(psi, vecs[I, k], absolute, dtype)
                    t1, t2 = t1 + s1, t2 + s2
            g1[k] += w[I] * t1
            g2[k] += w[I] * t2
    return g1, g2


def transition_rdms(reg, vecs, dtype=np.float64, absolute=False):
    """[S, S, a, a], [S, S, a, a, a, a]: [I][J] = T(psi_I, psi_J)."""
    nS, a = vecs.shape[0], reg.ncas
    g1 = np.zeros((nS, nS, a, a), dtype=dtype)
    g2 = np.zeros((nS, nS, a, a, a, a), dtype=dtype)
    for I in range(nS):
        for J in range(nS):
            g1[I, J], g2[I, J] = reg.rdms(vecs[I, 0], vecs[J, 0], absolute, dtype)
    return g1, g2


def hessian(reg, vecs, w, n_theta, pairs, c1, c2, dtype=np.float64):
    """H [n_theta, n_theta] of the definition: sum_I w_I sum over T(psi_jk, psi), T(psi_j, psi_k), T(psi_k, psi_j),
    T(psi, psi_jk) of c1 . gamma + c2 . Gamma."""
    c1 = np.asarray(c1, dtype=dtype).reshape(-1)
    c2 = np.asarray(c2, dtype=dtype).reshape(-1)
    w = np.asarray(w, dtype=dtype)

    def Q(b, k):
        g1, g2 = reg.rdms(b, k, dtype=dtype)
        return c1 @ g1.reshape(-1) + c2 @ g2.reshape(-1)

    H = np.zeros((n_theta, n_theta), dtype=dtype)
    for pr, (j, k) in enumerate(pairs):
        val = dtype(0)
        for I in range(vecs.shape[0]):
            psi, tj, tk, t2 = vecs[I, 0], vecs[I, 1 + j], vecs[I, 1 + k], vecs[I, 1 + n_theta + pr]
            val = val + w[I] * (Q(t2, psi) + Q(tj, tk) + Q(tk, tj) + Q(psi, t2))
        H[j, k] = H[k, j] = val
    return H


# ---- the oracle's simulator from a superposition ----------------------------------------------------------------------
def oracle_state(name, theta, init):
    """The oracle's simulator from the superposition ``init`` through the loops of uccd_state / gatefabric_state."""
    ncas, nelecas, ansatz, kw = CIRCUITS[name]
    n = 2 * ncas
    sv = R.Statevector(n, R.hf_state(nelecas, n))
    sv.psi = torch.as_tensor(init, dtype=R.CDT).reshape([2] * n)
    if ansatz == "ucc":
        singles, doubles = R.excitations(nelecas, n)
        s_wires, d_wires = R.excitations_to_wires(singles, doubles)
        if kw.get("add_singles"):
            for i, (w1, w2) in enumerate(d_wires):
                R.fermionic_double_excitation(sv, theta[len(s_wires) + i], w1, w2)
            for j, w in enumerate(s_wires):
                R.fermionic_single_excitation(sv, theta[j], w)
        else:
            for i, (w1, w2) in enumerate(d_wires):
                R.fermionic_double_excitation(sv, theta[i], w1, w2)
        return sv.vector()
    n_layers = kw["n_layers"]
    full_shape = (n_layers, n // 2 - 1, 2)
    red = R.gatefabric_redundant_idx(ncas, nelecas)
    n_full = int(np.prod(full_shape))
    params_idx = [x for x in range(n_full) if x not in red]
    theta_full = torch.zeros(n_full, dtype=theta.dtype).index_put((torch.as_tensor(params_idx),), theta)
    theta_full = theta_full.reshape(full_shape)
    wires = list(range(n))
    blocks = [wires[i:i + 4] for i in range(0, n, 4) if i + 4 <= n]
    blocks += [wires[i:i + 4] for i in range(2, n, 4) if i + 4 <= n]
    for layer in range(n_layers):
        for i, bw in enumerate(blocks):
            R.double_excitation(sv, theta_full[layer, i, 0], bw)
            R.orbital_rotation(sv, theta_full[layer, i, 1], bw)
    return sv.vector()


# ---- bounds ---------------------------------------------------------------------------------------------------------
def vector_bounds(gates, n_theta, pairs, vecs):
    """[S, nv]: 2-norm bounds of the device's vectors against ``vecs`` (the exact ones, fp64 or longdouble)."""
    own = S.param_gates(gates, n_theta)
    es = C.state_bound(gates)
    m = [1] + [len(own[k]) for k in range(n_theta)] + [len(own[j]) * len(own[k]) for j, k in pairs]
    norms = np.linalg.norm(np.asarray(vecs, dtype=np.float64), axis=2)
    return np.array(m)[None, :] * (es + U) + U * norms * (np.array(m)[None, :] > 0)


def set_factor(D, nS):
    return 2.0 * (D + 13 + nS) * U


def rdm_bounds(reg, vecs, w, n_tan, vb):
    """bounds of gamma_sa / Gamma_sa (the kernel fed with the device's own vectors, bounds ``vb`` of vector_bounds)."""
    v64 = np.asarray(vecs, dtype=np.float64)
    a1, a2 = ensemble_rdms(reg, v64, w, n_tan, absolute=True)
    f = set_factor(reg.D, v64.shape[0])
    carried = np.zeros(1 + n_tan)
    for I in range(v64.shape[0]):
        carried += w[I] * C.set_input_errors(v64[I, 0], v64[I, 1:1 + n_tan], vb[I, 0], vb[I, 1:1 + n_tan])
    return f * a1 + 2.0 * carried[:, None, None], f * a2 + 6.0 * carried[:, None, None, None, None]


def transition_bounds(reg, vecs, vb):
    v64 = np.asarray(vecs, dtype=np.float64)
    a1, a2 = transition_rdms(reg, v64, absolute=True)
    f = set_factor(reg.D, 1)
    nrm = np.linalg.norm(v64[:, 0], axis=1)
    e = vb[:, 0]
    carried = nrm[:, None] * e[None, :] + nrm[None, :] * e[:, None] + e[:, None] * e[None, :]
    return f * a1 + 2.0 * carried[:, :, None, None], f * a2 + 6.0 * carried[:, :, None, None, None, None]


def hessian_bound(reg, vecs, w, n_theta, pairs, c1, c2, vb):
    v64 = np.asarray(vecs, dtype=np.float64)
    a = reg.ncas
    c1a = np.abs(np.asarray(c1, dtype=np.float64)).reshape(-1)
    c2a = np.abs(np.asarray(c2, dtype=np.float64)).reshape(-1)
    L = reg.hop_norm(c1, c2)
    f = 2.0 * (reg.D + 17 + v64.shape[0]) * U

    def dQ(b, db, k, dk):
        q1, q2 = reg.rdms(b, k, absolute=True)
        qabs = c1a @ q1.reshape(-1) + c2a @ q2.reshape(-1)
        nb, nk = float(np.linalg.norm(b)), float(np.linalg.norm(k))
        return f * qabs + L * (nb * dk + nk * db + db * dk), qabs

    B = np.zeros((n_theta, n_theta))
    for pr, (j, k) in enumerate(pairs):
        tot = 0.0
        for I in range(v64.shape[0]):
            v, e = v64[I], vb[I]
            p2 = 1 + n_theta + pr
            parts = [dQ(v[p2], e[p2], v[0], e[0]), dQ(v[1 + j], e[1 + j], v[1 + k], e[1 + k]),
                     dQ(v[1 + k], e[1 + k], v[1 + j], e[1 + j]), dQ(v[0], e[0], v[p2], e[p2])]
            tot += w[I] * (sum(p[0] for p in parts) + (a ** 4 + a * a + a + 16) * U * sum(p[1] for p in parts))
        B[j, k] = B[k, j] = tot
    return B


# ---- inputs ---------------------------------------------------------------------------------------------------------
def sector_indices(ncas, nelecas):
    """basis indices of the (N_alpha, N_beta) sector of the HF determinant"""
    n = 2 * ncas
    x = np.arange(1 << n)
    alpha = sum((x >> (n - 1 - 2 * p)) & 1 for p in range(ncas))
    beta = sum((x >> (n - 2 - 2 * p)) & 1 for p in range(ncas))
    return x[(alpha == (nelecas + 1) // 2) & (beta == nelecas // 2)]


def random_states(ncas, nelecas, nS, seed):
    """nS orthonormal random vectors in the sector (QR of a seeded normal matrix)."""
    idx = sector_indices(ncas, nelecas)
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((len(idx), nS)))
    out = np.zeros((nS, 1 << (2 * ncas)))
    out[:, idx] = q.T
    return out


def random_orthogonal(nS, seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).standard_normal((nS, nS)))
    return q * np.sign(np.diag(r))


# name -> (ncas, nelecas, ansatz, keyword arguments of Parameterized_circuit)
CIRCUITS = {
    "cas22_fabric1": (2, 2, "np_fabric", dict(n_layers=1)),
    "cas43_ucc": (3, 4, "ucc", dict()),
    "cas43_uccsd": (3, 4, "ucc", dict(add_singles=True)),
    "cas44_fabric2": (4, 4, "np_fabric", dict(n_layers=2)),
    "cas45_ucc": (5, 4, "ucc", dict()),
}


@functools.lru_cache(maxsize=None)
def gate_table(name):
    """(gates, n_theta) of a CIRCUITS entry, from the host-side builders (no device)."""
    ncas, nelecas, ansatz, kw = CIRCUITS[name]
    if ansatz == "ucc":
        return X.uccd_gates(ncas, nelecas, kw.get("add_singles", False))
    return X.gatefabric_gates(ncas, nelecas, kw["n_layers"])


@functools.lru_cache(maxsize=None)
def initial_states(name, kind):
    """kind: "hf" (S = 1), "singlet2", "singlet3", "random4" (four orthonormal random vectors in the sector)."""
    ncas, nelecas = CIRCUITS[name][:2]
    if kind == "hf":
        return ENS.singlet_states(ncas, nelecas, 1)
    if kind.startswith("singlet"):
        return ENS.singlet_states(ncas, nelecas, int(kind[-1]))
    return random_states(ncas, nelecas, 4, 77)


WEIGHTS = {"equal1": (1.0,), "equal2": (0.5, 0.5), "w73": (0.7, 0.3), "equal3": (1 / 3, 1 / 3, 1 / 3),
           "zero3": (0.6, 0.0, 0.4), "w4": (0.4, 0.3, 0.2, 0.1)}

# (circuit, states, weights, rows, with the second tangents and the Hessian)
KERNEL_CASES = [
    ("cas22_fabric1", "hf", "equal1", 1, True),
    ("cas22_fabric1", "singlet2", "w73", 3, True),
    ("cas22_fabric1", "singlet3", "zero3", 5, True),
    ("cas43_ucc", "singlet2", "equal2", 3, True),
    ("cas43_ucc", "random4", "w4", 1, True),
    ("cas43_uccsd", "singlet3", "equal3", 1, True),
    ("cas44_fabric2", "singlet2", "w73", 1, True),
    ("cas45_ucc", "singlet2", "equal2", 1, False),
]


def case_id(c):
    return f"{c[0]}_{c[1]}_{c[2]}_b{c[3]}"


def case_thetas(c):
    gates, n_theta = gate_table(c[0])
    return C.thetas(case_id(c), 5, n_theta)[:c[3]] if c[3] <= 5 else C.thetas(case_id(c), c[3], n_theta)


@functools.lru_cache(maxsize=None)
def reference(c, dtype=LD):
    """Everything the kernel test of case c compares with, computed once: dict(theta, psi0, w, pairs, vecs [G, S, nv, D],
    vb [G, S, nv], g1, g2, b1, b2, t1, t2, tb1, tb2, and with the Hessian c1, c2, H, HB)."""
    name, kind, wname, G, with_h = c
    ncas = CIRCUITS[name][0]
    n, reg = 2 * ncas, C.register(ncas)
    gates, n_theta = gate_table(name)
    psi0, w = initial_states(name, kind), np.array(WEIGHTS[wname])
    pairs = pair_list(n_theta) if with_h else []
    theta = case_thetas(c)
    out = dict(theta=theta, psi0=psi0, w=w, pairs=pairs, n_theta=n_theta, ncas=ncas, gates=gates)
    keys = ("vecs", "vb", "g1", "g2", "b1", "b2", "t1", "t2", "tb1", "tb2", "H", "HB")
    acc = {k: [] for k in keys}
    if with_h:
        out["c1"], out["c2"] = C.coefficients(ncas, 50 + ncas)
    for b in range(G):
        v = vectors(gates, n_theta, theta[b], n, psi0, pairs, dtype)
        vb = vector_bounds(gates, n_theta, pairs, v)
        g1, g2 = ensemble_rdms(reg, v, w, n_theta, dtype)
        b1, b2 = rdm_bounds(reg, v, w, n_theta, vb)
        t1, t2 = transition_rdms(reg, v, dtype)
        tb1, tb2 = transition_bounds(reg, v, vb)
        vals = [v, vb, g1, g2, b1, b2, t1, t2, tb1, tb2]
        if with_h:
            vals += [hessian(reg, v, w, n_theta, pairs, out["c1"], out["c2"], dtype),
                     hessian_bound(reg, v, w, n_theta, pairs, out["c1"], out["c2"], vb)]
        for k, x in zip(keys, vals):
            acc[k].append(np.asarray(x, dtype=np.float64))
    out.update({k: np.stack(x) for k, x in acc.items() if x})
    return out
