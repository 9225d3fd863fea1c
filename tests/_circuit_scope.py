"""Host twin of the dense-register circuit and RDM kernels (csrc/circuit.hip, csrc/circuit_small.h,
csrc/spin_rdms.hip) for the whole-scope tests: numpy fp64, and ``np.longdouble`` through the ``dtype`` argument of every
routine, written from the definitions alone -- the gate table of include/oovqe.h on the full 2^n register, E_pq and
a^+_p a^+_q a_r a_s from Jordan-Wigner ladder operators, the transition RDMs and their derivative sets by the product
rule, H_jk from the twin's own states -- with none of the kernels' devices (no ``deposit``, no MFMA Gram layout, no
V[pq] staging order).  Wire j is bit n-1-j; spin orbital 2p is the alpha, 2p+1 the beta orbital of p.

Also here: the bounds of the device tests (no figure in them comes from device output; derivation in DESIGN.md, "The
dense-register kernels over their whole scope") and the case tables the CPU and the GPU tests both walk."""
import functools

import numpy as np

from auto_oo_amd import excitations as X
from tests import _sector_scope as S

U = 2.0 ** -53
LD = np.longdouble
TWO_PI = 2.0 * np.pi


# ---- the gate table on the full register ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bits(n):
    """(x, popcount table) of the n-qubit register."""
    x = np.arange(1 << n, dtype=np.int64)
    pc = np.zeros(1 << n, dtype=np.int64)
    for i in range(n):
        pc += (x >> i) & 1
    return x, pc


def apply_gates(gates, theta, n, init, deriv=(), dtype=np.float64, annihilate=True):
    """psi [2^n] of the gate table: selection (x & (hi|lo)) == hi, partner x ^ (hi|lo), sign popcount(x & mask_par),
    angle sign * theta / 2, gates with theta_idx < 0 skipped.  ``deriv``: up to two gate indices to differentiate --
    once: the 2 x 2 block becomes its derivative, twice (the same gate): -1/4 of the block; either way the gate
    annihilates the amplitudes it would leave alone (the derivative of an identity block).  ``annihilate=False`` is
    the planted defect of tests/test_circuit_scope_cpu.py."""
    x, pc = _bits(n)
    psi = np.zeros(1 << n, dtype=dtype)
    psi[init] = 1
    theta = np.asarray(theta, dtype=dtype)
    deriv = [g for g in deriv if g >= 0]
    for gi, g in enumerate(gates):
        if g.theta_idx < 0:
            continue
        hi, lo, par = int(g.mask_hi), int(g.mask_lo), int(g.mask_par)
        fm = hi | lo
        sel = x[(x & fm) == hi]
        y = sel ^ fm
        pi = np.where((pc[sel & par] & 1) == 1, -1, 1).astype(dtype)
        half = dtype(0.5 * g.sign)
        ang = half * theta[g.theta_idx]
        c, s = np.cos(ang), np.sin(ang)
        order = deriv.count(gi)
        if order == 1:
            c, s = -half * s, half * c
        elif order == 2:
            c, s = dtype(-0.25) * c, dtype(-0.25) * s
        ax, ay = psi[sel].copy(), psi[y].copy()
        if order and annihilate:
            psi = np.zeros(1 << n, dtype=dtype)
        psi[sel] = c * ax + pi * s * ay
        psi[y] = c * ay - pi * s * ax
    return psi


def tangent(gates, theta, n, init, k, n_theta, dtype=np.float64, first_only=False, annihilate=True):
    """d psi / d theta_k: the sum over the gates parameter k drives (exactly zero if it drives none).
    ``first_only``: the planted defect (the term of the first gate alone)."""
    own = S.param_gates(gates, n_theta)[k]
    out = np.zeros(1 << n, dtype=dtype)
    for g in (own[:1] if first_only else own):
        out = out + apply_gates(gates, theta, n, init, (g,), dtype, annihilate)
    return out


def second_tangent(gates, theta, n, init, j, k, n_theta, dtype=np.float64):
    own = S.param_gates(gates, n_theta)
    out = np.zeros(1 << n, dtype=dtype)
    for g in own[j]:
        for h in own[k]:
            out = out + apply_gates(gates, theta, n, init, (g, h), dtype)
    return out


# ---- Jordan-Wigner ladder operators --------------------------------------------------------------------------------
def ladder(x, j, n, create):
    """a_j (a^+_j with ``create``) on the basis indices x -> (indices, signs, alive): the phase is the parity of the
    occupied modes k < j, which sit on the higher bits."""
    _, pc = _bits(n)
    bit = 1 << (n - 1 - j)
    alive = ((x & bit) != 0) != create
    before = ((1 << n) - 1) & ~((bit << 1) - 1)
    sign = np.where((pc[x & before] & 1) == 1, -1, 1)
    return x ^ bit, sign, alive


class Register:
    """E_pq = a^+_{2p} a_{2q} + a^+_{2p+1} a_{2q+1} on the 2^(2 ncas) register."""

    def __init__(self, ncas):
        self.ncas, self.n, self.D = ncas, 2 * ncas, 1 << (2 * ncas)
        self._epq = None

    def epq(self):
        """(src, sign) [a, a, 2, D]: (E_pq v)[y] = sum_spin sign[p, q, spin, y] v[src[p, q, spin, y]] (sign 0 where
        the term is absent)."""
        if self._epq is None:
            a, n = self.ncas, self.n
            x, _ = _bits(n)
            src = np.zeros((a, a, 2, self.D), dtype=np.int64)
            sign = np.zeros((a, a, 2, self.D), dtype=np.int64)
            for p in range(a):
                for q in range(a):
                    for sp in (0, 1):
                        x1, s1, ok1 = ladder(x, 2 * q + sp, n, False)
                        x1 = np.where(ok1, x1, 0)
                        y, s2, ok2 = ladder(x1, 2 * p + sp, n, True)
                        ok = ok1 & ok2
                        src[p, q, sp, y[ok]] = x[ok]
                        sign[p, q, sp, y[ok]] = (s1 * s2)[ok]
            self._epq = (src, sign)
        return self._epq

    def apply_epq(self, v, absolute=False, jw=True):
        """V [a^2, D] = E_pq v.  ``absolute``: every sign and amplitude by its absolute value; ``jw=False``: the
        planted defect (no Jordan-Wigner sign)."""
        src, sign = self.epq()
        if absolute or not jw:
            sign = np.abs(sign)
        if absolute:
            v = np.abs(v)
        sign = sign.astype(v.dtype)
        return (sign[:, :, 0] * v[src[:, :, 0]] + sign[:, :, 1] * v[src[:, :, 1]]).reshape(-1, self.D)

    def apply_epq_rows_abs(self, W):
        """sum_pq |E_pq| W_pq for W [a^2, D] >= 0."""
        src, sign = self.epq()
        a2 = self.ncas ** 2
        sign = np.abs(sign).astype(W.dtype).reshape(a2, 2, self.D)
        src = src.reshape(a2, 2, self.D)
        rows = np.arange(a2)[:, None]
        return (sign[:, 0] * W[rows, src[:, 0]] + sign[:, 1] * W[rows, src[:, 1]]).sum(axis=0)

    def rdms(self, bra, ket, absolute=False, dtype=np.float64, jw=True, swap=False, delta=True):
        """transition RDMs gamma[p, q] = bra . E_pq ket, Gamma[p, q, r, s] = (E_qp bra) . (E_rs ket) - delta_qr
        gamma[p, s].  Planted defects: ``jw=False``, ``swap`` (E_pq bra in place of E_qp bra), ``delta=False``."""
        a = self.ncas
        bra, ket = np.asarray(bra, dtype=dtype), np.asarray(ket, dtype=dtype)
        Vb, Vk = self.apply_epq(bra, absolute, jw), self.apply_epq(ket, absolute, jw)
        gamma = (Vk @ (np.abs(bra) if absolute else bra)).reshape(a, a)
        if not swap:
            Vb = Vb.reshape(a, a, -1).transpose(1, 0, 2).reshape(a * a, -1)        # row pq = E_qp bra
        Gamma = (Vb @ Vk.T).reshape(a, a, a, a)
        if delta:
            for q in range(a):
                if absolute:
                    Gamma[:, q, q, :] += gamma
                else:
                    Gamma[:, q, q, :] -= gamma
        return gamma, Gamma

    def rdms_tangent(self, psi, dpsi, absolute=False, dtype=np.float64, **defect):
        """the sets of oovqe_rdms_tangent: set 0 the RDMs of psi, set k the product rule T(dpsi_k, psi) +
        T(psi, dpsi_k) of the bilinear transition RDMs T.  -> (gamma [1 + n_tan, a, a], Gamma [1 + n_tan, a, a, a, a])"""
        g1, g2 = [], []
        for k in range(1 + len(dpsi)):
            if k == 0:
                a1, a2 = self.rdms(psi, psi, absolute, dtype, **defect)
            else:
                b1, b2 = self.rdms(dpsi[k - 1], psi, absolute, dtype, **defect)
                c1, c2 = self.rdms(psi, dpsi[k - 1], absolute, dtype, **defect)
                a1, a2 = b1 + c1, b2 + c2
            g1.append(a1)
            g2.append(a2)
        return np.stack(g1), np.stack(g2)

    # ---- the operator norm of Hop = sum c1_pq E_pq + sum c2_pqrs (E_pq E_rs - delta_qr E_ps) -------------------------
    def hop_norm(self, c1, c2):
        """|| Hop ||_2 <= sqrt(largest absolute row sum x largest absolute column sum), with |E_pq|^T = |E_qp|."""
        a = self.ncas
        c1 = np.abs(np.asarray(c1, dtype=np.float64)).reshape(a * a)
        c2 = np.abs(np.asarray(c2, dtype=np.float64)).reshape(a, a, a, a)
        A = self.apply_epq(np.ones(self.D), absolute=True)                          # A_pq = |E_pq| 1
        At = A.reshape(a, a, -1).transpose(1, 0, 2).reshape(a * a, -1)              # row pq = A_qp
        d = np.einsum("pqqs->ps", c2).reshape(-1)
        C2 = c2.reshape(a * a, a * a)
        rows = c1 @ A + self.apply_epq_rows_abs(C2 @ A) + d @ A
        Wt = (C2.T @ At).reshape(a, a, -1).transpose(1, 0, 2).reshape(a * a, -1)    # row sr = sum_pq c2_pqrs A_qp
        cols = c1 @ At + self.apply_epq_rows_abs(Wt) + d @ At
        return float(np.sqrt(rows.max() * cols.max()))


@functools.lru_cache(maxsize=None)
def register(ncas):
    return Register(ncas)


def spin_rdms(bra, ket, n, absolute=False, dtype=np.float64, jw=True):
    """gamma[p, q] = bra . a^+_p a_q ket, Gamma[p, q, r, s] = bra . a^+_p a^+_q a_r a_s ket over the n spin orbitals
    (``jw=False``: the planted defect, no Jordan-Wigner sign)."""
    x, _ = _bits(n)
    bra, ket = np.asarray(bra, dtype=dtype), np.asarray(ket, dtype=dtype)
    if absolute:
        bra, ket = np.abs(bra), np.abs(ket)
    one = np.zeros((n, n), dtype=dtype)
    two = np.zeros((n, n, n, n), dtype=dtype)

    def step(state, j, create):
        xs, sg, ok = state
        y, s, alive = ladder(np.where(ok, xs, 0), j, n, create)
        return y, sg * s, ok & alive

    def close(state):
        y, sg, ok = state
        w = np.ones(len(y), dtype=dtype) if (absolute or not jw) else sg.astype(dtype)
        return (bra[y[ok]] * w[ok] * ket[ok]).sum()

    start = (x, np.ones(1 << n, dtype=np.int64), np.ones(1 << n, dtype=bool))
    for s in range(n):
        ks = step(start, s, False)
        for p in range(n):
            one[p, s] = close(step(ks, p, True))
        for r in range(n):
            kr = step(ks, r, False)
            if not kr[2].any():
                continue
            for q in range(n):
                kq = step(kr, q, True)
                for p in range(n):
                    two[p, q, r, s] = close(step(kq, p, True))
    return one, two


def spin_summed(one, two):
    """restricted RDMs from the spin-orbital ones: gamma[p, q] = sum_s one[2p+s, 2q+s], Gamma[p, q, r, s] =
    sum_{s t} two[2p+s, 2r+t, 2s+t, 2q+s]  (E_pq E_rs - delta_qr E_ps = sum a^+_{p s} a^+_{r t} a_{s t} a_{q s})."""
    a = one.shape[0] // 2
    g1 = np.zeros((a, a), dtype=one.dtype)
    g2 = np.zeros((a, a, a, a), dtype=one.dtype)
    for p in range(a):
        for q in range(a):
            g1[p, q] = one[2 * p, 2 * q] + one[2 * p + 1, 2 * q + 1]
            for r in range(a):
                for s in range(a):
                    g2[p, q, r, s] = sum(two[2 * p + sg, 2 * r + t, 2 * s + t, 2 * q + sg]
                                         for sg in (0, 1) for t in (0, 1))
    return g1, g2


# ---- the theta-theta Hessian of E = c1 . gamma + c2 . Gamma ---------------------------------------------------------
def hessian(gates, theta, ncas, init, c1, c2, n_theta, dtype=np.float64, bound=False, tangent_defect=None,
            rdm_defect=None):
    """H_jk = Q(psi_jk, psi) + Q(psi_j, psi_k) + Q(psi_k, psi_j) + Q(psi, psi_jk), Q(b, k) = c1 . gamma(b, k) +
    c2 . Gamma(b, k) bilinear, from the twin's own states.  ``bound``: also the bound of the device test,

        | delta Q(b, k) | <= |c1| . B_gamma + |c2| . B_Gamma + L (|| b || dk + || k || db + db dk)
        | delta H_jk |    <= sum of the four + (4 (a^4 + a^2) + 8) u sum of the four Qabs(b, k)

    B the RDM bounds, L >= || Hop ||_2, db / dk the state and tangent bounds (m gates: m e_s + u || tau ||; a pair
    of parameters with m_j and m_k gates: m_j m_k e_s + u || tau_jk ||), Qabs with every product by its absolute
    value; the last term is the one reduction over the 4 (a^4 + a^2) products of a pair."""
    reg, n = register(ncas), 2 * ncas
    c1 = np.asarray(c1, dtype=dtype).reshape(-1)
    c2 = np.asarray(c2, dtype=dtype).reshape(-1)
    own = S.param_gates(gates, n_theta)
    psi = apply_gates(gates, theta, n, init, (), dtype)
    tau = [tangent(gates, theta, n, init, k, n_theta, dtype, **(tangent_defect or {})) for k in range(n_theta)]
    H = np.zeros((n_theta, n_theta), dtype=dtype)
    B = np.zeros((n_theta, n_theta))
    if bound:
        es = state_bound(gates)
        d1 = [len(own[k]) * es + U * float(np.linalg.norm(tau[k])) for k in range(n_theta)]
        L = reg.hop_norm(c1, c2)
        a = ncas
        c1a, c2a = np.abs(c1), np.abs(c2)

    def Q(b, k):
        g1, g2 = reg.rdms(b, k, dtype=dtype, **(rdm_defect or {}))
        return c1 @ g1.reshape(-1) + c2 @ g2.reshape(-1)

    def dQ(b, db, k, dk):
        q1, q2 = reg.rdms(b, k, absolute=True)
        qabs = c1a @ q1.reshape(-1) + c2a @ q2.reshape(-1)
        f = 2.0 * (reg.D + 2 + 8) * U
        nb, nk = float(np.linalg.norm(b)), float(np.linalg.norm(k))
        return f * qabs + L * (nb * dk + nk * db + db * dk), qabs

    for j in range(n_theta):
        for k in range(j, n_theta):
            t2 = second_tangent(gates, theta, n, init, j, k, n_theta, dtype)
            H[j, k] = H[k, j] = Q(t2, psi) + Q(tau[j], tau[k]) + Q(tau[k], tau[j]) + Q(psi, t2)
            if bound:
                d2 = len(own[j]) * len(own[k]) * es + U * float(np.linalg.norm(t2))
                parts = [dQ(t2, d2, psi, es), dQ(tau[j], d1[j], tau[k], d1[k]), dQ(tau[k], d1[k], tau[j], d1[j]),
                         dQ(psi, es, t2, d2)]
                B[j, k] = B[k, j] = sum(p[0] for p in parts) \
                    + (4 * (a ** 4 + a * a) + 8) * U * sum(p[1] for p in parts)
    return (H, B) if bound else H


# ---- bounds --------------------------------------------------------------------------------------------------------
def state_bound(gates):
    """|| psi_dev - psi ||_2 <= 8 n_rot u (|| psi || <= 1): _sector_scope.state_bound on the whole register."""
    return 8.0 * S.n_rotations(gates) * U


def tangent_bound(gates, m, tau):
    """a tangent summed over m differentiated circuits: m state bounds + u || tau || for the sum."""
    return m * state_bound(gates) + U * float(np.linalg.norm(np.asarray(tau, dtype=np.float64)))


def rdm_factor(D):
    """2 (n + 8) u, n = D + 2 products per Gram element (V is a sum of two spin terms): one share for the device's
    summation order, one for the fp64 twin's own."""
    return 2.0 * (D + 2 + 8) * U


def rdm_bounds(reg, bra, ket):
    g1, g2 = reg.rdms(bra, ket, absolute=True)
    f = rdm_factor(reg.D)
    return f * g1, f * g2


def rdm_tangent_bounds(reg, psi, dpsi):
    g1, g2 = reg.rdms_tangent(psi, dpsi, absolute=True)
    f = rdm_factor(reg.D)
    return f * g1, f * g2


def set_input_errors(psi, dpsi, es, tb):
    """the RDM sets of oovqe_circuit_rdms are formed from the DEVICE's state and tangents, which are off the twin's
    by es and tb[k] in 2-norm: a bilinear form b . O k moves by at most || O || (|| b || dk + || k || db + db dk),
    || E_pq || <= 2, || E_pq E_rs - delta_qr E_ps || <= 6.  -> the bracket per set [1 + n_theta]: set 0 is
    psi . O psi, set k is tau_k . O psi + psi . O tau_k."""
    npsi = float(np.linalg.norm(np.asarray(psi, dtype=np.float64)))
    out = [2.0 * npsi * es + es * es]
    for k in range(len(dpsi)):
        nt = float(np.linalg.norm(np.asarray(dpsi[k], dtype=np.float64)))
        out.append(2.0 * (nt * es + npsi * tb[k] + es * tb[k]))
    return np.array(out)


def spin_rdm_bounds(bra, ket, n):
    g1, g2 = spin_rdms(bra, ket, n, absolute=True)
    f = rdm_factor(1 << n)
    return f * g1, f * g2


# ---- inputs --------------------------------------------------------------------------------------------------------
def dense_vector(D, seed):
    """not normalised, every amplitude non-zero."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(D)
    return np.where(np.abs(v) < 0.05, 0.05, v) * rng.choice([0.5, 1.0, 3.0])


def patterned_vector(D, seed):
    """exact zeros at every index with x % 3 == 2, from 6 qubits on also where bit 1 is set (2 amplitudes: at 0)."""
    v = dense_vector(D, seed)
    x = np.arange(D)
    zero = (x % 3 == 2) if D > 2 else (x == 0)
    if D >= 64:
        zero |= (x >> 1) & 1 == 1
    v[zero] = 0.0
    return v


def basis_vector(D, seed):
    v = np.zeros(D)
    v[np.random.default_rng(seed).integers(D)] = -1.75
    return v


def make_vectors(D, seed, n):
    """n vectors of the whole register: dense, with exact zeros, one basis state, then dense ones."""
    makers = [dense_vector, patterned_vector, basis_vector]
    return np.stack([(makers[i] if i < 3 else dense_vector)(D, seed + 17 * i) for i in range(n)])


def make_pairs(D, seed, n, same):
    """(bra, ket) [n, D]; bra != ket: the kets are other vectors, one kind further on (the dense bra meets the
    vector with zeros, the basis state a dense vector).  The first m pairs of n are the m pairs of (D, seed, m)."""
    bra = make_vectors(D, seed, n)
    if same:
        return bra, bra.copy()
    return bra, make_vectors(D, seed + 1000, n + 1)[1:]


def coefficients(ncas, seed):
    return S.coefficients(ncas, seed)


# ---- gate lists ----------------------------------------------------------------------------------------------------
def _hf(nelec, n):
    return X.basis_index(X.hf_state(nelec, n))


def hand_gates(n):
    """a hand-made list for any register: both signs, nfix 2 and (n >= 4) 4, fixed bits at bit 0 and at bit n-1,
    parity masks spanning the register, parameter 0 driving three non-adjacent gates, parameter 2 driving none, one
    gate with theta_idx = -1, and two gates that do not conserve the number of set bits (mask_lo = 0), so that the
    start indices 0 and D-1 move as well."""
    top, b0 = 1 << (n - 1), 1
    mid = (top - 1) & ~1
    nxt = top >> 1 if n >= 3 else b0
    G = [X._gate(top | b0, 0, mid, 1, +1),
         X._gate(top, b0, mid, 0, +1),
         X._gate(2, 1, 0, 3, -1) if n >= 3 else X._gate(b0, top, 0, 3, -1),
         X._gate(top, b0, 0, -1, +1),
         X._gate(b0, top, mid, 0, -1)]
    if n >= 4:
        G += [X._gate(top | 2, b0 | nxt, mid & ~2 & ~nxt, 4, +1),
              X._gate(b0 | 2, 4 | 8, mid & ~(2 | 4 | 8), 5, -1)]
    G += [X._gate(nxt | b0 if n >= 3 else top | b0, 0, 0, 3, -1),
          X._gate(top, nxt, 0, 0, +1)]
    return G, (6 if n >= 4 else 5)


def spread_params(gates, n_params):
    """the same gates driven by n_params parameters in turn (gate i by parameter i % n_params)."""
    return [X._gate(int(g.mask_hi), int(g.mask_lo), int(g.mask_par), i % n_params, int(g.sign))
            for i, g in enumerate(gates)], n_params


UCCSD_ELECTRONS = {4: 2, 6: 3, 8: 4, 10: 2, 12: 2}
FABRIC_ELECTRONS = {4: 2, 6: 2, 8: 4, 10: 4, 12: 6, 14: 6}


@functools.lru_cache(maxsize=None)
def gate_list(kind, n):
    """(gates, n_theta, Hartree-Fock start index) of a named list on n qubits."""
    ncas = n // 2
    if kind == "kupccd":
        return X.kupccd_gates(ncas, 1) + (_hf(2 * (ncas // 2), n),)
    if kind == "uccsd":
        return X.uccd_gates(ncas, UCCSD_ELECTRONS[n], True) + (_hf(UCCSD_ELECTRONS[n], n),)
    if kind == "fabric":
        return X.gatefabric_gates(ncas, FABRIC_ELECTRONS[n], 2) + (_hf(FABRIC_ELECTRONS[n], n),)
    if kind == "fabric14":                       # gatefabric_gates(7, 6, 2) on the low 14 bits of a wider register
        g, nt = X.gatefabric_gates(7, 6, 2)
        return g, nt, _hf(6, 14) | ((1 << n) - (1 << 14))
    if kind == "ladder":
        return S.ladder_gates(ncas) + (_hf(ncas, n),)
    if kind == "ladder_shared":
        return S.ladder_gates(ncas, shared=True) + (_hf(ncas, n),)
    if kind == "hand":
        return hand_gates(n) + (((1 << n) - 1) & ~((1 << (n - n // 2)) - 1),)
    if kind == "hand0":                          # from index 0, where the gates that create pairs of set bits act
        return hand_gates(n) + (0,)
    if kind.startswith("ladder/"):               # ladder gates (twice for ladder2) driven by P parameters in turn
        g = S.ladder_gates(ncas)[0]
        return spread_params(g, int(kind.split("/")[1])) + (_hf(ncas, n),)
    if kind.startswith("ladder2/"):
        g = S.ladder_gates(ncas)[0]
        return spread_params(g + g, int(kind.split("/")[1])) + (_hf(ncas, n),)
    if kind == "singles3":                       # two parameters, parameter 0 drives an alpha and a beta single
        g = S.singles_gates(ncas, [(ncas // 2 - 1, ncas // 2), (ncas // 2 - 2, ncas // 2 - 1)],
                            [(ncas // 2 - 1, ncas // 2)])[0]
        return [X._gate(int(q.mask_hi), int(q.mask_lo), int(q.mask_par), i, int(q.sign))
                for q, i in zip(g, (0, 1, 0))], 2, _hf(2 * (ncas // 2), n)
    raise ValueError(kind)


def start_index(case):
    n, kind, start = case[0], case[1], case[2]
    return {"hf": gate_list(kind, n)[2], "0": 0, "D-1": (1 << n) - 1}[start]


def thetas(case_id, batch, n_theta):
    """uniform in [-2 pi, 2 pi], distinct per batch element, an exact 0 and an exact pi among the entries."""
    seed = int.from_bytes(case_id.encode(), "little") % (2 ** 32)
    th = np.random.default_rng(seed).uniform(-TWO_PI, TWO_PI, (batch, n_theta))
    if th.size >= 3:
        th.flat[th.size - 1] = 0.0
        th.flat[th.size // 2] = np.pi
    return th


# ---- the device cases ----------------------------------------------------------------------------------------------
LDS_STATE_MAX_QUBITS = 13
# (qubits, gate list, start, batch): each case runs with and without tangents; every parameter is compared
STATE_CASES = [
    (2, "hand", "hf", 1), (2, "hand", "0", 3), (2, "hand", "D-1", 33),
    (3, "hand", "hf", 33), (3, "hand", "0", 1), (3, "hand", "D-1", 3),
    (4, "kupccd", "hf", 1), (4, "uccsd", "hf", 3), (4, "fabric", "hf", 33), (4, "ladder", "hf", 1),
    (4, "ladder_shared", "hf", 3), (4, "hand", "0", 1),
    (5, "hand", "hf", 3), (5, "hand", "D-1", 1),
    (6, "kupccd", "hf", 3), (6, "uccsd", "hf", 1), (6, "fabric", "hf", 3), (6, "ladder", "hf", 1),
    (6, "ladder_shared", "hf", 33), (6, "hand", "hf", 1),
    (8, "kupccd", "hf", 33), (8, "uccsd", "hf", 1), (8, "fabric", "hf", 3), (8, "ladder", "hf", 1),
    (8, "ladder_shared", "hf", 1), (8, "hand", "D-1", 3),
    (10, "kupccd", "hf", 1), (10, "uccsd", "hf", 1), (10, "fabric", "hf", 1), (10, "ladder_shared", "hf", 1),
    (10, "hand", "0", 1),
    (12, "kupccd", "hf", 1), (12, "uccsd", "hf", 1), (12, "fabric", "hf", 1), (12, "ladder_shared", "hf", 1),
    (12, "hand", "hf", 1),
    (13, "hand", "hf", 1), (13, "hand", "0", 1), (13, "hand", "D-1", 1),
    (14, "fabric", "hf", 2), (14, "hand", "hf", 1), (14, "ladder_shared", "hf", 1), (14, "kupccd", "hf", 1),
    (15, "fabric14", "hf", 1), (15, "hand", "0", 1), (15, "hand", "D-1", 1),
]
# (ncas, batch, bra is ket)
RDM_CASES = [(a, b, same) for a in range(1, 8) for b in ([1, 3, 17] if a <= 5 else [1, 3]) for same in (True, False)]
# (ncas, n_tan, batch)
RDM_TANGENT_CASES = [(a, t, b) for a in range(1, 8) for t in (0, 1, 5) for b in (1, 2)]
RDM_TANGENT_LIMIT = (2, 16383)                  # ncas, the largest nvec with nvec ncas^2 <= 65535
RDM_TANGENT_LIMIT_SETS = [0, 1, 2, 8191, 16381, 16382]
# (ncas, gate list, one-workgroup route?): both sides of the switch at ncas 3 and 4
CIRCUIT_RDMS_CASES = [
    (1, "hand0", True), (2, "fabric", True), (2, "ladder_shared", True),
    (3, "ladder2/15", True), (3, "ladder2/16", False),
    (4, "ladder/2", True), (4, "ladder/3", False),
    (5, "fabric", False), (7, "ladder/2", False),
]
CIRCUIT_RDMS_BATCHES = [1, 5]
# (ncas, gate list)
HESSIAN_CASES = [(2, "fabric"), (3, "uccsd"), (4, "kupccd"), (5, "ladder/3"), (7, "singles3")]
SPIN_CASES = [(n, b) for n in (1, 2, 3, 4, 5, 6, 7, 8, 10) for b in (1, 3)]


@functools.lru_cache(maxsize=None)
def _state_reference(case, dtype, first_only, annihilate):
    n, kind, _, batch = case
    gates, n_theta, _ = gate_list(kind, n)
    init = start_index(case)
    th = thetas(state_id(case), batch, n_theta)
    psi = np.stack([apply_gates(gates, th[b], n, init, (), dtype) for b in range(batch)])
    dpsi = np.stack([np.stack([tangent(gates, th[b], n, init, k, n_theta, dtype, first_only, annihilate)
                               for k in range(n_theta)]) for b in range(batch)])
    return th, psi, dpsi


def state_reference(case, dtype=np.float64, first_only=False, annihilate=True):
    """(theta [batch, n_theta], psi [batch, D], dpsi [batch, n_theta, D]) of a STATE_CASES entry (computed once)."""
    return _state_reference(case, dtype, first_only, annihilate)


def state_bounds(case, dpsi):
    """(bound of psi, bounds of the tangents [batch, n_theta]) in 2-norm."""
    gates, n_theta, _ = gate_list(case[1], case[0])
    own = S.param_gates(gates, n_theta)
    return state_bound(gates), np.array([[tangent_bound(gates, len(own[k]), dpsi[b, k]) for k in range(n_theta)]
                                         for b in range(dpsi.shape[0])])


@functools.lru_cache(maxsize=None)
def rdm_reference(ncas, i, same, dtype=np.float64):
    """pair i of the RDM cases of ncas: (bra, ket, gamma, Gamma, bound of gamma, bound of Gamma)."""
    reg = register(ncas)
    bra, ket = make_pairs(reg.D, 4000 + 10 * ncas, i + 1, same)
    g1, g2 = reg.rdms(bra[i], ket[i], dtype=dtype)
    b1, b2 = rdm_bounds(reg, bra[i], ket[i])
    return bra[i], ket[i], g1, g2, b1, b2


@functools.lru_cache(maxsize=None)
def tangent_vectors(ncas, b):
    """psi and five 'tangents' of batch element b of the derivative-RDM cases (any vectors: the sets are bilinear)."""
    v = make_vectors(1 << (2 * ncas), 7000 + 100 * ncas + b, 6)
    return v[b % 3], np.delete(v, b % 3, axis=0)


@functools.lru_cache(maxsize=None)
def rdm_tangent_reference(ncas, b, n_tan, dtype=np.float64):
    reg = register(ncas)
    psi, dpsi = tangent_vectors(ncas, b)
    g1, g2 = reg.rdms_tangent(psi, dpsi[:n_tan], dtype=dtype)
    b1, b2 = rdm_tangent_bounds(reg, psi, dpsi[:n_tan])
    return g1, g2, b1, b2


@functools.lru_cache(maxsize=None)
def spin_reference(n, i, dtype=np.float64):
    bra, ket = make_pairs(1 << n, 9000 + 10 * n, i + 1, False)
    g1, g2 = spin_rdms(bra[i], ket[i], n, dtype=dtype)
    b1, b2 = spin_rdm_bounds(bra[i], ket[i], n)
    return bra[i], ket[i], g1, g2, b1, b2


def circuit_case(ncas, kind, batch):
    """(gates, n_theta, init, theta [batch, n_theta]) of a CIRCUIT_RDMS_CASES / HESSIAN_CASES entry."""
    gates, n_theta, init = gate_list(kind, 2 * ncas)
    return gates, n_theta, init, thetas(f"c{ncas}_{kind}", batch, n_theta)


@functools.lru_cache(maxsize=None)
def circuit_rdms_reference(ncas, kind, b, dtype=np.float64, first_only=False, annihilate=True):
    """batch element b (of 5): psi, dpsi [n_theta, D], the RDM sets and their bounds, the state bounds."""
    gates, n_theta, init, th = circuit_case(ncas, kind, 5)
    n, reg = 2 * ncas, register(ncas)
    psi = apply_gates(gates, th[b], n, init, (), dtype)
    dpsi = np.stack([tangent(gates, th[b], n, init, k, n_theta, dtype, first_only, annihilate)
                     for k in range(n_theta)])
    g1, g2 = reg.rdms_tangent(psi, dpsi, dtype=dtype)
    b1, b2 = rdm_tangent_bounds(reg, psi, dpsi)
    own = S.param_gates(gates, n_theta)
    es = state_bound(gates)
    tb = np.array([tangent_bound(gates, len(own[k]), dpsi[k]) for k in range(n_theta)])
    carried = set_input_errors(psi, dpsi, es, tb)
    b1 = b1 + 2.0 * carried[:, None, None]
    b2 = b2 + 6.0 * carried[:, None, None, None, None]
    return psi, dpsi, g1, g2, b1, b2, es, tb


@functools.lru_cache(maxsize=None)
def hessian_reference(ncas, kind, dtype=np.float64):
    gates, n_theta, init, th = circuit_case(ncas, kind, 1)
    c1, c2 = coefficients(ncas, 50 + ncas)
    if dtype is np.float64:
        return (th[0], c1, c2) + hessian(gates, th[0], ncas, init, c1, c2, n_theta, bound=True)
    return th[0], c1, c2, hessian(gates, th[0], ncas, init, c1, c2, n_theta, dtype), None


def state_id(c):
    return f"q{c[0]}_{c[1].replace('/', '-')}_{c[2]}_b{c[3]}"


def route(n):
    """which realisation oovqe_circuit_state takes: the register in LDS or in global memory."""
    return "lds" if n <= LDS_STATE_MAX_QUBITS else "global"
