"""Host twin of the particle-number-sector engine (csrc/sector.hip) for the whole-scope tests: numpy fp64 (and
``np.longdouble``) written from the definitions alone -- gate-table semantics of tests/_emulate.py restricted to the
sector's determinants, E_pq from the spin-orbital a^+_P a_Q, RDMs and lam(v) = (Hop + Hop^T) v assembled from E_pq --
with none of the kernels' devices (rank tables, excitation tables, the sigma basis, G_a / G_b, pair lists).

Layout (``auto_oo_amd.sector.string_tables``): orbital p of a string at bit ncas-1-p, strings ascending by value,
c = ia * nb + ib, full register index x = spread(alpha) << 1 | spread(beta) (spin orbital 2p = alpha_p = qubit 2p =
bit 2 ncas - 1 - 2p).  Also here: the bounds of the device tests (no figure in them comes from device output) and a
replica of the entry points' dispatch arithmetic, written from the thresholds documented in DESIGN.md."""
from itertools import combinations

import numpy as np

from auto_oo_amd import excitations as X

U = 2.0 ** -53


def _popcount(v):
    v = np.asarray(v, dtype=np.uint64)
    out = np.zeros(v.shape, dtype=np.int64)
    while True:
        nz = v != 0
        if not nz.any():
            return out
        out += (v & np.uint64(1)).astype(np.int64)
        v = v >> np.uint64(1)


def strings(ncas, n):
    out = []
    for occ in combinations(range(ncas), n):
        m = 0
        for p in occ:
            m |= 1 << (ncas - 1 - p)
        out.append(m)
    return np.array(sorted(out), dtype=np.int64)


def _spread(v, ncas):
    out = np.zeros_like(v)
    for i in range(ncas):
        out |= ((v >> i) & 1) << (2 * i)
    return out


class Sector:
    """The (N_alpha, N_beta) sector of ncas orbitals, any 0 <= N <= ncas."""

    def __init__(self, ncas, n_alpha, n_beta):
        self.ncas, self.n_alpha, self.n_beta = ncas, n_alpha, n_beta
        self.ua, self.ub = strings(ncas, n_alpha), strings(ncas, n_beta)
        self.na, self.nb = len(self.ua), len(self.ub)
        self.Dc = self.na * self.nb
        self.x = ((_spread(self.ua, ncas) << 1)[:, None] | _spread(self.ub, ncas)[None, :]).reshape(-1)
        self._order = np.argsort(self.x)
        self._sorted = self.x[self._order]
        self._epq = None
        self._count = None

    def lookup(self, x):
        """compressed index of full indices x (-1 outside the sector)."""
        x = np.asarray(x, dtype=np.int64)
        pos = np.clip(np.searchsorted(self._sorted, x), 0, self.Dc - 1)
        return np.where(self._sorted[pos] == x, self._order[pos], -1)

    def occupation(self, occ_alpha=None, occ_beta=None):
        """interleaved occupation vector (the ``hfstate`` argument of SectorEngine) of one determinant: the given
        orbitals, or the lowest ones."""
        occ_alpha = range(self.n_alpha) if occ_alpha is None else occ_alpha
        occ_beta = range(self.n_beta) if occ_beta is None else occ_beta
        occ = np.zeros(2 * self.ncas, dtype=int)
        for p in occ_alpha:
            occ[2 * p] = 1
        for p in occ_beta:
            occ[2 * p + 1] = 1
        return occ

    # ---- E_pq = E^alpha_pq + E^beta_pq from a^+_P a_Q --------------------------------------------------------------
    def epq(self):
        """(src [a, a, 2, Dc], sign [a, a, 2, Dc]): (E_pq v)[c] = sum_spin sign[p, q, spin, c] v[src[p, q, spin, c]]
        (sign 0 where the term is absent; src 0 there).  a^+_P a_Q |c'> = (-1)^(occupied spin orbitals strictly
        between P and Q) |c>, c = c' with Q emptied and P filled."""
        if self._epq is None:
            a, n, x = self.ncas, 2 * self.ncas, self.x
            src = np.zeros((a, a, 2, self.Dc), dtype=np.int64)
            sign = np.zeros((a, a, 2, self.Dc))
            for p in range(a):
                for q in range(a):
                    for sp in (0, 1):
                        P, Q = 2 * p + sp, 2 * q + sp
                        bP, bQ = 1 << (n - 1 - P), 1 << (n - 1 - Q)
                        if P == Q:
                            ok = (x & bP) != 0
                            src[p, q, sp] = np.arange(self.Dc)
                            sign[p, q, sp] = ok.astype(float)
                            continue
                        ok = ((x & bP) != 0) & ((x & bQ) == 0)            # c holds P and not Q; c' = c - P + Q
                        between = 0
                        for R in range(min(P, Q) + 1, max(P, Q)):
                            between |= 1 << (n - 1 - R)
                        par = _popcount(x & between) & 1
                        s = self.lookup(np.where(ok, x ^ (bP | bQ), x))
                        assert (s[ok] >= 0).all()
                        src[p, q, sp] = np.where(ok, s, 0)
                        sign[p, q, sp] = np.where(ok, np.where(par == 1, -1.0, 1.0), 0.0)
            self._epq = (src, sign)
        return self._epq

    def apply_epq(self, v, absolute=False):
        """V [a^2, Dc] = E_pq v (``absolute``: every sign and amplitude by its absolute value)."""
        src, sign = self.epq()
        a = self.ncas
        if absolute:
            v, sign = np.abs(v), np.abs(sign)
        sign = sign.astype(v.dtype)
        return (sign[:, :, 0] * v[src[:, :, 0]] + sign[:, :, 1] * v[src[:, :, 1]]).reshape(a * a, self.Dc)

    def apply_epq_rows(self, W, absolute=False):
        """sum_pq E_pq W_pq for W [a^2, Dc]."""
        src, sign = self.epq()
        a = self.ncas
        if absolute:
            W, sign = np.abs(W), np.abs(sign)
        sign = sign.astype(W.dtype).reshape(a * a, 2, self.Dc)
        src = src.reshape(a * a, 2, self.Dc)
        rows = np.arange(a * a)[:, None]
        return (sign[:, 0] * W[rows, src[:, 0]] + sign[:, 1] * W[rows, src[:, 1]]).sum(axis=0)

    # ---- RDMs ---------------------------------------------------------------------------------------------------
    def rdms(self, v, absolute=False, dtype=np.float64):
        """gamma [a, a], Gamma [a, a, a, a] of one vector: V_pq = E_pq v, gamma_pq = v . V_pq,
        Gamma_pqrs = V_qp . V_rs - delta_qr gamma_ps (include/oovqe.h); no symmetry assumed."""
        a = self.ncas
        v = np.asarray(v, dtype=dtype)
        V = self.apply_epq(v, absolute)
        gamma = (V @ (np.abs(v) if absolute else v)).reshape(a, a)
        Vt = V.reshape(a, a, -1).transpose(1, 0, 2).reshape(a * a, -1)             # row pq = V_qp
        Gamma = (Vt @ V.T).reshape(a, a, a, a)
        for q in range(a):
            if absolute:
                Gamma[:, q, q, :] += gamma
            else:
                Gamma[:, q, q, :] -= gamma
        return gamma, Gamma

    # ---- lam(v) = (Hop + Hop^T) v ----------------------------------------------------------------------------------
    def lam(self, v, c1, c2, absolute=False, dtype=np.float64):
        """Hop = sum c1_pq E_pq + sum c2_pqrs (E_pq E_rs - delta_qr E_ps), c1, c2 not symmetric.  E_pq^T = E_qp, so
        Hop v   = sum_pq c1_pq V_pq + sum_pq E_pq (sum_rs c2_pqrs V_rs) - sum_pqs c2_pqqs V_ps
        Hop^T v = sum_pq c1_pq V_qp + sum_rs E_sr (sum_pq c2_pqrs V_qp) - sum_pqs c2_pqqs V_sp."""
        a = self.ncas
        v = np.asarray(v, dtype=dtype)
        c1 = np.asarray(c1, dtype=dtype).reshape(a, a)
        c2 = np.asarray(c2, dtype=dtype).reshape(a, a, a, a)
        if absolute:
            c1, c2 = np.abs(c1), np.abs(c2)
        V = self.apply_epq(v, absolute)
        Vt = V.reshape(a, a, -1).transpose(1, 0, 2).reshape(a * a, -1)             # row pq = V_qp
        C2 = c2.reshape(a * a, a * a)
        one = c1.reshape(-1) @ V + c1.reshape(-1) @ Vt
        W = C2 @ V                                                                 # [pq] = sum_rs c2_pqrs V_rs
        Wt = (C2.T @ Vt).reshape(a, a, -1).transpose(1, 0, 2).reshape(a * a, -1)   # [sr] = sum_pq c2_pqrs V_qp
        two = self.apply_epq_rows(W, absolute) + self.apply_epq_rows(Wt, absolute)
        d = np.einsum("pqqs->ps", c2).reshape(-1)
        corr = d @ V + d @ Vt
        return one + two + corr if absolute else one + two - corr

    def lam_count(self):
        """the largest number of non-zero products any element of lam receives (unit coefficients, unit vector)."""
        if self._count is None:
            a = self.ncas
            self._count = float(self.lam(np.ones(self.Dc), np.ones((a, a)), np.ones((a,) * 4), absolute=True).max())
        return self._count

    def lam_norm(self, c1, c2):
        """||Hop + Hop^T||_2 <= largest row sum of its absolute value (the matrix is symmetric)."""
        return float(self.lam(np.ones(self.Dc), c1, c2, absolute=True).max())

    def energy(self, psi, c1, c2):
        g1, g2 = self.rdms(psi)
        return float((np.asarray(c1).reshape(-1) * g1.reshape(-1)).sum()
                     + (np.asarray(c2).reshape(-1) * g2.reshape(-1)).sum())


# ---- circuits ------------------------------------------------------------------------------------------------------
def apply_gates(gates, theta, sec, init, deriv=()):
    """The gate table in the sector (tests/_emulate.py on the Dc determinants): selection (x & (hi|lo)) == hi,
    partner x ^ (hi|lo), parity popcount(x & mask_par), angle sign * theta / 2.  ``deriv``: up to two gate indices
    to differentiate -- the 2 x 2 block becomes its derivative and the gate annihilates what it would leave alone
    (the derivative of an identity block).  -> (psi [Dc], pairs per gate)."""
    psi = np.zeros(sec.Dc)
    c0 = int(sec.lookup(np.array([init]))[0])
    assert c0 >= 0
    psi[c0] = 1.0
    counts = np.zeros(len(gates), dtype=np.int64)
    deriv = [g for g in deriv if g >= 0]
    for gi, g in enumerate(gates):
        if g.theta_idx < 0:
            continue
        fm = g.mask_hi | g.mask_lo
        sel = np.nonzero((sec.x & fm) == g.mask_hi)[0]
        y = sec.lookup(sec.x[sel] ^ fm)
        assert (y >= 0).all(), "the gate leaves the sector"
        counts[gi] = len(sel)
        pi = np.where((_popcount(sec.x[sel] & g.mask_par) & 1) == 1, -1.0, 1.0)
        ang = 0.5 * g.sign * theta[g.theta_idx]
        c, s = np.cos(ang), np.sin(ang)
        order = deriv.count(gi)
        h = 0.5 * g.sign
        if order == 1:
            c, s = -h * s, h * c
        elif order == 2:
            c, s = -0.25 * c, -0.25 * s
        ax, ay = psi[sel].copy(), psi[y].copy()
        if order:
            psi = np.zeros(sec.Dc)
        psi[sel] = c * ax + pi * s * ay
        psi[y] = c * ay - pi * s * ax
    return psi, counts


def param_gates(gates, n_theta):
    owner = [[] for _ in range(n_theta)]
    for gi, g in enumerate(gates):
        if g.theta_idx >= 0:
            owner[g.theta_idx].append(gi)
    return owner


def tangent(gates, theta, sec, init, k, n_theta):
    """d psi / d theta_k: the sum over the gates parameter k drives."""
    return sum(apply_gates(gates, theta, sec, init, (g,))[0] for g in param_gates(gates, n_theta)[k])


def second_tangent(gates, theta, sec, init, j, k, n_theta):
    owner = param_gates(gates, n_theta)
    return sum(apply_gates(gates, theta, sec, init, (g, h))[0] for g in owner[j] for h in owner[k])


def adjoint(gates, theta, sec, init, c1, c2, n_theta, psi=None):
    """d/dtheta_k of psi . Hop psi = tau_k . lam(psi)."""
    psi = apply_gates(gates, theta, sec, init)[0] if psi is None else psi
    lam = sec.lam(psi, c1, c2)
    return np.array([tangent(gates, theta, sec, init, k, n_theta) @ lam for k in range(n_theta)]), lam


def hessian(gates, theta, sec, init, c1, c2, n_theta):
    """H_jk = tau_jk . lam(psi) + tau_j . lam(tau_k)."""
    psi = apply_gates(gates, theta, sec, init)[0]
    lam0 = sec.lam(psi, c1, c2)
    tau = [tangent(gates, theta, sec, init, k, n_theta) for k in range(n_theta)]
    lamt = [sec.lam(t, c1, c2) for t in tau]
    H = np.zeros((n_theta, n_theta))
    for j in range(n_theta):
        for k in range(n_theta):
            H[j, k] = second_tangent(gates, theta, sec, init, j, k, n_theta) @ lam0 + tau[j] @ lamt[k]
    return H


def n_rotations(gates):
    return sum(1 for g in gates if g.theta_idx >= 0)


# ---- inputs --------------------------------------------------------------------------------------------------------
def dense_vector(sec, seed):
    """not normalised, every amplitude non-zero."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(sec.Dc)
    return np.where(np.abs(v) < 0.05, 0.05, v) * rng.choice([0.5, 1.0, 3.0])


def patterned_vector(sec, seed):
    """exact zeros in every second alpha row and every third beta column."""
    v = dense_vector(sec, seed).reshape(sec.na, sec.nb).copy()
    v[1::2, :] = 0.0
    v[:, 2::3] = 0.0
    return v.reshape(-1)


def single_determinant(sec, seed):
    v = np.zeros(sec.Dc)
    v[np.random.default_rng(seed).integers(sec.Dc)] = -1.75
    return v


def make_vectors(sec, seed, n):
    """n vectors: dense, patterned, one determinant, then dense ones (distinct seeds)."""
    makers = [dense_vector, patterned_vector, single_determinant]
    return np.stack([(makers[i] if i < 3 else dense_vector)(sec, seed + 17 * i) for i in range(n)])


def coefficients(ncas, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((ncas, ncas)), rng.standard_normal((ncas,) * 4)


def singles_gates(ncas, alpha_pairs, beta_pairs, shared=False):
    """a hand-made list: single excitations (p -> q) of the alpha, then of the beta electrons."""
    n = 2 * ncas
    gates = []
    for p, q in alpha_pairs:
        lo, hi = min(p, q), max(p, q)
        gates.append(X.fse_gate(list(range(2 * lo, 2 * hi + 1)), n, 0 if shared else len(gates)))
    for p, q in beta_pairs:
        lo, hi = min(p, q), max(p, q)
        gates.append(X.fse_gate(list(range(2 * lo + 1, 2 * hi + 2)), n, 0 if shared else len(gates)))
    return gates, (1 if shared else len(gates))


def ladder_gates(ncas, shared=False):
    """alpha and beta singles between neighbouring orbitals, up and down the ladder: reaches every determinant of
    any sector from any start."""
    ups = [(p, p + 1) for p in range(ncas - 1)]
    return singles_gates(ncas, ups + ups[::-1], ups + ups[::-1], shared)


def circuit(kind, ncas, n_alpha, n_beta):
    """(gates, n_theta) of a named gate list for a sector."""
    nel = n_alpha + n_beta
    if kind == "kupccd":
        return X.kupccd_gates(ncas, 1)
    if kind == "uccsd":
        return X.uccd_gates(ncas, nel, True)
    if kind == "fabric":
        return X.gatefabric_gates(ncas, nel, 2)
    if kind == "ladder":
        return ladder_gates(ncas)
    raise ValueError(kind)


# ---- bounds (section "Bounds" of DESIGN.md, "The sector engine over its whole scope") ------------------------------
def rdm_bounds(sec, v):
    """per element 2 (n + 8) u |.|-twin, n = Dc + 2 products per Gram element (V is a sum of two spin terms).  The
    factor 2: one share for the device's summation order, one for the fp64 twin's own (test_sector_scope_cpu)."""
    g1, g2 = sec.rdms(v, absolute=True)
    f = 2.0 * (sec.Dc + 2 + 8) * U
    return f * g1, f * g2


def lam_bound(sec, v, c1, c2):
    return 2.0 * (sec.lam_count() + 8) * U * sec.lam(v, c1, c2, absolute=True)


def state_bound(gates):
    """|| psi_dev - psi_twin ||_2 <= 8 n_gates u || psi ||_2, || psi || <= 1: per Givens pass two products and a sum
    per amplitude from a cosine and a sine good to a couple of ulp; earlier errors ride through orthogonal maps."""
    return 8.0 * n_rotations(gates) * U


def adjoint_bound(sec, gates, n_theta, psi, lam, blam):
    """d theta_k = sum_{g of k} (sign_g / 2) lam_g^T A_g psi_g with psi_g, lam_g the two vectors swept back to gate g
    and A_g the gate's generator (|| A_g || = 1).  The sweep starts from lam_dev = lam + e, || e ||_2 <= || B_lam ||_2
    (psi is uploaded exactly); each of the two sweeps adds at most 8 n_gates u of its vector's norm (state_bound),
    and the scalar product of Dc terms (Dc + 2) u || lam || || psi ||:
        | d theta_k - twin | <= (gates of k) / 2 [ || B_lam || + (16 n_gates + Dc + 2) u || lam || ] || psi ||."""
    per = 0.5 * (np.linalg.norm(blam) + (16 * n_rotations(gates) + sec.Dc + 2) * U * np.linalg.norm(lam)) \
        * np.linalg.norm(psi)
    return np.array([max(1, len(g)) for g in param_gates(gates, n_theta)]) * per


def hessian_bound(sec, gates, n_theta, theta, init, c1, c2, by_rdms):
    """H_jk = tau_jk . lam(psi) + tau_j . lam(tau_k) from device states d = twin + delta, || delta ||_2 <= m e_s
    (e_s = state_bound, m = weighted number of differentiated circuits summed into the tangent, + u || d || for the sum).
    With L = || Hop + Hop^T ||_2 (<= the largest absolute row sum):
      lam route:  | delta (x . lam(y)) | <= dx (|| lam(y) || + L dy) + || x || (|| B_lam(y) || + L dy)
                                            + (Dc + 2) u || x || || lam(y) ||
      RDM route:  H_jk = sum of four Q(v) / 2, Q(v) = c1 . gamma(v) + c2 . Gamma(v) = v . Hop v:
                  | delta Q(v) | <= |c1| . B_gamma + |c2| . B_Gamma + (a^4 + a^2 + 8) u Qabs(v) + L || v || dv (2 + dv)
    (first order in every error plus the products of two)."""
    owner = param_gates(gates, n_theta)
    es = state_bound(gates)
    L = sec.lam_norm(c1, c2)
    a = sec.ncas
    psi = apply_gates(gates, theta, sec, init)[0]
    tau = [tangent(gates, theta, sec, init, k, n_theta) for k in range(n_theta)]
    d1 = [len(owner[k]) * es + U * np.linalg.norm(tau[k]) for k in range(n_theta)]
    B = np.zeros((n_theta, n_theta))
    c1a, c2a = np.abs(c1).reshape(-1), np.abs(c2).reshape(-1)

    def dq(v, dv):
        b1, b2 = rdm_bounds(sec, v)
        q1, q2 = sec.rdms(v, absolute=True)
        qabs = c1a @ q1.reshape(-1) + c2a @ q2.reshape(-1)
        return c1a @ b1.reshape(-1) + c2a @ b2.reshape(-1) + (a ** 4 + a * a + 8) * U * qabs \
            + L * np.linalg.norm(v) * dv * (2 + dv)

    def dot(x, dx, y, dy):
        ly = sec.lam(y, c1, c2)
        nl = np.linalg.norm(ly)
        return dx * (nl + L * dy) + np.linalg.norm(x) * (np.linalg.norm(lam_bound(sec, y, c1, c2)) + L * dy) \
            + (sec.Dc + 2) * U * np.linalg.norm(x) * nl

    for j in range(n_theta):
        for k in range(j, n_theta):
            t2 = second_tangent(gates, theta, sec, init, j, k, n_theta)
            d2 = len(owner[j]) * len(owner[k]) * es + U * np.linalg.norm(t2)
            if by_rdms:
                b = 0.5 * (dq(t2 + psi, d2 + es + U) + dq(t2 - psi, d2 + es + U)
                           + dq(tau[j] + tau[k], d1[j] + d1[k] + U) + dq(tau[j] - tau[k], d1[j] + d1[k] + U))
            else:
                b = dot(t2, d2, psi, es) + dot(tau[j], d1[j], tau[k], d1[k])
            B[j, k] = B[k, j] = b
    return B


# ---- the dispatch arithmetic of the entry points (from the thresholds in DESIGN.md, not from the library) ---------
KB = 1024
CH, RCH, RCHP, LCH, CHP_MAX, MAXSTR = 128, 144, 146, 144, 144, 2048


def _fused_lds(na, nb, a):
    Dc, a2 = na * nb, a * a
    return (Dc + (Dc & 1) + a2 * CHP_MAX) * 8 + (((na + nb) * a2 * 2 + 7) & ~7)


def _rows_lds(na, nb, a):
    a2, NBp = a * a, (nb + 8) & ~7
    NRC = RCH // NBp
    if NRC < 1:
        return 1 << 30
    nchunk = -(-na // NRC)
    NR = max(nchunk * NRC, na + 1)
    return (NR * NBp + a2 * RCHP) * 8 + (a2 * na * 4 + 7) // 8 * 8


def _lambda_lds(na, nb, a):
    return ((nb + 1) * ((na + 8) & ~7) + a * a * LCH + 4 * LCH) * 8


def _fused_ok(na, nb, a, unfused):
    a2 = a * a
    return a2 % 16 == 0 and a2 <= 64 and _fused_lds(na, nb, a) <= 140 * KB and na < MAXSTR and nb < MAXSTR \
        and not unfused


def rdm_route(a, na, nb, batch, cus=256, unfused=0, r3=0):
    """the kernels oovqe_sector_rdms launches, as 'name[:detail]' strings."""
    Dc, a2 = na * nb, a * a
    MT, NT = (a2 + 1 + 15) // 16, (a2 + 15) // 16
    if (a2 in (16, 64) and _rows_lds(na, nb, a) + 8 * 256 * 8 <= 160 * KB and na < MAXSTR and nb < MAXSTR
            and max(na, nb) * a2 * 2 <= a2 * RCHP * 8 and not unfused and (r3 == 2 or (r3 == 0 and batch >= 16))):
        NRC = RCH // ((nb + 8) & ~7)
        nsplit = max(1, min(8, cus // batch, -(-na // NRC)))
        return [f"rdm_rows<{4 if a2 == 64 else 1}>:nsplit={nsplit}"]
    if _fused_ok(na, nb, a, unfused):
        nsplit = min(1 if batch >= 128 else 2 if batch >= 64 else 4 if batch >= 16 else 8, -(-Dc // CH))
        return [f"rdm_fused<{NT}>:nsplit={nsplit}"]
    epq_lds = (Dc + (Dc & 1)) * 8 + 2 * (1 << a) * 4
    out = ["epq_rows" if epq_lds <= 64 * KB and batch >= 8 else "epq"]
    nsplit = 1 if batch >= 32 else 2 if batch >= 8 else 8
    inst = {(5, 4): "gram_rows<4,4,true>", (4, 4): "gram_rows<4,4,false>", (3, 3): "gram_rows<3,3,false>",
            (2, 2): "gram_rows<2,2,false>", (2, 1): "gram_rows<1,1,true>"}
    if batch * nsplit >= 32 and (MT, NT) in inst:
        out.append(f"{inst[(MT, NT)]}:nsplit={nsplit}" + (":odd" if Dc & 1 else ""))
    else:
        out.append(f"gram<MT={MT},NT={NT}>:nsplit={nsplit}")
    return out


def string_driven_ok(a, na, nb, batch, unfused=0):
    a2, Dc = a * a, na * nb
    r4 = lambda n: (n + 3) // 4 * 4
    ta, tb = (na + 15) // 16 * 16, (nb + 15) // 16 * 16
    dense_lds = max(ta, r4(na)) * (max(tb, r4(nb)) + 4) * 8 + (na * na + nb * nb) * 8
    gmat_lds = a2 * max(na, nb) * 10 + 8
    room = na * na + nb * nb + Dc + ((na + nb) * a2 + 3) // 4 + (nb * a2 + 1) // 2 + 2 <= batch * (2 * a2 + 1) * Dc
    return (_fused_ok(na, nb, a, unfused) and a2 in (16, 64) and ((na + 8) & ~7) <= LCH
            and _lambda_lds(na, nb, a) <= 160 * KB and dense_lds <= 160 * KB and gmat_lds <= 160 * KB and room)


def lam_route(a, na, nb, batch, cus=256, unfused=0, lambda_w=0, per_set=False):
    a2, Dc = a * a, na * nb
    NT = (a2 + 15) // 16
    if string_driven_ok(a, na, nb, batch, unfused) and (per_set or lambda_w == 2 or (lambda_w == 0 and batch >= 32)):
        LA = (na + 8) & ~7
        nsplit = max(1, min(8, cus // batch, -(-nb // (LCH // LA))))
        return ["gmat", "lambda_dense", f"lambda_fused<{4 if a2 == 64 else 1}>:nsplit={nsplit}"]
    if per_set:
        return ["refused"]
    fused = _fused_ok(na, nb, a, unfused)
    if fused:
        nsplit = min(1 if batch >= 128 else 2 if batch >= 64 else 4 if batch >= 16 else 8, -(-Dc // CH))
        out = [f"w_fused<{NT}>:nsplit={nsplit}"]
    else:
        epq_lds = (Dc + (Dc & 1)) * 8 + 2 * (1 << a) * 4
        out = ["epq_rows" if epq_lds <= 64 * KB and batch >= 8 else "epq", "mode_contract"]
    if fused and (na + nb) * a2 * 2 <= (a2 * a2 + a2) * 8:
        out.append("lambda_tab")
    else:
        out.append("lambda:lds=%d" % (256 * 8 + 2 * (1 << a) * 4))
    return out


def sweep_route(a, na, nb, n_gates, n_theta, max_pairs, pair_lists=True, kind="state"):
    """state / deriv / adjoint sweeps: the MAXP instance from mp = ceil(max_pairs / 512) with pair lists, the MAXIT
    instance from nit = ceil(Dc / 1024) without; 'refused' past the LDS limits."""
    Dc = na * nb
    words = na + nb + 2 * (1 << a) + Dc
    if pair_lists:
        lds = ((2 * Dc + 2 * n_gates + n_gates * 8) * 8 + 12 * n_gates + 8 if kind == "adjoint"
               else (Dc + 2 * n_gates) * 8 + 4 * n_gates + 8)
        if Dc > 32767 or lds > 160 * KB or max_pairs > 16 * 512:
            return "refused"
        mp = -(-max_pairs // 512)
        return f"{kind}_pl<{1 if mp <= 1 else 2 if mp <= 2 else 4 if mp <= 4 else 8 if mp <= 8 else 16}>"
    lds = ((2 * Dc + 2 * n_gates + n_gates * 16 + n_theta) * 8 + 40 * n_gates + 4 * words if kind == "adjoint"
           else (Dc + 2 * n_gates) * 8 + 40 * n_gates + 4 * words)
    if lds > 160 * KB or Dc > 8 * 1024:
        return "refused"
    nit = -(-Dc // 1024)
    return f"{kind}<{1 if nit <= 1 else 2 if nit <= 2 else 5 if nit <= 5 else 8}>"


# ---- the device cases ----------------------------------------------------------------------------------------------
# (ncas, N_alpha, N_beta, circuit, what the sector is there for)
SECTORS = [
    (2, 1, 1, "ladder", "smallest; MT = NT = 1"),
    (3, 2, 1, "uccsd", "odd Dc = 9, different strings per spin"),
    (4, 2, 2, "kupccd", "a^2 = 16: rows / fused / string-driven routes"),
    (4, 2, 1, "uccsd", "a^2 = 16, unequal 6 x 4"),
    (4, 1, 3, "ladder", "a^2 = 16, equal sizes 4 x 4 but different strings"),
    (4, 0, 2, "ladder", "a^2 = 16, na = 1"),
    (5, 2, 2, "uccsd", "gram_rows<2,2>"),
    (5, 1, 1, "ladder", "gram_rows<2,2>, odd Dc = 25"),
    (5, 2, 1, "uccsd", "gram_rows<2,2>, Dc % 4 = 2"),
    (6, 3, 3, "fabric", "gram_rows<3,3>"),
    (6, 2, 2, "uccsd", "gram_rows<3,3>, odd Dc = 225"),
    (6, 3, 2, "uccsd", "gram_rows<3,3>, 20 x 15; the public odd-electron route"),
    (7, 3, 3, "ladder", "gram_rows<4,4,false>, odd Dc = 1225"),
    (7, 4, 3, "ladder", "gram_rows<4,4,false>, 35 x 35 with different strings"),
    (7, 2, 3, "ladder", "gram_rows<4,4,false>, 21 x 35"),
    (8, 4, 4, "kupccd", "a^2 = 64, 70 x 70: NBp = LA = 72"),
    (8, 3, 5, "ladder", "a^2 = 64, 56 x 56 with different strings: NBp = LA = 64"),
    (8, 4, 3, "ladder", "a^2 = 64, 70 x 56"),
    (8, 4, 1, "ladder", "a^2 = 64, 70 x 8: NBp = 16, LA = 72"),
    (8, 1, 4, "ladder", "a^2 = 64, 8 x 70: NBp = 72, LA = 16"),
    (8, 2, 1, "ladder", "a^2 = 64, 28 x 8: NBp = 16, LA = 32"),
    (8, 0, 4, "ladder", "a^2 = 64, 1 x 70: LA = 8"),
    (9, 1, 1, "ladder", "generic gram, MT = NT = 6, odd Dc = 81"),
    (9, 3, 3, "ladder", "generic gram, 84 x 84: MAXIT = 8, MAXP = 4, last size of epq_rows"),
    (10, 2, 4, "ladder", "45 x 210, 2 520 pairs per beta single: adjoint_pl<8> at 151 KB LDS; epq at any batch"),
    (12, 1, 1, "ladder", "a^2 = 144 = 9 x 16 > 64: no fused route"),
    (13, 1, 1, "ladder", "the documented limit; lambda kernel at 67 584 B LDS"),
    (13, 2, 1, "ladder", "the documented limit, 78 x 13"),
    (13, 1, 2, "ladder", "the documented limit, 13 x 78"),
]
# state and differentiated states only (the RDM workspace of these grows past what a quick test should allocate)
STATE_ONLY = [
    (9, 4, 4, "ladder", "state_pl / deriv_pl at 4 410 pairs per single: MAXP = 16"),
    (9, 4, 3, "ladder", "126 x 84: MAXP = 8"),
]
RDM_WALK_GENERIC = [(5, 1, 1), (6, 3, 2), (7, 2, 3), (9, 1, 1)]
RDM_BATCHES_EACH = [1, 8, 16]            # every sector of the table: both E_pq kernels, both Gram kernels
RDM_BATCHES_GENERIC = [1, 3, 4, 7, 8, 15, 16, 31, 32]
RDM_WALK_FUSED = [(4, 2, 1), (8, 4, 3)]
RDM_BATCHES_FUSED = [1, 4, 15, 16, 33, 64, 128, 130]   # (4: the unfused rows Gram at nsplit = 8)
RDM_OPTIONS = [{}, {"sector_rdm_r3": 1}, {"sector_rdm_r3": 2}, {"sector_unfused": 1}]
LAM_OPTIONS = [{}, {"sector_lambda_w": 1}, {"sector_lambda_w": 2}, {"sector_unfused": 1}]
LAM_BATCHES = [1, 31, 32, 33]
LAM_BATCHES_FUSED_EXTRA = [64, 130]       # at the sectors of RDM_WALK_FUSED: nsplit 2 and 1 of the round-3 and round-4 kernels


def sector_id(s):
    return f"a{s[0]}_{s[1]}_{s[2]}"
