"""Host twin of the ADAPT-VQE pool gradients (auto_oo_amd/adapt.py, csrc/pool.hip): numpy only, written from the
definitions -- E_pq from the bit rules of a^+_P a_Q on the sector's determinants, Hop as a dense matrix, every pool
operator's generator from the closed form in the docstring of auto_oo_amd/excitations.py -- with none of the engine's
devices (pair lists, string-driven operator, excitation tables).

Layout (auto_oo_amd.sector): orbital p of a string at bit ncas-1-p, strings ascending by value, c = ia * nb + ib, full
register index x = spread(alpha) << 1 | spread(beta): spin orbital 2p (+1) = alpha (beta) of orbital p = qubit 2p (+1)
= bit 2 ncas - 1 - 2p (-1)."""
from itertools import combinations

import numpy as np

EPS = 2.0 ** -52


def strings(ncas, n):
    out = []
    for occ in combinations(range(ncas), n):
        m = 0
        for p in occ:
            m |= 1 << (ncas - 1 - p)
        out.append(m)
    return sorted(out)


def _spread(v, ncas):
    out = 0
    for i in range(ncas):
        out |= ((v >> i) & 1) << (2 * i)
    return out


class Twin:
    """The (n_alpha, n_beta) sector of ncas orbitals: determinants, dense E_pq, dense Hop."""

    def __init__(self, ncas, n_alpha, n_beta, operators=True):
        self.ncas, self.n = ncas, 2 * ncas
        ua, ub = strings(ncas, n_alpha), strings(ncas, n_beta)
        self.na, self.nb = len(ua), len(ub)
        self.x = [(_spread(sa, ncas) << 1) | _spread(sb, ncas) for sa in ua for sb in ub]
        self.Dc = len(self.x)
        self.index = {x: c for c, x in enumerate(self.x)}
        self.E = self._epq() if operators else None      # (large sectors: the determinants alone)

    def _epq(self):
        """E[p, q] [Dc, Dc]: E_pq = sum_spin a^+_P a_Q, P = 2p + spin, Q = 2q + spin; a^+_P a_Q |x'> = (-1)^(occupied spin
        orbitals strictly between P and Q) |x' - Q + P> when x' holds Q and (P == Q or not P)."""
        a, n = self.ncas, self.n
        E = np.zeros((a, a, self.Dc, self.Dc))
        for p in range(a):
            for q in range(a):
                for sp in (0, 1):
                    P, Q = 2 * p + sp, 2 * q + sp
                    bP, bQ = 1 << (n - 1 - P), 1 << (n - 1 - Q)
                    for c, x in enumerate(self.x):               # column: the determinant acted on
                        if not x & bQ:
                            continue
                        if P == Q:
                            E[p, q, c, c] += 1.0
                            continue
                        if x & bP:
                            continue
                        between = sum((x >> (n - 1 - R)) & 1 for R in range(min(P, Q) + 1, max(P, Q)))
                        E[p, q, self.index[x ^ bP ^ bQ], c] += -1.0 if between & 1 else 1.0
        return E

    def hop(self, c1, c2, absolute=False, dtype=np.longdouble):
        """Hop = sum c1_pq E_pq + sum c2_pqrs (E_pq E_rs - delta_qr E_ps); c1, c2 not symmetric.  ``absolute``: every
        coefficient and matrix element by its absolute value (the - becomes +)."""
        a = self.ncas
        c1 = np.asarray(c1, dtype=dtype).reshape(a, a)
        c2 = np.asarray(c2, dtype=dtype).reshape(a, a, a, a)
        E = self.E.astype(dtype)
        if absolute:
            c1, c2, E = np.abs(c1), np.abs(c2), np.abs(E)
        H = np.einsum("pq,pqij->ij", c1, E)
        for p in range(a):
            for q in range(a):
                for r in range(a):
                    for s in range(a):
                        H = H + c2[p, q, r, s] * (E[p, q] @ E[r, s])
                        if q == r:
                            H = H + c2[p, q, r, s] * E[p, s] if absolute else H - c2[p, q, r, s] * E[p, s]
        return H

    def embed(self, v):
        """the sector vector in the full register of 2^n amplitudes."""
        full = np.zeros(1 << self.n)
        full[self.x] = v
        return full

    def restrict(self, full):
        return np.asarray(full)[self.x]

    def generator(self, gates, absolute=False, dtype=np.longdouble):
        """G with d psi / d theta at theta = 0 = G psi for one parameter driving ``gates``: per gate, for every x with the
        mask_hi bits set and the mask_lo bits clear and y = x ^ (mask_hi | mask_lo),
        psi'[x] = c psi[x] + pi s psi[y], psi'[y] = c psi[y] - pi s psi[x] at the angle sign * theta / 2, pi =
        (-1)^popcount(x & mask_par).  -> (G, pairs rotated by these gates in this sector)."""
        G = np.zeros((self.Dc, self.Dc), dtype=dtype)
        pairs = 0
        for g in gates:
            fm = int(g.mask_hi) | int(g.mask_lo)
            for c, x in enumerate(self.x):
                if (x & fm) != int(g.mask_hi):
                    continue
                y = self.index[x ^ fm]
                pi = -1.0 if bin(x & int(g.mask_par)).count("1") & 1 else 1.0
                h = 0.5 * int(g.sign) * pi
                pairs += 1
                if absolute:
                    G[c, y] += abs(h)
                    G[y, c] += abs(h)
                else:
                    G[c, y] += h
                    G[y, c] -= h
        return G, pairs


def pool_gradients(twin, pool, psi, c1, c2):
    """-> (g [P], bound [P], pairs [P]): g_k = psi^T (Hop + Hop^T) G_k psi in extended precision, and the bound on the
    error of an fp64 evaluation whose longest chain of additions has n = a^4 + a^2 + pairs_k terms:
    n 2^-52 A_k, A_k the same formula with |c1|, |c2|, |psi| and the absolute values of every matrix element."""
    a = twin.ncas
    ld = np.longdouble
    psi = np.asarray(psi, dtype=ld)
    H = twin.hop(c1, c2)
    Ha = twin.hop(c1, c2, absolute=True)
    lam, lam_a = (H + H.T) @ psi, (Ha + Ha.T) @ np.abs(psi)
    g, bound, count = [], [], []
    for op in pool.operators:
        G, pairs = twin.generator(op)
        Ga, _ = twin.generator(op, absolute=True)
        g.append(float(lam @ (G @ psi)))
        bound.append(float((a ** 4 + a ** 2 + pairs) * EPS * (lam_a @ (Ga @ np.abs(psi)))))
        count.append(pairs)
    return np.array(g), np.array(bound), np.array(count)


def sparse_gradients(twin, pool, psi, lam):
    """The kernel's own formula from given psi and lam (any sector size; no dense matrix):
    g_k = sum over the gates of k, over their pairs (x, y)  (sign / 2) pi(x) (psi[y] lam[x] - psi[x] lam[y]), with the
    bound pairs_k 2^-52 sum |sign / 2| (|psi[y]| |lam[x]| + |psi[x]| |lam[y]|) plus one rounding of each product.
    -> (g [P], bound [P], pairs [P])."""
    x = np.array(twin.x, dtype=np.int64)
    order = np.argsort(x)
    psi, lam = np.asarray(psi, dtype=np.longdouble), np.asarray(lam, dtype=np.longdouble)
    g, bound, count = [], [], []
    for op in pool.operators:
        tot, mag, pairs = np.longdouble(0), np.longdouble(0), 0
        for gt in op:
            fm = int(gt.mask_hi) | int(gt.mask_lo)
            sel = np.nonzero((x & fm) == int(gt.mask_hi))[0]
            y = order[np.searchsorted(x[order], x[sel] ^ fm)]
            assert (x[y] == (x[sel] ^ fm)).all()
            par = np.zeros(len(sel), dtype=np.int64)
            m = x[sel] & int(gt.mask_par)
            while m.any():
                par ^= m & 1
                m = m >> 1
            pi = np.where(par == 1, -1.0, 1.0) * 0.5 * int(gt.sign)
            tot += (pi * (psi[y] * lam[sel] - psi[sel] * lam[y])).sum()
            mag += (0.5 * (np.abs(psi[y] * lam[sel]) + np.abs(psi[sel] * lam[y]))).sum()
            pairs += len(sel)
        g.append(float(tot))
        bound.append(float((pairs + 2) * EPS * mag))
        count.append(pairs)
    return np.array(g), np.array(bound), np.array(count)


def random_case(twin, batch, seed):
    """normalised random states [batch, Dc] and NON-symmetric coefficients c1 [batch, a, a], c2 [batch, a, a, a, a]."""
    rng = np.random.default_rng(seed)
    a = twin.ncas
    psi = rng.standard_normal((batch, twin.Dc))
    psi /= np.linalg.norm(psi, axis=1, keepdims=True)
    return psi, rng.standard_normal((batch, a, a)), rng.standard_normal((batch, a, a, a, a))


def gsd_count(n):
    """Size of the generalised singles-and-doubles pool over n spin orbitals (even = alpha), counted from the definition
    by brute force over index tuples -- independent of auto_oo_amd.adapt.gsd_excitations."""
    spin = lambda w: 1 if w % 2 == 0 else -1                                              # noqa: E731
    singles = sum(1 for r in range(n) for p in range(n) if r < p and spin(r) == spin(p))
    seen = set()
    for i in range(n):
        for j in range(n):
            for k in range(n):
                for l in range(n):
                    if len({i, j, k, l}) == 4 and spin(i) + spin(j) == spin(k) + spin(l):
                        seen.add(frozenset((frozenset((i, j)), frozenset((k, l)))))
    return singles + len(seen)


# ---- the molecule case of the comparisons with the existing route ----------------------------------------------------
FORMAL = (140, 80)                 # formaldimine without spatial symmetry
THETA_SEED, KAPPA_SEED = 20261, 20262


def formaldimine_case(point=FORMAL, n_theta=4):
    """(molecule, OAO->MO coefficients, theta): STO-3G formaldimine at ``point``, the RHF orbitals rotated by
    expm of a seeded skew matrix with entries ~ N(0, 0.1^2), thetas ~ N(0, 0.3^2).  Host work only."""
    from scipy.linalg import expm
    from auto_oo_amd.oo_energy import mo_ao_to_mo_oao
    from tests import _replay
    mol = _replay.sto3g_molecule(*point)
    mol.run_rhf()
    c = np.asarray(mo_ao_to_mo_oao(mol.hf.mo_coeff, mol.overlap))
    k = 0.1 * np.random.default_rng(KAPPA_SEED).standard_normal((mol.nao, mol.nao))
    theta = 0.3 * np.random.default_rng(THETA_SEED).standard_normal(n_theta)
    return mol, c @ expm(np.tril(k, -1) - np.tril(k, -1).T), theta
