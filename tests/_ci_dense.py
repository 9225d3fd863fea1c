"""Host dense determinant CI for the CI-solver tests: the Hamiltonian of the (N_alpha = N_beta) sector built
from spin-orbital single excitations (spin orbital 2p = alpha_p, 2p + 1 = beta_p; a^+_P a_Q carries the parity
of the occupied spin orbitals strictly between P and Q), in the sector layout c = ia * nb + ib of the circuit
engine.  Independent of the string-driven sigma of the device solver."""
from itertools import combinations

import numpy as np


def strings(ncas, n):
    out = []
    for occ in combinations(range(ncas), n):
        m = 0
        for p in occ:
            m |= 1 << (ncas - 1 - p)
        out.append(m)
    return sorted(out)


def _spin_occ(sa, sb, a):
    """occupied spin orbitals (sorted) of the determinant (alpha string, beta string)."""
    occ = []
    for p in range(a):
        if sa & (1 << (a - 1 - p)):
            occ.append(2 * p)
        if sb & (1 << (a - 1 - p)):
            occ.append(2 * p + 1)
    return occ


def excitation_matrices(ncas, nelecas, sparse=False):
    """E[p, q] [Dc, Dc]: the spin-summed E_pq = sum_sigma a^+_{p sigma} a_{q sigma} (``sparse``: a nested list of
    scipy CSR matrices instead of the dense array)."""
    a, n = ncas, nelecas // 2
    st = strings(a, n)
    dets = [frozenset(_spin_occ(sa, sb, a)) for sa in st for sb in st]
    index = {d: i for i, d in enumerate(dets)}
    Dc = len(dets)
    E = None if sparse else np.zeros((a, a, Dc, Dc))
    trip = [[([], [], []) for _ in range(a)] for _ in range(a)]
    for j, d in enumerate(dets):
        for p in range(a):
            for q in range(a):
                for s in (0, 1):
                    P, Q = 2 * p + s, 2 * q + s
                    if Q not in d or (P in d and P != Q):
                        continue
                    new = (d - {Q}) | {P}
                    lo, hi = min(P, Q), max(P, Q)
                    sign = (-1) ** sum(1 for x in d if lo < x < hi)
                    if sparse:
                        t = trip[p][q]
                        t[0].append(index[frozenset(new)]); t[1].append(j); t[2].append(float(sign))
                    else:
                        E[p, q, index[frozenset(new)], j] += sign
    if sparse:
        from scipy.sparse import csr_matrix
        return [[csr_matrix((t[2], (t[0], t[1])), shape=(Dc, Dc)) for t in row] for row in trip]
    return E


def apply_hamiltonian(c0, c1, c2, Es, x):
    """H x with the sparse excitation matrices of ``excitation_matrices(.., sparse=True)``."""
    a = len(Es)
    ex = [[Es[r][s] @ x for s in range(a)] for r in range(a)]
    y = c0 * x
    for p in range(a):
        for q in range(a):
            inner = c1[p, q] * x - sum(c2[p, r, r, q] * x for r in range(a))
            inner = inner + sum(c2[p, q, r, s] * ex[r][s] for r in range(a) for s in range(a))
            y = y + Es[p][q] @ inner
    return y


def hamiltonian(c0, c1, c2, ncas, nelecas, E=None):
    """H = c0 + sum c1_pq E_pq + sum c2_pqrs (E_pq E_rs - delta_qr E_ps) as a dense [Dc, Dc] matrix."""
    a = ncas
    if E is None:
        E = excitation_matrices(ncas, nelecas)
    Dc = E.shape[-1]
    H = c0 * np.eye(Dc) + np.einsum("pq,pqij->ij", c1, E)
    Ef = E.reshape(a * a, Dc, Dc)
    c2f = c2.reshape(a * a, a * a)
    for pq in range(a * a):
        Y = np.einsum("r,rij->ij", c2f[pq], Ef)            # sum_rs c2_pqrs E_rs
        H += Ef[pq] @ Y
    H -= np.einsum("pqqs,psij->ij", c2, E)
    return 0.5 * (H + H.T)


def random_coefficients(ncas, rng, scale=1.0):
    """c0, c1 symmetric, c2 = g / 2 with g 8-fold symmetric (real orbitals)."""
    a = ncas
    h = rng.standard_normal((a, a)) * scale
    h = 0.5 * (h + h.T)
    g = rng.standard_normal((a, a, a, a)) * 0.3 * scale
    g = g + g.transpose(1, 0, 2, 3)
    g = g + g.transpose(0, 1, 3, 2)
    g = g + g.transpose(2, 3, 0, 1)
    g = g / 8 + np.einsum("pq,rs->pqrs", np.eye(a), np.eye(a)) * 0.5 * scale   # (a positive Coulomb-like part)
    return float(rng.standard_normal()), h, 0.5 * g


def mo_coefficients(mol, mo):
    """(nuc, h_mo, g_mo / 2): the full-space coefficients of a molecule at AO->MO orbitals mo (host numpy)."""
    h = mo.T @ mol.int1e_ao @ mo
    g = np.einsum("pqrs,pi,qj,rk,sl->ijkl", mol.int2e_ao, mo, mo, mo, mo, optimize=True)
    return mol.nuc, h, 0.5 * g
