"""Host dense determinant CI for the CI-solver tests: the Hamiltonian of the (N_alpha = N_beta) sector built
from spin-orbital single excitations (spin orbital 2p = alpha_p, 2p + 1 = beta_p; a^+_P a_Q carries the parity
of the occupied spin orbitals strictly between P and Q), in the sector layout c = ia * nb + ib of the circuit
engine.  Independent of the string-driven sigma of the device solver."""
from itertools import combinations
from math import comb

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


def spin_excitation_matrices(ncas, nelecas):
    """(Ea, Eb): nested lists of CSR matrices, E^alpha_pq = a^+_{p alpha} a_{q alpha} and E^beta_pq, built the
    way ``excitation_matrices`` builds their sum."""
    from scipy.sparse import csr_matrix
    a, n = ncas, nelecas // 2
    st = strings(a, n)
    dets = [frozenset(_spin_occ(sa, sb, a)) for sa in st for sb in st]
    index = {d: i for i, d in enumerate(dets)}
    Dc = len(dets)
    trip = [[[([], [], []) for _ in range(a)] for _ in range(a)] for _ in (0, 1)]
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
                    t = trip[s][p][q]
                    t[0].append(index[frozenset(new)]); t[1].append(j); t[2].append(float(sign))
    return tuple([[csr_matrix((t[2], (t[0], t[1])), shape=(Dc, Dc)) for t in row] for row in trip[s]]
                 for s in (0, 1))


def s2_matrix(ncas, nelecas):
    """Dense S^2 of the sector.  At Ms = 0, S^2 = S_- S_+ = N_beta - sum_pq E^alpha_pq E^beta_qp."""
    a, n = ncas, nelecas // 2
    Ea, Eb = spin_excitation_matrices(ncas, nelecas)
    Dc = Ea[0][0].shape[0]
    S = n * np.eye(Dc)
    for p in range(a):
        for q in range(a):
            S -= (Ea[p][q] @ Eb[q][p]).toarray()
    return S


def singlet_count(ncas, nelecas):
    """Number of singlets of ``nelecas`` electrons in ``ncas`` orbitals (Weyl's formula at S = 0)."""
    a, n = ncas, nelecas // 2
    return comb(a + 1, n) * comb(a + 1, n + 1) // (a + 1)


def singlet_basis(S2):
    """Orthonormal basis [Dc, n_singlet] of the null space of the dense S^2."""
    w, U = np.linalg.eigh(S2)
    return U[:, np.abs(w) < 1e-8]


def hamiltonian_sparse(c0, c1, c2, ncas, nelecas, Es=None):
    """The matrix of ``hamiltonian`` assembled from the CSR E_pq of ``excitation_matrices(.., sparse=True)`` and
    turned dense: for sectors whose dense [a, a, Dc, Dc] excitation array does not fit."""
    from scipy.sparse import identity
    a = ncas
    if Es is None:
        Es = excitation_matrices(ncas, nelecas, sparse=True)
    Dc = Es[0][0].shape[0]
    H = c0 * identity(Dc, format="csr")
    for p in range(a):
        for q in range(a):
            inner = (c1[p, q] - sum(c2[p, r, r, q] for r in range(a))) * identity(Dc, format="csr")
            for r in range(a):
                for s in range(a):
                    if c2[p, q, r, s] != 0.0:
                        inner = inner + c2[p, q, r, s] * Es[r][s]
            H = H + Es[p][q] @ inner
    H = H.toarray()
    return 0.5 * (H + H.T)


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
