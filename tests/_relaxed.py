"""Shared by tests/test_relaxed_cpu.py and tests/test_relaxed_gpu.py: a CASCI on host integrals written from the
definitions (RHF by ``gaussian.rhf``, the dense determinant Hamiltonian of tests/_ci_dense.py), its AO densities and
generalised Fock matrix, and the finite-difference references of the orbital-relaxed gradient.

The reference of the CPU tests is the 2nd-order central difference of the CASCI energies with the orbitals RE-SOLVED by
RHF at every displaced geometry, h = 1e-3 Bohr; the same difference at h = 2e-3 gives its disagreement with itself and
every bound is 10 x that figure.  Nothing in a bound comes from the code under test."""
import functools

import numpy as np

from auto_oo_amd import gaussian, nucgrad
from auto_oo_amd.gaussian import BOHR

from . import _ci_dense

H1, H2 = 1e-3, 2e-3
WATER = np.array([[0.0, 0.01, 0.02], [0.3, 0.75, 0.55], [-0.2, -0.70, 0.62]])      # tests/_casci_gradients.py
WATER_SYMBOLS = ("O", "H", "H")
COORDINATES = ((1, 1), (0, 2), (2, 0))       # (atom, axis): H1 y, O z, H2 x


def host_integrals(symbols, xyz_bohr):
    """(S, h, g, nuc) of an STO-3G molecule on the host."""
    m = gaussian.Moldata_sto3g([(s, tuple(r * BOHR)) for s, r in zip(symbols, xyz_bohr)])
    return m.overlap, m.int1e_ao, m.int2e_ao, m.nuc


def host_casci(S, h, g, nuc, nelectron, ncas, nelecas, nroots, mo_coeff=None, mo_energy=None):
    """Singlet CASCI roots on RHF orbitals (made here unless given) -> dict with C, eps, the energies [R] and per root
    the active RDMs in the convention of the batch."""
    n_occ = nelectron // 2
    n_core = (nelectron - nelecas) // 2
    if mo_coeff is None:
        mo_coeff, mo_energy, _ = gaussian.rhf(h, g, S, n_occ, conv_tol=1e-13)
    C = np.asarray(mo_coeff)
    hm = C.T @ h @ C
    gm = np.einsum("pqrs,pi,qj,rk,sl->ijkl", g, C, C, C, C, optimize=True)
    c, a = slice(0, n_core), slice(n_core, n_core + ncas)
    c0 = nuc + 2.0 * np.trace(hm[c, c]) + 2.0 * np.einsum("iijj->", gm[c, c, c, c]) - np.einsum("ijji->", gm[c, c, c, c])
    c1 = hm[a, a] + 2.0 * np.einsum("pqii->pq", gm[a, a, c, c]) - np.einsum("piiq->pq", gm[a, c, c, a])
    c2 = 0.5 * gm[a, a, a, a]
    E = _ci_dense.excitation_matrices(ncas, nelecas)
    H = _ci_dense.hamiltonian(c0, c1, c2, ncas, nelecas, E)
    B = _ci_dense.singlet_basis(_ci_dense.s2_matrix(ncas, nelecas))
    e, v = np.linalg.eigh(B.T @ H @ B)
    vecs = (B @ v[:, :nroots]).T
    gam, Gam = [], []
    for x in vecs:
        Ex = np.einsum("pqij,j->pqi", E, x)                              # E_pq x
        g1 = np.einsum("i,pqi->pq", x, Ex)
        g2 = np.einsum("qpi,rsi->pqrs", Ex, Ex) - np.einsum("qr,ps->pqrs", np.eye(ncas), g1)
        gam.append(g1)
        Gam.append(g2)
    return dict(C=C, eps=np.asarray(mo_energy), e=e[:nroots], gamma=gam, Gamma=Gam, n_occ=n_occ, n_core=n_core)


def host_state_quantities(S, h, g, sol, ncas, root):
    """(D1, D2, F, WQ) of a root of ``host_casci`` from the numpy twins of auto_oo_amd/nucgrad.py."""
    C = sol["C"]
    d1, d2 = nucgrad.cas_ao_densities_host(C, sol["n_core"], ncas, sol["gamma"][root], sol["Gamma"][root])
    F = nucgrad.generalised_fock_host(h, g, S, C, d1, d2)
    s, V = np.linalg.eigh(S)
    U = (V * np.sqrt(s)) @ V.T @ C
    de_dc = 2.0 * (V * np.sqrt(s)) @ V.T @ U @ F.T                      # dE/dC = 2 X^-1 U F^T
    return d1, d2, F, nucgrad.overlap_pullback_host(S, de_dc @ U.T)


@functools.lru_cache(maxsize=None)
def water_stencil():
    """The host integrals of distorted water at the centre and, per coordinate of COORDINATES, at +h, -h for h = 1e-3
    and 2e-3 -> (centre, {(coordinate index, signed step): integrals})."""
    xyz = WATER / BOHR
    out = {}
    for k, (atom, axis) in enumerate(COORDINATES):
        for h in (H1, -H1, H2, -H2):
            r = xyz.copy()
            r[atom, axis] += h
            out[(k, h)] = host_integrals(WATER_SYMBOLS, r)
    return host_integrals(WATER_SYMBOLS, xyz), out


def central(f, k, h):
    """2nd-order central difference of ``f(integrals)`` along coordinate k of ``water_stencil``."""
    st = water_stencil()[1]
    return (f(*st[(k, h)]) - f(*st[(k, -h)])) / (2.0 * h)
