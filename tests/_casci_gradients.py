"""Shared by tests/test_casci_gradients_cpu.py and tests/test_casci_gradients_gpu.py: the small molecules of
tests/test_nucgrad_gpu.py restated, seeded density sets, the finite-difference stacks, and the reference of the CASCI
gradient matrix made from code that existed before ``OO_pqc_batch.casci_nuclear_gradients``.

The reference everywhere is the 4th-order central difference (8 (f(+h) - f(-h)) - (f(+2h) - f(-2h))) / 12h with
h = 1e-3 Bohr; the same difference with h = 2e-3 gives its disagreement with itself, and every bound is 10 x that figure
of the very case under test.  Nothing in a bound comes from the code under test."""
import functools

import numpy as np
import torch

import auto_oo_amd as aoo
from auto_oo_amd import gto
from auto_oo_amd.gaussian import BOHR
from auto_oo_amd.moldata import get_formal_geo

from . import _ci_dense

F64 = torch.float64
H1, H2 = 1e-3, 2e-3
POINTS = [(140.0, 80.0), (100.0, 0.0), (180.0, 90.0)]       # tests/test_nucgrad_gpu.py
WATER = np.array([[0.0, 0.01, 0.02], [0.3, 0.75, 0.55], [-0.2, -0.70, 0.62]])


def dev():
    return torch.device("cuda", torch.cuda.current_device())


@functools.lru_cache(maxsize=None)
def formal_basis():
    return gto.GTOBasis(["N", "C", "H", "H", "H"])


@functools.lru_cache(maxsize=None)
def case(name):
    """(basis, coordinates [G, natm, 3] in Bohr as a host array): one geometry, formaldimine at the three POINTS"""
    if name == "h2":
        # one 1-primitive and one 6-primitive s shell per atom (36 primitive pairs are no multiple of 8), off-axis
        table = {"H": [(0, [0.6], [1.0]),
                       (0, [30.0, 8.0, 2.5, 0.9, 0.35, 0.12], [0.02, 0.08, 0.25, 0.4, 0.3, 0.1])]}
        return gto.GTOBasis(["H", "H"], table), np.array([[[0.1, 0.2, 0.3], [0.55, -0.35, 0.8]]]) / BOHR
    if name == "hf":
        return gto.GTOBasis(["H", "F"]), np.array([[[0.0, 0.0, 0.0], [0.0, 0.0, 1.1]]]) / BOHR
    if name == "water":
        return gto.GTOBasis(["O", "H", "H"]), WATER[None] / BOHR
    basis = formal_basis()
    return basis, basis.coordinates([get_formal_geo(*p) for p in POINTS]) / BOHR


def five_geometries():
    pts = POINTS + [(120.0, 40.0), (160.0, 60.0)]
    return formal_basis().coordinates([get_formal_geo(*p) for p in pts]) / BOHR


def fd_stack(xyz, h):
    """[natm, 3] (Bohr, host) -> [4 * 3 * natm, natm, 3]: per coordinate +h, -h, +2h, -2h."""
    natm = xyz.shape[0]
    out = np.repeat(xyz[None], 12 * natm, axis=0)
    for a in range(natm):
        for d in range(3):
            for k, s in enumerate((1.0, -1.0, 2.0, -2.0)):
                out[(a * 3 + d) * 4 + k, a, d] += s * h
    return out


def fd_combine(f, h):
    """f [..., 4 * 3 * natm] of the stack above -> [..., natm, 3]"""
    f = f.reshape(f.shape[:-1] + (-1, 3, 4))
    return (8.0 * (f[..., 0] - f[..., 1]) - (f[..., 2] - f[..., 3])) / (12.0 * h)


# ---- seeded density sets ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def density_sets(name, K):
    """K sets of seeded standard-normal D1, WQ, D2 (seed 100 + k), symmetrised by adding their transposes -> device
    tensors [K, N, N], [K, N, N], [K, N, N, N, N]; set k is the same whatever K"""
    N = case(name)[0].nao
    out = ([], [], [])
    for k in range(K):
        rng = np.random.default_rng(100 + k)
        d1, wq, d2 = rng.standard_normal((N, N)), rng.standard_normal((N, N)), rng.standard_normal((N,) * 4)
        d1, wq = d1 + d1.T, wq + wq.T
        d2 = d2 + d2.transpose(1, 0, 2, 3)
        d2 = d2 + d2.transpose(0, 1, 3, 2)
        d2 = d2 + d2.transpose(2, 3, 0, 1)
        for lst, x in zip(out, (d1, wq, d2)):
            lst.append(x)
    return tuple(torch.as_tensor(np.stack(x)).to(dev()).contiguous() for x in out)


def nuc_bits(K):
    """alternating nuclear flags, set 0 with the term"""
    return [k % 2 == 0 for k in range(K)]


def expand(t, G):
    return t[None].expand((G,) + tuple(t.shape)).contiguous()


# ---- orbitals and batches ---------------------------------------------------------------------------------------------
def circuit(ncas, nelecas):
    if (ncas, nelecas) == (2, 2):
        return aoo.Parameterized_circuit(2, 2, None, ansatz="np_fabric", n_layers=1)
    return aoo.Parameterized_circuit(ncas, nelecas, None, ansatz="ucc")


@functools.lru_cache(maxsize=None)
def rotated_orbitals(name):
    """OAO -> MO coefficients per geometry of the case: device RHF times expm of a seeded skew matrix of norm 0.1, so
    that the pull-back through S^-1/2 is exercised"""
    basis, xyz = case(name)
    b = aoo.OO_pqc_batch.from_geometries(circuit(2, 2), basis, xyz * BOHR, 2, 2, oao_mo_coeffs="rhf")
    rng = np.random.default_rng(17)
    out = []
    for U in b.oao_mo_coeff.cpu().numpy():
        K = rng.standard_normal(U.shape)
        K = K - K.T
        K *= 0.1 / np.linalg.norm(K)
        out.append(U @ torch.linalg.matrix_exp(torch.as_tensor(K)).numpy())
    return out


@functools.lru_cache(maxsize=None)
def batch(name, ncas, nelecas):
    basis, xyz = case(name)
    return aoo.OO_pqc_batch.from_geometries(circuit(ncas, nelecas), basis, xyz * BOHR, ncas, nelecas,
                                            oao_mo_coeffs=rotated_orbitals(name))


def cas_coefficients(b):
    """c0 [G], c1 [G, a, a], c2 [G, a, a, a, a] of every geometry of a batch (host arrays), read from the batch's CAS
    call exactly as ``OO_pqc_batch.casci`` reads them"""
    a, G = b.ncas, b.G
    zero1 = torch.zeros((G, 1, a, a), dtype=F64, device=b.device)
    zero2 = torch.zeros((G, 1) + (a,) * 4, dtype=F64, device=b.device)
    cas, _, _ = b._cas_batch(zero1, zero2, G)
    cas = cas.cpu().numpy()
    o = 3 + b.n_kappa
    return (cas[:, 0], cas[:, o:o + a * a].reshape(G, a, a),
            cas[:, o + a * a:o + a * a + a ** 4].reshape((G,) + (a,) * 4))


def displaced_batch(name, ncas, nelecas, g):
    """the 2 x 12 natm copies of geometry g of the case displaced by h = 1e-3 and 2e-3, the same orbitals in each"""
    basis, xyz = case(name)
    stack = np.concatenate([fd_stack(xyz[g], h) for h in (H1, H2)])
    U = [rotated_orbitals(name)[g]] * len(stack)
    return aoo.OO_pqc_batch.from_geometries(circuit(ncas, nelecas), basis, stack * BOHR, ncas, nelecas, oao_mo_coeffs=U)


def matrix_reference(name, ncas, nelecas, g, ci_vectors, nroots=None, fix_singlet=True):
    """Finite differences of ``M(R) = c^T H_dense(R) c`` with the CI vectors ``ci_vectors`` [R, Dc] (host) of the centre
    held fixed -> (matrix [R, R, natm, 3] at h = 1e-3, its disagreement with h = 2e-3, and -- ``nroots`` given -- the
    same two for the finite differences of the ``casci`` energies [R, natm, 3] of the displaced copies)."""
    bd = displaced_batch(name, ncas, nelecas, g)
    c0, c1, c2 = cas_coefficients(bd)
    E = _ci_dense.excitation_matrices(ncas, nelecas)
    c = np.asarray(ci_vectors)
    M = np.stack([c @ _ci_dense.hamiltonian(c0[k], c1[k], c2[k], ncas, nelecas, E) @ c.T for k in range(bd.G)])
    n = bd.G // 2
    M = np.moveaxis(M, 0, -1)                                    # [R, R, 2 n]
    a, b = fd_combine(M[..., :n], H1), fd_combine(M[..., n:], H2)
    out = (a, np.abs(a - b).max())
    if nroots is not None:
        e = bd.casci(nroots, fix_singlet)[0].cpu().numpy().T     # [R, 2 n]
        ea, eb = fd_combine(e[:, :n], H1), fd_combine(e[:, n:], H2)
        out += (ea, np.abs(ea - eb).max())
    return out
