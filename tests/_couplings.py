"""Shared by tests/test_couplings_cpu.py and tests/test_couplings_gpu.py: seeded general matrices, dense CI roots, and
the reference of the derivative couplings made from code that existed before
``OO_pqc_batch.casci_derivative_couplings``.

The reference of ``d_IJ^A = <Psi_I | d Psi_J / dR_A>`` is the 4th-order central difference of the EXACT overlaps
``<Psi_I(R_0)|Psi_J(R)>`` of ``OO_pqc_batch.casci_overlaps`` (true AO metric, core included) over the displaced copies of
tests/_casci_gradients.py (+-h, +-2h per coordinate, the same ``oao_mo_coeff`` in every copy) with the centre geometry
added to the stack.  The CI vectors of every copy come from dense host diagonalisation of ``_ci_dense.hamiltonian``, each
sign-aligned to the centre by its dot product; the same difference with h = 2e-3 gives the reference's disagreement with
itself.  Nothing in it comes from the code under test."""
import functools

import numpy as np
import torch

import auto_oo_amd as aoo
from auto_oo_amd.gaussian import BOHR

from . import _casci_gradients as C
from . import _ci_dense

H1, H2 = C.H1, C.H2


def fd4(f, h):
    """(8 (f(+h) - f(-h)) - (f(+2h) - f(-2h))) / 12h of f = (f(+h), f(-h), f(+2h), f(-2h))"""
    return (8.0 * (f[0] - f[1]) - (f[2] - f[3])) / (12.0 * h)


def general_matrices(N, K):
    """K seeded standard-normal [N, N] matrices (seed 300 + k), neither symmetric nor antisymmetric; matrix k is the
    same whatever K"""
    return np.stack([np.random.default_rng(300 + k).standard_normal((N, N)) for k in range(K)])


@functools.lru_cache(maxsize=None)
def _sector_tools(ncas, nelecas):
    E = _ci_dense.excitation_matrices(ncas, nelecas)
    return E, _ci_dense.singlet_basis(_ci_dense.s2_matrix(ncas, nelecas))


def dense_roots(c0, c1, c2, ncas, nelecas, R, fix_singlet):
    """The lowest R eigenpairs of the dense CAS Hamiltonian (of its singlet block with ``fix_singlet``) -> (energies [R],
    vectors [R, Dc])"""
    E, B = _sector_tools(ncas, nelecas)
    H = _ci_dense.hamiltonian(c0, c1, c2, ncas, nelecas, E)
    H = 0.5 * (H + H.T)
    if fix_singlet:
        w, v = np.linalg.eigh(B.T @ H @ B)
        v = B @ v
    else:
        w, v = np.linalg.eigh(H)
    return w[:R], v[:, :R].T.copy()


@functools.lru_cache(maxsize=None)
def coupling_reference(name, ncas, nelecas, g, R, fix_singlet):
    """-> (d [R, R, natm, 3] at h = 1e-3, its disagreement with h = 2e-3, the centre's energies [R], the centre's CI
    vectors [R, Dc] with the signs ``casci`` fixes: the largest |component| positive)"""
    basis, xyz = C.case(name)
    natm = xyz.shape[1]
    stack = np.concatenate([C.fd_stack(xyz[g], H1), C.fd_stack(xyz[g], H2), xyz[g][None]])
    U = [C.rotated_orbitals(name)[g]] * len(stack)
    bd = aoo.OO_pqc_batch.from_geometries(C.circuit(ncas, nelecas), basis, stack * BOHR, ncas, nelecas, oao_mo_coeffs=U)
    c0, c1, c2 = C.cas_coefficients(bd)
    centre = bd.G - 1
    e0, v0 = dense_roots(c0[centre], c1[centre], c2[centre], ncas, nelecas, R, fix_singlet)
    for v in v0:
        if v[np.argmax(np.abs(v))] < 0.0:
            v *= -1.0
    vecs = np.empty((bd.G, R, v0.shape[1]))
    vecs[centre] = v0
    for k in range(centre):
        _, v = dense_roots(c0[k], c1[k], c2[k], ncas, nelecas, R, fix_singlet)
        vecs[k] = v * np.sign(np.einsum("rc,rc->r", v, v0))[:, None]
    pairs = [(centre, k) for k in range(centre)]
    O = bd.casci_overlaps(R, pairs=pairs, fix_singlet=fix_singlet, vecs=torch.as_tensor(vecs))[2].cpu().numpy()
    n = centre // 2
    O = np.moveaxis(O, 0, -1)                                       # [R, R, 2 n]
    a, b = C.fd_combine(O[..., :n], H1), C.fd_combine(O[..., n:], H2)
    assert a.shape == (R, R, natm, 3)
    return a, float(np.abs(a - b).max()), e0, v0
