"""Host-side checks of the orbital-relaxed CASCI gradients (no device): the numpy twins of the Z-vector equations and of
the relaxed densities against finite differences of CASCI energies whose orbitals are re-solved by RHF at every
displaced geometry, the block elimination against the full linear system, the new symbols and the refusals that need no
device.

Distorted water, STO-3G, CAS(2e,2o), singlet roots 0 and 1, the coordinates H1 y, O z, H2 x (tests/_relaxed.py).
Measured here (Hartree / Bohr), per (root, coordinate): the reference's disagreement with itself between h = 1e-3 and
2e-3 is 1.7e-9 .. 1.2e-6, so the bounds are 1.7e-8 .. 1.2e-5; the relaxed formula misses the reference by 6e-10 ..
3.9e-7 (about a thirtieth of its bound, i.e. the reference's own error at h = 1e-3); the fixed-orbital
derivative misses it by 1.2e-4 .. 2.7e-2."""
import ctypes
import os
import re

import numpy as np
import pytest

from auto_oo_amd import _lib, nucgrad, scf

from . import _relaxed as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("oovqe_fock_jk_sets_batch", "oovqe_zvector_work_size", "oovqe_zvector_solve_batch", "oovqe_response_d2_batch")
NELECTRON, NCAS, NELECAS, NROOTS = 10, 2, 2, 2


def test_new_symbols_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "oovqe.h")) as fh:
        header = fh.read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    for name in ("orbital_gradient", "zvector", "relaxed_densities", "response_d2", "zvector_host",
                 "relaxed_densities_host"):
        assert hasattr(nucgrad, name), name
    assert hasattr(scf, "fock_jk_sets")


def test_work_size_answers_without_a_device_and_refuses_what_is_out_of_scope():
    lib = _lib.load()
    n, no, K, G = 13, 8, 2, 5
    size = lib.oovqe_zvector_work_size(n, no, K, G)
    # trial density, J, K and the vectors r, p of every (geometry, set)
    assert size >= G * K * (3 * n * n + 2 * no * (n - no))
    for bad in ((1, 1, 1, 1), (65, 8, 1, 1), (13, 0, 1, 1), (13, 13, 1, 1), (13, 8, 0, 1), (13, 8, 11, 1), (13, 8, 2, 0)):
        assert lib.oovqe_zvector_work_size(*bad) < 0, bad
        assert "oovqe_zvector_work_size" in lib.oovqe_last_error().decode()


def _centre():
    (S, h, g, nuc), _ = R.water_stencil()
    sol = R.host_casci(S, h, g, nuc, NELECTRON, NCAS, NELECAS, NROOTS)
    return S, h, g, nuc, sol


def _energies(S, h, g, nuc):
    return R.host_casci(S, h, g, nuc, NELECTRON, NCAS, NELECAS, NROOTS)["e"]


def _contraction(d1, d2, wq):
    return lambda S, h, g, nuc: (d1 * h).sum() + 0.5 * (d2 * g).sum() + (wq * S).sum() + nuc


def _derivative(f, k):
    """the derivative of a function that is LINEAR in the integrals: Richardson's combination of the two steps, so that
    what is left of the stencil's error (h^4) is far below every bound"""
    return (4.0 * R.central(f, k, R.H1) - R.central(f, k, R.H2)) / 3.0


def test_orbital_gradient_sign_against_a_finite_difference_of_the_host_energy():
    """w_pq = 2 (F_qp - F_pq) = dE_I / dkappa_pq for C exp(kappa), on a virt-occ, a core-active and an active-external
    pair, against the central difference of the host CASCI energy at kappa_pq = +-1e-4 (error ~1e-8 |w|)."""
    from scipy.linalg import expm
    S, h, g, nuc, sol = _centre()
    C, N = sol["C"], sol["C"].shape[0]
    for root in range(NROOTS):
        w = nucgrad.orbital_gradient_host(R.host_state_quantities(S, h, g, sol, NCAS, root)[2])
        for p, q in ((5, 2), (4, 1), (6, 5)):
            def e_of(t):
                k = np.zeros((N, N))
                k[p, q], k[q, p] = t, -t
                return R.host_casci(S, h, g, nuc, NELECTRON, NCAS, NELECAS, NROOTS, C @ expm(k), sol["eps"])["e"][root]
            fd = (e_of(1e-4) - e_of(-1e-4)) / 2e-4
            assert abs(w[p, q] - fd) < 1e-7 * max(1.0, abs(fd)) + 1e-9, (root, p, q, w[p, q], fd)
        # inside a class the CASCI energy does not change
        vo, dg = nucgrad.response_pairs(N, sol["n_core"], NCAS, sol["n_occ"])
        inside = np.tril(np.ones((N, N), dtype=bool), -1) & ~vo & ~dg
        assert np.abs(w[inside]).max() < 1e-10


def test_block_elimination_equals_the_full_linear_system():
    """Steps 2 to 4 (the occ-occ and virt-virt pairs, the right-hand side, the symmetric virt-occ system) against the
    dense solve of L^T z = w over all pairs: 1e-12.  A is symmetric and positive definite."""
    S, h, g, nuc, sol = _centre()
    for root in range(NROOTS):
        w = nucgrad.orbital_gradient_host(R.host_state_quantities(S, h, g, sol, NCAS, root)[2])
        args = (g, sol["C"], sol["eps"], sol["n_core"], NCAS, sol["n_occ"], w)
        z = nucgrad.zvector_host(*args)
        z2, A, b = nucgrad.zvector_host(*args, eliminate=True)
        print(f"root {root}: max |z| = {np.abs(z).max():.3e}, elimination - full = {np.abs(z - z2).max():.3e}")
        assert np.abs(z - z2).max() < 1e-12
        assert np.abs(A - A.T).max() < 1e-12
        assert np.linalg.eigvalsh(0.5 * (A + A.T)).min() > 0.0
        assert np.abs(np.triu(z)).max() == 0.0


@pytest.mark.parametrize("root", range(NROOTS))
def test_relaxed_densities_against_the_total_finite_difference(root):
    """dE_I/dR with the RHF orbitals re-solved at every displacement, against D1_rel . dh + 1/2 D2_rel . dg + WQ_rel .
    dS + dE_nuc.  Bound per coordinate: 10 x the disagreement of the reference between h = 1e-3 and 2e-3.  The
    fixed-orbital derivative must lie OUTSIDE that bound."""
    S, h, g, nuc, sol = _centre()
    d1, d2, F, wq = R.host_state_quantities(S, h, g, sol, NCAS, root)
    assert abs((d1 * h).sum() + 0.5 * (d2 * g).sum() + nuc - sol["e"][root]) < 1e-10
    z = nucgrad.zvector_host(g, sol["C"], sol["eps"], sol["n_core"], NCAS, sol["n_occ"], nucgrad.orbital_gradient_host(F))
    rel = nucgrad.relaxed_densities_host(h, g, S, sol["C"], sol["n_occ"], z, d1, d2, wq)
    for k in range(len(R.COORDINATES)):
        total = [R.central(lambda *a: _energies(*a)[root], k, step) for step in (R.H1, R.H2)]
        bound = 10.0 * abs(total[0] - total[1])
        fixed = _derivative(_contraction(d1, d2, wq), k)
        relaxed = _derivative(_contraction(*rel), k)
        print(f"root {root} coordinate {R.COORDINATES[k]}: total {total[0]:+.8f} fixed {fixed:+.8f} relaxed "
              f"{relaxed:+.8f} | relaxed - total {relaxed - total[0]:+.2e}, fixed - total {fixed - total[0]:+.2e}, "
              f"bound {bound:.2e}")
        assert abs(relaxed - total[0]) < bound
        assert abs(fixed - total[0]) > bound


def test_host_side_argument_errors_and_refusals():
    with pytest.raises(ValueError, match="Fermi level"):
        nucgrad.response_pairs(7, 5, 2, 5 + 3)
    with pytest.raises(ValueError, match="Fermi level"):
        nucgrad.response_pairs(7, 3, 2, 2)
    vo, dg = nucgrad.response_pairs(7, 4, 2, 5)
    assert vo.sum() == 10 and dg.sum() == 4 + 1 and not (vo & dg).any()
    assert dg[4, :4].all() and dg[6, 5]
    # no core, one occupied orbital (h2): nothing inside occ-occ
    vo, dg = nucgrad.response_pairs(4, 0, 2, 1)
    assert vo.sum() == 3 and dg.sum() == 2 and dg[2:, 1].all()
    import torch
    with pytest.raises(TypeError):
        scf.fock_jk_sets(None, np.zeros((2, 3, 3)))
    with pytest.raises(ValueError, match="densities per geometry"):
        scf.fock_jk_sets(torch.zeros((3,) * 4, dtype=torch.float64), torch.zeros((11, 3, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="fock_jk_sets covers"):
        scf.fock_jk_sets(torch.zeros((65,) * 4, dtype=torch.float64, device="meta"),
                         torch.zeros((1, 65, 65), dtype=torch.float64, device="meta"))
    with pytest.raises(ValueError, match=r"expected \[G, K, N, N\]"):
        nucgrad.zvector(None, None, None, 0, 2, 1, torch.zeros((4, 4), dtype=torch.float64))
