"""Host-side checks of the nuclear-gradient feature (no device): the new symbols, the size function and its limits, the
overlap pull-back formula against autograd through ``eigh``, and the numpy twins of the device helpers against the CPU
oracle."""
import ctypes
import os
import re

import numpy as np
import torch

from auto_oo_amd import _lib, gto, nucgrad
from oracle import cpu_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("oovqe_gto_gradient_work_size", "oovqe_gto_gradient_batch", "oovqe_cas_ao_densities_batch")


def test_new_symbols_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "oovqe.h")) as fh:
        header = fh.read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert hasattr(gto, "gradient_batch") and hasattr(gto, "gradient_into")


def test_work_size_answers_without_a_device_and_refuses_too_many_primitives():
    lib = _lib.load()
    nshell, natm, G = 9, 5, 4
    base = lib.oovqe_gto_work_size(nshell, 3, G)
    size = lib.oovqe_gto_gradient_work_size(nshell, 3, natm, G)
    npair = nshell * (nshell + 1) // 2
    assert base > 0 and size > base
    # room for the records of every pair (one per nucleus and one for S, T) and of both sides of every unique quartet
    assert size - base >= G * (npair * (natm + 1) + npair * (npair + 1)) * 16
    assert lib.oovqe_gto_gradient_work_size(nshell, 3, natm, 0) == lib.oovqe_gto_work_size(nshell, 3, 0)
    assert lib.oovqe_gto_gradient_work_size(nshell, gto.MAX_PRIM, natm, G) > 0
    assert lib.oovqe_gto_gradient_work_size(nshell, gto.MAX_PRIM + 1, natm, G) < 0
    msg = lib.oovqe_last_error().decode()
    assert "oovqe_gto_gradient_work_size" in msg and f"{gto.MAX_PRIM + 1} primitives" in msg
    assert lib.oovqe_gto_gradient_work_size(nshell, 3, 0, G) < 0
    assert "natm" in lib.oovqe_last_error().decode()


def test_overlap_pullback_formula_matches_autograd_through_eigh():
    """E(S) = tr(G_X S^-1/2) for a fixed symmetric G_X: dE/dS from the divided-difference formula of
    ``nucgrad.overlap_pullback_host`` against torch autograd through ``eigh``, on a random SPD matrix, to 1e-12."""
    rng = np.random.default_rng(11)
    n = 9
    a = rng.standard_normal((n, n))
    S = a @ a.T / n + 0.5 * np.eye(n)
    gx = rng.standard_normal((n, n))
    gx = gx + gx.T
    St = torch.tensor(S, requires_grad=True)
    w, V = torch.linalg.eigh(0.5 * (St + St.T))
    X = V @ torch.diag(w ** -0.5) @ V.T
    (torch.tensor(gx) * X).sum().backward()
    wq = nucgrad.overlap_pullback_host(S, gx)
    assert np.abs(wq - wq.T).max() < 1e-13
    assert np.abs(wq - St.grad.numpy()).max() < 1e-12


def _oracle_problem():
    N, ncas, nelecas, nelec = 7, 3, 4, 8
    P = R.synthetic_problem(N, 3)
    mol = R.OracleMol(P["int1e_ao"], P["int2e_ao"], P["overlap"], P["nuc"], nelec)
    oo = R.OracleOOEnergy(mol, ncas, nelecas, P["oao_mo_coeff"])
    pqc = R.OraclePQC(ncas, nelecas, "ucc")
    theta = torch.tensor(np.random.default_rng(0).uniform(0, 2 * np.pi, pqc.theta_shape))
    g1, g2 = pqc.get_rdms(theta)
    return P, oo, g1, g2


def test_host_twin_of_the_ao_densities_reproduces_the_oracle_energy():
    """The convention of D1 / D2 against the energy expression of oracle/cpu_ref.py: D1 . h + 1/2 D2 . g + nuc = E."""
    P, oo, g1, g2 = _oracle_problem()
    C = oo.mo_coeff
    E = oo.energy_from_mo_coeff(C, g1, g2).item()
    d1, d2 = nucgrad.cas_ao_densities_host(C.numpy(), len(oo.occ_idx), oo.ncas, g1.numpy(), g2.numpy())
    h, g = np.asarray(P["int1e_ao"]), np.asarray(P["int2e_ao"])
    assert abs((d1 * h).sum() + 0.5 * (d2 * g).sum() + P["nuc"] - E) < 1e-10
    for perm in ((1, 0, 2, 3), (0, 1, 3, 2), (2, 3, 0, 1)):
        assert np.abs(d2 - d2.transpose(perm)).max() < 1e-14


def test_orbital_derivative_of_the_energy_is_twice_the_fock_matrix_pulled_back():
    """dE/dC = C^-T (2 F^T), F the generalised Fock matrix: what ``nucgrad.overlap_pullback`` starts from."""
    _, oo, g1, g2 = _oracle_problem()
    C = oo.mo_coeff.clone().requires_grad_(True)
    oo.energy_from_mo_coeff(C, g1, g2).backward()
    Cd = C.detach()
    F = oo.fock_generalized(R.int1e_transform(oo.int1e_ao, Cd), R.int2e_transform(oo.int2e_ao, Cd), g1, g2)
    assert (torch.linalg.inv(Cd).T @ (2 * F.T) - C.grad).abs().max().item() < 1e-11
