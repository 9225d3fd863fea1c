"""Host-side pieces of the CI solver's feature: Cartesian geometry strings, STO-3G fluorine, and the dense
determinant-CI helper the GPU tests compare against (pinned to the reference's FCI literal of HF/STO-3G,
test/test_moldata_pyscf.py:96-104)."""
import numpy as np
import pytest

from auto_oo_amd.gaussian import Moldata_sto3g, rhf, zmatrix_to_cartesian
from tests import _ci_dense as D

FCI_HF = [-98.595121449139, -98.283973390815]


def test_cartesian_string_equals_the_list_form():
    a = Moldata_sto3g("H 0 0 0; F 0 0 1.1")
    b = Moldata_sto3g([("H", (0, 0, 0)), ("F", (0, 0, 1.1))])
    assert a.nao == b.nao == 6 and a.nelectron == b.nelectron == 10
    for x, y in ((a.int1e_ao, b.int1e_ao), (a.int2e_ao, b.int2e_ao), (a.overlap, b.overlap)):
        assert np.array_equal(x, y)
    assert a.nuc == b.nuc


def test_zmatrix_lines_are_unchanged():
    sym, xyz = zmatrix_to_cartesian("N\nC 1 1.5\nH 2 1.0 1 120.0")
    assert sym == ["N", "C", "H"] and np.allclose(xyz[1], [1.5, 0, 0])
    sym, xyz = zmatrix_to_cartesian("O 0.1 0.2 0.3; H 1 0 0")
    assert np.allclose(xyz, [[0.1, 0.2, 0.3], [1, 0, 0]])


def test_dense_fci_reproduces_the_reference_literal():
    mol = Moldata_sto3g("H 0 0 0; F 0 0 1.1")
    C, _, _ = rhf(mol.int1e_ao, mol.int2e_ao, mol.overlap, mol.nelectron // 2)
    c0, c1, c2 = D.mo_coefficients(mol, C)
    H = D.hamiltonian(c0, c1, c2, mol.nao, mol.nelectron)
    w = np.linalg.eigvalsh(H)
    assert abs(w[0] - FCI_HF[0]) < 1e-6
    # the Ms = 0 sector also holds the 3Pi pair (-98.31715) below the 1Pi pair of the second singlet
    assert abs(w[1] - w[2]) < 1e-9 and abs(w[1] + 98.317150) < 1e-5
    assert abs(w[3] - FCI_HF[1]) < 1e-6 and abs(w[4] - FCI_HF[1]) < 1e-6


SHAPES = [(1, 0), (1, 2), (2, 2), (3, 2), (3, 4), (4, 4), (4, 6), (5, 4), (5, 6), (6, 6), (6, 2)]


@pytest.mark.parametrize("ncas,nelecas", SHAPES)
def test_dense_s2_spectrum_and_singlet_count(ncas, nelecas):
    S = D.s2_matrix(ncas, nelecas)
    assert np.array_equal(S, S.T)
    w = np.linalg.eigvalsh(S)
    spin = np.round((-1 + np.sqrt(1 + 4 * np.abs(w))) / 2)         # the S of S (S + 1) nearest each eigenvalue
    assert np.abs(w - spin * (spin + 1)).max() < 1e-10
    assert spin.max() <= min(nelecas, 2 * ncas - nelecas) / 2
    assert int((np.abs(w) < 1e-8).sum()) == D.singlet_count(ncas, nelecas)
    assert D.singlet_basis(S).shape == (S.shape[0], D.singlet_count(ncas, nelecas))


def test_singlet_count_literals():
    # CAS(2,2): 3 singlets of 4 determinants; (4e,4o): 20 of 36; (8e,8o): 1764 of 4900
    assert [D.singlet_count(*s) for s in ((2, 2), (4, 4), (8, 8), (3, 0), (3, 6))] == [3, 20, 1764, 1, 1]


@pytest.mark.parametrize("ncas,nelecas", [(2, 2), (3, 4), (4, 4), (5, 6), (6, 4)])
def test_dense_hamiltonian_commutes_with_s2(ncas, nelecas):
    S = D.s2_matrix(ncas, nelecas)
    for seed in range(3):
        c0, c1, c2 = D.random_coefficients(ncas, np.random.default_rng(1000 + seed))
        H = D.hamiltonian(c0, c1, c2, ncas, nelecas)
        assert np.abs(H @ S - S @ H).max() < 1e-9


@pytest.mark.parametrize("ncas,nelecas", [(4, 4), (5, 4)])
def test_sparse_assembly_equals_dense_hamiltonian(ncas, nelecas):
    for seed in range(2):
        c0, c1, c2 = D.random_coefficients(ncas, np.random.default_rng(1000 + seed))
        H = D.hamiltonian(c0, c1, c2, ncas, nelecas)
        assert np.abs(D.hamiltonian_sparse(c0, c1, c2, ncas, nelecas) - H).max() < 1e-12
    # coefficients without any symmetry: both assemblies take them as given and symmetrise the matrix
    rng = np.random.default_rng(7)
    c1, c2 = rng.standard_normal((ncas,) * 2), rng.standard_normal((ncas,) * 4)
    H = D.hamiltonian(0.3, c1, c2, ncas, nelecas)
    assert np.abs(D.hamiltonian_sparse(0.3, c1, c2, ncas, nelecas) - H).max() < 1e-12
