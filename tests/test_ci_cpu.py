"""Host-side pieces of the CI solver's feature: Cartesian geometry strings, STO-3G fluorine, and the dense
determinant-CI helper the GPU tests compare against (pinned to the reference's FCI literal of HF/STO-3G,
test/test_moldata_pyscf.py:96-104)."""
import numpy as np

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
