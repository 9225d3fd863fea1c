"""Batched determinant CI on the device (ci.hip: oovqe_ci_davidson_batch) and the solver methods built on it:
run_fci / run_casci / run_casscf / run_sa_casscf of Moldata, OO_pqc_batch.casci."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import auto_oo_amd as aoo                                  # noqa: E402
from auto_oo_amd import ci as CI                           # noqa: E402
from auto_oo_amd.oo_energy import OO_energy, mo_ao_to_mo_oao   # noqa: E402
from tests import _ci_dense as D                           # noqa: E402
from tests import _replay as P                             # noqa: E402

DEV = torch.device("cuda", 0)
FCI_HF = [-98.595121449139, -98.283973390815]
with open(os.path.join(os.path.dirname(__file__), "golden", "notebook_runs.json")) as fh:
    RUNS = json.load(fh)


def _t(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float64), device=DEV)


def test_fci_literal_with_singlet_roots():
    mol = aoo.Moldata_sto3g("H 0 0 0; F 0 0 1.1")
    res = mol.run_fci(2)
    assert mol.fci is res and res.converged
    assert np.abs(np.asarray(res.e_tot) - FCI_HF).max() < 1e-6
    assert np.all(np.abs(res.s2) < 1e-8)


def test_fci_out_of_scope_raises_before_launch():
    mol = P.sto3g_molecule(140, 80)
    with pytest.raises(ValueError):
        mol.run_fci()
    with pytest.raises(ValueError):
        mol.run_casci(9, 4)
    with pytest.raises(ValueError):
        mol.run_casci(4, 3)


def test_moldata_without_orbitals_raises_like_run_rhf():
    P_ = aoo.Moldata(np.eye(2), np.zeros((2, 2, 2, 2)), np.eye(2), 0.0, 2)
    with pytest.raises(RuntimeError):
        P_.run_casci(2, 2)


@pytest.mark.parametrize("ncas", [2, 4, 6])
def test_davidson_equals_dense(ncas):
    rng = np.random.default_rng(100 + ncas)
    E = D.excitation_matrices(ncas, ncas)
    for nroots in range(1, 5):
        c0, c1, c2 = D.random_coefficients(ncas, rng)
        H = D.hamiltonian(c0, c1, c2, ncas, ncas, E)
        w, U = np.linalg.eigh(H)
        res = aoo.casci(c0, c1, c2, ncas, ncas, nroots=nroots, fix_singlet=False, tol=1e-10)
        assert bool(res.converged.all()), res.rnorm
        e = res.energies[0].cpu().numpy()
        assert np.abs(e - w[:nroots]).max() < 1e-10
        X = res.ci[0].cpu().numpy()
        assert np.abs(X @ X.T - np.eye(nroots)).max() < 1e-10
        # eigenvectors: by the projector onto each (possibly degenerate) eigenvalue cluster
        for k in range(nroots):
            cl = np.abs(w - w[k]) < 1e-6
            proj = U[:, cl] @ (U[:, cl].T @ X[k])
            assert np.linalg.norm(proj - X[k]) < 1e-7
            assert np.linalg.norm(H @ X[k] - e[k] * X[k]) < 1e-8


def test_davidson_cas88_residual_and_batch():
    rng = np.random.default_rng(8)
    c0, c1, c2 = zip(*[D.random_coefficients(8, rng) for _ in range(2)])
    res = aoo.casci(np.array(c0), np.stack(c1), np.stack(c2), 8, 8, nroots=2)
    assert bool(res.converged.all()), res.rnorm
    Es = D.excitation_matrices(8, 8, sparse=True)
    for b in range(2):
        for k in range(2):
            x = res.ci[b, k].cpu().numpy()
            hx = D.apply_hamiltonian(c0[b], c1[b], c2[b], Es, x)
            assert np.linalg.norm(hx - res.energies[b, k].item() * x) <= 1e-7


def test_small_cases_dc1_and_nroots_equal_dc():
    rng = np.random.default_rng(3)
    c0, c1, c2 = D.random_coefficients(2, rng)
    res = aoo.casci(c0, c1, c2, 2, 0)                          # Dc = 1: the empty string
    assert res.ci.shape == (1, 1, 1) and abs(res.energies.item() - c0) < 1e-12
    res = aoo.casci(c0, c1, c2, 2, 4)                          # Dc = 1: closed shell
    H = D.hamiltonian(c0, c1, c2, 2, 4)
    assert abs(res.energies.item() - H[0, 0]) < 1e-12
    H = D.hamiltonian(c0, c1, c2, 2, 2)
    res = aoo.casci(c0, c1, c2, 2, 2, nroots=4, fix_singlet=False)
    assert np.abs(res.energies[0].cpu().numpy() - np.linalg.eigvalsh(H)).max() < 1e-10
    with pytest.raises(ValueError):
        aoo.casci(c0, c1, c2, 2, 2, nroots=5)
    with pytest.raises(ValueError):
        aoo.casci(c0, c1, c2, 2, 1)


def test_energy_equals_rdm_contraction():
    rng = np.random.default_rng(11)
    for ncas, nel in ((3, 4), (4, 4), (8, 8)):
        c0, c1, c2 = D.random_coefficients(ncas, rng)
        res = aoo.casci(c0, c1, c2, ncas, nel, nroots=2)
        g1, g2 = CI.sector_rdms(res.ci[0], ncas, nel)
        e = c0 + (g1 * _t(c1)).sum((1, 2)) + (g2 * _t(c2)).sum((1, 2, 3, 4))
        assert (e - res.energies[0]).abs().max().item() < 1e-10


def test_casci_and_casscf_literals():
    run = RUNS["tutorial_auto_oo"]
    mol = P.sto3g_molecule(*run["formal_geo"])
    casci = mol.run_casci(run["ncas"], run["nelecas"])
    assert abs(casci.e_tot - run["printed_hf_casci_casscf"][1]) < 1e-6
    casscf = mol.run_casscf(run["ncas"], run["nelecas"])
    assert casscf.converged
    assert abs(casscf.e_tot - run["printed_hf_casci_casscf"][2]) < 1e-6
    # orbital gradient at casscf.mo_coeff
    oo = OO_energy(mol, run["ncas"], run["nelecas"], oao_mo_coeff=mo_ao_to_mo_oao(casscf.mo_coeff, mol.overlap),
                   freeze_active=True)
    c0, c1, c2 = oo.get_active_integrals(oo.mo_coeff)
    res = aoo.casci(c0, c1, c2, run["ncas"], run["nelecas"])
    assert abs(res.energies.item() - casscf.e_tot) < 1e-9
    g1, g2 = CI.sector_rdms(res.ci[0], run["ncas"], run["nelecas"])
    g = oo.kappa_matrix_to_vector(oo.analytic_gradient(g1[0], g2[0]))
    assert g.abs().max().item() <= 1e-5


def test_casscf_berry_point0_literal():
    run = RUNS["tutorial_berry_phase"]
    mol = P.sto3g_molecule(*P.loop_points(run)[0])
    res = mol.run_casscf(run["ncas"], run["nelecas"])
    assert abs(res.e_tot - run["preopt_casscf_energy"]) < 1e-7


def test_sa_casscf():
    mol = P.sto3g_molecule(140, 80)
    res = mol.run_sa_casscf(2, 2)
    assert res.converged
    assert abs(res.e_tot - res.e_states.mean()) < 1e-12
    oo = OO_energy(mol, 2, 2, oao_mo_coeff=mo_ao_to_mo_oao(res.mo_coeff, mol.overlap), freeze_active=True)
    c0, c1, c2 = oo.get_active_integrals(oo.mo_coeff)
    H = D.hamiltonian(c0.item(), c1.cpu().numpy(), c2.cpu().numpy(), 2, 2)
    vecs = np.stack([v.reshape(-1) for v in res.ci])
    for k in range(2):
        assert np.linalg.norm(H @ vecs[k] - res.e_states[k] * vecs[k]) <= 1e-7
    g1, g2 = CI.sector_rdms(_t(vecs), 2, 2)
    g = oo.kappa_matrix_to_vector(oo.analytic_gradient(g1.mean(0), g2.mean(0)))
    assert g.abs().max().item() <= 1e-5


def test_batch_casci_equals_per_geometry():
    pts = [(120 + 2.5 * i, 80 + i) for i in range(16)]
    mols = [aoo.Moldata_sto3g(aoo.get_formal_geo(*p)) for p in pts]
    for m in mols:
        m.run_rhf()
    pqc = aoo.Parameterized_circuit(3, 4, None, ansatz="np_fabric", n_layers=1)
    orbs = [mo_ao_to_mo_oao(m.hf.mo_coeff, m.overlap) for m in mols]
    bat = aoo.OO_pqc_batch(pqc, mols, 3, 4, oao_mo_coeffs=orbs, freeze_active=True)
    e, vecs = bat.casci(nroots=2)
    assert e.shape == (16, 2) and vecs.shape == (16, 2, 9)
    for g, m in enumerate(mols):
        one = m.run_casci(3, 4, n_roots=2)
        assert np.abs(e[g].cpu().numpy() - one.e_tot).max() < 1e-12


def test_batch_cas88_stack_converges():
    rng = np.random.default_rng(88)
    G = 256
    c0, c1, c2 = zip(*[D.random_coefficients(8, rng) for _ in range(4)])
    idx = np.arange(G) % 4
    res = aoo.casci(np.array(c0)[idx], np.stack(c1)[idx], np.stack(c2)[idx], 8, 8, nroots=1)
    assert (res.info == 0).all().item()
    e = res.energies[:, 0].cpu().numpy()
    for k in range(4):
        assert np.array_equal(e[idx == k], np.full((idx == k).sum(), e[k]))     # one workgroup per problem
