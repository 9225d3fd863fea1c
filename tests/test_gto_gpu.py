"""The batched device integral engine (csrc/gto.hip, auto_oo_amd/gto.py, OO_pqc_batch.from_geometries /
set_geometries) against the host integrals of auto_oo_amd/gaussian.py and the reference's literals.

Bounds (none of them taken from what the device code gives):

* Boys function: relative 2.5e-14 = 10 x the error of the host function ``gaussian._boys`` itself against 40-digit
  arithmetic (mpmath; at most 2.3e-15 relative for n <= 4 on [0, 400], 4.8e-16 on [400, 2000]): the device cannot be
  asked to agree with the host more closely than the host agrees with the truth.
* Integrals, element by element: the host integrals of all test geometries (formaldimine at (140, 80), (100, 0),
  (180, 90), the 16-point ring, H-F) were built twice on the CPU, once as they are and once with ``gaussian._boys``
  multiplied by 1 + 2.5e-14 * (+-1 at random) -- the disagreement the Boys test allows.  Largest elementwise
  difference over all these geometries: MEASURED_H = 9.4e-13 for h (ring point 8), MEASURED_G = 4.9e-14 for g (H-F);
  on the three formaldimine points alone 8.1e-13 and 4.2e-14.  The test bounds are 10 x these (the factor covers the
  different summation order of the kernels): 9.4e-12 for ``int1e_ao``, 4.9e-13 for ``int2e_ao`` and, having no Boys
  function of their own, for ``overlap`` and ``nuc``.
* S^-1/2: 1e-10 against ``moldata.ao_to_oao`` and 2e-8 against the reference's 9-digit literal, the figures of
  tests/test_molecule_goldens.py.
* Energies and gradients 1e-9 (the project's bound), Hessians 1e-8 (tests/test_newton_gpu.py).
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import auto_oo_amd as aoo                                   # noqa: E402
from auto_oo_amd import gaussian, gto, ops                  # noqa: E402
from auto_oo_amd.gaussian import Moldata_sto3g              # noqa: E402
from auto_oo_amd.moldata import ao_to_oao, get_formal_geo   # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "molecule_cases.json")) as fh:
    CASES = json.load(fh)
with open(os.path.join(HERE, "golden", "notebook_runs.json")) as fh:
    BERRY = json.load(fh)["tutorial_berry_phase"]

BOYS_RTOL = 2.5e-14
MEASURED_H, MEASURED_G = 9.4e-13, 4.9e-14
TOL_H, TOL_G = 10 * MEASURED_H, 10 * MEASURED_G
E_RHF, E_CAS22 = -92.66372193556138, -92.74923236954386

POINTS = [(140.0, 80.0), (100.0, 0.0), (180.0, 90.0)]
HF = "H 0 0 0; F 0 0 1.1"


def ring(n=16):
    """n points around the loop of the Berry-phase notebook (tests/_replay.loop_points, closed ring)."""
    phase = np.pi / BERRY["phase_pi_over"]
    return [(BERRY["origin"][0] + BERRY["radius"][0] * np.cos(2 * np.pi * k / n + phase),
             BERRY["origin"][1] + BERRY["radius"][1] * np.sin(2 * np.pi * k / n + phase)) for k in range(n)]


@functools.lru_cache(maxsize=None)
def host_mol(geometry):
    return Moldata_sto3g(geometry)


def formal(p):
    return get_formal_geo(*p)


@functools.lru_cache(maxsize=None)
def formal_basis():
    return gto.GTOBasis(["N", "C", "H", "H", "H"])


def case(name):
    return [c for c in CASES if c["test"] == name][0]


def np_fabric():
    return aoo.Parameterized_circuit(2, 2, None, ansatz="np_fabric", n_layers=1)


def rhf_orbitals(geometry):
    m = host_mol(geometry)
    m.run_rhf()
    return aoo.mo_ao_to_mo_oao(m.hf.mo_coeff, m.overlap)


# ---- 1. Boys function ---------------------------------------------------------------------------------------------
def test_boys_function_against_the_host():
    """oovqe_boys, n = 0..4, against gaussian._boys at T = 0, on a grid over [0, 40] and on one over [40, 2000]:
    relative difference below 2.5e-14 (10 x the host function's own error of 2.3e-15, see the module docstring)."""
    T = np.concatenate(([0.0], np.linspace(0.0, 40.0, 4001), np.linspace(40.0, 2000.0, 4001)))
    ref = np.stack([gaussian._boys(n, T) for n in range(5)], axis=1)
    for nmax in range(5):
        F = gto.boys(nmax, torch.as_tensor(T).cuda()).cpu().numpy()
        rel = np.abs(F - ref[:, :nmax + 1]) / ref[:, :nmax + 1]
        print(f"boys nmax={nmax}: max rel {rel.max():.3e} at T = {T[np.argmax(rel.max(axis=1))]}")
        assert rel.max() < BOYS_RTOL
    assert gto.boys(4, torch.zeros(1, dtype=torch.float64).cuda()).cpu().numpy()[0] == pytest.approx(
        [1.0, 1 / 3, 1 / 5, 1 / 7, 1 / 9], rel=BOYS_RTOL)


# ---- 2. + 3. integrals element by element, exact structure ----------------------------------------------------------
def _compare(I, k, mol, label):
    d = {"overlap": np.abs(I.overlap[k].cpu().numpy() - mol.overlap).max(),
         "int1e_ao": np.abs(I.int1e_ao[k].cpu().numpy() - mol.int1e_ao).max(),
         "int2e_ao": np.abs(I.int2e_ao[k].cpu().numpy() - mol.int2e_ao).max(),
         "nuc": abs(I.nuc[k].item() - mol.nuc)}
    print(label, {n: f"{v:.2e}" for n, v in d.items()})
    assert d["overlap"] < TOL_G and d["int2e_ao"] < TOL_G and d["nuc"] < TOL_G and d["int1e_ao"] < TOL_H
    assert np.abs(I.oao_coeff[k].cpu().numpy() - ao_to_oao(mol.overlap)).max() < 1e-10


def _assert_exact_structure(I):
    g = I.int2e_ao
    assert torch.equal(g, g.permute(0, 2, 1, 3, 4)) and torch.equal(g, g.permute(0, 1, 2, 4, 3))
    assert torch.equal(g, g.permute(0, 3, 4, 1, 2))
    assert torch.equal(I.overlap, I.overlap.transpose(1, 2)) and torch.equal(I.int1e_ao, I.int1e_ao.transpose(1, 2))
    assert torch.equal(I.oao_coeff, I.oao_coeff.transpose(1, 2))
    assert not torch.isnan(g).any() and int(I.info.abs().sum()) == 0


def test_formaldimine_integrals_element_by_element():
    geos = [formal(p) for p in POINTS]
    I = gto.integrals_batch(formal_basis(), geos)
    for k, geo in enumerate(geos):
        _compare(I, k, host_mol(geo), f"formaldimine {POINTS[k]}")
    _assert_exact_structure(I)


def test_ring_integrals_element_by_element():
    geos = [formal(p) for p in ring()]
    I = gto.integrals_batch(formal_basis(), geos)
    for k, geo in enumerate(geos):
        _compare(I, k, host_mol(geo), f"ring point {k}")
    _assert_exact_structure(I)


def test_hydrogen_fluoride_integrals_element_by_element():
    """Atoms on an axis (exact zeros in P - Q), one-centre quartets (T = 0), a second element table, nao = 6."""
    basis = gto.GTOBasis(["H", "F"])
    assert basis.nao == 6
    I = gto.integrals_batch(basis, [HF])
    _compare(I, 0, host_mol(HF), "HF")
    _assert_exact_structure(I)
    # the same through coordinates and through an explicit basis dict
    par = gaussian._STO3G
    table = {"H": [("s", par["H"]["1s"], gaussian._STO3G_1S_COEF)],
             "F": [(0, par["F"]["1s"], gaussian._STO3G_1S_COEF), (0, par["F"]["2sp"], gaussian._STO3G_2S_COEF),
                   (1, par["F"]["2sp"], gaussian._STO3G_2P_COEF)]}
    J = gto.integrals_batch(gto.GTOBasis(["H", "F"], table), np.array([[[0, 0, 0], [0, 0, 1.1]]], dtype=float))
    assert torch.equal(I.int2e_ao, J.int2e_ao) and torch.equal(I.int1e_ao, J.int1e_ao)


def test_batch_reports_both_symmetry_flags_after_set_geometries():
    pts = ring()[:4]
    batch = aoo.OO_pqc_batch.from_geometries(np_fabric(), formal_basis(), [formal(p) for p in pts], 2, 2,
                                             oao_mo_coeffs=[rhf_orbitals(formal(pts[0]))] * 4, freeze_active=True)
    assert batch.eri_flags == 3 and batch._eri_packed is not None
    batch.set_geometries([formal(p) for p in ring()[4:8]])
    assert batch.eri_flags == 3 and batch._eri_packed is not None
    assert ops.eri_flags(batch.int2e_ao[2]) == 3
    batch.set_geometries([formal(ring()[9])], index=[1])
    assert batch.eri_flags == 3 and batch._eri_packed is not None


# ---- 4. S^-1/2 ------------------------------------------------------------------------------------------------------
def test_invsqrt_against_the_reference_literal():
    c = case("test_ao_to_oao")
    I = gto.integrals_batch(formal_basis(), [formal(tuple(c["geometry"]["formal_geo"]))])
    X = I.oao_coeff[0].cpu().numpy()
    print("S^-1/2 vs literal", np.abs(X - np.array(c["oao_coeff_ref"])).max())
    assert np.abs(X - np.array(c["oao_coeff_ref"])).max() < 2e-8
    assert np.abs(X - ao_to_oao(I.overlap[0].cpu().numpy())).max() < 1e-10


def test_invsqrt_batch_flags_a_dependent_overlap_and_solves_the_rest():
    rng = np.random.default_rng(7)
    mats = []
    for n_bad in (0, 1, 0, 0):
        q, _ = np.linalg.qr(rng.standard_normal((13, 13)))
        w = rng.uniform(0.05, 2.0, 13)
        if n_bad:
            w[4] = 0.1 * gto.INVSQRT_MIN_EIG              # one eigenvalue below the documented threshold
        m = q @ np.diag(w) @ q.T
        mats.append(0.5 * (m + m.T))
    S = torch.as_tensor(np.stack(mats)).cuda()
    X, info = gto.sym_invsqrt_batch(S)
    assert info.cpu().tolist() == [0, -1, 0, 0]
    assert torch.isnan(X[1]).all()
    for k in (0, 2, 3):
        ref = ao_to_oao(mats[k])
        assert np.abs(X[k].cpu().numpy() - ref).max() < 1e-10 * max(1.0, np.abs(ref).max())
        assert torch.equal(X[k], X[k].T)
    # the limits of the entry points come back as errors, not as garbage
    with pytest.raises(aoo._lib.OovqeError):
        gto.sym_invsqrt_batch(torch.eye(gto.INVSQRT_MAX_N + 1, dtype=torch.float64).cuda()[None])


# ---- 5. end to end --------------------------------------------------------------------------------------------------
def test_batch_from_geometries_matches_batch_from_host_molecules():
    geos = [formal(p) for p in POINTS]
    pqc = np_fabric()
    coeffs = [rhf_orbitals(g) for g in geos]
    dev = aoo.OO_pqc_batch.from_geometries(pqc, formal_basis(), geos, 2, 2, oao_mo_coeffs=coeffs, freeze_active=True)
    host = aoo.OO_pqc_batch(pqc, [host_mol(g) for g in geos], 2, 2, oao_mo_coeffs=coeffs, freeze_active=True)
    thetas = torch.as_tensor(np.random.default_rng(3).uniform(-0.5, 0.5, (3, dev.n_theta))).cuda()
    a, b = dev.energy_and_gradient(thetas), host.energy_and_gradient(thetas)
    print("dE", (a[:, 0] - b[:, 0]).abs().max().item(), "dgrad", (a[:, 1:] - b[:, 1:]).abs().max().item())
    assert (a[:, 0] - b[:, 0]).abs().max().item() < 1e-9
    assert (a[:, 1:] - b[:, 1:]).abs().max().item() < 1e-9
    Ea, ga, Ha = dev.energy_gradient_hessian(thetas)
    Eb, gb, Hb = host.energy_gradient_hessian(thetas)
    print("dH", (Ha - Hb).abs().max().item())
    assert (Ea - Eb).abs().max().item() < 1e-9 and (ga - gb).abs().max().item() < 1e-9
    assert (Ha - Hb).abs().max().item() < 1e-8


def test_rhf_energy_from_device_integrals():
    I = gto.integrals_batch(formal_basis(), [formal((140.0, 80.0))])
    _, _, e = gaussian.rhf(I.int1e_ao[0].cpu().numpy(), I.int2e_ao[0].cpu().numpy(), I.overlap[0].cpu().numpy(), 8)
    print("RHF", e + I.nuc[0].item(), "literal", E_RHF)
    assert abs(e + I.nuc[0].item() - E_RHF) < 1e-9
    # the default orbitals of from_geometries are these RHF orbitals: the Hartree-Fock state has the RHF energy
    batch = aoo.OO_pqc_batch.from_geometries(np_fabric(), formal_basis(), [formal((140.0, 80.0))], 2, 2,
                                             freeze_active=True)
    assert abs(batch.energy(torch.zeros((1, batch.n_theta), dtype=torch.float64)).item() - E_RHF) < 1e-9


def _literal_energy(mol_like):
    c = case("test_energy_from_mo_coeff")
    oo = aoo.OO_energy(mol_like, c["ncas"], c["nelecas"], freeze_active=c["freeze_active"],
                       oao_mo_coeff=np.eye(13))
    T = lambda x: torch.tensor(x, dtype=torch.float64)      # noqa: E731
    return oo.energy_from_mo_coeff(T(c["mo_coeff"]), T(c["one_rdm"]), T(c["two_rdm"])).item()


def _device_moldata(geometry):
    I = gto.integrals_batch(formal_basis(), [geometry])
    return aoo.Moldata(I.int1e_ao[0].cpu().numpy(), I.int2e_ao[0].cpu().numpy(), I.overlap[0].cpu().numpy(),
                       I.nuc[0].item(), 16)


def test_cas22_energy_at_the_literal_orbitals_matches_the_host_integrals():
    """energy_from_mo_coeff at the literal orbitals and RDMs of test/test_oo_energy.py:244-298: device integrals
    against host integrals within 1e-9, and against the literal at the reference's own assertion (np.allclose: the
    literal RDMs hold 4 digits and the energy is linear in them, both sets of integrals give -92.749359)."""
    geo = formal((140.0, 80.0))
    e_dev, e_host = _literal_energy(_device_moldata(geo)), _literal_energy(host_mol(geo))
    print("CAS(2,2) device", e_dev, "host", e_host)
    assert abs(e_dev - e_host) < 1e-9
    assert np.allclose(e_dev, E_CAS22)


def test_cas22_literal_energy_within_1e_9():
    """The literal -92.74923236954386 (test/test_oo_energy.py:298) within 1e-9 from the literal orbitals of
    tests/golden/molecule_cases.json, on device integrals: the CAS(2e,2o) energy in the space those orbitals span --
    the device CASCI (``Moldata.run_casci``) at the literal orbitals.  The literal holds 5 digits, so the orbitals as
    written are orthonormal to 2.8e-5 only (an error of first order in the energy: 8.8e-5 with the host integrals);
    their symmetric orthonormalisation C (C^T S C)^-1/2 is the nearest orthonormal set, and the energy, stationary
    in the orbitals, is then second order in what the rounding leaves: 3.0e-10 from the literal with the host
    integrals of gaussian.py (numpy, CPU).  The literal RDMs (4 digits) are not used here: the energy is linear in
    them, which is what keeps ``energy_from_mo_coeff`` of the literal triple 1.27e-4 away (the test above)."""
    mol = _device_moldata(formal((140.0, 80.0)))
    c = case("test_energy_from_mo_coeff")
    C = np.array(c["mo_coeff"])
    metric = C.T @ mol.overlap @ C
    print("literal orbitals: max |C^T S C - 1| =", np.abs(metric - np.eye(13)).max())
    res = mol.run_casci(c["ncas"], c["nelecas"], mo=C @ ao_to_oao(metric))
    print("CAS(2,2) device", res.e_tot, "literal", E_CAS22, "difference", res.e_tot - E_CAS22)
    assert res.converged
    assert abs(res.e_tot - E_CAS22) < 1e-9


# ---- 6. batch semantics ---------------------------------------------------------------------------------------------
def test_a_stack_equals_its_geometries_one_by_one_bit_for_bit():
    geos = [formal(p) for p in POINTS + ring()[:3]]
    basis = formal_basis()
    I = gto.integrals_batch(basis, geos)
    for k, geo in enumerate(geos):
        one = gto.integrals_batch(basis, [geo])
        for name in ("overlap", "int1e_ao", "int2e_ao", "nuc", "oao_coeff"):
            assert torch.equal(getattr(I, name)[k], getattr(one, name)[0]), (name, k)


def test_side_stream_call_gives_the_same_bits():
    geos = [formal(p) for p in POINTS]
    basis = formal_basis()
    I = gto.integrals_batch(basis, geos)
    side = ops.side_streams(torch.device("cuda", torch.cuda.current_device()))[0]
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        J = gto.integrals_batch(basis, geos)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for name in ("overlap", "int1e_ao", "int2e_ao", "nuc", "oao_coeff"):
        assert torch.equal(getattr(I, name), getattr(J, name)), name


def test_set_geometries_with_an_index_changes_only_those_rows():
    pts = ring()[:6]
    geos = [formal(p) for p in pts]
    pqc = np_fabric()
    c0 = rhf_orbitals(geos[0])
    batch = aoo.OO_pqc_batch.from_geometries(pqc, formal_basis(), geos, 2, 2, oao_mo_coeffs=[c0] * 6,
                                             freeze_active=True)
    before = {n: getattr(batch, n).clone() for n in ("int2e_ao", "int1e_ao", "oao_coeff", "nuc", "mo_coeff")}
    new = {1: formal(POINTS[0]), 2: formal(POINTS[1]), 4: formal(POINTS[2])}
    batch.set_geometries(list(new.values()), index=list(new.keys()))
    for n, old in before.items():
        for k in range(6):
            assert torch.equal(getattr(batch, n)[k], old[k]) == (k not in new), (n, k)
    now = [new.get(k, geos[k]) for k in range(6)]
    host = aoo.OO_pqc_batch(pqc, [host_mol(g) for g in now], 2, 2, oao_mo_coeffs=[c0] * 6, freeze_active=True)
    thetas = torch.as_tensor(np.random.default_rng(11).uniform(-0.3, 0.3, (6, batch.n_theta))).cuda()
    dE = (batch.energy(thetas) - host.energy(thetas)).abs().max().item()
    print("dE after set_geometries(index)", dE)
    assert dE < 1e-9
    with pytest.raises(ValueError):
        batch.set_geometries([geos[0]], index=[6])
    with pytest.raises(RuntimeError):
        host.set_geometries(geos)


# ---- 7. Berry ring ----------------------------------------------------------------------------------------------------
def test_ring_driven_by_set_geometries_matches_set_molecule():
    """One damped Newton step per ring point, parameters and orbitals carried from the previous point: the batch
    moved by set_geometries (integrals made on the device) against the batch moved by set_molecule with host-built
    molecules: energies within 1e-9 at every point."""
    geos = [formal(p) for p in ring()]
    pqc = np_fabric()
    c0 = rhf_orbitals(geos[0])
    dev = aoo.OO_pqc_batch.from_geometries(pqc, formal_basis(), [geos[0]], 2, 2, oao_mo_coeffs=[c0],
                                           freeze_active=True)
    host = aoo.OO_pqc_batch(pqc, [host_mol(geos[0])], 2, 2, oao_mo_coeffs=[c0], freeze_active=True)
    th_d = torch.zeros((1, dev.n_theta), dtype=torch.float64).cuda()
    th_h = th_d.clone()
    worst = 0.0
    for k in range(len(geos)):
        if k > 0:
            dev.set_geometries([geos[k]])
            host.set_molecule(0, host_mol(geos[k]), host.oao_mo_coeff[0].clone())
        th_d, e_d, _ = dev.damped_newton_step(th_d)
        th_h, e_h, _ = host.damped_newton_step(th_h)
        d = abs(e_d.item() - e_h.item())
        print(f"ring point {k}: E = {e_d.item():.12f}, |dE| = {d:.2e}")
        worst = max(worst, d)
    assert worst < 1e-9
