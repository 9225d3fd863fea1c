"""Host checks of the scope tests of the density and orbital-response kernels (tests/_response_scope.py): the closed
form of the virt-occ system against ``nucgrad.zvector_host``, the fixtures, the generator's conditions, and the negative
definite case.  No device is needed."""
import os

import numpy as np
import pytest

from auto_oo_amd import nucgrad
from tests import _response_scope as V


def _geometry(name, k):
    n, n_occ, seeds = V.Z_CASES[name]
    f = V.fixture(name)
    P = V.problem(name, k)
    V.check_g(name, k, P["int2e_ao"])
    return n, n_occ, P, f["mo_coeff"][k], f["mo_energy"][k]


@pytest.mark.parametrize("name,window", [("2_1", (0, 2)), ("9_4", (2, 5)), ("12_5", (1, 8)), ("12_5", (4, 8)),
                                         ("12_5", (5, 0))])
def test_closed_form_system_is_that_of_zvector_host(name, window):
    """A, b and z of the closed form against ``zvector_host(eliminate=True)``, and z against the full linear system
    (``eliminate=False``).  Both routes build an element of A or b from four n-term contractions and at most n^2
    further terms, so they differ by at most 2 (4 n + n^2 + 2) U53 times the same sums over absolute values.
    Measured: A 4.4e-16 (n = 2, bound 2.5e-14), 1.8e-15 (n = 9, 3.8e-12), 3.6e-15 (n = 12, 1.1e-11); b at most 1.3e-15
    (bounds 8.5e-16 for b = w exactly at n = 2, up to 3.0e-11); z of the closed form against the full system at most
    7.8e-16 for bounds of 5.4e-11 .. 1.2e-10."""
    n_core, ncas = window
    n, n_occ, P, C, eps = _geometry(name, 0)
    g = P["int2e_ao"]
    w = V.masked_rhs(n, n_core, ncas, n_occ, 1, 7)[0]
    z_host, A_host, b_host = nucgrad.zvector_host(g, C, eps, n_core, ncas, n_occ, w, eliminate=True)
    gm = V.mo_integrals(g, C)
    A = V.closed_form_matrix(gm, eps, n_occ)
    zd, b = V.closed_form_rhs(gm, eps, n_core, ncas, n_occ, w)
    g_abs = V.mo_integrals(np.abs(g), np.abs(C)).max()
    m = 2.0 * (4 * n + n * n + 2) * V.U53
    bound_A = m * (np.abs(eps).max() * 2 + 6.0 * g_abs)
    bound_b = m * (np.abs(w).max() + 6.0 * g_abs * np.abs(zd).sum())
    err_A, err_b = np.abs(A - A_host).max(), np.abs(b - b_host).max()
    print(f"{name} window {window}: A {err_A:.2e} / {bound_A:.2e}, b {err_b:.2e} / {bound_b:.2e}")
    assert err_A <= bound_A and err_b <= bound_b
    assert np.abs(A - A.T).max() <= bound_A
    lam_min, lam_max, _ = V.spectrum(A, eps, n_occ)
    z = V.reference_z(gm, A, eps, n_core, ncas, n_occ, w[None])[0]
    full = nucgrad.zvector_host(g, C, eps, n_core, ncas, n_occ, w)
    # the bound of the device tests, with room to spare for two dense solves
    bound_z = V.z_bound(lam_min, lam_max, full)
    print(f"    z: eliminated {np.abs(z - z_host).max():.2e}, full system {np.abs(z - full).max():.2e} / {bound_z:.2e}")
    assert np.abs(z - z_host).max() <= bound_z and np.abs(z - full).max() <= bound_z


@pytest.mark.parametrize("name", list(V.Z_CASES))
def test_fixture_is_complete_and_meets_the_generators_conditions(name):
    """From the fixture's orbitals and the g rebuilt from the seed: the Fock matrix is diagonal (RHF converged), the
    aufbau gap is positive, lambda_min(A) > 0 -- recomputed here, and equal to the recorded figures."""
    n, n_occ, seeds = V.Z_CASES[name]
    f = V.fixture(name)
    G = len(seeds)
    assert os.path.getsize(V.fixture_path(name)) <= V.MAX_FIXTURE_BYTES
    assert f["mo_coeff"].shape == (G, n, n) and f["mo_energy"].shape == (G, n) and list(f["seeds"]) == list(seeds)
    for key in ("lam_min", "lam_max", "cond_pre", "off_diagonal", "aufbau_gap", "class_gap", "g_sum"):
        assert f[key].shape == (G,), key
    assert f["g_probes"].shape == (G, 4)
    n_core, ncas = V.active_window(n, n_occ)
    for k in range(G):
        _, _, P, C, eps = _geometry(name, k)
        S, h, g = P["overlap"], P["int1e_ao"], P["int2e_ao"]
        Co = C[:, :n_occ]
        fock = C.T @ (h + nucgrad._g_host(g, 2.0 * Co @ Co.T)) @ C
        off = np.abs(fock - np.diag(np.diag(fock))).max()
        assert off < 1e-8 and np.abs(np.diag(fock) - eps).max() < 1e-8
        assert np.abs(C.T @ S @ C - np.eye(n)).max() < 1e-12
        assert eps[n_occ] - eps[n_occ - 1] > 0.0 and (np.diff(eps) > 0.0).all()
        assert abs((eps[n_occ] - eps[n_occ - 1]) - f["aufbau_gap"][k]) == 0.0
        _, dg = nucgrad.response_pairs(n, n_core, ncas, n_occ)
        if dg.any():
            assert np.abs(eps[:, None] - eps[None, :])[dg].min() > 1e3 * V.MIN_GAP
        lam_min, lam_max, cond_pre = V.spectrum(V.closed_form_matrix(V.mo_integrals(g, C), eps, n_occ), eps, n_occ)
        assert lam_min > 0.0
        assert abs(lam_min - f["lam_min"][k]) < 1e-9 * lam_max and abs(lam_max - f["lam_max"][k]) < 1e-9 * lam_max
        assert abs(cond_pre - f["cond_pre"][k]) < 1e-6 * cond_pre
        # conjugate gradients lose at least the factor (sqrt c - 1) / (sqrt c + 1) per iteration, c the condition number
        # of the preconditioned matrix: 0.77 at c = 60, eleven digits in max_iter = 100 iterations in the worst case
        assert cond_pre < 60.0


@pytest.mark.parametrize("name", ["2_1", "9_4", "12_5"])
def test_small_fixtures_regenerate_bit_for_bit(name):
    new, _ = V.make_z_case(name)
    old = V.fixture(name)
    assert set(new) == set(old)
    for key in new:
        assert np.array_equal(np.asarray(new[key]), old[key]), key


def test_the_shapes_reach_the_edges_they_are_named_for():
    lds = {name: V.step_lds_bytes(*V.Z_CASES[name][:2]) for name in V.Z_DEVICE_CASES}
    assert lds["47_23"] <= 65536 < lds["48_24"] and lds["64_32"] == 116288 <= 160 * 1024
    nvo = [V.Z_CASES[name][1] * (V.Z_CASES[name][0] - V.Z_CASES[name][1]) for name in V.Z_DEVICE_CASES]
    assert nvo == [1, 63, 63, 255, 256, 272, 552, 576, 1024]
    assert V.density_lds_bytes(36, 28, 8) <= 65536 < V.density_lds_bytes(37, 29, 8)
    assert V.density_lds_bytes(64, 56, 8) == 128 * 1024
    for name in V.Z_DEVICE_CASES:
        n, n_occ, _ = V.Z_CASES[name]
        nucgrad.response_pairs(n, *V.active_window(n, n_occ), n_occ)
    for n_core, ncas in V.EDGES.values():
        nucgrad.response_pairs(12, n_core, ncas, 5)


def test_negative_definite_case():
    """lambda_max(A) < 0 for the integrals ``-c g`` of ``negative_definite_problem``, so that ``p^T A p < 0`` for every
    direction, the first one included; the same construction with the plain g has an indefinite two-electron part."""
    n, n_occ, _ = V.Z_CASES[V.NEGATIVE_CASE]
    f = V.fixture(V.NEGATIVE_CASE)
    eps = f["mo_energy"][0]
    g_neg, A = V.negative_definite_problem()
    lam = np.linalg.eigvalsh(0.5 * (A + A.T))
    gaps = eps[n_occ:, None] - eps[None, :n_occ]
    print(f"lambda(A_neg) = {lam[0]:.2f} .. {lam[-1]:.2f}, gaps up to {gaps.max():.2f}")
    assert lam[-1] <= -gaps.max() * (1.0 - 1e-12) < 0.0
    _, _, P, C, _ = _geometry(V.NEGATIVE_CASE, 0)
    two = V.closed_form_matrix(V.mo_integrals(P["int2e_ao"], C), eps, n_occ) - np.diag(gaps.reshape(-1))
    lam = np.linalg.eigvalsh(0.5 * (two + two.T))
    assert lam[0] < 0.0 < lam[-1]
    # the first direction of the solve for a masked right-hand side
    n_core, ncas = V.active_window(n, n_occ)
    w = V.masked_rhs(n, n_core, ncas, n_occ, 1, 5)[0]
    _, b = V.closed_form_rhs(V.mo_integrals(g_neg, C), eps, n_core, ncas, n_occ, w)
    p = (b / gaps).reshape(-1)
    assert p @ A @ p < 0.0


def test_references_of_the_density_tests_agree_with_extended_precision():
    """The twin of ``cas_ao_densities`` against the same contractions in extended precision at (13, 5, 8), random RDMs
    without symmetry: inside its half of the bound of the device test."""
    n, n_core, ncas = 13, 5, 8
    _, _, C = V.scope_orbitals(n, 1305)
    rng = np.random.default_rng(8)
    gam, Gam = rng.standard_normal((ncas,) * 2), rng.standard_normal((ncas,) * 4)
    d1, d2 = nucgrad.cas_ao_densities_host(C, n_core, ncas, gam, Gam)
    L = np.longdouble
    x1, x2 = nucgrad.cas_ao_densities_host(C.astype(L), n_core, ncas, gam.astype(L), Gam.astype(L))
    b1, b2 = V.density_bounds(C, n_core, ncas, gam, Gam)
    s1, s2 = V.share(np.abs(d1 - x1), 0.5 * b1), V.share(np.abs(d2 - x2), 0.5 * b2)
    print(f"twin against extended precision: D1 {s1:.4f}, D2 {s2:.4f} of its half of the bound")
    assert s1 <= 1.0 and s2 <= 1.0
