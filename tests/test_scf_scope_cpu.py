"""The references and the problem family of the scope tests of the iterative solvers (tests/_scf_scope.py), without a
device: the family has the symmetries it claims, every problem a device test runs satisfies ``CONDITIONS`` on the host
solution alone, ``host_rhf_counted`` is ``gaussian.rhf``, the dense Hessian is the matrix of ``nucgrad.zvector_host``,
``host_pcg`` solves it, and the closed forms the DIIS tests of the device rely on hold for the host twin."""
import numpy as np
import pytest
import scipy.linalg

from auto_oo_amd import gaussian, nucgrad
from tests import _scf_scope as V


def test_the_family_has_its_symmetries_and_its_levels():
    n, n_occ = 9, 4
    P = V.gapped_problem(n, n_occ, 5, 0.6, 1.0)
    h, g, S = P["int1e_ao"], P["int2e_ao"], P["overlap"]
    assert np.array_equal(S, S.T) and np.array_equal(h, h.T)
    for perm in ((1, 0, 2, 3), (0, 1, 3, 2), (2, 3, 0, 1)):
        assert np.array_equal(g, g.transpose(perm))
    lam = np.linalg.eigvalsh(S)
    assert 0.5 <= lam[0] and lam[-1] <= 1.5
    # without the noise and without g the generalised eigenvalues of (h, S) are the levels: the noise moves them by at
    # most its 2-norm, below 2 x 0.05 (a symmetric Gaussian matrix of element size s / sqrt(n) has norm about 2 s)
    e = scipy.linalg.eigh(h, S, eigvals_only=True)
    levels = np.concatenate([np.linspace(-3.0, -1.0, n_occ), np.linspace(-0.4, 2.6, n - n_occ)])
    print("levels moved by", np.abs(e - levels).max())
    assert np.abs(e - levels).max() <= 0.1
    Q = V.gapped_problem(n, n_occ, 6, 0.6, 1.0)
    assert not np.array_equal(Q["overlap"], S)
    R = V.gapped_problem(n, n_occ, 5, 0.6, 2.0)
    assert np.array_equal(R["overlap"], S) and np.array_equal(R["int1e_ao"], h)
    assert np.abs(R["int2e_ao"] - 2.0 * g).max() <= 4 * V.EPS * np.abs(g).max()


@pytest.mark.parametrize("key", V.all_problems(), ids=lambda k: "{}-{}-seed{}-{}".format(*k))
def test_conditions_of_every_problem_the_device_tests_use(key):
    sol = V.host_solution(*key)
    n, n_occ = key[0], key[1]
    A = sol["A"]
    d = (sol["e"][n_occ:, None] - sol["e"][None, :n_occ]).reshape(-1)
    its = []
    for w in V.z_rhs(n, n_occ, 10, key[2]):
        b = w[n_occ:, :n_occ].reshape(-1)
        x, it = V.host_pcg(A, b, d)
        assert np.linalg.norm(A @ x - b) <= 10 * V.Z_TOL
        its.append(it)
    print(f"{key}: host iterations {sol['iterations']}, gap {sol['gap']:.3f}, lambda_min(A) {sol['lam_min']:.3f}, "
          f"cond(A) {sol['cond']:.1f}, lambda_min(S) {sol['lam_s']:.3f}, asymmetry {sol['asym']:.1e}, "
          f"pcg {min(its)}-{max(its)}")
    c = V.CONDITIONS
    assert sol["converged"] and sol["iterations"] <= c["max_iterations"]
    assert sol["gap"] >= c["min_gap"]
    assert sol["lam_min"] >= c["min_lambda"]
    assert sol["asym"] <= c["asymmetry"]


@pytest.mark.parametrize("key", [(13, 6, 1, "firm"), (17, 6, 1, "firm")], ids=["n13", "n17"])
def test_host_rhf_counted_is_gaussian_rhf_and_the_dense_hessian_is_that_of_zvector_host(key):
    n, n_occ = key[0], key[1]
    P = V.problem(*key)
    sol = V.host_solution(*key)
    C, e, e_elec = gaussian.rhf(P["int1e_ao"], P["int2e_ao"], P["overlap"], n_occ)
    assert np.array_equal(C, sol["C"]) and np.array_equal(e, sol["e"]) and e_elec == sol["e_elec"]
    w = V.z_rhs(n, n_occ, 1, key[2])[0]
    z, A, b = nucgrad.zvector_host(P["int2e_ao"], C, e, 0, n, n_occ, w, eliminate=True)
    d_a = np.abs(A - sol["A"]).max() / np.abs(A).max()
    z_dense = np.linalg.solve(sol["A"], w[n_occ:, :n_occ].reshape(-1)).reshape(n - n_occ, n_occ)
    d_z = np.abs(z[n_occ:, :n_occ] - z_dense).max() / np.abs(z_dense).max()
    print(f"n = {n}: dense A against zvector_host {d_a:.1e} of max |A|, z {d_z:.1e} of max |z|")
    assert np.array_equal(b, w[n_occ:, :n_occ])              # (n_core = 0, ncas = n: nothing is eliminated)
    assert d_a <= 1e-14
    assert d_z <= 10 * sol["cond"] * V.EPS


@pytest.mark.parametrize("n,n_occ", V.NEARLY_SINGULAR_PAIRS)
def test_without_g_the_host_twin_stops_after_two_iterations_at_the_generalised_eigenvalues(n, n_occ):
    """What the nearly singular DIIS test of the device relies on: with g = 0 the second commutator is rounding noise,
    the bordered system has a B of size 1e-32, and the twin still returns the generalised eigenvalues of (h, S)."""
    P = V.problem(n, n_occ, 1, "firm")
    h, S = P["int1e_ao"], P["overlap"]
    C, e, E, count, last, converged = V.host_rhf_counted(h, np.zeros((n, n, n, n)), S, n_occ)
    ref = scipy.linalg.eigh(h, S, eigvals_only=True)
    d_e = abs(E - 2.0 * ref[:n_occ].sum()) / abs(E)
    d_eps = np.abs(e - ref).max()
    print(f"n = {n}: {count} iterations, commutator {last:.1e}, E {d_e:.1e} relative, mo_energy {d_eps:.1e}")
    assert converged and count == 2
    assert d_e <= 1e-12 and d_eps <= 1e-10
