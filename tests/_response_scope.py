"""Shared by tests/test_response_scope_cpu.py, tests/test_response_scope_gpu.py and tests/golden/make_response_scope.py:
the cases and the host references of the scope tests of the density and orbital-response kernels
(``cas_ao_densities``, ``response_d2``, ``zvector``, ``overlap_pullback``, ``connection_pullback``,
``relaxed_densities``) over all of N <= 64, ncas <= 8.

Inputs.  S, h, g of a Z-vector case are ``synthetic.synthetic_problem(n, seed)`` (``G_SCALE`` names one exception); its canonical orbitals are those of the
host ``gaussian.rhf`` at ``conv_tol = 1e-12``, made ONCE by the generator and kept in tests/golden/response_scope_z_*.npz
(host RHF takes seconds at n = 64); a test rebuilds g from the seed and checks it against the sum and four elements that
the fixture keeps.  The density and pull-back tests need orbitals and an overlap of the right shape only:
``scope_orbitals`` (an SPD overlap with the spectrum of ``synthetic_problem``, ``C = S^-1/2 U``), made in the test.

Reference of the Z-vector.  ``zvector_host(eliminate=True)`` builds A from one Fock build per unknown, too slow at 1024
unknowns.  In the MO basis

    A[ai,bj] = delta_ab delta_ij (eps_a - eps_i) + 4 (ai|bj) - (ab|ij) - (aj|ib),
    b_ai     = w_ai - 4 sum_pq zt_pq [(ai|pq) - (ap|iq) / 2],

one staged transform of g and a dense solve (``closed_form_system``); tests/test_response_scope_cpu.py holds it against
``zvector_host`` at n <= 12 before the device tests rely on it.

Bounds.  ``U53 = 2^-53`` is the unit roundoff.  A sum of m products computed in any order differs from the exact sum by
at most ``m U53`` times the same sum over absolute values (to first order), so two routes differ by at most twice that:
the ``*_abs`` functions evaluate the expressions of the twins with |C|, |gamma|, |Gamma| and every sign positive.
Nothing in a bound comes from the code under test."""
import functools
import os

import numpy as np

from auto_oo_amd import gaussian, nucgrad, synthetic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U53 = 2.0 ** -53
TOL, MAX_ITER, MIN_GAP = 1e-10, 100, 1e-6
MAX_FIXTURE_BYTES = 182 * 1024

# ---- the Z-vector cases: name -> (n, n_occ, seeds of its geometries) ---------------------------------------------------
# nvo = n_occ (n - n_occ): 1; 63 twice (one occupied, one virtual orbital); 255, 256, 272 around the 256 threads of the
# step kernel; 552 (61912 bytes of LDS), 576 (65728, the first shape above 64 KB), 1024 (the limit, 113.6 KB).  "12_5" serves the
# class edges and the closed form against zvector_host, "9_4" the latter.
Z_CASES = {
    "2_1": (2, 1, (11, 12, 13)),
    "9_4": (9, 4, (22,)),
    "12_5": (12, 5, (22, 23)),
    "64_1": (64, 1, (6,)),
    "64_63": (64, 63, (8,)),
    "32_15": (32, 15, (31, 32, 33)),
    "32_16": (32, 16, (34, 35, 36)),
    "33_16": (33, 16, (2, 37, 38)),
    "47_23": (47, 23, (9,)),
    "48_24": (48, 24, (10,)),
    "64_32": (64, 32, (4, 14)),
}
# With one doubly occupied orbital the host RHF does not converge on a synthetic problem of any seed tried (5 .. 59 at
# n = 64, 5 .. 7 at n = 8 .. 48): the exchange part of these random integrals outweighs their Coulomb part, and the aufbau
# iteration oscillates (largest off-diagonal Fock element 2 .. 7).  g times 0.03 leaves a problem that converges; every
# other case has the integrals as they are.
G_SCALE = {"64_1": 0.03}
Z_DEVICE_CASES = ("2_1", "64_1", "64_63", "32_15", "32_16", "33_16", "47_23", "48_24", "64_32")
PROBES = ((0, 0, 0, 0), (1, 0, 1, 0), (-1, 0, -1, 1), (-1, -1, -1, -1))       # the four elements of g a fixture keeps

# the class edges of response_pairs at n = 12, n_occ = 5: (n_core, ncas)
EDGES = {"n_core = 0": (0, 7), "n_core = n_occ": (5, 3), "n_core + ncas = n_occ": (2, 3), "n_core + ncas = n": (4, 8),
         "ncas = 0": (5, 0)}

# cas_ao_densities: (n, n_core, ncas, geometries)
DENSITY_CASES = [(1, 1, 0, 3), (1, 0, 1, 3), (5, 0, 5, 3), (13, 5, 8, 3), (36, 28, 8, 3), (37, 29, 8, 3), (64, 56, 8, 2),
                 (64, 32, 0, 1)]


def active_window(n, n_occ):
    """(n_core, ncas) of a Z-vector case: up to four occupied and four virtual orbitals around the Fermi level."""
    n_core = max(0, n_occ - 4)
    return n_core, min(8, n - n_core)


def step_lds_bytes(n, n_occ):
    return (3 * n * (n | 1) + 2 * n_occ * (n - n_occ) + 8) * 8


def density_lds_bytes(n, n_core, ncas):
    return (n * (n_core + ncas) + 2 * n * n + ncas ** 4) * 8


def fixture_path(name):
    return os.path.join(GOLDEN, f"response_scope_z_{name}.npz")


@functools.lru_cache(maxsize=None)
def fixture(name):
    with np.load(fixture_path(name)) as f:
        return {k: f[k] for k in f.files}


@functools.lru_cache(maxsize=2)
def problem(name, k):
    """S, h, g of geometry ``k`` of a Z-vector case: ``synthetic_problem(n, seed)``, g times the case's ``G_SCALE``."""
    n, _, seeds = Z_CASES[name]
    P = dict(synthetic.synthetic_problem(n, int(seeds[k])))
    if name in G_SCALE:
        P["int2e_ao"] = G_SCALE[name] * P["int2e_ao"]
    return P


def g_marks(g):
    """What a fixture keeps of g: its sum and the elements ``PROBES``."""
    return float(g.sum()), np.array([g[p] for p in PROBES])


def check_g(name, k, g):
    """A rebuilt g against the fixture: numpy's random stream (or the construction) has not drifted.  1e-9 of the
    scale: the products of the construction may round differently from one BLAS to the next, a different stream
    changes every figure in the first digit."""
    f = fixture(name)
    total, probes = g_marks(g)
    scale = np.abs(g).sum()
    assert abs(total - f["g_sum"][k]) <= 1e-9 * scale, (name, k, total, f["g_sum"][k])
    assert np.abs(probes - f["g_probes"][k]).max() <= 1e-9 * np.abs(g).max(), (name, k)


# ---- the closed form of the virt-occ system --------------------------------------------------------------------------
def mo_integrals(g, C):
    """(pq|rs) in the MO basis: the four indices one after the other."""
    x = np.tensordot(g, C, axes=([3], [0]))                 # pqr l
    x = np.tensordot(x, C, axes=([2], [0]))                 # pq l k
    x = np.tensordot(x, C, axes=([1], [0]))                 # p l k j
    x = np.tensordot(x, C, axes=([0], [0]))                 # l k j i
    return np.ascontiguousarray(x.transpose(3, 2, 1, 0))


def closed_form_matrix(gm, eps, n_occ):
    """A [nvo, nvo] in the order (a, i) of the device from the MO integrals ``gm``."""
    n = gm.shape[0]
    o, v = slice(0, n_occ), slice(n_occ, n)
    nvo = n_occ * (n - n_occ)
    A = 4.0 * gm[v, o, v, o] - gm[v, v, o, o].transpose(0, 2, 1, 3) - gm[v, o, o, v].transpose(0, 2, 3, 1)
    A = A.reshape(nvo, nvo).copy()
    A[np.diag_indices(nvo)] += (eps[v, None] - eps[None, o]).reshape(-1)
    return A


def closed_form_rhs(gm, eps, n_core, ncas, n_occ, w):
    """(z of the pairs inside occ-occ and virt-virt [n, n], b [n_virt, n_occ]) for one right-hand side ``w`` [n, n]."""
    n = gm.shape[0]
    _, dg = nucgrad.response_pairs(n, n_core, ncas, n_occ)
    z = np.zeros((n, n))
    delta = eps[:, None] - eps[None, :]
    z[dg] = w[dg] / delta[dg]
    zt = 0.5 * (z + z.T)
    gz = np.einsum("pqrs,rs->pq", gm, zt) - 0.5 * np.einsum("prqs,rs->pq", gm, zt)
    return z, (w - 4.0 * gz)[n_occ:, :n_occ]


def spectrum(A, eps, n_occ):
    """(lambda_min, lambda_max, condition number of the preconditioned matrix M^-1/2 A M^-1/2) of the symmetric part."""
    A = 0.5 * (A + A.T)
    lam = np.linalg.eigvalsh(A)
    d = (eps[n_occ:, None] - eps[None, :n_occ]).reshape(-1) ** -0.5
    pre = np.linalg.eigvalsh(A * d[:, None] * d[None, :])
    return float(lam[0]), float(lam[-1]), float(pre[-1] / pre[0])


def masked_rhs(n, n_core, ncas, n_occ, K, seed):
    """K seeded standard-normal right-hand sides [K, n, n], zero outside the pairs of ``response_pairs``."""
    vo, dg = nucgrad.response_pairs(n, n_core, ncas, n_occ)
    return np.random.default_rng(seed).standard_normal((K, n, n)) * (vo | dg)


def reference_z(gm, A, eps, n_core, ncas, n_occ, ws):
    """z [K, n, n] of the dense solve for the right-hand sides ``ws`` [K, n, n]."""
    n = gm.shape[0]
    out = []
    for w in ws:
        z, b = closed_form_rhs(gm, eps, n_core, ncas, n_occ, w)
        z[n_occ:, :n_occ] = np.linalg.solve(A, b.reshape(-1)).reshape(n - n_occ, n_occ)
        out.append(z)
    return np.stack(out)


def z_bound(lam_min, lam_max, z_ref):
    """max |z - z_ref| of a solve with residual 2-norm ``TOL`` (``||dz||_2 <= TOL / lambda_min``), plus the dense
    solve's own error, 100 U53 cond(A) max |z_ref|."""
    return TOL / lam_min + 100.0 * U53 * (lam_max / lam_min) * np.abs(z_ref).max()


# ---- a negative definite A ------------------------------------------------------------------------------------------------
NEGATIVE_CASE, NEGATIVE_AUX = "12_5", 64


@functools.lru_cache(maxsize=None)
def negative_definite_problem(k=0):
    """Integrals ``-c g`` that make A negative definite on the orbitals of geometry ``k`` of ``NEGATIVE_CASE`` ->
    (g_neg, A_neg).  With the g of ``synthetic_problem(n, seed)`` itself no c does: the exchange terms make the
    two-electron part of A indefinite (eigenvalues -4.2 .. 18.7 here).  With ``NEGATIVE_AUX`` n auxiliary factors the
    same construction tends to ``(pq|rs) -> (delta_pr delta_qs + delta_ps delta_qr) / 2``, whose two-electron part is
    ``1.5 x`` the unit matrix for orthonormal orbitals; here it is positive definite (asserted), and ``c = 2 max(eps_a -
    eps_i) / lambda_min`` of it gives ``lambda_max(A_neg) <= -max(eps_a - eps_i)``."""
    n, n_occ, seeds = Z_CASES[NEGATIVE_CASE]
    f = fixture(NEGATIVE_CASE)
    C, eps = f["mo_coeff"][k], f["mo_energy"][k]
    g = synthetic.synthetic_problem(n, int(seeds[k]), n_aux=NEGATIVE_AUX * n)["int2e_ao"]
    gaps = (eps[n_occ:, None] - eps[None, :n_occ]).reshape(-1)
    two = closed_form_matrix(mo_integrals(g, C), eps, n_occ) - np.diag(gaps)
    lam = np.linalg.eigvalsh(0.5 * (two + two.T))[0]
    assert lam > 0.0, lam
    g_neg = -(2.0 * gaps.max() / lam) * g
    return g_neg, closed_form_matrix(mo_integrals(g_neg, C), eps, n_occ)


# ---- the generator's side ----------------------------------------------------------------------------------------------
def make_z_case(name):
    """The fixture of a Z-vector case -> (dict of arrays, list of report lines).  Refuses (AssertionError) a geometry
    unless its RHF converged, its aufbau gap is positive and lambda_min(A) > 0 -- and unless the pairs of step one of
    its ``active_window`` are further apart than ``MIN_GAP``."""
    n, n_occ, seeds = Z_CASES[name]
    n_core, ncas = active_window(n, n_occ)
    out = {k: [] for k in ("mo_coeff", "mo_energy", "lam_min", "lam_max", "cond_pre", "off_diagonal", "aufbau_gap",
                           "class_gap", "g_sum", "g_probes")}
    lines = []
    for seed in seeds:
        P = problem(name, len(lines))
        S, h, g = P["overlap"], P["int1e_ao"], P["int2e_ao"]
        C, eps, _ = gaussian.rhf(h, g, S, n_occ, conv_tol=1e-12)
        Co = C[:, :n_occ]
        f = C.T @ (h + nucgrad._g_host(g, 2.0 * Co @ Co.T)) @ C
        off = float(np.abs(f - np.diag(np.diag(f))).max())
        ortho = float(np.abs(C.T @ S @ C - np.eye(n)).max())
        gap = float(eps[n_occ] - eps[n_occ - 1])
        assert off < 1e-8 and ortho < 1e-12 and np.abs(np.diag(f) - eps).max() < 1e-8, \
            f"{name}, seed {seed}: RHF did not converge (off-diagonal of f {off:.1e})"
        assert gap > 0.0 and (np.diff(eps) > 0.0).all(), f"{name}, seed {seed}: aufbau gap {gap:.2e}"
        _, dg = nucgrad.response_pairs(n, n_core, ncas, n_occ)
        class_gap = float(np.abs(eps[:, None] - eps[None, :])[dg].min()) if dg.any() else np.inf
        assert class_gap > 1e3 * MIN_GAP, f"{name}, seed {seed}: class gap {class_gap:.2e}"
        A = closed_form_matrix(mo_integrals(g, C), eps, n_occ)
        assert np.abs(A - A.T).max() < 1e-12
        lam_min, lam_max, cond_pre = spectrum(A, eps, n_occ)
        assert lam_min > 0.0, f"{name}, seed {seed}: lambda_min(A) = {lam_min:.3e}"
        total, probes = g_marks(g)
        for k, v in zip(out, (C, eps, lam_min, lam_max, cond_pre, off, gap, class_gap, total, probes)):
            out[k].append(v)
        lines.append(f"{name} seed {seed}: nvo {n_occ * (n - n_occ)}, lambda_min(A) {lam_min:.3f}, lambda_max "
                     f"{lam_max:.2f}, cond of the preconditioned matrix {cond_pre:.1f}, off-diagonal of f {off:.1e}, "
                     f"aufbau gap {gap:.3f}, class gap {class_gap:.2e}")
    out = {k: np.array(v) for k, v in out.items()}
    out["seeds"] = np.array(seeds)
    return out, lines


# ---- orbitals and overlaps of the density and pull-back tests ---------------------------------------------------------------
def scope_orbitals(n, seed, spectrum_="synthetic"):
    """(S, U, C): an SPD overlap with the spectrum of ``synthetic_problem`` (uniform in 0.3 .. 1.7), or the unit matrix
    (``"unit"``: every eigenvalue degenerate), or with its smallest eigenvalue 1e-4 (``"small"``); an orthogonal ``U``
    and ``C = S^-1/2 U``."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = rng.uniform(0.3, 1.7, size=n)
    if spectrum_ == "unit":
        lam[:] = 1.0
    elif spectrum_ == "small":
        lam[0] = 1e-4
    S = (Q * lam) @ Q.T
    S = 0.5 * (S + S.T)
    if spectrum_ == "unit":
        S = np.eye(n)
    U, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return S, U, (Q * lam ** -0.5) @ Q.T @ U


def cas_ao_densities_abs(C, n_core, ncas, one_rdm=None, two_rdm=None):
    """The expressions of ``cas_ao_densities_host`` over absolute values with every sign positive -> (D1_abs, D2_abs)."""
    C = np.abs(np.asarray(C))
    Cc, Ca = C[:, :n_core], C[:, n_core:n_core + ncas]
    Dc = 2.0 * Cc @ Cc.T
    e = np.einsum
    d2 = e("pq,rs->pqrs", Dc, Dc) + 0.5 * e("pr,qs->pqrs", Dc, Dc)
    Da = np.zeros_like(Dc)
    if ncas > 0:
        Da = Ca @ np.abs(one_rdm) @ Ca.T
        d2 = d2 + 2.0 * (e("pq,rs->pqrs", Dc, Da) + 0.5 * e("pr,qs->pqrs", Dc, Da))
        d2 = d2 + e("tuvw,pt,qu,rv,sw->pqrs", np.abs(two_rdm), Ca, Ca, Ca, Ca, optimize=True)
    d1 = Dc + Da
    return 0.5 * (d1 + d1.T), nucgrad.sym8_host(d2)


def density_bounds(C, n_core, ncas, one_rdm=None, two_rdm=None):
    """Per element: 2 (ncas^4 + 16) U53 (the expression over absolute values), device and twin each once."""
    a1, a2 = cas_ao_densities_abs(C, n_core, ncas, one_rdm, two_rdm)
    m = 2.0 * (ncas ** 4 + 16) * U53
    return m * a1, m * a2


def response_d2_abs(Z, D0):
    return nucgrad.sym8_host(2.0 * np.einsum("pq,rs->pqrs", np.abs(Z), np.abs(D0))
                             + np.einsum("pr,qs->pqrs", np.abs(Z), np.abs(D0)))


def share(err, bound):
    """The largest share of its bound that an element's error takes (0 / 0 = 0)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0.0, 0.0, np.asarray(err) / np.asarray(bound))
    return float(np.max(r))


def pullback_bound(S, g_x):
    """10 . 8 n U53 max |K_ij| ||G_X||_F: the forward error of the eight n-term products of the route, a factor ten
    for the eigenvectors.  ``G_X`` as the products deliver it, before it is symmetrised: that is what their rounding
    errors are proportional to (for S = 1 and an antisymmetric ``a`` the symmetric part of ``X^-1 U a U^T`` vanishes,
    the errors of the products do not)."""
    s = np.linalg.eigvalsh(S)
    n = S.shape[0]
    return 10.0 * 8 * n * U53 * (0.5 * s.min() ** -1.5) * np.linalg.norm(g_x)


def overlap_pullback_gx(S, U, F):
    """``G_X`` of ``overlap_pullback`` on the host: ``(dE/dC) U^T`` with ``dE/dC = 2 X^-1 U F^T``."""
    s, V = np.linalg.eigh(S)
    return 2.0 * (V * np.sqrt(s)) @ V.T @ U @ F.T @ U.T


def connection_gx(S, U, a):
    s, V = np.linalg.eigh(S)
    return (V * np.sqrt(s)) @ V.T @ U @ a @ U.T
