"""The references, twins and bounds of the rotation scope tests (tests/_rotation_scope.py) without a device:
``expm_ref`` against 50-digit mpmath and against scipy, the closed form against ``expm_ref``, the bound of every case a
device test runs printed and held under ``_rotation_scope.cap``, the line-search twin on cases worked out by hand, and
the condition of the Frechet helpers of ``oo_energy._OrbitalRotationRule``.

The condition (``test_frechet_helpers_hand_expm_a_balanced_matrix``): the helpers run here on host tensors with
``ops.expm`` replaced by the float64 twin of the kernel, so the matrix they hand over is the one the device would get,
and their result is compared with the block of ``expm_ref`` of the plain block matrix.  Error / largest element of the
wanted block, over ``_rotation_scope.block_cases()`` (measured on the CPU):
  * balanced (the helpers as they are): 1.3e-16 .. 3.5e-15, the largest at 2N, N = 24, K 1e-4, blocks 100;
  * unbalanced (the plain block matrix through the same twin) over the cases with blocks of magnitude 30 and 100:
    4.9e-14 (3N, N = 16, K 0.05, blocks 30) .. 5.5e-13 (2N, N = 24, K 0.05, blocks 100); with blocks of magnitude 1 the
    plain matrix gives 1.4e-15 .. 8.8e-15.
``FRECHET_THRESHOLD`` = 1.5e-14 is 4.3 x the largest balanced figure and 3.3 x below the smallest unbalanced one.
With the helpers of the parent commit (no balancing) the test is red in those cases.
"""
import types

import numpy as np
import pytest
import scipy.linalg
import torch

from auto_oo_amd import oo_energy
from tests import _rotation_scope as V

LD = V.LD


# ---- the references against each other ----------------------------------------------------------------------------------
def _mp_expm(X):
    import mpmath
    with mpmath.workdps(50):
        E = mpmath.expm(mpmath.matrix(X.tolist()), method="taylor")
        return np.array([[LD(mpmath.nstr(E[i, j], 25)) for j in range(X.shape[1])] for i in range(X.shape[0])])


MP_CASES = [("skew", n, x) for n, x in ((2, 0.01), (3, 1.0), (5, 40.0), (8, 1e3))] + \
           [("block", n, x) for n, x in ((2, 0.01), (4, 3.0), (4, 100.0))]


@pytest.mark.parametrize("kind,n,x", MP_CASES, ids=lambda v: str(v))
def test_expm_ref_against_mpmath_at_50_digits(kind, n, x):
    if kind == "skew":
        X = V.skew(n, x, 40 + n)
    else:                                          # [[K, A], [0, K]], K of norm 0.5, A of magnitude x
        K, offs = V.block_parts(2, n, 0.5, x)
        X = V.block_matrix(K, offs)
    ref, exact = V.expm_ref(X), _mp_expm(X)
    scale = max(1.0, float(np.abs(exact).max()))
    d = float(np.abs(ref - exact).max())
    # longdouble: 2^-64 per operation; the squarings of norm x lose x 2^-64, a few products more: 100 x 2^-64 max(1, x)
    limit = 100 * 2.0 ** -64 * max(1.0, V.norm1(X)) * scale
    print(f"{kind} n = {n} norm {V.norm1(X):.3g}: expm_ref - mpmath {d:.2e} (limit {limit:.2e})")
    assert d <= limit


@pytest.mark.parametrize("n", [4, 13, 48, 50])
def test_expm_ref_against_scipy(n):
    for x in (0.01, 0.45, 3.0, 40.0):
        X = V.skew(n, x, n)
        d = float(np.abs(V.expm_ref(X) - scipy.linalg.expm(X)).max())
        print(f"n = {n} norm {x}: expm_ref - scipy {d:.2e}")
        assert d <= 2e-13 * max(1.0, x)                     # (scipy's own float64 Pade: the figure of test_expm)


def test_closed_form_against_expm_ref():
    K, U = V.planar(9, [0.3, -2.0, 40.0, 1e-8], seed=3)
    assert float(np.abs(V.expm_ref(K) - U).max()) <= 100 * 2.0 ** -64 * 40
    for _, K, U in V.one_column_cases(65):
        assert float(np.abs(V.expm_ref(K) - U).max()) <= 100 * 2.0 ** -64 * V.norm1(K) * float(np.abs(U).max())
        cols = np.abs(K).sum(axis=0)
        assert np.sort(cols)[-3] < 0.4 and cols.max() >= 40.0


def test_twin_in_longdouble_is_the_reference_and_reports_s_and_degree():
    for x, s, deg in ((0.0, 0, 8), (0.05, 0, 8), (0.2, 0, 12), (0.45, 0, 16), (3.0, 3, 16), (1e3, 11, 16)):
        X = V.skew(7, x, 5)
        tw, s_t, d_t = V.expm_twin(X, LD)
        assert (s_t, d_t) == (s, deg)
        # truncation of the kernel's polynomial: 3e-17 relative, times the 2^s of the squarings
        assert float(np.abs(tw - V.expm_ref(X)).max()) <= 4e-17 * 2 ** s
    for i, x in enumerate(V.EDGE_NORMS):
        _, s_t, d_t = V.expm_twin(V.skew_with_exact_norm(17, x, 1))
        assert (s_t, d_t) == ((0, 8), (0, 12), (0, 12), (0, 16), (0, 16), (1, 12))[i]


# ---- the bound of every case of the device tests --------------------------------------------------------------------------
def _hold(label, X, ref=None):
    b, s, deg, mx, _ = V.expm_bound(X, ref)
    c = V.cap(X, mx)
    print(f"{label}: bound {b:.2e} (s = {s}, degree {deg}, max |exp| {mx:.3g}, cap {c:.2e})")
    assert b <= c
    return b


@pytest.mark.parametrize("n", V.SMALL_SIZES + V.LARGE_SIZES)
def test_bounds_of_the_expm_cases(n):
    for label, X in V.expm_cases(n):
        _hold(f"N = {n} {label}", X)


@pytest.mark.parametrize("n", [65, 129, 257])
def test_bounds_of_the_one_column_cases(n):
    for label, K, U in V.one_column_cases(n):
        _hold(f"N = {n} {label}", K, U)


@pytest.mark.parametrize("nb,n", V.BLOCK_SHAPES)
def test_bounds_of_the_block_matrices(nb, n):
    for ks in V.K_SCALES:
        for mag in V.OFF_MAGNITUDES:
            K, offs = V.block_parts(nb, n, ks, mag)
            _hold(f"{nb}N, N = {n}, K {ks:g}, blocks {mag:g}", V.block_matrix(K, offs))


@pytest.mark.parametrize("n", [5, 16, 33, 48, 49, 64])
def test_bounds_of_the_rotation_cases(n):
    rows, cols = V.pair_tables(n, "nonredundant")
    C = V.orbitals(n, n)
    for i, x in enumerate(V.MIXED_NORMS):
        kappa = V.kappa_of_norm(n, rows, cols, x, 60 * n + i)
        _, _, b_c, b_u, s, deg = V.rotation_reference(n, rows, cols, kappa, C)
        print(f"N = {n} kappa norm {x:g}: bound of U {b_u:.2e}, of C U {b_c:.2e} (s = {s}, degree {deg})")
        assert b_u <= V.cap(V.scatter(n, rows, cols, kappa), 1.0)


# ---- the Frechet helpers ------------------------------------------------------------------------------------------------------
def host_rule(n, monkeypatch, record=None):
    """``_OrbitalRotationRule`` on host tensors: ``ops.expm`` is the float64 twin (and records what it was handed), the two
    products are torch's."""
    def expm(X, sign=1.0):
        M = sign * X.numpy()
        if record is not None:
            record.append(M.copy())
        return torch.from_numpy(V.expm_twin(M)[0])

    monkeypatch.setattr(oo_energy, "ops", types.SimpleNamespace(expm=expm, matmul_nn=lambda a, b: a @ b,
                                                                matmul_tn=lambda a, b: a.T @ b))
    rows, cols = V.pair_tables(n, "nonredundant")
    oo = types.SimpleNamespace(nao=n, device=torch.device("cpu"), _kap_row=torch.from_numpy(rows),
                               _kap_col=torch.from_numpy(cols))
    return oo_energy._OrbitalRotationRule(oo)


def frechet_figures(nb, n, ks, mag, rule):
    """(error of the helper / max of the wanted block, the same for the plain block matrices through the twin).
    ``_frechet2`` returns the sum of the (1,3) blocks of both orders of its two blocks, so that sum is what is wanted."""
    K, offs = V.block_parts(nb, n, ks, mag)
    orders = [offs] if nb == 2 else [offs, offs[::-1]]
    want = sum(V.expm_ref(V.block_matrix(K, o))[:n, (nb - 1) * n:] for o in orders)
    plain = sum(V.expm_twin(V.block_matrix(K, o))[0][:n, (nb - 1) * n:] for o in orders)
    top = float(np.abs(want).max())
    Kt, ot = torch.from_numpy(K), [torch.from_numpy(a) for a in offs]
    got = (rule._frechet(Kt, ot[0]) if nb == 2 else rule._frechet2(Kt, ot[0], ot[1])).numpy()
    return float(np.abs(got - want).max()) / top, float(np.abs(plain - want).max()) / top


@pytest.mark.parametrize("nb,n", V.BLOCK_SHAPES)
def test_frechet_helpers_hand_expm_a_balanced_matrix(nb, n, monkeypatch):
    record = []
    rule = host_rule(n, monkeypatch, record)
    for ks in V.K_SCALES:
        for mag in V.OFF_MAGNITUDES:
            bal, plain = frechet_figures(nb, n, ks, mag, rule)
            handed = record[-1]
            print(f"{nb}N, N = {n}, K {ks:g}, blocks {mag:g}: helper {bal:.2e}, plain matrix {plain:.2e} of the block; "
                  f"handed norm {V.norm1(handed):.3g}, s = {V.expm_twin(handed)[1]}")
            assert bal <= V.FRECHET_THRESHOLD
            if mag >= 30.0:
                assert plain > V.FRECHET_THRESHOLD          # (what balancing is for; nothing of the product depends on it)


def test_kappa_gradient_goes_through_the_balanced_helper(monkeypatch):
    n = 24
    record = []
    rule = host_rule(n, monkeypatch, record)
    rng = np.random.default_rng(77)
    K = V.skew(n, 0.5, 3)
    U = np.asarray(V.expm_ref(-K), dtype=np.float64)
    fock = rng.uniform(-50.0, 50.0, (n, n))
    g = rule.kappa_gradient(torch.from_numpy(fock), None, torch.from_numpy(U), torch.from_numpy(K)).numpy()
    Xm = U @ (2.0 * fock.T)
    want = -V.expm_ref(V.block_matrix(K, [Xm]))[:n, n:]
    r, c = rule.oo._kap_row.numpy(), rule.oo._kap_col.numpy()
    want = np.asarray(want[r, c] - want[c, r], dtype=np.float64)
    d = float(np.abs(g - want).max() / np.abs(want).max())
    print(f"kappa_gradient: {d:.2e} of the largest element; handed norm {V.norm1(record[-1]):.3g} (plain "
          f"{V.norm1(V.block_matrix(K, [Xm])):.3g})")
    assert d <= 2 * V.FRECHET_THRESHOLD                     # (a difference of two elements of the block)
    assert V.norm1(record[-1]) <= 2 * 0.5 * (1 + 1e-12)


def test_balance_exponent():
    f = oo_energy._balance_exponent
    floor = oo_energy._BALANCE_FLOOR
    assert f(1.0, 1.0) == 0 and f(1.0, 0.5) == 0 and f(1.0, np.nextafter(1.0, 2.0)) == 1
    assert f(1.0, 2.0) == 1 and f(1.0, 2.5) == 2 and f(0.75, 96.0) == 7 and f(0.75, 96.1) == 8
    assert f(0.0, 0.0) == 0 and f(0.0, floor) == 0 and f(0.0, 1.0) == 6 and f(1e-300, 100.0) == 13
    assert f(float("nan"), 5.0) == 0 and f(1.0, float("inf")) == 0 and f(float("inf"), 1.0) == 0
    rng = np.random.default_rng(1)
    for nd, no in zip(10.0 ** rng.uniform(-6, 3, 200), 10.0 ** rng.uniform(-6, 4, 200)):
        e = f(nd, no)
        ref = max(nd, floor)
        assert np.ldexp(no, -e) <= ref and (e == 0 or np.ldexp(no, -(e - 1)) > ref)


# ---- the line-search twin ------------------------------------------------------------------------------------------------------
def test_update_twin_on_a_search_worked_out_by_hand():
    energy, slope = [1.0, 2.0, 3.0, 4.0], [-0.5, -0.25, float("nan"), 0.0]
    t, active, best = [1.0] * 4, [0.0] * 4, [9.0] * 4
    fl = V.ls_update_twin([0.5, 1.76, 0.0, 4.5], energy, slope, [1.0, 0.0, -2.0, 1.0], 0.5, 1, 0, t, active, best)
    # 0: 0.5 <= 1 - 0.5 passes on the threshold; 1: 1.76 > 1.75; 2: NaN threshold never passes; 3: 4.5 > 4
    assert (t, active, best) == ([1.0, 0.5, 0.5, 0.5], [0.0, 1.0, 1.0, 1.0], [0.5, 9.0, 9.0, 9.0])
    assert fl == [1.0, -2.0, 1.0, 1.0]
    fl = V.ls_update_twin([-9.0, float("nan"), 0.0, 4.0], energy, slope, None, 0.5, 0, 0, t, active, best)
    # 0 has accepted: keeps t and best; 1: a NaN trial never passes; 3: 4 <= 4 + 0.5 * 0 passes
    assert (t, active, best) == ([1.0, 0.25, 0.25, 0.5], [0.0, 1.0, 1.0, 0.0], [0.5, 9.0, 9.0, 4.0])
    assert fl == [1.0, 0.0, 1.0, 1.0]                        # flags[3]: problem 2 is searching with a NaN slope
    fl = V.ls_update_twin(None, energy, slope, None, 0.5, 0, 1, t, active, best)
    assert (t, active, best) == ([1.0, 0.0, 0.0, 0.5], [0.0] * 4, [0.5, 2.0, 3.0, 4.0])
    assert fl == [0.0, 0.0, 1.0, 0.0]


@pytest.mark.parametrize("batch", V.UPDATE_BATCHES)
def test_scripted_search_accepts_in_round_b_mod_7(batch):
    S = V.scripted_search(batch)
    for b in range(batch):
        k = b % 7
        t, active, best, _ = S["states"][V.ROUNDS - 1]
        if k < V.ROUNDS:
            t_k = 1.0
            for _ in range(k):
                t_k *= 0.3
            assert active[b] == 0.0 and t[b] == t_k and best[b] == S["trials"][k][b]
            assert all(S["states"][r][0][b] == t_k and S["states"][r][2][b] == best[b] for r in range(k, V.ROUNDS + 1))
        else:
            assert active[b] == 1.0
            assert S["states"][V.ROUNDS][0][b] == 0.0 and S["states"][V.ROUNDS][2][b] == S["energy"][b]
    assert S["states"][V.ROUNDS][3][0] == 0.0
    assert [st[3][0] for st in S["states"][:V.ROUNDS]] == [1.0 if batch > min(r + 1, 6) else 0.0 for r in range(V.ROUNDS)]


def test_points_twin_is_exact_on_the_dyadic_data():
    """t a multiple of 2^-10 below 2, dp and flat multiples of 2^-20 below 2^10: t dp is a multiple of 2^-30 below 2^11
    (41 bits) and the sum one below 2^12 (42 bits), so neither the product nor the sum rounds and a fused multiply-add
    gives the same bits."""
    rng = np.random.default_rng(2)
    f, d = V.dyadic(rng, 600), V.dyadic(rng, 600)
    t = float(V.dyadic(rng, 1, 10, 2.0)[0])
    pa, pb = V.ls_points_twin(f, d, t, 0)
    from fractions import Fraction
    assert pb == [] and all(Fraction(p) == Fraction(t) * Fraction(float(di)) + Fraction(float(fi))
                            for p, di, fi in zip(pa, d, f))
    pa, pb = V.ls_points_twin(f, d, t, 599)
    assert len(pa) == 599 and len(pb) == 1
