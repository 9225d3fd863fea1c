"""Overlaps between geometries, host side: the host twin of the cross overlap and its identities, the kernel bodies of
csrc/gto_cross.hip run on the CPU against it, the independent reference of tests/_overlaps.py against the oracle's dense
operator and against itself through the core fold, root tracking, and the interface (header, bindings, refusals).  No GPU.
"""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests import _gto_d as D
from tests import _overlaps as V
from auto_oo_amd import _lib, berry, gaussian, gto, overlaps
from auto_oo_amd.berry import sector_tables
from auto_oo_amd.sector import sector_of
from oracle import cpu_ref as R

BOHR = gaussian.BOHR
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECTORS = [(2, 2), (3, 4), (3, 2), (4, 4)]                 # (ncas, nelecas)


def _sector(ncas, nelecas):
    return sector_of([1 if i < nelecas else 0 for i in range(2 * ncas)], ncas)


def _host_overlap(basis, xyz):
    shells = gaussian.shells_from_table(basis.table, np.asarray(xyz) / BOHR)
    U = gaussian.basis_transform(basis.table, basis.d_functions or "spherical")
    return U @ gaussian.one_electron_integrals(shells, (), ())[0] @ U.T


def _cases():
    water = gto.GTOBasis(["O", "H", "H"])
    return [("m1-spherical", D.m1_basis("spherical"), D.M1_XYZ, D.M1_MOVED),
            ("m1-cartesian", D.m1_basis("cartesian"), D.M1_XYZ, D.M1_MOVED),
            ("water-sto3g", water, D.WATER, D.WATER_2)]


# ---- 1. host cross overlap ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_host_cross_overlap_identities(case):
    _, basis, xa, xb = case
    form = basis.d_functions or "spherical"
    cross = lambda a, b: gaussian.cross_overlap_from_table(basis.table, a / BOHR, b / BOHR, form)      # noqa: E731
    assert np.abs(cross(xa, xa) - _host_overlap(basis, xa)).max() < 1e-14
    ab, ba = cross(xa, xb), cross(xb, xa)
    assert ab.shape == (basis.nao, basis.nao)
    assert np.abs(ab - ba.T).max() <= 1e-15
    assert np.abs(ab - ab.T).max() > 1e-3                       # (not symmetric: the test would not see a transposition)
    assert np.abs(cross(xa + D.SHIFT, xb + D.SHIFT) - ab).max() < 1e-14


@pytest.mark.parametrize("form", ["spherical", "cartesian"])
def test_cross_kernel_bodies_on_the_cpu_against_the_host_twin(form):
    """All six pair classes, same-shell pairs at two positions, contracted d: the bound of the GPU test (6.3e-13)."""
    basis = D.m1_basis(form)
    xa = np.stack([D.M1_XYZ, D.M1_XYZ, D.M1_XYZ])
    xb = np.stack([D.M1_XYZ, D.M1_XYZ + np.array([0.05, 0.0, 0.0]), D.M1_MOVED])
    got = V.run_cross_bodies(basis, xa, xb)
    assert np.isfinite(got).all()                               # every element is written by some body
    for p in range(3):
        ref = gaussian.cross_overlap_from_table(basis.table, xa[p] / BOHR, xb[p] / BOHR, form)
        err = np.abs(got[p] - ref).max()
        print(f"cross bodies {form} pair {p}: {err:.2e}")
        assert err < 6.3e-13


def test_cross_kernel_bodies_on_the_cpu_s_and_p_classes():
    basis = gto.GTOBasis(["O", "H", "H"])
    got = V.run_cross_bodies(basis, D.WATER[None], D.WATER_2[None])[0]
    ref = gaussian.cross_overlap_from_table(basis.table, D.WATER / BOHR, D.WATER_2 / BOHR)
    assert np.abs(got - ref).max() < 6.3e-13


# ---- 2. the active-space expression against the oracle's dense operator ---------------------------------------------
@pytest.mark.parametrize("ncas,nelecas", SECTORS)
@pytest.mark.parametrize("kind", ["orthogonal", "improper", "nonorthogonal"])
def test_brute_force_is_the_orbital_rotation_operator_on_the_sector(ncas, nelecas, kind):
    U = V.trial_matrices(ncas, 100 * ncas + nelecas)[kind]
    if kind == "improper":
        assert np.linalg.det(U) < 0
    na_, nb_ = _sector(ncas, nelecas)
    _, _, x, _ = sector_tables(ncas, na_, nb_)
    eye = np.eye(x.size)
    got = V.brute_force(U, 0, ncas, na_, nb_, eye, eye)          # [J, I]
    G = R.orbital_rotation_operator(U)
    ref = G[np.ix_(x.reshape(-1), x.reshape(-1))]
    assert np.abs(got - ref).max() < 1e-12
    fold, det = V.core_fold(U, 0, ncas, na_, nb_, eye, eye)
    assert det == 1.0 and np.abs(fold - ref).max() < 1e-12


# ---- 3. core fold ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_core", [2, 5])
@pytest.mark.parametrize("ncas,nelecas", SECTORS)
def test_core_fold_equals_brute_force(n_core, ncas, nelecas):
    rng = np.random.default_rng(7 * n_core + ncas + nelecas)
    m = n_core + ncas
    s = np.eye(m) + 0.2 * rng.standard_normal((m, m))
    na_, nb_ = _sector(ncas, nelecas)
    Dc = sector_tables(ncas, na_, nb_)[2].size
    bra, ket = rng.standard_normal((2, Dc)), rng.standard_normal((3, Dc))
    bra, ket = bra / np.linalg.norm(bra, axis=1)[:, None], ket / np.linalg.norm(ket, axis=1)[:, None]
    ref = V.brute_force(s, n_core, ncas, na_, nb_, bra, ket)
    out, det = V.core_fold(s, n_core, ncas, na_, nb_, bra, ket)
    assert np.abs(det * det * out - ref).max() < 1e-12


# ---- 4. root tracking ----------------------------------------------------------------------------------------------------
def _planted(R_, G, seed):
    """A chain of near-identity overlaps seen through planted permutations and signs (geometry 0 untouched)."""
    rng = np.random.default_rng(seed)
    true = np.stack([0.9 * np.eye(R_) + 0.08 * rng.standard_normal((R_, R_)) for _ in range(G - 1)])
    perms = list(itertools.permutations(range(R_)))
    perm = np.array([list(range(R_))] + [perms[rng.integers(len(perms))] for _ in range(G - 1)])
    sign = np.vstack([np.ones(R_), rng.choice([-1.0, 1.0], size=(G - 1, R_))])
    O = np.empty_like(true)
    for g in range(G - 1):
        for i in range(R_):
            for j in range(R_):
                O[g, perm[g, i], perm[g + 1, j]] = sign[g, i] * sign[g + 1, j] * true[g, i, j]
    return O, perm, sign, rng


@pytest.mark.parametrize("R_", [2, 3, 4])
def test_track_roots_recovers_planted_permutations_and_signs(R_):
    G = 6
    O, perm, sign, rng = _planted(R_, G, 40 + R_)
    p, s = overlaps.track_roots(O)
    assert p.dtype == np.int64 and np.array_equal(p, perm) and np.array_equal(s, sign)
    pt, st = overlaps.track_roots(torch.as_tensor(O))
    assert np.array_equal(pt.numpy(), perm) and np.array_equal(st.numpy(), sign)
    # planted results: energies, vectors and a [G, R, R, 3] state matrix come back as they were before the tampering
    e_true = np.sort(rng.standard_normal((G, R_)), axis=1)
    v_true = rng.standard_normal((G, R_, 7))
    x_true = rng.standard_normal((G, R_, R_, 3))
    x_true = x_true + x_true.transpose(0, 2, 1, 3)
    e, v, x = np.empty_like(e_true), np.empty_like(v_true), np.empty_like(x_true)
    for g in range(G):
        for i in range(R_):
            e[g, perm[g, i]] = e_true[g, i]
            v[g, perm[g, i]] = sign[g, i] * v_true[g, i]
            for j in range(R_):
                x[g, perm[g, i], perm[g, j]] = sign[g, i] * sign[g, j] * x_true[g, i, j]
    assert np.array_equal(overlaps.apply_tracking(e, p, s), e_true)
    assert np.array_equal(overlaps.apply_tracking(v, p, s), v_true)
    assert np.array_equal(overlaps.apply_tracking(x, p, s), x_true)
    assert np.array_equal(overlaps.apply_tracking(x[..., 0], p, s, kind="matrices"), x_true[..., 0])
    xt = overlaps.apply_tracking(torch.as_tensor(x), pt, st)
    assert isinstance(xt, torch.Tensor) and np.array_equal(xt.numpy(), x_true)
    # diagonal blocks are unchanged by the signs
    k = np.arange(R_)
    assert np.array_equal(overlaps.apply_tracking(x, p, np.ones_like(s))[:, k, k], x_true[:, k, k])


def test_track_roots_resolves_a_tie_by_the_lowest_permutation():
    p, s = overlaps.track_roots(np.full((1, 2, 2), 0.5))
    assert np.array_equal(p, [[0, 1], [0, 1]]) and np.array_equal(s, np.ones((2, 2)))
    # three roots: (0, 2, 1) and (1, 2, 0) both reach 2.0; the lower one in lexicographic order wins, and the matched
    # negative overlap turns the sign
    O = np.array([[[0.5, 0.5, 0.0], [0.0, 0.0, -1.0], [0.5, 0.5, 0.0]]])
    p, s = overlaps.track_roots(O)
    assert np.array_equal(p[1], [0, 2, 1]) and np.array_equal(s[1], [1.0, -1.0, 1.0])
    with pytest.raises(ValueError):
        overlaps.track_roots(np.zeros((2, 5, 5)))
    with pytest.raises(ValueError):
        overlaps.apply_tracking(np.zeros((2, 2)), p, s)


# ---- 5. interface -----------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("oovqe_gto_cross_overlap_batch", "oovqe_sector_overlap_batch")


def test_header_bindings_and_exports():
    with open(os.path.join(ROOT, "include", "oovqe.h")) as fh:
        hdr = fh.read()
    declared = set(re.findall(r"\b(oovqe_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    from auto_oo_amd import ci
    for macro, value in (("OOVQE_OVERLAP_MAX_NCAS", overlaps.MAX_NCAS), ("OOVQE_OVERLAP_MAX_M", overlaps.MAX_M),
                         ("OOVQE_OVERLAP_MAX_STRINGS", overlaps.MAX_STRINGS),
                         ("OOVQE_OVERLAP_MAX_ROOTS", overlaps.MAX_ROOTS)):
        assert int(re.search(rf"#define {macro} (\S+)", hdr).group(1)) == value
    assert (overlaps.MAX_NCAS, overlaps.MAX_M, overlaps.MAX_STRINGS) == (8, 48, 70)
    assert overlaps.MAX_ROOTS == ci.MAX_ROOTS
    import auto_oo_amd as aoo
    for name in ("overlaps", "sector_overlaps", "state_overlaps_oao", "track_roots", "apply_tracking",
                 "cross_overlap_batch"):
        assert hasattr(aoo, name) and name in aoo.__all__
    for name in ("state_overlaps", "berry_phase", "casci_overlaps"):
        assert callable(getattr(aoo.OO_pqc_batch, name))
    assert "track_roots" in aoo.OO_pqc_batch.casci_dipole_matrix.__doc__
    assert "track_roots" in aoo.OO_pqc_batch.casci_nuclear_gradients.__doc__


def _sector_call(lib, **kw):
    a = dict(m=3, n_core=0, ncas=3, n_alpha=2, n_beta=2, npair=1, rb=1, rk=1, ld=9, mode=0)
    a.update(kw)
    return lib.oovqe_sector_overlap_batch(None, a["m"], a["n_core"], a["ncas"], a["n_alpha"], a["n_beta"], a["npair"],
                                          None, a["rb"], None, a["rk"], None, ctypes.c_int64(a["ld"]), a["mode"], 1,
                                          None, None, None)


@pytest.mark.parametrize("kw,text", [(dict(ncas=9, m=9), "ncas = 9"), (dict(m=49, n_core=46), "m = 49"),
                                     (dict(m=4), "m = 4"), (dict(n_alpha=4), "(4, 2)"), (dict(rb=5), "5 bra"),
                                     (dict(rk=0), "0 ket"), (dict(mode=2), "mode = 2"), (dict(ld=8), "ld = 8"),
                                     (dict(npair=-1), "npair = -1"), (dict(), "null pointer")])
def test_the_sector_entry_refuses_what_is_out_of_scope_before_any_launch(kw, text):
    lib = _lib.load()
    assert _sector_call(lib, **kw) < 0
    assert text in lib.oovqe_last_error().decode()


def test_the_cross_entry_refuses_bad_sizes_before_any_launch():
    lib = _lib.load()
    call = lambda nshell, npair: lib.oovqe_gto_cross_overlap_batch(nshell, None, 3, None, None, 2, npair, None, None,  # noqa: E731
                                                                   2, None, None)
    assert call(0, 1) < 0 and b"nshell = 0" in lib.oovqe_last_error()
    assert call(129, 1) < 0 and b"nshell = 129" in lib.oovqe_last_error()
    assert call(2, -1) < 0 and b"npair = -1" in lib.oovqe_last_error()
    assert call(2, 1) < 0 and b"null pointer" in lib.oovqe_last_error()
    assert call(2, 0) == 0


def test_python_errors_come_before_any_device_call():
    z = np.zeros((1, 3, 3))
    v = np.zeros((1, 1, 9))
    with pytest.raises(ValueError, match="ActiveSpaceRotation"):
        overlaps.sector_overlaps(z, 0, 3, 2, 2, v, v, orthogonalize="polar")
    with pytest.raises(ValueError, match="givens"):
        overlaps.sector_overlaps(z, 0, 3, 2, 2, v, v, orthogonalize="qr")
    with pytest.raises(ValueError, match="ncas = 9"):
        overlaps.sector_overlaps(np.zeros((1, 9, 9)), 0, 9, 2, 2, v, v)
    with pytest.raises(ValueError, match="at most 48"):
        overlaps.sector_overlaps(np.zeros((1, 49, 49)), 45, 4, 2, 2, v, v)
    with pytest.raises(ValueError, match="ActiveSpaceRotation"):
        overlaps.state_overlaps_oao(v[:, 0], v[:, 0], z, z, [0, 1, 2], 4, orthogonalize="polar")


# ---- 6. the determinant and sign routines of the sector kernel on the CPU ---------------------------------------------
def _strings(ncas, k):
    return [v for v in range(1 << ncas) if bin(v).count("1") == k]


def _minor_cases():
    mats = dict(V.pivot_matrices(8))
    mats["random"] = V.trial_matrices(8, 88)["nonorthogonal"]
    mats["permutation"] = V.trial_matrices(8, 88)["permutation"]
    out = [(8, name, U) for name, U in mats.items()]
    out.append((5, "random", V.trial_matrices(5, 55)["nonorthogonal"]))       # (another ncas: the strings' bit order)
    out.append((5, "exchange", V.pivot_matrices(5)["exchange"]))
    return out


@pytest.mark.parametrize("case", _minor_cases(), ids=lambda c: f"{c[1]}{c[0]}")
def test_ovl_minor_on_the_cpu_against_mpmath_det(case):
    """Every order K = 0 .. ncas, every pair of strings: ``ovl_minor<K>`` through the kernel's switch against
    ``np.linalg.det`` of the submatrix, and 40 seeded pairs per order against 40-digit ``mpmath.det``.  Bound: 1e-13 x
    the Hadamard bound of the submatrix (the product of the norms of its rows) -- an LU of order <= 8 in float64 loses
    a few 1e-16 of that.  Measured: at most 3.9e-16 of it (mpmath), 1.1e-15 (numpy, whose own LU is in that figure)."""
    ncas, name, U = case
    res = V.run_overlap_host([(ncas, k, U, _strings(ncas, k), _strings(ncas, k)) for k in range(ncas + 1)])
    rng = np.random.default_rng(ncas)
    worst_mp = worst_np = 0.0
    for k, (got, _) in enumerate(res):
        strs = _strings(ncas, k)
        occ = [[p for p in range(ncas) if (m >> (ncas - 1 - p)) & 1] for m in strs]
        assert got.shape == (len(strs), len(strs)) and np.isfinite(got).all()
        if k == 0:
            assert got[0, 0] == 1.0
            continue
        sub = np.stack([[U[np.ix_(oj, oi)] for oi in occ] for oj in occ])            # [J, I, k, k]
        hadamard = np.prod(np.linalg.norm(sub, axis=3), axis=2)
        err = np.abs(got - np.linalg.det(sub))
        assert (err <= 1e-13 * hadamard).all(), (name, k)
        worst_np = max(worst_np, (err / np.maximum(hadamard, 1e-300)).max())
        # where a column or a row of the submatrix vanishes, the minor is exactly 0
        dead = (np.abs(sub).max(axis=2) == 0).any(axis=2) | (np.abs(sub).max(axis=3) == 0).any(axis=2)
        assert (got[dead] == 0.0).all()
        if name in ("zero_column", "zero_row"):
            assert dead.sum() == (len(strs) * sum(1 for o in occ if 2 in o))
        pairs = {(int(a), int(b)) for a, b in rng.integers(0, len(strs), (40, 2))} | {(0, 0), (len(strs) - 1, 0)}
        for j, i in sorted(pairs):
            ref = float(V.exact_det(sub[j, i].tolist()))
            e = abs(got[j, i] - ref)
            assert e <= 1e-13 * hadamard[j, i], (name, k, j, i, got[j, i], ref)
            if hadamard[j, i] > 0:
                worst_mp = max(worst_mp, e / hadamard[j, i])
    print(f"ovl_minor {name} ncas {ncas}: worst {worst_mp:.2e} (mpmath), {worst_np:.2e} (numpy) of the Hadamard bound")


def test_ovl_minor_sees_a_transposition_and_a_missed_exchange():
    """The test above would notice: the minors of U^T, and the minors without their exchange signs, differ from those
    of U by far more than the bound."""
    U = V.pivot_matrices(8)["exchange"]
    strs = _strings(8, 4)
    (a, _), (b, _) = V.run_overlap_host([(8, 4, U, strs, strs), (8, 4, U.T.copy(), strs, strs)])
    assert np.abs(a - b.T).max() < 1e-13 and np.abs(a - b).max() > 1e-2
    assert np.abs(np.abs(a) - a).max() > 1e-2                   # (both signs occur: a lost exchange would show)


def test_ovl_sign_on_the_cpu_is_the_sign_table_of_every_sector():
    recs, want = [], []
    for ncas in range(1, 9):
        for n_alpha in range(ncas + 1):
            for n_beta in range(ncas + 1):
                ua, ub, _, sign = sector_tables(ncas, n_alpha, n_beta)
                assert list(ua) == _strings(ncas, n_alpha) and list(ub) == _strings(ncas, n_beta)
                recs.append((ncas, -1, np.eye(ncas), list(ua), list(ub)))
                want.append(sign)
    for (minors, got), ref, rec in zip(V.run_overlap_host(recs), want, recs):
        assert minors is None and np.array_equal(got, ref), rec[0]


# ---- 7. the 40-digit reference and its fixtures -----------------------------------------------------------------------
def test_exact_reference_is_the_host_route_and_brute_force():
    rng = np.random.default_rng(17)
    s = V._generic_s(5, 2, rng)
    bra, ket = rng.standard_normal((2, 9)), rng.standard_normal((3, 9))
    out, det, U = V.exact_reference(s, 2, 3, 2, 1, bra, ket)
    brute = V.brute_force(s, 2, 3, 2, 1, bra, ket)
    assert np.abs(det * det * out - brute).max() < 1e-13 and abs(det - np.linalg.det(s[:2, :2])) < 1e-15
    # unsigned, through an index table with entries outside the vector, and the Q factor
    index = np.array([3, -1, 0, 9, 8, 1, 2, 7, 4])
    out1, _, Q = V.exact_reference(s, 2, 3, 2, 1, bra, ket, index, 1, False)
    host, _ = V.host_reference(s, 2, 3, 2, 1, bra, ket, index, 1, False)
    assert np.abs(out1 - host).max() < 1e-13
    assert np.abs(Q.T @ Q - np.eye(3)).max() < 1e-15
    assert np.abs(Q - berry.givens_orthogonal(U)).max() < 1e-14 and (np.diag(Q.T @ U) > 0).all()


def test_the_scope_fixtures_are_complete_and_one_regenerates():
    for name in V.SCOPE_CASES:
        f = V.scope_fixture(name)
        ncas, n_alpha, n_beta, n_core, mode, P, rb, rk, _ = V.SCOPE_CASES[name]
        assert (int(f["ncas"]), int(f["n_alpha"]), int(f["n_beta"]), int(f["n_core"]), int(f["mode"])) == \
            (ncas, n_alpha, n_beta, n_core, mode)
        assert f["out"].shape == (P, rb, rk) and f["core_det"].shape == (P,) and np.isfinite(f["out"]).all()
        assert os.path.getsize(V.scope_fixture_path(name)) < 120 * 1024
        if V.SCOPE_CASES[name][8] == "generic" and n_core > 1:
            assert f["cond_core"].max() < 5.0
            assert (np.abs(f["s"][:, 1:n_core, 0]).max(axis=1) > np.abs(f["s"][:, 0, 0])).all()      # the first search swaps
    for name, cond in (("c4_32_cond3", 1e3), ("c4_32_cond6", 1e6)):
        assert np.abs(V.scope_fixture(name)["cond_core"] / cond - 1).max() < 1e-6
    for name, cond in (("c6_42_q2", 1e2), ("c6_42_q5", 1e5)):
        assert np.abs(V.scope_fixture(name)["cond_U"] / cond - 1).max() < 1e-6
    f = V.scope_fixture("c4_21_perm6")
    assert np.array_equal(np.abs(f["core_det"]), np.ones(2)) and (np.diagonal(f["s"][:, :6, :6], axis1=1, axis2=2) == 0).all()
    a, b = V.scope_fixture("c8_43_core40"), V.scope_fixture("c8_34_core40")
    assert np.array_equal(a["s"], b["s"]) and not np.array_equal(a["out"], b["out"])
    new, old = V.make_scope_case("c5_05_core3"), V.scope_fixture("c5_05_core3")
    assert set(new) == set(old)
    for key in new:
        assert np.array_equal(np.asarray(new[key]), old[key]), key
