"""The references and cases of the edge tests of the Gaussian-integral kernels (tests/_gto_edges.py) checked on the host:
the host Boys function on the stretched grid, the closed forms for s shells against the host twin and against 30-digit
arithmetic, the fixtures against the host twin they were recorded from, and the properties the cases are there for.
No GPU.  Every test prints its figures before it asserts; the recorded ones are in tests/_gto_edges.py."""
import os

import numpy as np
import pytest

from auto_oo_amd import _lib, gaussian, gto
from tests import _gto_d as D
from tests import _gto_edges as E


# ---- (a) and the host Boys function ---------------------------------------------------------------------------------
def test_host_boys_function_on_the_stretched_grid():
    """``gaussian._boys`` (scipy's hyp1f1) from T = 0 to 1e8 against 40 digits: within ``_gto_d.HOST_BOYS_ERROR``, the
    error the project's Boys bound was derived from, so the host twin is a reference for the stretched cases too."""
    T = E.boys_grid()
    assert T.size == 3 + 200 + 11 + 400 and T[1] == 5e-324 and np.sum(T == 5.0) == 1
    assert np.sum((T > 4.99999) & (T < 5.0)) == 5 and np.sum((T > 5.0) & (T < 5.00001)) == 5
    ref = E.boys_exact(8, T)
    assert ref[0] == pytest.approx([1.0 / (2 * n + 1) for n in range(9)], rel=1e-16)
    worst = []
    for n in range(9):
        rel = np.abs(gaussian._boys(n, T) - ref[:, n]) / ref[:, n]
        worst.append(rel.max())
        print(f"host boys n={n}: max rel {rel.max():.2e} at T = {T[np.argmax(rel)]!r} (recorded "
              f"{E.HOST_BOYS_EDGE[n]:.1e}, HOST_BOYS_ERROR {D.HOST_BOYS_ERROR[n]:.1e})")
    for n in range(9):
        assert worst[n] < D.HOST_BOYS_ERROR[n] and E.HOST_BOYS_EDGE[n] < D.HOST_BOYS_ERROR[n]


# ---- (b) closed forms -----------------------------------------------------------------------------------------------
def test_closed_forms_against_the_host_twin_on_four_shells():
    table = {"H": [("s", [6.0, 1.1], [0.3, 0.8]), ("s", [0.4], [1.0])],
             "O": [("s", [30.0, 2.4, 0.28], [0.2, -0.35, 0.9]), ("s", [0.9], [1.0])]}
    basis = gto.GTOBasis(["H", "O"], table)
    xyz = np.array([[0.1, -0.2, 0.3], [1.4, 0.9, -0.6]])
    S, h, g, nuc = gaussian.integrals_from_table(basis.table, basis.charges, xyz)
    ref = E.SClosed(xyz[[0, 0, 1, 1]], [(e, c) for _, _, e, c in basis.table], basis.charges, xyz)
    S2, h2 = ref.matrices()
    g2, g3 = ref.eri_full(), np.empty_like(g)
    idx = np.indices((4,) * 4).reshape(4, -1)
    g3.reshape(-1)[:] = ref.eri(*idx)
    d = [np.abs(S - S2).max(), np.abs(h - h2).max(), np.abs(g - g2).max(), np.abs(g - g3).max(), abs(nuc - ref.nuc())]
    print("closed forms against the host twin: S %.2e h %.2e g (blocked) %.2e g (listed) %.2e nuc %.2e" % tuple(d))
    assert max(d[:1] + d[2:]) < 2e-15 and d[1] < 2e-14                    # |h| up to 30
    assert np.array_equal(E.pack_g(E.unpack_g(E.pack_g(g), 4)), E.pack_g(g))
    assert np.array_equal(E.unpack_g(E.pack_g(g), 4), g)


def test_closed_forms_against_mpmath():
    """SAMPLE_N seeded elements each of S, h and g of N64 and two hand-made pairs of shells (T = 2.4e4 between two
    6000-exponent primitives 2 Bohr apart; T = 1e-9, below the switch to the Taylor series) at 30 digits."""
    _, _, ref = E.n_case(64)
    rng = np.random.default_rng(30)
    worst = {}
    i, j = rng.integers(0, 64, (2, E.SAMPLE_N))
    s, h = ref.one_electron(i, j)
    exact = np.array([ref.mp_element((a, b)) for a, b in zip(i, j)])
    S, H = ref.matrices()
    worst["S"] = np.abs(s - exact[:, 0]).max() / np.abs(S).max()
    worst["h"] = np.abs(h - exact[:, 1]).max() / np.abs(H).max()
    q = rng.integers(0, 64, (4, E.SAMPLE_N))
    q[:, :8] = np.arange(8)                                              # some of the largest: (aa|aa)
    got = ref.eri(*q)
    exact = np.array([ref.mp_element(tuple(c)) for c in q.T])
    big = ref.eri(*[np.arange(64)] * 4).max()
    worst["g"] = np.abs(got - exact).max() / big
    tight = E.SClosed([[0.0, 0.0, 0.0], [0.0, 1.2, 1.6], [0.0, 1.2, 1.6 + 2e-5]],
                      [([6000.0], [1.0]), ([6000.0, 5.0], [0.5, 0.5]), ([5.0], [1.0])], [1.0], [[0.0, 0.0, 0.0]])
    quartets = [(0, 0, 1, 1), (1, 1, 2, 2), (1, 2, 1, 2), (0, 1, 0, 1), (2, 2, 2, 2)]
    got = tight.eri(*np.array(quartets).T)
    exact = np.array([tight.mp_element(c) for c in quartets])
    assert 0.49 < got[0] < 0.51                                          # two point-like charges 2 Bohr apart
    worst["g, T = 2.4e4 and 1e-9"] = np.abs(got - exact).max() / np.abs(exact).max()
    print("closed forms against 30 digits, relative to the largest element:",
          {k: f"{v:.2e}" for k, v in worst.items()}, f"(recorded {E.CLOSED_FORM_DEVIATION:.1e})")
    assert max(worst.values()) <= E.CLOSED_FORM_DEVIATION


@pytest.mark.parametrize("nshell", [64, 128])
def test_the_large_tables_are_regular(nshell):
    basis, ang, ref = E.n_case(nshell)
    assert basis.nshell == basis.nao == nshell and basis.natm == nshell // 4
    assert sorted(set(basis.shells[:, 2].tolist())) == [1, 2]
    xyz = ang / E.BOHR
    dist = np.linalg.norm(xyz[:, None] - xyz[None, :], axis=-1) + 10.0 * np.eye(len(xyz))
    low = np.linalg.eigvalsh(ref.matrices()[0])[0]
    print(f"N{nshell}: smallest distance {dist.min():.3f} Bohr, smallest eigenvalue of S {low:.2e}")
    assert dist.min() >= 1.2 and low > 1e-4


def test_a_table_of_129_shells_is_refused_by_the_size_function():
    lib = _lib.load()
    assert lib.oovqe_gto_work_size(128, 2, 1) > 0
    assert lib.oovqe_gto_work_size(129, 1, 1) < 0
    assert b"nshell" in lib.oovqe_last_error()


# ---- the cases ------------------------------------------------------------------------------------------------------
def test_the_contraction_cases_are_what_they_are_there_for():
    want = {"Lss": (0, 0, 10, 10), "Lps": (1, 0, 8, 1), "Lpp": (1, 1, 1, 8), "Lds": (0, 2, 9, 7), "Ldp": (2, 1, 3, 10),
            "Ldd": (2, 2, 10, 3)}
    classes, longer_on_higher_l, longer_on_earlier, swapped = set(), set(), set(), set()
    for name, (la, lb, na, nb) in want.items():
        b = E.basis_of(name)
        assert (b.shells[:, 1] & 255).tolist() == [la, lb] and b.shells[:, 2].tolist() == [na, nb]
        assert b.shells[:, 0].tolist() == [0, 1]
        classes.add((max(la, lb), min(la, lb)))
        if na != nb:
            longer_on_earlier.add(na > nb)
            if la != lb:
                longer_on_higher_l.add((na > nb) == (la > lb))
        if la != lb:
            swapped.add(la > lb)                      # the higher-l shell comes first in the table: stored the other way
    assert classes == {(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)}
    assert longer_on_higher_l == {True, False} and longer_on_earlier == {True, False} and swapped == {True, False}
    three = E.basis_of("L3")
    assert three.shells[:, 2].tolist() == [10, 9, 8] and (three.shells[:, 1] & 255).tolist() == [0, 1, 2]
    assert three.max_nprim ** 2 == 100 and three.charges[0] == 1.0
    assert {E.form_of(n) for n in ("Lds", "Ldp", "Ldd", "L3")} == {"spherical", "cartesian"}
    for name in list(E.L_CASES) + ["LSP"]:
        for _, _, ex, co in E.basis_of(name).table:
            if len(co) >= 7:
                assert 0.25 <= np.mean(np.asarray(co) < 0) <= 0.4 and np.all(np.diff(ex) < 0)
    assert E.basis_of("LSP").shells[:, 2].tolist() == [10, 8, 9] and E.basis_of("LSP").max_l == 1


def test_the_geometry_cases_are_what_they_are_there_for():
    x = {n: E.xyz_of(n) for n in E.G_NAMES}
    dist = lambda r: np.linalg.norm(r[:, None] - r[None, :], axis=-1)[np.triu_indices(3, 1)]          # noqa: E731
    assert dist(x["G1"]).max() < 3.5 and dist(x["G2"]).min() >= 59.0 and dist(x["G2"]).max() > 295.0
    assert dist(x["G3"]).min() == pytest.approx(1e-3, rel=1e-9)
    assert np.allclose(x["G4"] - x["G1"], E.G4_SHIFT, atol=1e-13)
    assert np.all(x["G5"][:, :2] == 0.0)
    low = {n: np.linalg.eigvalsh(E.fixture(n)["S"])[0] for n in E.G_NAMES}
    print("smallest eigenvalue of the host overlap:", {n: f"{v:.2e}" for n, v in low.items()})
    assert low["G3"] < 0.9 * gto.INVSQRT_MIN_EIG and all(v > 1e-3 for n, v in low.items() if n != "G3")
    # the host twin itself has exact zeros between the fragments of G2, and no NaN
    f, frag = E.fixture("G2"), E.fragment_of_ao(E.basis_of("G2"))
    apart = frag[:, None] != frag[None, :]
    assert all(np.isfinite(f[k]).all() for k in ("S", "h", "g", "mom", "cross"))
    assert np.abs(f["S"][apart]).max() < 1e-300 and np.abs(f["g"][apart]).max() < 1e-300


def test_the_reordered_tables_are_permutations_of_the_originals():
    for name, atoms in (("L3", (2, 0, 1)), ("G1", (2, 1, 0))):
        new, ang, ao = E.reordered(name, atoms)
        ls = (new.shells[:, 1] & 255).tolist()
        assert ls[0] == 2 and new.nao == E.basis_of(name).nao and sorted(ao.tolist()) == list(range(new.nao))
        for a in range(new.natm):
            mine = [l for l, at in zip(ls, new.shells[:, 0]) if at == a]
            assert mine == sorted(mine, reverse=True)
        S = gaussian.one_electron_integrals(gaussian.shells_from_table(new.table, ang / E.BOHR), [], [])[0]
        U = gaussian.basis_transform(new.table, E.form_of(name))
        S = U @ S @ U.T
        want = E.fixture(name)["S"][np.ix_(ao, ao)]
        print(f"{name} reordered: host overlap against the permuted fixture {np.abs(S - want).max():.2e}")
        assert np.abs(S - want).max() < 1e-14


# ---- the kernel bodies on the host ----------------------------------------------------------------------------------
def test_kernel_bodies_on_the_host_against_the_fixtures_and_the_closed_forms():
    """The bodies of csrc/gto.hip and gto_d.hip as a host program (tools/gto_host.hip, one lane per group) on every
    fixture case and on the one-electron part of N128, at the bounds of the device tests: what a device run can still
    add is the device's exp, erf and sqrt, the contraction of a * b + c, and the butterfly over 8 lanes."""
    for name in E.FIXTURES:
        f = E.fixture(name)
        S, h, nuc, g = E.run_host_bodies(E.basis_of(name), E.xyz_of(name)[None])
        assert np.isfinite(S).all() and np.isfinite(h).all() and np.isfinite(g).all()          # every element written
        d = (np.abs(S[0] - f["S"]).max(), np.abs(h[0] - f["h"]).max(), np.abs(g[0] - f["g"]).max(),
             abs(nuc[0] - float(f["nuc"])))
        print(f"{name}: bodies on the host against the fixture: S {d[0]:.2e}, h {d[1]:.2e} (bound {f['bound_h']:.2e}), "
              f"g {d[2]:.2e}, nuc {d[3]:.2e} (bound {f['bound_g']:.2e})")
        assert d[1] < f["bound_h"] and max(d[0], d[2], d[3]) < f["bound_g"], name
    basis, ang, ref = E.n_case(128)
    S, h, nuc, _ = E.run_host_bodies(basis, (ang / E.BOHR)[None], with_g=False)
    Sr, hr = ref.matrices()
    for n, got, want in (("S", S[0], Sr), ("h", h[0], hr), ("nuc", nuc, np.array([ref.nuc()]))):
        err, big = np.abs(got - want).max(), np.abs(want).max()
        print(f"N128 {n}: bodies on the host against the closed forms {err:.2e} (bound {E.N_RTOL * big:.2e})")
        assert err < E.N_RTOL * big, n


# ---- (c) the fixtures -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.FIXTURES)
def test_fixtures_are_those_of_the_generator(name):
    """A seeded sample of every fixture through the host twin, one shell pair (for g: one element) at a time: equal to
    1e-14 of the largest element of the block."""
    f, basis = E.fixture(name), E.basis_of(name)
    assert os.path.getsize(E.fixture_path(name)) <= 182210                # the largest file of tests/golden before
    assert 0.0 < f["diff_g"] < 1e-10 and 0.0 < f["diff_h"] < 1e-9
    shell, N = E.shell_of_ao(basis), basis.nao
    rng = np.random.default_rng(sum(map(ord, name)))
    worst = 0.0
    for _ in range(2):
        sa, sb = rng.integers(0, basis.nshell, 2)
        rows, cols = np.nonzero(shell == sa)[0], np.nonzero(shell == sb)[0]
        for what, key in (("S", "S"), ("h", "h"), ("mom", "mom"), ("cross", "cross")):
            got = E.host_pair_block(name, int(sa), int(sb), what)
            want = f[key][..., rows[:, None], cols[None, :]]
            rel = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
            worst = max(worst, rel)
            assert rel <= 1e-14, (name, what, sa, sb, rel)
    for _ in range(2):
        idx = tuple(int(i) for i in rng.integers(0, N, 4))
        got, want = E.host_quartet(name, idx), f["g"][idx]
        block = f["g"][np.ix_(*[np.nonzero(shell == shell[i])[0] for i in idx])]
        rel = abs(got - want) / max(np.abs(block).max(), 1e-300)
        worst = max(worst, rel)
        assert rel <= 1e-14, (name, idx, got, want)
    nuc = sum(basis.charges[i] * basis.charges[j] / np.linalg.norm(E.xyz_of(name)[i] - E.xyz_of(name)[j])
              for i in range(basis.natm) for j in range(i))
    assert float(f["nuc"]) == nuc
    print(f"{name}: sampled blocks and elements reproduce the fixture to {worst:.1e} (bound 1e-14); diff_h "
          f"{float(f['diff_h']):.2e}, diff_g {float(f['diff_g']):.2e}")
    if name == "G4":
        print("G4 - G1 by the host twin:", {k: f"{float(f[k]):.2e}" for k in f if k.startswith("g4_")})
        assert all(0.0 < float(f[k]) < 1e-10 for k in f if k.startswith("g4_"))
