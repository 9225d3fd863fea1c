"""The Gaussian-integral kernels (csrc/gto.hip, gto_d.hip, gto_moments.hip, gto_cross.hip, gto_grad.hip,
gto_grad_sets.hip) at the limits of their shell table: contractions of 1 to 10 primitives in both orientations of a
pair, Boys arguments from 0 to 1e8, dissociated, nearly coincident, far-away and collinear geometries, tables of 64
and 128 shells, and tables listed d, p, s.  Cases and references: tests/_gto_edges.py.

Bounds (none taken from device output):

* Boys function: ``_gto_d.BOYS_RTOL[n]`` per order against 40-digit arithmetic.
* L-, G- and O-cases: 10 x the change that a Boys function perturbed by BOYS_RTOL makes to the host twin's h and g of
  the very case (stored in the fixture: ``diff_h``, ``diff_g``); S, nuc, moments and cross overlaps take the bound of
  g.  G4 against G1: 10 x what the host twin shows between the two (``g4_*`` of the G4 fixture).
  The moments alone get a term for the number format added to that bound: 4 x 2^-52 x the largest moment element of the
  case (two roundings each for the reference and the device).  A second moment grows with the square of the distance
  from the origin; in G2 the largest element is 5.8e4, whose neighbours in fp64 are 7.3e-12 apart, and the 3z^2 - r^2
  and x^2 - y^2 functions of the d shell subtract such elements from each other: there no computation in fp64 meets an
  absolute 3e-12 (the device and the host twin differ by two spacings, 1.5e-11).  For every other case the term is below
  1e-14 and the bound is that of g.
* N-cases: ``_gto_edges.N_RTOL`` (10 x the deviation of the closed forms from their 30-digit evaluation) times the
  largest element of the quantity; S^-1/2 of N64 against ``moldata.ao_to_oao`` at 1e-10.
* Gradients: 10 x the disagreement of the 4th-order finite difference of ``gto.integrals_into`` at h = 1e-3 with itself
  at h = 2e-3, per term (the rule and the helpers of tests/test_nucgrad_gpu.py); a set of ``gradient_sets_batch``
  against ``gradient_batch`` of its densities at 1e-12 (tests/test_casci_gradients_gpu.py).

Every test prints its figures next to the bound before it asserts.  Measured on an MI355X (largest deviation / bound):

    Boys function, n = 0 .. 8   2.8e-16 2.7e-16 4.5e-16 5.2e-16 6.5e-16 7.8e-16 1.2e-15 2.1e-15 4.2e-15 (n >= 6 at T = 5,
                                n = 1 .. 5 at T = 7e3 .. 1.8e6, n = 0 one spacing below 5) / 2.1e-14 .. 1.6e-12
    case   overlap   int1e_ao            int2e_ao            moments   cross overlap
    Lss    2.2e-16   8.5e-14 / 3.1e-11   6.7e-15 / 7.2e-13   4.4e-16   5.6e-17
    Lps    4.4e-16   4.3e-14 / 4.3e-12   2.7e-15 / 6.4e-12   8.9e-16   3.3e-16
    Lpp    4.4e-16   1.8e-14 / 4.1e-11   2.7e-15 / 4.4e-12   1.6e-15   4.4e-16
    Lds    8.9e-16   1.4e-14 / 3.3e-11   6.1e-15 / 3.7e-12   2.2e-15   1.1e-15
    Ldp    1.0e-15   1.1e-13 / 3.8e-11   2.9e-15 / 4.6e-12   3.6e-15   1.0e-15
    Ldd    1.0e-15   1.4e-14 / 8.7e-12   8.1e-15 / 3.0e-12   2.7e-15   5.6e-16
    L3     6.7e-16   5.7e-14 / 3.5e-11   1.1e-14 / 6.2e-12   2.2e-15   8.3e-16     (the same reordered)
    G1     3.3e-16   1.4e-14 / 1.1e-11   3.2e-15 / 3.1e-12   1.8e-15   6.7e-16     (reordered: 1.1e-14, 4.6e-15)
    G2     2.2e-16   3.6e-14 / 9.0e-12   3.2e-15 / 3.1e-12   1.5e-11 / 5.5e-11 (largest element 5.8e4)   6.7e-16
    G3     8.9e-16   3.4e-14 / 1.4e-11   6.8e-15 / 4.6e-12   1.3e-15   8.9e-16
    G4     2.2e-16   1.0e-13 / 1.1e-11   6.0e-15 / 3.1e-12   2.8e-14   1.3e-15
    G5     3.3e-16   8.0e-15 / 1.0e-11   3.2e-15 / 3.1e-12   2.2e-15   6.7e-16
    G4 - G1 on the device: S 6.6e-15 / 6.5e-14, h 1.8e-13 / 1.6e-12, g 8.7e-15 / 1.1e-13; between the fragments of G2 every
    element of S, h, g and of the cross overlaps G1/G2 is 0.0; info of G1 .. G5 = 0, 0, -1, 0, 0.
    N64    S 3.3e-16 / 2.4e-15, h 2.8e-14 / 1.9e-13, g 4.4e-16 / 4.5e-15, nuc 0 / 5.9e-12, S^-1/2 1.4e-12 / 1e-10
    N128   S 4.4e-16 / 2.4e-15, h 4.3e-14 / 2.4e-13, nuc 0 / 1.8e-11, g (250000 elements) 5.6e-16 / 4.4e-15
    gradients (error / bound), D1 . dh | WQ . dS | 1/2 D2 . dg | nuclear | six sets against the single-set entry:
    Lss    2.4e-11 / 8.1e-10 | 2.6e-13 / 3.3e-12 | 1.1e-12 / 8.7e-11 | 4.9e-13 / 1.1e-11 | 0
    Lps    6.5e-11 / 7.5e-10 | 4.8e-13 / 1.3e-11 | 1.9e-11 / 7.4e-10 | 4.9e-13 / 1.1e-11 | 8.2e-16
    Lpp    1.3e-11 / 5.2e-10 | 3.3e-13 / 1.6e-11 | 1.3e-11 / 9.8e-10 | 4.9e-13 / 1.1e-11 | 1.2e-14
    LSP    2.1e-10 / 4.7e-9  | 7.3e-13 / 6.2e-11 | 2.2e-10 / 1.9e-9  | 5.1e-13 / 9.3e-12 | 1.6e-15
    G3sp   5.1e-10 / 1.0e-7  | 3.3e-12 / 2.2e-10 | 1.1e-9 / 2.4e-8   | closed form 1.8e-15 (largest 3.9e7) | 5.8e-16
    G5sp   8.2e-11 / 3.6e-9  | 9.4e-13 / 1.2e-10 | 2.8e-10 / 7.6e-9  | 4.0e-12 / 4.3e-10 | 3.3e-16
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from auto_oo_amd import _lib, gto, moldata, ops             # noqa: E402
from tests import _gto_d as D                               # noqa: E402
from tests import _gto_edges as E                           # noqa: E402
from tests.test_nucgrad_gpu import H1, H2, fd_combine, fd_stack   # noqa: E402

F64 = torch.float64
BOHR = E.BOHR
NAMES = ("overlap", "int1e_ao", "int2e_ao", "nuc")


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def to_dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dev())


def into_nan_filled(basis, xyz_bohr):
    """``integrals_into`` on outputs that start as NaN -> (S, h, g, nuc)"""
    G, N = int(xyz_bohr.shape[0]), basis.nao
    out = [torch.full(s, float("nan"), dtype=F64, device=dev()) for s in ((G, N, N), (G, N, N), (G, N, N, N, N), (G,))]
    gto.integrals_into(basis, xyz_bohr, *out)
    return out


def assert_structure(S, h, g):
    assert torch.equal(g, g.permute(0, 2, 1, 3, 4)) and torch.equal(g, g.permute(0, 1, 2, 4, 3))
    assert torch.equal(g, g.permute(0, 3, 4, 1, 2))
    assert torch.equal(S, S.transpose(1, 2)) and torch.equal(h, h.transpose(1, 2))


def stack_and_members(basis, ang):
    """``integrals_batch`` and ``integrals_into`` of the stack ``ang`` [G, natm, 3] (Angstrom): every element written, no
    NaN or Inf, the same bits from both entries and from every member alone, exact symmetries, eri_flags 3.
    -> the namespace of ``integrals_batch``"""
    I = gto.integrals_batch(basis, ang, check_overlap=False)
    out = into_nan_filled(basis, gto.coords_to_device(basis, ang))
    for name, x in zip(NAMES, out):
        assert torch.isfinite(x).all(), name
        assert torch.equal(x, getattr(I, name)), name
    for k in range(ang.shape[0]):
        one = gto.integrals_batch(basis, ang[k:k + 1], check_overlap=False)
        for name in NAMES:
            assert torch.equal(getattr(I, name)[k], getattr(one, name)[0]), (name, k)
        assert int(one.info[0]) == int(I.info[k])
        assert torch.equal(torch.nan_to_num(one.oao_coeff[0], nan=7.0), torch.nan_to_num(I.oao_coeff[k], nan=7.0))
        assert ops.eri_flags(one.int2e_ao[0]) == 3
    assert_structure(I.overlap, I.int1e_ao, I.int2e_ao)
    assert ops.eri_flags(I.int2e_ao) == 3
    return I


def compare(tag, I, k, ref, bound_h, bound_g, perm=None):
    """geometry k of the device integrals (functions ``perm`` of them) against the reference dict"""
    sel = (lambda x: x) if perm is None else (lambda x: x[np.ix_(*([perm] * x.ndim))])
    d = {"overlap": np.abs(sel(I.overlap[k].cpu().numpy()) - ref["S"]).max(),
         "int1e_ao": np.abs(sel(I.int1e_ao[k].cpu().numpy()) - ref["h"]).max(),
         "int2e_ao": np.abs(sel(I.int2e_ao[k].cpu().numpy()) - ref["g"]).max(),
         "nuc": abs(I.nuc[k].item() - float(ref["nuc"]))}
    print(f"{tag}: " + ", ".join(f"{n} {v:.2e}" for n, v in d.items()) + f" (bounds: h {bound_h:.2e}, others {bound_g:.2e})")
    assert d["int1e_ao"] < bound_h, (tag, d)
    assert d["overlap"] < bound_g and d["int2e_ao"] < bound_g and d["nuc"] < bound_g, (tag, d)


def moments_and_cross(tag, name, basis, ang, ang_disp, perm=None):
    """order-2 moments about ``origin_of(name)`` and the cross overlap with the displaced copy against the fixture; the
    cross overlap of a geometry with itself is S"""
    f = E.fixture(name)
    xyz = gto.coords_to_device(basis, np.stack([ang, ang_disp]))
    origin = to_dev(np.broadcast_to(E.origin_of(name), (2, 3)))
    M = torch.full((2, 9, basis.nao, basis.nao), float("nan"), dtype=F64, device=dev())
    gto.moment_integrals_into(basis, xyz, M, 2, origin)
    assert torch.isfinite(M).all()
    assert torch.equal(M, M.transpose(2, 3))
    one = torch.empty_like(M[:1])
    gto.moment_integrals_into(basis, xyz[:1].contiguous(), one, 2, origin[:1].contiguous())
    assert torch.equal(one[0], M[0])
    sel = (lambda x: x) if perm is None else (lambda x: x[..., perm, :][..., :, perm])
    m = sel(M[0].cpu().numpy())
    dm, big = np.abs(m - f["mom"]).max(), np.abs(f["mom"]).max()
    bound_m = f["bound_g"] + 4 * 2.0 ** -52 * big
    X = torch.full((3, basis.nao, basis.nao), float("nan"), dtype=F64, device=dev())
    gto.cross_overlap_into(basis, xyz[[0, 0, 1]].contiguous(), xyz[[1, 0, 0]].contiguous(), X)
    assert torch.isfinite(X).all()
    x = X.cpu().numpy()
    dc = np.abs(sel(x[0]) - f["cross"]).max()
    ds = np.abs(sel(x[1]) - f["S"]).max()
    print(f"{tag}: moments {dm:.2e} (largest element {big:.3g}, bound {bound_m:.2e}), cross overlap {dc:.2e}, cross "
          f"overlap of the geometry with itself against S {ds:.2e} (bound {f['bound_g']:.2e})")
    assert dm < bound_m and dc < f["bound_g"] and ds < f["bound_g"]
    assert np.abs(x[2] - x[0].T).max() < f["bound_g"]                   # S_ab(b, a) = S_ab(a, b)^T


# ---- B: the Boys function -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def boys_reference():
    T = E.boys_grid()
    return T, E.boys_exact(8, T)


@pytest.mark.parametrize("nmax", [0, 4, 8])
def test_boys_function_from_zero_to_1e8_against_40_digits(nmax):
    T, ref = boys_reference()
    F = gto.boys(nmax, to_dev(T)).cpu().numpy()
    assert np.isfinite(F).all()
    rel = np.abs(F - ref[:, :nmax + 1]) / ref[:, :nmax + 1]
    for n in range(nmax + 1):
        print(f"boys nmax={nmax} n={n}: max rel {rel[:, n].max():.3e} at T = {T[np.argmax(rel[:, n])]!r} "
              f"(bound {D.BOYS_RTOL[n]:.1e})")
    for n in range(nmax + 1):
        assert rel[:, n].max() < D.BOYS_RTOL[n]


# ---- L: contraction length ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.L_CASES))
def test_long_contractions_element_by_element(name):
    basis, f = E.basis_of(name), E.fixture(name)
    ang = np.stack([E.angstrom_of(name), E.displaced_angstrom(name)])
    I = stack_and_members(basis, ang)
    assert int(I.info.abs().sum()) == 0
    compare(name, I, 0, f, f["bound_h"], f["bound_g"])
    moments_and_cross(name, name, basis, ang[0], ang[1])


# ---- G: geometry ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def g_stack():
    basis = E.basis_of("G1")
    ang = np.stack([E.angstrom_of(n) for n in E.G_NAMES])
    return basis, ang, stack_and_members(basis, ang)


@pytest.mark.parametrize("name", E.G_NAMES)
def test_geometries_element_by_element(name):
    basis, ang, I = g_stack()
    k, f = E.G_NAMES.index(name), E.fixture(name)
    compare(name, I, k, f, f["bound_h"], f["bound_g"])
    moments_and_cross(name, name, basis, ang[k], E.displaced_angstrom(name))


def test_the_nearly_singular_overlap_is_flagged_and_the_rest_of_the_stack_untouched():
    _, _, I = g_stack()
    k = E.G_NAMES.index("G3")
    info = I.info.cpu().tolist()
    print("info of G1 .. G5:", info)
    assert info == [-1 if n == "G3" else 0 for n in E.G_NAMES]
    assert torch.isnan(I.oao_coeff[k]).all()
    rest = [i for i in range(len(E.G_NAMES)) if i != k]
    assert torch.isfinite(I.oao_coeff[rest]).all()
    for i in rest:
        S = I.overlap[i].cpu().numpy()
        d = np.abs(I.oao_coeff[i].cpu().numpy() - moldata.ao_to_oao(S)).max()
        print(f"{E.G_NAMES[i]}: S^-1/2 against the host {d:.2e} (bound 1e-10)")
        assert d < 1e-10


def test_dissociated_fragments_give_exact_zeros():
    basis, ang, I = g_stack()
    k = E.G_NAMES.index("G2")
    frag = E.fragment_of_ao(basis)
    apart = to_dev(frag[:, None] != frag[None, :])
    S, h, g = I.overlap[k], I.int1e_ao[k], I.int2e_ao[k]
    worst = {"S": S[apart].abs().max().item(), "h": h[apart].abs().max().item(),
             "g (bra)": g[apart].abs().max().item(), "g (ket)": g[:, :, apart].abs().max().item()}
    X = gto.cross_overlap_batch(basis, ang[[0, k]], ang[[k, 0]])
    moved = to_dev(frag != 0)                 # atom 0 stands still; the others are 60 and 300 Bohr from every atom of G1
    worst["cross overlap G1/G2"] = X[0][:, moved].abs().max().item()
    worst["cross overlap G2/G1"] = X[1][moved, :].abs().max().item()
    assert X[0][~moved][:, ~moved].abs().max().item() > 0.1
    print("largest elements between fragments (0.0 or below 1e-300):", worst)
    assert all(v < 1e-300 for v in worst.values())
    assert torch.isfinite(X).all()
    # within a fragment the Coulomb integrals between fragments are those of two distant charge clouds: not zero
    a, b = int(np.nonzero(frag == 0)[0][0]), int(np.nonzero(frag == 2)[0][0])
    assert 1.0 / 400.0 < g[a, a, b, b].item() < 1.0 / 200.0


def test_a_translation_by_100_bohr_changes_nothing_beyond_the_host_twin_s_own_rounding():
    _, _, I = g_stack()
    a, b, f = E.G_NAMES.index("G1"), E.G_NAMES.index("G4"), E.fixture("G4")
    for name, key in (("overlap", "g4_S"), ("int1e_ao", "g4_h"), ("int2e_ao", "g4_g")):
        d = (getattr(I, name)[a] - getattr(I, name)[b]).abs().max().item()
        print(f"G4 - G1 {name}: {d:.2e} (host twin {float(f[key]):.2e}, bound {10 * float(f[key]):.2e})")
        assert d < 10 * float(f[key])


# ---- O: order of the table ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,atoms", [("L3", (2, 0, 1)), ("G1", (2, 1, 0))])
def test_a_table_listed_d_p_s_with_the_atoms_permuted_gives_the_permuted_integrals(name, atoms):
    basis, ang, ao = E.reordered(name, atoms)
    assert basis.shells[0, 1] & 255 == 2 and sorted(ao.tolist()) == list(range(basis.nao))
    f = E.fixture(name)
    disp = E.displaced_angstrom(name)[list(atoms)]
    I = stack_and_members(basis, np.stack([ang, disp]))
    inv = np.argsort(ao)                     # function inv[j] of the reordered basis is function j of the original
    compare(f"{name} reordered", I, 0, f, f["bound_h"], f["bound_g"], perm=inv)
    moments_and_cross(f"{name} reordered", name, basis, ang, disp, perm=inv)
    # and against the device integrals of the original order
    J = gto.integrals_batch(E.basis_of(name), E.angstrom_of(name)[None], check_overlap=False)
    ix = to_dev(inv)
    dg = (I.int2e_ao[0][ix][:, ix][:, :, ix][:, :, :, ix] - J.int2e_ao[0]).abs().max().item()
    dh = (I.int1e_ao[0][ix][:, ix] - J.int1e_ao[0]).abs().max().item()
    print(f"{name}: reordered against original on the device: h {dh:.2e} (bound {f['bound_h']:.2e}), g {dg:.2e} "
          f"(bound {f['bound_g']:.2e})")
    assert dh < f["bound_h"] and dg < f["bound_g"]


# ---- N: table size --------------------------------------------------------------------------------------------------
def test_64_s_shells_against_the_closed_forms():
    basis, ang, ref = E.n_case(64)
    S, h = ref.matrices()
    g = ref.eri_full()
    I = stack_and_members(basis, np.stack([ang, ang + 0.05]))
    assert int(I.info.abs().sum()) == 0
    d = {"overlap": (np.abs(I.overlap[0].cpu().numpy() - S).max(), np.abs(S).max()),
         "int1e_ao": (np.abs(I.int1e_ao[0].cpu().numpy() - h).max(), np.abs(h).max()),
         "int2e_ao": (np.abs(I.int2e_ao[0].cpu().numpy() - g).max(), np.abs(g).max()),
         "nuc": (abs(I.nuc[0].item() - ref.nuc()), ref.nuc())}
    for n, (err, big) in d.items():
        print(f"N64 {n}: {err:.2e}, largest element {big:.4g}, bound {E.N_RTOL * big:.2e}")
    X = moldata.ao_to_oao(S)
    dx = np.abs(I.oao_coeff[0].cpu().numpy() - X).max()
    print(f"N64 S^-1/2: {dx:.2e} (bound 1e-10; smallest eigenvalue of S {np.linalg.eigvalsh(S)[0]:.2e})")
    for n, (err, big) in d.items():
        assert err < E.N_RTOL * big, n
    assert dx < 1e-10


@functools.lru_cache(maxsize=None)
def n128():
    basis, ang, ref = E.n_case(128)
    return basis, gto.coords_to_device(basis, ang[None]), ref


def test_128_s_shells_one_electron_part():
    basis, xyz, ref = n128()
    assert basis.nshell == 128 == basis.nao
    S = torch.full((1, 128, 128), float("nan"), dtype=F64, device=dev())
    h, nuc = torch.full_like(S, float("nan")), torch.full((1,), float("nan"), dtype=F64, device=dev())
    gto.integrals_into(basis, xyz, S, h, None, nuc)
    assert torch.isfinite(S).all() and torch.isfinite(h).all() and torch.isfinite(nuc).all()
    assert torch.equal(S, S.transpose(1, 2)) and torch.equal(h, h.transpose(1, 2))
    Sr, hr = ref.matrices()
    for n, got, want in (("overlap", S[0].cpu().numpy(), Sr), ("int1e_ao", h[0].cpu().numpy(), hr),
                         ("nuc", nuc.cpu().numpy(), np.array([ref.nuc()]))):
        err, big = np.abs(got - want).max(), np.abs(want).max()
        print(f"N128 {n}: {err:.2e}, largest element {big:.4g}, bound {E.N_RTOL * big:.2e}")
        assert err < E.N_RTOL * big, n


def test_128_s_shells_two_electron_part():
    """The whole tensor (2.1 GB) stays on the device: no NaN, the three permutation equalities, and a seeded sample of
    250000 elements (a million takes the host 4 s) gathered there against the closed forms."""
    basis, xyz, ref = n128()
    g = torch.full((1,) + (128,) * 4, float("nan"), dtype=F64, device=dev())
    gto.integrals_into(basis, xyz, None, None, g, None)
    assert torch.isfinite(g).all()
    assert torch.equal(g, g.permute(0, 2, 1, 3, 4))
    assert torch.equal(g, g.permute(0, 1, 2, 4, 3))
    assert torch.equal(g, g.permute(0, 3, 4, 1, 2))
    idx = np.random.default_rng(128).integers(0, 128, (4, 250000))
    idx[:, :128] = np.arange(128)                                   # the diagonal (aa|aa): the largest elements
    flat = ((idx[0] * 128 + idx[1]) * 128 + idx[2]) * 128 + idx[3]
    got = g.reshape(-1)[to_dev(flat)].cpu().numpy()
    want = ref.eri(*idx)
    err, big = np.abs(got - want).max(), np.abs(want).max()
    print(f"N128 int2e_ao, 250000 sampled elements: {err:.2e}, largest element {big:.4g}, bound {E.N_RTOL * big:.2e}")
    assert err < E.N_RTOL * big


# ---- gradients ------------------------------------------------------------------------------------------------------
def seeded_sets(N, K):
    """K seeded sets of symmetrised standard-normal D1, WQ, D2 -> three device tensors [1, K, ...]"""
    rng = np.random.default_rng(6)
    d1, wq, d2 = rng.standard_normal((K, N, N)), rng.standard_normal((K, N, N)), rng.standard_normal((K,) + (N,) * 4)
    d1, wq = d1 + d1.transpose(0, 2, 1), wq + wq.transpose(0, 2, 1)
    d2 = d2 + d2.transpose(0, 2, 1, 3, 4)
    d2 = d2 + d2.transpose(0, 1, 2, 4, 3)
    d2 = d2 + d2.transpose(0, 3, 4, 1, 2)
    return tuple(to_dev(x)[None].contiguous() for x in (d1, wq, d2))


def fd_terms(basis, sets, xyz_bohr, h):
    """finite-difference gradients of D1_k . h, WQ_k . S, 1/2 D2_k . g, E_nuc -> [4, K, natm, 3] (host)"""
    d1, wq, d2 = sets
    K = d1.shape[1]
    S, hh, g, nuc = into_nan_filled(basis, to_dev(fd_stack(xyz_bohr, h)))
    vals = torch.stack((torch.einsum("gpq,kpq->kg", hh, d1[0]), torch.einsum("gpq,kpq->kg", S, wq[0]),
                        0.5 * torch.einsum("gpqrs,kpqrs->kg", g, d2[0]), nuc[None].expand(K, -1)))
    return fd_combine(vals, h).cpu().numpy()


def nuclear_repulsion_gradient(charges, xyz):
    """d/dR_A of sum_{i > j} Z_i Z_j / |R_i - R_j| -> [natm, 3]"""
    out = np.zeros_like(xyz)
    for a in range(len(charges)):
        for b in range(len(charges)):
            if a != b:
                r = xyz[a] - xyz[b]
                out[a] -= charges[a] * charges[b] * r / np.linalg.norm(r) ** 3
    return out


@pytest.mark.parametrize("name", ["Lss", "Lps", "Lpp", "LSP", "G3sp", "G5sp"])
def test_gradients_of_long_contractions_and_odd_geometries(name):
    """``gradient_batch`` term by term against finite differences, and the six sets of ``gradient_sets_batch`` (two
    passes of GRAD_SETS_TILE = 5) against ``gradient_batch`` of each.  G3sp / G5sp: the s and p shells of the G molecule
    (its d shell left out: the derivative kernels refuse one) at the geometries G3 and G5.  In G3 two nuclei are 1e-3
    Bohr apart, which is the step of the finite difference: 1 / R cannot be differentiated that way, so the nuclear
    repulsion term of G3 is compared with its closed form to 1e-12 of its largest component instead and left out of the
    sets; every integral is smooth there, and the other three terms keep the finite-difference reference."""
    if name.endswith("sp"):
        table = {k: [s for s in v if s[0] != "d"] for k, v in E.G_TABLE.items()}
        basis, ang = gto.GTOBasis(E.G_SYMBOLS, table), E.angstrom_of(name[:2])
    else:
        basis, ang = E.basis_of(name), E.angstrom_of(name)
    K, N = 6, basis.nao
    assert K > gto.GRAD_SETS_TILE
    sets = seeded_sets(N, K)
    xyz = ang / BOHR
    a, b = fd_terms(basis, sets, xyz, H1), fd_terms(basis, sets, xyz, H2)
    fd_nuc = name != "G3sp"
    if not fd_nuc:
        a[3] = b[3] = 0.0
    x = to_dev(xyz[None])
    for t, term in enumerate(("dm1", "wq", "dm2", "nuc")):
        arg = {n: (s[:, 0].contiguous() if n == term else None) for n, s in zip(("dm1", "wq", "dm2"), sets)}
        got = gto.gradient_into(basis, x, arg["dm1"], arg["wq"], arg["dm2"], term == "nuc")[0].cpu().numpy()
        if term == "nuc" and not fd_nuc:
            want = nuclear_repulsion_gradient(basis.charges, xyz)
            err, bound = np.abs(got - want).max(), 1e-12 * np.abs(want).max()
            print(f"{name} nuc: max |grad| {np.abs(want).max():.3g}, against the closed form {err:.2e} (bound {bound:.2e})")
        else:
            dis = np.abs(a[t] - b[t]).max()
            err, bound = np.abs(got - a[t, 0]).max(), 10 * dis
            print(f"{name} {term}: max |grad| {np.abs(a[t, 0]).max():.3g}, reference disagreement {dis:.2e}, bound "
                  f"{bound:.2e}, error {err:.2e}")
        assert err < bound, (name, term)
    many = gto.gradient_sets_into(basis, x, *sets, nuc=fd_nuc)
    assert tuple(many.shape) == (1, K, basis.natm, 3) and torch.isfinite(many).all()
    ref_all, worst, worst_fd = a.sum(axis=0), 0.0, 0.0
    dis_all = np.abs(a.sum(axis=0) - b.sum(axis=0)).reshape(K, -1).max(axis=1)
    for k in range(K):
        single = gto.gradient_into(basis, x, *(s[:, k].contiguous() for s in sets), fd_nuc)
        worst = max(worst, ((many[:, k] - single).abs().max() / single.abs().max()).item())
        err = np.abs(many[0, k].cpu().numpy() - ref_all[k]).max()
        worst_fd = max(worst_fd, err / (10 * dis_all[k]))
        assert err < 10 * dis_all[k], (name, k, err, dis_all[k])
    print(f"{name}: six sets against the single-set entry {worst:.2e} of the largest component (bound 1e-12); "
          f"against finite differences at most {worst_fd:.2f} of the bound")
    assert worst <= 1e-12


def test_gradients_of_the_d_cases_stay_refused():
    basis = E.basis_of("Lds")
    with pytest.raises(NotImplementedError, match="d shells"):
        gto.gradient_batch(basis, E.angstrom_of("Lds")[None])
    with pytest.raises(NotImplementedError, match="d shells"):
        gto.gradient_sets_batch(basis, E.angstrom_of("Lds")[None], dm1=torch.zeros((1, 6, basis.nao, basis.nao)))


def test_a_table_of_129_shells_is_refused_before_any_launch():
    lib = _lib.load()
    S = torch.zeros((1, 4, 4), dtype=F64, device=dev())
    rc = lib.oovqe_gto_integrals_batch(129, None, 129, None, None, 1, None, 1, None, 129, _lib.dptr(S), None, None, None,
                                       None, _lib.stream_ptr())
    assert rc < 0 and b"nshell" in lib.oovqe_last_error()
    torch.cuda.synchronize()
    assert torch.equal(S, torch.zeros_like(S))
