"""The orbital-rotation kernels (csrc/expm.hip: ``oovqe_expm``, ``oovqe_expm_skew``, ``oovqe_rotate_orbitals_batch``) and
the line-search kernels (csrc/linesearch.hip: ``oovqe_linesearch_points``, ``oovqe_linesearch_update``) over their whole
scope.  tests/_rotation_scope.py has the cases, the host twins and the references and says where they come from;
tests/test_rotation_scope_cpu.py holds the references against each other, prints the bound of every case used here and
holds it under a cap.

Bounds (nothing in one comes from the device's output):
  * exponential, per case: 10 x max |expm_twin(X, float64) - expm_ref(X)|, the float64 twin of the kernel's algorithm
    against the longdouble reference (a closed form at N = 257 and in the one-column cases); the factor 10 allows for
    the MFMA's order of summation.  ``want_K`` is the scattered matrix exactly, ``n_kappa = 0`` the identity exactly.
  * Frechet helpers: the same rule for the matrix a helper hands to ``ops.expm`` (caught on its way in); the helper's
    result is held to 10 x ``FRECHET_THRESHOLD`` of the largest element of the wanted block, the threshold being the
    host figure of tests/test_rotation_scope_cpu.py.
  * rotated orbitals C expm(-K): the bound of expm(-K) plus 10 x N 2^-53 max |C| N for the product.
  * line search: points, t, active, best and flags bit for bit as the twin.  The points are exact by construction (t a
    multiple of 2^-10 below 2, flat and dp multiples of 2^-20 below 2^10: the product has 41 bits, the sum 42, so fused
    and unfused agree); the thresholds energy + t slope are rounded once (dyadic energies, slopes -2^k), so a trial ON the
    threshold passes and the next float above it does not.  Generic points: 2 ulp of max(|flat|, |t dp|).  Slope:
    10 x n 2^-53 alpha sum |g_i dp_i| against the exact sum.
  * non-finite input (pinned, not specified anywhere): N <= 48 returns with every element NaN for a NaN, some element
    non-finite for an Inf; beyond 48 both are refused.

Defects.  (1) ``oovqe_linesearch_points`` refused n_a = 0 without points_b, against include/oovqe.h
(``test_points_*`` with n_a = 0).  (2) The block matrices of the Frechet helpers were handed over unbalanced
(tests/test_rotation_scope_cpu.py).  (3) Found by these tests' preparation, by reading: beyond N = 48 a NaN never reached
the host's test for a non-finite input, because ``norm1_kernel`` took its maximum with ``fmax``, which drops a NaN: the
column with the NaN was left out of the norm and the call returned a matrix of NaN without an error (a matrix of NaN
only: norm 0).  ``norm1_kernel`` now keeps a NaN (``test_non_finite_input_beyond_48_is_refused``).

Measured on an MI355X (one run; nothing below was used to set a bound).  Largest deviation / bound per group, with s and
the degree of the extreme case:
  expm, both signs, N = 1 .. 129                       0.12   N = 17, norm 40, sign -  (s = 7, degree 16); 0.10 .. 0.12 at
                                                             every size, i.e. the device's error is the twin's own;
                                                             norm 1e6 (s = 21): deviation 1.4e-11 .. 3.5e-11
  expm of a number                                     0.10   exp(0.05)  (s = 0, degree 8)
  expm_skew, three pair tables, N = 2 .. 129           0.16   N = 4, non-redundant, norm 1e3  (s = 11, degree 16)
  norm in one column, N = 65, 129, 257                 0.10   (s = 7, degree 16)
  closed form at N = 257                               0.10   largest angle 0.2  (s = 0, degree 12)
  block matrices 2N, 3N as they come                   0.10   3N, N = 17, K 3, blocks 100: 8.6e-9 of 8.6e-8 (s = 12,
                                                             degree 12) is the largest deviation in absolute terms
  matrices handed over by the Frechet helpers          0.10   K 1e-4, blocks 1  (s = 0, degree 8); s <= 4 throughout
  block returned by the helpers / 10 x threshold       0.02   2N, K 1e-4, blocks 100
  kappa_gradient                                       0.10   the matrix handed over, K 0.05  (s = 0, degree 12)
  rotated orbitals, N = 5 .. 48, batch 1, 3, 70        0.14   N = 5, batch 70, element 21, kappa norm 1e3, C U  (s = 11)
  rotated orbitals, N = 49, 64, batch 2                0.10   kappa norm 1e3, U  (s = 11, degree 16)
  points, generic data                                 1.00 ulp (bound 2); slope: at most 2.2e-4 of its bound
  points on dyadic data, t, active, best, flags        bit for bit
Slowest cases 1.1 s (``test_expm_skew_over_three_pair_tables[129]`` and ``test_expm_of_both_signs_over_the_norm_list[129]``:
the longdouble references), the file 10.5 s.

Mutation check (scratch copies of the kernels, one edit each, this file against each library; all nine red):
  * the parent commit's library: ``test_points_on_dyadic_data_bit_for_bit`` (all 15), ``test_points_on_generic_data
    _within_two_ulp[1-3]`` and ``test_points_refusals`` (n_a = 0 refused), ``test_non_finite_input_beyond_48_is_refused``
    (all 3: "DID NOT RAISE").
  * ``ksteps = N / 4`` in ``expm_small_kernel``: red in the expm and expm_skew tests at N = 2, 3, 5, 15, 17, 31, 33, 47
    (every N that is no multiple of 4), ``test_expm_of_a_number``, the rotation tests at N = 5 and 33 and the
    non-finite test at N = 1.
  * the remainder loop of ``norm1_partial_kernel`` removed: red in ``test_norm_in_one_column`` at 65, 129 and 257 (the
    heavy element in the last row), in the expm test at N = 49 (norm 1e3: 4e-12 against 1.6e-13) and the non-finite test
    at 49.  Dense matrices at the other sizes stay green: the lost rows cost two or three squarings, and degree 16 has
    that much room when the 2-norm of a dense matrix is a third of its 1-norm; the last-row case was added for this.
  * ``norm1_kernel`` reading only its first 256 columns: red in ``test_norm_in_one_column[257]`` and the non-finite test
    at 257.
  * ``THETA12`` where ``THETA8`` belongs: red in the expm and expm_skew tests at N = 2, 3, 4, 5, 17, 48 (norm 0.2 and the
    thresholds 0.06 .. 0.3: degree 8 leaves 5e-11), ``test_expm_of_a_number``, ``test_closed_form_at_257`` and the
    rotation test at N = 5, batch 3 and 70 (at N = 17 and 48 through the threshold cases: dense matrices of N >= 15 at
    norm 0.2 stay green for the reason above).
  * one pass in place of the batch stride of ``linesearch_update_kernel``: red in the scripted search at batch 257 and
    1000 (both layouts of ``trial``), in the deciding-problem test at (257, 256) and every index of 1000, and in
    ``test_run_search_with_scripted_energies[257-some-give-up]``.
  * ``act = tr > e0 + tb * sl``: red in the scripted search at batch 255 .. 1000, in every deciding-problem case and in
    the run_search test of 257 (batch 1 of the scripted search has no NaN trial: its one problem accepts at once).
  * ``flags[3]`` for resting problems as well: red in all six deciding-problem cases.
  * one pass in place of the stride over n in ``linesearch_points_kernel``: red in both points tests at n = 257 and 600.
"""
import ctypes
import functools
import math
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from auto_oo_amd import _lib, newton_raphson, oo_energy, ops        # noqa: E402
from auto_oo_amd._lib import OovqeError, check, dptr, stream_ptr    # noqa: E402
from tests import _rotation_scope as V                              # noqa: E402

F64 = torch.float64
LD = V.LD
NAN = float("nan")


def dev():
    return torch.device("cuda", 0)


def cuda(x, dtype=np.float64):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=dtype))).to(dev())


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    """Bit equality of two float64 arrays, NaN equal to NaN (and -0.0 different from 0.0)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(nan_a, nan_b) and \
        np.array_equal(a[~nan_a].view(np.int64), b[~nan_b].view(np.int64))


def same_values(a, b):
    """Equality of two arrays as numbers (0.0 == -0.0: the scatter's "undo" of the sign leaves -0.0 in K)."""
    return a.shape == b.shape and np.array_equal(a, b)


class Worst:
    """The largest deviation / bound of a group, with the case it came from."""

    def __init__(self, group):
        self.group, self.ratio, self.where = group, 0.0, "-"

    def hold(self, label, got, ref, bound, s=None, deg=None):
        d = float(np.abs(np.asarray(got, dtype=LD) - ref).max())
        tag = f"{label} (s = {s}, degree {deg})" if s is not None else label
        print(f"{self.group}: {tag}: deviation {d:.2e}, bound {bound:.2e}")
        assert np.isfinite(np.asarray(got)).all(), tag
        assert d <= bound, f"{tag}: {d:.3e} > {bound:.3e}"
        if bound > 0 and d / bound > self.ratio:
            self.ratio, self.where = d / bound, tag

    def report(self):
        print(f"{self.group}: largest deviation / bound {self.ratio:.2f} at {self.where}")


# ---- 1. ops.expm / ops.expm_skew ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", V.SMALL_SIZES + V.LARGE_SIZES)
def test_expm_of_both_signs_over_the_norm_list(n):
    w = Worst(f"expm N = {n}")
    for label, X in V.expm_cases(n):
        Xd = cuda(X)
        bound, s, deg, _, ref = V.expm_bound(X)
        w.hold(label + " +", host(ops.expm(Xd, 1.0)), ref, bound, s, deg)
        # (X is skew: exp(-X) is the transpose; the twin runs on -X itself)
        bound_m, s, deg, _, _ = V.expm_bound(-X, ref.T)
        w.hold(label + " -", host(ops.expm(Xd, -1.0)), ref.T, bound_m, s, deg)
    w.report()


def test_expm_of_a_number():
    w = Worst("expm N = 1")
    for a in V.SCALARS:
        X = np.array([[a]])
        tw, s, deg = V.expm_twin(X)
        ref = np.exp(LD(a)).reshape(1, 1)
        w.hold(f"exp({a:g})", host(ops.expm(cuda(X), 1.0)), ref, 10.0 * float(abs(LD(tw[0, 0]) - ref[0, 0])), s, deg)
    w.report()


def raw_expm_skew(n, kappa, rows, cols, n_kappa, want_K):
    """``oovqe_expm_skew`` with an explicit n_kappa (``ops.expm_skew`` cannot say 0: the library wants pointers)."""
    U = torch.full((n, n), NAN, dtype=F64, device=dev())
    K = torch.full((n, n), NAN, dtype=F64, device=dev()) if want_K else None
    work = torch.empty(7 * n * n, dtype=F64, device=dev()) if n > 48 else None
    check(_lib.load().oovqe_expm_skew(dptr(kappa), dptr(rows, torch.int32), dptr(cols, torch.int32), n_kappa, n, dptr(K),
                                      dptr(U), dptr(work), stream_ptr()), "oovqe_expm_skew")
    return U, K


SKEW_NORMS = {n: (0.0, 1e-8, 0.2, 3.0, 1e3) for n in V.SMALL_SIZES}
SKEW_NORMS.update({n: (0.2, 1e3) for n in V.LARGE_SIZES})


@pytest.mark.parametrize("n", V.SMALL_SIZES[1:] + V.LARGE_SIZES)
def test_expm_skew_over_three_pair_tables(n):
    w = Worst(f"expm_skew N = {n}")
    for which in ("nonredundant", "full", "last"):
        rows, cols = V.pair_tables(n, which)
        rd, cd = cuda(rows, np.int32), cuda(cols, np.int32)
        for i, x in enumerate(SKEW_NORMS[n]):
            kappa = V.kappa_of_norm(n, rows, cols, x, 31 * n + i)
            K = V.scatter(n, rows, cols, kappa)
            bound, s, deg, _, ref = V.expm_bound(-K)
            U, Kd = ops.expm_skew(cuda(kappa), rd, cd, n, want_K=True)
            assert same_values(host(Kd), K), f"{which} norm {x:g}: K is not the scattered matrix"
            w.hold(f"{which} norm {x:g}", host(U), ref, bound, s, deg)
            U2 = ops.expm_skew(cuda(kappa), rd, cd, n)
            assert same_bits(host(U2), host(U))              # (with and without K: the same U)
    w.report()


@pytest.mark.parametrize("n", V.SMALL_SIZES + V.LARGE_SIZES)
def test_no_kappa_gives_the_identity_exactly(n):
    one = torch.full((1,), 5.0, dtype=F64, device=dev())
    idx = torch.zeros(1, dtype=torch.int32, device=dev())
    for want_K in (True, False):
        U, K = raw_expm_skew(n, one, idx, idx, 0, want_K)
        assert same_values(host(U), np.eye(n))
        assert K is None or same_values(host(K), np.zeros((n, n)))


# ---- 2. the large route: the norm in one column, the second pass of norm1_kernel ------------------------------------------
@pytest.mark.parametrize("n", [65, 129, 257])
def test_norm_in_one_column(n):
    w = Worst(f"one column N = {n}")
    for label, K, U in V.one_column_cases(n):
        tw, s, deg = V.expm_twin(K)
        w.hold(label, host(ops.expm(cuda(K), 1.0)), U, 10.0 * float(np.abs(tw.astype(LD) - U).max()), s, deg)
    w.report()


def test_closed_form_at_257():
    n = 257
    w = Worst("closed form N = 257")
    rng = np.random.default_rng(257)
    for top in (0.0, 0.2, 3.0, 40.0, 1e3):
        angles = list(rng.uniform(-1.0, 1.0, n // 2) * top)
        angles[-1] = top                                     # (the seeded permutation decides where it sits)
        K, U = V.planar(n, angles, seed=int(top * 10) + 1)
        tw, s, deg = V.expm_twin(K)
        w.hold(f"largest angle {top:g}", host(ops.expm(cuda(K), 1.0)), U,
               10.0 * float(np.abs(tw.astype(LD) - U).max()), s, deg)
    rows, cols = V.pair_tables(n, "last")
    kappa = np.zeros(n - 1)
    kappa[0] = 40.0                                          # the plane (256, 0): K[256, 0] = 40
    K, U = V.planar(n, [(0, n - 1, 40.0)])
    assert same_values(K, V.scatter(n, rows, cols, kappa))
    tw, s, deg = V.expm_twin(-K)
    Ud, Kd = ops.expm_skew(cuda(kappa), cuda(rows, np.int32), cuda(cols, np.int32), n, want_K=True)
    assert same_values(host(Kd), K)
    w.hold("expm_skew, angle 40 in columns 0, 256", host(Ud), U.T, 10.0 * float(np.abs(tw.astype(LD) - U.T).max()), s, deg)
    w.report()


# ---- 3. non-normal input ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,n", V.BLOCK_SHAPES)
def test_block_triangular_matrices(nb, n):
    w = Worst(f"{nb}N blocks N = {n}")
    for ks in V.K_SCALES:
        for mag in V.OFF_MAGNITUDES:
            K, offs = V.block_parts(nb, n, ks, mag)
            M = V.block_matrix(K, offs)
            bound, s, deg, _, ref = V.expm_bound(M)
            w.hold(f"K {ks:g}, blocks {mag:g}", host(ops.expm(cuda(M), 1.0)), ref, bound, s, deg)
    w.report()


def device_rule(n, monkeypatch, record):
    """``_OrbitalRotationRule`` of a stand-in for an ``OO_energy`` of n orbitals; every matrix handed to ``ops.expm`` and
    what came back are appended to ``record``."""
    real = ops.expm

    def expm(X, sign=1.0):
        out = real(X, sign)
        record.append((sign * host(X), host(out)))
        return out

    monkeypatch.setattr(ops, "expm", expm)
    rows, cols = V.pair_tables(n, "nonredundant")
    oo = types.SimpleNamespace(nao=n, device=dev(), _kap_row=cuda(rows, np.int32), _kap_col=cuda(cols, np.int32))
    return oo_energy._OrbitalRotationRule(oo)


@pytest.mark.parametrize("nb,n", V.BLOCK_SHAPES)
def test_frechet_helpers(nb, n, monkeypatch):
    record = []
    rule = device_rule(n, monkeypatch, record)
    w, w_block = Worst(f"handed by the {nb}N helper, N = {n}"), Worst(f"block of the {nb}N helper, N = {n}")
    for ks in V.K_SCALES:
        for mag in V.OFF_MAGNITUDES:
            K, offs = V.block_parts(nb, n, ks, mag)
            orders = [offs] if nb == 2 else [offs, offs[::-1]]
            want = sum(V.expm_ref(V.block_matrix(K, o))[:n, (nb - 1) * n:] for o in orders)
            del record[:]
            od = [cuda(a) for a in offs]
            got = rule._frechet(cuda(K), od[0]) if nb == 2 else rule._frechet2(cuda(K), od[0], od[1])
            assert len(record) == len(orders)
            for handed, out in record:
                bound, s, deg, _, ref = V.expm_bound(handed)
                w.hold(f"K {ks:g}, blocks {mag:g}", out, ref, bound, s, deg)
            w_block.hold(f"K {ks:g}, blocks {mag:g}", host(got), want,
                         10.0 * V.FRECHET_THRESHOLD * float(np.abs(want).max()))
    w.report()
    w_block.report()


@pytest.mark.parametrize("n", [24, 25])
def test_kappa_gradient(n, monkeypatch):
    record = []
    rule = device_rule(n, monkeypatch, record)
    w = Worst(f"kappa_gradient N = {n}")
    rng = np.random.default_rng(700 + n)
    rows, cols = V.pair_tables(n, "nonredundant")
    for ks in (0.05, 0.5, 3.0):
        kappa = V.kappa_of_norm(n, rows, cols, ks, n + int(10 * ks))
        K = V.scatter(n, rows, cols, kappa)
        U = np.asarray(V.expm_ref(-K), dtype=np.float64)
        fock = rng.uniform(-50.0, 50.0, (n, n))
        del record[:]
        g = host(rule.kappa_gradient(cuda(fock), None, cuda(U), cuda(K)))
        (handed, out), = record
        bound, s, deg, _, ref = V.expm_bound(handed)
        w.hold(f"K {ks:g}: handed", out, ref, bound, s, deg)
        assert V.norm1(handed) <= 2.0 * max(V.norm1(K), oo_energy._BALANCE_FLOOR)      # balanced
        Xm = np.asarray(U, dtype=LD) @ (2.0 * fock.T)
        blockK = np.asarray(V.expm_ref(V.block_matrix(K, [np.asarray(Xm, dtype=np.float64)])), dtype=LD)[:n, n:]
        want = -(blockK[rows, cols] - blockK[cols, rows])
        top = float(np.abs(blockK).max())
        # two elements of the block, and the product U (2 F^T) formed on the device in front of it
        w.hold(f"K {ks:g}: gradient", g, want, 2 * 10.0 * V.FRECHET_THRESHOLD * top + 10.0 * n * V.EPS * 100.0 * n)
    w.report()


# ---- 4. oovqe_rotate_orbitals_batch -------------------------------------------------------------------------------------------
def raw_rotate(n, kappas, rows, cols, C, out, want_U, work="auto"):
    batch, n_kappa = kappas.shape
    U = torch.full((batch, n, n), NAN, dtype=F64, device=dev()) if want_U else None
    if isinstance(work, str):
        work = torch.empty((batch + 7) * n * n, dtype=F64, device=dev()) if n > 48 else None
    check(_lib.load().oovqe_rotate_orbitals_batch(dptr(kappas), dptr(rows, torch.int32), dptr(cols, torch.int32), n_kappa,
                                                  n, batch, dptr(C), dptr(out), dptr(U), dptr(work), stream_ptr()),
          "oovqe_rotate_orbitals_batch")
    return U


@functools.lru_cache(maxsize=None)
def rotation_set(n):
    """The five kappas of ``MIXED_NORMS`` with the reference of each, and seven orbital matrices."""
    rows, cols = V.pair_tables(n, "nonredundant")
    kappas = [V.kappa_of_norm(n, rows, cols, x, 60 * n + i) for i, x in enumerate(V.MIXED_NORMS)]
    Cs = [V.orbitals(n, 10 * n + j) for j in range(7)]
    refs = [V.rotation_reference(n, rows, cols, k, Cs[0])[1:] for k in kappas]      # (U, b_c, b_u, s, deg)
    return rows, cols, kappas, Cs, refs


def check_rotation(n, batch, w):
    rows, cols, kappas, Cs, refs = rotation_set(n)
    pick = [(b + 3) % 5 for b in range(batch)]              # (a batch of one gets the norm 3, of three 3, 1e3 and 0)
    kap = np.stack([kappas[i] for i in pick])
    C = np.stack([Cs[b % 7] for b in range(batch)])
    kd, rd, cd, Cd = cuda(kap), cuda(rows, np.int32), cuda(cols, np.int32), cuda(C)
    want = [np.asarray(C[b], dtype=LD) @ refs[pick[b]][0] for b in range(batch)]
    modes = [("U", True, False), ("no U", False, False)]
    modes += [("C_out = C", True, True)] if n <= 48 else []
    for name, want_U, alias in modes:
        Cin = Cd.clone()
        out = Cin if alias else torch.full_like(Cd, NAN)
        U = raw_rotate(n, kd, rd, cd, Cin, out, want_U)
        assert alias or torch.equal(Cin, Cd)
        for b in range(batch):
            Uref, _, b_u, s, deg = refs[pick[b]]
            b_c = b_u + 10.0 * n * V.EPS * float(np.abs(C[b]).max()) * n
            label = f"batch {batch}, {name}, element {b} (kappa norm {V.MIXED_NORMS[pick[b]]:g})"
            w.hold(label + ": C U", host(out[b]), want[b], b_c, s, deg)
            if want_U:
                w.hold(label + ": U", host(U[b]), Uref, b_u, s, deg)


@pytest.mark.parametrize("batch", [1, 3, 70])
@pytest.mark.parametrize("n", [5, 16, 33, 48])
def test_rotate_orbitals_batch_in_lds(n, batch):
    w = Worst(f"rotate N = {n} batch {batch}")
    check_rotation(n, batch, w)
    w.report()


@pytest.mark.parametrize("n", [49, 64])
def test_rotate_orbitals_batch_beyond_48(n):
    w = Worst(f"rotate N = {n} batch 2")
    check_rotation(n, 2, w)                                  # (without U the rotation matrices live in ``work``)
    w.report()


def test_rotate_orbitals_batch_refusals_at_49():
    n = 49
    rows, cols, kappas, Cs, _ = rotation_set(n)
    kd, rd, cd = cuda(np.stack(kappas[:2])), cuda(rows, np.int32), cuda(cols, np.int32)
    C = cuda(np.stack(Cs[:2]))
    before = C.clone()
    with pytest.raises(OovqeError, match="alias"):
        raw_rotate(n, kd, rd, cd, C, C, False)
    with pytest.raises(OovqeError, match="work"):
        raw_rotate(n, kd, rd, cd, C, torch.empty_like(C), False, work=None)
    torch.cuda.synchronize()
    assert torch.equal(C, before)


# ---- 5. non-finite input (what the code does today) ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 17, 48])
def test_non_finite_input_up_to_48_comes_back_non_finite(n):
    for value in (NAN, float("inf")):
        X = V.skew(n, 0.2, n) if n > 1 else np.zeros((1, 1))
        X[n // 2, 0] = value
        U = host(ops.expm(cuda(X), 1.0))                     # (returns: the s < 60 cap bounds the squarings)
        if value != value:
            assert np.isnan(U).all()
        else:
            assert not np.isfinite(U).all()


@pytest.mark.parametrize("n", [49, 64, 257])
def test_non_finite_input_beyond_48_is_refused(n):
    """A NaN alone in its column, a NaN in the last column, a matrix of NaN, and an Inf."""
    rows, cols = V.pair_tables(n, "full")
    for value, where in ((NAN, (n // 2, 0)), (NAN, (0, n - 1)), (NAN, None), (float("inf"), (n // 2, 0))):
        X = V.skew(n, 0.2, n)
        if where is None:
            X[:] = value
        else:
            X[where] = value
        with pytest.raises(OovqeError, match="non-finite"):
            ops.expm(cuda(X), 1.0)
    kappa = np.full(len(rows), 0.01)
    kappa[len(rows) // 2] = NAN
    with pytest.raises(OovqeError, match="non-finite"):
        ops.expm_skew(cuda(kappa), cuda(rows, np.int32), cuda(cols, np.int32), n)
    with pytest.raises(OovqeError, match="non-finite"):      # (a refused Newton direction: every element NaN)
        ops.expm_skew(cuda(np.full(len(rows), NAN)), cuda(rows, np.int32), cuda(cols, np.int32), n)


# ---- 6. oovqe_linesearch_points ------------------------------------------------------------------------------------------------
GUARD = 8


def guarded(count):
    """``count`` doubles of NaN between two guard bands of NaN."""
    buf = torch.full((count + 2 * GUARD,), NAN, dtype=F64, device=dev())
    return buf, buf[GUARD:GUARD + count]


def raw_points(flat, dp, t, grad, alpha, n, n_a, batch, with_pb, with_slope):
    n_first = n if n_a == 0 else n_a
    buf_a, pa = guarded(batch * n_first)
    buf_b, pb = guarded(batch * (n - n_first)) if with_pb else (None, None)
    buf_s, slope = guarded(batch) if with_slope else (None, None)
    check(_lib.load().oovqe_linesearch_points(dptr(flat), dptr(dp), dptr(t), dptr(grad), float(alpha), n, n_a, batch,
                                              dptr(pa), dptr(pb), dptr(slope), stream_ptr()), "oovqe_linesearch_points")
    for buf, count in ((buf_a, batch * n_first), (buf_b, batch * (n - n_first)), (buf_s, batch)):
        if buf is not None:
            b = host(buf)
            assert np.isnan(b[:GUARD]).all() and np.isnan(b[GUARD + count:]).all(), "a store outside the output"
    return (host(pa).reshape(batch, n_first), host(pb).reshape(batch, n - n_first) if with_pb else None,
            host(slope) if with_slope else None)


def splits(n):
    """(n_a, points_b given): no split both ways the header allows, and the two extreme splits."""
    out = [(n, False), (0, False), (n, True), (0, True)]
    return out + ([(1, True), (n - 1, True)] if n > 1 else [])


@pytest.mark.parametrize("batch", [1, 3, 300])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 600])
def test_points_on_dyadic_data_bit_for_bit(n, batch):
    rng = np.random.default_rng(1000 * n + batch)
    flat, dp, grad = V.dyadic(rng, (batch, n)), V.dyadic(rng, (batch, n)), rng.standard_normal((batch, n))
    t = V.dyadic(rng, batch, 10, 2.0)
    t[batch // 2] = 0.0
    alpha = 1e-4
    fd, dd, td, gd = cuda(flat), cuda(dp), cuda(t), cuda(grad)
    exact = [math.fsum(float(g) * float(d) for g, d in zip(grad[b], dp[b])) for b in range(batch)]      # to 2^-53 each
    limit = [10.0 * n * V.EPS * alpha * float(np.abs(grad[b] * dp[b]).sum()) for b in range(batch)]
    worst = 0.0
    for n_a, with_pb in splits(n):
        twin = [V.ls_points_twin(flat[b], dp[b], t[b], n_a) for b in range(batch)]
        for with_slope in (True, False):
            pa, pb, slope = raw_points(fd, dd, td, gd if with_slope else None, alpha, n, n_a, batch, with_pb, with_slope)
            assert same_bits(pa, np.array([tw[0] for tw in twin]).reshape(pa.shape)), (n_a, with_pb, with_slope)
            if with_pb and pa.shape[1] < n:
                assert same_bits(pb, np.array([tw[1] for tw in twin]).reshape(pb.shape)), (n_a, with_slope)
            elif with_pb:
                assert pb.size == 0
            if with_slope:
                for b in range(batch):
                    d = abs(slope[b] - alpha * exact[b])
                    assert d <= limit[b], (b, d, limit[b])
                    worst = max(worst, d / limit[b] if limit[b] > 0 else 0.0)
    print(f"points n = {n} batch {batch}: slope, largest deviation / bound {worst:.1e}")


@pytest.mark.parametrize("n,batch", [(1, 3), (257, 3), (600, 300)])
def test_points_on_generic_data_within_two_ulp(n, batch):
    rng = np.random.default_rng(n + batch)
    flat, dp = rng.standard_normal((batch, n)) * 10.0 ** rng.uniform(-3, 3, (batch, n)), rng.standard_normal((batch, n))
    t = 0.3 ** rng.integers(0, 8, batch)
    pa, pb, _ = raw_points(cuda(flat), cuda(dp), cuda(t), None, 1e-4, n, max(n // 3, 1) if n > 1 else 0, batch, n > 1, False)
    got = np.concatenate([pa, pb], axis=1) if pb is not None else pa
    td = t[:, None].astype(LD) * dp.astype(LD)
    ulp = np.spacing(np.maximum(np.abs(flat), np.abs(td).astype(np.float64)))
    ratio = float((np.abs(got.astype(LD) - (td + flat.astype(LD))) / ulp).max())
    print(f"points n = {n} batch {batch}: generic data, largest deviation {ratio:.2f} ulp")
    assert ratio <= 2.0


def test_points_refusals():
    lib = _lib.load()
    z = torch.zeros(8, dtype=F64, device=dev())
    p = dptr(z)
    assert lib.oovqe_linesearch_points(p, p, p, None, 1e-4, 4, 2, 1, p, None, None, stream_ptr()) != 0     # a split needs b
    assert lib.oovqe_linesearch_points(p, p, p, None, 1e-4, 4, 5, 1, p, p, None, stream_ptr()) != 0        # n_a > n
    assert lib.oovqe_linesearch_points(p, p, p, None, 1e-4, 4, 4, 1, p, None, p, stream_ptr()) != 0        # slope, no grad
    assert lib.oovqe_linesearch_points(p, p, p, None, 1e-4, 4, 0, 1, p, None, None, stream_ptr()) == 0     # the header's n_a = 0
    torch.cuda.synchronize()


# ---- 7. oovqe_linesearch_update ------------------------------------------------------------------------------------------------
class DeviceSearch:
    """t, active, best and flags of ``batch`` problems on the device, with stale contents."""

    def __init__(self, energy, slope, t=None, active=None, best=None):
        self.batch = len(energy)
        self.energy, self.slope = cuda(energy), cuda(slope)
        self.t = cuda(t if t is not None else [1.0] * self.batch)
        self.active = cuda(active if active is not None else [0.0] * self.batch)     # (stale: "nobody is searching")
        self.best = cuda(best if best is not None else [-5.0] * self.batch)
        self.flags = torch.full((4,), NAN, dtype=F64, device=dev())

    def update(self, trial, info, beta, first, give_up, strided=False):
        ptr, stride = None, 1
        if trial is not None and strided:
            packed = torch.full((self.batch, 7), -3e9, dtype=F64, device=dev())      # (-3e9 would pass everywhere)
            packed[:, 1] = cuda(trial)
            ptr, stride = ctypes.c_void_p(packed[:, 1].data_ptr()), packed.stride(0)
        elif trial is not None:
            keep = cuda(trial)
            ptr = dptr(keep)
        check(_lib.load().oovqe_linesearch_update(ptr, stride, dptr(self.energy), dptr(self.slope),
                                                  dptr(cuda(info)) if info is not None else None, float(beta), int(first),
                                                  int(give_up), self.batch, dptr(self.t), dptr(self.active),
                                                  dptr(self.best), dptr(self.flags), stream_ptr()),
              "oovqe_linesearch_update")
        return host(self.t), host(self.active), host(self.best), host(self.flags)

    def agrees(self, state, what):
        t, active, best, flags = state
        for name, got, ref in (("t", self.t, t), ("active", self.active, active), ("best", self.best, best),
                               ("flags", self.flags, flags)):
            assert same_bits(host(got), np.array(ref)), f"{what}: {name}"


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "stride7"])
@pytest.mark.parametrize("batch", V.UPDATE_BATCHES)
def test_update_through_a_scripted_search(batch, strided):
    S = V.scripted_search(batch)
    D = DeviceSearch(S["energy"], S["slope"])
    for r in range(V.ROUNDS):
        D.update(S["trials"][r], None, 0.3, r == 0, 0, strided)
        D.agrees(S["states"][r], f"round {r}")
    D.update(None, None, 0.3, 0, 1)
    D.agrees(S["states"][V.ROUNDS], "give-up")
    t, best = host(D.t), host(D.best)
    for b in range(batch):                                   # (what the script is for, said once more without the twin)
        if b % 7 == 6:
            assert t[b] == 0.0 and best[b] == S["energy"][b]
        else:
            assert best[b] == S["trials"][b % 7][b] and t[b] > 0.0


@pytest.mark.parametrize("batch,idx", [(1, 0), (257, 256), (1000, 0), (1000, 255), (1000, 256), (1000, 999)])
def test_update_flags_follow_one_deciding_problem(batch, idx):
    rng = np.random.default_rng(batch + idx)
    energy = V.dyadic(rng, batch, 12, 2.0 ** 8).tolist()
    base_slope = [-0.5] * batch
    passing = [e - 1.0 for e in energy]                      # energy + t slope = energy - 0.5 at t = 1

    def run(what, slope, trial, info, first, active):
        t, act, best = [1.0] * batch, list(active), [-5.0] * batch
        D = DeviceSearch(energy, slope, t, act, best)
        D.update(trial, info, 0.5, first, 0)
        flags = V.ls_update_twin(trial, energy, slope, info, 0.5, first, 0, t, act, best)
        D.agrees((t, act, best, flags), what)
        return flags

    everyone = [1.0] * batch
    assert run("all pass", base_slope, passing, None, 1, everyone) == [0.0, 0.0, 0.0, 0.0]
    trial = list(passing)
    trial[idx] = energy[idx]                                 # above the threshold: this problem alone goes on
    assert run("one goes on", base_slope, trial, None, 1, everyone) == [1.0, 0.0, 0.0, 0.0]
    trial[idx] = NAN
    assert run("a NaN trial", base_slope, trial, None, 1, everyone) == [1.0, 0.0, 0.0, 0.0]
    info = [1.0] * batch
    info[idx] = -2.0
    assert run("info", base_slope, passing, info, 1, everyone) == [0.0, -2.0, 0.0, 0.0]
    info = [float(b % 3) for b in range(batch)]
    info[batch - 1] = -3.0                                   # a negative entry in the last problem
    assert run("info, last", base_slope, passing, info, 1, everyone)[1] == -3.0
    slope = list(base_slope)
    slope[idx] = NAN
    assert run("NaN slope, searching", slope, passing, None, 1, everyone) == [1.0, 0.0, 1.0, 1.0]
    resting = list(everyone)
    resting[idx] = 0.0
    assert run("NaN slope, resting", slope, passing, None, 0, resting) == [0.0, 0.0, 1.0, 0.0]
    for up in (0.0, 0.25):
        slope[idx] = up
        trial = list(passing)
        trial[idx] = energy[idx] + 1.0
        assert run("slope not negative, searching", slope, trial, None, 1, everyone) == [1.0, 0.0, 0.0, 1.0]
        assert run("slope not negative, resting", slope, trial, None, 0, resting) == [0.0, 0.0, 0.0, 0.0]
        assert run("slope not negative, passes now", slope, passing, None, 1, everyone) == [0.0, 0.0, 0.0, 0.0]
    stale = [0.0] * batch
    assert run("first = 1 over a stale active", base_slope, trial, None, 1, stale) == [1.0, 0.0, 0.0, 0.0]
    assert run("first = 0 reads active", base_slope, trial, None, 0, stale) == [0.0, 0.0, 0.0, 0.0]


# ---- 8. BatchedNewtonStep.run_search end to end ------------------------------------------------------------------------------
@pytest.mark.parametrize("G,period", [(257, 8), (5, 8)], ids=["257-some-give-up", "5-all-accept"])
def test_run_search_with_scripted_energies(G, period):
    """Problem b accepts its (b mod period)-th trial; lmax + 1 = 6 trials are made, so b mod 8 = 6, 7 give up.  alpha is
    2^-13, the gradient -e_0 and dp has powers of two, so the slope alpha <g, dp> is the script's -2^k exactly and
    flat + t dp is exact for every t = 0.3^j."""
    lmax, alpha, beta, n = 5, 2.0 ** -13, 0.3, 3
    S = V.scripted_search(G, beta=beta, seed=3, period=period, rounds=lmax + 1)
    rng = np.random.default_rng(G)
    flat = V.dyadic(rng, (G, n))
    grad = np.tile(np.array([-1.0, 0.0, 0.0]), (G, 1))
    dp = np.stack([-np.array(S["slope"]) / alpha, np.full(G, 0.125), np.full(G, -4.0)], axis=1)
    table = cuda(np.array(S["trials"]))
    kw = dict(dtype=F64, device=dev())
    state = torch.full((3, G), NAN, **kw)
    s = newton_raphson.LockstepSearch(flat=cuda(flat), g=cuda(grad), H=None, dp=cuda(dp), low=None, nu=None, info=None,
                                      energy=cuda(S["energy"]), t=torch.ones(G, **kw), active=state[0], best=state[1],
                                      slope=state[2], flags=torch.full((4,), NAN, **kw), pa=torch.full((G, n), NAN, **kw),
                                      pb=None)
    seen = []

    def objective(points):
        seen.append(host(points).copy())
        return table[len(seen) - 1]

    step = newton_raphson.BatchedNewtonStep(alpha=alpha, beta=beta, lmax=lmax, verbose=0)
    step.run_search(s, objective)
    assert same_bits(host(s.slope), np.array(S["slope"]))
    t_before = [[1.0] * G] + [st[0] for st in S["states"][:-2]]
    never = [b for b in range(G) if b % period > lmax]
    assert len(seen) == (lmax + 1 if never else min(G, lmax + 1))
    for k, pts in enumerate(seen):                           # the points of every trial
        assert same_bits(pts, flat + np.array(t_before[k])[:, None] * dp), f"trial {k}"
    t_end, _, best_end, _ = S["states"][-1] if never else S["states"][len(seen) - 1]
    assert same_bits(host(s.t), np.array(t_end))
    assert same_bits(host(s.pa), flat + np.array(t_end)[:, None] * dp)
    assert same_bits(host(s.best), np.array(best_end))
    for b in range(G):
        assert best_end[b] == (S["energy"][b] if b in never else S["trials"][b % period][b])
    assert step.last_search_gave_up == bool(never)
