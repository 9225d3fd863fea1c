"""The contraction kernels (csrc/contract.hip, K1; csrc/contract_pair.hip, K1P) over every build their plan can choose.

Every dense product of the project runs on these kernels, and K1 is 91 template builds (tests/_contract_scope.py has
the table and the references, tests/test_contract_scope_cpu.py holds the table to the planning rule).  Here every
build, and every edge row, runs once on the device:

  * T, Cm and out each live inside a larger buffer of NaN: guard bands in front and behind (even lengths where 16-byte
    alignment is wanted, odd where it is not), NaN in the columns of Cm past J when ldc > J, NaN in the gaps between
    batch elements, NaN in out itself.  After the call every element outside the results is still NaN and no result
    is: nothing was stored past an edge, nothing outside T or Cm was read and multiplied in, not even by a zero.
  * integer inputs (|T|, |Cm| <= 8): the result equals the host product bit for bit, every element.  There is no
    tolerance; whatever order a build sums in, whichever fragments it fuses, the sums are integers below 2^53.
  * an Inf and a NaN planted in slab 1 (INNER) or in row 1 and the last row but one (LAST): every other slab / row
    stays exact, the planted ones are non-finite throughout -- the k-steps that pad K to the chunk depth read nothing
    of a neighbour.
  * real inputs, plain and with the rows of Cm scaled by 2^+-300, against np.longdouble within
    (K + 2) 2^-53 sum_k |Cm[k, j]| |T[a, k, b]| -- the only tolerance in this file, derived in _contract_scope.py.

Measured error / bound of the rounded cases on an MI355X, the largest over the builds visited of each family (nothing
below was used to set the bound):

    family              INNER     LAST        (builds nt = 1, 6, 13; short: 1, 4; normal and 2^+-300-scaled inputs)
    short               0.107     0.285
    deep    (20 rows)   0.107     0.104
    shallow (12 rows)   0.083     0.087
    wide                0.083       -
    pair, 20 rows       0.113       -
    pair, 12 rows       0.092       -

The circuit-hosting launches (contract_circuit_kernel) belong to tests/test_cas_scope_gpu.py."""
import numpy as np
import pytest
import torch

from auto_oo_amd import _lib, ops
from tests import _contract_scope as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
GUARD = 64                       # doubles in front of and behind every tensor (one more in front where it is to be misaligned)


class Placed:
    """A tensor of ``batch`` elements of ``length`` doubles, ``stride`` apart, inside a NaN-filled device buffer."""

    def __init__(self, length, stride, batch, odd, host=None):
        self.length, self.stride, self.batch = length, stride, batch
        self.front = GUARD + (1 if odd else 0)
        self.count = 1 if stride == 0 else batch
        total = self.front + (self.count - 1) * stride + length + GUARD
        if host is None:
            self.buf = torch.full((total,), NAN, dtype=torch.float64, device=DEV)
        else:
            h = np.full(total, NAN)
            for b in range(self.count):
                h[self.front + b * stride:self.front + b * stride + length] = host[b].reshape(-1)
            self.buf = torch.from_numpy(h).to(DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.first = self.buf[self.front:]
        assert (self.first.data_ptr() % 16 == 8) == bool(odd)

    def element(self, b):
        o = self.front + b * self.stride
        return self.buf[o:o + self.length]

    def outside_is_nan(self):
        """every element of the buffer that belongs to no batch element is NaN"""
        rest = self.buf.clone()
        for b in range(self.count):
            o = self.front + b * self.stride
            rest[o:o + self.length] = NAN
        return bool(torch.isnan(rest).all())


def _cm_host(c, Cm):
    """Cm [n, K, J] -> [n, K * ldc] rows of pitch ldc, NaN in the columns past J"""
    wide = np.full((Cm.shape[0], c.K, c.ldc), NAN)
    wide[:, :, :c.J] = Cm
    return wide.reshape(Cm.shape[0], -1)


def _place(c, T, Cm):
    t = Placed(c.A * c.K * c.B, c.t_bs, c.batch, c.t_odd, T.reshape(c.batch, -1))
    cm = Placed(c.K * c.ldc, c.c_bs, c.batch, False, _cm_host(c, Cm))
    out = Placed(c.A * c.J * c.B, c.o_bs, c.batch, c.out_odd)
    return t, cm, out


def _call(c, t, cm, out):
    with _lib.debug_options(**c.opts):
        ops.mode_contract_batch(t.first, cm.first, out.first, c.A, c.K, c.J, c.B, c.ldc, c.last, c.batch,
                                c.t_bs if c.batch > 1 else 0, c.c_bs if c.batch > 1 else 0,
                                c.o_bs if c.batch > 1 else 0)
    torch.cuda.synchronize()


def _bits(x):
    return x.contiguous().view(torch.int64)


def _result(c, out):
    return torch.stack([out.element(b) for b in range(c.batch)]).reshape(c.batch, c.A, c.J, c.B)


def _exact(c, isolation):
    """One case on integer inputs: NaN guards, every element bit for bit; then, with ``isolation``, the planted Inf / NaN"""
    T, Cm = S.integer_inputs(c)
    ref = S.exact_reference(c, T, Cm)
    ref += 0.0                                     # (a host product may return -0; the device's sums begin at +0)
    t, cm, out = _place(c, T, Cm)
    _call(c, t, cm, out)
    got = _result(c, out)
    assert out.outside_is_nan(), f"{c.name}: a store outside the result"
    assert not bool(torch.isnan(got).any()), f"{c.name}: NaN in the result (a guard was read)"
    refd = torch.from_numpy(ref).to(DEV)
    wrong = _bits(got) != _bits(refd)
    assert not bool(wrong.any()), (c.name, int(wrong.sum()), torch.nonzero(wrong)[:4].tolist())
    if not isolation:
        return
    # slab / row 1, and for LAST the last row but one as well: its strip is one the workgroup prefetches under the last
    # chunk of an earlier strip, where row 1's is loaded by the prologue
    planted = [1] + ([c.A - 2] if c.last else [])
    assert c.A >= 3 and len(set(planted)) == len(planted)
    for b in range(c.batch):
        slab = t.element(b).view(c.A, c.K, c.B)
        for a in planted:
            slab[a, 0, :] = float("inf")
            slab[a, min(3, c.K - 1), min(5, c.B - 1)] = NAN
    out.buf.fill_(NAN)
    _call(c, t, cm, out)
    got = _result(c, out)
    assert out.outside_is_nan(), c.name
    keep = torch.ones(c.A, dtype=torch.bool, device=DEV)
    keep[planted] = False
    assert torch.equal(_bits(got[:, keep]), _bits(refd[:, keep])), f"{c.name}: a planted slab / row leaked"
    assert not bool(torch.isfinite(got[:, ~keep]).any()), f"{c.name}: finite results in a planted slab / row"


@pytest.mark.parametrize("c", S.BUILD_CASES, ids=lambda c: c.name)
def test_every_build_is_exact_guarded_and_isolates_slabs(c):
    assert S.build_id(S.build_of(c)) == c.name
    _exact(c, isolation=True)


@pytest.mark.parametrize("c", S.EDGE_CASES, ids=lambda c: c.name)
def test_every_edge_row_is_exact_and_guarded(c):
    _exact(c, isolation=False)


IDENTITY = [c for c in S.BUILD_CASES if c.name in ("pair20-inner-nt13", "pair12-inner-nt7", "deep-last-nt13",
                                                   "shallow-last-nt6", "short-inner-nt4", "short-last-nt4")]


@pytest.mark.parametrize("c", IDENTITY, ids=lambda c: c.name)
def test_every_realisation_of_one_contraction_returns_the_same_bits(c):
    """The same integer inputs through every build the options can reach from one shape -- the pair kernel against
    k1_no_pair, the long-stride kernel against both, every k1_force_nt from 1 to 13 against the free choice: equal,
    element for element, to each other and to the host."""
    T, Cm = S.integer_inputs(c)
    ref = S.exact_reference(c, T, Cm)
    ref += 0.0
    refd = _bits(torch.from_numpy(ref).to(DEV))
    t, cm, out = _place(c, T, Cm)
    variants = [{}] + [dict(k1_force_nt=nt) for nt in range(1, 14)]
    if not c.last:
        variants += [dict(k1_no_pair=1), dict(k1_force_wide=1)]
        variants += [dict(k1_no_pair=1, k1_force_nt=nt) for nt in (5, 9, 12)]
        variants += [dict(k1_force_wide=1, k1_force_nt=nt) for nt in (2, 7)]
    seen = set()
    for opts in variants:
        v = c._replace(opts=opts)
        seen.add(S.build_of(v))
        out.buf.fill_(NAN)
        _call(v, t, cm, out)
        assert out.outside_is_nan(), opts
        assert torch.equal(_bits(_result(c, out)), refd), (c.name, opts, S.build_of(v))
    JT = -(-c.J // 16)                                 # (a forced tile count splits the JT tiles evenly over its j-groups)
    assert {b[3] for b in seen} >= {-(-JT // -(-JT // nt)) for nt in range(1, JT + 1)}, seen
    if not c.last:
        assert {b[0] for b in seen} >= {"wide"} and len({b[0] for b in seen}) >= 2


ROUNDED = [c for c, b in zip(S.BUILD_CASES, S.BUILDS) if b[3] in (1, 6, 13) or (b[0] == "short" and b[3] == 4)]


@pytest.mark.parametrize("scaled", [False, True], ids=["normal", "scaled"])
@pytest.mark.parametrize("c", ROUNDED, ids=lambda c: c.name)
def test_rounded_results_stay_within_the_dot_product_bound(c, scaled):
    T, Cm = S.real_inputs(c, scaled)
    t, cm, out = _place(c, T, Cm)
    _call(c, t, cm, out)
    got = _result(c, out)
    assert out.outside_is_nan() and bool(torch.isfinite(got).all())
    idx = S.sample(c.A if c.last else c.B)
    ref, bound = S.rounded_reference(c, T, Cm, idx)
    ix = torch.from_numpy(idx).to(DEV)
    part = (got[:, ix] if c.last else got[:, :, :, ix]).cpu().numpy()
    ratio = float((np.abs(part.astype(S.LD) - ref) / bound.astype(S.LD)).max())
    print(f"error/bound {c.name} {'scaled' if scaled else 'normal'}: {ratio:.4f}")
    assert ratio <= 1.0, (c.name, scaled, ratio)


# ---- refusals: an error code and a message, nothing launched ---------------------------------------------------------
def test_refusals_launch_nothing():
    lib = _lib.load()
    c = S.case("r", 2, 30, 37, 50, batch=2)          # (room for two elements, should a refusal ever fail to refuse)
    T, Cm = S.integer_inputs(c)
    t, cm, out = _place(c, T, Cm)
    base = dict(T=t.first.data_ptr(), Cm=cm.first.data_ptr(), out=out.first.data_ptr(), A=2, K=30, J=37, B=50, ldc=37,
                last=0, batch=1, t_bs=0, c_bs=0, o_bs=0)
    order = ("T", "Cm", "out", "A", "K", "J", "B", "ldc", "last", "batch", "t_bs", "c_bs", "o_bs")

    def batch_call(**kw):
        a = dict(base, **kw)
        return lib.oovqe_mode_contract_batch(*[a[k] for k in order], _lib.stream_ptr())

    def plain_call(**kw):
        a = dict(base, **kw)
        return lib.oovqe_mode_contract(*[a[k] for k in order[:9]], _lib.stream_ptr())

    n_t, n_c, n_o = 2 * 30 * 50, 29 * 37 + 37, 2 * 37 * 50
    refused = [
        (dict(ldc=36), "bad dims"), (dict(last=1), "last-mode needs B == 1"), (dict(batch=0), "batch=0"),
        (dict(batch=65536), "batch=65536"), (dict(A=2_000_000_000, B=16), "too many strips"),
        (dict(T=None), "null pointer"), (dict(Cm=None), "null pointer"), (dict(out=None), "null pointer"),
        (dict(A=0), "bad dims"), (dict(K=0), "bad dims"), (dict(J=0), "bad dims"), (dict(B=0), "bad dims"),
    ]
    strides = [
        (dict(batch=2, t_bs=n_t, c_bs=n_c, o_bs=n_o - 1), "o_bs"), (dict(batch=2, t_bs=n_t, c_bs=n_c, o_bs=0), "o_bs"),
        (dict(batch=2, t_bs=n_t - 1, c_bs=n_c, o_bs=n_o), "t_bs"), (dict(batch=2, t_bs=-n_t, c_bs=n_c, o_bs=n_o), "t_bs"),
        (dict(batch=2, t_bs=n_t, c_bs=n_c - 1, o_bs=n_o), "c_bs"), (dict(batch=2, t_bs=n_t, c_bs=-1, o_bs=n_o), "c_bs"),
        (dict(batch=1, o_bs=-1), "o_bs"),
    ]
    for kw, msg in refused:
        for call in (batch_call, plain_call):
            if call is plain_call and "batch" in kw:
                continue
            assert call(**kw) != 0, kw
            assert msg in lib.oovqe_last_error().decode(), (kw, lib.oovqe_last_error())
    for kw, msg in strides:
        assert batch_call(**kw) != 0, kw
        assert msg in lib.oovqe_last_error().decode(), (kw, lib.oovqe_last_error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.buf).all()), "a refused call wrote to out"
    assert batch_call() == 0 and plain_call() == 0           # the same arguments, unharmed, are served
    torch.cuda.synchronize()


# ---- the thin entry points ---------------------------------------------------------------------------------------------
def _ints(rng, *shape, vmax=S.VMAX):
    return rng.integers(-vmax, vmax + 1, shape).astype(np.float64)


def test_matmul_entry_points_on_integer_inputs():
    """matmul_nn, matmul_tn and matmul_nn_batch on rectangular shapes that run more than one tile per wave"""
    rng = np.random.default_rng(11)
    M, K, N = 32_790, 50, 45
    assert ops.contract_plan(M, K, N, 1, True)["nt"] == 3
    A, B = _ints(rng, M, K), _ints(rng, K, N)
    got = ops.matmul_nn(torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV))
    assert np.array_equal(got.cpu().numpy(), A @ B)
    # matmul_tn(A [K, M], B [K, N]) = A^T B: INNER with one slab, J = M, the columns of B streamed
    M, K, N = 45, 50, 32_790
    assert ops.contract_plan(1, K, M, N, False)["nt"] == 3
    A, B = _ints(rng, K, M), _ints(rng, K, N)
    got = ops.matmul_tn(torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV))
    assert np.array_equal(got.cpu().numpy(), A.T @ B)
    for G, M, K, N, nt in ((3, 50, 37, 21, 1), (8, 8200, 30, 40, 3)):
        assert ops.contract_plan(M, K, N, 1, True, G, t_bs=M * K, o_bs=M * N)["nt"] == nt
        A, B = _ints(rng, G, M, K), _ints(rng, G, K, N)
        got = ops.matmul_nn_batch(torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV))
        assert np.array_equal(got.cpu().numpy(), A @ B)


@pytest.mark.parametrize("N", [17, 33])
def test_four_index_transform_on_integer_inputs(N):
    """Odd N: ragged in all four steps.  |M| <= 2, |C| <= 2: every sum stays below 2 (2 N)^4 < 2^53."""
    rng = np.random.default_rng(N)
    M = _ints(rng, N, N, N, N, vmax=2)
    C = [_ints(rng, N, N, vmax=2) for _ in range(4)]
    assert 2 * (2 * N) ** 4 < 2 ** 53
    ref = M.astype(np.int64)
    for axis, Ci in enumerate(C):                     # out[.., i, ..] = sum_p C[p, i] M[.., p, ..], one index at a time
        ref = np.moveaxis(np.tensordot(ref, Ci.astype(np.int64), axes=([axis], [0])), -1, axis)
    got = ops.general_4index_transform(*(torch.from_numpy(x).to(DEV) for x in [M] + C))
    assert np.array_equal(got.cpu().numpy(), ref.astype(np.float64))
