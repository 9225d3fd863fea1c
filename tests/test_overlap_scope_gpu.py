"""The sector-overlap kernel (csrc/overlap.hip) over its whole scope: every (N_alpha, N_beta) sector of ncas = 1 .. 8
against the host route, the fixture cases of tests/golden/overlap_scope_*.npz against 40-digit arithmetic, the index
table with entries outside the vectors, a pair list longer than the device has compute units, singular and non-finite
pairs, and ``state_overlaps_oao`` with an odd number of active electrons.

Bounds.  Against the host route: 1e-12 max(1, |reference|), the bound of tests/test_overlaps_gpu.py.  Against a fixture:
max(1e-12, 10 x host error) max(1, |reference|), where the host error is the error of the float64 host route on the same
inputs against the 40 digits, recorded in the fixture (``_overlaps.scope_bound``).  Neither is taken from the device.

Measured on the MI355X (error / max(1, |reference|); DESIGN.md, "The sector kernel over its whole scope", has the table
per case).  Every sector against the host route: worst 1.8e-15 (ncas = 8 and 6; 1.8e-16 at ncas = 1), the mirror identity
1.2e-15.  Fixtures, device error / host error: the generic cases up to m = 48 1.7e-18 .. 3.3e-16 / 5.2e-18 .. 4.3e-16 (the
148 000-byte launch 6.9e-18 / 6.9e-18, its mirror 1.7e-18 / 5.2e-18), signed-permutation core 1.1e-16 / 1.1e-16 with
core_det = +-1 exactly, core of cond 1e3 2.6e-15 / 9.3e-15, of cond 1e6 3.1e-12 / 1.4e-11 (bound 1.4e-10), Q factor of a
U of cond 1e2 5.6e-17 / 2.0e-16, of cond 1e5 4.8e-15 / 1.9e-13 (bound 1.9e-12), the pivoting matrices at (5, 3), (6, 2),
(8, 8) at most 1.4e-16 / 1.1e-15; core_det at most 2.3e-15 where the core is well conditioned, 1.7e-12 / 6.4e-12 at cond
1e6.  All 16 (rb, rk): 8.3e-17.  Index table: 1.1e-16, with entries outside the vectors 1.7e-16.  300 pairs: 5.4e-16.
A NaN in s_cc comes back as core_det = 0 and NaN overlaps, like a singular core.
"""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from auto_oo_amd import overlaps                                                                     # noqa: E402
from auto_oo_amd.berry import (bogoliubov_atob_cas, givens_orthogonal, minor_matrix, sector_tables,   # noqa: E402
                               state_overlap)
from tests import _overlaps as V                                                                     # noqa: E402

F64 = torch.float64
KINDS = ("orthogonal", "improper", "nonorthogonal", "permutation")


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def to_dev(x, dtype=F64):
    return torch.as_tensor(np.ascontiguousarray(x)).to(device=dev(), dtype=dtype)


def _rel(got, ref):
    return np.abs(np.asarray(got) - ref).max() / max(1.0, np.abs(ref).max())


def _mirror(v, na, nb):
    """[..., na nb] -> [..., nb na]: every vector transposed from [na, nb] to [nb, na]."""
    return np.ascontiguousarray(np.swapaxes(v.reshape(v.shape[:-1] + (na, nb)), -1, -2)).reshape(v.shape)


# ---- a. every sector ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncas", range(1, 9))
def test_every_sector_against_the_host_route(ncas):
    """All (N_alpha, N_beta) in 0 .. ncas squared, the four kinds of ``trial_matrices`` as the four pairs of one call,
    U as it is and its Q factor, signed, (rb, rk) = (2, 3).  The host's minor matrices are made once per (U, order).
    For an unequal sector also unsigned, and the mirror identity: the (N_beta, N_alpha) call on the transposed vectors
    returns the same numbers."""
    mats = V.trial_matrices(ncas, 1000 + ncas)
    U = np.stack([mats[k] for k in KINDS])
    assert np.abs(U[2] - U[2].T).max() > 1e-2 or ncas == 1       # (not symmetric: a transposed table would show)
    Ud = to_dev(U)
    strings = [sector_tables(ncas, k, k)[0] for k in range(ncas + 1)]
    rng = np.random.default_rng(ncas)
    worst = worst_mirror = 0.0
    for orthogonalize in (False, "givens"):
        Uh = np.stack([givens_orthogonal(u) for u in U]) if orthogonalize else U
        minors = [[minor_matrix(u, strings[k], ncas) for k in range(ncas + 1)] for u in Uh]
        for na_, nb_ in itertools.product(range(ncas + 1), repeat=2):
            sign = sector_tables(ncas, na_, nb_)[3]
            na, nb = sign.shape
            bra = rng.standard_normal((4, 2, na * nb)) / np.sqrt(na * nb)
            ket = rng.standard_normal((4, 3, na * nb)) / np.sqrt(na * nb)
            b, k = to_dev(bra), to_dev(ket)
            for signed in ((True,) if na_ == nb_ else (True, False)):
                ref = np.stack([V.contract(minors[p][na_], minors[p][nb_], sign, bra[p], ket[p], signed)
                                for p in range(4)])
                out, core = overlaps.sector_overlaps(Ud, 0, ncas, na_, nb_, b, k, orthogonalize=orthogonalize,
                                                     signed=signed)
                assert out.shape == (4, 2, 3) and torch.equal(core, torch.ones_like(core))
                got = out.cpu().numpy()
                for p, kind in enumerate(KINDS):
                    err = _rel(got[p], ref[p])
                    worst = max(worst, err)
                    assert err < 1e-12, (kind, na_, nb_, orthogonalize, signed, err)
            if na_ != nb_:
                back, core = overlaps.sector_overlaps(Ud, 0, ncas, nb_, na_, to_dev(_mirror(bra, na, nb)),
                                                      to_dev(_mirror(ket, na, nb)), orthogonalize=orthogonalize,
                                                      signed=False)
                assert torch.equal(core, torch.ones_like(core))
                back = back.cpu().numpy()
                for p, kind in enumerate(KINDS):
                    err = np.abs(back[p] - got[p]).max() / max(1.0, np.abs(ref[p]).max())
                    worst_mirror = max(worst_mirror, err)
                    assert err < 1e-12, ("mirror", kind, na_, nb_, orthogonalize, err)
    print(f"every sector, ncas {ncas}: worst {worst:.2e}, mirror {worst_mirror:.2e}")


# ---- b. the fixture cases against 40 digits ------------------------------------------------------------------------------
def _run_fixture(f, rb=None, rk=None):
    args = (int(f["n_core"]), int(f["ncas"]), int(f["n_alpha"]), int(f["n_beta"]))
    bra, ket = f["bra"][:, :rb], f["ket"][:, :rk]
    out, core = overlaps.sector_overlaps(to_dev(f["s"]), *args, to_dev(bra), to_dev(ket),
                                         orthogonalize="givens" if int(f["mode"]) else False, signed=bool(f["signed"]))
    return out.cpu().numpy(), core.cpu().numpy()


@pytest.mark.parametrize("name", list(V.SCOPE_CASES))
def test_fixture_case_against_forty_digits(name):
    f = V.scope_fixture(name)
    got, core = _run_fixture(f)
    bound, bound_core = V.scope_bound(f["host_err"]), V.scope_bound(f["host_core_err"])
    assert got.shape == f["out"].shape
    for p in range(got.shape[0]):
        err = _rel(got[p], f["out"][p])
        err_core = abs(core[p] - f["core_det"][p]) / max(1.0, abs(f["core_det"][p]))
        print(f"{name} pair {p}: error {err:.2e} (host {float(f['host_err']):.2e}, bound {bound:.2e}), core_det "
              f"{err_core:.2e} (host {float(f['host_core_err']):.2e}), cond(s_cc) {f['cond_core'][p]:.3g}, cond(U) "
              f"{f['cond_U'][p]:.3g}")
        assert err < bound
        assert err_core < bound_core
    if int(f["n_core"]) == 0 or V.SCOPE_CASES[name][8] == "permutation":
        assert np.array_equal(core, f["core_det"])              # 1, or +-1 of a signed permutation: exactly


def test_the_mirror_of_the_largest_launch():
    """ncas = 8, (4, 3) with m = 48 (148 000 bytes of LDS) and (3, 4) on the transposed vectors: unsigned, the same
    numbers."""
    a, b = V.scope_fixture("c8_43_core40"), V.scope_fixture("c8_34_core40")
    assert np.array_equal(a["s"], b["s"]) and np.array_equal(_mirror(a["bra"], 70, 56), b["bra"])
    res = []
    for f in (a, b):
        out, core = overlaps.sector_overlaps(to_dev(f["s"]), 40, 8, int(f["n_alpha"]), int(f["n_beta"]), to_dev(f["bra"]),
                                             to_dev(f["ket"]), signed=False)
        res.append((out.cpu().numpy(), core.cpu().numpy()))
    err = np.abs(res[0][0] - res[1][0]).max()
    print(f"mirror of the largest launch: {err:.2e}")
    assert err < 1e-12 and np.array_equal(res[0][1], res[1][1])


def test_all_sixteen_vector_counts():
    f = V.scope_fixture(V.ROOTS_CASE)
    assert f["out"].shape[1:] == (4, 4)
    bound = V.scope_bound(f["host_err"])
    worst = 0.0
    for rb, rk in itertools.product(range(1, 5), repeat=2):
        got, _ = _run_fixture(f, rb, rk)
        assert got.shape[1:] == (rb, rk)
        err = _rel(got, f["out"][:, :rb, :rk])
        worst = max(worst, err)
        assert err < bound, (rb, rk, err)
    print(f"all (rb, rk): worst {worst:.2e}")


@pytest.mark.parametrize("kind", ["zero_column", "zero_row"])
def test_vanishing_minors_are_exact_zeros(kind):
    """Column 2 (row 2) of U vanishes: a ket (bra) that lives on the alpha strings which occupy orbital 2 meets only
    minors through it, and the result is 0 exactly, not a small number.  At (8, 8) the one determinant is 0."""
    U = V.pivot_matrices(8)[kind]
    ua, ub, _, _ = sector_tables(8, 5, 3)
    rng = np.random.default_rng(53)
    through = np.array([(int(m) >> (8 - 1 - 2)) & 1 for m in ua], dtype=float)
    mask = np.repeat(through, len(ub))
    bra, ket = rng.standard_normal((1, 2, mask.size)), rng.standard_normal((1, 3, mask.size))
    if kind == "zero_column":
        ket = ket * mask
    else:
        bra = bra * mask
    for signed in (True, False):
        out, _ = overlaps.sector_overlaps(to_dev(U[None]), 0, 8, 5, 3, to_dev(bra), to_dev(ket), signed=signed)
        assert torch.equal(out, torch.zeros_like(out))
    one = to_dev(np.ones((1, 1, 1)))
    out, _ = overlaps.sector_overlaps(to_dev(U[None]), 0, 8, 8, 8, one, one)
    assert out.item() == 0.0


# ---- c. index table ----------------------------------------------------------------------------------------------------------
def test_index_table_with_entries_outside_the_vectors():
    ncas, na_, nb_ = 5, 3, 2
    x = sector_tables(ncas, na_, nb_)[2].reshape(-1)
    index = overlaps.dense_index(ncas, na_, nb_, dev())
    assert index.dtype == torch.int32 and np.array_equal(index.cpu().numpy(), x)
    ld = 1 << (2 * ncas)
    rng = np.random.default_rng(532)
    U = V.trial_matrices(ncas, 532)["nonorthogonal"]
    bra, ket = rng.standard_normal((1, 2, ld)) / 10, rng.standard_normal((1, 3, ld)) / 10
    out, _ = overlaps.sector_overlaps(to_dev(U[None]), 0, ncas, na_, nb_, to_dev(bra), to_dev(ket), index=index)
    ref = V.host_route(U, ncas, na_, nb_, bra[0][:, x], ket[0][:, x])
    err = _rel(out[0].cpu().numpy(), ref)
    assert err < 1e-12
    # entries outside the vector read zero
    table = x.copy()
    lost = rng.permutation(x.size)[:30]
    table[lost[:10]] = -1
    table[lost[10:20]] = ld
    table[lost[20:25]] = ld + 12345
    table[lost[25:]] = -(2 ** 31)
    keep = np.ones(x.size)
    keep[lost] = 0.0
    ref0 = V.host_route(U, ncas, na_, nb_, bra[0][:, x] * keep, ket[0][:, x] * keep)
    assert _rel(ref0, ref) > 1e-3                               # (the lost amplitudes matter)
    for signed in (True, False):
        ref0 = V.host_route(U, ncas, na_, nb_, bra[0][:, x] * keep, ket[0][:, x] * keep, signed=signed)
        out, _ = overlaps.sector_overlaps(to_dev(U[None]), 0, ncas, na_, nb_, to_dev(bra), to_dev(ket), signed=signed,
                                          index=to_dev(table, torch.int32))
        err0 = _rel(out[0].cpu().numpy(), ref0)
        print(f"index table, signed {signed}: {err:.2e}, with entries outside {err0:.2e}")
        assert err0 < 1e-12


# ---- d. pair list and bits ------------------------------------------------------------------------------------------------------
NCAS_D, SECTOR_D, CORE_D = 4, (3, 1), 3


def _list_case(P, seed):
    rng = np.random.default_rng(seed)
    m = CORE_D + NCAS_D
    s = np.stack([V._generic_s(m, CORE_D, rng) for _ in range(P)])
    bra, ket = rng.standard_normal((P, 2, 16)) / 4, rng.standard_normal((P, 2, 16)) / 4
    return s, bra, ket


def _alone(s, bra, ket, p):
    out, core = overlaps.sector_overlaps(s[p:p + 1], CORE_D, NCAS_D, *SECTOR_D, bra[p:p + 1], ket[p:p + 1])
    return out[0], core[0]


def test_three_hundred_pairs_and_their_bits():
    P = 300
    assert P > torch.cuda.get_device_properties(dev()).multi_processor_count
    s, bra, ket = _list_case(P, 431)
    sd, bd, kd = to_dev(s), to_dev(bra), to_dev(ket)
    out, core = overlaps.sector_overlaps(sd, CORE_D, NCAS_D, *SECTOR_D, bd, kd)
    got, det = out.cpu().numpy(), core.cpu().numpy()
    worst = 0.0
    for p in range(P):
        ref, d = V.core_fold(s[p], CORE_D, NCAS_D, *SECTOR_D, bra[p], ket[p])
        worst = max(worst, _rel(got[p], ref), abs(det[p] - d) / max(1.0, abs(d)))
    print(f"300 pairs: worst {worst:.2e}")
    assert worst < 1e-12
    alone = [_alone(sd, bd, kd, p) for p in range(P)]
    assert torch.equal(torch.stack([a[0] for a in alone]), out) and torch.equal(torch.stack([a[1] for a in alone]), core)
    order = torch.as_tensor(np.random.default_rng(1).permutation(P), device=dev())
    moved, moved_core = overlaps.sector_overlaps(sd[order], CORE_D, NCAS_D, *SECTOR_D, bd[order], kd[order])
    assert torch.equal(moved, out[order]) and torch.equal(moved_core, core[order])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other, other_core = overlaps.sector_overlaps(sd, CORE_D, NCAS_D, *SECTOR_D, bd, kd)
    side.synchronize()
    assert torch.equal(other, out) and torch.equal(other_core, core)


# ---- e. singular and non-finite pairs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["zero core column", "NaN in s_cc"])
def test_a_singular_or_non_finite_pair_between_two_others(what):
    s, bra, ket = _list_case(3, 77)
    if what == "zero core column":
        s[1, :CORE_D, 1] = 0.0
    else:
        s[1, 2, 0] = np.nan
    sd, bd, kd = to_dev(s), to_dev(bra), to_dev(ket)
    out, core = overlaps.sector_overlaps(sd, CORE_D, NCAS_D, *SECTOR_D, bd, kd)
    assert bool(torch.isnan(out[1]).all())
    print(f"{what}: core_det {core[1].item()}")
    if what == "zero core column":
        assert core[1].item() == 0.0
    for p in (0, 2):
        o, c = _alone(sd, bd, kd, p)
        assert torch.equal(o, out[p]) and torch.equal(c, core[p]) and bool(torch.isfinite(out[p]).all())
        ref, d = V.core_fold(s[p], CORE_D, NCAS_D, *SECTOR_D, bra[p], ket[p])
        assert _rel(out[p].cpu().numpy(), ref) < 1e-12 and abs(c.item() - d) < 1e-12


# ---- f. the route above the kernel with an unequal sector ------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["dense", "sector"])
def test_state_overlaps_oao_with_three_electrons_in_three_orbitals(layout):
    """nelecas = 3 in ncas = 3 is the sector (2, 1) (``hf_state`` fills high spin first): ``state_overlaps_oao`` accepts
    it, in both layouts of the states, and agrees with the loop of ``bogoliubov_atob_cas`` + ``state_overlap``."""
    ncas, nelecas, N, P, act = 3, 3, 7, 3, [2, 3, 4]
    x = sector_tables(ncas, 2, 1)[2].reshape(-1)
    rng = np.random.default_rng(321)
    oao_a = np.stack([V.random_orthogonal(N, rng) for _ in range(P)])
    oao_b = np.stack([V.random_orthogonal(N, rng, improper=bool(p % 2)) for p in range(P)])
    vec = rng.standard_normal((2, P, x.size))
    vec /= np.linalg.norm(vec, axis=2, keepdims=True)
    dense = np.zeros((2, P, 1 << (2 * ncas)))
    dense[:, :, x] = vec
    bra, ket = (dense if layout == "dense" else vec)
    got = overlaps.state_overlaps_oao(to_dev(bra), to_dev(ket), to_dev(oao_a), to_dev(oao_b), act, nelecas)
    got = got.cpu().numpy()
    assert got.shape == (P,)
    for p in range(P):
        rot = bogoliubov_atob_cas(oao_a[p].T @ oao_b[p], act, nelecas)
        assert rot.M_alpha.shape == (3, 3) and rot.M_beta.shape == (3, 3) and len(rot.strings_a) == 3
        ref = state_overlap(to_dev(dense[0, p]), rot, to_dev(dense[1, p])).item()
        print(f"oao overlap (2, 1) {layout} pair {p}: {got[p]:+.12f} against {ref:+.12f}")
        assert abs(got[p] - ref) < 1e-12
