"""The particle-number-sector engine (csrc/sector.hip) over its whole scope against the host twin of
tests/_sector_scope.py (validated in tests/test_sector_scope_cpu.py): unequal and empty spin sectors, dense vectors at
every ncas from 2 to 13, odd sector sizes, every batch threshold of every route and every debug option, the
per-geometry forms, the refusals.  Every output buffer starts as NaN (the engine's allocations are swapped for
NaN-filled ones, its workspace included), every element is compared, and every test prints its largest
error / bound before it asserts.  The bounds are derived in tests/_sector_scope.py and DESIGN.md ("The sector engine
over its whole scope"); none comes from device output.

Largest error / bound measured on an MI355X (256 CUs; every route landed where the case tables of
tests/test_sector_scope_cpu.py put it), per group of cases -- all 209 cases passed, no bound was changed:
    states and differentiated states (2-norm, 8 n_gates u)      0.046  (ncas 4, (2,2), batch 3; ncas 13: 0.006)
    RDMs of every sector, with and without the table block      0.078  (ncas 3, (2,1), gamma; ncas 13: 0.008)
    RDM batch walks, every option                               0.054  (ncas 4, (2,1), batch 130, row chunks)
    lam, every option, batches 1 .. 130                         0.005  (ncas 2; ncas 8 and 13: 0.001)
    adjoint, pair lists and gate sweep                          0.001
    per-geometry coefficients (lam, adjoint, every sector)      0.004
    theta-theta block, both routes                              < 0.0005
    the public odd-electron route (RDMs and their derivatives)  0.001; E off by 5e-15 (bound 1e-9)
(the bounds are worst-case sums over up to 4 (a^4 + a^3 + a^2) products: a wrong sign or index is an error of order
one, 10^10 bounds and more -- DESIGN.md lists what three planted defects did).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from auto_oo_amd import _lib, excitations as X, sector as sector_mod
from auto_oo_amd._lib import debug_options, dptr, stream_ptr
from auto_oo_amd.sector import SectorEngine
from tests import _sector_scope as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
FIGURES = {}


class _NanTorch:
    """``torch`` as auto_oo_amd.sector sees it during these tests: ``empty`` hands out NaN (outputs, workspace)."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(*args, **kwargs):
        t = torch.empty(*args, **kwargs)
        if t.dtype.is_floating_point:
            t.fill_(float("nan"))
        return t


@pytest.fixture(autouse=True)
def nan_outputs(monkeypatch):
    monkeypatch.setattr(sector_mod, "torch", _NanTorch())


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=F64, device=DEV)


def dev(x, dtype=F64):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def record(group, what, err, bound):
    """print the figure next to its bound, remember the largest ratio of the group, assert every element."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert np.isfinite(err).all(), f"{what}: NaN or Inf in the result"
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    print(f"{group}: {what}: largest error {float(err.max()):.3e}, bound there "
          f"{float(np.broadcast_to(bound, err.shape).reshape(-1)[int(err.argmax())]):.3e}, largest error / bound {ratio:.3f}")
    FIGURES[group] = max(FIGURES.get(group, 0.0), ratio)
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} elements past their bound (ratio {ratio:.3f})"


@functools.lru_cache(maxsize=None)
def twin_sector(ncas, na, nb):
    return S.Sector(ncas, na, nb)


@functools.lru_cache(maxsize=None)
def case(ncas, na, nb, kind):
    sec = twin_sector(ncas, na, nb)
    gates, n_theta = S.circuit(kind, ncas, na, nb)
    occ = sec.occupation()
    return sec, gates, n_theta, occ, X.basis_index(occ)


def engine(ncas, na, nb, kind):
    sec, gates, n_theta, occ, init = case(ncas, na, nb, kind)
    gd = torch.as_tensor(X.gates_to_numpy(gates)).to(DEV)
    eng = SectorEngine(ncas, occ, gd, len(gates), n_theta, init, torch.device(DEV))
    assert (eng.na, eng.nb) == (sec.na, sec.nb)
    assert np.array_equal(eng.unrank_a.cpu().numpy(), sec.ua) and np.array_equal(eng.unrank_b.cpu().numpy(), sec.ub)
    return eng


@functools.lru_cache(maxsize=None)
def twin_rdms(ncas, na, nb, seed, n):
    sec = twin_sector(ncas, na, nb)
    vecs = S.make_vectors(sec, seed, n)
    return vecs, [sec.rdms(v) for v in vecs], [S.rdm_bounds(sec, v) for v in vecs]


@functools.lru_cache(maxsize=None)
def twin_lam(ncas, na, nb, seed, n):
    sec = twin_sector(ncas, na, nb)
    vecs = S.make_vectors(sec, seed, n)
    c1, c2 = S.coefficients(ncas, seed + 1)
    return vecs, c1, c2, [sec.lam(v, c1, c2) for v in vecs], [S.lam_bound(sec, v, c1, c2) for v in vecs]


def tiled(vecs, batch):
    idx = np.arange(batch) % len(vecs)
    return dev(vecs[idx]), idx


def check_rdms(group, what, g1, g2, idx, refs, bounds):
    g1, g2 = g1.cpu().numpy(), g2.cpu().numpy()
    first = {}
    for b, i in enumerate(idx):
        if i in first:      # a repeated vector: the same bits as its first copy, wherever it stands in the batch
            assert np.array_equal(g1[b], g1[first[i]]) and np.array_equal(g2[b], g2[first[i]]), (what, b)
            continue
        first[i] = b
        record(group, f"{what} gamma[{b}]", np.abs(g1[b] - refs[i][0]), bounds[i][0])
        record(group, f"{what} Gamma[{b}]", np.abs(g2[b] - refs[i][1]), bounds[i][1])


def plain_rdms(eng, vecs):
    """oovqe_sector_rdms: no table block (every workgroup builds the excitation tables from the strings)."""
    batch, a = vecs.shape[0], eng.ncas
    g1, g2 = nan(batch, a, a), nan(batch, a, a, a, a)
    rc = eng.lib.oovqe_sector_rdms(dptr(vecs), a, *eng._tabs(), batch, dptr(g1), dptr(g2), dptr(eng.work(batch)),
                                   stream_ptr())
    assert rc == 0, eng.lib.oovqe_last_error()
    return g1, g2


ALL = S.SECTORS + S.STATE_ONLY


# ---- states and differentiated states ------------------------------------------------------------------------------
@pytest.mark.parametrize("s", ALL, ids=S.sector_id)
def test_states_and_differentiated_states(s):
    ncas, na, nb, kind = s[:4]
    sec, gates, n_theta, occ, init = case(ncas, na, nb, kind)
    eng = engine(ncas, na, nb, kind)
    lib = eng.lib
    counts = S.apply_gates(gates, np.zeros(n_theta), sec, init)[1]
    pairs, max_pairs = eng.pair_lists()
    assert np.array_equal(pairs[:len(gates)].cpu().numpy(), counts) and max_pairs == counts.max()
    live = [g for g in range(len(gates)) if counts[g] > 0]
    idle = [g for g in range(len(gates)) if gates[g].theta_idx >= 0 and counts[g] == 0]
    g, h = live[0], live[-1]
    specs = [(-1, -1), (g, -1), (h, -1), (g, g), (g, h), (h, g)]
    if idle:        # a gate with no pair in this sector: differentiated, it annihilates everything
        specs += [(idle[0], -1), (g, idle[0])]
    bound = S.state_bound(gates)
    gd = eng.gates_dev
    for batch in (1, 3):
        theta = np.random.default_rng(100 * ncas + 10 * na + nb + batch).uniform(0, 2 * np.pi, (batch, n_theta))
        th = dev(theta)
        ref = np.array([[S.apply_gates(gates, theta[b], sec, init, sp)[0] for sp in specs] for b in range(batch)])
        psi = eng.state(th)
        der = eng.derivative_states(th, specs)
        record("states", f"{S.sector_id(s)} batch {batch} state_pl", np.linalg.norm(psi.cpu().numpy() - ref[:, 0], axis=1),
               bound)
        record("states", f"{S.sector_id(s)} batch {batch} deriv_pl",
               np.linalg.norm(der.cpu().numpy() - ref, axis=2), bound)
        assert torch.equal(der[:, 0], psi)
        if 2 * ncas <= 20:
            psi2, dense = eng.state(th, dense=True)
            assert torch.equal(psi2, psi)
            dn = dense.cpu().numpy()
            assert np.array_equal(dn[:, sec.x], psi.cpu().numpy()) and \
                np.count_nonzero(dn) == np.count_nonzero(psi.cpu().numpy())
        # the plain entries (the gate sweep): the same numbers where the sector fits them, refused before any launch
        # where it does not
        spec = dev(np.asarray(specs, dtype=np.int32), torch.int32)
        psi0, der0 = nan(batch, sec.Dc), nan(batch, len(specs), sec.Dc)
        rc = lib.oovqe_sector_state(dptr(th), n_theta, dptr(gd, torch.uint8), len(gates), ncas, ctypes.c_uint32(init),
                                    *eng._tabs(), batch, dptr(psi0), None, stream_ptr())
        rcd = lib.oovqe_sector_state_deriv(dptr(th), n_theta, dptr(gd, torch.uint8), len(gates), ncas,
                                           ctypes.c_uint32(init), *eng._tabs(), batch, dptr(spec, torch.int32),
                                           len(specs), dptr(der0), stream_ptr())
        if S.sweep_route(ncas, sec.na, sec.nb, len(gates), n_theta, max_pairs, False, "state") == "refused":
            assert rc != 0 and rcd != 0 and torch.isnan(psi0).all() and torch.isnan(der0).all()
        else:
            assert rc == 0 and rcd == 0, lib.oovqe_last_error()
            assert torch.equal(psi0, psi) and torch.equal(der0, der)       # the same arithmetic on the same pairs
    assert S.sweep_route(ncas, sec.na, sec.nb, len(gates), n_theta, max_pairs, True, "state") != "refused"


# ---- RDMs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", S.SECTORS, ids=S.sector_id)
def test_rdms_of_every_sector(s):
    """dense, zero-patterned and one-determinant vectors at batches on both sides of the E_pq and Gram thresholds, with
    and without the table block."""
    ncas, na, nb, kind = s[:4]
    sec = twin_sector(ncas, na, nb)
    eng = engine(ncas, na, nb, kind)
    vecs, refs, bounds = twin_rdms(ncas, na, nb, 7, 4)
    for batch in S.RDM_BATCHES_EACH:
        v, idx = tiled(vecs, batch)
        route = S.rdm_route(ncas, sec.na, sec.nb, batch, cus())
        print(S.sector_id(s), "batch", batch, "->", route)
        check_rdms("rdms", f"{S.sector_id(s)} batch {batch}", *eng.rdms(v), idx, refs, bounds)
        check_rdms("rdms", f"{S.sector_id(s)} batch {batch} no tables", *plain_rdms(eng, v), idx, refs, bounds)
        eng._work.clear()


@pytest.mark.parametrize("batch", S.RDM_BATCHES_GENERIC)
@pytest.mark.parametrize("key", S.RDM_WALK_GENERIC, ids=lambda k: "a%d_%d_%d" % k)
def test_rdm_batch_walk_generic(key, batch):
    ncas, na, nb = key
    s = next(t for t in S.SECTORS if t[:3] == key)
    sec = twin_sector(ncas, na, nb)
    eng = engine(*s[:4])
    vecs, refs, bounds = twin_rdms(ncas, na, nb, 11, 5)
    v, idx = tiled(vecs, batch)
    print("route:", S.rdm_route(ncas, sec.na, sec.nb, batch, cus()))
    check_rdms("rdms walk", f"a{ncas} ({na},{nb}) batch {batch}", *eng.rdms(v), idx, refs, bounds)


@pytest.mark.parametrize("opt", S.RDM_OPTIONS, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()) or "default")
@pytest.mark.parametrize("batch", S.RDM_BATCHES_FUSED)
@pytest.mark.parametrize("key", S.RDM_WALK_FUSED, ids=lambda k: "a%d_%d_%d" % k)
def test_rdm_batch_walk_fused(key, batch, opt):
    ncas, na, nb = key
    s = next(t for t in S.SECTORS if t[:3] == key)
    sec = twin_sector(ncas, na, nb)
    eng = engine(*s[:4])
    vecs, refs, bounds = twin_rdms(ncas, na, nb, 13, 5)
    v, idx = tiled(vecs, batch)
    route = S.rdm_route(ncas, sec.na, sec.nb, batch, cus(), opt.get("sector_unfused", 0), opt.get("sector_rdm_r3", 0))
    assumed = S.rdm_route(ncas, sec.na, sec.nb, batch, 256, opt.get("sector_unfused", 0), opt.get("sector_rdm_r3", 0))
    print("route:", route, "" if route == assumed else f"(the case table assumes 256 CUs: {assumed})")
    with debug_options(**opt):
        check_rdms("rdms walk", f"a{ncas} ({na},{nb}) batch {batch} {opt}", *eng.rdms(v), idx, refs, bounds)
        check_rdms("rdms walk", f"a{ncas} ({na},{nb}) batch {batch} {opt} no tables", *plain_rdms(eng, v), idx, refs,
                   bounds)


def test_rdms_chunked_across_a_chunk_edge():
    s = next(t for t in S.SECTORS if t[:3] == (8, 4, 3))
    eng = engine(*s[:4])
    vecs, refs, bounds = twin_rdms(8, 4, 3, 13, 5)
    v, idx = tiled(vecs, 21)
    g1, g2 = eng.rdms_chunked(v, chunk=16)            # 16 (row chunks) + 5 (chunks of 128 determinants)
    assert g1.shape[0] == 21
    for lo, hi in ((0, 16), (16, 21)):
        check_rdms("rdms walk", f"chunked [{lo}:{hi}]", g1[lo:hi], g2[lo:hi], idx[lo:hi], refs, bounds)


# ---- lam and the reverse sweep -------------------------------------------------------------------------------------
def _adjoint_case(s, batch):
    ncas, na, nb, kind = s[:4]
    sec, gates, n_theta, occ, init = case(ncas, na, nb, kind)
    theta = np.random.default_rng(3 * ncas + na).uniform(0, 2 * np.pi, (2, n_theta))
    c1, c2 = S.coefficients(ncas, 31)
    out = []
    for b in range(2):
        psi = S.apply_gates(gates, theta[b], sec, init)[0]
        g, lam = S.adjoint(gates, theta[b], sec, init, c1, c2, n_theta, psi)
        out.append((psi, g, S.adjoint_bound(sec, gates, n_theta, psi, lam, S.lam_bound(sec, psi, c1, c2))))
    idx = np.arange(batch) % 2
    return theta[idx], np.array([out[i][0] for i in idx]), c1, c2, out, idx


_adjoint_case = functools.lru_cache(maxsize=None)(_adjoint_case)


def check_adjoint(group, what, dth, out, idx):
    dth = dth.cpu().numpy()
    first = {}
    for b, i in enumerate(idx):
        if i in first:
            assert np.array_equal(dth[b], dth[first[i]]), (what, b)
            continue
        first[i] = b
        record(group, f"{what} dtheta[{b}]", np.abs(dth[b] - out[i][1]), out[i][2])


@pytest.mark.parametrize("s", S.SECTORS, ids=S.sector_id)
def test_lam_and_adjoint_of_every_sector(s):
    ncas, na, nb, kind = s[:4]
    sec, gates, n_theta, occ, init = case(ncas, na, nb, kind)
    eng = engine(ncas, na, nb, kind)
    vecs, c1, c2, refs, bounds = twin_lam(ncas, na, nb, 5, 4)
    c1d, c2d = dev(c1), dev(c2)
    batches = S.LAM_BATCHES + (S.LAM_BATCHES_FUSED_EXTRA if s[:3] in S.RDM_WALK_FUSED else [])
    for opt in (S.LAM_OPTIONS if ncas in (4, 8) else [{}]):
        with debug_options(**opt):
            for batch in batches:
                v, idx = tiled(vecs, batch)
                print(S.sector_id(s), opt, "batch", batch, "->",
                      S.lam_route(ncas, sec.na, sec.nb, batch, cus(), opt.get("sector_unfused", 0),
                                  opt.get("sector_lambda_w", 0)))
                lam = eng.lam(v, c1d, c2d).cpu().numpy()
                first = {}
                for b, i in enumerate(idx):
                    if i in first:
                        assert np.array_equal(lam[b], lam[first[i]]), (opt, batch, b)
                        continue
                    first[i] = b
                    record("lam", f"{S.sector_id(s)} {opt} batch {batch} lam[{b}]", np.abs(lam[b] - refs[i]), bounds[i])
                eng._work.clear()
            for batch in (1, 33):
                theta, psi, a1, a2, out, idx = _adjoint_case(s, batch)
                th_d, psi_d, a1_d, a2_d = dev(theta), dev(psi), dev(a1), dev(a2)
                dth = eng.adjoint(th_d, psi_d, a1_d, a2_d)
                check_adjoint("adjoint", f"{S.sector_id(s)} {opt} batch {batch}", dth, out, idx)
                # the gate sweep without pair lists
                d0 = nan(batch, n_theta)
                rc = eng.lib.oovqe_sector_adjoint(dptr(th_d), n_theta, dptr(eng.gates_dev, torch.uint8),
                                                  len(gates), ncas, *eng._tabs(), batch, dptr(psi_d), dptr(a1_d),
                                                  dptr(a2_d), dptr(eng.work(batch)), dptr(d0), stream_ptr())
                if S.sweep_route(ncas, sec.na, sec.nb, len(gates), n_theta, 0, False, "adjoint") == "refused":
                    assert rc != 0 and torch.isnan(d0).all()
                else:
                    assert rc == 0, eng.lib.oovqe_last_error()
                    check_adjoint("adjoint", f"{S.sector_id(s)} {opt} batch {batch} plain", d0, out, idx)
                eng._work.clear()


@pytest.mark.parametrize("key", [(4, 2, 1), (8, 4, 3), (6, 3, 2)], ids=lambda k: "a%d_%d_%d" % k)
def test_adjoint_after_rdms_on_the_same_workspace_and_on_a_fresh_engine(key):
    s = next(t for t in S.SECTORS if t[:3] == key)
    theta, psi, c1, c2, out, idx = _adjoint_case(s, 3)
    eng = engine(*s[:4])
    eng.rdms(dev(psi))
    after = eng.adjoint(dev(theta), dev(psi), dev(c1), dev(c2))
    fresh = engine(*s[:4]).adjoint(dev(theta), dev(psi), dev(c1), dev(c2))
    check_adjoint("adjoint", f"a{key} after rdms", after, out, idx)
    assert torch.equal(after, fresh)


# ---- per-geometry coefficients --------------------------------------------------------------------------------------
def _geometry_rows(ncas, G, seed):
    """[G, stride] rows NaN padded around c1 | c2, as OO_pqc_batch hands the columns of its packed outputs over."""
    a2 = ncas * ncas
    off, stride = 3, 3 + a2 + a2 * a2 + 6
    wide = np.full((G, stride), np.nan)
    cs = []
    for g in range(G):
        c1, c2 = S.coefficients(ncas, seed + g)
        wide[g, off:off + a2] = c1.reshape(-1)
        wide[g, off + a2:off + a2 + a2 * a2] = c2.reshape(-1)
        cs.append((c1, c2))
    wd = dev(wide)
    return wd, wd[:, off:off + a2], stride, cs


@pytest.mark.parametrize("key", [(4, 2, 2), (4, 2, 1), (4, 1, 3), (8, 4, 3), (8, 1, 4), (8, 2, 1)],
                         ids=lambda k: "a%d_%d_%d" % k)
def test_lam_and_adjoint_geometries(key):
    s = next(t for t in S.SECTORS if t[:3] == key)
    ncas, na, nb, kind = s[:4]
    sec, gates, n_theta, occ, init = case(ncas, na, nb, kind)
    eng = engine(ncas, na, nb, kind)
    assert eng.geometry_coefficients_ok()
    G = 3
    wide, c1view, stride, cs = _geometry_rows(ncas, G, 50)
    for group in (1, 1 + n_theta):
        vecs = S.make_vectors(sec, 60 + group, min(G * group, 6))
        v, idx = tiled(vecs, G * group)
        lam = eng.lam_geometries(v, group, c1view, stride).cpu().numpy()
        for b, i in enumerate(idx):
            c1, c2 = cs[b // group]
            record("geometries", f"a{key} group {group} lam[{b}]", np.abs(lam[b] - sec.lam(vecs[i], c1, c2)),
                   S.lam_bound(sec, vecs[i], c1, c2))
    theta = np.random.default_rng(ncas).uniform(0, 2 * np.pi, (G, n_theta))
    psi = np.array([S.apply_gates(gates, theta[g], sec, init)[0] for g in range(G)])
    dth = eng.adjoint_geometries(dev(theta), dev(psi), c1view, stride).cpu().numpy()
    for g in range(G):
        c1, c2 = cs[g]
        ref, lam = S.adjoint(gates, theta[g], sec, init, c1, c2, n_theta, psi[g])
        record("geometries", f"a{key} adjoint[{g}]", np.abs(dth[g] - ref),
               S.adjoint_bound(sec, gates, n_theta, psi[g], lam, S.lam_bound(sec, psi[g], c1, c2)))
    assert torch.isnan(wide[:, :3]).all() and torch.isnan(wide[:, -6:]).all()


def _lam_pg(eng, v, group, c1view, stride, out):
    a = eng.ncas
    eng.pair_lists()
    p1 = c1view.data_ptr()
    return eng.lib.oovqe_sector_lambda_pg(dptr(v), a, *eng._tabs(), v.shape[0], int(group), ctypes.c_void_p(p1),
                                          ctypes.c_void_p(p1 + 8 * a * a), int(stride), eng._tables_ptr,
                                          dptr(eng.work(v.shape[0])), dptr(out), stream_ptr())


@pytest.mark.parametrize("ncas", [4, 8])
def test_geometry_coefficients_ok_agrees_with_the_call(ncas):
    """every (N_alpha, N_beta) with 1 <= N <= ncas - 1, and the sectors of one string (N = 0) of the table: where the
    library says yes the call succeeds and meets the twin (one state per geometry: the tightest workspace), where it
    says no the call is refused before any launch."""
    sectors = [(na, nb) for na in range(1, ncas) for nb in range(1, ncas)] + [(0, ncas // 2), (ncas // 2, 0)]
    yes = no = 0
    wide, c1view, stride, cs = _geometry_rows(ncas, 2, 80)
    for na, nb in sectors:
        sec = twin_sector(ncas, na, nb)
        eng = engine(ncas, na, nb, "ladder")
        vecs = S.make_vectors(sec, 90, 2)
        for unfused in (0, 1):
            with debug_options(sector_unfused=unfused):
                ok = eng.geometry_coefficients_ok()
                out = nan(2, sec.Dc)
                rc = _lam_pg(eng, dev(vecs), 1, c1view, stride, out)
                if ok:
                    yes += 1
                    assert rc == 0, (na, nb, eng.lib.oovqe_last_error())
                    for g in range(2):
                        record("geometries", f"a{ncas} ({na},{nb}) lam_pg[{g}]",
                               np.abs(out[g].cpu().numpy() - sec.lam(vecs[g], *cs[g])), S.lam_bound(sec, vecs[g], *cs[g]))
                else:
                    no += 1
                    assert rc != 0 and torch.isnan(out).all(), (na, nb, unfused)
        assert not (sec.na == 1 or sec.nb == 1) or not eng.geometry_coefficients_ok()
    print(f"ncas {ncas}: {yes} accepted, {no} refused")
    assert yes >= (ncas - 1) ** 2 and no >= len(sectors)


# ---- the theta-theta block -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("by_rdms", [False, True])
@pytest.mark.parametrize("ncas,na,nb,kind", [(4, 2, 1, "uccsd"), (4, 2, 1, "fabric")])
def test_circuit_hessian(ncas, na, nb, kind, by_rdms):
    sec, gates, n_theta, occ, init = case(ncas, na, nb, kind)
    eng = engine(ncas, na, nb, kind)
    theta = np.random.default_rng(ncas + n_theta).uniform(0, 2 * np.pi, n_theta)
    c1, c2 = S.coefficients(ncas, 41)
    H = eng.circuit_hessian(dev(theta[None]), gates, dev(c1), dev(c2), by_rdms=by_rdms).cpu().numpy()
    ref = S.hessian(gates, theta, sec, init, c1, c2, n_theta)
    record("hessian", f"a{ncas} ({na},{nb}) {kind} by_rdms={by_rdms}", np.abs(H - ref),
           S.hessian_bound(sec, gates, n_theta, theta, init, c1, c2, by_rdms))


# ---- bit equality ---------------------------------------------------------------------------------------------------
def _same_bits(run, vecs, small, large, what):
    """state b of a batch = the same state in another batch, elsewhere in it (``small`` and ``large`` states)."""
    n = vecs.shape[0]
    perm = np.random.default_rng(large).permutation(large) % n
    a = [t.cpu().numpy() for t in run(dev(vecs[np.arange(small) % n]))]
    b = [t.cpu().numpy() for t in run(dev(vecs[perm]))]
    for x, y in zip(a, b):
        for pos, i in enumerate(perm):
            if i < small:
                assert np.array_equal(y[pos], x[i]), (what, pos, i)


def test_bit_equality_across_batches_and_positions():
    """The sums of a state do not depend on its neighbours: the same state alone, in a batch, and at another place of
    a permuted batch gives the same bits -- compared WITHIN one nsplit, because the number of workgroups that share
    a state's chunks sets the order of its sums (different nsplit: different bits by construction)."""
    n_cu = cus()
    s8, s4, s6 = [next(t for t in S.SECTORS if t[:3] == k) for k in ((8, 4, 3), (4, 2, 1), (6, 3, 2))]
    for s in (s8, s4):
        ncas, na, nb, kind = s[:4]
        sec = twin_sector(ncas, na, nb)
        eng = engine(ncas, na, nb, kind)
        vecs = S.make_vectors(sec, 3, 5)
        c1, c2 = S.coefficients(ncas, 4)
        c1d, c2d = dev(c1), dev(c2)
        # row chunks (forced below their threshold of 16 states) at 1 and 16 states; chunks of 128 at 1 and 15, 16 and 33
        for opt, small, large in (({"sector_rdm_r3": 2}, 1, 16), ({"sector_rdm_r3": 1}, 1, 15),
                                  ({"sector_rdm_r3": 1}, 16, 33), ({"sector_unfused": 1}, 4, 7),
                                  ({"sector_unfused": 1}, 16, 31)):
            r = [S.rdm_route(ncas, sec.na, sec.nb, b, n_cu, opt.get("sector_unfused", 0), opt.get("sector_rdm_r3", 0))
                 for b in (small, large)]
            r = [[k.replace("epq_rows", "epq") for k in x] for x in r]     # (the two E_pq kernels: the same sums)
            if r[0] != r[1]:
                print(f"{S.sector_id(s)} {opt}: batches {small} and {large} take {r[0]} and {r[1]} on {n_cu} CUs:"
                      " not compared")
                continue
            with debug_options(**opt):
                _same_bits(eng.rdms, vecs, small, large, (S.sector_id(s), opt))
        # the string-driven lambda (forced below its threshold of 32 states) and W in memory, each on both sides
        for opt, small, large in (({"sector_lambda_w": 2}, 1, 32), ({"sector_lambda_w": 1}, 1, 15),
                                  ({"sector_lambda_w": 1}, 33, 40)):
            r = [S.lam_route(ncas, sec.na, sec.nb, b, n_cu, opt.get("sector_unfused", 0), opt.get("sector_lambda_w", 0))
                 for b in (small, large)]
            if r[0] != r[1]:
                print(f"{S.sector_id(s)} {opt}: batches {small} and {large} take {r[0]} and {r[1]} on {n_cu} CUs:"
                      " not compared")
                continue
            with debug_options(**opt):
                _same_bits(lambda v: (eng.lam(v, c1d, c2d),), vecs, small, large, (S.sector_id(s), opt))
        eng._work.clear()
    # the Gram from V in memory (6 orbitals): both kernels, within one nsplit each
    ncas, na, nb, kind = s6[:4]
    sec = twin_sector(ncas, na, nb)
    eng = engine(ncas, na, nb, kind)
    vecs = S.make_vectors(sec, 3, 5)
    for small, large in ((1, 3), (4, 7), (8, 15), (16, 31)):
        _same_bits(eng.rdms, vecs, small, large, ("a6", small, large))
    # the pair-list sweeps: one workgroup per state whatever the batch
    for s in (s8, s6):
        ncas, na, nb, kind = s[:4]
        sec, gates, n_theta, occ, init = case(ncas, na, nb, kind)
        eng = engine(ncas, na, nb, kind)
        thetas = np.random.default_rng(8).uniform(0, 2 * np.pi, (5, n_theta))
        _same_bits(lambda t: (eng.state(t),), thetas, 1, 7, "state_pl")
        spec = [(-1, -1), (0, -1), (0, 1)]
        _same_bits(lambda t: (eng.derivative_states(t, spec),), thetas, 1, 7, "deriv_pl")
        if ncas != 8:
            continue          # (below 8 orbitals lam goes through the general contraction kernels: not this file's)
        c1, c2 = S.coefficients(ncas, 4)
        big = eng.state(dev(thetas[np.arange(7) % 5]))
        d_big = eng.adjoint(dev(thetas[np.arange(7) % 5]), big, dev(c1), dev(c2))
        d_one = eng.adjoint(dev(thetas[3:4]), big[3:4].contiguous(), dev(c1), dev(c2))
        assert S.lam_route(ncas, sec.na, sec.nb, 1, n_cu) == S.lam_route(ncas, sec.na, sec.nb, 7, n_cu)
        assert torch.equal(d_big[3], d_one[0])


# ---- refusals before any launch -----------------------------------------------------------------------------------
def _raw_engine(ncas, na_el, nb_el):
    """string tables on the device without an engine's pair lists (shapes the engine itself would refuse)."""
    ua, ra = sector_mod.string_tables(ncas, na_el)
    ub, rb = sector_mod.string_tables(ncas, nb_el)
    t = [dev(ua.astype(np.int32), torch.int32), dev(ub.astype(np.int32), torch.int32), dev(ra, torch.int32),
         dev(rb, torch.int32)]
    return t, [dptr(x, torch.int32) for x in t] + [len(ua), len(ub)]


def test_refusals_leave_every_output_untouched():
    lib = _lib.load()

    def entries(ncas, tabs, na, nb, gates, n_theta, pairs, max_pairs, want, batch=2):
        """the entry points named in ``want``, once each (and no other: a call that is not refused would run): all must be
        refused, with every output and the workspace (full size) still NaN."""
        Dc, a = na * nb, ncas
        gd = torch.as_tensor(X.gates_to_numpy(gates)).to(DEV)
        th, psi = dev(np.zeros((batch, n_theta))), dev(np.zeros((batch, Dc)))
        c1, c2 = dev(np.zeros((a, a))), dev(np.zeros((a,) * 4))
        work = nan(int(lib.oovqe_sector_work_size(a, na, nb, batch)))
        spec = dev(np.array([[-1, -1]], dtype=np.int32), torch.int32)
        pp = dptr(pairs, torch.int32)
        g8, ng, init = dptr(gd, torch.uint8), len(gates), ctypes.c_uint32(0)
        o = {"state": [nan(batch, Dc)], "state_pl": [nan(batch, Dc)], "deriv": [nan(batch, Dc)],
             "deriv_pl": [nan(batch, Dc)], "rdms": [nan(batch, a, a), nan(batch, a ** 4)],
             "adjoint": [nan(batch, n_theta)], "adjoint_pl": [nan(batch, n_theta)], "lam": [nan(batch, Dc)]}
        calls = {
            "state": lambda: lib.oovqe_sector_state(dptr(th), n_theta, g8, ng, a, init, *tabs, batch,
                                                    dptr(o["state"][0]), None, stream_ptr()),
            "state_pl": lambda: lib.oovqe_sector_state_pl(dptr(th), n_theta, g8, ng, a, init, *tabs, batch, pp,
                                                          max_pairs, dptr(o["state_pl"][0]), None, stream_ptr()),
            "deriv": lambda: lib.oovqe_sector_state_deriv(dptr(th), n_theta, g8, ng, a, init, *tabs, batch,
                                                          dptr(spec, torch.int32), 1, dptr(o["deriv"][0]),
                                                          stream_ptr()),
            "deriv_pl": lambda: lib.oovqe_sector_state_deriv_pl(dptr(th), n_theta, g8, ng, a, init, *tabs, batch, pp,
                                                                max_pairs, dptr(spec, torch.int32), 1,
                                                                dptr(o["deriv_pl"][0]), stream_ptr()),
            "rdms": lambda: lib.oovqe_sector_rdms(dptr(psi), a, *tabs, batch, dptr(o["rdms"][0]), dptr(o["rdms"][1]),
                                                  dptr(work), stream_ptr()),
            "adjoint": lambda: lib.oovqe_sector_adjoint(dptr(th), n_theta, g8, ng, a, *tabs, batch, dptr(psi), dptr(c1),
                                                        dptr(c2), dptr(work), dptr(o["adjoint"][0]), stream_ptr()),
            "adjoint_pl": lambda: lib.oovqe_sector_adjoint_pl(dptr(th), n_theta, g8, ng, a, *tabs, batch, dptr(psi),
                                                              dptr(c1), dptr(c2), pp, max_pairs, None, dptr(work),
                                                              dptr(o["adjoint_pl"][0]), stream_ptr()),
            "lam": lambda: lib.oovqe_sector_lambda(dptr(psi), a, *tabs, batch, dptr(c1), dptr(c2), None, dptr(work),
                                                   dptr(o["lam"][0]), stream_ptr()),
        }
        for name in want:
            assert calls[name]() != 0, name
        torch.cuda.synchronize()
        for name in want:
            assert all(torch.isnan(t).all() for t in o[name]), name
        assert torch.isnan(work).all()

    SWEEPS = ("state", "state_pl", "deriv", "deriv_pl", "adjoint", "adjoint_pl")
    dummy_pairs = torch.zeros(64, dtype=torch.int32, device=DEV)
    # 14 orbitals: past the documented limit on every entry
    _, tabs = _raw_engine(14, 1, 1)
    gates, n_theta = S.ladder_gates(14)
    entries(14, tabs, 14, 14, gates, n_theta, dummy_pairs, 1, SWEEPS + ("rdms", "lam"))
    # more than 32 767 determinants with pair lists (13 orbitals, 286 x 286), and the lists themselves
    _, tabs = _raw_engine(13, 3, 3)
    gates, n_theta = S.ladder_gates(13)
    entries(13, tabs, 286, 286, gates, n_theta, dummy_pairs, 1, SWEEPS)
    out = torch.full((64,), -7, dtype=torch.int32, device=DEV)
    gd = torch.as_tensor(X.gates_to_numpy(gates)).to(DEV)
    assert lib.oovqe_sector_pairs(dptr(gd, torch.uint8), len(gates), 13, *tabs, dptr(out, torch.int32),
                                  stream_ptr()) != 0
    assert int(lib.oovqe_sector_pairs_size(len(gates), 286, 286)) > 0 and (out == -7).all()
    # sectors whose LDS formula passes 160 KB: 286 x 78 for the pair-list states (178 KB), 126 x 126 for the gate
    # sweeps and both reverse sweeps (two vectors: 254 KB)
    _, tabs = _raw_engine(13, 3, 2)
    entries(13, tabs, 286, 78, gates, n_theta, dummy_pairs, 1, SWEEPS)
    _, tabs = _raw_engine(9, 4, 4)
    gates, n_theta = S.ladder_gates(9)
    entries(9, tabs, 126, 126, gates, n_theta, dummy_pairs, 1, ("state", "deriv", "adjoint", "adjoint_pl"))
    # null pointers, one argument at a time, and a batch that is no multiple of the group
    s = next(t for t in S.SECTORS if t[:3] == (4, 2, 1))
    eng = engine(*s[:4])
    sec = twin_sector(4, 2, 1)
    pairs, max_pairs = eng.pair_lists()
    th, psi = dev(np.zeros((2, eng.n_theta))), dev(np.zeros((2, sec.Dc)))
    c1, c2 = dev(np.zeros((4, 4))), dev(np.zeros((4,) * 4))
    g8, init = dptr(eng.gates_dev, torch.uint8), ctypes.c_uint32(eng.init_index)
    o1, o2, o3 = nan(2, sec.Dc), nan(2, 4, 4), nan(2, 256)
    work = eng.work(2)
    tb = list(eng._tabs())
    for i in range(4):
        bad = tb[:i] + [None] + tb[i + 1:]
        assert lib.oovqe_sector_state_pl(dptr(th), eng.n_theta, g8, eng.n_gates, 4, init, *bad, 2,
                                         dptr(pairs, torch.int32), max_pairs, dptr(o1), None, stream_ptr()) != 0
        assert lib.oovqe_sector_rdms_tb(dptr(psi), 4, *bad, 2, eng._tables_ptr, dptr(o2), dptr(o3), dptr(work),
                                        stream_ptr()) != 0
        assert lib.oovqe_sector_lambda(dptr(psi), 4, *bad, 2, dptr(c1), dptr(c2), eng._tables_ptr, dptr(work), dptr(o1),
                                       stream_ptr()) != 0
    assert lib.oovqe_sector_state_pl(None, eng.n_theta, g8, eng.n_gates, 4, init, *tb, 2, dptr(pairs, torch.int32),
                                     max_pairs, dptr(o1), None, stream_ptr()) != 0
    assert lib.oovqe_sector_state_pl(dptr(th), eng.n_theta, None, eng.n_gates, 4, init, *tb, 2,
                                     dptr(pairs, torch.int32), max_pairs, dptr(o1), None, stream_ptr()) != 0
    assert lib.oovqe_sector_rdms_tb(None, 4, *tb, 2, eng._tables_ptr, dptr(o2), dptr(o3), dptr(work), stream_ptr()) != 0
    assert lib.oovqe_sector_rdms_tb(dptr(psi), 4, *tb, 2, eng._tables_ptr, dptr(o2), dptr(o3), None, stream_ptr()) != 0
    assert lib.oovqe_sector_lambda(dptr(psi), 4, *tb, 2, None, dptr(c2), eng._tables_ptr, dptr(work), dptr(o1),
                                   stream_ptr()) != 0
    assert lib.oovqe_sector_lambda(dptr(psi), 4, *tb, 2, dptr(c1), dptr(c2), eng._tables_ptr, dptr(work), None,
                                   stream_ptr()) != 0
    wide, c1view, stride, cs = _geometry_rows(4, 2, 1)
    v3, out3 = dev(np.zeros((3, sec.Dc))), nan(3, sec.Dc)
    assert _lam_pg(eng, v3, 2, c1view, stride, out3) != 0          # 3 states in groups of 2
    assert _lam_pg(eng, v3, 0, c1view, stride, out3) != 0
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in (o1, o2, o3, out3))


# ---- the public route -----------------------------------------------------------------------------------------------
def test_odd_electron_circuit_through_the_public_classes():
    """Parameterized_circuit(6, 5): 3 alpha and 2 beta electrons, 20 x 15 determinants, 12 qubits: the sector engine."""
    import auto_oo_amd as aoo
    from oracle import cpu_ref as R
    ncas, nelecas = 6, 5
    pqc = aoo.Parameterized_circuit(ncas, nelecas, None, ansatz="ucc")
    assert pqc._use_sector and (pqc._sector.n_alpha, pqc._sector.n_beta) == (3, 2)
    sec = twin_sector(6, 3, 2)
    gates, n_theta = X.uccd_gates(ncas, nelecas, False)
    init = X.basis_index(X.hf_state(nelecas, 2 * ncas))
    theta = np.random.default_rng(65).uniform(0, 2 * np.pi, n_theta)
    psi = S.apply_gates(gates, theta, sec, init)[0]
    es = S.state_bound(gates)

    def rdm_bound(v, dv):
        """the bound of the RDMs of the exact vector, plus what an input error of 2-norm dv does to a quadratic form
        whose operators have norm <= 2 (E_pq) and <= 4 + 2 (E_qp^T E_rs and the delta term)."""
        b1, b2 = S.rdm_bounds(sec, v)
        nv = np.linalg.norm(v)
        return b1 + 2 * (2 * nv * dv + dv * dv), b2 + 6 * (2 * nv * dv + dv * dv)

    g1, g2 = pqc.get_rdms(torch.tensor(theta))
    r1, r2 = sec.rdms(psi)
    b1, b2 = rdm_bound(psi, es)
    record("public", "get_rdms gamma", np.abs(g1.cpu().numpy() - r1), b1)
    record("public", "get_rdms Gamma", np.abs(g2.cpu().numpy() - r2), b2)
    d1, d2 = pqc.rdms_with_derivatives(torch.tensor(theta))
    d1, d2 = d1.cpu().numpy(), d2.cpu().numpy()
    record("public", "derivatives set 0", np.abs(d1[0] - r1), b1)
    for k in range(n_theta):
        tau = S.tangent(gates, theta, sec, init, k, n_theta)
        # d gamma_pq = tau . V_pq(psi) + psi . V_pq(tau), d Gamma likewise: the bilinear form, not the polarisation
        Vp, Vt = sec.apply_epq(psi), sec.apply_epq(tau)
        a = ncas
        t1 = (Vp @ tau + Vt @ psi).reshape(a, a)
        sw = lambda V: V.reshape(a, a, -1).transpose(1, 0, 2).reshape(a * a, -1)
        t2 = (sw(Vt) @ Vp.T + sw(Vp) @ Vt.T).reshape(a, a, a, a)
        for q in range(a):
            t2[:, q, q, :] -= t1
        bp, bm = rdm_bound(psi + tau, 2 * es + S.U * 2), rdm_bound(psi - tau, 2 * es + S.U * 2)
        record("public", f"d gamma / d theta_{k}", np.abs(d1[1 + k] - t1), 0.5 * (bp[0] + bm[0]) + S.U * np.abs(t1))
        record("public", f"d Gamma / d theta_{k}", np.abs(d2[1 + k] - t2), 0.5 * (bp[1] + bm[1]) + S.U * np.abs(t2))
    # OO_pqc: energy and circuit gradient against the twin's energy and its central differences
    N, nelec = 13, 15
    P = R.synthetic_problem(N, 20265)
    mol = aoo.Moldata(P["int1e_ao"], P["int2e_ao"], P["overlap"], P["nuc"], nelec)
    oo = aoo.OO_pqc(pqc, mol, ncas, nelecas, oao_mo_coeff=P["oao_mo_coeff"])
    omol = R.OracleMol(P["int1e_ao"], P["int2e_ao"], P["overlap"], P["nuc"], nelec)
    ooo = R.OracleOOEnergy(omol, ncas, nelecas, P["oao_mo_coeff"])

    def energy(t):
        q1, q2 = sec.rdms(S.apply_gates(gates, t, sec, init)[0])
        return float(ooo.energy_from_mo_coeff(ooo.mo_coeff, torch.tensor(q1), torch.tensor(q2)))

    E, grad = oo.energy_and_gradient(torch.tensor(theta))
    e_ref = energy(theta)
    # 1e-9 and 1e-8: what the suite's smoke test asks of the energy and the gradient of this pipeline at this N
    print(f"public: E {E.item():.12f}, twin {e_ref:.12f}, error {abs(E.item() - e_ref):.2e}, bound 1e-9")
    assert abs(E.item() - e_ref) <= 1e-9
    h = 1e-4
    gd = grad.cpu().numpy()[:n_theta]
    for k in range(n_theta):
        e = np.zeros(n_theta)
        e[k] = 1.0
        # one Givens pass per parameter: psi is linear in cos, sin of theta_k / 2, so E = a + b cos theta_k +
        # c sin theta_k along the line and its third derivative is at most the amplitude hypot(b, c), read from three
        # points of the twin: central differences are off by h^2 / 6 of it, plus the twin's own rounding (1e-12 at
        # |E| ~ 30) twice over h
        e_half, e_pi = energy(theta + 0.5 * np.pi * e), energy(theta + np.pi * e)
        amp = np.hypot(e_ref - 0.5 * (e_ref + e_pi), e_half - 0.5 * (e_ref + e_pi))
        fd = (energy(theta + h * e) - energy(theta - h * e)) / (2 * h)
        bound = h * h / 6 * amp + 2e-12 / h + 1e-8
        print(f"public: dE/dtheta_{k} {gd[k]:+.10f}, central difference {fd:+.10f}, error {abs(gd[k] - fd):.2e}, "
              f"bound {bound:.2e}")
        assert abs(gd[k] - fd) <= bound


def test_figures_summary():
    for group, ratio in sorted(FIGURES.items()):
        print(f"largest error / bound, {group}: {ratio:.3f}")
