"""Overlaps between the states of a geometry stack on the device: the cross overlap against its host twin, the sector
kernel against the host route of berry.py and the brute-force reference of tests/_overlaps.py, the batch's calls in both
metrics, the recorded notebook loop, root tracking end to end, and the errors of the interface.

Bounds.  Cross overlap: the bound tests/test_gto_d_gpu.py gives the overlap (6.3e-13).  Sector kernel: 1e-12 max(1,
|reference|).  Exact metric: 10 x the disagreement of the two host forms (whole-block determinants against the core
fold) on the case, floor 1e-13.  Measured on the MI355X ("Overlaps between geometries")."""
import functools
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import auto_oo_amd as aoo                                            # noqa: E402
from auto_oo_amd import gaussian, gto, overlaps                       # noqa: E402
from auto_oo_amd.berry import ActiveSpaceRotation, bogoliubov_atob_cas, sector_tables, state_overlap   # noqa: E402
from auto_oo_amd.moldata import get_formal_geo                        # noqa: E402
from auto_oo_amd.sector import sector_of                              # noqa: E402
from auto_oo_amd.synthetic import synthetic_problem                   # noqa: E402
from tests import _gto_d as D                                         # noqa: E402
from tests import _overlaps as V                                      # noqa: E402
from tests import _replay as P                                        # noqa: E402

F64 = torch.float64
BOHR = gaussian.BOHR
TOL_S = 6.3e-13                # tests/test_gto_d_gpu.py: the overlap against the host integrals


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def to_dev(x, dtype=F64):
    return torch.as_tensor(np.ascontiguousarray(x)).to(device=dev(), dtype=dtype)


def _sector(ncas, nelecas):
    return sector_of([1 if i < nelecas else 0 for i in range(2 * ncas)], ncas)


# ---- 1. cross overlap ------------------------------------------------------------------------------------------------------
def _cross_case(name):
    if name == "formaldimine":
        basis = gto.GTOBasis(["N", "C", "H", "H", "H"])
        pts = basis.coordinates([get_formal_geo(130.0, 85.0), get_formal_geo(127.0, 92.0)])
        return basis, np.stack([pts[0], pts[0]]), np.stack([pts[0], pts[1]])
    basis = D.m1_basis(name)
    xa = np.stack([D.M1_XYZ, D.M1_XYZ, D.M1_XYZ])
    xb = np.stack([D.M1_XYZ, D.M1_XYZ + np.array([0.05, 0.0, 0.0]), D.M1_MOVED])
    return basis, xa, xb


@pytest.mark.parametrize("name", ["spherical", "cartesian", "formaldimine"])
def test_cross_overlap_against_the_host_twin(name):
    basis, xa, xb = _cross_case(name)
    form = basis.d_functions or "spherical"
    got_dev = gto.cross_overlap_batch(basis, xa, xb)
    got = got_dev.cpu().numpy()
    assert got.shape == (len(xa), basis.nao, basis.nao) and np.isfinite(got).all()
    for p in range(len(xa)):
        ref = gaussian.cross_overlap_from_table(basis.table, xa[p] / BOHR, xb[p] / BOHR, form)
        err = np.abs(got[p] - ref).max()
        print(f"cross overlap {name} pair {p}: {err:.2e}")
        assert err < TOL_S
    # the pair (g, g) is the overlap of the geometry
    S = gto.integrals_batch(basis, xa[:1]).overlap[0].cpu().numpy()
    err = np.abs(got[0] - S).max()
    print(f"cross overlap {name} (g, g) against overlap: {err:.2e}")
    assert err < TOL_S
    # bits: a pair alone, at another place in the list, on another stream
    last = len(xa) - 1
    alone = gto.cross_overlap_batch(basis, xa[last:], xb[last:])
    assert torch.equal(alone[0], got_dev[last])
    order = list(range(len(xa)))[::-1]
    moved = gto.cross_overlap_batch(basis, xa[order], xb[order])
    assert torch.equal(moved[0], got_dev[last]) and torch.equal(moved[last], got_dev[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = gto.cross_overlap_batch(basis, xa, xb)
    side.synchronize()
    assert torch.equal(other, got_dev)
    # S_ab(a, b) = S_ab(b, a)^T
    back = gto.cross_overlap_batch(basis, xb, xa).cpu().numpy()
    assert np.abs(back.transpose(0, 2, 1) - got).max() < TOL_S


# ---- 2. the sector kernel against the host route ----------------------------------------------------------------------------
KINDS = ("orthogonal", "improper", "nonorthogonal", "permutation")


@pytest.mark.parametrize("orthogonalize", [False, "givens"], ids=["plain", "givens"])
@pytest.mark.parametrize("ncas,nelecas", [(2, 2), (3, 4), (3, 2), (4, 4), (6, 6), (8, 8)])
def test_sector_kernel_against_the_host_route(ncas, nelecas, orthogonalize):
    na_, nb_ = _sector(ncas, nelecas)
    mats = V.trial_matrices(ncas, 10 * ncas + nelecas)
    U = np.stack([mats[k] for k in KINDS])
    rots = [ActiveSpaceRotation(u, ncas, na_, nb_, orthogonalize=orthogonalize) for u in U]
    x = sector_tables(ncas, na_, nb_)[2].reshape(-1)
    Dc, Dfull = x.size, 1 << (2 * ncas)
    rng = np.random.default_rng(ncas + nelecas)
    index = overlaps.dense_index(ncas, na_, nb_, dev())
    assert np.array_equal(index.cpu().numpy(), x)
    worst = 0.0
    for (rb, rk), signed, dense in itertools.product([(1, 1), (4, 3)], [True, False], [False, True]):
        bra = rng.standard_normal((len(U), rb, Dc)) / np.sqrt(Dc)
        ket = rng.standard_normal((len(U), rk, Dc)) / np.sqrt(Dc)
        ref = np.stack([V.contract(r.M_alpha, r.M_beta, r.sign, bra[p], ket[p], signed) for p, r in enumerate(rots)])
        if dense:
            b, k = np.zeros((len(U), rb, Dfull)), np.zeros((len(U), rk, Dfull))
            b[:, :, x], k[:, :, x] = bra, ket
        else:
            b, k = bra, ket
        args = (ncas, na_, nb_)
        kw = dict(orthogonalize=orthogonalize, signed=signed, index=index if dense else None)
        out, core = overlaps.sector_overlaps(to_dev(U), 0, *args, to_dev(b), to_dev(k), **kw)
        assert out.shape == (len(U), rb, rk) and torch.equal(core, torch.ones_like(core))
        got = out.cpu().numpy()
        for p, kind in enumerate(KINDS):
            scale = max(1.0, np.abs(ref[p]).max())
            err = np.abs(got[p] - ref[p]).max() / scale
            worst = max(worst, err)
            assert err < 1e-12, (kind, rb, rk, signed, dense, err)
        # bits under a permutation of the pair list
        order = [2, 0, 3, 1]
        again, _ = overlaps.sector_overlaps(to_dev(U[order]), 0, *args, to_dev(b[order]), to_dev(k[order]), **kw)
        assert torch.equal(again, out[order])
    print(f"sector kernel ({ncas}, {nelecas}) {orthogonalize}: worst {worst:.2e}")


@pytest.mark.parametrize("n_core", [0, 2, 5])
@pytest.mark.parametrize("ncas,nelecas", [(2, 2), (3, 4), (3, 2), (4, 4)])
def test_sector_kernel_core_fold_against_brute_force(ncas, nelecas, n_core):
    na_, nb_ = _sector(ncas, nelecas)
    m = n_core + ncas
    rng = np.random.default_rng(100 * n_core + 10 * ncas + nelecas)
    s = np.stack([np.eye(m) + 0.2 * rng.standard_normal((m, m)) for _ in range(3)])
    Dc = sector_tables(ncas, na_, nb_)[2].size
    bra, ket = rng.standard_normal((3, 2, Dc)), rng.standard_normal((3, 3, Dc))
    out, core = overlaps.sector_overlaps(to_dev(s), n_core, ncas, na_, nb_, to_dev(bra), to_dev(ket))
    got = (out * (core * core)[:, None, None]).cpu().numpy()
    for p in range(3):
        ref = V.brute_force(s[p], n_core, ncas, na_, nb_, bra[p], ket[p])
        det = np.linalg.det(s[p][:n_core, :n_core]) if n_core else 1.0
        assert abs(core[p].item() - det) < 1e-12 * max(1.0, abs(det))
        err = np.abs(got[p] - ref).max() / max(1.0, np.abs(ref).max())
        print(f"core fold ({ncas}, {nelecas}) n_core {n_core} pair {p}: {err:.2e}")
        assert err < 1e-12


# ---- 3. state_overlaps(metric="oao") against the loop of berry.py ------------------------------------------------------------
def _synthetic_batch(ansatz, ncas, nelecas, G, **kw):
    N, nelec = 13, 16
    pqc = aoo.Parameterized_circuit(ncas, nelecas, None, ansatz=ansatz, **kw)
    probs = [synthetic_problem(N, 9100 + g) for g in range(G)]
    mols = [aoo.Moldata(p["int1e_ao"], p["int2e_ao"], p["overlap"], p["nuc"], nelec) for p in probs]
    batch = aoo.OO_pqc_batch(pqc, mols, ncas, nelecas, oao_mo_coeffs=[p["oao_mo_coeff"] for p in probs])
    rng = np.random.default_rng(3)
    thetas = to_dev(rng.uniform(-0.6, 0.6, (G, batch.n_theta)))
    return pqc, batch, thetas


@pytest.mark.parametrize("ansatz,ncas,nelecas,G,kw", [("ucc", 3, 4, 4, {}), ("kupccd", 6, 6, 2, {"k": 1})],
                         ids=["ucc-dense", "kupccd-sector"])
def test_state_overlaps_oao_against_the_loop_of_berry(ansatz, ncas, nelecas, G, kw):
    pqc, batch, thetas = _synthetic_batch(ansatz, ncas, nelecas, G, **kw)
    assert bool(getattr(pqc, "_use_sector", False)) == (ansatz == "kupccd")
    pairs = [(g, (g + 1) % G) for g in range(G)] + [(0, 0), (G - 1, 0)]
    got = batch.state_overlaps(thetas, pairs=np.array(pairs), metric="oao").cpu().numpy()
    loop = batch.state_overlaps(thetas, metric="oao").cpu().numpy()
    assert np.array_equal(loop, got[:G])
    states = [pqc.state_real(thetas[g]) for g in range(G)]
    orb = batch.oao_mo_coeff.cpu().numpy()
    for (a, b), val in zip(pairs, got):
        rot = bogoliubov_atob_cas(orb[a].T @ orb[b], batch.act_idx, nelecas)
        ref = state_overlap(states[b], rot, states[a]).item()
        print(f"oao overlap {ansatz} pair ({a}, {b}): {val:+.12f} against {ref:+.12f}")
        assert abs(val - ref) < 1e-12
    W, o = batch.berry_phase(thetas)
    assert np.array_equal(o.cpu().numpy(), loop) and abs(W.item() - np.prod(loop)) < 1e-14


# ---- 4. the recorded notebook loop ---------------------------------------------------------------------------------------------
def test_the_recorded_berry_phase_loop_from_one_call():
    run = P.RUNS["tutorial_berry_phase"]
    pqc = aoo.Parameterized_circuit(run["ncas"], run["nelecas"], None, ansatz=run["ansatz"], n_layers=run["n_layers"])

    def make(mol, oao_mo_coeff):
        return aoo.OO_pqc(pqc, mol, run["ncas"], run["nelecas"], oao_mo_coeff=oao_mo_coeff,
                          freeze_active=run["freeze_active"])
    out = P.berry_loop(make, aoo.NewtonStep(verbose=0), run, dev())
    states = [pqc.state_real(t) for t in out["thetas"]]
    n = len(states)
    nxt = [(i + 1) % n for i in range(n)]
    ovl = overlaps.state_overlaps_oao([states[j] for j in nxt], states, out["orbitals"],
                                      [out["orbitals"][j] for j in nxt], out["act_idx"], run["nelecas"])
    ovl = ovl.cpu().numpy()
    assert ovl.shape == (n,) and n == len(run["overlaps"]) + 1
    assert np.abs(ovl[:-1] - np.array(run["overlaps"])).max() < 5e-7
    assert abs(ovl[-1] - run["final_overlap"]) < 5e-7 and ovl[-1] < -0.99
    # the same loop as a batch: berry_phase
    basis = gto.GTOBasis(["N", "C", "H", "H", "H"])
    coords = basis.coordinates([get_formal_geo(*p) for p in P.loop_points(run)])
    batch = aoo.OO_pqc_batch.from_geometries(pqc, basis, coords, run["ncas"], run["nelecas"],
                                             oao_mo_coeffs=out["orbitals"], freeze_active=run["freeze_active"])
    W, o = batch.berry_phase(torch.stack([t.reshape(-1) for t in out["thetas"]]))
    assert np.abs(o.cpu().numpy() - ovl).max() < 1e-12
    assert W.item() < 0


# ---- 5. exact metric --------------------------------------------------------------------------------------------------------------
def _exact_case(name):
    """(basis, two geometries in Angstrom, ncas, nelecas)"""
    if name == "h2":
        return gto.GTOBasis(["H", "H"], V.H2_TABLE), np.stack([V.H2_XYZ, V.H2_XYZ_2]), 2, 2
    if name == "water":
        return gto.GTOBasis(["O", "H", "H"]), np.stack([D.WATER, D.WATER_2]), 3, 4
    return D.m2_basis(), np.stack([D.WATER, D.WATER_2]), 3, 4


@functools.lru_cache(maxsize=None)
def _exact_batch(name):
    basis, xyz, ncas, nelecas = _exact_case(name)
    pqc = aoo.Parameterized_circuit(ncas, nelecas, None, ansatz="ucc")
    return pqc, aoo.OO_pqc_batch.from_geometries(pqc, basis, xyz, ncas, nelecas, oao_mo_coeffs="rhf")


PAIRS = np.array([[0, 1], [1, 0], [0, 0], [1, 1]])


@pytest.mark.parametrize("name", ["h2", "water", "m2"])
def test_exact_overlaps_against_brute_force(name):
    basis, xyz, ncas, nelecas = _exact_case(name)
    pqc, batch = _exact_batch(name)
    n_core, M = batch._n_occ, batch._n_occ + ncas
    na_, nb_ = _sector(ncas, nelecas)
    C = batch.mo_coeff.cpu().numpy()
    thetas = to_dev(np.random.default_rng(5).uniform(-0.5, 0.5, (2, batch.n_theta)))
    e, vecs, O = batch.casci_overlaps(nroots=2, pairs=PAIRS)
    ovl = batch.state_overlaps(thetas, pairs=PAIRS, metric="ao").cpu().numpy()
    O, v = O.cpu().numpy(), vecs.cpu().numpy()
    assert e.shape == (2, 2) and O.shape == (4, 2, 2) and ovl.shape == (4,)
    x = sector_tables(ncas, na_, nb_)[2].reshape(-1)
    psi = np.stack([pqc.state_real(thetas[g]).cpu().numpy()[x] for g in range(2)])
    for p, (a, b) in enumerate(PAIRS):
        s = V.host_s(basis, xyz[a], xyz[b], C[a], C[b], M)
        for what, bra, ket, got in (("casci", v[a], v[b], O[p]), ("state", psi[a:a + 1], psi[b:b + 1], ovl[p:p + 1])):
            brute = V.brute_force(s, n_core, ncas, na_, nb_, bra, ket)
            fold, det = V.core_fold(s, n_core, ncas, na_, nb_, bra, ket)
            yard = np.abs(det * det * fold - brute).max()
            tol = max(10 * yard, 1e-13)
            err = np.abs(np.asarray(got).reshape(brute.shape) - brute).max()
            print(f"exact {name} {what} pair ({a}, {b}): error {err:.2e}, host forms disagree by {yard:.2e}, bound {tol:.2e}")
            assert err < tol
            if a == b:
                assert np.abs(np.asarray(got).reshape(brute.shape) - np.eye(len(bra))).max() < tol
    # O(a, b) = O(b, a)^T
    assert np.abs(O[0] - O[1].T).max() < 1e-13 and abs(ovl[0] - ovl[1]) < 1e-13


def test_exact_overlaps_do_not_see_a_common_translation():
    basis, xyz, ncas, nelecas = _exact_case("water")
    pqc, base = _exact_batch("water")
    orb = list(base.oao_mo_coeff.cpu().numpy())
    stack = np.concatenate([xyz, xyz + D.SHIFT])
    batch = aoo.OO_pqc_batch.from_geometries(pqc, basis, stack, ncas, nelecas, oao_mo_coeffs=orb + orb)
    thetas = to_dev(np.random.default_rng(5).uniform(-0.5, 0.5, (2, batch.n_theta))).repeat(2, 1)
    vecs = base.casci(nroots=2)[1].repeat(2, 1, 1)
    pairs = np.array([[0, 1], [2, 3]])
    O = batch.casci_overlaps(nroots=2, pairs=pairs, vecs=vecs)[2].cpu().numpy()
    o = batch.state_overlaps(thetas, pairs=pairs, metric="ao").cpu().numpy()
    err = max(np.abs(O[0] - O[1]).max(), abs(o[0] - o[1]))
    print(f"common translation: {err:.2e}")
    assert err < 1e-12


def test_exact_overlaps_under_a_common_rotation_with_rhf_orbitals():
    """|O| is invariant under a rigid rotation of both geometries when the orbitals are recomputed: RHF converged with
    err_tol = 1e-11 as the RHF-gradient test does, so 1e-8 (first order in the orbital residual)."""
    basis, xyz, ncas, nelecas = _exact_case("water")
    pqc, _ = _exact_batch("water")
    stack = np.concatenate([xyz, xyz @ D.ROTATION.T])
    batch = aoo.OO_pqc_batch.from_geometries(pqc, basis, stack, ncas, nelecas, oao_mo_coeffs="rhf")
    res = batch.rhf(conv_tol=1e-13, err_tol=1e-11)
    assert int(res.info.abs().max().item()) == 0
    batch.oao_mo_coeff.copy_(res.oao_mo_coeff)
    batch.refresh_mo_coeff()
    pairs = np.array([[0, 1], [2, 3]])
    O = batch.casci_overlaps(nroots=2, pairs=pairs)[2].abs().cpu().numpy()
    err = np.abs(O[0] - O[1]).max()
    print(f"common rotation: {err:.2e}")
    assert err < 1e-8


# ---- 6. tracking end to end -----------------------------------------------------------------------------------------------------
def test_tracking_repairs_tampered_roots_along_a_path():
    basis = gto.GTOBasis(["O", "H", "H"])
    path = np.stack([D.WATER + t * (D.WATER_2 - D.WATER) for t in (0.0, 1 / 3, 2 / 3, 1.0)])
    pqc = aoo.Parameterized_circuit(3, 4, None, ansatz="ucc")
    batch = aoo.OO_pqc_batch.from_geometries(pqc, basis, path, 3, 4, oao_mo_coeffs="rhf")
    e, vecs = batch.casci(nroots=3)
    _, dip = batch.casci_dipole_matrix(nroots=3)
    e0, v0, O0 = batch.casci_overlaps(nroots=3)
    assert torch.equal(e0, e) and torch.equal(v0, vecs) and O0.shape == (3, 3, 3)
    perm0, sign0 = overlaps.track_roots(O0)
    # tamper: root 1 of geometry 2 changes sign, roots 0 and 1 of geometry 3 change places
    swap = [1, 0, 2]
    vt, et, dt = vecs.clone(), e.clone(), dip.clone()
    vt[2, 1] = -vt[2, 1]
    dt[2, 1, :] = -dt[2, 1, :]
    dt[2, :, 1] = -dt[2, :, 1]
    vt[3], et[3], dt[3] = vecs[3, swap], e[3, swap], dip[3][swap][:, swap]
    none, v1, O1 = batch.casci_overlaps(nroots=3, vecs=vt)
    assert none is None and torch.equal(v1, vt)
    perm, sign = overlaps.track_roots(O1)
    # relative to the tracking of the untampered roots, exactly the tampering comes back
    want_perm, want_sign = perm0.clone(), sign0.clone()
    want_sign[2, (perm0[2] == 1).nonzero()[0, 0]] *= -1
    want_perm[3] = torch.as_tensor(swap, device=perm0.device)[perm0[3]]
    assert torch.equal(perm, want_perm) and torch.equal(sign, want_sign)
    print("tracking of the untampered roots:", perm0.tolist(), sign0.tolist())
    assert torch.equal(overlaps.apply_tracking(et, perm, sign), e)
    assert bool((e[:, 1:] >= e[:, :-1]).all())
    assert torch.equal(overlaps.apply_tracking(vt, perm, sign), overlaps.apply_tracking(vecs, perm0, sign0))
    tracked = overlaps.apply_tracking(dt, perm, sign)
    assert torch.equal(tracked, overlaps.apply_tracking(dip, perm0, sign0))
    # the tracked transition dipoles of neighbouring geometries keep their signs
    t = tracked.cpu().numpy()
    for g in range(3):
        for i, j in ((0, 1), (0, 2), (1, 2)):
            big = (np.abs(t[g, i, j]) > 1e-3) & (np.abs(t[g + 1, i, j]) > 1e-3)
            assert (np.sign(t[g, i, j][big]) == np.sign(t[g + 1, i, j][big])).all()
    # ... which the tampered ones do not
    assert not torch.equal(dt, dip)


# ---- 7. errors, before any launch -----------------------------------------------------------------------------------------------
def test_errors_of_the_interface():
    pqc, batch = _exact_batch("water")
    th = torch.zeros((2, batch.n_theta), dtype=F64)
    with pytest.raises(ValueError, match="rows in 0..1"):
        batch.state_overlaps(th, pairs=[[0, 2]])
    with pytest.raises(ValueError, match="rows in 0..1"):
        batch.casci_overlaps(pairs=[[-1, 0]])
    with pytest.raises(ValueError, match=r"\[P, 2\]"):
        batch.state_overlaps(th, pairs=[[0.5, 1.0]])
    with pytest.raises(ValueError, match="metric"):
        batch.state_overlaps(th, metric="mo")
    with pytest.raises(ValueError, match="ActiveSpaceRotation"):
        batch.state_overlaps(th, orthogonalize="polar")
    with pytest.raises(ValueError, match="ActiveSpaceRotation"):
        batch.state_overlaps(th, metric="oao", orthogonalize="polar")
    with pytest.raises(ValueError):
        batch.casci_overlaps(nroots=2, vecs=torch.zeros((2, 3, 9), dtype=F64))
    p = synthetic_problem(13, 9100)
    host = aoo.OO_pqc_batch(aoo.Parameterized_circuit(3, 4, None, ansatz="ucc"),
                            [aoo.Moldata(p["int1e_ao"], p["int2e_ao"], p["overlap"], p["nuc"], 16)], 3, 4,
                            oao_mo_coeffs=[p["oao_mo_coeff"]])
    th1 = torch.zeros((1, host.n_theta), dtype=F64)
    with pytest.raises(RuntimeError, match="from_geometries"):
        host.state_overlaps(th1, metric="ao")
    with pytest.raises(RuntimeError, match="from_geometries"):
        host.casci_overlaps()
    with pytest.raises(RuntimeError, match="from_geometries"):
        host.berry_phase(th1, metric="ao")
    assert abs(host.state_overlaps(th1, metric="oao").item() - 1.0) < 1e-12           # (any batch serves "oao")
    z = torch.zeros((1, 9, 9), dtype=F64, device=dev())
    v = torch.zeros((1, 1, 9), dtype=F64, device=dev())
    with pytest.raises(ValueError, match="ncas = 9"):
        overlaps.sector_overlaps(z, 0, 9, 2, 2, v, v)
    with pytest.raises(ValueError, match="length"):
        overlaps.sector_overlaps(z[:, :3, :3], 0, 3, 2, 2, v, v[:, :, :8])
    with pytest.raises(ValueError, match="complex"):
        overlaps.state_overlaps_oao(v[:, 0].to(torch.complex128), v[:, 0], z, z, [0, 1, 2], 4)
