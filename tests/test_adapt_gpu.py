"""ADAPT-VQE on the device: the pool-gradient kernel (csrc/pool.hip) against the host twin of tests/_adapt.py, the Python
entry points against the route that existed before (a circuit per candidate, ``circuit_gradient``), the behaviour of a
stack (``OO_pqc_batch.pool_gradients`` / ``set_circuit``), the driver ``adapt_vqe`` and the refusals."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import auto_oo_amd as aoo                                  # noqa: E402
from auto_oo_amd import _lib, adapt, excitations as X      # noqa: E402
from auto_oo_amd._lib import dptr                          # noqa: E402
from auto_oo_amd.oo_energy import mo_ao_to_mo_oao          # noqa: E402
from auto_oo_amd.sector import SectorEngine                # noqa: E402
from tests import _adapt as A                              # noqa: E402

DEV = torch.device("cuda", 0)
F64 = torch.float64
NULL = ctypes.c_void_p(0)


def _t(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float64), device=DEV)


def _engine(ncas, nelecas):
    """the sector tables of CAS(nelecas, ncas) on the device (no circuit: the kernels under test take psi)."""
    return SectorEngine(ncas, X.hf_state(nelecas, 2 * ncas), None, 0, 0, 0, DEV)


def _from_coefficients(eng, pool, psi, c1, c2):
    """oovqe_pool_gradients_from_coefficients_batch on psi [B, Dc], c1 [B, a, a], c2 [B, a, a, a, a]; out prefilled NaN."""
    lib = _lib.load()
    B, a = psi.shape[0], eng.ncas
    c = torch.cat((_t(c1).reshape(B, -1), _t(c2).reshape(B, -1)), dim=1).contiguous()
    pairs, tabs, first, sign = pool.device_tables(eng)
    work = torch.empty(int(lib.oovqe_pool_gradients_from_coefficients_work_size(a, eng.na, eng.nb, B)), dtype=F64,
                       device=DEV)
    out = torch.full((B, len(pool)), float("nan"), dtype=F64, device=DEV)
    psi_d = _t(psi)
    i32 = torch.int32
    rc = lib.oovqe_pool_gradients_from_coefficients_batch(
        dptr(psi_d), a, *eng._tabs(), B, dptr(c), ctypes.c_void_p(c.data_ptr() + 8 * a * a), int(c.stride(0)), tabs,
        dptr(pairs, i32), pool.n_gates, dptr(first, i32), dptr(sign, i32), len(pool), dptr(work), dptr(out),
        _lib.stream_ptr())
    assert rc == 0, lib.oovqe_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _compare(name, dev, tw, pool, psi, c1, c2):
    worst = 0.0
    for b in range(psi.shape[0]):
        g, bound, pairs = A.pool_gradients(tw, pool, psi[b], c1[b], c2[b])
        err = np.abs(dev[b] - g)
        k = int(np.argmax(err / np.maximum(bound, 1e-300)))
        print(f"{name} state {b}: P = {len(g)}, max err {err.max():.3e}, at its worst operator err {err[k]:.3e} "
              f"bound {bound[k]:.3e} ({pairs[k]} pairs), max |g| {np.abs(g).max():.3e}")
        assert (err <= bound).all()
        assert (dev[b][pairs == 0] == 0.0).all() and not np.isnan(dev[b]).any()
        worst = max(worst, float(err.max()))
    return worst


# ---- 1: the kernel against the twin ------------------------------------------------------------------------------------
CASES = [("cas22-sd", 2, 2, "sd"), ("cas22-gsd", 2, 2, "gsd"), ("cas43-gsd", 3, 4, "gsd"), ("3e4o-gsd", 4, 3, "gsd"),
         ("cas44-gsd", 4, 4, "gsd"), ("cas43-one", 3, 4, "one"), ("cas43-rot", 3, 4, "rot")]


@pytest.mark.parametrize("name,ncas,nelecas,kind", CASES, ids=[c[0] for c in CASES])
def test_kernel_against_twin(name, ncas, nelecas, kind):
    """Random normalised psi, random NON-symmetric c1, c2 (the operator must enter as Hop + Hop^T), three states with
    coefficients of their own: |g_dev - g_twin| <= (a^4 + a^2 + pairs) 2^-52 A per operator.  Dc = 4 (one pair per gate),
    9, 24 (na = 6, nb = 4; operators without pairs -> exactly 0.0 over a NaN prefill), 36 (the per-geometry route of the
    sector engine); a pool of one operator; a two-gate operator."""
    n = 2 * ncas
    if kind == "one":
        pool = aoo.OperatorPool(ncas, nelecas, [[X.fde_gate([0, 1], [2, 3], n, 0)]])
    elif kind == "rot":
        pool = aoo.OperatorPool(ncas, nelecas, [X.orbital_rotation_gates([0, 1, 2, 3], n, 0),
                                                X.orbital_rotation_gates([2, 3, 4, 5], n, 0),
                                                [X.fse_gate(range(1, 4), n, 0)]])
        assert pool.n_gates == 5
    else:
        pool = aoo.OperatorPool(ncas, nelecas, kind)
    eng = _engine(ncas, nelecas)
    tw = A.Twin(ncas, eng.n_alpha, eng.n_beta)
    assert (tw.na, tw.nb) == (eng.na, eng.nb)
    lib = _lib.load()
    per_geometry = bool(lib.oovqe_sector_geometry_coefficients_ok(ncas, eng.na, eng.nb))
    print(f"{name}: na = {eng.na}, nb = {eng.nb}, per-geometry coefficients in one launch sequence: {per_geometry}")
    assert per_geometry if name == "cas44-gsd" else (per_geometry is False or ncas == 4)
    psi, c1, c2 = A.random_case(tw, 3, 100 + ncas * 10 + nelecas)
    dev = _from_coefficients(eng, pool, psi, c1, c2)
    _compare(name, dev, tw, pool, psi, c1, c2)
    if name == "3e4o-gsd":
        empty = A.pool_gradients(tw, pool, psi[0], c1[0], c2[0])[2] == 0
        assert empty.any() and (dev[:, empty] == 0.0).all()
    if name == "cas22-sd":
        assert list(A.pool_gradients(tw, pool, psi[0], c1[0], c2[0])[2]) == [2, 2, 1]     # (the double: one pair)
    # symmetrised coefficients would hide a missing Hop^T: the case must tell Hop + Hop^T from 2 Hop
    H = np.asarray(tw.hop(c1[0], c2[0]), dtype=float)
    assert np.abs(H - H.T).max() > 1e-2


def test_kernel_alone_in_lds_and_through_l2():
    """oovqe_pool_gradients_batch on given psi and lam against the formula evaluated on the host: CAS(4e,4o) (Dc = 36: psi
    and lam in LDS) and CAS(8e,9o) (Dc = 15 876: 254 016 bytes, read through L2), the "pair" pool, two states.  Bound:
    (pairs + 2) 2^-52 sum |terms|."""
    lib = _lib.load()
    i32 = torch.int32
    for ncas, nelecas in ((4, 4), (9, 8)):
        eng = _engine(ncas, nelecas)
        pool = aoo.OperatorPool(ncas, nelecas, "pair")
        tw = A.Twin(ncas, eng.n_alpha, eng.n_beta, operators=False)
        assert tw.Dc == eng.Dc and (16 * eng.Dc > 80 * 1024) == (ncas == 9)
        rng = np.random.default_rng(9 + ncas)
        psi, lam = rng.standard_normal((2, eng.Dc)), rng.standard_normal((2, eng.Dc))
        pairs, _, first, sign = pool.device_tables(eng)
        out = torch.full((2, len(pool)), float("nan"), dtype=F64, device=DEV)
        psi_d, lam_d = _t(psi), _t(lam)
        rc = lib.oovqe_pool_gradients_batch(dptr(psi_d), dptr(lam_d), eng.na, eng.nb, 2, dptr(pairs, i32), pool.n_gates,
                                            dptr(first, i32), dptr(sign, i32), len(pool), dptr(out), _lib.stream_ptr())
        assert rc == 0, lib.oovqe_last_error()
        dev = out.cpu().numpy()
        for b in range(2):
            g, bound, count = A.sparse_gradients(tw, pool, psi[b], lam[b])
            err = np.abs(dev[b] - g)
            print(f"CAS({nelecas}e,{ncas}o) state {b}: {count.max()} pairs, max err {err.max():.3e}, "
                  f"smallest bound {bound.min():.3e}")
            assert (err <= bound).all()


# ---- 2: against the route that exists ------------------------------------------------------------------------------------
def _formaldimine_oo(point=A.FORMAL):
    mol, C, theta = A.formaldimine_case(point)
    pqc = aoo.Parameterized_circuit(3, 4, None, ansatz="ucc")
    return aoo.OO_pqc(pqc, mol, 3, 4, oao_mo_coeff=C), pqc, _t(theta)


def _reference_by_appended_circuits(oo, pqc, theta, pool, which):
    """dE/dtheta_new of the circuit with operator k appended at theta_new = 0, by ``circuit_gradient`` of the same
    OO_pqc: the P + 1 evaluations the kernel replaces."""
    nt = int(np.prod(pqc.theta_shape))
    ext = torch.cat((theta.reshape(-1), torch.zeros(1, dtype=F64, device=DEV)))
    ref = []
    for k in which:
        big = aoo.Parameterized_circuit(pqc.ncas, pqc.nelecas, None,
                                        ansatz=list(pqc._gates) + pool.operator_gates(k, nt))
        adapt.swap_circuit(oo, big)
        ref.append(float(oo.circuit_gradient(ext)[-1]))
    adapt.swap_circuit(oo, pqc)
    return np.array(ref)


@pytest.mark.parametrize("kind", ["sd", "gsd"])
def test_pool_gradients_equal_appended_circuits(kind):
    """Formaldimine(140, 80) STO-3G (no spatial symmetry), UCCD CAS(4e,3o) at seeded thetas ~ N(0, 0.3), orbitals rotated
    by a seeded rotation of size 0.1: every operator of the pool within 1e-9 (the project's parity threshold; both sides
    O(1e-2 .. 1e-1)).  The seeds were checked on the CPU with the oracle's state and coefficients
    (tests/test_adapt_cpu.py): 0 of the 8 "sd" and 4 of the 24 "gsd" reference values lie below 1e-8."""
    oo, pqc, theta = _formaldimine_oo()
    pool = aoo.OperatorPool(3, 4, kind)
    g = oo.pool_gradients(theta, pool).cpu().numpy()
    assert g.shape == (len(pool),)
    ref = _reference_by_appended_circuits(oo, pqc, theta, pool, range(len(pool)))
    small = int((np.abs(ref) < 1e-8).sum())
    print(f"{kind}: {len(pool)} operators, max |g - ref| = {np.abs(g - ref).max():.3e}, max |ref| = "
          f"{np.abs(ref).max():.3e}, {small} reference values below 1e-8")
    assert 4 * small <= len(pool)
    assert np.abs(g - ref).max() < 1e-9


def test_pool_gradients_sector_engine_cas88():
    """kUpCCD CAS(8e,8o) on formaldimine (sector engine, Dc = 4 900, psi and lam in LDS): five operators of the "pair" pool
    against the appended circuits, 1e-9."""
    mol, C, _ = A.formaldimine_case()
    pqc = aoo.Parameterized_circuit(8, 8, None, ansatz="kupccd", k=1)
    assert pqc._use_sector and pqc._sector.Dc == 4900
    oo = aoo.OO_pqc(pqc, mol, 8, 8, oao_mo_coeff=C)
    theta = _t(0.3 * np.random.default_rng(A.THETA_SEED).standard_normal(pqc.theta_shape))
    pool = aoo.OperatorPool(8, 8, "pair")
    which = [0, 13, 27, 41, 55]
    g = oo.pool_gradients(theta, pool).cpu().numpy()
    ref = _reference_by_appended_circuits(oo, pqc, theta, pool, which)
    print("CAS(8e,8o) pair operators", which, "g", g[which], "ref", ref, "max diff", np.abs(g[which] - ref).max())
    assert int((np.abs(ref) < 1e-8).sum()) <= 1
    assert np.abs(g[which] - ref).max() < 1e-9


# ---- 3: a stack ---------------------------------------------------------------------------------------------------------
POINTS = [(140, 80), (130, 85), (120, 70), (135, 60)]


def _stack(order=(0, 1, 2, 3)):
    pqc = aoo.Parameterized_circuit(3, 4, None, ansatz="ucc")
    cases = [A.formaldimine_case(POINTS[i]) for i in order]
    batch = aoo.OO_pqc_batch(pqc, [c[0] for c in cases], 3, 4, oao_mo_coeffs=[c[1] for c in cases])
    thetas = _t(0.3 * np.random.default_rng(31).standard_normal((4, pqc.theta_shape)))[list(order)].contiguous()
    return batch, pqc, cases, thetas


def test_stack_rows_permutation_stream_and_set_circuit():
    batch, pqc, cases, thetas = _stack()
    pool = aoo.OperatorPool(3, 4, "gsd")
    g = batch.pool_gradients(thetas, pool)
    assert g.shape == (4, len(pool))
    # each row = that geometry alone, within the bound of the kernel test (both within it of the twin)
    tw = A.Twin(3, 2, 2)
    for i, (mol, C, _) in enumerate(cases):
        one = aoo.OO_pqc(pqc, mol, 3, 4, oao_mo_coeff=C)
        g1 = one.pool_gradients(thetas[i], pool)
        _, c1, c2 = one.get_active_integrals(one.mo_coeff)
        psi = pqc._sector.state(thetas[i:i + 1])[0].cpu().numpy()
        ref, bound, _ = A.pool_gradients(tw, pool, psi, c1.cpu().numpy(), c2.cpu().numpy())
        e_b, e_1 = np.abs(g[i].cpu().numpy() - ref), np.abs(g1.cpu().numpy() - ref)
        d = (g[i] - g1).abs().cpu().numpy()
        print(f"geometry {i}: stack-vs-alone {d.max():.3e}, stack-vs-twin {e_b.max():.3e}, alone-vs-twin "
              f"{e_1.max():.3e}, smallest non-zero bound {bound[bound > 0].min():.3e}")
        # (the twin takes psi, c1, c2 of the geometry alone; the stack's evaluation rounds its c1, c2 on another route:
        # a perturbation of the inputs by a few ulp, itself below the bound, on top of the arithmetic)
        assert (e_1 <= bound).all() and (e_b <= 2 * bound).all() and (d <= bound).all()
    # rows of index
    assert torch.equal(batch.pool_gradients(thetas, pool, index=[2, 0]), g[[2, 0]])
    # another stream: the same bits
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g_side = batch.pool_gradients(thetas, pool)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(g_side, g)
    # a permuted stack: the permuted rows, the same bits
    order = (2, 0, 3, 1)
    batch_p, _, _, thetas_p = _stack(order)
    assert torch.equal(batch_p.pool_gradients(thetas_p, pool), g[list(order)])
    # set_circuit with the chosen operator appended at 0
    k = int(torch.argmax((g * g).sum(dim=0)))
    nt = batch.n_theta
    e0 = batch.energy(thetas).clone()
    p2e, ppk = batch.int2e_ao.data_ptr(), (None if batch._eri_packed is None else batch._eri_packed.data_ptr())
    oao = batch.oao_mo_coeff.clone()
    flags = batch.eri_flags
    batch.set_circuit(aoo.Parameterized_circuit(3, 4, None, ansatz=list(pqc._gates) + pool.operator_gates(k, nt)))
    assert batch.n_theta == nt + 1 and batch.int2e_ao.data_ptr() == p2e and batch.eri_flags == flags
    assert (None if batch._eri_packed is None else batch._eri_packed.data_ptr()) == ppk
    assert torch.equal(batch.oao_mo_coeff, oao)
    ext = torch.cat((thetas, torch.zeros((4, 1), dtype=F64, device=DEV)), dim=1).contiguous()
    e1 = batch.energy(ext)
    col = batch.full_gradient(ext)[:, nt]
    print("set_circuit: max |dE| =", float((e1 - e0).abs().max()), " new column vs pool gradient:",
          float((col - g[:, k]).abs().max()), " |g_k| =", g[:, k].abs().tolist())
    assert (e1 - e0).abs().max() < 1e-12
    assert (col - g[:, k]).abs().max() < 1e-9
    with pytest.raises(ValueError):
        batch.set_circuit(aoo.Parameterized_circuit(2, 2, None, ansatz="ucc"))
    # the lockstep Newton step runs on the new circuit
    new, e_new, _ = batch.damped_newton_step(ext)
    assert new.shape == (4, nt + 1) and bool((e_new <= e1 + 1e-12).all())


# ---- 4: the driver ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", ["H 0 0 0; H 0 0 0.74", None], ids=["H2", "formaldimine"])
def test_adapt_fixed_orbitals_reaches_casci(geometry):
    """CAS(2e,2o), the "sd" pool (two singles, one double: they span the singlet tangent space), orbitals fixed at RHF:
    the energy never rises, every choice is the argmax of |g|, the final pool-gradient norm is below 1e-7 and the energy
    is the CASCI energy at the same orbitals to 1e-9 Ha.  H2 (the singles vanish by symmetry) and formaldimine(140, 80)
    (no symmetry: the singles are needed)."""
    mol = aoo.Moldata_sto3g(geometry) if geometry else A.formaldimine_case()[0]
    mol.run_rhf()
    ref = float(np.atleast_1d(mol.run_casci(2, 2).e_tot)[0])
    pqc = aoo.Parameterized_circuit(2, 2, None, ansatz="ucc")
    oo = aoo.OO_pqc(pqc, mol, 2, 2, oao_mo_coeff=mo_ao_to_mo_oao(mol.hf.mo_coeff, mol.overlap))
    pool = aoo.OperatorPool(2, 2, "sd")
    res = aoo.adapt_vqe(oo, pool, max_operators=8, grad_tol=1e-7, orbital_optimization=False)
    print("chosen", res.operators, "energies", res.energies, "norms", res.gradient_norms, "CASCI", ref)
    assert res.converged and res.gradient_norms[-1] < 1e-7 and 1 <= len(res.operators) <= 8
    e = np.array(res.energies)
    assert (np.diff(e) <= 1e-12).all()
    for k, g in zip(res.operators, res.pool_gradients):
        assert k == int(torch.argmax(g.abs()))
    assert len(res.gates) == len(res.operators) and res.thetas.shape == (len(res.operators),)
    assert res.oo is oo and int(np.prod(oo.pqc.theta_shape)) == len(res.operators)
    assert abs(oo.energy_from_parameters(res.thetas).item() - e[-1]) < 1e-12
    assert abs(e[-1] - ref) < 1e-9


def test_adapt_with_orbital_optimization_one_geometry_and_stack():
    """CAS(4e,3o) on formaldimine with the orbitals optimised along, "gsd" pool, four additions: energies non-increasing
    per geometry and never below the CASCI energy at the orbitals of that moment (- 1e-9); the stack ends with ONE gate
    table.  Gaps to CASCI as measured on an MI355X (reported, not asserted): one geometry 1.1e-05 after one operator,
    2.8e-14 after two (then the pool-gradient norm is below 1e-6); the stack 1.1e-05 / 9.4e-05 / 3.9e-05 after one,
    0 / 0 / 0 after two."""
    pool = aoo.OperatorPool(3, 4, "gsd")
    # one geometry
    mol, _, _ = A.formaldimine_case()
    pqc = aoo.Parameterized_circuit(3, 4, None, ansatz="ucc")
    oo = aoo.OO_pqc(pqc, mol, 3, 4, oao_mo_coeff=mo_ao_to_mo_oao(mol.hf.mo_coeff, mol.overlap))
    gaps = []

    def gap_one(n, obj, thetas, energy):
        ci = float(np.atleast_1d(mol.run_casci(3, 4, mo=obj.mo_coeff.cpu().numpy()).e_tot)[0])
        gaps.append(energy - ci)
        print(f"one geometry, {n} operators: E = {energy:.10f}, E - E_CASCI(same orbitals) = {energy - ci:.3e}")

    res = aoo.adapt_vqe(oo, pool, max_operators=4, grad_tol=1e-6, callback=gap_one)
    e = np.array(res.energies)
    assert len(res.operators) >= 1 and (np.diff(e) <= 1e-10).all() and min(gaps) >= -1e-9
    # a stack of three
    cases = [A.formaldimine_case(p) for p in POINTS[:3]]
    batch = aoo.OO_pqc_batch(pqc, [c[0] for c in cases], 3, 4,
                             oao_mo_coeffs=[mo_ao_to_mo_oao(c[0].hf.mo_coeff, c[0].overlap) for c in cases])
    gaps_s = []

    def gap_stack(n, obj, thetas, energy):
        ci = obj.casci()[0][:, 0]
        gaps_s.append((energy - ci).cpu().numpy())
        print(f"stack, {n} operators: E - E_CASCI(same orbitals) =", gaps_s[-1])

    res = aoo.adapt_vqe(batch, pool, max_operators=4, grad_tol=1e-6, callback=gap_stack)
    es = torch.stack(res.energies).cpu().numpy()                       # [additions, G]
    assert es.shape[1] == 3 and (np.diff(es, axis=0) <= 1e-10).all() and np.min(gaps_s) >= -1e-9
    assert res.oo is batch and batch.n_theta == len(res.operators) == len(res.gates)
    assert res.thetas.shape == (3, len(res.operators))
    assert [(g.mask_hi, g.mask_lo, g.theta_idx) for g in batch.pqc._gates] == \
        [(g.mask_hi, g.mask_lo, g.theta_idx) for g in res.gates]
    for k, g in zip(res.operators, res.pool_gradients):
        assert k == int(torch.argmax((g * g).sum(dim=0)))


# ---- 5: refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(monkeypatch):
    lib = _lib.load()
    i32 = torch.int32
    # the library: more than 32 767 determinants, a null pointer, an empty stack -- the NaN prefill is untouched
    eng = _engine(3, 4)
    pool = aoo.OperatorPool(3, 4, "sd")
    pairs, tabs, first, sign = pool.device_tables(eng)
    buf = torch.full((64,), float("nan"), dtype=F64, device=DEV)
    torch.cuda.synchronize()
    args = lambda na, nb, batch, p=pairs: (dptr(buf), dptr(buf), na, nb, batch, dptr(p, i32) if p is not None else NULL,   # noqa: E731
                                           pool.n_gates, dptr(first, i32), dptr(sign, i32), len(pool), dptr(buf),
                                           _lib.stream_ptr())
    for bad in (args(252, 252, 1), args(3, 3, 0), args(3, 3, 70000), args(3, 3, 1, None)):
        assert lib.oovqe_pool_gradients_batch(*bad) != 0
        assert lib.oovqe_last_error()
    assert lib.oovqe_pool_gradients_batch(*args(252, 252, 1)) != 0 and b"determinants" in lib.oovqe_last_error()
    rc = lib.oovqe_pool_gradients_from_coefficients_batch(
        dptr(buf), 10, *eng._tabs()[:4], 252, 252, 1, dptr(buf), dptr(buf), 1, tabs, dptr(pairs, i32), pool.n_gates,
        dptr(first, i32), dptr(sign, i32), len(pool), dptr(buf), dptr(buf), _lib.stream_ptr())
    assert rc != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
    # Python: nothing reaches the library, the evaluation or the circuit
    oo, pqc, theta = _formaldimine_oo()
    batch = aoo.OO_pqc_batch(pqc, [A.formaldimine_case()[0]], 3, 4, oao_mo_coeffs=[A.formaldimine_case()[1]])
    calls = []
    stub = lambda *a, **k: calls.append(1) or 0                                   # noqa: E731
    monkeypatch.setattr(lib, "oovqe_pool_gradients_from_coefficients_batch", stub)
    monkeypatch.setattr(lib, "oovqe_pool_gradients_batch", stub)
    monkeypatch.setattr(lib, "oovqe_sector_pairs", stub)
    monkeypatch.setattr(oo, "_evaluate", stub)
    monkeypatch.setattr(batch, "evaluate", stub)
    monkeypatch.setattr(pqc._sector, "state", stub)
    other = aoo.OperatorPool(2, 2, "sd")
    for call in (lambda: oo.pool_gradients(theta, None), lambda: batch.pool_gradients(theta[None], None),
                 lambda: oo.pool_gradients(theta, other), lambda: batch.pool_gradients(theta[None], other),
                 lambda: oo.pool_gradients(theta[:3], pool), lambda: batch.pool_gradients(theta[None, :3], pool),
                 lambda: batch.pool_gradients(torch.zeros((2, 4), dtype=F64, device=DEV), pool),
                 lambda: batch.pool_gradients(theta[None], pool, index=[1]),
                 lambda: aoo.adapt_vqe(oo, other, 2), lambda: aoo.adapt_vqe(batch, None, 2)):
        with pytest.raises(ValueError):
            call()
    big = SimpleNamespace(ncas=10, nelecas=10, _sector=SimpleNamespace(Dc=252 * 252))
    with pytest.raises(ValueError, match="determinants"):
        adapt.check_pool(aoo.OperatorPool(10, 10, "pair"), big)
    assert calls == []
