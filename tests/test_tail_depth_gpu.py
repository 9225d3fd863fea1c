"""The k-depth builds of cas_tail_kernel (the one-launch tail of the packed-triangle path): 41 <= N <= 44 run the
11-step build (44 rows of T3s; the rows p >= N of a wave's share are neither loaded nor multiplied and written as
zeros), 33..40 and 45..48 the 12-step build.  Every shape against the three-launch tail (option ``tail_split``),
which the tail equals sum for sum, and one other active space (another table of kept g_mo entries) against the CPU
oracle as well."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _batch(N, G, seed, ncas=3, nelecas=4, nelec=16):
    """four synthetic base problems, reused over the G geometries (tests/test_stage1_tail_fused_gpu.py::_batch)"""
    import auto_oo_amd as aoo
    from auto_oo_amd.synthetic import synthetic_problem
    pqc = aoo.Parameterized_circuit(ncas, nelecas, None, ansatz="ucc")
    base = [synthetic_problem(N, seed + g) for g in range(4)]
    mols = [aoo.Moldata(base[g % 4]["int1e_ao"], base[g % 4]["int2e_ao"], base[g % 4]["overlap"],
                        base[g % 4]["nuc"] + 0.001 * g, nelec) for g in range(G)]
    batch = aoo.OO_pqc_batch(pqc, mols, ncas, nelecas, oao_mo_coeffs=[base[g % 4]["oao_mo_coeff"] for g in range(G)])
    assert batch.eri_flags == 3 and batch._eri_packed is not None
    thetas = torch.tensor(np.random.default_rng(seed).uniform(0, 2 * np.pi, (G, pqc.theta_shape)), device=DEV)
    return pqc, base, batch, thetas


def _evaluate(batch, thetas, **opts):
    """energy + gradient of every geometry, and the launches of the evaluation by profile label"""
    from auto_oo_amd import _lib, ops
    with _lib.debug_options(**opts):
        batch.energy_and_gradient(thetas)              # (workspace and plan set up outside the bracket)
        torch.cuda.synchronize()
        ops.profile_begin(detail=True)
        eg = batch.energy_and_gradient(thetas).clone()
        torch.cuda.synchronize()
        _, _, by = ops.profile_end()
    return eg, {k: v[1] for k, v in by.items()}


@pytest.mark.parametrize("N, G", [(41, 193), (44, 193), (45, 193), (40, 193), (43, 300)])
def test_tail_depths_equal_the_three_launch_tail(N, G):
    """(41, 193): three zero rows in the 11-step build; (44, 193): no zero row; (45, 193): first size of the 12-step
    build; (40, 193): last size that keeps its old build; (43, 300): the bench size, more workgroups than CUs.
    193 is the smallest batch that takes the tail at 6 core + 3 active orbitals (tests/test_eval_plan.py: up to 192
    geometries the circuit rides along sym_gm_kernel and the three-launch tail runs)."""
    _, _, batch, thetas = _batch(N, G, 9300 + N)
    eg, launches = _evaluate(batch, thetas)
    eg_split, launches_split = _evaluate(batch, thetas, tail_split=1)
    assert torch.isfinite(eg).all()
    assert launches["contract_p_to_n"] == 1 and launches["column"] == 0 and launches["final"] == 0
    assert launches_split["column"] == 1 and launches_split["final"] == 1
    diff = (eg - eg_split).abs().max().item()
    diff_e = (batch.energy(thetas) - eg[:, 0]).abs().max().item()
    print(f"N={N} G={G}: tail vs split {diff:.3e}, energy() vs column 0 {diff_e:.3e}")
    assert diff <= 1e-11
    assert diff_e <= 1e-11


@pytest.mark.parametrize("nelec, G", [(8, 385), (14, 193)])
def test_tail_other_active_space(nelec, G):
    """CAS(2e,2o) at N = 43 (the 11-step build), another table of kept g_mo entries than 6 core + 3 active:
    8 electrons, 3 core orbitals, M = 5: one tile of (y <= z), so the second register set is never filled from
    memory; it takes the tail from 385 geometries on (below, the circuit rides along sym_gm_kernel);
    14 electrons, 6 core orbitals, M = 8: three tiles; the nearest active space that takes the tail at 193.
    Against the three-launch tail and, geometry 0, the CPU oracle at the smoke() tolerances."""
    from oracle import cpu_ref as R
    ncas, nelecas = 2, 2
    pqc, base, batch, thetas = _batch(43, G, 9400, ncas, nelecas, nelec)
    eg, launches = _evaluate(batch, thetas)
    eg_split, _ = _evaluate(batch, thetas, tail_split=1)
    assert torch.isfinite(eg).all()
    assert launches["contract_p_to_n"] == 1 and launches["column"] == 0 and launches["final"] == 0
    diff = (eg - eg_split).abs().max().item()
    print(f"CAS(2e,2o), {nelec} electrons: tail vs split {diff:.3e}")
    assert diff <= 1e-11
    P = base[0]
    omol = R.OracleMol(P["int1e_ao"], P["int2e_ao"], P["overlap"], P["nuc"], nelec)
    ooo = R.OracleOOPQC(R.OraclePQC(ncas, nelecas, "ucc"), omol, ncas, nelecas, P["oao_mo_coeff"])
    th = thetas[0].cpu()
    de = abs(eg[0, 0].item() - ooo.energy_from_parameters(th).item())
    dg = (eg[0, 1:].cpu() - ooo.full_gradient(th)).abs().max().item()
    print(f"CAS(2e,2o), {nelec} electrons: oracle energy {de:.3e}, gradient {dg:.3e}")
    assert de < 1e-9
    assert dg < 1e-8
