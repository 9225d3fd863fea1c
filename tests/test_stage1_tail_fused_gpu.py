"""The one-workgroup-per-geometry tail of the packed-triangle path (cas_tail_kernel: q -> x, p -> n, Fock
columns and assembly in one launch, g_mo kept in LDS) against the three-launch tail it replaces
(sym_gm_kernel, cas_panel_kernel, cas_final_kernel; option ``tail_split``) and against the CPU oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NCAS, NELECAS, NELEC = 3, 4, 16


def _batch(N, G, seed):
    import auto_oo_amd as aoo
    from auto_oo_amd.synthetic import synthetic_problem
    pqc = aoo.Parameterized_circuit(NCAS, NELECAS, None, ansatz="ucc")
    base = [synthetic_problem(N, seed + g) for g in range(4)]
    mols = [aoo.Moldata(base[g % 4]["int1e_ao"], base[g % 4]["int2e_ao"], base[g % 4]["overlap"],
                        base[g % 4]["nuc"] + 0.001 * g, NELEC) for g in range(G)]
    batch = aoo.OO_pqc_batch(pqc, mols, NCAS, NELECAS, oao_mo_coeffs=[base[g % 4]["oao_mo_coeff"] for g in range(G)])
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


@pytest.mark.parametrize("N, G", [(43, 256), (43, 300), (48, 256), (20, 256)])
def test_tail_equals_the_three_launch_tail(N, G):
    """N = 43 is the bench shape (KS = 12, 3 tiles of y <= z); G = 300 runs the tail in two rounds; N = 48
    leaves no zero rows in q -> x, N = 20 takes the KS = 8 build."""
    _, _, batch, thetas = _batch(N, G, 9700 + N)
    eg, launches = _evaluate(batch, thetas)
    eg_split, launches_split = _evaluate(batch, thetas, tail_split=1)
    assert torch.isfinite(eg).all()
    # one tail launch (label of the p -> n step) and no panel / final launch; the split tail has all three
    assert launches["contract_p_to_n"] == 1 and launches["column"] == 0 and launches["final"] == 0
    assert launches_split["contract_p_to_n"] == 1 and launches_split["column"] == 1 and launches_split["final"] == 1
    assert (eg - eg_split).abs().max().item() <= 1e-11
    # energy only (one RDM set) through the same kernel
    assert (batch.energy(thetas) - eg[:, 0]).abs().max().item() <= 1e-11


def test_tail_matches_the_oracle():
    """Geometries of the bench-shaped 256-batch against the plain-torch oracle (the smoke() tolerances)."""
    from oracle import cpu_ref as R
    pqc, base, batch, thetas = _batch(43, 256, 9800)
    eg, launches = _evaluate(batch, thetas)
    assert launches["column"] == 0
    for g in (0, 129, 255):
        P = base[g % 4]
        omol = R.OracleMol(P["int1e_ao"], P["int2e_ao"], P["overlap"], P["nuc"] + 0.001 * g, NELEC)
        ooo = R.OracleOOPQC(R.OraclePQC(NCAS, NELECAS, "ucc"), omol, NCAS, NELECAS, P["oao_mo_coeff"])
        th = thetas[g].cpu()
        assert abs(eg[g, 0].item() - ooo.energy_from_parameters(th).item()) < 1e-9
        assert (eg[g, 1:].cpu() - ooo.full_gradient(th)).abs().max().item() < 1e-8


def test_small_batch_keeps_the_three_launch_tail():
    """64 geometries (four stage-1 workgroups per geometry, a quarter of the chip with one workgroup per geometry)
    stay on sym_gm / panel / final and equal the same geometries inside a batch that takes the tail."""
    _, _, big, thetas = _batch(43, 256, 9900)
    eg_big, launches_big = _evaluate(big, thetas)
    assert launches_big["column"] == 0
    import auto_oo_amd as aoo
    from auto_oo_amd.synthetic import synthetic_problem
    pqc = aoo.Parameterized_circuit(NCAS, NELECAS, None, ansatz="ucc")
    base = [synthetic_problem(43, 9900 + g) for g in range(4)]
    mols = [aoo.Moldata(base[g % 4]["int1e_ao"], base[g % 4]["int2e_ao"], base[g % 4]["overlap"],
                        base[g % 4]["nuc"] + 0.001 * g, NELEC) for g in range(64, 128)]
    small = aoo.OO_pqc_batch(pqc, mols, NCAS, NELECAS,
                             oao_mo_coeffs=[base[g % 4]["oao_mo_coeff"] for g in range(64, 128)])
    eg_small, launches_small = _evaluate(small, thetas[64:128].contiguous())
    assert launches_small["column"] == 1 and launches_small["final"] == 1
    assert (eg_small - eg_big[64:128]).abs().max().item() <= 1e-11
