"""cas_tail_kernel with q -> x writing the kept entries of g_mo into a packed array and p -> n running once over its
column tiles, in place: every kept value is the same product chain over the same operands in the same order as in
the three-launch tail (option ``tail_split``), so the outputs are equal bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _batch(N, G, seed, ncas=3, nelecas=4, nelec=16):
    """four synthetic base problems, reused over the G geometries (tests/test_tail_depth_gpu.py::_batch)"""
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


# (N, G, ncas, nelecas, electrons)
CASES = [
    (41, 193, 3, 4, 16),    # zero rows of the 11-step build; the last n-block partly filled
    (43, 193, 3, 4, 16),    # the bench shape; NC = 210: the last column tile has 2 live columns
    (33, 193, 3, 4, 16),    # 15 zero rows; rows n < N of a 48-row array
    (48, 193, 3, 4, 16),    # the tightest LDS
    (20, 193, 3, 4, 16),    # the 8-step build
    (43, 385, 2, 2, 8),     # CAS(2e,2o), 3 core orbitals: one tile of (y <= z); NC = 54
    (43, 193, 2, 2, 14),    # CAS(2e,2o), 6 core orbitals: NC = 138
]


@pytest.mark.parametrize("N, G, ncas, nelecas, nelec", CASES)
def test_packed_tail_equals_the_three_launch_tail_exactly(N, G, ncas, nelecas, nelec):
    _, _, batch, thetas = _batch(N, G, 9500 + N, ncas, nelecas, nelec)
    eg, launches = _evaluate(batch, thetas)
    eg_split, launches_split = _evaluate(batch, thetas, tail_split=1)
    assert torch.isfinite(eg).all()
    assert launches["contract_p_to_n"] == 1 and launches["column"] == 0 and launches["final"] == 0
    assert launches_split["column"] == 1 and launches_split["final"] == 1
    e = batch.energy(thetas)
    diff = (eg - eg_split).abs().max().item()
    diff_e = (e - eg[:, 0]).abs().max().item()
    print(f"N={N} G={G} CAS({nelecas}e,{ncas}o): tail vs split {diff:.3e}, energy() vs column 0 {diff_e:.3e}")
    assert torch.equal(eg, eg_split)
    assert torch.equal(e, eg[:, 0])
