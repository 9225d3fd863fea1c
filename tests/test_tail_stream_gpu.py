"""cas_tail_kernel with its inputs staged through registers in one round trip, three register sets of J in rotation
where a tile has three groups of rows, and stage 3 compiled for 2 and 3 active orbitals: every chain and every sum keeps
its operands and its order, so the outputs equal, bit for bit, those of the three-launch tail (option ``tail_split``)
and those of stage 3 with the active-space size at run time (option ``tail_generic``).

Every shape is checked on the host first: the plan sends it to the one-launch tail with the build named here."""
import pytest
import torch

from auto_oo_amd import excitations as X, ops
from tests.test_tail_packed_gpu import _batch, _evaluate

pytestmark = pytest.mark.gpu

# (N, G, ncas, nelecas, electrons, build of the tail)
CASES = [
    (41, 193, 3, 4, 16, 11),    # the 11-step build with zero rows; three sets
    (43, 193, 3, 4, 16, 11),    # the bench build
    (33, 193, 3, 4, 16, 12),    # the 12-step build, 15 zero rows
    (48, 193, 3, 4, 16, 12),    # the tightest LDS
    (20, 193, 3, 4, 16, 8),     # the 8-step build: two groups a tile, two sets kept
    (43, 385, 2, 2, 8, 11),     # CAS(2e,2o), 3 core orbitals: the instance for 2 active orbitals, one tile of (y <= z)
    (43, 193, 2, 2, 14, 11),    # CAS(2e,2o), 6 core orbitals: the instance for 2 active orbitals
    (43, 300, 3, 4, 16, 11),    # more geometries than CUs: two resident rounds of the tail
]


@pytest.mark.parametrize("N, G, ncas, nelecas, nelec, build", CASES)
def test_tail_equals_the_split_and_the_generic_tail_exactly(N, G, ncas, nelecas, nelec, build):
    n_occ = (nelec - nelecas) // 2
    gates, n_theta = X.uccd_gates(ncas, nelecas, False)
    n_kappa = len(X.non_redundant_indices(list(range(n_occ)), list(range(n_occ, n_occ + ncas)),
                                          list(range(n_occ + ncas, N)), False))
    plan = ops.eval_plan(N, n_occ, ncas, n_kappa, G, 3, True, n_theta, len(gates), True, True)
    assert plan["path"] == "packed_tail" and plan["tail"] == f"cas_tail_kernel<{build}>", plan

    _, _, batch, thetas = _batch(N, G, 9700 + N, ncas, nelecas, nelec)
    eg, launches = _evaluate(batch, thetas)
    eg_split, launches_split = _evaluate(batch, thetas, tail_split=1)
    eg_generic, launches_generic = _evaluate(batch, thetas, tail_generic=1)
    assert torch.isfinite(eg).all()
    for by in (launches, launches_generic):
        assert by["contract_p_to_n"] == 1 and by["column"] == 0 and by["final"] == 0
    assert launches_split["column"] == 1 and launches_split["final"] == 1
    e = batch.energy(thetas)
    print(f"N={N} G={G} CAS({nelecas}e,{ncas}o): tail vs split {(eg - eg_split).abs().max().item():.3e}, "
          f"vs generic {(eg - eg_generic).abs().max().item():.3e}, "
          f"energy() vs column 0 {(e - eg[:, 0]).abs().max().item():.3e}")
    assert torch.equal(eg, eg_split)
    assert torch.equal(eg, eg_generic)
    assert torch.equal(e, eg[:, 0])
