"""The k-depth build and LDS size of cas_tail_kernel as the plan of a batched evaluation reports them (fields
``tail`` and ``tail_lds`` of oovqe_oo_eval_plan_describe, present on the packed_tail path only); no device needed."""
import pytest

from auto_oo_amd import excitations as X, ops


def _plan(N, n_occ, ncas, nelecas, batch, flags=3, packed=True):
    gates, n_theta = X.uccd_gates(ncas, nelecas, False)
    n_kappa = len(X.non_redundant_indices(list(range(n_occ)), list(range(n_occ, n_occ + ncas)),
                                          list(range(n_occ + ncas, N)), False))
    return ops.eval_plan(N, n_occ, ncas, n_kappa, batch, flags, packed, n_theta, len(gates), True, True)


@pytest.mark.parametrize("N", range(33, 49))
def test_tail_depth_by_size(N):
    """Both flags, a packed copy, 256 geometries: the one-launch tail for every N of the two deepest stage-1 rows,
    in its 11-step build where 11 steps cover N (41..44) and the 12-step build elsewhere; within 160 KB of LDS."""
    p = _plan(N, 6, 3, 4, 256)
    assert p["path"] == "packed_tail"
    assert p["tail"] == ("cas_tail_kernel<11>" if 41 <= N <= 44 else "cas_tail_kernel<12>")
    assert 0 < int(p["tail_lds"]) <= 160 * 1024


def test_tail_depth_of_smaller_sizes_and_other_paths():
    """The shallower builds keep their depths; a path without the tail reports neither field."""
    assert _plan(20, 6, 3, 4, 256)["tail"] == "cas_tail_kernel<8>"
    assert _plan(32, 6, 3, 4, 256)["tail"] == "cas_tail_kernel<8>"
    p = _plan(43, 6, 3, 4, 64)
    assert p["path"] == "packed_split" and "tail" not in p and "tail_lds" not in p


def test_tail_takes_the_small_active_spaces():
    """The shapes of tests/test_tail_depth_gpu.py at N = 43: CAS(2e,2o) with 3 core orbitals takes the tail from 385
    geometries on, with 6 core orbitals from 193 on, as 6 core + 3 active orbitals do; all in the 11-step build."""
    for n_occ, ncas, nelecas, batch in ((3, 2, 2, 385), (6, 2, 2, 193), (6, 3, 4, 193)):
        assert _plan(43, n_occ, ncas, nelecas, batch - 1)["path"] == "packed_split"
        p = _plan(43, n_occ, ncas, nelecas, batch)
        assert p["path"] == "packed_tail" and p["tail"] == "cas_tail_kernel<11>"
        assert 0 < int(p["tail_lds"]) <= 160 * 1024
