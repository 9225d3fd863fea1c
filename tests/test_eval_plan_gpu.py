"""The plan says what ran: for one shape per path of the batched evaluation (the smallest that reaches it), the
launches by profile label and the stage-1 kernel of a real evaluation equal those of its plan
(ops.eval_plan, computed without launching), and the result agrees with the CPU oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NCAS, NELECAS = 3, 4

# path, N, geometries, occupied orbitals, integrals perturbed so that neither symmetry flag is set
CASES = [("column", 20, 30, 6, False), ("packed_split", 20, 31, 6, False), ("packed_tail", 20, 193, 6, False),
         ("fused", 20, 31, 6, True), ("fused", 13, 73, 6, False), ("staged", 24, 2, 18, False)]


@pytest.mark.parametrize("path, N, G, n_occ, perturb", CASES, ids=[f"{c[0]}-N{c[1]}-G{c[2]}{'-flags0' if c[4] else ''}" for c in CASES])
def test_plan_says_what_ran(path, N, G, n_occ, perturb):
    import auto_oo_amd as aoo
    from auto_oo_amd import _lib, ops
    from auto_oo_amd.synthetic import synthetic_problem
    from oracle import cpu_ref as R
    nelec = 2 * n_occ + NELECAS
    pqc = aoo.Parameterized_circuit(NCAS, NELECAS, None, ansatz="ucc")
    base = [synthetic_problem(N, 7300 + N + g) for g in range(4)]
    if perturb:
        for P in base:
            P["int2e_ao"] = np.array(P["int2e_ao"], copy=True)
            # one ulp on one element: both symmetry flags (exact comparisons) fall, the numbers stay what they were, so
            # the oracle's agreement does not hinge on how either side treats integrals without the symmetries
            P["int2e_ao"][0, 1, 2, 3] = np.nextafter(P["int2e_ao"][0, 1, 2, 3], np.inf)
    mols = [aoo.Moldata(base[g % 4]["int1e_ao"], base[g % 4]["int2e_ao"], base[g % 4]["overlap"],
                        base[g % 4]["nuc"] + 0.001 * g, nelec) for g in range(G)]
    batch = aoo.OO_pqc_batch(pqc, mols, NCAS, NELECAS, oao_mo_coeffs=[base[g % 4]["oao_mo_coeff"] for g in range(G)])
    assert batch.eri_flags == (0 if perturb else 3) and batch._n_occ == n_occ
    thetas = torch.tensor(np.random.default_rng(N + G).uniform(0, 2 * np.pi, (G, pqc.theta_shape)), device=DEV)

    plan = ops.eval_plan(N, n_occ, NCAS, batch.n_kappa, G, batch.eri_flags, batch._eri_packed is not None,
                         batch.n_theta, pqc._n_gates)
    assert plan["path"] == path

    batch.energy_and_gradient(thetas)                  # (workspace set up outside the bracket)
    torch.cuda.synchronize()
    ops.profile_begin(detail=True)
    eg = batch.energy_and_gradient(thetas).clone()
    torch.cuda.synchronize()
    _, _, by = ops.profile_end()
    assert {k: v[1] for k, v in by.items()} == plan["labels"]
    assert _lib.load().oovqe_last_stage1_kernel().decode() == plan["stage1"]

    for g in (0, G - 1):
        P = base[g % 4]
        omol = R.OracleMol(P["int1e_ao"], P["int2e_ao"], P["overlap"], P["nuc"] + 0.001 * g, nelec)
        ooo = R.OracleOOPQC(R.OraclePQC(NCAS, NELECAS, "ucc"), omol, NCAS, NELECAS, P["oao_mo_coeff"])
        th = thetas[g].cpu()
        assert abs(eg[g, 0].item() - ooo.energy_from_parameters(th).item()) < 1e-9
        assert (eg[g, 1:].cpu() - ooo.full_gradient(th)).abs().max().item() < 1e-8
