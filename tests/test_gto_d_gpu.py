"""d shells on the device (csrc/gto_d.hip, ``GTOBasis(..., d_functions=...)``) against the host twin
``gaussian.integrals_from_table`` and end to end.  The molecules M1 and M2 are described in tests/_gto_d.py.

Bounds (none of them taken from what the device code gives; all measured on the CPU):

* Boys function, orders up to 8: per order 10 x the error of the host function ``gaussian._boys`` against 40-digit
  arithmetic (``_gto_d.HOST_BOYS_ERROR``: 2.1e-15 at n = 0 growing to 1.6e-13 at n = 8, scipy's ``hyp1f1`` loses
  digits with the order; the scheme of the kernels evaluated in fp64 on the CPU is within 4.8e-15 for n <= 8).
* M1 element by element: the host integrals of M1 built twice, plain and with ``gaussian._boys`` of order n multiplied
  by 1 + BOYS_RTOL[n] * (+-1 at random) -- the disagreement the Boys test allows.  Largest elementwise difference, both
  forms: MEASURED_H = 4.1e-13 for h, MEASURED_G = 6.3e-14 for g.  The bounds are 10 x these (the factor covers the
  different summation order of the kernels); overlap and nuclear repulsion, having no Boys function, take the bound
  of g.
* Energies and gradients 1e-9 (the project's bound).

Before their first device run the kernel bodies were run on the CPU (they are host functions of the lane index) against
the same host twin: M1 agrees to 4.4e-16 (S), 5.3e-15 (h), 5.6e-16 (g) in both forms.  Device figures are not recorded
here yet."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import auto_oo_amd as aoo                                   # noqa: E402
from auto_oo_amd import _lib, gaussian, gto, ops, scf       # noqa: E402
from oracle import cpu_ref as R                             # noqa: E402
from tests import _gto_d as D                               # noqa: E402

MEASURED_H, MEASURED_G = 4.1e-13, 6.3e-14
TOL_H, TOL_G = 10 * MEASURED_H, 10 * MEASURED_G
NAMES = ("overlap", "int1e_ao", "int2e_ao", "nuc", "oao_coeff")


# ---- 4. Boys function -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nmax", [5, 6, 7, 8])
def test_boys_function_of_the_d_orders_against_the_host(nmax):
    T = np.concatenate(([0.0], np.linspace(0.0, 40.0, 4001), np.linspace(40.0, 2000.0, 4001)))
    ref = np.stack([gaussian._boys(n, T) for n in range(nmax + 1)], axis=1)
    F = gto.boys(nmax, torch.as_tensor(T).cuda()).cpu().numpy()
    rel = np.abs(F - ref) / ref
    for n in range(nmax + 1):
        print(f"boys nmax={nmax} n={n}: max rel {rel[:, n].max():.3e} at T = {T[np.argmax(rel[:, n])]} "
              f"(bound {D.BOYS_RTOL[n]:.1e})")
    for n in range(nmax + 1):
        assert rel[:, n].max() < D.BOYS_RTOL[n]
    assert F[0] == pytest.approx([1.0 / (2 * n + 1) for n in range(nmax + 1)], rel=1e-15)


# ---- 5. M1 element by element ---------------------------------------------------------------------------------------
def _assert_exact_structure(I):
    g = I.int2e_ao
    assert torch.equal(g, g.permute(0, 2, 1, 3, 4)) and torch.equal(g, g.permute(0, 1, 2, 4, 3))
    assert torch.equal(g, g.permute(0, 3, 4, 1, 2))
    assert torch.equal(I.overlap, I.overlap.transpose(1, 2)) and torch.equal(I.int1e_ao, I.int1e_ao.transpose(1, 2))
    assert not torch.isnan(g).any() and int(I.info.abs().sum()) == 0


@pytest.mark.parametrize("form", ["spherical", "cartesian"])
def test_m1_integrals_element_by_element(form):
    basis = D.m1_basis(form)
    S, h, g, nuc = D.m1_host(form)
    # every element of the outputs is written: the tensors start as NaN
    N = basis.nao
    xyz = gto.coords_to_device(basis, D.M1_XYZ[None])
    out = [torch.full(s, float("nan"), dtype=torch.float64, device=xyz.device)
           for s in ((1, N, N), (1, N, N), (1, N, N, N, N), (1,))]
    gto.integrals_into(basis, xyz, *out)
    assert not any(torch.isnan(x).any().item() for x in out)
    I = gto.integrals_batch(basis, D.M1_XYZ[None])
    assert all(torch.equal(a, b) for a, b in zip(out, (I.overlap, I.int1e_ao, I.int2e_ao, I.nuc)))
    d = {"overlap": np.abs(I.overlap[0].cpu().numpy() - S).max(), "int1e_ao": np.abs(I.int1e_ao[0].cpu().numpy() - h).max(),
         "int2e_ao": np.abs(I.int2e_ao[0].cpu().numpy() - g).max(), "nuc": abs(I.nuc[0].item() - nuc)}
    print(form, {n: f"{v:.2e}" for n, v in d.items()})
    assert d["overlap"] < TOL_G and d["int2e_ao"] < TOL_G and d["nuc"] < TOL_G and d["int1e_ao"] < TOL_H
    _assert_exact_structure(I)
    assert ops.eri_flags(I.int2e_ao[0]) == 3


# ---- 6. a stack of three M1 geometries ------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["spherical", "cartesian"])
def test_m1_stack_bits_and_rigid_motions(form):
    basis = D.m1_basis(form)
    geos = np.stack([D.M1_XYZ, D.M1_ROTATED, D.M1_SHIFTED])
    I = gto.integrals_batch(basis, geos)
    _assert_exact_structure(I)
    for k in range(3):
        one = gto.integrals_batch(basis, geos[k:k + 1])
        for name in NAMES:
            assert torch.equal(getattr(I, name)[k], getattr(one, name)[0]), (name, k)
    side = ops.side_streams(torch.device("cuda", torch.cuda.current_device()))[0]
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        J = gto.integrals_batch(basis, geos)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for name in NAMES:
        assert torch.equal(getattr(I, name), getattr(J, name)), name
    res = scf.rhf_batch(I.int1e_ao, I.int2e_ao, I.overlap, basis.nelectron // 2, oao_coeff=I.oao_coeff)
    scf.raise_unless_converged(res.info, [0, 1, 2])
    e = (res.e_elec + I.nuc).cpu().numpy()
    print(form, "RHF of the geometry, its rotated and its translated copy:", e, "spread", e.max() - e.min())
    assert e.max() - e.min() < 1e-9
    # a translation leaves every integral over these functions unchanged up to rounding; a rotation does not
    assert (I.int2e_ao[0] - I.int2e_ao[2]).abs().max().item() < TOL_G
    assert (I.int2e_ao[0] - I.int2e_ao[1]).abs().max().item() > 1e-3


# ---- 7. M2 end to end -----------------------------------------------------------------------------------------------
def test_m2_from_geometries_to_a_newton_step():
    basis = D.m2_basis()
    geos = np.stack([D.WATER, D.WATER_2])
    pqc = aoo.Parameterized_circuit(2, 2, None, ansatz="np_fabric", n_layers=1)
    dev = aoo.OO_pqc_batch.from_geometries(pqc, basis, geos, 2, 2, oao_mo_coeffs="rhf", freeze_active=True)
    assert dev.nao == 18 and dev.eri_flags == 3 and dev._eri_packed is not None
    assert [ops.eri_flags(dev.int2e_ao[k]) for k in range(2)] == [3, 3]
    coeffs = [dev.oao_mo_coeff[k].cpu().numpy() for k in range(2)]
    mols = [aoo.Moldata(dev.int1e_ao[k].cpu().numpy(), dev.int2e_ao[k].cpu().numpy(), dev.overlap[k].cpu().numpy(),
                        dev.nuc[k].item(), basis.nelectron) for k in range(2)]
    host = aoo.OO_pqc_batch(pqc, mols, 2, 2, oao_mo_coeffs=coeffs, freeze_active=True)
    thetas = torch.as_tensor(np.random.default_rng(3).uniform(-0.5, 0.5, (2, dev.n_theta))).cuda()
    a, b = dev.energy_and_gradient(thetas), host.energy_and_gradient(thetas)
    print("dE", (a[:, 0] - b[:, 0]).abs().max().item(), "dgrad", (a[:, 1:] - b[:, 1:]).abs().max().item())
    assert (a[:, 0] - b[:, 0]).abs().max().item() < 1e-9
    assert (a[:, 1:] - b[:, 1:]).abs().max().item() < 1e-9
    # the CPU oracle on the same integrals
    omol = R.OracleMol(mols[0].int1e_ao, mols[0].int2e_ao, mols[0].overlap, mols[0].nuc, basis.nelectron)
    ooo = R.OracleOOPQC(R.OraclePQC(2, 2, "np_fabric", n_layers=1), omol, 2, 2, torch.as_tensor(coeffs[0]),
                        freeze_active=True)
    e_ref = ooo.energy_from_parameters(thetas[0].cpu()).item()
    print("E device", a[0, 0].item(), "oracle", e_ref)
    assert abs(a[0, 0].item() - e_ref) < 1e-9
    # the Hartree-Fock state at the RHF orbitals has the RHF energy, and one damped Newton step lowers every energy
    zero = torch.zeros((2, dev.n_theta), dtype=torch.float64).cuda()
    e0 = dev.energy(zero)
    assert (e0 - dev.rhf().e_tot).abs().max().item() < 1e-9
    _, e1, _ = dev.damped_newton_step(zero)
    print("E before", e0.cpu().numpy(), "after one damped Newton step", e1.cpu().numpy())
    assert (e1 < e0).all()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------
def test_nuclear_gradients_of_a_d_basis_are_refused_before_any_launch():
    basis = D.m2_basis()
    pqc = aoo.Parameterized_circuit(2, 2, None, ansatz="np_fabric", n_layers=1)
    batch = aoo.OO_pqc_batch.from_geometries(pqc, basis, D.WATER[None], 2, 2, oao_mo_coeffs="rhf", freeze_active=True)
    thetas = torch.zeros((1, batch.n_theta), dtype=torch.float64).cuda()
    with pytest.raises(NotImplementedError, match="d shells"):
        batch.nuclear_gradient(thetas)
    with pytest.raises(NotImplementedError, match="d shells"):
        batch.rhf_nuclear_gradient()
    with pytest.raises(NotImplementedError, match="d shells"):
        gto.gradient_batch(basis, D.WATER[None])
    # the C entry itself: a negative code whose text names l = 2, nothing launched
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    t = basis.device_tables(dev)
    xyz = gto.coords_to_device(basis, D.WATER[None], dev)
    size = int(lib.oovqe_gto_gradient_work_size(basis.nshell, basis.max_nprim, basis.natm, 1))
    assert size > 0
    work = torch.empty(size, dtype=torch.float64, device=dev)
    grad = torch.zeros((1, basis.natm, 3), dtype=torch.float64, device=dev)
    rc = lib.oovqe_gto_gradient_batch(basis.nshell, _lib.dptr(t.shells, torch.int32), int(basis.exps.size),
                                      _lib.dptr(t.exps), _lib.dptr(t.coefs), basis.natm, _lib.dptr(t.charges), 1,
                                      _lib.dptr(xyz), basis.nao, None, None, None, 1, _lib.dptr(grad), _lib.dptr(work),
                                      _lib.stream_ptr())
    assert rc < 0 and b"l = 2" in lib.oovqe_last_error()
    torch.cuda.synchronize()
    assert torch.equal(grad, torch.zeros_like(grad))
    # and the integrals of a table with an f shell or a misplaced flag are refused the same way
    bad = t.shells.clone()
    bad[0, 1] = gto.CARTESIAN                              # the Cartesian flag on an s shell
    I = torch.empty((1, basis.nao, basis.nao), dtype=torch.float64, device=dev)
    rc = lib.oovqe_gto_integrals_batch(basis.nshell, _lib.dptr(bad, torch.int32), int(basis.exps.size),
                                       _lib.dptr(t.exps), _lib.dptr(t.coefs), basis.natm, _lib.dptr(t.charges), 1,
                                       _lib.dptr(xyz), basis.nao, _lib.dptr(I), None, None, None,
                                       _lib.dptr(basis.work(dev, 1)), _lib.stream_ptr())
    assert rc < 0 and b"OOVQE_GTO_CARTESIAN" in lib.oovqe_last_error()
