"""The gradient-sets contraction (csrc/gto_grad_sets.hip, ``gto.gradient_sets_into``) and the state and interstate
gradients of CASCI roots (``OO_pqc_batch.casci_nuclear_gradients``, ``nucgrad.branching_plane``) on the device.

Raw contraction: every set of a call against ``gto.gradient_into`` on that set alone (1e-12 absolute: the same integrals
summed in another association; tests/test_nucgrad_gpu.py measured 7e-15 for the whole against its parts), against 4th-order
finite differences of ``gto.integrals_into`` contractions, and bit for bit against itself in other company.

CASCI gradients: the reference is made from entry points that existed before the feature.  The CI vectors c come from the
call under test at the centre; the displaced copies (+-h, +-2h per coordinate, the same ``oao_mo_coeff``) give c0 | c1 | c2
through the batch's CAS call as ``OO_pqc_batch.casci`` reads them, ``tests/_ci_dense.hamiltonian`` makes H(R) of each, and
the finite difference of ``M(R) = c^T H(R) c`` is the whole [R, R, natm, 3] matrix.  Every bound is 10 x the disagreement
of that reference at h = 1e-3 with itself at h = 2e-3, per case; the figures are printed before every assertion.

The diagonal is compared with finite differences of ``casci`` energies too, for roots more than 1e-3 Ha from their
neighbours; that reference has an error of its own, so the bound there is 10 x the larger of the two references'
disagreements with themselves.

No figure is quoted here: no MI355X was available when these tests were written ("State and interstate
gradients").  Every test prints its figures before it asserts."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import auto_oo_amd as aoo                                   # noqa: E402
from auto_oo_amd import gto, nucgrad, ops                   # noqa: E402
from auto_oo_amd.gaussian import BOHR                       # noqa: E402
from auto_oo_amd.moldata import get_formal_geo              # noqa: E402
from tests import _casci_gradients as C                     # noqa: E402
from tests import _gto_d as D                               # noqa: E402

F64 = torch.float64
T = gto.GRAD_SETS_TILE
TERMS = ("dm1", "wq", "dm2")


def sets_call(name, K, which, xyz=None, order=None, nuc=None):
    """the sets contraction of the case with the seeded sets (``order``: a permutation of them) at every geometry"""
    basis, centre = C.case(name)
    x = torch.as_tensor(centre if xyz is None else xyz).to(C.dev()).contiguous()
    G = int(x.shape[0])
    d = C.density_sets(name, K)
    bits = C.nuc_bits(K) if nuc is None else nuc
    if order is not None:
        d = tuple(t[order].contiguous() for t in d)
        bits = [bits[k] for k in order]
    arg = {t: C.expand(v, G) if t in which else None for t, v in zip(TERMS, d)}
    return gto.gradient_sets_into(basis, x, arg["dm1"], arg["wq"], arg["dm2"], bits)


def single_call(name, k, K, which, with_nuc, xyz=None):
    basis, centre = C.case(name)
    x = torch.as_tensor(centre if xyz is None else xyz).to(C.dev()).contiguous()
    G = int(x.shape[0])
    d = C.density_sets(name, K)
    arg = {t: C.expand(v[k], G) if t in which else None for t, v in zip(TERMS, d)}
    return gto.gradient_into(basis, x, arg["dm1"], arg["wq"], arg["dm2"], with_nuc)


# ---- 1. the raw contraction against the single-set entry ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["h2", "hf", "water", "formaldimine"])
def test_every_set_against_the_single_set_entry(name):
    """K = 1, 2, T, T + 1 and 10 sets of different seeds with alternating nuclear flags, each term alone and all
    together: every set within 1e-12 of ``gto.gradient_into`` on that set."""
    worst = 0.0
    for K in sorted({1, 2, T, T + 1, gto.MAX_GRAD_SETS}):
        for which in (("dm1",), ("wq",), ("dm2",), TERMS):
            got = sets_call(name, K, which)
            assert tuple(got.shape) == (C.case(name)[1].shape[0], K) + tuple(C.case(name)[1].shape[1:])
            for k in range(K):
                want = single_call(name, k, K, which, C.nuc_bits(K)[k])
                err = (got[:, k] - want).abs().max().item()
                worst = max(worst, err)
                assert err <= 1e-12, (name, K, which, k, err)
    print(f"{name}: largest difference of a set from the single-set entry {worst:.2e} (bound 1e-12)")


# ---- 2. against finite differences ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["water", "hf"])
def test_three_sets_against_finite_differences(name):
    """K = 3: 4th-order central differences of D1_k . h + WQ_k . S + 1/2 D2_k . g (+ E_nuc where set k has the flag) from
    ``gto.integrals_into`` at h = 1e-3; bound per set 10 x that reference's disagreement with h = 2e-3."""
    basis, centre = C.case(name)
    K, N = 3, basis.nao
    d1, wq, d2 = C.density_sets(name, K)
    flags = torch.as_tensor(C.nuc_bits(K), dtype=F64, device=C.dev())
    ref = []
    for h in (C.H1, C.H2):
        xyz = torch.as_tensor(C.fd_stack(centre[0], h)).to(C.dev()).contiguous()
        G = int(xyz.shape[0])
        S = torch.empty((G, N, N), dtype=F64, device=C.dev())
        hc = torch.empty_like(S)
        g = torch.empty((G,) + (N,) * 4, dtype=F64, device=C.dev())
        nuc = torch.empty(G, dtype=F64, device=C.dev())
        gto.integrals_into(basis, xyz, S, hc, g, nuc)
        val = ((hc[None] * d1[:, None]).sum(dim=(2, 3)) + (S[None] * wq[:, None]).sum(dim=(2, 3))
               + 0.5 * (g[None] * d2[:, None]).sum(dim=(2, 3, 4, 5)) + flags[:, None] * nuc[None])          # [K, G]
        ref.append(C.fd_combine(val, h).cpu().numpy())
    got = sets_call(name, K, TERMS)[0].cpu().numpy()
    for k in range(K):
        dis = np.abs(ref[0][k] - ref[1][k]).max()
        err = np.abs(got[k] - ref[0][k]).max()
        print(f"{name} set {k}: max |grad| {np.abs(ref[0][k]).max():.3g}, reference disagreement {dis:.2e}, "
              f"bound {10 * dis:.2e}, error {err:.2e}")
        assert err < 10 * dis, (name, k, err, dis)


# ---- 3. bits --------------------------------------------------------------------------------------------------------------
def test_a_set_has_the_same_bits_alone_among_others_and_at_another_place():
    xyz = C.five_geometries()
    K = gto.MAX_GRAD_SETS
    full = sets_call("formaldimine", K, TERMS, xyz)
    bits = C.nuc_bits(K)
    for k in (0, 3, T, K - 1):
        alone = sets_call("formaldimine", K, TERMS, xyz, order=[k])
        assert torch.equal(alone[:, 0], full[:, k]), k
    order = [7, 2, 9, 0, 5, 1, 8, 3, 6, 4]
    assert torch.equal(sets_call("formaldimine", K, TERMS, xyz, order=order), full[:, order])
    few = sets_call("formaldimine", K, TERMS, xyz, order=[8, 1, 4])                   # one tile, other neighbours
    assert torch.equal(few, full[:, [8, 1, 4]])
    assert not torch.equal(full[:, 0], full[:, 2])
    # the flags follow their sets: with all of them flipped every set differs
    flipped = sets_call("formaldimine", K, TERMS, xyz, nuc=[not b for b in bits])
    assert all(not torch.equal(flipped[:, k], full[:, k]) for k in range(K))


def test_a_permuted_stack_and_a_geometry_alone_give_the_same_bits():
    xyz = C.five_geometries()
    full = sets_call("formaldimine", T + 1, TERMS, xyz)
    perm = [3, 0, 4, 2, 1]
    assert torch.equal(sets_call("formaldimine", T + 1, TERMS, xyz[perm]), full[perm])
    for g in range(5):
        assert torch.equal(sets_call("formaldimine", T + 1, TERMS, xyz[g:g + 1])[0], full[g]), g
    assert not torch.equal(full[0], full[1])


def test_a_call_on_another_stream_gives_the_same_bits():
    xyz = C.five_geometries()
    full = sets_call("formaldimine", T + 1, TERMS, xyz)
    side = ops.side_streams(C.dev())[0]
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = sets_call("formaldimine", T + 1, TERMS, xyz)          # (the basis keeps one work buffer per stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(full, other)


# ---- 4. CASCI gradients -----------------------------------------------------------------------------------------------------
CASES = [("h2", 2, 2, 3, True), ("hf", 2, 2, 2, True), ("water", 3, 4, 2, True), ("water", 3, 4, 2, False),
         ("formaldimine", 2, 2, 3, True), ("formaldimine", 3, 4, 4, True)]
LINEAR = ("h2", "hf")


@pytest.mark.parametrize("name,ncas,nelecas,R,fix_singlet", CASES)
def test_casci_gradient_matrix_against_finite_differences(name, ncas, nelecas, R, fix_singlet):
    """The whole matrix against finite differences of c^T H(R) c at fixed c; the diagonal of well separated roots against
    finite differences of the ``casci`` energies as well (not for H-F, whose roots are degenerate by symmetry); exact
    symmetry in (I, J); the net force of every element; ``branching_plane``."""
    b = C.batch(name, ncas, nelecas)
    res = b.casci_nuclear_gradients(nroots=R, fix_singlet=fix_singlet)
    G, natm = b.G, b.basis.natm
    assert tuple(res.energies.shape) == (G, R) and tuple(res.gradients.shape) == (G, R, R, natm, 3)
    assert tuple(res.ci.shape[:2]) == (G, R)
    e_ref, c_ref = b.casci(R, fix_singlet)
    assert torch.equal(res.energies, e_ref) and torch.equal(res.ci, c_ref)
    grads = res.gradients
    assert torch.equal(grads, grads.transpose(1, 2))
    got = grads.cpu().numpy()
    energies = res.energies.cpu().numpy()
    for g in range(G):
        with_e = name != "hf"
        ref = C.matrix_reference(name, ncas, nelecas, g, res.ci[g].cpu().numpy(), R if with_e else None, fix_singlet)
        want, dis = ref[0], ref[1]
        err = np.abs(got[g] - want).max()
        diag = max(np.abs(want[i, i]).max() for i in range(R))
        off = max([np.abs(want[i, j]).max() for i in range(R) for j in range(i)] or [0.0])
        net = np.abs(got[g].sum(axis=2)).max()
        print(f"{name} CAS({nelecas}e,{ncas}o) R = {R} singlet {fix_singlet} geometry {g}: elements up to {diag:.3g} "
              f"(diagonal), {off:.3g} (off-diagonal); reference disagreement {dis:.2e}, bound {10 * dis:.2e}, error "
              f"{err:.2e}, net force {net:.2e}")
        assert err < 10 * dis, (name, g, err, dis)
        assert net < 10 * dis, (name, g, net, dis)
        if with_e:
            e_fd, e_dis = ref[2], ref[3]
            e = energies[g]
            gap = [min([abs(e[i] - e[j]) for j in (i - 1, i + 1) if 0 <= j < R]) for i in range(R)]
            ok = [i for i in range(R) if gap[i] > 1e-3]
            for i in ok:
                d = np.abs(got[g, i, i] - e_fd[i]).max()
                print(f"    root {i}: gap {gap[i]:.3g}, dE/dR against finite differences of casci energies {d:.2e} "
                      f"(their disagreement {e_dis:.2e}, bound {10 * max(dis, e_dis):.2e})")
                assert d < 10 * max(dis, e_dis), (name, g, i, d)
            if name not in LINEAR:
                assert len(ok) >= 2, (name, g, gap)
    if R > 1:
        gv, hv = nucgrad.branching_plane(res, 0, 1)
        assert torch.equal(gv, 0.5 * (grads[:, 1, 1] - grads[:, 0, 0])) and torch.equal(hv, grads[:, 0, 1])


def test_index_chunk_and_one_root():
    b = C.batch("formaldimine", 3, 4)
    full = b.casci_nuclear_gradients(nroots=2)
    by_one = b.casci_nuclear_gradients(nroots=2, chunk=1)
    assert torch.equal(by_one.gradients, full.gradients) and torch.equal(by_one.energies, full.energies)
    part = b.casci_nuclear_gradients(nroots=2, index=[2, 0])
    assert torch.equal(part.gradients, full.gradients[[2, 0]]) and torch.equal(part.energies, full.energies[[2, 0]])
    assert torch.equal(part.ci, full.ci[[2, 0]])
    one = b.casci_nuclear_gradients(nroots=2, index=1)
    assert torch.equal(one.gradients, full.gradients[1:2])
    # one root alone: the [0, 0] block, up to what the two solves differ by (10 x the CASCI tolerance of 1e-9)
    single = b.casci_nuclear_gradients(nroots=1)
    assert tuple(single.gradients.shape) == (3, 1, 1, 5, 3)
    d = (single.gradients[:, 0, 0] - full.gradients[:, 0, 0]).abs().max().item()
    print(f"nroots = 1 against the [0, 0] block of nroots = 2: {d:.2e} (bound 1e-8)")
    assert d < 10 * 1e-9


def test_errors(monkeypatch):
    pqc = C.circuit(2, 2)
    from auto_oo_amd.gaussian import Moldata_sto3g
    mol = Moldata_sto3g(get_formal_geo(*C.POINTS[0]))
    host = aoo.OO_pqc_batch(pqc, [mol], 2, 2, oao_mo_coeffs=[np.eye(13)])
    with pytest.raises(RuntimeError, match="from_geometries"):
        host.casci_nuclear_gradients()
    dbatch = aoo.OO_pqc_batch.from_geometries(pqc, D.m2_basis(), D.WATER[None], 2, 2, oao_mo_coeffs="rhf",
                                              freeze_active=True)
    with pytest.raises(NotImplementedError, match="d shells"):
        dbatch.casci_nuclear_gradients()
    b = C.batch("formaldimine", 2, 2)
    with pytest.raises(ValueError):
        b.casci_nuclear_gradients(index=[3])
    with pytest.raises(ValueError, match="nroots"):
        b.casci_nuclear_gradients(nroots=5)                    # ci.check_scope
    with pytest.raises(ValueError, match="nroots"):
        b.casci_nuclear_gradients(nroots=0)
    big = copy.copy(b)
    big.ncas = nucgrad.MAX_NCAS + 1
    with pytest.raises(NotImplementedError, match="ncas"):
        big.casci_nuclear_gradients()
    # a solve that reports itself unconverged raises as in ``casci`` (the flag of geometry 1 set on the solver's way out)
    from auto_oo_amd import ci
    solver = ci.casci_packed

    def unconverged(*args, **kw):
        e, vecs, s2, rn, info = solver(*args, **kw)
        info = info.clone()
        info[1] = 7
        return e, vecs, s2, rn, info
    monkeypatch.setattr(ci, "casci_packed", unconverged)
    with pytest.raises(RuntimeError, match=r"geometries \[1\] did not converge"):
        b.casci_nuclear_gradients(nroots=2)
    monkeypatch.undo()
    basis, xyz = C.case("formaldimine")
    x = torch.as_tensor(xyz).to(C.dev())
    N = basis.nao
    z = torch.zeros((3, 2, N, N), dtype=F64, device=C.dev())
    with pytest.raises(ValueError):
        gto.gradient_sets_into(basis, x, dm1=z[:2])
    with pytest.raises(ValueError):
        gto.gradient_sets_into(basis, x, dm1=z, nuc=[True])
    # densities of zeros: the nuclear term alone where the flag is set, exact zeros elsewhere; Angstrom input
    g = gto.gradient_sets_batch(basis, xyz * BOHR, dm1=z, nuc=[True, False])
    assert g[:, 1].abs().max().item() == 0.0
    assert torch.equal(g[:, 0], gto.gradient_into(basis, x, torch.zeros((3, N, N), dtype=F64, device=C.dev())))
