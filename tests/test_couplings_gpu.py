"""The derivative couplings of CASCI roots on the device: the one-sided overlap-derivative contraction
(csrc/gto_connection.hip, ``gto.overlap_connection_batch``), the transition 1-RDM (csrc/sector_trdm.hip,
``ci.transition_rdm1``) and ``OO_pqc_batch.casci_derivative_couplings``.

Raw contraction: against the host twin ``gaussian.overlap_connection_from_table`` contracted in numpy and, for symmetric
matrices, against ``gto.gradient_batch(wq=D / 2)``, 1e-12 absolute on values of order 1 (fp64, the same formulas), and bit
for bit against itself in other company.  Transition RDM: against ``c_I^T E_pq c_J`` with the dense excitation matrices of
tests/_ci_dense.py, 1e-13.

Couplings: the reference is the finite difference of exact overlaps of tests/_couplings.py, made from entry points that
existed before the feature.  Every bound is 10 x the disagreement of that reference at h = 1e-3 with itself at h = 2e-3, per
case, and a case counts only if that disagreement is below 1e-4 of the largest coupling of the reference and every gap of
the case exceeds 1e-3 Ha.  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import auto_oo_amd as aoo                                   # noqa: E402
from auto_oo_amd import ci, gaussian, gto, ops, overlaps   # noqa: E402
from auto_oo_amd.gaussian import BOHR                       # noqa: E402
from auto_oo_amd.moldata import get_formal_geo              # noqa: E402
from tests import _casci_gradients as C                     # noqa: E402
from tests import _ci_dense                                 # noqa: E402
from tests import _couplings as Q                           # noqa: E402
from tests import _gto_d as D                               # noqa: E402

F64 = torch.float64
NAMES = ["h2", "hf", "water", "formaldimine"]
NSETS = [1, 5, 6, 10]                                       # one tile, a full tile, two tiles (3 + 3, 5 + 5)


def first_point(name):
    basis, xyz = C.case(name)
    return basis, xyz[:1]


def connection_call(name, mats, xyz=None):
    """``gto.overlap_connection_into`` for the matrices ``mats`` [K, N, N] (host), the same in every geometry"""
    basis, x0 = first_point(name)
    x = torch.as_tensor(x0 if xyz is None else xyz).to(C.dev())
    return gto.overlap_connection_into(basis, x, C.expand(torch.as_tensor(mats).to(C.dev()), int(x.shape[0])))


# ---- 1. the one-sided overlap-derivative contraction -------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_connection_against_the_host_twin(name):
    basis, xyz = first_point(name)
    T = gaussian.overlap_connection_from_table(basis.table, xyz[0])
    for K in NSETS:
        mats = Q.general_matrices(basis.nao, K)
        assert np.abs(mats[0] - mats[0].T).max() > 0.5 and np.abs(mats[0] + mats[0].T).max() > 0.5
        got = connection_call(name, mats).cpu().numpy()
        assert got.shape == (1, K, basis.natm, 3)
        want = np.einsum("kmn,admn->kad", mats, T)
        err = np.abs(got[0] - want).max()
        print(f"{name} nset = {K}: values up to {np.abs(want).max():.3g}, against the host twin {err:.2e} (bound 1e-12)")
        assert err < 1e-12, (name, K, err)


@pytest.mark.parametrize("name", NAMES)
def test_connection_of_a_symmetric_matrix_is_half_the_overlap_gradient(name):
    basis, xyz = first_point(name)
    mats = Q.general_matrices(basis.nao, 6)
    sym = mats + mats.transpose(0, 2, 1)
    got = connection_call(name, sym)[0]
    for k in range(6):
        wq = torch.as_tensor(0.5 * sym[k:k + 1]).to(C.dev())
        want = gto.gradient_batch(basis, xyz * BOHR, wq=wq, nuc=False)[0]
        err = (got[k] - want).abs().max().item()
        print(f"{name} set {k}: values up to {want.abs().max().item():.3g}, against gradient_batch(wq = D / 2) {err:.2e} "
              "(bound 1e-12)")
        assert err < 1e-12, (name, k, err)


def test_connection_has_the_same_bits_in_other_company():
    """a matrix alone, among others, at another place and in another tile split; a permuted stack; a geometry alone"""
    basis, xyz = C.case("formaldimine")
    mats = Q.general_matrices(basis.nao, 10)
    full = connection_call("formaldimine", mats, xyz)                                   # two tiles of 5
    assert tuple(full.shape) == (3, 10, basis.natm, 3)
    for k in (0, 4, 7):
        assert torch.equal(connection_call("formaldimine", mats[k:k + 1], xyz)[:, 0], full[:, k])
    order = [8, 1, 4, 6]
    assert torch.equal(connection_call("formaldimine", mats[order], xyz), full[:, order])      # one tile
    assert torch.equal(connection_call("formaldimine", mats[:6], xyz), full[:, :6])            # tiles of 3
    perm = [2, 0, 1]
    assert torch.equal(connection_call("formaldimine", mats, xyz[perm]), full[perm])
    assert torch.equal(connection_call("formaldimine", mats, xyz[1:2]), full[1:2])
    five = connection_call("formaldimine", mats, C.five_geometries())                   # more than one workgroup
    assert torch.equal(five[:3], full)
    # Angstrom input, and the argument checks
    dm = C.expand(torch.as_tensor(mats[:2]).to(C.dev()), 3)
    assert torch.equal(gto.overlap_connection_batch(basis, xyz * BOHR, dm), full[:, :2])
    x = torch.as_tensor(xyz).to(C.dev())
    with pytest.raises(ValueError):
        gto.overlap_connection_into(basis, x, dm[:2])
    with pytest.raises(ValueError):
        gto.overlap_connection_into(basis, x, dm[:, 0])
    with pytest.raises(ValueError):
        gto.overlap_connection_into(basis, x, C.expand(torch.as_tensor(Q.general_matrices(basis.nao, 11)).to(C.dev()), 3))
    with pytest.raises(NotImplementedError, match="d shells"):
        dbasis = D.m2_basis()
        gto.overlap_connection_batch(dbasis, D.WATER[None], torch.zeros((1, 1, dbasis.nao, dbasis.nao), dtype=F64,
                                                                        device=C.dev()))


# ---- 2. the transition 1-RDM --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncas,nelecas,n", [(2, 2, 4), (3, 4, 4), (8, 8, 1)])
def test_transition_rdm1_against_dense_excitation_matrices(ncas, nelecas, n):
    dc = ci.ci_dimension(ncas, nelecas)
    rng = np.random.default_rng(7 + ncas)
    bra, ket = rng.standard_normal((n, dc)), rng.standard_normal((n, dc))
    bra /= np.linalg.norm(bra, axis=1, keepdims=True)
    ket /= np.linalg.norm(ket, axis=1, keepdims=True)
    tb, tk = torch.as_tensor(bra).to(C.dev()), torch.as_tensor(ket).to(C.dev())
    got = ci.transition_rdm1(tb, tk, ncas, nelecas)
    assert tuple(got.shape) == (n, ncas, ncas)
    Es = _ci_dense.excitation_matrices(ncas, nelecas, sparse=True)
    want = np.array([[[bra[k] @ (Es[p][q] @ ket[k]) for q in range(ncas)] for p in range(ncas)] for k in range(n)])
    err = np.abs(got.cpu().numpy() - want).max()
    asym = np.abs(want - want.transpose(0, 2, 1)).max()
    print(f"CAS({nelecas}e,{ncas}o), {dc} determinants: elements up to {np.abs(want).max():.3g}, antisymmetric part up to "
          f"{asym / 2:.3g}; against c_I^T E_pq c_J {err:.2e} (bound 1e-13)")
    assert err < 1e-13
    assert asym > 1e-3                                       # NOT symmetric for different vectors
    assert (got - got.transpose(1, 2)).abs().max().item() > 1e-3
    # bra and ket exchanged: the transpose; a pair has the same bits alone
    back = ci.transition_rdm1(tk, tb, ncas, nelecas)
    assert (back - got.transpose(1, 2)).abs().max().item() < 1e-13
    assert torch.equal(ci.transition_rdm1(tb[-1:], tk[-1:], ncas, nelecas), got[-1:])
    # equal bra and ket: the gamma of sector_rdms
    same = ci.transition_rdm1(tk, tk, ncas, nelecas)
    g1 = ci.sector_rdms(tk, ncas, nelecas)[0]
    d = (same - g1).abs().max().item()
    print(f"    equal bra and ket against sector_rdms: {d:.2e} (bound 1e-13)")
    assert d < 1e-13


def test_transition_rdm1_errors():
    z = torch.zeros((2, 9), dtype=F64, device=C.dev())
    with pytest.raises(ValueError):
        ci.transition_rdm1(z, z[:1], 3, 4)
    with pytest.raises(ValueError):
        ci.transition_rdm1(z, z, 2, 2)
    with pytest.raises(ValueError):
        ci.transition_rdm1(z, z, 9, 8)
    assert tuple(ci.transition_rdm1(z[:0], z[:0], 3, 4).shape) == (0, 3, 3)


# ---- 3. the couplings -----------------------------------------------------------------------------------------------------
# (water without ``fix_singlet``: three roots, not two -- the two lowest states of the sector are a singlet and a triplet,
# whose coupling vanishes by spin symmetry, so that the reference of that pair alone is noise: measured 1.5e-11 with a
# disagreement of 2.2e-10)
CASES = [("h2", 2, 2, 3, True), ("hf", 2, 2, 2, True), ("water", 3, 4, 2, True), ("water", 3, 4, 3, False),
         ("formaldimine", 2, 2, 3, True)]


def connection_net(b, res, R):
    """sum over the atoms of the ``Da . T^A`` part alone [G, R, R, 3], from the public pieces"""
    G, a, N = b.G, b.ncas, b.nao
    out = torch.zeros((G, R, R, 3), dtype=F64, device=b.device)
    Ca = b.mo_coeff[:, :, b._n_occ:b._n_occ + a].contiguous()
    for i in range(R):
        for j in range(i):
            t = ci.transition_rdm1(res.ci[:, i], res.ci[:, j], a, b.nelecas)
            asym = (0.5 * (t - t.transpose(1, 2))).contiguous()
            Da = ops.matmul_nn_batch(ops.matmul_nn_batch(Ca, asym), Ca.transpose(1, 2).contiguous())
            net = gto.overlap_connection_into(b.basis, b.coords_bohr, Da[:, None])[:, 0].sum(1)
            out[:, i, j], out[:, j, i] = net, -net
    return out


@pytest.mark.parametrize("name,ncas,nelecas,R,fix_singlet", CASES)
def test_couplings_against_finite_differences_of_exact_overlaps(name, ncas, nelecas, R, fix_singlet):
    """``couplings`` of geometry 0 of the case against the reference; couplings = ci_term + orbital_term; exact
    antisymmetry and a zero diagonal; the sum rule: the net over the atoms is that of the ``Da . T^A`` part alone."""
    b = C.batch(name, ncas, nelecas)
    res = b.casci_derivative_couplings(nroots=R, fix_singlet=fix_singlet, tol=1e-11)
    G, natm = b.G, b.basis.natm
    for x in (res.gradients, res.couplings, res.ci_term, res.orbital_term):
        assert tuple(x.shape) == (G, R, R, natm, 3)
    assert tuple(res.energies.shape) == (G, R) and tuple(res.ci.shape[:2]) == (G, R)
    k = torch.arange(R)
    for x in (res.couplings, res.ci_term, res.orbital_term):
        assert torch.equal(x, -x.transpose(1, 2))
        assert x[:, k, k].abs().max().item() == 0.0
    assert torch.equal(res.couplings, res.ci_term + res.orbital_term)
    plain = b.casci_nuclear_gradients(nroots=R, fix_singlet=fix_singlet, tol=1e-11)
    assert torch.equal(res.gradients, plain.gradients) and torch.equal(res.energies, plain.energies)
    assert torch.equal(res.ci, plain.ci)

    want, dis, e_ref, c_ref = Q.coupling_reference(name, ncas, nelecas, 0, R, fix_singlet)
    top = np.abs(want).max()
    gaps = [abs(e_ref[i] - e_ref[j]) for i in range(R) for j in range(i)]
    got = res.couplings[0].cpu().numpy()
    orb = res.orbital_term[0].abs().max().item()
    # (the reference's vectors carry the signs ``casci`` fixes; where two components tie the dot product decides)
    dots = np.einsum("rc,rc->r", res.ci[0].cpu().numpy(), c_ref)
    want = want * (np.sign(dots)[:, None] * np.sign(dots)[None, :])[:, :, None, None]
    signs = np.abs(dots)
    err = np.abs(got - want).max()
    net = (res.couplings.sum(3) - connection_net(b, res, R))[0].abs().max().item()
    print(f"{name} CAS({nelecas}e,{ncas}o) R = {R} singlet {fix_singlet}: couplings up to {top:.3g} (orbital term up to "
          f"{orb:.3g}), smallest gap {min(gaps):.3g} Ha; reference disagreement {dis:.2e} ({dis / top:.1e} of the largest), "
          f"bound {10 * dis:.2e}, error {err:.2e}; net of the CI and S^-1/2 terms over the atoms {net:.2e}; "
          f"|<c|c_ref>| from {signs.min():.12f}")
    # the reference alone: tight enough to see a failure, and well separated roots
    assert dis < 1e-4 * top, (name, dis, top)
    assert min(gaps) > 1e-3, (name, gaps)
    assert err < 10 * dis, (name, err, dis)
    assert net < 10 * dis, (name, net, dis)
    if name in ("hf", "water"):
        assert orb > 1e-3 * np.abs(got).max(), (name, orb)


def test_index_chunk_and_the_gap(monkeypatch):
    b = C.batch("formaldimine", 3, 4)
    full = b.casci_derivative_couplings(nroots=3)
    by_one = b.casci_derivative_couplings(nroots=3, chunk=1)
    part = b.casci_derivative_couplings(nroots=3, index=[2, 0])
    one = b.casci_derivative_couplings(nroots=3, index=1)
    for f in ("energies", "ci", "gradients", "couplings", "ci_term", "orbital_term"):
        x = getattr(full, f)
        assert torch.equal(getattr(by_one, f), x), f
        assert torch.equal(getattr(part, f), x[[2, 0]]), f
        assert torch.equal(getattr(one, f), x[1:2]), f
    # a gap below min_gap: raised before the pass over the derivative integrals, or marked
    e = full.energies.cpu().numpy()
    gaps = sorted((abs(e[k, i] - e[k, j]), k, i, j) for k in range(3) for i in range(3) for j in range(i))
    (_, g, i, j), between = gaps[0], 0.5 * (gaps[0][0] + gaps[1][0])
    called = []
    keep = gto.gradient_sets_into
    monkeypatch.setattr(gto, "gradient_sets_into", lambda *a, **kw: called.append(1) or keep(*a, **kw))
    with pytest.raises(ValueError, match=rf"\({g}, {i}, {j}\)"):
        b.casci_derivative_couplings(nroots=3, min_gap=between)
    assert not called
    b.casci_derivative_couplings(nroots=3, min_gap=between, index=[k for k in range(3) if k != g])
    assert called
    monkeypatch.undo()
    marked = b.casci_derivative_couplings(nroots=3, min_gap=between, small_gap="nan")
    nan = torch.isnan(marked.couplings)
    want = torch.zeros_like(nan)
    want[g, i, j] = want[g, j, i] = True
    assert torch.equal(nan, want) and torch.equal(torch.isnan(marked.ci_term), want)
    assert torch.equal(marked.orbital_term, full.orbital_term) and bool(torch.isfinite(marked.orbital_term).all())
    assert torch.equal(marked.couplings[~want], full.couplings[~want])
    with pytest.raises(ValueError, match="small_gap"):
        b.casci_derivative_couplings(small_gap="ignore")


def test_errors():
    pqc = C.circuit(2, 2)
    from auto_oo_amd.gaussian import Moldata_sto3g
    mol = Moldata_sto3g(get_formal_geo(*C.POINTS[0]))
    host = aoo.OO_pqc_batch(pqc, [mol], 2, 2, oao_mo_coeffs=[np.eye(13)])
    with pytest.raises(RuntimeError, match="from_geometries"):
        host.casci_derivative_couplings()
    dbatch = aoo.OO_pqc_batch.from_geometries(pqc, D.m2_basis(), D.WATER[None], 2, 2, oao_mo_coeffs="rhf",
                                              freeze_active=True)
    with pytest.raises(NotImplementedError, match="d shells"):
        dbatch.casci_derivative_couplings()
    b = C.batch("formaldimine", 2, 2)
    with pytest.raises(ValueError):
        b.casci_derivative_couplings(index=[3])
    with pytest.raises(ValueError, match="nroots"):
        b.casci_derivative_couplings(nroots=5)
    one = b.casci_derivative_couplings(nroots=1)                   # one root: nothing to couple
    assert tuple(one.couplings.shape) == (3, 1, 1, 5, 3) and one.couplings.abs().max().item() == 0.0


def test_apply_tracking_restores_the_couplings(monkeypatch):
    """a two-geometry path; the roots of the second geometry swapped and one of them turned round by hand"""
    basis, xyz = C.case("water")
    two = np.concatenate([xyz, xyz])
    two[1, 1, 0] += 0.01
    U = [C.rotated_orbitals("water")[0]] * 2
    b = aoo.OO_pqc_batch.from_geometries(C.circuit(3, 4), basis, two * BOHR, 3, 4, oao_mo_coeffs=U)
    R = 3
    true = b.casci_derivative_couplings(nroots=R, tol=1e-11)
    e, vecs = b.casci(R, True, 1e-11, 200)
    p0, s0 = overlaps.track_roots(b.casci_overlaps(R, vecs=vecs)[2])
    e2, v2 = e.clone(), vecs.clone()
    e2[1] = e[1, [1, 0, 2]]
    v2[1] = vecs[1, [1, 0, 2]]
    v2[1, 0] *= -1.0
    monkeypatch.setattr(b, "casci", lambda *a, **kw: (e2, v2))
    mixed = b.casci_derivative_couplings(nroots=R, tol=1e-11)
    monkeypatch.undo()
    p, s = overlaps.track_roots(b.casci_overlaps(R, vecs=v2)[2])
    assert p[1].tolist() != p0[1].tolist()
    want = overlaps.apply_tracking(true.couplings, p0, s0)
    got = overlaps.apply_tracking(mixed.couplings, p, s)
    top = want.abs().max().item()
    changed = (mixed.couplings - true.couplings).abs().max().item()
    err = (got - want).abs().max().item()
    # the same products in another order and with other signs: rounding alone, 1e-10 of the largest element
    print(f"couplings up to {top:.3g}; swapping and turning changed them by {changed:.3g}; after apply_tracking {err:.2e} "
          f"(bound {1e-10 * top:.2e})")
    assert changed > 1e-3 * top
    assert err < 1e-10 * top
    assert torch.equal(got, -got.transpose(1, 2))
