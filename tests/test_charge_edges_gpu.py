"""The point-charge kernels (csrc/gto_charges.hip) and the connection kernel (csrc/gto_connection.hip) at the limits of
their shell table: contractions of 1 to 10 primitives in both orientations of a pair, clouds beyond one pass of the
operator's 256 lanes, d shells of both forms at Boys orders up to 4 and arguments from 0 to 1e8, dissociated, nearly
coincident, far-away and collinear geometries, two-centre pp and unswapped ps pairs in the gradient, and molecules
whose atoms' shares fill the dynamic LDS of the gradient kernel up to its limit.  Cases, clouds and references:
tests/_charge_edges.py.

Bounds (none taken from device output):

* operator against the host twin ``gaussian.point_charge_integrals_from_table``: 10 x the largest change that a Boys
  function perturbed by ``_gto_d.BOYS_RTOL`` makes to the twin's V_ext of the very case, d form and cloud (``diff`` of
  the fixture) -- the rule of tests/test_gto_edges_gpu.py.  G4 against G1: 10 x what the twin shows between the two.
  Between the fragments of G2 the twin gives exactly 0.0, and so must the device.
* the nuclei as the charges against ``int1e_ao`` minus the host kinetic energy: 10 x ``diff_nuclei`` (the same change
  for that cloud) plus ``diff_h`` of the gto_edges fixture.
* gradients against central differences of the host twin: per component ``max(1e-9, 10 |FD - FD'|)`` with the two steps
  of the rule stored in the fixture (tests/_charge_edges.py lists every case's disagreement; all are below 1e-8); the
  classical term against its closed form at 1e-12 relative; the net force of atoms and charges together below
  1e-10 x (natm + M) Ha/Bohr -- the rules of tests/test_charges_gpu.py.
* connection against ``einsum(mats, gaussian.overlap_connection_from_table)`` and, for symmetric matrices, against
  ``gto.gradient_batch(wq = D / 2)``: 1e-12 x the largest sum of |mats| |T| of the case
  (``_charge_edges.connection_scale``).

Every test prints its figures next to the bound before it asserts.  Measured on an MI355X (largest deviation / bound):

    operator, |device - host twin| / bound (10 x the Boys change), M = 1 | 255 | 256 | 257 | 513:
    Lss    1.3e-15 / 3.2e-13 | 4.0e-15 / 2.6e-12 | 1.8e-15 / 5.2e-12 | 2.2e-15 / 4.5e-12 | 1.3e-15 / 1.2e-12
    Ldd    1.1e-15 / 6.4e-13 | 2.9e-15 / 1.3e-12 | 3.3e-15 / 2.3e-12 | 3.3e-15 / 2.0e-12 | 4.1e-15 / 1.9e-12  (worse form)
    L3     1.3e-15 / 3.2e-13 | 2.7e-15 / 3.7e-12 | 1.8e-15 / 1.4e-12 | 2.2e-15 / 4.2e-12 | 3.6e-15 / 2.9e-12  (both forms)
    G1     5.0e-16 / 5.8e-13 | 1.3e-15 / 1.1e-12 | 1.8e-15 / 2.8e-12 | 2.0e-15 / 2.1e-12 | 3.8e-15 / 2.7e-12  (both forms)
    M = 257, both forms where there is a d shell: Lps 1.8e-15 / 1.5e-12, Lpp 2.9e-15 / 1.8e-12, Lds 2.7e-15 / 1.9e-12,
    Ldp 3.9e-15 / 2.9e-12, G2 6.2e-15 / 2.0e-12, G3 2.7e-15 / 2.2e-12, G4 1.2e-14 / 2.1e-12, G5 2.4e-15 / 2.2e-12, L3 and
    G1 reordered as L3 and G1.  G2 between fragments: 0.0.  G4 - G1: 1.6e-14 / 1.3e-13 (host twin 1.3e-14).
    nuclei as charges against int1e_ao - T: Lss 6.9e-14 / 3.5e-11, Lps 4.2e-14 / 4.6e-12, Lpp 4.6e-14 / 5.2e-11,
    Lds 2.0e-14 / 2.2e-11, Ldp 1.4e-13 / 2.9e-11, Ldd 1.5e-14 / 1.4e-11, L3 6.4e-14 / 3.9e-11, G1 1.1e-14 / 1.2e-11,
    G2 3.6e-15 / 1.0e-11, G3 1.4e-14 / 1.2e-11, G4 1.2e-14 / 1.1e-11, G5 1.8e-14 / 9.3e-12.
    gradients, |device - FD| of gA | gQ (bound 1e-9 per component: 10 x the disagreement stays below it), net force:
    Lss           1.1e-11 | 8.0e-12   4.4e-16        G1sp          3.7e-11 | 1.5e-11   6.7e-16
    Lps           9.0e-12 | 4.4e-12   1.8e-15        G3sp          4.7e-11 | 1.8e-11   1.3e-15
    Lpp M = 1     4.7e-12 | 4.5e-12   1.0e-17        G5sp          1.9e-11 | 1.2e-11   4.4e-16
    Lpp M = 65    1.4e-11 | 4.5e-12   1.1e-16        HF*           2.2e-11 | 1.3e-11   4.4e-16
    Lpp M = 200   2.0e-11 | 5.2e-12   3.3e-16        formaldimine  4.8e-11 | 4.3e-11   1.3e-15
    LSP           1.8e-11 | 1.9e-11   1.8e-15
    42 atoms      1.6e-10 | 2.5e-10 (0.10, 0.12 of the bound)   1.7e-15
    43 atoms      2.8e-10 | 3.2e-10 (0.13, 0.14 of the bound)   1.6e-15
    106 atoms     6.9e-10 | 5.0e-10 (0.18, 0.13 of the bound)   1.2e-15
    classical term, atoms | charges, relative to the largest: at most 1e-15 (G3sp: 2.3e-9 of 3.4e6 | 4.7e-10 of 5.7e6)
    connection, nset = 10 against the host twin / bound | symmetric sets against gradient_batch(wq = D / 2), at most:
    Lss 5.6e-17 / 2.6e-13 | 3.5e-18   Lps 4.2e-16 / 1.3e-13 | 2.8e-17      Lpp 5.4e-16 / 6.5e-13 | 1.1e-16
    LSP 3.6e-15 / 1.8e-12 | 1.1e-16   G3sp 1.8e-15 / 8.6e-12 | 6.7e-16     G5sp 2.2e-15 / 8.7e-12 | 8.9e-16

With the stride of the operator's lanes doubled, the 32 operator tests with M >= 257 fail and tests/test_charges_gpu.py
passes; with ``deg = 1`` in the pp class of the gradient, the 8 gradient tests of the cases with a two-centre pp pair
fail and tests/test_charges_gpu.py passes (with ``deg = 1`` in every class both suites fail).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import auto_oo_amd as aoo                                   # noqa: E402
from auto_oo_amd import gaussian, gto                       # noqa: E402
from tests import _charges as C                             # noqa: E402
from tests import _charge_edges as X                        # noqa: E402
from tests import _couplings as Q                           # noqa: E402
from tests import _gto_edges as E                           # noqa: E402
from tests.test_couplings_gpu import NSETS                  # noqa: E402

F64 = torch.float64
BOHR = X.BOHR
NAN = float("nan")


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def to_dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=F64).to(dev())


def operator_into_nan(basis, ang, q, r):
    """``point_charge_integrals_into`` of the stack (ang [G, natm, 3], q [G, M], r [G, M, 3]; Angstrom) on an output that
    starts as NaN: every element written, finite, exactly symmetric -> [G, N, N] (device)"""
    ang, q, r = np.asarray(ang), np.asarray(q), np.asarray(r)
    out = torch.full((ang.shape[0], basis.nao, basis.nao), NAN, dtype=F64, device=dev())
    got = gto.point_charge_integrals_into(basis, to_dev(ang / BOHR), to_dev(q), to_dev(r / BOHR), out)
    assert got is out
    assert torch.isfinite(out).all()
    assert torch.equal(out, out.transpose(1, 2))
    return out


# ---- 1. the operator at the limits ------------------------------------------------------------------------------------
OPERATOR = [(n, f, M) for n in X.OPERATOR_CASES for f in X.forms_of(n) for M in X.sizes_of(n)]


def neighbours(name, ang, M, place):
    """two other geometries of the case with clouds of other seeds (they differ with the place in the stack)"""
    base = X.O_CASES[name][0] if name in X.O_CASES else name
    out = []
    for k in range(2):
        x = ang + 0.05 * (k + 1) * BOHR * np.array([0.3, -0.2, 0.5]) * np.arange(1, ang.shape[0] + 1)[:, None]
        out.append((x, X.cloud(x, M, base, seed=20240607 + 100 + k + 7 * place)))
    return out


@pytest.mark.parametrize("name,form,M", OPERATOR, ids=[f"{n}-{f}-{M}" for n, f, M in OPERATOR])
def test_operator_at_the_limits_against_the_host_twin(name, form, M):
    basis, ang, _, _ = X.operator_case(name, form)
    q, r = X.operator_cloud(name, M)
    ref, diff = X.operator_fixture(name, form, M)
    V = operator_into_nan(basis, ang[None], q[None], r[None])
    err = np.abs(V[0].cpu().numpy() - ref).max()
    print(f"{name} {form} M = {M}: max |V_ext| {np.abs(ref).max():.3g}, |device - host| {err:.2e} (bound {10 * diff:.2e})")
    assert err < 10 * diff
    assert torch.equal(gto.point_charge_integrals_batch(basis, ang, q, r), V)
    if M != 257:
        return
    # the same bits at places 0 and 2 of a stack of three
    for place in (0, 2):
        items = neighbours(name, ang, M, place)
        items.insert(place, (ang, (q, r)))
        S = operator_into_nan(basis, [i[0] for i in items], [i[1][0] for i in items], [i[1][1] for i in items])
        assert torch.equal(S[place], V[0]), (name, place)
        assert not torch.equal(S[1], V[0])


@pytest.mark.parametrize("form", X.forms_of("G2"))
def test_operator_between_dissociated_fragments_is_exactly_zero(form):
    basis, ang, _, _ = X.operator_case("G2", form)
    q, r = X.operator_cloud("G2", 257)
    ref, _ = X.operator_fixture("G2", form, 257)
    frag = E.fragment_of_ao(basis)
    apart = frag[:, None] != frag[None, :]
    assert not ref[apart].any()                                   # the host twin: exactly 0
    V = operator_into_nan(basis, ang[None], q[None], r[None])[0].cpu().numpy()
    worst = np.abs(V[apart]).max()
    print(f"G2 {form}: largest element between fragments {worst!r} (exactly 0.0), within {np.abs(V[~apart]).max():.3g}")
    assert worst == 0.0
    assert np.abs(V[~apart]).max() > 1.0


@pytest.mark.parametrize("form", X.forms_of("G4"))
def test_operator_after_a_translation_by_100_bohr(form):
    """G4 against G1, the cloud moved along: within 10 x what the host twin shows between the two"""
    basis, a1, _, _ = X.operator_case("G1", form)
    _, a4, _, _ = X.operator_case("G4", form)
    (q1, r1), (q4, r4) = X.operator_cloud("G1", 257), X.operator_cloud("G4", 257)
    assert np.array_equal(q1, q4) and np.abs((r4 - r1) / BOHR - E.G4_SHIFT).max() < 1e-12
    V = operator_into_nan(basis, [a1, a4], [q1, q4], [r1, r4])
    host = float(X._load("op", "G4")["g4_" + X.key_of(form, 257)])
    d = (V[0] - V[1]).abs().max().item()
    print(f"G4 - G1 {form}: {d:.2e} (host twin {host:.2e}, bound {10 * host:.2e})")
    assert d < 10 * host


@pytest.mark.parametrize("name", tuple(E.L_CASES) + E.G_NAMES)
def test_operator_with_the_nuclei_as_charges_is_the_nuclear_attraction_of_the_device(name):
    """two device paths (csrc/gto_charges.hip; csrc/gto.hip, gto_d.hip) against each other, the kinetic energy from
    the host"""
    basis, ang, f = E.basis_of(name), E.angstrom_of(name), E.fixture(name)
    R = E.xyz_of(name)
    V = operator_into_nan(basis, ang[None], basis.charges[None], ang[None])[0].cpu().numpy()
    S = torch.full((1, basis.nao, basis.nao), NAN, dtype=F64, device=dev())
    h = torch.full_like(S, NAN)
    gto.integrals_into(basis, to_dev(R[None]), S, h, None, None)
    T = gaussian.one_electron_integrals(gaussian.shells_from_table(basis.table, R), (), ())[1]
    U = gaussian.basis_transform(basis.table, E.form_of(name))
    err = np.abs(V - (h[0].cpu().numpy() - U @ T @ U.T)).max()
    bound = 10 * X.nuclei_fixture(name) + float(f["diff_h"])
    print(f"{name}: max |V| {np.abs(V).max():.3g}, V_ext(Z, R) against int1e_ao - T {err:.2e} (bound {bound:.2e})")
    assert err < bound


# ---- 2. the gradient beyond water -------------------------------------------------------------------------------------
GRADIENT = [(n, M) for n in X.GRADIENT_CASES for M in X.GRADIENT_SIZES.get(n, (X.M_GRAD,))]


def gradient_call(basis, ang, q, r, Dm, nuc=False):
    gA, gQ = gto.point_charge_gradient_batch(basis, ang[None], q, r, Dm[None], nuc=nuc)
    assert tuple(gA.shape) == (1, basis.natm, 3) and tuple(gQ.shape) == (1, q.size, 3)
    assert torch.isfinite(gA).all() and torch.isfinite(gQ).all()
    return gA[0], gQ[0]


def against_differences(tag, f, M, gA, gQ):
    """the device against the stored differences, per component max(1e-9, 10 x the reference's own disagreement); the
    components outside the sample of a many-atom case are NaN in the fixture and left out"""
    worst = {}
    for w, got in (("A", gA.cpu().numpy()), ("Q", gQ.cpu().numpy())):
        ref, dis = f[f"g{w}_{M}"], f[f"d{w}_{M}"]
        mask = ~np.isnan(ref)
        err = np.abs(got - ref)[mask]
        bound = np.maximum(1e-9, 10 * dis[mask])
        worst[w] = (np.abs(ref[mask]).max(), dis[mask].max(), err.max(), (err / bound).max())
        assert dis[mask].max() < X.FD_CAP
    print(f"{tag} ({str(f['rule'])}): " + "; ".join(
        f"g{w}: max {v[0]:.3g}, FD disagreement {v[1]:.2e}, device - FD {v[2]:.2e}, {v[3]:.3f} of the bound"
        for w, v in worst.items()))
    assert all(v[3] < 1.0 for v in worst.values()), (tag, worst)


def net_force(tag, gA, gQ, natm, M):
    net = (gA.sum(dim=0) + gQ.sum(dim=0)).abs().max().item()
    print(f"{tag}: net force {net:.2e} (bound {1e-10 * (natm + M):.1e})")
    assert net < 1e-10 * (natm + M)


@pytest.mark.parametrize("name,M", GRADIENT, ids=[f"{n}-{M}" for n, M in GRADIENT])
def test_gradients_against_differences_of_the_host_twin(name, M):
    basis, ang = X.gradient_case(name)
    f = X.gradient_fixture(name)
    q, r = X.gradient_cloud(name, M)
    Dm = to_dev(C.random_symmetric(basis.nao, X.D_SEED))
    gA, gQ = gradient_call(basis, ang, q, r, Dm)
    against_differences(f"{name} M = {M}", f, M, gA, gQ)
    net_force(f"{name} M = {M}", gA, gQ, basis.natm, M)
    if M > 3:
        assert not gQ[3].any()                                          # q = 0: exactly zero
    if M == X.M_GRAD:
        # a charge in the rest of the last chunk (192 .. 199) has the same bits when the cloud ends right after it
        # (the atoms' gradient of the cut cloud is another sum of chunks: covered by the bound above alone)
        for last in (195, 192):
            _, cut = gradient_call(basis, ang, q[:last + 1], r[:last + 1], Dm)
            assert torch.equal(cut[last], gQ[last]) and torch.equal(cut, gQ[:last + 1]), (name, last)
    else:
        _, full = gradient_call(basis, ang, *X.gradient_cloud(name, X.M_GRAD), Dm)
        assert torch.equal(full[:M], gQ)


@pytest.mark.parametrize("name", X.GRADIENT_CASES)
def test_classical_term_of_the_gradients(name):
    """``nuc=True`` minus ``nuc=False`` against the closed form (no charge ON a nucleus; in G3sp one is 1e-3 Bohr from
    a nucleus and the term reaches 1e6)"""
    basis, ang = X.gradient_case(name)
    q, r = X.gradient_cloud(name, X.M_GRAD, on_nucleus=False)
    Dm = to_dev(C.random_symmetric(basis.nao, X.D_SEED))
    a0, q0 = gradient_call(basis, ang, q, r, Dm)
    a1, q1 = gradient_call(basis, ang, q, r, Dm, nuc=True)
    R, rb = ang / BOHR, C.bohr(r)
    d = R[:, None, :] - rb[None, :, :]
    f = basis.charges[:, None, None] * q[None, :, None] * d / np.linalg.norm(d, axis=2)[..., None] ** 3
    ea = np.abs((a1 - a0).cpu().numpy() + f.sum(axis=1)).max()
    eq = np.abs((q1 - q0).cpu().numpy() - f.sum(axis=0)).max()
    ba, bq = 1e-12 * np.abs(f).sum(axis=1).max(), 1e-12 * np.abs(f.sum(axis=0)).max()
    print(f"{name} classical term: atoms {ea:.2e} of {np.abs(f.sum(axis=1)).max():.3g} (bound {ba:.2e}), charges "
          f"{eq:.2e} of {np.abs(f.sum(axis=0)).max():.3g} (bound {bq:.2e})")
    assert ea < ba and eq < bq
    net_force(f"{name} with the classical term", a1, q1, basis.natm, q.size)


@pytest.mark.parametrize("natm", X.MANY_ATOMS)
def test_gradients_of_many_atoms(natm):
    """the atoms' shares of a chunk in dynamic LDS: 42 atoms stay below 64 KB, 43 pass it, 106 reach the entry's limit"""
    basis, ang = X.many_atoms(natm)
    M = X.MANY_ATOMS_M
    q, r = X.gradient_cloud(natm, M)
    Dm = to_dev(C.random_symmetric(basis.nao, X.D_SEED))
    gA, gQ = gradient_call(basis, ang, q, r, Dm)
    against_differences(f"{natm} atoms", X.gradient_fixture(natm), M, gA, gQ)
    net_force(f"{natm} atoms", gA, gQ, natm, M)
    assert not gQ[3].any()
    if natm != 43:
        return
    # the same bits alone and at either place of a stack of two
    ang2 = ang + 0.03
    q2, r2 = X.cloud(ang2, M, seed=20240607 + 5)
    D2 = to_dev(C.random_symmetric(basis.nao, X.D_SEED + 1))
    for place in (0, 1):
        order = [(ang, q, r, Dm), (ang2, q2, r2, D2)][::1 if place == 0 else -1]
        A, Qg = gto.point_charge_gradient_batch(basis, np.stack([o[0] for o in order]), np.stack([o[1] for o in order]),
                                                np.stack([o[2] for o in order]), torch.stack([o[3] for o in order]),
                                                nuc=False)
        assert torch.equal(A[place], gA) and torch.equal(Qg[place], gQ), place
        assert not torch.equal(A[1 - place], gA)


def test_107_atoms_are_refused_before_any_launch():
    basis, ang = X.many_atoms(107)
    M = 4
    q, r = X.cloud(ang, M)
    x, qd, rd = to_dev(ang / BOHR)[None], to_dev(q)[None], to_dev(C.bohr(r))[None]
    Dm = to_dev(C.random_symmetric(basis.nao, 1))[None]
    lib = aoo._lib.load()
    assert lib.oovqe_gto_point_charge_gradient_work_size(basis.nshell, 1, 107, 1, M) < 0
    assert b"natm" in lib.oovqe_last_error()
    assert lib.oovqe_gto_point_charge_gradient_work_size(106, 1, 106, 1, M) > 0
    with pytest.raises(aoo._lib.OovqeError, match="natm = 107"):
        gto.point_charge_gradient_into(basis, x, qd, rd, Dm)
    with pytest.raises(aoo._lib.OovqeError, match="natm = 107"):
        gto.point_charge_gradient_batch(basis, ang[None], q, r, Dm)
    # the C entry itself: a negative code, the message, outputs untouched
    t = basis.device_tables(dev())
    p = aoo._lib.dptr
    gA = torch.full((1, 107, 3), 7.0, dtype=F64, device=dev())
    gQ = torch.full((1, M, 3), 7.0, dtype=F64, device=dev())
    work = torch.full((basis.work(dev(), 1).numel() + 107 * 3 + 64,), 7.0, dtype=F64, device=dev())
    rc = lib.oovqe_gto_point_charge_gradient_batch(basis.nshell, p(t.shells, torch.int32), int(basis.exps.size),
                                                   p(t.exps), p(t.coefs), basis.natm, p(t.charges), 1, p(x), basis.nao, M,
                                                   p(qd), p(rd), p(Dm), 0, p(gA), p(gQ), p(work), aoo._lib.stream_ptr())
    msg = lib.oovqe_last_error()
    torch.cuda.synchronize()
    print(f"107 atoms: return code {rc}, message {msg!r}")
    assert rc < 0 and b"natm = 107" in msg
    assert bool((gA == 7.0).all()) and bool((gQ == 7.0).all()) and bool((work == 7.0).all())
    # the operator has no such limit
    V = gto.point_charge_integrals_batch(basis, ang, q, r)
    assert torch.isfinite(V).all()


# ---- 3. the connection at the limits ----------------------------------------------------------------------------------
def connection_call(basis, xyz_bohr, mats):
    """``gto.overlap_connection_into`` for the host matrices ``mats`` [K, N, N], the same in every geometry"""
    x = to_dev(xyz_bohr)
    D = to_dev(mats)[None].expand((x.shape[0],) + tuple(mats.shape)).contiguous()
    return gto.overlap_connection_into(basis, x, D)


@pytest.mark.parametrize("name", X.CONNECTION_CASES)
def test_connection_at_the_limits_against_the_host_twin(name):
    basis, ang = X.gradient_case(name)
    R = ang / BOHR
    T = X.connection_reference(name)
    ten = Q.general_matrices(basis.nao, 10)
    scale = X.connection_scale(ten, T)
    bound = 1e-12 * scale
    full = None
    for K in NSETS:
        got = connection_call(basis, R[None], ten[:K])
        assert tuple(got.shape) == (1, K, basis.natm, 3) and torch.isfinite(got).all()
        want = np.einsum("kmn,admn->kad", ten[:K], T)
        err = np.abs(got[0].cpu().numpy() - want).max()
        print(f"{name} nset = {K}: values up to {np.abs(want).max():.3g}, sum of |mats| |T| up to {scale:.3g}, against the "
              f"host twin {err:.2e} (bound {bound:.2e})")
        assert err < bound, (name, K, err)
        full = got
    # the same bits for a set alone and among ten, for the case alone and inside a stack of two
    for k in (0, 4, 7):
        assert torch.equal(connection_call(basis, R[None], ten[k:k + 1])[:, 0], full[:, k]), (name, k)
    assert torch.equal(connection_call(basis, R[None], ten[:6]), full[:, :6])
    other = E.displaced(name[:2]) if name.endswith("sp") else E.displaced(name)
    two = connection_call(basis, np.stack([other, R]), ten)
    assert torch.equal(two[1], full[0]) and not torch.equal(two[0], full[0])
    assert torch.equal(connection_call(basis, np.stack([R, other]), ten)[0], full[0])
    # symmetric matrices: half the overlap gradient
    sym = ten[:6] + ten[:6].transpose(0, 2, 1)
    bound = 1e-12 * X.connection_scale(sym, T)
    got = connection_call(basis, R[None], sym)[0]
    for k in range(6):
        want = gto.gradient_batch(basis, ang[None], wq=to_dev(0.5 * sym[k:k + 1]), nuc=False)[0]
        err = (got[k] - want).abs().max().item()
        print(f"{name} symmetric set {k}: values up to {want.abs().max().item():.3g}, against gradient_batch(wq = D / 2) "
              f"{err:.2e} (bound {bound:.2e})")
        assert err < bound, (name, k, err)
