"""The cases and references of the edge tests of the point-charge and connection kernels (tests/_charge_edges.py)
checked on the host: the clouds, the fixtures against the host twin they were recorded from, the cap of the gradient
references, the orientations the gradient cases cover and the scale of the connection bound.  No GPU.  Every test
prints its figures before it asserts."""
import os

import numpy as np
import pytest

from auto_oo_amd import gaussian
from tests import _charges as C
from tests import _charge_edges as X
from tests import _couplings as Q
from tests import _gto_edges as E


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


# ---- clouds -----------------------------------------------------------------------------------------------------------
def test_the_larger_clouds_keep_the_130_charges_as_a_prefix():
    xyz = E.angstrom_of("G1")
    q0, r0 = C.cloud(xyz)
    for on in (True, False):
        qa, ra = C.cloud(xyz, on_nucleus=on)
        for M in (131, 257, 513):
            q, r = X.cloud(xyz, M, "G1", on_nucleus=on)
            assert q.shape == (M,) and r.shape == (M, 3)
            assert np.array_equal(q[:130], qa) and np.array_equal(r[:130], ra)
    q5, r5 = X.cloud(xyz, 513)
    q2, r2 = X.cloud(xyz, 257)
    assert np.array_equal(q5[:257], q2) and np.array_equal(r5[:257], r2)
    assert np.array_equal(X.cloud(xyz, 64)[1], r0[:64])
    d = np.linalg.norm(r5[130:] / X.BOHR - xyz[0] / X.BOHR, axis=1)
    assert 3.0 <= d.min() and d.max() <= 12.0 and np.abs(q5).max() <= 1.0 and q5[130:].min() < 0 < q5[130:].max()
    assert np.array_equal(r0[1], xyz[1])                              # ON atom 1, bit for bit


def test_the_clouds_of_g2_and_g3_do_what_they_are_there_for():
    """G2: every fragment has charges within 12 Bohr and beyond 40; G3: one charge 1e-3 Bohr from nucleus 0"""
    R = E.xyz_of("G2")
    _, r = X.operator_cloud("G2", 257)
    d = np.linalg.norm(r[:, None, :] / X.BOHR - R[None], axis=2)            # [M, natm]
    near, far = (d < 12.0).sum(axis=0), (d > 40.0).sum(axis=0)
    print("G2: charges within 12 Bohr of each atom", near, "beyond 40 Bohr", far)
    assert near.min() >= 40 and far.min() >= 80
    R = E.xyz_of("G3")
    q, r = X.operator_cloud("G3", 257)
    d = np.linalg.norm(r / X.BOHR - R[0], axis=1)
    # (charge 1 is ON atom 1, itself 1e-3 Bohr from atom 0)
    assert abs(d[130] - 1e-3) < 1e-12 and q[130] != 0.0 and np.nonzero(d < 0.1)[0].tolist() == [1, 130]
    q, r = X.gradient_cloud("G3sp", X.M_GRAD, on_nucleus=False)
    assert abs(np.linalg.norm(r[130] / X.BOHR - R[0]) - 1e-3) < 1e-12
    assert np.linalg.norm(r[:, None, :] / X.BOHR - R[None], axis=2).min() > 5e-4      # no charge on a nucleus


# ---- operator fixtures ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Lss", "Lps", "G3"])
def test_operator_fixtures_against_the_host_twin(name):
    """re-made: the reference and the Boys-perturbation change of every (form, M) stored, 1e-13 relative; the
    spherical form here comes from the twin itself, not from ``_charge_edges.in_form``"""
    basis = E.basis_of(name)
    R = E.xyz_of(name)
    for form in X.forms_of(name):
        b = X.operator_case(name, form)[0]
        for M in X.sizes_of(name):
            q, r = X.operator_cloud(name, M)
            V = X.host_operator(b.table, R, q, C.bohr(r), form)
            V2 = X.host_operator(b.table, R, q, C.bohr(r), form, E.perturbed_boys(1))
            ref, diff = X.operator_fixture(name, form, M)
            d = (rel(V, ref), abs(np.abs(V2 - V).max() - diff) / diff)
            print(f"{name} {form} M = {M}: max |V_ext| {np.abs(V).max():.3g}, fixture against the twin {d[0]:.1e}, its "
                  f"diff {diff:.2e} against the re-made one {d[1]:.1e} (bound 1e-13; the bound of the device test is "
                  f"{10 * diff:.2e})")
            assert V.shape == (b.nao, b.nao) and d[0] < 1e-13
            # (the perturbation draws its signs per call: the same sequence of calls gives the same figure)
            assert d[1] < 1e-13
    Vn = X.host_operator(basis.table, R, basis.charges, R, E.form_of(name))
    Vn2 = X.host_operator(basis.table, R, basis.charges, R, E.form_of(name), E.perturbed_boys(1))
    assert abs(np.abs(Vn2 - Vn).max() - X.nuclei_fixture(name)) < 1e-13 * X.nuclei_fixture(name)
    # the nuclei as the charges: the nuclear attraction of the gto_edges fixture
    T = gaussian.one_electron_integrals(gaussian.shells_from_table(basis.table, R), (), ())[1]
    U = gaussian.basis_transform(basis.table, E.form_of(name))
    d = np.abs(Vn - (E.fixture(name)["h"] - U @ T @ U.T)).max()
    print(f"{name}: V_ext of the nuclei against h - T of the gto_edges fixture {d:.2e}")
    assert d < 1e-12


def test_every_operator_fixture_is_complete_and_small():
    for name in X.OPERATOR_CASES:
        for form in X.forms_of(name):
            b = X.operator_case(name, form)[0]
            for M in X.sizes_of(name):
                V, diff = X.operator_fixture(name, form, M)
                assert V.shape == (b.nao, b.nao) and np.array_equal(V, V.T) and np.isfinite(V).all()
                # a dropped pass of charges changes elements by 1e-2 or more: the bounds are ten orders below
                assert 0.0 < 10 * diff < 1e-11, (name, form, M, diff)
    for name in tuple(E.L_CASES) + E.G_NAMES:
        assert os.path.getsize(X.fixture_path("op", name)) < 64 * 1024
        assert 0.0 < X.nuclei_fixture(name) < 1e-11


def test_reordered_cases_hold_the_same_functions():
    for name, (base, perm) in X.O_CASES.items():
        for form in X.forms_of(name):
            basis, ang, ao, b = X.operator_case(name, form)
            new, ang2, ao2 = E.reordered(base, perm)
            assert b == base and basis.shells[0, 1] & 255 == 2 and sorted(ao.tolist()) == list(range(basis.nao))
            assert np.array_equal(ang, ang2)
            if form == E.form_of(base):
                assert np.array_equal(ao, ao2) and np.array_equal(basis.shells, new.shells)
    # one element by hand: a function pair of O-G1 through the twin on the reordered table
    basis, ang, ao, _ = X.operator_case("O-G1", "spherical")
    q, r = X.operator_cloud("O-G1", 257)
    V = X.host_operator(basis.table, ang / X.BOHR, q, C.bohr(r), "spherical")
    ref, diff = X.operator_fixture("O-G1", "spherical", 257)
    d = np.abs(V - ref).max()
    print(f"O-G1: the twin on the reordered table against the permuted fixture {d:.2e} (bound {10 * diff:.2e})")
    assert d < 10 * diff


def test_dissociated_fragments_are_exact_zeros_on_the_host_and_the_translation_is_rounding():
    basis = E.basis_of("G2")
    frag = E.fragment_of_ao(basis)
    apart = frag[:, None] != frag[None, :]
    for form in X.forms_of("G2"):
        b = X.operator_case("G2", form)[0]
        fr = E.fragment_of_ao(b)
        V, _ = X.operator_fixture("G2", form, 257)
        assert not V[fr[:, None] != fr[None, :]].any() and np.abs(V[fr[:, None] == fr[None, :]]).max() > 1.0
    assert apart.sum() > 0
    f = X._load("op", "G4")
    for form in X.forms_of("G4"):
        g4 = float(f["g4_" + X.key_of(form, 257)])
        d = np.abs(X.operator_fixture("G4", form, 257)[0] - X.operator_fixture("G1", form, 257)[0]).max()
        print(f"G4 - G1 on the host ({form}): {g4:.2e}")
        assert d == g4 and 0.0 < g4 < 1e-12


# ---- gradient fixtures ------------------------------------------------------------------------------------------------
def test_every_gradient_reference_is_below_the_cap():
    for name in X.GRADIENT_CASES + X.MANY_ATOMS:
        f = X.gradient_fixture(name)
        many = not isinstance(name, str)
        basis = (X.many_atoms(name) if many else X.gradient_case(name))[0]
        sizes = (X.MANY_ATOMS_M,) if many else X.GRADIENT_SIZES.get(name, (X.M_GRAD,))
        worst = 0.0
        for M in sizes:
            assert f[f"gA_{M}"].shape == (basis.natm, 3) and f[f"gQ_{M}"].shape == (M, 3)
            for w in "AQ":
                d, g = f[f"d{w}_{M}"], f[f"g{w}_{M}"]
                assert np.array_equal(np.isnan(d), np.isnan(g)) and np.isnan(g).any() == many
                worst = max(worst, np.nanmax(d))
        if many:
            assert np.isfinite(f[f"gA_{M}"][[0, name // 2, name - 1]]).all() and np.isfinite(f[f"gA_{M}"]).sum() == 9
            assert np.isfinite(f[f"gQ_{M}"][list(X.SAMPLE_CHARGES)]).all() and np.isfinite(f[f"gQ_{M}"]).sum() == 12
        print(f"{name}: rule {str(f['rule'])}, near charge {float(f['near'])} Bohr, largest disagreement {worst:.2e} "
              f"(cap {X.FD_CAP:.0e})")
        assert worst < X.FD_CAP
        assert str(f["rule"]) in X.RULES and float(f["near"]) == X.NEAR_OF.get(name, C.NEAR)
        assert os.path.getsize(X.fixture_path("grad", name)) < 64 * 1024


def test_one_gradient_fixture_against_the_host_twin():
    """HF* re-made with its stored rule"""
    name = "HF*"
    f = X.gradient_fixture(name)
    basis, ang = X.gradient_case(name)
    order, h, other = X.RULES[str(f["rule"])]
    q, r = X.gradient_cloud(name, X.M_GRAD)
    Dm = C.random_symmetric(basis.nao, X.D_SEED)
    fa, fq = X.fd_gradients(basis, ang / X.BOHR, q, C.bohr(r), Dm, order, h)
    d = (rel(fa.sum(axis=0), f[f"gA_{X.M_GRAD}"]), rel(fq, f[f"gQ_{X.M_GRAD}"]))
    print(f"{name}: re-made gA {d[0]:.1e}, gQ {d[1]:.1e} of the largest component (bound 1e-13)")
    assert max(d) < 1e-13
    assert not f[f"gQ_{X.M_GRAD}"][3].any()                              # q = 0


def test_the_gradient_cases_cover_every_orientation():
    seen = {name: X.orientations(X.gradient_case(name)[0]) for name in X.GRADIENT_CASES}
    for name, kinds in seen.items():
        print(f"{name}: {sorted(kinds) or '-'}")
    assert set().union(*seen.values()) == set(X.KINDS)
    # what the module docstring says of the single cases, and what water -- the one molecule of
    # tests/test_charges_gpu.py -- lacks
    assert seen["Lss"] == set() and seen["Lps"] == {X.KINDS[0], X.KINDS[3]} and seen["Lpp"] == {X.KINDS[2], X.KINDS[3]}
    assert seen["LSP"] == {X.KINDS[1], X.KINDS[2], X.KINDS[3]} and seen["HF*"] == {X.KINDS[1], X.KINDS[3]}
    for name in ("G1sp", "G3sp", "G5sp", "formaldimine"):
        assert seen[name] == set(X.KINDS)
    assert X.orientations(C.water_basis()) == {X.KINDS[0], X.KINDS[3]}
    assert X.gradient_case("formaldimine")[0].natm == 5
    assert max(b.max_nprim for b in (X.gradient_case(n)[0] for n in ("Lss", "LSP"))) == 10


def test_many_atom_cases():
    for natm in X.MANY_ATOMS:
        basis, ang = X.many_atoms(natm)
        R = ang / X.BOHR
        d = np.linalg.norm(R[:, None] - R[None], axis=2) + 10.0 * np.eye(natm)
        lds = natm * 3 * 64 * 8
        print(f"{natm} atoms: closest pair {d.min():.3f} Bohr, LDS of the gradient kernel {lds} bytes")
        assert basis.natm == basis.nshell == basis.nao == natm and basis.max_nprim == 1 and d.min() >= 1.2
    assert 42 * 1536 <= 64 * 1024 < 43 * 1536 and 106 * 1536 <= 160 * 1024 < 107 * 1536


# ---- connection -------------------------------------------------------------------------------------------------------
def test_connection_scale():
    """the scale of the connection bound is what the module docstring of tests/_charge_edges.py says (three digits)"""
    for name in X.CONNECTION_CASES:
        basis, _ = X.gradient_case(name)
        T = X.connection_reference(name)
        mats = Q.general_matrices(basis.nao, 10)
        scale = X.connection_scale(mats, T)
        want = np.einsum("kmn,admn->kad", mats, T)
        by_hand = max(np.sum(np.abs(mats[k]) * np.abs(T[a, d])) for k in range(10) for a in range(basis.natm)
                      for d in range(3))
        print(f"{name}: scale {scale:.4g} (recorded {X.CONNECTION_SCALE[name]}), largest |T| {np.abs(T).max():.3g}, values "
              f"up to {np.abs(want).max():.3g}, bound {1e-12 * scale:.2e}")
        assert abs(scale - X.CONNECTION_SCALE[name]) < 5e-3 * scale
        assert abs(scale - by_hand) < 1e-12 * scale and np.abs(want).max() <= scale
        # T^A + T^A^T = dS / dR_A sums to zero over the atoms; T is non-zero only for nu on atom A
        assert np.abs((T + T.transpose(0, 1, 3, 2)).sum(axis=0)).max() < 1e-12
