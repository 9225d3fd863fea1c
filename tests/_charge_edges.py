"""Cases, clouds and references of the edge tests of the point-charge and connection kernels (csrc/gto_charges.hip,
csrc/gto_connection.hip; tests/test_charge_edges_cpu.py, tests/test_charge_edges_gpu.py).  The fixtures
tests/golden/charge_edges_*.npz are written by tests/golden/make_charge_edges.py.  The shell tables and geometries are
those of tests/_gto_edges.py (L-, G- and O-cases, LSP), the clouds extend ``_charges.cloud``.

Clouds (``cloud``): the first 130 charges are ``_charges.cloud`` bit for bit (0.2 Bohr from atom 0, ON atom 1, 50 Bohr
away, q = 0, then a shell of 3 .. 12 Bohr around atom 0).  Charges 130 .. 512 are drawn once from a second seed in the
same shell, so that every size is a prefix of the largest.  G2 (fragments 60 and 300 Bohr apart): appended charge k
stands around atom k % 3, so every fragment sees Boys arguments from below 1 to above 1e4.  G3: appended charge 130 is
1e-3 Bohr from nucleus 0.

Operator references (``operator_fixture``): ``gaussian.point_charge_integrals_from_table`` per (case, d form, M), next
to the largest change a Boys function perturbed by ``_gto_d.BOYS_RTOL`` makes to it (``diff``; the bound is 10 x that).
The spherical form is made from the Cartesian one the way the twin makes it (U V U^T, then the mean with the transpose),
which tests/test_charge_edges_cpu.py checks against the twin itself.

Gradient cases (s and p shells) and the orientation of the pairs they hold, from ``gto_pair_ref`` of csrc/gto.h (a
pair of shells i >= j of the table is stored (higher l, lower l), at equal l (i, j); ``swapped`` = first < second):

    case      two-centre ps swapped   two-centre ps unswapped   two-centre pp   pp of a shell with itself
    Lss       -                       -                         -               -         (two s10 shells)
    Lps       p8 | s1                 -                         -               p8
    Lpp       -                       -                         p8 | p1         p1, p8
    LSP       -                       C p9 | H s10              C p9 | H p8     p8, p9    (one-centre ps unswapped too)
    G1sp ..   N p | later N s, O s    later N p | first N s     N p | N p       both
    HF*       -                       F 2p | H 1s               -               F 2p
    formald.  N 2p | C s, H s;        C 2p | N s                C 2p | N 2p     both
              C 2p | H s

``orientations`` derives this table on the host and tests/test_charge_edges_cpu.py asserts that the set covers all four.

Gradient references (``gradient_fixture``): central differences of ``sum D . V_ext(per_charge=True)`` of the host twin
in every atom coordinate and, per charge, in its own coordinates, with D = ``_charges.random_symmetric(nao, D_SEED)``
and ``nuc=False``.  Three candidate rules were evaluated per case on the CPU -- the 2nd-order difference at h = 1e-5
against h / 2 (tests/test_charges_gpu.py), and the 4th-order stencil of tests/test_nucgrad_gpu.py at h against 2h with
h = 1e-3 and with h = 1e-4 -- and the one with the smallest disagreement with itself is stored (the reference is the
finer step of the pair).  A case counts only below 1e-8.  Measured (make_charge_edges.py prints them), largest
|FD - FD'| over atoms and charges, Ha/Bohr:

    case           2nd order, 1e-5 / 5e-6   4th order, 1e-3 / 2e-3   4th order, 1e-4 / 2e-4   stored
    Lss            2.0e-9                   3.2e-8                   1.4e-11                  fd4 1e-4
    Lps            1.2e-8                   2.7e-7                   4.0e-11                  fd4 1e-4
    Lpp (1, 65, 200 charges)  8.0e-10       4.4e-8                   2.2e-11                  fd4 1e-4
    LSP            7.0e-9                   1.8e-7                   3.3e-11                  fd4 1e-4
    G1sp           5.7e-10                  1.0e-10                  3.2e-11                  fd4 1e-4
    G3sp           7.1e-10                  2.7e-10                  3.6e-11                  fd4 1e-4
    G5sp           3.4e-10                  1.2e-10                  4.3e-11                  fd4 1e-4
    HF*            1.6e-9                   3.4e-8                   2.6e-11                  fd4 1e-4
    formaldimine   5.2e-9                   3.4e-8                   5.6e-11                  fd4 1e-4
    42 atoms       2.4e-10                  -                        -                        fd2 1e-5
    43 atoms       3.1e-10                  -                        -                        fd2 1e-5
    106 atoms      9.9e-10                  -                        -                        fd2 1e-5

(h = 1e-3 is too long for the 5.3e3 exponents of the L-cases and for the charge 0.2 Bohr from atom 0; no case needed its
near charge moved: ``NEAR_OF`` is empty.)

The many-atom cases (``many_atoms``: natm single-primitive s shells on H atoms, no two closer than 1.2 Bohr, M = 70)
hold a sample only: all coordinates of the first, a middle and the last atom and of charges 0, 63, 64, 69, with the
2nd-order rule alone (an evaluation of the 106-atom table takes the host twin seconds).

Connection: the bound of tests/test_couplings_gpu.py is 1e-12 on values of order 1 (fp64, the same formulas as the
host twin).  Here the bound follows the size of what is summed: 1e-12 times ``connection_scale``, the largest over
(set, atom, direction) of sum_{mu nu} |mats[k, mu, nu]| |T[A, d, mu, nu]| -- the sum the kernel forms, taken in absolute
value.  For the ten sets of ``_couplings.general_matrices`` it is CONNECTION_SCALE below (checked on the host by
tests/test_charge_edges_cpu.py): 0.13 to 8.7, the elements of ``T`` staying below 0.74 -- the normalised contracted
functions keep them of order 1 whatever the exponents, so the bounds come out between 1.3e-13 and 8.7e-12.
"""
import functools
import os

import numpy as np

from auto_oo_amd import gaussian, gto
from auto_oo_amd.moldata import get_formal_geo
from tests import _charges as C
from tests import _gto_edges as E

BOHR = gaussian.BOHR
GOLDEN = E.GOLDEN
M_BIG = 513
M_EDGES = (1, 255, 256, 257, 513)          # one pass of 256 lanes, its edges, a third pass with one live lane
M_ONE = (257,)
MANY_M = ("Lss", "Ldd", "L3", "G1")
EXTRA_SEED = 20240608
D_SEED = 11
M_GRAD = 200                               # three chunks of 64 and a rest of 8
FD_CAP = 1e-8
O_CASES = {"O-L3": ("L3", (2, 0, 1)), "O-G1": ("G1", (2, 1, 0))}
OPERATOR_CASES = tuple(E.L_CASES) + E.G_NAMES + tuple(O_CASES)
GRADIENT_CASES = ("Lss", "Lps", "Lpp", "LSP", "G1sp", "G3sp", "G5sp", "HF*", "formaldimine")
GRADIENT_SIZES = {"Lpp": (1, 65, M_GRAD)}
CONNECTION_CASES = ("Lss", "Lps", "Lpp", "LSP", "G3sp", "G5sp")
MANY_ATOMS = (42, 43, 106)                 # LDS of the gradient kernel: below 64 KB, just above it, the entry's limit
MANY_ATOMS_M = 70
SAMPLE_CHARGES = (0, 63, 64, 69)
# python -m pytest tests/test_charge_edges_cpu.py -s -k connection_scale
CONNECTION_SCALE = {"Lss": 0.258, "Lps": 0.13, "Lpp": 0.651, "LSP": 1.81, "G3sp": 8.57, "G5sp": 8.74}
# name: (order, the step of the reference, the step it is compared with)
RULES = {"fd2 1e-5": (2, 5e-6, 1e-5), "fd4 1e-3": (4, 1e-3, 2e-3), "fd4 1e-4": (4, 1e-4, 2e-4)}
NEAR_OF = {}                               # case: distance of charge 0 from atom 0 where 0.2 Bohr missed FD_CAP


# ---- cases ------------------------------------------------------------------------------------------------------------
def forms_of(name):
    """the d forms an operator case is run in"""
    base = O_CASES[name][0] if name in O_CASES else name
    return ("spherical", "cartesian") if E.case(base)[2] else (None,)


@functools.lru_cache(maxsize=None)
def operator_case(name, form=None):
    """-> (basis, geometry [natm, 3] Angstrom, ao, base): the L-, G- or O-case ``name`` with its d shells in ``form``.
    ``ao``: function i of this basis is function ao[i] of the case ``base`` in its table's order (None: the same)."""
    if name in O_CASES:
        base, perm = O_CASES[name]
        sym, table, _, _ = E.case(base)
        rev = {k: list(reversed(v)) for k, v in table.items()}
        basis = gto.GTOBasis([sym[a] for a in perm], rev, d_functions=form)
        orig = operator_case(base, form)[0]
        width = [6 if f == (2 | gto.CARTESIAN) else 2 * (f & 255) + 1 for f in orig.shells[:, 1]]
        start = np.concatenate(([0], np.cumsum(width)))
        ao = []
        for a in perm:
            for k in reversed([k for k in range(orig.nshell) if orig.shells[k, 0] == a]):
                ao += list(range(start[k], start[k + 1]))
        return basis, E.angstrom_of(base)[list(perm)], np.array(ao), base
    sym, table, _, _ = E.case(name)
    return gto.GTOBasis(sym, table, d_functions=form), E.angstrom_of(name), None, name


def sp_table():
    return {k: [s for s in v if s[0] != "d"] for k, v in E.G_TABLE.items()}


@functools.lru_cache(maxsize=None)
def gradient_case(name):
    """-> (basis, geometry [natm, 3] Angstrom) of a gradient or connection case (s and p shells)"""
    if name.endswith("sp"):
        return gto.GTOBasis(E.G_SYMBOLS, sp_table()), E.angstrom_of(name[:2])
    if name == "HF*":
        return C.hf_basis(), C.HF_XYZ
    if name == "formaldimine":
        basis = gto.GTOBasis(["N", "C", "H", "H", "H"])
        return basis, basis.coordinates([get_formal_geo(140.0, 80.0)])[0]
    return E.basis_of(name), E.angstrom_of(name)


@functools.lru_cache(maxsize=None)
def many_atoms(natm):
    """``natm`` H atoms with one single-primitive s shell each (exponent 0.8) at seeded positions no two closer than
    1.2 Bohr -> (basis, geometry [natm, 3] Angstrom)"""
    rng = np.random.default_rng(1000 + natm)
    pts = []
    while len(pts) < natm:
        x = rng.uniform(-3.0, 3.0, 3) * (natm / 16) ** (1.0 / 3.0)
        if all(np.linalg.norm(x - y) >= 1.2 for y in pts):
            pts.append(x)
    return gto.GTOBasis(["H"] * natm, {"H": [("s", [0.8], [1.0])]}), np.array(pts) * BOHR


# ---- clouds -----------------------------------------------------------------------------------------------------------
def cloud(xyz_angstrom, M, name=None, on_nucleus=True, seed=20240607, near=C.NEAR):
    """-> (q [M], positions [M, 3] Angstrom): ``_charges.cloud`` for M <= 130, its 130 charges followed by seeded ones
    beyond (module docstring); ``name`` "G2" or "G3" (with or without "sp") places the appended charges as those cases
    ask."""
    q, ang = C.cloud(xyz_angstrom, min(M, C.M_MAX), on_nucleus, seed, near)
    if M <= C.M_MAX:
        return q, ang
    n = M_BIG - C.M_MAX
    assert M <= M_BIG
    rng = np.random.default_rng(EXTRA_SEED + (seed - 20240607))
    R = np.asarray(xyz_angstrom, dtype=float) / BOHR
    qe = rng.uniform(-1.0, 1.0, n)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    centre = np.repeat(R[:1], n, axis=0)
    if name and name.startswith("G2"):
        centre = R[np.arange(n) % 3]
    r = centre + u * rng.uniform(3.0, 12.0, n)[:, None]
    if name and name.startswith("G3"):
        qe[0], r[0] = 0.6, R[0] + 1e-3 * np.array([0.6, 0.0, 0.8])
    return np.concatenate((q, qe[:M - C.M_MAX])), np.concatenate((ang, (r * BOHR)[:M - C.M_MAX]))


def operator_cloud(name, M, seed=20240607):
    """the cloud of an operator case: that of its base case (an O-case holds the same points in another order)"""
    base = O_CASES[name][0] if name in O_CASES else name
    return cloud(E.angstrom_of(base), M, base, seed=seed)


def gradient_cloud(name, M, on_nucleus=True):
    xyz = gradient_case(name)[1] if isinstance(name, str) else many_atoms(name)[1]
    return cloud(xyz, M, name if isinstance(name, str) else None, on_nucleus, near=NEAR_OF.get(name, C.NEAR))


def sizes_of(name):
    base = O_CASES[name][0] if name in O_CASES else name
    return M_EDGES if (base in MANY_M and name not in O_CASES) else M_ONE


# ---- host references --------------------------------------------------------------------------------------------------
def host_operator(table, xyz_bohr, q, r_bohr, form, boys=None):
    """``gaussian.point_charge_integrals_from_table``, with ``boys`` in the place of ``gaussian._boys`` for the
    duration of the call (as ``cartesian_integrals_from_table(boys=)`` does it)"""
    keep = gaussian._boys
    if boys is not None:
        gaussian._boys = boys
    try:
        return gaussian.point_charge_integrals_from_table(table, xyz_bohr, q, r_bohr, form or "spherical")
    finally:
        gaussian._boys = keep


def in_form(table, V_cart, form):
    """what ``point_charge_integrals_from_table`` makes of its Cartesian matrix"""
    U = gaussian.basis_transform(table, form or "spherical")
    V = U @ V_cart @ U.T
    return 0.5 * (V + V.T)


def make_operator(name, M, forms):
    """-> {form: (V, diff)} of the base case ``name`` with the first M charges of its cloud"""
    sym, table, _, _ = E.case(name)
    basis = operator_case(name, forms[0])[0]
    q, r = cloud(E.angstrom_of(name), M, name)
    R, rb = E.xyz_of(name), C.bohr(r)
    if forms == (None,):
        V = host_operator(basis.table, R, q, rb, None)
        V2 = host_operator(basis.table, R, q, rb, None, E.perturbed_boys(1))
        return {None: (V, np.abs(V2 - V).max())}
    Vc = host_operator(basis.table, R, q, rb, "cartesian")
    Vc2 = host_operator(basis.table, R, q, rb, "cartesian", E.perturbed_boys(1))
    out = {}
    for f in forms:
        V, V2 = in_form(basis.table, Vc, f), in_form(basis.table, Vc2, f)
        out[f] = (V, np.abs(V2 - V).max())
    return out


def per_charge_values(basis, Dm, q, R, rb):
    return np.einsum("kmn,mn->k", gaussian.point_charge_integrals_from_table(basis.table, R, q, rb, per_charge=True), Dm)


def fd_gradients(basis, xyz_bohr, q, r_bohr, Dm, order, h, atoms=None, charges=None):
    """central differences (2nd order, or the 4th-order stencil +-h, +-2h) of sum D . V_ext of the host twin
    -> (per-charge derivative in the atoms' coordinates [M, natm, 3], in each charge's own coordinates [M, 3]); only
    the atoms ``atoms`` and the charges ``charges`` are filled when given (the rest is NaN)"""
    steps = ((1.0, 1.0 / (2 * h)), (-1.0, -1.0 / (2 * h))) if order == 2 else (
        (1.0, 8.0 / (12 * h)), (-1.0, -8.0 / (12 * h)), (2.0, -1.0 / (12 * h)), (-2.0, 1.0 / (12 * h)))
    M, natm = q.size, xyz_bohr.shape[0]
    fa, fq = np.full((M, natm, 3), np.nan), np.full((M, 3), np.nan)
    ks = np.arange(M) if charges is None else np.asarray(charges)
    for d in range(3):
        acc = np.zeros(len(ks))
        for s, w in steps:
            rr = r_bohr[ks].copy()
            rr[:, d] += s * h
            acc += w * per_charge_values(basis, Dm, q[ks], xyz_bohr, rr)       # (each charge feels only itself)
        fq[ks, d] = acc
        for at in (range(natm) if atoms is None else atoms):
            acc = np.zeros(M)
            for s, w in steps:
                Rp = xyz_bohr.copy()
                Rp[at, d] += s * h
                acc += w * per_charge_values(basis, Dm, q, Rp, r_bohr)
            fa[:, at, d] = acc
    return fa, fq


def classical_gradients(charges, xyz_bohr, q, r_bohr):
    """d/dR_A and d/dr_k of sum Z_A q_k / |R_A - r_k| -> ([natm, 3], [M, 3], the largest sum of |terms| of each)"""
    d = xyz_bohr[:, None, :] - r_bohr[None, :, :]
    f = charges[:, None, None] * q[None, :, None] * d / np.linalg.norm(d, axis=2)[..., None] ** 3
    return -f.sum(axis=1), f.sum(axis=0), np.abs(f).sum(axis=1).max(), np.abs(f).sum(axis=0).max()


# ---- orientations -----------------------------------------------------------------------------------------------------
KINDS = ("two-centre ps swapped", "two-centre ps unswapped", "two-centre pp", "pp of a shell with itself")


def orientations(basis):
    """the kinds of KINDS among the shell pairs of a basis, by the rule of ``gto_pair_ref``"""
    out = set()
    sh = basis.shells
    for i in range(basis.nshell):
        for j in range(i + 1):
            li, lj = int(sh[i, 1]) & 255, int(sh[j, 1]) & 255
            sa, sb = (i, j) if li >= lj else (j, i)
            two = sh[sa, 0] != sh[sb, 0]
            if (max(li, lj), min(li, lj)) == (1, 0) and two:
                out.add(KINDS[0] if sa < sb else KINDS[1])
            if li == lj == 1:
                if two:
                    out.add(KINDS[2])
                elif sa == sb:
                    out.add(KINDS[3])
    return out


# ---- connection -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def connection_reference(name):
    """-> (T [natm, 3, N, N] of the host twin, read-only)"""
    basis, ang = gradient_case(name)
    T = gaussian.overlap_connection_from_table(basis.table, ang / BOHR)
    T.setflags(write=False)
    return T


def connection_scale(mats, T):
    return float(np.einsum("kmn,admn->kad", np.abs(mats), np.abs(T)).max())


# ---- fixtures ---------------------------------------------------------------------------------------------------------
def fixture_path(kind, name):
    return os.path.join(GOLDEN, f"charge_edges_{kind}_{str(name).replace('*', 'star')}.npz")


def key_of(form, M):
    return f"{(form or 'none')[:4]}_{M}"


@functools.lru_cache(maxsize=None)
def _load(kind, name):
    with np.load(fixture_path(kind, name)) as z:
        out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def operator_fixture(name, form, M):
    """-> (V_ext of the host twin [N, N] in the order of the case's functions, diff) ; O-cases read their base case"""
    basis, _, ao, base = operator_case(name, form)
    f = _load("op", base)
    V = f["V_" + key_of(form, M)]
    if ao is not None:
        V = V[np.ix_(ao, ao)]
    return V, float(f["diff_" + key_of(form, M)])


def nuclei_fixture(name):
    """-> (diff of V_ext with the nuclei as charges, in the case's own d form)"""
    return float(_load("op", name)["diff_nuclei"])


def gradient_fixture(name):
    """-> dict: rule, and per size M: gA_M [natm, 3], gQ_M [M, 3], dA_M, dQ_M (|FD - FD'| of each component; NaN
    outside the sample of a many-atom case)"""
    return _load("grad", name)
