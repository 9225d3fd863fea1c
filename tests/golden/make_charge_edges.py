"""Writes tests/golden/charge_edges_op_<case>.npz and charge_edges_grad_<case>.npz, the recorded host-twin results of the
edge tests of the point-charge kernels (cases, clouds and readers: tests/_charge_edges.py).  Host only.

    python tests/golden/make_charge_edges.py                 # everything
    python tests/golden/make_charge_edges.py op Lss G2       # some operator cases
    python tests/golden/make_charge_edges.py grad LSP 43     # some gradient cases (a number: a many-atom case)

op, per (d form, M): V_<form>_<M> from ``gaussian.point_charge_integrals_from_table`` and diff_<form>_<M>, the largest
elementwise change when every Boys order n is multiplied by 1 + ``_gto_d.BOYS_RTOL[n]`` * (+-1 at random, seed 1);
diff_nuclei: the same change with the nuclei as the charges, in the case's own d form; G4 also g4_<form>, its largest
difference from G1 at M = 257.  G2: the elements between fragments are asserted to be exactly 0.

grad, per size M: gA_<M>, gQ_<M> (the finer step of the chosen rule) and dA_<M>, dQ_<M> (its disagreement with the other
step), rule, near.  The rule is the one of ``_charge_edges.RULES`` with the smallest disagreement; the run fails if that
exceeds ``FD_CAP`` = 1e-8 -- the answer to that is a larger ``NEAR_OF[case]``, never a larger cap.

The files are reproduced bit for bit by a second run.  Run time on one core: op 25 s in all (Ldd 10 s, L3 6 s); grad
4 s (Lss, HF*) to 35 s (LSP, formaldimine, 106 atoms) per case, 3 minutes in all."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import _charges as C           # noqa: E402
from tests import _charge_edges as X      # noqa: E402
from tests import _gto_edges as E         # noqa: E402


def make_op(name):
    t0 = time.time()
    forms = X.forms_of(name)
    out, worst = {}, 0.0
    for M in X.sizes_of(name):
        for form, (V, diff) in X.make_operator(name, M, forms).items():
            out["V_" + X.key_of(form, M)], out["diff_" + X.key_of(form, M)] = V, diff
            worst = max(worst, diff)
    basis = E.basis_of(name)
    R = E.xyz_of(name)
    Vn = X.host_operator(basis.table, R, basis.charges, R, E.form_of(name))
    Vn2 = X.host_operator(basis.table, R, basis.charges, R, E.form_of(name), E.perturbed_boys(1))
    out["diff_nuclei"] = np.abs(Vn2 - Vn).max()
    extra = ""
    if name == "G4":
        for form in forms:
            V1 = X.make_operator("G1", 257, (form,))[form][0]
            out["g4_" + X.key_of(form, 257)] = np.abs(out["V_" + X.key_of(form, 257)] - V1).max()
            extra += f", G4 - G1 ({form}) {out['g4_' + X.key_of(form, 257)]:.2e}"
    if name == "G2":
        frag = E.fragment_of_ao(basis)
        apart = frag[:, None] != frag[None, :]
        assert not out["V_" + X.key_of("spherical", 257)][apart].any()
        extra += ", between fragments exactly 0"
    np.savez(X.fixture_path("op", name), **out)
    V = out["V_" + X.key_of(forms[0], X.sizes_of(name)[-1])]
    print(f"op {name}: nao {V.shape[0]}, max |V_ext| {np.abs(V).max():.3g}, largest diff {worst:.2e}, diff_nuclei "
          f"{out['diff_nuclei']:.2e}{extra}, {os.path.getsize(X.fixture_path('op', name))} bytes, {time.time() - t0:.0f} s",
          flush=True)


def make_grad(name):
    t0 = time.time()
    many = not isinstance(name, str)
    basis, ang = X.many_atoms(name) if many else X.gradient_case(name)
    sizes = (X.MANY_ATOMS_M,) if many else X.GRADIENT_SIZES.get(name, (X.M_GRAD,))
    M = max(sizes)
    q, r = X.gradient_cloud(name, M)
    R, rb = ang / X.BOHR, C.bohr(r)
    Dm = C.random_symmetric(basis.nao, X.D_SEED)
    atoms = (0, basis.natm // 2, basis.natm - 1) if many else None
    charges = X.SAMPLE_CHARGES if many else None
    best = None
    for rule, (order, h, other) in X.RULES.items():
        if many and order != 2:
            continue
        fine = X.fd_gradients(basis, R, q, rb, Dm, order, h, atoms, charges)
        coarse = X.fd_gradients(basis, R, q, rb, Dm, order, other, atoms, charges)
        res = {}
        for m in sizes:
            gA, gA2 = fine[0][:m].sum(axis=0), coarse[0][:m].sum(axis=0)
            res.update({f"gA_{m}": gA, f"gQ_{m}": fine[1][:m], f"dA_{m}": np.abs(gA - gA2),
                        f"dQ_{m}": np.abs(fine[1][:m] - coarse[1][:m])})
        dis = max(np.nanmax(res[f"d{w}_{m}"]) for m in sizes for w in "AQ")
        print(f"    {name} {rule}: disagreement {dis:.2e}", flush=True)
        if best is None or dis < best[0]:
            best = (dis, rule, res)
    dis, rule, res = best
    near = X.NEAR_OF.get(name, C.NEAR)
    assert dis < X.FD_CAP, (name, rule, dis, "move the near charge outward: _charge_edges.NEAR_OF")
    np.savez(X.fixture_path("grad", name), rule=np.array(rule), near=np.float64(near), **res)
    print(f"grad {name}: {rule}, near charge at {near} Bohr, max |gA| {np.nanmax(np.abs(res[f'gA_{M}'])):.3g}, max |gQ| "
          f"{np.nanmax(np.abs(res[f'gQ_{M}'])):.3g}, disagreement {dis:.2e}, "
          f"{os.path.getsize(X.fixture_path('grad', name))} bytes, {time.time() - t0:.0f} s", flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    kinds = [a for a in args if a in ("op", "grad")] or ["op", "grad"]
    names = [a for a in args if a not in ("op", "grad")]
    if "op" in kinds:
        for case in (names or tuple(E.L_CASES) + E.G_NAMES):
            make_op(case)
    if "grad" in kinds:
        for case in (names or X.GRADIENT_CASES + X.MANY_ATOMS):
            make_grad(int(case) if str(case).isdigit() else case)
