"""Recorder: every tensor the stack-property methods of ``OO_pqc_batch`` return, written to one ``.npz`` file, so that
two checkouts can be compared bit for bit.

Batches: three geometries of water in STO-3G with ``oao_mo_coeffs="rhf"`` and CAS(2e,2o), plain (``water``) and embedded
in two point charges (``embedded``), and the two-geometry CAS(4e,3o) formaldimine batch of tests/test_moments_gpu.py
(``cas``: RHF orbitals times the exponential of a seeded skew matrix of norm 0.1).  Calls: ``rhf``, ``nuclear_gradient``,
``point_charge_gradient``, ``rhf_point_charge_gradient``, ``rhf_nuclear_gradient``, ``casci_nuclear_gradients``,
``casci_derivative_couplings``, ``casci_relaxed_gradients``, ``multipole_moments``, ``dipole_moment``,
``rhf_dipole_moment``, ``casci_dipole_matrix``, ``electrostatic_potential``, ``rhf_electrostatic_potential``,
``casci_electrostatic_potential`` (with and without the field), ``state_overlaps``, ``casci_overlaps``; ``nroots`` 1, 2,
3, ``index`` None / [2, 0] / 1, ``chunk`` None / 1 and ``small_gap="nan"`` where a method takes them.  A call that
raises is recorded as the type and text of what it raised (a batch without point charges refuses the charge methods,
the ``cas`` batch has no row 2 and its orbitals are not canonical: those refusals are part of the record).

  python tools/record_stack_properties.py --root CHECKOUT --out FILE.npz
  python tools/record_stack_properties.py --compare A.npz B.npz       np.array_equal of every array, NaNs at equal places
"""
import argparse
import json
import os
import sys

import numpy as np

WATER = np.array([[0.0, 0.01, 0.02], [0.3, 0.75, 0.55], [-0.2, -0.70, 0.62]])           # Angstrom (tools/gto_bench.py)
POINTS = [(140.0, 80.0), (100.0, 0.0)]                                                    # tests/test_moments_gpu.py


def compare(a, b):
    A, B = np.load(a), np.load(b)
    names = sorted(set(A.files) | set(B.files))
    bad = [n for n in names if n not in A.files or n not in B.files]
    for n in names:
        if n in bad:
            continue
        x, y = A[n], B[n]
        same = x.shape == y.shape and x.dtype == y.dtype and (
            np.array_equal(x, y, equal_nan=True) if x.dtype.kind == "f" else np.array_equal(x, y))
        if not same:
            bad.append(n)
    values = sum(int(A[n].size) for n in names if n in A.files)
    errors = sum(1 for n in names if n.endswith("/error"))
    nans = sum(int(np.isnan(A[n]).sum()) for n in names if n in A.files and A[n].dtype.kind == "f")
    print(json.dumps({"arrays": len(names), "values": values, "recorded_refusals": errors, "nan_values": nans,
                      "different": bad, "identical": not bad}))
    return 0 if not bad else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default="stack_properties.npz")
    ap.add_argument("--compare", nargs=2, metavar="FILE")
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    sys.path.insert(0, a.root)
    import torch
    import auto_oo_amd as aoo
    from auto_oo_amd import gto
    from auto_oo_amd.moldata import get_formal_geo

    device = aoo._lib.require_device()
    rng = np.random.default_rng(7)
    record = {}

    def put(name, value):
        """tensors, and tuples of tensors or None at any depth, as ``name``, ``name/0``, ``name/1/0``, ..."""
        if value is None:
            record[name + "/none"] = np.zeros(0)
        elif isinstance(value, torch.Tensor):
            record[name] = value.detach().cpu().numpy()
        elif isinstance(value, (bool, int, float, str)):
            record[name] = np.array(value)
        else:
            for k, v in enumerate(value):
                put(f"{name}/{k}", v)

    def call(name, f):
        try:
            put(name, f())
        except Exception as err:                                                # noqa: BLE001  (a refusal is a result)
            record[name + "/error"] = np.array(f"{type(err).__name__}: {err}")

    # ---- the three batches ----
    water = gto.GTOBasis(["O", "H", "H"])
    w_xyz = WATER[None] + rng.uniform(-0.05, 0.05, (3,) + WATER.shape)
    q = np.array([0.4, -0.3])
    q_xyz = np.array([[2.5, 0.5, -0.3], [-1.0, -2.8, 1.2]])                     # Angstrom
    pqc2 = aoo.Parameterized_circuit(2, 2, None, ansatz="np_fabric", n_layers=1)
    batches = {
        "water": aoo.OO_pqc_batch.from_geometries(pqc2, water, w_xyz, 2, 2, oao_mo_coeffs="rhf"),
        "embedded": aoo.OO_pqc_batch.from_geometries(pqc2, water, w_xyz, 2, 2, oao_mo_coeffs="rhf",
                                                     point_charges=(q, q_xyz))}
    formal = gto.GTOBasis(["N", "C", "H", "H", "H"])
    f_xyz = formal.coordinates([get_formal_geo(*p) for p in POINTS])
    pqc3 = aoo.Parameterized_circuit(3, 4, None, ansatz="ucc")
    start = aoo.OO_pqc_batch.from_geometries(pqc3, formal, f_xyz, 3, 4, oao_mo_coeffs="rhf")
    rot = np.random.default_rng(17)
    orbitals = []
    for U in start.oao_mo_coeff.cpu().numpy():
        K = rot.standard_normal(U.shape)
        K = K - K.T
        K *= 0.1 / np.linalg.norm(K)
        orbitals.append(U @ torch.linalg.matrix_exp(torch.as_tensor(K)).numpy())
    batches["cas"] = aoo.OO_pqc_batch.from_geometries(pqc3, formal, f_xyz, 3, 4, oao_mo_coeffs=orbitals)

    for tag, b in batches.items():
        G = b.G
        th = torch.as_tensor(np.random.default_rng(5).uniform(-0.6, 0.6, (G, b.n_theta))).to(device)
        pts = np.random.default_rng(11).uniform(-3.0, 3.0, (G, 3, 3)) + 4.0       # M = 3 points per geometry, Angstrom
        put(f"{tag}/orbitals", b.oao_mo_coeff)
        for index in (None, [2, 0], 1):
            p = pts if index is None else pts[np.atleast_1d(index) % G]
            i = f"{tag}/index={index}"
            call(f"{i}/rhf", lambda: b.rhf(index=index))
            call(f"{i}/point_charge_gradient", lambda: b.point_charge_gradient(th, index=index))
            call(f"{i}/rhf_point_charge_gradient", lambda: b.rhf_point_charge_gradient(index=index))
            call(f"{i}/rhf_nuclear_gradient", lambda: b.rhf_nuclear_gradient(index=index))
            call(f"{i}/multipole_moments", lambda: b.multipole_moments(th, index=index))
            call(f"{i}/multipole_moments/origin", lambda: b.multipole_moments(th, order=1, index=index,
                                                                               origin=np.array([0.1, -0.2, 0.3])))
            call(f"{i}/dipole_moment", lambda: b.dipole_moment(th, index=index))
            call(f"{i}/rhf_dipole_moment", lambda: b.rhf_dipole_moment(index=index))
            for field in (False, True):
                call(f"{i}/electrostatic_potential/field={field}",
                     lambda: b.electrostatic_potential(th, p, index=index, field=field))
                call(f"{i}/electrostatic_potential/shared/field={field}",
                     lambda: b.electrostatic_potential(th, pts[0], index=index, field=field))
                call(f"{i}/rhf_electrostatic_potential/field={field}",
                     lambda: b.rhf_electrostatic_potential(p, index=index, field=field))
            for chunk in (None, 1):
                c = f"{i}/chunk={chunk}"
                call(f"{c}/nuclear_gradient", lambda: b.nuclear_gradient(th, index=index, chunk=chunk))
                for R in (1, 2, 3):
                    kw = dict(nroots=R, index=index, chunk=chunk)
                    call(f"{c}/casci_nuclear_gradients/R={R}", lambda: b.casci_nuclear_gradients(**kw))
                    call(f"{c}/casci_derivative_couplings/R={R}",
                         lambda: b.casci_derivative_couplings(small_gap="nan", **kw))
                    call(f"{c}/casci_derivative_couplings/min_gap=10/R={R}",
                         lambda: b.casci_derivative_couplings(small_gap="nan", min_gap=10.0, **kw))
                    call(f"{c}/casci_relaxed_gradients/R={R}", lambda: b.casci_relaxed_gradients(small_gap="nan", **kw))
        # an RHF result handed in, and the refusal of one with another number of geometries
        res = b.rhf()
        call(f"{tag}/result/rhf_nuclear_gradient", lambda: b.rhf_nuclear_gradient(res))
        call(f"{tag}/result/rhf_dipole_moment", lambda: b.rhf_dipole_moment(res))
        call(f"{tag}/result/rhf_electrostatic_potential", lambda: b.rhf_electrostatic_potential(pts, res, field=True))
        call(f"{tag}/result/rhf_point_charge_gradient", lambda: b.rhf_point_charge_gradient(res))
        call(f"{tag}/result/wrong_count", lambda: b.rhf_dipole_moment(res, index=[0]))
        for R in (1, 2, 3):
            call(f"{tag}/casci_dipole_matrix/R={R}", lambda: b.casci_dipole_matrix(nroots=R))
            for field in (False, True):
                call(f"{tag}/casci_electrostatic_potential/R={R}/field={field}",
                     lambda: b.casci_electrostatic_potential(pts, nroots=R, field=field))
            call(f"{tag}/casci_overlaps/R={R}", lambda: b.casci_overlaps(nroots=R))
        for metric in ("ao", "oao"):
            call(f"{tag}/state_overlaps/{metric}", lambda: b.state_overlaps(th, metric=metric))
        # refusals of the arguments
        call(f"{tag}/refusal/small_gap", lambda: b.casci_derivative_couplings(small_gap="zero"))
        call(f"{tag}/refusal/small_gap/relaxed", lambda: b.casci_relaxed_gradients(small_gap="zero"))
        call(f"{tag}/refusal/index", lambda: b.nuclear_gradient(th, index=[G]))
        call(f"{tag}/refusal/points", lambda: b.electrostatic_potential(th, np.zeros((3, 2))))
        call(f"{tag}/refusal/points/none", lambda: b.electrostatic_potential(th, np.zeros((G, 0, 3))))
        call(f"{tag}/refusal/points/finite", lambda: b.electrostatic_potential(th, np.full((3, 3), np.nan)))
        call(f"{tag}/refusal/nroots", lambda: b.casci_nuclear_gradients(nroots=5))
    torch.cuda.synchronize()
    out = os.path.abspath(a.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez(out, **record)
    errors = sorted(n for n in record if n.endswith("/error"))
    print(json.dumps({"tool": "record_stack_properties", "root": a.root, "arrays": len(record),
                      "recorded_refusals": len(errors), "out": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
