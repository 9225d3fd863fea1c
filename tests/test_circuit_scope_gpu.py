"""The dense-register circuit and RDM kernels (csrc/circuit.hip, csrc/circuit_small.h, csrc/spin_rdms.hip) over their
whole scope, through ops.circuit_state / rdms / rdms_tangent / circuit_rdms / circuit_hessian / spin_rdms, against the
host twin of tests/_circuit_scope.py (validated in tests/test_circuit_scope_cpu.py): odd registers, the last
LDS-resident register (13 qubits) and the first two in global memory (14, 15), both sides of every route switch,
transition RDMs with bra != ket, tangents of parameters that drive several gates, batches, the refusals.  Every output
starts as NaN (ops' allocations are swapped for NaN-filled ones), every element is compared, and every test prints
its largest error / bound before it asserts.  The bounds are derived in tests/_circuit_scope.py and DESIGN.md ("The
dense-register kernels over their whole scope"); none comes from device output.

The 14- and 15-qubit cases with a parameter that drives several gates (GateFabric, the hand-made list, the shared
ladder), the 14-qubit Hessian and the 14-qubit circuit_rdms derivative sets are the ones that failed before the
tangent of such a parameter was summed over all of its gates beyond the LDS-resident register.

Largest error / bound measured on an MI355X, per family (all 237 cases passed):
    state 0.148    tangent 0.060    RDM 0.081    derivative RDM 0.081    Hessian 0.0016    spin RDM 0.053
(at 14 and 15 qubits: state 0.016, tangent 0.006, the others below 0.0005)."""
import ctypes

import numpy as np
import pytest
import torch

from auto_oo_amd import _lib, excitations as X, ops
from auto_oo_amd._lib import OovqeError, check, dptr, stream_ptr
from tests import _circuit_scope as C
from tests import _sector_scope as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
FIGURES = {}


class _NanTorch:
    """``torch`` as auto_oo_amd.ops sees it during these tests: ``empty`` hands out NaN (outputs, workspace)."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(*args, **kwargs):
        t = torch.empty(*args, **kwargs)
        if t.dtype.is_floating_point:
            t.fill_(float("nan"))
        return t


@pytest.fixture(autouse=True)
def nan_outputs(monkeypatch):
    monkeypatch.setattr(ops, "torch", _NanTorch())
    ops._CHESS_WORK.clear()
    yield
    ops._CHESS_WORK.clear()


@pytest.fixture(scope="module", autouse=True)
def figures():
    yield
    for group in sorted(FIGURES):
        print(f"largest error / bound, {group}: {FIGURES[group]:.4f}")


def dev(x, dtype=F64):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def gates_dev(gates):
    return torch.as_tensor(X.gates_to_numpy(gates)).to(DEV)


def record(group, what, err, bound):
    """print the figure next to its bound, remember the largest ratio of the group, assert every element."""
    err = np.atleast_1d(np.asarray(err, dtype=np.float64))
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    assert np.isfinite(err).all(), f"{what}: NaN or Inf in the result"
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    print(f"{group}: {what}: largest error {float(err.max()):.3e}, bound there "
          f"{float(bound.reshape(-1)[int(err.argmax())]):.3e}, largest error / bound {ratio:.3f}")
    FIGURES[group] = max(FIGURES.get(group, 0.0), ratio)
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} elements past their bound (ratio {ratio:.3f})"


def norms(d):
    return np.linalg.norm(d, axis=-1)


def shared(gates, n_theta):
    return any(len(own) > 1 for own in S.param_gates(gates, n_theta))


# ---- states and tangents ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tangents", [False, True], ids=["state", "tangents"])
@pytest.mark.parametrize("case", C.STATE_CASES, ids=C.state_id)
def test_circuit_state(case, tangents):
    n, kind, _, batch = case
    gates, n_theta, _ = C.gate_list(kind, n)
    init = C.start_index(case)
    th, psi, dpsi = C.state_reference(case)
    es, tb = C.state_bounds(case, dpsi)
    gd = gates_dev(gates)
    assert ops.shares_parameters(gd, len(gates)) == shared(gates, n_theta)
    res = ops.circuit_state(dev(th), gd, len(gates), n, init, tangents=tangents)
    got = (res[0] if tangents else res).cpu().numpy()
    record("state", C.state_id(case), norms(got - psi), es)
    if tangents:
        got = res[1].cpu().numpy()
        record("tangent", C.state_id(case), norms(got - dpsi), tb)
        for k, own in enumerate(S.param_gates(gates, n_theta)):
            if not own:
                assert not got[:, k].any()           # a parameter with no gate: exactly zero


def test_state_table_has_both_sides_of_the_lds_edge():
    assert ops.LDS_STATE_MAX == 1 << C.LDS_STATE_MAX_QUBITS
    assert {C.route(c[0]) for c in C.STATE_CASES} == {"lds", "global"}
    for route in ("lds", "global"):
        assert any(C.route(c[0]) == route and shared(*C.gate_list(c[1], c[0])[:2]) for c in C.STATE_CASES)
        assert any(C.route(c[0]) == route and not shared(*C.gate_list(c[1], c[0])[:2]) for c in C.STATE_CASES)


def _state_abi(name, th, gd, n_gates, n, init, tangents, scratch=None):
    lib = _lib.load()
    batch, n_theta = th.shape
    psi = torch.full((batch, 1 << n), float("nan"), dtype=F64, device=DEV)
    dpsi = torch.full((batch, n_theta, 1 << n), float("nan"), dtype=F64, device=DEV) if tangents else None
    args = [dptr(th), n_theta, dptr(gd, torch.uint8), n_gates, n, ctypes.c_uint32(init), batch, dptr(psi), dptr(dpsi)]
    if name == "oovqe_circuit_state_ws":
        args.append(dptr(scratch))
    check(getattr(lib, name)(*args, stream_ptr()), name)
    return psi, dpsi


def test_entry_point_without_scratch_beyond_the_lds_register():
    """oovqe_circuit_state has no scratch: a parameter that drives several gates is refused at 14 qubits, not answered
    with the first gate's term; a list without one goes through and gives the bits of the entry point with scratch."""
    gates, n_theta, init = C.gate_list("hand", 14)
    th = dev(C.thetas("abi", 1, n_theta))
    gd = gates_dev(gates)
    with pytest.raises(OovqeError, match="several gates"):
        _state_abi("oovqe_circuit_state", th, gd, len(gates), 14, init, True)
    with pytest.raises(OovqeError, match="several gates"):
        _state_abi("oovqe_circuit_state_ws", th, gd, len(gates), 14, init, True, None)
    psi, _ = _state_abi("oovqe_circuit_state", th, gd, len(gates), 14, init, False)      # no tangents: no scratch
    assert torch.isfinite(psi).all()
    gates, n_theta, init = C.gate_list("kupccd", 14)
    th = dev(C.thetas("abi2", 1, n_theta))
    gd = gates_dev(gates)
    a = _state_abi("oovqe_circuit_state", th, gd, len(gates), 14, init, True)
    b = ops.circuit_state(th, gd, len(gates), 14, init, tangents=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- RDMs ------------------------------------------------------------------------------------------------------------
def check_rdm_sets(group, what, g1, g2, refs):
    """refs: per batch element (gamma, Gamma, bound, bound)."""
    g1, g2 = g1.cpu().numpy(), g2.cpu().numpy()
    for b, (r1, r2, b1, b2) in enumerate(refs):
        record(group, f"{what} gamma[{b}]", np.abs(g1[b] - r1), b1)
        record(group, f"{what} Gamma[{b}]", np.abs(g2[b] - r2), b2)


@pytest.mark.parametrize("ncas,batch,same", C.RDM_CASES)
def test_rdms(ncas, batch, same):
    refs = [C.rdm_reference(ncas, i, same) for i in range(batch)]
    bra, ket = np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs])
    g1, g2 = ops.rdms(dev(bra), dev(ket), ncas)
    check_rdm_sets("RDM", f"ncas {ncas} batch {batch} {'bra = ket' if same else 'bra != ket'}", g1, g2,
                   [r[2:] for r in refs])


def tangent_refs(ncas, batch, n_tan):
    """the sets 0 .. n_tan of the five-tangent reference of each element."""
    return [tuple(x[:1 + n_tan] for x in C.rdm_tangent_reference(ncas, b, 5)) for b in range(batch)]


@pytest.mark.parametrize("ncas,n_tan,batch", C.RDM_TANGENT_CASES)
def test_rdms_tangent(ncas, n_tan, batch):
    vecs = [C.tangent_vectors(ncas, b) for b in range(batch)]
    psi = dev(np.stack([v[0] for v in vecs]))
    dpsi = dev(np.stack([v[1][:n_tan] for v in vecs])) if n_tan else None
    g1, g2 = ops.rdms_tangent(psi, dpsi, ncas)
    assert g1.shape == (batch, 1 + n_tan, ncas, ncas)
    check_rdm_sets("derivative RDM", f"ncas {ncas} n_tan {n_tan} batch {batch}", g1, g2, tangent_refs(ncas, batch, n_tan))


def test_rdms_tangent_at_the_grid_limit():
    ncas, nvec = C.RDM_TANGENT_LIMIT
    assert nvec * ncas * ncas <= 65535 < (nvec + 1) * ncas * ncas
    D, reg = 1 << (2 * ncas), C.register(ncas)
    rng = np.random.default_rng(31)
    psi, dpsi = rng.standard_normal(D), rng.standard_normal((nvec, D))
    g1, g2 = ops.rdms_tangent(dev(psi[None]), dev(dpsi[None, :nvec - 1]), ncas)
    assert torch.isfinite(g1).all() and torch.isfinite(g2).all()
    g1, g2 = g1.cpu().numpy()[0], g2.cpu().numpy()[0]
    for k in C.RDM_TANGENT_LIMIT_SETS:
        one = dpsi[k - 1:k] if k else dpsi[:0]                   # set k of the call = set len(one) of this twin call
        r1, r2 = reg.rdms_tangent(psi, one)
        b1, b2 = C.rdm_tangent_bounds(reg, psi, one)
        record("derivative RDM", f"grid limit, set {k} gamma", np.abs(g1[k] - r1[-1]), b1[-1])
        record("derivative RDM", f"grid limit, set {k} Gamma", np.abs(g2[k] - r2[-1]), b2[-1])
    with pytest.raises(OovqeError, match="grid too large"):
        ops.rdms_tangent(dev(psi[None]), dev(dpsi[None]), ncas)


# ---- state + tangents + RDM sets in one call -------------------------------------------------------------------------
def test_circuit_rdms_table_has_both_sides_of_the_switch():
    lib = _lib.load()
    for ncas, kind, small in C.CIRCUIT_RDMS_CASES:
        gates, n_theta, _ = C.gate_list(kind, 2 * ncas)
        assert bool(lib.oovqe_circuit_rdms_is_small(2 * ncas, ncas, 1 + n_theta, len(gates))) == small, (ncas, kind)
    for ncas in (3, 4):
        assert {c[2] for c in C.CIRCUIT_RDMS_CASES if c[0] == ncas} == {True, False}
    for n_theta in (1, 2, 15, 40):          # five orbitals: never the one-workgroup kernel
        assert not lib.oovqe_circuit_rdms_is_small(10, 5, 1 + n_theta, 20)
    assert not lib.oovqe_circuit_rdms_is_small(10, 5, 1, 1)


@pytest.mark.parametrize("want_states", [False, True], ids=["sets", "sets+states"])
@pytest.mark.parametrize("tangents", [False, True], ids=["state", "tangents"])
@pytest.mark.parametrize("ncas,kind,small", C.CIRCUIT_RDMS_CASES)
def test_circuit_rdms(ncas, kind, small, tangents, want_states):
    lib = _lib.load()
    n = 2 * ncas
    for batch in (C.CIRCUIT_RDMS_BATCHES if ncas < 7 else C.CIRCUIT_RDMS_BATCHES[:1]):
        gates, n_theta, init, th = C.circuit_case(ncas, kind, 5)
        if tangents:
            assert bool(lib.oovqe_circuit_rdms_is_small(n, ncas, 1 + n_theta, len(gates))) == small
        refs = [C.circuit_rdms_reference(ncas, kind, b) for b in range(batch)]
        out = ops.circuit_rdms(dev(th[:batch]), gates_dev(gates), len(gates), n, ncas, init, tangents=tangents,
                               want_states=want_states)
        what = f"ncas {ncas} {kind} batch {batch}"
        n_set = 1 + n_theta if tangents else 1
        assert out[0].shape[:2] == (batch, n_set)
        check_rdm_sets("derivative RDM" if tangents else "RDM", what, out[0], out[1],
                       [tuple(x[:n_set] for x in r[2:6]) for r in refs])
        if want_states:
            record("state", what, norms(out[2].cpu().numpy() - np.stack([r[0] for r in refs])), refs[0][6])
            if tangents:
                record("tangent", what, norms(out[3].cpu().numpy() - np.stack([r[1] for r in refs])),
                       np.stack([r[7] for r in refs]))
            else:
                assert out[3] is None


# ---- the theta-theta Hessian -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncas,kind", C.HESSIAN_CASES)
def test_circuit_hessian(ncas, kind):
    gates, n_theta, init, _ = C.circuit_case(ncas, kind, 1)
    th, c1, c2, H, B = C.hessian_reference(ncas, kind)
    got = ops.circuit_hessian(dev(th), gates_dev(gates), len(gates), 2 * ncas, ncas, init, dev(c1), dev(c2))
    got = got.cpu().numpy()
    assert got.shape == (n_theta, n_theta)
    record("Hessian", f"ncas {ncas} {kind}", np.abs(got - H), B)         # both triangles, every element


# ---- spin-orbital RDMs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch", C.SPIN_CASES)
def test_spin_rdms(n, batch):
    refs = [C.spin_reference(n, i) for i in range(batch)]
    g1, g2 = ops.spin_rdms(dev(np.stack([r[0] for r in refs])), dev(np.stack([r[1] for r in refs])), n)
    check_rdm_sets("spin RDM", f"{n} qubits batch {batch}", g1, g2, [r[2:] for r in refs])


# ---- the refusals ----------------------------------------------------------------------------------------------------
def tiny(n=4):
    return torch.zeros(n, dtype=F64, device=DEV)


def test_refusals_of_circuit_state():
    lib = _lib.load()
    gates, n_theta, init = C.gate_list("hand", 4)
    gd, th = gates_dev(gates), dev(np.zeros((1, n_theta)))
    for name in ("oovqe_circuit_state", "oovqe_circuit_state_ws"):
        for n in (1, 27):                    # the check precedes any access: the buffers may be tiny
            args = [dptr(th), n_theta, dptr(gd, torch.uint8), len(gates), n, ctypes.c_uint32(0), 1, dptr(tiny()), None]
            if name.endswith("_ws"):
                args.append(None)
            with pytest.raises(OovqeError, match="n_qubits"):
                check(getattr(lib, name)(*args, stream_ptr()), name)
    for bad in (16, 17, 2 ** 32 - 1):
        with pytest.raises(OovqeError, match="init_index"):
            ops.circuit_state(th, gd, len(gates), 4, bad)
    assert torch.isfinite(ops.circuit_state(th, gd, len(gates), 4, 15)).all()


def test_refusals_of_the_rdm_entry_points():
    lib = _lib.load()
    t = tiny(64)
    with pytest.raises(OovqeError, match="bad sizes"):
        check(lib.oovqe_rdms(dptr(t), dptr(t), 5, 2, 1, dptr(t), dptr(t), dptr(t), stream_ptr()), "oovqe_rdms")
    with pytest.raises(OovqeError, match="bad sizes"):
        check(lib.oovqe_rdms(dptr(t), dptr(t), 3, 2, 1, dptr(t), dptr(t), dptr(t), stream_ptr()), "oovqe_rdms")
    # the general route puts the batch into a 16-bit grid dimension (argument check only: nothing is launched)
    with pytest.raises(OovqeError, match="batch too large"):
        check(lib.oovqe_rdms(dptr(t), dptr(t), 10, 5, 65536, dptr(t), dptr(t), dptr(t), stream_ptr()), "oovqe_rdms")
    for n in (0, 21):
        with pytest.raises(OovqeError, match="n_qubits"):
            check(lib.oovqe_spin_rdms(dptr(t), dptr(t), n, 1, dptr(t), dptr(t), stream_ptr()), "oovqe_spin_rdms")
