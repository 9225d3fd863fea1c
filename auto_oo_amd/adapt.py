"""ADAPT-VQE: a circuit grown from the Hamiltonian, one pool operator at a time.

At fixed orbitals E(theta) = c0 + Q(psi(theta)), Q(v) = c1 . gamma(v) + c2 . Gamma(v) = v^T Hop v.  A pool operator
is one parameter driving 1 to 4 gates of the ordinary gate table (``excitations.GateT``); appended behind the circuit
with its parameter at 0 its energy derivative is
    g = sum over its gates, over the gate's determinant pairs (x, y)  (sign / 2) pi(x) (psi[y] lam[x] - psi[x] lam[y]),
    lam = (Hop + Hop^T) psi
-- ONE application of the operator per state and one sparse scalar product per pool operator
(``oovqe_pool_gradients_from_coefficients_batch``, csrc/pool.hip) where appending each candidate to a circuit of its
own and differentiating that takes P + 1 evaluations.

``OperatorPool`` is host data (building one touches no device); ``OO_pqc.pool_gradients`` /
``OO_pqc_batch.pool_gradients`` evaluate it, ``OO_pqc_batch.set_circuit`` hands a stack a new circuit without touching
its resident integrals, ``adapt_vqe`` is the driver for one geometry or a stack.
"""
import ctypes
from collections import namedtuple
from itertools import combinations

import numpy as np
import torch

from . import _lib, excitations as X
from ._lib import GateT, check, dptr, stream_ptr

F64 = torch.float64
MAX_GATES_PER_OPERATOR = 4
MAX_DETERMINANTS = 32767          # the pair lists hold 15-bit determinant indices (oovqe_sector_pairs)

AdaptResult = namedtuple("AdaptResult",
                         "gates operators thetas energies gradient_norms max_gradients pool_gradients oo converged")
AdaptResult.__doc__ = """What ``adapt_vqe`` returns: ``gates`` the final gate table; ``operators`` the pool index
chosen at every addition; ``thetas`` the final parameters ([n] for one geometry, [G, n] for a stack); ``energies``,
``gradient_norms``, ``max_gradients``: after every addition and its re-optimisation the energy (a float, or [G] per
geometry), the pool-gradient norm and the largest |g| (for a stack: the largest over the geometries);
``pool_gradients``: the gradients ([P], or [G, P]) every choice was made from; ``oo`` the final object (its circuit
is the grown one); ``converged``: the pool-gradient norm fell below ``grad_tol``."""


def _copy_gate(g, theta_idx):
    return X._gate(int(g.mask_hi), int(g.mask_lo), int(g.mask_par), int(theta_idx), int(g.sign))


def _alpha_mask(n):
    """bits of the even wires (alpha spin orbitals); wire w sits at bit n - 1 - w."""
    m = 0
    for w in range(0, n, 2):
        m |= 1 << (n - 1 - w)
    return m


def _popc(v):
    return bin(int(v)).count("1")


def gsd_excitations(n):
    """The generalised singles and doubles over ``n`` spin orbitals (even = alpha): every single [r, p], r < p, between
    two spin orbitals of equal spin; every double between two disjoint pairs of spin orbitals of equal total s_z, each
    unordered {pair, pair} once, as ([i, j], [k, l]) with i < j, k < l and i the lowest of the four."""
    singles = [[r, p] for r in range(n) for p in range(r + 1, n) if (r - p) % 2 == 0]
    sz2 = lambda pr: (1 if pr[0] % 2 == 0 else -1) + (1 if pr[1] % 2 == 0 else -1)         # noqa: E731
    pairs = list(combinations(range(n), 2))
    doubles = [(list(a), list(b)) for ia, a in enumerate(pairs) for b in pairs[ia + 1:]
               if not set(a) & set(b) and sz2(a) == sz2(b)]
    return singles, doubles


def gsd_double_gate(pair_hi, pair_lo, n, theta_idx):
    """The Givens gate between the determinants with ``pair_hi`` occupied / ``pair_lo`` empty and the reverse, with the
    Jordan-Wigner parity over the spin orbitals strictly between the lowest two and strictly between the highest two
    of the four (``fde_gate`` when the pairs do not interleave)."""
    idx = sorted(list(pair_hi) + list(pair_lo))
    par = 0
    for w in list(range(idx[0] + 1, idx[1])) + list(range(idx[2] + 1, idx[3])):
        par |= X._bit(w, n)
    return X._gate(X._bit(pair_hi[0], n) | X._bit(pair_hi[1], n), X._bit(pair_lo[0], n) | X._bit(pair_lo[1], n), par,
                   theta_idx, +1)


class OperatorPool:
    """The candidate operators of an ADAPT-VQE run on CAS(nelecas, ncas).

    ``kind``: ``"sd"`` -- the singles and doubles of ``excitations.excitations`` out of the Hartree-Fock determinant, as
    the gates of ``uccd_gates(add_singles=True)`` (singles first, in its parameter order); ``"gsd"`` -- generalised
    singles and doubles (``gsd_excitations``); ``"pair"`` -- ``generalized_pair_doubles``; or a list of operators, each
    a list of 1 to 4 ``GateT`` sharing one parameter (their ``theta_idx`` is ignored).  Every gate must conserve
    (N_alpha, N_beta): ValueError otherwise.  Host data only; the pair lists of a sector are made on first use on a
    device (``oovqe_sector_pairs``) and cached."""

    def __init__(self, ncas, nelecas, kind="sd"):
        self.ncas, self.nelecas = int(ncas), int(nelecas)
        n = self.n_qubits = 2 * self.ncas
        if not (1 <= self.ncas <= 13 and 0 <= self.nelecas <= n):
            raise ValueError(f"no pool for CAS({nelecas}e, {ncas}o)")
        if isinstance(kind, str):
            self.kind = kind
            if kind == "sd":
                gates, n_theta = X.uccd_gates(self.ncas, self.nelecas, add_singles=True)
                ops_ = [[g for g in gates if g.theta_idx == k] for k in range(n_theta)]
            elif kind == "gsd":
                singles, doubles = gsd_excitations(n)
                ops_ = [[X.fse_gate(range(r, p + 1), n, 0)] for r, p in singles]
                ops_ += [[gsd_double_gate(a, b, n, 0)] for a, b in doubles]
            elif kind == "pair":
                ops_ = [[X.fde_gate(w1, w2, n, 0)] for w1, w2 in X.generalized_pair_doubles(range(n))]
            else:
                raise ValueError(f"unknown pool {kind!r}: 'sd', 'gsd', 'pair' or a list of operators")
        else:
            self.kind = "custom"
            ops_ = [list(op) if isinstance(op, (list, tuple)) else [op] for op in kind]
        if not ops_:
            raise ValueError("an operator pool needs at least one operator")
        alpha = _alpha_mask(n)
        beta = ((1 << n) - 1) ^ alpha
        self.operators = []
        for k, op in enumerate(ops_):
            if not 1 <= len(op) <= MAX_GATES_PER_OPERATOR or not all(isinstance(g, GateT) for g in op):
                raise ValueError(f"operator {k}: 1 to {MAX_GATES_PER_OPERATOR} excitations.GateT gates sharing one "
                                 "parameter")
            for g in op:
                hi, lo = int(g.mask_hi), int(g.mask_lo)
                if hi & lo or not (hi | lo) or (hi | lo | int(g.mask_par)) >> n or int(g.sign) not in (1, -1):
                    raise ValueError(f"operator {k}: a gate with overlapping, empty or out-of-register masks, or a "
                                     "sign other than +-1")
                if _popc(hi & alpha) != _popc(lo & alpha) or _popc(hi & beta) != _popc(lo & beta):
                    raise ValueError(f"operator {k} does not conserve (N_alpha, N_beta): hi = {hi:0{n}b}, "
                                     f"lo = {lo:0{n}b}")
            self.operators.append([_copy_gate(g, k) for g in op])
        self.n_operators = len(self.operators)
        self.gates = [g for op in self.operators for g in op]
        self.n_gates = len(self.gates)
        if self.n_gates > 65535:
            raise ValueError(f"a pool of {self.n_gates} gates (at most 65 535)")
        first = np.zeros(self.n_operators + 1, dtype=np.int32)
        first[1:] = np.cumsum([len(op) for op in self.operators])
        self.op_first = first
        self.gate_sign = np.array([int(g.sign) for g in self.gates], dtype=np.int32)
        self._tables = {}

    def __len__(self):
        return self.n_operators

    def operator_gates(self, k, theta_idx):
        """The gates of operator ``k`` driven by parameter ``theta_idx`` -- what appending it adds to a gate table."""
        return [_copy_gate(g, theta_idx) for g in self.operators[int(k)]]

    def device_tables(self, engine):
        """(pairs, tables pointer, op_first, gate_sign) of this pool in the sector of ``engine`` (a ``SectorEngine``)
        on its device: ``oovqe_sector_pairs`` once per (sector, device)."""
        key = (engine.n_alpha, engine.n_beta, str(engine.device))
        hit = self._tables.get(key)
        if hit is None:
            lib = _lib.load()
            if engine.Dc > MAX_DETERMINANTS:
                raise ValueError(f"pool gradients: {engine.Dc} determinants (pair lists hold at most "
                                 f"{MAX_DETERMINANTS})")
            n = int(lib.oovqe_sector_pairs_size(self.n_gates, engine.na, engine.nb))
            nt = int(lib.oovqe_sector_tables_size(self.ncas, engine.na, engine.nb))
            pairs = torch.empty(n + nt, dtype=torch.int32, device=engine.device)
            gates_dev = torch.as_tensor(X.gates_to_numpy(self.gates)).to(engine.device)
            check(lib.oovqe_sector_pairs(dptr(gates_dev, torch.uint8), self.n_gates, self.ncas, *engine._tabs(),
                                         dptr(pairs, torch.int32), stream_ptr()), "oovqe_sector_pairs")
            hit = self._tables[key] = (pairs, ctypes.c_void_p(pairs.data_ptr() + 4 * n),
                                       torch.as_tensor(self.op_first).to(engine.device),
                                       torch.as_tensor(self.gate_sign).to(engine.device), gates_dev)
        return hit[:4]


def check_pool(pool, pqc, who="pool_gradients"):
    """The refusals every entry point makes before anything is enqueued."""
    if not isinstance(pool, OperatorPool):
        raise ValueError(f"{who}: pool must be an OperatorPool, got {type(pool).__name__}")
    if pool.ncas != int(pqc.ncas) or pool.nelecas != int(pqc.nelecas):
        raise ValueError(f"{who}: the pool is for CAS({pool.nelecas}e, {pool.ncas}o), the circuit for "
                         f"CAS({pqc.nelecas}e, {pqc.ncas}o)")
    if pqc._sector.Dc > MAX_DETERMINANTS:
        raise ValueError(f"{who}: {pqc._sector.Dc} determinants (pair lists hold at most {MAX_DETERMINANTS})")


def check_thetas(thetas, rows, n_theta, who="pool_gradients"):
    n = int(np.prod(tuple(thetas.shape))) if hasattr(thetas, "shape") else int(np.size(thetas))
    if n != rows * n_theta:
        raise ValueError(f"{who}: thetas of shape {tuple(getattr(thetas, 'shape', (n,)))} for {rows} state(s) of "
                         f"{n_theta} parameters")


def gradients_from_coefficients(pqc, pool, thetas, c1, c2, c_stride):
    """[B, P]: the pool gradients of the states psi(thetas[b]) of ``pqc`` with the CAS coefficients of state b at
    ``c1`` + b ``c_stride``, ``c2`` + b ``c_stride`` (device tensors / views; doubles) -- one library call."""
    lib = _lib.load()
    eng = pqc._sector
    B = int(thetas.shape[0])
    pairs, tabs, op_first, sign = pool.device_tables(eng)
    psi = eng.state(thetas)
    key = ("pool", B)
    if key not in eng._work:
        n = lib.oovqe_pool_gradients_from_coefficients_work_size(eng.ncas, eng.na, eng.nb, B)
        eng._work[key] = torch.empty(int(n), dtype=F64, device=eng.device)
    out = torch.empty((B, pool.n_operators), dtype=F64, device=eng.device)
    i32 = torch.int32
    check(lib.oovqe_pool_gradients_from_coefficients_batch(
        dptr(psi), eng.ncas, *eng._tabs(), B, ctypes.c_void_p(c1.data_ptr()), ctypes.c_void_p(c2.data_ptr()),
        int(c_stride), tabs, dptr(pairs, i32), pool.n_gates, dptr(op_first, i32), dptr(sign, i32),
        pool.n_operators, dptr(eng._work[key]), dptr(out), stream_ptr()),
        "oovqe_pool_gradients_from_coefficients_batch")
    return out


# ---- the driver ---------------------------------------------------------------------------------------------------------
def _circuit(ncas, nelecas, gates):
    from .pqc import Parameterized_circuit
    return Parameterized_circuit(ncas, nelecas, None, ansatz=list(gates))


def swap_circuit(oo, pqc):
    """Give a one-geometry ``OO_pqc`` another circuit of the same active space: the plans made for the old one go."""
    if int(pqc.ncas) != int(oo.ncas) or int(pqc.nelecas) != int(oo.nelecas):
        raise ValueError("swap_circuit: a circuit of another active space")
    oo.pqc = pqc
    for k in ("_plans2", "_hess1_plans"):
        oo.__dict__.pop(k, None)
    hit = oo.__dict__.get("_stack1")
    if hit is not None:                  # (the one-geometry stack of full_optimization keeps its resident integrals)
        hit[1].set_circuit(pqc)


def _optimize_theta(oo, theta, max_iterations, gtol, **newton):
    """Newton on theta alone at fixed orbitals (``NewtonStep`` with ``circuit_gradient`` /
    ``circuit_circuit_hessian``) until the largest |dE/dtheta| is below ``gtol`` -> (theta, energy)."""
    from .newton_raphson import NewtonStep
    opt = NewtonStep(verbose=0, **newton)
    for _ in range(max_iterations):
        grad = oo.circuit_gradient(theta)
        if float(grad.abs().max().item()) < gtol:
            break
        new, _ = opt.damped_newton_step(oo.energy_from_parameters, (theta,), grad,
                                        oo.circuit_circuit_hessian(theta), defer_lowest=True)
        theta = new.reshape(theta.shape)
    return theta, oo.energy_from_parameters(theta).item()


def adapt_vqe(oo, pool, max_operators, grad_tol=1e-3, orbital_optimization=True, theta=None, max_iterations=50,
              conv_tol=1e-10, theta_gtol=1e-9, verbose=0, callback=None, **newton):
    """ADAPT-VQE on one geometry (``oo``: an ``OO_pqc``) or on a stack (``OO_pqc_batch``, ONE circuit for all its
    geometries -- the Berry loop and the overlaps need that).

    Each addition: the pool gradients at the current state; stop when their norm (for a stack: the largest over the
    geometries) is below ``grad_tol`` or ``max_operators`` were added; otherwise append the operator with the largest
    |g| (stack: the largest sum over the geometries of g^2; the same operator may be chosen again) with its parameter
    at 0 behind the circuit, keep the old parameters, and re-optimise through the existing drivers: one geometry --
    ``full_optimization`` (``orbital_optimization``) or Newton on theta alone until the largest |dE/dtheta| is below
    ``theta_gtol``; a stack -- ``set_circuit``, then lockstep
    ``damped_newton_step`` until the largest energy change falls below ``conv_tol`` (orbitals always on: that is the
    step the stack has).

    ``theta=None`` starts from the Hartree-Fock determinant (the circuit ``oo`` came with is replaced); otherwise the
    run continues from ``oo``'s circuit at ``theta`` ([n_theta], or [G, n_theta]).  ``**newton``: hyper-parameters of
    ``NewtonStep``; ``callback(n_added, oo, thetas, energy)`` is called after every addition and its re-optimisation.
    -> ``AdaptResult``."""
    from .batch import OO_pqc_batch
    from .newton_raphson import BatchedNewtonStep
    stack = isinstance(oo, OO_pqc_batch)
    check_pool(pool, oo.pqc, "adapt_vqe")
    if stack and not orbital_optimization:
        raise ValueError("adapt_vqe: a stack is re-optimised by lockstep Newton steps on circuit and orbitals together")
    ncas, nelecas, dev = pool.ncas, pool.nelecas, oo.device
    G = oo.G if stack else 1
    swap = oo.set_circuit if stack else (lambda pqc: swap_circuit(oo, pqc))
    if theta is None:
        gates, n_theta = [], 0
        thetas = torch.zeros((G, 0), dtype=F64, device=dev)
    else:
        gates = list(oo.pqc._gates)
        n_theta = int(np.prod(oo.pqc.theta_shape))
        check_thetas(theta, G, n_theta, "adapt_vqe")
        thetas = torch.as_tensor(theta).to(device=dev, dtype=F64).reshape(G, n_theta).clone()
    chosen, energies, norms, maxima, history = [], [], [], [], []

    def gradients():
        if gates:
            return oo.pool_gradients(thetas if stack else thetas[0], pool).reshape(G, -1)
        # the Hartree-Fock determinant as a circuit: any pool operator at angle 0
        swap(_circuit(ncas, nelecas, pool.operator_gates(0, 0)))
        zero = torch.zeros((G, 1), dtype=F64, device=dev)
        return oo.pool_gradients(zero if stack else zero[0], pool).reshape(G, -1)

    converged = False
    while True:
        g = gradients()
        norm = float(g.norm(dim=1).max().item())
        if chosen:                                   # (the state the last addition and its re-optimisation left)
            norms.append(norm)
            maxima.append(float(g.abs().max().item()))
        if verbose:
            print(f"adapt {len(chosen):3d}: pool-gradient norm {norm:.3e}, largest |g| {float(g.abs().max()):.3e}")
        if norm < grad_tol:
            converged = True
            break
        if len(chosen) >= max_operators:
            break
        k = int(torch.argmax((g * g).sum(dim=0)).item())         # (one geometry: the largest |g|)
        history.append(g if stack else g[0])
        chosen.append(k)
        gates = gates + pool.operator_gates(k, n_theta)
        n_theta += 1
        thetas = torch.cat((thetas, torch.zeros((G, 1), dtype=F64, device=dev)), dim=1).contiguous()
        swap(_circuit(ncas, nelecas, gates))
        if stack:
            opt = BatchedNewtonStep(verbose=0, **newton)
            e_old = oo.energy(thetas)
            for _ in range(max_iterations):
                thetas, e_new, _ = oo.damped_newton_step(thetas, opt, defer_lowest=True)
                change = float((e_new - e_old).abs().max().item())
                e_old = e_new
                if change < conv_tol:
                    break
            energies.append(e_old.clone())
        elif orbital_optimization:
            e_l, th_l = oo.full_optimization(thetas[0], max_iterations=max_iterations, conv_tol=conv_tol, verbose=None,
                                             **newton)[:2]
            thetas = th_l[-1].reshape(1, n_theta).contiguous()
            energies.append(float(e_l[-1]))
        else:
            th, e = _optimize_theta(oo, thetas[0], max_iterations, theta_gtol, **newton)
            thetas = th.reshape(1, n_theta).contiguous()
            energies.append(e)
        if callback is not None:
            callback(len(chosen), oo, thetas if stack else thetas[0], energies[-1])
    if not gates:
        raise ValueError("adapt_vqe: the pool gradient is below grad_tol at the Hartree-Fock determinant: nothing to "
                         "add")
    return AdaptResult(gates, chosen, thetas if stack else thetas[0], energies, norms, maxima, history, oo, converged)
