"""State-averaged OO-VQE for a geometry stack: several orthonormal initial states through ONE circuit U(theta) and one
set of orbitals, the weighted energy E_SA = sum_I w_I <Phi_I| U^T H U |Phi_I> minimised over (theta, kappa), the states
resolved at the end by diagonalising the small Hamiltonian inside the ensemble.

The CAS path is linear in the RDMs: fed with the ensemble-averaged RDM sets (``oovqe_ensemble_rdms``) the evaluation
of ``OO_pqc_batch`` gives the state-averaged energy, gradient and kappa blocks of the Hessian with ONE N^4 sweep per
stack, not one per state.  The front end is csrc/ensemble.hip: the circuit, its tangents and second tangents from
initial vectors that are superpositions, the weighted RDM sets, the theta-theta block.

``singlet_states`` and ``check_ensemble`` are host-only: they need no device.  Dense-register circuits only (at most 10
qubits); there is no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _lib, excitations as X, ops
from ._lib import check, dptr, stream_ptr

F64 = torch.float64
MAX_STATES = 4
MAX_QUBITS = 10


# ---- host-only helpers ----------------------------------------------------------------------------------------------
def _apply_epq(v, p, q, n):
    """E_pq v on the 2^n register, E_pq = a+_{2p} a_{2q} + a+_{2p+1} a_{2q+1}: Jordan-Wigner with spin orbital j on
    wire j = bit n-1-j, the sign of the RDM kernels (parity of the occupied modes strictly between)."""
    x = np.arange(1 << n, dtype=np.int64)
    out = np.zeros_like(v)
    for sp in (0, 1):
        bP, bQ = 1 << (n - 1 - (2 * p + sp)), 1 << (n - 1 - (2 * q + sp))
        if p == q:
            out += np.where(x & bP, v, 0.0)
            continue
        hi, lo = max(bP, bQ), min(bP, bQ)
        between = (hi - 1) & ~((lo << 1) - 1)
        par = np.zeros(1 << n, dtype=np.int64)
        for i in range(n):
            par += ((x & between) >> i) & 1
        sel = ((x & bP) != 0) & ((x & bQ) == 0)
        out += np.where(sel, np.where(par & 1, -1.0, 1.0) * v[x ^ (bP | bQ)], 0.0)
    return out


def singlet_states(ncas, nelecas, nstates=2):
    """[nstates, 2^(2 ncas)] orthonormal singlets of CAS(nelecas, ncas) to start an ensemble from: state 0 the
    Hartree-Fock determinant of ``excitations.hf_state``; state 1 the open-shell singlet E_{lumo,homo} |HF> / sqrt 2
    (defined through the operator, which fixes its sign); state 2 the determinant with the HOMO pair moved to the
    LUMO."""
    if nelecas % 2 or nelecas < 2 or nelecas > 2 * ncas - 2:
        raise ValueError(f"singlet_states: CAS({nelecas}e, {ncas}o) has no closed-shell HF determinant with a HOMO and "
                         "a LUMO inside the active space")
    if not 1 <= nstates <= 3:
        raise ValueError(f"singlet_states: nstates = {nstates} (1 .. 3)")
    n = 2 * ncas
    occ = X.hf_state(nelecas, n)
    homo, lumo = nelecas // 2 - 1, nelecas // 2
    out = np.zeros((nstates, 1 << n))
    out[0, X.basis_index(occ)] = 1.0
    if nstates > 1:
        out[1] = _apply_epq(out[0], lumo, homo, n) / np.sqrt(2.0)
    if nstates > 2:
        occ2 = occ.copy()
        occ2[2 * homo:2 * homo + 2] = 0
        occ2[2 * lumo:2 * lumo + 2] = 1
        out[2, X.basis_index(occ2)] = 1.0
    return out


def check_ensemble(states, weights, ncas, nelecas):
    """Validate an ensemble -> (states [S, D] float64, weights [S] float64).  ``states``: real, [S, 2^(2 ncas)],
    1 <= S <= 4, orthonormal to 1e-12, every one wholly in the (N_alpha, N_beta) sector of the HF determinant (the CAS
    path assumes that electron count); ``weights``: >= 0, summing to 1 within 1e-12 (None: equal weights).  Raises
    ValueError naming what is wrong."""
    states = np.asarray(states)
    if np.iscomplexobj(states):
        raise ValueError("check_ensemble: the states must be real")
    states = np.array(states, dtype=np.float64)
    n = 2 * ncas
    if states.ndim != 2 or states.shape[1] != 1 << n:
        raise ValueError(f"check_ensemble: states of shape {states.shape}, expected [S, {1 << n}] for {n} qubits")
    S = states.shape[0]
    if not 1 <= S <= MAX_STATES:
        raise ValueError(f"check_ensemble: {S} states (1 .. {MAX_STATES})")
    gram = states @ states.T
    dev = np.abs(gram - np.eye(S)).max()
    if not dev <= 1e-12:
        raise ValueError(f"check_ensemble: the states are not orthonormal (largest deviation of the Gram matrix "
                         f"{dev:.3g}, limit 1e-12)")
    x = np.arange(1 << n, dtype=np.int64)
    alpha = sum((x >> (n - 1 - 2 * p)) & 1 for p in range(ncas))
    beta = sum((x >> (n - 2 - 2 * p)) & 1 for p in range(ncas))
    occ = X.hf_state(nelecas, n)
    na, nb = int(occ[0::2].sum()), int(occ[1::2].sum())
    outside = np.abs(states[:, (alpha != na) | (beta != nb)])
    if outside.size and outside.max() != 0.0:
        bad = int(np.argmax(outside.max(axis=1)))
        raise ValueError(f"check_ensemble: state {bad} has weight outside the (N_alpha, N_beta) = ({na}, {nb}) sector "
                         "of the HF determinant")
    if weights is None:
        weights = np.full(S, 1.0 / S)
    weights = np.array(weights, dtype=np.float64).reshape(-1)
    if weights.shape[0] != S:
        raise ValueError(f"check_ensemble: {weights.shape[0]} weights for {S} states")
    if not (weights >= 0.0).all():
        raise ValueError(f"check_ensemble: negative weight {weights.min():.3g}")
    if not abs(weights.sum() - 1.0) <= 1e-12:
        raise ValueError(f"check_ensemble: the weights sum to {weights.sum():.15g}, not to 1 (within 1e-12)")
    return states, weights


# ---- the ensemble on the device -------------------------------------------------------------------------------------
class StateEnsemble:
    """The initial states and weights of a state-averaged calculation, validated (``check_ensemble``) and resident on
    the device: ``psi0`` [S, D], ``weights`` [S].  ``states`` None: ``singlet_states(ncas, nelecas, nstates)``."""

    def __init__(self, pqc, states=None, weights=None, nstates=2):
        if getattr(pqc, "_use_sector", False) or pqc.n_qubits > MAX_QUBITS:
            raise NotImplementedError("StateEnsemble covers dense-register circuits; circuits in the sector engine "
                                      f"(more than {MAX_QUBITS} qubits) are not implemented")
        if states is None:
            states = singlet_states(pqc.ncas, pqc.nelecas, nstates)
        states, weights = check_ensemble(states, weights, pqc.ncas, pqc.nelecas)
        self.pqc = pqc
        self.nstates = int(states.shape[0])
        self.states_host, self.weights_host = states, weights
        self.device = pqc.device
        self.psi0 = ops.as_device(states, self.device)
        self.weights = ops.as_device(weights, self.device)


class SA_OO_pqc_batch:
    """State-averaged OO-VQE on an existing ``OO_pqc_batch``: the batch's resident integrals, orbitals, kappa tables
    and CAS evaluation are used as they are (no integral is copied or read again) and the wrapped batch keeps working
    as before.  Every method takes ``thetas`` [G, n_theta], one parameter set per geometry."""

    def __init__(self, batch, ensemble):
        if ensemble.pqc is not batch.pqc:
            raise ValueError("SA_OO_pqc_batch: the ensemble was made for another circuit than the batch's")
        self.batch, self.ensemble = batch, ensemble
        self.lib, self.device = batch.lib, batch.device
        self.G, self.S = batch.G, ensemble.nstates
        self._vecs = {}

    # ---- shapes ------------------------------------------------------------------------------------------------------
    @property
    def n_theta(self):
        return self.batch.n_theta

    @property
    def n_kappa(self):
        return self.batch.n_kappa

    def _layout(self, nrdm):
        """The packed rows of the batch's CAS path fed with ``nrdm`` ensemble RDM sets."""
        return ops.PackedLayout.for_rdm_sets(nrdm, self.n_kappa, self.batch.ncas)

    def _thetas(self, thetas, who):
        nt = self.n_theta
        shape = tuple(thetas.shape) if hasattr(thetas, "shape") else tuple(np.shape(thetas))
        if shape != (self.G, nt) and not (self.G == 1 and shape == (nt,)):
            raise ValueError(f"SA_OO_pqc_batch.{who}: thetas of shape {shape}, expected ({self.G}, {nt})")
        return ops.as_device(thetas, self.device).reshape(self.G, nt)

    # ---- the three library calls ---------------------------------------------------------------------------------------
    def _states(self, thetas, pairs_dev):
        """vecs [G, S, 1 + n_theta + n_pairs, D] (``oovqe_ensemble_states``), in a buffer kept per shape and stream."""
        pqc, nt = self.batch.pqc, self.n_theta
        n_pairs = 0 if pairs_dev is None else int(pairs_dev.shape[0])
        key = (nt, n_pairs, torch.cuda.current_stream().cuda_stream)
        if key not in self._vecs:
            size = int(self.lib.oovqe_ensemble_work_size(nt, pqc.n_qubits, self.S, n_pairs, self.G))
            if size < 0:
                check(size, "oovqe_ensemble_work_size")
            self._vecs[key] = torch.empty(size, dtype=F64, device=self.device)
        vecs = self._vecs[key]
        check(self.lib.oovqe_ensemble_states(
            dptr(thetas), nt, dptr(pqc._gates_dev, torch.uint8), pqc._n_gates, pqc.n_qubits, dptr(self.ensemble.psi0),
            self.S, None if pairs_dev is None else dptr(pairs_dev, torch.int32), n_pairs, self.G, dptr(vecs),
            stream_ptr()), "oovqe_ensemble_states")
        return vecs.view(self.G, self.S, 1 + nt + n_pairs, 1 << pqc.n_qubits)

    def _rdms(self, vecs, n_tan, transition):
        a, G, S = self.batch.ncas, self.G, self.S
        g1 = torch.empty((G, 1 + n_tan, a, a), dtype=F64, device=self.device)
        g2 = torch.empty((G, 1 + n_tan, a, a, a, a), dtype=F64, device=self.device)
        t1 = torch.empty((G, S, S, a, a), dtype=F64, device=self.device) if transition else None
        t2 = torch.empty((G, S, S, a, a, a, a), dtype=F64, device=self.device) if transition else None
        check(self.lib.oovqe_ensemble_rdms(
            dptr(vecs), int(vecs.shape[2]), dptr(self.ensemble.weights), 2 * a, a, S, n_tan, G, dptr(g1), dptr(g2),
            dptr(t1), dptr(t2), stream_ptr()), "oovqe_ensemble_rdms")
        return g1, g2, t1, t2

    # ---- RDMs and the Hamiltonian inside the ensemble -----------------------------------------------------------------
    def rdms(self, thetas, derivatives=False, transition=False):
        """The ensemble RDM sets gamma [G, nset, a, a], Gamma [G, nset, a, a, a, a] (set 0 = sum_I w_I RDM(psi_I); with
        ``derivatives`` sets k = 1 .. n_theta = d/dtheta_k); with ``transition`` also the state and transition RDMs
        [G, S, S, a, a], [G, S, S, a, a, a, a], [I][J] = T(psi_I, psi_J)."""
        thetas = self._thetas(thetas, "rdms")
        g1, g2, t1, t2 = self._rdms(self._states(thetas, None), self.n_theta if derivatives else 0, transition)
        return (g1, g2, t1, t2) if transition else (g1, g2)

    def hamiltonian(self, thetas):
        """[G, S, S]: H_IJ = c0 delta_IJ + c1 . gamma^IJ + c2 . Gamma^IJ at the batch's current orbitals, symmetrised;
        the coefficients come from one CAS evaluation of the stack (off the diagonal the nuclear repulsion and the
        core energy drop out: the states are orthonormal)."""
        thetas = self._thetas(thetas, "hamiltonian")
        g1, g2, t1, t2 = self.rdms(thetas, transition=True)
        out, _, _ = self.batch._cas_batch(g1, g2, self.G)
        L = self._layout(1)
        c1 = out[:, L.c1].reshape(self.G, 1, 1, -1)
        c2 = out[:, L.c2].reshape(self.G, 1, 1, -1)
        H = (t1.reshape(self.G, self.S, self.S, -1) * c1).sum(dim=3) \
            + (t2.reshape(self.G, self.S, self.S, -1) * c2).sum(dim=3)
        H = 0.5 * (H + H.transpose(1, 2))
        eye = torch.eye(self.S, dtype=F64, device=self.device)
        return H + out[:, L.c0, None, None] * eye

    def state_energies(self, thetas):
        """[G, S]: <psi_I| H |psi_I>, the diagonal of ``hamiltonian``."""
        return torch.diagonal(self.hamiltonian(thetas), dim1=1, dim2=2)

    def resolve(self, thetas):
        """(E [G, S] ascending, U [G, S, S]): the eigen-decomposition of ``hamiltonian`` -- the states of the ensemble
        resolved, column k of U[g] the k-th state in the basis of the circuit states, its largest component positive.
        G x S x S numbers, diagonalised on the host once at the end; host arrays."""
        H = self.hamiltonian(thetas).cpu().numpy()
        E, U = np.linalg.eigh(H)
        for g in range(U.shape[0]):
            for k in range(U.shape[2]):
                if U[g, np.argmax(np.abs(U[g, :, k])), k] < 0.0:
                    U[g, :, k] = -U[g, :, k]
        return E, U

    # ---- energy, gradient, Hessian ------------------------------------------------------------------------------------
    def _energy_at(self, thetas, mo_coeff):
        g1, g2 = self.rdms(thetas)
        return self.batch._cas_batch(g1, g2, self.G, mo_coeff=mo_coeff)[0][:, ops.PackedLayout.E]

    def energy(self, thetas, kappas=None):
        """[G]: E_SA at the batch's orbitals, or (``kappas`` [G, n_kappa]) at mo_coeff[g] expm(-K(kappa[g]))."""
        thetas = self._thetas(thetas, "energy")
        return self._energy_at(thetas, None if kappas is None else self.batch.rotated_mo_coeff(kappas))

    def energy_and_gradient(self, thetas):
        """[G, 1 + n_theta + n_kappa]: column 0 = E_SA, then dE_SA/dtheta, then dE_SA/dkappa."""
        thetas = self._thetas(thetas, "energy_and_gradient")
        g1, g2 = self.rdms(thetas, derivatives=True)
        out, _, _ = self.batch._cas_batch(g1, g2, self.G)
        return out[:, self._layout(1 + self.n_theta).energy_and_gradient]

    def energy_gradient_hessian(self, thetas):
        """(E_SA [G], gradient [G, n], Hessian [G, n, n]), n = n_theta + n_kappa, in the block layout of
        ``OO_pqc_batch.energy_gradient_hessian``: [[tt, (kt)^T], [kt, kk]]."""
        thetas = self._thetas(thetas, "energy_gradient_hessian")
        a, nt = self.batch.ncas, self.n_theta
        pairs_dev, _, _ = ops._hessian_pair_tables(nt, self.device)
        vecs = self._states(thetas, pairs_dev)
        gamma, Gamma, _, _ = self._rdms(vecs, nt, False)

        def theta_theta(out, c12, c_stride):
            L = self._layout(1 + nt)
            Htt = torch.empty((self.G, nt, nt), dtype=F64, device=self.device)
            check(self.lib.oovqe_ensemble_circuit_hessian_batch(
                dptr(vecs), dptr(self.ensemble.weights), 2 * a, a, self.S, nt, dptr(pairs_dev, torch.int32),
                int(pairs_dev.shape[0]), self.G, ctypes.c_void_p(out[:, L.c1].data_ptr()),
                ctypes.c_void_p(out[:, L.c2].data_ptr()), int(c_stride), dptr(Htt), stream_ptr()),
                "oovqe_ensemble_circuit_hessian_batch")
            return Htt

        return self.batch._hessian_from_rdm_sets(gamma, Gamma, theta_theta)

    # ---- optimisation ---------------------------------------------------------------------------------------------------
    def damped_newton_step(self, thetas, opt=None):
        """One damped Newton step on (theta, kappa) of every geometry in lockstep (``OO_pqc_batch._lockstep_step``
        driven stage by stage): gradient + Hessian of E_SA, the G directions, a line search whose trials evaluate the
        ensemble energy of all geometries at once.  The accepted orbitals are adopted by the wrapped batch.
        -> (new thetas [G, n_theta], E_SA at the new parameters [G], lowest Hessian eigenvalues [G])."""
        new_thetas, energies, low = self.batch._lockstep_step(self._thetas(thetas, "damped_newton_step"), opt,
                                                              self._energy_at, self.energy_gradient_hessian)
        return new_thetas, energies, low.checked()

    def full_optimization(self, thetas, max_iterations=50, conv_tol=1e-10):
        """Damped Newton steps on all geometries in lockstep until every geometry's last energy change is below
        ``conv_tol`` (or ``max_iterations`` steps) -> (energies [n_iter + 1, G] (host), thetas [G, n_theta])."""
        thetas = self._thetas(thetas, "full_optimization")
        energies = [self.energy(thetas).cpu().numpy()]
        for _ in range(int(max_iterations)):
            thetas, e, _ = self.damped_newton_step(thetas)
            energies.append(e.cpu().numpy())
            if np.abs(energies[-1] - energies[-2]).max() < conv_tol:
                break
        return np.stack(energies), thetas

    # ---- nuclear gradient -----------------------------------------------------------------------------------------------
    def nuclear_gradient(self, thetas, index=None, chunk=None):
        """dE_SA/dR of every geometry -> [G', natm, 3] (device, Hartree / Bohr) at fixed ``theta`` and fixed
        ``oao_mo_coeff``: ``OO_pqc_batch.nuclear_gradient`` with the ensemble RDMs in place of the circuit's."""
        b = self.batch
        rows = b._gradient_rows(index, "SA_OO_pqc_batch.nuclear_gradient")
        b._refuse_large_ncas("SA_OO_pqc_batch.nuclear_gradient")
        thetas = self._thetas(thetas, "nuclear_gradient")
        g1, g2 = self.rdms(thetas)
        return b._nuclear_gradient_from_rdms(g1[:, 0], g2[:, 0], rows, chunk)
