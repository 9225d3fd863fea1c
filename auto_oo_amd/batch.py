"""Batched evaluation over molecular geometries (the Berry-phase-loop batch of the north star).

The reference evaluates one geometry at a time (examples/Tutorial_Berry_phase.ipynb builds a new
``OO_pqc`` per point).  At cc-pVDZ size one evaluation is only ~27 MB of HBM traffic, far too
little to fill an MI355X, so ``OO_pqc_batch`` stacks the per-geometry tensors of G ``OO_pqc``-like
problems (same basis size, same active space, same circuit) and evaluates all of them with ONE
call of ``oovqe_oo_eval_batch`` -- 5 kernel launches in which the geometry index is a grid
dimension.  Per geometry the arithmetic is exactly that of ``OO_pqc.energy_and_gradient``.

Circuits whose state lives in the (N_alpha, N_beta)-sector engine (more than 10 qubits: kUpCCD CAS(8e,8o), GateFabric
CAS(6e,6o), ...) take the same entry points (round 5): states, RDMs and derivative RDMs of ALL geometries from the
sector kernels with the geometry as their batch index, the CAS path of all geometries in one ``oovqe_cas_eval_batch``
call, the orbital Hessians in one ``oovqe_orbital_hessian_batch`` call, directions and line search in lockstep; only
the stages that take ONE set of CAS coefficients per call (the reverse sweep's operator, the theta-theta block) run
geometry by geometry.
"""
import ctypes
import time
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, excitations as X, gto as GTO, nucgrad, ops, scf
from ._lib import check, dptr, stream_ptr
from .gaussian import rhf
from .moldata import Moldata
from .oo_energy import mo_ao_to_mo_oao, non_redundant_indices

F64 = torch.float64

CASCIGradients = namedtuple("CASCIGradients", "energies ci gradients")
CASCICouplings = namedtuple("CASCICouplings", "energies ci gradients couplings ci_term orbital_term")
CASCIRelaxedGradients = namedtuple("CASCIRelaxedGradients",
                                   "energies ci gradients fixed_orbital z_info charge_gradients")


def _host_point_charges(basis, coords, point_charges):
    """``point_charges = (q, xyz in Angstrom)`` of ``from_geometries`` / ``set_geometries`` -> host arrays ([G, M],
    [G, M, 3] in Angstrom) checked against the number of geometries in ``coords``, or None.  Host work only."""
    if point_charges is None:
        return None
    if not isinstance(point_charges, (tuple, list)) or len(point_charges) != 2:
        raise ValueError("point_charges must be a pair (q, xyz): charges [G, M] or [M], positions [G, M, 3] or [M, 3] "
                         "in Angstrom")
    if isinstance(coords, torch.Tensor) and coords.is_cuda:
        G = 1 if coords.dim() == 2 else int(coords.shape[0])
    else:
        G = int(basis.coordinates(coords).shape[0])
    return GTO.point_charges_host(G, point_charges[0], point_charges[1])


# ---- shared steps of the stack properties; plain functions of values -----------------------------
def stack_rows(G, index):
    """``index`` of a property method (None: all; one row; a sequence of rows) -> the list of rows of a stack of ``G``
    geometries, ValueError for a row outside it."""
    if index is None:
        return list(range(G))
    rows = [int(i) for i in np.atleast_1d(index)]
    if any(not 0 <= r < G for r in rows):
        raise ValueError(f"index must hold rows in 0..{G - 1}")
    return rows


def rows_selector(rows, device=None):
    """What takes the ``rows`` out of a stacked tensor: consecutive rows -> a slice (a view: no copy of the integrals),
    anything else -> an index tensor on ``device``."""
    if rows == list(range(rows[0], rows[0] + len(rows))):
        return slice(rows[0], rows[0] + len(rows))
    return torch.as_tensor(rows, device=device)


def pair_matrix(values, R, sign=1):
    """The values of the sets of ``R`` states -> the matrix [c, R, R, ...] over the states.  ``sign = 1``: ``values``
    [c, R + P, ...], the R state values (the diagonal) and then those of the P pairs (I, J), I > J, in the order of
    ``nucgrad.state_pairs``, each stored to (I, J) and (J, I): symmetric exactly.  ``sign = -1``: ``values`` [c, P, ...],
    the pairs alone, stored to (I, J) and negated to (J, I): antisymmetric exactly, the diagonal exactly zero."""
    R, states = int(R), (int(R) if sign > 0 else 0)
    pairs = nucgrad.state_pairs(R)
    P = int(values.shape[1]) - states
    if sign not in (1, -1) or P != len(pairs):
        raise ValueError(f"values of shape {tuple(values.shape)} for {R} states and sign {sign}")
    mat = torch.empty((int(values.shape[0]), R, R) + tuple(values.shape[2:]), dtype=values.dtype, device=values.device)
    k = torch.arange(R, device=values.device)
    mat[:, k, k] = values[:, :R] if sign > 0 else 0.0
    if P:
        ii = torch.as_tensor([p[0] for p in pairs], dtype=torch.long, device=values.device)
        jj = torch.as_tensor([p[1] for p in pairs], dtype=torch.long, device=values.device)
        mat[:, ii, jj] = values[:, states:]
        mat[:, jj, ii] = values[:, states:] if sign > 0 else -values[:, states:]
    return mat


def check_small_gap(small_gap):
    """The ``small_gap`` argument of the methods that divide by a gap."""
    if small_gap not in ("raise", "nan"):
        raise ValueError(f"small_gap = {small_gap!r} ('raise' or 'nan')")


# what the two steps of the CASCI gradient methods hand each other: the rows asked for; energies [G, R] and ci [G, R, Dc]
# of the WHOLE stack; the RDMs [G, n, ...] of the n vectors (states, then the +, then the - polarisation vectors of
# ``pairs``) and the generalised Fock matrices [G, R + P, N, N] of the sets; ``extra``: the number of density sets the
# caller adds to the pass
CASCISets = namedtuple("CASCISets", "rows energies ci nroots pairs extra gamma Gamma fock")


class OO_pqc_batch:
    def __init__(self, pqc, mols, ncas, nelecas, oao_mo_coeffs=None, freeze_active=False):
        """
        Args:
            pqc: Parameterized_circuit shared by all geometries
            mols: sequence of Moldata (same nao, same electron count)
            ncas, nelecas: active space
            oao_mo_coeffs: sequence of [N,N] OAO->MO coefficients (default: from mol.hf.mo_coeff)
            freeze_active: freeze active-active rotations (oo_energy.py:139-140)
        """
        if len(mols) < 1:
            raise ValueError("need at least one geometry")
        for m in mols:
            if m.nao != mols[0].nao or m.nelectron != mols[0].nelectron:
                raise ValueError("all geometries of a batch must share nao and the electron count")
        self._allocate(pqc, len(mols), mols[0].nao, mols[0].nelectron, ncas, nelecas, freeze_active)
        nuc_host = np.empty(self.G)
        for g, m in enumerate(mols):
            self.int2e_ao[g].copy_(ops.as_device(m.int2e_ao, self.device))
            self.int1e_ao[g].copy_(ops.as_device(m.int1e_ao, self.device))
            self.oao_coeff[g].copy_(ops.as_device(m.oao_coeff, self.device))
            if oao_mo_coeffs is None:
                m.run_rhf()
                c = mo_ao_to_mo_oao(m.hf.mo_coeff, m.overlap)
            else:
                c = oao_mo_coeffs[g]
            self.set_oao_mo_coeff(g, c)
            nuc_host[g] = m.nuc
        self.nuc.copy_(torch.as_tensor(nuc_host))
        # exact p<->q / r<->s symmetry of every geometry's integrals (true for PySCF's int2e), verified
        # bit for bit per geometry, and the packed resident copy the batched N^4 pass streams: ONE pass over the
        # stack (oovqe_eri_ingest).  The batch runs on the flags ALL its geometries share.  int2e_ao must
        # not be modified in place afterwards (set_molecule / reverify_integrals are the ways in).
        self._ingest()

    def _allocate(self, pqc, G, nao, nelectron, ncas, nelecas, freeze_active):
        """Tables and (uninitialised) per-geometry tensors of a batch of G geometries."""
        self.lib = _lib.load()
        self.device = _lib.require_device()
        self.pqc = pqc
        self.G = int(G)
        if self.G < 1:
            raise ValueError("need at least one geometry")
        self.nao = int(nao)
        self.nelectron = int(nelectron)
        self.ncas, self.nelecas = ncas, nelecas
        self.occ_idx, self.act_idx, self.virt_idx = Moldata.get_active_space_idx(
            SimpleNamespace(nelectron=int(nelectron), nao=self.nao), ncas, nelecas)
        self._n_occ = len(self.occ_idx)
        self.params_idx = non_redundant_indices(self.occ_idx, self.act_idx, self.virt_idx,
                                                freeze_active)
        self.n_kappa = len(self.params_idx)
        rows, cols = X.tril_tables(self.nao, self.params_idx)
        self._kap_row = torch.as_tensor(rows).to(self.device)
        self._kap_col = torch.as_tensor(cols).to(self.device)
        self.n_theta = int(np.prod(pqc.theta_shape))

        N = self.nao
        self.int2e_ao = torch.empty((self.G, N, N, N, N), dtype=F64, device=self.device)
        self.int1e_ao = torch.empty((self.G, N, N), dtype=F64, device=self.device)
        self.oao_coeff = torch.empty((self.G, N, N), dtype=F64, device=self.device)
        self.oao_mo_coeff = torch.empty((self.G, N, N), dtype=F64, device=self.device)
        self.mo_coeff = torch.empty((self.G, N, N), dtype=F64, device=self.device)
        self.nuc = torch.empty(self.G, dtype=F64, device=self.device)
        self._eri_packed = None
        self._plans = {}
        self._flat0 = None
        self._trial_orbitals = None
        self._step_args = None
        self._all_pd_last_step = False
        self.step_by_calls = False
        self.basis = None
        self.coords_bohr = None
        self.charge_q = None            # point charges of an embedded batch [G, M] and
        self.charge_xyz_bohr = None     # their positions [G, M, 3] in Bohr (from_geometries(point_charges=...))
        self._grad_dm2 = None

    # ---- integrals made on the device (auto_oo_amd/gto.py) ----------------------------------------------------------
    @classmethod
    def from_geometries(cls, pqc, basis, coords, ncas, nelecas, oao_mo_coeffs=None, freeze_active=False,
                        point_charges=None):
        """A batch whose AO integrals are computed on the device (``gto.integrals_batch``) instead of being copied
        from host-built molecules.

        Args:
            pqc: Parameterized_circuit shared by all geometries
            basis: gto.GTOBasis of the molecule
            coords: [G, natm, 3] in Angstrom, or a list of geometries as ``Moldata_sto3g`` takes them
            ncas, nelecas: active space
            oao_mo_coeffs: [G][N, N] OAO->MO coefficients, or ``"rhf"``: RHF orbitals of every geometry from the device
                solver (``OO_pqc_batch.rhf``; no integral tensor is copied to the host, ``OovqeError`` names the
                geometries that did not converge).  Default (None): RHF orbitals from the host ``gaussian.rhf`` on
                the integrals copied back once -- slow for a large stack, prefer ``"rhf"``
            point_charges: ``(q, xyz)``: an environment of M fixed point charges per geometry, ``q`` [G, M] (or [M],
                shared by all geometries) in units of e and ``xyz`` [G, M, 3] (or [M, 3]) in Angstrom.  The batch is then
                the molecule EMBEDDED in these charges: ``int1e_ao`` holds the attraction of the electrons by them
                (``gto.point_charge_integrals_batch``) and ``nuc`` the energy of the nuclei in their field, so energies,
                orbital derivatives, ``rhf``, ``casci`` and the Newton steps are those of the polarised molecule;
                ``nuclear_gradient`` and its kin include the charges' pull on the atoms and ``point_charge_gradient``
                gives the derivative with respect to the charges' positions.  No charge-charge energy is added.  M is
                fixed for the life of the batch; the charges are kept in ``charge_q`` / ``charge_xyz_bohr`` (Bohr).
        """
        self = cls.__new__(cls)
        pc = _host_point_charges(basis, coords, point_charges)       # (checked before the device is touched)
        xyz = GTO.coords_to_device(basis, coords)
        self._allocate(pqc, int(xyz.shape[0]), basis.nao, basis.nelectron, ncas, nelecas, freeze_active)
        self.basis = basis
        if pc is not None:
            self.charge_q = torch.as_tensor(pc[0]).to(self.device)
            self.charge_xyz_bohr = torch.as_tensor(pc[1] / GTO.BOHR).to(self.device)
        self._write_integrals(xyz, None)
        if isinstance(oao_mo_coeffs, str):
            self._rhf_orbitals(oao_mo_coeffs, None)
            oao_mo_coeffs = ()
        elif oao_mo_coeffs is None:
            S, h, g = self.overlap.cpu().numpy(), self.int1e_ao.cpu().numpy(), self.int2e_ao.cpu().numpy()
            oao_mo_coeffs = [mo_ao_to_mo_oao(rhf(h[k], g[k], S[k], basis.nelectron // 2)[0], S[k])
                             for k in range(self.G)]
        for g_, c in enumerate(oao_mo_coeffs):
            self.oao_mo_coeff[g_].copy_(ops.as_device(c, self.device))
        self._ingest()
        self.refresh_mo_coeff()
        return self

    def _write_integrals(self, xyz_bohr, index):
        """Integrals, S^-1/2 and nuclear repulsion of the geometries ``xyz_bohr`` (device, Bohr) into the rows ``index``
        of the stack (None: all rows), written in place by the integral kernels: runs of consecutive rows take one
        call each."""
        if getattr(self, "overlap", None) is None:
            self.overlap = torch.empty((self.G, self.nao, self.nao), dtype=F64, device=self.device)
        rows = list(range(self.G)) if index is None else [int(i) for i in index]
        if len(rows) != int(xyz_bohr.shape[0]):
            raise ValueError(f"{int(xyz_bohr.shape[0])} geometries for {len(rows)} rows")
        if any(not 0 <= r < self.G for r in rows) or len(set(rows)) != len(rows):
            raise ValueError(f"index must hold distinct rows in 0..{self.G - 1}")
        # the coordinates stay with the batch (Bohr): nuclear_gradient differentiates with respect to them
        if self.coords_bohr is None:
            self.coords_bohr = torch.empty((self.G, self.basis.natm, 3), dtype=F64, device=self.device)
        if index is None:
            self.coords_bohr.copy_(xyz_bohr)
        else:
            self.coords_bohr[torch.as_tensor(rows, device=self.device)] = xyz_bohr
        infos = []
        k = 0
        while k < len(rows):
            e = k + 1
            while e < len(rows) and rows[e] == rows[e - 1] + 1:
                e += 1
            a, b = rows[k], rows[e - 1] + 1
            GTO.integrals_into(self.basis, xyz_bohr[k:e], self.overlap[a:b], self.int1e_ao[a:b], self.int2e_ao[a:b],
                               self.nuc[a:b])
            if self.charge_q is not None:
                # the embedded molecule: the electrons' attraction by the charges and the nuclei's energy in their field
                q, r = self.charge_q[a:b], self.charge_xyz_bohr[a:b]
                self.int1e_ao[a:b] += GTO.point_charge_integrals_into(self.basis, xyz_bohr[k:e], q, r)
                Z = self.basis.device_tables(self.device).charges
                dist = (xyz_bohr[k:e, :, None, :] - r[:, None, :, :]).norm(dim=-1)
                self.nuc[a:b] += (Z[None, :, None] * q[:, None, :] / dist).sum(dim=(1, 2))
            infos.append(GTO.sym_invsqrt_batch(self.overlap[a:b], out=self.oao_coeff[a:b])[1])
            k = e
        GTO.raise_if_dependent(torch.cat(infos), rows)

    def set_geometries(self, coords, index=None, oao_mo_coeffs=None, point_charges=None):
        """Move the batch (or its rows ``index``) to new geometries: ``int2e_ao``, ``int1e_ao``, ``oao_coeff`` and
        ``nuc`` are computed in place on the device, then the symmetry flags / packed copy are re-made (``_ingest``)
        and ``mo_coeff = S^-1/2 C_oao`` refreshed.  ``oao_mo_coeffs=None`` keeps the current orbitals (the tracking
        regime of a Berry-phase loop); ``"rhf"`` takes the RHF orbitals of the new geometries from the device solver
        (``OO_pqc_batch.rhf``; ``OovqeError`` names the geometries that did not converge); otherwise one [N, N] matrix
        per new geometry.  No integral tensor passes through the host.  ``point_charges``: ``(q, xyz)`` as for
        ``from_geometries``, one cloud per new geometry, for a batch that was built with point charges (ValueError
        otherwise, and for another M); None keeps the stored charges of those rows -- a frozen environment."""
        if self.basis is None:
            raise RuntimeError("set_geometries needs a batch made by OO_pqc_batch.from_geometries")
        if point_charges is not None and self.charge_q is None:
            raise ValueError("set_geometries: this batch was built without point charges (give them to "
                             "from_geometries: their number is fixed at construction)")
        pc = _host_point_charges(self.basis, coords, point_charges)
        if pc is not None and pc[0].shape[1] != int(self.charge_q.shape[1]):
            raise ValueError(f"set_geometries: {pc[0].shape[1]} point charges per geometry, the batch was built with "
                             f"{int(self.charge_q.shape[1])}")
        xyz = GTO.coords_to_device(self.basis, coords, self.device)
        rows = None if index is None else [int(i) for i in np.atleast_1d(index)]
        if pc is not None:
            if len(pc[0]) != (self.G if rows is None else len(rows)):
                raise ValueError(f"{len(pc[0])} clouds of point charges for {self.G if rows is None else len(rows)} rows")
            where = slice(None) if rows is None else torch.as_tensor(rows, device=self.device)
            self.charge_q[where] = torch.as_tensor(pc[0]).to(self.device)
            self.charge_xyz_bohr[where] = torch.as_tensor(pc[1] / GTO.BOHR).to(self.device)
        self._write_integrals(xyz, rows)
        if isinstance(oao_mo_coeffs, str):
            self._rhf_orbitals(oao_mo_coeffs, rows)
        elif oao_mo_coeffs is not None:
            targets = range(self.G) if rows is None else rows
            if len(oao_mo_coeffs) != len(targets):
                raise ValueError("one orbital matrix per new geometry")
            for g_, c in zip(targets, oao_mo_coeffs):
                self.oao_mo_coeff[g_].copy_(ops.as_device(c, self.device))
        if rows is not None and len(rows) == 1:
            self._ingest(rows[0])
        else:
            self._ingest()
        self.refresh_mo_coeff()

    # ---- starting orbitals made on the device (auto_oo_amd/scf.py) ---------------------------------------------------
    def rhf(self, index=None, **kw):
        """Closed-shell RHF of the batch's geometries (or its rows ``index``) on the batch's own device tensors
        (``scf.rhf_batch``; keywords ``conv_tol``, ``err_tol``, ``max_cycle``) -> ``scf.RHFResult`` with ``e_tot =
        e_elec + nuc``.  The batch is not changed.  Needs the overlap, so a batch made by ``from_geometries``."""
        if getattr(self, "overlap", None) is None:
            raise RuntimeError("OO_pqc_batch.rhf needs a batch made by OO_pqc_batch.from_geometries")
        scf.check_scope(self.nao, nelectron=self.nelectron)
        sel = rows_selector(stack_rows(self.G, index), self.device)
        res = scf.rhf_batch(self.int1e_ao[sel], self.int2e_ao[sel], self.overlap[sel], self.nelectron // 2,
                            oao_coeff=self.oao_coeff[sel], **kw)
        return res._replace(e_tot=res.e_elec + self.nuc[sel])

    # ---- forces (auto_oo_amd/nucgrad.py, csrc/gto_grad.hip) ----------------------------------------------------------
    def _moment_rows(self, index, who):
        """The rows ``index`` of a batch made by ``from_geometries`` (RuntimeError otherwise, under the name ``who``)."""
        if self.basis is None or self.coords_bohr is None:
            raise RuntimeError(f"{who} needs a batch made by OO_pqc_batch.from_geometries")
        return stack_rows(self.G, index)

    def _gradient_rows(self, index, who):
        rows = self._moment_rows(index, who)
        GTO.refuse_d_gradient(self.basis)         # before anything is launched
        return rows

    def _point_charge_rows(self, index, who):
        rows = self._gradient_rows(index, who)
        if self.charge_q is None:
            raise RuntimeError(f"{who} needs a batch made by OO_pqc_batch.from_geometries(point_charges=...)")
        return rows

    def _charge_pull(self, sel, d1, nuc):
        """``gto.point_charge_gradient_into`` of the density ``d1`` at the rows ``sel`` (an index tensor) of an embedded
        batch -> (the charges' pull on the atoms [len(sel), natm, 3], the derivative with respect to the charges'
        positions [len(sel), M, 3]); ``nuc``: with the nuclei's term."""
        return GTO.point_charge_gradient_into(self.basis, self.coords_bohr[sel], self.charge_q[sel],
                                              self.charge_xyz_bohr[sel], d1, nuc)

    def _refuse_large_ncas(self, who, verb="covers"):
        if self.ncas > nucgrad.MAX_NCAS:
            raise NotImplementedError(f"{who} {verb} ncas <= {nucgrad.MAX_NCAS}")

    def _circuit_rdms(self, thetas, who, verb="covers", sector=False):
        """The RDMs gamma [G, a, a], Gamma [G, a, a, a, a] of the circuit states at ``thetas`` [G, n_theta], whole stack,
        as the evaluation path makes them (dense register: ``ops.circuit_rdms``; sector engine: the RDMs of
        ``_evaluate_sector``, served only with ``sector``: NotImplementedError otherwise)."""
        pqc = self.pqc
        in_sector = self._sector
        if in_sector and not sector:
            raise NotImplementedError(f"{who} covers dense-register circuits; circuits in the sector engine "
                                      "(more than 10 qubits) are not implemented")
        self._refuse_large_ncas(who, verb)
        thetas = ops.as_device(thetas, self.device).reshape(self.G, self.n_theta)
        if in_sector:
            return pqc._sector.rdms(pqc._sector.state(thetas))
        gamma, Gamma = ops.circuit_rdms(thetas, pqc._gates_dev, pqc._n_gates, pqc.n_qubits, self.ncas,
                                        pqc._init_index, tangents=False)
        return gamma[:, 0], Gamma[:, 0]

    def _rhf_density(self, result, index, rows):
        """``(result, index, rows) -> (result, D1)``: the ``scf.RHFResult`` of the rows (``self.rhf(index=index)``, which
        must converge, when none is given; ValueError for one of another number of geometries) and its closed-shell
        ``D1 = 2 C_o C_o^T`` [len(rows), N, N]."""
        if result is None:
            result = self.rhf(index=index)
            scf.raise_unless_converged(result.info, rows)
        if int(result.mo_coeff.shape[0]) != len(rows):
            raise ValueError(f"the RHF result holds {int(result.mo_coeff.shape[0])} geometries, {len(rows)} rows asked "
                             "for")
        return result, nucgrad.cas_ao_densities(result.mo_coeff, self.nelectron // 2, 0, want_d2=False)[0]

    def _dm2_buffer(self, n):
        """[n, N, N, N, N] for the AO two-particle density of a chunk: the size of ``int2e_ao`` per geometry, so it is
        made on first use and kept at the largest chunk asked for."""
        if self._grad_dm2 is None or int(self._grad_dm2.shape[0]) < n:
            self._grad_dm2 = torch.empty((n,) + (self.nao,) * 4, dtype=F64, device=self.device)
        return self._grad_dm2

    def nuclear_gradient(self, thetas, index=None, chunk=None):
        """dE/dR of every geometry -> [G, natm, 3] (device, Hartree / Bohr): the derivative of each geometry's
        ``energy_from_parameters(theta_g)`` with respect to its own nuclear coordinates at fixed ``theta_g`` and fixed
        ``oao_mo_coeff`` -- what central differences over ``set_geometries(..., oao_mo_coeffs=None)`` measure, exact at
        any parameters and orbitals, converged or not (the dependence of ``S^-1/2`` on the geometry is pulled back to
        the overlap, ``nucgrad.overlap_pullback``).

        Args:
            thetas: [G, n_theta], one parameter set per geometry of the batch
            index: rows of the batch to differentiate (default all); the result then has one entry per row asked for
            chunk: geometries per pass of the two-electron part (default all at once): the AO two-particle density
                is as large as ``int2e_ao`` and is kept for ``chunk`` geometries only

        A geometry's gradient has the same bits whatever ``index`` and ``chunk``.  Needs a batch made by
        ``from_geometries`` (RuntimeError otherwise).  Dense-register circuits only: a circuit in the sector engine
        (more than 10 qubits) raises NotImplementedError -- its RDMs would serve, that path has not been tested."""
        rows = self._gradient_rows(index, "nuclear_gradient")
        gamma, Gamma = self._circuit_rdms(thetas, "nuclear_gradient")
        return self._nuclear_gradient_from_rdms(gamma, Gamma, rows, chunk)

    def _nuclear_gradient_from_rdms(self, gamma, Gamma, rows, chunk):
        """``nuclear_gradient`` behind its RDMs: gamma [G, a, a], Gamma [G, a, a, a, a] of the whole stack (the
        circuit's, or those of an ensemble: ``ensemble.SA_OO_pqc_batch.nuclear_gradient``) -> [len(rows), natm, 3]."""
        _, _, fock = self._cas_batch(gamma[:, None], Gamma[:, None], self.G, want_fock=True)
        step = len(rows) if chunk is None else max(1, int(chunk))
        out = torch.empty((len(rows), self.basis.natm, 3), dtype=F64, device=self.device)
        for k in range(0, len(rows), step):
            sel = torch.as_tensor(rows[k:k + step], device=self.device)
            d1, d2 = nucgrad.cas_ao_densities(self.mo_coeff[sel], self._n_occ, self.ncas, gamma[sel], Gamma[sel],
                                              out=self._dm2_buffer(len(sel)))
            wq = nucgrad.overlap_pullback(self.overlap[sel], self.oao_mo_coeff[sel], fock[sel])
            out[k:k + step] = GTO.gradient_into(self.basis, self.coords_bohr[sel], d1, wq, d2, True)
            if self.charge_q is not None:
                out[k:k + step] += self._charge_pull(sel, d1, True)[0]
        return out

    def point_charge_gradient(self, thetas, index=None):
        """dE/dr_k of every geometry of an embedded batch -> [G', M, 3] (device, Hartree / Bohr): the derivative of
        ``energy_from_parameters(theta_g)`` with respect to the positions of the geometry's point charges at fixed
        parameters and orbitals; the force on a charge is its negative.  Only the operator's centre moves (the basis
        does not depend on the charges), so this is ``D1 . dV_ext/dr_k`` plus the nuclei's term, exact at any
        parameters.  ``index``, the scope and the errors are those of ``nuclear_gradient``; RuntimeError for a batch
        without point charges."""
        rows = self._point_charge_rows(index, "point_charge_gradient")
        gamma, Gamma = self._circuit_rdms(thetas, "point_charge_gradient")
        sel = torch.as_tensor(rows, device=self.device)
        d1 = nucgrad.cas_ao_densities(self.mo_coeff[sel], self._n_occ, self.ncas, gamma[sel], Gamma[sel],
                                      want_d2=False)[0]
        return self._charge_pull(sel, d1, True)[1]

    def rhf_point_charge_gradient(self, result=None, index=None):
        """dE_RHF/dr_k -> [G', M, 3] (device, Hartree / Bohr) of an embedded batch from a converged ``scf.RHFResult``
        of the rows ``index`` (``self.rhf(index=index)`` is run when none is given), as ``rhf_nuclear_gradient``."""
        rows = self._point_charge_rows(index, "rhf_point_charge_gradient")
        _, d1 = self._rhf_density(result, index, rows)
        return self._charge_pull(torch.as_tensor(rows, device=self.device), d1, True)[1]

    def casci_nuclear_gradients(self, nroots=2, fix_singlet=True, index=None, chunk=None, tol=1e-9, max_iter=200):
        """CASCI states of every geometry at its current orbitals (``casci``) with their state and interstate nuclear
        gradients -> ``CASCIGradients(energies [G', R], ci [G', R, Dc], gradients [G', R, R, natm, 3])`` on the device,
        Hartree / Bohr (G' = the rows asked for, R = ``nroots``).

        ``gradients[g, I, I]`` is dE_I/dR at fixed ``oao_mo_coeff`` -- exact, because the c_I are eigenvectors of the
        CAS Hamiltonian (Hellmann-Feynman for the CI coefficients; the dependence of ``S^-1/2`` on the geometry is
        pulled back to the overlap as in ``nuclear_gradient``).  ``gradients[g, I, J]``, I != J, is the interstate
        coupling ``h_IJ = c_I^T (dH/dR) c_J`` with both CI vectors held fixed, the pull-back through ``S^-1/2``
        included; it is symmetric in (I, J) exactly (one set is computed and stored to both places).  All R (R + 1) / 2
        elements come from ONE pass over the derivative integrals (``gto.gradient_sets_into``): the transition
        densities and Fock matrices are half-differences of those of ``(c_I +- c_J) / sqrt 2``, from which the
        core-only parts and the nuclear term drop out exactly.  ``nucgrad.branching_plane`` picks ``(G_jj - G_ii) / 2``
        and ``G_ij``, the two vectors that span the branching plane of a conical intersection.

        - The SIGN of an off-diagonal element is that of the product of the two CI vectors' signs as ``casci`` fixes
          them (largest |component| positive), as for the transition dipoles of ``casci_dipole_matrix``.
          ``overlaps.track_roots`` on the ``O`` of ``casci_overlaps`` gives the order and signs that are continuous along
          a path, ``overlaps.apply_tracking`` applies them to ``gradients``.
        - Within a degenerate pair of roots only the 2 x 2 block is defined (up to a rotation of the pair), not its
          split into elements.
        - ``G_IJ / (E_J - E_I)`` is the CI part of the derivative coupling only: ``casci_derivative_couplings`` adds the
          orbital-connection term ``<p|dq/dR>`` and returns the whole nonadiabatic coupling vector.

        Args:
            nroots, fix_singlet, tol, max_iter: as for ``casci`` (which raises when a solve does not converge)
            index: rows of the batch (default all); the result then has one entry per row asked for
            chunk: geometries per pass of the contraction (default all at once): the AO two-particle densities are kept
                for ``chunk`` geometries only, ``chunk (R (R + 1) / 2 + 2) N^4`` doubles

        The same bits whatever ``index`` and ``chunk``.  Works for any batch whatever its circuit (only orbitals and
        integrals are used).  Needs a batch made by ``from_geometries`` (RuntimeError otherwise); d shells and
        ``ncas > nucgrad.MAX_NCAS`` raise NotImplementedError, a CI problem out of scope ValueError
        (``ci.check_scope``)."""
        sets = self._casci_sets("casci_nuclear_gradients", nroots, fix_singlet, index, tol, max_iter)
        values, _ = self._casci_derivative_pass(sets, chunk)
        sel = torch.as_tensor(sets.rows, device=self.device)
        return CASCIGradients(sets.energies[sel], sets.ci[sel], pair_matrix(values, sets.nroots))

    def _casci_gradient_scope(self, who, nroots, index):
        """The rows ``index`` and the refusals the CASCI gradient methods share, in their order."""
        from . import ci
        rows = self._gradient_rows(index, who)
        self._refuse_large_ncas(who)
        ci.check_scope(self.ncas, self.nelecas, nroots)
        return rows

    def _casci_sets(self, who, nroots, fix_singlet, index, tol, max_iter, interstate=True, extra=0):
        """Step one of the CASCI gradient methods -> ``CASCISets``: the CASCI solve of the whole stack, then the RDMs of
        the R states and of the 2 P polarisation vectors of their pairs and the generalised Fock matrices of the R + P
        sets.  ``interstate=False`` leaves the pair sets out.  ``extra``: the number of further density sets the caller
        will add to the pass (they count towards ``gto.MAX_GRAD_SETS``)."""
        from . import ci
        rows = self._casci_gradient_scope(who, nroots, index)
        e, vecs = self.casci(nroots, fix_singlet, tol, max_iter)
        G, R, a, N = self.G, int(nroots), self.ncas, self.nao
        pairs = nucgrad.state_pairs(R) if interstate else []
        P = len(pairs)
        n, K = R + 2 * P, R + P
        if K + extra > GTO.MAX_GRAD_SETS:
            raise ValueError(f"{who}: {K + extra} density sets per geometry (1 .. {GTO.MAX_GRAD_SETS})")
        # RDMs and generalised Fock matrices of the R states and the 2 P polarisation vectors, whole stack
        stack = nucgrad.polarisation_vectors(vecs) if interstate else vecs
        gamma, Gamma = ci.sector_rdms(stack.reshape(G * n, -1), a, self.nelecas)
        gamma = gamma.reshape(G, n, a, a)
        Gamma = Gamma.reshape((G, n) + (a,) * 4)
        fock = torch.empty((G, n, N, N), dtype=F64, device=self.device)
        for s in range(n):      # (the CAS path takes the RDMs of set 0 for the Fock matrix: one call per vector)
            fock[:, s] = self._cas_batch(gamma[:, s:s + 1], Gamma[:, s:s + 1], G, want_fock=True)[2]
        fock = nucgrad.transition_sets(fock, R) if interstate else fock
        return CASCISets(rows, e, vecs, R, pairs, int(extra), gamma, Gamma, fock)

    def _casci_derivative_pass(self, sets, chunk, more_sets=None):
        """Step two: the chunked pass over the derivative integrals for the ``CASCISets`` of step one -> ``(values
        [len(rows), R + P + extra, natm, 3], charge_values)``: the nuclear gradients of the R states, the P interstate
        elements and the extra sets, the charges' pull on the atoms included for an embedded batch.

        ``more_sets(k0, sel, d1, d2, wq, out)`` provides ``sets.extra`` more density sets per geometry: it is given the
        fixed-orbital densities of the R states of the chunk ``sel = rows[k0:k0 + c]`` and the place ``out`` [c, extra,
        N, N, N, N] for their two-particle densities, and returns their (D1, WQ) [c, extra, N, N]; they ride in the same
        pass, as states, and ``charge_values`` [len(rows), extra, M, 3] is their ``point_charge_gradient`` (None without
        extra sets or point charges)."""
        rows, R, pairs, gamma, Gamma, fock = sets.rows, sets.nroots, sets.pairs, sets.gamma, sets.Gamma, sets.fock
        a, N, natm = self.ncas, self.nao, self.basis.natm
        P, X = len(pairs), sets.extra
        K = R + P
        values = torch.empty((len(rows), K + X, natm, 3), dtype=F64, device=self.device)
        charge_values = None
        if X and self.charge_q is not None:
            charge_values = torch.empty((len(rows), X, int(self.charge_q.shape[1]), 3), dtype=F64, device=self.device)
        step = len(rows) if chunk is None else max(1, int(chunk))
        for k0 in range(0, len(rows), step):
            sel = torch.as_tensor(rows[k0:k0 + step], device=self.device)
            c = len(sel)
            C = self.mo_coeff[sel]
            d1 = nucgrad.transition_sets(
                nucgrad.cas_ao_densities(C, self._n_occ, a, gamma[sel], Gamma[sel], want_d2=False)[0], R)
            buf = self._dm2_buffer(c * (K + X + 2))
            d2 = buf[:c * (K + X)].view((c, K + X) + (N,) * 4)
            tmp = buf[c * (K + X):c * (K + X + 2)]
            for s in range(R):
                t = nucgrad.cas_ao_densities(C, self._n_occ, a, gamma[sel, s], Gamma[sel, s], out=tmp)[1]
                d2[:, s].copy_(t)
            for p in range(P):      # the pair's + and - densities side by side, their half-difference in place
                pm = [R + p, R + P + p]
                t = nucgrad.cas_ao_densities(C, self._n_occ, a, gamma[sel][:, pm], Gamma[sel][:, pm], out=tmp)[1]
                d2[:, R + p].copy_(t[:, 0].sub_(t[:, 1]).mul_(0.5))
            wq = nucgrad.overlap_pullback(self.overlap[sel], self.oao_mo_coeff[sel], fock[sel])
            if more_sets is not None:
                more = more_sets(k0, sel, d1[:, :R], d2[:, :R], wq[:, :R], d2[:, K:])
                d1, wq = torch.cat((d1, more[0]), dim=1), torch.cat((wq, more[1]), dim=1)
            val = GTO.gradient_sets_into(self.basis, self.coords_bohr[sel], d1, wq, d2,
                                         [True] * R + [False] * P + [True] * X)
            if self.charge_q is not None:
                # the charges' pull on the atoms, one pass per set: with the nuclei's term for a state (or an extra set),
                # without it for a transition density
                for s in range(K + X):
                    pull = self._charge_pull(sel, d1[:, s], s < R or s >= K)
                    val[:, s] += pull[0]
                    if s >= K:
                        charge_values[k0:k0 + c, s - K] = pull[1]
            values[k0:k0 + c] = val
        return values, charge_values

    def casci_derivative_couplings(self, nroots=2, fix_singlet=True, index=None, chunk=None, tol=1e-9, max_iter=200,
                                   min_gap=1e-6, small_gap="raise"):
        """CASCI states of every geometry at its current orbitals with their nonadiabatic (derivative) coupling vectors
        ``d_IJ^A = <Psi_I | d Psi_J / dR_A>`` -> ``CASCICouplings(energies [G', R], ci [G', R, Dc], gradients, couplings,
        ci_term, orbital_term)`` on the device; the last four are [G', R, R, natm, 3], ``gradients`` in Hartree / Bohr
        and exactly what ``casci_nuclear_gradients`` returns for the same roots, the others in 1 / Bohr:

            couplings = ci_term + orbital_term,   ci_term_IJ = G_IJ / (E_J - E_I),
            orbital_term_IJ^A = sum_pq gamma^IJ_pq <phi_p | d phi_q / dR_A> = Da . T^A + WQc . dS/dR_A

        with the transition 1-RDM ``gamma^IJ_pq = <c_I|E_pq|c_J>`` (``ci.transition_rdm1``), of which only the
        antisymmetric part ``a = (gamma^IJ - gamma^IJ^T) / 2`` enters (``<phi_p|d phi_q>`` is antisymmetric; the core
        contributes nothing), ``Da = C_act a C_act^T`` contracted with the derivative of the ket of the AO overlap
        (``gto.overlap_connection_into``), and ``WQc`` the pull-back of the dependence of ``S^-1/2`` on the geometry
        (``nucgrad.connection_pullback``) contracted with ``dS/dR`` (``gto.gradient_sets_into``).  Exact for the wave
        functions the batch defines: orbitals ``C(R) = S(R)^-1/2 U`` with ``U`` fixed, CASCI roots of those orbitals.
        No electron-translation factors: ``sum_A couplings`` is the net of the ``Da . T^A`` part, not zero.

        - All three matrices are antisymmetric in (I, J) exactly (one element is computed and stored to both places
          with opposite sign) and their diagonal is exactly zero.
        - The SIGN of an element is that of the product of the two CI vectors' signs as ``casci`` fixes them;
          ``overlaps.apply_tracking(couplings, perm, sign)`` gives the couplings of the tracked states.
        - Within a (near-)degenerate pair the coupling diverges.  ``min_gap``: a pair with ``|E_J - E_I|`` below it is
          handled as ``small_gap`` says: ``"raise"``: ValueError naming the geometries and pairs, before the pass over
          the derivative integrals; ``"nan"``: NaN in ``ci_term`` and ``couplings`` for those elements only,
          ``orbital_term`` still filled.

        ``index``, ``chunk``, the scope and the errors are those of ``casci_nuclear_gradients``; the same bits whatever
        ``index`` and ``chunk``."""
        from . import ci
        check_small_gap(small_gap)
        who = "casci_derivative_couplings"
        min_gap = float(min_gap)
        sets = self._casci_sets(who, nroots, fix_singlet, index, tol, max_iter)
        rows, R, pairs, a, N = sets.rows, sets.nroots, sets.pairs, self.ncas, self.nao
        if small_gap == "raise" and pairs:
            # (before the pass over the derivative integrals)
            eh = sets.energies.detach().cpu().numpy()
            bad = [(g, i, j) for g in rows for i, j in pairs if abs(eh[g, i] - eh[g, j]) < min_gap]
            if bad:
                raise ValueError(f"{who}: |E_J - E_I| < {min_gap:g} Ha for (geometry, I, J) = "
                                 + ", ".join(str(b) for b in bad) + ": the coupling diverges there "
                                 "(small_gap='nan' marks these elements instead)")
        grads = pair_matrix(self._casci_derivative_pass(sets, chunk)[0], R)
        natm = self.basis.natm
        sel = torch.as_tensor(rows, device=self.device)
        c, P = len(rows), len(pairs)
        e, vecs = sets.energies[sel], sets.ci[sel]
        if not (P and c):       # no pair or no row: nothing to compute, the matrices are zero
            orb_val = ci_val = torch.empty((c, P, natm, 3), dtype=F64, device=self.device)
        else:
            ii = torch.as_tensor([p[0] for p in pairs], dtype=torch.long, device=self.device)
            jj = torch.as_tensor([p[1] for p in pairs], dtype=torch.long, device=self.device)
            # transition 1-RDMs <c_I|E_pq|c_J> of the pairs (I > J) and their antisymmetric parts
            t = ci.transition_rdm1(vecs[:, ii].reshape(c * P, -1), vecs[:, jj].reshape(c * P, -1), a, self.nelecas)
            asym = (0.5 * (t - t.transpose(1, 2))).contiguous()
            # Da = C_act a C_act^T, and a in the whole MO basis for the pull-back through S^-1/2
            Ca = self.mo_coeff[sel][:, :, self._n_occ:self._n_occ + a]
            Ca = Ca[:, None].expand(c, P, N, a).reshape(c * P, N, a).contiguous()
            Da = ops.matmul_nn_batch(ops.matmul_nn_batch(Ca, asym), Ca.transpose(1, 2).contiguous())
            a_mo = torch.zeros((c * P, N, N), dtype=F64, device=self.device)
            a_mo[:, self._n_occ:self._n_occ + a, self._n_occ:self._n_occ + a] = asym
            wqc = nucgrad.connection_pullback(self.overlap[sel], self.oao_mo_coeff[sel], a_mo.view(c, P, N, N))
            xyz = self.coords_bohr[sel]
            orb_val = GTO.overlap_connection_into(self.basis, xyz, Da.view(c, P, N, N))
            orb_val = orb_val + GTO.gradient_sets_into(self.basis, xyz, None, wqc, None, False)
            gap = e[:, jj] - e[:, ii]                                    # E_J - E_I of element (I, J)
            ci_val = grads[:, ii, jj] / gap[:, :, None, None]
            if small_gap == "nan":
                ci_val = torch.where((gap.abs() < min_gap)[:, :, None, None], torch.full_like(ci_val, float("nan")),
                                     ci_val)
        ci_term, orb = pair_matrix(ci_val, R, -1), pair_matrix(orb_val, R, -1)
        return CASCICouplings(e, vecs, grads, ci_term + orb, ci_term, orb)

    def casci_relaxed_gradients(self, nroots=2, fix_singlet=True, index=None, chunk=None, tol=1e-9, max_iter=200,
                                z_tol=1e-10, z_max_iter=100, brillouin_tol=1e-8, min_gap=1e-6, small_gap="raise"):
        """CASCI states of every geometry on its canonical RHF orbitals with their ORBITAL-RELAXED nuclear gradients:
        the slope of the surface ``E_I(R)`` on which the orbitals are re-made by RHF at every geometry (``from_geometries(
        ..., oao_mo_coeffs="rhf")``), which ``casci_nuclear_gradients`` -- the derivative at fixed ``oao_mo_coeff`` --
        is not: a CASCI energy is not stationary with respect to the orbitals.  -> ``CASCIRelaxedGradients(energies
        [G', R], ci [G', R, Dc], gradients [G', R, natm, 3], fixed_orbital [G', R, natm, 3], z_info [G', R],
        charge_gradients [G', R, M, 3] or None)`` on the device, Hartree / Bohr.

        ``gradients`` is the derivative at fixed ``oao_mo_coeff`` of the Lagrangian ``E_I - sum_{p>q} z_pq f_pq`` (``f``
        the RHF Fock matrix in the MO basis, whose off-diagonal elements vanish at every geometry): one Z-vector solve
        per state (``nucgrad.zvector``: conjugate gradients on the device to a residual ``z_tol``, at most
        ``z_max_iter`` iterations), three corrected densities (``nucgrad.relaxed_densities``) and the same single pass
        over the derivative integrals that gives ``fixed_orbital`` -- the diagonal of what ``casci_nuclear_gradients``
        returns, bit for bit.  For an embedded batch the charges' pull on the atoms uses the relaxed one-particle
        density, and ``charge_gradients`` is the relaxed derivative with respect to the charges' positions.

        - The orbitals must be the canonical RHF orbitals of their geometry, wherever they came from: ``f = C^T (h +
          G[D0]) C`` is formed from the batch's own orbitals and a geometry whose largest off-diagonal ``|f_pq|`` exceeds
          ``brillouin_tol`` raises ValueError.  The Fermi level must lie inside the active space.
        - A core / active-occupied or active-virtual / external pair of orbitals closer in energy than ``min_gap`` makes
          the response diverge: ``small_gap="raise"``: ValueError naming the geometries and pairs, before the CASCI
          solve; ``"nan"``: NaN in ``gradients`` (and ``charge_gradients``) for the states of those geometries only and
          ``z_info = -4`` there, ``fixed_orbital`` still filled.
        - Any other ``z_info != 0`` (``nucgrad.Z_INFO``) raises ``OovqeError`` naming geometry, state and code.

        ``index``, ``chunk``, the other arguments, the scope and the errors are those of ``casci_nuclear_gradients``; the
        same bits whatever ``index``, ``chunk`` and the stack around a geometry.  Not covered: relaxed interstate
        elements and derivative couplings, orbitals other than RHF orbitals, d shells."""
        who = "casci_relaxed_gradients"
        check_small_gap(small_gap)
        rows = self._casci_gradient_scope(who, nroots, index)
        scf.check_scope(self.nao, nelectron=self.nelectron)
        R, a, N, n_core, n_occ = int(nroots), self.ncas, self.nao, self._n_occ, self.nelectron // 2
        _, dg = nucgrad.response_pairs(N, n_core, a, n_occ)
        take = rows_selector(rows, self.device)
        # the RHF Fock matrix of the batch's own orbitals: canonical? gaps?
        g, h, C = self.int2e_ao[take], self.int1e_ao[take], self.mo_coeff[take].contiguous()
        mm = ops.matmul_nn_batch
        Co = C[:, :, :n_occ].contiguous()
        D0 = 2.0 * mm(Co, Co.transpose(1, 2).contiguous())
        J0, K0 = scf.fock_jk(g, D0)
        fock_ao = h + J0 - 0.5 * K0
        f = mm(mm(C.transpose(1, 2).contiguous(), fock_ao), C)
        eps = torch.diagonal(f, dim1=1, dim2=2).contiguous()
        off = (f - torch.diag_embed(eps)).abs().flatten(1).amax(dim=1).cpu().numpy()
        bad = [(r, float(x)) for r, x in zip(rows, off) if not x <= float(brillouin_tol)]
        if bad:
            raise ValueError(f"{who}: the orbitals are not canonical RHF orbitals (largest off-diagonal |f_pq| > "
                             f"{float(brillouin_tol):g}) for geometries " + ", ".join(f"{r} ({x:.3g})" for r, x in bad))
        eh = eps.cpu().numpy()
        pq = np.argwhere(dg)
        close = [(r, int(p), int(q)) for k, r in enumerate(rows) for p, q in pq
                 if abs(eh[k, p] - eh[k, q]) < float(min_gap)]
        if close and small_gap == "raise":
            raise ValueError(f"{who}: |eps_p - eps_q| < {float(min_gap):g} Ha for (geometry, p, q) = "
                             + ", ".join(str(c) for c in close) + ": the orbital response diverges there "
                             "(small_gap='nan' marks the states of these geometries instead)")
        # the states alone, and R more sets in the pass: the relaxed densities
        sets = self._casci_sets(who, nroots, fix_singlet, index, tol, max_iter, interstate=False, extra=R)
        # one Z-vector solve per state, from the orbital gradient of its generalised Fock matrix
        w = nucgrad.orbital_gradient(sets.fock[take])
        res = nucgrad.zvector(g, C, eps, n_core, a, n_occ, w, z_tol, z_max_iter, min_gap)
        z_info = res.info
        codes = z_info.cpu().numpy()
        wrong = [(r, i, int(codes[k, i])) for k, r in enumerate(rows) for i in range(R) if codes[k, i] not in (0, -4)]
        if wrong:
            raise _lib.OovqeError(f"{who}: the Z-vector solve failed for (geometry, state: code) = " + ", ".join(
                f"({r}, {i}: {c} {nucgrad.Z_INFO.get(c, '')})" for r, i, c in wrong))
        z = torch.where((z_info == -4)[:, :, None, None], torch.zeros_like(res.z), res.z)

        def relaxed_sets(k0, sel, d1, d2, wq, out):
            c = len(sel)
            out.copy_(d2)
            d1r, _, wqr = nucgrad.relaxed_densities(h[k0:k0 + c], g[k0:k0 + c], self.overlap[sel],
                                                    self.oao_mo_coeff[sel], C[k0:k0 + c], n_occ, z[k0:k0 + c], d1,
                                                    out, wq, fock_ao=fock_ao[k0:k0 + c])
            return d1r, wqr

        values, grad_q = self._casci_derivative_pass(sets, chunk, relaxed_sets)
        sel = torch.as_tensor(rows, device=self.device)
        marked = (z_info == -4)[:, :, None, None]
        grad = torch.where(marked, torch.full_like(values[:, R:], float("nan")), values[:, R:])
        if grad_q is not None:
            grad_q = torch.where(marked, torch.full_like(grad_q, float("nan")), grad_q)
        return CASCIRelaxedGradients(sets.energies[sel], sets.ci[sel], grad, values[:, :R].contiguous(), z_info, grad_q)

    def rhf_nuclear_gradient(self, result=None, index=None):
        """Closed-shell Hartree-Fock gradient -> [G, natm, 3] (device, Hartree / Bohr) from a converged
        ``scf.RHFResult`` of the rows ``index`` (default all; ``self.rhf(index=index)`` is run when none is given):
        ``D = 2 C_o C_o^T`` and the energy-weighted density ``WQ = -2 C_o eps_o C_o^T``.  Exact for converged orbitals
        only (the orbital gradient is taken as zero)."""
        rows = self._gradient_rows(index, "rhf_nuclear_gradient")
        result, d1 = self._rhf_density(result, index, rows)
        sel = torch.as_tensor(rows, device=self.device)
        grad = nucgrad.rhf_gradient(self.basis, self.coords_bohr[sel], result.mo_coeff, result.mo_energy,
                                    self.nelectron // 2)
        if self.charge_q is not None:
            grad += self._charge_pull(sel, d1, True)[0]
        return grad

    # ---- dipole and second moments (auto_oo_amd/properties.py, csrc/gto_moments.hip) -----------------------------------
    def _moments_of(self, rows, dens, order, origin, nuclear=True):
        """Moments [len(rows), nd, 3 or 9] of the densities ``dens`` [len(rows), nd, N, N] at the geometries ``rows``;
        ``origin`` [3] or [len(rows), 3] in Angstrom."""
        from . import properties
        sel = torch.as_tensor(rows, device=self.device)
        o = GTO.origin_to_device(origin, len(rows), self.device, 1.0 / GTO.BOHR)
        return properties.multipole_moments(self.basis, self.coords_bohr[sel], dens, order, o, nuclear)

    def _state_density(self, thetas, rows):
        """``D1`` [len(rows), N, N] of the circuit states at ``thetas`` and the batch's current orbitals, from the RDMs
        the evaluation path makes (dense register: ``ops.circuit_rdms``; sector engine: the RDMs of
        ``_evaluate_sector``)."""
        gamma, Gamma = self._circuit_rdms(thetas, "the moments of a circuit state", "cover", sector=True)
        sel = torch.as_tensor(rows, device=self.device)
        return nucgrad.cas_ao_densities(self.mo_coeff[sel], self._n_occ, self.ncas, gamma[sel], Gamma[sel],
                                        want_d2=False)[0]

    def multipole_moments(self, thetas, order=2, index=None, origin=None):
        """Dipole moment and second moments of every geometry's state at ``thetas`` [G, n_theta] and the batch's
        current orbitals, in atomic units: ``mu = sum_A Z_A (R_A - O) - tr(D1 r)``, ``Q_ij = sum_A Z_A (R_A - O)_i
        (R_A - O)_j - tr(D1 r_i r_j)`` (``properties.traceless_quadrupole`` makes the traceless form).

        Args:
            order: 2 -> (dipole [G, 3], second moments [G, 3, 3]); 1 -> the dipole alone
            index: rows of the batch (default all); the result then has one entry per row asked for
            origin: [3] or one [3] per row, in Angstrom like the geometries (default: the origin of the coordinates)

        Expectation values of a state that is not variational in every parameter are not energy derivatives.  Needs a
        batch made by ``from_geometries`` (RuntimeError otherwise); ncas <= 8.  Same bits whatever ``index``."""
        rows = self._moment_rows(index, "multipole_moments")
        GTO.moment_components(order)
        from . import properties
        out = self._moments_of(rows, self._state_density(thetas, rows)[:, None], order, origin)[:, 0]
        return out if order == 1 else properties.split_moments(out)

    def dipole_moment(self, thetas, index=None, origin=None):
        """Dipole moment [G, 3] (device, atomic units; times ``properties.DEBYE`` for Debye) of every geometry's state
        at ``thetas``: ``multipole_moments(thetas, order=1, ...)``."""
        self._moment_rows(index, "dipole_moment")
        return self.multipole_moments(thetas, order=1, index=index, origin=origin)

    def rhf_dipole_moment(self, result=None, index=None, origin=None):
        """Closed-shell Hartree-Fock dipole moment [G, 3] (device, atomic units) from a ``scf.RHFResult`` of the rows
        ``index`` (default all; ``self.rhf(index=index)`` is run when none is given): ``D = 2 C_o C_o^T``."""
        rows = self._moment_rows(index, "rhf_dipole_moment")
        _, d1 = self._rhf_density(result, index, rows)
        return self._moments_of(rows, d1[:, None], 1, origin)[:, 0]

    def _casci_densities(self, who, nroots, fix_singlet, tol, max_iter):
        """The CASCI solve of the whole stack and the AO one-particle densities of its roots and pairs of roots ->
        (energies [G, R], dens [G, R + P, N, N], nuclear [R + P]): the R states' ``D1``, then for the P pairs of
        ``nucgrad.state_pairs`` the transition density as the half-difference of the densities of ``(c_I +- c_J) /
        sqrt 2`` (``nucgrad.polarisation_vectors``, ``nucgrad.transition_sets``); ``nuclear``: which sets carry the
        nuclear term (the states)."""
        from . import ci
        self._refuse_large_ncas(who)
        e, vecs = self.casci(nroots, fix_singlet, tol, max_iter)
        G, R, a = self.G, int(nroots), self.ncas
        stack = nucgrad.polarisation_vectors(vecs)
        n = int(stack.shape[1])
        gamma, Gamma = ci.sector_rdms(stack.reshape(G * n, -1), a, self.nelecas)
        d1 = nucgrad.cas_ao_densities(self.mo_coeff, self._n_occ, a, gamma.reshape(G, n, a, a),
                                      Gamma.reshape((G, n) + (a,) * 4), want_d2=False)[0]
        return e, nucgrad.transition_sets(d1, R), [True] * R + [False] * ((n - R) // 2)

    def casci_dipole_matrix(self, nroots=2, fix_singlet=True, origin=None, tol=1e-9, max_iter=200):
        """CASCI states of every geometry at its current orbitals (``casci``) and their dipole matrix -> (energies
        [G, nroots], dipoles [G, nroots, nroots, 3]) on the device, atomic units.

        ``dipoles[g, I, I]`` is the dipole moment of root I, nuclear part included.  ``dipoles[g, I, J]``, I != J, is
        the transition dipole ``-tr(D^IJ r)`` with ``D^IJ = C_a gamma^IJ C_a^T`` and ``gamma^IJ = (<I|E_pq|J> +
        <J|E_pq|I>) / 2``, taken as ``(gamma_+ - gamma_-) / 2`` from the RDMs of ``(c_I +- c_J) / sqrt 2``: no nuclear
        term, and the core density drops out.  The matrix is symmetric in (I, J), exactly.  The SIGN of a transition
        dipole is that of the product of the two CI vectors' signs, which ``casci`` fixes by making the largest
        |component| of each vector positive; along a path on which that component changes, the sign can flip:
        ``overlaps.track_roots`` on the ``O`` of ``casci_overlaps`` gives the order and signs that are continuous along a
        path, ``overlaps.apply_tracking`` applies them to ``dipoles``."""
        rows = self._moment_rows(None, "casci_dipole_matrix")
        e, dens, nuclear = self._casci_densities("casci_dipole_matrix", nroots, fix_singlet, tol, max_iter)
        return e, pair_matrix(self._moments_of(rows, dens, 1, origin, nuclear=nuclear), int(nroots))

    # ---- electrostatic potential and field at arbitrary points (csrc/gto_potential.hip) ---------------------------------
    def _potential_of(self, rows, dens, points, field, nuclear=True):
        """``gto.potential_into`` of the densities ``dens`` [len(rows), nd, N, N] at the geometries ``rows``; ``points``
        [M, 3] or [len(rows), M, 3] in Angstrom.  More than ``gto.MAX_GRAD_SETS`` densities go in several calls (a set has
        the same bits whatever the other sets of its call)."""
        sel = torch.as_tensor(rows, device=self.device)
        pts = torch.as_tensor(GTO.points_host(points, len(rows))).to(self.device)
        nd = int(dens.shape[1])
        flags = [bool(nuclear)] * nd if isinstance(nuclear, (bool, np.bool_)) else [bool(f) for f in nuclear]
        xyz = self.coords_bohr[sel]
        phis, fields = [], []
        for a in range(0, nd, GTO.MAX_GRAD_SETS):
            b = min(nd, a + GTO.MAX_GRAD_SETS)
            out = GTO.potential_into(self.basis, xyz, pts, dens[:, a:b], flags[a:b], field)
            phis.append(out[0] if field else out)
            if field:
                fields.append(out[1])
        phi = phis[0] if len(phis) == 1 else torch.cat(phis, dim=1)
        if not field:
            return phi
        return phi, (fields[0] if len(fields) == 1 else torch.cat(fields, dim=1))

    def electrostatic_potential(self, thetas, points, index=None, field=False):
        """The electrostatic potential every geometry's state at ``thetas`` [G, n_theta] and the batch's current orbitals
        makes at ``points``, in atomic units: ``phi[g, m] = sum_A Z_A / |R_A - r_m| - tr(D1 <1 / |r - r_m|>)``
        (``gto.potential_batch`` of the density of ``_state_density``).

        Args:
            points: [M, 3] shared by all rows, or one [M, 3] per row asked for, in Angstrom like the geometries
            index: rows of the batch (default all); the result then has one entry per row asked for
            field: also return ``F = -d phi / d r`` [G, M, 3] in Hartree / (e Bohr)

        Returns ``phi`` [G, M] in Hartree / e on the device, or ``(phi, F)``.  For an embedded batch
        (``from_geometries(point_charges=...)``) this is the potential of the POLARISED MOLECULE ALONE: the external
        charges' own potential is not included.  Needs a batch made by ``from_geometries`` (RuntimeError otherwise);
        ncas <= 8.  Same bits whatever ``index``."""
        rows = self._moment_rows(index, "electrostatic_potential")
        out = self._potential_of(rows, self._state_density(thetas, rows)[:, None], points, field)
        return (out[0][:, 0], out[1][:, 0]) if field else out[:, 0]

    def rhf_electrostatic_potential(self, points, result=None, index=None, field=False):
        """Closed-shell Hartree-Fock electrostatic potential [G, M] (and field [G, M, 3]; device, atomic units) at
        ``points`` from a ``scf.RHFResult`` of the rows ``index`` (default all; ``self.rhf(index=index)`` is run when none
        is given): ``D = 2 C_o C_o^T``.  ``points``, ``field`` and the embedded case as for
        ``electrostatic_potential``: with the orbitals of an embedded batch, ``phi`` at the position of charge k is
        ``dE_RHF / dq_k``."""
        rows = self._moment_rows(index, "rhf_electrostatic_potential")
        _, d1 = self._rhf_density(result, index, rows)
        out = self._potential_of(rows, d1[:, None], points, field)
        return (out[0][:, 0], out[1][:, 0]) if field else out[:, 0]

    def casci_electrostatic_potential(self, points, nroots=2, fix_singlet=True, field=False, tol=1e-9, max_iter=200):
        """CASCI states of every geometry at its current orbitals (``casci``) and the matrix of their electrostatic
        potentials at ``points`` -> (energies [G, nroots], phi [G, nroots, nroots, M]) on the device, atomic units; with
        ``field`` also F [G, nroots, nroots, M, 3].

        ``phi[g, I, I]`` is the potential of root I, nuclear part included.  ``phi[g, I, J]``, I != J, is the transition
        potential ``-tr(D^IJ <1 / |r - r_m|>)`` with the ``D^IJ`` of ``casci_dipole_matrix`` (the same ``gamma^IJ``
        construction): no nuclear term, exactly symmetric in (I, J), and with the sign convention described there
        (``overlaps.apply_tracking`` works on it).  ``points`` and the embedded case as for
        ``electrostatic_potential``."""
        rows = self._moment_rows(None, "casci_electrostatic_potential")
        e, dens, nuclear = self._casci_densities("casci_electrostatic_potential", nroots, fix_singlet, tol, max_iter)
        out = self._potential_of(rows, dens, points, field, nuclear=nuclear)
        return (e, *(pair_matrix(val, int(nroots)) for val in (out if field else (out,))))

    # ---- electron density, its gradient and orbital values at arbitrary points (csrc/gto_density.hip) -------------------
    def _density_of(self, rows, dens, points, gradient):
        """``gto.density_into`` of the densities ``dens`` [len(rows), nd, N, N] at the geometries ``rows``; ``points``
        [M, 3] or [len(rows), M, 3] in Angstrom.  More than ``gto.MAX_GRAD_SETS`` densities go in several calls (a set has
        the same bits whatever the other sets of its call)."""
        sel = torch.as_tensor(rows, device=self.device)
        pts = torch.as_tensor(GTO.points_host(points, len(rows))).to(self.device)
        nd = int(dens.shape[1])
        xyz = self.coords_bohr[sel]
        rhos, grads = [], []
        for a in range(0, nd, GTO.MAX_GRAD_SETS):
            out = GTO.density_into(self.basis, xyz, pts, dens[:, a:min(nd, a + GTO.MAX_GRAD_SETS)], gradient)
            rhos.append(out[0] if gradient else out)
            if gradient:
                grads.append(out[1])
        rho = rhos[0] if len(rhos) == 1 else torch.cat(rhos, dim=1)
        if not gradient:
            return rho
        return rho, (grads[0] if len(grads) == 1 else torch.cat(grads, dim=1))

    def electron_density(self, thetas, points, index=None, gradient=False):
        """The electron density of every geometry's state at ``thetas`` [G, n_theta] and the batch's current orbitals at
        ``points``, in atomic units: ``rho[g, m] = sum D1[mu, nu] chi_mu(r_m) chi_nu(r_m)`` (``gto.density_batch`` of the
        density of ``_state_density``).

        Args:
            points: [M, 3] shared by all rows, or one [M, 3] per row asked for, in Angstrom like the geometries
            index: rows of the batch (default all); the result then has one entry per row asked for
            gradient: also return ``d rho / d r`` [G, M, 3] in e / Bohr^4

        Returns ``rho`` [G, M] in e / Bohr^3 on the device, or ``(rho, drho)``.  Needs a batch made by ``from_geometries``
        (RuntimeError otherwise); ncas <= 8; dense-register circuits only: a circuit of the sector engine (more than 10
        qubits) raises NotImplementedError before anything is launched.  Same bits whatever ``index``."""
        rows = self._moment_rows(index, "electron_density")
        if self._sector:
            raise NotImplementedError("electron_density covers dense-register circuits; circuits in the sector engine "
                                      "(more than 10 qubits) are not implemented")
        out = self._density_of(rows, self._state_density(thetas, rows)[:, None], points, gradient)
        return (out[0][:, 0], out[1][:, 0]) if gradient else out[:, 0]

    def rhf_electron_density(self, points, result=None, index=None, gradient=False):
        """Closed-shell Hartree-Fock electron density [G, M] (and its gradient [G, M, 3]; device, atomic units) at
        ``points`` from a ``scf.RHFResult`` of the rows ``index`` (default all; ``self.rhf(index=index)`` is run when none
        is given): ``D = 2 C_o C_o^T``.  ``points`` and ``gradient`` as for ``electron_density``."""
        rows = self._moment_rows(index, "rhf_electron_density")
        _, d1 = self._rhf_density(result, index, rows)
        out = self._density_of(rows, d1[:, None], points, gradient)
        return (out[0][:, 0], out[1][:, 0]) if gradient else out[:, 0]

    def casci_electron_density(self, points, nroots=2, fix_singlet=True, gradient=False, tol=1e-9, max_iter=200):
        """CASCI states of every geometry at its current orbitals (``casci``) and the matrix of their densities at
        ``points`` -> (energies [G, nroots], rho [G, nroots, nroots, M]) on the device, atomic units; with ``gradient``
        also drho [G, nroots, nroots, M, 3].

        ``rho[g, I, I]`` is the density of root I.  ``rho[g, I, J]``, I != J, is the transition density ``sum D^IJ chi
        chi`` with the ``D^IJ`` of ``casci_dipole_matrix`` (the same ``gamma^IJ`` construction): exactly symmetric in
        (I, J), and with the sign convention described there (``overlaps.apply_tracking`` works on it)."""
        rows = self._moment_rows(None, "casci_electron_density")
        e, dens, _ = self._casci_densities("casci_electron_density", nroots, fix_singlet, tol, max_iter)
        out = self._density_of(rows, dens, points, gradient)
        return (e, *(pair_matrix(val, int(nroots)) for val in (out if gradient else (out,))))

    def orbital_values(self, points, columns=None, index=None, gradient=False):
        """The values of the batch's current orbitals ``mo_coeff`` at ``points`` -> psi [G, ncol, M] in Bohr^-3/2 on the
        device, with ``gradient`` ``(psi, dpsi [G, ncol, M, 3])`` (``gto.orbital_values_batch``).

        Args:
            points: as for ``electron_density``
            columns: orbitals (columns of ``mo_coeff``) in the order wanted; default: the doubly occupied and the active
                ones.  More than ``gto.MAX_GRAD_SETS`` go in several calls (same bits).
            index: rows of the batch (default all)"""
        rows = self._moment_rows(index, "orbital_values")
        n = int(self.mo_coeff.shape[-1])
        cols = list(range(self._n_occ + self.ncas)) if columns is None else [int(c) for c in columns]
        if not cols or min(cols) < 0 or max(cols) >= n:
            raise ValueError(f"columns = {columns!r}: orbitals 0 .. {n - 1}, at least one")
        sel = torch.as_tensor(rows, device=self.device)
        pts = torch.as_tensor(GTO.points_host(points, len(rows))).to(self.device)
        C = self.mo_coeff[sel][:, :, torch.as_tensor(cols, device=self.device)]
        xyz = self.coords_bohr[sel]
        outs = [GTO.orbital_values_into(self.basis, xyz, pts, C[:, :, a:a + GTO.MAX_GRAD_SETS].contiguous(), gradient)
                for a in range(0, len(cols), GTO.MAX_GRAD_SETS)]
        if not gradient:
            return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)
        return tuple(o[0] if len(outs) == 1 else torch.cat(o, dim=1) for o in zip(*outs))

    # ---- overlaps between the states of different geometries (auto_oo_amd/overlaps.py, csrc/overlap.hip) --------------
    def _pair_rows(self, pairs, closed):
        """``pairs`` -> ([P] rows a, [P] rows b) on the host; the default is the loop (g, g + 1 mod G) when ``closed``,
        else the open path (g, g + 1)."""
        if pairs is None:
            a = list(range(self.G if closed else self.G - 1))
            return a, [(g + 1) % self.G for g in a]
        p = pairs.detach().cpu().numpy() if isinstance(pairs, torch.Tensor) else np.asarray(pairs)
        p = p.reshape(-1, 2) if p.size else p.reshape(0, 2)
        if p.ndim != 2 or p.shape[1] != 2 or not np.issubdtype(p.dtype, np.integer):
            raise ValueError("pairs must be [P, 2] integer rows of the batch")
        if p.size and (p.min() < 0 or p.max() >= self.G):
            raise ValueError(f"pairs must hold rows in 0..{self.G - 1}")
        return [int(v) for v in p[:, 0]], [int(v) for v in p[:, 1]]

    def _exact_overlaps(self, ra, rb, bra, ket, n_alpha, n_beta, orthogonalize, index):
        """``core_det^2 out`` of ``overlaps.sector_overlaps`` in the true AO metric for the pairs (ra[p], rb[p]):
        ``s = C_a[:, :M]^T S_ab C_b[:, :M]``, M = core + active orbitals, ``S_ab`` from ``gto.cross_overlap_into``."""
        from . import overlaps
        M = self._n_occ + self.ncas
        ia = torch.as_tensor(ra, device=self.device)
        ib = torch.as_tensor(rb, device=self.device)
        S_ab = GTO.cross_overlap_into(self.basis, self.coords_bohr[ia], self.coords_bohr[ib])
        Ca_t = self.mo_coeff[ia][:, :, :M].transpose(1, 2).contiguous()
        Cb = self.mo_coeff[ib][:, :, :M].contiguous()
        s = ops.matmul_nn_batch(Ca_t, ops.matmul_nn_batch(S_ab, Cb))
        out, core = overlaps.sector_overlaps(s, self._n_occ, self.ncas, n_alpha, n_beta, bra, ket, orthogonalize, True,
                                             index)
        return out * (core * core)[:, None, None]

    def state_overlaps(self, thetas, pairs=None, metric="ao", orthogonalize=None):
        """Overlaps between the circuit states of pairs of geometries -> [P] on the device, all pairs from one launch
        of ``oovqe_sector_overlap_batch``.

        Args:
            thetas: [G, n_theta], the parameters of every geometry's state
            pairs: [P, 2] rows (a, b) of the batch; default the closed loop (g, g + 1 mod G)
            metric: ``"ao"``: the exact ``<Psi_a|Psi_b>`` of the two all-electron wave functions at the batch's current
                orbitals, ``s = C_a[:, :M]^T S_ab C_b[:, :M]`` with the AO overlap ``S_ab`` between the two geometries
                (``gto.cross_overlap_batch``), core included; needs a batch made by ``from_geometries`` (RuntimeError
                otherwise).  ``"oao"``: the reference notebook's estimator ``<psi_b| G_{a->b} |psi_a>``
                (``overlaps.state_overlaps_oao``: the two orthonormal-AO bases treated as one, no core), any batch
            orthogonalize: ``"givens"`` or False; default ``"givens"`` for ``"oao"``, False for ``"ao"``

        Both circuit engines are served (dense registers through the index table of the sector).  ncas <= 8; every
        error is raised before anything is launched."""
        from . import overlaps
        from .sector import sector_of
        if metric not in ("ao", "oao"):
            raise ValueError(f"metric = {metric!r} ('ao' or 'oao')")
        if orthogonalize is None:
            orthogonalize = "givens" if metric == "oao" else False
        overlaps.orthogonalize_mode(orthogonalize)
        n_alpha, n_beta = sector_of(self.pqc.hfstate, self.ncas)
        overlaps.check_scope(self.ncas, n_alpha, n_beta, self._n_occ if metric == "ao" else 0)
        if metric == "ao" and (self.basis is None or self.coords_bohr is None):
            raise RuntimeError("state_overlaps(metric='ao') needs a batch made by OO_pqc_batch.from_geometries")
        ra, rb = self._pair_rows(pairs, closed=True)
        thetas = ops.as_device(thetas, self.device).reshape(self.G, self.n_theta)
        if not ra:
            return torch.empty(0, dtype=F64, device=self.device)
        pqc = self.pqc
        if self._sector:
            psi, index = pqc._sector.state(thetas), None
        else:
            psi = ops.circuit_state(thetas, pqc._gates_dev, pqc._n_gates, pqc.n_qubits, pqc._init_index)
            index = overlaps.dense_index(self.ncas, n_alpha, n_beta, self.device)
        ia = torch.as_tensor(ra, device=self.device)
        ib = torch.as_tensor(rb, device=self.device)
        if metric == "oao":
            return overlaps.state_overlaps_oao(psi[ib], psi[ia], self.oao_mo_coeff[ia], self.oao_mo_coeff[ib],
                                               self.act_idx, self.nelecas, orthogonalize)
        return self._exact_overlaps(ra, rb, psi[ia][:, None], psi[ib][:, None], n_alpha, n_beta, orthogonalize,
                                    index)[:, 0, 0]

    def berry_phase(self, thetas, metric="oao"):
        """The Berry-phase estimator of the closed loop the batch's geometries form -> ``(W, overlaps)`` on the device:
        ``overlaps`` [G] are ``state_overlaps(thetas, metric=metric)`` of the pairs (g, g + 1 mod G) and ``W`` their
        product (-1 around a conical intersection, +1 otherwise, for a finely sampled loop)."""
        o = self.state_overlaps(thetas, None, metric)
        return torch.prod(o), o

    def casci_overlaps(self, nroots=2, pairs=None, fix_singlet=True, vecs=None, tol=1e-9, max_iter=200):
        """CASCI states of every geometry at its current orbitals (``casci``) and their exact overlaps between pairs
        of geometries -> ``(energies [G, R], vecs [G, R, Dc], O [P, R, R])`` on the device, ``O[p, I, J] =
        <Psi_I(R_a)|Psi_J(R_b)>`` in the true AO metric (core included) for the pair p = (a, b).

        Args:
            nroots, fix_singlet, tol, max_iter: as for ``casci``
            pairs: [P, 2] rows of the batch; default the open path (g, g + 1), which is what
                ``overlaps.track_roots`` takes
            vecs: [G, R, Dc] CI vectors of an earlier ``casci`` to use instead of solving again (``energies`` is then
                returned as None)

        Needs a batch made by ``from_geometries`` (RuntimeError otherwise)."""
        from . import ci, overlaps
        ci.check_scope(self.ncas, self.nelecas, nroots)
        n = self.nelecas // 2
        overlaps.check_scope(self.ncas, n, n, self._n_occ)
        if self.basis is None or self.coords_bohr is None:
            raise RuntimeError("casci_overlaps needs a batch made by OO_pqc_batch.from_geometries")
        ra, rb = self._pair_rows(pairs, closed=False)
        e = None
        if vecs is None:
            e, vecs = self.casci(nroots, fix_singlet, tol, max_iter)
        else:
            vecs = ops.as_device(vecs, self.device)
            if vecs.dim() != 3 or tuple(vecs.shape[:2]) != (self.G, int(nroots)):
                raise ValueError(f"vecs has shape {tuple(vecs.shape)}, expected [{self.G}, {int(nroots)}, Dc]")
        R = int(nroots)
        if not ra:
            return e, vecs, torch.empty((0, R, R), dtype=F64, device=self.device)
        ia = torch.as_tensor(ra, device=self.device)
        ib = torch.as_tensor(rb, device=self.device)
        return e, vecs, self._exact_overlaps(ra, rb, vecs[ia], vecs[ib], n, n, False, None)

    def _rhf_orbitals(self, how, rows):
        """``oao_mo_coeffs="rhf"``: the orbitals of the rows (None: all) from the device solver."""
        if how != "rhf":
            raise ValueError(f"oao_mo_coeffs = {how!r}: the only named choice is 'rhf'")
        res = self.rhf(index=rows)
        scf.raise_unless_converged(res.info, rows)
        if rows is None:
            self.oao_mo_coeff.copy_(res.oao_mo_coeff)
        else:
            self.oao_mo_coeff[torch.as_tensor(rows, device=self.device)] = res.oao_mo_coeff

    def set_oao_mo_coeff(self, g, oao_mo_coeff):
        """Replace the orbitals of geometry g and refresh mo_coeff[g] = S^-1/2 C_oao
        (oo_energy.py:173-176)."""
        c = ops.as_device(oao_mo_coeff, self.device)
        self.oao_mo_coeff[g].copy_(c)
        self.mo_coeff[g].copy_(ops.matmul_nn(self.oao_coeff[g].contiguous(), c))

    def reverify_integrals(self):
        """Call after writing into ``int2e_ao`` (or ``int1e_ao`` / ``oao_coeff`` / ``nuc``) in place,
        e.g. when the integrals of many geometries are produced on the device: re-checks the
        symmetry flags of the whole stack bit for bit, rebuilds the packed resident copy (or drops
        it) -- one pass over the stack -- and refreshes ``mo_coeff = S^-1/2 C_oao`` of every geometry."""
        self._ingest()
        self.refresh_mo_coeff()

    def set_molecule(self, g, mol, oao_mo_coeff=None):
        """Replace geometry g of the batch (the next point of a Berry-phase loop, say): integrals,
        OAO basis, nuclear repulsion and orbitals.  The symmetry flags of the batch are re-verified
        for the new integrals and its slice of the packed copy is rebuilt (one pass over the new tensor) -- never
        write into ``int2e_ao`` directly, the flags and the packed copy would go stale."""
        if mol.nao != self.nao:
            raise ValueError("all geometries of a batch must share nao")
        self.int2e_ao[g].copy_(ops.as_device(mol.int2e_ao, self.device))
        self.int1e_ao[g].copy_(ops.as_device(mol.int1e_ao, self.device))
        self.oao_coeff[g].copy_(ops.as_device(mol.oao_coeff, self.device))
        self.nuc[g] = float(mol.nuc)
        if oao_mo_coeff is None:
            mol.run_rhf()
            oao_mo_coeff = mo_ao_to_mo_oao(mol.hf.mo_coeff, mol.overlap)
        self.set_oao_mo_coeff(g, oao_mo_coeff)
        self._ingest(g)

    def _ingest(self, g=None):
        """Symmetry flags and packed copy of geometry ``g`` (None: of the whole stack) from one pass over the
        integrals (``ops.eri_ingest``).  eri_flags = the symmetries every geometry of the stack has (a geometry
        replaced by a symmetric one can RESTORE a flag, not only drop it); the packed copy (slabs p <= q, upper
        triangle of each slab: about a quarter of the tensor) exists while every geometry carries both."""
        both = ops.ERI_PQ_SYMMETRIC | ops.ERI_RS_SYMMETRIC
        psz = int(self.lib.oovqe_eri_packed_size(self.nao))
        want = psz > 0 and not (self.nao <= 48 and self._n_occ + self.ncas > 16)
        had = self._eri_packed is not None
        if want and not had:
            self._eri_packed = torch.empty((self.G, psz), dtype=F64, device=self.device)
        if g is None:
            self._flags_g, _ = ops.eri_ingest(self.int2e_ao, pack=want, out=self._eri_packed)
        else:
            (self._flags_g[g],), _ = ops.eri_ingest(self.int2e_ao[g], pack=want,
                                                    out=self._eri_packed[g] if want else None)
        flags = both
        for f in self._flags_g:
            flags &= f
        self.eri_flags = flags
        if flags != both:
            self._eri_packed = None
        elif want and not had and g is not None:
            # the new geometry restored the last missing flag: the other slices of the copy are made now
            check(self.lib.oovqe_eri_pack(dptr(self.int2e_ao), self.nao, self.G, dptr(self._eri_packed),
                                          stream_ptr()), "oovqe_eri_pack")

    def refresh_mo_coeff(self):
        """mo_coeff[g] = S^-1/2[g] C_oao[g] for the whole stack (oo_energy.py:173-176), one launch."""
        ops.matmul_nn_batch(self.oao_coeff, self.oao_mo_coeff, out=self.mo_coeff)

    _sector = property(lambda self: getattr(self.pqc, "_use_sector", False))      # the circuit is in the sector engine

    def _layout(self, derivatives):
        """The packed output row of ``evaluate`` (``ops.PackedLayout``)."""
        return ops.PackedLayout(self.n_theta, self.n_kappa, self.ncas, bool(derivatives))

    def _workspace(self, key, work_size, *args, row=None):
        """``_plans[key]`` = (workspace of ``work_size(*args)`` doubles per geometry, the library's size of a packed
        output row with the ``ops.PackedLayout`` fields ``row``, or 0), made on first use."""
        if key not in self._plans:
            osz = self.lib.oovqe_oo_eval_out_size(*row) if row else 0
            self._plans[key] = (torch.empty(self.G * work_size(*args), dtype=F64, device=self.device), int(osz))
        return self._plans[key]

    def _plan(self, derivatives, slot=0):
        key, der, pqc = (bool(derivatives), slot), int(bool(derivatives)), self.pqc     # (looked up on every evaluation)
        return self._plans.get(key) or self._workspace(
            key, self.lib.oovqe_oo_eval_work_size, self.n_theta, pqc._n_gates, pqc.n_qubits, self.nao, self._n_occ,
            self.ncas, der, row=(self.n_theta, self.n_kappa, self.ncas, der))

    def _hessian_workspace(self, n_pairs):          # (``energy_gradient_hessian`` and the one-call step share it)
        return self._workspace(("hessian", 0), self.lib.oovqe_oo_hessian_work_size, self.n_theta, self.pqc._n_gates,
                               self.pqc.n_qubits, self.nao, self._n_occ, self.ncas, n_pairs,
                               row=(self.n_theta, self.n_kappa, self.ncas, 1))

    def evaluate(self, thetas, derivatives=True, count=None, slot=0, mo_coeff=None):
        """thetas [G, n_theta] (device, fp64) -> packed outputs [G, out_size]
        ([c0 | E | dE/dtheta | gvec rows | c1 | c2] per geometry, include/oovqe.h: ``ops.PackedLayout``).
        ``count``: evaluate only the first ``count`` geometries of the batch.
        ``slot``: workspace slot -- calls issued on different HIP streams must use different slots
        (their kernels then overlap: the HBM-bound N^4 sweep of one call runs beside the
        latency-bound tail kernels of the other).
        ``mo_coeff``: [G, N, N] orbitals to evaluate at instead of ``self.mo_coeff`` (rotated trial
        orbitals of a line search)."""
        G = self.G if count is None else int(count)
        if not 1 <= G <= self.G:
            raise ValueError(f"count must be in 1..{self.G}")
        thetas = ops.as_device(thetas, self.device).reshape(-1, self.n_theta)[:G]
        if self._sector:
            return self._evaluate_sector(thetas, derivatives, G, slot, mo_coeff)
        work, osz = self._plan(derivatives, slot)
        out = torch.empty((G, osz), dtype=F64, device=self.device)
        pqc = self.pqc
        check(self.lib.oovqe_oo_eval_batch(
            dptr(thetas), self.n_theta, dptr(pqc._gates_dev, torch.uint8), pqc._n_gates,
            pqc.n_qubits, ctypes.c_uint32(pqc._init_index), dptr(self.int2e_ao),
            dptr(self.int1e_ao), dptr(self.mo_coeff if mo_coeff is None else mo_coeff), dptr(self.nuc),
            self.nao, self._n_occ,
            self.ncas, dptr(self._kap_row, torch.int32), dptr(self._kap_col, torch.int32),
            self.n_kappa, int(bool(derivatives)), G, dptr(work), dptr(out), int(self.eri_flags),
            dptr(self._eri_packed) if self.eri_flags == 3 else None, stream_ptr()),
            "oovqe_oo_eval_batch")
        return out

    # ---- circuits in the sector engine ---------------------------------------------------------------
    def _cas_batch(self, gamma, Gamma, G, slot=0, mo_coeff=None, want_fock=False):
        """The CAS path of the first G geometries from RDM sets gamma [G, nrdm, a, a], Gamma [G, nrdm, a,a,a,a]
        (``oovqe_cas_eval_batch``) -> (packed rows [G, osz] of ``ops.PackedLayout.for_rdm_sets``, n_t, fock or None)."""
        nrdm = int(gamma.shape[1])
        work, osz = self._workspace(("cas", nrdm, slot), self.lib.oovqe_cas_eval_work_size, self.nao, self._n_occ,
                                    self.ncas, nrdm, row=(nrdm - 1, self.n_kappa, self.ncas, int(nrdm > 1)))
        out = torch.empty((G, osz), dtype=F64, device=self.device)
        fock = torch.empty((G, self.nao, self.nao), dtype=F64, device=self.device) if want_fock else None
        gamma = gamma if gamma.is_contiguous() else gamma.contiguous()
        Gamma = Gamma if Gamma.is_contiguous() else Gamma.contiguous()
        check(self.lib.oovqe_cas_eval_batch(
            dptr(self.int2e_ao), dptr(self.int1e_ao), dptr(self.mo_coeff if mo_coeff is None else mo_coeff),
            dptr(gamma), dptr(Gamma), nrdm, dptr(self.nuc), self.nao, self._n_occ, self.ncas,
            dptr(self._kap_row, torch.int32), dptr(self._kap_col, torch.int32), self.n_kappa, G, dptr(work), dptr(out),
            dptr(fock), int(self.eri_flags), dptr(self._eri_packed) if self.eri_flags == 3 else None, stream_ptr()),
            "oovqe_cas_eval_batch")
        return out, (nrdm - 1 if nrdm > 1 else 1), fock

    def _evaluate_sector(self, thetas, derivatives, G, slot, mo_coeff):
        """``evaluate`` for a circuit in the sector engine: the states and RDMs of all geometries in one launch each
        (the geometry is the sector kernels' batch index), the CAS path of all geometries in one call, dE/dtheta by
        the reverse sweep with each geometry's (c1, c2) as cotangents (oo_pqc.py:86-95).  The packed layout is that
        of the dense path; the rows d gvec / d theta_k (the kappa-theta block, which the reverse sweep does not
        produce) are NaN here -- ``energy_gradient_hessian`` delivers them."""
        eng, a = self.pqc._sector, self.ncas
        psi = eng.state(thetas)
        g1, g2 = eng.rdms(psi)
        cas, _, _ = self._cas_batch(g1[:, None], g2[:, None], G, slot, mo_coeff)
        if not derivatives:
            return cas
        Lc, L = self._layout(False), self._layout(True)
        out = cas.new_full((G, int(self.lib.oovqe_oo_eval_out_size(*L))), float("nan"))
        out[:, :2] = cas[:, :2]                                                 # c0, E
        L.gvec_rows(out)[:, 0] = Lc.gvec_rows(cas)[:, 0]                        # gvec row 0 = dE/dkappa
        out[:, L.c12] = cas[:, Lc.c12]                                          # c1 | c2
        if eng.geometry_coefficients_ok():
            # every geometry's reverse sweep in one launch sequence, its (c1 | c2) read where the CAS path left them
            out[:, L.dE] = eng.adjoint_geometries(thetas, psi, cas[:, Lc.c12], cas.stride(0))
        else:
            c1, c2 = cas[:, Lc.c1].reshape(G, a, a), cas[:, Lc.c2].reshape(G, a, a, a, a)
            for g in range(G):      # (the operator of the reverse sweep takes ONE set of coefficients per call)
                out[g, L.dE] = eng.adjoint(thetas[g:g + 1], psi[g:g + 1], c1[g], c2[g])[0]
        return out

    def _hessian_from_rdm_sets(self, gamma, Gamma, theta_theta):
        """``energy_gradient_hessian`` of the whole stack from RDM sets gamma [G, 1 + n_theta, a, a], Gamma [G, 1 +
        n_theta, a, a, a, a] (set 0 the RDMs, set k their derivatives by theta_k: the sector engine's, an ensemble's).
        Launches, in this order: the CAS path with Fock matrices (E, gradient, kappa-theta blocks), the kappa-kappa
        blocks in one ``oovqe_orbital_hessian_batch`` call, then the caller's ``theta_theta(out, c12, c_stride) ->
        [G, n_theta, n_theta]``, given the packed rows ``out`` of the CAS path (``ops.PackedLayout.for_rdm_sets``),
        their columns ``c12`` (c1 | c2 of every geometry, to be read where they lie) and the stride between rows."""
        G, nk, nt = self.G, self.n_kappa, int(gamma.shape[1]) - 1
        L = ops.PackedLayout.for_rdm_sets(1 + nt, nk, self.ncas)
        out, _, fock = self._cas_batch(gamma, Gamma, G, want_fock=True)
        gv = L.gvec_rows(out)
        work, _ = self._workspace(("orbital_hessian", 0), self.lib.oovqe_orbital_hessian_work_size, self.nao, self._n_occ,
                                  self.ncas)
        Hkk = torch.empty((G, nk, nk), dtype=F64, device=self.device)
        # the copies stay referenced until the call is enqueued: a temporary freed inside the argument list goes back
        # to the caching allocator at once, and the next copy can land in it before the kernel has read it
        gamma0, Gamma0 = gamma[:, 0].contiguous(), Gamma[:, 0].contiguous()
        check(self.lib.oovqe_orbital_hessian_batch(
            dptr(self.int2e_ao), dptr(self.int1e_ao), dptr(self.mo_coeff), dptr(gamma0), dptr(Gamma0), dptr(fock),
            self.nao, self._n_occ, self.ncas, dptr(self._kap_row, torch.int32), dptr(self._kap_col, torch.int32), nk, G,
            dptr(work), dptr(Hkk), int(self.eri_flags), stream_ptr()), "oovqe_orbital_hessian_batch")
        H = torch.empty((G, nt + nk, nt + nk), dtype=F64, device=self.device)
        H[:, :nt, :nt] = theta_theta(out, out[:, L.c12], out.stride(0))
        H[:, nt:, nt:] = Hkk
        H[:, nt:, :nt] = gv[:, 1:].transpose(1, 2)
        H[:, :nt, nt:] = gv[:, 1:]
        return out[:, L.E], torch.cat((out[:, L.dE], gv[:, 0]), dim=1), H

    def _energy_gradient_hessian_sector(self, thetas):
        pqc, eng = self.pqc, self.pqc._sector
        G, nt, a = self.G, self.n_theta, self.ncas
        st = eng.tangent_states(thetas, pqc._gates, second=True)                 # [G, 1 + nt + n_pairs, Dc]
        psi, tau = st[:, 0:1], st[:, 1:1 + nt]
        # derivative RDMs by polarisation of the plain RDM kernel (exact: the RDMs are quadratic forms of the real
        # state), all geometries in one list of sector vectors
        vecs = torch.cat((psi, psi + tau, psi - tau), dim=1).reshape(G * (2 * nt + 1), eng.Dc)
        r1, r2 = eng.rdms_chunked(vecs)
        r1 = r1.reshape(G, 2 * nt + 1, a, a)
        r2 = r2.reshape(G, 2 * nt + 1, a, a, a, a)
        gamma = torch.cat((r1[:, 0:1], 0.5 * (r1[:, 1:1 + nt] - r1[:, 1 + nt:])), dim=1)
        Gamma = torch.cat((r2[:, 0:1], 0.5 * (r2[:, 1:1 + nt] - r2[:, 1 + nt:])), dim=1)

        def theta_theta(out, c12, c_stride):
            if not eng.geometry_coefficients_ok():
                L = self._layout(True)
                c1, c2 = out[:, L.c1].reshape(G, a, a), out[:, L.c2].reshape(G, a, a, a, a)
                # (one set of CAS coefficients per application of the operator)
                return torch.stack([eng.circuit_hessian_from_states(st[g], pqc._gates, c1[g].contiguous(),
                                                                    c2[g].contiguous()) for g in range(G)])
            # H_jk = tau_jk . lam(psi) + tau_j . lam(tau_k), lam = the operator of EACH geometry applied to its psi and
            # first tangents -- one launch sequence for all geometries
            ja, ka, _ = eng.hessian_pair_tables(pqc._gates)
            lam = eng.lam_geometries(st[:, :1 + nt].reshape(G * (1 + nt), eng.Dc), 1 + nt, c12,
                                     c_stride).reshape(G, 1 + nt, eng.Dc)
            first = (st[:, 1 + nt:] * lam[:, 0:1]).sum(dim=2)                           # [G, n_pairs]
            # tau_j . lam(tau_k): scalar products over the sector dimension, geometry by geometry (elementwise multiply
            # + sum, as SectorEngine.circuit_hessian_from_states: no vendor GEMM on this path)
            second = torch.stack([(st[g, 1:1 + nt, None, :] * lam[g, None, 1:, :]).sum(dim=2) for g in range(G)])
            val = first + second[:, ja, ka]
            Htt = torch.zeros((G, nt, nt), dtype=F64, device=self.device)
            Htt[:, ja, ka] = val
            Htt[:, ka, ja] = val
            return Htt

        return self._hessian_from_rdm_sets(gamma, Gamma, theta_theta)

    def evaluate_deferred(self, thetas, derivatives=True, count=None, mo_coeff=None, view=None):
        """``evaluate`` enqueued on one of the library's two side streams (taken in turn, each with a workspace of its
        own) -> ``ops.PendingTensor``; ``.result()`` joins it to the stream that is current then.  For INDEPENDENT calls
        issued back to back (a scan over parameter sets, the points of several loops, a benchmark's steps): the
        latency-bound tail of one call (q -> x / p -> n, Fock panels, assembly: a quarter of a 256-geometry call,
        during which HBM idles) runs under the N^4 sweep of the next call instead of in front of it.  The inputs
        must be complete on the current stream when this is called (the side stream is forked from it here);
        per call the launches and the arithmetic are those of ``evaluate``: the same bits."""
        if self._sector:
            # the sector engine keeps ONE workspace per batch size (not per stream): its calls stay in order on the
            # current stream; the result is complete in stream order, the handle has nothing to wait for
            out = self.evaluate(thetas, derivatives=derivatives, count=count, mo_coeff=mo_coeff)
            return ops.PendingTensor(out, None, view)
        side_streams = ops.side_streams(self.device)
        k = self._defer_next = (getattr(self, "_defer_next", 1) + 1) & 1
        side = side_streams[k]
        side.wait_stream(torch.cuda.current_stream())
        thetas = ops.as_device(thetas, self.device)
        with torch.cuda.stream(side):
            out = self.evaluate(thetas, derivatives=derivatives, count=count, slot=1 + k, mo_coeff=mo_coeff)
            event = torch.cuda.Event()
            event.record(side)
        thetas.record_stream(side)
        if mo_coeff is not None:
            mo_coeff.record_stream(side)
        return ops.PendingTensor(out, event, view)

    def energy_and_gradient(self, thetas, count=None, slot=0, defer=False):
        """-> [G, 1 + n_theta + n_kappa]: column 0 = E, then dE/dtheta, then dE/dkappa.
        ``defer``: -> ``ops.PendingTensor`` of the same (``evaluate_deferred``)."""
        piece = self._layout(True).energy_and_gradient
        if defer:
            return self.evaluate_deferred(thetas, derivatives=True, count=count, view=lambda o: o[:, piece])
        return self.evaluate(thetas, derivatives=True, count=count, slot=slot)[:, piece]

    def _energy_at(self, thetas, mo_coeff):
        """[G]: the energies at ``thetas`` and the orbitals ``mo_coeff`` [G, N, N] (None: the current ones)."""
        return self.evaluate(thetas, derivatives=False, mo_coeff=mo_coeff)[:, ops.PackedLayout.E]

    def energy(self, thetas, kappas=None):
        """-> [G] energies (OO_pqc.energy_from_parameters(theta, kappa) per geometry, oo_pqc.py:64-84).
        ``kappas`` [G, n_kappa]: evaluate at the rotated orbitals mo_coeff[g] expm(-K(kappa[g])) --
        one extra launch for all geometries (oovqe_rotate_orbitals_batch)."""
        return self._energy_at(thetas, None if kappas is None else self.rotated_mo_coeff(kappas))

    # ---- ADAPT-VQE on a stack (auto_oo_amd/adapt.py) ----------------------------------------
    def pool_gradients(self, thetas, pool, index=None):
        """[G, P] (the rows of ``index``): the energy derivative of every geometry with respect to every operator of
        ``pool`` (``adapt.OperatorPool``) appended behind the circuit with its parameter at 0, at the states
        psi(thetas[g]) and the current orbitals.  The CAS coefficients come from the evaluation of the stack, read
        where it leaves them; the operator on every state and the P sparse scalar products per state are ONE library
        call (``oovqe_pool_gradients_from_coefficients_batch``).  A row has the same bits wherever its geometry stands
        in the stack and whatever stream the call runs on."""
        from . import adapt
        adapt.check_pool(pool, self.pqc, "OO_pqc_batch.pool_gradients")
        adapt.check_thetas(thetas, self.G, self.n_theta, "OO_pqc_batch.pool_gradients")
        rows = stack_rows(self.G, index)
        thetas = ops.as_device(thetas, self.device).reshape(self.G, self.n_theta)        # (contiguous)
        out = self.evaluate(thetas, derivatives=False)
        if index is not None:
            sel = rows_selector(rows, self.device)
            thetas, out = thetas[sel].contiguous(), out[sel].contiguous()
        L = self._layout(False)                              # c1 | c2 of every geometry, read where they lie
        return adapt.gradients_from_coefficients(self.pqc, pool, thetas, out[:, L.c1], out[:, L.c2], out.stride(0))

    def set_circuit(self, pqc):
        """Hand the stack another circuit of the same active space (ADAPT-VQE appends a gate per step).  The resident
        integrals, their packed copy and symmetry flags, the orbitals and the geometry data stay as they are -- no
        integral is read again; ``n_theta``, the evaluation plans and the cached step arguments, which are sized by
        the circuit, are made afresh on next use."""
        if int(pqc.ncas) != int(self.ncas) or int(pqc.nelecas) != int(self.nelecas):
            raise ValueError(f"set_circuit: a circuit for CAS({pqc.nelecas}e, {pqc.ncas}o) on a stack of "
                             f"CAS({self.nelecas}e, {self.ncas}o)")
        # the workspaces about to be dropped may still be read by work enqueued on the side streams
        torch.cuda.synchronize(self.device)
        self.pqc = pqc
        self.n_theta = int(np.prod(pqc.theta_shape))
        self._plans = {}
        self._step_args = None
        self._flat0 = None
        self._all_pd_last_step = False
        self.__dict__.pop("_slabs_in_flight", None)

    # ---- exact reference of the stack ------------------------------------------------------------------
    def casci(self, nroots=1, fix_singlet=True, tol=1e-9, max_iter=200):
        """CASCI of every geometry at its current orbitals: the CAS coefficients of the whole stack from ONE
        ``oovqe_cas_eval_batch`` call, then ONE Davidson launch (``oovqe_ci_davidson_batch``) reading c0 | c1 | c2
        where that call leaves them.  -> (energies [G, nroots], ci [G, nroots, Dc]) on the device; the CI vectors
        are in the sector layout of the circuit engine.  Raises when a geometry's solve does not converge."""
        from . import ci
        ci.check_scope(self.ncas, self.nelecas, nroots)
        a = self.ncas
        zero1 = torch.zeros((self.G, 1, a, a), dtype=F64, device=self.device)
        zero2 = torch.zeros((self.G, 1) + (a,) * 4, dtype=F64, device=self.device)
        cas, _, _ = self._cas_batch(zero1, zero2, self.G)
        e, vecs, _, rn, info = ci.casci_packed(cas, ops.PackedLayout.for_rdm_sets(1, self.n_kappa, a).c12.start, a,
                                               self.nelecas, nroots, fix_singlet, tol, max_iter)
        bad = torch.nonzero(info != 0).flatten().tolist()
        if bad:
            raise RuntimeError(f"OO_pqc_batch.casci: geometries {bad} did not converge "
                               f"(residuals {rn[bad].tolist()})")
        return e, vecs

    # ---- orbital rotations of the whole stack -------------------------------------------------------
    def _rotate(self, C, kappas, out):
        kappas = ops.as_device(kappas, self.device).reshape(self.G, self.n_kappa)
        N = self.nao
        work = None
        if N > 48:
            work = torch.empty((self.G + 7) * N * N, dtype=F64, device=self.device)
        check(self.lib.oovqe_rotate_orbitals_batch(
            dptr(kappas), dptr(self._kap_row, torch.int32), dptr(self._kap_col, torch.int32),
            self.n_kappa, N, self.G, dptr(C), dptr(out), None, dptr(work), stream_ptr()),
            "oovqe_rotate_orbitals_batch")
        return out

    def rotated_mo_coeff(self, kappas):
        """[G, N, N]: mo_coeff[g] @ expm(-K(kappas[g])) (OO_energy.get_transformed_mo per geometry)."""
        return self._rotate(self.mo_coeff, kappas, torch.empty_like(self.mo_coeff))

    def rotate_(self, kappas):
        """oao_mo_coeff[g] <- oao_mo_coeff[g] @ expm(-K(kappas[g])) for every geometry (the update of
        oo_pqc.py:191) and mo_coeff = S^-1/2 C_oao refreshed."""
        if self.nao <= 48:      # (one workgroup per geometry, all in LDS: the result may overwrite its input)
            self._rotate(self.oao_mo_coeff, kappas, self.oao_mo_coeff)
        else:
            new = self._rotate(self.oao_mo_coeff, kappas, torch.empty_like(self.oao_mo_coeff))
            self.oao_mo_coeff.copy_(new)
        self.refresh_mo_coeff()

    # ---- configs[3]'s unit of work, batched -----------------------------------------------------------
    def energy_gradient_hessian(self, thetas):
        """E [G], full gradient [G, n] and full Hessian [G, n, n] (n = n_theta + n_kappa) of every
        geometry from ONE library call (``oovqe_oo_hessian_batch``): OO_pqc.full_gradient +
        OO_pqc.full_hessian (oo_pqc.py:132-148) with the geometry index as a grid dimension of every
        launch.  Block layout of the Hessian as the reference's: [[tt, (kt)^T], [kt, kk]]."""
        G, nt, nk = self.G, self.n_theta, self.n_kappa
        thetas = ops.as_device(thetas, self.device).reshape(G, nt)
        pqc = self.pqc
        if self._sector:
            return self._energy_gradient_hessian_sector(thetas)
        pairs_dev, _, _ = ops._hessian_pair_tables(nt, self.device)
        n_pairs = pairs_dev.shape[0]
        work, osz = self._hessian_workspace(n_pairs)
        out = torch.empty((G, osz), dtype=F64, device=self.device)
        H = torch.empty((G, nt + nk, nt + nk), dtype=F64, device=self.device)
        check(self.lib.oovqe_oo_hessian_batch(
            dptr(thetas), nt, dptr(pqc._gates_dev, torch.uint8), pqc._n_gates, pqc.n_qubits,
            ctypes.c_uint32(pqc._init_index), dptr(self.int2e_ao), dptr(self.int1e_ao), dptr(self.mo_coeff),
            dptr(self.nuc), self.nao, self._n_occ, self.ncas, dptr(self._kap_row, torch.int32),
            dptr(self._kap_col, torch.int32), nk, dptr(pairs_dev, torch.int32), n_pairs, G, dptr(work),
            dptr(out), dptr(H), int(self.eri_flags),
            dptr(self._eri_packed) if self.eri_flags == 3 else None, stream_ptr()), "oovqe_oo_hessian_batch")
        return out[:, ops.PackedLayout.E], out[:, self._layout(True).gradient], H

    def full_gradient(self, thetas):
        """-> [G, n_theta + n_kappa] (OO_pqc.full_gradient per geometry, oo_pqc.py:132-134)."""
        return self.energy_and_gradient(thetas)[:, 1:]

    def full_hessian(self, thetas):
        """-> [G, n, n] (OO_pqc.full_hessian per geometry, oo_pqc.py:136-148)."""
        return self.energy_gradient_hessian(thetas)[2]

    def damped_newton_step(self, thetas, opt=None, defer_lowest=False):
        """One damped Newton step on (theta, kappa) of EVERY geometry in lockstep -- the body of
        OO_pqc.full_optimization / of the Berry-phase loop (oo_pqc.py:172-196), per geometry the
        arithmetic of NewtonStep.damped_newton_step: gradient + Hessian, the G directions, a line search
        whose trials evaluate all geometries at once, then the orbitals of every geometry rotated.
        Returns (new thetas [G, n_theta], energies at the new parameters [G], lowest Hessian eigenvalues [G]).
        ``defer_lowest``: the eigenvalues come as an ``ops.PendingLowest`` -- they are a diagnostic
        (hess_eig_l of the reference's loops) computed on a side stream beside the line search; ``.result()``
        joins them.

        The whole step up to the first verdict of the line search is ONE library call
        (``oovqe_oo_newton_step_batch``: ~45 launches back to back) and one 32-byte readback; only further trials
        (rare) are driven from here.  ``step_by_calls=True`` (attribute; for tests and measurements) drives every
        stage through its own entry point instead -- the same launches, the same bits."""
        thetas = ops.as_device(thetas, self.device).reshape(self.G, self.n_theta)        # (contiguous)
        by_calls = (self.step_by_calls or self.n_theta + self.n_kappa > self.lib.oovqe_newton_direction_max_n()
                    or self.G > 32767 or self._sector)
        new_thetas, energies, low = self._lockstep_step(thetas, opt, self._energy_at,
                                                        self.energy_gradient_hessian if by_calls else None)
        return new_thetas, energies, (low if defer_lowest else low.checked())

    def _lockstep_step(self, thetas, opt, energy_at, egh):
        """The body of ``damped_newton_step`` for every driver on the stack (dense, sector engine, ``ensemble``):
        ``energy_at(thetas, mo_coeff) -> [G]`` is the driver's energy at given orbitals, ``egh(thetas) -> (E, grad, H)``
        at the current ones (None: the dense stack's ``_newton_step_one_call``, which makes them inside its library
        call).  -> (new thetas, energies there, lowest eigenvalues as ``ops.PendingLowest``); the orbitals are adopted."""
        from .newton_raphson import BatchedNewtonStep
        nt, opt = self.n_theta, (BatchedNewtonStep(verbose=0) if opt is None else opt)
        if self._trial_orbitals is None:
            self._trial_orbitals = (torch.empty_like(self.oao_mo_coeff), torch.empty_like(self.mo_coeff))

        def trial(pa, pb):
            # the orbitals of a trial are formed as an accepted step forms them -- C_oao expm(-K), then
            # S^-1/2 (C_oao U) (oo_pqc.py:191, oo_energy.py:173-176) -- so the accepted trial's orbitals ARE the new
            # ones: the step adopts them by exchanging buffers, nothing is launched behind the last readback
            t_oao, t_mo = self._trial_orbitals
            self._rotate(self.oao_mo_coeff, pb, t_oao)
            ops.matmul_nn_batch(self.oao_coeff, t_oao, out=t_mo)
            return energy_at(pa, t_mo)

        if egh is None:
            new_thetas, new_kappas, low, energies = self._newton_step_one_call(thetas, opt, trial)
        else:
            E, grad, H = egh(thetas)
            if self._flat0 is None:
                self._flat0 = torch.zeros((self.G, nt + self.n_kappa), dtype=F64, device=self.device)
            self._flat0[:, :nt] = thetas             # (the kappa part stays zero: steps start at the current orbitals)
            # the energy at the accepted trial point IS the energy at the new parameters, so the loop body's closing
            # evaluation (oo_pqc.py:195) is not repeated
            (new_thetas, new_kappas), low, energies = opt.damped_newton_steps_flat(
                trial, self._flat0, grad, H, energy0=E, defer_lowest=True, split=nt, return_energy=True)
        if opt.last_search_gave_up:
            self.rotate_(new_kappas)                 # (some problems went back to their old parameters)
        else:
            # every trial evaluates ALL geometries at their current points, the accepted ones at their accepted
            # point: the last trial's orbitals are the new orbitals of the whole stack.  Like the reference's
            # `self.oao_mo_coeff = ...` the attributes are rebound, not written in place.
            t_oao, t_mo = self._trial_orbitals
            self._trial_orbitals = (self.oao_mo_coeff, self.mo_coeff)
            self.oao_mo_coeff, self.mo_coeff = t_oao, t_mo
        return new_thetas, energies, low

    def _step_block(self):
        """The argument block of oovqe_oo_newton_step_batch with everything that does not change from step to
        step filled in (made once per batch object)."""
        if self._step_args is not None:
            return self._step_args
        lib, pqc, G, N = self.lib, self.pqc, self.G, self.nao
        nt, nk = self.n_theta, self.n_kappa
        n = nt + nk
        pairs_dev, _, _ = ops._hessian_pair_tables(nt, self.device)
        n_pairs = int(pairs_dev.shape[0])
        osz0 = int(lib.oovqe_oo_eval_out_size(nt, nk, self.ncas, 0))
        work_hessian, osz1 = self._hessian_workspace(n_pairs)
        work_eval, _ = self._plan(False, 0)
        b = _lib.NewtonStepT()
        keep = {"pairs": pairs_dev, "trial_out": torch.empty((G, osz0), dtype=F64, device=self.device),
                "flat": torch.empty((G, n), dtype=F64, device=self.device)}
        # the first trial's verdict goes straight into pinned host memory (the library's last kernel of the step writes
        # its four flags through the device-visible pointer; the host polls them instead of a 32-byte memcpy + stream
        # synchronisation: ~12 us of every step); later trials (rare) keep a device tensor and a readback
        keep["flags_host"] = torch.full((4,), float("nan"), dtype=F64).pin_memory()
        keep["flags_np"] = keep["flags_host"].numpy()
        keep["flags_dev"] = torch.empty(4, dtype=F64, device=self.device)
        has_pd = bool(lib.oovqe_newton_direction_has_pd(n, 1))
        if has_pd:
            keep["work_pd"] = torch.empty(int(lib.oovqe_newton_direction_pd_work_size(n, G)), dtype=F64,
                                          device=self.device)
        rest = int(lib.oovqe_newton_direction_rest_work_size(n, G))
        keep["work_rest"] = torch.empty(rest, dtype=F64, device=self.device)
        # one workspace per side stream: the eigenvalue routes of consecutive steps run beside each other
        keep["work_side"] = [torch.empty(rest, dtype=F64, device=self.device) for _ in range(2)]
        if N > 48:
            keep["work_rotate"] = torch.empty((G + 7) * N * N, dtype=F64, device=self.device)
        b.gates = pqc._gates_dev.data_ptr()
        b.kap_row, b.kap_col = self._kap_row.data_ptr(), self._kap_col.data_ptr()
        b.pairs = pairs_dev.data_ptr()
        b.work_hessian = work_hessian.data_ptr()
        b.work_eval = work_eval.data_ptr()
        b.work_pd = keep["work_pd"].data_ptr() if has_pd else None
        b.work_rest = keep["work_rest"].data_ptr()
        b.work_rotate = keep["work_rotate"].data_ptr() if N > 48 else None
        b.flat = keep["flat"].data_ptr()
        b.trial_out = keep["trial_out"].data_ptr()
        b.n_theta, b.n_gates, b.n_qubits, b.N, b.n_occ, b.ncas = nt, pqc._n_gates, pqc.n_qubits, N, self._n_occ, self.ncas
        b.n_kappa, b.n_pairs, b.batch = nk, n_pairs, G
        b.init_index = pqc._init_index
        # the eigenvalue route beside the line search keeps to a quarter of the chip (half for larger stacks):
        # ops.newton_direction
        b.side_wg = max(1, 64 // G) if G <= 16 else max(1, 128 // G)
        # per-step slab (doubles): out | H | grad | energy | dp | low | nu | info | t | state | flags | pa | pb
        sizes = [("out", G * osz1), ("hessian", G * n * n), ("grad", G * n), ("energy", G), ("dp", G * n),
                 ("lowest", G), ("shift", G), ("info", G), ("t", G), ("state", 3 * G), ("flags", 4),
                 ("points_a", G * nt), ("points_b", G * nk)]
        offs, o = {}, 0
        for k, sz in sizes:
            offs[k] = (o, sz)
            o += (sz + 1) & ~1                      # (16-byte aligned pieces)
        self._step_args = (b, keep, offs, o, osz0)
        return self._step_args

    def _newton_step_one_call(self, thetas, opt, trial):
        from .newton_raphson import LockstepSearch
        b, keep, offs, total, osz0 = self._step_block()
        G, nt, nk = self.G, self.n_theta, self.n_kappa
        n = nt + nk
        slab = torch.empty(total, dtype=F64, device=self.device)
        base = slab.data_ptr()
        for k, (o, _) in offs.items():
            setattr(b, k, base + 8 * o)
        flags_np = keep["flags_np"]
        flags_np[:] = np.nan
        b.flags = keep["flags_host"].data_ptr()

        def view(k, *shape):
            o, sz = offs[k]
            return slab[o:o + sz].view(*shape)

        t_oao, t_mo = self._trial_orbitals
        b.theta = thetas.data_ptr()
        b.g_ao, b.h_ao, b.nuc = self.int2e_ao.data_ptr(), self.int1e_ao.data_ptr(), self.nuc.data_ptr()
        b.g_packed = (self._eri_packed.data_ptr() if (self.eri_flags == 3 and self._eri_packed is not None)
                      else None)        # (no packed copy exists for M > 16 at N <= 48: _refresh_flags)
        b.eri_flags = int(self.eri_flags)
        b.oao_coeff, b.oao_mo_coeff, b.mo_coeff = (self.oao_coeff.data_ptr(), self.oao_mo_coeff.data_ptr(),
                                                   self.mo_coeff.data_ptr())
        b.trial_oao, b.trial_mo = t_oao.data_ptr(), t_mo.data_ptr()
        b.lambda_min, b.mu, b.rho, b.alpha, b.beta = opt.lambda_min, opt.mu, opt.rho, opt.alpha, opt.beta
        b.aug = int(bool(opt.aug))
        # when the previous step of this stack found every Hessian positive definite, the band route of "the
        # others" is not waited for (it runs beside the trial; flags[1] says whether that was right)
        spec = bool(self._all_pd_last_step)
        b.speculate = int(spec)
        side = ops._side_stream(self.device)
        b.work_rest_side = keep["work_side"][ops.side_streams(self.device).index(side)].data_ptr()
        refused = False
        try:
            check(self.lib.oovqe_oo_newton_step_batch(ctypes.byref(b), stream_ptr(), ctypes.c_void_p(side.cuda_stream)),
                  "oovqe_oo_newton_step_batch")
        except _lib.OovqeError:
            # beyond N = 48 the trial's orbital rotation fails loudly on a direction the library refused (dp = NaN):
            # the search below repeats that direction without inter-workgroup waits / through eigh, or raises
            torch.cuda.current_stream().wait_stream(side)
            if min(slab[offs["info"][0]:offs["info"][0] + G].tolist()) >= 0:
                raise
            refused = True
        event = torch.cuda.Event()
        event.record(side)
        # the side stream's route reads and writes this slab: it stays referenced here until that route's event has
        # completed (a host-side query per step) -- record_stream() on a megabyte block costs the allocator ~35 us at the
        # NEXT torch.empty (event bookkeeping on the critical path of the next step)
        held = self.__dict__.setdefault("_slabs_in_flight", [])
        held[:] = [(sl, ev) for sl, ev in held if not ev.query()]
        held.append((slab, event))
        # (the views are made while the device works through the step, the readback comes last)
        state = view("state", 3, G)
        lam_args = (float(opt.lambda_min), float(opt.mu), float(opt.rho), int(bool(opt.aug)))

        def retry_lowest():
            # eigenvalues the side route could not deliver: again on the calling stream, one workgroup per problem
            check(self.lib.oovqe_newton_direction_rest(
                dptr(view("hessian", G, n, n)), dptr(view("grad", G, n)), n, G, *lam_args, dptr(view("info", G)), 2, 1,
                dptr(keep["work_rest"]), dptr(view("dp", G, n)), dptr(view("lowest", G)), dptr(view("shift", G)),
                stream_ptr()), "oovqe_newton_direction_rest")

        s = LockstepSearch(flat=keep["flat"], g=view("grad", G, n), H=view("hessian", G, n, n), dp=view("dp", G, n),
                           low=ops.PendingLowest(view("lowest", G), event, retry_lowest), nu=view("shift", G),
                           info=view("info", G), energy=view("energy", G), t=view("t", G), active=state[0],
                           best=state[1], slope=state[2], flags=keep["flags_dev"], pa=view("points_a", G, nt),
                           pb=view("points_b", G, nk))
        if refused:
            fl = [1.0, -1.0, 0.0, 0.0]
        else:
            # the verdict of the first trial: polled in pinned memory (falls back to a stream synchronisation should
            # the flags not arrive within seconds -- a failed launch surfaces there)
            t_poll = time.perf_counter()
            while np.isnan(flags_np).any():
                if time.perf_counter() - t_poll > 5.0:
                    torch.cuda.current_stream().synchronize()
                    if np.isnan(flags_np).any():
                        raise _lib.OovqeError("oovqe_oo_newton_step_batch: the step's verdict never arrived")
            fl = flags_np.tolist()
        self._all_pd_last_step = fl[1] >= 1.0
        if refused:
            s.t.fill_(1.0)
            fl = None
        elif spec and fl[1] < 1.0:
            # some Hessian was not positive definite after all: its direction is still on the side stream.  Join it
            # and search from the start.
            torch.cuda.current_stream().wait_event(event)
            s.t.fill_(1.0)
            fl = None
        opt.run_search(s, trial, split=nt, first_flags=fl)
        return s.pa, s.pb, s.low, s.best

