"""Exact active-space solutions: batched determinant CI (``oovqe_ci_davidson_batch``, ci.hip) and the
``run_fci`` / ``run_casci`` / ``run_casscf`` / ``run_sa_casscf`` methods of ``Moldata``
(the reference's ``moldata_pyscf.py:63-105``).

CI vectors are in the sector layout of the circuit engine: ``c[ia * nb + ib]`` over the alpha and beta
strings of ``sector.string_tables`` (ascending by value, orbital p at bit ncas - 1 - p) with the signs of
the interleaved spin-orbital ordering, so a CI vector can be handed to the sector RDM kernels or overlapped
with a circuit state.  This is NOT PySCF's string order or sign convention.
"""
import ctypes
from collections import namedtuple
from math import comb
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, ops
from ._lib import check, dptr, stream_ptr
from .sector import string_tables

F64 = torch.float64
MAX_NCAS = 8
MAX_DET = 4900
MAX_ROOTS = 4

SPIN_SHIFT = 1.0            # the S^2 penalty a fix_singlet solve starts with
MAX_SPIN_SHIFT = 64.0       # ... and the largest one tried
S2_TOL = 1e-6               # |<S^2>| below which a root counts as a singlet

CIResult = namedtuple("CIResult", "energies ci s2 converged rnorm info shift")


def ci_dimension(ncas, nelecas):
    """Number of determinants of the (N_alpha = N_beta) sector."""
    return comb(int(ncas), int(nelecas) // 2) ** 2


def check_scope(ncas, nelecas, nroots=1):
    """ValueError for a problem outside the solver's scope (before anything is launched)."""
    ncas, nelecas, nroots = int(ncas), int(nelecas), int(nroots)
    if not 1 <= ncas <= MAX_NCAS:
        raise ValueError(f"CI solver: ncas = {ncas} outside 1..{MAX_NCAS}")
    if nelecas < 0 or nelecas > 2 * ncas or nelecas % 2:
        raise ValueError(f"CI solver: nelecas = {nelecas} must be even and in 0..2 ncas (N_alpha = N_beta)")
    dc = ci_dimension(ncas, nelecas)
    if dc > MAX_DET:
        raise ValueError(f"CI solver: {dc} determinants > {MAX_DET} (CAS(8e,8o))")
    if not 1 <= nroots <= min(MAX_ROOTS, dc):
        raise ValueError(f"CI solver: nroots = {nroots} outside 1..{min(MAX_ROOTS, dc)}")
    return dc


def singlet_count(ncas, nelecas):
    """Number of singlets among the determinants of the sector (Weyl's dimension formula at S = 0)."""
    a, n = int(ncas), int(nelecas) // 2
    return comb(a + 1, n) * comb(a + 1, n + 1) // (a + 1)


def _launch(coef, c1_offset, a, nelecas, nroots, shift, tol, max_iter, B):
    """One ``oovqe_ci_davidson_shift_batch`` launch on the first B rows of ``coef``."""
    lib = _lib.load()
    dc = ci_dimension(a, nelecas)
    dev = coef.device
    e = torch.empty((B, nroots), dtype=F64, device=dev)
    ci = torch.empty((B, nroots, dc), dtype=F64, device=dev)
    s2 = torch.empty((B, nroots), dtype=F64, device=dev)
    rn = torch.empty((B, nroots), dtype=F64, device=dev)
    info = torch.empty(B, dtype=torch.int32, device=dev)
    nw = int(lib.oovqe_ci_work_size(a, int(nelecas), int(nroots), B))
    if nw < 0:
        check(nw, "oovqe_ci_work_size")
    work = torch.empty(max(nw, 1), dtype=F64, device=dev)
    p0 = coef.data_ptr()
    p1 = p0 + 8 * int(c1_offset)
    check(lib.oovqe_ci_davidson_shift_batch(a, int(nelecas), int(nroots), B, ctypes.c_void_p(p0),
                                            ctypes.c_void_p(p1), ctypes.c_void_p(p1 + 8 * a * a),
                                            int(coef.stride(0)), float(shift), float(tol), int(max_iter), dptr(e),
                                            dptr(ci), dptr(s2), dptr(rn), dptr(info, torch.int32), dptr(work),
                                            stream_ptr()), "oovqe_ci_davidson_shift_batch")
    return e, ci, s2, rn, info


def _solve_packed(coef, c1_offset, ncas, nelecas, nroots, fix_singlet, tol, max_iter, count):
    """``casci_packed`` and the spin shift each problem was solved with, [B]."""
    check_scope(ncas, nelecas, nroots)
    B = coef.shape[0] if count is None else int(count)
    a, nroots = int(ncas), int(nroots)
    if coef.dtype != F64 or not coef.is_cuda or coef.stride(1) != 1:
        raise ValueError("coef must be a row-major fp64 device tensor")
    if not 0 <= B <= coef.shape[0]:
        raise ValueError(f"count = {B} outside the {coef.shape[0]} rows of coef")
    lam = SPIN_SHIFT if fix_singlet else 0.0
    out = _launch(coef, c1_offset, a, nelecas, nroots, lam, tol, max_iter, B)
    shift = torch.full((B,), lam, dtype=F64, device=coef.device)
    if not fix_singlet or B == 0:
        return out + (shift,)
    e, ci, s2, rn, info = out
    want = min(nroots, singlet_count(a, nelecas))
    while lam < MAX_SPIN_SHIFT:
        # Solved again, together, with the shift doubled: converged problems whose lowest roots are not all
        # singlets (a state of higher spin lies more than lam S (S + 1) below one of them), and problems that stopped
        # short of max_iter (a lifted state lies at a root, the Ritz vectors mix the two and the residual of H does
        # not fall).  A solve that ran out of iterations is left as it is.
        few = (s2.abs() < S2_TOL).sum(1) < want
        redo = torch.nonzero(((info == 0) & few) | ((info > 0) & (info < max_iter))).flatten()
        if redo.numel() == 0:
            break
        lam *= 2.0
        sub = _launch(coef[:B][redo].contiguous(), c1_offset, a, nelecas, nroots, lam, tol, max_iter, redo.numel())
        for full, part in zip((e, ci, s2, rn, info), sub):
            full[redo] = part
        shift[redo] = lam
    if want < nroots:
        # fewer singlets than roots: the singlets first, then the other states, each group in its order
        order = torch.argsort((s2.abs() >= S2_TOL).to(torch.int8), dim=1, stable=True)
        e, s2, rn = (torch.gather(t, 1, order) for t in (e, s2, rn))
        ci = torch.gather(ci, 1, order[:, :, None].expand_as(ci))
    return e, ci, s2, rn, info, shift


def casci_packed(coef, c1_offset, ncas, nelecas, nroots=1, fix_singlet=True, tol=1e-9, max_iter=200, count=None):
    """CI of the problems whose coefficients sit in the rows of ``coef`` [B, stride] (device fp64, rows contiguous
    in memory one ``coef.stride(0)`` apart): c0 at column 0, c1 [a, a] at ``c1_offset``, c2 [a, a, a, a] right
    behind c1 -- the layout of ``oovqe_cas_eval_batch``'s packed outputs.  ``count``: solve the first ``count`` rows
    only.  ONE launch for all rows; with ``fix_singlet`` one more for those rows, if any, whose roots came out with
    a state of higher spin among them (see ``casci``), which costs one device-to-host read of a flag.
    -> energies, ci, s2, rnorm, info as in ``casci``."""
    return _solve_packed(coef, c1_offset, ncas, nelecas, nroots, fix_singlet, tol, max_iter, count)[:5]


def casci(c0, c1, c2, ncas, nelecas, nroots=1, fix_singlet=True, tol=1e-9, max_iter=200):
    """Lowest ``nroots`` eigenpairs of H = c0 + c1 . E + c2 . (E E - E) (``c2 = g / 2``, the convention of
    ``molecular_hamiltonian_coefficients``: E = c0 + c1.gamma + c2.Gamma) in the N_alpha = N_beta sector.

    Batched over a leading dimension: c0 [B] (or scalar), c1 [B, a, a], c2 [B, a, a, a, a]; unbatched inputs give
    B = 1.  c1 and c2 need no index symmetry: H is that of the coefficients averaged over c1_pq <-> c1_qp and
    c2_pqrs <-> c2_rspq, c2_qpsr, c2_srqp, which leaves c0 + c1.gamma + c2.Gamma of every real state unchanged.

    ``fix_singlet=False``: the lowest eigenpairs of H in the whole sector, whatever their spin.

    ``fix_singlet=True``: the lowest SINGLET eigenpairs.  The solver iterates on H + shift S^2, which lifts a state
    of spin S by shift S (S + 1); it starts at shift = 1, and a problem whose roots hold fewer than
    min(nroots, number of singlets) states with |<S^2>| < 1e-6, or whose solve stopped short of ``max_iter``
    without converging (a lifted state sits on a root), is solved again with the shift doubled, up to shift = 64.
    When that bound is reached the roots are returned as they are and ``s2`` shows which are not singlets;
    ``run_casscf`` / ``run_sa_casscf`` raise on such a root.  The energies are <H>, without the penalty.  A sector with fewer singlets than ``nroots`` (only CAS(2e,2o) with nroots = 4: 3 singlets of 4
    determinants) returns the singlets first, in ascending order, and then the lowest remaining states of
    H + shift S^2, in ascending order of that operator, with their <S^2> in ``s2``.

    ``tol``: a problem counts as converged when, for every root, the residual norm |H c - E c| is below ``tol``,
    and with ``fix_singlet`` that of H + shift S^2 as well; ``rnorm`` is the larger of the two where both were
    evaluated (at acceptance) and the residual norm of the operator iterated on otherwise.  Converged therefore
    means: each energy lies within ``rnorm`` of an eigenvalue of H.  The guess space holds a vector with a
    component on every determinant, so that no eigenvector is out of reach by symmetry; that a converged root is
    the k-th LOWEST is nevertheless what a Davidson iteration finds in practice, not what it can prove.

    -> CIResult(energies [B, nroots], ci [B, nroots, Dc] (sector layout, orthonormal, the largest |component| of
    each vector positive), s2 [B, nroots] (<S^2>), converged [B] bool, rnorm [B, nroots], info [B] int32,
    shift [B]).  Unconverged problems are reported through ``converged`` / ``info`` (> 0: iterations done), not
    hidden, and one that used all ``max_iter`` iterations is not solved again with another shift; invalid input
    raises."""
    check_scope(ncas, nelecas, nroots)
    a = int(ncas)
    dev = _lib.require_device()
    c1 = torch.as_tensor(c1, dtype=F64).to(dev).reshape(-1, a * a)
    c2 = torch.as_tensor(c2, dtype=F64).to(dev).reshape(-1, a ** 4)
    B = c1.shape[0]
    c0 = torch.as_tensor(c0, dtype=F64).to(dev).reshape(-1).expand(B)
    if c2.shape[0] != B:
        raise ValueError(f"c1 holds {B} problems, c2 {c2.shape[0]}")
    coef = torch.cat((c0[:, None], c1, c2), dim=1).contiguous()
    e, ci, s2, rn, info, shift = _solve_packed(coef, 1, a, nelecas, nroots, fix_singlet, tol, max_iter, None)
    return CIResult(e, ci, s2, info == 0, rn, info, shift)


# ---- RDMs of CI vectors (the sector engine's kernel) ---------------------------------------------------------
def sector_rdms(vecs, ncas, nelecas):
    """gamma [n, a, a], Gamma [n, a, a, a, a] of sector vectors vecs [n, Dc] (``oovqe_sector_rdms_tb``)."""
    lib = _lib.load()
    a, n_s = int(ncas), int(nelecas) // 2
    ua, ra = string_tables(a, n_s)
    dev = vecs.device
    un = torch.as_tensor(ua.astype(np.int32)).to(dev)
    rk = torch.as_tensor(ra).to(dev)
    na = len(ua)
    vecs = vecs.reshape(-1, na * na).contiguous()
    n = vecs.shape[0]
    gamma = torch.empty((n, a, a), dtype=F64, device=dev)
    Gamma = torch.empty((n, a, a, a, a), dtype=F64, device=dev)
    work = torch.empty(int(lib.oovqe_sector_work_size(a, na, na, n)), dtype=F64, device=dev)
    i32 = torch.int32
    check(lib.oovqe_sector_rdms_tb(dptr(vecs), a, dptr(un, i32), dptr(un, i32), dptr(rk, i32), dptr(rk, i32), na,
                                   na, n, None, dptr(gamma), dptr(Gamma), dptr(work), stream_ptr()),
          "oovqe_sector_rdms_tb")
    return gamma, Gamma


def transition_rdm1(bra, ket, ncas, nelecas):
    """Spin-summed transition 1-RDMs ``gamma[n, p, q] = <bra_n| E_pq |ket_n>`` [n, a, a] of pairs of sector vectors
    bra, ket [n, Dc] (``oovqe_sector_transition_rdm1``, csrc/sector_trdm.hip).  NOT symmetric in (p, q) for different
    vectors and not symmetrised: ``gamma[n].T`` is the matrix with bra and ket exchanged.  Equal vectors give the gamma
    of ``sector_rdms``.  The scope is ``check_scope``'s; a pair's matrix has the same bits whatever the other pairs."""
    a = int(ncas)
    dc = check_scope(a, nelecas)
    lib = _lib.load()
    ua, ra = string_tables(a, int(nelecas) // 2)
    na = len(ua)
    if not isinstance(bra, torch.Tensor) or not isinstance(ket, torch.Tensor) or not bra.is_cuda:
        raise ValueError("bra and ket must be device tensors")
    if bra.shape != ket.shape or bra.dim() < 1 or int(bra.shape[-1]) != dc:
        raise ValueError(f"bra of shape {tuple(bra.shape)}, ket of shape {tuple(ket.shape)}: expected two [n, {dc}]")
    dev = bra.device
    bra = bra.to(F64).reshape(-1, dc).contiguous()
    ket = ket.to(device=dev, dtype=F64).reshape(-1, dc).contiguous()
    n = int(bra.shape[0])
    gamma = torch.empty((n, a, a), dtype=F64, device=dev)
    if n == 0:
        return gamma
    un = torch.as_tensor(ua.astype(np.int32)).to(dev)
    rk = torch.as_tensor(ra).to(dev)
    i32 = torch.int32
    check(lib.oovqe_sector_transition_rdm1(dptr(bra), dptr(ket), a, dptr(un, i32), dptr(un, i32), dptr(rk, i32),
                                           dptr(rk, i32), na, na, n, dptr(gamma), stream_ptr()),
          "oovqe_sector_transition_rdm1")
    return gamma


# ---- the reference's solver methods ---------------------------------------------------------------------------
def _need_orbitals(mol):
    mol.run_rhf()            # (raises the RuntimeError of run_rhf when the container has no orbitals)
    return np.asarray(mol.hf.mo_coeff, dtype=np.float64)


def _active_coefficients(mol, mo, ncas, nelecas, dev):
    """(c0, c1, c2) of the active space at AO->MO orbitals ``mo`` (device transforms)."""
    from .active_space import molecular_hamiltonian_coefficients
    from .oo_energy import int1e_transform, int2e_transform
    C = ops.as_device(mo, dev)
    h = int1e_transform(ops.as_device(mol.int1e_ao, dev), C)
    g = int2e_transform(ops.as_device(mol.int2e_ao, dev), C)
    occ, act, _ = mol.get_active_space_idx(ncas, nelecas)
    return molecular_hamiltonian_coefficients(mol.nuc, h, g, occ, act)


def _result(e, ci_vecs, s2, conv, na, nroots, mo, **extra):
    e = e.detach().cpu().numpy()
    vecs = ci_vecs.detach().cpu().numpy().reshape(nroots, na, na)
    out = SimpleNamespace(e_tot=float(e[0]) if nroots == 1 else e.copy(),
                          ci=vecs[0] if nroots == 1 else [v for v in vecs],
                          s2=s2.detach().cpu().numpy(), converged=bool(conv), mo_coeff=mo, **extra)
    return out


def run_casci(mol, ncas, nelecas, n_roots=1, mo=None, fix_singlet=1, verbose=0):
    check_scope(ncas, nelecas, n_roots)
    mo = _need_orbitals(mol) if mo is None else np.asarray(mo, dtype=np.float64)
    dev = _lib.require_device()
    c0, c1, c2 = _active_coefficients(mol, mo, ncas, nelecas, dev)
    res = casci(c0, c1, c2, ncas, nelecas, n_roots, bool(fix_singlet))
    na = comb(int(ncas), int(nelecas) // 2)
    out = _result(res.energies[0], res.ci[0], res.s2[0], res.converged[0].item(), na, n_roots, mo,
                  ncas=ncas, nelecas=nelecas)
    if verbose:
        print(f"CASCI({nelecas}e,{ncas}o) E = {out.e_tot}")
    return out


def _casscf(mol, ncas, nelecas, weights, fix_singlet, verbose, max_macro=100, e_tol=1e-10, g_tol=1e-6):
    """Two-step CASSCF: CASCI at the current orbitals, RDMs of the (weighted) roots, damped Newton steps of the
    orbitals with the orbital gradient / Hessian of ``OO_energy`` (active-active rotations frozen)."""
    from .newton_raphson import NewtonStep
    from .oo_energy import OO_energy, mo_ao_to_mo_oao
    nroots = len(weights)
    check_scope(ncas, nelecas, nroots)
    mo = _need_orbitals(mol)
    oo = OO_energy(mol, ncas, nelecas, oao_mo_coeff=mo_ao_to_mo_oao(mo, mol.overlap), freeze_active=True)
    dev = oo.device
    w = torch.as_tensor(weights, dtype=F64, device=dev)
    opt = NewtonStep(verbose=0)
    e_prev, conv = None, False
    for it in range(max_macro):
        c0, c1, c2 = oo.get_active_integrals(oo.mo_coeff)
        res = casci(c0, c1, c2, ncas, nelecas, nroots, bool(fix_singlet))
        if not bool(res.converged.all()):
            raise RuntimeError(f"CASSCF: CASCI did not converge (residuals {res.rnorm.tolist()})")
        if fix_singlet and not bool((res.s2.abs() < S2_TOL).all()):
            raise RuntimeError(f"CASSCF: a root is not a singlet (<S^2> = {res.s2.tolist()}, spin shift "
                               f"{res.shift.tolist()}): it is not averaged into the energy")
        g1s, g2s = sector_rdms(res.ci[0], ncas, nelecas)
        g1 = (w[:, None, None] * g1s).sum(0)
        g2 = (w.reshape(-1, 1, 1, 1, 1) * g2s).sum(0)
        e = float((w * res.energies[0]).sum())
        grad = oo.kappa_matrix_to_vector(oo.analytic_gradient(g1, g2))
        gnorm = float(torch.linalg.norm(grad)) if grad.numel() else 0.0
        if verbose:
            print(f"CASSCF macro {it:03d}: E = {e:.12f}  |g_orb| = {gnorm:.3e}")
        if e_prev is not None and abs(e - e_prev) < e_tol and gnorm < g_tol:
            conv = True
            break
        if grad.numel() == 0:
            conv = True
            break
        e_prev = e
        hess = oo.analytic_hessian_matrix(g1, g2)
        kappa0 = torch.zeros(oo.n_kappa, dtype=F64, device=dev)

        def objective(kappa, g1=g1, g2=g2):
            return oo.energy_from_kappa(kappa, g1, g2)
        kappa, _ = opt.damped_newton_step(objective, (kappa0,), grad, hess)
        oo.oao_mo_coeff = ops.matmul_nn(oo._t(oo.oao_mo_coeff), oo.kappa_to_mo_coeff(kappa))
    mo_fin = oo.mo_coeff.detach().cpu().numpy()
    return res, e, conv, mo_fin, gnorm


def run_casscf(mol, ncas, nelecas, fix_singlet=1, verbose=0):
    res, e, conv, mo, gnorm = _casscf(mol, ncas, nelecas, [1.0], fix_singlet, verbose)
    na = comb(int(ncas), int(nelecas) // 2)
    return _result(res.energies[0], res.ci[0], res.s2[0], conv, na, 1, mo, ncas=ncas, nelecas=nelecas,
                   orbital_gradient_norm=gnorm)


def run_sa_casscf(mol, ncas, nelecas, fix_singlet=1, verbose=0):
    weights = [0.5, 0.5]
    res, e, conv, mo, gnorm = _casscf(mol, ncas, nelecas, weights, fix_singlet, verbose)
    na = comb(int(ncas), int(nelecas) // 2)
    out = _result(res.energies[0], res.ci[0], res.s2[0], conv, na, 2, mo, ncas=ncas, nelecas=nelecas,
                  weights=np.array(weights), orbital_gradient_norm=gnorm)
    out.e_states = np.asarray(out.e_tot)
    out.e_tot = float(np.dot(weights, out.e_states))
    return out
