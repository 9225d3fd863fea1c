"""Analytic nuclear gradients of a geometry stack on the device (auto_oo_amd/csrc/gto_grad.hip).

The energy of a batch made by ``OO_pqc_batch.from_geometries`` depends on the nuclear coordinates R through the AO
integrals ``h``, ``g``, the nuclear repulsion, and through ``X = S^-1/2`` (the orbitals are ``C = X U`` with a fixed
OAO-to-MO matrix ``U``).  With the AO densities ``D1``, ``D2`` of the wave function (``cas_ao_densities``) and the
pull-back ``WQ`` of the energy's dependence on ``X`` to the overlap (``overlap_pullback``)

    dE/dR = D1 . dh/dR + 1/2 D2 . dg/dR + WQ . dS/dR + dE_nuc/dR,

exact at any circuit parameters and any ``U``, converged or not; the contraction with the derivative integrals is
``gto.gradient_batch`` (no derivative integral is stored).  Where the orbital gradient vanishes ``WQ`` is minus the
energy-weighted density, which is what ``rhf_gradient`` uses.  The functions ending in ``_host`` are numpy twins of
the device helpers (the oracle of the tests; the product path never calls them).
"""
import numpy as np
import torch

from . import _lib, ops, scf
from ._lib import check, dptr, stream_ptr

F64 = torch.float64
MAX_NCAS = 8


def _t(x):
    return x.transpose(1, 2).contiguous()


def cas_ao_densities(mo_coeff, n_core, ncas, one_rdm=None, two_rdm=None, want_d2=True, out=None):
    """``D1`` [G, N, N] and the 8-fold symmetric ``D2`` [G, N, N, N, N] of a CAS wave function (``E = D1 . h + 1/2 D2 .
    g + nuc``) from orbitals ``mo_coeff`` [G, N, N] (AO x MO: ``n_core`` doubly occupied, then ``ncas`` active) and the
    active RDMs [G, a, a], [G, a, a, a, a] in the convention of the batch (``oovqe_cas_ao_densities_batch``).
    ``ncas = 0``: closed shell.  ``out``: a [>= G, N, N, N, N] tensor to take ``D2``.  -> (D1, D2 or None)."""
    if ncas > 0 and one_rdm is not None and two_rdm is not None and one_rdm.dim() == 4:
        # K sets of RDMs per geometry [G, K, a, a], [G, K, a, a, a, a] -> D1 [G, K, N, N], D2 [G, K, N, N, N, N]: the
        # orbitals repeated per set, every (geometry, set) an entry of the batch
        G, K, N = int(one_rdm.shape[0]), int(one_rdm.shape[1]), int(mo_coeff.shape[-1])
        if tuple(mo_coeff.shape) != (G, N, N) or two_rdm.dim() != 6 or tuple(two_rdm.shape[:2]) != (G, K):
            raise ValueError(f"mo_coeff of shape {tuple(mo_coeff.shape)}, RDM sets of shapes {tuple(one_rdm.shape)}, "
                             f"{tuple(two_rdm.shape)}: expected [G, N, N], [G, K, a, a], [G, K, a, a, a, a]")
        C = mo_coeff[:, None].expand(G, K, N, N).reshape(G * K, N, N)
        d1, d2 = cas_ao_densities(C, n_core, ncas, one_rdm.reshape((G * K,) + tuple(one_rdm.shape[2:])),
                                  two_rdm.reshape((G * K,) + tuple(two_rdm.shape[2:])), want_d2, out)
        return d1.reshape(G, K, N, N), None if d2 is None else d2.reshape(G, K, N, N, N, N)
    lib = _lib.load()
    _lib.require_device()
    C = mo_coeff.contiguous()
    G, N = int(C.shape[0]), int(C.shape[-1])
    if tuple(C.shape) != (G, N, N):
        raise ValueError(f"mo_coeff has shape {tuple(C.shape)}, expected [G, N, N]")
    a = int(ncas)
    if a > 0:
        if one_rdm is None or two_rdm is None:
            raise ValueError("an active space needs its RDMs")
        if tuple(one_rdm.shape) != (G, a, a) or tuple(two_rdm.shape) != (G, a, a, a, a):
            raise ValueError(f"RDMs of shapes {tuple(one_rdm.shape)}, {tuple(two_rdm.shape)}, expected "
                             f"{(G, a, a)}, {(G, a, a, a, a)}")
        one_rdm, two_rdm = one_rdm.contiguous(), two_rdm.contiguous()
    else:
        one_rdm = two_rdm = None
    d1 = torch.empty((G, N, N), dtype=F64, device=C.device)
    d2 = None
    if want_d2:
        d2 = torch.empty((G, N, N, N, N), dtype=F64, device=C.device) if out is None else out[:G]
    check(lib.oovqe_cas_ao_densities_batch(dptr(C), N, int(n_core), a, dptr(one_rdm), dptr(two_rdm), G, dptr(d1),
                                           dptr(d2), stream_ptr()), "oovqe_cas_ao_densities_batch")
    return d1, d2


def overlap_pullback(overlap, oao_mo_coeff, fock):
    """``WQ`` [G, N, N] with ``WQ . dS = `` the change of the energy through ``X = S^-1/2`` at fixed ``U``:
    ``G_X = sym((dE/dC) U^T)`` with ``dE/dC = 2 X^-1 U F^T`` (``F`` the generalised Fock matrix of the CAS path),
    ``S = V diag(s) V^T``, ``WQ = V [K o (V^T G_X V)] V^T``, ``K_ij = -1 / (sqrt(s_i) sqrt(s_j) (sqrt(s_i) +
    sqrt(s_j)))`` (the divided differences of ``s^-1/2``).  N x N work per geometry on the device: the eigensolver of
    the SCF kernels and the batched small products; no matrix passes through the host."""
    if fock.dim() == 4:
        # K Fock matrices per geometry [G, K, N, N] -> WQ [G, K, N, N]: overlap and U repeated per set (WQ is linear in F)
        G, K, N = int(fock.shape[0]), int(fock.shape[1]), int(fock.shape[-1])
        rep = lambda x: x[:, None].expand(G, K, N, N).reshape(G * K, N, N)
        return overlap_pullback(rep(overlap), rep(oao_mo_coeff), fock.reshape(G * K, N, N)).reshape(G, K, N, N)
    w, V, _ = scf.sym_eigh_batch(overlap.contiguous())
    mm = ops.matmul_nn_batch
    sq = torch.sqrt(w)
    Vt = _t(V)
    U = oao_mo_coeff.contiguous()
    x_inv = mm((V * sq[:, None, :]).contiguous(), Vt)
    de_dc = 2.0 * mm(mm(x_inv, U), _t(fock))
    gx = mm(de_dc, _t(U))
    gx = 0.5 * (gx + gx.transpose(1, 2))
    return _pull_back(gx, sq, V, Vt)


def _pull_back(gx, sq, V, Vt):
    """``V [K o (V^T G_X V)] V^T``, symmetrised: a symmetric ``G_X = d./dX`` [G, N, N] pulled back to the overlap
    ``S = V diag(sq^2) V^T``."""
    mm = ops.matmul_nn_batch
    m = mm(mm(Vt, gx.contiguous()), V)
    k = -1.0 / (sq[:, :, None] * sq[:, None, :] * (sq[:, :, None] + sq[:, None, :]))
    wq = mm(mm(V, (k * m).contiguous()), Vt)
    return (0.5 * (wq + wq.transpose(1, 2))).contiguous()


def connection_pullback(overlap, oao_mo_coeff, a):
    """``WQc`` [G, N, N] with ``WQc . dS = sum_pq a_pq (U^T X^-1 dX U)_pq``, the part of the orbital connection
    ``<phi_p|d phi_q>`` of ``C = X U`` that comes from ``X = S^-1/2`` at fixed ``U``, contracted with ``a`` [G, N, N]
    in the MO basis (for a derivative coupling the antisymmetric part of a transition 1-RDM, zero outside the active
    block): ``G_X = sym(X^-1 U a U^T)`` -- which does not vanish for antisymmetric ``a``, since ``X^-1`` stands on one
    side only -- pulled back to the overlap with the divided differences of ``overlap_pullback``.  ``a`` [G, K, N, N]:
    K sets per geometry -> [G, K, N, N]."""
    if a.dim() == 4:
        G, K, N = int(a.shape[0]), int(a.shape[1]), int(a.shape[-1])
        rep = lambda x: x[:, None].expand(G, K, N, N).reshape(G * K, N, N)
        return connection_pullback(rep(overlap), rep(oao_mo_coeff), a.reshape(G * K, N, N)).reshape(G, K, N, N)
    w, V, _ = scf.sym_eigh_batch(overlap.contiguous())
    mm = ops.matmul_nn_batch
    sq = torch.sqrt(w)
    Vt = _t(V)
    U = oao_mo_coeff.contiguous()
    x_inv = mm((V * sq[:, None, :]).contiguous(), Vt)
    gx = mm(mm(x_inv, U), mm(a.contiguous(), _t(U)))
    gx = 0.5 * (gx + gx.transpose(1, 2))
    return _pull_back(gx, sq, V, Vt)


def energy_weighted_pullback(mo_coeff, mo_energy, n_occ):
    """``WQ = -2 C_o diag(eps_o) C_o^T`` [G, N, N]: what ``overlap_pullback`` reduces to for converged closed-shell
    orbitals."""
    Co = mo_coeff[:, :, :n_occ]
    left = (Co * mo_energy[:, None, :n_occ]).contiguous()
    wq = -2.0 * ops.matmul_nn_batch(left, _t(Co))
    return (0.5 * (wq + wq.transpose(1, 2))).contiguous()


def rhf_gradient(basis, coords_bohr, mo_coeff, mo_energy, n_occ):
    """Closed-shell gradient [G, natm, 3] (Hartree / Bohr) from converged RHF orbitals: ``D = 2 C_o C_o^T``, the
    closed-shell ``D2`` and ``WQ = -2 C_o eps_o C_o^T``."""
    from . import gto
    d1, d2 = cas_ao_densities(mo_coeff, n_occ, 0)
    wq = energy_weighted_pullback(mo_coeff, mo_energy, n_occ)
    return gto.gradient_into(basis, coords_bohr, d1, wq, d2, True)


# ---- several states of one geometry --------------------------------------------------------------------------------
def state_pairs(nroots):
    """The pairs (I, J), I > J, of ``nroots`` states in the order of the interstate sets: (1, 0), (2, 0), (2, 1), ...;
    with the ``nroots`` states in front of them, ``nroots (nroots + 1) / 2`` sets."""
    return [(i, j) for i in range(int(nroots)) for j in range(i)]


def polarisation_vectors(vecs):
    """CI vectors [G, R, Dc] -> [G, R + 2 P, Dc]: the R vectors, then ``(c_I + c_J) / sqrt 2`` for the P pairs of
    ``state_pairs``, then ``(c_I - c_J) / sqrt 2``.  RDMs, AO densities and the Fock matrix are quadratic forms of the
    vector, so half the difference of a ``+`` and a ``-`` quantity is the symmetrised transition quantity ``(<I|.|J> +
    <J|.|I>) / 2``; whatever does not depend on the vector (the core-only parts, the nuclear term) drops out exactly."""
    pairs = state_pairs(vecs.shape[1])
    if not pairs:
        return vecs
    ii = torch.as_tensor([p[0] for p in pairs], dtype=torch.long, device=vecs.device)
    jj = torch.as_tensor([p[1] for p in pairs], dtype=torch.long, device=vecs.device)
    r2 = 0.5 ** 0.5
    return torch.cat((vecs, r2 * (vecs[:, ii] + vecs[:, jj]), r2 * (vecs[:, ii] - vecs[:, jj])), dim=1)


def transition_sets(x, nroots):
    """``x`` [G, R + 2 P, ...] of the vectors of ``polarisation_vectors`` -> [G, R + P, ...]: the R state quantities,
    then the P half-differences ``(x_+ - x_-) / 2``."""
    R, P = int(nroots), len(state_pairs(nroots))
    if P == 0:
        return x.contiguous()
    return torch.cat((x[:, :R], 0.5 * (x[:, R:R + P] - x[:, R + P:])), dim=1).contiguous()


def branching_plane(result, i, j):
    """The two vectors that span the branching plane of states i and j from a result of
    ``OO_pqc_batch.casci_nuclear_gradients`` (anything with ``gradients`` [G, R, R, natm, 3]) -> ``(g, h)``, each
    [G, natm, 3]: the gradient half-difference ``g = (G_jj - G_ii) / 2`` and the interstate coupling ``h = G_ij``."""
    grads = result.gradients
    R = int(grads.shape[1])
    i, j = int(i), int(j)
    if not (0 <= i < R and 0 <= j < R) or i == j:
        raise ValueError(f"states i = {i}, j = {j}: two different states of 0..{R - 1}")
    return 0.5 * (grads[:, j, j] - grads[:, i, i]), grads[:, i, j]


# ---- numpy twins (tests) ----------------------------------------------------------------------------------------------
def sym8_host(t):
    """Average of a [N, N, N, N] array over the 8 index permutations of (pq|rs)."""
    t = 0.5 * (t + t.transpose(1, 0, 2, 3))
    t = 0.5 * (t + t.transpose(0, 1, 3, 2))
    return 0.5 * (t + t.transpose(2, 3, 0, 1))


def cas_ao_densities_host(mo_coeff, n_core, ncas, one_rdm=None, two_rdm=None):
    """numpy twin of ``cas_ao_densities`` for ONE geometry, written from the definition in the header."""
    C = np.asarray(mo_coeff)
    Cc, Ca = C[:, :n_core], C[:, n_core:n_core + ncas]
    Dc = 2.0 * Cc @ Cc.T
    e = np.einsum
    d2 = e("pq,rs->pqrs", Dc, Dc) - 0.5 * e("pr,qs->pqrs", Dc, Dc)
    Da = np.zeros_like(Dc)
    if ncas > 0:
        Da = Ca @ np.asarray(one_rdm) @ Ca.T
        d2 = d2 + 2.0 * (e("pq,rs->pqrs", Dc, Da) - 0.5 * e("pr,qs->pqrs", Dc, Da))
        d2 = d2 + e("tuvw,pt,qu,rv,sw->pqrs", np.asarray(two_rdm), Ca, Ca, Ca, Ca, optimize=True)
    d1 = Dc + Da
    return 0.5 * (d1 + d1.T), sym8_host(d2)


def overlap_pullback_host(overlap, g_x):
    """numpy twin of the last step of ``overlap_pullback`` for ONE geometry: ``WQ`` from a symmetric ``G_X = dE/dX``."""
    s, V = np.linalg.eigh(np.asarray(overlap))
    sq = np.sqrt(s)
    k = -1.0 / (sq[:, None] * sq[None, :] * (sq[:, None] + sq[None, :]))
    g_x = 0.5 * (g_x + g_x.T)
    return V @ (k * (V.T @ g_x @ V)) @ V.T


def connection_pullback_host(overlap, oao_mo_coeff, a):
    """numpy twin of ``connection_pullback`` for ONE geometry: ``G_X = X^-1 U a U^T`` (``overlap_pullback_host``
    symmetrises it)."""
    s, V = np.linalg.eigh(np.asarray(overlap))
    U = np.asarray(oao_mo_coeff)
    x_inv = (V * np.sqrt(s)) @ V.T
    return overlap_pullback_host(overlap, x_inv @ U @ np.asarray(a) @ U.T)
