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
import ctypes
from collections import namedtuple

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


# ---- orbital response of CASCI states on canonical RHF orbitals (auto_oo_amd/csrc/zvector.hip) ------------------------
ZVector = namedtuple("ZVector", "z info iterations residual")
Z_INFO = {1: "max_iter reached", -2: "p^T A p <= 0: unstable RHF solution", -3: "NaN or Inf in the inputs",
          -4: "orbital-energy gap below min_gap"}


def orbital_gradient(fock):
    """``w_pq = dE/dkappa_pq = 2 (F_qp - F_pq)``, p > q, of the rotation ``C exp(kappa)`` from the generalised Fock
    matrix ``F`` [..., N, N] of the CAS path (``dE/dC = C^-T 2 F^T``) -> [..., N, N], the strictly lower triangle
    filled."""
    return torch.tril(2.0 * (fock.transpose(-1, -2) - fock), -1).contiguous()


def _per_set(x, K):
    """[G, N, M] -> [G K, N, M]: a geometry's matrix repeated for its K sets."""
    G = int(x.shape[0])
    return x[:, None].expand((G, K) + tuple(x.shape[1:])).reshape((G * K,) + tuple(x.shape[1:])).contiguous()


def _mo_to_ao(C, m):
    """``C m C^T`` for C [G, N, N], m [G, K, N, N] -> [G, K, N, N]"""
    G, K, N = int(m.shape[0]), int(m.shape[1]), int(m.shape[-1])
    Ck = _per_set(C, K)
    return ops.matmul_nn_batch(ops.matmul_nn_batch(Ck, m.reshape(G * K, N, N).contiguous()), _t(Ck)).view(G, K, N, N)


def _g_sets(int2e, dms):
    J, K = scf.fock_jk_sets(int2e, dms)
    return J - 0.5 * K


def zvector(int2e, mo_coeff, mo_energy, n_core, ncas, n_occ, w, tol=1e-10, max_iter=100, min_gap=1e-6):
    """The Z-vector of K states per geometry: ``L^T z = w`` over the orbital pairs of ``response_pairs`` (see
    ``zvector_host``), for canonical RHF orbitals ``mo_coeff`` [G, N, N] with energies ``mo_energy`` [G, N] (``n_occ``
    doubly occupied; the CASCI has ``n_core`` inactive and ``ncas`` active orbitals), the integrals ``int2e`` and the
    orbital gradients ``w`` [G, K, N, N] of ``orbital_gradient``.  Block elimination: the pairs inside occ-occ and
    virt-virt are ``z_pq = w_pq / (eps_p - eps_q)``; their density ``Z_d = C zt_d C^T`` (``zt`` symmetric, ``zt_pq =
    z_pq / 2``) gives the right-hand side ``b_ai = w_ai - 4 [C^T G[Z_d] C]_ai`` of the symmetric virt-occ system,
    which ``oovqe_zvector_solve_batch`` solves by preconditioned conjugate gradients to a residual 2-norm ``tol``.

    -> ``ZVector(z [G, K, N, N] (strictly lower triangle), info [G, K], iterations [G, K], residual [G, K])`` on the
    device.  ``info``: 0, or a key of ``Z_INFO``; -4 marks every state of a geometry with a pair of step one closer
    than ``min_gap``.  ``z`` of a state with a negative code is NaN; nothing is read back."""
    if w.dim() != 4:
        raise ValueError(f"w has shape {tuple(w.shape)}, expected [G, K, N, N]")
    G, K, N = int(w.shape[0]), int(w.shape[1]), int(w.shape[-1])
    vo, dg = response_pairs(N, n_core, ncas, n_occ)
    if tuple(mo_coeff.shape) != (G, N, N) or tuple(mo_energy.shape) != (G, N):
        raise ValueError(f"mo_coeff of shape {tuple(mo_coeff.shape)}, mo_energy of shape {tuple(mo_energy.shape)}: "
                         f"expected {(G, N, N)}, {(G, N)}")
    if not (tol > 0 and int(max_iter) >= 1):
        raise ValueError(f"tol = {tol}, max_iter = {max_iter}")
    lib = _lib.load()
    dev = _lib.require_device()
    C, eps, w = mo_coeff.contiguous(), mo_energy.contiguous(), w.contiguous()
    no, nv = int(n_occ), N - int(n_occ)
    # pairs inside occ-occ and virt-virt
    delta = (eps[:, :, None] - eps[:, None, :])[:, None]
    mask = torch.as_tensor(dg, device=dev)
    small = ((delta.abs() < float(min_gap)) & mask).flatten(1).any(dim=1)               # [G]
    use = mask & ~small[:, None, None, None]
    zd = torch.where(use, w / torch.where(use, delta, torch.ones_like(delta)), torch.zeros_like(w))
    # right-hand side of the virt-occ block
    Zd = _mo_to_ao(C, 0.5 * (zd + zd.transpose(2, 3)))
    Ck = _per_set(C, K)
    gz = ops.matmul_nn_batch(ops.matmul_nn_batch(_t(Ck), _g_sets(int2e, Zd).reshape(G * K, N, N)), Ck).view(G, K, N, N)
    b = (w - 4.0 * gz)[:, :, no:, :no].contiguous()
    size = int(lib.oovqe_zvector_work_size(N, no, K, G))
    if size < 0:
        check(size, "oovqe_zvector_work_size")
    work = torch.empty(size, dtype=F64, device=dev)
    zvo = torch.empty((G, K, nv, no), dtype=F64, device=dev)
    resid = torch.empty((G, K), dtype=F64, device=dev)
    iters = torch.empty((G, K), dtype=torch.int32, device=dev)
    info = torch.empty((G, K), dtype=torch.int32, device=dev)
    verdict = scf._verdict_words(dev)
    check(lib.oovqe_zvector_solve_batch(dptr(int2e.contiguous()), dptr(C), dptr(eps), N, no, K, G, dptr(b), float(tol),
                                        int(max_iter), dptr(zvo), dptr(resid), dptr(iters, torch.int32),
                                        dptr(info, torch.int32), dptr(work), ctypes.c_void_p(verdict.data_ptr()),
                                        stream_ptr()), "oovqe_zvector_solve_batch")
    z = zd
    z[:, :, no:, :no] = zvo
    nan = torch.full_like(z, float("nan"))
    info = torch.where(small[:, None], torch.full_like(info, -4), info)
    z = torch.where((info < 0)[:, :, None, None], nan, z)
    return ZVector(z, info, iters, resid)


def response_d2(Z, D0, d2):
    """``d2 -= sym8[2 Z_pq D0_rs - Z_pr D0_qs]`` in place for symmetric ``Z``, ``D0`` [rows, N, N] and an 8-fold
    symmetric ``d2`` [rows, N, N, N, N] (``oovqe_response_d2_batch``) -> ``d2``.  Each ``d2[row]`` must be contiguous;
    the rows may lie any distance apart (a view ``x[:, k]`` of a [rows, K, N, N, N, N] tensor serves)."""
    rows, N = int(d2.shape[0]), int(d2.shape[-1])
    if tuple(d2.shape) != (rows,) + (N,) * 4 or tuple(Z.shape) != (rows, N, N) or tuple(D0.shape) != (rows, N, N):
        raise ValueError(f"Z, D0, d2 of shapes {tuple(Z.shape)}, {tuple(D0.shape)}, {tuple(d2.shape)}: expected "
                         "[rows, N, N] twice and [rows, N, N, N, N]")
    if tuple(d2.stride()[1:]) != (N ** 3, N ** 2, N, 1) or (rows > 1 and d2.stride(0) < N ** 4) or not d2.is_cuda \
            or d2.dtype != F64:
        raise ValueError("every d2[row] must be a contiguous float64 device tensor: it is changed in place")
    lib = _lib.load()
    _lib.require_device()
    stride = N ** 4 if rows <= 1 else int(d2.stride(0))
    check(lib.oovqe_response_d2_batch(dptr(Z.contiguous()), dptr(D0.contiguous()), N, rows,
                                      ctypes.c_void_p(d2.data_ptr()), stride, stream_ptr()), "oovqe_response_d2_batch")
    return d2


def relaxed_densities(int1e, int2e, overlap, oao_mo_coeff, mo_coeff, n_occ, z, d1, d2, wq, fock_ao=None):
    """The densities of ``E_I - sum_{p>q} z_pq f_pq`` (``f = C^T (h + G[D0]) C`` the RHF Fock matrix, whose off-diagonal
    elements vanish at every geometry) from those of ``E_I``, K states per geometry: with ``zt`` the symmetric matrix
    ``zt_pq = z_pq / 2``, ``Z = C zt C^T`` and ``D0 = 2 C_o C_o^T``

        D1_rel = D1 - Z,   D2_rel = D2 - sym8[2 Z_pq D0_rs - Z_pr D0_qs],   WQ_rel = WQ - pull_back(sym(dPhi/dC U^T)),
        dPhi/dC = 2 (h + G[D0]) C zt, plus 4 G[Z] C_o on the occupied columns.

    ``z``, ``d1``, ``wq`` [G, K, N, N]; ``d2`` [G, K, N, N, N, N] (every ``d2[g, k]`` contiguous), CHANGED IN PLACE; ``fock_ao`` = ``h +
    G[D0]`` [G, N, N] when the caller has it.  -> (D1_rel, D2_rel (``d2`` itself), WQ_rel)."""
    G, K, N = int(z.shape[0]), int(z.shape[1]), int(z.shape[-1])
    mm = ops.matmul_nn_batch
    C = mo_coeff.contiguous()
    Co = C[:, :, :n_occ].contiguous()
    D0 = 2.0 * mm(Co, _t(Co))
    D0 = (0.5 * (D0 + D0.transpose(1, 2))).contiguous()
    if fock_ao is None:
        J0, K0 = scf.fock_jk(int2e, D0)
        fock_ao = int1e + J0 - 0.5 * K0
    zt = (0.5 * (z + z.transpose(2, 3))).reshape(G * K, N, N).contiguous()
    Ck = _per_set(C, K)
    Czt = mm(Ck, zt)
    Z = mm(Czt, _t(Ck))
    Z = (0.5 * (Z + Z.transpose(1, 2))).contiguous()
    dphi = 2.0 * mm(_per_set(fock_ao, K), Czt)
    gz = _g_sets(int2e, Z.view(G, K, N, N)).reshape(G * K, N, N)
    dphi[:, :, :n_occ] += 4.0 * mm(gz, _per_set(Co, K))
    U = _per_set(oao_mo_coeff, K)
    gx = mm(dphi, _t(U))
    gx = 0.5 * (gx + gx.transpose(1, 2))
    sw, V, _ = scf.sym_eigh_batch(overlap.contiguous())
    sq, V = _per_set(torch.sqrt(sw), K), _per_set(V, K)
    wq_rel = wq - _pull_back(gx, sq, V, _t(V)).view(G, K, N, N)
    Zs = Z.view(G, K, N, N)
    for k in range(K):
        response_d2(Zs[:, k], D0, d2[:, k])
    return d1 - Z.view(G, K, N, N), d2, wq_rel


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


# ---- orbital response of CASCI states on RHF orbitals: numpy twins (tests) ----------------------------------------------
def _g_host(int2e, dm):
    """``G[D] = J[D] - K[D] / 2`` on the host."""
    return np.einsum("pqrs,rs->pq", int2e, dm) - 0.5 * np.einsum("prqs,rs->pq", int2e, dm)


def generalised_fock_host(int1e, int2e, overlap, mo_coeff, d1, d2):
    """The generalised Fock matrix ``F`` (MO basis, ``dE/dC = C^-T 2 F^T``) of a wave function with the AO densities
    ``d1``, ``d2`` of ``cas_ao_densities_host``: ``F^T = C^T (h D1 + T) S C``, ``T_mn = sum g_mlrs D2_nlrs``."""
    C = np.asarray(mo_coeff)
    y = C.T @ (np.asarray(int1e) @ d1 + np.einsum("mlrs,nlrs->mn", int2e, d2)) @ np.asarray(overlap) @ C
    return y.T


def orbital_gradient_host(fock):
    """numpy twin of ``orbital_gradient``."""
    F = np.asarray(fock)
    return np.tril(2.0 * (F.T - F), -1)


def response_pairs(n, n_core, ncas, n_occ):
    """The pairs p > q of ``n`` canonical RHF orbitals (``n_occ`` doubly occupied) that carry an orbital response of a
    CASCI with ``n_core`` inactive and ``ncas`` active orbitals -> boolean [n, n] masks ``(vo, diag)``: the virt-occ
    block, and the pairs inside occ-occ and virt-virt that join two classes (core x active-occupied, active-virtual x
    external).  The CASCI energy does not change under a rotation inside a class."""
    n, n_core, ncas, n_occ = int(n), int(n_core), int(ncas), int(n_occ)
    if not 0 <= n_core <= n_occ <= n_core + ncas <= n or not 0 < n_occ < n:
        raise ValueError(f"n = {n}, n_core = {n_core}, ncas = {ncas}, n_occ = {n_occ}: the Fermi level must lie inside "
                         "the active space, 0 <= n_core <= n_occ <= n_core + ncas <= n, 0 < n_occ < n")
    vo = np.zeros((n, n), dtype=bool)
    vo[n_occ:, :n_occ] = True
    diag = np.zeros((n, n), dtype=bool)
    diag[n_core:n_occ, :n_core] = True
    diag[n_core + ncas:, n_occ:n_core + ncas] = True
    return vo, diag


def zvector_host(int2e, mo_coeff, mo_energy, n_core, ncas, n_occ, w, eliminate=False):
    """numpy twin of ``zvector`` for ONE geometry and ONE state: ``z`` [N, N] (strictly lower triangle) with ``L^T z =
    w`` over the pairs of ``response_pairs``, ``(L kappa)_pq = (eps_p - eps_q) kappa_pq + [C^T G[dD(kappa)] C]_pq``,
    ``dD(kappa) = C (kappa n - n kappa) C^T``, ``n = diag(2 .. 2, 0 .. 0)``: the explicit matrix and a dense solve.
    ``eliminate``: the block elimination the device runs instead (the occ-occ and virt-virt pairs first, then the
    symmetric virt-occ system ``A z_vo = b``, dense) -> ``(z, A, b)``."""
    C, eps, w = np.asarray(mo_coeff), np.asarray(mo_energy), np.asarray(w)
    N = C.shape[0]
    vo, dg = response_pairs(N, n_core, ncas, n_occ)
    occ = np.zeros(N)
    occ[:n_occ] = 2.0
    delta = eps[:, None] - eps[None, :]

    def apply(kappa):
        dD = C @ (kappa * occ[None, :] - occ[:, None] * kappa) @ C.T
        return delta * kappa + C.T @ _g_host(int2e, dD) @ C

    def unit(p, q):
        k = np.zeros((N, N))
        k[p, q], k[q, p] = 1.0, -1.0
        return k

    z = np.zeros((N, N))
    if not eliminate:
        idx = np.argwhere(vo | dg)
        L = np.stack([apply(unit(p, q))[idx[:, 0], idx[:, 1]] for p, q in idx], axis=1)
        z[idx[:, 0], idx[:, 1]] = np.linalg.solve(L.T, w[idx[:, 0], idx[:, 1]])
        return z
    z[dg] = w[dg] / delta[dg]
    zt = 0.5 * (z + z.T)
    nv = N - n_occ
    b = (w - 4.0 * C.T @ _g_host(int2e, C @ zt @ C.T) @ C)[n_occ:, :n_occ]
    idx = np.argwhere(vo)
    A = np.stack([apply(unit(p, q))[vo] for p, q in idx], axis=1)
    z[n_occ:, :n_occ] = np.linalg.solve(A, b.reshape(-1)).reshape(nv, n_occ)
    return z, A, b


def response_d2_host(Z, D0):
    """``sym8[2 Z_pq D0_rs - Z_pr D0_qs]``: what the Lagrangian term ``sum z_pq f_pq`` adds to the AO two-particle
    density (twin of ``response_d2``, which subtracts it)."""
    return sym8_host(2.0 * np.einsum("pq,rs->pqrs", Z, D0) - np.einsum("pr,qs->pqrs", Z, D0))


def relaxed_densities_host(int1e, int2e, overlap, mo_coeff, n_occ, z, d1, d2, wq):
    """numpy twin of ``relaxed_densities`` for ONE geometry and ONE state: the densities of ``E_I - sum_{p>q} z_pq
    f_pq`` at fixed ``U``, from those of ``E_I`` -> ``(D1_rel, D2_rel, WQ_rel)``."""
    C, S = np.asarray(mo_coeff), np.asarray(overlap)
    zt = 0.5 * (z + z.T)
    Z = C @ zt @ C.T
    Co = C[:, :n_occ]
    D0 = 2.0 * Co @ Co.T
    dphi = 2.0 * (np.asarray(int1e) + _g_host(int2e, D0)) @ C @ zt
    dphi[:, :n_occ] += 4.0 * _g_host(int2e, Z) @ Co
    s, V = np.linalg.eigh(S)
    U = (V * np.sqrt(s)) @ V.T @ C                       # U = X^-1 C
    return d1 - Z, d2 - response_d2_host(Z, D0), wq - overlap_pullback_host(S, dphi @ U.T)
