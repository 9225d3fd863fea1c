"""Overlaps between the wave functions of different geometries on the device, and what is built on them: the Berry-phase
estimator of a whole loop and root tracking for CASCI results.

``sector_overlaps`` is the kernel (``oovqe_sector_overlap_batch``, csrc/overlap.hip): for P pairs at once, the overlaps of
(N_alpha, N_beta)-sector vectors over non-orthogonal orbitals, the doubly occupied core folded in.  ``berry.py`` computes
the same active-space expression one pair at a time on the host (``minor_matrix`` + two small products) and stays the
reference: rows of U go with the bra, columns with the ket, exactly as in ``berry.ActiveSpaceRotation.apply`` with bra =
``state_b`` and ket = ``state_a``.

``state_overlaps_oao`` is the reference notebook's estimator (orthonormal-AO metric, active block re-orthogonalised, no
core) for tensors that are not in a batch; ``OO_pqc_batch.state_overlaps`` / ``berry_phase`` / ``casci_overlaps`` are the
batch's own calls, with the exact AO metric between two geometries (``gto.cross_overlap_batch``) as the other choice.
``track_roots`` / ``apply_tracking`` repair the order and the signs of CASCI roots along a path.
"""
import ctypes
import functools
import itertools

import numpy as np
import torch

from . import _lib, ops
from ._lib import check, dptr, stream_ptr
from .sector import sector_of

F64 = torch.float64
MAX_NCAS = 8                   # OOVQE_OVERLAP_MAX_NCAS
MAX_M = 48                     # OOVQE_OVERLAP_MAX_M
MAX_STRINGS = 70               # OOVQE_OVERLAP_MAX_STRINGS
MAX_ROOTS = 4                  # OOVQE_OVERLAP_MAX_ROOTS (= ci.MAX_ROOTS)


def orthogonalize_mode(orthogonalize):
    """``orthogonalize`` -> the kernel's mode: False -> 0 (U as it is), ``"givens"`` (or True) -> 1 (the Q factor of
    U = Q R with a positive diagonal of R, what ``berry.givens_orthogonal`` makes)."""
    if orthogonalize is False or orthogonalize is None:
        return 0
    if orthogonalize is True or orthogonalize == "givens":
        return 1
    if orthogonalize == "polar":
        raise ValueError("orthogonalize='polar' is not served on the device (an SVD is not worth a kernel here): use "
                         "berry.ActiveSpaceRotation(..., orthogonalize='polar') on the host")
    raise ValueError(f"orthogonalize = {orthogonalize!r} ('givens' or False)")


def check_scope(ncas, n_alpha, n_beta, n_core=0):
    if not 1 <= int(ncas) <= MAX_NCAS:
        raise ValueError(f"ncas = {ncas}: the overlaps cover 1 <= ncas <= {MAX_NCAS}")
    if not (0 <= int(n_alpha) <= ncas and 0 <= int(n_beta) <= ncas):
        raise ValueError(f"(N_alpha, N_beta) = ({n_alpha}, {n_beta}) in {ncas} orbitals")
    if int(n_core) < 0 or int(n_core) + int(ncas) > MAX_M:
        raise ValueError(f"n_core + ncas = {int(n_core) + int(ncas)}: the overlaps cover at most {MAX_M} occupied-plus-"
                         "active orbitals")


@functools.lru_cache(maxsize=None)
def _dense_index_host(ncas, n_alpha, n_beta):
    from .berry import sector_tables
    return sector_tables(ncas, n_alpha, n_beta)[2].reshape(-1).astype(np.int32)


_DENSE_INDEX = {}


def dense_index(ncas, n_alpha, n_beta, device):
    """int32 [na nb] on the device: where element (ia, ib) of the sector sits in a dense register of 2^(2 ncas)
    amplitudes (the gather of ``berry.sector_tables``)."""
    key = (ncas, n_alpha, n_beta, str(device))
    if key not in _DENSE_INDEX:
        _DENSE_INDEX[key] = torch.as_tensor(_dense_index_host(ncas, n_alpha, n_beta)).to(device)
    return _DENSE_INDEX[key]


def sector_overlaps(s, n_core, ncas, n_alpha, n_beta, bra, ket, orthogonalize=False, signed=True, index=None):
    """Overlaps of sector vectors over non-orthogonal orbitals for P pairs in one launch.

    Args:
        s: [P, M, M], M = n_core + ncas: the overlap of the doubly occupied (first ``n_core``) and active orbitals of the
            bra geometry (rows) with those of the ket geometry (columns)
        bra, ket: [P, Rb, L] and [P, Rk, L] (a 2-D tensor is one vector per pair), in the sector layout
            ``c[ia * nb + ib]`` of ``sector.string_tables`` (L = na nb), or with ``index`` in any layout
        orthogonalize: False (U as it is) or ``"givens"`` (the Q factor of U, ``berry.givens_orthogonal``)
        signed: multiply both sides with the alpha-before-beta sign table of ``berry.sector_tables`` (the states of the
            circuit engines and CI vectors carry the interleaved order)
        index: int32 [na nb]: element (ia, ib) is read at ``index[ia * nb + ib]`` of a vector (``dense_index`` for a
            dense 2^(2 ncas) register)

    Returns ``(out [P, Rb, Rk], core_det [P])`` on the device: ``out[p, i, j] = sum bra_i[Ja, Jb] det U[Ja, Ia]
    det U[Jb, Ib] ket_j[Ia, Ib]`` with ``U = s_aa - s_ac s_cc^-1 s_ca`` and ``core_det = det(s_cc)``; the all-electron
    overlap of two CAS wave functions is ``core_det**2 * out``.  Scope: ncas <= 8, M <= 48, Rb, Rk <= 4; the same
    bits wherever a pair stands in the list."""
    mode = orthogonalize_mode(orthogonalize)
    check_scope(ncas, n_alpha, n_beta, n_core)
    lib = _lib.load()
    s = ops.as_device(s)
    dev = s.device
    if s.dim() == 2:
        s = s[None]
    m = int(n_core) + int(ncas)
    if s.dim() != 3 or tuple(s.shape[1:]) != (m, m):
        raise ValueError(f"s has shape {tuple(s.shape)}, expected [P, {m}, {m}]")
    P = int(s.shape[0])
    vec = []
    for name, x in (("bra", bra), ("ket", ket)):
        x = ops.as_device(x, dev)
        if x.dim() == 2:
            x = x[:, None]
        if x.dim() != 3 or int(x.shape[0]) != P or not 1 <= int(x.shape[1]) <= MAX_ROOTS:
            raise ValueError(f"{name} has shape {tuple(x.shape)}, expected [{P}, 1 .. {MAX_ROOTS}, L]")
        vec.append(x.contiguous())
    bra, ket = vec
    ld = int(bra.shape[2])
    if int(ket.shape[2]) != ld:
        raise ValueError(f"bra vectors of length {ld}, ket vectors of length {int(ket.shape[2])}")
    from math import comb
    D = comb(ncas, n_alpha) * comb(ncas, n_beta)
    if index is None:
        if ld != D:
            raise ValueError(f"vectors of length {ld}: the ({n_alpha}, {n_beta}) sector of {ncas} orbitals has {D} "
                             "determinants (pass index= for another layout)")
    else:
        index = torch.as_tensor(index).to(device=dev, dtype=torch.int32).contiguous()
        if index.numel() != D:
            raise ValueError(f"index holds {index.numel()} entries for {D} determinants")
    out = torch.empty((P, int(bra.shape[1]), int(ket.shape[1])), dtype=F64, device=dev)
    core_det = torch.empty(P, dtype=F64, device=dev)
    check(lib.oovqe_sector_overlap_batch(
        dptr(s), m, int(n_core), int(ncas), int(n_alpha), int(n_beta), P, dptr(bra), int(bra.shape[1]), dptr(ket),
        int(ket.shape[1]), dptr(index, torch.int32), ctypes.c_int64(ld), mode, int(bool(signed)), dptr(out),
        dptr(core_det), stream_ptr()), "oovqe_sector_overlap_batch")
    return out, core_det


def _stack(x, device):
    if isinstance(x, (list, tuple)):
        return torch.stack([ops.as_device(_real(v), device) for v in x])
    return ops.as_device(_real(x), device)


def _device_of(*xs):
    """The device of the first device tensor among the arguments (sequences included), else the current one."""
    for x in xs:
        for v in (x if isinstance(x, (list, tuple)) else (x,)):
            if isinstance(v, torch.Tensor) and v.is_cuda:
                return v.device
    return _lib.require_device()


def _real(v):
    if isinstance(v, torch.Tensor) and v.is_complex():
        raise ValueError("complex states are not served by the batched overlaps (berry.state_overlap takes them)")
    return v


def state_overlaps_oao(bra_states, ket_states, oao_a, oao_b, act_idx, nelecas, orthogonalize="givens"):
    """The reference notebook's overlap estimator for P pairs (a -> b) in one launch:

        out[p] = <bra_p| G_{a->b} |ket_p>,   U_p = (oao_a[p]^T oao_b[p])[act, act]

    exactly ``berry.state_overlap(bra_p, berry.bogoliubov_atob_cas(oao_a[p].T @ oao_b[p], act_idx, nelecas), ket_p)``:
    the ket is the state of geometry a, the bra that of geometry b; the two orthonormal-AO bases are treated as one and
    the core is ignored.

    Args:
        bra_states, ket_states: [P, L] real states (or sequences of P of them): dense registers (L = 2^(2 ncas)) or
            sector vectors (L = na nb)
        oao_a, oao_b: [P, N, N] ``oao_mo_coeff`` of the ket's and of the bra's geometry (or sequences)
        act_idx: the active orbitals; nelecas: active electrons (closed shell or high spin first, as ``hf_state``)
        orthogonalize: ``"givens"`` (the notebook) or False

    Returns [P] on the device."""
    orthogonalize_mode(orthogonalize)
    act = [int(i) for i in act_idx]
    ncas = len(act)
    occ = [1 if i < nelecas else 0 for i in range(2 * ncas)]
    n_alpha, n_beta = sector_of(occ, ncas)
    check_scope(ncas, n_alpha, n_beta)
    dev = _device_of(bra_states, ket_states, oao_a, oao_b)
    bra = _stack(bra_states, dev)
    ket = _stack(ket_states, dev)
    A = _stack(oao_a, dev)
    B = _stack(oao_b, dev)
    if bra.dim() != 2 or ket.shape != bra.shape:
        raise ValueError(f"states of shapes {tuple(bra.shape)} and {tuple(ket.shape)}, expected two [P, L]")
    P = int(bra.shape[0])
    if A.dim() != 3 or A.shape != B.shape or int(A.shape[0]) != P or A.shape[1] != A.shape[2]:
        raise ValueError(f"orbitals of shapes {tuple(A.shape)} and {tuple(B.shape)}, expected two [{P}, N, N]")
    if any(not 0 <= i < int(A.shape[1]) for i in act):
        raise ValueError(f"act_idx {act} outside 0..{int(A.shape[1]) - 1}")
    from math import comb
    L, D = int(bra.shape[1]), comb(ncas, n_alpha) * comb(ncas, n_beta)
    if L == 1 << (2 * ncas) and L != D:
        index = dense_index(ncas, n_alpha, n_beta, dev)
    elif L == D:
        index = None
    else:
        raise ValueError(f"states of length {L}: expected {1 << (2 * ncas)} (dense register) or {D} (sector)")
    sel = torch.as_tensor(act, device=dev)
    U = ops.matmul_nn_batch(A[:, :, sel].transpose(1, 2).contiguous(), B[:, :, sel].contiguous())
    out, _ = sector_overlaps(U, 0, ncas, n_alpha, n_beta, bra, ket, orthogonalize, True, index)
    return out[:, 0, 0]


# ---- root tracking ---------------------------------------------------------------------------------------------------
def track_roots(O):
    """Order and signs of the roots along an open path from the overlaps of neighbouring geometries.

    Args:
        O: [G - 1, R, R], ``O[g, I, J] = <Psi_I(R_g)|Psi_J(R_g+1)>`` (``OO_pqc_batch.casci_overlaps``), R <= 4

    Returns ``(perm [G, R] int64, sign [G, R] float64)`` (tensors where ``O`` is one, on its device; else numpy): tracked
    state i is root ``perm[g, i]`` of geometry g times ``sign[g, i]``.  Geometry 0 keeps its order and signs.  Every later
    geometry takes the assignment that maximises ``sum_i |<tracked i at g | root perm(i) at g + 1>|`` over all R!
    permutations -- on a tie the lowest permutation in lexicographic order -- and then the signs that make the matched
    overlaps positive (a matched overlap of exactly 0 keeps +1), chained along the path."""
    is_tensor = isinstance(O, torch.Tensor)
    o = O.detach().cpu().numpy() if is_tensor else np.asarray(O, dtype=np.float64)
    if o.ndim != 3 or o.shape[1] != o.shape[2]:
        raise ValueError(f"O has shape {o.shape}, expected [G - 1, R, R]")
    R = o.shape[1]
    if not 1 <= R <= MAX_ROOTS:
        raise ValueError(f"{R} roots (1 .. {MAX_ROOTS})")
    G = o.shape[0] + 1
    perm = np.zeros((G, R), dtype=np.int64)
    sign = np.ones((G, R))
    perm[0] = np.arange(R)
    rows = np.arange(R)
    for g in range(G - 1):
        t = sign[g][:, None] * o[g][perm[g]]                 # <tracked i at g | root j at g + 1>
        best, best_val = None, -1.0
        for cand in itertools.permutations(range(R)):
            val = float(np.abs(t[rows, list(cand)]).sum())
            if val > best_val:
                best, best_val = cand, val
        perm[g + 1] = best
        matched = t[rows, perm[g + 1]]
        sign[g + 1] = np.where(matched < 0, -1.0, 1.0)
    if is_tensor:
        return torch.as_tensor(perm).to(O.device), torch.as_tensor(sign).to(O.device)
    return perm, sign


def apply_tracking(x, perm, sign, kind=None):
    """Reorder and re-sign per-root results along a path with the output of ``track_roots``.

    - [G, R] energies: reordered;
    - [G, R, dim] vectors: reordered and multiplied by their signs;
    - [G, R, R, ...] state matrices (``casci_nuclear_gradients(...).gradients``, the dipoles of
      ``casci_dipole_matrix``): both state indices reordered, element (I, J) multiplied by sign_I sign_J -- diagonal
      blocks are unchanged by the signs.

    ``kind`` ("energies", "vectors", "matrices") overrides the choice by the number of dimensions (2, 3, >= 4): a bare
    [G, R, R] matrix needs ``kind="matrices"``."""
    is_tensor = isinstance(x, torch.Tensor)
    xp = x if is_tensor else torch.as_tensor(np.asarray(x))
    p = torch.as_tensor(perm).to(device=xp.device, dtype=torch.long)
    sg = torch.as_tensor(sign).to(device=xp.device, dtype=xp.dtype if xp.is_floating_point() else F64)
    if kind is None:
        kind = {2: "energies", 3: "vectors"}.get(xp.dim(), "matrices")
    if kind not in ("energies", "vectors", "matrices"):
        raise ValueError(f"kind = {kind!r} ('energies', 'vectors' or 'matrices')")
    G, R = p.shape
    need = {"energies": 2, "vectors": 3, "matrices": 3}[kind]
    if xp.dim() < need or tuple(xp.shape[:2]) != (G, R) or (kind == "matrices" and int(xp.shape[2]) != R):
        raise ValueError(f"x of shape {tuple(xp.shape)} does not go with a tracking of shape {(G, R)} as {kind}")
    g = torch.arange(G, device=xp.device)[:, None]
    if kind == "energies":
        out = xp[g, p]
    elif kind == "vectors":
        out = xp[g, p] * sg.reshape((G, R) + (1,) * (xp.dim() - 2))
    else:
        out = xp[g[:, :, None], p[:, :, None], p[:, None, :]]
        w = sg[:, :, None] * sg[:, None, :]
        out = out * w.reshape((G, R, R) + (1,) * (xp.dim() - 3))
    return out if is_tensor else out.numpy()
