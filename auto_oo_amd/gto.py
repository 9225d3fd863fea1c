"""AO integrals of a stack of geometries on the device (``oovqe_gto_integrals_batch``, csrc/gto.hip).

``gaussian.py`` builds the integrals of ONE molecule with numpy loops on the host (0.7 s for formaldimine in
STO-3G); a scan over the points of a Berry-phase loop spends its time there.  Here one basis description --
``GTOBasis``: flat tables of contracted s, p and d shells (d as 5 spherical or 6 Cartesian functions), built on the
host once -- is shared by all
geometries, and ``integrals_batch`` fills overlap, core Hamiltonian, ``S^-1/2``, nuclear repulsion and ``(pq|rs)``
of G geometries on the device.  Conventions are those of ``gaussian.py`` (atoms in input order; per atom 1s, 2s,
2px, 2py, 2pz; contracted functions normalised); coordinates are in Angstrom here (``gaussian.BOHR``) and in Bohr
at the C ABI.  There is no host fallback: without the HIP library and a device these functions raise.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from ._lib import check, dptr, stream_ptr
from .gaussian import BOHR, _Shell, component_norm, _STO3G, _STO3G_1S_COEF, _STO3G_2S_COEF, _STO3G_2P_COEF, zmatrix_to_cartesian

F64 = torch.float64
MAX_L = 2                      # OOVQE_GTO_MAX_L
MAX_PRIM = 10                  # OOVQE_GTO_MAX_PRIM
CARTESIAN = 0x100              # OOVQE_GTO_CARTESIAN: flag of the l field of a d shell of 6 Cartesian functions
MAX_MOMENT = 2                 # OOVQE_GTO_MAX_MOMENT
MAX_GRAD_SETS = 10             # OOVQE_GTO_GRAD_MAX_SETS
GRAD_SETS_TILE = 5             # OOVQE_GTO_GRAD_SETS_TILE
INVSQRT_MAX_N = 64             # OOVQE_INVSQRT_MAX_N
INVSQRT_MIN_EIG = 1e-8         # OOVQE_INVSQRT_MIN_EIG

_Z = {s: i + 1 for i, s in enumerate(
    "H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar".split())}
_L_OF = {"s": 0, "p": 1, "d": 2, "f": 3}


def _sto3g_shells(symbol):
    key = symbol.capitalize()
    if key not in _STO3G:
        raise ValueError(f"no STO-3G parameters for element {symbol!r} ({', '.join(_STO3G)} are built in)")
    par = _STO3G[key]
    shells = [(0, par["1s"], _STO3G_1S_COEF)]
    if "2sp" in par:
        shells += [(0, par["2sp"], _STO3G_2S_COEF), (1, par["2sp"], _STO3G_2P_COEF)]
    return par["Z"], shells


class GTOBasis:
    """Flat shell tables of a molecule's basis, shared by every geometry of a stack.

    Args:
        symbols: element symbols, in the order of the atoms of every geometry
        basis: ``"sto-3g"`` (the tables of ``gaussian.py``: H, C, N, O, F), or a dict
            ``{element: [(l, exponents, coefficients), ...]}`` of s / p / d shells (``l`` = 0, 1, 2 or ``"s"``,
            ``"p"``, ``"d"``), coefficients those of normalised primitives as basis-set tables list them, at most
            ``MAX_PRIM`` primitives per shell.  Shells are segmented: a general contraction such as cc-pVDZ is
            passed as one shell per contracted function, each repeating the primitives it uses.
        d_functions: the form of the d shells, required as soon as the table holds one (there is no default between
            5d and 6d).  ``"spherical"``: 5 functions per shell, each normalised, in the order xy, yz, 3z^2 - r^2, xz,
            x^2 - y^2 (m = -2 .. 2, PySCF's order, with the signs of these polynomials).  ``"cartesian"``: 6
            functions in the order xx, xy, xz, yy, yz, zz, EACH normalised to 1 -- libcint scales its Cartesian d
            functions differently (there xx, yy, zz share the radial normalisation of xy and have norm^2 = 3).

    Host arrays: ``shells`` [nshell, 4] int32 (atom, l field, number of primitives, offset; the l field of a Cartesian
    d shell is ``2 | CARTESIAN``), ``exps``, ``coefs`` (contraction coefficients of the NORMALISED contracted
    function, primitive norms included -- ``_Shell.coefs`` of ``gaussian.py``; for a d shell those that normalise
    xx), ``charges`` [natm]; ``table`` [(atom, l, exponents, coefficients as given)]; ``nao``, ``nelectron`` (neutral
    molecule), ``max_nprim``, ``max_l``.
    """

    def __init__(self, symbols, basis="sto-3g", d_functions=None):
        self.symbols = [str(s) for s in symbols]
        if not self.symbols:
            raise ValueError("GTOBasis needs at least one atom")
        if d_functions not in (None, "spherical", "cartesian"):
            raise ValueError(f"d_functions = {d_functions!r} (None, 'spherical' or 'cartesian')")
        self.d_functions = d_functions
        self.table = []
        rows, exps, coefs, charges = [], [], [], []
        for atom, sym in enumerate(self.symbols):
            if isinstance(basis, str):
                if basis.lower().replace("-", "") != "sto3g":
                    raise ValueError("the only built-in basis is 'sto-3g'; pass any other s/p basis as a dict "
                                     "{element: [(l, exponents, coefficients), ...]}")
                z, shells = _sto3g_shells(sym)
            else:
                key = sym.capitalize()
                if key not in basis:
                    raise ValueError(f"the basis has no shells for element {sym!r}")
                if key not in _Z:
                    raise ValueError(f"unknown element {sym!r}")
                z, shells = _Z[key], basis[key]
            charges.append(float(z))
            for l, ex, co in shells:
                l = _L_OF.get(str(l).lower(), l)
                if not isinstance(l, (int, np.integer)) or l < 0:
                    raise ValueError(f"shell of {sym!r}: angular momentum {l!r}")
                if l > MAX_L:
                    raise ValueError(f"shell of {sym!r} has l = {l}: only s, p and d shells (l <= {MAX_L}) are "
                                     "implemented")
                if l == 2 and d_functions is None:
                    raise ValueError(f"shell of {sym!r} has l = 2: say which functions a d shell stands for, "
                                     "d_functions='spherical' (5) or d_functions='cartesian' (6)")
                ex = np.asarray(ex, dtype=np.float64).ravel()
                co = np.asarray(co, dtype=np.float64).ravel()
                if ex.size != co.size or not 1 <= ex.size <= MAX_PRIM:
                    raise ValueError(f"shell of {sym!r}: {ex.size} exponents, {co.size} coefficients "
                                     f"(1 .. {MAX_PRIM} primitives per shell)")
                norm = _Shell(np.zeros(3), (int(l), 0, 0), ex, co)      # l <= 1: the same for px, py, pz
                field = int(l) | (CARTESIAN if (l == 2 and d_functions == "cartesian") else 0)
                rows.append((atom, field, ex.size, len(exps)))
                self.table.append((atom, int(l), ex.copy(), co.copy()))
                exps.extend(norm.exps.tolist())
                # (_Shell leaves xx with norm^2 = 3; the kernels take the coefficients that normalise xx)
                coefs.extend((norm.coefs * component_norm((int(l), 0, 0))).tolist())
        self.shells = np.asarray(rows, dtype=np.int32).reshape(-1, 4)
        self.exps = np.asarray(exps, dtype=np.float64)
        self.coefs = np.asarray(coefs, dtype=np.float64)
        self.charges = np.asarray(charges, dtype=np.float64)
        self.natm = len(self.symbols)
        self.nshell = self.shells.shape[0]
        ls = self.shells[:, 1] & 255
        self.max_l = int(ls.max())
        self.nao = int(sum(6 if f == (2 | CARTESIAN) else 2 * (f & 255) + 1 for f in self.shells[:, 1]))
        self.nelectron = int(round(self.charges.sum()))
        self.max_nprim = int(self.shells[:, 2].max())
        self._dev = {}
        self._work = {}

    # ---- geometry input ----------------------------------------------------------------------------------------
    def coordinates(self, coords):
        """``coords`` -> [G, natm, 3] float64 in Angstrom (host).  Accepts an array [G, natm, 3] (or [natm, 3]) or
        a sequence of the geometries ``Moldata_sto3g`` takes: Z-matrix / Cartesian strings, or lists of
        ``(symbol, (x, y, z))``.  The Z-matrix conversion runs on the host (microseconds per geometry)."""
        if isinstance(coords, torch.Tensor):
            coords = coords.detach().cpu().numpy()
        if isinstance(coords, str) or (isinstance(coords, (list, tuple)) and coords
                                       and isinstance(coords[0], (tuple, list)) and len(coords[0]) == 2
                                       and isinstance(coords[0][0], str)):
            coords = [coords]
        if isinstance(coords, np.ndarray):
            xyz = np.asarray(coords, dtype=np.float64)
            if xyz.ndim == 2:
                xyz = xyz[None]
        else:
            xyz = np.empty((len(coords), self.natm, 3))
            for g, geo in enumerate(coords):
                if isinstance(geo, str):
                    sym, pos = zmatrix_to_cartesian(geo)
                elif isinstance(geo, np.ndarray):
                    sym, pos = self.symbols, np.asarray(geo, dtype=np.float64)
                else:
                    sym = [a[0] for a in geo]
                    pos = np.array([a[1] for a in geo], dtype=np.float64)
                if [s.capitalize() for s in sym] != [s.capitalize() for s in self.symbols]:
                    raise ValueError(f"geometry {g} has atoms {sym}, the basis was built for {self.symbols}")
                xyz[g] = pos
        if xyz.ndim != 3 or xyz.shape[1:] != (self.natm, 3):
            raise ValueError(f"coordinates of shape {xyz.shape}, expected [G, {self.natm}, 3]")
        return np.ascontiguousarray(xyz)

    # ---- device side -------------------------------------------------------------------------------------------
    def device_tables(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = SimpleNamespace(
                shells=torch.as_tensor(self.shells).contiguous().to(device),
                exps=torch.as_tensor(self.exps).to(device), coefs=torch.as_tensor(self.coefs).to(device),
                charges=torch.as_tensor(self.charges).to(device))
        return self._dev[key]

    def _work_for(self, kind, device, export, *args):
        """The buffer of the ``*_work_size`` export ``export(nshell, max_nprim, *args)``: one per (kind, device, stream),
        grown when the export asks for more; a refusal of the export raises."""
        key = kind + (str(device), torch.cuda.current_stream().cuda_stream)
        buf = self._work.get(key)
        size = int(getattr(_lib.load(), export)(self.nshell, self.max_nprim, *args))
        if size < 0:
            check(size, export)
        if buf is None or buf.numel() < size:
            buf = self._work[key] = torch.empty(size, dtype=F64, device=device)
        return buf

    def work(self, device, G):
        """Work buffer for G geometries, one per (device, stream): calls on different streams never share one."""
        return self._work_for((), device, "oovqe_gto_work_size", G)

    def gradient_work(self, device, G, nset=1):
        """Work buffer of ``oovqe_gto_gradient_batch`` for G geometries (``nset`` > 1: of
        ``oovqe_gto_gradient_sets_batch`` for that many density sets per geometry), one per (device, stream) like
        ``work``."""
        if nset > 1:
            return self._work_for(("gradient",), device, "oovqe_gto_gradient_sets_work_size", self.natm, G, int(nset))
        return self._work_for(("gradient",), device, "oovqe_gto_gradient_work_size", self.natm, G)

    def connection_work(self, device, G, nset):
        """Work buffer of ``oovqe_gto_overlap_connection_batch`` for G geometries of ``nset`` matrices, one per
        (device, stream) like ``work``."""
        return self._work_for(("connection",), device, "oovqe_gto_overlap_connection_work_size", self.natm, G,
                              int(nset))


def _head(basis, device):
    """The arguments every geometry-stack entry of the C ABI begins with: the shell table, its primitives, the atoms
    and their charges (``oovqe_gto_cross_overlap_batch`` takes them without the charges)."""
    t = basis.device_tables(device)
    return (basis.nshell, dptr(t.shells, torch.int32), int(basis.exps.size), dptr(t.exps), dptr(t.coefs), basis.natm,
            dptr(t.charges))


def _check_stack(basis, x, name="coordinates", stack="G"):
    """``x`` must be a [G, natm, 3] tensor of geometries."""
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or tuple(x.shape[1:]) != (basis.natm, 3):
        raise ValueError(f"{name} of shape {tuple(getattr(x, 'shape', ()))}, expected [{stack}, {basis.natm}, 3]")


def _check_shape(name, x, shape, tensor=False):
    """``x`` must have the shape ``shape`` (``tensor``: and be a tensor)."""
    if (tensor and not isinstance(x, torch.Tensor)) or tuple(getattr(x, "shape", ())) != tuple(shape):
        raise ValueError(f"{name} has shape {tuple(getattr(x, 'shape', ()))}, expected {shape}")


def integrals_into(basis, coords_bohr, overlap=None, int1e_ao=None, int2e_ao=None, nuc=None):
    """The integrals of the geometries ``coords_bohr`` ([G, natm, 3] device tensor, Bohr) written into the given
    contiguous device tensors ([G, N, N], [G, N, N], [G, N, N, N, N], [G]; None skips one), on the current stream."""
    lib = _lib.load()
    G = int(coords_bohr.shape[0])
    dev = coords_bohr.device
    N = basis.nao
    for name, x, shape in (("overlap", overlap, (G, N, N)), ("int1e_ao", int1e_ao, (G, N, N)),
                           ("int2e_ao", int2e_ao, (G, N, N, N, N)), ("nuc", nuc, (G,))):
        if x is not None:
            _check_shape(name, x, shape)
    work = basis.work(dev, G)
    check(lib.oovqe_gto_integrals_batch(
        *_head(basis, dev), G, dptr(coords_bohr), N, dptr(overlap), dptr(int1e_ao), dptr(int2e_ao), dptr(nuc),
        dptr(work), stream_ptr()), "oovqe_gto_integrals_batch")


def moment_components(order):
    """Number of components of the moment integrals: 3 (x, y, z) for order 1, 9 (then xx, xy, xz, yy, yz, zz) for 2."""
    if order not in (1, MAX_MOMENT):
        raise ValueError(f"order = {order!r}: moment integrals are implemented for order 1 (dipole) and "
                         f"{MAX_MOMENT} (dipole and second moments)")
    return 3 if order == 1 else 9


def origin_to_device(origin, G, device, scale=1.0):
    """``origin`` ([3] or [G, 3], host or device; None: the origin of the coordinates) -> [G, 3] device tensor times
    ``scale``, or None."""
    if origin is None:
        return None
    o = origin.detach().to(F64) if isinstance(origin, torch.Tensor) else torch.as_tensor(
        np.asarray(origin, dtype=np.float64))
    if tuple(o.shape) == (3,):
        o = o.expand(G, 3)
    if tuple(o.shape) != (G, 3):
        raise ValueError(f"origin of shape {tuple(o.shape)}, expected [3] or [{G}, 3]")
    return (o.to(device) * scale).contiguous()


def moment_integrals_into(basis, coords_bohr, moments, order=1, origin_bohr=None):
    """``moment_integrals_batch`` for geometries that are already a [G, natm, 3] device tensor in Bohr, written into
    the contiguous device tensor ``moments`` [G, 3 or 9, N, N] on the current stream.  ``origin_bohr``: [G, 3] device
    tensor in Bohr, or None."""
    lib = _lib.load()
    ncomp = moment_components(order)
    _check_stack(basis, coords_bohr)
    G, N = int(coords_bohr.shape[0]), basis.nao
    _check_shape("moments", moments, (G, ncomp, N, N))
    if origin_bohr is not None and tuple(origin_bohr.shape) != (G, 3):
        raise ValueError(f"origin of shape {tuple(origin_bohr.shape)}, expected [{G}, 3]")
    dev = coords_bohr.device
    work = basis.work(dev, G)
    check(lib.oovqe_gto_moments_batch(
        *_head(basis, dev), G, dptr(coords_bohr), N, int(order), dptr(origin_bohr), dptr(moments), dptr(work),
        stream_ptr()), "oovqe_gto_moments_batch")
    return moments


def moment_integrals_batch(basis, coords, order=1, origin=None):
    """Dipole (and second-moment) integrals of G geometries on the device (``oovqe_gto_moments_batch``,
    csrc/gto_moments.hip): ``M[g, c, mu, nu] = <mu| (x - Ox)^ex (y - Oy)^ey (z - Oz)^ez |nu>`` over the functions of
    ``integrals_batch``, in atomic units.

    Args:
        basis: GTOBasis (s, p and d shells, both d forms)
        coords: geometries in the forms ``integrals_batch`` takes (Angstrom)
        order: 1 -> 3 components x, y, z; 2 -> 9 components x, y, z, xx, xy, xz, yy, yz, zz (the first three are those
            of order 1 bit for bit)
        origin: [3] or [G, 3] in Angstrom (default: the origin of the coordinates)

    Returns [G, 3 or 9, N, N] on the device; every matrix is exactly symmetric and a geometry has the same bits whatever
    stack it is part of."""
    ncomp = moment_components(order)
    device = _lib.require_device()
    xyz = coords_to_device(basis, coords, device)
    G = int(xyz.shape[0])
    out = torch.empty((G, ncomp, basis.nao, basis.nao), dtype=F64, device=device)
    return moment_integrals_into(basis, xyz, out, order, origin_to_device(origin, G, device, 1.0 / BOHR))


def cross_overlap_into(basis, coords_a_bohr, coords_b_bohr, out=None):
    """``cross_overlap_batch`` for geometries that are already [P, natm, 3] device tensors in Bohr, written into the
    contiguous device tensor ``out`` [P, N, N] (made when None) on the current stream."""
    lib = _lib.load()
    _check_stack(basis, coords_a_bohr, "coords_a_bohr", "P")
    _check_stack(basis, coords_b_bohr, "coords_b_bohr", "P")
    P, N = int(coords_a_bohr.shape[0]), basis.nao
    if int(coords_b_bohr.shape[0]) != P:
        raise ValueError(f"{P} bra geometries and {int(coords_b_bohr.shape[0])} ket geometries")
    dev = coords_a_bohr.device
    if out is None:
        out = torch.empty((P, N, N), dtype=F64, device=dev)
    else:
        _check_shape("out", out, (P, N, N))
    xa = coords_a_bohr.to(F64).contiguous()
    xb = coords_b_bohr.to(device=dev, dtype=F64).contiguous()
    check(lib.oovqe_gto_cross_overlap_batch(       # (the head without the charges)
        *_head(basis, dev)[:-1], P, dptr(xa), dptr(xb), N, dptr(out), stream_ptr()), "oovqe_gto_cross_overlap_batch")
    return out


def cross_overlap_batch(basis, coords_a, coords_b):
    """AO overlap between two geometries, for P pairs on the device (``oovqe_gto_cross_overlap_batch``,
    csrc/gto_cross.hip): ``S_ab[p, mu, nu] = <chi_mu at coords_a[p] | chi_nu at coords_b[p]>`` over the functions of
    ``integrals_batch`` (s, p and d shells, both d forms).

    Args:
        basis: GTOBasis
        coords_a, coords_b: P geometries each, in the forms ``integrals_batch`` takes (Angstrom)

    Returns [P, N, N] on the device.  The matrices are not symmetric (``S_ab(a, b) = S_ab(b, a)^T``); a pair has the
    same bits wherever it stands in the list."""
    device = _lib.require_device()
    return cross_overlap_into(basis, coords_to_device(basis, coords_a, device),
                              coords_to_device(basis, coords_b, device))


def refuse_d_gradient(basis):
    """Nuclear derivatives of d shells need f-type intermediates, which the derivative kernels do not have."""
    if basis.max_l >= 2:
        raise NotImplementedError("nuclear gradients are implemented for s and p shells only: this basis has d shells "
                                  "(l = 2)")


def gradient_into(basis, coords_bohr, dm1=None, wq=None, dm2=None, nuc=True, work=None):
    """``gradient_batch`` for geometries that are already a [G, natm, 3] device tensor in Bohr, on the current stream.
    ``work``: a buffer of ``oovqe_gto_gradient_work_size`` doubles to use instead of the basis' own."""
    refuse_d_gradient(basis)
    lib = _lib.load()
    _check_stack(basis, coords_bohr)
    G, N = int(coords_bohr.shape[0]), basis.nao
    dev = coords_bohr.device
    ins = []
    for name, x, shape in (("dm1", dm1, (G, N, N)), ("wq", wq, (G, N, N)), ("dm2", dm2, (G, N, N, N, N))):
        if x is not None:
            _check_shape(name, x, shape, tensor=True)
            x = x.to(device=dev, dtype=F64).contiguous()
        ins.append(x)
    grad = torch.empty((G, basis.natm, 3), dtype=F64, device=dev)
    if G == 0:
        return grad
    if work is None:
        work = basis.gradient_work(dev, G)
    xyz = coords_bohr.to(F64).contiguous()
    check(lib.oovqe_gto_gradient_batch(
        *_head(basis, dev), G, dptr(xyz), N, dptr(ins[0]), dptr(ins[1]), dptr(ins[2]), int(bool(nuc)), dptr(grad),
        dptr(work), stream_ptr()), "oovqe_gto_gradient_batch")
    return grad


def gradient_batch(basis, coords, dm1=None, wq=None, dm2=None, nuc=True):
    """Derivative integrals of G geometries contracted with densities on the device (``oovqe_gto_gradient_batch``,
    csrc/gto_grad.hip; no derivative integral is stored):

        grad[g, A, :] = dm1[g] . dh/dR_A + wq[g] . dS/dR_A + 1/2 dm2[g] . d(pq|rs)/dR_A + (nuc) dE_nuc/dR_A

    Args:
        basis: GTOBasis
        coords: geometries in the forms ``integrals_batch`` takes (Angstrom)
        dm1, wq: [G, N, N] device tensors, taken as symmetric -- symmetrising them is the caller's business (of the
            two elements (p, q) and (q, p) only one is read, once per shell pair; a non-symmetric matrix is not an
            error, it gives the gradient for the matrix mirrored from the elements read)
        dm2: [G, N, N, N, N] with the 8-fold symmetry of ``int2e_ao`` (``nucgrad.cas_ao_densities`` makes one),
            likewise the caller's business
        nuc: add the derivative of the nuclear repulsion
        (None skips a term)

    Returns [G, natm, 3] on the device, in Hartree / Bohr.  A geometry's gradient has the same bits whatever stack it
    is part of."""
    refuse_d_gradient(basis)
    device = _lib.require_device()
    return gradient_into(basis, coords_to_device(basis, coords, device), dm1, wq, dm2, nuc)


def gradient_sets_into(basis, coords_bohr, dm1=None, wq=None, dm2=None, nuc=True, work=None):
    """``gradient_sets_batch`` for geometries that are already a [G, natm, 3] device tensor in Bohr, on the current
    stream.  ``work``: a buffer of ``oovqe_gto_gradient_sets_work_size`` doubles to use instead of the basis' own."""
    refuse_d_gradient(basis)
    lib = _lib.load()
    _check_stack(basis, coords_bohr)
    G, N = int(coords_bohr.shape[0]), basis.nao
    given = [(name, x) for name, x in (("dm1", dm1), ("wq", wq), ("dm2", dm2)) if x is not None]
    if not given:
        raise ValueError("gradient_sets_into takes the number of sets from dm1, wq or dm2: give at least one")
    for name, x in given:
        if not isinstance(x, torch.Tensor) or x.dim() < 2:
            raise ValueError(f"{name} has shape {tuple(getattr(x, 'shape', ()))}, expected [G, K, ...]")
    K = int(given[0][1].shape[1])
    if not 1 <= K <= MAX_GRAD_SETS:
        raise ValueError(f"{K} density sets per geometry (1 .. {MAX_GRAD_SETS})")
    dev = coords_bohr.device
    ins = []
    for name, x, shape in (("dm1", dm1, (G, K, N, N)), ("wq", wq, (G, K, N, N)), ("dm2", dm2, (G, K, N, N, N, N))):
        if x is not None:
            _check_shape(name, x, shape)
            x = x.to(device=dev, dtype=F64).contiguous()
        ins.append(x)
    if isinstance(nuc, (bool, np.bool_)):
        bits = [bool(nuc)] * K
    else:
        bits = [bool(b) for b in nuc]
        if len(bits) != K:
            raise ValueError(f"nuc holds {len(bits)} flags for {K} sets")
    mask = sum(1 << k for k, b in enumerate(bits) if b)
    grad = torch.empty((G, K, basis.natm, 3), dtype=F64, device=dev)
    if G == 0:
        return grad
    if work is None:
        work = basis.gradient_work(dev, G, K)
    xyz = coords_bohr.to(F64).contiguous()
    check(lib.oovqe_gto_gradient_sets_batch(
        *_head(basis, dev), G, dptr(xyz), N, K, dptr(ins[0]), dptr(ins[1]), dptr(ins[2]), ctypes.c_uint(mask), dptr(grad),
        dptr(work), stream_ptr()), "oovqe_gto_gradient_sets_batch")
    return grad


def gradient_sets_batch(basis, coords, dm1=None, wq=None, dm2=None, nuc=True):
    """``gradient_batch`` for K density sets per geometry in ONE pass over the derivative integrals
    (``oovqe_gto_gradient_sets_batch``, csrc/gto_grad_sets.hip): the integrals of a primitive quartet are evaluated
    once and weighted with every set -- the state and interstate gradients of several CASCI roots.

    Args:
        basis: GTOBasis (s and p shells)
        coords: geometries in the forms ``integrals_batch`` takes (Angstrom)
        dm1, wq: [G, K, N, N], dm2: [G, K, N, N, N, N], symmetric as for ``gradient_batch`` (None skips a term for all
            sets); K (1 .. ``MAX_GRAD_SETS``) is taken from the tensors
        nuc: add the derivative of the nuclear repulsion: a bool, or one bool per set

    Returns [G, K, natm, 3] on the device, in Hartree / Bohr.  A set's gradient has the same bits whatever the stack,
    the other sets of the call, their number and its place among them."""
    refuse_d_gradient(basis)
    device = _lib.require_device()
    return gradient_sets_into(basis, coords_to_device(basis, coords, device), dm1, wq, dm2, nuc)


def overlap_connection_into(basis, coords_bohr, D, work=None):
    """``overlap_connection_batch`` for geometries that are already a [G, natm, 3] device tensor in Bohr, on the current
    stream.  ``work``: a buffer of ``oovqe_gto_overlap_connection_work_size`` doubles to use instead of the basis'
    own."""
    refuse_d_gradient(basis)
    lib = _lib.load()
    _check_stack(basis, coords_bohr)
    G, N = int(coords_bohr.shape[0]), basis.nao
    if not isinstance(D, torch.Tensor) or D.dim() != 4:
        raise ValueError(f"D has shape {tuple(getattr(D, 'shape', ()))}, expected [G, K, N, N]")
    K = int(D.shape[1])
    if not 1 <= K <= MAX_GRAD_SETS:
        raise ValueError(f"{K} matrices per geometry (1 .. {MAX_GRAD_SETS})")
    _check_shape("D", D, (G, K, N, N))
    dev = coords_bohr.device
    D = D.to(device=dev, dtype=F64).contiguous()
    out = torch.empty((G, K, basis.natm, 3), dtype=F64, device=dev)
    if G == 0:
        return out
    if work is None:
        work = basis.connection_work(dev, G, K)
    xyz = coords_bohr.to(F64).contiguous()
    check(lib.oovqe_gto_overlap_connection_batch(
        *_head(basis, dev), G, dptr(xyz), N, K, dptr(D), dptr(out), dptr(work), stream_ptr()),
        "oovqe_gto_overlap_connection_batch")
    return out


def overlap_connection_batch(basis, coords, D):
    """The derivative of the ket of the overlap contracted with K general matrices per geometry on the device
    (``oovqe_gto_overlap_connection_batch``, csrc/gto_connection.hip; no derivative integral is stored):

        out[g, k, A, :] = sum over mu, and nu on atom A, of D[g, k, mu, nu] <chi_mu | grad_A chi_nu>

    -- with ``D = C_a a C_a^T`` the AO part ``Da . T^A`` of the orbital-connection term of a derivative coupling
    (``gaussian.overlap_connection_from_table`` is ``T`` on the host).

    Args:
        basis: GTOBasis (s and p shells)
        coords: geometries in the forms ``integrals_batch`` takes (Angstrom)
        D: [G, K, N, N] device tensor, K = 1 .. ``MAX_GRAD_SETS``; NOT taken as symmetric or antisymmetric: both
            (mu, nu) and (nu, mu) are read.  For symmetric D the result is ``gradient_batch(wq=D / 2, nuc=False)``

    Returns [G, K, natm, 3] on the device, in 1 / Bohr.  Functions on ONE atom contribute (``<s|d p>`` on one centre).
    A (geometry, matrix) has the same bits whatever the stack, the other matrices, their number and its place among
    them."""
    refuse_d_gradient(basis)
    device = _lib.require_device()
    return overlap_connection_into(basis, coords_to_device(basis, coords, device), D)


# ---- point-charge embedding (csrc/gto_charges.hip) ---------------------------------------------------------------------
MAX_POINT_CHARGES = 65535      # per geometry


def point_charges_host(G, charges, charge_coords):
    """``charges`` ([G, M], or [M] shared by all geometries) and ``charge_coords`` ([G, M, 3] or [M, 3]) -> host arrays
    ([G, M], [G, M, 3]) float64, checked: matching M, 1 <= M <= ``MAX_POINT_CHARGES``, finite values.  Runs on the host
    only: nothing here touches the device."""
    def host(x):
        return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x
    q = np.asarray(host(charges), dtype=np.float64)
    r = np.asarray(host(charge_coords), dtype=np.float64)
    if q.ndim == 1:
        q = np.broadcast_to(q, (G,) + q.shape)
    if r.ndim == 2:
        r = np.broadcast_to(r, (G,) + r.shape)
    if q.ndim != 2 or q.shape[0] != G:
        raise ValueError(f"point charges of shape {np.shape(charges)}, expected [M] or [{G}, M]")
    M = int(q.shape[1])
    if r.shape != (G, M, 3):
        raise ValueError(f"positions of the point charges of shape {np.shape(charge_coords)}, expected [{M}, 3] or "
                         f"[{G}, {M}, 3] for {M} charges")
    if not 1 <= M <= MAX_POINT_CHARGES:
        raise ValueError(f"{M} point charges per geometry (1 .. {MAX_POINT_CHARGES})")
    if not (np.isfinite(q).all() and np.isfinite(r).all()):
        raise ValueError("point charges and their positions must be finite")
    return np.array(q, order="C"), np.array(r, order="C")            # (copies: a broadcast view is read-only)


def _check_point_charges(basis, coords_bohr, q, qxyz_bohr):
    """The device-tensor arguments of the ``point_charge_*_into`` functions -> (G, M, coords, q, qxyz) contiguous."""
    _check_stack(basis, coords_bohr)
    G = int(coords_bohr.shape[0])
    if G > 65535:
        raise ValueError(f"{G} geometries in one call (at most 65535)")
    if not isinstance(q, torch.Tensor) or q.dim() != 2 or int(q.shape[0]) != G:
        raise ValueError(f"point charges of shape {tuple(getattr(q, 'shape', ()))}, expected [{G}, M]")
    M = int(q.shape[1])
    if not isinstance(qxyz_bohr, torch.Tensor) or tuple(qxyz_bohr.shape) != (G, M, 3):
        raise ValueError(f"positions of the point charges of shape {tuple(getattr(qxyz_bohr, 'shape', ()))}, expected "
                         f"[{G}, {M}, 3]")
    if not 1 <= M <= MAX_POINT_CHARGES:
        raise ValueError(f"{M} point charges per geometry (1 .. {MAX_POINT_CHARGES})")
    dev = coords_bohr.device
    xyz = coords_bohr.to(F64).contiguous()
    q = q.to(device=dev, dtype=F64).contiguous()
    r = qxyz_bohr.to(device=dev, dtype=F64).contiguous()
    if not (bool(torch.isfinite(xyz).all()) and bool(torch.isfinite(q).all()) and bool(torch.isfinite(r).all())):
        raise ValueError("coordinates, point charges and their positions must be finite")
    return G, M, xyz, q, r


def point_charge_integrals_into(basis, coords_bohr, q, qxyz_bohr, out=None):
    """``point_charge_integrals_batch`` for geometries [G, natm, 3], charges [G, M] and positions [G, M, 3] that are
    already device tensors in atomic units (Bohr), written into the contiguous device tensor ``out`` [G, N, N] (made
    when None) on the current stream."""
    G, M, xyz, q, r = _check_point_charges(basis, coords_bohr, q, qxyz_bohr)
    N = basis.nao
    dev = xyz.device
    if out is None:
        out = torch.empty((G, N, N), dtype=F64, device=dev)
    else:
        _check_shape("out", out, (G, N, N))
    if G == 0:
        return out
    lib = _lib.load()
    work = basis.work(dev, G)
    check(lib.oovqe_gto_point_charge_batch(
        *_head(basis, dev), G, dptr(xyz), N, M, dptr(q), dptr(r), dptr(out), dptr(work), stream_ptr()),
        "oovqe_gto_point_charge_batch")
    return out


def point_charge_integrals_batch(basis, coords, charges, charge_coords):
    """The embedding operator of G geometries, each in its own cloud of M point charges, on the device
    (``oovqe_gto_point_charge_batch``, csrc/gto_charges.hip):

        V_ext[g, mu, nu] = - sum_k q[g, k] <chi_mu | 1 / |r - r[g, k]| | chi_nu>

    over the functions of ``integrals_batch`` (s, p and d shells, both d forms); ``int1e_ao + V_ext`` is the core
    Hamiltonian of the embedded molecule.

    Args:
        basis: GTOBasis
        coords: geometries in the forms ``integrals_batch`` takes (Angstrom)
        charges: [G, M], or [M] shared by all geometries (units of e), 1 <= M <= ``MAX_POINT_CHARGES``
        charge_coords: [G, M, 3] or [M, 3] in Angstrom; a charge may lie anywhere, also on a nucleus

    Returns [G, N, N] on the device; every matrix is exactly symmetric and a geometry has the same bits wherever it
    stands in the stack (``gaussian.point_charge_integrals_from_table`` is the host twin)."""
    xyz = basis.coordinates(coords) if not (isinstance(coords, torch.Tensor) and coords.is_cuda) else coords
    q, r = point_charges_host(int(xyz.shape[0]) if xyz.ndim == 3 else 1, charges, charge_coords)
    device = _lib.require_device()
    return point_charge_integrals_into(basis, coords_to_device(basis, xyz, device), torch.as_tensor(q).to(device),
                                       torch.as_tensor(r / BOHR).to(device))


def refuse_d_point_charge_gradient(basis):
    if basis.max_l >= 2:
        raise NotImplementedError("point-charge gradients are implemented for s and p shells only: this basis has "
                                  "d shells (l = 2)")


def point_charge_gradient_work(basis, device, G, M):
    """Work buffer of ``oovqe_gto_point_charge_gradient_batch``, one per (device, stream) like ``GTOBasis.work``."""
    return basis._work_for(("point_charges",), device, "oovqe_gto_point_charge_gradient_work_size", basis.natm, G, M)


def point_charge_gradient_into(basis, coords_bohr, q, qxyz_bohr, dm1, nuc=True):
    """``point_charge_gradient_batch`` for device tensors in atomic units (geometries [G, natm, 3], charges [G, M],
    positions [G, M, 3] in Bohr), on the current stream -> (gA [G, natm, 3], gQ [G, M, 3])."""
    refuse_d_point_charge_gradient(basis)
    G, M, xyz, q, r = _check_point_charges(basis, coords_bohr, q, qxyz_bohr)
    N = basis.nao
    _check_shape("dm1", dm1, (G, N, N), tensor=True)
    dev = xyz.device
    # (the size of the work buffer is asked for first: a molecule the entry refuses raises here, before any allocation)
    work = point_charge_gradient_work(basis, dev, G, M)
    gA = torch.empty((G, basis.natm, 3), dtype=F64, device=dev)
    gQ = torch.empty((G, M, 3), dtype=F64, device=dev)
    if G == 0:
        return gA, gQ
    lib = _lib.load()
    d1 = dm1.to(device=dev, dtype=F64).contiguous()
    check(lib.oovqe_gto_point_charge_gradient_batch(
        *_head(basis, dev), G, dptr(xyz), N, M, dptr(q), dptr(r), dptr(d1), int(bool(nuc)), dptr(gA), dptr(gQ),
        dptr(work), stream_ptr()), "oovqe_gto_point_charge_gradient_batch")
    return gA, gQ


def point_charge_gradient_batch(basis, coords, charges, charge_coords, dm1, nuc=True):
    """The derivatives of the embedding operator of ``point_charge_integrals_batch`` contracted with a one-particle
    density on the device (``oovqe_gto_point_charge_gradient_batch``; no derivative integral is stored):

        gA[g, A, :] = sum dm1[g] . dV_ext[g] / dR_A      (the basis functions move with atom A)
        gQ[g, k, :] = sum dm1[g] . dV_ext[g] / dr_k      (the centre of the operator moves)

    Args:
        basis: GTOBasis (s and p shells; d shells raise NotImplementedError)
        coords, charges, charge_coords: as for ``point_charge_integrals_batch`` (Angstrom)
        dm1: [G, N, N] device tensor, taken as symmetric as ``gradient_batch`` takes it
        nuc: add the derivatives of the classical term ``sum_{A, k} Z_A q_k / |R_A - r_k|`` to both (a charge ON a
            nucleus then gives NaN; there is no charge-charge term)

    Returns (gA [G, natm, 3], gQ [G, M, 3]) on the device, in Hartree / Bohr; the force on a charge is ``-gQ``.  Pairs of
    functions on one atom contribute to both.  A geometry has the same bits wherever it stands in the stack."""
    refuse_d_point_charge_gradient(basis)
    xyz = basis.coordinates(coords) if not (isinstance(coords, torch.Tensor) and coords.is_cuda) else coords
    G = int(xyz.shape[0]) if xyz.ndim == 3 else 1
    q, r = point_charges_host(G, charges, charge_coords)
    _check_shape("dm1", dm1, (G, basis.nao, basis.nao), tensor=True)
    device = _lib.require_device()
    return point_charge_gradient_into(basis, coords_to_device(basis, xyz, device), torch.as_tensor(q).to(device),
                                      torch.as_tensor(r / BOHR).to(device), dm1, nuc)


# ---- electrostatic potential and field at arbitrary points (csrc/gto_potential.hip) -------------------------------------
MAX_POINTS = 65535             # per geometry


def potential_work(basis, device, G, nset=1):
    """Work buffer of ``oovqe_gto_potential_batch``, one per (device, stream) like ``GTOBasis.work``."""
    return basis._work_for(("potential",), device, "oovqe_gto_potential_work_size", basis.natm, G, int(nset))


def _nuc_mask(nuc, K):
    """``nuc`` (a bool, or one bool per set) -> the bit mask of the sets that carry the nuclear term."""
    if isinstance(nuc, (bool, np.bool_)):
        bits = [bool(nuc)] * K
    else:
        bits = [bool(b) for b in nuc]
        if len(bits) != K:
            raise ValueError(f"nuc holds {len(bits)} flags for {K} sets")
    return sum(1 << k for k, b in enumerate(bits) if b)


def points_host(points, G):
    """``points`` of ``potential_batch`` and of the batch's potential methods ([M, 3] shared by all geometries, or
    [G, M, 3], in Angstrom; array or tensor) -> a checked host array [G, M, 3] in Bohr: the shape, 1 <= M <=
    ``MAX_POINTS``, finite.  Host work only."""
    r = points.detach().cpu().numpy() if isinstance(points, torch.Tensor) else points
    r = np.asarray(r, dtype=np.float64)
    if r.ndim == 2:
        r = np.broadcast_to(r, (G,) + r.shape)
    if r.ndim != 3 or r.shape[0] != G or r.shape[2] != 3:
        raise ValueError(f"points of shape {np.shape(points)}, expected [M, 3] or [{G}, M, 3]")
    if not 1 <= r.shape[1] <= MAX_POINTS:
        raise ValueError(f"{r.shape[1]} points per geometry (1 .. {MAX_POINTS})")
    if not np.isfinite(r).all():
        raise ValueError("the points must be finite")
    return np.array(r / BOHR)


def potential_into(basis, coords_bohr, points_bohr, dm, nuc=True, field=False, work=None):
    """``potential_batch`` for device tensors in atomic units (geometries [G, natm, 3] and points [G, M, 3] in Bohr, ``dm``
    [G, K, N, N]), on the current stream -> ``phi`` [G, K, M], or ``(phi, F [G, K, M, 3])`` with ``field``.  ``work``: a
    buffer of ``oovqe_gto_potential_work_size`` doubles to use instead of the basis' own."""
    _check_stack(basis, coords_bohr)
    G, N = int(coords_bohr.shape[0]), basis.nao
    if G > 65535:
        raise ValueError(f"{G} geometries in one call (at most 65535)")
    if not isinstance(points_bohr, torch.Tensor) or points_bohr.dim() != 3 or tuple(points_bohr.shape[::2]) != (G, 3):
        raise ValueError(f"points of shape {tuple(getattr(points_bohr, 'shape', ()))}, expected [{G}, M, 3]")
    M = int(points_bohr.shape[1])
    if not 1 <= M <= MAX_POINTS:
        raise ValueError(f"{M} points per geometry (1 .. {MAX_POINTS})")
    if not isinstance(dm, torch.Tensor) or dm.dim() != 4:
        raise ValueError(f"dm has shape {tuple(getattr(dm, 'shape', ()))}, expected [G, K, N, N]")
    K = int(dm.shape[1])
    if not 1 <= K <= MAX_GRAD_SETS:
        raise ValueError(f"{K} density sets per geometry (1 .. {MAX_GRAD_SETS})")
    _check_shape("dm", dm, (G, K, N, N))
    mask = _nuc_mask(nuc, K)
    dev = coords_bohr.device
    xyz = coords_bohr.to(F64).contiguous()
    pts = points_bohr.to(device=dev, dtype=F64).contiguous()
    dm = dm.to(device=dev, dtype=F64).contiguous()
    if not (bool(torch.isfinite(xyz).all()) and bool(torch.isfinite(pts).all()) and bool(torch.isfinite(dm).all())):
        raise ValueError("coordinates, points and densities must be finite")
    phi = torch.empty((G, K, M), dtype=F64, device=dev)
    F = torch.empty((G, K, M, 3), dtype=F64, device=dev) if field else None
    if G > 0:
        if work is None:
            work = potential_work(basis, dev, G, K)
        check(_lib.load().oovqe_gto_potential_batch(
            *_head(basis, dev), G, dptr(xyz), N, K, dptr(dm), M, dptr(pts), ctypes.c_uint(mask), dptr(phi), dptr(F),
            dptr(work), stream_ptr()), "oovqe_gto_potential_batch")
    return (phi, F) if field else phi


def potential_batch(basis, coords, points, dm, nuc=True, field=False):
    """The electrostatic potential (and field) the molecule makes at M points, for G geometries and K densities per
    geometry on the device (``oovqe_gto_potential_batch``, csrc/gto_potential.hip; no operator is stored):

        phi[g, k, m]  = (nuc_k) sum_A Z_A / |R_A - r_m|  -  sum_{mu nu} dm[g, k, mu, nu] <mu| 1 / |r - r_m| |nu>
        F[g, k, m, :] = - d phi[g, k, m] / d r_m

    over the functions of ``integrals_batch`` (s, p and d shells, both d forms).

    Args:
        basis: GTOBasis
        coords: geometries in the forms ``integrals_batch`` takes (Angstrom)
        points: [M, 3] shared by all geometries, or [G, M, 3], in Angstrom, 1 <= M <= ``MAX_POINTS``; a point may lie
            anywhere (on a nucleus, with ``nuc``, its own entries are inf / NaN and no other entry changes)
        dm: [G, N, N] or [G, K, N, N] device tensor, K = 1 .. ``MAX_GRAD_SETS``; NOT taken as symmetric: both (mu, nu)
            and (nu, mu) are read and only the symmetric part matters, so transition densities go in as they are
        nuc: add the potential of the nuclei: a bool, or one bool per set
        field: also return F

    Returns ``phi`` [G, K, M] in Hartree / e, or ``(phi, F)`` with F [G, K, M, 3] in Hartree / (e Bohr), on the device;
    the K axis is dropped for a 3-d ``dm``.  A (geometry, set, point) has the same bits wherever it stands in the stack,
    whatever the other points and sets, and with or without the field
    (``gaussian.potential_from_table`` is the host twin)."""
    xyz = basis.coordinates(coords) if not (isinstance(coords, torch.Tensor) and coords.is_cuda) else coords
    G = int(xyz.shape[0]) if xyz.ndim == 3 else 1
    N = basis.nao
    r = points_host(points, G)
    if not isinstance(dm, torch.Tensor) or dm.dim() not in (3, 4):
        raise ValueError(f"dm has shape {tuple(getattr(dm, 'shape', ()))}, expected [{G}, {N}, {N}] or [{G}, K, {N}, {N}]")
    squeeze = dm.dim() == 3
    d4 = dm[:, None] if squeeze else dm
    K = int(d4.shape[1])
    if not 1 <= K <= MAX_GRAD_SETS:
        raise ValueError(f"{K} density sets per geometry (1 .. {MAX_GRAD_SETS})")
    _check_shape("dm", d4, (G, K, N, N))
    _nuc_mask(nuc, K)
    if not bool(torch.isfinite(d4).all()):
        raise ValueError("the densities must be finite")
    device = _lib.require_device()
    out = potential_into(basis, coords_to_device(basis, xyz, device), torch.as_tensor(r).to(device), d4, nuc, field)
    if not squeeze:
        return out
    return (out[0][:, 0], out[1][:, 0]) if field else out[:, 0]


# ---- electron density, its gradient and orbital values at arbitrary points (csrc/gto_density.hip) ------------------------
def _points_call(basis, coords_bohr, points_bohr, x, name, inner):
    """The checks ``density_into`` and ``orbital_values_into`` share -> (G, M, K, xyz, pts, x) with contiguous float64
    tensors on the device of the geometries; ``x`` is [G, K, *inner]."""
    _check_stack(basis, coords_bohr)
    G = int(coords_bohr.shape[0])
    if G > 65535:
        raise ValueError(f"{G} geometries in one call (at most 65535)")
    if not isinstance(points_bohr, torch.Tensor) or points_bohr.dim() != 3 or tuple(points_bohr.shape[::2]) != (G, 3):
        raise ValueError(f"points of shape {tuple(getattr(points_bohr, 'shape', ()))}, expected [{G}, M, 3]")
    M = int(points_bohr.shape[1])
    if not 1 <= M <= MAX_POINTS:
        raise ValueError(f"{M} points per geometry (1 .. {MAX_POINTS})")
    if not isinstance(x, torch.Tensor) or x.dim() != 2 + len(inner):
        raise ValueError(f"{name} has shape {tuple(getattr(x, 'shape', ()))}, expected "
                         f"{'[G, K, N, N]' if name == 'dm' else '[G, N, ncol]'}")
    K = int(x.shape[1 if name == "dm" else 2])
    if not 1 <= K <= MAX_GRAD_SETS:
        raise ValueError(f"{K} {'density sets' if name == 'dm' else 'coefficient columns'} per geometry "
                         f"(1 .. {MAX_GRAD_SETS})")
    _check_shape(name, x, (G, K) + inner if name == "dm" else (G,) + inner + (K,))
    dev = coords_bohr.device
    xyz = coords_bohr.to(F64).contiguous()
    pts = points_bohr.to(device=dev, dtype=F64).contiguous()
    x = x.to(device=dev, dtype=F64).contiguous()
    if not (bool(torch.isfinite(xyz).all()) and bool(torch.isfinite(pts).all()) and bool(torch.isfinite(x).all())):
        raise ValueError(f"coordinates, points and {name} must be finite")
    return G, M, K, xyz, pts, x


DENSITY_LDS_COLUMNS = 121      # (DEN_LDS_MAX - sizeof(gto_den_lds_t)) / 512: LDS columns of 64 doubles a workgroup may hold


def density_max_sets(basis, gradient=False):
    """The most density sets one call of ``density_into`` takes for this basis: the density kernel holds K + nshell LDS
    columns (4 K + 2 nshell with the gradient) of ``DENSITY_LDS_COLUMNS``, and never more than ``MAX_GRAD_SETS`` sets.
    0: the table has too many shells for the kernel (more than 120, or 58 with the gradient)."""
    left = DENSITY_LDS_COLUMNS - basis.nshell * (2 if gradient else 1)
    return max(0, min(MAX_GRAD_SETS, left // (4 if gradient else 1)))


def density_into(basis, coords_bohr, points_bohr, dm, gradient=False):
    """``density_batch`` for device tensors in atomic units (geometries [G, natm, 3] and points [G, M, 3] in Bohr, ``dm``
    [G, K, N, N]), on the current stream -> ``rho`` [G, K, M], or ``(rho, drho [G, K, M, 3])`` with ``gradient``.  The
    entry has no work buffer.  Where the table has so many shells that the kernel's LDS holds fewer than K sets
    (``density_max_sets``), the sets go in several launches: a set has the same bits whatever the other sets of its
    launch."""
    N = basis.nao
    G, M, K, xyz, pts, dm = _points_call(basis, coords_bohr, points_bohr, dm, "dm", (N, N))
    dev = xyz.device
    step = density_max_sets(basis, gradient) or K            # (0: one call, which the library refuses with its message)
    rhos, grads = [], []
    for a in range(0, K, step):
        k = min(step, K - a)
        d = dm if k == K else dm[:, a:a + k].contiguous()
        rho = torch.empty((G, k, M), dtype=F64, device=dev)
        drho = torch.empty((G, k, M, 3), dtype=F64, device=dev) if gradient else None
        if G > 0:
            check(_lib.load().oovqe_gto_density_batch(
                *_head(basis, dev)[:-1], G, dptr(xyz), N, k, dptr(d), M, dptr(pts), dptr(rho), dptr(drho), stream_ptr()),
                "oovqe_gto_density_batch")
        rhos.append(rho)
        grads.append(drho)
    rho = rhos[0] if len(rhos) == 1 else torch.cat(rhos, dim=1)
    if not gradient:
        return rho
    return rho, (grads[0] if len(grads) == 1 else torch.cat(grads, dim=1))


def orbital_values_into(basis, coords_bohr, points_bohr, C, gradient=False):
    """``orbital_values_batch`` for device tensors in atomic units (points [G, M, 3] in Bohr, ``C`` [G, N, ncol]), on the
    current stream -> ``psi`` [G, ncol, M], or ``(psi, dpsi [G, ncol, M, 3])`` with ``gradient``."""
    N = basis.nao
    G, M, K, xyz, pts, C = _points_call(basis, coords_bohr, points_bohr, C, "C", (N,))
    dev = xyz.device
    psi = torch.empty((G, K, M), dtype=F64, device=dev)
    dpsi = torch.empty((G, K, M, 3), dtype=F64, device=dev) if gradient else None
    if G > 0:
        check(_lib.load().oovqe_gto_orbital_values_batch(
            *_head(basis, dev)[:-1], G, dptr(xyz), N, K, dptr(C), M, dptr(pts), dptr(psi), dptr(dpsi), stream_ptr()),
            "oovqe_gto_orbital_values_batch")
    return (psi, dpsi) if gradient else psi


def density_batch(basis, coords, points, dm, gradient=False):
    """The electron density (and its gradient) at M points, for G geometries and K densities per geometry on the device
    (``oovqe_gto_density_batch``, csrc/gto_density.hip):

        rho[g, k, m]     = sum_{mu nu} dm[g, k, mu, nu] chi_mu(r_m) chi_nu(r_m)
        drho[g, k, m, :] = d rho[g, k, m] / d r_m

    over the functions of ``integrals_batch`` (s, p and d shells, both d forms).

    Args:
        basis: GTOBasis
        coords: geometries in the forms ``integrals_batch`` takes (Angstrom)
        points: [M, 3] shared by all geometries, or [G, M, 3], in Angstrom, 1 <= M <= ``MAX_POINTS``; a point may lie
            anywhere (ON a nucleus the values are finite and exact; far outside they are exact zeros)
        dm: [G, N, N] or [G, K, N, N] device tensor, K = 1 .. ``MAX_GRAD_SETS``; NOT taken as symmetric: both (mu, nu)
            and (nu, mu) are read and only the symmetric part matters, so transition densities go in as they are
        gradient: also return drho

    Returns ``rho`` [G, K, M] in e / Bohr^3, or ``(rho, drho)`` with drho [G, K, M, 3] in e / Bohr^4, on the device; the K
    axis is dropped for a 3-d ``dm``.  A (geometry, set, point) has the same bits wherever it stands in the stack,
    whatever the other points and sets, and with or without the gradient (``gaussian.density_from_table`` is the host
    twin)."""
    xyz = basis.coordinates(coords) if not (isinstance(coords, torch.Tensor) and coords.is_cuda) else coords
    G = int(xyz.shape[0]) if xyz.ndim == 3 else 1
    N = basis.nao
    r = points_host(points, G)
    if not isinstance(dm, torch.Tensor) or dm.dim() not in (3, 4):
        raise ValueError(f"dm has shape {tuple(getattr(dm, 'shape', ()))}, expected [{G}, {N}, {N}] or [{G}, K, {N}, {N}]")
    squeeze = dm.dim() == 3
    d4 = dm[:, None] if squeeze else dm
    K = int(d4.shape[1])
    if not 1 <= K <= MAX_GRAD_SETS:
        raise ValueError(f"{K} density sets per geometry (1 .. {MAX_GRAD_SETS})")
    _check_shape("dm", d4, (G, K, N, N))
    if not bool(torch.isfinite(d4).all()):
        raise ValueError("the densities must be finite")
    device = _lib.require_device()
    out = density_into(basis, coords_to_device(basis, xyz, device), torch.as_tensor(r).to(device), d4, gradient)
    if not squeeze:
        return out
    return (out[0][:, 0], out[1][:, 0]) if gradient else out[:, 0]


def orbital_values_batch(basis, coords, points, C, gradient=False):
    """The values (and gradients) of orbitals at M points, for G geometries on the device
    (``oovqe_gto_orbital_values_batch``, csrc/gto_density.hip): ``psi[g, i, m] = sum_mu C[g, mu, i] chi_mu(r_m)``.

    Args:
        basis, coords, points: as for ``density_batch``
        C: [G, N, ncol] device tensor of coefficient columns (AO x orbital, as ``mo_coeff``), ncol = 1 ..
            ``MAX_GRAD_SETS``
        gradient: also return dpsi = d psi / d r_m

    Returns ``psi`` [G, ncol, M] in Bohr^-3/2, or ``(psi, dpsi [G, ncol, M, 3])``, on the device, with the guarantees of
    ``density_batch`` (``gaussian.orbital_values_from_table`` is the host twin)."""
    xyz = basis.coordinates(coords) if not (isinstance(coords, torch.Tensor) and coords.is_cuda) else coords
    G = int(xyz.shape[0]) if xyz.ndim == 3 else 1
    N = basis.nao
    r = points_host(points, G)
    if not isinstance(C, torch.Tensor) or C.dim() != 3:
        raise ValueError(f"C has shape {tuple(getattr(C, 'shape', ()))}, expected [{G}, {N}, ncol]")
    K = int(C.shape[2])
    if not 1 <= K <= MAX_GRAD_SETS:
        raise ValueError(f"{K} coefficient columns per geometry (1 .. {MAX_GRAD_SETS})")
    _check_shape("C", C, (G, N, K))
    if not bool(torch.isfinite(C).all()):
        raise ValueError("the coefficients must be finite")
    device = _lib.require_device()
    return orbital_values_into(basis, coords_to_device(basis, xyz, device), torch.as_tensor(r).to(device), C, gradient)


def sym_invsqrt_batch(S, out=None):
    """``S^-1/2`` (symmetric principal root) of a stack [G, n, n] of symmetric positive definite device matrices ->
    (X [G, n, n], info [G] int32 on the device: 0, or -1 where S has an eigenvalue below ``INVSQRT_MIN_EIG`` -- that
    matrix of X is NaN)."""
    lib = _lib.load()
    if S.dim() == 2:
        S = S[None]
    G, n = int(S.shape[0]), int(S.shape[-1])
    X = torch.empty_like(S) if out is None else out
    info = torch.empty(G, dtype=torch.int32, device=S.device)
    check(lib.oovqe_sym_invsqrt_batch(dptr(S), n, G, dptr(X), dptr(info, torch.int32), stream_ptr()),
          "oovqe_sym_invsqrt_batch")
    return X, info


def boys(nmax, T):
    """F_0 .. F_nmax (nmax <= 4 * MAX_L = 8) of the device Boys function for a device tensor T -> [len(T), nmax + 1]."""
    lib = _lib.load()
    T = T.contiguous()
    out = torch.empty((T.numel(), nmax + 1), dtype=F64, device=T.device)
    check(lib.oovqe_boys(int(nmax), dptr(T), ctypes.c_int64(T.numel()), dptr(out), stream_ptr()), "oovqe_boys")
    return out


def coords_to_device(basis, coords, device=None):
    """Geometries as ``GTOBasis.coordinates`` takes them -> [G, natm, 3] device tensor in Bohr."""
    device = _lib.require_device() if device is None else device
    if isinstance(coords, torch.Tensor) and coords.is_cuda:
        xyz = coords.to(F64)
        if xyz.dim() == 2:
            xyz = xyz[None]
        _check_stack(basis, xyz)
        return (xyz / BOHR).contiguous()
    return torch.as_tensor(basis.coordinates(coords) / BOHR).to(device)


def integrals_batch(basis, coords, check_overlap=True):
    """AO integrals of G geometries on the device.

    Args:
        basis: GTOBasis
        coords: [G, natm, 3] in Angstrom, or a list of geometries (see ``GTOBasis.coordinates``)
        check_overlap: read ``info`` back (G integers) and raise for a linearly dependent basis

    Returns a namespace of device tensors: ``overlap`` [G, N, N], ``int1e_ao`` [G, N, N] (kinetic + nuclear
    attraction), ``oao_coeff`` [G, N, N] (``S^-1/2``), ``nuc`` [G], ``int2e_ao`` [G, N, N, N, N], ``info`` [G]."""
    device = _lib.require_device()
    xyz = coords_to_device(basis, coords, device)
    G, N = int(xyz.shape[0]), basis.nao
    out = SimpleNamespace(
        overlap=torch.empty((G, N, N), dtype=F64, device=device),
        int1e_ao=torch.empty((G, N, N), dtype=F64, device=device),
        int2e_ao=torch.empty((G, N, N, N, N), dtype=F64, device=device),
        nuc=torch.empty(G, dtype=F64, device=device))
    integrals_into(basis, xyz, out.overlap, out.int1e_ao, out.int2e_ao, out.nuc)
    out.oao_coeff, out.info = sym_invsqrt_batch(out.overlap)
    if check_overlap:
        raise_if_dependent(out.info)
    return out


def raise_if_dependent(info, rows=None):
    bad = torch.nonzero(info < 0).flatten().tolist()
    if bad:
        if rows is not None:
            bad = [int(rows[b]) for b in bad]
        raise _lib.OovqeError(f"overlap of geometries {bad} has an eigenvalue below {INVSQRT_MIN_EIG}: "
                              "linearly dependent basis (atoms on top of each other?)")
