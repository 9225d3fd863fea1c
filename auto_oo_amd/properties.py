"""Multipole moments of the wave functions of a geometry stack on the device (auto_oo_amd/csrc/gto_moments.hip).

In atomic units, with the AO one-particle density ``D1`` of a state (``nucgrad.cas_ao_densities``), the moment
integrals ``M^c`` of ``gto.moment_integrals_batch`` and an origin ``O``

    mu_c = sum_A Z_A (R_A - O)^c - tr(D1 M^c),        c = x, y, z | xx, xy, xz, yy, yz, zz

(electrons count negative).  The dipole of a neutral molecule does not depend on ``O``; second moments do.  A
transition moment between two states is ``-tr(D^IJ M^c)`` with the symmetrised transition density and no nuclear term.
The contraction (``oovqe_gto_moments_expect_batch``) adds in a fixed order: a geometry's moments have the same bits
whatever stack, position, stream or chunk they are computed in.
"""
import torch

from . import _lib, gto
from ._lib import check, dptr, stream_ptr

F64 = torch.float64
DEBYE = 2.541746473            # Debye per atomic unit of dipole moment (e a0)
# places of xx, xy, xz, yy, yz, zz among the 9 components of order 2, as a symmetric 3 x 3 matrix
_SECOND = ((3, 4, 5), (4, 6, 7), (5, 7, 8))


def moments_expectation(moments, dens, charges=None, coords_bohr=None, origin_bohr=None, nuclear=True):
    """``out[g, k, c] = -tr(dens[g, k] moments[g, c]) + (nuclear[k]) sum_A Z_A (R_A - O)^c`` on the device.

    Args:
        moments: [G, 3 or 9, N, N] from ``gto.moment_integrals_into``
        dens: [G, nd, N, N] device tensor
        charges, coords_bohr: [natm], [G, natm, 3] device tensors (needed where ``nuclear`` is set)
        origin_bohr: the [G, 3] device tensor the integrals were made with, or None
        nuclear: bool, or one bool per density (a transition density takes no nuclear term)
    """
    lib = _lib.load()
    G, ncomp, N = int(moments.shape[0]), int(moments.shape[1]), int(moments.shape[-1])
    if dens.dim() != 4 or int(dens.shape[0]) != G or tuple(dens.shape[2:]) != (N, N):
        raise ValueError(f"dens has shape {tuple(dens.shape)}, expected [{G}, nd, {N}, {N}]")
    nd = int(dens.shape[1])
    flags = [bool(f) for f in nuclear] if hasattr(nuclear, "__len__") else [bool(nuclear)] * nd
    if len(flags) != nd:
        raise ValueError(f"nuclear holds {len(flags)} flags for {nd} densities")
    with_nuc = None
    natm = 1
    if any(flags):
        if charges is None or coords_bohr is None:
            raise ValueError("the nuclear term needs charges and coordinates")
        natm = int(coords_bohr.shape[1])
        with_nuc = torch.as_tensor(flags, dtype=torch.int32).to(moments.device)
    dens = dens.to(F64).contiguous()
    out = torch.empty((G, nd, ncomp), dtype=F64, device=moments.device)
    check(lib.oovqe_gto_moments_expect_batch(
        dptr(moments), ncomp, N, G, dptr(dens), nd, natm, dptr(charges), dptr(coords_bohr), dptr(origin_bohr),
        dptr(with_nuc, torch.int32), dptr(out), stream_ptr()), "oovqe_gto_moments_expect_batch")
    return out


def multipole_moments(basis, coords_bohr, dens, order=1, origin=None, nuclear=True):
    """Multipole moments of densities ``dens`` at the geometries ``coords_bohr``, in atomic units.

    Args:
        basis: gto.GTOBasis
        coords_bohr: [G, natm, 3] device tensor in Bohr
        dens: AO one-particle densities, [G, N, N] or [G, nd, N, N] device tensor (``D1`` of
            ``nucgrad.cas_ao_densities``; taken as symmetric)
        order: 1 -> the components x, y, z; 2 -> x, y, z, xx, xy, xz, yy, yz, zz
        origin: [3] or [G, 3] in Bohr (default: the origin of the coordinates)
        nuclear: add ``sum_A Z_A (R_A - O)^c``; one flag for all densities or one per density

    Returns [G, 3 or 9] for ``dens`` [G, N, N], otherwise [G, nd, 3 or 9], on the device.  ``split_moments`` turns
    the 9 components into the dipole and the 3 x 3 matrix of second moments."""
    ncomp = gto.moment_components(order)
    if not isinstance(coords_bohr, torch.Tensor) or not coords_bohr.is_cuda:
        raise ValueError("coords_bohr must be a [G, natm, 3] device tensor in Bohr")
    xyz = coords_bohr.to(F64).contiguous()
    G, N, dev = int(xyz.shape[0]), basis.nao, xyz.device
    single = dens.dim() == 3
    d = dens[:, None] if single else dens
    o = gto.origin_to_device(origin, G, dev)
    M = torch.empty((G, ncomp, N, N), dtype=F64, device=dev)
    gto.moment_integrals_into(basis, xyz, M, order, o)
    out = moments_expectation(M, d, basis.device_tables(dev).charges, xyz, o, nuclear)
    return out[:, 0] if single else out


def split_moments(values):
    """[..., 9] (order 2) -> (dipole [..., 3], second moments [..., 3, 3], symmetric)."""
    idx = torch.as_tensor(_SECOND, device=values.device)
    return values[..., :3], values[..., idx]


def traceless_quadrupole(second):
    """Traceless quadrupole ``Theta_ij = (3 Q_ij - delta_ij tr Q) / 2`` from second moments ``Q`` [..., 3, 3] (torch
    tensor or numpy array; the convention of Buckingham: ``Theta_zz = sum q (3 z^2 - r^2) / 2``)."""
    if isinstance(second, torch.Tensor):
        eye = torch.eye(3, dtype=second.dtype, device=second.device)
        trace = second.diagonal(dim1=-2, dim2=-1).sum(-1)
    else:
        import numpy as np
        second = np.asarray(second)
        eye = np.eye(3)
        trace = np.trace(second, axis1=-2, axis2=-1)
    return 1.5 * second - 0.5 * trace[..., None, None] * eye


# ---- uniform grids for densities and orbitals (host only; the values come from gto.density_batch and the batch methods) ----
def cube_grid(coords, spacing, margin):
    """A uniform grid around a molecule -> (origin [3] in Angstrom, shape (nx, ny, nz), points [nx ny nz, 3] in Angstrom, x
    the slowest and z the fastest index, as a cube file lists them).  ``coords`` [natm, 3], ``spacing`` and ``margin``
    (the least distance from an atom to the faces of the box) are in Angstrom.  At most ``gto.MAX_POINTS`` points go into
    one call of the device functions: cut ``points`` into slabs."""
    import numpy as np
    R = np.asarray(coords, dtype=float).reshape(-1, 3)
    h, margin = float(spacing), float(margin)
    if not (h > 0.0 and margin >= 0.0 and np.isfinite(R).all()):
        raise ValueError(f"spacing = {spacing!r} (> 0), margin = {margin!r} (>= 0), finite coordinates")
    lo, hi = R.min(axis=0) - margin, R.max(axis=0) + margin
    shape = tuple(int(n) for n in np.ceil((hi - lo) / h - 1e-9).astype(int) + 1)
    origin = 0.5 * (lo + hi) - 0.5 * h * (np.asarray(shape) - 1)
    axes = [origin[d] + h * np.arange(shape[d]) for d in range(3)]
    points = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
    return origin, shape, points


def integrate_grid(values, spacing):
    """``sum_m values[..., m] h^3`` with h = ``spacing`` (Angstrom, as ``cube_grid`` takes it) in Bohr: the integral of
    values in atomic units (e / Bohr^3 -> e) over a uniform grid, along the last axis (tensor or array; with a trailing
    component axis, as a gradient has, move the points last first)."""
    h = float(spacing) / gto.BOHR
    return values.sum(-1) * h ** 3


def write_cube(path, symbols, coords, origin, shape, spacing, values, comment="auto_oo_amd"):
    """A Gaussian cube file of ``values`` [nx ny nz] (or [nx, ny, nz]; atomic units, tensor or array) on the grid of
    ``cube_grid``: ``coords`` [natm, 3], ``origin`` and ``spacing`` in Angstrom (the file holds Bohr)."""
    import numpy as np
    v = values.detach().cpu().numpy() if isinstance(values, torch.Tensor) else np.asarray(values)
    v = np.asarray(v, dtype=float)
    nx, ny, nz = (int(n) for n in shape)
    if v.size != nx * ny * nz:
        raise ValueError(f"{v.size} values for a grid of {nx} x {ny} x {nz} points")
    R = np.asarray(coords, dtype=float).reshape(-1, 3) / gto.BOHR
    if len(symbols) != R.shape[0]:
        raise ValueError(f"{len(symbols)} symbols for {R.shape[0]} atoms")
    o, h = np.asarray(origin, dtype=float).reshape(3) / gto.BOHR, float(spacing) / gto.BOHR
    with open(path, "w") as fh:
        fh.write(f"{comment}\nx slowest, z fastest; atomic units\n")
        fh.write(f"{R.shape[0]:5d}{o[0]:12.6f}{o[1]:12.6f}{o[2]:12.6f}\n")
        for d, n in enumerate((nx, ny, nz)):
            step = [h if k == d else 0.0 for k in range(3)]
            fh.write(f"{n:5d}{step[0]:12.6f}{step[1]:12.6f}{step[2]:12.6f}\n")
        for sym, xyz in zip(symbols, R):
            z = gto._Z[str(sym).capitalize()]
            fh.write(f"{z:5d}{float(z):12.6f}{xyz[0]:12.6f}{xyz[1]:12.6f}{xyz[2]:12.6f}\n")
        for row in v.reshape(nx * ny, nz):
            for k in range(0, nz, 6):
                fh.write("".join(f"{x:13.5E}" for x in row[k:k + 6]) + "\n")


def fit_esp_charges(phi, points_bohr, coords_bohr, total_charge=0.0):
    """Atomic charges fitted to an electrostatic potential: the ``q`` [..., natm] that minimise
    ``sum_m (phi[..., m] - sum_A q_A / |r_m - R_A|)^2`` under ``sum_A q_A = total_charge`` (a Lagrange constraint), batched
    over the leading axes of ``phi``.

    Args:
        phi: [..., M] potential at the points in Hartree / e (``gto.potential_batch``, the batch methods), tensor or array
        points_bohr: [M, 3] or [..., M, 3] in Bohr, M >= natm, none of them on an atom
        coords_bohr: [natm, 3] or [..., natm, 3] in Bohr
        total_charge: a number, or one per leading index of ``phi``

    No points are selected and no restraints applied: which points enter (a shell of van der Waals surfaces, a grid) is
    the caller's business.  The constraint is eliminated (``q = total_charge / natm + Z y`` with the columns of Z orthogonal
    to (1, .., 1)) and the rest solved by a QR factorisation, so the conditioning is that of the design matrix, not of
    its square; the result is the solution of the normal equations with the multiplier.  Runs on the device of ``phi``."""
    phi = torch.as_tensor(phi).to(F64)
    dev = phi.device
    r = torch.as_tensor(points_bohr).to(device=dev, dtype=F64)
    R = torch.as_tensor(coords_bohr).to(device=dev, dtype=F64)
    if r.dim() < 2 or R.dim() < 2 or r.shape[-1] != 3 or R.shape[-1] != 3 or phi.dim() < 1:
        raise ValueError(f"phi {tuple(phi.shape)}, points {tuple(r.shape)}, atoms {tuple(R.shape)}: expected [..., M], "
                         "[..., M, 3], [..., natm, 3]")
    M, n = int(r.shape[-2]), int(R.shape[-2])
    if int(phi.shape[-1]) != M or M < n or n < 1:
        raise ValueError(f"{int(phi.shape[-1])} values of phi at {M} points for {n} atoms (M >= natm points, one value each)")
    lead = tuple(phi.shape[:-1])
    A = 1.0 / (r[..., :, None, :] - R[..., None, :, :]).norm(dim=-1)
    if not (bool(torch.isfinite(A).all()) and bool(torch.isfinite(phi).all())):
        raise ValueError("phi must be finite and no point may lie on an atom")
    A = A.expand(lead + (M, n))
    Q = torch.as_tensor(total_charge, dtype=F64, device=dev).expand(lead)
    q0 = (Q / n)[..., None].expand(lead + (n,))
    if n == 1:
        return q0.clone()
    Z = torch.linalg.qr(torch.ones((n, 1), dtype=F64, device=dev), mode="complete").Q[:, 1:]
    rhs = phi - (A @ q0[..., None])[..., 0]
    Qm, Rm = torch.linalg.qr(A @ Z)
    y = torch.linalg.solve_triangular(Rm, Qm.transpose(-1, -2) @ rhs[..., None], upper=True)[..., 0]
    return q0 + y @ Z.T
