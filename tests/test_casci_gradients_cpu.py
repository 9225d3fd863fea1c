"""Host-side checks of the gradient-sets contraction and the CASCI gradients (no device): the new symbols, the size
function and its limits, the argument errors raised before anything touches a device, and ``branching_plane``."""
import ctypes
import os
import re
from collections import namedtuple

import numpy as np
import pytest
import torch

from tests import _gto_d as D
from auto_oo_amd import _lib, batch, gto, nucgrad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("oovqe_gto_gradient_sets_work_size", "oovqe_gto_gradient_sets_batch")
F64 = torch.float64


def test_new_symbols_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "oovqe.h")) as fh:
        header = fh.read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    m = re.search(r"#define OOVQE_GTO_GRAD_MAX_SETS (\d+)", header)
    assert m and int(m.group(1)) == gto.MAX_GRAD_SETS == 10
    m = re.search(r"#define OOVQE_GTO_GRAD_SETS_TILE (\d+)", header)
    assert m and int(m.group(1)) == gto.GRAD_SETS_TILE
    assert 1 <= gto.GRAD_SETS_TILE <= gto.MAX_GRAD_SETS
    for name in ("gradient_sets_into", "gradient_sets_batch"):
        assert hasattr(gto, name), name
    assert hasattr(nucgrad, "branching_plane")
    assert hasattr(batch.OO_pqc_batch, "casci_nuclear_gradients")
    assert batch.CASCIGradients._fields == ("energies", "ci", "gradients")


def test_work_size_grows_with_the_sets_and_refuses_what_is_out_of_range():
    lib = _lib.load()
    nshell, natm, G = 9, 5, 4
    size = [lib.oovqe_gto_gradient_sets_work_size(nshell, 3, natm, G, k) for k in range(1, gto.MAX_GRAD_SETS + 1)]
    assert all(b > a > 0 for a, b in zip(size, size[1:]))
    # one set: the records of the single-set entry, so its size; every further set adds the same records
    assert size[0] == lib.oovqe_gto_gradient_work_size(nshell, 3, natm, G)
    base = lib.oovqe_gto_work_size(nshell, 3, G)
    assert all(s - base == (k + 1) * (size[0] - base) for k, s in enumerate(size))
    for bad in (0, gto.MAX_GRAD_SETS + 1, -1):
        assert lib.oovqe_gto_gradient_sets_work_size(nshell, 3, natm, G, bad) == -1, bad          # OOVQE_ERR_ARG
        msg = lib.oovqe_last_error().decode()
        assert "oovqe_gto_gradient_sets_work_size" in msg and f"nset = {bad}" in msg
    assert lib.oovqe_gto_gradient_sets_work_size(nshell, gto.MAX_PRIM, natm, G, 3) > 0
    assert lib.oovqe_gto_gradient_sets_work_size(nshell, gto.MAX_PRIM + 1, natm, G, 3) == -1
    msg = lib.oovqe_last_error().decode()
    assert "oovqe_gto_gradient_sets_work_size" in msg and f"{gto.MAX_PRIM + 1} primitives" in msg
    assert lib.oovqe_gto_gradient_sets_work_size(nshell, 3, 0, G, 3) == -1
    assert "natm" in lib.oovqe_last_error().decode()


def test_host_side_argument_errors():
    basis = gto.GTOBasis(["H", "F"])
    N = basis.nao
    xyz = torch.zeros((2, 2, 3), dtype=F64)
    z = lambda *shape: torch.zeros(shape, dtype=F64)                 # noqa: E731
    with pytest.raises(ValueError, match="coordinates"):
        gto.gradient_sets_into(basis, xyz[:, :1], dm1=z(2, 3, N, N))
    with pytest.raises(ValueError, match="at least one"):
        gto.gradient_sets_into(basis, xyz)
    with pytest.raises(ValueError, match="density sets"):
        gto.gradient_sets_into(basis, xyz, dm1=z(2, gto.MAX_GRAD_SETS + 1, N, N))
    with pytest.raises(ValueError, match="density sets"):
        gto.gradient_sets_into(basis, xyz, dm1=z(2, 0, N, N))
    with pytest.raises(ValueError, match="dm1"):
        gto.gradient_sets_into(basis, xyz, dm1=z(1, 3, N, N))
    with pytest.raises(ValueError, match="wq"):
        gto.gradient_sets_into(basis, xyz, dm1=z(2, 3, N, N), wq=z(2, 2, N, N))
    with pytest.raises(ValueError, match="dm2"):
        gto.gradient_sets_into(basis, xyz, dm1=z(2, 3, N, N), dm2=z(2, 3, N, N, N))
    with pytest.raises(ValueError, match="dm2"):
        gto.gradient_sets_into(basis, xyz, dm2=z(2))
    with pytest.raises(ValueError, match="nuc"):
        gto.gradient_sets_into(basis, xyz, dm1=z(2, 3, N, N), nuc=[True, False])
    d = D.m1_basis("spherical")
    with pytest.raises(NotImplementedError, match="d shells"):
        gto.gradient_sets_into(d, torch.zeros((1, d.natm, 3), dtype=F64), dm1=z(1, 2, d.nao, d.nao))
    with pytest.raises(NotImplementedError, match="d shells"):
        gto.gradient_sets_batch(d, D.M1_XYZ[None], dm1=z(1, 2, d.nao, d.nao))


def test_state_pairs_and_transition_sets():
    assert nucgrad.state_pairs(1) == []
    assert nucgrad.state_pairs(3) == [(1, 0), (2, 0), (2, 1)]
    assert len(nucgrad.state_pairs(4)) + 4 == gto.MAX_GRAD_SETS
    rng = np.random.default_rng(3)
    v = torch.as_tensor(rng.standard_normal((2, 3, 5)))
    p = nucgrad.polarisation_vectors(v)
    assert tuple(p.shape) == (2, 9, 5) and torch.equal(p[:, :3], v)
    # a quadratic form of the vectors: the half-difference is the symmetrised transition element
    A = torch.as_tensor(rng.standard_normal((5, 5)))
    q = torch.einsum("gki,ij,gkj->gk", p, A, p)
    t = nucgrad.transition_sets(q, 3)
    assert tuple(t.shape) == (2, 6)
    As = 0.5 * (A + A.T)
    for n, (i, j) in enumerate(nucgrad.state_pairs(3)):
        want = torch.einsum("gi,ij,gj->g", v[:, i], As, v[:, j])
        assert (t[:, 3 + n] - want).abs().max().item() < 1e-13
    one = nucgrad.polarisation_vectors(v[:, :1])
    assert torch.equal(one, v[:, :1]) and torch.equal(nucgrad.transition_sets(q[:, :1], 1), q[:, :1])


def test_branching_plane_on_a_hand_made_result():
    grads = torch.as_tensor(np.random.default_rng(5).standard_normal((2, 3, 3, 4, 3)))
    grads = 0.5 * (grads + grads.transpose(1, 2))
    res = batch.CASCIGradients(None, None, grads)
    g, h = nucgrad.branching_plane(res, 0, 2)
    assert torch.equal(g, 0.5 * (grads[:, 2, 2] - grads[:, 0, 0])) and torch.equal(h, grads[:, 0, 2])
    g2, h2 = nucgrad.branching_plane(res, 2, 0)
    assert torch.equal(g2, -g) and torch.equal(h2, h)
    other = namedtuple("Other", "gradients")(grads)                  # anything with .gradients
    assert torch.equal(nucgrad.branching_plane(other, 1, 2)[1], grads[:, 1, 2])
    for i, j in ((0, 0), (0, 3), (-1, 1)):
        with pytest.raises(ValueError):
            nucgrad.branching_plane(res, i, j)
