"""Host side of the device Hartree-Fock solver (auto_oo_amd/scf.py): the C ABI's declarations and the scope errors,
which are raised before any device is asked for.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import auto_oo_amd as aoo
from auto_oo_amd import _lib, gto, scf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("oovqe_fock_jk_batch", "oovqe_sym_eig_batch", "oovqe_rhf_work_size", "oovqe_rhf_batch")


def test_new_symbols_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "oovqe.h")) as fh:
        hdr = fh.read()
    declared = set(re.findall(r"\b(oovqe_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    assert scf.MAX_N == gto.INVSQRT_MAX_N
    # the size function answers without a device, and refuses what the kernels do not cover
    n, G = 13, 16
    assert lib.oovqe_rhf_work_size(n, G) >= G * (3 + 8 + 8 + 1) * n * n
    assert lib.oovqe_rhf_work_size(scf.MAX_N, 1) > 0
    assert lib.oovqe_rhf_work_size(scf.MAX_N + 1, 1) < 0
    assert b"n = 65" in lib.oovqe_last_error()
    assert lib.oovqe_rhf_work_size(13, 0) < 0


def test_the_library_refuses_sizes_out_of_scope_before_any_launch():
    lib = _lib.load()
    null = [None] * 4
    outs = [None] * 8

    def call(n, n_occ, batch, max_cycle=200):
        return lib.oovqe_rhf_batch(*null, n, n_occ, batch, 1e-12, 1e-9, max_cycle, *outs, None, None)
    assert call(65, 8, 1) < 0 and b"n = 65" in lib.oovqe_last_error()
    assert call(13, 13, 1) < 0 and b"n_occ" in lib.oovqe_last_error()
    assert call(13, 0, 1) < 0 and b"n_occ" in lib.oovqe_last_error()
    assert call(13, 8, 0) < 0 and b"batch" in lib.oovqe_last_error()
    assert call(13, 8, 1, max_cycle=0) < 0 and b"max_cycle" in lib.oovqe_last_error()
    assert lib.oovqe_fock_jk_batch(None, None, 65, 1, None, None, None) < 0
    assert lib.oovqe_sym_eig_batch(None, 65, 1, None, None, None, None) < 0


def test_scope_errors_are_raised_without_a_device():
    z = lambda *s: torch.zeros(s, dtype=torch.float64)          # noqa: E731
    with pytest.raises(ValueError, match="N = 65"):
        scf.rhf_batch(z(65, 65), z(1, 1, 1, 1), z(65, 65), 3)
    with pytest.raises(ValueError, match="n_occ = 4"):
        scf.rhf_batch(z(2, 4, 4), z(2, 4, 4, 4, 4), z(2, 4, 4), 4)
    with pytest.raises(ValueError, match="n_occ = 0"):
        scf.rhf_batch(z(4, 4), z(4, 4, 4, 4), z(4, 4), 0)
    with pytest.raises(ValueError, match="int2e has shape"):
        scf.rhf_batch(z(4, 4), z(4, 4, 4), z(4, 4), 2)
    with pytest.raises(ValueError, match="same number of geometries"):
        scf.rhf_batch(z(2, 4, 4), z(3, 4, 4, 4, 4), z(2, 4, 4), 2)
    with pytest.raises(ValueError, match="even electron count"):
        scf.check_scope(13, nelectron=15)
    with pytest.raises(ValueError, match="n = 65"):
        scf.sym_eigh_batch(z(65, 65))
    with pytest.raises(ValueError, match="N = 65"):
        scf.fock_jk(z(1, 1, 1, 1), z(65, 65))
    scf.check_scope(13, nelectron=16)
    scf.check_scope(64, n_occ=63)


def test_moldata_run_rhf_checks_the_scope_first_and_keeps_its_default():
    rng = np.random.default_rng(0)
    s = np.eye(4)
    h = rng.standard_normal((4, 4))
    g = np.zeros((4, 4, 4, 4))
    odd = aoo.Moldata(h + h.T, g, s, 0.0, 3)
    with pytest.raises(ValueError, match="even electron count"):
        odd.run_rhf(device=True)
    full = aoo.Moldata(h + h.T, g, s, 0.0, 8)
    with pytest.raises(ValueError, match="n_occ = 4"):
        full.run_rhf(device=True)
    with pytest.raises(RuntimeError, match="no RHF engine"):
        full.run_rhf()
    given = aoo.Moldata(h + h.T, g, s, 0.0, 4, mo_coeff=np.eye(4))
    given.run_rhf()
    assert np.array_equal(given.hf.mo_coeff, np.eye(4))
    assert aoo.RHFResult is scf.RHFResult and aoo.rhf_batch is scf.rhf_batch
    assert scf.RHFResult._fields[:8] == ("mo_coeff", "oao_mo_coeff", "mo_energy", "e_elec", "converged",
                                         "iterations", "diis_error", "info")
