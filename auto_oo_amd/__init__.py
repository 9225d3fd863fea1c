"""auto_oo_amd: MI355X-native orbital-optimized VQE engine behind auto_oo's cost-function API.

Export list mirrors the reference's src/auto_oo/__init__.py:3-27 for the hot path
(OO_energy / OO_pqc / Parameterized_circuit and helpers); ``Moldata`` is the array-backed stand-in
for ``Moldata_pyscf``.  Importing the package needs the built HIP library
(auto_oo_amd/lib/liboovqe_hip.so): there is no CPU fallback.
"""
from . import _lib

_lib.load()   # fail loudly at import time when the HIP extension is missing

from .pqc import Parameterized_circuit                      # noqa: E402
from .moldata import Moldata, ao_to_oao, get_formal_geo                     # noqa: E402
from .gaussian import Moldata_sto3g                         # noqa: E402
from . import gto, nucgrad, properties, scf                 # noqa: E402
from .scf import RHFResult, rhf_batch                       # noqa: E402
from .gto import GTOBasis, integrals_batch, moment_integrals_batch   # noqa: E402
from .properties import DEBYE, multipole_moments, traceless_quadrupole     # noqa: E402
from .oo_pqc import OO_pqc                                  # noqa: E402
from .batch import OO_pqc_batch                             # noqa: E402
from .oo_energy import (                                    # noqa: E402
    OO_energy,
    mo_ao_to_mo_oao,
    int1e_transform,
    int2e_transform,
    general_4index_transform,
    uniform_4index_transform,
    vector_to_skew_symmetric,
    skew_symmetric_to_vector,
    non_redundant_indices,
)
from .newton_raphson import NewtonStep, BatchedNewtonStep   # noqa: E402
from .berry import ActiveSpaceRotation, bogoliubov_atob_cas, state_overlap   # noqa: E402
from .excitations import generalized_pair_doubles           # noqa: E402
from .active_space import active_space_integrals, molecular_hamiltonian_coefficients   # noqa: E402
from .ci import casci, CIResult, transition_rdm1            # noqa: E402
from . import overlaps                                      # noqa: E402
from .overlaps import sector_overlaps, state_overlaps_oao, track_roots, apply_tracking   # noqa: E402
from .gto import cross_overlap_batch, overlap_connection_batch   # noqa: E402
from .gto import point_charge_integrals_batch, point_charge_gradient_batch   # noqa: E402
from .gto import potential_batch, potential_into   # noqa: E402
from .gto import density_batch, density_into, orbital_values_batch   # noqa: E402
from . import adapt                                         # noqa: E402
from .adapt import AdaptResult, OperatorPool, adapt_vqe     # noqa: E402
from . import ensemble                                      # noqa: E402
from .ensemble import SA_OO_pqc_batch, StateEnsemble, check_ensemble, singlet_states   # noqa: E402

__all__ = [
    "Parameterized_circuit", "Moldata", "Moldata_sto3g", "GTOBasis", "integrals_batch", "gto", "scf", "nucgrad", "RHFResult", "rhf_batch", "ao_to_oao", "get_formal_geo", "OO_pqc", "OO_pqc_batch", "OO_energy", "mo_ao_to_mo_oao",
    "int1e_transform", "int2e_transform", "general_4index_transform", "uniform_4index_transform",
    "vector_to_skew_symmetric", "skew_symmetric_to_vector", "non_redundant_indices", "NewtonStep", "BatchedNewtonStep", "ActiveSpaceRotation", "bogoliubov_atob_cas", "state_overlap",
    "generalized_pair_doubles", "active_space_integrals", "molecular_hamiltonian_coefficients", "casci", "CIResult",
    "properties", "moment_integrals_batch", "multipole_moments", "traceless_quadrupole", "DEBYE",
    "overlaps", "sector_overlaps", "state_overlaps_oao", "track_roots", "apply_tracking", "cross_overlap_batch",
    "transition_rdm1", "overlap_connection_batch", "point_charge_integrals_batch", "point_charge_gradient_batch",
    "potential_batch", "potential_into", "density_batch", "density_into", "orbital_values_batch",
    "adapt", "AdaptResult", "OperatorPool", "adapt_vqe",
    "ensemble", "SA_OO_pqc_batch", "StateEnsemble", "check_ensemble", "singlet_states",
]
