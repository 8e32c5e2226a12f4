"""mcpar_amd -- MI355X-native parallel Metropolis-Hastings engine (drop-in for the chain-step hot
path of rplzzz/mcpar).  The product is libmcx.so (hand-written HIP for gfx950 behind the C ABI of
include/mcx.h); this package is the thin ctypes host binding used by bench.py and the tests.

There is no CPU fallback: importing works anywhere, but every compute call needs the built HIP
library and a GPU, and raises McxError otherwise.
"""
from ._lib import McxError, load, lib_path  # noqa: F401
from .engine import (Engine, VL_DEVICE, VL_SOURCE, VL_DUALGAUSS, VL_GAUSSIAN, VL_GAUSSMIX, VL_HOST,  # noqa: F401
                     VL_ROSENBROCK1, VL_ROSENBROCK2, debug_normals, debug_numerics, device_info,
                     make_vlfunc, vlfunc_eval)
from .engine import (DerivedStore, debug_derive_compile, debug_draw_indices, derive_linear, derive_rows,  # noqa: F401
                     derive_source, user_source_available)
from .engine import RowSet, clip_rows, debug_clip_thresholds, debug_store_geometry  # noqa: F401
from .engine import debug_chains_geometry, keep_chains, rows_chain_table, select_chains_rows  # noqa: F401
from .engine import (debug_density2d_finish, debug_density2d_grid, debug_rows_density2d_bins,  # noqa: F401
                     rows_density2d)
from .engine import (Proposal, evidence_iterate, evidence_proposal, proposal_from_modes, rows_evidence)  # noqa: F401
from .engine import profile_drop, profile_interval, rows_profile, rows_profile2d  # noqa: F401
from .engine import mutinfo_finish, rows_mutual_info  # noqa: F401

__all__ = ["Engine", "McxError", "load", "lib_path", "make_vlfunc", "vlfunc_eval", "device_info", "RowSet", "clip_rows",
           "debug_clip_thresholds", "debug_store_geometry", "rows_density2d", "debug_density2d_grid", "debug_density2d_finish",
           "debug_rows_density2d_bins", "rows_chain_table", "keep_chains", "select_chains_rows", "debug_chains_geometry",
           "debug_numerics", "debug_normals", "DerivedStore", "derive_linear", "derive_source", "derive_rows",
           "debug_draw_indices", "debug_derive_compile", "user_source_available", "Proposal", "rows_evidence", "evidence_proposal",
           "evidence_iterate", "proposal_from_modes", "rows_profile", "rows_profile2d", "profile_interval", "profile_drop",
           "rows_mutual_info", "mutinfo_finish"]
