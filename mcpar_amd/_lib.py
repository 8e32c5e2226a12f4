"""ctypes loader for libmcx.so.  Fails loudly when the HIP library has not been built."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))


class McxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("mcx status %d: %s" % (code, msg))
        self.code = code


HOSTFN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float))
XCHGFN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p)
OUTFN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int)
SINKFN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float))
TEXTSINKFN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t)


class VLFunc(C.Structure):
    _fields_ = [("kind", C.c_int), ("d", C.c_int), ("ncomp", C.c_int),
                ("params", C.POINTER(C.c_float)), ("fn", HOSTFN), ("ctx", C.c_void_p)]


class Derive(C.Structure):
    """include/mcx.h mcx_derive"""
    _fields_ = [("kind", C.c_int), ("nout", C.c_int), ("npar", C.c_int), ("par", C.POINTER(C.c_float)),
                ("source", C.c_char_p)]


class DensitySpecC(C.Structure):
    """include/mcx.h mcx_density_spec"""
    _fields_ = [("n", C.c_int), ("adjust", C.c_double), ("clip_lo", C.c_double), ("clip_hi", C.c_double),
                ("bw", C.POINTER(C.c_double)), ("from_", C.POINTER(C.c_double)), ("to", C.POINTER(C.c_double))]


class Density2dSpecC(C.Structure):
    """include/mcx.h mcx_density2d_spec"""
    _fields_ = [("g", C.c_int), ("adjust", C.c_double), ("clip_lo", C.c_double), ("clip_hi", C.c_double),
                ("bw", C.POINTER(C.c_double)), ("from_", C.POINTER(C.c_double)), ("to", C.POINTER(C.c_double)),
                ("npairs", C.c_int), ("pairs", C.POINTER(C.c_int))]


class ClipSpecC(C.Structure):
    """include/mcx.h mcx_clip_spec"""
    _fields_ = [("qlo", C.c_double), ("qhi", C.c_double), ("ll_hi", C.c_double),
                ("lo", C.POINTER(C.c_double)), ("hi", C.POINTER(C.c_double))]


class StoreGeometry(C.Structure):
    """include/mcx.h mcx_store_geometry"""
    _fields_ = [(n, C.c_longlong) for n in ("nrows", "derive_rows", "derive_lds_bytes", "derive_workgroups", "clip_rows",
                                            "clip_mask_words", "clip_lds_bytes", "clip_workgroups", "clip_scan_blocks",
                                            "rank_tiles", "rank_step_chunk", "rank_grid_y", "gather_chunk_rows")]


class ChainRule(C.Structure):
    """include/mcx.h mcx_chain_rule"""
    _fields_ = [("z", C.c_double), ("min_moves", C.c_longlong), ("max_stay", C.c_longlong),
                ("use_col", C.POINTER(C.c_ubyte))]


class ChainsGeometry(C.Structure):
    """include/mcx.h mcx_chains_geometry"""
    _fields_ = [(n, C.c_longlong) for n in ("block", "lds_bytes", "series_tile_cols", "series_tile_chains", "series_col_tiles",
                                            "series_workgroups", "series_ll_workgroups", "rows_lanes_per_chain",
                                            "rows_values_per_lane", "rows_chains_per_workgroup", "rows_workgroups",
                                            "select_vec4", "select_items", "select_workgroups")]


class StepRule(C.Structure):
    """include/mcx.h mcx_step_rule"""
    _fields_ = [("tol_mean", C.c_double), ("tol_sd", C.c_double), ("ref_frac", C.c_double), ("use_col", C.POINTER(C.c_ubyte))]


class SteptableGeometry(C.Structure):
    """include/mcx.h mcx_steptable_geometry"""
    _fields_ = [(n, C.c_longlong) for n in ("block", "moments_tile_cols", "moments_stride_chains", "moments_col_tiles",
                                            "moments_workgroups", "moments_lds_bytes", "select_slots", "select_tile_cols",
                                            "select_stride_chains", "select_col_tiles", "select_workgroups", "select_lds_bytes",
                                            "rows_lanes_per_chain", "rows_values_per_lane", "rows_chains_per_pass", "rows_chunks",
                                            "rows_workgroups", "scratch_doubles", "scratch_words")]


class TextSpec(C.Structure):
    """include/mcx.h mcx_text_spec"""
    _fields_ = [("ncol", C.c_int), ("nc", C.c_int), ("skip_lines", C.c_int64), ("max_rows", C.c_int64), ("piece_bytes", C.c_size_t)]


class TextReport(C.Structure):
    """include/mcx.h mcx_text_report"""
    _fields_ = [(n, C.c_int64) for n in ("nrows", "nlines", "ntokens", "nfallback", "npieces")] + [("ncol", C.c_int)]


class CompareSpecC(C.Structure):
    """include/mcx.h mcx_compare_spec"""
    _fields_ = [("flags", C.c_int)]


class CompareGeometry(C.Structure):
    """include/mcx.h mcx_compare_geometry"""
    _fields_ = [(n, C.c_longlong) for n in ("block", "tile_keys", "tiles_a", "tiles_b", "window_lds_keys", "lds_bytes",
                                            "group_cols", "scratch_bytes_per_col", "sort_tiles_a", "sort_tiles_b",
                                            "bounds_workgroups_a", "bounds_workgroups_b", "step_chunk_a", "step_chunk_b",
                                            "grid_y_a", "grid_y_b")]


class EnergySpecC(C.Structure):
    """include/mcx.h mcx_energy_spec"""
    _fields_ = [("n_a", C.c_int), ("n_b", C.c_int), ("nperm", C.c_int), ("seed", C.c_uint32), ("flags", C.c_uint)]


class EnergyResultC(C.Structure):
    """include/mcx.h mcx_energy_result"""
    _fields_ = ([(n, C.c_double) for n in ("e", "h", "mean_ab", "mean_aa", "mean_bb", "p_value")] + [("nge", C.c_longlong)] +
                [(n, C.c_int) for n in ("n_a", "n_b", "nperm", "nused")] + [("na_rows", C.c_longlong), ("nb_rows", C.c_longlong)])


class EnergyGeometry(C.Structure):
    """include/mcx.h mcx_energy_geometry"""
    _fields_ = [(n, C.c_longlong) for n in ("block", "tile_rows", "tiles", "slab_rows", "slabs", "label_cols", "label_blocks",
                                            "chunk_blocks", "chunks", "col_chunk", "workgroups", "lds_bytes", "scratch_bytes")]


class MutinfoSpecC(C.Structure):
    """include/mcx.h mcx_mutinfo_spec"""
    _fields_ = [("n", C.c_int), ("k", C.c_int), ("nperm", C.c_int), ("seed", C.c_uint32), ("flags", C.c_uint), ("npairs", C.c_int),
                ("pairs", C.POINTER(C.c_int))]


class MutinfoResultC(C.Structure):
    """include/mcx.h mcx_mutinfo_result"""
    _fields_ = [("n_rows", C.c_longlong)] + [(n, C.c_int) for n in ("n_sel", "ndup", "m", "k", "npairs", "nperm", "nused")]


class MutinfoGeometry(C.Structure):
    """include/mcx.h mcx_mutinfo_geometry"""
    _fields_ = [(n, C.c_longlong) for n in ("block", "queries_per_lane", "tile_rows", "stage_rows", "stages", "tiles", "workgroups",
                                            "lds_bytes", "scratch_bytes")]


class WeightsC(C.Structure):
    """include/mcx.h mcx_weights"""
    _fields_ = [("kind", C.c_int), ("logw", C.POINTER(C.c_float)), ("store", C.c_void_p), ("col", C.c_int), ("scale", C.c_double)]


class ReweightResultC(C.Structure):
    """include/mcx.h mcx_reweight_result"""
    _fields_ = [("n", C.c_longlong), ("nzero", C.c_longlong), ("lwmax", C.c_double), ("sumq", C.c_longlong),
                ("sumq2_hi", C.c_ulonglong), ("sumq2_lo", C.c_ulonglong), ("ess_kish", C.c_double), ("log_mean_w", C.c_double),
                ("tail_m", C.c_longlong), ("khat", C.c_double), ("tail_sigma", C.c_double), ("flags", C.c_int), ("reserved", C.c_int)]


class ReweightGeometry(C.Structure):
    """include/mcx.h mcx_reweight_geometry"""
    _fields_ = [(n, C.c_longlong) for n in ("block", "scan_tile_rows", "scan_tiles", "hist_targets", "hist_prefixes", "hist_launches",
                                            "hist_tile_cols", "hist_lds_bytes", "hist_lds_budget", "tail_m", "sort_tiles",
                                            "draw_workgroups", "scratch_bytes", "scan_tiles_per_lane", "hist_step_chunks")]


class IntervalSpecC(C.Structure):
    """include/mcx.h mcx_interval_spec"""
    _fields_ = [("nmass", C.c_int), ("nprobs", C.c_int), ("mass", C.POINTER(C.c_double)), ("probs", C.POINTER(C.c_double))]


class IntervalsGeometry(C.Structure):
    """include/mcx.h mcx_intervals_geometry"""
    _fields_ = [(n, C.c_longlong) for n in ("block", "window_tile", "window_tiles", "slab_entries", "slab_bytes", "reduce_workgroups",
                                            "pick_ranks", "transforms", "sort_tiles", "step_chunk", "grid_y", "group_cols", "groups",
                                            "store_scratch_bytes", "scratch_bytes_per_col")]


class LagcovSpecC(C.Structure):
    """include/mcx.h mcx_lagcov_spec"""
    _fields_ = [("max_lag", C.c_int), ("nlags_out", C.c_int), ("with_ll", C.c_int)]


class LagcovResultC(C.Structure):
    """include/mcx.h mcx_lagcov_result"""
    _fields_ = [("N", C.c_longlong)] + [(n, C.c_int) for n in ("p", "s", "k_used", "lags_used", "lags_computed", "flags")] + \
               [(n, C.c_double) for n in ("mess", "logdet_lambda", "logdet_sigma")]


class LagcovGeometry(C.Structure):
    """include/mcx.h mcx_lagcov_geometry"""
    _fields_ = [(n, C.c_longlong) for n in ("block", "window_lags", "rows_per_iteration", "units", "workgroups", "tiles",
                                            "pairs_lag0", "pairs", "slab_rows", "windows", "launches", "lags_computed", "scratch_bytes",
                                            "units_lag0", "workgroups_lag0")]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("naccept_burn", "naccept_main", "nsteps_burn", "nsteps_main",
                                          "remote_steps", "remote_passes", "exchanges", "kernel_launches",
                                          "remote_pairs", "remote_pairs_evaluated", "meet_timeouts", "meet_timeouts_total",
                                          "small_n_launches", "small_n_blocks_per_lane", "exchange_waits",
                                          "exchange_wait_ns")]


K_NAMES = ("fused_burn", "fused_main", "propose", "eval", "accept", "remote", "tuner", "misc", "remote_sweep",
           "gen_normals", "run_small", "remote_screen")


class PlanItem(C.Structure):
    _fields_ = [("kind", C.c_int), ("first", C.c_int), ("nsteps", C.c_int), ("aux", C.c_int)]


class ModesSpecC(C.Structure):
    """include/mcx.h mcx_modes_spec"""
    _fields_ = [("k", C.c_int), ("max_iter", C.c_int), ("scale", C.c_int), ("seed_rows", C.c_int), ("seed", C.c_uint32),
                ("centres", C.POINTER(C.c_double))]


class ModesResultC(C.Structure):
    """include/mcx.h mcx_modes_result"""
    _fields_ = [("k", C.c_int), ("iters", C.c_int), ("flags", C.c_int), ("reserved", C.c_int), ("n", C.c_longlong),
                ("n_nonfinite", C.c_longlong), ("n_changed", C.c_longlong), ("inertia", C.c_double)]


class ModesGeometry(C.Structure):
    """include/mcx.h mcx_modes_geometry"""
    _fields_ = [(n, C.c_longlong) for n in ("block", "rows_per_tile", "tiles", "workgroups", "lane_groups", "centre_blocks",
                                            "uniform_centres", "sum_subgroups", "table_columns", "table_subgroups",
                                            "assign_lds_bytes", "table_lds_bytes", "mark_workgroups", "mark_mask_words",
                                            "chains_workgroups", "steps_workgroups", "scratch_bytes")]


class EvidenceMixtureC(C.Structure):
    """include/mcx.h mcx_evidence_mixture"""
    _fields_ = [("k", C.c_int), ("reserved", C.c_int), ("weights", C.POINTER(C.c_double)), ("centres", C.POINTER(C.c_double)),
                ("covs", C.POINTER(C.c_double)), ("scale", C.c_double)]


class EvidenceSpecC(C.Structure):
    """include/mcx.h mcx_evidence_spec"""
    _fields_ = [("ndraw", C.c_longlong), ("seed", C.c_uint32), ("fit_steps", C.c_int), ("use_neff", C.c_int), ("max_iter", C.c_int),
                ("tol", C.c_double), ("scale", C.c_double)]


class EvidenceResultC(C.Structure):
    """include/mcx.h mcx_evidence_result"""
    _fields_ = [("n1", C.c_longlong), ("n2", C.c_longlong), ("k", C.c_int), ("fit_steps", C.c_int)] + \
               [(n, C.c_double) for n in ("neff", "lstar", "log_z", "se", "re2_draws", "re2_rows", "ess_f2", "log_z_is", "log_z_ris")] + \
               [("ndraw_zero", C.c_longlong), ("iters", C.c_int), ("flags", C.c_int)]


class EvidenceGeometry(C.Structure):
    """include/mcx.h mcx_evidence_geometry"""
    _fields_ = [(n, C.c_longlong) for n in ("block", "tile_rows", "slices", "sweep_tiles", "sweep_workgroups", "sweep_max_workgroups",
                                            "sweep_lds_bytes", "use_mfma", "w_chunk_rows", "draw_rows", "draw_workgroups", "draw_lds_bytes",
                                            "terms_workgroups_rows", "terms_workgroups_draws", "scratch_bytes")]


class ProfileSpecC(C.Structure):
    """include/mcx.h mcx_profile_spec"""
    _fields_ = [("n", C.c_int), ("clip_lo", C.c_double), ("clip_hi", C.c_double), ("from_", C.POINTER(C.c_double)),
                ("to", C.POINTER(C.c_double)), ("nlevels", C.c_int), ("levels", C.POINTER(C.c_double)), ("levels_are_drops", C.c_int)]


class Profile2dSpecC(C.Structure):
    """include/mcx.h mcx_profile2d_spec"""
    _fields_ = [("g", C.c_int), ("clip_lo", C.c_double), ("clip_hi", C.c_double), ("from_", C.POINTER(C.c_double)),
                ("to", C.POINTER(C.c_double)), ("npairs", C.c_int), ("pairs", C.POINTER(C.c_int)), ("nlevels", C.c_int),
                ("levels", C.POINTER(C.c_double)), ("levels_are_drops", C.c_int)]


class ProfileGeometry(C.Structure):
    """include/mcx.h mcx_profile_geometry"""
    _fields_ = [(n, C.c_longlong) for n in ("block", "tile_columns", "chains_per_workgroup", "column_tiles", "chain_blocks", "chunk_steps",
                                            "chunks", "workgroups", "lds_bytes", "unroll", "pair_block", "pair_chunk_rows", "pair_chunks",
                                            "pair_workgroups", "pair_lds_bytes", "scratch_bytes", "keys_workgroups",
                                            "keys_max_workgroups")]


class Profile(C.Structure):
    _fields_ = [("ms", C.c_double * 12), ("launches", C.c_uint64 * 12), ("chain_steps", C.c_uint64 * 12)]


def lib_path():
    # MCX_LIBMCX: another build of the same library (tools/persist_ab.py times variants of one kernel on one box)
    return os.environ.get("MCX_LIBMCX") or os.path.join(HERE, "libmcx.so")


_lib = None
ABI_VERSION = 5  # include/mcx.h MCX_ABI_VERSION
ERR_NONFINITE = 8  # include/mcx.h MCX_ERR_NONFINITE: McxError.code of a Murray step that could not end


def load():
    """dlopen libmcx.so and declare every entry point of include/mcx.h"""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise McxError(-1, "%s not found: build it with `make lib` (hipcc --offload-arch=gfx950); "
                           "there is no CPU fallback" % p)
    L = C.CDLL(p)
    fp, u32p, vp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_void_p
    dp = C.POINTER(C.c_double)
    sig = {
        "mcx_vlfunc_eval": [C.POINTER(VLFunc), C.c_int, fp, fp],
        "mcx_create": [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                       C.c_float, C.c_float, C.c_float, C.c_int, C.c_uint32],
        "mcx_destroy": [vp],
        "mcx_run": [vp, C.c_int, C.c_int, fp, C.POINTER(VLFunc), fp],
        "mcx_stage_pinit": [vp, fp],
        "mcx_gen_local": [vp, C.c_uint32, fp, fp, fp],
        "mcx_gen_remote": [vp, C.c_uint32, fp, fp, fp, fp, fp, fp, C.POINTER(C.c_int)],
        "mcx_covar_setup": [vp, fp, fp],
        "mcx_set_exchange": [vp, XCHGFN, vp],
        "mcx_set_output_hook": [vp, OUTFN, vp],
        "mcx_set_sink": [vp, SINKFN, vp, C.c_int],
        "mcx_set_text_sink": [vp, TEXTSINKFN, vp, C.c_int],
        "mcx_sink_text": [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)],
        "mcx_set_option": [vp, C.c_int, C.c_int64],
        "mcx_get_counters": [vp, C.POINTER(Counters)],
        "mcx_get_state": [vp, fp], "mcx_get_loglike": [vp, fp], "mcx_get_mean": [vp, fp],
        "mcx_get_var": [vp, fp], "mcx_get_musigall": [vp, fp], "mcx_get_chol": [vp, fp],
        "mcx_synchronize": [vp],
        "mcx_get_accept_counts": [vp, u32p],
        "mcx_get_accept_mask": [vp, C.POINTER(C.c_uint8)],
        "mcx_get_tuner_trace": [vp, fp, C.c_int, C.POINTER(C.c_int)],
        "mcx_samples_steps": [vp, C.POINTER(C.c_int)],
        "mcx_samples_copy": [vp, C.c_int, C.c_int, fp],
        "mcx_samples_text": [vp, C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)],
        "mcx_format_rows": [fp, C.c_size_t, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)],
        "mcx_samples_maxlike": [vp, fp, fp],
        "mcx_samples_summary": [vp, C.c_int, C.c_int, dp, C.c_int, vp, dp],
        "mcx_rows_summary": [fp, C.c_int, C.c_int, C.c_int, dp, C.c_int, vp, dp],
        "mcx_debug_summary_finish": [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, dp, C.c_int, fp,
                                     C.c_longlong, dp, C.c_int, C.c_int, vp, dp, C.POINTER(C.c_int)],
        "mcx_debug_summary_windows": [vp, C.c_int, C.c_int, C.POINTER(C.c_int)],
        "mcx_debug_select_step": [C.POINTER(C.c_ulonglong), C.c_longlong, C.POINTER(C.c_int), C.POINTER(C.c_longlong)],
        "mcx_debug_rows_acov": [fp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp],
        "mcx_samples_covariance": [vp, C.c_int, C.c_int, dp, dp, C.POINTER(C.c_int)],
        "mcx_rows_covariance": [fp, C.c_int, C.c_int, C.c_int, dp, dp, C.POINTER(C.c_int)],
        "mcx_proposal_from_cov": [C.c_int, dp, C.c_int, C.c_double, fp],
        "mcx_debug_covariance_times": [vp, C.c_int, C.c_int, dp],
        "mcx_samples_rank_summary": [vp, C.c_int, C.c_int, vp],
        "mcx_rows_rank_summary": [fp, C.c_int, C.c_int, C.c_int, vp],
        "mcx_debug_rows_rank_transform": [fp, C.c_int, C.c_int, C.c_int, C.c_int, dp, fp],
        "mcx_debug_normal_quantile": [dp, C.c_int, dp],
        "mcx_debug_rank_summary_times": [vp, C.c_int, C.c_int, dp],
        "mcx_samples_derive": [vp, C.c_int, C.c_int, C.POINTER(Derive), C.POINTER(vp)],
        "mcx_rows_derive": [fp, C.c_int, C.c_int, C.c_int, C.POINTER(Derive), C.POINTER(vp)],
        "mcx_store_destroy": [vp],
        "mcx_store_shape": [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)],
        "mcx_store_copy": [vp, C.c_int, C.c_int, fp],
        "mcx_store_summary": [vp, dp, C.c_int, vp, dp],
        "mcx_store_rank_summary": [vp, vp],
        "mcx_store_covariance": [vp, dp, dp, C.POINTER(C.c_int)],
        "mcx_debug_derive_compile": [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_size_t)],
        "mcx_debug_derive_times": [vp, C.c_int, C.c_int, C.POINTER(Derive), dp],
        "mcx_samples_draw": [vp, C.c_int, C.c_int, C.c_uint32, C.c_int64, fp, C.POINTER(C.c_int64)],
        "mcx_store_draw": [vp, C.c_uint32, C.c_int64, fp, C.POINTER(C.c_int64)],
        "mcx_debug_draw_indices": [C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_int64)],
        "mcx_samples_density": [vp, C.c_int, C.c_int, C.POINTER(DensitySpecC), vp, dp, dp],
        "mcx_rows_density": [fp, C.c_int, C.c_int, C.c_int, C.POINTER(DensitySpecC), vp, dp, dp],
        "mcx_store_density": [vp, C.POINTER(DensitySpecC), vp, dp, dp],
        "mcx_debug_density_grid": [C.c_longlong, C.c_double, C.c_double, C.c_float, C.c_float, C.c_double, C.c_double,
                                   C.c_double, C.c_double, C.c_int, C.c_int, C.POINTER(DensitySpecC), vp],
        "mcx_debug_density_finish": [vp, C.POINTER(C.c_ulonglong), C.c_int, dp, dp],
        "mcx_debug_rows_density_bins": [fp, C.c_int, C.c_int, C.c_int, dp, dp, C.POINTER(C.c_ulonglong)],
        "mcx_debug_density_times": [vp, C.c_int, C.c_int, C.POINTER(DensitySpecC), dp],
        "mcx_debug_store_density_times": [vp, C.POINTER(DensitySpecC), dp],
        "mcx_samples_density2d": [vp, C.c_int, C.c_int, C.POINTER(Density2dSpecC), vp, dp, vp, dp],
        "mcx_rows_density2d": [fp, C.c_int, C.c_int, C.c_int, C.POINTER(Density2dSpecC), vp, dp, vp, dp],
        "mcx_store_density2d": [vp, C.POINTER(Density2dSpecC), vp, dp, vp, dp],
        "mcx_debug_density2d_grid": [C.c_longlong, C.c_double, C.c_double, C.c_float, C.c_float, C.c_double, C.c_double,
                                     C.c_double, C.c_double, C.c_int, C.c_int, C.POINTER(Density2dSpecC), vp],
        "mcx_debug_density2d_finish": [vp, vp, C.c_int, C.POINTER(C.c_ulonglong), C.c_int, dp],
        "mcx_debug_rows_density2d_bins": [fp, C.c_int, C.c_int, C.c_int, dp, dp, C.c_int, C.c_int, C.POINTER(C.c_int),
                                          C.POINTER(C.c_ulonglong)],
        "mcx_debug_density2d_times": [vp, C.c_int, C.c_int, C.POINTER(Density2dSpecC), dp],
        "mcx_samples_clip": [vp, C.c_int, C.c_int, C.POINTER(ClipSpecC), vp, C.POINTER(C.c_longlong), C.POINTER(vp)],
        "mcx_rows_clip": [fp, C.c_int, C.c_int, C.c_int, C.POINTER(ClipSpecC), vp, C.POINTER(C.c_longlong), C.POINTER(vp)],
        "mcx_store_clip": [vp, C.POINTER(ClipSpecC), vp, C.POINTER(C.c_longlong), C.POINTER(vp)],
        "mcx_rowset_destroy": [vp],
        "mcx_rowset_shape": [vp, C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.POINTER(C.c_longlong)],
        "mcx_rowset_copy": [vp, C.c_longlong, C.c_longlong, fp],
        "mcx_rowset_index": [vp, C.c_longlong, C.c_longlong, C.POINTER(C.c_longlong)],
        "mcx_rowset_draw": [vp, C.c_uint32, C.c_int64, fp, C.POINTER(C.c_int64)],
        "mcx_rowset_store": [vp, C.c_longlong, C.c_int, C.c_int, C.POINTER(vp)],
        "mcx_debug_clip_thresholds": [C.c_int, dp, C.POINTER(ClipSpecC), dp, dp],
        "mcx_debug_clip_times": [vp, C.c_int, C.c_int, C.POINTER(ClipSpecC), dp],
        "mcx_debug_store_geometry": [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(StoreGeometry)],
        "mcx_debug_fill_allocations": [C.c_int, C.POINTER(C.c_ulonglong)],
        "mcx_debug_fill_scratch": [vp, vp, C.c_int, C.POINTER(C.c_size_t)],
        "mcx_samples_chain_table": [vp, C.c_int, C.c_int, vp, vp],
        "mcx_rows_chain_table": [fp, C.c_int, C.c_int, C.c_int, vp, vp],
        "mcx_store_chain_table": [vp, vp, vp],
        "mcx_chains_keep": [C.c_int, C.c_int, vp, vp, C.POINTER(ChainRule), C.POINTER(C.c_int), dp, C.POINTER(C.c_int)],
        "mcx_samples_select_chains": [vp, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(vp)],
        "mcx_rows_select_chains": [fp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(vp)],
        "mcx_store_select_chains": [vp, C.POINTER(C.c_int), C.c_int, C.POINTER(vp)],
        "mcx_debug_chains_geometry": [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(ChainsGeometry)],
        "mcx_debug_chain_table_times": [vp, C.c_int, C.c_int, dp],
        "mcx_samples_step_table": [vp, C.c_int, C.c_int, dp, C.c_int, vp, vp, dp],
        "mcx_rows_step_table": [fp, C.c_int, C.c_int, C.c_int, dp, C.c_int, vp, vp, dp],
        "mcx_store_step_table": [vp, dp, C.c_int, vp, vp, dp],
        "mcx_steps_settle": [C.c_int, C.c_int, vp, C.POINTER(StepRule), vp, C.POINTER(C.c_int)],
        "mcx_debug_steptable_geometry": [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(SteptableGeometry)],
        "mcx_debug_step_table_times": [vp, C.c_int, C.c_int, dp, C.c_int, dp],
        "mcx_text_store": [C.c_char_p, C.c_size_t, C.POINTER(TextSpec), C.POINTER(vp), C.POINTER(TextReport)],
        "mcx_text_rows": [C.c_char_p, C.c_size_t, C.POINTER(TextSpec), fp, C.c_int64, C.POINTER(TextReport)],
        "mcx_file_store": [C.c_char_p, C.POINTER(TextSpec), C.POINTER(vp), C.POINTER(TextReport)],
        "mcx_debug_parse_token": [C.c_char_p, C.c_size_t, u32p, C.POINTER(C.c_int)],
        "mcx_debug_text_times": [C.c_char_p, C.c_size_t, C.POINTER(TextSpec), C.POINTER(TextReport), dp],
        "mcx_store_compare": [vp, vp, C.POINTER(CompareSpecC), vp],
        "mcx_rows_compare": [fp, C.c_int, C.c_int, fp, C.c_int, C.c_int, C.c_int, C.POINTER(CompareSpecC), vp],
        "mcx_samples_compare": [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(CompareSpecC), vp],
        "mcx_samples_compare_store": [vp, C.c_int, C.c_int, vp, C.POINTER(CompareSpecC), vp],
        "mcx_ks_prob": [C.c_double, C.c_double, C.c_double, dp, dp],
        "mcx_debug_compare_geometry": [C.c_longlong, C.c_longlong, C.c_int, C.POINTER(CompareGeometry)],
        "mcx_debug_compare_store_geometry": [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(CompareGeometry)],
        "mcx_debug_compare_times": [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(CompareSpecC), dp],
        "mcx_store_energy": [vp, vp, C.POINTER(EnergySpecC), C.POINTER(EnergyResultC), vp, dp],
        "mcx_rows_energy": [fp, C.c_int, C.c_int, fp, C.c_int, C.c_int, C.c_int, C.POINTER(EnergySpecC), C.POINTER(EnergyResultC), vp, dp],
        "mcx_samples_energy": [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(EnergySpecC), C.POINTER(EnergyResultC), vp, dp],
        "mcx_samples_energy_store": [vp, C.c_int, C.c_int, vp, C.POINTER(EnergySpecC), C.POINTER(EnergyResultC), vp, dp],
        "mcx_debug_energy_labels": [C.c_uint32, C.c_int, C.c_int, C.c_int, vp],
        "mcx_debug_energy_sums": [fp, C.c_int, C.c_int, fp, C.c_int, C.c_int, C.c_int, C.POINTER(EnergySpecC), dp],
        "mcx_debug_energy_geometry": [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(EnergyGeometry)],
        "mcx_debug_energy_times": [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(EnergySpecC), dp],
        "mcx_store_reweight": [vp, C.POINTER(WeightsC), dp, C.c_int, C.POINTER(ReweightResultC), vp, dp],
        "mcx_samples_reweight": [vp, C.c_int, C.c_int, C.POINTER(WeightsC), dp, C.c_int, C.POINTER(ReweightResultC), vp, dp],
        "mcx_rows_reweight": [fp, C.c_int, C.c_int, C.c_int, C.POINTER(WeightsC), dp, C.c_int, C.POINTER(ReweightResultC), vp, dp],
        "mcx_store_resample": [vp, C.POINTER(WeightsC), C.c_uint32, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(C.c_int64)],
        "mcx_samples_resample": [vp, C.c_int, C.c_int, C.POINTER(WeightsC), C.c_uint32, C.c_int, C.c_int, C.POINTER(vp),
                                 C.POINTER(C.c_int64)],
        "mcx_rows_resample": [fp, C.c_int, C.c_int, C.c_int, C.POINTER(WeightsC), C.c_uint32, C.c_int, C.c_int, C.POINTER(vp),
                              C.POINTER(C.c_int64)],
        "mcx_khat_of_tail": [dp, C.c_longlong, dp, dp, C.POINTER(C.c_int)],
        "mcx_debug_reweight_q": [vp, fp, C.c_int, C.c_int, C.c_int, C.POINTER(WeightsC), u32p, dp],
        "mcx_debug_reweight_geometry": [C.c_longlong, C.c_int, C.c_int, C.c_longlong, C.POINTER(ReweightGeometry)],
        "mcx_debug_reweight_store_geometry": [C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.POINTER(ReweightGeometry)],
        "mcx_debug_reweight_times": [vp, C.c_int, C.c_int, C.POINTER(WeightsC), dp, C.c_int, C.c_uint32, C.c_int, C.c_int, dp],
        "mcx_samples_intervals": [vp, C.c_int, C.c_int, C.POINTER(IntervalSpecC), vp, vp, vp],
        "mcx_rows_intervals": [fp, C.c_int, C.c_int, C.c_int, C.POINTER(IntervalSpecC), vp, vp, vp],
        "mcx_store_intervals": [vp, C.POINTER(IntervalSpecC), vp, vp, vp],
        "mcx_beta_quantile": [C.c_double, C.c_double, C.c_double, dp],
        "mcx_intervals_quantile_ranks": [C.c_longlong, C.c_double, C.c_double, dp, dp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)],
        "mcx_debug_intervals_geometry": [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(IntervalsGeometry)],
        "mcx_debug_intervals_times": [vp, C.c_int, C.c_int, C.POINTER(IntervalSpecC), dp],
        "mcx_samples_lagcov": [vp, C.c_int, C.c_int, C.POINTER(LagcovSpecC), C.POINTER(LagcovResultC), vp, dp, dp],
        "mcx_rows_lagcov": [fp, C.c_int, C.c_int, C.c_int, C.POINTER(LagcovSpecC), C.POINTER(LagcovResultC), vp, dp, dp],
        "mcx_store_lagcov": [vp, C.POINTER(LagcovSpecC), C.POINTER(LagcovResultC), vp, dp, dp],
        "mcx_mess_finish": [C.c_int, C.c_int, C.c_longlong, dp, C.POINTER(C.c_ubyte), C.POINTER(LagcovResultC), vp, dp],
        "mcx_debug_lagcov_geometry": [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(LagcovGeometry)],
        "mcx_debug_lagcov_times": [vp, C.c_int, C.c_int, C.POINTER(LagcovSpecC), C.POINTER(LagcovResultC), dp],
        "mcx_samples_modes": [vp, C.c_int, C.c_int, C.POINTER(ModesSpecC), C.POINTER(ModesResultC), vp, dp, dp, dp, dp, dp, C.POINTER(vp)],
        "mcx_rows_modes": [fp, C.c_int, C.c_int, C.c_int, C.POINTER(ModesSpecC), C.POINTER(ModesResultC), vp, dp, dp, dp, dp, dp,
                           C.POINTER(vp)],
        "mcx_store_modes": [vp, C.POINTER(ModesSpecC), C.POINTER(ModesResultC), vp, dp, dp, dp, dp, dp, C.POINTER(vp)],
        "mcx_modes_destroy": [vp],
        "mcx_modes_shape": [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)],
        "mcx_modes_labels": [vp, C.c_longlong, C.c_longlong, C.POINTER(C.c_ubyte)],
        "mcx_modes_chain_table": [vp, vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)],
        "mcx_modes_indicator_store": [vp, C.POINTER(vp)],
        "mcx_samples_mode_rows": [vp, C.c_int, C.c_int, vp, C.c_int, C.POINTER(vp)],
        "mcx_rows_mode_rows": [fp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.POINTER(vp)],
        "mcx_store_mode_rows": [vp, vp, C.c_int, C.POINTER(vp)],
        "mcx_modes_seed": [fp, C.c_longlong, C.c_int, C.c_int, C.c_uint32, dp, C.POINTER(C.c_longlong)],
        "mcx_debug_modes_assign": [fp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, C.POINTER(C.c_ubyte), dp,
                                   C.POINTER(C.c_longlong), dp],
        "mcx_debug_modes_geometry": [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(ModesGeometry)],
        "mcx_debug_modes_times": [vp, C.c_int, C.c_int, C.POINTER(ModesSpecC), C.POINTER(ModesResultC), dp],
        "mcx_samples_evidence": [vp, C.c_int, C.c_int, C.POINTER(VLFunc), C.POINTER(EvidenceSpecC), C.POINTER(EvidenceMixtureC),
                                 C.POINTER(EvidenceResultC)],
        "mcx_rows_evidence": [fp, C.c_int, C.c_int, C.c_int, C.POINTER(VLFunc), C.POINTER(EvidenceSpecC), C.POINTER(EvidenceMixtureC),
                              C.POINTER(EvidenceResultC)],
        "mcx_store_evidence": [vp, C.POINTER(VLFunc), C.POINTER(EvidenceSpecC), C.POINTER(EvidenceMixtureC), C.POINTER(EvidenceResultC)],
        "mcx_evidence_proposal": [C.c_int, C.POINTER(EvidenceMixtureC), dp, dp, dp],
        "mcx_evidence_iterate": [dp, C.c_longlong, dp, C.c_longlong, C.c_double, C.c_double, C.c_int, C.POINTER(EvidenceResultC)],
        "mcx_debug_evidence_logg": [fp, C.c_longlong, C.c_int, C.POINTER(EvidenceMixtureC), dp],
        "mcx_debug_evidence_draws": [C.c_int, C.POINTER(EvidenceMixtureC), C.POINTER(VLFunc), C.c_uint32, C.c_longlong, fp,
                                     C.POINTER(C.c_int), dp, fp],
        "mcx_debug_evidence_l": [fp, C.c_int, C.c_int, C.c_int, C.POINTER(VLFunc), C.POINTER(EvidenceSpecC), C.POINTER(EvidenceMixtureC),
                                 C.POINTER(EvidenceResultC), dp, dp],
        "mcx_debug_evidence_geometry": [C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.POINTER(EvidenceGeometry)],
        "mcx_debug_evidence_times": [vp, C.c_int, C.c_int, C.POINTER(VLFunc), C.POINTER(EvidenceSpecC), C.POINTER(EvidenceMixtureC),
                                     C.POINTER(EvidenceResultC), dp],
        "mcx_samples_profile": [vp, C.c_int, C.c_int, C.POINTER(ProfileSpecC), vp, C.POINTER(C.c_ulonglong), fp, C.POINTER(C.c_longlong), fp,
                                dp, dp, vp, fp],
        "mcx_rows_profile": [fp, C.c_int, C.c_int, C.c_int, C.POINTER(ProfileSpecC), vp, C.POINTER(C.c_ulonglong), fp, C.POINTER(C.c_longlong),
                             fp, dp, dp, vp, fp],
        "mcx_store_profile": [vp, C.POINTER(ProfileSpecC), vp, C.POINTER(C.c_ulonglong), fp, C.POINTER(C.c_longlong), fp, dp, dp, vp, fp],
        "mcx_samples_profile2d": [vp, C.c_int, C.c_int, C.POINTER(Profile2dSpecC), vp, vp, C.POINTER(C.c_ulonglong), fp,
                                  C.POINTER(C.c_longlong), fp, fp, dp, C.POINTER(C.c_longlong)],
        "mcx_rows_profile2d": [fp, C.c_int, C.c_int, C.c_int, C.POINTER(Profile2dSpecC), vp, vp, C.POINTER(C.c_ulonglong), fp,
                               C.POINTER(C.c_longlong), fp, fp, dp, C.POINTER(C.c_longlong)],
        "mcx_store_profile2d": [vp, C.POINTER(Profile2dSpecC), vp, vp, C.POINTER(C.c_ulonglong), fp, C.POINTER(C.c_longlong), fp, fp, dp,
                                C.POINTER(C.c_longlong)],
        "mcx_profile_interval": [C.c_int, dp, dp, C.c_double, dp, dp, C.POINTER(C.c_int), C.POINTER(C.c_int)],
        "mcx_profile_drop": [C.c_double, C.c_int, dp],
        "mcx_debug_profile_finish": [C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), fp, C.c_ulonglong, C.c_int, dp, C.c_int, fp,
                                     C.POINTER(C.c_longlong), dp, dp, vp, C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.POINTER(C.c_int)],
        "mcx_debug_rows_profile_bins": [fp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong),
                                        C.POINTER(C.c_ulonglong)],
        "mcx_debug_profile_geometry": [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(ProfileGeometry)],
        "mcx_debug_profile_times": [vp, C.c_int, C.c_int, C.POINTER(ProfileSpecC), dp],
        "mcx_debug_store_profile_times": [vp, C.POINTER(ProfileSpecC), dp],
        "mcx_debug_profile2d_times": [vp, C.c_int, C.c_int, C.POINTER(Profile2dSpecC), dp],
        "mcx_store_mutinfo": [vp, C.POINTER(MutinfoSpecC), C.POINTER(MutinfoResultC), vp, vp, dp],
        "mcx_rows_mutinfo": [fp, C.c_int, C.c_int, C.c_int, C.POINTER(MutinfoSpecC), C.POINTER(MutinfoResultC), vp, vp, dp],
        "mcx_samples_mutinfo": [vp, C.c_int, C.c_int, C.POINTER(MutinfoSpecC), C.POINTER(MutinfoResultC), vp, vp, dp],
        "mcx_debug_mutinfo_rows": [C.c_longlong, C.c_int, C.POINTER(C.c_longlong)],
        "mcx_debug_mutinfo_perm": [C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_int)],
        "mcx_debug_mutinfo_psi": [C.c_int, dp],
        "mcx_mutinfo_finish": [dp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, dp, C.POINTER(C.c_longlong)],
        "mcx_debug_mutinfo_points": [fp, C.c_int, C.c_int, C.c_int, C.POINTER(MutinfoSpecC), C.POINTER(MutinfoResultC),
                                     C.POINTER(C.c_longlong), C.POINTER(C.c_ubyte), vp, dp],
        "mcx_debug_mutinfo_geometry": [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(MutinfoGeometry)],
        "mcx_debug_mutinfo_counts": [fp, C.c_int, C.c_int, C.c_int, C.POINTER(MutinfoSpecC), C.c_int, C.c_int, dp, C.POINTER(C.c_int),
                                     C.POINTER(C.c_int)],
        "mcx_debug_mutinfo_times": [vp, C.c_int, C.c_int, C.POINTER(MutinfoSpecC), dp],
        "mcx_get_profile": [vp, C.POINTER(Profile)],
        "mcx_copy_to_host": [vp, vp, C.c_size_t, vp],
        "mcx_copy_to_device": [vp, vp, C.c_size_t, vp],
        "mcx_plan": [C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int,
                     C.c_int, C.c_int, C.c_int, C.POINTER(PlanItem), C.c_int, C.POINTER(C.c_int)],
        "mcx_abi_version": [],
        "mcx_device_info": [C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_size_t)],
        "mcx_set_device": [C.c_int],
        "mcx_device_count": [C.POINTER(C.c_int)],
        "mcx_device_pci_bus_id": [C.c_char_p, C.c_size_t],
        "mcx_rccl_available": [],
        "mcx_user_source_available": [],
        "mcx_debug_user_source_compile": [C.c_char_p, C.c_int, C.POINTER(C.c_size_t)],
        "mcx_debug_user_source_compile_small": [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)],
        "mcx_user_kernel_compile": [C.c_char_p, C.c_char_p, C.POINTER(vp)],
        "mcx_rccl_unique_id": [vp],
        "mcx_exchange_rccl_init": [vp, vp],
        "mcx_exchange_rccl_adopt": [vp, vp],
        "mcx_exchange_rccl_destroy": [vp],
        "mcx_exchange_rccl_info": [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)],
        "mcx_debug_exchange": [vp],
        "mcx_debug_fill_slot": [vp, C.c_float],
        "mcx_debug_persist_deal": [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), u32p, C.c_int],
        "mcx_debug_step_instances": [vp, u32p, C.c_int, C.POINTER(C.c_int)],
        "mcx_debug_step_instance_list": [u32p, C.c_int, C.POINTER(C.c_int)],
        "mcx_debug_small_stretch": [C.POINTER(PlanItem), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                    C.POINTER(C.c_int)],
        "mcx_debug_copy_bandwidth": [C.c_size_t, C.c_int, C.POINTER(C.c_double)],
        "mcx_debug_live_resources": [C.POINTER(C.c_uint64)],
        "mcx_debug_numerics": [C.c_int, C.c_int, u32p, u32p],
        "mcx_debug_murray_screen": [C.c_int, C.c_int, C.c_int, fp, fp, C.c_int, C.c_int, C.POINTER(C.c_uint64)],
        "mcx_debug_murray_decode": [C.POINTER(C.c_uint64), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.POINTER(C.c_uint64)],
        "mcx_debug_normals": [C.c_uint32] * 6 + [C.c_int, fp],
        "mcx_debug_sqrt_sweep": [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), u32p],
    }
    for name, args in sig.items():
        try:
            f = getattr(L, name)
        except AttributeError:
            if os.environ.get("MCX_LIBMCX"):  # an older build of the library under tools/persist_ab.py: what it lacks is not called
                continue
            raise
        f.argtypes = args
        f.restype = C.c_int
    L.mcx_last_error.restype = C.c_char_p
    L.mcx_last_error.argtypes = []
    if os.environ.get("MCX_LIBMCX"):
        # a substituted build (tools/persist_ab.py) must at least speak this binding's ABI: the structs above are laid out for it
        import sys
        print("mcpar_amd: using MCX_LIBMCX=%s instead of the package's libmcx.so" % p, file=sys.stderr)
        got = L.mcx_abi_version()
        if got != ABI_VERSION:
            raise McxError(-1, "MCX_LIBMCX=%s is ABI %d, this binding is for ABI %d" % (p, got, ABI_VERSION))
    _lib = L
    return L


def check(code):
    if code != 0:
        raise McxError(code, load().mcx_last_error().decode("utf-8", "replace"))
