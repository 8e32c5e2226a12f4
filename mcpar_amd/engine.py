"""Host-side mirror of the reference's MCPar interface (src/mcpar.hh:32-42) over the C ABI."""
import collections
import ctypes as C

import numpy as np

from ._lib import (HOSTFN, K_NAMES, OUTFN, SINKFN, TEXTSINKFN, XCHGFN, ChainRule, ChainsGeometry, ClipSpecC, CompareGeometry, CompareSpecC, Counters, EnergyGeometry, EnergyResultC, EnergySpecC, EvidenceGeometry, EvidenceMixtureC, EvidenceResultC, EvidenceSpecC, Density2dSpecC,
                   DensitySpecC, Derive, IntervalSpecC, IntervalsGeometry, LagcovGeometry, LagcovResultC, LagcovSpecC, ModesGeometry, ModesResultC, ModesSpecC, MutinfoGeometry, MutinfoResultC, MutinfoSpecC, PlanItem, Profile, Profile2dSpecC, ProfileGeometry, ProfileSpecC, ReweightGeometry, ReweightResultC, StepRule, SteptableGeometry, StoreGeometry, TextReport, TextSpec, VLFunc, WeightsC, check, load)
from ._lib import ERR_NONFINITE  # noqa: F401

VL_ROSENBROCK1, VL_ROSENBROCK2, VL_GAUSSIAN, VL_DUALGAUSS, VL_GAUSSMIX, VL_HOST = 1, 2, 3, 4, 5, 100
VL_DEVICE = 101
VL_SOURCE = 102
VL_ROSENBROCK2_FIXED = 6
OPT_SAMPLES, OPT_ACCEPT_MASK, OPT_FUSE, OPT_MAX_SEGMENT, OPT_PROFILE, OPT_STREAM, OPT_EAGER_EXCHANGE = 1, 2, 3, 4, 5, 6, 7
OPT_SAMPLE_STRIDE = 8
OPT_SPLIT_RNG = 9
OPT_PERSIST = 10
OPT_MEET_TIMEOUT_MS = 11
OPT_DEBUG_MEET = 12
OPT_CULL = 13
OPT_BLOCKS_PER_LANE = 14
OPT_ASYNC_TAIL = 15
OPT_SINK_TEXT = 16
OPT_MEET_UNDER_GATHER = 17
OPT_MURRAY_OVERLAP = 18
OPT_ASYNC_RUN = 19
OPT_REFERENCE_CALLS = 20
OPT_SELF_REPORT = 21
OPT_MURRAY_MAX_PASSES = 22
XCHG_BEGIN, XCHG_WAIT = 0, 1
SUMMARY_NONFINITE = 1  # mcx_col_summary.flags: the column holds an inf or NaN
# include/mcx.h mcx_col_summary
SUMMARY_DTYPE = np.dtype([("mean", np.float64), ("sd", np.float64), ("min", np.float32), ("max", np.float32),
                          ("rhat", np.float64), ("ess", np.float64), ("mcse_mean", np.float64), ("ess_lag", np.int32),
                          ("flags", np.int32)], align=True)
assert SUMMARY_DTYPE.itemsize == 56
# include/mcx.h mcx_col_rank_summary
RANK_SUMMARY_DTYPE = np.dtype([("rhat", np.float64), ("rhat_bulk", np.float64), ("rhat_folded", np.float64),
                               ("ess_bulk", np.float64), ("ess_tail", np.float64), ("ess_q05", np.float64),
                               ("ess_q95", np.float64), ("q05", np.float64), ("median", np.float64), ("q95", np.float64),
                               ("ess_bulk_lag", np.int32), ("flags", np.int32)], align=True)
assert RANK_SUMMARY_DTYPE.itemsize == 88
# include/mcx.h mcx_col_density
DENSITY_DTYPE = np.dtype([("bw", np.float64), ("from", np.float64), ("to", np.float64), ("lo", np.float64), ("up", np.float64),
                          ("mean", np.float64), ("sd", np.float64), ("nvalues", np.int64), ("nbinned", np.int64),
                          ("flags", np.int32)], align=True)
assert DENSITY_DTYPE.itemsize == 80
# include/mcx.h mcx_col_clip
CLIP_DTYPE = np.dtype([("lo", np.float64), ("hi", np.float64), ("nbelow", np.int64), ("nabove", np.int64), ("flags", np.int32)],
                      align=True)
assert CLIP_DTYPE.itemsize == 40
# include/mcx.h mcx_pair_density
PAIR_DENSITY_DTYPE = np.dtype([("a", np.int32), ("b", np.int32), ("nbinned", np.int64), ("flags", np.int32)], align=True)
assert PAIR_DENSITY_DTYPE.itemsize == 24
# include/mcx.h mcx_chain_col, mcx_chain_row
CHAIN_COL_DTYPE = np.dtype([("mean", np.float64), ("sd", np.float64), ("rho1", np.float64)], align=True)
CHAIN_ROW_DTYPE = np.dtype([("moves", np.int64), ("longest_stay", np.int64), ("ll_max", np.float32), ("ll_max_step", np.int32),
                            ("flags", np.int32)], align=True)
assert CHAIN_COL_DTYPE.itemsize == 24 and CHAIN_ROW_DTYPE.itemsize == 32
CHAIN_NONFINITE, CHAIN_STUCK, CHAIN_OUTLIER = 1, 2, 4  # mcx_chains_keep's reasons
STEP_COL_DTYPE = np.dtype([("mean", np.float64), ("sd", np.float64), ("min", np.float32), ("max", np.float32), ("flags", np.int32),
                           ("reserved", np.int32)], align=True)
STEP_ROW_DTYPE = np.dtype([("moved", np.int32), ("ll_max", np.float32), ("ll_max_chain", np.int32), ("flags", np.int32)], align=True)
STEP_SETTLE_DTYPE = np.dtype([("m_ref", np.float64), ("s_ref", np.float64), ("max_dev_mean", np.float64), ("max_dev_sd", np.float64),
                              ("last_out", np.int32), ("reserved", np.int32)], align=True)
assert STEP_COL_DTYPE.itemsize == 32 and STEP_ROW_DTYPE.itemsize == 16 and STEP_SETTLE_DTYPE.itemsize == 40
# include/mcx.h mcx_col_compare
COMPARE_DTYPE = np.dtype([("ks_plus_num", np.int64), ("ks_minus_num", np.int64), ("ks_plus_x", np.float64), ("ks_minus_x", np.float64),
                          ("ks", np.float64), ("w1", np.float64), ("mean_a", np.float64), ("sd_a", np.float64), ("ess_a", np.float64),
                          ("mean_b", np.float64), ("sd_b", np.float64), ("ess_b", np.float64), ("z_mean", np.float64),
                          ("ks_neff", np.float64), ("ks_p", np.float64), ("na", np.int64), ("nb", np.int64), ("flags", np.int32),
                          ("reserved", np.int32)], align=True)
assert COMPARE_DTYPE.itemsize == 144
COMPARE_IID = 1                                   # mcx_compare_spec.flags
COMPARE_NONFINITE_A, COMPARE_NONFINITE_B = 1, 2   # mcx_col_compare.flags
ENERGY_COL_DTYPE = np.dtype([("scale", np.float64), ("flags", np.int32)], align=True)  # include/mcx.h mcx_energy_col
assert ENERGY_COL_DTYPE.itemsize == 16
ENERGY_WITH_LL, ENERGY_RAW = 1, 2                                        # mcx_energy_spec.flags
ENERGY_COL_NONFINITE, ENERGY_COL_CONSTANT, ENERGY_COL_UNUSED = 1, 2, 4   # mcx_energy_col.flags
ENERGY_MAX_SIDE, ENERGY_MAX_PERM = 16384, 4095
MUTINFO_COL_DTYPE = np.dtype([("scale", np.float64), ("flags", np.int32)], align=True)  # include/mcx.h mcx_mutinfo_col
MUTINFO_PAIR_DTYPE = np.dtype([("a", np.int32), ("b", np.int32), ("mi", np.float64), ("r_info", np.float64), ("pearson", np.float64),
                               ("perm_mean", np.float64), ("perm_sd", np.float64), ("p_value", np.float64), ("nge", np.int64),
                               ("nzero", np.int64), ("flags", np.int32)], align=True)  # include/mcx.h mcx_mutinfo_pair
assert MUTINFO_COL_DTYPE.itemsize == 16 and MUTINFO_PAIR_DTYPE.itemsize == 80
MUTINFO_WITH_LL, MUTINFO_RAW = 1, 2                                          # mcx_mutinfo_spec.flags
MUTINFO_COL_NONFINITE, MUTINFO_COL_CONSTANT, MUTINFO_COL_UNUSED = 1, 2, 4    # mcx_mutinfo_col.flags
MUTINFO_PAIR_UNUSED, MUTINFO_PAIR_FEW, MUTINFO_PAIR_TIES = 1, 2, 4           # mcx_mutinfo_pair.flags
MUTINFO_MAX_ROWS, MUTINFO_MAX_PERM, MUTINFO_MAX_K = 16384, 999, 8
MUTINFO_MAX_PAIRS = 1024
# include/mcx.h mcx_col_reweight
REWEIGHT_DTYPE = np.dtype([("mean", np.float64), ("sd", np.float64), ("mcse_mean", np.float64), ("min", np.float32), ("max", np.float32),
                           ("flags", np.int32), ("reserved", np.int32)], align=True)
assert REWEIGHT_DTYPE.itemsize == 40
WEIGHT_HOST, WEIGHT_STORE, WEIGHT_LL = 1, 2, 3   # mcx_weights.kind
REWEIGHT_NO_TAIL, REWEIGHT_KHAT_HIGH = 1, 2      # mcx_reweight_result.flags
REWEIGHT_NONFINITE = 1                           # mcx_col_reweight.flags
REWEIGHT_MAX_PROBS = 64
STEP_MAX_PROBS = 8  # include/mcx.h MCX_STEP_MAX_PROBS
# include/mcx.h mcx_col_intervals, mcx_col_hdi, mcx_col_quantile_se
INTERVALS_DTYPE = np.dtype([("mean", np.float64), ("sd", np.float64), ("ess_sd", np.float64), ("mcse_sd", np.float64),
                            ("ess_sd_lag", np.int32), ("flags", np.int32)], align=True)
HDI_DTYPE = np.dtype([("width", np.float64), ("index", np.int64), ("span", np.int64), ("lo", np.float32), ("hi", np.float32)], align=True)
QUANTILE_SE_DTYPE = np.dtype([("q", np.float64), ("ess_q", np.float64), ("u_lo", np.float64), ("u_hi", np.float64), ("mcse_q", np.float64),
                              ("k_lo", np.int64), ("k_hi", np.int64), ("s_lo", np.float32), ("s_hi", np.float32),
                              ("ess_q_lag", np.int32), ("reserved", np.int32)], align=True)
assert INTERVALS_DTYPE.itemsize == 40 and HDI_DTYPE.itemsize == 32 and QUANTILE_SE_DTYPE.itemsize == 72
INTERVAL_MAX_MASSES, INTERVAL_MAX_PROBS, INTERVAL_TIMES = 8, 8, 12
# include/mcx.h mcx_col_lagcov, its flags beside SUMMARY_NONFINITE, and mcx_lagcov_result.flags
LAGCOV_DTYPE = np.dtype([("mean", np.float64), ("ess", np.float64), ("mcse", np.float64), ("flags", np.int32), ("reserved", np.int32)], align=True)
assert LAGCOV_DTYPE.itemsize == 32
LAGCOV_CONSTANT = 2
MESS_NOT_PD, MESS_TRUNCATED, MESS_LAMBDA_SINGULAR = 1, 2, 4
LAGCOV_TIMES = 5
DENSITY_GRID = 512  # grid points per column; a column's slots are [DENSITY_GRID + 1, 2] uint64 (cnt, frac)
RANK_Z, RANK_Z_FOLDED, RANK_I05, RANK_I95 = 0, 1, 2, 3  # mcx_debug_rows_rank_transform's `what`
DERIVE_LINEAR, DERIVE_SOURCE = 1, 2  # include/mcx.h mcx_derive.kind
EVIDENCE_MAX_K, EVIDENCE_TIMES = 8, 8                   # include/mcx.h MCX_EVIDENCE_MAX_K, MCX_EVIDENCE_TIMES
EVIDENCE_NOT_CONVERGED, EVIDENCE_NO_ESS = 1, 2          # mcx_evidence_result.flags
EVIDENCE_STREAM = 8                                     # the Philox stream of the proposal's draws
# include/mcx.h mcx_col_profile, mcx_profile_interval_t, mcx_pair_profile
COL_PROFILE_DTYPE = np.dtype([("from", np.float64), ("to", np.float64), ("lhat", np.float64), ("xhat", np.float64), ("row_hat", np.int64),
                              ("nvalues", np.int64), ("nbinned", np.int64), ("ndropped", np.int64), ("nempty", np.int32),
                              ("flags", np.int32)], align=True)
PROFILE_INTERVAL_DTYPE = np.dtype([("p", np.float64), ("drop", np.float64), ("lo", np.float64), ("hi", np.float64), ("lo_hull", np.float64),
                                   ("hi_hull", np.float64), ("nseg", np.int32), ("flags", np.int32)], align=True)
PAIR_PROFILE_DTYPE = np.dtype([("a", np.int32), ("b", np.int32), ("nbinned", np.int64), ("nempty", np.int32), ("flags", np.int32)], align=True)
assert COL_PROFILE_DTYPE.itemsize == 72 and PROFILE_INTERVAL_DTYPE.itemsize == 56 and PAIR_PROFILE_DTYPE.itemsize == 24
PROFILE_MAX_LEVELS = 8  # include/mcx.h MCX_PROFILE_MAX_LEVELS
# flags beside SUMMARY_NONFINITE: of a column or pair, then of an interval
PROFILE_LL_NONFINITE, PROFILE_OPEN_LO, PROFILE_OPEN_HI, PROFILE_NO_BIN, PROFILE_HULL_OPEN_LO, PROFILE_HULL_OPEN_HI = 2, 4, 8, 16, 32, 64


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def format_rows(rows):
    """rows [nrows, ncol] float32 -> the bytes MCout::output prints for them (src/mcout.cc:41-45), formatted on the GPU"""
    rows = np.ascontiguousarray(rows, np.float32)
    nrows, ncol = rows.shape
    nb = C.c_size_t(0)
    check(load().mcx_format_rows(_fp(rows), nrows, ncol, None, 0, C.byref(nb)))
    buf = C.create_string_buffer(max(nb.value, 1))
    check(load().mcx_format_rows(_fp(rows), nrows, ncol, buf, nb.value, C.byref(nb)))
    return buf.raw[:nb.value]


def user_source_available():
    return bool(load().mcx_user_source_available())


def compile_user_kernel(source, symbol):
    """HIP source of a whole kernel with the MCX_VL_DEVICE contract -> its hipFunction_t (int), through hiprtc"""
    fn = C.c_void_p()
    check(load().mcx_user_kernel_compile(source.encode(), symbol.encode(), C.byref(fn)))
    return fn.value


def make_vlfunc(kind, d, params=None, ncomp=0, host_fn=None, device_fn=None, source=None):
    """Build an mcx_vlfunc.  host_fn(x[npset, d]) -> y[npset] wraps a user VLFunc (src/vlfunc.hh:9-12);
    device_fn is a hipFunction_t (int) of a user kernel f(int npset, const float *x, float *y);
    source (VL_SOURCE) is HIP text of the user's device functions, params their `par`.
    Returns (struct, keepalive)."""
    p = None if params is None else np.ascontiguousarray(params, dtype=np.float32)
    if source is not None:
        txt = C.create_string_buffer(source.encode() if isinstance(source, str) else bytes(source))
        v = VLFunc(kind, d, 0 if p is None else p.size, _fp(p) if p is not None else None, HOSTFN(), C.cast(txt, C.c_void_p))
        return v, (p, txt)
    cb = HOSTFN()
    if host_fn is not None:
        def tramp(ctx, npset, x, y):
            xa = np.ctypeslib.as_array(x, shape=(npset, d))
            ya = np.ctypeslib.as_array(y, shape=(npset,))
            ya[:] = np.asarray(host_fn(xa), dtype=np.float32)
            return 0
        cb = HOSTFN(tramp)
    v = VLFunc(kind, d, ncomp, _fp(p) if p is not None else None, cb,
               C.c_void_p(device_fn) if device_fn is not None else None)
    return v, (p, cb)


def vlfunc_eval(kind, d, x, params=None, ncomp=0):
    """VLFunc::operator()(npset, x, y) on the GPU"""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, d)
    y = np.empty(x.shape[0], dtype=np.float32)
    v, keep = make_vlfunc(kind, d, params, ncomp)
    check(load().mcx_vlfunc_eval(C.byref(v), x.shape[0], _fp(x), _fp(y)))
    return y


PLAN_NAMES = {1: "burn_segment", 2: "tuner", 3: "init_moments", 4: "output", 5: "publish", 6: "gather_begin",
              7: "gather_wait", 8: "remote_step", 9: "main_segment", 10: "sink"}


def plan(nsamp, nburn, sync=10, pl=0.9, seed=8675309, tbase=0, nshards=1, eager=0, fused=1, max_segment=256,
         has_output_hook=0, sink_block=0):
    """the launch schedule mcx_run executes for these settings (host logic only, needs no GPU)"""
    n = C.c_int(0)
    check(load().mcx_plan(nsamp, nburn, sync, pl, seed, tbase, nshards, eager, fused, max_segment, has_output_hook,
                          sink_block, None, 0, C.byref(n)))
    items = (PlanItem * max(1, n.value))()
    check(load().mcx_plan(nsamp, nburn, sync, pl, seed, tbase, nshards, eager, fused, max_segment, has_output_hook,
                          sink_block, items, n.value, C.byref(n)))
    return [(PLAN_NAMES[it.kind], it.first, it.nsteps, it.aux) for it in items[:n.value]]


def small_stretch(items, index, nsamp, gather_in_flight=False):
    """what one launch of the one-launch small-n kernel takes of the plan `items` (as plan() returns it) when mcx_run stands
    at items[index]: (end, burn steps, main steps, init_moments, first main step, snap_after); zero steps and end = index
    where nothing can be merged (host logic only, needs no GPU)"""
    kinds = {v: k for k, v in PLAN_NAMES.items()}
    arr = (PlanItem * max(1, len(items)))(*[PlanItem(kinds[k], f, n, a) for k, f, n, a in items])
    end, out = C.c_int(0), (C.c_int * 5)()
    check(load().mcx_debug_small_stretch(arr, len(items), index, nsamp, int(bool(gather_in_flight)), C.byref(end), out))
    return (end.value,) + tuple(out)


# ---- the step-kernel template instances (include/mcx.h: mcx_debug_step_instances) ----
STEP_FAMILIES = {1: "fast", 2: "fastb", 3: "fast_full", 4: "fastb_full", 5: "pregen", 6: "gen_normals", 7: "generic",
                 8: "persist", 9: "user"}
LIK_NAMES = {0: "", 1: "LIK_ROSEN1", 2: "LIK_ROSEN2", 3: "LIK_GAUSS", 5: "LIK_MIX", 6: "LIK_ROSEN2F", 7: "LIK_USER"}
EMIT_NAMES = {0: "", 1: "EMIT_NONE", 2: "EMIT_EVERY", 3: "EMIT_THIN"}
StepInstance = collections.namedtuple("StepInstance", "family lanes bpl lik main emit rec")


def step_instance_decode(word):
    """the id of one compiled step-kernel instance -> StepInstance(family, lanes, bpl, lik, main, emit, rec), names for
    family, lik and emit"""
    w = int(word)
    return StepInstance(STEP_FAMILIES[w & 15], (w >> 4) & 127, (w >> 11) & 7, LIK_NAMES[(w >> 14) & 15], bool((w >> 18) & 1),
                        EMIT_NAMES[(w >> 19) & 3], bool((w >> 21) & 1))


def step_instance_encode(rec):
    inv = lambda m, v: next(k for k, name in m.items() if name == v)  # noqa: E731
    return (inv(STEP_FAMILIES, rec.family) | rec.lanes << 4 | rec.bpl << 11 | inv(LIK_NAMES, rec.lik) << 14 | int(rec.main) << 18 |
            inv(EMIT_NAMES, rec.emit) << 19 | int(rec.rec) << 21)


def step_instance_name(r):
    """the record as the C++ instance the launcher names, e.g. k_fused_fastb<2,4,true,LIK_MIX>"""
    b = lambda v: "true" if v else "false"  # noqa: E731
    f = r.family
    if f == "fast":
        return "k_fused_fast<%d,%s,%s,false,false,%s>" % (r.lanes, b(r.main), r.lik, r.emit)
    if f == "fastb":
        return "k_fused_fastb<%d,%d,%s,%s>" % (r.lanes, r.bpl, b(r.main), r.lik)
    if f == "fast_full":
        return "k_fused_fast<%d,%s,%s,false,true>" % (r.lanes, b(r.main), r.lik)
    if f == "fastb_full":
        return "k_fused_fastb<%d,%d,%s,%s,true>" % (r.lanes, r.bpl, b(r.main), r.lik)
    if f == "pregen":
        return "k_fused_fast<%d,%s,%s,true>" % (r.lanes, b(r.main), r.lik)
    if f == "gen_normals":
        return "k_gen_normals<%d>" % r.lanes
    if f == "generic":
        return "k_fused_steps<%d,%s,%s>" % (r.lanes, r.lik, b(r.main))
    if f == "persist":
        return "k_run_small<%d,%d,%s,%s>" % (r.lanes, r.bpl, r.lik, b(r.rec))
    return "user<lanes=%d,bpl=%d,main=%s,rec=%s>" % (r.lanes, r.bpl, b(r.main), b(r.rec))


def _step_ids(call):
    n = C.c_int(0)
    check(call(None, 0, C.byref(n)))
    ids = np.zeros(max(n.value, 1), np.uint32)
    check(call(ids.ctypes.data_as(C.POINTER(C.c_uint32)), n.value, C.byref(n)))
    return [step_instance_decode(w) for w in ids[:n.value]]


def step_instance_list():
    """every step-kernel instance the launchers can launch (mcx_debug_step_instance_list; host logic only, needs no GPU)"""
    return _step_ids(load().mcx_debug_step_instance_list)


def _probs(probs):
    p = np.ascontiguousarray(np.asarray(probs, np.float64).reshape(-1))
    return p, p.ctypes.data_as(C.POINTER(C.c_double))


def _summary_dict(cols, q):
    out = {name: cols[name].copy() for name in SUMMARY_DTYPE.names}
    out["quantiles"] = q
    return out


def rows_summary(rows, nsteps, nc, probs=(0.01, 0.5, 0.99)):
    """mcx_rows_summary: Engine.summary's dict for rows [nsteps * nc, np + 1] on the host (MCout layout)"""
    rows = np.ascontiguousarray(rows, np.float32)
    ncol = rows.shape[1]
    p, pp = _probs(probs)
    cols = np.zeros(ncol, SUMMARY_DTYPE)
    q = np.zeros((ncol, len(p)), np.float64)
    check(load().mcx_rows_summary(_fp(rows), nsteps, nc, ncol - 1, pp, len(p), cols.ctypes.data_as(C.c_void_p),
                                  q.ctypes.data_as(C.POINTER(C.c_double))))
    return _summary_dict(cols, q)


def _rank_summary_dict(cols):
    return {name: cols[name].copy() for name in RANK_SUMMARY_DTYPE.names}


def rows_rank_summary(rows, nsteps, nc):
    """mcx_rows_rank_summary: Engine.rank_summary's dict for rows [nsteps * nc, np + 1] on the host (MCout layout)"""
    rows = np.ascontiguousarray(rows, np.float32)
    ncol = rows.shape[1]
    cols = np.zeros(ncol, RANK_SUMMARY_DTYPE)
    check(load().mcx_rows_rank_summary(_fp(rows), nsteps, nc, ncol - 1, cols.ctypes.data_as(C.c_void_p)))
    return _rank_summary_dict(cols)


def debug_rows_rank_transform(rows, nsteps, nc, what, want_ranks=False):
    """mcx_debug_rows_rank_transform: one transformed store of rows_rank_summary as rows [nsteps * nc, np + 1] (what =
    RANK_Z, RANK_Z_FOLDED, RANK_I05 or RANK_I95); with want_ranks (RANK_Z / RANK_Z_FOLDED) also the average ranks as
    float64 in the same layout: (out_rows, ranks)"""
    rows = np.ascontiguousarray(rows, np.float32)
    out = np.zeros_like(rows)
    ranks = np.zeros(rows.shape, np.float64) if want_ranks else None
    check(load().mcx_debug_rows_rank_transform(_fp(rows), nsteps, nc, rows.shape[1] - 1, what,
                                               None if ranks is None else ranks.ctypes.data_as(C.POINTER(C.c_double)),
                                               _fp(out)))
    return (out, ranks) if want_ranks else out


def debug_normal_quantile(p):
    """mcx_debug_normal_quantile (host only): PPND16 of every p, float64"""
    p = np.ascontiguousarray(np.asarray(p, np.float64).reshape(-1))
    z = np.zeros_like(p)
    check(load().mcx_debug_normal_quantile(p.ctypes.data_as(C.POINTER(C.c_double)), p.size,
                                           z.ctypes.data_as(C.POINTER(C.c_double))))
    return z


def debug_rows_acov(rows, nsteps, nc, nlags):
    """mcx_debug_rows_acov: (acov [np + 1, nlags], sumsq [np + 1]), the device's raw autocovariance sums over the
    half-chains of rows [nsteps * nc, np + 1] and its centred sums of squares"""
    rows = np.ascontiguousarray(rows, np.float32)
    ncol = rows.shape[1]
    acov = np.zeros((ncol, nlags), np.float64)
    sumsq = np.zeros(ncol, np.float64)
    check(load().mcx_debug_rows_acov(_fp(rows), nsteps, nc, ncol - 1, nlags, acov.ctypes.data_as(C.POINTER(C.c_double)),
                                     sumsq.ctypes.data_as(C.POINTER(C.c_double))))
    return acov, sumsq


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _covariance_dict(mean, cov, flags):
    """mean, cov, flags and corr = cov_ij / sqrt(cov_ii cov_jj): NaN where a variance is 0 or NaN, else exactly 1 on the diagonal"""
    v = np.diag(cov).copy()
    v[~(v > 0)] = np.nan
    s = np.sqrt(v)
    with np.errstate(invalid="ignore"):
        corr = cov / np.outer(s, s)
    k = np.flatnonzero(~np.isnan(v))
    corr[k, k] = 1.0
    return dict(mean=mean, cov=cov, corr=corr, flags=flags)


def rows_covariance(rows, nsteps, nc):
    """mcx_rows_covariance: Engine.covariance's dict for rows [nsteps * nc, np + 1] on the host (MCout layout)"""
    rows = np.ascontiguousarray(rows, np.float32)
    ncol = rows.shape[1]
    mean, cov, flags = np.zeros(ncol), np.zeros((ncol, ncol)), np.zeros(ncol, np.int32)
    check(load().mcx_rows_covariance(_fp(rows), nsteps, nc, ncol - 1, _dp(mean), _dp(cov),
                                     flags.ctypes.data_as(C.POINTER(C.c_int))))
    return _covariance_dict(mean, cov, flags)


# ---- densities (include/mcx.h) ----
class DensitySpec:
    """an mcx_density_spec and the arrays it points to: n output points, adjust times the nrd0 bandwidth, clip = (qlo, qhi)
    quantiles as the range ((0, 1): min to max), bw / from_ / to = None or [ncol] with NaN for a column's default"""

    def __init__(self, n=512, adjust=1.0, clip=(0, 1), bw=None, from_=None, to=None):
        arr = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1))  # noqa: E731
        ptr = lambda a: None if a is None else _dp(a)  # noqa: E731
        self.n, self.bw, self.from_, self.to = int(n), arr(bw), arr(from_), arr(to)
        self.c = DensitySpecC(self.n, float(adjust), float(clip[0]), float(clip[1]), ptr(self.bw), ptr(self.from_), ptr(self.to))

    def fits(self, ncol):
        for a in (self.bw, self.from_, self.to):
            if a is not None and a.size != ncol:
                raise ValueError("bw, from_ and to take one entry per column (%d), NaN for a column's default" % ncol)
        return self


def _density_out(ncol, n):
    n = min(max(int(n), 1), DENSITY_GRID)  # (a refused n still gets buffers)
    return np.zeros(ncol, DENSITY_DTYPE), np.zeros((ncol, n)), np.zeros((ncol, n))


def _density_dict(cols, x, y):
    out = {name: cols[name].copy() for name in DENSITY_DTYPE.names}
    out["x"], out["y"] = x, y
    return out


def rows_density(rows, nsteps, nc, n=512, adjust=1.0, clip=(0, 1), bw=None, from_=None, to=None):
    """mcx_rows_density: Engine.density's dict for rows [nsteps * nc, np + 1] on the host (MCout layout)"""
    rows = np.ascontiguousarray(rows, np.float32)
    ncol = rows.shape[1]
    spec = DensitySpec(n, adjust, clip, bw, from_, to).fits(ncol)
    cols, x, y = _density_out(ncol, n)
    check(load().mcx_rows_density(_fp(rows), nsteps, nc, ncol - 1, C.byref(spec.c), cols.ctypes.data_as(C.c_void_p), _dp(x), _dp(y)))
    return _density_dict(cols, x, y)


def debug_density_grid(N, mean, sd, min_, max_, q25, q75, qclip=(np.nan, np.nan), is_last_col=False, col=0, spec=None):
    """mcx_debug_density_grid (host only): the record (DENSITY_DTYPE) of one column from its statistics"""
    spec = spec or DensitySpec()
    out = np.zeros(1, DENSITY_DTYPE)
    check(load().mcx_debug_density_grid(int(N), mean, sd, min_, max_, q25, q75, qclip[0], qclip[1], int(bool(is_last_col)), col,
                                        C.byref(spec.c), out.ctypes.data_as(C.c_void_p)))
    return out[0]


def debug_density_finish(col, slots, n=512):
    """mcx_debug_density_finish (host only): (x [n], y [n]) of one column from its record and slots [513, 2] uint64"""
    rec = np.zeros(1, DENSITY_DTYPE)
    rec[0] = col
    sl = np.ascontiguousarray(slots, np.uint64)
    if sl.shape != (DENSITY_GRID + 1, 2):
        raise ValueError("slots must be [513, 2]")
    x, y = np.zeros(max(n, 1)), np.zeros(max(n, 1))
    check(load().mcx_debug_density_finish(rec.ctypes.data_as(C.c_void_p), sl.ctypes.data_as(C.POINTER(C.c_ulonglong)), n, _dp(x), _dp(y)))
    return x, y


def debug_rows_density_bins(rows, nsteps, nc, lo, up):
    """mcx_debug_rows_density_bins: the binning sweep alone over rows [nsteps * nc, np + 1] on the grids lo [np + 1] < up
    [np + 1] -- slots [np + 1, 513, 2] uint64 (cnt, frac)"""
    rows = np.ascontiguousarray(rows, np.float32)
    ncol = rows.shape[1]
    lo = np.ascontiguousarray(np.asarray(lo, np.float64).reshape(-1))
    up = np.ascontiguousarray(np.asarray(up, np.float64).reshape(-1))
    if lo.size != ncol or up.size != ncol:
        raise ValueError("lo and up take one entry per column")
    slots = np.zeros((ncol, DENSITY_GRID + 1, 2), np.uint64)
    check(load().mcx_debug_rows_density_bins(_fp(rows), nsteps, nc, ncol - 1, _dp(lo), _dp(up),
                                             slots.ctypes.data_as(C.POINTER(C.c_ulonglong))))
    return slots


# ---- pair densities (include/mcx.h) ----
DENSITY2D_F = 4096  # the fixed-point unit of a value's fraction between two nodes


class Density2dSpec:
    """an mcx_density2d_spec and the arrays it points to: g nodes per axis, pairs = None (every a < b) or [npairs, 2]
    columns, the other fields as DensitySpec's"""

    def __init__(self, g=64, pairs=None, adjust=1.0, clip=(0, 1), bw=None, from_=None, to=None):
        arr = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1))  # noqa: E731
        ptr = lambda a: None if a is None else _dp(a)  # noqa: E731
        self.g, self.bw, self.from_, self.to = int(g), arr(bw), arr(from_), arr(to)
        self.pairs = None if pairs is None else np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        self.c = Density2dSpecC(self.g, float(adjust), float(clip[0]), float(clip[1]), ptr(self.bw), ptr(self.from_), ptr(self.to),
                                0 if self.pairs is None else self.pairs.shape[0],
                                None if self.pairs is None else self.pairs.ctypes.data_as(C.POINTER(C.c_int)))

    def fits(self, ncol):
        for a in (self.bw, self.from_, self.to):
            if a is not None and a.size != ncol:
                raise ValueError("bw, from_ and to take one entry per column (%d), NaN for a column's default" % ncol)
        return self

    def npairs(self, ncol):
        return ncol * (ncol - 1) // 2 if self.pairs is None else self.pairs.shape[0]


def _density2d_call(fn, spec, ncol):
    """fn(spec, cols, axes, pairs_out, z) -> the dict of a pair density call"""
    g = min(max(spec.g, 1), 64)  # (a refused g or list of pairs still gets buffers)
    npairs = min(max(spec.npairs(ncol), 1), 1024)
    cols, axes = np.zeros(ncol, DENSITY_DTYPE), np.zeros((ncol, g))
    po, z = np.zeros(npairs, PAIR_DENSITY_DTYPE), np.zeros((npairs, g, g))
    check(fn(C.byref(spec.c), cols.ctypes.data_as(C.c_void_p), _dp(axes), po.ctypes.data_as(C.c_void_p), _dp(z)))
    out = {name: cols[name].copy() for name in DENSITY_DTYPE.names if name not in ("nbinned", "flags")}
    out["col_flags"] = cols["flags"].copy()
    out["axes"], out["z"] = axes, z
    out["pairs"] = np.stack([po["a"], po["b"]], axis=1)
    out["nbinned"], out["flags"] = po["nbinned"].copy(), po["flags"].copy()
    return out


def rows_density2d(rows, nsteps, nc, g=64, pairs=None, adjust=1.0, clip=(0, 1), bw=None, from_=None, to=None):
    """mcx_rows_density2d: Engine.density2d's dict for rows [nsteps * nc, np + 1] on the host (MCout layout)"""
    rows = np.ascontiguousarray(rows, np.float32)
    ncol = rows.shape[1]
    spec = Density2dSpec(g, pairs, adjust, clip, bw, from_, to).fits(ncol)
    return _density2d_call(lambda *a: load().mcx_rows_density2d(_fp(rows), nsteps, nc, ncol - 1, *a), spec, ncol)


def debug_density2d_grid(N, mean, sd, min_, max_, q25, q75, qclip=(np.nan, np.nan), is_last_col=False, col=0, spec=None):
    """mcx_debug_density2d_grid (host only): the record (DENSITY_DTYPE) of one column from its statistics"""
    spec = spec or Density2dSpec()
    out = np.zeros(1, DENSITY_DTYPE)
    check(load().mcx_debug_density2d_grid(int(N), mean, sd, min_, max_, q25, q75, qclip[0], qclip[1], int(bool(is_last_col)), col,
                                          C.byref(spec.c), out.ctypes.data_as(C.c_void_p)))
    return out[0]


def debug_density2d_finish(col_a, col_b, slots, g, b_first=False):
    """mcx_debug_density2d_finish (host only): z [g, g] of one pair from its two records and slots [(g + 1)^2, 4] uint64 =
    (cnt, Sa, Sb, Sab); b_first: the order of the sums of a pair a > b"""
    rec = np.zeros(2, DENSITY_DTYPE)
    rec[0], rec[1] = col_a, col_b
    sl = np.ascontiguousarray(slots, np.uint64).reshape(-1, 4)
    if not 1 <= g <= 64 or sl.shape[0] != (g + 1) ** 2:
        raise ValueError("slots must be [(g + 1)^2, 4]")
    z = np.zeros((g, g))
    check(load().mcx_debug_density2d_finish(rec[0:1].ctypes.data_as(C.c_void_p), rec[1:2].ctypes.data_as(C.c_void_p), g,
                                            sl.ctypes.data_as(C.POINTER(C.c_ulonglong)), int(bool(b_first)), _dp(z)))
    return z


def debug_rows_density2d_bins(rows, nsteps, nc, lo, up, g, pairs=None):
    """mcx_debug_rows_density2d_bins: the code, pair and reduce sweeps alone over rows [nsteps * nc, np + 1] on the grids lo
    [np + 1] < up [np + 1] -- slots [npairs, (g + 1)^2, 4] uint64 = (cnt, Sa, Sb, Sab)"""
    rows = np.ascontiguousarray(rows, np.float32)
    ncol = rows.shape[1]
    lo = np.ascontiguousarray(np.asarray(lo, np.float64).reshape(-1))
    up = np.ascontiguousarray(np.asarray(up, np.float64).reshape(-1))
    if lo.size != ncol or up.size != ncol:
        raise ValueError("lo and up take one entry per column")
    spec = Density2dSpec(g, pairs)
    slots = np.zeros((min(max(spec.npairs(ncol), 1), 1024), (min(max(g, 1), 64) + 1) ** 2, 4), np.uint64)
    check(load().mcx_debug_rows_density2d_bins(_fp(rows), nsteps, nc, ncol - 1, _dp(lo), _dp(up), g, spec.c.npairs, spec.c.pairs,
                                               slots.ctypes.data_as(C.POINTER(C.c_ulonglong))))
    return slots


# ---- derived columns and bootstrap draws (include/mcx.h) ----
class DeriveSpec:
    """an mcx_derive and the arrays it points to"""

    def __init__(self, kind, nout, par=None, source=None):
        self.par = None if par is None else np.ascontiguousarray(par, np.float32).reshape(-1)
        self.text = None if source is None else (source.encode() if isinstance(source, str) else bytes(source))
        self.c = Derive(kind, nout, 0 if self.par is None else self.par.size, None if self.par is None else _fp(self.par),
                        self.text)


def derive_linear(A, b):
    """MCX_DERIVE_LINEAR: out = b + A x, A [nout, np], b [nout]; acc = b[j], then acc = acc + A[j][k] * x[k] for k in
    order, every product and sum rounded to float32"""
    A = np.ascontiguousarray(A, np.float32)
    b = np.ascontiguousarray(b, np.float32).reshape(-1)
    if A.ndim != 2 or A.shape[0] != b.size:
        raise ValueError("A must be [nout, np] and b [nout]")
    return DeriveSpec(DERIVE_LINEAR, A.shape[0], np.concatenate([A.reshape(-1), b]))


def derive_source(text, nout, par=None):
    """MCX_DERIVE_SOURCE: HIP text that defines mcx_user_derive(x, d, ly, par, out, nout) (mcpar_amd/examples/derive_*.hip)"""
    return DeriveSpec(DERIVE_SOURCE, nout, par, text)


class DerivedStore:
    """an mcx_store: nout derived columns, then log L, of every row of a step range.  It owns its device memory."""

    def __init__(self, handle):
        self.h = handle

    def close(self):
        if self.h:
            load().mcx_store_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def shape(self):
        """(nsteps, nc, ncol), ncol = nout + 1"""
        t, nc, ncol = C.c_int(0), C.c_int(0), C.c_int(0)
        check(load().mcx_store_shape(self.h, C.byref(t), C.byref(nc), C.byref(ncol)))
        return t.value, nc.value, ncol.value

    def rows(self, first_step=0, nsteps=None):
        """MCout rows [nsteps * nc, ncol] of steps [first_step, first_step + nsteps) -- nsteps None: to the end"""
        t, nc, ncol = self.shape
        if nsteps is None:
            nsteps = t - first_step
        out = np.empty((max(nsteps, 0) * nc, ncol), np.float32)
        check(load().mcx_store_copy(self.h, first_step, nsteps, _fp(out)))
        return out

    def summary(self, probs=(0.01, 0.5, 0.99)):
        """Engine.summary's dict for the derived columns, then log L"""
        ncol = self.shape[2]
        p, pp = _probs(probs)
        cols = np.zeros(ncol, SUMMARY_DTYPE)
        q = np.zeros((ncol, len(p)), np.float64)
        check(load().mcx_store_summary(self.h, pp, len(p), cols.ctypes.data_as(C.c_void_p), _dp(q)))
        return _summary_dict(cols, q)

    def rank_summary(self):
        """Engine.rank_summary's dict"""
        cols = np.zeros(self.shape[2], RANK_SUMMARY_DTYPE)
        check(load().mcx_store_rank_summary(self.h, cols.ctypes.data_as(C.c_void_p)))
        return _rank_summary_dict(cols)

    def covariance(self):
        """Engine.covariance's dict"""
        ncol = self.shape[2]
        mean, cov, flags = np.zeros(ncol), np.zeros((ncol, ncol)), np.zeros(ncol, np.int32)
        check(load().mcx_store_covariance(self.h, _dp(mean), _dp(cov), flags.ctypes.data_as(C.POINTER(C.c_int))))
        return _covariance_dict(mean, cov, flags)

    def density(self, n=512, adjust=1.0, clip=(0, 1), bw=None, from_=None, to=None):
        """Engine.density's dict for the derived columns, then log L"""
        ncol = self.shape[2]
        spec = DensitySpec(n, adjust, clip, bw, from_, to).fits(ncol)
        cols, x, y = _density_out(ncol, n)
        check(load().mcx_store_density(self.h, C.byref(spec.c), cols.ctypes.data_as(C.c_void_p), _dp(x), _dp(y)))
        return _density_dict(cols, x, y)

    def density2d(self, g=64, pairs=None, adjust=1.0, clip=(0, 1), bw=None, from_=None, to=None):
        """Engine.density2d's dict for the derived columns, then log L"""
        ncol = self.shape[2]
        spec = Density2dSpec(g, pairs, adjust, clip, bw, from_, to).fits(ncol)
        return _density2d_call(lambda *a: load().mcx_store_density2d(self.h, *a), spec, ncol)

    def density_times(self, n=512, adjust=1.0, clip=(0, 1)):
        """mcx_debug_store_density_times: Engine.density_times' four stage times for this store"""
        spec = DensitySpec(n, adjust, clip)
        ms = np.zeros(4)
        check(load().mcx_debug_store_density_times(self.h, C.byref(spec.c), _dp(ms)))
        return ms

    def draw(self, ndraw, seed):
        """ndraw rows with replacement: (rows [ndraw, ncol], index [ndraw] int64), the index Engine.draw gives for the
        same seed and number of rows"""
        rows, index = np.empty((max(ndraw, 0), self.shape[2]), np.float32), np.empty(max(ndraw, 0), np.int64)
        check(load().mcx_store_draw(self.h, seed, ndraw, _fp(rows), index.ctypes.data_as(C.POINTER(C.c_int64))))
        return rows, index

    def clip(self, qlo=0.01, qhi=0.99, ll_hi=0.0, lo=None, hi=None, count_only=False):
        """Engine.clip's RowSet for the rows of this store (the derived columns, then log L)"""
        t, nc, ncol = self.shape
        spec = ClipSpec(qlo, qhi, ll_hi, lo, hi).fits(ncol)
        return _clip_call(lambda *a: load().mcx_store_clip(self.h, *a), spec, ncol, t * nc, count_only)

    def chain_table(self):
        """Engine.chain_table's dict for the chains of this store"""
        _, nc, ncol = self.shape
        return _chain_table_call(lambda *a: load().mcx_store_chain_table(self.h, *a), nc, ncol)

    def select_chains(self, chains):
        """Engine.select_chains' DerivedStore of chains (any order, repeats allowed) of this store"""
        return _select_call(lambda *a: load().mcx_store_select_chains(self.h, *a), chains)

    def step_table(self, probs=(0.05, 0.5, 0.95)):
        """Engine.step_table's dict for the steps of this store"""
        t, _, ncol = self.shape
        return _step_table_call(lambda *a: load().mcx_store_step_table(self.h, *a), t, ncol, probs)

    def reweight(self, weights, probs=(0.05, 0.5, 0.95)):
        """mcx_store_reweight: reweight_rows' dict for the rows of this store"""
        return _reweight_call(lambda *a: load().mcx_store_reweight(self.h, *a), weights, self.shape[2], probs)

    def resample(self, weights, nsteps_out, nc_out, seed, with_index=False):
        """mcx_store_resample: resample_rows' DerivedStore of nsteps_out * nc_out weighted draws of this store's rows"""
        return _resample_call(lambda *a: load().mcx_store_resample(self.h, *a), weights, nsteps_out, nc_out, seed, with_index)

    def intervals(self, hdi=(0.9,), probs=(0.05, 0.5, 0.95)):
        """mcx_store_intervals: Engine.intervals' dict for the columns of this store"""
        return _intervals_call(lambda *a: load().mcx_store_intervals(self.h, *a), self.shape[2], hdi, probs)

    def lagcov(self, max_lag=None, nlags=0, with_ll=False):
        """mcx_store_lagcov: Engine.lagcov's dict for the columns of this store"""
        return _lagcov_call(lambda *a: load().mcx_store_lagcov(self.h, *a), self.shape[0], self.shape[2], max_lag, nlags, with_ll)

    def modes(self, k, **spec):
        """mcx_store_modes: Engine.modes' Modes for the rows of this store (which must outlive the Modes' rows() calls)"""
        t, nc, ncol = self.shape
        return _modes_call(lambda *a: load().mcx_store_modes(self.h, *a), _modes_spec(k, ncol - 1, **spec), ncol - 1, (t, nc, ncol),
                           lambda *a: load().mcx_store_mode_rows(self.h, *a))

    def evidence(self, vl, proposal=None, **spec):
        """mcx_store_evidence: Engine.evidence's dict for a store whose columns are the parameters vl was sampled in"""
        return _evidence_call(lambda *a: load().mcx_store_evidence(self.h, *a), vl, proposal, **spec)

    def profile_likelihood(self, n=64, levels=None, drops=None, clip=(0, 1), from_=None, to=None, path=False):
        """mcx_store_profile: Engine.profile_likelihood's dict for the columns of this store (of a derived store: the profile
        likelihood of its outputs, functions of the parameters)"""
        ncol = self.shape[2] - 1
        spec = ProfileSpec(n, clip, from_, to, levels, drops).fits(ncol)
        return _profile_call(lambda *a: load().mcx_store_profile(self.h, *a), spec, ncol, path)

    def profile_likelihood2d(self, g=32, pairs=None, levels=None, drops=None, clip=(0, 1), from_=None, to=None):
        """mcx_store_profile2d: Engine.profile_likelihood2d's dict for the columns of this store"""
        ncol = self.shape[2] - 1
        spec = ProfileSpec(g, clip, from_, to, levels, drops, pairs, two_d=True).fits(ncol)
        return _profile2d_call(lambda *a: load().mcx_store_profile2d(self.h, *a), spec, ncol)

    def profile_likelihood_times(self, n=64, clip=(0, 1)):
        """mcx_debug_store_profile_times: Engine.profile_likelihood_times' four stage times for this store"""
        spec = ProfileSpec(n, clip)
        ms = np.zeros(4)
        check(load().mcx_debug_store_profile_times(self.h, C.byref(spec.c), _dp(ms)))
        return ms

    def compare(self, other, iid=False):
        """compare_stores(self, other)"""
        return compare_stores(self, other, iid)

    def energy(self, other, **kw):
        """energy_stores(self, other)"""
        return energy_stores(self, other, **kw)

    def mutual_info(self, **kw):
        """mcx_store_mutinfo: rows_mutual_info's dict for this store's outputs (with_ll: and its last column)"""
        return _mutinfo_call(lambda *a: load().mcx_store_mutinfo(self.h, *a), self.shape[2], **kw)


def derive_rows(rows, nsteps, nc, spec):
    """mcx_rows_derive: the DerivedStore of rows [nsteps * nc, np + 1] on the host (MCout layout)"""
    rows = np.ascontiguousarray(rows, np.float32)
    h = C.c_void_p()
    check(load().mcx_rows_derive(_fp(rows), nsteps, nc, rows.shape[1] - 1, None if spec is None else C.byref(spec.c), C.byref(h)))
    return DerivedStore(h)


# ---- tail-clipped rows (include/mcx.h) ----
TEXT_FALLBACK_CAPACITY = 1024  # include/mcx.h MCX_TEXT_FALLBACK_CAPACITY
PARSE_OK, PARSE_BAD, PARSE_NEEDS_HOST = 0, 1, 2  # mcx_debug_parse_token's status


def _text_spec(nc, ncol, skip_lines, max_rows, piece_bytes):
    return TextSpec(ncol, nc, skip_lines, max_rows, piece_bytes)


def _text_report(rep):
    return {n: getattr(rep, n) for n in ("nrows", "nlines", "ntokens", "nfallback", "npieces", "ncol")}


def parse_text(text, nc, ncol=0, skip_lines=0, max_rows=-1, piece_bytes=0):
    """mcx_text_rows: sample text (bytes: lines of ncol numbers, what MCout::output prints) parsed on the GPU ->
    (rows [nrows, ncol] float32 in MCout layout, the report as a dict of include/mcx.h's fields)"""
    text = bytes(text)
    spec, rep = _text_spec(nc, ncol, skip_lines, max_rows, piece_bytes), TextReport()
    if ncol == 0:  # the report first: it names the columns
        check(load().mcx_text_rows(text, len(text), C.byref(spec), None, 0, C.byref(rep)))
        ncol = rep.ncol
    cap = text.count(b"\n") + 1  # (a row is a line)
    rows = np.empty((cap, max(ncol, 1)), np.float32)
    check(load().mcx_text_rows(text, len(text), C.byref(spec), _fp(rows), cap, C.byref(rep)))
    return rows[:rep.nrows].copy(), _text_report(rep)


def store_from_text(text, nc, ncol=0, skip_lines=0, max_rows=-1, piece_bytes=0):
    """mcx_text_store: (DerivedStore of ncol - 1 columns, then the last column as log L, T = nrows / nc steps; the report)"""
    text = bytes(text)
    spec, rep, h = _text_spec(nc, ncol, skip_lines, max_rows, piece_bytes), TextReport(), C.c_void_p()
    check(load().mcx_text_store(text, len(text), C.byref(spec), C.byref(h), C.byref(rep)))
    return DerivedStore(h), _text_report(rep)


def store_from_file(path, nc, ncol=0, skip_lines=0, max_rows=-1, piece_bytes=0):
    """mcx_file_store: store_from_text of a file, read in pieces"""
    spec, rep, h = _text_spec(nc, ncol, skip_lines, max_rows, piece_bytes), TextReport(), C.c_void_p()
    check(load().mcx_file_store(str(path).encode(), C.byref(spec), C.byref(h), C.byref(rep)))
    return DerivedStore(h), _text_report(rep)


def debug_parse_token(tok):
    """mcx_debug_parse_token (host only): one token (bytes or str) -> (float32 bit pattern, status PARSE_*)"""
    tok = tok.encode() if isinstance(tok, str) else bytes(tok)
    bits, status = C.c_uint32(0), C.c_int(0)
    check(load().mcx_debug_parse_token(tok, len(tok), C.byref(bits), C.byref(status)))
    return bits.value, status.value


def debug_text_times(text, nc, ncol=0, piece_bytes=0):
    """mcx_debug_text_times: (ms[8] = upload, mark, scan, scatter, parse, host line count, host staging, whole call; the report)"""
    text = bytes(text)
    spec, rep, ms = _text_spec(nc, ncol, 0, -1, piece_bytes), TextReport(), np.zeros(8)
    check(load().mcx_debug_text_times(text, len(text), C.byref(spec), C.byref(rep), _dp(ms)))
    return ms, _text_report(rep)


class ClipSpec:
    """an mcx_clip_spec and the arrays it points to: the probabilities (qlo, qhi) of the default thresholds, ll_hi the upper
    threshold of log L (NaN: its qhi quantile; inf: none), lo / hi = None or [ncol] with NaN for a column's default"""

    def __init__(self, qlo=0.01, qhi=0.99, ll_hi=0.0, lo=None, hi=None):
        arr = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1))  # noqa: E731
        self.lo, self.hi = arr(lo), arr(hi)
        self.c = ClipSpecC(float(qlo), float(qhi), float(ll_hi), None if self.lo is None else _dp(self.lo),
                           None if self.hi is None else _dp(self.hi))

    def fits(self, ncol):
        for a in (self.lo, self.hi):
            if a is not None and a.size != ncol:
                raise ValueError("lo and hi take one entry per column (%d), NaN for a column's default" % ncol)
        return self


class RowSet:
    """an mcx_rowset: the rows a clip kept, in source order, with their source row indices.  It owns its device memory.
    report: CLIP_DTYPE [ncol] (lo, hi, nbelow, nabove, flags); nrows = K, nsource = N.  After count_only there is no handle:
    report, nrows, nsource and ncol are all it has."""

    def __init__(self, handle, report, nrows, nsource):
        self.h, self.report, self.nrows, self.nsource, self.ncol = handle, report, int(nrows), int(nsource), len(report)
        self.dropped = 0  # on the DerivedStore of store(): the kept rows from first_row on that its shape left out

    def close(self):
        if self.h:
            load().mcx_rowset_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _span(self, first, n):
        return max(self.nrows - first, 0) if n is None else n

    def rows(self, first=0, n=None):
        """MCout rows [n, ncol] of kept rows [first, first + n) -- n None: to the end"""
        n = self._span(first, n)
        out = np.empty((max(n, 0), self.ncol), np.float32)
        check(load().mcx_rowset_copy(self.h, first, n, _fp(out)))
        return out

    def index(self, first=0, n=None):
        """the source row (step * nc + chain of the clipped range) of kept rows [first, first + n), int64, ascending"""
        n = self._span(first, n)
        out = np.empty(max(n, 0), np.int64)
        check(load().mcx_rowset_index(self.h, first, n, out.ctypes.data_as(C.POINTER(C.c_longlong))))
        return out

    def draw(self, ndraw, seed):
        """ndraw kept rows with replacement: (rows [ndraw, ncol], index [ndraw] int64 into the row set), the index
        debug_draw_indices(seed, nrows, 0, ndraw) gives"""
        rows, index = np.empty((max(ndraw, 0), self.ncol), np.float32), np.empty(max(ndraw, 0), np.int64)
        check(load().mcx_rowset_draw(self.h, seed, ndraw, _fp(rows), index.ctypes.data_as(C.POINTER(C.c_int64))))
        return rows, index

    def store(self, nc=1024, first_row=0, nsteps=None):
        """mcx_rowset_store: kept rows [first_row, first_row + nsteps * nc) as a DerivedStore of nsteps steps of nc
        pseudo-chains, for summary / covariance / density / draw of exactly these rows (its R-hat and ESS mean nothing).
        nsteps None: (nrows - first_row) // nc; the store's .dropped = the kept rows behind first_row it leaves out"""
        if nsteps is None:
            nsteps = (self.nrows - first_row) // nc if nc > 0 else 0
        h = C.c_void_p()
        check(load().mcx_rowset_store(self.h, first_row, nsteps, nc, C.byref(h)))
        st = DerivedStore(h)
        st.dropped = self.dropped = self.nrows - first_row - nsteps * nc
        return st


def _clip_call(fn, spec, ncol, nsource, count_only):
    """fn(spec, cols, nkept, out) of one of the three clip entry points over nsource rows -> RowSet"""
    cols, k, h = np.zeros(ncol, CLIP_DTYPE), C.c_longlong(0), C.c_void_p()
    check(fn(C.byref(spec.c), cols.ctypes.data_as(C.c_void_p), C.byref(k), None if count_only else C.byref(h)))
    return RowSet(h, cols, k.value, nsource)


def clip_rows(rows, nsteps, nc, qlo=0.01, qhi=0.99, ll_hi=0.0, lo=None, hi=None, count_only=False):
    """mcx_rows_clip: Engine.clip's RowSet for rows [nsteps * nc, np + 1] on the host (MCout layout)"""
    rows = np.ascontiguousarray(rows, np.float32)
    ncol = rows.shape[1]
    spec = ClipSpec(qlo, qhi, ll_hi, lo, hi).fits(ncol)
    return _clip_call(lambda *a: load().mcx_rows_clip(_fp(rows), nsteps, nc, ncol - 1, *a), spec, ncol, nsteps * nc, count_only)


def debug_clip_thresholds(q, qlo=0.01, qhi=0.99, ll_hi=0.0, lo=None, hi=None, spec=None):
    """mcx_debug_clip_thresholds (host only): (lo [ncol], hi [ncol]) from q [ncol, 2], the columns' (qlo, qhi) quantiles"""
    q = np.ascontiguousarray(np.asarray(q, np.float64).reshape(-1, 2))
    ncol = q.shape[0]
    spec = spec or ClipSpec(qlo, qhi, ll_hi, lo, hi).fits(ncol)
    tl, th = np.zeros(max(ncol, 1)), np.zeros(max(ncol, 1))
    check(load().mcx_debug_clip_thresholds(ncol, _dp(q), C.byref(spec.c), _dp(tl), _dp(th)))
    return tl[:ncol], th[:ncol]


# ---- the chain table and stores of chosen chains (include/mcx.h) ----
def _chain_table_call(fn, nc, ncol):
    """fn(cols, chains) of one of the three table entry points -> the dict of arrays: mean, sd, rho1 [nc, ncol]; moves,
    longest_stay, ll_max, ll_max_step, flags [nc]"""
    cols, rows = np.zeros((nc, ncol), CHAIN_COL_DTYPE), np.zeros(nc, CHAIN_ROW_DTYPE)
    check(fn(cols.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p)))
    out = {name: cols[name].copy() for name in CHAIN_COL_DTYPE.names}
    out.update({name: rows[name].copy() for name in CHAIN_ROW_DTYPE.names})
    return out


def rows_chain_table(rows, nsteps, nc):
    """mcx_rows_chain_table: Engine.chain_table's dict for rows [nsteps * nc, np + 1] on the host (MCout layout)"""
    rows = np.ascontiguousarray(rows, np.float32)
    ncol = rows.shape[1]
    return _chain_table_call(lambda *a: load().mcx_rows_chain_table(_fp(rows), nsteps, nc, ncol - 1, *a), nc, ncol)


def keep_chains(table, z=5.0, min_moves=1, max_stay=0, use_col=None):
    """mcx_chains_keep (host only) on a chain_table dict: (reasons [nc] int32 -- 0 = kept, else CHAIN_NONFINITE | CHAIN_STUCK |
    CHAIN_OUTLIER --, centre [ncol, 2] = (median, 1.4826 MAD) of the chain means per column that takes part, kept_indices
    int32).  use_col: None = every column, else [ncol], non-zero = the column takes part in the outlier test"""
    mean = np.asarray(table["mean"], np.float64)
    nc, ncol = mean.shape
    cols, rows = np.zeros((nc, ncol), CHAIN_COL_DTYPE), np.zeros(nc, CHAIN_ROW_DTYPE)
    for name in CHAIN_COL_DTYPE.names:
        cols[name] = table[name]
    for name in CHAIN_ROW_DTYPE.names:
        rows[name] = table[name]
    use = None
    if use_col is not None:
        use = np.ascontiguousarray(np.asarray(use_col).reshape(-1) != 0, np.uint8)
        if use.size != ncol:
            raise ValueError("use_col takes one entry per column (%d)" % ncol)
    rule = ChainRule(float(z), int(min_moves), int(max_stay), None if use is None else use.ctypes.data_as(C.POINTER(C.c_ubyte)))
    reasons, centre, nkept = np.zeros(nc, np.int32), np.zeros((ncol, 2)), C.c_int(0)
    check(load().mcx_chains_keep(nc, ncol, cols.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p), C.byref(rule),
                                 reasons.ctypes.data_as(C.POINTER(C.c_int)), _dp(centre), C.byref(nkept)))
    kept = np.flatnonzero(reasons == 0).astype(np.int32)
    assert kept.size == nkept.value
    return reasons, centre, kept


def _select_call(fn, chains):
    """fn(chains, nsel, out) of one of the three selection entry points -> DerivedStore"""
    sel = np.ascontiguousarray(np.asarray(chains).reshape(-1), np.int32)
    h = C.c_void_p()
    check(fn(sel.ctypes.data_as(C.POINTER(C.c_int)), sel.size, C.byref(h)))
    return DerivedStore(h)


def select_chains_rows(rows, nsteps, nc, chains):
    """mcx_rows_select_chains: Engine.select_chains' DerivedStore for rows [nsteps * nc, np + 1] on the host (MCout layout)"""
    rows = np.ascontiguousarray(rows, np.float32)
    return _select_call(lambda *a: load().mcx_rows_select_chains(_fp(rows), nsteps, nc, rows.shape[1] - 1, *a), chains)


def debug_chains_geometry(np_, nsteps, nc, nsel=1):
    """mcx_debug_chains_geometry (host only): the launch geometry of the series, row and gather sweeps for a store of nsteps
    steps of nc chains of np_ parameters and a selection of nsel chains, as a dict of include/mcx.h's fields"""
    g = ChainsGeometry()
    check(load().mcx_debug_chains_geometry(np_, nsteps, nc, nsel, C.byref(g)))
    return {name: int(getattr(g, name)) for name, _ in ChainsGeometry._fields_}


# ---- the step table and where the ensemble settled (include/mcx.h) ----
def _step_table_call(fn, nsteps, ncol, probs):
    """fn(probs, nprobs, cols, steps, quantiles) of one of the three table entry points -> the dict of arrays: mean, sd, min,
    max, flags [T, ncol]; quantiles [T, ncol, nprobs]; moved, ll_max, ll_max_chain, step_flags [T]"""
    p, pp = _probs(probs)
    T = max(int(nsteps), 0)
    cols, rows = np.zeros((T, ncol), STEP_COL_DTYPE), np.zeros(T, STEP_ROW_DTYPE)
    q = np.zeros((T, ncol, len(p)), np.float64)
    check(fn(pp if len(p) else None, len(p), cols.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p),
             _dp(q) if len(p) else None))
    out = {name: cols[name].copy() for name in ("mean", "sd", "min", "max", "flags")}
    out["quantiles"] = q
    out.update({name: rows[name].copy() for name in ("moved", "ll_max", "ll_max_chain")})
    out["step_flags"] = rows["flags"].copy()
    return out


def rows_step_table(rows, nsteps, nc, probs=(0.05, 0.5, 0.95)):
    """mcx_rows_step_table: Engine.step_table's dict for rows [nsteps * nc, np + 1] on the host (MCout layout)"""
    rows = np.ascontiguousarray(rows, np.float32)
    ncol = rows.shape[1]
    return _step_table_call(lambda *a: load().mcx_rows_step_table(_fp(rows), nsteps, nc, ncol - 1, *a), nsteps, ncol, probs)


def settle_steps(table, tol_mean=0.1, tol_sd=0.1, ref_frac=0.5, use_col=None):
    """mcx_steps_settle (host only) on a step_table dict: (settled_step, per-column dict).  settled_step = 1 + the last step
    whose mean or sd of a column that takes part lies outside the band around the last ceil(ref_frac T) steps' (m_ref, s_ref);
    0 when every step is in band; -1 = not settled.  The dict holds m_ref, s_ref, max_dev_mean, max_dev_sd (in units of s_ref)
    and last_out [ncol].  use_col: None = every column, else [ncol], non-zero = the column takes part"""
    mean = np.asarray(table["mean"], np.float64)
    T, ncol = mean.shape
    cols = np.zeros((T, ncol), STEP_COL_DTYPE)
    for name in ("mean", "sd", "min", "max", "flags"):
        cols[name] = table[name]
    use = None
    if use_col is not None:
        use = np.ascontiguousarray(np.asarray(use_col).reshape(-1) != 0, np.uint8)
        if use.size != ncol:
            raise ValueError("use_col takes one entry per column (%d)" % ncol)
    rule = StepRule(float(tol_mean), float(tol_sd), float(ref_frac), None if use is None else use.ctypes.data_as(C.POINTER(C.c_ubyte)))
    out, settled = np.zeros(ncol, STEP_SETTLE_DTYPE), C.c_int(0)
    check(load().mcx_steps_settle(T, ncol, cols.ctypes.data_as(C.c_void_p), C.byref(rule), out.ctypes.data_as(C.c_void_p),
                                  C.byref(settled)))
    return settled.value, {name: out[name].copy() for name in ("m_ref", "s_ref", "max_dev_mean", "max_dev_sd", "last_out")}


def debug_steptable_geometry(np_, nsteps, nc, nprobs=3):
    """mcx_debug_steptable_geometry (host only): the launch geometry of the moments, select and row sweeps for a table of
    nsteps steps of nc chains of np_ parameters and nprobs probabilities, as a dict of include/mcx.h's fields"""
    g = SteptableGeometry()
    check(load().mcx_debug_steptable_geometry(np_, nsteps, nc, nprobs, C.byref(g)))
    return {name: int(getattr(g, name)) for name, _ in SteptableGeometry._fields_}


# ---- two stores compared (include/mcx.h) ----
def _compare_call(fn, ncol, iid):
    """fn(spec, cols) of one of the four compare entry points -> the dict of arrays [ncol]: ks_plus_num, ks_minus_num (int64),
    ks_plus_x, ks_minus_x, ks, w1, mean_a, sd_a, ess_a, mean_b, sd_b, ess_b, z_mean, ks_neff, ks_p, na, nb, flags"""
    spec = CompareSpecC(COMPARE_IID if iid else 0)
    cols = np.zeros(max(int(ncol), 1), COMPARE_DTYPE)
    check(fn(C.byref(spec), cols.ctypes.data_as(C.c_void_p)))
    return {name: cols[name].copy() for name in COMPARE_DTYPE.names if name != "reserved"}


def compare_rows(rows_a, nsteps_a, nc_a, rows_b, nsteps_b, nc_b, iid=False):
    """mcx_rows_compare: do rows_a [nsteps_a * nc_a, np + 1] and rows_b [nsteps_b * nc_b, np + 1] (MCout layout) sample the same
    distribution?  Per column the exact two-sample Kolmogorov-Smirnov distance, the Wasserstein-1 distance, each side's mean,
    sd and ESS, the z of the means and the Kolmogorov probability at the effective sizes (iid: at the sample sizes)"""
    rows_a, rows_b = np.ascontiguousarray(rows_a, np.float32), np.ascontiguousarray(rows_b, np.float32)
    ncol = rows_a.shape[1]
    if rows_b.shape[1] != ncol:
        raise ValueError("rows_a has %d columns and rows_b %d" % (ncol, rows_b.shape[1]))
    return _compare_call(lambda *a: load().mcx_rows_compare(_fp(rows_a), nsteps_a, nc_a, _fp(rows_b), nsteps_b, nc_b, ncol - 1, *a),
                         ncol, iid)


def compare_stores(a, b, iid=False):
    """mcx_store_compare: compare_rows' dict for two DerivedStores on one device"""
    return _compare_call(lambda *args: load().mcx_store_compare(a.h, b.h, *args), a.shape[2], iid)


def ks_prob(ks, ess_a, ess_b):
    """mcx_ks_prob (host only): (ks_neff, ks_p) of a Kolmogorov-Smirnov distance between samples of effective sizes ess_a, ess_b"""
    neff, p = C.c_double(0.0), C.c_double(0.0)
    check(load().mcx_ks_prob(ks, ess_a, ess_b, C.byref(neff), C.byref(p)))
    return neff.value, p.value


def debug_compare_geometry(na, nb, ncol):
    """mcx_debug_compare_geometry (host only): the launch geometry of a comparison of na against nb values per column, as a dict
    of include/mcx.h's fields"""
    g = CompareGeometry()
    check(load().mcx_debug_compare_geometry(na, nb, ncol, C.byref(g)))
    return {name: int(getattr(g, name)) for name, _ in CompareGeometry._fields_}


def debug_compare_store_geometry(nsteps_a, nc_a, nsteps_b, nc_b, ncol):
    """mcx_debug_compare_store_geometry (host only): debug_compare_geometry of nsteps_a * nc_a against nsteps_b * nc_b values,
    with the step chunks of the key sweeps, which depend on the steps"""
    g = CompareGeometry()
    check(load().mcx_debug_compare_store_geometry(nsteps_a, nc_a, nsteps_b, nc_b, ncol, C.byref(g)))
    return {name: int(getattr(g, name)) for name, _ in CompareGeometry._fields_}


# ---- two stores compared jointly (include/mcx.h) ----
def _energy_spec(n_a=0, n_b=0, nperm=999, seed=0, with_ll=False, raw=False):
    return EnergySpecC(n_a, n_b, nperm, seed, (ENERGY_WITH_LL if with_ll else 0) | (ENERGY_RAW if raw else 0))


def _energy_call(fn, ncol, **kw):
    """fn(spec, res, cols, perm_e) of one of the four energy entry points -> the dict of mcx_energy_result's fields (e, h,
    mean_ab, mean_aa, mean_bb, p_value, nge, n_a, n_b, nperm, nused, na_rows, nb_rows), scale and flags [ncol] per column and
    perm_e [nperm]"""
    spec, res = _energy_spec(**kw), EnergyResultC()
    cols = np.zeros(max(int(ncol), 1), ENERGY_COL_DTYPE)
    perm_e = np.zeros(max(int(spec.nperm), 0))
    check(fn(C.byref(spec), C.byref(res), cols.ctypes.data_as(C.c_void_p), _dp(perm_e) if len(perm_e) else None))
    out = {name: getattr(res, name) for name, _ in EnergyResultC._fields_}
    out.update(scale=cols["scale"].copy(), flags=cols["flags"].copy(), perm_e=perm_e)
    return out


def energy_rows(rows_a, nsteps_a, nc_a, rows_b, nsteps_b, nc_b, **kw):
    """mcx_rows_energy: do rows_a [nsteps_a * nc_a, np + 1] and rows_b [nsteps_b * nc_b, np + 1] (MCout layout) sample the same
    joint distribution?  The energy distance between n_a rows of A and n_b of B (> 0: draws with replacement, 0: min(rows, 2048)
    draws, -1: every row) in the columns scaled by their pooled sd (raw: unscaled; with_ll: log L too), and its law under nperm
    permutations of the pooled labels: e, h, p_value = (1 + nge) / (1 + nperm).  Exact for exchangeable rows only"""
    rows_a, rows_b = np.ascontiguousarray(rows_a, np.float32), np.ascontiguousarray(rows_b, np.float32)
    ncol = rows_a.shape[1]
    if rows_b.shape[1] != ncol:
        raise ValueError("rows_a has %d columns and rows_b %d" % (ncol, rows_b.shape[1]))
    return _energy_call(lambda *a: load().mcx_rows_energy(_fp(rows_a), nsteps_a, nc_a, _fp(rows_b), nsteps_b, nc_b, ncol - 1, *a),
                        ncol, **kw)


def energy_stores(a, b, **kw):
    """mcx_store_energy: energy_rows' dict for two DerivedStores on one device"""
    return _energy_call(lambda *args: load().mcx_store_energy(a.h, b.h, *args), a.shape[2], **kw)


def debug_energy_sums(rows_a, nsteps_a, nc_a, rows_b, nsteps_b, nc_b, **kw):
    """mcx_debug_energy_sums: energy_rows' device sums -- (S, S_A [1 + nperm], S_AA [1 + nperm]), label vector 0 first"""
    rows_a, rows_b = np.ascontiguousarray(rows_a, np.float32), np.ascontiguousarray(rows_b, np.float32)
    spec = _energy_spec(**kw)
    sums = np.zeros(3 + 2 * spec.nperm)
    check(load().mcx_debug_energy_sums(_fp(rows_a), nsteps_a, nc_a, _fp(rows_b), nsteps_b, nc_b, rows_a.shape[1] - 1, C.byref(spec),
                                       _dp(sums)))
    return sums[0], sums[1::2].copy(), sums[2::2].copy()


def debug_energy_labels(seed, n_a, n_b, p):
    """mcx_debug_energy_labels (host only): the label vector [n_a + n_b] (uint8, n_a ones) of permutation p"""
    labels = np.zeros(max(n_a, 0) + max(n_b, 0), np.uint8)
    check(load().mcx_debug_energy_labels(seed, n_a, n_b, p, labels.ctypes.data_as(C.c_void_p)))
    return labels


def debug_energy_geometry(n_a, n_b, nused, nperm):
    """mcx_debug_energy_geometry (host only): the launch geometry of n_a against n_b rows of nused columns with nperm
    permutations, as a dict of include/mcx.h's fields"""
    g = EnergyGeometry()
    check(load().mcx_debug_energy_geometry(n_a, n_b, nused, nperm, C.byref(g)))
    return {name: int(getattr(g, name)) for name, _ in EnergyGeometry._fields_}


# ---- mutual information between columns of a store (include/mcx.h) ----
class _MutinfoSpec:
    """mcx_mutinfo_spec and the array its pair list points into"""

    def __init__(self, n=0, k=0, nperm=0, seed=0, pairs=None, with_ll=False, raw=False):
        self.pairs = None if pairs is None else np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        flags = (MUTINFO_WITH_LL if with_ll else 0) | (MUTINFO_RAW if raw else 0)
        self.c = MutinfoSpecC(n, k, nperm, seed, flags, 0 if self.pairs is None else len(self.pairs),
                              None if self.pairs is None else self.pairs.ctypes.data_as(C.POINTER(C.c_int)))
        self.with_ll = bool(with_ll)

    def npairs(self, ncol):
        """how many pairs the call answers with (what the library refuses is sized for generously)"""
        if self.pairs is not None:
            return max(len(self.pairs), 1)
        u = max(int(ncol) - (0 if self.with_ll else 1), 2)
        return u * (u - 1) // 2


def _mutinfo_call(fn, ncol, **kw):
    """fn(spec, res, cols, pairs, perm_mi) of one of the three entry points -> the dict of mcx_mutinfo_result's fields (n_rows,
    n_sel, ndup, m, k, npairs, nperm, nused), scale and flags [ncol] per column, pairs (MUTINFO_PAIR_DTYPE [npairs]: a, b, mi,
    r_info, pearson, perm_mean, perm_sd, p_value, nge, nzero, flags) and perm_mi [npairs, nperm]"""
    spec, res = _MutinfoSpec(**kw), MutinfoResultC()
    cols = np.zeros(max(int(ncol), 1), MUTINFO_COL_DTYPE)
    room = spec.npairs(ncol)
    pairs = np.zeros(room, MUTINFO_PAIR_DTYPE)
    perm_mi = np.zeros((room, max(int(spec.c.nperm), 0)))
    check(fn(C.byref(spec.c), C.byref(res), cols.ctypes.data_as(C.c_void_p), pairs.ctypes.data_as(C.c_void_p),
             _dp(perm_mi) if perm_mi.size else None))
    out = {name: getattr(res, name) for name, _ in MutinfoResultC._fields_}
    out.update(scale=cols["scale"].copy(), flags=cols["flags"].copy(), pairs=pairs[:res.npairs], perm_mi=perm_mi[:res.npairs])
    return out


def rows_mutual_info(rows, nsteps, nc, **kw):
    """mcx_rows_mutinfo: which columns of rows [nsteps * nc, np + 1] (MCout layout) depend on each other at all -- the mutual
    information of every pair of parameters (pairs: [(a, b), ...] names them; with_ll: log L too) in nats by the k-nearest-neighbour
    estimator (k, default 3) on n rows evenly spaced in store order (0: min(rows, 4096), -1: all) scaled by their sd (raw:
    unscaled), repeated rows dropped (ndup), with nperm permutations of the second column as the null: mi, r_info (on the scale of
    a correlation), pearson, p_value = (1 + nge) / (1 + nperm)"""
    rows = np.ascontiguousarray(rows, np.float32)
    return _mutinfo_call(lambda *a: load().mcx_rows_mutinfo(_fp(rows), nsteps, nc, rows.shape[1] - 1, *a), rows.shape[1], **kw)


def debug_mutinfo_rows(N, n):
    """mcx_debug_mutinfo_rows (host only): the n rows floor(i N / n) taken of N"""
    index = np.zeros(max(int(n), 1), np.int64)
    check(load().mcx_debug_mutinfo_rows(N, n, index.ctypes.data_as(C.POINTER(C.c_longlong))))
    return index


def debug_mutinfo_perm(seed, m, p):
    """mcx_debug_mutinfo_perm (host only): pi_p on [0, m)"""
    perm = np.zeros(max(int(m), 1), np.int32)
    check(load().mcx_debug_mutinfo_perm(seed, m, p, perm.ctypes.data_as(C.POINTER(C.c_int))))
    return perm


def debug_mutinfo_psi(q_max):
    """mcx_debug_mutinfo_psi (host only): table[q - 1] = psi(q), q = 1 ... q_max"""
    table = np.zeros(max(int(q_max), 1))
    check(load().mcx_debug_mutinfo_psi(q_max, _dp(table)))
    return table


def mutinfo_finish(eps, na, nb, k):
    """mcx_mutinfo_finish (host only): eps, na, nb [m] of one pair -> (mi, nzero)"""
    eps = np.ascontiguousarray(eps, np.float64)
    na, nb = np.ascontiguousarray(na, np.int32), np.ascontiguousarray(nb, np.int32)
    mi, nzero = C.c_double(0.0), C.c_longlong(0)
    check(load().mcx_mutinfo_finish(_dp(eps), na.ctypes.data_as(C.POINTER(C.c_int)), nb.ctypes.data_as(C.POINTER(C.c_int)), len(eps), k,
                                    C.byref(mi), C.byref(nzero)))
    return mi.value, nzero.value


def debug_mutinfo_points(rows, nsteps, nc, **kw):
    """mcx_debug_mutinfo_points (host only): the host half on host rows -- mcx_mutinfo_result's fields, index and kept [n_sel],
    scale and flags [ncol], z [ncol, m]"""
    rows = np.ascontiguousarray(rows, np.float32)
    ncol = rows.shape[1]
    spec, res = _MutinfoSpec(**kw), MutinfoResultC()
    N = int(nsteps) * int(nc)
    room = max(spec.c.n if spec.c.n > 0 else min(N, 4096) if spec.c.n == 0 else N, 1)
    index, kept = np.zeros(room, np.int64), np.zeros(room, np.uint8)
    cols, z = np.zeros(ncol, MUTINFO_COL_DTYPE), np.zeros(ncol * room)
    check(load().mcx_debug_mutinfo_points(_fp(rows), nsteps, nc, ncol - 1, C.byref(spec.c), C.byref(res),
                                          index.ctypes.data_as(C.POINTER(C.c_longlong)), kept.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                          cols.ctypes.data_as(C.c_void_p), _dp(z)))
    out = {name: getattr(res, name) for name, _ in MutinfoResultC._fields_}
    out.update(index=index[:res.n_sel], kept=kept[:res.n_sel], scale=cols["scale"].copy(), flags=cols["flags"].copy(),
               z=z[:ncol * res.m].reshape(ncol, res.m).copy())
    return out


def debug_mutinfo_geometry(m, npairs, nperm, k):
    """mcx_debug_mutinfo_geometry (host only): the launch geometry as a dict of include/mcx.h's fields"""
    g = MutinfoGeometry()
    check(load().mcx_debug_mutinfo_geometry(m, npairs, nperm, k, C.byref(g)))
    return {name: int(getattr(g, name)) for name, _ in MutinfoGeometry._fields_}


def debug_mutinfo_counts(rows, nsteps, nc, pair, p, **kw):
    """mcx_debug_mutinfo_counts: (eps, na, nb) [m] of pair `pair` of the call's list under permutation p, from k_mi_pairs itself"""
    rows = np.ascontiguousarray(rows, np.float32)
    m = debug_mutinfo_points(rows, nsteps, nc, **kw)["m"]
    spec = _MutinfoSpec(**kw)
    eps, na, nb = np.zeros(m), np.zeros(m, np.int32), np.zeros(m, np.int32)
    check(load().mcx_debug_mutinfo_counts(_fp(rows), nsteps, nc, rows.shape[1] - 1, C.byref(spec.c), pair, p, _dp(eps),
                                          na.ctypes.data_as(C.POINTER(C.c_int)), nb.ctypes.data_as(C.POINTER(C.c_int))))
    return eps, na, nb


# ---- importance weights on a store (include/mcx.h) ----
class Weights:
    """an mcx_weights and what it points to"""

    def __init__(self, kind, logw=None, store=None, col=0, scale=1.0):
        self.logw = None if logw is None else np.ascontiguousarray(np.asarray(logw, np.float32).reshape(-1))
        self.store = store
        self.c = WeightsC(kind, None if self.logw is None else _fp(self.logw), None if store is None else store.h, col, scale)


def weights_host(logw):
    """MCX_WEIGHT_HOST: one log-weight per row, in row order (step-major, the chain within the step)"""
    return Weights(WEIGHT_HOST, logw=logw)


def weights_column(store, col, scale=1.0):
    """MCX_WEIGHT_STORE: scale times column col of a DerivedStore of the same steps and chains (col = ncol - 1: its log L)"""
    return Weights(WEIGHT_STORE, store=store, col=col, scale=scale)


def weights_loglike(scale):
    """MCX_WEIGHT_LL: scale times the rows' own log L column (scale = beta - 1: the power posterior L^beta)"""
    return Weights(WEIGHT_LL, scale=scale)


def _reweight_call(fn, weights, ncol, probs):
    """fn(w, probs, nprobs, res, cols, quantiles) of one of the three reweight entry points -> the dict of
    mcx_reweight_result's fields (n, nzero, lwmax, sumq, sumq2_hi, sumq2_lo, sumq2 as a Python integer, ess_kish, log_mean_w,
    tail_m, khat, tail_sigma, flags), cols (arrays [ncol]: mean, sd, mcse_mean, min, max, flags) and quantiles [ncol, nprobs]"""
    p, pp = _probs(probs)
    res = ReweightResultC()
    cols = np.zeros(max(int(ncol), 1), REWEIGHT_DTYPE)
    q = np.zeros((max(int(ncol), 1), len(p)), np.float64)
    check(fn(None if weights is None else C.byref(weights.c), pp if len(p) else None, len(p), C.byref(res),
             cols.ctypes.data_as(C.c_void_p), _dp(q) if len(p) else None))
    out = {name: getattr(res, name) for name, _ in ReweightResultC._fields_ if name != "reserved"}
    out["sumq2"] = (int(res.sumq2_hi) << 64) | int(res.sumq2_lo)
    out["cols"] = {name: cols[name].copy() for name in REWEIGHT_DTYPE.names if name != "reserved"}
    out["quantiles"] = q
    return out


def reweight_rows(rows, nsteps, nc, weights, probs=(0.05, 0.5, 0.95)):
    """mcx_rows_reweight: rows [nsteps * nc, np + 1] (MCout layout) under importance weights -- Kish's effective size, the
    log of the mean weight, the Pareto tail index k-hat of the largest weights, and per column the weighted mean, sd, error
    of the mean, min, max and exact weighted quantiles (no interpolation)"""
    rows = np.ascontiguousarray(rows, np.float32)
    ncol = rows.shape[1]
    return _reweight_call(lambda *a: load().mcx_rows_reweight(_fp(rows), nsteps, nc, ncol - 1, *a), weights, ncol, probs)


def _resample_call(fn, weights, nsteps_out, nc_out, seed, with_index):
    """fn(w, seed, nsteps_out, nc_out, out, index) of one of the three resample entry points -> the DerivedStore, or
    (DerivedStore, index [nsteps_out * nc_out] int64) with with_index"""
    h = C.c_void_p()
    index = np.empty(max(int(nsteps_out) * int(nc_out), 0), np.int64) if with_index else None
    check(fn(None if weights is None else C.byref(weights.c), seed, nsteps_out, nc_out, C.byref(h),
             index.ctypes.data_as(C.POINTER(C.c_int64)) if with_index else None))
    st = DerivedStore(h)
    return (st, index) if with_index else st


def resample_rows(rows, nsteps, nc, weights, nsteps_out, nc_out, seed, with_index=False):
    """mcx_rows_resample: nsteps_out * nc_out rows of rows [nsteps * nc, np + 1] drawn with replacement in proportion to their
    weights, as a DerivedStore of shape (nsteps_out, nc_out, np + 1) whose rows are exchangeable draws, not chains"""
    rows = np.ascontiguousarray(rows, np.float32)
    return _resample_call(lambda *a: load().mcx_rows_resample(_fp(rows), nsteps, nc, rows.shape[1] - 1, *a), weights, nsteps_out,
                          nc_out, seed, with_index)


def khat_of_tail(x):
    """mcx_khat_of_tail (host only): (khat, sigma, flags) of the rising exceedances x of a tail over its cutoff"""
    x = np.ascontiguousarray(np.asarray(x, np.float64).reshape(-1))
    k, s, f = C.c_double(0.0), C.c_double(0.0), C.c_int(0)
    check(load().mcx_khat_of_tail(_dp(x), len(x), C.byref(k), C.byref(s), C.byref(f)))
    return k.value, s.value, f.value


def debug_reweight_q(weights, rows=None, nsteps=0, nc=0, store=None):
    """mcx_debug_reweight_q: (q [N] uint32, lwmax) -- the fixed-point weights of host rows (rows, nsteps, nc) or of a
    DerivedStore (store)"""
    if store is not None:
        t, c, _ = store.shape
        q, mx = np.zeros(t * c, np.uint32), C.c_double(0.0)
        check(load().mcx_debug_reweight_q(store.h, None, 0, 0, 0, C.byref(weights.c), q.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(mx)))
        return q, mx.value
    rows = np.ascontiguousarray(rows, np.float32)
    q, mx = np.zeros(max(nsteps * nc, 1), np.uint32), C.c_double(0.0)
    check(load().mcx_debug_reweight_q(None, _fp(rows), nsteps, nc, rows.shape[1] - 1, C.byref(weights.c),
                                      q.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(mx)))
    return q[:nsteps * nc], mx.value


class IntervalSpec:
    """mcx_interval_spec: the masses of the highest-density intervals and the probabilities of the quantiles with an error"""

    def __init__(self, hdi=(0.9,), probs=(0.05, 0.5, 0.95)):
        self.mass, mp = _probs(hdi)
        self.probs, pp = _probs(probs)
        self.c = IntervalSpecC(len(self.mass), len(self.probs), mp if len(self.mass) else None, pp if len(self.probs) else None)


def _intervals_call(fn, ncol, hdi, probs):
    """fn(spec, cols, hdi, qse) of one of the three intervals entry points -> a dict of arrays [ncol]: mean, sd, ess_sd,
    mcse_sd, ess_sd_lag, flags; hdi: a dict of arrays [ncol, nmass] (width, index, span, lo, hi); quantiles: a dict of arrays
    [ncol, nprobs] (q, ess_q, u_lo, u_hi, mcse_q, k_lo, k_hi, s_lo, s_hi, ess_q_lag)"""
    spec = IntervalSpec(hdi, probs)
    ncol = max(int(ncol), 1)
    cols = np.zeros(ncol, INTERVALS_DTYPE)
    h = np.zeros((ncol, len(spec.mass)), HDI_DTYPE)
    q = np.zeros((ncol, len(spec.probs)), QUANTILE_SE_DTYPE)
    check(fn(C.byref(spec.c), cols.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p) if h.size else None,
             q.ctypes.data_as(C.c_void_p) if q.size else None))
    out = {name: cols[name].copy() for name in INTERVALS_DTYPE.names}
    out["hdi"] = {name: h[name].copy() for name in HDI_DTYPE.names}
    out["quantiles"] = {name: q[name].copy() for name in QUANTILE_SE_DTYPE.names if name != "reserved"}
    return out


def rows_intervals(rows, nsteps, nc, hdi=(0.9,), probs=(0.05, 0.5, 0.95)):
    """mcx_rows_intervals: Engine.intervals' dict for rows [nsteps * nc, np + 1] on the host (MCout layout)"""
    rows = np.ascontiguousarray(rows, np.float32)
    ncol = rows.shape[1]
    return _intervals_call(lambda *a: load().mcx_rows_intervals(_fp(rows), nsteps, nc, ncol - 1, *a), ncol, hdi, probs)


def beta_quantile(p, a, b):
    """mcx_beta_quantile (host only): the quantile of probability p of the beta law (a, b), a >= 1 and b >= 1, float64"""
    x = C.c_double()
    check(load().mcx_beta_quantile(p, a, b, C.byref(x)))
    return x.value


def intervals_quantile_ranks(N, prob, ess):
    """mcx_intervals_quantile_ranks (host only): (u_lo, u_hi, k_lo, k_hi) around the quantile of probability prob of N sorted
    values whose indicator has the effective size ess"""
    ul, uh, kl, kh = C.c_double(), C.c_double(), C.c_longlong(), C.c_longlong()
    check(load().mcx_intervals_quantile_ranks(N, prob, ess, C.byref(ul), C.byref(uh), C.byref(kl), C.byref(kh)))
    return ul.value, uh.value, kl.value, kh.value


def debug_intervals_geometry(nsteps, nc, np_, nmass=1, nprobs=3):
    """mcx_debug_intervals_geometry (host only): the launch geometry of an intervals call on nsteps steps of nc chains of np_
    parameters with nmass masses and nprobs probabilities, as a dict of include/mcx.h's fields"""
    g = IntervalsGeometry()
    check(load().mcx_debug_intervals_geometry(nsteps, nc, np_, nmass, nprobs, C.byref(g)))
    return {name: int(getattr(g, name)) for name, _ in IntervalsGeometry._fields_}


def _lagcov_dict(res, cols, sigma, gamma):
    """the fields of mcx_lagcov_result; mean, ess, mcse, col_flags [ncol]; sigma and mcse_cov = sigma / N [ncol, ncol]; gamma
    [nlags, ncol, ncol] and ccf = G(t)_ij / sqrt(G(0)_ii G(0)_jj): NaN where a variance is 0 or NaN, else exactly 1 on the diagonal
    of lag 0"""
    out = {name: getattr(res, name) for name, _ in LagcovResultC._fields_}
    out.update(mean=cols["mean"].copy(), ess=cols["ess"].copy(), mcse=cols["mcse"].copy(), col_flags=cols["flags"].copy(),
               sigma=sigma, mcse_cov=sigma / res.N, gamma=gamma)
    ccf = gamma.copy()
    if gamma.shape[0]:
        v = np.diag(gamma[0]).copy()
        v[~(v > 0)] = np.nan
        sd = np.sqrt(v)
        with np.errstate(invalid="ignore"):
            ccf = gamma / np.outer(sd, sd)
        k = np.flatnonzero(~np.isnan(v))
        ccf[0, k, k] = 1.0
    out["ccf"] = ccf
    return out


def _lagcov_call(fn, nsteps, ncol, max_lag, nlags, with_ll):
    """fn(spec, res, cols, sigma, gamma) of one of the three lagcov entry points -> _lagcov_dict.  max_lag None: every lag of the
    range"""
    spec = LagcovSpecC(max(int(nsteps) - 1, 1) if max_lag is None else int(max_lag), int(nlags), 1 if with_ll else 0)
    ncol = max(int(ncol), 1)
    res, cols, sigma = LagcovResultC(), np.zeros(ncol, LAGCOV_DTYPE), np.zeros((ncol, ncol))
    gamma = np.zeros((max(int(nlags), 0), ncol, ncol))
    check(fn(C.byref(spec), C.byref(res), cols.ctypes.data_as(C.c_void_p), _dp(sigma), _dp(gamma) if gamma.size else None))
    return _lagcov_dict(res, cols, sigma, gamma)


def rows_lagcov(rows, nsteps, nc, max_lag=None, nlags=0, with_ll=False):
    """mcx_rows_lagcov: Engine.lagcov's dict for rows [nsteps * nc, np + 1] on the host (MCout layout)"""
    rows = np.ascontiguousarray(rows, np.float32)
    ncol = rows.shape[1]
    return _lagcov_call(lambda *a: load().mcx_rows_lagcov(_fp(rows), nsteps, nc, ncol - 1, *a), nsteps, ncol, max_lag, nlags, with_ll)


def mess_finish(gamma, N, use=None):
    """mcx_mess_finish (host only): the walk of DESIGN.md section 24 on given matrices gamma [nlags, ncol, ncol] of N rows, use
    [ncol] the chosen columns (None: all) -> _lagcov_dict (mean is NaN; gamma and ccf are those given)"""
    gamma = np.ascontiguousarray(gamma, np.float64)
    nlags, ncol = gamma.shape[0], gamma.shape[1] if gamma.ndim == 3 else 0
    res, cols, sigma = LagcovResultC(), np.zeros(max(ncol, 1), LAGCOV_DTYPE), np.zeros((max(ncol, 1),) * 2)
    u = None if use is None else np.ascontiguousarray(np.asarray(use, bool), np.uint8)
    check(load().mcx_mess_finish(ncol, nlags, int(N), _dp(gamma), None if u is None else u.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                 C.byref(res), cols.ctypes.data_as(C.c_void_p), _dp(sigma)))
    return _lagcov_dict(res, cols, sigma, gamma)


def debug_lagcov_geometry(nsteps, nc, np_, nlags=1):
    """mcx_debug_lagcov_geometry (host only): the launch geometry of a lagcov call on nsteps steps of nc chains of np_ parameters
    that computes lags 0 .. nlags - 1, as a dict of include/mcx.h's fields"""
    g = LagcovGeometry()
    check(load().mcx_debug_lagcov_geometry(nsteps, nc, np_, nlags, C.byref(g)))
    return {name: int(getattr(g, name)) for name, _ in LagcovGeometry._fields_}


# ---- modes of a store (include/mcx.h) ----
MODES_MAX_K, MODE_NONE, MODES_TIMES = 32, 255, 8  # include/mcx.h MCX_MODES_MAX_K, MCX_MODE_NONE, MCX_MODES_TIMES
MODES_CONVERGED, MODES_NOT_CONVERGED, MODES_EMPTY = 1, 2, 4
MODE_ROW_DTYPE = np.dtype([("n", np.int64), ("ll_max_row", np.int64), ("weight", np.float64), ("inertia", np.float64),
                           ("ll_mean", np.float64), ("ll_max", np.float32), ("flags", np.int32)], align=True)
MODE_CHAIN_DTYPE = np.dtype([("hops", np.int64), ("dominant_steps", np.int64), ("dominant", np.int32), ("first_label", np.int32),
                             ("last_label", np.int32), ("reserved", np.int32)], align=True)
assert MODE_ROW_DTYPE.itemsize == 48 and MODE_CHAIN_DTYPE.itemsize == 32


def _modes_spec(k, np_, max_iter=50, scale=True, seed_rows=16384, seed=0, centres=None):
    """(mcx_modes_spec, the array it points to)"""
    c = None
    if centres is not None:
        c = np.ascontiguousarray(np.asarray(centres, np.float64).reshape(-1))
        if c.size != int(k) * np_:
            raise ValueError("centres takes [k, np] = [%d, %d] values" % (k, np_))
    return ModesSpecC(int(k), int(max_iter), 1 if scale else 0, int(seed_rows), int(seed) & 0xffffffff, None if c is None else _dp(c)), c


class Modes:
    """an mcx_modes with the tables of its call: the labels of every row of the source stay on the device, owned by this object.
    result: dict of mcx_modes_result's fields; table: dict of arrays [k] (n, weight, inertia, ll_mean, ll_max, ll_max_row, flags)
    and [k, np] (mean, sd, unscaled); centres, centres_scaled [k, np]; scale [np].  source: how to reach the rows again
    (rows() needs them: the handle does not own them)."""

    def __init__(self, handle, result, table, centres, centres_scaled, scale, shape, source):
        self.h, self.result, self.table, self.centres, self.centres_scaled, self.scale = handle, result, table, centres, centres_scaled, scale
        self.nsteps, self.nc, self.ncol = shape
        self.k = result["k"]
        self._source = source

    def close(self):
        if self.h:
            load().mcx_modes_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def labels(self, first=0, n=None):
        """uint8 labels of source rows [first, first + n), row = step * nc + chain; MODE_NONE for a row that is not finite"""
        n = max(self.nsteps * self.nc - first, 0) if n is None else n
        out = np.empty(max(n, 0), np.uint8)
        check(load().mcx_modes_labels(self.h, first, n, out.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return out

    def chain_table(self):
        """mcx_modes_chain_table: dict of hops, dominant, dominant_steps, first_label, last_label [nc]; visits [nc, k]; trans [k, k];
        occupancy [nsteps, k], all integers"""
        chains = np.zeros(self.nc, MODE_CHAIN_DTYPE)
        visits, trans, occ = (np.zeros(s, np.int64) for s in ((self.nc, self.k), (self.k, self.k), (self.nsteps, self.k)))
        llp = lambda a: a.ctypes.data_as(C.POINTER(C.c_longlong))  # noqa: E731
        check(load().mcx_modes_chain_table(self.h, chains.ctypes.data_as(C.c_void_p), llp(visits), llp(trans), llp(occ)))
        out = {name: chains[name].copy() for name in MODE_CHAIN_DTYPE.names if name != "reserved"}
        out.update(visits=visits, trans=trans, occupancy=occ)
        return out

    def rows(self, k):
        """the rows of mode k in source order as a RowSet (its report is empty: nothing was clipped)"""
        h = C.c_void_p()
        check(self._source(self.h, int(k), C.byref(h)))
        nrows = C.c_longlong(0)
        check(load().mcx_rowset_shape(h, C.byref(nrows), None, None))
        rs = RowSet(h, np.zeros(self.ncol, CLIP_DTYPE), nrows.value, self.nsteps * self.nc)
        return rs

    def indicators(self):
        """mcx_modes_indicator_store: the DerivedStore of k columns of 1.0 / 0.0, log L = 0"""
        h = C.c_void_p()
        check(load().mcx_modes_indicator_store(self.h, C.byref(h)))
        return DerivedStore(h)

    def weights(self):
        """section 9's summary of the indicators, per mode: dict of mean (= the weight when every row is finite), sd, mcse_mean,
        rhat, ess [k]"""
        st = self.indicators()
        try:
            s = st.summary(probs=())
        finally:
            st.close()
        return {name: np.asarray(s[name])[:self.k].copy() for name in ("mean", "sd", "mcse_mean", "rhat", "ess")}


def _modes_call(fn, spec_and_centres, np_, shape, source):
    """fn(spec, res, table, cs, c, means, sds, scale, out) of one of the three modes entry points -> Modes"""
    spec, _keep = spec_and_centres
    k = min(max(int(spec.k), 1), MODES_MAX_K)  # (what the tables are sized for; a k outside is refused by the call)
    res, table, h = ModesResultC(), np.zeros(k, MODE_ROW_DTYPE), C.c_void_p()
    cs, c, means, sds = (np.zeros((k, np_)) for _ in range(4))
    scale = np.zeros(np_)
    check(fn(C.byref(spec), C.byref(res), table.ctypes.data_as(C.c_void_p), _dp(cs), _dp(c), _dp(means), _dp(sds), _dp(scale), C.byref(h)))
    result = {name: getattr(res, name) for name in ("k", "iters", "flags", "n", "n_nonfinite", "n_changed", "inertia")}
    tab = {name: table[name].copy() for name in MODE_ROW_DTYPE.names}
    tab.update(mean=means, sd=sds)
    return Modes(h, result, tab, c, cs, scale, shape, source)


def rows_modes(rows, nsteps, nc, k, **spec):
    """mcx_rows_modes: Engine.modes' Modes for rows [nsteps * nc, np + 1] on the host (MCout layout)"""
    rows = np.ascontiguousarray(rows, np.float32)
    np_ = rows.shape[1] - 1
    return _modes_call(lambda *a: load().mcx_rows_modes(_fp(rows), nsteps, nc, np_, *a), _modes_spec(k, np_, **spec), np_,
                       (nsteps, nc, np_ + 1), lambda *a: load().mcx_rows_mode_rows(_fp(rows), nsteps, nc, np_, *a))


def seed_modes(rows, k, seed=0, scale=None):
    """mcx_modes_seed (host only): the int64 indices of the k k-means++ seed rows of rows [M, np + 1]; scale: s [np], None = ones"""
    rows = np.ascontiguousarray(rows, np.float32)
    np_ = rows.shape[1] - 1
    s = np.ones(np_) if scale is None else np.ascontiguousarray(np.asarray(scale, np.float64).reshape(-1))
    if s.size != np_:
        raise ValueError("scale takes one entry per parameter (%d)" % np_)
    idx = np.zeros(max(int(k), 1), np.int64)
    check(load().mcx_modes_seed(_fp(rows), rows.shape[0], np_, int(k), int(seed) & 0xffffffff, _dp(s),
                                idx.ctypes.data_as(C.POINTER(C.c_longlong))))
    return idx


def debug_modes_assign(rows, nsteps, nc, centres_scaled, scale):
    """mcx_debug_modes_assign: one pass -> (labels [N] uint8, d2 [N], n [k] int64, S [k, np])"""
    rows = np.ascontiguousarray(rows, np.float32)
    np_ = rows.shape[1] - 1
    c = np.ascontiguousarray(np.asarray(centres_scaled, np.float64).reshape(-1, np_))
    s = np.ascontiguousarray(np.asarray(scale, np.float64).reshape(-1))
    if s.size != np_:
        raise ValueError("scale takes one entry per parameter (%d)" % np_)
    k, N = c.shape[0], nsteps * nc
    labels, d2, n, S = np.zeros(N, np.uint8), np.zeros(N), np.zeros(max(k, 1), np.int64), np.zeros((max(k, 1), np_))
    check(load().mcx_debug_modes_assign(_fp(rows), nsteps, nc, np_, k, _dp(c), _dp(s), labels.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                        _dp(d2), n.ctypes.data_as(C.POINTER(C.c_longlong)), _dp(S)))
    return labels, d2, n[:k], S[:k]


def debug_modes_geometry(np_, nsteps, nc, k):
    """mcx_debug_modes_geometry (host only): the launch geometry of a modes call as a dict of include/mcx.h's fields"""
    g = ModesGeometry()
    check(load().mcx_debug_modes_geometry(np_, nsteps, nc, k, C.byref(g)))
    return {name: int(getattr(g, name)) for name, _ in ModesGeometry._fields_}


# ---- evidence: log Z by bridge sampling ---------------------------------------------------------------------
class Proposal:
    """an mcx_evidence_mixture: weights [k], centres [k, np], covs [k, np, np] in float64 and a scale of the standard deviations"""

    def __init__(self, weights, centres, covs, scale=1.0):
        self.weights = np.ascontiguousarray(np.asarray(weights, np.float64).reshape(-1))
        self.k = self.weights.size
        self.centres = np.ascontiguousarray(np.asarray(centres, np.float64).reshape(self.k, -1))
        self.np = self.centres.shape[1]
        self.covs = np.ascontiguousarray(np.asarray(covs, np.float64).reshape(self.k, self.np, self.np))
        self.scale = float(scale)
        self.c = EvidenceMixtureC(self.k, 0, _dp(self.weights), _dp(self.centres), _dp(self.covs), self.scale)


def _evidence_spec(ndraw=0, seed=0, fit_steps=-1, use_neff=True, max_iter=1000, tol=1e-10, scale=1.0):
    return EvidenceSpecC(int(ndraw), int(seed) & 0xffffffff, int(fit_steps), 1 if use_neff else 0, int(max_iter), float(tol), float(scale))


def _evidence_dict(res):
    return {name: getattr(res, name) for name, _ in EvidenceResultC._fields_}


def _evidence_call(fn, vl, proposal, **spec):
    """fn(L, spec, proposal, res) of one of the evidence entry points -> the dict of mcx_evidence_result's fields"""
    res, sp = EvidenceResultC(), _evidence_spec(**spec)
    check(fn(None if vl is None else C.byref(vl), C.byref(sp), None if proposal is None else C.byref(proposal.c), C.byref(res)))
    return _evidence_dict(res)


def rows_evidence(rows, nsteps, nc, vl, proposal=None, **spec):
    """mcx_rows_evidence: Engine.evidence's dict for rows [nsteps * nc, np + 1] on the host (MCout layout) and the likelihood vl
    (make_vlfunc's struct) they were sampled from"""
    rows = np.ascontiguousarray(rows, np.float32)
    np_ = rows.shape[1] - 1
    return _evidence_call(lambda *a: load().mcx_rows_evidence(_fp(rows), nsteps, nc, np_, *a), vl, proposal, **spec)


def evidence_proposal(proposal):
    """mcx_evidence_proposal (host only): (C [k, np, np] lower Cholesky factors of scale^2 covs, W = their inverses, lc [k])"""
    k, np_ = min(max(proposal.k, 1), EVIDENCE_MAX_K), proposal.np
    Cf, W, lc = np.zeros((k, np_, np_)), np.zeros((k, np_, np_)), np.zeros(k)
    check(load().mcx_evidence_proposal(np_, C.byref(proposal.c), _dp(Cf), _dp(W), _dp(lc)))
    return Cf, W, lc


def evidence_iterate(l1, l2, neff=None, tol=1e-10, max_iter=1000):
    """mcx_evidence_iterate (host only): the bridge on host arrays l1 (rows) and l2 (draws; -inf = a draw with L = 0) -> the dict of
    mcx_evidence_result's fields (ess_f2 = n1: the host has no spectral estimate).  neff None: n1"""
    l1 = np.ascontiguousarray(np.asarray(l1, np.float64).reshape(-1))
    l2 = np.ascontiguousarray(np.asarray(l2, np.float64).reshape(-1))
    res = EvidenceResultC()
    check(load().mcx_evidence_iterate(_dp(l1), l1.size, _dp(l2), l2.size, float(l1.size if neff is None else neff), float(tol),
                                      int(max_iter), C.byref(res)))
    return _evidence_dict(res)


def proposal_from_modes(modes, scale=1.0, nc=1):
    """a k-component Proposal from a Modes (section 25): the weights and centres (the modes' means) of the mode table, each
    component's covariance from section 10 on the rows of that mode (modes.rows(k) as a store of nc pseudo-chains)"""
    k = modes.k
    np_ = modes.ncol - 1
    covs = np.zeros((k, np_, np_))
    for j in range(k):
        rs = modes.rows(j)
        try:
            st = rs.store(nc=nc)
            try:
                covs[j] = st.covariance()["cov"][:np_, :np_]
            finally:
                st.close()
        finally:
            rs.close()
    return Proposal(np.asarray(modes.table["weight"], np.float64), np.asarray(modes.table["mean"], np.float64), covs, scale)


def debug_evidence_logg(x, proposal):
    """mcx_debug_evidence_logg: log g of rows x [n, np] (parameters alone) by the sweep kernel -> lg [n] float64"""
    x = np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1, proposal.np))
    lg = np.zeros(x.shape[0])
    check(load().mcx_debug_evidence_logg(_fp(x), x.shape[0], proposal.np, C.byref(proposal.c), _dp(lg)))
    return lg


def debug_evidence_draws(proposal, ndraw, seed=0, vl=None):
    """mcx_debug_evidence_draws: (x [ndraw, np] float32, comp [ndraw] int32, lg [ndraw] float64, ll [ndraw] float32 or None)"""
    n = max(int(ndraw), 1)
    x, comp, lg = np.zeros((n, proposal.np), np.float32), np.zeros(n, np.int32), np.zeros(n)
    ll = None if vl is None else np.zeros(n, np.float32)
    check(load().mcx_debug_evidence_draws(proposal.np, C.byref(proposal.c), None if vl is None else C.byref(vl), int(seed) & 0xffffffff,
                                          int(ndraw), _fp(x), comp.ctypes.data_as(C.POINTER(C.c_int)), _dp(lg),
                                          None if ll is None else _fp(ll)))
    return x, comp, lg, ll


def debug_evidence_l(rows, nsteps, nc, vl, proposal=None, **spec):
    """mcx_debug_evidence_l: (rows_evidence's dict, l1 [N1], l2 [N2]) as the bridge passes read them"""
    rows = np.ascontiguousarray(rows, np.float32)
    np_ = rows.shape[1] - 1
    sp = _evidence_spec(**spec)
    fit = sp.fit_steps if sp.fit_steps >= 0 else (0 if proposal is not None else nsteps // 2)
    n1 = max((nsteps - fit) * nc, 1)
    n2 = sp.ndraw if sp.ndraw > 0 else min(n1, 1 << 20)
    l1, l2, res = np.zeros(n1), np.zeros(n2), EvidenceResultC()
    check(load().mcx_debug_evidence_l(_fp(rows), nsteps, nc, np_, C.byref(vl), C.byref(sp), None if proposal is None else C.byref(proposal.c),
                                      C.byref(res), _dp(l1), _dp(l2)))
    return _evidence_dict(res), l1, l2


def debug_evidence_geometry(np_, n1, n2, k=1):
    """mcx_debug_evidence_geometry (host only): the launch geometry of an evidence call as a dict of include/mcx.h's fields"""
    g = EvidenceGeometry()
    check(load().mcx_debug_evidence_geometry(np_, n1, n2, k, C.byref(g)))
    return {name: int(getattr(g, name)) for name, _ in EvidenceGeometry._fields_}


# ---- profile likelihoods (include/mcx.h) ----
def _ullp(a):
    return a.ctypes.data_as(C.POINTER(C.c_ulonglong))


def _llp(a):
    return a.ctypes.data_as(C.POINTER(C.c_longlong))


class ProfileSpec:
    """an mcx_profile_spec / mcx_profile2d_spec and the arrays it points to: n bins per column (g nodes per axis with pairs or
    two_d), clip = (qlo, qhi) quantiles as the range ((0, 1): min to max), from_ / to = None or [ncol] with NaN for a column's
    default, levels = confidence levels in (0, 1) (None: 0.6827 and 0.9545) or drops = drops of log L instead"""

    def __init__(self, n=64, clip=(0, 1), from_=None, to=None, levels=None, drops=None, pairs=None, two_d=False):
        arr = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1))  # noqa: E731
        ptr = lambda a: None if a is None else _dp(a)  # noqa: E731
        if levels is not None and drops is not None:
            raise ValueError("levels or drops, not both")
        self.n, self.from_, self.to = int(n), arr(from_), arr(to)
        self.lv = arr(drops if drops is not None else levels)
        nlv = 0 if self.lv is None else self.lv.size
        self.nlevels = nlv if nlv else 2
        head = (self.n, float(clip[0]), float(clip[1]), ptr(self.from_), ptr(self.to))
        tail = (nlv, ptr(self.lv) if nlv else None, int(drops is not None))
        if two_d or pairs is not None:
            self.pairs = None if pairs is None else np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
            self.c = Profile2dSpecC(*head, 0 if self.pairs is None else self.pairs.shape[0],
                                    None if self.pairs is None else self.pairs.ctypes.data_as(C.POINTER(C.c_int)), *tail)
        else:
            self.c = ProfileSpecC(*head, *tail)

    def fits(self, ncol):
        for a in (self.from_, self.to):
            if a is not None and a.size != ncol:
                raise ValueError("from_ and to take one entry per profiled column (%d), NaN for a column's default" % ncol)
        return self

    def npairs(self, ncol):
        return ncol * (ncol - 1) // 2 if self.pairs is None else self.pairs.shape[0]


def _profile_call(fn, spec, ncol, path):
    """fn(spec, cols, cnt, lmax, row, xat, pl, plh, intervals, path) of one of the three profile entry points -> a dict: the
    fields of mcx_col_profile as arrays [ncol] (from, to, lhat, xhat, row_hat, nvalues, nbinned, ndropped, nempty, flags); cnt,
    lmax, row, xat, pl, plh [ncol, n]; intervals [ncol, L] of PROFILE_INTERVAL_DTYPE; path [ncol, n, ncol + 1] when asked"""
    n = min(max(spec.n, 1), 512)  # (a refused n still gets buffers)
    nl = min(spec.nlevels, PROFILE_MAX_LEVELS)
    cols = np.zeros(ncol, COL_PROFILE_DTYPE)
    cnt, lmax, row, xat = np.zeros((ncol, n), np.uint64), np.zeros((ncol, n), np.float32), np.zeros((ncol, n), np.int64), np.zeros((ncol, n), np.float32)
    pl, plh, iv = np.zeros((ncol, n)), np.zeros((ncol, n)), np.zeros((ncol, nl), PROFILE_INTERVAL_DTYPE)
    pa = np.zeros((ncol, n, ncol + 1), np.float32) if path else None
    check(fn(C.byref(spec.c), cols.ctypes.data_as(C.c_void_p), _ullp(cnt), _fp(lmax), _llp(row), _fp(xat), _dp(pl), _dp(plh),
             iv.ctypes.data_as(C.c_void_p), None if pa is None else _fp(pa)))
    out = {name: cols[name].copy() for name in COL_PROFILE_DTYPE.names}
    out.update(cnt=cnt, lmax=lmax, row=row, xat=xat, pl=pl, plh=plh, intervals=iv)
    if path:
        out["path"] = pa
    return out


def _profile2d_call(fn, spec, ncol):
    """fn(spec, cols, pairs_out, cnt, lmax, row, xat_a, xat_b, z, nlevel) -> a dict: from, to, lhat, xhat, row_hat, nvalues and
    col_flags [ncol]; pairs [npairs, 2], nbinned, nempty, flags [npairs]; cnt, lmax, row, xat_a, xat_b, z [npairs, g, g], cell
    (ia, ib) of the pair's two grids; drops [L], nlevel [npairs, L]"""
    g = min(max(spec.n, 1), 64)  # (a refused g or list of pairs still gets buffers)
    npairs = min(max(spec.npairs(ncol), 1), 1024)
    nl = min(spec.nlevels, PROFILE_MAX_LEVELS)
    cols, po = np.zeros(ncol, COL_PROFILE_DTYPE), np.zeros(npairs, PAIR_PROFILE_DTYPE)
    sh = (npairs, g, g)
    cnt, lmax, row = np.zeros(sh, np.uint64), np.zeros(sh, np.float32), np.zeros(sh, np.int64)
    xa, xb, z, nlev = np.zeros(sh, np.float32), np.zeros(sh, np.float32), np.zeros(sh), np.zeros((npairs, nl), np.int64)
    check(fn(C.byref(spec.c), cols.ctypes.data_as(C.c_void_p), po.ctypes.data_as(C.c_void_p), _ullp(cnt), _fp(lmax), _llp(row), _fp(xa),
             _fp(xb), _dp(z), _llp(nlev)))
    out = {name: cols[name].copy() for name in ("from", "to", "lhat", "xhat", "row_hat", "nvalues")}
    out["col_flags"] = cols["flags"].copy()
    out["pairs"] = np.stack([po["a"], po["b"]], axis=1)
    out["nbinned"], out["nempty"], out["flags"] = po["nbinned"].copy(), po["nempty"].copy(), po["flags"].copy()
    out.update(cnt=cnt, lmax=lmax, row=row, xat_a=xa, xat_b=xb, z=z, nlevel=nlev)
    return out


def rows_profile(rows, nsteps, nc, n=64, levels=None, drops=None, clip=(0, 1), from_=None, to=None, path=False):
    """mcx_rows_profile: Engine.profile_likelihood's dict for rows [nsteps * nc, np + 1] on the host (MCout layout)"""
    rows = np.ascontiguousarray(rows, np.float32)
    ncol = rows.shape[1] - 1
    spec = ProfileSpec(n, clip, from_, to, levels, drops).fits(ncol)
    return _profile_call(lambda *a: load().mcx_rows_profile(_fp(rows), nsteps, nc, ncol, *a), spec, ncol, path)


def rows_profile2d(rows, nsteps, nc, g=32, pairs=None, levels=None, drops=None, clip=(0, 1), from_=None, to=None):
    """mcx_rows_profile2d: Engine.profile_likelihood2d's dict for rows [nsteps * nc, np + 1] on the host (MCout layout)"""
    rows = np.ascontiguousarray(rows, np.float32)
    ncol = rows.shape[1] - 1
    spec = ProfileSpec(g, clip, from_, to, levels, drops, pairs, two_d=True).fits(ncol)
    return _profile2d_call(lambda *a: load().mcx_rows_profile2d(_fp(rows), nsteps, nc, ncol, *a), spec, ncol)


def profile_interval(x, y, drop):
    """mcx_profile_interval (host only): the outermost interval of the curve y at y >= -drop over the points x (ascending; NaN
    for an empty bin) -> (lo, hi, nseg, flags)"""
    x = np.ascontiguousarray(np.asarray(x, np.float64).reshape(-1))
    y = np.ascontiguousarray(np.asarray(y, np.float64).reshape(-1))
    if x.size != y.size:
        raise ValueError("x and y take one entry per bin")
    lo, hi, nseg, flags = C.c_double(0), C.c_double(0), C.c_int(0), C.c_int(0)
    check(load().mcx_profile_interval(x.size, _dp(x), _dp(y), float(drop), C.byref(lo), C.byref(hi), C.byref(nseg), C.byref(flags)))
    return lo.value, hi.value, nseg.value, flags.value


def profile_drop(p, nparams=1):
    """mcx_profile_drop (host only): the drop of log L of confidence level p for one parameter or a pair"""
    d = C.c_double(0)
    check(load().mcx_profile_drop(float(p), nparams, C.byref(d)))
    return d.value


def debug_profile_finish(keys, cnt, xat, hat, levels=None, drops=None):
    """mcx_debug_profile_finish (host only): one column from its swept keys [n], counts [n], values at the keys [n] and the
    maximum key of all rows -> a dict: lmax, row, pl, plh [n], intervals [L], nbinned, nempty, flags"""
    keys, cnt = np.ascontiguousarray(keys, np.uint64), np.ascontiguousarray(cnt, np.uint64)
    xat = np.ascontiguousarray(xat, np.float32)
    n = keys.size
    spec = ProfileSpec(2, levels=levels, drops=drops)
    lmax, row, pl, plh = np.zeros(n, np.float32), np.zeros(n, np.int64), np.zeros(n), np.zeros(n)
    iv = np.zeros(min(spec.nlevels, PROFILE_MAX_LEVELS), PROFILE_INTERVAL_DTYPE)
    nb, ne, fl = C.c_longlong(0), C.c_int(0), C.c_int(0)
    check(load().mcx_debug_profile_finish(n, _ullp(keys), _ullp(cnt), _fp(xat), int(hat), spec.c.nlevels, spec.c.levels, spec.c.levels_are_drops,
                                          _fp(lmax), _llp(row), _dp(pl), _dp(plh), iv.ctypes.data_as(C.c_void_p), C.byref(nb), C.byref(ne),
                                          C.byref(fl)))
    return dict(lmax=lmax, row=row, pl=pl, plh=plh, intervals=iv, nbinned=nb.value, nempty=ne.value, flags=fl.value)


def debug_rows_profile_bins(rows, nsteps, nc, n, from_, to):
    """mcx_debug_rows_profile_bins: the sweep alone over rows [nsteps * nc, np + 1] on the grids from_ [np] <= to [np] -> (keys
    [np, n] uint64, cnt [np, n] uint64, the maximum key of all rows)"""
    rows = np.ascontiguousarray(rows, np.float32)
    ncol = rows.shape[1] - 1
    from_ = np.ascontiguousarray(np.asarray(from_, np.float64).reshape(-1))
    to = np.ascontiguousarray(np.asarray(to, np.float64).reshape(-1))
    if from_.size != ncol or to.size != ncol:
        raise ValueError("from_ and to take one entry per parameter")
    keys, cnt, hat = np.zeros((ncol, max(n, 1)), np.uint64), np.zeros((ncol, max(n, 1)), np.uint64), np.zeros(1, np.uint64)
    check(load().mcx_debug_rows_profile_bins(_fp(rows), nsteps, nc, ncol, n, _dp(from_), _dp(to), _ullp(keys), _ullp(cnt), _ullp(hat)))
    return keys, cnt, int(hat[0])


def debug_profile_geometry(np_, nsteps, nc, n=64, g=32, npairs=1):
    """mcx_debug_profile_geometry (host only): the launch geometry of the sweeps of a profile and a pair profile call"""
    geo = ProfileGeometry()
    check(load().mcx_debug_profile_geometry(np_, nsteps, nc, n, g, npairs, C.byref(geo)))
    return {name: int(getattr(geo, name)) for name, _ in ProfileGeometry._fields_}


def debug_reweight_geometry(N, ncol, nprobs=3, K=0):
    """mcx_debug_reweight_geometry (host only): the launch geometry of a reweight of N rows of ncol columns with nprobs
    probabilities and of a resample of K draws, as a dict of include/mcx.h's fields"""
    g = ReweightGeometry()
    check(load().mcx_debug_reweight_geometry(N, ncol, nprobs, K, C.byref(g)))
    return {name: int(getattr(g, name)) for name, _ in ReweightGeometry._fields_}


def debug_reweight_store_geometry(nsteps, nc, ncol, nprobs=3, K=0):
    """mcx_debug_reweight_store_geometry (host only): debug_reweight_geometry of nsteps * nc rows, with hist_step_chunks, which
    depends on the steps"""
    g = ReweightGeometry()
    check(load().mcx_debug_reweight_store_geometry(nsteps, nc, ncol, nprobs, K, C.byref(g)))
    return {name: int(getattr(g, name)) for name, _ in ReweightGeometry._fields_}


def debug_store_geometry(np_, nout, nsteps, nc):
    """mcx_debug_store_geometry (host only): the launch geometry of the derive, clip, rank and gather code for a store of
    nsteps steps of nc chains of np_ parameters and nout derived outputs (0: none), as a dict of include/mcx.h's fields"""
    g = StoreGeometry()
    check(load().mcx_debug_store_geometry(np_, nout, nsteps, nc, C.byref(g)))
    return {name: int(getattr(g, name)) for name, _ in StoreGeometry._fields_}


def debug_fill_allocations(byte=-1):
    """mcx_debug_fill_allocations (host only): from now on every device allocation the library makes is filled with byte
    (0..255; -1: off, the default) before it is used.  Returns the allocations filled under the setting this call ends."""
    n = C.c_ulonglong(0)
    check(load().mcx_debug_fill_allocations(byte, C.byref(n)))
    return int(n.value)


def debug_fill_scratch(owner, byte):
    """mcx_debug_fill_scratch: the analyses' three scratch buffers of an Engine or a DerivedStore filled with byte (0..255) to
    their present capacity; returns the bytes filled per buffer (doubles, 64-bit words, 32-bit words; 0: not allocated yet)"""
    out = (C.c_size_t * 3)()
    e, s = (owner.h, None) if isinstance(owner, Engine) else (None, owner.h)
    check(load().mcx_debug_fill_scratch(e, s, byte, out))
    return tuple(int(v) for v in out)


def debug_live_resources():
    """mcx_debug_live_resources (needs no GPU): (device allocations, pinned allocations, streams, events) the library holds now"""
    out = (C.c_uint64 * 4)()
    check(load().mcx_debug_live_resources(out))
    return tuple(int(v) for v in out)


def debug_draw_indices(seed, N, first, n):
    """mcx_debug_draw_indices (host only): the rows of draws first .. first + n - 1 among N rows, int64"""
    out = np.empty(max(n, 0), np.int64)
    check(load().mcx_debug_draw_indices(seed, N, first, n, out.ctypes.data_as(C.POINTER(C.c_int64))))
    return out


def debug_derive_compile(text, np_, nout):
    """mcx_debug_derive_compile (needs no GPU): bytes of the code object of a derive text for rows of np_ parameters"""
    nb = C.c_size_t(0)
    check(load().mcx_debug_derive_compile(text.encode() if isinstance(text, str) else text, np_, nout, C.byref(nb)))
    return nb.value


def proposal_from_cov(cov, np_, scale=None):
    """mcx_proposal_from_cov (host only): the np_ x np_ parameter block of cov (any leading dimension >= np_) times scale
    (None: 2.38^2 / np_), rounded to float32 and exactly symmetric -- the incov of Engine.run.  McxError when an entry is
    not finite or the float Cholesky of mcx_covar_setup rejects the matrix."""
    cov = np.ascontiguousarray(cov, np.float64)
    if cov.ndim != 2 or cov.shape[0] < np_ or cov.shape[1] < np_:
        raise ValueError("cov must be a matrix of at least np_ x np_ entries")
    out = np.zeros((np_, np_), np.float32)
    check(load().mcx_proposal_from_cov(np_, _dp(cov), cov.shape[1], 0.0 if scale is None else float(scale), _fp(out)))
    return out


def debug_summary_finish(n, M, mean, var_all, var_means, acov, ostat, N, probs=(), flags=0):
    """mcx_debug_summary_finish for one column: (record of SUMMARY_DTYPE, quantiles, lags still needed)"""
    a = np.ascontiguousarray(acov, np.float64)
    o = np.ascontiguousarray(ostat, np.float32)
    p, pp = _probs(probs)
    col = np.zeros(1, SUMMARY_DTYPE)
    q = np.zeros(max(len(p), 1), np.float64)
    need = C.c_int(0)
    check(load().mcx_debug_summary_finish(n, M, mean, var_all, var_means, a.ctypes.data_as(C.POINTER(C.c_double)), len(a),
                                          _fp(o), N, pp, len(p), flags, col.ctypes.data_as(C.c_void_p),
                                          q.ctypes.data_as(C.POINTER(C.c_double)), C.byref(need)))
    return col[0], q[:len(p)], need.value


def debug_select_step(hist, rem):
    """mcx_debug_select_step (host only): one digit of the summary's radix select -- (digit, rank within its bucket) of the
    target of rank rem among the keys that hist [256] counts by their next 8 bits"""
    h = np.ascontiguousarray(hist, np.uint64)
    if h.shape != (256,):
        raise ValueError("hist must hold 256 counts")
    digit, out = C.c_int(0), C.c_longlong(0)
    check(load().mcx_debug_select_step(h.ctypes.data_as(C.POINTER(C.c_ulonglong)), int(rem), C.byref(digit), C.byref(out)))
    return digit.value, out.value


def device_count():
    n = C.c_int(0)
    check(load().mcx_device_count(C.byref(n)))
    return n.value


def rccl_available():
    return bool(load().mcx_rccl_available())


def rccl_unique_id():
    """ncclGetUniqueId: call on one rank, ship the 128 bytes to every rank, pass them to Engine.rccl_init"""
    buf = C.create_string_buffer(128)
    check(load().mcx_rccl_unique_id(buf))
    return buf.raw


def device_info():
    name = C.create_string_buffer(256)
    cu = C.c_int(0)
    mem = C.c_size_t(0)
    check(load().mcx_device_info(name, 256, C.byref(cu), C.byref(mem)))
    return name.value.decode(), cu.value, mem.value


def debug_numerics(what, words):
    w = np.ascontiguousarray(words, dtype=np.uint32)
    out = np.empty_like(w)
    u32p = C.POINTER(C.c_uint32)
    check(load().mcx_debug_numerics(what, w.size, w.ctypes.data_as(u32p), out.ctypes.data_as(u32p)))
    return out


def debug_murray_screen(x, musig, own0=0, sums=True):
    """the per-pair screen of the Murray sweeps alone (mcx_screen.hpp): masks[(N + 63) // 64, (n + 127) // 128] uint64 for
    chains x[n, d] (groups of 128, in this order) against Gaussians musig[N, d, 2] = (mu, sig2)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    musig = np.ascontiguousarray(musig, dtype=np.float32)
    n, d = x.shape
    N = musig.shape[0]
    masks = np.zeros(((N + 63) // 64, (n + 127) // 128), np.uint64)
    check(load().mcx_debug_murray_screen(d, n, N, _fp(x), _fp(musig), int(own0), int(bool(sums)),
                                         masks.ctypes.data_as(C.POINTER(C.c_uint64))))
    return masks


def murray_decode(words, it, multi, cull_can, nact_before, N):
    """what the counter block of one kernel turn of a Murray step says (mcx_debug_murray_decode; host logic only, needs no
    GPU): (survivors, passes the turn stood for, pairs those passes swept, pairs kept by the min-arg screen, by the sum
    screens) from words[>= 132] uint64 as include/mcx.h lays them out"""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    out = np.zeros(5, np.uint64)
    u64p = C.POINTER(C.c_uint64)
    check(load().mcx_debug_murray_decode(w.ctypes.data_as(u64p), w.size, it, int(bool(multi)), int(bool(cull_can)), nact_before, N,
                                         out.ctypes.data_as(u64p)))
    return tuple(int(v) for v in out)


def debug_normals(seed, stream, t, g0, a, q, n):
    out = np.empty((n, 4), np.float32)
    check(load().mcx_debug_normals(seed, stream, t, g0, a, q, n, _fp(out)))
    return out


class Engine:
    """MCPar(np, nc, mpisiz, mpirank, pl, armin, armax, dfac, ifac, sync) -- src/mcpar.hh:32-33 --
    with shards in place of MPI ranks."""

    def __init__(self, np_, nc, nshards=1, shard=0, pl=0.9, armin=0.2, armax=0.5, dfac=0.2,
                 ifac=1.5, sync=10, seed=8675309):
        self.np, self.nc, self.nshards, self.shard = np_, nc, nshards, shard
        self.h = C.c_void_p()
        self._keep = []
        check(load().mcx_create(C.byref(self.h), np_, nc, nshards, shard, pl, armin, armax, dfac,
                                ifac, sync, seed))
        self.nburn = self.nsamp = 0

    def close(self):
        if self.h:
            load().mcx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, opt, value):
        check(load().mcx_set_option(self.h, opt, int(value)))

    def set_exchange(self, pyfn):
        """pyfn(phase, musigall_dev_ptr, slot_floats, shard, nshards, stream_ptr) -> 0 on success"""
        def tramp(ctx, phase, ptr, slot, shard, nshards, stream):
            try:
                return int(pyfn(phase, ptr, slot, shard, nshards, stream) or 0)
            except Exception:  # never unwind through C
                import traceback
                traceback.print_exc()
                return 1
        cb = XCHGFN(tramp)
        self._keep.append(cb)
        check(load().mcx_set_exchange(self.h, cb, None))

    def rccl_init(self, unique_id):
        """install the library's own exchange: in-place ncclAllGather over the nshards engines (collective)"""
        assert len(unique_id) == 128
        self._keep.append(unique_id)
        check(load().mcx_exchange_rccl_init(self.h, C.c_char_p(unique_id)))

    def rccl_init_raw(self, ptr):
        check(load().mcx_exchange_rccl_init(self.h, ptr))

    def rccl_info(self):
        """(ncclCommCount, ncclCommUserRank) of the installed RCCL exchange"""
        nr, rk = C.c_int(0), C.c_int(0)
        check(load().mcx_exchange_rccl_info(self.h, C.byref(nr), C.byref(rk)))
        return nr.value, rk.value

    def rccl_destroy(self):
        check(load().mcx_exchange_rccl_destroy(self.h))

    def debug_exchange(self):
        check(load().mcx_debug_exchange(self.h))

    def synchronize(self):
        """wait for what the last run() left in flight (MCX_OPT_ASYNC_TAIL: a sharded run's last all-gather)"""
        check(load().mcx_synchronize(self.h))

    def exchange_self_check(self):
        """every shard fills its slot with shard + 1, one exchange, then slot r must be full of r + 1 on every
        shard: True / False.  Collective over the shards (each calls it)."""
        check(load().mcx_debug_fill_slot(self.h, float(self.shard + 1)))
        self.debug_exchange()
        ms = self.musigall.reshape(self.nshards, -1)
        ok = bool(all(np.all(ms[r] == np.float32(r + 1)) for r in range(self.nshards)))
        check(load().mcx_debug_fill_slot(self.h, 0.0))  # leave the slots as a fresh engine has them
        self.debug_exchange()
        return ok

    def set_output_hook(self, pyfn):
        def tramp(ctx, steps_done):
            try:
                return int(pyfn(steps_done) or 0)
            except Exception:
                import traceback
                traceback.print_exc()
                return 1
        cb = OUTFN(tramp)
        self._keep.append(cb)
        check(load().mcx_set_output_hook(self.h, cb, None))

    def set_sink(self, pyfn, block_steps):
        """pyfn(first_step, nsteps, rows[nsteps*nc, np+1]) -> 0; rows is a view of pinned memory valid during the call.
        pyfn = None removes the sink."""
        if pyfn is None:
            check(load().mcx_set_sink(self.h, SINKFN(), None, 0))
            return
        nc, ncol = self.nc, self.np + 1

        def tramp(ctx, first, nsteps, rows):
            try:
                view = np.ctypeslib.as_array(rows, shape=(nsteps * nc, ncol))
                return int(pyfn(first, nsteps, view) or 0)
            except Exception:
                import traceback
                traceback.print_exc()
                return 1
        cb = SINKFN(tramp)
        self._keep.append(cb)
        check(load().mcx_set_sink(self.h, cb, None, int(block_steps)))

    def sink_text(self):
        """inside a row sink's callback of a run with OPT_SINK_TEXT: the block's rows as text (bytes)"""
        ptr, nb = C.c_void_p(0), C.c_size_t(0)
        check(load().mcx_sink_text(self.h, C.byref(ptr), C.byref(nb)))
        return C.string_at(ptr.value, nb.value) if nb.value else b""

    def set_text_sink(self, pyfn, block_steps):
        """pyfn(first_step, nsteps, text: bytes-like memoryview) -> 0: every block as the text MCout::output prints for it
        (src/mcout.cc:41-45), formatted on the device.  pyfn = None removes the sink."""
        if pyfn is None:
            check(load().mcx_set_text_sink(self.h, TEXTSINKFN(), None, 0))
            return

        def tramp(ctx, first, nsteps, text, nbytes):
            try:
                view = (C.c_char * nbytes).from_address(text) if nbytes else b""
                return int(pyfn(first, nsteps, memoryview(view)) or 0)
            except Exception:
                import traceback
                traceback.print_exc()
                return 1
        cb = TEXTSINKFN(tramp)
        self._keep.append(cb)
        check(load().mcx_set_text_sink(self.h, cb, None, int(block_steps)))

    def stage_pinit(self, pinit):
        """put the initial chain state in HBM ahead of time; run(..., pinit=None, ...) starts from it"""
        pinit = np.ascontiguousarray(pinit, dtype=np.float32).reshape(-1)
        if pinit.size != self.np * self.nc:
            raise ValueError("pinit must have nc*np elements")
        check(load().mcx_stage_pinit(self.h, _fp(pinit)))

    def run(self, nsamp, nburn, pinit, vl, incov=None):
        """MCPar::run(nsamp, nburn, pinit, L, outsamples, incov) -- src/mcpar.hh:36-37"""
        if pinit is not None:
            pinit = np.ascontiguousarray(pinit, dtype=np.float32).reshape(-1)
            if pinit.size != self.np * self.nc:
                raise ValueError("pinit must have nc*np elements")
        ic = None if incov is None else np.ascontiguousarray(incov, dtype=np.float32)
        check(load().mcx_run(self.h, nsamp, nburn, _fp(pinit) if pinit is not None else None, C.byref(vl),
                             _fp(ic) if ic is not None else None))
        self.nburn, self.nsamp = nburn, nsamp

    def gen_local(self, t, pvals):
        pv = np.ascontiguousarray(pvals, np.float32)
        pt = np.empty_like(pv)
        cf = np.empty(self.nc, np.float32)
        check(load().mcx_gen_local(self.h, t, _fp(pv), _fp(pt), _fp(cf)))
        return pt, cf

    def gen_remote(self, t, pvals, musigall):
        pv = np.ascontiguousarray(pvals, np.float32)
        ms = np.ascontiguousarray(musigall, np.float32)
        pt, mt, sg = np.empty_like(pv), np.empty_like(pv), np.empty_like(pv)
        cf = np.empty(self.nc, np.float32)
        npass = C.c_int(0)
        check(load().mcx_gen_remote(self.h, t, _fp(pv), _fp(ms), _fp(pt), _fp(cf), _fp(mt), _fp(sg),
                                    C.byref(npass)))
        return pt, cf, mt, sg, npass.value

    def covar_setup(self, incov=None):
        out = np.empty((self.np, self.np), np.float32)
        ic = None if incov is None else np.ascontiguousarray(incov, np.float32)
        check(load().mcx_covar_setup(self.h, _fp(ic) if ic is not None else None, _fp(out)))
        return out

    @property
    def state(self): return self._getf("mcx_get_state", (self.nc, self.np))
    @property
    def loglike(self): return self._getf("mcx_get_loglike", (self.nc,))
    @property
    def mean(self): return self._getf("mcx_get_mean", (self.nc, self.np))
    @property
    def var(self): return self._getf("mcx_get_var", (self.nc, self.np))
    @property
    def musigall(self): return self._getf("mcx_get_musigall", (self.nshards * self.nc, self.np, 2))
    @property
    def chol(self): return self._getf("mcx_get_chol", (self.np, self.np))

    def _getf(self, name, shape):
        out = np.empty(shape, np.float32)
        check(getattr(load(), name)(self.h, _fp(out)))
        return out

    @property
    def accept_counts(self):
        out = np.empty(self.nc, np.uint32)
        check(load().mcx_get_accept_counts(self.h, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    @property
    def accept_mask(self):
        out = np.empty((self.nburn + self.nsamp, self.nc), np.uint8)
        check(load().mcx_get_accept_mask(self.h, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    @property
    def counters(self):
        c = Counters()
        check(load().mcx_get_counters(self.h, C.byref(c)))
        return {n: int(getattr(c, n)) for n, _ in Counters._fields_}

    @property
    def step_instances(self):
        """the distinct step-kernel instances launched since the last run() began, in order of first launch
        (mcx_debug_step_instances): StepInstance records"""
        return _step_ids(lambda ids, cap, n: load().mcx_debug_step_instances(self.h, ids, cap, n))

    @property
    def tuner_trace(self):
        buf = np.zeros(256, np.float32)
        n = C.c_int(0)
        check(load().mcx_get_tuner_trace(self.h, _fp(buf), 256, C.byref(n)))
        return buf[:min(n.value, 256)].copy()

    @property
    def samples(self):
        """MCout rows (np+1 columns), step-major then chain (src/mcout.cc:129-145)"""
        ns = C.c_int(0)
        check(load().mcx_samples_steps(self.h, C.byref(ns)))
        out = np.empty((ns.value * self.nc, self.np + 1), np.float32)
        if ns.value:
            check(load().mcx_samples_copy(self.h, 0, ns.value, _fp(out)))
        return out

    def samples_into(self, out, first_step=0, nsteps=None):
        """copy sample rows into a caller-owned float32 array of (nsteps*nc, np+1) elements"""
        if nsteps is None:
            ns = C.c_int(0)
            check(load().mcx_samples_steps(self.h, C.byref(ns)))
            nsteps = ns.value - first_step
        if out.dtype != np.float32 or not out.flags.c_contiguous or out.size < nsteps * self.nc * (self.np + 1):
            raise ValueError("out must be a C-contiguous float32 array of nsteps*nc*(np+1) elements")
        if nsteps:
            check(load().mcx_samples_copy(self.h, first_step, nsteps, _fp(out)))
        return nsteps

    def samples_range(self, first_step, nsteps):
        out = np.empty((nsteps * self.nc, self.np + 1), np.float32)
        if nsteps:
            check(load().mcx_samples_copy(self.h, first_step, nsteps, _fp(out)))
        return out

    def samples_text(self, first_step, nsteps):
        """the rows of samples_range(first_step, nsteps) as the bytes MCout::output prints for them (src/mcout.cc:41-45),
        formatted on the device"""
        nb = C.c_size_t(0)
        check(load().mcx_samples_text(self.h, first_step, nsteps, None, 0, C.byref(nb)))
        buf = C.create_string_buffer(max(nb.value, 1))
        check(load().mcx_samples_text(self.h, first_step, nsteps, buf, nb.value, C.byref(nb)))
        return buf.raw[:nb.value]

    def samples_text_into(self, first_step, nsteps, buf):
        """the same into a caller's uint8 array (None: the size only); returns the number of bytes"""
        nb = C.c_size_t(0)
        if buf is None:
            check(load().mcx_samples_text(self.h, first_step, nsteps, None, 0, C.byref(nb)))
        else:
            check(load().mcx_samples_text(self.h, first_step, nsteps, buf.ctypes.data_as(C.c_char_p), buf.size, C.byref(nb)))
        return nb.value

    def _on_store(self, fn, first_step, nsteps, *args):
        """fn(engine, first_step, nsteps, *args) of kept steps [first_step, first_step + nsteps) -- nsteps None: to the
        end of the store --; McxError with mcx_last_error's text on a status other than 0"""
        if nsteps is None:
            ns = C.c_int(0)
            check(load().mcx_samples_steps(self.h, C.byref(ns)))
            nsteps = ns.value - first_step
        check(fn(self.h, first_step, nsteps, *args))

    def summary(self, probs=(0.01, 0.5, 0.99), first_step=0, nsteps=None):
        """mcx_samples_summary: per column (the parameters, then log L) of kept steps [first_step, first_step + nsteps)
        -- a dict of arrays [np + 1]: mean, sd, min, max, rhat, ess, mcse_mean, ess_lag, flags; quantiles [np + 1, nprobs]"""
        p, pp = _probs(probs)
        cols = np.zeros(self.np + 1, SUMMARY_DTYPE)
        q = np.zeros((self.np + 1, len(p)), np.float64)
        self._on_store(load().mcx_samples_summary, first_step, nsteps, pp, len(p), cols.ctypes.data_as(C.c_void_p),
                       q.ctypes.data_as(C.POINTER(C.c_double)))
        return _summary_dict(cols, q)

    def rank_summary(self, first_step=0, nsteps=None):
        """mcx_samples_rank_summary: per column (the parameters, then log L) of kept steps [first_step, first_step + nsteps)
        -- a dict of arrays [np + 1]: rhat, rhat_bulk, rhat_folded, ess_bulk, ess_tail, ess_q05, ess_q95, q05, median, q95,
        ess_bulk_lag, flags"""
        cols = np.zeros(self.np + 1, RANK_SUMMARY_DTYPE)
        self._on_store(load().mcx_samples_rank_summary, first_step, nsteps, cols.ctypes.data_as(C.c_void_p))
        return _rank_summary_dict(cols)

    def rank_summary_times(self, first_step=0, nsteps=None):
        """mcx_debug_rank_summary_times: the 20 stage times of one rank_summary() call in ms (include/mcx.h lists them)"""
        ms = np.zeros(20)
        self._on_store(load().mcx_debug_rank_summary_times, first_step, nsteps, _dp(ms))
        return ms

    def covariance(self, first_step=0, nsteps=None):
        """mcx_samples_covariance of kept steps [first_step, first_step + nsteps): a dict of mean [np + 1] (summary()'s,
        bit for bit), cov and corr [np + 1, np + 1] (the parameters, then log L) and flags [np + 1]"""
        ncol = self.np + 1
        mean, cov, flags = np.zeros(ncol), np.zeros((ncol, ncol)), np.zeros(ncol, np.int32)
        self._on_store(load().mcx_samples_covariance, first_step, nsteps, _dp(mean), _dp(cov),
                       flags.ctypes.data_as(C.POINTER(C.c_int)))
        return _covariance_dict(mean, cov, flags)

    def covariance_times(self, first_step=0, nsteps=None):
        """mcx_debug_covariance_times: ms of (the column-sum sweep, the covariance sweep, the partials' reducer) of one call"""
        ms = np.zeros(3)
        self._on_store(load().mcx_debug_covariance_times, first_step, nsteps, _dp(ms))
        return ms

    def density(self, n=512, adjust=1.0, clip=(0, 1), bw=None, from_=None, to=None, first_step=0, nsteps=None):
        """mcx_samples_density: per column (the parameters, then log L) of kept steps [first_step, first_step + nsteps) the
        kernel density estimate of R's density() / geom_density -- a dict of arrays [np + 1]: bw, from, to, lo, up, mean, sd,
        nvalues, nbinned, flags; x and y [np + 1, n], the points and the density at them"""
        spec = DensitySpec(n, adjust, clip, bw, from_, to).fits(self.np + 1)
        cols, x, y = _density_out(self.np + 1, n)
        self._on_store(load().mcx_samples_density, first_step, nsteps, C.byref(spec.c), cols.ctypes.data_as(C.c_void_p), _dp(x), _dp(y))
        return _density_dict(cols, x, y)

    def density_times(self, n=512, adjust=1.0, clip=(0, 1), first_step=0, nsteps=None):
        """mcx_debug_density_times: ms of (the statistics passes, the binning sweep, the host grid and finish, the whole call)
        of one density() call"""
        spec = DensitySpec(n, adjust, clip)
        ms = np.zeros(4)
        self._on_store(load().mcx_debug_density_times, first_step, nsteps, C.byref(spec.c), _dp(ms))
        return ms

    def density2d(self, g=64, pairs=None, adjust=1.0, clip=(0, 1), bw=None, from_=None, to=None, first_step=0, nsteps=None):
        """mcx_samples_density2d, the corner plot: per pair of columns (pairs [npairs, 2]; None: every a < b) of kept steps
        [first_step, first_step + nsteps) the joint kernel density estimate of MASS::kde2d / geom_density_2d on g x g nodes --
        a dict of the column arrays [np + 1] bw, from, to, lo, up, mean, sd, nvalues, col_flags; axes [np + 1, g]; pairs
        [npairs, 2], nbinned and flags [npairs]; z [npairs, g, g], z[p, j, k] the density at (axes[a, j], axes[b, k])"""
        spec = Density2dSpec(g, pairs, adjust, clip, bw, from_, to).fits(self.np + 1)
        return _density2d_call(lambda *a: self._on_store(load().mcx_samples_density2d, first_step, nsteps, *a) or 0, spec,
                               self.np + 1)

    def density2d_times(self, g=64, pairs=None, adjust=1.0, clip=(0, 1), first_step=0, nsteps=None):
        """mcx_debug_density2d_times: ms of (the statistics passes, k_density2d_codes, k_density2d_pairs, k_density2d_reduce,
        the host grids and finish, the whole call) of one density2d() call"""
        spec = Density2dSpec(g, pairs, adjust, clip)
        ms = np.zeros(6)
        self._on_store(load().mcx_debug_density2d_times, first_step, nsteps, C.byref(spec.c), _dp(ms))
        return ms

    def clip(self, qlo=0.01, qhi=0.99, ll_hi=0.0, lo=None, hi=None, first_step=0, nsteps=None, count_only=False):
        """mcx_samples_clip, the reference's mcparam.clip.tails: the RowSet of the rows of kept steps [first_step, first_step
        + nsteps) that lie strictly between the thresholds of every column (the parameters, then log L) -- by default a
        column's (qlo, qhi) quantiles, summary()'s numbers, and ll_hi as the upper threshold of log L; lo / hi [np + 1]
        replace them where not NaN.  count_only: the report and the count, no rows"""
        spec = ClipSpec(qlo, qhi, ll_hi, lo, hi).fits(self.np + 1)
        if nsteps is None:
            ns = C.c_int(0)
            check(load().mcx_samples_steps(self.h, C.byref(ns)))
            nsteps = ns.value - first_step
        return _clip_call(lambda *a: load().mcx_samples_clip(self.h, first_step, nsteps, *a), spec, self.np + 1,
                          max(nsteps, 0) * self.nc, count_only)

    def clip_times(self, qlo=0.01, qhi=0.99, ll_hi=0.0, first_step=0, nsteps=None):
        """mcx_debug_clip_times: ms of (the thresholds, the mark sweep, the scan, the scatter sweep, the whole call) of one
        clip() call"""
        spec = ClipSpec(qlo, qhi, ll_hi)
        ms = np.zeros(5)
        self._on_store(load().mcx_debug_clip_times, first_step, nsteps, C.byref(spec.c), _dp(ms))
        return ms

    def _nsteps(self, first_step, nsteps):
        if nsteps is None:
            ns = C.c_int(0)
            check(load().mcx_samples_steps(self.h, C.byref(ns)))
            nsteps = ns.value - first_step
        return nsteps

    def chain_table(self, first_step=0, nsteps=None):
        """mcx_samples_chain_table: what every chain did over kept steps [first_step, first_step + nsteps) -- a dict of
        arrays: mean, sd, rho1 [nc, np + 1] per (chain, column) series (the parameters, then log L); moves, longest_stay,
        ll_max, ll_max_step, flags [nc] per chain"""
        nsteps = self._nsteps(first_step, nsteps)
        return _chain_table_call(lambda *a: load().mcx_samples_chain_table(self.h, first_step, nsteps, *a), self.nc, self.np + 1)

    def chain_table_times(self, first_step=0, nsteps=None):
        """mcx_debug_chain_table_times: ms of (the series sweep, the row sweep, the whole call) of one chain_table() call"""
        ms = np.zeros(3)
        self._on_store(load().mcx_debug_chain_table_times, first_step, nsteps, _dp(ms))
        return ms

    def step_table(self, first_step=0, nsteps=None, probs=(0.05, 0.5, 0.95)):
        """mcx_samples_step_table: what the ensemble looked like at every kept step of [first_step, first_step + nsteps) -- a
        dict of arrays: mean, sd, min, max, flags [T, np + 1] per (step, column) over the nc chains (the parameters, then log
        L); quantiles [T, np + 1, nprobs]; moved (the chains whose row changed from the step before, -1 for the first step),
        ll_max, ll_max_chain, step_flags [T] per step"""
        nsteps = self._nsteps(first_step, nsteps)
        return _step_table_call(lambda *a: load().mcx_samples_step_table(self.h, first_step, nsteps, *a), nsteps, self.np + 1, probs)

    def compare(self, first_a, nsteps_a, first_b, nsteps_b, iid=False):
        """mcx_samples_compare: compare_rows' dict for kept steps [first_a, first_a + nsteps_a) against [first_b, first_b +
        nsteps_b) of this engine's store (the ranges may overlap)"""
        return _compare_call(lambda *a: load().mcx_samples_compare(self.h, first_a, nsteps_a, first_b, nsteps_b, *a), self.np + 1, iid)

    def compare_store(self, first_step, nsteps, other, iid=False):
        """mcx_samples_compare_store: kept steps [first_step, first_step + nsteps) (nsteps None: to the end) against the
        DerivedStore other"""
        nsteps = self._nsteps(first_step, nsteps)
        return _compare_call(lambda *a: load().mcx_samples_compare_store(self.h, first_step, nsteps, other.h, *a), self.np + 1, iid)

    def compare_times(self, first_a, nsteps_a, first_b, nsteps_b, iid=False):
        """mcx_debug_compare_times: ms[10] of one compare() call -- the summaries, A's keys, A's sort, B's keys, B's sort, the
        bounds, the sweep of A, the sweep of B, the reducer, the whole call"""
        spec, ms = CompareSpecC(COMPARE_IID if iid else 0), np.zeros(10)
        check(load().mcx_debug_compare_times(self.h, first_a, nsteps_a, first_b, nsteps_b, C.byref(spec), _dp(ms)))
        return ms

    def energy(self, first_a, nsteps_a, first_b, nsteps_b, **kw):
        """mcx_samples_energy: energy_rows' dict for kept steps [first_a, first_a + nsteps_a) against [first_b, first_b +
        nsteps_b) of this engine's store (the ranges may overlap)"""
        return _energy_call(lambda *a: load().mcx_samples_energy(self.h, first_a, nsteps_a, first_b, nsteps_b, *a), self.np + 1, **kw)

    def energy_store(self, first_step, nsteps, other, **kw):
        """mcx_samples_energy_store: kept steps [first_step, first_step + nsteps) (nsteps None: to the end) against the
        DerivedStore other"""
        nsteps = self._nsteps(first_step, nsteps)
        return _energy_call(lambda *a: load().mcx_samples_energy_store(self.h, first_step, nsteps, other.h, *a), self.np + 1, **kw)

    def energy_times(self, first_a, nsteps_a, first_b, nsteps_b, **kw):
        """mcx_debug_energy_times: ms[7] of one energy() call -- the gather, scale and flags (host), the label vectors (host), the
        uploads, k_energy_pairs, the reducer, the whole call (host clock)"""
        spec, ms = _energy_spec(**kw), np.zeros(7)
        check(load().mcx_debug_energy_times(self.h, first_a, nsteps_a, first_b, nsteps_b, C.byref(spec), _dp(ms)))
        return ms

    def mutual_info(self, first_step=0, nsteps=None, **kw):
        """mcx_samples_mutinfo: rows_mutual_info's dict for kept steps [first_step, first_step + nsteps) (nsteps None: to the end)"""
        nsteps = self._nsteps(first_step, nsteps)
        return _mutinfo_call(lambda *a: load().mcx_samples_mutinfo(self.h, first_step, nsteps, *a), self.np + 1, **kw)

    def mutual_info_times(self, first_step=0, nsteps=None, **kw):
        """mcx_debug_mutinfo_times: ms[8] of one mutual_info() call -- the gather, the points (host), the permutations and the
        table (host), the uploads, k_mi_pairs, the reducer, pearson and the null (host), the whole call (host clock)"""
        nsteps = self._nsteps(first_step, nsteps)
        spec, ms = _MutinfoSpec(**kw), np.zeros(8)
        check(load().mcx_debug_mutinfo_times(self.h, first_step, nsteps, C.byref(spec.c), _dp(ms)))
        return ms

    def reweight(self, weights, probs=(0.05, 0.5, 0.95), first_step=0, nsteps=None):
        """mcx_samples_reweight: reweight_rows' dict for kept steps [first_step, first_step + nsteps)"""
        nsteps = self._nsteps(first_step, nsteps)
        return _reweight_call(lambda *a: load().mcx_samples_reweight(self.h, first_step, nsteps, *a), weights, self.np + 1, probs)

    def resample(self, weights, nsteps_out, nc_out, seed, with_index=False, first_step=0, nsteps=None):
        """mcx_samples_resample: resample_rows' DerivedStore of weighted draws of kept steps [first_step, first_step + nsteps)"""
        nsteps = self._nsteps(first_step, nsteps)
        return _resample_call(lambda *a: load().mcx_samples_resample(self.h, first_step, nsteps, *a), weights, nsteps_out, nc_out,
                              seed, with_index)

    def intervals(self, hdi=(0.9,), probs=(0.05, 0.5, 0.95), first_step=0, nsteps=None):
        """mcx_samples_intervals: per column (the parameters, then log L) of kept steps [first_step, first_step + nsteps) the
        highest-density interval of every mass in hdi and the Monte-Carlo errors of the sd and of the quantiles of probs, with
        the effective sizes behind them (_intervals_call lists the fields)"""
        nsteps = self._nsteps(first_step, nsteps)
        return _intervals_call(lambda *a: load().mcx_samples_intervals(self.h, first_step, nsteps, *a), self.np + 1, hdi, probs)

    def intervals_times(self, hdi=(0.9,), probs=(0.05, 0.5, 0.95), first_step=0, nsteps=None):
        """mcx_debug_intervals_times: the 12 stage times of one intervals() call in ms (include/mcx.h lists them)"""
        spec = IntervalSpec(hdi, probs)
        ms = np.zeros(INTERVAL_TIMES)
        self._on_store(load().mcx_debug_intervals_times, first_step, nsteps, C.byref(spec.c), _dp(ms))
        return ms

    def lagcov(self, max_lag=None, nlags=0, with_ll=False, first_step=0, nsteps=None):
        """mcx_samples_lagcov of kept steps [first_step, first_step + nsteps): the lagged covariance matrices G(0) .. G(nlags - 1) of
        the columns (the parameters, then log L) and their cross-correlations, the multivariate initial sequence estimator sigma of
        the chosen columns (the parameters, and log L with with_ll) walked over the lags up to max_lag, the multivariate effective
        sample size mess and the ess and mcse per column made of sigma (_lagcov_dict lists the fields)"""
        nsteps = self._nsteps(first_step, nsteps)
        return _lagcov_call(lambda *a: load().mcx_samples_lagcov(self.h, first_step, nsteps, *a), nsteps, self.np + 1, max_lag, nlags,
                            with_ll)

    def modes(self, k, first_step=0, nsteps=None, **spec):
        """mcx_samples_modes of kept steps [first_step, first_step + nsteps): the rows partitioned into k modes by k-means on the
        device -> Modes (the mode table, the centres, the labels on the device, and from them the chains' hops, the rows of one
        mode and the indicator store).  spec: max_iter=50, scale=True (1 / sd per column), seed_rows=16384, seed=0, centres=None
        or [k, np] unscaled starting centres in place of the k-means++ seeding"""
        nsteps = self._nsteps(first_step, nsteps)
        return _modes_call(lambda *a: load().mcx_samples_modes(self.h, first_step, nsteps, *a), _modes_spec(k, self.np, **spec), self.np,
                           (nsteps, self.nc, self.np + 1),
                           lambda *a: load().mcx_samples_mode_rows(self.h, first_step, nsteps, *a))

    def evidence(self, vl=None, proposal=None, first_step=0, nsteps=None, **spec):
        """mcx_samples_evidence of kept steps [first_step, first_step + nsteps): log Z of the sampled function by bridge sampling
        -> a dict of mcx_evidence_result's fields (log_z, se, neff, iters, flags, the by-products log_z_is and log_z_ris, ...).
        vl None: the last run's likelihood.  proposal None: one Gaussian fitted on the first fit_steps steps, which are then left
        out.  spec: ndraw=0 (min(N1, 2^20)), seed=0, fit_steps=-1, use_neff=True, max_iter=1000, tol=1e-10, scale=1.0"""
        nsteps = self._nsteps(first_step, nsteps)
        return _evidence_call(lambda *a: load().mcx_samples_evidence(self.h, first_step, nsteps, *a), vl, proposal, **spec)

    def evidence_times(self, vl=None, proposal=None, first_step=0, nsteps=None, **spec):
        """mcx_debug_evidence_times: (ms[EVIDENCE_TIMES] of one evidence() call -- include/mcx.h lists them --, the result dict)"""
        nsteps = self._nsteps(first_step, nsteps)
        ms = np.zeros(EVIDENCE_TIMES)
        res = _evidence_call(lambda *a: load().mcx_debug_evidence_times(self.h, first_step, nsteps, *a, _dp(ms)), vl, proposal, **spec)
        return ms, res

    def profile_likelihood(self, n=64, levels=None, drops=None, clip=(0, 1), from_=None, to=None, path=False, first_step=0, nsteps=None):
        """mcx_samples_profile: per parameter of kept steps [first_step, first_step + nsteps) the profile likelihood pl(x) = max
        { log L of the rows whose value is in the bin of x } - max log L on n bins, its least concave majorant plh, and per level
        (confidence levels, or drops of log L) the interval where the curve is within the drop (_profile_call lists the fields).
        xat, the value in the winning row, is the abscissa.  (Engine.profile is the kernel timing table; hence the name.)"""
        nsteps = self._nsteps(first_step, nsteps)
        spec = ProfileSpec(n, clip, from_, to, levels, drops).fits(self.np)
        return _profile_call(lambda *a: load().mcx_samples_profile(self.h, first_step, nsteps, *a), spec, self.np, path)

    def profile_likelihood2d(self, g=32, pairs=None, levels=None, drops=None, clip=(0, 1), from_=None, to=None, first_step=0, nsteps=None):
        """mcx_samples_profile2d: per pair of parameters (pairs [npairs, 2]; None: every a < b) the profile likelihood z = max log
        L of the cell - max log L on g x g cells, for contours on the corner plot (_profile2d_call lists the fields)"""
        nsteps = self._nsteps(first_step, nsteps)
        spec = ProfileSpec(g, clip, from_, to, levels, drops, pairs, two_d=True).fits(self.np)
        return _profile2d_call(lambda *a: load().mcx_samples_profile2d(self.h, first_step, nsteps, *a), spec, self.np)

    def profile_likelihood_times(self, n=64, clip=(0, 1), first_step=0, nsteps=None):
        """mcx_debug_profile_times: ms of (the statistics passes, k_profile_bins, the host grids and finish, the whole call) of one
        profile_likelihood() call"""
        spec = ProfileSpec(n, clip)
        ms = np.zeros(4)
        self._on_store(load().mcx_debug_profile_times, first_step, nsteps, C.byref(spec.c), _dp(ms))
        return ms

    def profile_likelihood2d_times(self, g=32, pairs=None, clip=(0, 1), first_step=0, nsteps=None):
        """mcx_debug_profile2d_times: ms of (the statistics passes, the code and key sweeps, k_profile_pairs, k_profile_at, the host
        grids and finish, the whole call) of one profile_likelihood2d() call"""
        spec = ProfileSpec(g, clip, pairs=pairs, two_d=True)
        ms = np.zeros(6)
        self._on_store(load().mcx_debug_profile2d_times, first_step, nsteps, C.byref(spec.c), _dp(ms))
        return ms

    def modes_times(self, k, first_step=0, nsteps=None, **spec):
        """mcx_debug_modes_times: (ms[MODES_TIMES] of one modes() call -- include/mcx.h lists them --, the result dict)"""
        nsteps = self._nsteps(first_step, nsteps)
        sp, _keep = _modes_spec(k, self.np, **spec)
        res, ms = ModesResultC(), np.zeros(MODES_TIMES)
        check(load().mcx_debug_modes_times(self.h, first_step, nsteps, C.byref(sp), C.byref(res), _dp(ms)))
        return ms, {name: getattr(res, name) for name in ("k", "iters", "flags", "n", "n_nonfinite", "n_changed", "inertia")}

    def lagcov_times(self, max_lag=None, nlags=0, with_ll=False, first_step=0, nsteps=None):
        """mcx_debug_lagcov_times: (the 5 stage times of one lagcov() call in ms -- include/mcx.h lists them --, lags_computed)"""
        nsteps = self._nsteps(first_step, nsteps)
        spec = LagcovSpecC(max(nsteps - 1, 1) if max_lag is None else int(max_lag), int(nlags), 1 if with_ll else 0)
        res, ms = LagcovResultC(), np.zeros(LAGCOV_TIMES)
        check(load().mcx_debug_lagcov_times(self.h, first_step, nsteps, C.byref(spec), C.byref(res), _dp(ms)))
        return ms, res.lags_computed

    def reweight_times(self, weights, probs=(0.05, 0.5, 0.95), nsteps_out=0, nc_out=0, seed=0, first_step=0, nsteps=None):
        """mcx_debug_reweight_times: ms[8] of one reweight() and, with nsteps_out * nc_out > 0, one resample() call -- the
        maximum, q and the scan, the moment passes, the histogram passes, the sort of q, the draw, the whole reweight, the whole
        resample"""
        p, pp = _probs(probs)
        ms = np.zeros(8)
        self._on_store(load().mcx_debug_reweight_times, first_step, nsteps, C.byref(weights.c), pp if len(p) else None, len(p), seed,
                       nsteps_out, nc_out, _dp(ms))
        return ms

    def step_table_times(self, first_step=0, nsteps=None, probs=(0.05, 0.5, 0.95)):
        """mcx_debug_step_table_times: ms of (the moments sweep, the select sweep, the row sweep and its reducer, the whole
        call) of one step_table() call"""
        p, pp = _probs(probs)
        ms = np.zeros(4)
        self._on_store(load().mcx_debug_step_table_times, first_step, nsteps, pp if len(p) else None, len(p), _dp(ms))
        return ms

    def select_chains(self, chains, first_step=0, nsteps=None):
        """mcx_samples_select_chains: the DerivedStore of chains (any order, repeats allowed; e.g. keep_chains' kept_indices)
        over kept steps [first_step, first_step + nsteps): real chains, for every analysis of a store"""
        nsteps = self._nsteps(first_step, nsteps)
        return _select_call(lambda *a: load().mcx_samples_select_chains(self.h, first_step, nsteps, *a), chains)

    def derive(self, spec, first_step=0, nsteps=None):
        """mcx_samples_derive: the DerivedStore of spec (derive_linear / derive_source) applied to every row of kept steps
        [first_step, first_step + nsteps)"""
        h = C.c_void_p()
        self._on_store(load().mcx_samples_derive, first_step, nsteps, None if spec is None else C.byref(spec.c), C.byref(h))
        return DerivedStore(h)

    def derive_times(self, spec, first_step=0, nsteps=None):
        """mcx_debug_derive_times: ms of one derive sweep of spec over the range (the second of two into one store)"""
        ms = np.zeros(1)
        self._on_store(load().mcx_debug_derive_times, first_step, nsteps, C.byref(spec.c), _dp(ms))
        return float(ms[0])

    def draw(self, ndraw, seed, first_step=0, nsteps=None):
        """mcx_samples_draw: ndraw rows of kept steps [first_step, first_step + nsteps) with replacement -- (rows [ndraw,
        np + 1], index [ndraw] int64 into the rows of the range)"""
        rows, index = np.empty((max(ndraw, 0), self.np + 1), np.float32), np.empty(max(ndraw, 0), np.int64)
        self._on_store(load().mcx_samples_draw, first_step, nsteps, seed, ndraw, _fp(rows),
                       index.ctypes.data_as(C.POINTER(C.c_int64)))
        return rows, index

    def proposal_cov(self, scale=None, first_step=0, nsteps=None):
        """covariance() then proposal_from_cov(): the incov of the next run from this run's store"""
        return proposal_from_cov(self.covariance(first_step, nsteps)["cov"], self.np, scale)

    def summary_windows(self, first_step=0, nsteps=None):
        """how many 32-lag autocovariance windows the summary of that range computes (mcx_debug_summary_windows)"""
        nw = C.c_int(0)
        self._on_store(load().mcx_debug_summary_windows, first_step, nsteps, C.byref(nw))
        return nw.value

    def maxlike(self):
        lm = C.c_float(0)
        p = np.empty(self.np, np.float32)
        check(load().mcx_samples_maxlike(self.h, C.byref(lm), _fp(p)))
        return lm.value, p

    @property
    def profile(self):
        p = Profile()
        check(load().mcx_get_profile(self.h, C.byref(p)))
        return {K_NAMES[i]: dict(ms=p.ms[i], launches=int(p.launches[i]), chain_steps=int(p.chain_steps[i]))
                for i in range(len(K_NAMES))}
