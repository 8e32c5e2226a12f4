"""The rank-normalised summaries without a GPU: the float64 reference (tests/rank_ref.py) against the counting definition
of a rank, the host's PPND16 against statistics.NormalDist, the header as C99, the argument errors, and the two cases the
basic diagnostics call converged."""
import ctypes as C
import math
import os
import statistics
import subprocess

import numpy as np
import pytest

import rank_cases as K
import rank_ref as RR
import summary_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ND = statistics.NormalDist()


def counting_ranks(v):
    """#less + (#equal + 1) / 2, O(N^2), in float comparisons (-0 == +0)"""
    v = np.asarray(v, np.float32).astype(np.float64)
    less = (v[None, :] < v[:, None]).sum(axis=1)
    equal = (v[None, :] == v[:, None]).sum(axis=1)
    return less + (equal + 1) / 2.0


RANK_ARRAYS = [
    [1.0, 2.0, 3.0, 4.0],
    [3.0, 3.0, 3.0, 3.0, 3.0],
    [2.0, -1.0, 2.0, -1.0, 0.5, 2.0],
    [0.0, -0.0, 1e-45, -1e-45, 0.0, 1.1754942e-38, -1.1754942e-38, -0.0],
    [-3.5, -3.5, -7.25, 0.0, -0.0, 2.0, -1e30, 1e30, -1e30],
    [1e-45, 2e-45, 1e-45, 3e-45, 0.0, -2e-45, -2e-45],
]


@pytest.mark.parametrize("k", range(len(RANK_ARRAYS) + 1))
def test_reference_ranks_are_the_counting_definition(k):
    if k < len(RANK_ARRAYS):
        v = np.array(RANK_ARRAYS[k], np.float32)
    else:
        rng = np.random.default_rng(3)
        v = rng.integers(-20, 20, 500).astype(np.float32) * np.float32(0.25)
    r = RR.ranks(v)
    assert r.dtype == np.float64
    assert np.array_equal(r, counting_ranks(v))
    assert np.array_equal(r * 2, np.round(r * 2))  # multiples of 0.5
    assert r.sum() == v.size * (v.size + 1) / 2


def test_sort_based_ranks_are_the_reference_ranks():
    """rank_ref.ranks_by_sort (for the multi-million-value GPU case) against rank_ref.ranks: the small arrays above, every
    content kind of the GPU test at two of its shapes, NaNs, and the vectorised "mh" content"""
    rng = np.random.default_rng(11)
    cases = [np.array(a, np.float32) for a in RANK_ARRAYS]
    cases += [K.content(kind, T, nc, rng) for kind in K.KINDS for T, nc in ((37, 33), (257, 3))]
    cases.append(np.array([2.0, np.nan, -1.0, np.nan, 2.0, np.inf, -np.inf], np.float32))
    cases.append(np.array([7.0], np.float32))
    src = K.repeats(5000, 2, rng, 0.3)
    mh = rng.standard_normal((5000, 2)).astype(np.float32)[src, np.arange(2)]
    assert 0.25 < (np.diff(src, axis=0) == 0).mean() < 0.35 and (mh[1:] == mh[:-1]).mean() > 0.25
    cases.append(mh)
    for v in cases:
        got, want = RR.ranks_by_sort(v), RR.ranks(v)
        assert got.dtype == np.float64 and np.array_equal(got, want)
    assert np.array_equal(RR.ranks_by_sort(cases[0]), counting_ranks(cases[0]))


def test_the_large_case_is_what_its_gpu_test_says():
    """rank_cases.big_columns(), the content of test_gpu_rank_summary.py's case past the size switches: all three switches
    crossed, tie runs across the boundaries of the sort tiles, every byte of the keys varying behind tile 255 and behind
    tile 511 too, log L negative -- and the sort-based ranks against rank_ref.ranks on a stretch of it"""
    np_, nc, T = K.BIG_SHAPE
    N = T * nc
    assert -(-N // 8192) == 514 and N % 8192 == 38 and max(64, (T + 32767) // 32768) == 65
    cols = K.big_columns()
    assert (cols[1] < 0).all() and np.isfinite(cols[0]).all() and np.isfinite(cols[1]).all()
    tiles = np.arange(N) // 8192
    for c in cols:
        flat = c.reshape(-1)
        assert c.dtype == np.float32 and c.shape == (T, nc) and 0.29 < (c[1:] == c[:-1]).mean() < 0.31
        tied = flat[2:] == flat[:-2]  # a chain's consecutive steps are nc = 2 apart
        assert (tied & (tiles[2:] != tiles[:-2])).sum() > 100
        k = R.okey(flat)
        for lo in (0, 256 * 8192, 512 * 8192):
            for shift, least in ((0, 256), (8, 256), (16, 256), (24, 4)):
                assert np.count_nonzero(np.bincount((k[lo:] >> shift) & 255, minlength=256)) >= least, (lo, shift)
        part = c[:50000]
        assert np.array_equal(RR.ranks_by_sort(part), RR.ranks(part))


def test_reference_normal_scores():
    N = 1221
    r = np.arange(1, N + 1, dtype=np.float64)
    z = RR.normal_scores(r, N)
    assert z.dtype == np.float32
    want = np.array([ND.inv_cdf((k - 0.375) / (N + 0.25)) for k in r]).astype(np.float32)
    assert np.array_equal(z, want)
    assert (np.diff(z.astype(np.float64)) > 0).all()  # monotone in the rank
    assert np.array_equal(z, -z[::-1])                 # and odd about the middle rank
    half = RR.normal_scores(np.array([1.5, 1.5, 3.0]), 3)
    assert half[0] == half[1] < half[2]


def ppnd_grid():
    p = [0.5, 0.075, 0.925, np.nextafter(0.075, 0), np.nextafter(0.075, 1), np.nextafter(0.925, 0), np.nextafter(0.925, 1),
         math.exp(-25.0), np.nextafter(math.exp(-25.0), 0), np.nextafter(math.exp(-25.0), 1), 1.0 - math.exp(-25.0),
         1e-300, 5e-324, 1e-20, 1.0 - 2.0 ** -53]
    for N in (4.0, 6.6e7):
        p += [(1 - 0.375) / (N + 0.25), 1.0 - (1 - 0.375) / (N + 0.25), (N - 0.375) / (N + 0.25)]
    p += list(np.linspace(1e-6, 1 - 1e-6, 4001)) + list(np.logspace(-40, -1, 400))
    return np.array(p, np.float64)


def test_normal_quantile_matches_normaldist():
    from mcpar_amd import engine as E
    p = ppnd_grid()
    z = E.debug_normal_quantile(p)
    want = np.array([ND.inv_cdf(float(v)) for v in p])
    ulp = np.abs(z - want) / np.spacing(np.abs(want))
    print("largest difference from NormalDist().inv_cdf: %.2f ulp" % ulp[want != 0].max())
    assert ulp[want != 0].max() <= 4
    assert z[0] == 0.0 and want[0] == 0.0  # exactly 0 at p = 0.5
    assert np.isnan(E.debug_normal_quantile([0.0, 1.0, -0.1, 1.5, float("nan")])).all()
    assert E.debug_normal_quantile([]).size == 0


def test_header_is_plain_c99_with_rank_summary(tmp_path):
    src = tmp_path / "cabi_rank.c"
    src.write_text('#include "mcx.h"\nint main(void){ mcx_col_rank_summary c; double p = 0.5, z = 1.0;\n'
                   ' c.flags = MCX_SUMMARY_NONFINITE; c.ess_bulk_lag = 0; c.rhat = c.rhat_bulk = c.rhat_folded = 0.0;\n'
                   ' c.ess_bulk = c.ess_tail = c.ess_q05 = c.ess_q95 = c.q05 = c.median = c.q95 = 0.0; (void)c;\n'
                   ' if (mcx_debug_normal_quantile(&p, 1, &z) != MCX_OK || z != 0.0) return 2;\n'
                   ' if (mcx_rows_rank_summary(0, 3, 1, 1, &c) != MCX_ERR_INVALID) return 3;\n'
                   ' if (mcx_samples_rank_summary(0, 0, 4, &c) != MCX_ERR_INVALID) return 4;\n'
                   ' return mcx_abi_version() == MCX_ABI_VERSION ? 0 : 1; }\n')
    exe = tmp_path / "cabi_rank"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", os.path.join(ROOT, "mcpar_amd"), "-lmcx",
                           "-Wl,-rpath," + os.path.join(ROOT, "mcpar_amd")])
    assert subprocess.call([str(exe)]) == 0


def test_argument_errors_need_no_device():
    import mcpar_amd as M
    from mcpar_amd import engine as E
    lib = M.load()
    rows = np.zeros((8, 2), np.float32)
    cols = np.zeros(2, E.RANK_SUMMARY_DTYPE)
    cp, fp = cols.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.POINTER(C.c_float))
    INVALID = 1
    assert lib.mcx_rows_rank_summary(fp, 3, 2, 1, cp) == INVALID      # nsteps < 4
    assert b"nsteps >= 4" in lib.mcx_last_error()
    assert lib.mcx_rows_rank_summary(fp, 4, 2, 1, None) == INVALID    # NULL cols
    assert lib.mcx_rows_rank_summary(None, 4, 2, 1, cp) == INVALID    # NULL rows
    assert lib.mcx_rows_rank_summary(fp, 4, 0, 1, cp) == INVALID      # no chains
    assert lib.mcx_rows_rank_summary(fp, 4, 2, 257, cp) == INVALID    # np > 256
    assert lib.mcx_samples_rank_summary(None, 0, 4, cp) == INVALID    # NULL engine
    out = np.zeros_like(rows)
    op = out.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.mcx_debug_rows_rank_transform(fp, 4, 2, 1, 4, None, op) == INVALID  # what out of range
    assert lib.mcx_debug_rows_rank_transform(fp, 4, 2, 1, 0, None, None) == INVALID
    dbl = np.zeros(16)
    assert lib.mcx_debug_rows_rank_transform(fp, 4, 2, 1, 2, dbl.ctypes.data_as(C.POINTER(C.c_double)), op) == INVALID
    with pytest.raises(M.McxError) as ei:
        E.rows_rank_summary(rows, 3, 2)
    assert ei.value.code == INVALID


def test_scale_case_on_the_reference():
    """one chain of four has 3 x the scale: the basic diagnostics see nothing, the folded R-hat and the tail ESS do"""
    x = K.demo_scale()
    b, r = R.restate_column(x, ()), RR.restate_column(x)
    print("scale case: basic rhat %.4f ess %.0f | rhat_folded %.4f ess_tail %.1f (%.1f / %.1f)"
          % (b["rhat"], b["ess"], r["rhat_folded"], r["ess_tail"], r["ess_q05"], r["ess_q95"]))
    K.check_demo_scale(b["rhat"], b["ess"], r["rhat_folded"], r["ess_tail"])
    assert RR.guard_ok(r)


def test_cauchy_case_on_the_reference():
    """four Cauchy chains, one shifted by 1: basic R-hat and ESS rest on moments that do not exist"""
    x = K.demo_cauchy()
    b, r = R.restate_column(x, ()), RR.restate_column(x)
    print("cauchy case: basic rhat %.4f ess %.0f | rhat_bulk %.4f ess_bulk %.1f" % (b["rhat"], b["ess"], r["rhat_bulk"], r["ess_bulk"]))
    K.check_demo_cauchy(b["rhat"], b["ess"], r["ess_bulk"])
    assert RR.guard_ok(r)


def test_reference_degenerate_and_nonfinite_columns():
    T, nc = 12, 3
    const = RR.restate_column(np.full((T, nc), 2.5, np.float32))
    assert const["flags"] == 0 and const["median"] == 2.5
    for f in ("rhat", "rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "ess_q05", "ess_q95"):
        assert math.isnan(const[f]), f
    x = np.arange(T * nc, dtype=np.float32).reshape(T, nc)
    x[5, 1] = np.inf
    bad = RR.restate_column(x)
    assert bad["flags"] == 1 and all(math.isnan(bad[f]) for f in RR.FIELDS)
