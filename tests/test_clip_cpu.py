"""The host half of the tail clip: mcx_debug_clip_thresholds against tests/clip_ref.py, the spec's
refusals without a device, clip_ref against a transcription of the three statements of the reference's mcparam.clip.tails,
and the stand-alone sanitizer check of the host code.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import clip_ref as R
from mcpar_amd import McxError
from mcpar_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def table(seed=3, n=200, ncol=4):
    rng = np.random.default_rng(seed)
    rows = rng.normal(0.0, 1.0, (n, ncol)).astype(np.float32)
    rows[:, -1] = -np.abs(rows[:, -1]) + 0.1  # a log L column with a few values above 0
    return rows


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    assert np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)]), (got, want)


@pytest.mark.parametrize("ll_hi", [0.0, INF, NAN])
def test_thresholds_ll_rule(ll_hi):
    q = R.column_quantiles(table(), 0.05, 0.9)
    tl, th = E.debug_clip_thresholds(q, 0.05, 0.9, ll_hi)
    rl, rh = R.thresholds_from_quantiles(q, ll_hi)
    same(tl, rl)
    same(th, rh)
    assert np.array_equal(tl, q[:, 0]) and np.array_equal(th[:-1], q[:-1, 1])
    assert th[-1] == (q[-1, 1] if np.isnan(ll_hi) else ll_hi)


def test_thresholds_ll_hi_overridden_by_hi():
    q = R.column_quantiles(table(), 0.01, 0.99)
    hi = [NAN, NAN, NAN, -0.25]
    tl, th = E.debug_clip_thresholds(q, ll_hi=0.0, hi=hi)
    same(th, R.thresholds_from_quantiles(q, 0.0, None, hi)[1])
    assert th[-1] == -0.25 and np.array_equal(th[:-1], q[:-1, 1]) and np.array_equal(tl, q[:, 0])


def test_thresholds_nan_entries_are_defaults_and_inf_overrides():
    q = R.column_quantiles(table(), 0.01, 0.99)
    lo, hi = [NAN, -INF, 0.5, NAN], [INF, NAN, NAN, NAN]
    tl, th = E.debug_clip_thresholds(q, ll_hi=0.0, lo=lo, hi=hi)
    rl, rh = R.thresholds_from_quantiles(q, 0.0, lo, hi)
    same(tl, rl)
    same(th, rh)
    assert tl[0] == q[0, 0] and tl[1] == -INF and tl[2] == 0.5 and tl[3] == q[3, 0]
    assert th[0] == INF and th[1] == q[1, 1] and th[2] == q[2, 1] and th[3] == 0.0


def test_thresholds_nan_quantiles_stay_nan_unless_given():
    q = np.array([[NAN, NAN], [-1.0, 1.0]])
    tl, th = E.debug_clip_thresholds(q, ll_hi=NAN)
    assert np.isnan(tl[0]) and np.isnan(th[0]) and tl[1] == -1.0 and th[1] == 1.0
    tl, th = E.debug_clip_thresholds(q, ll_hi=NAN, lo=[-2.0, NAN], hi=[2.0, NAN])
    assert tl[0] == -2.0 and th[0] == 2.0


def test_thresholds_refusals():
    from mcpar_amd._lib import load
    import ctypes as C
    spec = E.ClipSpec()
    out = np.zeros(2)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    assert load().mcx_debug_clip_thresholds(0, dp, C.byref(spec.c), dp, dp) == 1
    assert load().mcx_debug_clip_thresholds(1, dp, None, dp, dp) == 1
    assert load().mcx_debug_clip_thresholds(1, dp, C.byref(spec.c), None, dp) == 1


@pytest.mark.parametrize("qlo,qhi", [(0.5, 0.5), (0.9, 0.1), (-0.1, 0.9), (0.1, 1.5), (NAN, 0.9), (0.1, NAN)])
def test_spec_refusals_need_no_device(qlo, qhi):
    """MCX_ERR_INVALID (1), not MCX_ERR_NO_DEVICE: the spec is checked before a device is touched"""
    rows = table()
    with pytest.raises(McxError) as ei:
        E.clip_rows(rows, 50, 4, qlo, qhi)
    assert ei.value.code == 1 and "qlo < qhi" in str(ei.value)


def test_null_arguments_need_no_device():
    from mcpar_amd._lib import load
    import ctypes as C
    rows = table()
    fp = rows.ctypes.data_as(C.POINTER(C.c_float))
    spec = E.ClipSpec()
    cols, k, h = np.zeros(4, E.CLIP_DTYPE), C.c_longlong(0), C.c_void_p()
    cp = cols.ctypes.data_as(C.c_void_p)
    L = load()
    assert L.mcx_rows_clip(fp, 50, 4, 3, None, cp, C.byref(k), C.byref(h)) == 1
    assert b"spec is NULL" in L.mcx_last_error()
    assert L.mcx_rows_clip(fp, 50, 4, 3, C.byref(spec.c), None, C.byref(k), C.byref(h)) == 1
    assert L.mcx_rows_clip(fp, 50, 4, 3, C.byref(spec.c), cp, None, C.byref(h)) == 1
    assert b"cols or nkept is NULL" in L.mcx_last_error()
    assert L.mcx_rows_clip(fp, 0, 4, 3, C.byref(spec.c), cp, C.byref(k), C.byref(h)) == 1
    assert L.mcx_samples_clip(None, 0, 4, C.byref(spec.c), cp, C.byref(k), C.byref(h)) == 1
    assert b"engine is NULL" in L.mcx_last_error()
    assert L.mcx_store_clip(None, C.byref(spec.c), cp, C.byref(k), C.byref(h)) == 1
    for fn, args in ((L.mcx_rowset_copy, (0, 0, None)), (L.mcx_rowset_index, (0, 0, None)), (L.mcx_rowset_draw, (1, 0, None, None)),
                     (L.mcx_rowset_store, (0, 1, 1, C.byref(h))), (L.mcx_rowset_shape, (None, None, None))):
        assert fn(None, *args) == 1
        assert b"row set r is NULL" in L.mcx_last_error()
    assert L.mcx_rowset_destroy(None) == 0
    assert not h


def test_lo_hi_take_one_entry_per_column():
    with pytest.raises(ValueError):
        E.clip_rows(table(), 50, 4, lo=[0.0, 0.0])


def test_ref_against_the_reference_statements():
    """mcparam.clip.tails, its three statements on a small table:
         quants <- apply(mc.data, 2, function(x) quantile(x, probs = c(qlo, qhi)))
         quants[2, ncol(quants)] <- 0.0
         keep <- apply(mc.data, 1, function(x) all(x > quants[1,] & x < quants[2,]))
    R's quantile() default is type 7, numpy's "linear"."""
    rows = table(seed=11, n=157, ncol=5)
    d = rows.astype(np.float64)
    quants = np.quantile(d, [0.05, 0.95], axis=0)
    quants[1, -1] = 0.0
    keep = np.array([np.all((x > quants[0]) & (x < quants[1])) for x in d])
    ref = R.clip(rows, 0.05, 0.95, 0.0)
    np.testing.assert_allclose(ref["lo"], quants[0], rtol=1e-14)
    np.testing.assert_allclose(ref["hi"], quants[1], rtol=1e-14)
    assert np.array_equal(ref["keep"], keep) and 0 < keep.sum() < keep.size
    assert np.array_equal(ref["rows"], rows[keep])
    assert np.array_equal(ref["nbelow"], (~(d > quants[0])).sum(axis=0)) and np.array_equal(ref["nabove"], (~(d < quants[1])).sum(axis=0))


def test_ref_nan_and_ties():
    rows = np.array([[0.0, -1.0], [1.0, -2.0], [np.nan, -3.0], [2.0, -4.0], [1.0, -5.0]], np.float32)
    r = R.clip(rows, 0.0, 1.0, INF)
    assert np.isnan(r["lo"][0]) and r["keep"].sum() == 0 and r["nbelow"][0] == 5 and r["nabove"][0] == 5
    r = R.clip(rows, 0.0, 1.0, INF, lo=[0.0, NAN], hi=[2.0, NAN])
    # column 0: strict on both sides, the NaN counts in both; column 1, log L: its minimum goes, no upper clip
    assert r["nbelow"].tolist() == [2, 1] and r["nabove"].tolist() == [2, 0]
    assert r["index"].tolist() == [1]


def test_host_code_under_sanitizers(tmp_path):
    """tests/cpp/clip_thresholds_check.cc: the host half (csrc/mcx_clip_host.hpp, what mcx_debug_clip_thresholds and the
    spec check are made of) as a stand-alone program under AddressSanitizer and UBSan"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "clip_thresholds_check"
    b = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", ROOT,
                        os.path.join(ROOT, "tests", "cpp", "clip_thresholds_check.cc"), "-o", str(exe)], capture_output=True, timeout=300)
    if b.returncode != 0 and b"cannot find" in b.stderr and (b"asan" in b.stderr or b"ubsan" in b.stderr):
        pytest.skip("the host compiler has no sanitizer runtimes")
    assert b.returncode == 0, b.stderr.decode()
    r = subprocess.run([str(exe)], capture_output=True, timeout=60)
    assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()
    assert b"clip_thresholds_check ok" in r.stdout
