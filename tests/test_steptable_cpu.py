"""The host half of the step table: the restatement tests/steptable_ref.py against hand-worked tiny
cases, mcx_debug_steptable_geometry on both sides of every size switch it reports, what the entry points refuse without a
device, mcx_steps_settle against the restatement on planted tables, the header as C99 and the host code under sanitizers.
No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import steptable_ref as R
from mcpar_amd import McxError
from mcpar_amd import engine as E
from mcpar_amd._lib import StepRule, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


# ---- the restatement, by hand ---------------------------------------------------------------------------------------------------
def test_restatement_one_chain_one_step():
    t = R.table(np.array([[2.5, -1.0]], np.float32), 1, 1, probs=(0.0, 0.3, 1.0))
    assert t["mean"].tolist() == [[2.5, -1.0]] and np.isnan(t["sd"]).all()
    assert t["min"].tolist() == [[2.5, -1.0]] and t["max"].tolist() == [[2.5, -1.0]]
    assert t["quantiles"].tolist() == [[[2.5] * 3, [-1.0] * 3]]
    assert t["moved"].tolist() == [-1] and t["ll_max"].tolist() == [-1.0] and t["ll_max_chain"].tolist() == [0]
    assert t["flags"].tolist() == [[0, 0]] and t["step_flags"].tolist() == [0]


def test_restatement_ties_and_the_ends():
    # one step of five chains: column 0 = 1, 3, 3, 3, 7; log L = -4, -2, -2, -9, -5
    rows = np.array([[1, -4], [3, -2], [3, -2], [3, -9], [7, -5]], np.float32)
    t = R.table(rows, 1, 5, probs=(0.0, 0.25, 0.3, 0.5, 0.9, 1.0))
    assert t["mean"][0, 0] == 17 / 5 and t["sd"][0, 0] == np.sqrt((2.4 ** 2 + 3 * 0.4 ** 2 + 3.6 ** 2) / 4)
    assert t["min"][0].tolist() == [1.0, -9.0] and t["max"][0].tolist() == [7.0, -2.0]
    # h = 4 p: 0, 1, 1.2, 2, 3.6, 4 -> 1, 3, 3 (a tie: x(lo) itself), 3, 3 + 0.6 * 4, 7
    assert t["quantiles"][0, 0].tolist() == [1.0, 3.0, 3.0, 3.0, 3.0 + (3.6 - 3) * 4.0, 7.0]
    assert t["ll_max"][0] == -2.0 and t["ll_max_chain"][0] == 1  # the lowest chain of two that hold it


def test_restatement_moved_and_signed_zeros():
    a = np.zeros((3, 2, 2), np.float32)  # T = 3, nc = 2
    a[1, 0, 0] = -0.0                    # chain 0: +0 -> -0 -> +0 in column 0: two moves; chain 1 never moves
    t = R.table(a.reshape(6, 2), 3, 2, probs=(0.0, 0.5, 1.0))
    assert t["moved"].tolist() == [-1, 1, 1]
    assert np.signbit(t["min"][1, 0]) and not np.signbit(t["max"][1, 0])  # -0 before +0
    assert np.signbit(t["quantiles"][1, 0, 0]) and not np.signbit(t["quantiles"][1, 0, 2])
    assert t["quantiles"][1, 0, 1] == 0.0 and np.signbit(t["quantiles"][1, 0, 1])  # -0 == +0: x(lo) itself
    a[:, 1, 1] = [0.0, -0.0, -0.0]       # log L of chain 1: +0, -0, -0; chain 0 keeps +0
    t = R.table(a.reshape(6, 2), 3, 2, probs=())
    assert t["moved"].tolist() == [-1, 2, 1] and t["ll_max_chain"].tolist() == [0, 0, 0] and t["quantiles"].shape == (3, 2, 0)
    # one NaN pattern repeated is no move
    a[:, 0, 0] = np.array([0x7fc01234], np.uint32).view(np.float32)[0]
    t = R.table(a.reshape(6, 2), 3, 2, probs=(0.5,))
    assert t["moved"].tolist() == [-1, 1, 0]


def test_restatement_nan_and_inf():
    a = np.arange(24, dtype=np.float32).reshape(2, 4, 3)  # T = 2, nc = 4, two parameters and log L
    a[0, 1, 0] = NAN
    a[1, 2, 1] = INF
    a[1, 3, 2] = -INF
    t = R.table(a.reshape(8, 3), 2, 4, probs=(0.0, 0.5, 0.1))
    assert t["flags"].tolist() == [[1, 0, 0], [0, 1, 1]] and t["step_flags"].tolist() == [1, 1]
    assert np.isnan(t["mean"][0, 0]) and np.isnan(t["sd"][0, 0]) and np.isnan(t["min"][0, 0]) and np.isnan(t["max"][0, 0])
    assert np.isnan(t["quantiles"][0, 0]).all()
    assert np.isnan(t["mean"][1, 1]) and t["max"][1, 1] == INF and t["min"][1, 1] == 13.0 and t["quantiles"][1, 1, 0] == 13.0
    assert t["min"][1, 2] == -INF and t["ll_max"][1] == 20.0 and t["ll_max_chain"][1] == 2
    assert t["quantiles"][1, 2, 1] == 15.5 and np.isnan(t["quantiles"][1, 2, 2])  # -inf + 0.3 (14 - -inf): what the formula gives
    assert t["mean"][0, 1] == (1 + 4 + 7 + 10) / 4 and t["flags"][0, 1] == 0
    a[0, 2, 2] = NAN
    t = R.table(a.reshape(8, 3), 2, 4, probs=(0.5,))
    assert np.isnan(t["ll_max"][0]) and t["ll_max_chain"][0] == -1 and t["ll_max_chain"][1] == 2


# ---- the geometry -----------------------------------------------------------------------------------------------------------------
def test_geometry_moments_tiles():
    g = E.debug_steptable_geometry
    a = g(15, 3, 17)
    assert (a["block"], a["moments_tile_cols"], a["moments_stride_chains"], a["moments_col_tiles"], a["moments_workgroups"]) == \
        (256, 15, 17, 1, 6)
    b, c = g(16, 3, 17), g(17, 3, 17)
    assert (b["moments_tile_cols"], b["moments_stride_chains"], b["moments_col_tiles"], b["moments_workgroups"]) == (16, 16, 1, 6)
    assert (c["moments_tile_cols"], c["moments_col_tiles"], c["moments_workgroups"]) == (16, 2, 9)
    assert g(1, 1, 1)["moments_stride_chains"] == 256 and g(256, 2, 3)["moments_col_tiles"] == 16
    assert a["moments_lds_bytes"] == 256 * 8 + 2 * 16 * 4


@pytest.mark.parametrize("nprobs,width", [(1, 16), (2, 15), (3, 10), (4, 7), (5, 6), (6, 5), (7, 4), (8, 3)])
def test_geometry_select_tile_narrows_with_the_slots(nprobs, width):
    """1 KiB per (column, target rank) and 63 KiB of bins: min(np, 16, 63 // (2 nprobs)) columns per tile"""
    g = E.debug_steptable_geometry(40, 5, 9, nprobs)
    assert g["select_slots"] == 2 * nprobs and g["select_tile_cols"] == width and g["select_stride_chains"] == 256 // width
    assert g["select_col_tiles"] == -(-40 // width) and g["select_workgroups"] == 5 * (g["select_col_tiles"] + 1)
    assert g["select_lds_bytes"] == width * 2 * nprobs * 1024 + 1024 <= 65536
    at, over = E.debug_steptable_geometry(width, 5, 9, nprobs), E.debug_steptable_geometry(width + 1, 5, 9, nprobs)
    assert at["select_col_tiles"] == 1 and at["select_tile_cols"] == width
    assert over["select_col_tiles"] == 2 and over["select_tile_cols"] == width


def test_geometry_no_select_without_probabilities():
    g = E.debug_steptable_geometry(5, 7, 9, 0)
    assert (g["select_slots"], g["select_tile_cols"], g["select_workgroups"], g["select_lds_bytes"]) == (0, 0, 0, 0)
    assert g["scratch_doubles"] == 7 * 6 * 4 and E.debug_steptable_geometry(5, 7, 9, 3)["scratch_doubles"] == 7 * 6 * 7


@pytest.mark.parametrize("np_,G,V", [(1, 2, 1), (3, 4, 1), (15, 16, 1), (16, 32, 1), (40, 64, 1), (63, 64, 1), (64, 64, 2), (128, 64, 3),
                                     (192, 64, 4), (256, 64, 5)])
def test_geometry_row_groups_and_chunks(np_, G, V):
    """section 16's grouping; min(32, ceil(nc / chains per pass)) workgroups per step"""
    cpw = 256 // G
    g = E.debug_steptable_geometry(np_, 7, 1000)
    assert (g["rows_lanes_per_chain"], g["rows_values_per_lane"], g["rows_chains_per_pass"]) == (G, V, cpw)
    c = E.debug_chains_geometry(np_, 7, 1000)
    assert (c["rows_lanes_per_chain"], c["rows_values_per_lane"]) == (G, V)
    assert g["rows_chunks"] == min(32, -(-1000 // cpw)) and g["rows_workgroups"] == 7 * g["rows_chunks"]
    assert E.debug_steptable_geometry(np_, 7, cpw)["rows_chunks"] == 1 and E.debug_steptable_geometry(np_, 7, cpw + 1)["rows_chunks"] == 2
    assert E.debug_steptable_geometry(np_, 7, 32 * cpw)["rows_chunks"] == 32 and E.debug_steptable_geometry(np_, 7, 32 * cpw + 1)["rows_chunks"] == 32
    assert g["scratch_words"] == 7 * 2 * (g["rows_chunks"] + 1)


def test_geometry_refusals():
    for a in ((0, 1, 1, 1), (257, 1, 1, 1), (4, 0, 1, 1), (4, 1, 0, 1), (4, 1, 1, -1), (4, 1, 1, 9)):
        with pytest.raises(McxError) as ei:
            E.debug_steptable_geometry(*a)
        assert ei.value.code == 1
    assert load().mcx_debug_steptable_geometry(4, 1, 1, 1, None) == 1


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_arguments_refused_before_a_device_is_touched():
    """MCX_ERR_INVALID (1), not MCX_ERR_NO_DEVICE (2), and the entry named"""
    L = load()
    rows = np.zeros((8, 3), np.float32)
    fp = rows.ctypes.data_as(C.POINTER(C.c_float))
    cols, steps, q = np.zeros((2, 3), E.STEP_COL_DTYPE), np.zeros(2, E.STEP_ROW_DTYPE), np.zeros((2, 3, 8))
    cp, sp, qp = cols.ctypes.data_as(C.c_void_p), steps.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.POINTER(C.c_double))
    dp = C.POINTER(C.c_double)
    probs = np.array([0.1, 0.5, 0.9])
    pp = probs.ctypes.data_as(dp)
    err = L.mcx_last_error
    assert L.mcx_rows_step_table(fp, 2, 4, 2, pp, 3, None, sp, qp) == 1 and b"cols or steps is NULL" in err()
    assert L.mcx_rows_step_table(fp, 2, 4, 2, pp, 3, cp, None, qp) == 1 and b"cols or steps is NULL" in err()
    assert L.mcx_rows_step_table(fp, 0, 4, 2, pp, 3, cp, sp, qp) == 1 and b"at least one step" in err()
    assert L.mcx_rows_step_table(fp, 2, 4, 2, pp, 9, cp, sp, qp) == 1 and b"nprobs = 9" in err()
    assert L.mcx_rows_step_table(fp, 2, 4, 2, pp, -1, cp, sp, qp) == 1 and b"nprobs = -1" in err()
    assert L.mcx_rows_step_table(fp, 2, 4, 2, None, 3, cp, sp, qp) == 1 and b"probs is NULL" in err()
    assert L.mcx_rows_step_table(fp, 2, 4, 2, pp, 3, cp, sp, None) == 1 and b"quantiles is NULL" in err()
    for k, bad in ((0, -0.01), (1, NAN), (2, 1.5), (2, INF)):
        p2 = probs.copy()
        p2[k] = bad
        assert L.mcx_rows_step_table(fp, 2, 4, 2, p2.ctypes.data_as(dp), 3, cp, sp, qp) == 1
        assert ("probs[%d] = " % k).encode() in err() and b"[0, 1]" in err()
    assert L.mcx_samples_step_table(None, 0, 2, pp, 3, cp, sp, qp) == 1 and b"engine is NULL" in err()
    assert L.mcx_store_step_table(None, pp, 3, cp, sp, qp) == 1 and b"store s is NULL" in err()
    assert L.mcx_debug_step_table_times(None, 0, 2, pp, 3, None) == 1
    with pytest.raises(McxError) as ei:
        E.rows_step_table(rows, 2, 4, probs=(0.5, 2.0))
    assert ei.value.code == 1 and "probs[1] = 2" in str(ei.value)
    with pytest.raises(McxError) as ei:
        E.rows_step_table(rows, 2, 4, probs=np.linspace(0, 1, 9))
    assert ei.value.code == 1 and "nprobs = 9" in str(ei.value)


# ---- the settle rule --------------------------------------------------------------------------------------------------------------
def planted_table(T=40, ncol=3, seed=3):
    """a table as the device would return it: step means within 0.02 sd of (0, 1, 2), sds within 2 % of 1"""
    rng = np.random.default_rng(seed)
    return dict(mean=np.arange(ncol) + 0.02 * rng.uniform(-1, 1, (T, ncol)), sd=1.0 + 0.02 * rng.uniform(-1, 1, (T, ncol)),
                min=np.full((T, ncol), -3, np.float32), max=np.full((T, ncol), 3, np.float32), flags=np.zeros((T, ncol), np.int32))


def check_settle(t, **kw):
    got, want = E.settle_steps(t, **kw), R.settle(t, **kw)
    assert got[0] == want[0], (got[0], want[0])
    for name in want[1]:
        a, b = got[1][name], want[1][name]
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(b)], b[~np.isnan(b)]), (name, a, b)  # the same operations
    return got


def test_settle_every_step_in_band():
    s, c = check_settle(planted_table())
    assert s == 0 and (c["last_out"] == -1).all() and (c["max_dev_mean"] < 0.1).all() and (c["max_dev_sd"] < 0.1).all()
    np.testing.assert_allclose(c["m_ref"], [0, 1, 2], atol=0.02)


@pytest.mark.parametrize("k", [0, 7, 19])
def test_settle_a_drift_that_ends_at_step_k(k):
    t = planted_table()
    t["mean"][:k + 1, 1] += np.linspace(3.0, 0.5, k + 1)  # still 0.5 sd off at step k, in band from k + 1 on
    s, c = check_settle(t)
    assert s == k + 1 and c["last_out"].tolist() == [-1, k, -1] and c["max_dev_mean"][1] > 2.9
    t = planted_table()
    t["sd"][:k + 1, 2] *= 1.5  # the spread alone
    s, c = check_settle(t)
    assert s == k + 1 and c["last_out"].tolist() == [-1, -1, k] and 0.4 < c["max_dev_sd"][2] < 0.6


def test_settle_a_drift_that_reaches_into_the_window():
    t = planted_table()
    t["mean"][:25, 0] += 1.0  # T = 40, the window is steps 20 .. 39
    s, c = check_settle(t)
    assert s == -1 and c["last_out"][0] >= 20
    s, c = check_settle(t, ref_frac=0.25)  # the window is steps 30 .. 39: settled at 25
    assert s == 25 and c["last_out"].tolist() == [24, -1, -1]
    s, _ = check_settle(t, ref_frac=0.375)  # steps 25 .. 39: the first step the rule may name
    assert s == 25
    s, _ = check_settle(t, ref_frac=0.4)
    assert s == -1


def test_settle_use_col_hides_the_drifting_column():
    t = planted_table()
    t["mean"][:30, 2] += 5.0
    assert check_settle(t)[0] == -1
    s, c = check_settle(t, use_col=[1, 1, 0])
    assert s == 0 and np.isnan(c["m_ref"][2]) and np.isnan(c["max_dev_sd"][2]) and c["last_out"][2] == -1
    with pytest.raises(ValueError):
        E.settle_steps(t, use_col=[1, 0])
    with pytest.raises(McxError) as ei:
        E.settle_steps(t, use_col=[0, 0, 0])
    assert ei.value.code == 1 and "use_col names none" in str(ei.value)


def test_settle_non_finite_steps():
    t = planted_table()
    t["mean"][4, 1] = NAN
    t["sd"][4, 1] = NAN
    s, c = check_settle(t)
    assert s == 5 and c["last_out"].tolist() == [-1, 4, -1] and np.isfinite(c["max_dev_mean"]).all()
    t["sd"][33, 0] = INF  # inside the window: s_ref is not finite
    s, c = check_settle(t)
    assert s == -1 and np.isinf(c["s_ref"][0]) and np.isnan(c["max_dev_mean"][0])
    # one chain: every sd is NaN
    t = planted_table()
    t["sd"][:] = NAN
    s, c = check_settle(t)
    assert s == -1 and np.isnan(c["s_ref"]).all() and (c["last_out"] == 39).all()
    # a constant column: s_ref = 0
    t = planted_table()
    t["sd"][:, 1] = 0.0
    assert check_settle(t)[0] == -1 and check_settle(t, use_col=[1, 0, 1])[0] == 0


def test_settle_tolerances_and_window_of_one():
    t = planted_table(T=1)
    assert check_settle(t)[0] == 0
    t = planted_table(T=2)
    t["mean"][0, 0] = 7.0
    assert check_settle(t)[0] == 1 and check_settle(t, ref_frac=1.0)[0] == -1
    t = planted_table()
    assert check_settle(t, tol_mean=0.0, tol_sd=0.0)[0] == -1  # nothing equals the window's mean
    assert check_settle(t, tol_mean=INF, tol_sd=INF)[0] == 0


def test_settle_refusals():
    L = load()
    cols, out, s = np.zeros((2, 3), E.STEP_COL_DTYPE), np.zeros(3, E.STEP_SETTLE_DTYPE), C.c_int(0)
    cols["sd"] = 1.0
    cp, op = cols.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    good = StepRule(0.1, 0.1, 0.5, None)
    assert L.mcx_steps_settle(2, 3, cp, C.byref(good), op, C.byref(s)) == 0 and s.value == 0
    for r, text in ((StepRule(-1.0, 0.1, 0.5, None), b"tol_mean = -1"), (StepRule(0.1, NAN, 0.5, None), b"tol_sd = nan"),
                    (StepRule(0.1, 0.1, 0.0, None), b"ref_frac = 0"), (StepRule(0.1, 0.1, 1.01, None), b"ref_frac = 1.01"),
                    (StepRule(0.1, 0.1, NAN, None), b"ref_frac = nan")):
        assert L.mcx_steps_settle(2, 3, cp, C.byref(r), op, C.byref(s)) == 1 and text in L.mcx_last_error(), L.mcx_last_error()
    for T, ncol in ((0, 3), (2, 0), (-1, 3)):
        assert L.mcx_steps_settle(T, ncol, cp, C.byref(good), op, C.byref(s)) == 1 and b"at least one step" in L.mcx_last_error()
    for args in ((None, C.byref(good), op, C.byref(s)), (cp, None, op, C.byref(s)), (cp, C.byref(good), None, C.byref(s)),
                 (cp, C.byref(good), op, None)):
        assert L.mcx_steps_settle(2, 3, *args) == 1 and b"is NULL" in L.mcx_last_error()


# ---- the header and the host code on their own -------------------------------------------------------------------------------------
def test_header_is_plain_c99_with_the_step_declarations(tmp_path):
    src = tmp_path / "steps_cabi.c"
    src.write_text('#include "mcx.h"\n'
                   'int main(void){ mcx_step_col c[4]; mcx_step_row r[2]; mcx_step_settle_col o[2]; int settled = -7, i;\n'
                   ' mcx_step_rule rule = {0.1, 0.1, 0.5, 0}; mcx_steptable_geometry g; double p[1] = {0.5}, q[4];\n'
                   ' for (i = 0; i < 4; ++i) { c[i].mean = i % 2; c[i].sd = 1.0; c[i].min = -1.0f; c[i].max = 1.0f; c[i].flags = 0; c[i].reserved = 0; }\n'
                   ' r[0].moved = -1; r[0].ll_max = 0.0f; r[0].ll_max_chain = 0; r[0].flags = 0; r[1] = r[0];\n'
                   ' if (mcx_steps_settle(2, 2, c, &rule, o, &settled) != MCX_OK) return 2;\n'
                   ' if (settled != 0 || o[1].m_ref != 1.0 || o[1].s_ref != 1.0 || o[0].last_out != -1) return 3;\n'
                   ' if (mcx_debug_steptable_geometry(17, 3, 5, 8, &g) != MCX_OK || g.select_tile_cols != 3 || g.moments_col_tiles != 2) return 4;\n'
                   ' if (mcx_rows_step_table(0, 1, 1, 1, p, 1, c, r, q) != MCX_ERR_INVALID) return 5;\n'
                   ' if (mcx_rows_step_table((const float *)q, 1, 1, 1, p, 9, c, r, q) != MCX_ERR_INVALID) return 5;\n'
                   ' if (sizeof(mcx_step_col) != 32 || sizeof(mcx_step_row) != 16 || sizeof(mcx_step_settle_col) != 40) return 6;\n'
                   ' if (MCX_STEP_MAX_PROBS != 8) return 7;\n'
                   ' return mcx_abi_version() == MCX_ABI_VERSION && MCX_ABI_VERSION == 5 ? 0 : 1; }\n')
    exe = tmp_path / "steps_cabi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", os.path.join(ROOT, "mcpar_amd"), "-lmcx",
                           "-Wl,-rpath," + os.path.join(ROOT, "mcpar_amd")])
    assert subprocess.call([str(exe)]) == 0


def test_host_code_under_sanitizers(tmp_path):
    """tests/cpp/steps_settle_check.cc: the host half (csrc/mcx_steptable_host.hpp, what mcx_steps_settle is made of) as a
    stand-alone program under AddressSanitizer and UBSan"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "steps_settle_check"
    b = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", ROOT,
                        os.path.join(ROOT, "tests", "cpp", "steps_settle_check.cc"), "-o", str(exe)], capture_output=True, timeout=300)
    if b.returncode != 0 and b"cannot find" in b.stderr and (b"asan" in b.stderr or b"ubsan" in b.stderr):
        pytest.skip("the host compiler has no sanitizer runtimes")
    assert b.returncode == 0, b.stderr.decode()
    r = subprocess.run([str(exe)], capture_output=True, timeout=60)
    assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()
    assert b"steps_settle_check ok" in r.stdout
