"""The host half of the chain table: mcx_chains_keep against tests/chains_ref.py, what the entry
points refuse without a device, mcx_debug_chains_geometry on both sides of every size switch it reports, the restatement
itself against numpy's longdouble on an offset series, and the header as C99.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import chains_ref as R
from mcpar_amd import McxError
from mcpar_amd import engine as E
from mcpar_amd._lib import ChainRule, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def fake_table(nc, ncol=3, seed=5):
    """a table as the device would return it: means around 0 with two chains far off in column 1"""
    rng = np.random.default_rng(seed)
    t = dict(mean=rng.normal(0.0, 1.0, (nc, ncol)), sd=np.ones((nc, ncol)), rho1=np.full((nc, ncol), 0.5),
             moves=rng.integers(3, 9, nc).astype(np.int64), longest_stay=rng.integers(1, 4, nc).astype(np.int64),
             ll_max=np.zeros(nc, np.float32), ll_max_step=np.zeros(nc, np.int32), flags=np.zeros(nc, np.int32))
    if nc > 4:
        t["mean"][1, 1] = 40.0
        t["mean"][nc - 1, 1] = -55.0
    return t


def check_against_ref(t, **kw):
    got = E.keep_chains(t, **kw)
    want = R.keep(t, **kw)
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(np.isnan(got[1]), np.isnan(want[1]))
    assert np.array_equal(got[1][~np.isnan(want[1])], want[1][~np.isnan(want[1])]), (got[1], want[1])  # bit for bit: the same operations
    assert np.array_equal(got[2], want[2])
    return got


@pytest.mark.parametrize("nc", [1, 2, 9, 10, 33, 64])
def test_keep_even_and_odd_counts(nc):
    t = fake_table(nc)
    reasons, centre, kept = check_against_ref(t, z=5.0)
    m = t["mean"]
    for c in range(3):
        assert centre[c, 0] == np.median(m[:, c])
    if nc > 4:
        assert reasons[1] == E.CHAIN_OUTLIER and reasons[nc - 1] == E.CHAIN_OUTLIER and kept.size <= nc - 2


def test_keep_scale_zero_flags_exactly_what_differs():
    t = fake_table(9)
    t["mean"][:, 0] = 1.5
    t["mean"][6, 0] = np.nextafter(1.5, 2.0)
    reasons, centre, kept = check_against_ref(t, z=1e300, use_col=[1, 0, 0])
    assert centre[0, 0] == 1.5 and centre[0, 1] == 0.0
    assert reasons.tolist() == [0] * 6 + [E.CHAIN_OUTLIER] + [0] * 2 and kept.tolist() == [0, 1, 2, 3, 4, 5, 7, 8]


def test_keep_z_inf_is_no_outlier_test():
    t = fake_table(10)
    reasons, centre, kept = check_against_ref(t, z=INF)
    assert not reasons.any() and kept.size == 10
    assert centre[1, 0] == np.median(t["mean"][:, 1])  # (the centres are still reported)


def test_keep_use_col():
    t = fake_table(10)
    reasons, centre, _ = check_against_ref(t, z=5.0, use_col=[1, 0, 1])
    assert reasons[1] == 0 and reasons[9] == 0 and np.isnan(centre[1]).all() and not np.isnan(centre[[0, 2]]).any()
    reasons, _, _ = check_against_ref(t, z=5.0, use_col=[0, 1, 0])
    assert reasons[1] == E.CHAIN_OUTLIER and reasons[9] == E.CHAIN_OUTLIER
    with pytest.raises(ValueError):
        E.keep_chains(t, use_col=[1, 0])


def test_keep_stuck_thresholds():
    t = fake_table(4)
    t["moves"][:] = [0, 1, 2, 3]
    t["longest_stay"][:] = [9, 4, 5, 6]
    assert check_against_ref(t, z=INF, min_moves=1, max_stay=0)[0].tolist() == [E.CHAIN_STUCK, 0, 0, 0]
    assert check_against_ref(t, z=INF, min_moves=2, max_stay=0)[0].tolist() == [E.CHAIN_STUCK, E.CHAIN_STUCK, 0, 0]
    assert check_against_ref(t, z=INF, min_moves=0, max_stay=5)[0].tolist() == [E.CHAIN_STUCK, 0, 0, E.CHAIN_STUCK]
    assert check_against_ref(t, z=INF, min_moves=0, max_stay=4)[0].tolist() == [E.CHAIN_STUCK, 0, E.CHAIN_STUCK, E.CHAIN_STUCK]
    assert check_against_ref(t, z=INF, min_moves=0, max_stay=0)[0].tolist() == [0, 0, 0, 0]


def test_keep_stuck_and_outlier_together():
    t = fake_table(10)
    t["moves"][1] = 0
    reasons, _, _ = check_against_ref(t, z=5.0)
    assert reasons[1] == E.CHAIN_STUCK | E.CHAIN_OUTLIER


def test_keep_nonfinite_chain_left_out_of_the_medians():
    t = fake_table(10)
    t["mean"][3, 0] = NAN
    t["sd"][3, 0] = NAN
    t["flags"][3] = E.SUMMARY_NONFINITE
    t["moves"][3] = 0  # (it gets NONFINITE alone all the same)
    t["mean"][3, 2] = 1e6
    reasons, centre, kept = check_against_ref(t, z=5.0)
    assert reasons[3] == E.CHAIN_NONFINITE and 3 not in kept
    assert centre[0, 0] == np.median(np.delete(t["mean"][:, 0], 3))  # nine chains: column 0 without it
    assert centre[2, 0] == np.median(t["mean"][:, 2])  # its finite mean of column 2 takes part there
    # a chain whose flag alone says so
    t2 = fake_table(10)
    t2["flags"][0] = E.SUMMARY_NONFINITE
    assert check_against_ref(t2, z=5.0)[0][0] == E.CHAIN_NONFINITE


def test_keep_refusals():
    L = load()
    cols, rows = np.zeros((2, 3), E.CHAIN_COL_DTYPE), np.zeros(2, E.CHAIN_ROW_DTYPE)
    cp, rp = cols.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p)
    reasons, nk = np.zeros(2, np.int32), C.c_int(0)
    qp = reasons.ctypes.data_as(C.POINTER(C.c_int))
    good = ChainRule(5.0, 1, 0, None)
    assert L.mcx_chains_keep(2, 3, cp, rp, C.byref(good), qp, None, C.byref(nk)) == 0 and nk.value == 0  # (moves 0: both stuck)
    for z in (0.0, -1.0, NAN, -INF):
        assert L.mcx_chains_keep(2, 3, cp, rp, C.byref(ChainRule(z, 1, 0, None)), qp, None, C.byref(nk)) == 1
        assert b"z = " in L.mcx_last_error()
    for nc, ncol in ((0, 3), (-1, 3), (2, 0)):
        assert L.mcx_chains_keep(nc, ncol, cp, rp, C.byref(good), qp, None, C.byref(nk)) == 1
        assert b"at least one chain" in L.mcx_last_error()
    for args in ((None, rp, C.byref(good), qp, None, C.byref(nk)), (cp, None, C.byref(good), qp, None, C.byref(nk)),
                 (cp, rp, None, qp, None, C.byref(nk)), (cp, rp, C.byref(good), None, None, C.byref(nk)),
                 (cp, rp, C.byref(good), qp, None, None)):
        assert L.mcx_chains_keep(2, 3, *args) == 1
        assert b"is NULL" in L.mcx_last_error()
    with pytest.raises(McxError) as ei:
        E.keep_chains(fake_table(3), z=0)
    assert ei.value.code == 1


def test_arguments_refused_before_a_device_is_touched():
    """MCX_ERR_INVALID (1), not MCX_ERR_NO_DEVICE (2)"""
    L = load()
    rows = np.zeros((8, 3), np.float32)
    fp = rows.ctypes.data_as(C.POINTER(C.c_float))
    cols, tab = np.zeros((4, 3), E.CHAIN_COL_DTYPE), np.zeros(4, E.CHAIN_ROW_DTYPE)
    cp, rp = cols.ctypes.data_as(C.c_void_p), tab.ctypes.data_as(C.c_void_p)
    assert L.mcx_rows_chain_table(fp, 2, 4, 2, None, rp) == 1 and b"cols or chains is NULL" in L.mcx_last_error()
    assert L.mcx_rows_chain_table(fp, 2, 4, 2, cp, None) == 1
    assert L.mcx_rows_chain_table(fp, 0, 4, 2, cp, rp) == 1 and b"at least one step" in L.mcx_last_error()
    assert L.mcx_samples_chain_table(None, 0, 2, cp, rp) == 1 and b"engine is NULL" in L.mcx_last_error()
    assert L.mcx_store_chain_table(None, cp, rp) == 1 and b"store s is NULL" in L.mcx_last_error()
    assert L.mcx_debug_chain_table_times(None, 0, 2, None) == 1
    h = C.c_void_p()
    sel = np.array([0, 3, 4], np.int32)
    sp = sel.ctypes.data_as(C.POINTER(C.c_int))
    assert L.mcx_rows_select_chains(fp, 2, 4, 2, sp, 3, C.byref(h)) == 1 and b"chains[2] = 4" in L.mcx_last_error()
    sel[2] = -1
    assert L.mcx_rows_select_chains(fp, 2, 4, 2, sp, 3, C.byref(h)) == 1 and b"chains[2] = -1" in L.mcx_last_error()
    assert L.mcx_rows_select_chains(fp, 2, 4, 2, sp, 0, C.byref(h)) == 1 and b"nsel = 0" in L.mcx_last_error()
    assert L.mcx_rows_select_chains(fp, 2, 4, 2, None, 2, C.byref(h)) == 1
    assert L.mcx_rows_select_chains(fp, 2, 4, 2, sp, 2, None) == 1 and b"chains or out is NULL" in L.mcx_last_error()
    assert L.mcx_rows_select_chains(fp, 0, 4, 2, sp, 2, C.byref(h)) == 1
    assert L.mcx_samples_select_chains(None, 0, 2, sp, 2, C.byref(h)) == 1 and b"engine is NULL" in L.mcx_last_error()
    assert L.mcx_store_select_chains(None, sp, 2, C.byref(h)) == 1 and b"store s is NULL" in L.mcx_last_error()
    assert not h


def test_geometry_refusals():
    for a in ((0, 1, 1, 1), (257, 1, 1, 1), (4, 0, 1, 1), (4, 1, 0, 1), (4, 1, 1, 0)):
        with pytest.raises(McxError) as ei:
            E.debug_chains_geometry(*a)
        assert ei.value.code == 1
    assert load().mcx_debug_chains_geometry(4, 1, 1, 1, None) == 1


def test_geometry_series_tiles():
    """the tiling of k_sum_moments: up to 16 adjacent columns x 256 / columns chains, log L a tile set of its own"""
    g = E.debug_chains_geometry
    assert g(1, 5, 256)["series_tile_cols"] == 1 and g(1, 5, 256)["series_workgroups"] == 1 and g(1, 5, 257)["series_workgroups"] == 2
    assert g(15, 5, 17)["series_tile_cols"] == 15 and g(15, 5, 17)["series_tile_chains"] == 17 and g(15, 5, 17)["series_workgroups"] == 1
    assert g(15, 5, 18)["series_workgroups"] == 2
    a, b = g(16, 5, 16), g(17, 5, 16)
    assert (a["series_tile_cols"], a["series_tile_chains"], a["series_col_tiles"], a["series_workgroups"]) == (16, 16, 1, 1)
    assert (b["series_tile_cols"], b["series_tile_chains"], b["series_col_tiles"], b["series_workgroups"]) == (16, 16, 2, 2)
    assert g(16, 5, 17)["series_workgroups"] == 2 and g(17, 5, 17)["series_workgroups"] == 4
    assert g(256, 5, 3)["series_col_tiles"] == 16
    assert g(3, 5, 256)["series_ll_workgroups"] == 1 and g(3, 5, 257)["series_ll_workgroups"] == 2
    assert a["block"] == 256 and a["lds_bytes"] == 0


@pytest.mark.parametrize("np_,G,V", [(1, 2, 1), (2, 4, 1), (3, 4, 1), (4, 8, 1), (15, 16, 1), (16, 32, 1), (31, 32, 1), (32, 64, 1),
                                     (63, 64, 1), (64, 64, 2), (127, 64, 2), (128, 64, 3), (191, 64, 3), (192, 64, 4),
                                     (255, 64, 4), (256, 64, 5)])
def test_geometry_row_groups(np_, G, V):
    """G = min(64, the power of two >= np + 1) lanes per chain, V = ceil((np + 1) / G) values per lane"""
    g = E.debug_chains_geometry(np_, 7, 1000)
    assert (g["rows_lanes_per_chain"], g["rows_values_per_lane"], g["rows_chains_per_workgroup"]) == (G, V, 256 // G)
    assert G >= min(64, np_ + 1) and G * V >= np_ + 1 and (V == 1 or G * (V - 1) < np_ + 1)
    assert g["rows_workgroups"] == -(-1000 // (256 // G))
    cpw = 256 // G
    assert E.debug_chains_geometry(np_, 7, cpw)["rows_workgroups"] == 1 and E.debug_chains_geometry(np_, 7, cpw + 1)["rows_workgroups"] == 2


def test_geometry_select_paths():
    g = E.debug_chains_geometry
    assert g(3, 5, 7, 2)["select_vec4"] == 0 and g(3, 5, 7, 2)["select_items"] == 5 * 2 * 3 + 5 * 2
    assert g(4, 5, 7, 2)["select_vec4"] == 1 and g(4, 5, 7, 2)["select_items"] == 5 * 2 * 1 + 5 * 2
    assert g(8, 5, 7, 2)["select_items"] == 5 * 2 * 2 + 5 * 2 and g(6, 5, 7, 2)["select_vec4"] == 0
    assert g(4, 8, 7, 16)["select_items"] == 256 and g(4, 8, 7, 16)["select_workgroups"] == 1
    assert g(3, 8, 7, 8)["select_items"] == 256 and g(3, 8, 7, 8)["select_workgroups"] == 1
    assert g(3, 8, 7, 9)["select_workgroups"] == 2 and g(4, 129, 7, 1)["select_workgroups"] == 2


def offset_rows(T, nc, ncol, seed):
    g = np.random.default_rng(seed).standard_normal((T * nc, ncol))
    return (4096.0 + 2.0 ** -6 * g).astype(np.float32)


@pytest.mark.parametrize("T,nc,ncol", [(65, 64, 18), (33, 17, 17), (1000, 3, 2)])
def test_restatement_on_an_offset_series_against_longdouble(T, nc, ncol):
    """|mean| / sd near 2.6e5: the float64 restatement stays inside the tolerances the device is held to (mean and sd rtol
    1e-9, rho1 atol 8 T 2^-53) against numpy's longdouble"""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("numpy's longdouble is float64 here")
    rows = offset_rows(T, nc, ncol, 7)
    t = R.table(rows, T, nc)
    mean, sd, rho1 = R.table_longdouble(rows, T, nc)
    assert 1e5 < np.abs(t["mean"] / t["sd"]).min()
    np.testing.assert_allclose(t["mean"], mean.astype(np.float64), rtol=1e-9, atol=0)
    np.testing.assert_allclose(t["sd"], sd.astype(np.float64), rtol=1e-9, atol=0)
    # rho1: the issue's 8 T 2^-53 is the bound between two float64 evaluations about the SAME float64 mean (the device and the
    # restatement: the sum of T floats of one binade is exact, so their means are the same bits).  longdouble centres on a
    # better mean: m' = m + d with |d| <= 2^-53 |m| moves the numerator by d (c_0 + c_{T-1}) (the interior terms cancel as
    # sum c = 0) and the denominator by T d^2, so against longdouble the bound is wider by 2^-53 |m| (|c_0| + |c_{T-1}|) / ss
    x = rows.reshape(T, nc, ncol).astype(np.float64)
    c = x - t["mean"]
    centring = 2.0 ** -53 * np.abs(t["mean"]) * (np.abs(c[0]) + np.abs(c[-1])) / (c * c).sum(axis=0)
    err = np.abs(t["rho1"].astype(np.longdouble) - rho1).astype(np.float64)
    print("rho1: max error %.3g, 8 T 2^-53 = %.3g, the centring term up to %.3g" % (err.max(), 8 * T * 2.0 ** -53, centring.max()))
    assert (err <= 8 * T * 2.0 ** -53 + centring).all()
    # and what the offset test is there to reject: the plain sum of squares is off by orders of magnitude
    with np.errstate(invalid="ignore"):
        naive = np.sqrt(((x * x).sum(axis=0) - T * t["mean"] ** 2) / (T - 1))
    worst = np.nanmax(np.abs(naive / t["sd"] - 1.0)) if not np.isnan(naive).all() else np.inf
    print("sd from sum x^2: relative error up to %.3g" % worst)
    assert np.isnan(naive).any() or worst > 1e-7  # against the rtol of 1e-9


def test_restatement_planted_rows():
    rows = np.zeros((6 * 3, 3), np.float32)
    a = rows.reshape(6, 3, 3)
    a[:, 0] = [1.0, 2.0, -3.0]                         # chain 0 never moves
    a[:, 1, :2] = [5.0, 6.0]                           # chain 1 moves in log L alone, at steps 2 and 5
    a[:, 1, 2] = [-1.0, -1.0, -0.5, -0.5, -0.5, -0.25]
    a[:, 2] = np.arange(18, dtype=np.float32).reshape(6, 3)
    a[3, 2, 0] = a[2, 2, 0]
    a[3, 2, 1] = a[2, 2, 1]
    a[3, 2, 2] = a[2, 2, 2]                            # chain 2 stays once
    t = R.table(rows, 6, 3)
    assert t["moves"].tolist() == [0, 2, 4] and t["longest_stay"].tolist() == [6, 3, 2]
    assert t["sd"][0].tolist() == [0.0, 0.0, 0.0] and np.isnan(t["rho1"][0]).all()
    assert t["ll_max"].tolist() == [-3.0, -0.25, 17.0] and t["ll_max_step"].tolist() == [0, 5, 5]
    # -0 / +0 is a move and +0 the larger; one NaN pattern repeated is no move
    z = np.zeros((3, 2), np.float32)
    z[1, 1] = -0.0
    t = R.table(z, 3, 1)
    assert t["moves"][0] == 2 and t["ll_max_step"][0] == 0 and t["flags"][0] == 0
    z[:, 0] = NAN
    t = R.table(z, 3, 1)
    assert t["moves"][0] == 2 and t["flags"][0] == 1 and np.isnan(t["mean"][0, 0]) and t["mean"][0, 1] == 0.0
    z[:, 1] = [1.0, NAN, 3.0]
    t = R.table(z, 3, 1)
    assert np.isnan(t["ll_max"][0]) and t["ll_max_step"][0] == -1


def test_header_is_plain_c99_with_the_chain_declarations(tmp_path):
    src = tmp_path / "chains_cabi.c"
    src.write_text('#include "mcx.h"\n'
                   'int main(void){ mcx_chain_col c[2]; mcx_chain_row r[2]; int reasons[2], nkept = -1; double centre[2];\n'
                   ' mcx_chain_rule rule = {5.0, 1, 0, 0}; mcx_chains_geometry g; mcx_store *st = 0; (void)st;\n'
                   ' c[0].mean = 1.0; c[0].sd = 1.0; c[0].rho1 = 0.0; c[1] = c[0]; c[1].mean = 2.0;\n'
                   ' r[0].moves = 3; r[0].longest_stay = 1; r[0].ll_max = 0.0f; r[0].ll_max_step = 0; r[0].flags = 0; r[1] = r[0];\n'
                   ' r[1].moves = 0;\n'
                   ' if (mcx_chains_keep(2, 1, c, r, &rule, reasons, centre, &nkept) != MCX_OK) return 2;\n'
                   ' if (nkept != 1 || reasons[0] != 0 || reasons[1] != MCX_CHAIN_STUCK || centre[0] != 1.5) return 3;\n'
                   ' if (mcx_debug_chains_geometry(64, 3, 5, 2, &g) != MCX_OK || g.rows_values_per_lane != 2) return 4;\n'
                   ' if (mcx_rows_select_chains(0, 1, 1, 1, reasons, 1, &st) != MCX_ERR_INVALID) return 5;\n'
                   ' if (sizeof(mcx_chain_col) != 24 || sizeof(mcx_chain_row) != 32) return 6;\n'
                   ' return mcx_abi_version() == MCX_ABI_VERSION && MCX_ABI_VERSION == 5 ? 0 : 1; }\n')
    exe = tmp_path / "chains_cabi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", os.path.join(ROOT, "mcpar_amd"), "-lmcx",
                           "-Wl,-rpath," + os.path.join(ROOT, "mcpar_amd")])
    assert subprocess.call([str(exe)]) == 0


def test_host_code_under_sanitizers(tmp_path):
    """tests/cpp/chains_keep_check.cc: the host half (csrc/mcx_chains_host.hpp, what mcx_chains_keep is made of) as a
    stand-alone program under AddressSanitizer and UBSan"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "chains_keep_check"
    b = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", ROOT,
                        os.path.join(ROOT, "tests", "cpp", "chains_keep_check.cc"), "-o", str(exe)], capture_output=True, timeout=300)
    if b.returncode != 0 and b"cannot find" in b.stderr and (b"asan" in b.stderr or b"ubsan" in b.stderr):
        pytest.skip("the host compiler has no sanitizer runtimes")
    assert b.returncode == 0, b.stderr.decode()
    r = subprocess.run([str(exe)], capture_output=True, timeout=60)
    assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()
    assert b"chains_keep_check ok" in r.stdout
