"""Profile likelihoods of the sample store, everything that needs no GPU: the restatement
tests/profile_ref.py against a brute-force loop, the hull and the intervals on hand-made curves, the levels, the host entry
points of the library against the restatement, the refusals through the C ABI, the host half on its own (plain and under
AddressSanitizer and UBSan), and the statistical sanity of the definition on the restatement alone."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import profile_ref as R
from mcpar_amd import McxError
from mcpar_amd import engine as E
from mcpar_amd._lib import Profile2dSpecC, ProfileGeometry, ProfileSpecC, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mcx_samples_profile", "mcx_rows_profile", "mcx_store_profile", "mcx_samples_profile2d", "mcx_rows_profile2d",
                "mcx_store_profile2d", "mcx_profile_interval", "mcx_profile_drop", "mcx_debug_profile_finish", "mcx_debug_rows_profile_bins",
                "mcx_debug_profile_geometry", "mcx_debug_profile_times", "mcx_debug_store_profile_times", "mcx_debug_profile2d_times")


def test_entry_points_are_declared_and_exported_and_the_abi_is_5():
    L = load()
    header = open(os.path.join(ROOT, "include", "mcx.h")).read()
    for name in ENTRY_POINTS:
        assert getattr(L, name).argtypes is not None, name
        assert "int %s(" % name in header, name
    for name in ("mcx_profile_spec", "mcx_col_profile", "mcx_profile_interval_t", "mcx_profile2d_spec", "mcx_pair_profile", "mcx_profile_geometry"):
        assert "} %s;" % name in header, name
    assert L.mcx_abi_version() == 5 and "#define MCX_ABI_VERSION 5" in header
    assert C.sizeof(ProfileSpecC) == 64 and C.sizeof(Profile2dSpecC) == 80 and C.sizeof(ProfileGeometry) == 18 * 8
    assert (E.PROFILE_LL_NONFINITE, E.PROFILE_OPEN_LO, E.PROFILE_OPEN_HI, E.PROFILE_NO_BIN, E.PROFILE_HULL_OPEN_LO, E.PROFILE_HULL_OPEN_HI) == \
        (R.LL_NONFINITE, R.OPEN_LO, R.OPEN_HI, R.NO_BIN, R.HULL_OPEN_LO, R.HULL_OPEN_HI) == (2, 4, 8, 16, 32, 64)
    assert E.PROFILE_INTERVAL_DTYPE == R.INTERVAL_DTYPE and E.PROFILE_MAX_LEVELS == R.MAX_LEVELS == 8
    text = open(os.path.join(ROOT, "mcpar_amd", "csrc", "mcx_profile_host.hpp")).read()
    assert "hip" not in text.replace("mcx_profile.hip", "").replace("No HIP", "").lower().replace("__hipcc__", "")


# ---- the restatement against a brute-force loop ------------------------------------------------------------------------------------
def small_rows(seed, N=200, np_=2):
    """values and log L from small integers, so that ties and exact comparisons mean something"""
    rng = np.random.default_rng(seed)
    rows = np.empty((N, np_ + 1), np.float32)
    rows[:, :np_] = rng.integers(-6, 7, (N, np_)) * 0.25
    rows[:, np_] = rng.integers(-4, 4, N) * 0.5
    return rows


def test_key_order():
    ls = np.array([-np.inf, -3e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 2.5, 3e38, np.inf], np.float32)
    k = R.ll_key(ls)
    assert (np.diff(k.astype(np.int64)) > 0).all()                       # -0 before +0, the infinities at the ends
    assert np.array_equal(R.key_ll(k).view(np.uint32), ls.view(np.uint32))
    nan = np.array([np.nan, -np.nan], np.float32)
    assert (R.ll_key(nan) == R.ll_key(np.float32(-np.inf))).all()        # a NaN counts as -inf
    K = R.row_keys(np.array([1.0, 2.0, 2.0, np.nan, -np.inf], np.float32))
    assert int(R.key_row(K.max())) == 1 and (K != 0).all()               # the first row on ties
    assert int(R.key_row(K[3:].max())) == 3 and R.key_lmax(K[3]) == -np.inf
    assert int(R.key_row(np.uint64(0))) == -1 and R.key_lmax(np.uint64(0)) == -np.inf


@pytest.mark.parametrize("seed,bins,f,t", [(0, 7, None, None), (1, 2, None, None), (2, 12, -0.8, 0.9), (3, 5, 0.25, 0.25), (4, 64, -1.25, 1.375)])
def test_bins_of_the_restatement_against_a_loop(seed, bins, f, t):
    rows = small_rows(seed)
    if seed == 0:
        rows[::7, 2] = np.nan
        rows[::11, 2] = -np.inf
        rows[::13, 2] = np.inf
        rows[3, 2], rows[4, 2] = -0.0, 0.0
    v, ll = rows[:, 0], rows[:, 2]
    g = R.grid_of(v, bins, from_=f, to=t)
    ib = R.bins_of(v, bins, *g)
    keys, cnt = R.max_keys(ib, R.row_keys(ll), bins)
    bcnt, best = R.brute_bins(v, ll, bins, g[0], g[1])
    assert cnt.tolist() == bcnt and R.key_row(keys).tolist() == best
    assert int((ib < 0).sum()) == len(v) - sum(bcnt)
    if f is None:
        assert (ib >= 0).all() and ib[v == v.max()].min() == bins - 1    # v == to goes to the last bin
    elif f == t:
        assert set(ib[v == f]) == {0} and (ib[v != f] == -1).all()      # to == from: bin 0, everything else dropped
    else:
        assert (ib[(v < f) | (v > t)] == -1).all() and (ib < 0).any()    # both ends drop values
    lm = R.key_lmax(keys)
    for j, r in enumerate(best):
        want = -np.inf if r < 0 or np.isnan(ll[r]) else ll[r]
        assert np.float32(lm[j]).view(np.uint32) == np.float32(want).view(np.uint32)


def test_quantiles_and_the_clip_pair():
    v = np.arange(101, dtype=np.float32)
    f, t, inv = R.grid_of(v, 10, clip=(0.1, 0.95))
    assert (f, t) == (10.0, 95.0) and inv == 10 / 85.0
    s = np.sort(np.random.default_rng(5).normal(size=777).astype(np.float32))
    for p in (0.0, 0.013, 0.5, 0.987, 1.0):
        assert abs(R.quantile7(s, p) - np.quantile(s.astype(np.float64), p)) < 1e-12


# ---- the hull ------------------------------------------------------------------------------------------------------------------------
def rand_curve(seed, n=40):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.choice(np.arange(400), n, replace=False)) * 0.125
    y = -rng.integers(0, 60, n) * 0.25
    x[rng.random(n) < 0.2] = np.nan
    y[rng.random(n) < 0.1] = -np.inf
    return x, y


@pytest.mark.parametrize("seed", range(6))
def test_hull_majorises_and_is_concave(seed):
    x, y = rand_curve(seed)
    h = R.hull(x, y)
    live = ~np.isnan(x) & np.isfinite(y)
    assert np.isnan(h[np.isnan(x)]).all() and (h[~np.isnan(x) & ~np.isfinite(y)] == -np.inf).all()
    assert (h[live] >= y[live]).all()
    xs, hs = x[live], h[live]
    slopes = np.diff(hs) / np.diff(xs)
    assert (np.diff(slopes) <= 1e-12).all()
    assert hs[0] == y[live][0] and hs[-1] == y[live][-1] and hs.max() == y[live].max()
    # the least one: every vertex is a point of the curve
    vertex = np.concatenate([[True], np.abs(np.diff(slopes)) > 1e-12, [True]])
    assert (hs[vertex] == y[live][vertex]).all()


def test_hull_of_a_concave_curve_is_the_curve():
    x = np.array([0.0, 1.0, 2.5, 3.0, np.nan, 7.0])
    y = np.array([-9.0, -4.0, 0.0, -0.5, -np.inf, -30.0])
    h = R.hull(x, y)
    assert np.array_equal(h[[0, 1, 2, 3, 5]], y[[0, 1, 2, 3, 5]]) and np.isnan(h[4])
    xs = np.linspace(-3, 3, 41)
    assert np.array_equal(R.hull(xs, -0.5 * xs * xs), -0.5 * xs * xs)


# ---- the intervals -------------------------------------------------------------------------------------------------------------------
X9 = np.array([0.0, 1.0, 2.0, np.nan, 4.0, 5.0, 6.0, 7.0, 8.0])
Y9 = np.array([-4.0, -1.0, -3.0, -np.inf, -2.5, 0.0, -np.inf, -1.5, -6.0])


def test_intervals_on_hand_made_curves():
    lo, hi, nseg, op = R.interval(X9, Y9, 2.0)            # two humps and a shoulder: three runs
    assert (lo, hi, nseg, op) == (0.0 + 1.0 * (2.0 / 3.0), 8.0 - 1.0 * (4.0 / 4.5), 3, 0)
    assert R.interval(X9, Y9, 0.5) == (4.0 + 1.0 * (2.0 / 2.5), 5.0, 1, 0)   # the empty bin is skipped; the bin at -inf ends it at xat
    assert R.interval(X9, Y9, 100.0) == (0.0, 8.0, 2, 3)                      # both ends open
    two = np.array([-3.0, -0.25, -3.0, -3.0, 0.0, -3.0])
    assert R.interval(np.arange(6.0), two, 0.5)[2] == 2                      # nseg = 2 on a two-humped curve
    xe, ye = np.array([np.nan, 1.0, np.nan, 3.0]), np.array([-np.inf, -5.0, -np.inf, -4.0])
    lo, hi, nseg, op = R.interval(xe, ye, 1.0)
    assert math.isnan(lo) and math.isnan(hi) and (nseg, op) == (0, 4)
    assert R.interval(xe, ye, 4.5) == (2.0, 3.0, 1, 2)
    lo, hi, nseg, op = R.interval(xe, np.full(4, np.nan), 1.0)
    assert math.isnan(lo) and (nseg, op) == (0, 0)


@pytest.mark.parametrize("seed", range(6))
def test_library_interval_and_finish_equal_the_restatement(seed):
    """mcx_profile_interval and mcx_debug_profile_finish are host code: they run here"""
    x, y = rand_curve(seed)
    y[~np.isnan(x)] -= y[~np.isnan(x)].max()
    for drop in (0.25, 0.5, 2.0, 7.3, 100.0):
        lo, hi, nseg, op = R.interval(x, y, drop)
        glo, ghi, gnseg, gfl = E.profile_interval(x, y, drop)
        assert np.array_equal([lo, hi], [glo, ghi], equal_nan=True) and gnseg == nseg
        assert gfl == (R.OPEN_LO if op & 1 else 0) | (R.OPEN_HI if op & 2 else 0) | (R.NO_BIN if op & 4 else 0)
    for a, b in ((X9, Y9),):
        assert E.profile_interval(a, b, 2.0)[:3] == R.interval(a, b, 2.0)[:3]
    # a column's finish from keys
    rows = small_rows(seed + 10)
    v, ll = rows[:, 1], rows[:, 2]
    n = 9
    g = R.grid_of(v, n)
    K = R.row_keys(ll)
    keys, cnt = R.max_keys(R.bins_of(v, n, *g), K, n)
    keys[3], cnt[3] = 0, 0                                # an empty bin
    row = R.key_row(keys)
    xat = np.where(row >= 0, v[np.maximum(row, 0)], np.float32(7.0)).astype(np.float32)
    for hat in (K.max(), R.row_keys(np.array([np.inf], np.float32))[0]):
        got = E.debug_profile_finish(keys, cnt, xat, hat, drops=(0.5, 1.0, 2.0))
        lmax, lhat = R.key_lmax(keys), R.key_lmax(hat)
        xs = np.where(row >= 0, xat.astype(np.float64), np.nan)
        pl = R.curve(lmax, row, lhat)
        plh = R.hull(xs, pl) if np.isfinite(lhat) else np.full(n, np.nan)
        assert np.array_equal(got["lmax"].view(np.uint32), lmax.view(np.uint32)) and np.array_equal(got["row"], row)
        assert np.array_equal(got["pl"], pl, equal_nan=True) and np.array_equal(got["plh"], plh, equal_nan=True)
        want = R.intervals_of(xs, pl, plh, drops=(0.5, 1.0, 2.0))
        for name in R.INTERVAL_DTYPE.names:
            assert np.array_equal(got["intervals"][name], want[name], equal_nan=True), name
        assert (got["nbinned"], got["nempty"]) == (int(cnt.sum()), int((keys == 0).sum()))
        assert got["flags"] == (0 if np.isfinite(lhat) else R.LL_NONFINITE)


def test_levels():
    assert abs(R.drop_1d(0.6827) - 0.5) < 1e-4 and abs(R.drop_1d(0.9545) - 2.0) < 1e-4
    assert abs(E.profile_drop(0.6827) - 0.5) < 1e-4 and abs(E.profile_drop(0.9545) - 2.0) < 1e-4
    for p in (0.5, 0.6827, 0.9, 0.9545, 0.9973, 0.999999):
        assert abs(E.profile_drop(p) - R.drop_1d(p)) <= 1e-12 * R.drop_1d(p)
    for u in (1e-9, 0.001, 0.0749, 0.075, 0.3, 0.5, 0.8413447, 0.97725, 0.999):   # the three branches, against erfc
        z = R.normal_quantile(u)
        assert abs(0.5 * math.erfc(-z / math.sqrt(2.0)) - u) <= 1e-14 + 4e-16 * abs(z) * u / min(u, 1 - u)
        assert E.profile_drop(p, 2) == -math.log(1.0 - p) == R.drop_2d(p)        # half a chi-square of two: exact
    for bad in (0.0, 1.0, -1.0, np.nan):
        with pytest.raises(McxError):
            E.profile_drop(bad)
    with pytest.raises(McxError):
        E.profile_drop(0.5, 3)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_arguments_refused_before_a_device_is_touched():
    """MCX_ERR_INVALID (1) or MCX_ERR_UNSUPPORTED (4), never MCX_ERR_NO_DEVICE (2)"""
    rows = small_rows(0, 32, 3)

    def code(f, *a, **kw):
        with pytest.raises(McxError) as ei:
            f(*a, **kw)
        return ei.value.code, str(ei.value)

    for f, nb in ((E.rows_profile, "n"), (E.rows_profile2d, "g")):
        for bad in ((1, 513) if nb == "n" else (7, 65)):
            c, msg = code(f, rows, 8, 4, **{nb: bad})
            assert c == 1 and "bins per column" in msg
        for clip in ((0.5, 0.5), (-0.1, 0.9), (0.2, 1.1), (np.nan, 0.5)):
            assert code(f, rows, 8, 4, clip=clip)[0] == 1
        assert code(f, rows, 8, 4, from_=[np.nan, np.inf, np.nan])[0] == 1
        assert code(f, rows, 8, 4, from_=[np.nan, 2.0, np.nan], to=[np.nan, 1.0, np.nan])[0] == 1
        assert code(f, rows, 8, 4, levels=[0.5] * 9)[0] == 1
        for lv in (0.0, 1.0, -0.2, np.nan):
            c, msg = code(f, rows, 8, 4, levels=[0.5, lv])
            assert c == 1 and "levels[1]" in msg
        for d in (0.0, -1.0, np.inf, np.nan):
            assert code(f, rows, 8, 4, drops=[d])[0] == 1
        assert code(f, rows[:1], 1, 1)[0] == 1                                    # one row
        assert code(f, rows, 8, 0)[0] == 1
        c, msg = code(f, rows, 1 << 20, 1 << 12)                                  # 2^32 rows (never read: refused first)
        assert c == 4 and "2^32" in msg
    for pairs in ([[0, 0]], [[0, 3]], [[-1, 1]]):
        assert code(E.rows_profile2d, rows, 8, 4, pairs=pairs)[0] == 1
    assert code(E.rows_profile2d, rows[:, [0, 3]], 8, 4)[0] == 1                  # one column has no pair
    L, err = load(), load().mcx_last_error
    sp, sp2 = E.ProfileSpec(), E.ProfileSpec(two_d=True)
    assert L.mcx_rows_profile(None, 8, 4, 3, C.byref(sp.c), *([None] * 9)) == 1 and b"rows is NULL" in err()
    fp = rows.ctypes.data_as(C.POINTER(C.c_float))
    assert L.mcx_rows_profile(fp, 8, 4, 3, None, *([None] * 9)) == 1 and b"spec is NULL" in err()
    assert L.mcx_rows_profile(fp, 8, 4, 3, C.byref(sp.c), *([None] * 9)) == 1 and b"is NULL" in err()
    assert L.mcx_rows_profile(fp, 8, 4, 257, C.byref(sp.c), *([None] * 9)) == 1 and b"np = 257" in err()
    assert L.mcx_rows_profile2d(fp, 8, 4, 3, C.byref(sp2.c), *([None] * 9)) == 1 and b"is NULL" in err()
    assert L.mcx_samples_profile(None, 0, 8, C.byref(sp.c), *([None] * 9)) == 1 and b"engine is NULL" in err()
    assert L.mcx_samples_profile2d(None, 0, 8, C.byref(sp2.c), *([None] * 9)) == 1 and b"engine is NULL" in err()
    assert L.mcx_store_profile(None, C.byref(sp.c), *([None] * 9)) == 1 and b"store s is NULL" in err()
    assert L.mcx_store_profile2d(None, C.byref(sp2.c), *([None] * 9)) == 1 and b"store s is NULL" in err()
    ms = (C.c_double * 6)()
    assert L.mcx_debug_profile_times(None, 0, 8, C.byref(sp.c), ms) == 1 and L.mcx_debug_store_profile_times(None, C.byref(sp.c), ms) == 1
    assert L.mcx_debug_profile2d_times(None, 0, 8, C.byref(sp2.c), ms) == 1
    assert L.mcx_profile_interval(0, None, None, 1.0, None, None, None, None) == 1
    with pytest.raises(McxError):
        E.profile_interval([0.0, 1.0], [0.0, -1.0], 0.0)
    g = ProfileGeometry()
    assert L.mcx_debug_profile_geometry(3, 8, 4, 64, 32, 1, None) == 1 and L.mcx_debug_profile_geometry(0, 8, 4, 64, 32, 1, C.byref(g)) == 1
    assert L.mcx_debug_profile_geometry(3, 8, 4, 1, 32, 1, C.byref(g)) == 1 and L.mcx_debug_profile_geometry(3, 8, 4, 64, 65, 1, C.byref(g)) == 1


def test_geometry():
    g = E.debug_profile_geometry(1, 300, 300, 512)
    assert (g["block"], g["tile_columns"], g["chains_per_workgroup"], g["chunk_steps"], g["chunks"]) == (256, 1, 256, 256, 2)
    assert g["lds_bytes"] == 12 * 512 and g["chain_blocks"] == 2 and g["workgroups"] == 4
    g = E.debug_profile_geometry(17, 67, 37, 512, g=64, npairs=3)
    assert (g["tile_columns"], g["column_tiles"], g["chains_per_workgroup"], g["chunk_steps"], g["lds_bytes"]) == (8, 3, 32, 2048, 48 * 1024)
    assert g["pair_lds_bytes"] == 48 * 1024 and g["pair_chunks"] == 1 and g["pair_workgroups"] == 3
    g = E.debug_profile_geometry(3, 1 << 12, 1 << 9, 64, npairs=3)
    assert g["pair_chunks"] == 32 and g["pair_workgroups"] == 3 * 32 and g["tile_columns"] == 3 and g["chains_per_workgroup"] == 85


# ---- the header and the host half on their own -----------------------------------------------------------------------------------
def test_header_is_plain_c99_with_the_profile_declarations(tmp_path):
    src = tmp_path / "profile_cabi.c"
    src.write_text('#include "mcx.h"\n'
                   'int main(void){ double x[3] = {0.0, 1.0, 2.0}, y[3] = {-2.0, 0.0, -2.0}, lo, hi, d; int nseg, fl; float rows[6] = {0};\n'
                   ' mcx_profile_spec sp = {64, 0.0, 1.0, 0, 0, 0, 0, 0}; mcx_profile2d_spec s2 = {32, 0.0, 1.0, 0, 0, 0, 0, 0, 0, 0};\n'
                   ' mcx_profile_geometry g;\n'
                   ' if (mcx_profile_interval(3, x, y, 1.0, &lo, &hi, &nseg, &fl) != MCX_OK || lo != 0.5 || hi != 1.5 || nseg != 1 || fl) return 2;\n'
                   ' if (mcx_profile_drop(0.5, 2, &d) != MCX_OK || d <= 0.693 || d >= 0.694) return 3;\n'
                   ' if (mcx_debug_profile_geometry(9, 10, 10, 512, 64, 1, &g) != MCX_OK || g.lds_bytes != 49152 || g.pair_lds_bytes != 49152) return 4;\n'
                   ' if (mcx_rows_profile(rows, 2, 1, 2, &sp, 0, 0, 0, 0, 0, 0, 0, 0, 0) != MCX_ERR_INVALID) return 5;\n'
                   ' if (mcx_store_profile(0, &sp, 0, 0, 0, 0, 0, 0, 0, 0, 0) != MCX_ERR_INVALID) return 6;\n'
                   ' if (mcx_samples_profile2d(0, 0, 2, &s2, 0, 0, 0, 0, 0, 0, 0, 0, 0) != MCX_ERR_INVALID) return 7;\n'
                   ' if (sizeof(mcx_profile_spec) != 64 || sizeof(mcx_profile2d_spec) != 80 || sizeof(mcx_col_profile) != 72) return 8;\n'
                   ' if (sizeof(mcx_profile_interval_t) != 56 || sizeof(mcx_pair_profile) != 24 || sizeof(g) != 144) return 9;\n'
                   ' if (MCX_PROFILE_MAX_LEVELS != 8 || MCX_PROFILE_LL_NONFINITE != 2 || MCX_PROFILE_OPEN_LO != 4 || MCX_PROFILE_NO_BIN != 16) return 10;\n'
                   ' return mcx_abi_version() == MCX_ABI_VERSION && MCX_ABI_VERSION == 5 ? 0 : 1; }\n')
    exe = tmp_path / "profile_cabi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", os.path.join(ROOT, "mcpar_amd"), "-lmcx",
                           "-Wl,-rpath," + os.path.join(ROOT, "mcpar_amd")])
    assert subprocess.call([str(exe)]) == 0


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_host_code_alone(tmp_path, flags):
    """tests/cpp/profile_host_check.cc: the host half (csrc/mcx_profile_host.hpp) as a stand-alone program, plain and under
    AddressSanitizer and UBSan"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "profile_host_check"
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror"] + flags +
                   ["-I", ROOT, os.path.join(ROOT, "tests", "cpp", "profile_host_check.cc"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- the definition itself -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(100, 110))
def test_a_gaussian_gives_wilks_intervals(seed):
    """rows iid N(0, I_2), log L = -|x|^2 / 2 in float, N = 2^16, n = 64: the raw and the hull interval ends at a drop of 1/2 and of
    2 lie within 0.02 of +-1 and +-2 (the worst of these ten seeds: 0.0047).  On the restatement alone: the GPU tests hold the
    library to the restatement, not to the Gaussian"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((1 << 16, 2)).astype(np.float32)
    rows = np.concatenate([x, (-0.5 * (x.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)[:, None]], axis=1)
    o = R.profile(rows, n=64, drops=(0.5, 2.0))
    for c in range(2):
        iv = o["intervals"][c]
        for i, z in enumerate((1.0, 2.0)):
            for name in ("lo", "lo_hull"):
                assert abs(iv[name][i] + z) < 0.02, (c, name, iv[name][i])
            for name in ("hi", "hi_hull"):
                assert abs(iv[name][i] - z) < 0.02, (c, name, iv[name][i])
            assert iv["flags"][i] == 0
        live = o["row"][c] >= 0
        assert (o["plh"][c][live] >= o["pl"][c][live]).all() and o["ndropped"][c] == 0
