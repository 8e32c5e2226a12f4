"""Interval estimates of a store without a GPU: the entry points and the ABI, the refusals of every entry
point (all before a device is touched), the restatement tests/intervals_ref.py against brute force, the host's beta quantile and
ranks against scipy, the launch geometry, a numpy model of the window tiles against the brute-force HDI, the header as C99 and
the host half under sanitizers.

mcx_beta_quantile against scipy.stats.beta.ppf, in ranks |du| (a + b):
  a + b <= 2^24 + 2   bound 1e-3 (a thousandth of a rank: u N goes through floor and ceil); largest seen 6.3e-7
  beyond              bound 1.6e-2 = 4 x the largest seen, 3.98e-3 at p = 0.5, a = b = 2^31 + 1, where the exact answer is 1/2:
                      the library is 1.7e-16 from it, scipy 9.3e-13.  Where mpmath imports, a 50-digit quadrature of the beta
                      density says the same of every case it is asked: the library within 1e-6 of a rank, scipy up to 4e-3."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import intervals_ref as R
from mcpar_amd import McxError
from mcpar_amd import engine as E
from mcpar_amd._lib import IntervalSpecC, IntervalsGeometry, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mcx_samples_intervals", "mcx_rows_intervals", "mcx_store_intervals", "mcx_beta_quantile", "mcx_intervals_quantile_ranks",
                "mcx_debug_intervals_geometry", "mcx_debug_intervals_times")


def test_entry_points_are_declared_and_exported_and_the_abi_is_5():
    L = load()
    header = open(os.path.join(ROOT, "include", "mcx.h")).read()
    for name in ENTRY_POINTS:
        assert getattr(L, name).argtypes is not None, name
        assert "int %s(" % name in header, name
    for name in ("mcx_interval_spec", "mcx_col_intervals", "mcx_col_hdi", "mcx_col_quantile_se", "mcx_intervals_geometry"):
        assert "} %s;" % name in header, name
    assert L.mcx_abi_version() == 5 and "#define MCX_ABI_VERSION 5" in header


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_arguments_refused_before_a_device_is_touched():
    """MCX_ERR_INVALID (1) or MCX_ERR_UNSUPPORTED (4), never MCX_ERR_NO_DEVICE (2)"""
    L = load()
    err = L.mcx_last_error
    rows = np.zeros((16, 3), np.float32)
    fp = rows.ctypes.data_as(C.POINTER(C.c_float))
    cols = np.zeros(3, E.INTERVALS_DTYPE).ctypes.data_as(C.c_void_p)
    hdi = np.zeros((3, 8), E.HDI_DTYPE).ctypes.data_as(C.c_void_p)
    qse = np.zeros((3, 8), E.QUANTILE_SE_DTYPE).ctypes.data_as(C.c_void_p)
    dp = C.POINTER(C.c_double)

    def spec(mass=(0.9,), probs=(0.05, 0.5), nmass=None, nprobs=None, keep=[]):
        m, p = (C.c_double * max(len(mass), 1))(*mass), (C.c_double * max(len(probs), 1))(*probs)
        keep.append((m, p))
        return C.byref(IntervalSpecC(len(mass) if nmass is None else nmass, len(probs) if nprobs is None else nprobs,
                                     C.cast(m, dp) if mass is not None else None, C.cast(p, dp) if probs is not None else None))

    def call(r=fp, a=(4, 4), np_=2, s=None, c=cols, h=hdi, q=qse):
        return L.mcx_rows_intervals(r, a[0], a[1], np_, s or spec(), c, h, q)

    assert call(r=None) == 1 and b"rows is NULL" in err()
    assert call(np_=0) == 1 and call(np_=257) == 1 and b"np = 257" in err()
    assert call(a=(4, 0)) == 1 and b"nc = 0" in err()
    for T in (3, 0, -1):
        assert call(a=(T, 4)) == 1 and b"nsteps >= 4" in err()
    assert L.mcx_rows_intervals(fp, 4, 4, 2, None, cols, hdi, qse) == 1 and b"spec is NULL" in err()
    assert call(c=None) == 1 and b"cols is NULL" in err()
    assert call(h=None) == 1 and b"mass and hdi" in err()
    assert call(q=None) == 1 and b"probs and qse" in err()
    assert call(s=C.byref(IntervalSpecC(1, 0, None, None))) == 1 and b"mass and hdi" in err()
    assert call(s=C.byref(IntervalSpecC(0, 1, None, None))) == 1 and b"probs and qse" in err()
    for bad in (0.0, 1.0, -0.1, 1.5, math.nan):
        assert call(s=spec(mass=(0.5, bad))) == 1 and b"mass[1]" in err()
    for bad in (-0.01, 1.01, math.nan):
        assert call(s=spec(probs=(0.5, bad))) == 1 and b"probs[1]" in err()
    assert call(s=spec(nmass=9)) == 1 and b"nmass = 9" in err()
    assert call(s=spec(nmass=-1)) == 1 and b"nmass = -1" in err()
    assert call(s=spec(nprobs=9)) == 1 and b"nprobs = 9" in err()
    assert call(s=spec(nprobs=-1)) == 1 and b"nprobs = -1" in err()
    assert call(a=(65536, 32768)) == 4 and b"fewer than 2^31" in err()
    # nothing wrong but the rows: either count may be 0, and its arrays NULL
    assert call(r=None, s=C.byref(IntervalSpecC(0, 0, None, None)), h=None, q=None) == 1 and b"rows is NULL" in err()
    # the store and engine forms: a NULL owner
    assert L.mcx_store_intervals(None, spec(), cols, hdi, qse) == 1 and b"store s is NULL" in err()
    assert L.mcx_samples_intervals(None, 0, 4, spec(), cols, hdi, qse) == 1 and b"engine is NULL" in err()
    assert L.mcx_debug_intervals_times(None, 0, 4, spec(), (C.c_double * 12)()) == 1 and b"engine is NULL" in err()
    with pytest.raises(McxError) as ei:
        E.rows_intervals(rows, 4, 4, hdi=(1.0,))
    assert ei.value.code == 1
    # the host-only entry points
    x = C.c_double()
    assert L.mcx_beta_quantile(0.5, 2.0, 2.0, None) == 1
    for p, a, b in ((-0.1, 2, 2), (1.1, 2, 2), (0.5, 0.5, 2), (0.5, 2, 0.99), (0.5, math.inf, 2), (math.nan, 2, 2), (0.5, math.nan, 2)):
        assert L.mcx_beta_quantile(p, a, b, C.byref(x)) == 1 and math.isnan(x.value), (p, a, b)
    k = C.c_longlong()
    assert L.mcx_intervals_quantile_ranks(10, 0.5, 5.0, None, C.byref(x), C.byref(k), C.byref(k)) == 1
    assert L.mcx_intervals_quantile_ranks(0, 0.5, 5.0, C.byref(x), C.byref(x), C.byref(k), C.byref(k)) == 1
    assert L.mcx_intervals_quantile_ranks(10, 1.5, 5.0, C.byref(x), C.byref(x), C.byref(k), C.byref(k)) == 1
    for ess in (math.nan, 0.0, -3.0, math.inf):
        u_lo, u_hi, k_lo, k_hi = E.intervals_quantile_ranks(100, 0.5, ess)
        assert math.isnan(u_lo) and math.isnan(u_hi) and (k_lo, k_hi) == (-1, -1)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def metropolis_column(N, seed, stay=0.7):
    rng = np.random.default_rng([seed, N])
    x = rng.lognormal(0.0, 0.8, N).astype(np.float32)
    for i in range(1, N):
        if rng.random() < stay:
            x[i] = x[i - 1]
    return x


@pytest.mark.parametrize("N", [8, 40, 888])
def test_hdi_against_a_loop_over_every_window(N):
    cols = [metropolis_column(N, 1), np.arange(N, dtype=np.float32) * np.float32(0.25),  # every window ties: the first wins
            np.full(N, 3.5, np.float32), np.where(np.arange(N) % 2, np.float32(-0.0), np.float32(0.0)).astype(np.float32)]
    for c, x in enumerate(cols):
        srt = R.sorted_values(x)
        assert np.array_equal(srt, np.sort(x)) and not np.signbit(srt).any()  # (-0 is reported as +0)
        for p in (1e-9, 0.03, 0.5, 0.9, 0.94, 1 - 1e-12):
            got, want = R.hdi(srt, p), R.hdi_brute([float(v) for v in srt], p)
            assert (float(got[0]), float(got[1]), got[2], got[3], got[4]) == want, (c, p)
            assert got[4] == min(math.floor(p * N), N - 1)
        assert R.hdi(srt, 1e-9)[3:] == (0, 0) and R.hdi(srt, 1 - 1e-12)[3:] == (0, N - 1)
        if c in (1, 2, 3):
            assert all(R.hdi(srt, p)[3] == 0 for p in (0.03, 0.5, 0.9))


def test_the_two_forms_of_mcse_sd_agree():
    """Kenney and Keeping's form on the float32 c2 against posterior's moments in float64.  c2 is rounded to float32, a relative
    2^-24 each; through the variance of c2 (E[c2^2] / Var is 3/2 for a normal column), the root and the division by the mean
    that is 3 2^-24 = 1.8e-7 at the worst.  Seen: 3e-10 on 19 200 values, the roundings averaging out."""
    import summary_ref as S
    T, nc = 48, 400
    rng = np.random.default_rng(5)
    x = rng.normal(1.0, 2.0, (T, nc)).astype(np.float32)
    for t in range(1, T):
        rep = rng.random(nc) < 0.7
        x[t, rep] = x[t - 1, rep]
    r = R.restate_column(x, (), ())
    c2 = ((x.astype(np.float64) - r["mean"]) ** 2).astype(np.float32)
    rc = S.restate_column(c2, ())
    a, b = r["mcse_sd"], R.mcse_sd_posterior(x, rc["ess"])
    print("mcse_sd %.12g against posterior's form %.12g: relative %.3g" % (a, b, abs(a - b) / b))
    assert abs(a - b) <= 2e-7 * b and 0 < r["ess_sd"] < T * nc


# ---- the host half ---------------------------------------------------------------------------------------------------------------
RANK_CASES = [(0.05, 31.0), (0.5, 3793.2), (0.95, 412.7), (0.0, 100.0), (1.0, 57.3), (0.25, 12000.5)]


@pytest.mark.parametrize("N", [40, 888, 8, 19200])
def test_quantile_ranks_against_the_reference(N):
    for prob, ess in RANK_CASES:
        margin = R.rank_margin(N, prob, ess)
        assert margin >= 1e-3, (N, prob, ess, margin)  # scipy's u decides the case: (the library's is within 1e-3 of it, below)
        u_lo, u_hi, k_lo, k_hi = E.intervals_quantile_ranks(N, prob, ess)
        want = R.quantile_ranks(N, prob, ess)
        assert (k_lo, k_hi) == want[2:] and 0 <= k_lo <= k_hi <= N - 1, (N, prob, ess, k_lo, k_hi, want)
        assert abs(u_lo - want[0]) * N < 1e-3 and abs(u_hi - want[1]) * N < 1e-3


BETA_AB = [1.0, 1.5, 2.0, 3.7, 10.0, 100.0, 1e3, 12345.6, 2.0 ** 16, 2.0 ** 20 + 0.5, 2.0 ** 23, 2.0 ** 24 + 1, 2.0 ** 27, 2.0 ** 31 + 1]


def test_beta_quantile_against_scipy():
    from scipy.stats import beta
    worst = {True: (0.0, None), False: (0.0, None)}
    for p in (R.P_LO, R.P_HI, 0.5):
        for a in BETA_AB:
            for b in BETA_AB:
                d = abs(E.beta_quantile(p, a, b) - float(beta.ppf(p, a, b))) * (a + b)
                small = a + b <= 2 ** 24 + 2
                if d > worst[small][0]:
                    worst[small] = (d, (p, a, b))
    print("largest |du| (a + b): %.3g at %s for a + b <= 2^24 + 2, %.3g at %s beyond" % (worst[True] + worst[False]))
    assert worst[True][0] <= 1e-3
    assert worst[False][0] <= 4 * 3.98e-3
    assert E.beta_quantile(0.0, 2.0, 3.0) == 0.0 and E.beta_quantile(1.0, 2.0, 3.0) == 1.0
    assert abs(E.beta_quantile(0.3, 1.0, 1.0) - 0.3) < 1e-15  # the uniform law


def test_beta_quantile_beyond_scipy_against_a_quadrature():
    """whose error the difference beyond a + b = 2^24 is: I_u(a, b) - p by a 50-digit quadrature of the density over 40 standard
    deviations below u, turned into an error of u by the density at u.  The library is held to the thousandth of a rank."""
    mp = pytest.importorskip("mpmath")
    from scipy.stats import beta

    def error_of(u, p, a, b):
        a, b, u = mp.mpf(a), mp.mpf(b), mp.mpf(u)
        lb = mp.loggamma(a) + mp.loggamma(b) - mp.loggamma(a + b)
        dens = lambda x: mp.exp((a - 1) * mp.log(x) + (b - 1) * mp.log(1 - x) - lb)  # noqa: E731
        mu, sg = a / (a + b), mp.sqrt(a * b / ((a + b) ** 2 * (a + b + 1)))
        lo = max(mp.mpf(0), mu - 40 * sg)
        pts = [lo] + [mu + k * sg for k in range(-36, 40, 4) if lo < mu + k * sg < u] + [u]
        return abs(float((mp.quad(dens, pts) - mp.mpf(p)) / dens(u))) * float(a + b)

    with mp.workdps(50):
        for p, a, b in ((R.P_LO, 2.0 ** 24 + 1, 2.0 ** 27), (R.P_LO, 2.0 ** 31 + 1, 2.0 ** 31 + 1), (R.P_HI, 2.0 ** 27, 2.0 ** 31 + 1),
                        (0.5, 2.0 ** 31 + 1, 2.0 ** 31 + 1), (R.P_HI, 2.0 ** 23, 2.0 ** 23)):
            ours, theirs = error_of(E.beta_quantile(p, a, b), p, a, b), error_of(float(beta.ppf(p, a, b)), p, a, b)
            print("p = %g, a = %g, b = %g: the library is %.3g of a rank off, scipy %.3g" % (p, a, b, ours, theirs))
            assert ours <= 1e-3


# ---- the launch geometry ----------------------------------------------------------------------------------------------------------
def test_geometry_on_both_sides_of_every_switch(monkeypatch):
    monkeypatch.delenv("MCX_RANK_GROUP_COLS", raising=False)
    g = E.debug_intervals_geometry(4, 2, 1, 1, 3)
    wt = g["window_tile"]
    assert g["block"] == 256 and wt == 4096 and g["window_tiles"] == 1 and g["sort_tiles"] == 1 and g["grid_y"] == 1
    assert (g["slab_entries"], g["slab_bytes"], g["reduce_workgroups"], g["pick_ranks"], g["transforms"]) == (1, 16, 1, 6, 4)
    assert (g["group_cols"], g["groups"]) == (2, 1) and g["store_scratch_bytes"] == 8 * 2 * 4
    assert E.debug_intervals_geometry(wt // 4, 4, 1)["window_tiles"] == 1 and E.debug_intervals_geometry(wt // 4 + 1, 4, 1)["window_tiles"] == 2
    g = E.debug_intervals_geometry(3 * wt // 4 + 5, 4, 1, 8, 8)
    assert g["window_tiles"] == 4 and g["slab_entries"] == 32 and g["sort_tiles"] == 2 and g["pick_ranks"] == 16 and g["transforms"] == 9
    assert g["scratch_bytes_per_col"] >= 8 * (3 * wt + 20) + g["slab_bytes"]
    g = E.debug_intervals_geometry(24, 37, 17, 0, 0)
    assert (g["slab_entries"], g["reduce_workgroups"], g["pick_ranks"], g["transforms"], g["group_cols"], g["groups"]) == (0, 0, 0, 1, 18, 1)
    assert E.debug_intervals_geometry(64, 3, 2)["grid_y"] == 1 and E.debug_intervals_geometry(65, 3, 2)["grid_y"] == 2
    monkeypatch.setenv("MCX_RANK_GROUP_COLS", "4")
    g = E.debug_intervals_geometry(24, 37, 17)
    assert (g["group_cols"], g["groups"]) == (4, 5)
    monkeypatch.setenv("MCX_RANK_GROUP_COLS", "0")
    assert E.debug_intervals_geometry(24, 37, 17)["group_cols"] == 1
    for a, code in (((3, 2, 1, 1, 1), 1), ((4, 0, 1, 1, 1), 1), ((4, 2, 0, 1, 1), 1), ((4, 2, 257, 1, 1), 1), ((4, 2, 1, 9, 1), 1),
                    ((4, 2, 1, 1, -1), 1), ((65536, 32768, 1, 1, 1), 4)):
        with pytest.raises(McxError) as ei:
            E.debug_intervals_geometry(*a)
        assert ei.value.code == code
    assert load().mcx_debug_intervals_geometry(4, 2, 1, 1, 1, None) == 1
    assert C.sizeof(IntervalsGeometry) == 15 * 8


def tiled_hdi(srt, m, tile, block=256):
    """k_hdi_windows and k_hdi_reduce in numpy: thread t of a workgroup takes the starts base + e * block + t in ascending e and
    keeps its first least w; then the least (bits of w, i) over the threads, then over the tiles"""
    N = srt.size
    s = srt.astype(np.float64)
    ntiles = (N + tile - 1) // tile
    slab = []
    for b in range(ntiles):
        best = (2 ** 64 - 1, 2 ** 63 - 1)
        for t in range(block):
            mine = (2 ** 64 - 1, 2 ** 63 - 1)
            for i in range(b * tile + t, min((b + 1) * tile, N), block):
                if i < N - m:
                    wb = int(np.float64(s[i + m] - s[i]).view(np.uint64))
                    if wb < mine[0]:
                        mine = (wb, i)
            best = min(best, mine)
        slab.append(best)
    wb, i = min(slab)
    return float(np.uint64(wb).view(np.float64)), i


def test_window_tile_model_against_the_brute_force():
    tile = 512  # (the arithmetic is the kernel's at any tile that is a multiple of the block)
    N = 3 * tile + 77
    cols = [np.sort(metropolis_column(N, 3)), np.arange(N, dtype=np.float32)]
    late = np.arange(N, dtype=np.float32) * 2
    late[N - 40:] = late[N - 40] + np.arange(40, dtype=np.float32) * np.float32(0.5)  # the least windows lie in the last tile
    cols.append(late)
    for srt in cols:
        for m in (0, 1, 100, tile - 3, tile + 200, 2 * tile + 9, N - 1):
            _, _, w, i, _ = R.hdi_brute([float(v) for v in srt], (m + 0.5) / N)
            assert tiled_hdi(srt, m, tile) == (w, i), m


# ---- the header and the host half on their own ------------------------------------------------------------------------------------
def test_header_is_plain_c99_with_the_intervals_declarations(tmp_path):
    src = tmp_path / "intervals_cabi.c"
    src.write_text('#include "mcx.h"\n'
                   'int main(void){ double mass[1] = {0.9}, probs[1] = {0.5}, x, ul, uh; long long kl, kh; mcx_interval_spec s = {1, 1, 0, 0};\n'
                   ' mcx_col_intervals c[3]; mcx_col_hdi h[3]; mcx_col_quantile_se q[3]; mcx_intervals_geometry g; s.mass = mass; s.probs = probs;\n'
                   ' if (mcx_beta_quantile(0.5, 4.0, 4.0, &x) != MCX_OK || x < 0.4999999 || x > 0.5000001) return 2;\n'
                   ' if (mcx_intervals_quantile_ranks(888, 0.5, 100.0, &ul, &uh, &kl, &kh) != MCX_OK || kl != 399 || kh != 487) return 3;\n'
                   ' if (mcx_debug_intervals_geometry(4097, 1, 2, 1, 1, &g) != MCX_OK || g.window_tiles != 2) return 4;\n'
                   ' if (mcx_rows_intervals(0, 4, 4, 2, &s, c, h, q) != MCX_ERR_INVALID) return 5;\n'
                   ' if (mcx_store_intervals(0, &s, c, h, q) != MCX_ERR_INVALID) return 6;\n'
                   ' if (sizeof(mcx_col_intervals) != 40 || sizeof(mcx_col_hdi) != 32 || sizeof(mcx_col_quantile_se) != 72 ||\n'
                   '     sizeof(mcx_interval_spec) != 24) return 7;\n'
                   ' if (MCX_INTERVAL_MAX_MASSES != 8 || MCX_INTERVAL_MAX_PROBS != 8 || MCX_INTERVAL_TIMES != 12) return 8;\n'
                   ' return mcx_abi_version() == MCX_ABI_VERSION && MCX_ABI_VERSION == 5 ? 0 : 1; }\n')
    exe = tmp_path / "intervals_cabi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", os.path.join(ROOT, "mcpar_amd"), "-lmcx",
                           "-Wl,-rpath," + os.path.join(ROOT, "mcpar_amd")])
    assert subprocess.call([str(exe)]) == 0
    assert C.sizeof(IntervalSpecC) == 24


def test_host_code_under_sanitizers(tmp_path):
    """tests/cpp/intervals_host_check.cc: the host half (csrc/mcx_intervals_host.hpp: the beta quantile, the ranks, the spans) as a
    stand-alone program under AddressSanitizer and UBSan"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "intervals_host_check"
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", ROOT,
                    os.path.join(ROOT, "tests", "cpp", "intervals_host_check.cc"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_make_rows_without_its_loop_gives_the_loop_s_rows():
    """tests/test_gpu_intervals.py's make_rows (also lagcov_ref.dependent_rows') against its step-by-step definition"""
    from test_gpu_intervals import make_rows, make_rows_loop
    for a in ((1, 2, 4), (3, 5, 8), (17, 37, 24), (6, 2473, 5), (1, 1, 300), (1, 1, 1), (3, 37, 64)):
        assert make_rows(*a).tobytes() == make_rows_loop(*a).tobytes(), a
    assert make_rows(3, 7, 50, seed=13, stay=0.4).tobytes() == make_rows_loop(3, 7, 50, seed=13, stay=0.4).tobytes()
    assert make_rows(2, 3, 40, stay=0.0).tobytes() == make_rows_loop(2, 3, 40, stay=0.0).tobytes()
