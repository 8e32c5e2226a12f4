"""The two-store comparison without a GPU: the restatement tests/compare_ref.py against the counting
definition and against scipy, mcx_ks_prob against scipy's Kolmogorov survival function, the refusals of every entry point (all
before a device is touched) and the launch geometry at both sides of its switches."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import compare_cases as K
import compare_ref as R
from mcpar_amd import McxError
from mcpar_amd import engine as E
from mcpar_amd._lib import CompareSpecC, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
SIZES = [(7, 5), (1000, 777), (4096, 4096), (300, 9000), (1, 1), (5, 5)]


def tied(n, seed, levels):
    rng = np.random.default_rng([seed, n])
    return (np.round(rng.normal(0, 1, n) * levels) / levels).astype(np.float32)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("na, nb, levels", [(1, 1, 4), (5, 5, 2), (7, 5, 4), (40, 23, 8), (64, 64, 1e6)])
def test_restatement_against_the_counting_definition(na, nb, levels):
    a, b = tied(na, 1, levels), tied(nb, 2, levels)
    got, want = R.distances(a, b), R.counting(a, b)
    for f in ("ks_plus_num", "ks_minus_num", "ks_plus_x", "ks_minus_x", "ks"):
        assert got[f] == want[f], (f, got[f], want[f])
    assert got["w1"] == pytest.approx(want["w1"], rel=1e-13, abs=0)


def test_restatement_of_the_order():
    """-0 and +0 one point, the infinities end points, every NaN one point that sorts last"""
    a = np.array([-0.0, -0.0, 1.0], np.float32)
    b = np.array([0.0, 0.0, 1.0], np.float32)
    r = R.distances(a, b)
    assert (r["ks_plus_num"], r["ks_minus_num"], r["ks"], r["w1"]) == (0, 0, 0.0, 0.0)
    a = np.array([-INF, 0.0, NAN, NAN], np.float32)
    b = np.array([0.0, INF, 1.0, 2.0], np.float32)
    r = R.distances(a, b)
    # cA - cB over -inf, 0, 1, 2, inf, NaN: 1, 1, 0, -1, -2, 0 (times 4)
    assert (r["ks_plus_num"], r["ks_plus_x"]) == (4, -INF) and (r["ks_minus_num"], r["ks_minus_x"]) == (8, INF) and r["ks"] == 0.5
    assert math.isnan(r["w1"])
    r = R.distances(np.array([NAN], np.float32), np.array([1.0], np.float32))
    assert (r["ks_plus_num"], r["ks_minus_num"]) == (0, 1) and math.isnan(r["ks_plus_x"]) and r["ks_minus_x"] == 1.0


@pytest.mark.parametrize("na, nb", SIZES)
@pytest.mark.parametrize("levels", [8, 1e6])
def test_restatement_against_scipy(na, nb, levels):
    stats = pytest.importorskip("scipy.stats")
    a, b = tied(na, 3, levels), tied(nb, 4, levels) + np.float32(0.25)
    r = R.distances(a, b)
    assert abs(r["ks"] - stats.ks_2samp(a, b).statistic) <= 1e-15
    w = stats.wasserstein_distance(a.astype(np.float64), b.astype(np.float64))
    assert r["w1"] == pytest.approx(w, rel=1e-12, abs=1e-300)


def test_restatement_swap():
    a, b = tied(300, 5, 8), tied(77, 6, 8)
    r, s = R.distances(a, b), R.distances(b, a)
    assert (r["ks_plus_num"], r["ks_plus_x"], r["ks_minus_num"], r["ks_minus_x"]) == (s["ks_minus_num"], s["ks_minus_x"], s["ks_plus_num"],
                                                                                     s["ks_plus_x"])
    assert r["ks"] == s["ks"] and r["w1"] == s["w1"]


def test_a_statement_with_content_holds_for_the_restatement():
    a, b, b15 = K.content_rows()
    c = K.CONTENT
    K.check_content(R.restate(a, c["T"], c["nc"], b, c["T"], c["nc"]), R.restate(a, c["T"], c["nc"], b15, c["T"], c["nc"]))


# ---- mcx_ks_prob ----------------------------------------------------------------------------------------------------------------
LAMBDAS = (0.05, 0.2, 0.3, 1, 1.18, 1.36, 2, 3, 6)


def test_ks_prob_against_scipy():
    special = pytest.importorskip("scipy.special")
    ess = 200.0  # neff = 100
    for lam in LAMBDAS:
        ks = lam / (10.0 + 0.12 + 0.011)
        neff, p = E.ks_prob(ks, ess, ess)
        assert neff == 100.0
        lam_used = R.ks_lambda(ks, neff)
        assert abs(p - special.kolmogorov(lam_used)) <= 1e-12, (lam, p, special.kolmogorov(lam_used))
        assert abs(R.kolmogorov_q(lam_used) - special.kolmogorov(lam_used)) <= 1e-12
        assert abs(lam_used - lam) < 1e-12


def test_ks_prob_against_the_restatement_and_monotone():
    last = 2.0
    for ks in np.linspace(0.0, 1.0, 401):
        neff, p = E.ks_prob(float(ks), 37.5, 410.0)
        want = R.ks_prob(float(ks), 37.5, 410.0)
        assert neff == want[0] and abs(p - want[1]) <= 1e-15 and 0.0 <= p <= 1.0
        assert p <= last, (ks, p, last)
        last = p
    assert E.ks_prob(0.0, 10.0, 10.0) == (5.0, 1.0) and E.ks_prob(1.0, 1e4, 1e4)[1] == 0.0
    neff, p = E.ks_prob(0.3, NAN, 10.0)
    assert math.isnan(neff) and math.isnan(p)


def test_ks_prob_refusals():
    for a in ((-0.1, 1.0, 1.0), (1.5, 1.0, 1.0), (0.5, 0.0, 1.0), (0.5, 1.0, -2.0)):
        with pytest.raises(McxError) as ei:
            E.ks_prob(*a)
        assert ei.value.code == 1
    d = C.c_double(0)
    assert load().mcx_ks_prob(0.5, 1.0, 1.0, None, C.byref(d)) == 1 and load().mcx_ks_prob(0.5, 1.0, 1.0, C.byref(d), None) == 1


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_arguments_refused_before_a_device_is_touched():
    """MCX_ERR_INVALID (1) or MCX_ERR_UNSUPPORTED, never MCX_ERR_NO_DEVICE (2)"""
    L = load()
    err = L.mcx_last_error
    rows = np.zeros((8, 3), np.float32)
    fp = rows.ctypes.data_as(C.POINTER(C.c_float))
    cols = np.zeros(3, E.COMPARE_DTYPE)
    cp = cols.ctypes.data_as(C.c_void_p)
    spec, bad = CompareSpecC(0), CompareSpecC(2)
    assert L.mcx_rows_compare(None, 2, 4, fp, 2, 4, 2, C.byref(spec), cp) == 1 and b"rows_a is NULL" in err()
    assert L.mcx_rows_compare(fp, 2, 4, None, 2, 4, 2, C.byref(spec), cp) == 1 and b"rows_b is NULL" in err()
    assert L.mcx_rows_compare(fp, 2, 4, fp, 2, 4, 2, C.byref(spec), None) == 1 and b"cols is NULL" in err()
    assert L.mcx_rows_compare(fp, 2, 4, fp, 2, 4, 2, C.byref(bad), cp) == 1 and b"spec.flags = 2" in err()
    assert L.mcx_rows_compare(fp, 2, 4, fp, 2, 4, 0, C.byref(spec), cp) == 1 and b"np = 0" in err()
    assert L.mcx_rows_compare(fp, 2, 4, fp, 2, 4, 257, C.byref(spec), cp) == 1 and b"np = 257" in err()
    for a in ((0, 4, 2, 4), (2, 0, 2, 4), (2, 4, 0, 4), (2, 4, 2, -1)):
        assert L.mcx_rows_compare(fp, a[0], a[1], fp, a[2], a[3], 2, C.byref(spec), cp) == 1 and b"at least one step" in err()
    unsupported = 4  # include/mcx.h MCX_ERR_UNSUPPORTED
    assert L.mcx_rows_compare(fp, 65536, 32768, fp, 2, 4, 2, C.byref(spec), cp) == unsupported and b"2^31" in err()
    assert L.mcx_rows_compare(fp, 2, 4, fp, 32768, 65536, 2, C.byref(spec), cp) == unsupported and b"2^31" in err()
    assert L.mcx_store_compare(None, None, C.byref(spec), cp) == 1 and b"store a is NULL" in err()
    assert L.mcx_samples_compare(None, 0, 2, 0, 2, C.byref(spec), cp) == 1 and b"engine is NULL" in err()
    assert L.mcx_samples_compare_store(None, 0, 2, None, C.byref(spec), cp) == 1 and b"engine is NULL" in err()
    assert L.mcx_debug_compare_times(None, 0, 2, 0, 2, C.byref(spec), None) == 1
    with pytest.raises(ValueError):
        E.compare_rows(rows, 2, 4, np.zeros((8, 4), np.float32), 2, 4)
    with pytest.raises(McxError) as ei:
        E.compare_rows(rows, 0, 4, rows, 2, 4)
    assert ei.value.code == 1


# ---- geometry -------------------------------------------------------------------------------------------------------------------
def test_geometry_tiles_and_the_window_switch():
    g = E.debug_compare_geometry(K.TILE, K.TILE + 1, 2)
    assert (g["block"], g["tile_keys"], g["tiles_a"], g["tiles_b"]) == (256, K.TILE, 1, 2)
    assert g["window_lds_keys"] == K.TILE and g["lds_bytes"] == 4 * (K.TILE + 8 + 33) + 256 * 24 and g["lds_bytes"] <= 64 * 1024
    g = E.debug_compare_geometry(1, 2 * K.TILE, 5)
    assert (g["tiles_a"], g["tiles_b"], g["group_cols"]) == (1, 2, 5)
    g = E.debug_compare_geometry(2 * K.TILE + 1, 2 ** 31 - 1, 257)
    assert (g["tiles_a"], g["tiles_b"], g["group_cols"]) == (3, 2 ** 18, 257)
    assert g["scratch_bytes_per_col"] > 4 * (2 * K.TILE + 1 + 2 * (2 ** 31 - 1))


def test_geometry_group_cap(monkeypatch):
    monkeypatch.setenv("MCX_COMPARE_GROUP_COLS", "4")
    assert E.debug_compare_geometry(100, 100, 18)["group_cols"] == 4 and E.debug_compare_geometry(100, 100, 3)["group_cols"] == 3
    monkeypatch.setenv("MCX_COMPARE_GROUP_COLS", "0")
    assert E.debug_compare_geometry(100, 100, 18)["group_cols"] == 1


def test_geometry_refusals():
    for a in ((0, 1, 2), (1, 0, 2), (1, 1, 1), (1, 1, 258)):
        with pytest.raises(McxError) as ei:
            E.debug_compare_geometry(*a)
        assert ei.value.code == 1
    with pytest.raises(McxError) as ei:
        E.debug_compare_geometry(2 ** 31, 1, 2)
    assert ei.value.code == 4
    assert load().mcx_debug_compare_geometry(1, 1, 2, None) == 1


# ---- the header on its own ------------------------------------------------------------------------------------------------------
def test_header_is_plain_c99_with_the_compare_declarations(tmp_path):
    src = tmp_path / "compare_cabi.c"
    src.write_text('#include "mcx.h"\n'
                   'int main(void){ mcx_col_compare c[2]; mcx_compare_spec s = {MCX_COMPARE_IID}; mcx_compare_geometry g; double ne, p;\n'
                   ' if (mcx_ks_prob(0.0, 8.0, 8.0, &ne, &p) != MCX_OK || ne != 4.0 || p != 1.0) return 2;\n'
                   ' if (mcx_debug_compare_geometry(8193, 16400, 2, &g) != MCX_OK || g.tiles_a != 2 || g.tiles_b != 3) return 3;\n'
                   ' if (mcx_rows_compare(0, 1, 1, 0, 1, 1, 1, &s, c) != MCX_ERR_INVALID) return 4;\n'
                   ' if (mcx_store_compare(0, 0, &s, c) != MCX_ERR_INVALID) return 5;\n'
                   ' if (mcx_debug_compare_geometry(2147483648LL, 1, 2, &g) != MCX_ERR_UNSUPPORTED) return 7;\n'
                   ' if (sizeof(mcx_col_compare) != 144 || MCX_COMPARE_NONFINITE_B != 2) return 6;\n'
                   ' return mcx_abi_version() == MCX_ABI_VERSION ? 0 : 1; }\n')
    exe = tmp_path / "compare_cabi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", os.path.join(ROOT, "mcpar_amd"), "-lmcx",
                           "-Wl,-rpath," + os.path.join(ROOT, "mcpar_amd")])
    assert subprocess.call([str(exe)]) == 0


def test_host_code_under_sanitizers(tmp_path):
    """tests/cpp/compare_host_check.cc: the host half (csrc/mcx_compare_host.hpp, what mcx_ks_prob is made of) as a stand-alone
    program under AddressSanitizer and UBSan"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "compare_host_check"
    b = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", ROOT,
                        os.path.join(ROOT, "tests", "cpp", "compare_host_check.cc"), "-o", str(exe)], capture_output=True, timeout=300)
    if b.returncode != 0 and b"cannot find" in b.stderr and (b"asan" in b.stderr or b"ubsan" in b.stderr):
        pytest.skip("the host compiler has no sanitizer runtimes")
    assert b.returncode == 0, b.stderr.decode()
    r = subprocess.run([str(exe)], capture_output=True, timeout=60)
    assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()
    assert b"compare_host_check ok" in r.stdout


def test_distances_without_loops_are_distances():
    """compare_ref.distances_numpy (the reference of the GPU case of millions of values) against distances(): every field the same
    bits, on ties, shared values, non-finite values and signed zeros"""
    for seed in range(5):
        a, b = K.tie_rows(3, 5, 37, seed), K.tie_rows(3, 9, 11, seed + 10, shift=0.25 * (seed % 3))
        if seed == 3:
            a[3, 1], b[5, 1], a[7, 2], b[0, 0], a[1, 0] = np.nan, np.inf, -np.inf, -0.0, 0.0
        for c in range(a.shape[1]):
            want, got = R.distances(a[:, c], b[:, c]), R.distances_numpy(a[:, c], b[:, c])
            assert sorted(want) == sorted(got)
            for k in want:
                assert want[k] == got[k] or (math.isnan(want[k]) and math.isnan(got[k])), (seed, c, k, want[k], got[k])
    one = np.array([1.5], np.float32)
    assert R.distances(one, one) == R.distances_numpy(one, one)
