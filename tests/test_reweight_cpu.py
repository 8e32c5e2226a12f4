"""Importance weights on a store without a GPU: the restatement tests/reweight_ref.py against a brute-force
definition and against numpy at equal weights, mcx_khat_of_tail against the restatement and against scipy's generalised Pareto
draws, the refusals of every entry point (all before a device is touched), the launch geometry at both sides of its switches
and the header as C99.

mcx_khat_of_tail against the restatement: the same operations in the same order, so only the two libms differ; the bound is 1e-9
and the largest difference seen over the cases below is 0 (both sides call the same libm here)."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import reweight_ref as R
from mcpar_amd import McxError
from mcpar_amd import engine as E
from mcpar_amd._lib import ReweightResultC, WeightsC, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tied_rows(N, ncol, seed):
    """normal rows with ties: column 0 rounded to one decimal, a -0 and a +0 among them"""
    a = np.random.default_rng([seed, N, ncol]).normal(0.0, 1.0, (N, ncol)).astype(np.float32)
    a[:, 0] = np.round(a[:, 0], 1)
    a[0, 0], a[N - 1, 0] = np.float32(-0.0), np.float32(0.0)
    return a


def tied_weights(N, seed):
    """fixed-point weights with zeros, ties and rows of full weight"""
    rng = np.random.default_rng([seed, N])
    q = rng.integers(0, 2 ** 31, N, dtype=np.int64)
    q[rng.random(N) < 0.2] = 0
    q[rng.random(N) < 0.2] = 12345
    q[N // 2] = 2 ** 31
    return q.astype(np.uint32)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [7, 100, 1000])
def test_restatement_against_the_brute_force_definition(N):
    rows, q = tied_rows(N, 3, 1), tied_weights(N, 2)
    probs = (0.0, 1e-12, 0.05, 0.25, 0.5, 0.75, 0.999, 1.0)
    ref = R.restate(rows, q, 0.0, probs)
    qi = [int(v) for v in q]
    Q = sum(qi)
    assert ref["sumq"] == Q and ref["sumq2"] == sum(v * v for v in qi) and ref["nzero"] == qi.count(0)
    assert ref["sumq2"] == (ref["sumq2_hi"] << 64) + ref["sumq2_lo"]
    for c in range(3):
        for k, p in enumerate(probs):
            want = R.brute_quantile(rows[:, c], q, p)
            got = np.float32(ref["quantiles"][c, k])
            assert R.okey([got])[0] == R.okey([want])[0], (c, p)
        x = [float(v) for v in rows[:, c]]
        mean = sum(w * v for w, v in zip(qi, x)) / Q
        var = sum(w * (v - mean) ** 2 for w, v in zip(qi, x)) / Q
        mcse = math.sqrt(sum(w * w * (v - mean) ** 2 for w, v in zip(qi, x))) / Q
        assert ref["cols"]["mean"][c] == pytest.approx(mean, rel=1e-12, abs=1e-15)
        assert ref["cols"]["sd"][c] == pytest.approx(math.sqrt(var), rel=1e-12)
        assert ref["cols"]["mcse_mean"][c] == pytest.approx(mcse, rel=1e-12)
        used = rows[np.asarray(q) > 0, c]
        assert ref["cols"]["min"][c] == used.min() and ref["cols"]["max"][c] == used.max()
    assert ref["ess_kish"] == pytest.approx(Q * Q / ref["sumq2"], rel=1e-15)


@pytest.mark.parametrize("N", [7, 100, 1000])
def test_equal_weights_are_numpy(N):
    rows = tied_rows(N, 2, 3)
    q, lwmax = R.fixed_point(R.log_weights(rows[:, 1], 0.0))
    assert lwmax == 0.0 and np.all(q == 2 ** 31)
    probs = (0.0, 0.05, 0.31, 0.5, 0.95, 1.0)
    ref = R.restate(rows, q, lwmax, probs)
    for c in range(2):
        want = np.quantile(rows[:, c], probs, method="inverted_cdf")
        assert np.array_equal(ref["quantiles"][c], want.astype(np.float64))
        x = rows[:, c].astype(np.float64)
        assert ref["cols"]["mean"][c] == pytest.approx(np.mean(x), rel=1e-13, abs=1e-16)
        assert ref["cols"]["sd"][c] == pytest.approx(np.std(x, ddof=0), rel=1e-13)
    assert ref["ess_kish"] == float(N) and ref["log_mean_w"] == 0.0 and ref["nzero"] == 0


def test_fixed_point_weights():
    lw = np.array([0.0, -math.inf, math.log(0.5), -22.0, -23.0, math.log(2.0 ** -32), math.log(2.0 ** -33)])
    q, lwmax = R.fixed_point(lw + 3.0)
    assert lwmax == 3.0 and q[0] == 2 ** 31 and q[1] == 0 and abs(int(q[2]) - 2 ** 30) <= 1
    assert q[3] == round(2 ** 31 * math.exp(-22.0)) and q[4] == round(2 ** 31 * math.exp(-23.0)) == 0
    assert q[6] == 0  # below 2^-32 of the largest weight: (2^-33 2^31 = 1/4 rounds to 0; 2^-32 is the tie 1/2, to even: 0)
    assert R.first_refused(np.array([0.0, math.nan, math.inf])) == 1 and R.first_refused(lw) is None
    assert R.threshold(0.0, 10) == 1 and R.threshold(1.0, 10) == 10 and R.threshold(0.25, 10) == 3 and R.threshold(1e-30, 10) == 1


def test_draw_r_is_the_library_s_draw_rule():
    """(r N) >> 64 of reweight_ref.draw_r is mcx_debug_draw_indices' index: the same Philox block, the same words"""
    for seed, N in ((0, 1), (7, 444), (20240611, 10 ** 9 + 7)):
        want = E.debug_draw_indices(seed, N, 0, 50)
        got = [(R.draw_r(seed, k) * N) >> 64 for k in range(50)]
        assert list(want) == got
    q = np.full(444, 2 ** 31, np.uint32)
    idx, _ = R.resample_index(q, 7, 300)
    assert np.array_equal(idx, E.debug_draw_indices(7, 444, 0, 300))  # the nested floors agree


# ---- k-hat ----------------------------------------------------------------------------------------------------------------------
def test_khat_of_tail_against_the_restatement():
    worst = 0.0
    for seed, n, k in ((1, 5, 0.3), (2, 44, 0.1), (3, 300, 0.6), (4, 1342, 0.9), (5, 120, -0.3)):
        from scipy.stats import genpareto
        x = np.sort(genpareto(k).rvs(n, random_state=seed))
        got, want = E.khat_of_tail(x), R.khat_of_tail(x)
        assert got[2] == want[2]
        for a, b in zip(got[:2], want[:2]):
            assert abs(a - b) <= 1e-9 * max(1.0, abs(b))
            worst = max(worst, abs(a - b))
    print("largest difference of khat or sigma between the library and the restatement: %g" % worst)


@pytest.mark.parametrize("k", [-0.2, 0.3, 0.8])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_khat_of_tail_recovers_a_generalised_pareto_shape(k, seed):
    from scipy.stats import genpareto
    x = np.sort(genpareto(k).rvs(3000, random_state=seed))
    khat, sigma, flags = E.khat_of_tail(x)
    print("k = %g seed %d: khat = %.4f, sigma = %.4f" % (k, seed, khat, sigma))
    assert abs(khat - k) < 0.06
    assert flags == (R.KHAT_HIGH if khat > 0.7 else 0)


def test_no_tail():
    for x in ([0.1, 0.2, 0.3, 0.4],                 # n = 4
              [0.0] * 5 + [0.1 * i for i in range(1, 11)],  # xstar = x[3] = 0: ties at the cutoff reach a quarter into the tail
              [0.0] * 20):                            # a constant tail: x[n - 1] = 0
        for khat, sigma, flags in (E.khat_of_tail(x), R.khat_of_tail(x)):
            assert math.isnan(khat) and math.isnan(sigma) and flags == R.NO_TAIL
    assert E.khat_of_tail([])[2] == R.NO_TAIL
    for bad in ([0.2, 0.1, 0.3, 0.4, 0.5], [-0.1, 0.1, 0.2, 0.3, 0.4], [0.1, 0.2, 0.3, 0.4, math.nan], [0.1, 0.2, 0.3, 0.4, math.inf]):
        with pytest.raises(McxError) as ei:
            E.khat_of_tail(bad)
        assert ei.value.code == 1
    L = load()
    x = (C.c_double * 5)(0.1, 0.2, 0.3, 0.4, 0.5)
    k, s, f = C.c_double(), C.c_double(), C.c_int()
    assert L.mcx_khat_of_tail(x, 5, None, C.byref(s), C.byref(f)) == 1
    assert L.mcx_khat_of_tail(None, 5, C.byref(k), C.byref(s), C.byref(f)) == 1
    assert L.mcx_khat_of_tail(x, -1, C.byref(k), C.byref(s), C.byref(f)) == 1


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_arguments_refused_before_a_device_is_touched():
    """MCX_ERR_INVALID (1) or MCX_ERR_UNSUPPORTED (4), never MCX_ERR_NO_DEVICE (2)"""
    L = load()
    err = L.mcx_last_error
    rows = np.zeros((8, 3), np.float32)
    fp = rows.ctypes.data_as(C.POINTER(C.c_float))
    logw = np.zeros(8, np.float32)
    res = ReweightResultC()
    cols = np.zeros(3, E.REWEIGHT_DTYPE)
    cp = cols.ctypes.data_as(C.c_void_p)
    quant = (C.c_double * 9)()
    probs = (C.c_double * 3)(0.05, 0.5, 0.95)

    def wt(kind=E.WEIGHT_HOST, lw=logw, store=None, col=0, scale=1.0):
        return C.byref(WeightsC(kind, None if lw is None else lw.ctypes.data_as(C.POINTER(C.c_float)), store, col, scale))

    def rew(r=fp, a=(2, 4), np_=2, w=None, p=probs, n=3, rs=C.byref(res), c=cp, q=quant):
        return L.mcx_rows_reweight(r, a[0], a[1], np_, w or wt(), p, n, rs, c, q)

    assert rew(r=None) == 1 and b"rows is NULL" in err()
    assert rew(np_=0) == 1 and b"np = 0" in err()
    assert rew(np_=257) == 1 and b"np = 257" in err()
    assert rew(rs=None) == 1 and b"res is NULL" in err()
    assert rew(c=None) == 1 and b"cols is NULL" in err()
    assert rew(n=-1) == 1 and b"nprobs = -1" in err()
    assert rew(n=65) == 1 and b"nprobs = 65" in err()
    assert rew(p=None) == 1 and b"probs and quantiles" in err()
    assert rew(q=None) == 1 and b"probs and quantiles" in err()
    for bad in (-0.01, 1.01, math.nan):
        assert rew(p=(C.c_double * 3)(0.05, bad, 0.95)) == 1 and b"probs[1]" in err()
    for a in ((0, 4), (2, 0), (-1, 4)):
        assert rew(a=a) == 1 and b"at least one step" in err()
    assert rew(a=(65536, 32768)) == 4 and b"fewer than 2^31" in err()
    assert L.mcx_rows_reweight(fp, 2, 4, 2, None, probs, 3, C.byref(res), cp, quant) == 1 and b"w is NULL" in err()
    for kind in (0, 4, -1):
        assert rew(w=wt(kind=kind)) == 1 and b"w.kind" in err()
    for scale in (math.nan, math.inf, -math.inf):
        assert rew(w=wt(scale=scale)) == 1 and b"w.scale" in err()
    assert rew(w=wt(lw=None)) == 1 and b"w.logw is NULL" in err()
    assert rew(w=wt(kind=E.WEIGHT_STORE)) == 1 and b"w.store is NULL" in err()
    assert rew(n=0, p=None, q=None, r=None) == 1  # (nothing else wrong: the rows)

    out = C.c_void_p()

    def res_call(r=fp, a=(2, 4), np_=2, w=None, k=(5, 2), o=C.byref(out)):
        return L.mcx_rows_resample(r, a[0], a[1], np_, w or wt(), 1, k[0], k[1], o, None)

    assert res_call(r=None) == 1 and b"rows is NULL" in err()
    assert res_call(np_=257) == 1 and b"np = 257" in err()
    assert res_call(o=None) == 1 and b"out is NULL" in err()
    for k in ((0, 2), (5, 0), (-1, 2)):
        assert res_call(k=k) == 1 and b"nsteps_out" in err()
    assert res_call(k=(65536, 32768)) == 4 and b"fewer than 2^31" in err()
    assert res_call(a=(65536, 32768)) == 4
    assert res_call(a=(2, 0)) == 1
    assert res_call(w=wt(kind=9)) == 1 and b"w.kind" in err()
    assert res_call(w=wt(scale=math.nan)) == 1 and b"w.scale" in err()
    assert res_call(w=wt(kind=E.WEIGHT_STORE)) == 1 and b"w.store is NULL" in err()
    assert not out

    # the store and engine forms: a NULL owner
    assert L.mcx_store_reweight(None, wt(), probs, 3, C.byref(res), cp, quant) == 1 and b"store s is NULL" in err()
    assert L.mcx_store_resample(None, wt(), 1, 5, 2, C.byref(out), None) == 1 and b"store s is NULL" in err()
    assert L.mcx_samples_reweight(None, 0, 2, wt(), probs, 3, C.byref(res), cp, quant) == 1 and b"engine is NULL" in err()
    assert L.mcx_samples_resample(None, 0, 2, wt(), 1, 5, 2, C.byref(out), None) == 1 and b"engine is NULL" in err()
    assert L.mcx_debug_reweight_times(None, 0, 2, wt(), probs, 3, 1, 5, 2, quant) == 1 and b"engine is NULL" in err()
    q = np.zeros(8, np.uint32)
    qp, mx = q.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_double()
    assert L.mcx_debug_reweight_q(None, None, 2, 4, 2, wt(), qp, C.byref(mx)) == 1 and b"exactly one" in err()
    assert L.mcx_debug_reweight_q(None, fp, 2, 4, 2, wt(), None, C.byref(mx)) == 1 and b"q or lwmax" in err()
    assert L.mcx_debug_reweight_q(None, fp, 2, 4, 2, wt(kind=0), qp, C.byref(mx)) == 1 and b"w.kind" in err()
    assert L.mcx_debug_reweight_q(None, fp, 0, 4, 2, wt(), qp, C.byref(mx)) == 1 and b"at least one step" in err()
    with pytest.raises(McxError) as ei:
        E.reweight_rows(rows, 2, 4, None)
    assert ei.value.code == 1


# ---- the launch geometry ------------------------------------------------------------------------------------------------------
def test_geometry_on_both_sides_of_every_switch():
    g = E.debug_reweight_geometry(1024, 17, 3, 256)
    rs = g["scan_tile_rows"]
    assert rs == 1024 and g["block"] == 256 and rs & (rs - 1) == 0
    assert g["scan_tiles"] == 1 and g["draw_workgroups"] == 1
    g2 = E.debug_reweight_geometry(rs + 1, 17, 3, 257)
    assert g2["scan_tiles"] == 2 and g2["draw_workgroups"] == 2
    assert E.debug_reweight_geometry(2 * rs, 17)["scan_tiles"] == 2 and E.debug_reweight_geometry(2 * rs + 5, 17)["scan_tiles"] == 3
    assert E.debug_reweight_geometry(5, 17, 3, 0)["draw_workgroups"] == 0
    # the histogram tile narrows as the targets (min, max and the probabilities) grow: 64-bit bins within the budget
    want = {0: (2, 2, 1, 8), 2: (4, 4, 1, 4), 6: (8, 8, 1, 2), 14: (16, 16, 1, 1), 15: (17, 16, 2, 1), 30: (32, 16, 2, 1),
            31: (33, 16, 3, 1), 64: (66, 16, 5, 1)}
    for nprobs, (nt, gn, launches, ct) in want.items():
        g = E.debug_reweight_geometry(5000, 17, nprobs)
        assert (g["hist_targets"], g["hist_prefixes"], g["hist_launches"], g["hist_tile_cols"]) == (nt, gn, launches, ct), nprobs
        assert g["hist_tile_cols"] * g["hist_prefixes"] * 256 * 8 <= g["hist_lds_budget"] == 32768
        assert g["hist_lds_bytes"] == ct * gn * 256 * 8 + ct * gn * 4 + ct * 4
        assert 2 * g["hist_lds_bytes"] <= 160 * 1024  # two workgroups and more per compute unit
    assert E.debug_reweight_geometry(5000, 4, 0)["hist_tile_cols"] == 3   # three parameters: no wider than the store
    assert E.debug_reweight_geometry(5000, 4, 14)["hist_tile_cols"] == 1
    # the tail: M = min(N / 5, ceil(3 sqrt N)); no sort below five
    for N, M in ((1, 0), (24, 4), (25, 5), (225, 45), (226, 45), (230, 46), (40000, 600), (200000, 1342)):
        g = E.debug_reweight_geometry(N, 2)
        assert g["tail_m"] == M == R.tail_length(N)
        assert g["sort_tiles"] == (0 if M < 5 else (N + 8191) // 8192)
    a, b = E.debug_reweight_geometry(40000, 3, 3, 0), E.debug_reweight_geometry(40000, 3, 3, 1000)
    assert a["scratch_bytes"] > 8 * 40000 and b["scratch_bytes"] > 4 * 40000 + 8 * 1000


def test_geometry_refusals():
    for a, code in (((0, 2, 0, 0), 1), ((5, 1, 0, 0), 1), ((5, 258, 0, 0), 1), ((5, 2, -1, 0), 1), ((5, 2, 65, 0), 1), ((5, 2, 0, -1), 1),
                    ((2 ** 31, 2, 0, 0), 4), ((5, 2, 0, 2 ** 31), 4)):
        with pytest.raises(McxError) as ei:
            E.debug_reweight_geometry(*a)
        assert ei.value.code == code
    assert load().mcx_debug_reweight_geometry(5, 2, 0, 0, None) == 1


# ---- the header and the host half on their own ----------------------------------------------------------------------------------
def test_header_is_plain_c99_with_the_reweight_declarations(tmp_path):
    src = tmp_path / "reweight_cabi.c"
    src.write_text('#include "mcx.h"\n'
                   'int main(void){ float lw[4] = {0.0f, 0.0f, 0.0f, 0.0f}; mcx_weights w = {MCX_WEIGHT_HOST, 0, 0, 0, 1.0};\n'
                   ' mcx_reweight_result r; mcx_col_reweight c[3]; mcx_reweight_geometry g; mcx_store *o = 0;\n'
                   ' double x[5] = {0.1, 0.2, 0.3, 0.4, 0.5}, k, s, q[3], p[1] = {0.5}; int f; w.logw = lw;\n'
                   ' if (mcx_khat_of_tail(x, 5, &k, &s, &f) != MCX_OK || f & MCX_REWEIGHT_NO_TAIL) return 2;\n'
                   ' if (mcx_khat_of_tail(x, 4, &k, &s, &f) != MCX_OK || f != MCX_REWEIGHT_NO_TAIL || k == k) return 3;\n'
                   ' if (mcx_debug_reweight_geometry(1025, 3, 1, 257, &g) != MCX_OK || g.scan_tiles != 2 || g.draw_workgroups != 2) return 4;\n'
                   ' if (mcx_rows_reweight(0, 1, 4, 2, &w, p, 1, &r, c, q) != MCX_ERR_INVALID) return 5;\n'
                   ' if (mcx_store_reweight(0, &w, p, 1, &r, c, q) != MCX_ERR_INVALID) return 6;\n'
                   ' if (mcx_store_resample(0, &w, 1u, 1, 4, &o, 0) != MCX_ERR_INVALID || o) return 7;\n'
                   ' if (sizeof(mcx_reweight_result) != 96 || sizeof(mcx_col_reweight) != 40 || sizeof(mcx_weights) != 40) return 8;\n'
                   ' if (MCX_WEIGHT_LL != 3 || MCX_REWEIGHT_KHAT_HIGH != 2 || MCX_REWEIGHT_NONFINITE != 1 || MCX_REWEIGHT_MAX_PROBS != 64) return 9;\n'
                   ' return mcx_abi_version() == MCX_ABI_VERSION && MCX_ABI_VERSION == 5 ? 0 : 1; }\n')
    exe = tmp_path / "reweight_cabi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", os.path.join(ROOT, "mcpar_amd"), "-lmcx",
                           "-Wl,-rpath," + os.path.join(ROOT, "mcpar_amd")])
    assert subprocess.call([str(exe)]) == 0
    assert C.sizeof(ReweightResultC) == 96 and C.sizeof(WeightsC) == 40


def test_host_code_under_sanitizers(tmp_path):
    """tests/cpp/reweight_host_check.cc: the host half (csrc/mcx_reweight_host.hpp: k-hat, the thresholds and the finish) as a
    stand-alone program under AddressSanitizer and UBSan"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "reweight_host_check"
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", ROOT,
                    os.path.join(ROOT, "tests", "cpp", "reweight_host_check.cc"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_integer_sums_without_the_loop_are_the_loop_s():
    """reweight_ref.integer_sums (what restate() uses, for the cases of millions of rows) against the row-by-row definition"""
    rng = np.random.default_rng(23)
    for q in (rng.integers(0, 2 ** 31 + 1, 5000), np.full(3000, 2 ** 31), np.zeros(7), np.array([2 ** 32 - 1] * 100 + [0, 1]),
              np.where(rng.random(4000) < 0.5, 0, rng.integers(0, 2 ** 31 + 1, 4000))):
        q = np.asarray(q, np.uint32)
        assert R.integer_sums(q) == R.integer_sums_slow(q)
