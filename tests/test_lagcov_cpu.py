"""Lagged covariance and multivariate ESS of a store without a GPU: the entry points and the ABI, the
refusals of every entry point (all before a device is touched), the host walk mcx_mess_finish against tests/lagcov_ref.py on
reference matrices, the launch geometry for the shapes of tests/test_gpu_lagcov.py, the header as C99 and the host half alone,
plain and under sanitizers.

mess_finish is held to the reference at a relative 1e-9 (Sigma: of sqrt(Sigma_ii Sigma_jj)); its integers and flags exactly, on
inputs the reference says are decisive (lagcov_ref.decisive)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import lagcov_ref as R
from mcpar_amd import McxError
from mcpar_amd import engine as E
from mcpar_amd._lib import LagcovGeometry, LagcovResultC, LagcovSpecC, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mcx_samples_lagcov", "mcx_rows_lagcov", "mcx_store_lagcov", "mcx_mess_finish", "mcx_debug_lagcov_geometry",
                "mcx_debug_lagcov_times")


def test_entry_points_are_declared_and_exported_and_the_abi_is_5():
    L = load()
    header = open(os.path.join(ROOT, "include", "mcx.h")).read()
    for name in ENTRY_POINTS:
        assert getattr(L, name).argtypes is not None, name
        assert "int %s(" % name in header, name
    for name in ("mcx_lagcov_spec", "mcx_lagcov_result", "mcx_col_lagcov", "mcx_lagcov_geometry"):
        assert "} %s;" % name in header, name
    assert L.mcx_abi_version() == 5 and "#define MCX_ABI_VERSION 5" in header
    assert C.sizeof(LagcovSpecC) == 12 and C.sizeof(LagcovResultC) == 56 and E.LAGCOV_DTYPE.itemsize == 32
    assert (E.MESS_NOT_PD, E.MESS_TRUNCATED, E.MESS_LAMBDA_SINGULAR, E.LAGCOV_CONSTANT) == (R.NOT_PD, R.TRUNCATED, R.LAMBDA_SINGULAR, R.CONSTANT)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_arguments_refused_before_a_device_is_touched():
    """MCX_ERR_INVALID (1), never MCX_ERR_NO_DEVICE (2)"""
    L = load()
    err = L.mcx_last_error
    rows = np.zeros((16, 3), np.float32)
    fp = rows.ctypes.data_as(C.POINTER(C.c_float))
    dp = C.POINTER(C.c_double)
    res = C.byref(LagcovResultC())
    cols = np.zeros(3, E.LAGCOV_DTYPE).ctypes.data_as(C.c_void_p)
    sig = np.zeros((3, 3)).ctypes.data_as(dp)
    gam = np.zeros((8, 3, 3)).ctypes.data_as(dp)

    def spec(max_lag=3, nlags_out=2, with_ll=0):
        return C.byref(LagcovSpecC(max_lag, nlags_out, with_ll))

    def call(r=fp, a=(4, 4), np_=2, s=None, rs=res, c=cols, sg=sig, g=gam):
        return L.mcx_rows_lagcov(r, a[0], a[1], np_, s or spec(), rs, c, sg, g)

    assert call(r=None) == 1 and b"rows is NULL" in err()
    assert call(np_=0) == 1 and call(np_=257) == 1 and b"np = 257" in err()
    assert call(a=(4, 0)) == 1 and b"nc = 0" in err()
    for T in (3, 0, -1):
        assert call(a=(T, 4)) == 1 and b"nsteps >= 4" in err()
    assert L.mcx_rows_lagcov(fp, 4, 4, 2, None, res, cols, sig, gam) == 1 and b"spec is NULL" in err()
    for kw in (dict(rs=None), dict(c=None), dict(sg=None)):
        assert call(**kw) == 1 and b"is NULL" in err()
    for bad in (0, -1):
        assert call(s=spec(max_lag=bad)) == 1 and b"max_lag" in err()
    for bad in (-1, 5):
        assert call(s=spec(nlags_out=bad)) == 1 and b"nlags_out" in err()
    assert call(g=None) == 1 and b"gamma is NULL" in err()
    # gamma may be NULL when no lag is returned: only the rows are wrong then
    assert call(r=None, s=spec(nlags_out=0), g=None) == 1 and b"rows is NULL" in err()
    # the store and engine forms: a NULL owner
    assert L.mcx_store_lagcov(None, spec(), res, cols, sig, gam) == 1 and b"store s is NULL" in err()
    assert L.mcx_samples_lagcov(None, 0, 4, spec(), res, cols, sig, gam) == 1 and b"engine is NULL" in err()
    assert L.mcx_debug_lagcov_times(None, 0, 4, spec(), res, (C.c_double * 5)()) == 1 and b"engine is NULL" in err()
    with pytest.raises(McxError) as ei:
        E.rows_lagcov(rows, 4, 4, max_lag=0)
    assert ei.value.code == 1
    # the host walk
    g = np.zeros((4, 3, 3))
    gp = g.ctypes.data_as(dp)
    assert L.mcx_mess_finish(3, 4, 16, None, None, res, cols, sig) == 1 and b"NULL" in err()
    assert L.mcx_mess_finish(3, 4, 16, gp, None, None, cols, sig) == 1
    assert L.mcx_mess_finish(3, 4, 16, gp, None, res, None, sig) == 1
    assert L.mcx_mess_finish(3, 4, 16, gp, None, res, cols, None) == 1
    assert L.mcx_mess_finish(0, 4, 16, gp, None, res, cols, sig) == 1 and b"ncol = 0" in err()
    assert L.mcx_mess_finish(258, 4, 16, gp, None, res, cols, sig) == 1
    assert L.mcx_mess_finish(3, 1, 16, gp, None, res, cols, sig) == 1 and b"nlags = 1" in err()
    assert L.mcx_mess_finish(3, 4, 1, gp, None, res, cols, sig) == 1 and b"N = 1" in err()


# ---- the host walk --------------------------------------------------------------------------------------------------------------
def finish_both(gamma, N, use):
    got, ref = E.mess_finish(gamma, N, use), R.finish(gamma, N, use)
    assert R.decisive(ref), (ref["margins"], ref["pivot_ratio"])
    R.check_finish(got, ref)
    assert np.array_equal(got["col_flags"], ref["col_flags"]) and got["lags_computed"] == gamma.shape[0] and got["N"] == N
    assert np.array_equal(got["mcse_cov"], got["sigma"] / N, equal_nan=True) and np.isnan(got["mean"]).all()
    return got, ref


def test_mess_finish_on_a_plain_sequence():
    np_, nc, T = 3, 5, 16
    g, _, fl = R.gamma_of(R.dependent_rows(np_, nc, T), T, nc, T)
    got, ref = finish_both(g, T * nc, R.use_of(fl, False))
    assert (got["s"], got["p"], got["flags"]) == (0, 3, 0) and 0 <= got["k_used"] <= 4 and got["lags_used"] == 2 * got["k_used"] + 2
    assert np.isnan(got["sigma"][3]).all() and np.isnan(got["ess"][3]) and 0 < got["mess"] < T * nc
    # with log L, and with every column by default
    with_ll, _ = finish_both(g, T * nc, R.use_of(fl, True))
    assert with_ll["p"] == 4 and R.same(E.mess_finish(g, T * nc), with_ll)
    # two calls, the same bytes
    assert R.same(E.mess_finish(g, T * nc, R.use_of(fl, False)), got)


def test_mess_finish_on_antithetic_rows_starts_late():
    """AR(1) with phi = -0.9: S(t) alternates, P(k) = 0.1 0.81^k S(0), and -S(0) + 2 sum P turns positive near k = 14"""
    nc, T = 64, 96
    g, _, fl = R.gamma_of(R.antithetic_rows(3, nc, T, seed=7), T, nc, T)
    got, ref = finish_both(g, T * nc, R.use_of(fl, True))
    assert ref["s"] > 0 and 10 <= got["s"] <= 20 and got["k_used"] >= got["s"] and got["p"] == 3
    assert got["mess"] > T * nc  # antithetic: better than independent draws
    # with fewer lags than the start needs there is no estimate
    few = E.mess_finish(g[:2 * got["s"]], T * nc)
    assert few["flags"] == E.MESS_NOT_PD and few["s"] == -1


def test_mess_finish_with_max_lag_3_is_truncated():
    np_, nc, T = 3, 5, 16
    g, _, fl = R.gamma_of(R.dependent_rows(np_, nc, T), T, nc, 4)
    got, ref = finish_both(g, T * nc, R.use_of(fl, False))
    assert got["flags"] == E.MESS_TRUNCATED and got["k_used"] == 1 and got["lags_used"] == 4
    full = R.restate(R.dependent_rows(np_, nc, T), T, nc)
    assert full["k_used"] > 1 and not full["flags"] & R.TRUNCATED  # (the whole range goes further, and ends at a test)


def test_mess_finish_never_positive_definite():
    g = np.zeros((8, 2, 2))
    for t in range(8):
        g[t] = np.array([[1.0, 0.2], [0.2, 1.0]]) * (-0.95) ** t * (1.0 if t % 2 else 0.9)  # P(k) < 0 for every k
    got, ref = E.mess_finish(g, 100), R.finish(g, 100, [True, True])
    R.check_finish(got, ref)
    assert got["flags"] == E.MESS_NOT_PD and (got["s"], got["k_used"], got["lags_used"], got["p"]) == (-1, -1, 0, 2)
    for f in ("mess", "logdet_sigma", "logdet_lambda"):
        assert np.isnan(got[f]), f
    assert np.isnan(got["sigma"]).all() and np.isnan(got["ess"]).all() and np.isnan(got["mcse"]).all()


def test_mess_finish_leaves_out_constant_and_nan_columns():
    np_, nc, T = 3, 5, 16
    rows = R.dependent_rows(np_, nc, T)
    rows[:, 2] = np.float32(1.25)
    rows[7, 0] = np.nan
    g, _, fl = R.gamma_of(rows, T, nc, T)
    assert fl.tolist() == [1, 0, 0, 0] and (g[:, 2, 1:] == 0).all()
    got = E.mess_finish(g, T * nc, R.use_of(fl, True))
    ref = R.finish(g, T * nc, R.use_of(fl, True))
    R.check_finish(got, ref)
    assert got["p"] == 2 and got["col_flags"].tolist() == [E.SUMMARY_NONFINITE, 0, E.LAGCOV_CONSTANT, 0]
    assert np.isnan(got["ess"][[0, 2]]).all() and np.isfinite(got["ess"][[1, 3]]).all()
    # all columns by default: the two are left out all the same
    assert E.mess_finish(g, T * nc)["p"] == 2


# ---- the launch geometry ----------------------------------------------------------------------------------------------------------
def test_geometry_of_the_gpu_shapes_and_on_both_sides_of_every_switch():
    want = {(1, 2, 8): (1, 1, 1, 1, 1), (3, 5, 16): (3, 3, 1, 1, 1), (16, 37, 48): (56, 56, 1, 1, 1), (17, 37, 64): (74, 74, 2, 3, 4),
            (40, 8, 96): (24, 24, 3, 6, 9), (3, 7, 5): (2, 2, 1, 1, 1)}
    for (np_, nc, T), w in want.items():
        g = E.debug_lagcov_geometry(T, nc, np_, 1)
        assert (g["units"], g["workgroups"], g["tiles"], g["pairs_lag0"], g["pairs"]) == w, (np_, nc, T, g)
        assert (g["block"], g["window_lags"], g["rows_per_iteration"], g["windows"], g["launches"], g["lags_computed"]) == (256, 8, 32, 0, 1, 1)
        assert g["slab_rows"] == 2 * 16 * g["tiles"] + 1 + 256 * g["pairs"]
    W = 8
    for nlags, windows in ((1, 0), (2, 1), (W + 1, 1), (W + 2, 2), (2 * W + 1, 2), (96, 12)):
        g = E.debug_lagcov_geometry(96, 8, 40, nlags)
        assert (g["windows"], g["launches"], g["lags_computed"]) == (windows, 1 + windows, min(96, 1 + W * windows)), nlags
    # rows: a unit of 32; workgroups stop growing at 512 shared among the tile pairs, 32 at the least
    assert E.debug_lagcov_geometry(4, 8, 2)["units"] == 1 and E.debug_lagcov_geometry(4, 8, 2)["workgroups"] == 1
    assert E.debug_lagcov_geometry(11, 3, 2)["units"] == 2
    g = E.debug_lagcov_geometry(8, 32 * 64, 2)
    assert (g["units"], g["workgroups"]) == (512, 512)
    g = E.debug_lagcov_geometry(8, 32 * 64 + 1, 2)
    assert (g["units"], g["workgroups"]) == (513, 512)
    for np_, cap in ((16, 512), (17, 128), (33, 56), (49, 32), (256, 32)):
        g = E.debug_lagcov_geometry(8, 32 * 64, np_)
        assert (g["units"], g["workgroups"]) == (512, cap) and g["scratch_bytes"] <= 8 * (8 * g["slab_rows"] * (cap + 1) + (np_ + 1) * (3 * 2048 + 2))
    assert E.debug_lagcov_geometry(8, 32 * 64, 256)["scratch_bytes"] < 160e6
    for a in ((3, 2, 1, 1), (4, 0, 1, 1), (4, 2, 0, 1), (4, 2, 257, 1), (4, 2, 1, 0), (4, 2, 1, 5)):
        with pytest.raises(McxError) as ei:
            E.debug_lagcov_geometry(*a)
        assert ei.value.code == 1
    assert load().mcx_debug_lagcov_geometry(4, 2, 1, 1, None) == 1
    assert C.sizeof(LagcovGeometry) == 15 * 8


# ---- the header and the host half on their own ------------------------------------------------------------------------------------
def test_header_is_plain_c99_with_the_lagcov_declarations(tmp_path):
    src = tmp_path / "lagcov_cabi.c"
    src.write_text('#include "mcx.h"\n'
                   'int main(void){ double g[4] = {1.0, 0.5, 0.25, 0.125}, sigma[1]; mcx_lagcov_spec s = {3, 0, 0}; mcx_lagcov_result r;\n'
                   ' mcx_col_lagcov c[1]; mcx_lagcov_geometry q;\n'
                   ' if (mcx_mess_finish(1, 4, 100, g, 0, &r, c, sigma) != MCX_OK || r.k_used != 1 || r.flags != MCX_MESS_TRUNCATED) return 2;\n'
                   ' if (sigma[0] < 2.7499999 || sigma[0] > 2.7500001 || r.p != 1 || r.lags_used != 4 || c[0].flags != 0) return 3;\n'
                   ' if (mcx_debug_lagcov_geometry(96, 8, 40, 20, &q) != MCX_OK || q.launches != 4 || q.pairs != 9) return 4;\n'
                   ' if (mcx_rows_lagcov(0, 4, 4, 2, &s, &r, c, sigma, 0) != MCX_ERR_INVALID) return 5;\n'
                   ' if (mcx_store_lagcov(0, &s, &r, c, sigma, 0) != MCX_ERR_INVALID) return 6;\n'
                   ' if (sizeof(mcx_lagcov_spec) != 12 || sizeof(mcx_lagcov_result) != 56 || sizeof(mcx_col_lagcov) != 32) return 7;\n'
                   ' if (MCX_MESS_NOT_PD != 1 || MCX_MESS_LAMBDA_SINGULAR != 4 || MCX_LAGCOV_CONSTANT != 2 || MCX_LAGCOV_TIMES != 5) return 8;\n'
                   ' return mcx_abi_version() == MCX_ABI_VERSION && MCX_ABI_VERSION == 5 ? 0 : 1; }\n')
    exe = tmp_path / "lagcov_cabi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", os.path.join(ROOT, "mcpar_amd"), "-lmcx",
                           "-Wl,-rpath," + os.path.join(ROOT, "mcpar_amd")])
    assert subprocess.call([str(exe)]) == 0


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_host_code_alone(tmp_path, flags):
    """tests/cpp/lagcov_host_check.cc: the host half (csrc/mcx_lagcov_host.hpp: the factorisation, the walk, the flags) as a
    stand-alone program, plain and under AddressSanitizer and UBSan"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "lagcov_host_check"
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror"] + flags +
                   ["-I", ROOT, os.path.join(ROOT, "tests", "cpp", "lagcov_host_check.cc"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
