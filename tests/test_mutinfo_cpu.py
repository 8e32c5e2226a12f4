"""The host half of the mutual information between columns, without a device: the host-only entry points
against tests/mutinfo_ref.py bit for bit, the restatement itself against closed forms, and the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

import mutinfo_cases as K
import mutinfo_ref as R
from mcpar_amd import McxError
from mcpar_amd import engine as E
from mcpar_amd._lib import MutinfoGeometry, MutinfoResultC, MutinfoSpecC, load


# ---- the host-only entry points, bit for bit --------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,n", [(10, 10), (10, 2), (10, 3), (1000, 7), (12345, 4096), (2 ** 40 + 3, 16384), (2, 2), (5, 1)])
def test_row_rule(N, n):
    got = E.debug_mutinfo_rows(N, n)
    assert np.array_equal(got, R.row_index(N, n))
    assert got[0] == 0 and got[-1] < N and (np.diff(got) >= 1).all()
    if n == N:
        assert np.array_equal(got, np.arange(N))


@pytest.mark.parametrize("m", [1, 2, 3, 64, 257, 1000])
def test_permutations(m):
    assert np.array_equal(E.debug_mutinfo_perm(12345, m, 0), np.arange(m))
    for seed, p in ((0, 1), (12345, 1), (12345, 2), (4000000000, 999)):
        got = E.debug_mutinfo_perm(seed, m, p)
        assert np.array_equal(np.sort(got), np.arange(m))
        assert np.array_equal(got, R.perm(seed, m, p))
    if m >= 64:
        assert not np.array_equal(E.debug_mutinfo_perm(1, m, 1), E.debug_mutinfo_perm(1, m, 2))
        assert not np.array_equal(E.debug_mutinfo_perm(1, m, 1), E.debug_mutinfo_perm(2, m, 1))


@pytest.mark.parametrize("q", [1, 2, 9, 4096, 16384])
def test_psi_table(q):
    got = E.debug_mutinfo_psi(q)
    assert got.tobytes() == R.psi_table(q).tobytes()
    assert got[0] == -R.GAMMA
    if q >= 9:  # psi(9) = H_8 - gamma = 761 / 280 - gamma
        assert abs(got[8] - (761.0 / 280.0 - R.GAMMA)) < 1e-15


def points_agree(rows, nsteps, nc, **kw):
    got = E.debug_mutinfo_points(rows, nsteps, nc, **kw)
    pk = {f: kw[f] for f in ("n", "with_ll", "raw") if f in kw}
    ref = R.points(rows, **pk)
    for f in ("n_rows", "n_sel", "ndup", "m", "nused"):
        assert got[f] == ref[f], (f, got[f], ref[f])
    assert np.array_equal(got["index"], ref["index"]) and np.array_equal(got["kept"], ref["kept"])
    assert np.array_equal(got["flags"], ref["flags"])
    ok = ~np.isnan(ref["scale"])
    assert np.array_equal(np.isnan(got["scale"]), ~ok)
    assert (np.abs(got["scale"][ok] - ref["scale"][ok]) <= 4.0 * ref["n_sel"] * R.EPS * np.abs(ref["scale"][ok])).all()
    # z from the library's scale: the same division on the same bits
    assert got["z"].tobytes() == R.points(rows, scale=got["scale"], **pk)["z"].tobytes()
    return got


def test_points_repeats_dropped_in_order():
    rows = K.repeated_rows(90, 3, 1)
    got = points_agree(rows, 30, 3, n=-1)
    assert got["ndup"] == 60 and got["m"] == 30 and np.array_equal(np.flatnonzero(got["kept"]), np.arange(0, 90, 3))
    # a repeat that is not adjacent, -0 against +0, and a row that differs in log L alone (not a used column)
    rows = K.normal_rows(12, 2, 2)
    rows[7] = rows[2]
    rows[3, 0], rows[9] = 0.0, rows[3]
    rows[9, 0] = -0.0
    rows[11] = rows[5]
    rows[11, 2] -= 1.0
    got = points_agree(rows, 12, 1, n=-1)
    assert list(np.flatnonzero(got["kept"] == 0)) == [7, 9, 11] and got["ndup"] == 3
    got = points_agree(rows, 12, 1, n=-1, with_ll=True)
    assert list(np.flatnonzero(got["kept"] == 0)) == [7, 9]
    # spaced rows: n of N not divisible
    got = points_agree(K.normal_rows(101, 3, 3), 101, 1, n=7, raw=True)
    assert got["n_sel"] == 7 and (got["scale"][:3] == 1.0).all()
    got = points_agree(K.normal_rows(5000, 2, 4), 50, 100)
    assert got["n_sel"] == 4096


def test_points_flags():
    rows = K.normal_rows(40, 4, 5)
    rows[:, 1] = 0.25
    rows[17, 2] = K.INF
    got = points_agree(rows, 40, 1, n=-1)
    assert list(got["flags"]) == [0, R.COL_CONSTANT, R.COL_NONFINITE, 0, R.COL_UNUSED] and got["nused"] == 2
    assert got["scale"][1] == 0.0 and math.isnan(got["scale"][2]) and math.isnan(got["scale"][4])
    assert (got["z"][[1, 2, 4]] == 0.0).all()
    got = points_agree(rows, 40, 1, n=-1, raw=True, with_ll=True)
    assert list(got["flags"]) == [0, 0, R.COL_NONFINITE, 0, 0]
    # a repeat is judged on the columns without a flag: rows that differ in a flagged column alone are repeats
    rows[21] = rows[20]
    rows[21, 2] = 7.0
    got = points_agree(rows, 40, 1, n=-1)
    assert got["ndup"] == 1 and got["kept"][21] == 0
    # every column flagged: nothing to compare, nothing dropped
    rows = K.normal_rows(10, 2, 6)
    rows[:, :2] = 1.0
    got = points_agree(rows, 10, 1, n=-1)
    assert got["nused"] == 0 and got["ndup"] == 0 and got["m"] == 10


@pytest.mark.parametrize("m,k,gen", [(2, 1, "normal"), (4, 3, "normal"), (65, 3, "normal"), (200, 8, "integer"), (150, 2, "ties")])
def test_finish(m, k, gen):
    rows = dict(normal=lambda: K.normal_pair(m, 0.5, 7), integer=lambda: K.integer_rows(m, 2, 7), ties=lambda: K.one_column_ties(m, 7))[gen]()
    z = R.points(rows, n=-1, raw=True)["z"][:, :]
    eps, na, nb = R.counts(z[0], z[1], k)
    got = E.mutinfo_finish(eps, na, nb, k)
    want = R.finish(eps, na, nb, k)
    assert got == want, (got, want)
    exact, T = R.mi_exact(na, nb, k)
    assert abs(got[0] - exact) <= R.mi_bound(len(eps), k, T)


# ---- the restatement against closed forms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rho", [0.0, 0.6, 0.9])
@pytest.mark.parametrize("seed", K.NORMAL_SEEDS)
def test_restatement_bivariate_normal(rho, seed):
    ref = R.restate(K.normal_pair(1000, rho, seed), n=-1, k=3)
    o = ref["pairs"][0]
    assert ref["m"] == 1000 and o["flags"] == 0
    assert abs(o["mi"] - (-0.5 * math.log(1.0 - rho * rho))) <= 0.15, o["mi"]
    if rho > 0.0:  # (at rho = 0 the root turns an mi of 0.05 into 0.3: r_info is read against the null there)
        assert abs(o["r_info"] - rho) <= 0.15, o["r_info"]


def test_restatement_curved_pair():
    ref = R.restate(K.curved_pair(1000, K.CURVED_SEED), n=-1, k=3)
    o = ref["pairs"][0]
    assert o["mi"] >= 1.0 and abs(o["pearson"]) <= 0.2, (o["mi"], o["pearson"])
    assert o["r_info"] > 0.9


def test_restatement_null_of_the_curved_pair():
    ref = R.restate(K.curved_pair(400, K.CURVED_NULL_SEED), n=-1, k=3, nperm=19, seed=1)
    o = ref["pairs"][0]
    assert o["mi"] >= 1.0 and ref["perm_mi"].max() < 0.25 and o["nge"] == 0 and o["p_value"] == 1.0 / 20.0


def test_restatement_repeats_wreck_it_and_dropping_mends_it():
    """independent columns, every row four times: with the repeats left in each point has k = 3 neighbours at distance 0, every
    count is 0 and the estimate is psi(3) + psi(m) - 2 psi(1), nats high; with them dropped it is within the estimator's spread
    (0.03-0.04 at m = 1000, so below 0.15 at 300) of 0"""
    rows = K.repeated_rows(1200, 2, 8, every=4)
    z = rows[:, :2].astype(np.float64)
    eps, na, nb = R.counts(z[:, 0], z[:, 1], 3)
    t = R.psi_table(1200)
    assert (eps == 0.0).all() and abs(R.mi_exact(na, nb, 3)[0] - (t[2] + t[1199] - 2.0 * t[0])) < 1e-12
    ref = R.restate(rows, n=-1, k=3)
    assert ref["ndup"] == 900 and ref["m"] == 300 and abs(ref["pairs"][0]["mi"]) < 0.15 and ref["pairs"][0]["nzero"] == 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_arguments_refused_before_a_device_is_touched():
    """MCX_ERR_INVALID (1), never MCX_ERR_NO_DEVICE (2)"""
    L = load()
    err = L.mcx_last_error
    rows = np.zeros((8, 3), np.float32)
    fp = rows.ctypes.data_as(C.POINTER(C.c_float))
    res = MutinfoResultC()
    rp = C.byref(res)
    out = np.zeros(16, E.MUTINFO_PAIR_DTYPE)
    op = out.ctypes.data_as(C.c_void_p)
    keep = []

    def spec(n=-1, k=0, nperm=0, flags=0, pairs=None, npairs=None):
        arr = None if pairs is None else np.ascontiguousarray(pairs, np.int32)
        keep.append(arr)
        return C.byref(MutinfoSpecC(n, k, nperm, 0, flags, (0 if arr is None else len(arr)) if npairs is None else npairs,
                                    None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_int))))

    def call(nsteps=2, nc=4, np_=2, s=None, r=rp, ro=fp, o=op):
        return L.mcx_rows_mutinfo(ro, nsteps, nc, np_, s or spec(), r, None, o, None)

    assert call(ro=None) == 1 and b"rows is NULL" in err()
    assert call(r=None) == 1 and b"res is NULL" in err()
    assert call(o=None) == 1 and b"pairs is NULL" in err()
    assert call(s=spec(flags=4)) == 1 and b"spec.flags = 4" in err()
    assert call(s=spec(k=-1)) == 1 and b"spec.k = -1" in err()
    assert call(s=spec(k=9)) == 1 and b"spec.k = 9" in err()
    assert call(s=spec(nperm=-1)) == 1 and b"spec.nperm = -1" in err()
    assert call(s=spec(nperm=1000)) == 1 and b"spec.nperm = 1000" in err()
    assert call(np_=0) == 1 and b"np = 0" in err()
    assert call(np_=257) == 1 and b"np = 257" in err()
    assert call(nsteps=0) == 1 and b"at least one step" in err()
    assert call(nc=0) == 1 and b"at least one step" in err()
    assert call(s=spec(n=-2)) == 1 and b"spec.n = -2" in err()
    assert call(s=spec(n=1)) == 1 and b"1 rows" in err()
    assert call(s=spec(n=9)) == 1 and b"9 rows" in err()                # more than the store has
    assert call(nsteps=1, nc=1) == 1 and b"1 rows" in err()
    assert call(nsteps=16385, nc=1) == 1 and b"16385 rows" in err()     # every row of too many (rows is not read)
    assert call(np_=1) == 1 and b"1 used column" in err()
    assert call(np_=46) == 1 and b"46 used columns" in err()
    assert call(np_=45, s=spec(flags=1)) == 1 and b"46 used columns" in err()
    assert call(s=spec(pairs=[[0, 0]])) == 1 and b"spec.pairs[0] = (0, 0)" in err()
    assert call(s=spec(pairs=[[0, 1], [1, 2]])) == 1 and b"spec.pairs[1] = (1, 2)" in err()     # log L without WITH_LL
    assert call(s=spec(pairs=[[0, -1]])) == 1 and b"spec.pairs[0]" in err()
    assert call(s=spec(pairs=[[0, 1]], npairs=0)) == 1 and b"spec.npairs = 0" in err()
    assert call(s=spec(pairs=[[0, 1]], npairs=1025)) == 1 and b"spec.npairs = 1025" in err()
    assert call(s=spec(npairs=3)) == 1 and b"spec.pairs NULL" in err()
    dp = np.zeros(16).ctypes.data_as(C.POINTER(C.c_double))
    ip = np.zeros(16, np.int32).ctypes.data_as(C.POINTER(C.c_int))
    assert L.mcx_store_mutinfo(None, spec(), rp, None, op, None) == 1 and b"store s is NULL" in err()
    assert L.mcx_samples_mutinfo(None, 0, 2, spec(), rp, None, op, None) == 1 and b"engine is NULL" in err()
    assert L.mcx_debug_mutinfo_times(None, 0, 2, spec(), None) == 1 and b"ms is NULL" in err()
    assert L.mcx_debug_mutinfo_times(None, 0, 2, spec(), dp) == 1 and b"engine is NULL" in err()
    assert L.mcx_debug_mutinfo_counts(fp, 2, 4, 2, spec(), 0, 0, None, ip, ip) == 1 and b"NULL" in err()
    assert L.mcx_debug_mutinfo_counts(fp, 2, 4, 2, spec(), 1, 0, dp, ip, ip) == 1 and b"pair = 1" in err()
    assert L.mcx_debug_mutinfo_counts(fp, 2, 4, 2, spec(), 0, 1, dp, ip, ip) == 1 and b"p = 1" in err()
    lp = np.zeros(8, np.int64).ctypes.data_as(C.POINTER(C.c_longlong))
    assert L.mcx_debug_mutinfo_rows(4, 3, None) == 1 and b"index is NULL" in err()
    assert L.mcx_debug_mutinfo_rows(4, 5, lp) == 1 and b"n = 5" in err()
    assert L.mcx_debug_mutinfo_rows(4, 0, lp) == 1 and b"n = 0" in err()
    assert L.mcx_debug_mutinfo_perm(0, 0, 0, ip) == 1 and b"m = 0" in err()
    assert L.mcx_debug_mutinfo_perm(0, 4, 1000, ip) == 1 and b"p = 1000" in err()
    assert L.mcx_debug_mutinfo_psi(0, dp) == 1 and b"q_max = 0" in err()
    assert L.mcx_mutinfo_finish(dp, ip, ip, 3, 3, dp, None) == 1 and b"m = 3" in err()
    assert L.mcx_mutinfo_finish(dp, ip, ip, 4, 0, dp, None) == 1 and b"k = 0" in err()
    g = MutinfoGeometry()
    assert L.mcx_debug_mutinfo_geometry(3, 1, 0, 3, C.byref(g)) == 1 and b"m = 3" in err()
    assert L.mcx_debug_mutinfo_geometry(100, 0, 0, 3, C.byref(g)) == 1 and b"npairs = 0" in err()
    assert L.mcx_debug_mutinfo_geometry(100, 1, 0, 3, None) == 1 and b"g is NULL" in err()
    with pytest.raises(McxError) as ei:
        E.rows_mutual_info(rows, 2, 4, k=9)
    assert ei.value.code == 1


def test_geometry_at_its_boundaries(monkeypatch):
    monkeypatch.delenv("MCX_MUTINFO_STAGE_ROWS", raising=False)
    g = E.debug_mutinfo_geometry(4, 1, 0, 3)
    assert (g["block"], g["queries_per_lane"], g["tile_rows"], g["stage_rows"], g["stages"], g["tiles"], g["workgroups"]) == (256, 2, 512, 1024, 1, 1, 1)
    assert g["lds_bytes"] == 1024 * 16 + 2 * 256 * 8
    for m, tiles, stages in ((512, 1, 1), (513, 2, 1), (1024, 2, 1), (1025, 3, 2), (16384, 32, 16)):
        g = E.debug_mutinfo_geometry(m, 136, 99, 3)
        assert (g["tiles"], g["stages"], g["workgroups"]) == (tiles, stages, tiles * 136 * 100)
    monkeypatch.setenv("MCX_MUTINFO_STAGE_ROWS", "100")  # rounded down to whole wavefronts
    g = E.debug_mutinfo_geometry(130, 1, 0, 3)
    assert (g["stage_rows"], g["stages"]) == (64, 3)
    monkeypatch.setenv("MCX_MUTINFO_STAGE_ROWS", "1")
    assert E.debug_mutinfo_geometry(130, 1, 0, 3)["stage_rows"] == 64
    monkeypatch.setenv("MCX_MUTINFO_STAGE_ROWS", "99999")
    assert E.debug_mutinfo_geometry(130, 1, 0, 3)["stage_rows"] == 1024


def test_header_compiles_and_refuses_as_c(tmp_path):
    """the new declarations are plain C99, and a C caller gets the refusals without a device"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "mi.c"
    src.write_text('#include "mcx.h"\nint main(void){ mcx_mutinfo_spec s = {0, 0, 0, 0u, 0u, 0, 0}; mcx_mutinfo_result r; mcx_mutinfo_pair p[1];\n'
                   ' float rows[6] = {0}; long long idx[3]; double t[4];\n'
                   ' if (mcx_rows_mutinfo(0, 2, 1, 2, &s, &r, 0, p, 0) != MCX_ERR_INVALID) return 2;\n'
                   ' if (mcx_rows_mutinfo(rows, 2, 1, 2, &s, &r, 0, 0, 0) != MCX_ERR_INVALID) return 3;\n'
                   ' if (mcx_store_mutinfo(0, &s, &r, 0, p, 0) != MCX_ERR_INVALID) return 4;\n'
                   ' if (mcx_debug_mutinfo_rows(7, 3, idx) != MCX_OK || idx[0] != 0 || idx[1] != 2 || idx[2] != 4) return 5;\n'
                   ' if (mcx_debug_mutinfo_psi(4, t) != MCX_OK || t[1] - t[0] != 1.0) return 6;\n'
                   ' return MCX_MUTINFO_MAX_ROWS == 16384 && MCX_MUTINFO_MAX_PERM == 999 && MCX_MUTINFO_MAX_K == 8 ? 0 : 1; }\n')
    exe = tmp_path / "mi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(root, "include"), str(src), "-o",
                           str(exe), "-L", os.path.join(root, "mcpar_amd"), "-lmcx", "-Wl,-rpath," + os.path.join(root, "mcpar_amd")])
    assert subprocess.call([str(exe)]) == 0


def test_host_code_under_sanitizers(tmp_path):
    """tests/cpp/mutinfo_host_check.cc: the host half (csrc/mcx_mutinfo_host.hpp alone) as a stand-alone program under
    AddressSanitizer and UBSan"""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "mutinfo_host_check"
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", root,
                    os.path.join(root, "tests", "cpp", "mutinfo_host_check.cc"), "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, timeout=60)
    assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()
    assert b"mutinfo_host_check ok" in r.stdout
