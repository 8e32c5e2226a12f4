"""Modes of a store without a GPU: the entry points and the ABI, the refusals of every entry point (all
before a device is touched), the host seeding mcx_modes_seed against tests/modes_ref.py index for index, the launch geometry on
both sides of every switch, the header as C99, the host half alone, plain and under sanitizers -- and the proof that the inputs
of the GPU loop test (tests/test_gpu_modes.py) are decisive by the reference alone.

Decisive: at every pass of modes_ref.lloyd every row's relative margin (d2_2 - d2_1) / d2_2 between its two nearest centres is
at least 1e-9.  The device's S_k may differ from the reference's by at most (n_k + 16) 2^-53 sum |u|; for n <= 10^4 that moves a
distance by about 1e-12 relatively, so 1e-9 leaves three orders of margin and the device must find the same labels.  No row is
left out of the condition."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import modes_ref as R
from mcpar_amd import McxError
from mcpar_amd import engine as E
from mcpar_amd._lib import ModesGeometry, ModesResultC, ModesSpecC, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mcx_samples_modes", "mcx_rows_modes", "mcx_store_modes", "mcx_modes_destroy", "mcx_modes_shape", "mcx_modes_labels",
                "mcx_modes_chain_table", "mcx_modes_indicator_store", "mcx_samples_mode_rows", "mcx_rows_mode_rows",
                "mcx_store_mode_rows", "mcx_modes_seed", "mcx_debug_modes_assign", "mcx_debug_modes_geometry", "mcx_debug_modes_times")
MARGIN = 1e-9


def test_entry_points_are_declared_and_exported_and_the_abi_is_5():
    L = load()
    header = open(os.path.join(ROOT, "include", "mcx.h")).read()
    for name in ENTRY_POINTS:
        assert getattr(L, name).argtypes is not None, name
        assert "int %s(" % name in header, name
    for name in ("mcx_modes_spec", "mcx_modes_result", "mcx_mode_row", "mcx_mode_chain", "mcx_modes_geometry"):
        assert "} %s;" % name in header, name
    assert L.mcx_abi_version() == 5 and "#define MCX_ABI_VERSION 5" in header
    assert C.sizeof(ModesSpecC) == 32 and C.sizeof(ModesResultC) == 48 and C.sizeof(ModesGeometry) == 17 * 8
    assert (E.MODES_MAX_K, E.MODE_NONE) == (R.MAX_K, R.NONE) == (32, 255)
    assert (E.MODES_CONVERGED, E.MODES_NOT_CONVERGED, E.MODES_EMPTY) == (R.CONVERGED, R.NOT_CONVERGED, R.EMPTY)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_arguments_refused_before_a_device_is_touched():
    """MCX_ERR_INVALID (1), never MCX_ERR_NO_DEVICE (2)"""
    L = load()
    err = L.mcx_last_error
    rows = np.zeros((16, 3), np.float32)
    fp = rows.ctypes.data_as(C.POINTER(C.c_float))
    dp = C.POINTER(C.c_double)
    res = C.byref(ModesResultC())
    table = np.zeros(32, E.MODE_ROW_DTYPE).ctypes.data_as(C.c_void_p)
    w = [np.zeros((32, 2)).ctypes.data_as(dp) for _ in range(4)]
    sc = np.zeros(2).ctypes.data_as(dp)
    keep = []

    def spec(k=2, max_iter=50, scale=1, seed_rows=16384, seed=0, centres=None):
        c = None
        if centres is not None:
            keep.append(np.ascontiguousarray(centres, np.float64))
            c = keep[-1].ctypes.data_as(dp)
        return C.byref(ModesSpecC(k, max_iter, scale, seed_rows, seed, c))

    def call(r=fp, a=(4, 4), np_=2, s=None, rs=res, t=table, cs=w[0], c=w[1], m=w[2], sd=w[3], sl=sc, out=None, null_spec=False):
        return L.mcx_rows_modes(r, a[0], a[1], np_, None if null_spec else (s or spec()), rs, t, cs, c, m, sd, sl, out)

    assert call(null_spec=True) == 1 and b"NULL" in err()
    for kw in (dict(rs=None), dict(t=None), dict(cs=None), dict(c=None), dict(m=None), dict(sd=None), dict(sl=None)):
        assert call(**kw) == 1 and b"is NULL" in err(), kw
    for k in (0, -1, 33):
        assert call(s=spec(k=k)) == 1 and b"1 to 32 modes" in err()
    assert call(s=spec(k=17)) == 1 and b"k = 17 modes of 16 rows" in err()
    for bad in (0, -3):
        assert call(s=spec(max_iter=bad)) == 1 and b"max_iter" in err()
        assert call(s=spec(seed_rows=bad)) == 1 and b"seed_rows" in err()
    for T in (0, -1):
        assert call(a=(T, 4)) == 1 and b"nsteps" in err()
    assert call(s=spec(centres=[[0.0, 1.0], [np.nan, 0.0]])) == 1 and b"centres[1][0] is not finite" in err()
    assert call(s=spec(centres=[[0.0, -np.inf], [1.0, 0.0]])) == 1 and b"centres[0][1] is not finite" in err()
    assert call(r=None) == 1 and call(np_=0) == 1 and b"np = 0" in err() and call(np_=257) == 1 and b"np = 257" in err()
    assert call(a=(4, 0)) == 1
    # one row has no sd: refused with the scale, before the rows are looked at (a NULL rows pointer is not reached)
    assert call(r=None, a=(1, 1), s=spec(k=1)) == 1 and b"a scale needs nsteps * nc >= 2 rows, got 1" in err()
    assert call(r=None, a=(1, 1), s=spec(k=1, scale=0)) == 1 and b"scale" not in err()
    # the store and engine forms: a NULL owner
    assert L.mcx_store_modes(None, spec(), res, table, *w, sc, None) == 1 and b"store s is NULL" in err()
    assert L.mcx_samples_modes(None, 0, 4, spec(), res, table, *w, sc, None) == 1 and b"engine is NULL" in err()
    assert L.mcx_debug_modes_times(None, 0, 4, spec(), res, (C.c_double * 8)()) == 1 and b"engine is NULL" in err()
    # the handle's functions
    h = C.c_void_p()
    lab = (C.c_ubyte * 4)()
    assert L.mcx_modes_destroy(None) == 0
    assert L.mcx_modes_shape(None, None, None, None, None) == 1 and b"handle m is NULL" in err()
    assert L.mcx_modes_labels(None, 0, 4, lab) == 1 and L.mcx_modes_chain_table(None, None, None, None, None) == 1
    assert L.mcx_modes_indicator_store(None, C.byref(h)) == 1
    assert L.mcx_rows_mode_rows(fp, 4, 4, 2, None, 0, C.byref(h)) == 1 and b"handle m or out is NULL" in err()
    assert L.mcx_store_mode_rows(None, None, 0, C.byref(h)) == 1 and L.mcx_samples_mode_rows(None, 0, 4, None, 0, C.byref(h)) == 1
    # the seeding and the test hooks
    idx = (C.c_longlong * 4)()
    s2 = np.ones(2).ctypes.data_as(dp)
    assert L.mcx_modes_seed(None, 16, 2, 2, 0, s2, idx) == 1 and L.mcx_modes_seed(fp, 16, 2, 2, 0, None, idx) == 1
    assert L.mcx_modes_seed(fp, 16, 2, 2, 0, s2, None) == 1 and b"NULL" in err()
    assert L.mcx_modes_seed(fp, 16, 0, 2, 0, s2, idx) == 1 and L.mcx_modes_seed(fp, 16, 2, 33, 0, s2, idx) == 1
    assert L.mcx_modes_seed(fp, 0, 2, 2, 0, s2, idx) == 1 and b"nrows = 0" in err()
    assert L.mcx_debug_modes_assign(fp, 4, 4, 2, 2, None, s2, None, None, None, None) == 1
    assert L.mcx_debug_modes_assign(fp, 4, 4, 2, 0, s2, s2, None, None, None, None) == 1 and b"k = 0" in err()
    for k in (40, 1 << 30, -(1 << 30)):  # (a wild k is refused, not allocated for)
        with pytest.raises(McxError) as ei:
            E.rows_modes(rows, 4, 4, k)
        assert ei.value.code == 1 and "1 to 32 modes" in str(ei.value)
    with pytest.raises(McxError) as ei:
        E.seed_modes(np.full((8, 3), np.nan, np.float32), 2)
    assert ei.value.code == 1 and "0 rows with finite parameters" in str(ei.value)


# ---- the seeding ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("scale", [True, False], ids=["scaled", "raw"])
def test_seeding_equals_the_restatement_index_for_index(shape, scale):
    np_, nc, T, K = shape
    rows, _ = R.make_rows(np_, nc, T, K, seed=100 + np_)
    s = R.scale_of(rows, scale)
    for seed in (0, 1, 0xdeadbeef):
        got = E.seed_modes(rows, K, seed, s)
        assert np.array_equal(got, R.seed(rows, K, seed, s)), (seed, got)
        assert len(set(got.tolist())) == K and got[0] == int(np.argmax(rows[:, -1]))


def test_seeding_with_rows_that_are_not_finite_ties_and_one_point():
    rng = np.random.default_rng(5)
    rows = rng.normal(size=(300, 4)).astype(np.float32)
    rows[:150, 0] += 20
    rows[7, 1] = np.nan
    rows[11, 2] = np.inf
    rows[7, -1] = rows[11, -1] = 99.0  # the best log L, but not a row that can be a centre
    rows[40, -1] = rows[60, -1] = 50.0  # a tie: the first
    rows[5, -1] = np.nan
    s = R.scale_of(np.delete(rows, [7, 11], 0))
    for seed in range(20):
        got = E.seed_modes(rows, 6, seed, s)
        assert np.array_equal(got, R.seed(rows, 6, seed, s)) and got[0] == 40 and not {7, 11} & set(got.tolist())
    # different seeds do give different centres
    assert len({tuple(E.seed_modes(rows, 6, seed, s).tolist()) for seed in range(20)}) > 10
    same = np.ones((5, 3), np.float32)
    assert E.seed_modes(same, 4, 3).tolist() == [0, 1, 2, 3] and R.seed(same, 4, 3, np.ones(2)).tolist() == [0, 1, 2, 3]
    # a column that takes no part is not seen
    rows2 = rows.copy()
    rows2[:, 3 - 1] = rng.normal(size=300) * 1e6
    s0 = s.copy()
    s0[2] = 0.0
    ok = np.isfinite(rows[:, :3]).all(1)
    rows2[~ok] = rows[~ok]
    assert np.array_equal(E.seed_modes(rows2, 6, 4, s0), E.seed_modes(rows, 6, 4, s0))


# ---- the inputs of the GPU loop test are decisive -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_loop_inputs_are_decisive_by_the_reference_alone(shape):
    np_, nc, T, K = shape
    rows, _ = R.make_rows(np_, nc, T, K, seed=100 + np_)
    s = R.scale_of(rows)
    idx = R.seed(rows, K, 11, s)
    ref = R.lloyd(rows, R.scaled(rows, s)[idx], s)
    print("shape %s: %d passes, least margin per pass %s, n %s" % (shape, ref["iters"], ref["margins"], ref["n"].tolist()))
    assert min(ref["margins"]) >= MARGIN, ref["margins"]  # every row of every pass: none is left out
    assert ref["flags"] == R.CONVERGED and 2 <= ref["iters"] <= 50 and (ref["n"] > 0).all()
    # one pass only: not converged, and the labels are still decisive
    one = R.lloyd(rows, R.scaled(rows, s)[idx], s, max_iter=1)
    assert one["flags"] == R.NOT_CONVERGED and one["iters"] == 1 and one["n_changed"] == T * nc


def test_the_other_loop_inputs_of_the_gpu_tests_are_decisive_too():
    """tests/test_gpu_modes.py holds two more loops to the reference's labels: the (5, 33, 40, 3) rows seeded from a sample of 200
    drawn rows (seed 5), and the same rows unscaled (seed 11).  The same condition, no row left out."""
    np_, nc, T, K = R.SHAPES[1]
    rows, _ = R.make_rows(np_, nc, T, K, seed=100 + np_)
    s = R.scale_of(rows)
    sample = rows[E.debug_draw_indices(5, len(rows), 0, 200)]
    ref = R.lloyd(rows, R.scaled(sample, s)[R.seed(sample, K, 5, s)], s)
    print("a seed sample of 200 rows: %d passes, least margin per pass %s" % (ref["iters"], ref["margins"]))
    assert min(ref["margins"]) >= MARGIN and ref["flags"] == R.CONVERGED and (ref["n"] > 0).all()
    one = np.ones(np_)
    raw = R.lloyd(rows, rows[R.seed(rows, K, 11, one), :np_].astype(np.float64), one)
    assert min(raw["margins"]) >= MARGIN and raw["flags"] == R.CONVERGED


# ---- the launch geometry --------------------------------------------------------------------------------------------------------
def test_geometry_on_both_sides_of_every_switch():
    G = E.debug_modes_geometry
    # rows per tile follow the clip's (40 KiB of LDS): 256 rows to np = 39, 128 to 79, 64 to 159, 32 beyond; below 64 rows the
    # centre loads are per lane
    for np_, R_, uni in ((1, 256, 1), (39, 256, 1), (40, 128, 1), (79, 128, 1), (80, 64, 1), (159, 64, 1), (160, 32, 0), (256, 32, 0)):
        g = G(np_, 8, 64, 2)
        assert (g["rows_per_tile"], g["lane_groups"], g["uniform_centres"]) == (R_, 256 // R_, uni), (np_, g)
        assert g["rows_per_tile"] == E.debug_store_geometry(np_, 0, 8, 64)["clip_rows"]
        assert g["mark_mask_words"] == (R_ + 63) // 64 and g["block"] == 256
        assert g["sum_subgroups"] == 256 // np_ and g["table_columns"] == np_ + 2
        assert g["table_subgroups"] == 256 // min(np_ + 2, 256)
        assert g["assign_lds_bytes"] == 8 * (g["sum_subgroups"] * 2 * np_ + np_) + 4 * R_ * (np_ | 1)
        assert g["table_lds_bytes"] == 8 * (g["table_subgroups"] * 2 * (np_ + 2) + np_) + 4 * R_ * ((np_ | 1) + 1)
    # the assign pass' accumulators stop at 2048 doubles: fewer subgroups where K np of them would pass that
    for (np_, k), sub in {(16, 8): 16, (16, 9): 14, (16, 32): 4, (1, 8): 256, (1, 9): 227, (1, 32): 64, (64, 32): 1, (17, 2): 15, (17, 32): 3}.items():
        assert G(np_, 8, 64, k)["sum_subgroups"] == sub, (np_, k)
    for (np_, k), sub in {(16, 8): 14, (16, 32): 3, (1, 32): 21, (64, 32): 1, (62, 2): 4}.items():
        assert G(np_, 8, 64, k)["table_subgroups"] == sub, (np_, k)
    assert G(254, 8, 64, 2)["table_subgroups"] == 1 and G(255, 8, 64, 2)["table_columns"] == 257
    # centre blocks of eight
    for k, nb in ((1, 1), (8, 1), (9, 2), (16, 2), (17, 3), (32, 4)):
        assert G(16, 8, 64, k)["centre_blocks"] == nb
    # tiles and workgroups: one short of, equal to and one past a tile; the workgroups stop at 1024
    for N, tiles in ((255, 1), (256, 1), (257, 2), (256 * 1024, 1024), (256 * 1024 + 1, 1025), (2 * 1024 * 256 + 257, 2050)):
        g = G(16, 1, N, 8)
        assert (g["tiles"], g["workgroups"], g["mark_workgroups"]) == (tiles, min(tiles, 1024), tiles), N
    # the largest LDS a workgroup asks for stays inside a CU's 160 KiB, and the scratch is bounded by the 1024 slabs
    worst = max(max(G(np_, 8, 64, 32)["assign_lds_bytes"], G(np_, 8, 64, 32)["table_lds_bytes"]) for np_ in range(1, 257))
    assert worst <= 112 * 1024
    g = G(256, 1 << 20, 64, 32)
    # doubles: slabs and their sums K (np + 2) (1024 + 1); c, mean and the blocked centres 3 K np; s np.  words: 2 K + 2 + 2 K 1024
    assert g["workgroups"] == 1024 and g["scratch_bytes"] == 8 * (32 * 258 * 1025 + 3 * 32 * 256 + 256 + 2 * 32 * 1024 + 66)
    assert G(16, 50, 64, 8)["chains_workgroups"] == 1 and G(16, 50, 257, 8)["chains_workgroups"] == 2
    assert G(16, 4, 64, 8)["steps_workgroups"] == 1 and G(16, 5, 64, 8)["steps_workgroups"] == 2
    for a in ((0, 4, 4, 2), (257, 4, 4, 2), (2, 0, 4, 2), (2, 4, 0, 2), (2, 4, 4, 0), (2, 4, 4, 33)):
        with pytest.raises(McxError) as ei:
            G(*a)
        assert ei.value.code == 1
    assert load().mcx_debug_modes_geometry(2, 4, 4, 2, None) == 1


# ---- the header and the host half on their own ------------------------------------------------------------------------------------
def test_header_is_plain_c99_with_the_modes_declarations(tmp_path):
    src = tmp_path / "modes_cabi.c"
    src.write_text('#include "mcx.h"\n'
                   'int main(void){ float rows[8] = {0.f, -1.f, 5.f, -2.f, 0.25f, -3.f, 5.5f, -0.5f}; double s[1] = {1.0}, w[8];\n'
                   ' long long idx[2]; mcx_modes_spec sp = {2, 50, 1, 16384, 0u, 0}; mcx_modes_result r; mcx_mode_row t[2];\n'
                   ' mcx_mode_chain c; mcx_modes_geometry g; mcx_modes *m = 0; mcx_rowset *rs = 0;\n'
                   ' if (mcx_modes_seed(rows, 4, 1, 2, 0u, s, idx) != MCX_OK || idx[0] != 3 || idx[1] < 0 || idx[1] > 2) return 2;\n'
                   ' if (mcx_debug_modes_geometry(16, 50, 64, 8, &g) != MCX_OK || g.rows_per_tile != 256 || g.tiles != 13) return 3;\n'
                   ' if (mcx_rows_modes(0, 4, 4, 1, &sp, &r, t, w, w, w, w, s, &m) != MCX_ERR_INVALID) return 4;\n'
                   ' if (mcx_store_modes(0, &sp, &r, t, w, w, w, w, s, &m) != MCX_ERR_INVALID) return 5;\n'
                   ' if (mcx_rows_mode_rows(rows, 4, 1, 1, m, 0, &rs) != MCX_ERR_INVALID || mcx_modes_destroy(m) != MCX_OK) return 6;\n'
                   ' if (sizeof(mcx_modes_spec) != 32 || sizeof(mcx_modes_result) != 48 || sizeof(mcx_mode_row) != 48) return 7;\n'
                   ' if (sizeof(c) != 32 || MCX_MODES_MAX_K != 32 || MCX_MODE_NONE != 255 || MCX_MODES_EMPTY != 4) return 8;\n'
                   ' return mcx_abi_version() == MCX_ABI_VERSION && MCX_ABI_VERSION == 5 ? 0 : 1; }\n')
    exe = tmp_path / "modes_cabi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", os.path.join(ROOT, "mcpar_amd"), "-lmcx",
                           "-Wl,-rpath," + os.path.join(ROOT, "mcpar_amd")])
    assert subprocess.call([str(exe)]) == 0


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_host_code_alone(tmp_path, flags):
    """tests/cpp/modes_host_check.cc: the host half (csrc/mcx_modes_host.hpp: the seeding, the centre update, the refusals) as a
    stand-alone program, plain and under AddressSanitizer and UBSan"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "modes_host_check"
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror"] + flags +
                   ["-I", ROOT, os.path.join(ROOT, "tests", "cpp", "modes_host_check.cc"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
