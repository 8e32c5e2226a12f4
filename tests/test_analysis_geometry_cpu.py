"""The launch geometry entries of the lagged covariance, the reweight, the comparison, the intervals and the profiles
(include/mcx.h mcx_debug_{lagcov,reweight,compare,intervals,profile}_geometry; DESIGN.md sections 24, 22, 20, 23, 27), from the
functions the launch code calls.  Needs no GPU.  Every switch between "one item per workgroup (or lane)" and "a loop hands it a
second" is pinned one below, at and one above its threshold, and so is the exact shape of every large GPU case that crosses it:
those cases assert through the same entries that their shape lies past the switch, so a changed constant makes them say so
instead of testing less."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M20, M21 = 1 << 20, 1 << 21


def E():
    from mcpar_amd import engine
    return engine


def test_declared_exported_and_the_abi_version_stays():
    import mcpar_amd
    from mcpar_amd import _lib
    lib = mcpar_amd.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mcx_[a-z_0-9]+)\s*\(", src))
    for name in ("mcx_debug_lagcov_geometry", "mcx_debug_reweight_geometry", "mcx_debug_reweight_store_geometry",
                 "mcx_debug_compare_geometry", "mcx_debug_compare_store_geometry", "mcx_debug_intervals_geometry",
                 "mcx_debug_profile_geometry"):
        assert name in declared and hasattr(lib, name), name
    assert lib.mcx_abi_version() == 5
    # every binding's struct has the header's fields in the header's order; the new fields stand at the end
    tails = dict(lagcov=["units_lag0", "workgroups_lag0"], reweight=["scan_tiles_per_lane", "hist_step_chunks"],
                 compare=["sort_tiles_a", "sort_tiles_b", "bounds_workgroups_a", "bounds_workgroups_b", "step_chunk_a", "step_chunk_b",
                          "grid_y_a", "grid_y_b"],
                 intervals=[], profile=["keys_workgroups", "keys_max_workgroups"])
    for what, tail in tails.items():
        body = src[src.index("typedef struct mcx_%s_geometry {" % what):src.index("} mcx_%s_geometry;" % what)]
        fields = [n for decl in re.findall(r"long long ([\w, ]+);", body) for n in decl.split(", ")]
        assert fields == [n for n, _ in getattr(_lib, what.capitalize() + "Geometry")._fields_], what
        assert fields[len(fields) - len(tail):] == tail, what


# ---- lagged covariance: units of 32 rows over min(units, max(32, 512 / tiles^2)) workgroups; lag 0: units of 128 rows over four
# times as many workgroups at the most
def lag(N, np_=3, nlags=1):
    return E().debug_lagcov_geometry(N, 1, np_, nlags)


@pytest.mark.parametrize("np_, cap", [(1, 512), (16, 512), (17, 128), (32, 128), (33, 56), (48, 56), (49, 32), (64, 32), (65, 32), (256, 32)])
def test_lagcov_units_against_workgroups(np_, cap):
    nt = (np_ + 15) // 16
    assert cap == max(32, 512 // nt ** 2)
    for N, units, wgs in (((cap - 1) * 32, cap - 1, cap - 1), (cap * 32, cap, cap), (cap * 32 + 1, cap + 1, cap), (2 * cap * 32 + 1, 2 * cap + 1, cap)):
        g = lag(N, np_)
        assert (g["rows_per_iteration"], g["units"], g["workgroups"], g["tiles"]) == (32, units, wgs, nt), (np_, N)
    cap0 = 4 * cap
    for N, units, wgs in (((cap0 - 1) * 128, cap0 - 1, cap0 - 1), (cap0 * 128, cap0, cap0), (cap0 * 128 + 1, cap0 + 1, cap0)):
        g = lag(N, np_)
        assert (g["units_lag0"], g["workgroups_lag0"]) == (units, wgs), (np_, N)
        assert g["units_lag0"] <= g["units"] and g["workgroups_lag0"] <= 8 * max(g["workgroups"], 1)  # lag 0's slab fits the windows'


def test_lagcov_shapes_of_the_gpu_cases():
    g = E().debug_lagcov_geometry(887, 37, 3, 17)
    assert (g["units"], g["workgroups"], g["units_lag0"], g["workgroups_lag0"], g["tiles"]) == (1026, 512, 257, 257, 1)
    assert 887 * 37 - 1025 * 32 == 19 and (g["windows"], g["launches"], g["lags_computed"]) == (2, 3, 17)
    g = E().debug_lagcov_geometry(74917, 7, 3, 9)
    assert (g["units"], g["workgroups"], g["units_lag0"], g["workgroups_lag0"]) == (16389, 512, 4098, 2048) and g["lags_computed"] == 9
    g = E().debug_lagcov_geometry(4701, 7, 49, 17)
    assert (g["units"], g["workgroups"], g["units_lag0"], g["workgroups_lag0"]) == (1029, 32, 258, 128)
    assert (g["tiles"], g["pairs"], g["pairs_lag0"]) == (4, 16, 10)
    # the largest of the earlier shapes stays below the switch
    g = E().debug_lagcov_geometry(64, 37, 17, 64)
    assert g["units"] == g["workgroups"] == 74 and g["units_lag0"] == g["workgroups_lag0"] == 19


# ---- reweight: scan tiles of 1024 rows, a lane of the one-workgroup scan owns ceil(tiles / 256) of them; histogram chunks of
# 65 536 steps; sort tiles of 8192 values
def test_reweight_scan_tiles_per_lane():
    rw = E().debug_reweight_geometry
    for tiles, per in ((1, 1), (255, 1), (256, 1), (257, 2), (511, 2), (512, 2), (513, 3), (768, 3), (769, 4)):
        for N in ((tiles - 1) * 1024 + 1, tiles * 1024):
            g = rw(N, 2)
            assert (g["block"], g["scan_tile_rows"], g["scan_tiles"], g["scan_tiles_per_lane"]) == (256, 1024, tiles, per), N
            assert g["hist_step_chunks"] == 0  # (N alone does not say)
    for N, st in ((M21 - 1, 256), (M21, 256), (M21 + 1, 257)):
        assert rw(N, 2)["sort_tiles"] == st, N


def test_reweight_histogram_step_chunks():
    rws = E().debug_reweight_store_geometry
    for T, chunks in ((1, 1), (65535, 1), (65536, 1), (65537, 2), (131072, 2), (131073, 3)):
        for nc in (1, 3):
            g = rws(T, nc, 2)
            assert g["hist_step_chunks"] == chunks, (T, nc)
            assert g == dict(E().debug_reweight_geometry(T * nc, 2), hist_step_chunks=chunks)
    import mcpar_amd as M
    for args in ((0, 1, 2), (1, 0, 2), (1 << 20, 1 << 11, 2)):
        with pytest.raises(M.McxError):
            rws(*args)


def test_reweight_shapes_of_the_gpu_cases():
    rws = E().debug_reweight_store_geometry
    g = rws(65537, 8, 2, 3, 600)
    assert (g["scan_tiles"], g["scan_tiles_per_lane"], g["hist_step_chunks"], g["sort_tiles"], g["draw_workgroups"]) == (513, 3, 2, 65, 3)
    assert -(-513 // 3) == 171  # lane 171 and above own no tile
    g = rws(701783, 3, 2, 3, 600)
    assert (g["scan_tiles"], g["scan_tiles_per_lane"], g["hist_step_chunks"], g["sort_tiles"]) == (2057, 9, 11, 258)
    assert 2057 - 228 * 9 == 5  # lane 228 owns five
    g = rws(400, 500, 2, 3, 0)  # the largest of the earlier shapes: a tile a lane, one chunk
    assert (g["scan_tiles"], g["scan_tiles_per_lane"], g["hist_step_chunks"], g["sort_tiles"]) == (196, 1, 1, 25)


# ---- compare: tiles of 8192 keys per side; k_cmp_bounds a lane per tile; k_cmp_reduce a lane per 256 tiles; the key sweep 64
# steps a workgroup until grid.y would pass 2^15
def test_compare_tiles_bounds_and_step_chunks():
    cg, cs = E().debug_compare_geometry, E().debug_compare_store_geometry
    for na, tiles, wgs in ((M21 - 1, 256, 1), (M21, 256, 1), (M21 + 1, 257, 2), (2 * M21, 512, 2), (2 * M21 + 1, 513, 3)):
        g = cg(na, 100, 2)
        assert (g["tile_keys"], g["tiles_a"], g["sort_tiles_a"], g["bounds_workgroups_a"]) == (8192, tiles, tiles, wgs), na
        assert (g["tiles_b"], g["sort_tiles_b"], g["bounds_workgroups_b"]) == (1, 1, 1)
        assert (g["step_chunk_a"], g["step_chunk_b"], g["grid_y_a"], g["grid_y_b"]) == (0, 0, 0, 0)  # (na and nb alone do not say)
        g = cg(100, na, 2)
        assert (g["tiles_b"], g["sort_tiles_b"], g["bounds_workgroups_b"], g["bounds_workgroups_a"]) == (tiles, tiles, wgs, 1), na
    for T, chunk, gy in ((4, 64, 1), (64, 64, 1), (65, 64, 2), (M21 - 1, 64, 32768), (M21, 64, 32768), (M21 + 1, 65, 32264)):
        g = cs(T, 1, 100, 3, 2)
        assert (g["step_chunk_a"], g["grid_y_a"], g["step_chunk_b"], g["grid_y_b"]) == (chunk, gy, 64, 2), T
        g = cs(100, 3, T, 1, 2)
        assert (g["step_chunk_b"], g["grid_y_b"], g["step_chunk_a"], g["grid_y_a"]) == (chunk, gy, 64, 2), T
        assert {k: v for k, v in g.items() if not k.startswith(("step_chunk", "grid_y"))} == \
            {k: v for k, v in cg(300, T, 2).items() if not k.startswith(("step_chunk", "grid_y"))}
    assert cs(M20, 2, 100, 1, 2)["step_chunk_a"] == 64  # the steps count, not the values
    import mcpar_amd as M
    for args in ((0, 1, 4, 1, 2), (4, 0, 4, 1, 2), (4, 1, 0, 1, 2), (4, 1, 4, 0, 2), (4, 1, 4, 1, 1)):
        with pytest.raises(M.McxError):
            cs(*args)


def test_compare_shape_of_the_gpu_case():
    g = E().debug_compare_store_geometry(2105349, 1, 100001, 3, 2)
    assert (g["tiles_a"], g["sort_tiles_a"], g["bounds_workgroups_a"], g["step_chunk_a"], g["grid_y_a"]) == (258, 258, 2, 65, 32390)
    assert (g["tiles_b"], g["sort_tiles_b"], g["bounds_workgroups_b"], g["step_chunk_b"], g["grid_y_b"]) == (37, 37, 1, 64, 1563)
    g = E().debug_compare_store_geometry(1100, 64, 1100, 64, 2)  # the largest of the earlier shapes
    assert (g["tiles_a"], g["bounds_workgroups_a"], g["step_chunk_a"]) == (9, 1, 64)


# ---- intervals: window tiles of 4096 starts, a lane of k_hdi_reduce per 256 of them; the sort and the key sweep as above
def test_intervals_window_tiles_sort_tiles_and_step_chunks():
    iv = E().debug_intervals_geometry
    for N, wt in ((M20 - 1, 256), (M20, 256), (M20 + 1, 257), (2 * M20, 512), (2 * M20 + 1, 513)):
        g = iv(N, 1, 1, 3, 1)
        assert (g["block"], g["window_tile"], g["window_tiles"], g["slab_entries"], g["reduce_workgroups"]) == (256, 4096, wt, 3 * wt, 3), N
        assert iv(N // 2, 2, 1, 3, 1)["window_tiles"] == -(-(N // 2 * 2) // 4096)  # N counts, not T
    for N, st, chunk, gy in ((M21 - 1, 256, 64, 32768), (M21, 256, 64, 32768), (M21 + 1, 257, 65, 32264)):
        g = iv(N, 1, 1, 3, 1)
        assert (g["sort_tiles"], g["step_chunk"], g["grid_y"]) == (st, chunk, gy), N


def test_intervals_shape_of_the_gpu_case():
    g = E().debug_intervals_geometry(2105349, 1, 1, 3, 1)
    assert (g["window_tiles"], g["sort_tiles"], g["step_chunk"], g["grid_y"], g["transforms"], g["groups"]) == (515, 258, 65, 32390, 2, 1)
    g = E().debug_intervals_geometry(5, 2473, 6, 6, 3)  # the largest of the earlier shapes
    assert (g["window_tiles"], g["sort_tiles"], g["step_chunk"]) == (4, 2, 64)


# ---- pair profiles: k_profile_keys a lane per row up to 4096 workgroups of 256, a grid stride beyond
def test_profile_key_sweep_workgroups():
    pg = E().debug_profile_geometry
    for N, wgs in ((1, 1), (256, 1), (257, 2), (M20 - 256, 4095), (M20 - 255, 4096), (M20, 4096), (M20 + 1, 4096), (4 * M20, 4096)):
        g = pg(2, N, 1, 7, 8, 1)
        assert (g["block"], g["keys_workgroups"], g["keys_max_workgroups"]) == (256, wgs, 4096), N
    assert pg(2, M20 // 4, 4, 7, 8, 1)["keys_workgroups"] == 4096 and pg(2, M20 // 4 - 64, 4, 7, 8, 1)["keys_workgroups"] == 4095


def test_profile_shape_of_the_gpu_case():
    g = E().debug_profile_geometry(2, 349611, 3, 7, 8, 1)
    assert 349611 * 3 == 1048833 > g["keys_max_workgroups"] * g["block"] == M20
    assert (g["keys_workgroups"], g["pair_chunks"], g["pair_workgroups"]) == (4096, 17, 17)
    g = E().debug_profile_geometry(3, 218, 301, 7, 8, 3)  # the largest of the earlier shapes: two pair chunks, a lane a row
    assert g["pair_chunks"] == 2 and g["keys_workgroups"] == -(-218 * 301 // 256) < 4096
