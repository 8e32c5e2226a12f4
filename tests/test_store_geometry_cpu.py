"""mcx_debug_store_geometry (include/mcx.h): the launch geometry of the derive, clip, rank and gather code of the store
analyses (DESIGN.md sections 11, 12, 14), from the functions the launch code calls.  Needs no GPU.  Pinned here at both
sides of every size switch; the GPU tests that are there for a switch assert through the same query that their shape lies
past it, so a changed constant makes them say so instead of testing less."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_BUDGET = 40960


def geo(np_, nout, nsteps, nc):
    import mcpar_amd as M
    return M.debug_store_geometry(np_, nout, nsteps, nc)


def test_declared_exported_and_the_abi_version_stays():
    import mcpar_amd
    lib = mcpar_amd.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcx.h")).read(), flags=re.S)
    assert "mcx_debug_store_geometry" in set(re.findall(r"\b(mcx_[a-z_0-9]+)\s*\(", src))
    assert hasattr(lib, "mcx_debug_store_geometry") and lib.mcx_abi_version() == 5
    # the binding's struct has the header's fields in the header's order
    body = src[src.index("typedef struct mcx_store_geometry {"):src.index("} mcx_store_geometry;")]
    from mcpar_amd._lib import StoreGeometry
    assert re.findall(r"long long (\w+);", body) == [n for n, _ in StoreGeometry._fields_]


# (np, nout) -> rows per workgroup of the derive sweep; w = (np | 1) + (nout | 1) floats of LDS per row
R_TABLE = [
    (1, 1, 256), (20, 19, 256),       # w = 2; w = 40: all 40 960 bytes
    (20, 21, 128), (40, 39, 128),     # w = 42, 80
    (40, 41, 64), (80, 79, 64),       # w = 82, 160
    (80, 81, 32), (160, 159, 32),     # w = 162, 320
    (160, 161, 16), (256, 256, 16),   # w = 322, 514
    (40, 17, 128), (17, 40, 128), (100, 3, 64), (3, 100, 64), (256, 2, 32), (2, 256, 32),  # tests/test_gpu_derive.py's
    (41, 17, 128), (101, 3, 64), (255, 2, 32),
]


@pytest.mark.parametrize("np_, nout, R", R_TABLE)
def test_derive_rows_at_both_sides_of_every_switch(np_, nout, R):
    w = (np_ | 1) + (nout | 1)
    g = geo(np_, nout, 2 * R + 5, 1)
    assert g["derive_rows"] == R and g["derive_lds_bytes"] == R * w * 4 <= LDS_BUDGET
    assert R == 256 or 2 * R * w * 4 > LDS_BUDGET  # the largest power of two that fits
    assert g["nrows"] == 2 * R + 5 and g["derive_workgroups"] == 3
    assert geo(np_, nout, 2 * R, 1)["derive_workgroups"] == 2


def test_the_budgets_edge():
    assert geo(20, 19, 1, 1)["derive_lds_bytes"] == LDS_BUDGET and geo(39, 0, 1, 1)["clip_lds_bytes"] == LDS_BUDGET
    assert geo(20, 21, 1, 1)["derive_lds_bytes"] == 128 * 42 * 4


@pytest.mark.parametrize("np_, R, wpw", [(1, 256, 4), (39, 256, 4), (40, 128, 2), (41, 128, 2), (79, 128, 2), (80, 64, 1),
                                         (100, 64, 1), (101, 64, 1), (159, 64, 1), (160, 32, 1), (255, 32, 1), (256, 32, 1)])
def test_clip_rows_and_mask_words(np_, R, wpw):
    g = geo(np_, 0, 2 * R + 5, 1)
    assert (g["clip_rows"], g["clip_mask_words"], g["clip_workgroups"], g["clip_scan_blocks"]) == (R, wpw, 3, 1)
    assert g["clip_lds_bytes"] == R * ((np_ | 1) + 1) * 4 <= LDS_BUDGET
    assert g["derive_rows"] == R  # nout = 0: the clip's tile


def test_scan_depths():
    """the rows at which the multi-level scans take another carry step"""
    M21, M24 = 1 << 21, 1 << 24
    # rank sort: tiles of 8192 keys, k_rank_scan and k_rank_rowsum in steps of 256 tiles -> a second step above 2^21 values
    assert geo(1, 0, M21, 1)["rank_tiles"] == 256 and geo(1, 0, M21 + 1, 1)["rank_tiles"] == 257
    assert geo(1, 0, M21 // 2, 2)["rank_tiles"] == 256  # N counts, not T
    assert geo(1, 0, 2 * M21 + 1, 1)["rank_tiles"] == 513
    # the key and transform sweeps: 64 steps a workgroup until grid.y would pass 2^15
    for T, chunk, gy in ((M21, 64, 32768), (M21 + 1, 65, 32264), (4, 64, 1), (64, 64, 1), (65, 64, 2)):
        g = geo(1, 0, T, 1)
        assert (g["rank_step_chunk"], g["rank_grid_y"]) == (chunk, gy), T
    assert geo(1, 0, M24, 1)["rank_step_chunk"] == 512
    # clip: 256 rows a workgroup at np = 1, 256 workgroups a scan block, k_clip_scan<1> in steps of 256 blocks
    for N, nwg, nb in ((M24, 65536, 256), (M24 + 1, 65537, 257), (65536, 256, 1), (65537, 257, 2), (2 * M24 + 1, 131073, 513)):
        g = geo(1, 0, N, 1)
        assert (g["clip_workgroups"], g["clip_scan_blocks"]) == (nwg, nb), N
    assert geo(256, 0, M21, 1)["clip_scan_blocks"] == 256 and geo(256, 0, M21 + 1, 1)["clip_scan_blocks"] == 257  # 32 rows
    # the shapes of the large GPU cases
    g = geo(1, 0, 2101267, 2)
    assert (g["nrows"], g["rank_tiles"], g["rank_step_chunk"], g["rank_grid_y"]) == (4202534, 514, 65, 32328)
    g = geo(1, 0, 33631309, 1)
    assert (g["clip_workgroups"], g["clip_scan_blocks"]) == (131373, 514)


def test_gather_chunks(monkeypatch):
    monkeypatch.delenv("MCX_GATHER_CHUNK_ROWS", raising=False)
    cap = (64 << 20) // 8  # rows of two floats in 64 MiB
    assert geo(1, 0, cap, 1)["gather_chunk_rows"] == cap and geo(1, 0, cap + 1, 1)["gather_chunk_rows"] == cap
    assert geo(1, 0, 1000, 1)["gather_chunk_rows"] == 1000 and geo(1, 0, 7, 1)["gather_chunk_rows"] == 256
    assert geo(16, 0, 1 << 22, 1)["gather_chunk_rows"] == (64 << 20) // 68
    monkeypatch.setenv("MCX_GATHER_CHUNK_ROWS", "100")  # the tests' knob is the launch code's too
    assert geo(1, 0, cap, 1)["gather_chunk_rows"] == 100


def test_refusals():
    import mcpar_amd as M
    from mcpar_amd._lib import StoreGeometry
    for args, word in (((0, 1, 4, 1), "np"), ((257, 1, 4, 1), "np"), ((1, -1, 4, 1), "nout"), ((1, 257, 4, 1), "nout"),
                       ((1, 1, 0, 1), "nsteps"), ((1, 1, 4, 0), "nc")):
        with pytest.raises(M.McxError) as ei:
            geo(*args)
        assert ei.value.code == 1 and word in str(ei.value), (args, str(ei.value))
    assert M.load().mcx_debug_store_geometry(1, 1, 4, 1, None) == 1
    g = StoreGeometry()
    assert M.load().mcx_debug_store_geometry(1, 1, 4, 1, C.byref(g)) == 0 and g.nrows == 4
