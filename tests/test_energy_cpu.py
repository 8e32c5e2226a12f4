"""The joint comparison of two stores without a GPU: the restatement tests/energy_ref.py against a plain
double loop and against scipy, the label rule against a Python restatement, the host finish on made-up sums, the refusals of
every entry point (all before a device is touched), the launch geometry at both sides of its boundaries, the header as C99 and
the host half under sanitizers."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import energy_ref as R
from mcpar_amd import McxError
from mcpar_amd import engine as E
from mcpar_amd._lib import EnergyResultC, EnergySpecC, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def normal_rows(n, ncol, seed):
    return np.random.default_rng([seed, n, ncol]).normal(0.0, 1.0, (n, ncol)).astype(np.float32)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("na, nb", [(2, 2), (7, 5), (33, 20)])
def test_restatement_against_a_double_loop(na, nb):
    a, b = normal_rows(na, 4, 1), normal_rows(nb, 4, 2) + np.float32(0.5)
    ref = R.restate(a, b, -1, -1, nperm=3, seed=5)
    pooled = np.concatenate([a, b]).astype(np.float64)[:, :3]
    N = na + nb
    sd = [math.sqrt(sum((v - sum(pooled[:, c]) / N) ** 2 for v in pooled[:, c]) / (N - 1)) for c in range(3)]
    z = [[pooled[i, c] / sd[c] for c in range(3)] for i in range(N)]
    d = [[math.sqrt(sum((z[i][c] - z[j][c]) ** 2 for c in range(3))) for j in range(N)] for i in range(N)]
    for p in range(4):
        lab = R.labels(5, na, nb, p)
        ab = sum(d[i][j] for i in range(N) for j in range(N) if lab[i] and not lab[j]) / (na * nb)
        aa = sum(d[i][j] for i in range(N) for j in range(N) if lab[i] and lab[j]) / (na * na)
        bb = sum(d[i][j] for i in range(N) for j in range(N) if not lab[i] and not lab[j]) / (nb * nb)
        want = 2.0 * ab - aa - bb
        got = ref["e"] if p == 0 else ref["perm_e"][p - 1]
        assert got == pytest.approx(want, rel=0, abs=1e-12 * ab), (p, got, want)
        if p == 0:
            assert ref["mean_ab"] == pytest.approx(ab, rel=1e-13) and ref["mean_aa"] == pytest.approx(aa, rel=1e-13)
            assert ref["mean_bb"] == pytest.approx(bb, rel=1e-13) and ref["h"] == pytest.approx(want / (2.0 * ab), rel=1e-10)
    assert ref["S"] == pytest.approx(sum(map(sum, d)), rel=1e-13)


@pytest.mark.parametrize("na, nb", [(7, 5), (448, 320)])
def test_restatement_against_scipy(na, nb):
    from scipy import stats  # (a missing scipy fails the check, it does not skip it)
    a, b = normal_rows(na, 2, 3), normal_rows(nb, 2, 4) * np.float32(1.5)
    ref = R.restate(a, b, -1, -1, nperm=0, raw=True)
    want = stats.energy_distance(a[:, 0].astype(np.float64), b[:, 0].astype(np.float64)) ** 2
    assert ref["nused"] == 1 and ref["e"] == pytest.approx(want, rel=1e-12)
    assert math.isnan(ref["p_value"]) and ref["scale"][0] == 1.0 and ref["flags"][1] == R.COL_UNUSED


def test_restatement_drops_columns():
    a, b = normal_rows(6, 4, 5), normal_rows(5, 4, 6)
    a[:, 1] = b[:, 1] = 2.5
    a[2, 2] = NAN
    ref = R.restate(a, b, -1, -1, nperm=2, with_ll=True)
    assert list(ref["flags"]) == [0, R.COL_CONSTANT, R.COL_NONFINITE, 0] and ref["nused"] == 2
    assert ref["scale"][1] == 0.0 and math.isnan(ref["scale"][2])
    raw = R.restate(a, b, -1, -1, nperm=2, with_ll=True, raw=True)
    assert list(raw["flags"]) == [0, 0, R.COL_NONFINITE, 0] and list(raw["scale"][[0, 1, 3]]) == [1.0, 1.0, 1.0]
    a[:, 0] = b[:, 0] = -1.0
    none = R.restate(a, b, -1, -1, nperm=2)
    assert none["nused"] == 0 and math.isnan(none["e"]) and np.isnan(none["perm_e"]).all() and none["nge"] == 0


# ---- the label rule -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("na, nb", [(2, 2), (15, 2), (2, 15), (63, 66), (1, 40), (300, 1)])
def test_labels_against_the_restatement(na, nb):
    for seed, p in ((0, 0), (0, 1), (7, 1), (7, 2), (2 ** 32 - 1, 4095)):
        got = E.debug_energy_labels(seed, na, nb, p)
        assert got.dtype == np.uint8 and got.shape == (na + nb,) and int(got.sum()) == na and got.max() <= 1
        assert np.array_equal(got, R.labels(seed, na, nb, p)), (seed, p)
        if p == 0:
            assert got[:na].all() and not got[na:].any()


def test_labels_reach_every_labeling_of_four_rows():
    seen = {tuple(E.debug_energy_labels(0, 2, 2, p)) for p in range(1, 201)}
    assert len(seen) == 6 and all(sum(s) == 2 for s in seen)


def test_labels_refusals():
    for a in ((0, 0, 2, 0), (0, 2, 0, 0), (0, 16385, 2, 0), (0, 2, 2, -1), (0, 2, 2, 4096)):
        with pytest.raises(McxError) as ei:
            E.debug_energy_labels(*a)
        assert ei.value.code == 1
    assert load().mcx_debug_energy_labels(0, 2, 2, 0, None) == 1


# ---- the host finish (tests/cpp/energy_host_check.cc holds the same figures for the C++ side) -------------------------------------
def test_finish_on_made_up_sums():
    # A = {0, 1}, B = {3} on a line: d01 = 1, d02 = 3, d12 = 2
    f = R.finish(12.0, np.array([7.0, 9.0, 7.0]), np.array([2.0, 6.0, 2.0]), 2, 1)
    assert (f["mean_ab"], f["mean_aa"], f["mean_bb"], f["e"], f["h"]) == (2.5, 0.5, 0.0, 4.5, 0.9)
    assert list(f["perm_e"]) == [1.5, 4.5] and f["nge"] == 1 and f["p_value"] == 2.0 / 3.0
    f0 = R.finish(12.0, np.array([7.0]), np.array([2.0]), 2, 1)
    assert f0["e"] == 4.5 and f0["nge"] == 0 and math.isnan(f0["p_value"]) and len(f0["perm_e"]) == 0
    fz = R.finish(0.0, np.array([0.0]), np.array([0.0]), 2, 2)
    assert fz["e"] == 0.0 and math.isnan(fz["h"])


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_arguments_refused_before_a_device_is_touched():
    """MCX_ERR_INVALID (1), never MCX_ERR_NO_DEVICE (2)"""
    L = load()
    err = L.mcx_last_error
    rows = np.zeros((8, 3), np.float32)
    fp = rows.ctypes.data_as(C.POINTER(C.c_float))
    res, rp = EnergyResultC(), None
    rp = C.byref(res)

    def spec(n_a=-1, n_b=-1, nperm=3, flags=0):
        return C.byref(EnergySpecC(n_a, n_b, nperm, 0, flags))

    def rows_call(*a, np_=2, s=None, r=rp, ra=fp, rb=fp):
        a = a or (2, 4, 2, 4)
        return L.mcx_rows_energy(ra, a[0], a[1], rb, a[2], a[3], np_, s or spec(), r, None, None)

    assert rows_call(ra=None) == 1 and b"rows_a is NULL" in err()
    assert rows_call(rb=None) == 1 and b"rows_b is NULL" in err()
    assert rows_call(r=None) == 1 and b"res is NULL" in err()
    assert rows_call(s=spec(flags=4)) == 1 and b"spec.flags = 4" in err()
    assert rows_call(s=spec(nperm=-1)) == 1 and b"spec.nperm = -1" in err()
    assert rows_call(s=spec(nperm=4096)) == 1 and b"spec.nperm = 4096" in err()
    assert rows_call(np_=0) == 1 and b"np = 0" in err()
    assert rows_call(np_=257) == 1 and b"np = 257" in err()
    for a in ((0, 4, 2, 4), (2, 0, 2, 4), (2, 4, 0, 4), (2, 4, 2, -1)):
        assert rows_call(*a) == 1 and b"at least one step" in err()
    assert rows_call(s=spec(n_a=-2)) == 1 and b"spec.n_a = -2" in err()
    assert rows_call(s=spec(n_b=-2)) == 1 and b"spec.n_b = -2" in err()
    assert rows_call(s=spec(n_a=1)) == 1 and b"1 rows of side a" in err()
    assert rows_call(s=spec(n_b=16385)) == 1 and b"16385 rows of side b" in err()
    assert rows_call(1, 1, 2, 4) == 1 and b"1 rows of side a" in err()              # every row of a side of one row
    assert rows_call(1, 1, 2, 4, s=spec(n_a=0)) == 1 and b"1 rows of side a" in err()  # min(1, 2048) draws
    assert rows_call(2, 4, 16385, 1) == 1 and b"16385 rows of side b" in err()
    sums = np.zeros(9)
    dp = sums.ctypes.data_as(C.POINTER(C.c_double))
    assert L.mcx_debug_energy_sums(fp, 2, 4, fp, 2, 4, 2, spec(), None) == 1 and b"sums is NULL" in err()
    assert L.mcx_debug_energy_sums(None, 2, 4, fp, 2, 4, 2, spec(), dp) == 1 and b"rows_a is NULL" in err()
    assert L.mcx_store_energy(None, None, spec(), rp, None, None) == 1 and b"store a is NULL" in err()
    assert L.mcx_samples_energy(None, 0, 2, 0, 2, spec(), rp, None, None) == 1 and b"engine is NULL" in err()
    assert L.mcx_samples_energy_store(None, 0, 2, None, spec(), rp, None, None) == 1 and b"engine is NULL" in err()
    assert L.mcx_debug_energy_times(None, 0, 2, 0, 2, spec(), None) == 1 and b"ms is NULL" in err()
    assert L.mcx_debug_energy_times(None, 0, 2, 0, 2, spec(), dp) == 1 and b"engine is NULL" in err()
    with pytest.raises(ValueError):
        E.energy_rows(rows, 2, 4, np.zeros((8, 4), np.float32), 2, 4)
    with pytest.raises(McxError) as ei:
        E.energy_rows(rows, 0, 4, rows, 2, 4)
    assert ei.value.code == 1


# ---- geometry -------------------------------------------------------------------------------------------------------------------
def test_geometry_at_its_boundaries(monkeypatch):
    monkeypatch.delenv("MCX_ENERGY_SLAB_ROWS", raising=False)
    g = E.debug_energy_geometry(32, 32, 2, 0)
    assert (g["block"], g["tile_rows"], g["chunk_blocks"], g["col_chunk"], g["slab_rows"]) == (256, 64, 1, 32, 16384)
    assert (g["tiles"], g["slabs"], g["label_cols"], g["label_blocks"], g["chunks"], g["workgroups"]) == (1, 1, 2, 1, 1, 1)
    assert g["lds_bytes"] == 2 * 64 * 33 * 8 + 2 * 64 * 2 + 2 * 16 * 16 * 8
    g16 = E.debug_energy_geometry(32, 32, 2, 999)
    assert g16["lds_bytes"] == 2 * 64 * 33 * 8 + 16 * 64 * 2 + 2 * 16 * 16 * 8 and g16["lds_bytes"] <= 64 * 1024
    assert g["scratch_bytes"] == 64 * 2 * 8 + 64 * 2 + 2 * 16 * 8 + 2 * 16 * 8
    assert E.debug_energy_geometry(32, 33, 2, 0)["tiles"] == 2                                   # the tile: 64 rows
    for nperm, blocks in ((14, 1), (15, 2)):                                                      # the label block: 16 columns
        assert E.debug_energy_geometry(2, 2, 1, nperm)["label_blocks"] == blocks
    # the chunk: the power of two that holds the blocks, 16 at most
    for nperm, width in ((14, 1), (15, 2), (30, 2), (31, 4), (62, 4), (63, 8), (126, 8), (127, 16), (254, 16)):
        g = E.debug_energy_geometry(2, 2, 1, nperm)
        assert (g["chunk_blocks"], g["chunks"]) == (width, 1), nperm
    for nperm, chunks in ((254, 1), (255, 2), (510, 2), (511, 3), (4095, 17)):
        g = E.debug_energy_geometry(2, 2, 1, nperm)
        assert g["chunks"] == chunks and g["label_cols"] == nperm + 2 and g["workgroups"] == chunks and g["chunk_blocks"] == 16
    assert E.debug_energy_geometry(8192, 8192, 1, 0)["slabs"] == 1                               # the slab
    g = E.debug_energy_geometry(8192, 8193, 1, 999)
    assert (g["slabs"], g["tiles"], g["chunks"], g["workgroups"]) == (2, 257, 4, 2 * 257 * 4)
    g = E.debug_energy_geometry(16384, 16384, 257, 4095)
    assert (g["slabs"], g["tiles"], g["chunks"]) == (2, 512, 17) and g["scratch_bytes"] < 2 ** 28
    monkeypatch.setenv("MCX_ENERGY_SLAB_ROWS", "128")
    assert [E.debug_energy_geometry(64, n, 1, 0)["slabs"] for n in (64, 65, 192, 193)] == [1, 2, 2, 3]
    monkeypatch.setenv("MCX_ENERGY_SLAB_ROWS", "100")  # whole staged blocks: 64
    assert E.debug_energy_geometry(64, 64, 1, 0)["slab_rows"] == 64
    monkeypatch.setenv("MCX_ENERGY_SLAB_ROWS", "0")
    assert E.debug_energy_geometry(64, 64, 1, 0)["slab_rows"] == 64
    monkeypatch.setenv("MCX_ENERGY_SLAB_ROWS", "1000000")
    assert E.debug_energy_geometry(64, 64, 1, 0)["slab_rows"] == 16384


def test_geometry_refusals():
    for a in ((1, 2, 1, 0), (2, 1, 1, 0), (16385, 2, 1, 0), (2, 2, 0, 0), (2, 2, 258, 0), (2, 2, 1, -1), (2, 2, 1, 4096)):
        with pytest.raises(McxError) as ei:
            E.debug_energy_geometry(*a)
        assert ei.value.code == 1
    assert load().mcx_debug_energy_geometry(2, 2, 1, 0, None) == 1


# ---- the header and the host half on their own ----------------------------------------------------------------------------------
def test_header_is_plain_c99_with_the_energy_declarations(tmp_path):
    src = tmp_path / "energy_cabi.c"
    src.write_text('#include "mcx.h"\n'
                   'int main(void){ mcx_energy_spec s = {-1, -1, 3, 0u, MCX_ENERGY_WITH_LL | MCX_ENERGY_RAW}; mcx_energy_result r;\n'
                   ' mcx_energy_col c[3]; mcx_energy_geometry g; uint8_t l[4]; double pe[3];\n'
                   ' if (mcx_debug_energy_labels(0u, 2, 2, 0, l) != MCX_OK || l[0] != 1 || l[1] != 1 || l[2] != 0 || l[3] != 0) return 2;\n'
                   ' if (mcx_debug_energy_geometry(8192, 8193, 2, 999, &g) != MCX_OK || g.slabs != 2 || g.chunks != 4) return 3;\n'
                   ' if (mcx_rows_energy(0, 1, 1, 0, 1, 1, 1, &s, &r, c, pe) != MCX_ERR_INVALID) return 4;\n'
                   ' if (mcx_store_energy(0, 0, &s, &r, c, pe) != MCX_ERR_INVALID) return 5;\n'
                   ' if (sizeof(mcx_energy_result) != 88 || sizeof(mcx_energy_col) != 16 || sizeof(mcx_energy_spec) != 20) return 6;\n'
                   ' if (MCX_ENERGY_MAX_SIDE != 16384 || MCX_ENERGY_COL_CONSTANT != 2) return 7;\n'
                   ' return mcx_abi_version() == MCX_ABI_VERSION && MCX_ABI_VERSION == 5 ? 0 : 1; }\n')
    exe = tmp_path / "energy_cabi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", os.path.join(ROOT, "mcpar_amd"), "-lmcx",
                           "-Wl,-rpath," + os.path.join(ROOT, "mcpar_amd")])
    assert subprocess.call([str(exe)]) == 0


def test_host_code_under_sanitizers(tmp_path):
    """tests/cpp/energy_host_check.cc: the host half (csrc/mcx_energy_host.hpp: the label rule, the scale and the finish) as a
    stand-alone program under AddressSanitizer and UBSan"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "energy_host_check"
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", ROOT,
                    os.path.join(ROOT, "tests", "cpp", "energy_host_check.cc"), "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, timeout=60)
    assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()
    assert b"energy_host_check ok" in r.stdout
