"""The joint comparison of two stores on the GPU against the float64 restatement tests/energy_ref.py:
integer fields, flags and labels exact; S and every S_A, S_AA within 2 eps ref with eps = (N^2 + ncol + 4) 2^-53; e and every
perm_e within 16 eps S / min(n_a, n_b)^2; scale within 4 N 2^-53 relative; nge and p_value as the definition gives them from
the returned perm_e, and the reference's wherever no reference perm_e lies within twice the bound of e.

The shapes are the smallest at which the unit can go wrong: sides around the 16-row wavefront and the 64-row tile, label
vectors around the block of 16 and the chunk the geometry names, a lowered slab split, used columns around the staged chunk of
32.  WORST collects the largest error / bound seen (printed by the last test; DESIGN.md records it)."""
import math

import numpy as np
import pytest

import compare_ref as CR
import energy_cases as K
import energy_ref as R
from test_gpu_store_view import run

pytestmark = pytest.mark.gpu

WORST = {"ratio": 0.0}
ALL = dict(n_a=-1, n_b=-1)


def held(a, b, **kw):
    """energy_rows of host rows (one chain a side) held to the restatement, sums included -> the result"""
    from mcpar_amd import engine as E
    got = E.energy_rows(a, len(a), 1, b, len(b), 1, **kw)
    sums = E.debug_energy_sums(a, len(a), 1, b, len(b), 1, **kw)
    WORST["ratio"] = max(WORST["ratio"], R.check(got, R.restate(a, b, **kw), a.shape[1], sums))
    return got


def same_bytes(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


@pytest.mark.parametrize("nperm", [0, 1, 15, 16, 17])
@pytest.mark.parametrize("na, nb", [(2, 2), (15, 2), (16, 16), (17, 30), (63, 66)])
def test_sizes(na, nb, nperm):
    held(K.normal_rows(na, 3, 1), K.normal_rows(nb, 3, 2, shift=0.4), nperm=nperm, seed=11, **ALL)


def test_nperm_past_the_label_chunk():
    from mcpar_amd import engine as E
    most = E.debug_energy_geometry(17, 30, 3, E.ENERGY_MAX_PERM)["chunk_blocks"]  # the widest chunk
    nperm = most * 16 - 1  # nperm + 2 label columns: one past the chunk
    assert E.debug_energy_geometry(17, 30, 3, nperm)["chunks"] == 2 and E.debug_energy_geometry(17, 30, 3, nperm - 1)["chunks"] == 1
    held(K.normal_rows(17, 3, 3), K.normal_rows(30, 3, 4), nperm=nperm, seed=2, **ALL)
    held(K.normal_rows(17, 3, 3), K.normal_rows(30, 3, 4), nperm=nperm - 1, seed=2, **ALL)


@pytest.mark.parametrize("nperm, width", [(14, 1), (30, 2), (40, 4), (62, 4), (63, 8), (100, 8), (126, 8), (127, 16), (199, 16)])
def test_every_chunk_width(nperm, width):
    """a kernel instance per width; 40, 100 and 199 leave the last blocks of the chunk empty"""
    from mcpar_amd import engine as E
    assert E.debug_energy_geometry(20, 13, 3, nperm)["chunk_blocks"] == width
    held(K.normal_rows(20, 3, 16), K.normal_rows(13, 3, 17, shift=0.3), nperm=nperm, seed=12, **ALL)


def test_slab_split(monkeypatch):
    from mcpar_amd import engine as E
    a, b = K.normal_rows(63, 3, 5), K.normal_rows(66, 3, 6, shift=-0.3)
    monkeypatch.delenv("MCX_ENERGY_SLAB_ROWS", raising=False)
    one = held(a, b, nperm=31, seed=3, **ALL)
    monkeypatch.setenv("MCX_ENERGY_SLAB_ROWS", "64")
    g = E.debug_energy_geometry(63, 66, 3, 31)
    assert (g["slab_rows"], g["slabs"], g["tiles"]) == (64, 3, 3)  # 129 rows: two full slabs and one of a single row
    split = held(a, b, nperm=31, seed=3, **ALL)
    assert abs(split["e"] - one["e"]) <= 2.0 * R.e_bound(R.restate(a, b, nperm=31, seed=3, **ALL), 4)
    held(a[:62], b, nperm=31, seed=3, **ALL)  # 128 rows: exactly two slabs
    same_bytes(split, E.energy_rows(a, 63, 1, b, 66, 1, nperm=31, seed=3, **ALL))


@pytest.mark.parametrize("k", [1, 2, 16, 17, 32, 33, 40, 256])
def test_used_columns(k):
    got = held(K.normal_rows(23, k, 7), K.normal_rows(17, k, 8, shift=0.2), nperm=17, seed=4, **ALL)
    assert got["nused"] == k


def test_with_ll_and_raw():
    a, b = K.normal_rows(33, 2, 9), K.normal_rows(20, 2, 10, shift=0.5) * np.float32(3.0)
    plain = held(a, b, nperm=16, seed=5, **ALL)
    ll = held(a, b, nperm=16, seed=5, with_ll=True, **ALL)
    raw = held(a, b, nperm=16, seed=5, raw=True, **ALL)
    both = held(a, b, nperm=16, seed=5, with_ll=True, raw=True, **ALL)
    assert (plain["nused"], ll["nused"], raw["nused"], both["nused"]) == (2, 3, 2, 3)
    assert list(plain["flags"]) == [0, 0, R.COL_UNUSED] and list(ll["flags"]) == [0, 0, 0] and list(both["scale"]) == [1.0, 1.0, 1.0]
    assert len({plain["e"], ll["e"], raw["e"], both["e"]}) == 4


def test_the_draw():
    from mcpar_amd import engine as E
    a, b = K.normal_rows(100, 3, 11), K.normal_rows(80, 3, 12, shift=0.3)
    got = held(a, b, n_a=50, n_b=30, nperm=17, seed=77)
    ia, ib = E.debug_draw_indices(77, 100, 0, 50), E.debug_draw_indices(77, 80, 50, 30)
    gathered = held(a[ia], b[ib], nperm=17, seed=77, **ALL)
    assert (got["na_rows"], got["nb_rows"], gathered["na_rows"], gathered["nb_rows"]) == (100, 80, 50, 30)
    for d in (got, gathered):
        del d["na_rows"], d["nb_rows"]
    same_bytes(got, gathered)
    # the same store on both sides does not pick the same rows
    twice = held(a, a, n_a=40, n_b=40, nperm=17, seed=77)
    assert twice["mean_ab"] > 0 and not np.array_equal(E.debug_draw_indices(77, 100, 0, 40), E.debug_draw_indices(77, 100, 40, 40))
    # 0: min(rows, 2048) draws; one side drawn, the other whole
    dflt = held(a, b, nperm=3, seed=5)
    assert (dflt["n_a"], dflt["n_b"]) == (100, 80)
    mixed = held(a, b, n_a=-1, n_b=7, nperm=3, seed=5)
    assert (mixed["n_a"], mixed["n_b"]) == (100, 7)


NC, NP, STEPS = 37, 17, 30
FA, NA, FB, NB = 0, 12, 10, 20


@pytest.fixture(scope="module")
def world():
    from mcpar_amd import engine as E
    eg = run(NC, NP, STEPS)
    ra, rb = eg.samples_range(FA, NA), eg.samples_range(FB, NB)
    W = dict(eg=eg, ra=ra, rb=rb, sa=E.select_chains_rows(ra, NA, NC, list(range(NC))), sb=E.select_chains_rows(rb, NB, NC, list(range(NC))))
    yield W
    W["sa"].close()
    W["sb"].close()
    eg.close()


@pytest.mark.parametrize("kw", [dict(nperm=15, seed=9, **ALL), dict(n_a=60, n_b=0, nperm=16, seed=9, with_ll=True)], ids=["all", "draws"])
def test_the_forms_and_repeats(world, kw):
    from mcpar_amd import engine as E
    W = world
    eg, ra, rb = W["eg"], W["ra"], W["rb"]
    base = E.energy_rows(ra, NA, NC, rb, NB, NC, **kw)
    ref = R.restate(ra, rb, **kw)
    WORST["ratio"] = max(WORST["ratio"], R.check(base, ref, NP + 1, E.debug_energy_sums(ra, NA, NC, rb, NB, NC, **kw)))
    same_bytes(E.energy_rows(ra, NA, NC, rb, NB, NC, **kw), base)
    same_bytes(eg.energy(FA, NA, FB, NB, **kw), base)
    same_bytes(eg.energy(FA, NA, FB, NB, **kw), base)
    same_bytes(E.energy_stores(W["sa"], W["sb"], **kw), base)
    same_bytes(W["sa"].energy(W["sb"], **kw), base)
    same_bytes(eg.energy_store(FA, NA, W["sb"], **kw), base)
    if kw["n_a"] == -1:  # the swap reorders the sums (with draws it also draws other rows)
        swap = E.energy_rows(rb, NB, NC, ra, NA, NC, **kw)
        assert abs(swap["e"] - base["e"]) <= 2.0 * R.e_bound(ref, NP + 1) and swap["mean_aa"] == pytest.approx(base["mean_bb"], rel=1e-12)
    ms = eg.energy_times(FA, NA, FB, NB, **kw)
    assert ms.shape == (7,) and (ms >= 0).all() and ms[4] > 0 and ms[6] >= ms[4]


def test_engine_and_store_refusals(world):
    """the refusals that need a real engine or store (tests/test_energy_cpu.py has those that need none): every one is
    MCX_ERR_INVALID (1) with its own message.  Two stores on different devices cannot be made on one GPU: not run"""
    import ctypes as C
    from mcpar_amd import McxError
    from mcpar_amd import engine as E
    from mcpar_amd._lib import EnergyResultC, EnergySpecC, load
    W = world
    eg, sa, sb = W["eg"], W["sa"], W["sb"]

    def refused(call, text):
        with pytest.raises(McxError) as ei:
            call()
        assert ei.value.code == 1 and text in str(ei.value), (text, str(ei.value))

    # the ranges of both sides
    refused(lambda: eg.energy(-1, 4, 0, 4, **ALL), "steps [-1,3) not in the sample store")
    refused(lambda: eg.energy(0, STEPS + 1, 0, 4, **ALL), "steps [0,%d) not in the sample store" % (STEPS + 1))
    refused(lambda: eg.energy(0, 12, STEPS - 5, 6, **ALL), "B: steps [%d,%d) not in the sample store" % (STEPS - 5, STEPS + 1))
    refused(lambda: eg.energy(0, 12, -2, 6, **ALL), "B: steps [-2,4) not in the sample store")
    refused(lambda: eg.energy(0, 0, 0, 4, **ALL), "nsteps_a = 0, nsteps_b = 4")
    refused(lambda: eg.energy(0, 4, 0, -1, **ALL), "nsteps_a = 4, nsteps_b = -1")
    refused(lambda: eg.energy_store(0, 0, sb, **ALL), "nsteps = 0")
    refused(lambda: eg.energy_store(STEPS - 2, 3, sb, **ALL), "steps [%d,%d) not in the sample store" % (STEPS - 2, STEPS + 1))
    # the spec on every engine and store entry: permutations and sizes outside the limits
    for call in (lambda **kw: eg.energy(FA, NA, FB, NB, **kw), lambda **kw: eg.energy_store(FA, NA, sb, **kw),
                 lambda **kw: E.energy_stores(sa, sb, **kw), lambda **kw: eg.energy_times(FA, NA, FB, NB, **kw)):
        refused(lambda: call(nperm=-1), "spec.nperm = -1")
        refused(lambda: call(nperm=E.ENERGY_MAX_PERM + 1), "spec.nperm = %d" % (E.ENERGY_MAX_PERM + 1))
        refused(lambda: call(n_a=-2), "spec.n_a = -2")
        refused(lambda: call(n_a=1), "1 rows of side a")
        refused(lambda: call(n_b=E.ENERGY_MAX_SIDE + 1), "%d rows of side b" % (E.ENERGY_MAX_SIDE + 1))
    # unknown flags and a NULL res or store, which the Python forms cannot express
    L, res = load(), EnergyResultC()
    bad, ok = EnergySpecC(-1, -1, 3, 0, 4), EnergySpecC(-1, -1, 3, 0, 0)
    err = L.mcx_last_error
    assert L.mcx_samples_energy(eg.h, FA, NA, FB, NB, C.byref(bad), C.byref(res), None, None) == 1 and b"spec.flags = 4" in err()
    assert L.mcx_samples_energy_store(eg.h, FA, NA, sb.h, C.byref(bad), C.byref(res), None, None) == 1 and b"spec.flags = 4" in err()
    assert L.mcx_store_energy(sa.h, sb.h, C.byref(bad), C.byref(res), None, None) == 1 and b"spec.flags = 4" in err()
    assert L.mcx_samples_energy(eg.h, FA, NA, FB, NB, C.byref(ok), None, None, None) == 1 and b"res is NULL" in err()
    assert L.mcx_samples_energy_store(eg.h, FA, NA, sb.h, C.byref(ok), None, None, None) == 1 and b"res is NULL" in err()
    assert L.mcx_samples_energy_store(eg.h, FA, NA, None, C.byref(ok), C.byref(res), None, None) == 1 and b"store b is NULL" in err()
    assert L.mcx_store_energy(sa.h, sb.h, C.byref(ok), None, None, None) == 1 and b"res is NULL" in err()
    assert L.mcx_store_energy(sa.h, None, C.byref(ok), C.byref(res), None, None) == 1 and b"store b is NULL" in err()
    # a store of another column count, and one too small to give two rows
    other = E.select_chains_rows(K.normal_rows(40, 2, 21), 8, 5, [0, 1])
    refused(lambda: eg.energy_store(0, 8, other, **ALL), "A has %d columns and B 3" % (NP + 1))
    refused(lambda: E.energy_stores(sa, other, **ALL), "A has %d columns and B 3" % (NP + 1))
    refused(lambda: other.energy(sa, **ALL), "A has 3 columns and B %d" % (NP + 1))
    other.close()
    one = E.select_chains_rows(W["ra"][:NC], 1, NC, [0])
    refused(lambda: E.energy_stores(sa, one, **ALL), "1 rows of side b")
    refused(lambda: eg.energy_store(FA, NA, one, n_b=0), "1 rows of side b")
    one.close()
    # and the engine still answers
    same_bytes(eg.energy(FA, NA, FB, NB, nperm=15, seed=9, **ALL), E.energy_rows(W["ra"], NA, NC, W["rb"], NB, NC, nperm=15, seed=9, **ALL))


def test_dropped_columns():
    a, b = K.normal_rows(33, 5, 13), K.normal_rows(20, 5, 14, shift=0.25)
    keep = [0, 2, 4, 5]
    want = held(a[:, keep], b[:, keep], nperm=17, seed=6, **ALL)
    bound = R.e_bound(R.restate(a[:, keep], b[:, keep], nperm=17, seed=6, **ALL), 6)

    def near(got):
        assert got["nused"] == 3 and abs(got["e"] - want["e"]) <= 2.0 * bound and (np.abs(got["perm_e"] - want["perm_e"]) <= 2.0 * bound).all()
        assert got["nge"] == want["nge"]

    a1, b1 = a.copy(), b.copy()
    a1[:, 1] = b1[:, 1] = 7.25         # a constant column
    a1[:, 3] = 0.5
    a1[3, 3], a1[9, 3], b1[0, 3] = K.NAN, K.INF, -K.INF
    got = held(a1, b1, nperm=17, seed=6, **ALL)
    assert list(got["flags"]) == [0, R.COL_CONSTANT, 0, R.COL_NONFINITE, 0, R.COL_UNUSED] and got["scale"][1] == 0.0
    near(got)
    a2, b2 = a1.copy(), b1.copy()
    a2[:, 1], b2[:, 1] = -0.0, 0.0     # -0 against +0: one point, constant; under raw a column of zero distances
    got = held(a2, b2, nperm=17, seed=6, **ALL)
    assert list(got["flags"]) == [0, R.COL_CONSTANT, 0, R.COL_NONFINITE, 0, R.COL_UNUSED]
    near(got)
    raw_want = held(a[:, keep], b[:, keep], nperm=17, seed=6, raw=True, **ALL)
    raw = held(a2, b2, nperm=17, seed=6, raw=True, **ALL)
    assert list(raw["flags"]) == [0, 0, 0, R.COL_NONFINITE, 0, R.COL_UNUSED] and raw["nused"] == 4
    assert abs(raw["e"] - raw_want["e"]) <= 2.0 * R.e_bound(R.restate(a[:, keep], b[:, keep], nperm=17, seed=6, raw=True, **ALL), 6)
    # every column dropped
    a3, b3 = a2.copy(), b2.copy()
    a3[:, [0, 2, 4]] = b3[:, [0, 2, 4]] = 1.0
    none = held(a3, b3, nperm=17, seed=6, **ALL)
    assert none["nused"] == 0 and math.isnan(none["e"]) and math.isnan(none["p_value"]) and np.isnan(none["perm_e"]).all()


def test_identical_sides():
    a = K.normal_rows(40, 3, 15)
    got = held(a, a.copy(), nperm=19, seed=8, **ALL)
    assert abs(got["e"]) <= R.e_bound(R.restate(a, a, nperm=19, seed=8, **ALL), 4) and got["p_value"] == 1.0 and got["nge"] == 19


def test_the_finding_that_motivates_the_feature():
    """equal marginals, another joint law: the column-wise comparison sees nothing, the energy test sees it at once"""
    from mcpar_amd import engine as E
    c = K.FINDING
    a, b, bc = K.finding_rows()
    kw = dict(nperm=c["nperm"], seed=c["seed"], **ALL)
    same, corr = held(a, b, **kw), held(a, bc, **kw)
    assert same["p_value"] >= 0.05
    assert corr["p_value"] == 1.0 / 200.0 and corr["nge"] == 0
    cmp_ = E.compare_rows(a, c["na"], 1, bc, c["nb"], 1, iid=True)
    assert (cmp_["ks_p"][:2] > 0.01).all()
    # (and the reference alone meets all three)
    ra, rc = R.restate(a, b, **kw), R.restate(a, bc, **kw)
    assert ra["p_value"] >= 0.05 and rc["p_value"] == 1.0 / 200.0
    assert (CR.restate(a, c["na"], 1, bc, c["nb"], 1, iid=True)["ks_p"][:2] > 0.01).all()


def test_report_the_worst_ratio():
    print("\nenergy: largest error / bound seen = %.4g" % WORST["ratio"])
    assert WORST["ratio"] <= 1.0
