"""The mutual information between columns of a store on the GPU against the float64 restatement
tests/mutinfo_ref.py: eps, na, nb of k_mi_pairs itself, nzero, ndup, m, every flag and integer field exact; mi and every perm_mi
within the bound mutinfo_ref.mi_bound derives for a fixed-order fp64 sum of 2 m table values; scale within 4 n 2^-53 relative;
nge and p_value as the definition gives them from the returned perm_mi, and the reference's wherever no reference value lies
within twice the bound of mi.

The shapes are the smallest at which the kernel can go wrong: m around the wavefront, the tile of 512 queries and the stage of
1024 points, two and three stages under the lowered knob, every k that has an instance at its ends, ties at eps, repeats, flagged
columns.  WORST collects the largest error / bound seen (printed by the last test; DESIGN.md records it)."""
import math

import numpy as np
import pytest

import mutinfo_cases as K
import mutinfo_ref as R
from test_gpu_store_view import run

pytestmark = pytest.mark.gpu

WORST = {"ratio": 0.0}


def held(rows, nc=1, counts=((0, 0),), **kw):
    """rows_mutual_info of host rows held to the restatement made with its scale; for each (pair, p) of counts that is computed,
    the kernel's own eps, na, nb against the restatement's, exactly -> the result"""
    from mcpar_amd import engine as E
    kw.setdefault("n", -1)
    got = E.rows_mutual_info(rows, len(rows) // nc, nc, **kw)
    ref = R.restate(rows, scale=got["scale"], **kw)
    WORST["ratio"] = max(WORST["ratio"], R.check(got, ref))
    for pair, p in counts:
        if ref["pairs"][pair]["flags"] & (R.PAIR_UNUSED | R.PAIR_FEW):
            continue
        eps, na, nb = E.debug_mutinfo_counts(rows, len(rows) // nc, nc, pair, p, **kw)
        weps, wna, wnb = R.counts_of(ref, pair, p)
        assert eps.tobytes() == weps.tobytes() and np.array_equal(na, wna) and np.array_equal(nb, wnb), (pair, p)
        if p == 0:  # the host's finish on the kernel's integers is the call's mi up to the order of the sum
            o = ref["pairs"][pair]
            assert abs(E.mutinfo_finish(eps, na, nb, ref["k"])[0] - got["pairs"][pair]["mi"]) <= 2.0 * o["bound"]
    return got


def same_bytes(a, b):
    a, b = R.flat(a), R.flat(b)
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


@pytest.mark.parametrize("k", [1, 2, 3, 8])
@pytest.mark.parametrize("m", [2, 63, 64, 65])
def test_small_sizes(m, k):
    got = held(K.normal_pair(m, 0.5, m), k=k, nperm=1, seed=3, counts=((0, 0), (0, 1)))
    assert got["pairs"][0]["flags"] == (R.PAIR_FEW if m <= k else 0)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 8])
def test_k_plus_one_points(k):
    """m = k + 1: every other point is a neighbour, eps is the largest distance and the counts are at most k - 1"""
    got = held(K.normal_pair(k + 1, 0.3, 20 + k), k=k, nperm=2, seed=k, counts=((0, 0), (0, 2)))
    assert got["m"] == k + 1 and got["pairs"][0]["flags"] == 0
    few = held(K.normal_pair(k, 0.3, 20 + k), k=k) if k >= 2 else None
    assert few is None or (few["pairs"][0]["flags"] == R.PAIR_FEW and math.isnan(few["pairs"][0]["mi"]))


@pytest.mark.parametrize("m", [511, 512, 513, 1023, 1024, 1025])
def test_around_the_tile_and_the_stage(m):
    from mcpar_amd import engine as E
    g = E.debug_mutinfo_geometry(m, 1, 1, 3)
    assert (g["tiles"], g["stages"]) == ((m + 511) // 512, (m + 1023) // 1024)
    held(K.normal_pair(m, 0.6, m), nperm=1, seed=5, counts=((0, 0), (0, 1)))


@pytest.mark.parametrize("m, stages", [(128, 2), (129, 3), (190, 3), (600, 10)])
def test_stage_split(monkeypatch, m, stages):
    """the lowered stage: the same integers exactly, the same mi up to the bound (the order of the sum does not change with the
    stage, so in fact the same bytes), also where the tile's own points span several stages and where a stage spans two tiles"""
    from mcpar_amd import engine as E
    rows = K.normal_rows(m, 3, 7)
    kw = dict(nperm=2, seed=9, k=2)
    monkeypatch.delenv("MCX_MUTINFO_STAGE_ROWS", raising=False)
    one = held(rows, counts=((1, 0), (2, 2)), **kw)
    c1 = E.debug_mutinfo_counts(rows, m, 1, 1, 1, n=-1, **kw)
    monkeypatch.setenv("MCX_MUTINFO_STAGE_ROWS", "64")
    assert E.debug_mutinfo_geometry(m, 3, 2, 2)["stages"] == stages
    split = held(rows, counts=((1, 0), (2, 2)), **kw)
    c2 = E.debug_mutinfo_counts(rows, m, 1, 1, 1, n=-1, **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(c1, c2))
    ref = R.restate(rows, scale=one["scale"], n=-1, **kw)
    for i, o in enumerate(ref["pairs"]):
        assert abs(split["pairs"][i]["mi"] - one["pairs"][i]["mi"]) <= 2.0 * o["bound"]
        assert (np.abs(split["perm_mi"][i] - one["perm_mi"][i]) <= 2.0 * o["perm_bound"]).all()
    for f in ("nzero", "nge", "flags", "a", "b"):
        assert np.array_equal(split["pairs"][f], one["pairs"][f])
    same_bytes(split, E.rows_mutual_info(rows, m, 1, n=-1, **kw))


@pytest.mark.parametrize("k", [1, 3, 8])
def test_ties_at_eps(k):
    """integer-valued floats under raw: many distances equal eps exactly (< against <=), the k-th counts with multiplicity, and
    some points have all k neighbours at distance 0 (nzero)"""
    rows = K.integer_rows(150, 3, 11)
    got = held(rows, k=k, raw=True, nperm=1, seed=2, counts=((0, 0), (1, 0), (2, 1)))
    assert got["ndup"] > 0 and ((got["pairs"]["nzero"] > 0).all() if k <= 3 else (got["pairs"]["nzero"] == 0).all())  # (36 cells, 103 points)
    assert ((got["pairs"]["flags"] & R.PAIR_TIES) != 0).tolist() == (got["pairs"]["nzero"] > 0).tolist()
    wide = held(K.integer_rows(120, 2, 12, span=40), k=k, raw=True, counts=((0, 0),))
    assert wide["m"] > 100


def test_neighbours_at_zero_in_one_column_only():
    rows = K.one_column_ties(200, 13)
    got = held(rows, k=3, counts=((0, 0),), nperm=1, seed=1)
    eps, na, nb = R.counts_of(R.restate(rows, scale=got["scale"], n=-1, k=3), 0, 0)
    assert got["ndup"] == 0 and got["pairs"][0]["nzero"] == 0 and (eps > 0).all() and (na >= 3).all()
    # (and swapped: the tied column second)
    held(rows, k=3, pairs=[(1, 0)], counts=((0, 0),))


def test_repeated_rows():
    rows = K.repeated_rows(300, 3, 14)
    got = held(rows, nc=3, nperm=2, seed=4, counts=((0, 0), (2, 1)))
    assert got["ndup"] == 200 and got["m"] == 100 and got["n_sel"] == 300
    spaced = held(rows, nc=3, n=100)      # rows 0, 3, 6, ...: the repeats fall between the rows taken
    assert spaced["ndup"] == 0 and spaced["m"] == 100
    same = np.repeat(K.normal_rows(3, 2, 15), 20, axis=0)    # three points in all: m <= k
    few = held(same)
    assert few["m"] == 3 and few["ndup"] == 57 and few["pairs"][0]["flags"] == R.PAIR_FEW


def test_flagged_columns():
    rows = K.normal_rows(80, 4, 16)
    rows[:, 1] = 0.25
    rows[17, 2] = K.NAN
    got = held(rows, nperm=3, seed=5, counts=((2, 0), (2, 3)))
    assert list(got["flags"]) == [0, R.COL_CONSTANT, R.COL_NONFINITE, 0, R.COL_UNUSED] and got["nused"] == 2
    assert [int(f) for f in got["pairs"]["flags"]] == [R.PAIR_UNUSED, R.PAIR_UNUSED, 0, R.PAIR_UNUSED, R.PAIR_UNUSED, R.PAIR_UNUSED]
    assert np.isnan(got["perm_mi"][[0, 1, 3, 4, 5]]).all() and not np.isnan(got["perm_mi"][2]).any()
    # the computed pair is the pair of the two clean columns alone
    alone = held(np.ascontiguousarray(rows[:, [0, 3, 4]]), nperm=3, seed=5)
    assert alone["pairs"][0]["mi"] == got["pairs"][2]["mi"] and np.array_equal(alone["perm_mi"][0], got["perm_mi"][2])
    raw = held(rows, raw=True, counts=((0, 0),))
    # raw lets the constant column through: its distances are all 0, the joint distance is the other column's, na = k - 1 and
    # nb = m - 1 everywhere, and the estimate is psi(k) + psi(m) - psi(k) - psi(m)
    assert list(raw["flags"]) == [0, 0, R.COL_NONFINITE, 0, R.COL_UNUSED] and raw["pairs"][0]["flags"] == 0
    assert abs(raw["pairs"][0]["mi"]) <= 1e-12 and math.isnan(raw["pairs"][0]["pearson"])
    rows[:, [0, 3]] = 1.0
    none = held(rows)
    assert none["nused"] == 0 and none["ndup"] == 0 and (none["pairs"]["flags"] == R.PAIR_UNUSED).all()


def test_one_pair_and_every_pair_of_seventeen():
    one = held(K.normal_rows(70, 2, 17))
    assert one["npairs"] == 1 and (one["pairs"][0]["a"], one["pairs"][0]["b"]) == (0, 1)
    rows = K.normal_rows(90, 16, 18)
    got = held(rows, with_ll=True, counts=((0, 0), (135, 0), (77, 0)))
    assert got["npairs"] == 136 and got["nused"] == 17 and (got["pairs"][135]["a"], got["pairs"][135]["b"]) == (15, 16)


def test_named_pairs():
    rows = K.normal_rows(120, 4, 19)
    rows[:, 2] = rows[:, 0] ** 2 + np.float32(0.1) * rows[:, 2]
    pairs = [(2, 0), (0, 2), (3, 1), (0, 4), (2, 0)]
    got = held(rows, pairs=pairs, with_ll=True, nperm=17, seed=6, counts=((0, 0), (1, 5), (3, 17), (4, 1)))
    assert [(int(o["a"]), int(o["b"])) for o in got["pairs"]] == pairs and got["perm_mi"].shape == (5, 17)
    assert got["pairs"][0]["mi"] == got["pairs"][4]["mi"] and np.array_equal(got["perm_mi"][0], got["perm_mi"][4])
    # (b, a) permutes the other column: the same mi at p = 0 up to the order of the sum, another null
    ref = R.restate(rows, scale=got["scale"], n=-1, pairs=pairs, with_ll=True, nperm=17, seed=6)
    assert abs(got["pairs"][0]["mi"] - got["pairs"][1]["mi"]) <= 2.0 * ref["pairs"][0]["bound"]
    assert not np.array_equal(got["perm_mi"][0], got["perm_mi"][1])
    assert got["pairs"][0]["mi"] > 0.5 and got["pairs"][0]["p_value"] == 1.0 / 18.0 and got["pairs"][2]["p_value"] > 1.0 / 18.0


@pytest.mark.parametrize("nperm", [0, 1, 17])
def test_nperm(nperm):
    got = held(K.normal_pair(130, 0.7, 21), nperm=nperm, seed=7, counts=((0, 0), (0, nperm)))
    assert got["perm_mi"].shape == (1, nperm)
    if nperm == 17:
        assert got["pairs"][0]["nge"] == 0 and got["pairs"][0]["p_value"] == 1.0 / 18.0


def test_raw_and_with_ll():
    rows = K.normal_rows(100, 2, 22) * np.float32(3.0)
    plain, ll = held(rows), held(rows, with_ll=True, counts=((0, 0), (2, 0)))
    raw, both = held(rows, raw=True), held(rows, raw=True, with_ll=True)
    assert (plain["npairs"], ll["npairs"], raw["nused"], both["nused"]) == (1, 3, 2, 3)
    assert list(plain["flags"]) == [0, 0, R.COL_UNUSED] and list(both["scale"]) == [1.0, 1.0, 1.0]
    # the pair of the two parameters under with_ll: the same points unless log L tells two rows apart that the parameters do not
    assert ll["pairs"][0]["mi"] == plain["pairs"][0]["mi"]


def test_the_row_rule_on_the_device():
    """n of N rows, gathered on the device: the same as the call on those rows alone"""
    from mcpar_amd import engine as E
    rows = K.normal_rows(1000, 3, 23)
    got = held(rows, nc=10, n=77, nperm=2, seed=8)
    idx = E.debug_mutinfo_rows(1000, 77)
    alone = held(np.ascontiguousarray(rows[idx]), nperm=2, seed=8)
    assert (got["n_rows"], got["n_sel"], alone["n_rows"]) == (1000, 77, 77)
    a, b = R.flat(got), R.flat(alone)
    del a["n_rows"], b["n_rows"]
    assert all(a[f].tobytes() == b[f].tobytes() for f in a)


NC, NP, STEPS = 37, 17, 30


@pytest.fixture(scope="module")
def world():
    from mcpar_amd import engine as E
    eg = run(NC, NP, STEPS)
    rows = eg.samples_range(0, STEPS)
    W = dict(eg=eg, rows=rows, st=E.select_chains_rows(rows, STEPS, NC, list(range(NC))))
    yield W
    W["st"].close()
    eg.close()


@pytest.mark.parametrize("kw", [dict(n=-1, nperm=3, seed=9, pairs=[(0, 1), (16, 3), (5, 17)], with_ll=True), dict(n=200, k=2)],
                         ids=["all", "spaced"])
def test_the_forms_and_repeats(world, kw):
    from mcpar_amd import engine as E
    W = world
    eg, rows = W["eg"], W["rows"]
    base = E.rows_mutual_info(rows, STEPS, NC, **kw)
    WORST["ratio"] = max(WORST["ratio"], R.check(base, R.restate(rows, scale=base["scale"], **kw)))
    assert base["n_rows"] == STEPS * NC and base["m"] + base["ndup"] == base["n_sel"]
    same_bytes(E.rows_mutual_info(rows, STEPS, NC, **kw), base)
    same_bytes(eg.mutual_info(**kw), base)
    same_bytes(eg.mutual_info(0, STEPS, **kw), base)
    same_bytes(W["st"].mutual_info(**kw), base)
    same_bytes(W["st"].mutual_info(**kw), base)
    part = eg.mutual_info(5, 12, **dict(kw, n=min(kw["n"], 12 * NC)))
    same_bytes(part, E.rows_mutual_info(rows[5 * NC:17 * NC], 12, NC, **dict(kw, n=min(kw["n"], 12 * NC))))
    ms = eg.mutual_info_times(**kw)
    assert ms.shape == (8,) and (ms >= 0).all() and ms[4] > 0 and ms[7] >= ms[4]


def test_engine_and_store_refusals(world):
    """the refusals that need a real engine or store (tests/test_mutinfo_cpu.py has those that need none)"""
    from mcpar_amd import McxError
    W = world
    eg, st = W["eg"], W["st"]

    def refused(call, text):
        with pytest.raises(McxError) as ei:
            call()
        assert ei.value.code == 1 and text in str(ei.value), (text, str(ei.value))

    refused(lambda: eg.mutual_info(-1, 4), "steps [-1,3) not in the sample store")
    refused(lambda: eg.mutual_info(0, STEPS + 1), "steps [0,%d) not in the sample store" % (STEPS + 1))
    refused(lambda: eg.mutual_info(0, 0), "nsteps = 0")
    for call in (lambda **kw: eg.mutual_info(**kw), lambda **kw: st.mutual_info(**kw), lambda **kw: eg.mutual_info_times(**kw)):
        refused(lambda: call(k=9), "spec.k = 9")
        refused(lambda: call(nperm=1000), "spec.nperm = 1000")
        refused(lambda: call(n=STEPS * NC + 1), "%d rows" % (STEPS * NC + 1))
        refused(lambda: call(pairs=[(0, 17)]), "spec.pairs[0] = (0, 17)")
    same_bytes(eg.mutual_info(n=100), st.mutual_info(n=100))


def test_the_finding_that_motivates_the_feature():
    """a curved valley: no correlation to speak of, more than a nat of mutual information -- the CPU test's assertions on the GPU"""
    got = held(K.curved_pair(1000, K.CURVED_SEED), k=3)
    o = got["pairs"][0]
    assert o["mi"] >= 1.0 and abs(o["pearson"]) <= 0.2 and o["r_info"] > 0.9
    null = held(K.curved_pair(400, K.CURVED_NULL_SEED), k=3, nperm=19, seed=1, counts=())
    assert null["pairs"][0]["p_value"] == 1.0 / 20.0


def test_report_the_worst_ratio():
    print("\nmutual information: largest error / bound seen = %.4g" % WORST["ratio"])
    assert WORST["ratio"] <= 1.0
