"""mcx_*_compare on the GPU against tests/compare_ref.py.

Every case is held to the restatement by compare_ref.check: the integer fields, ks and the two points bit for bit; w1 at 1e-10
relative (all terms are non-negative, so a fixed-order fp64 sum of at most 2^20 terms is within 2^20 * 2^-53 = 1.2e-10 of any
other order); mean and sd at 1e-9 and ess at 1e-4, the tolerances of tests/test_gpu_summary.py.  Each test prints the largest
relative difference of w1 it saw (pytest -s shows it).

The tile-edge stores have NA = 8193 and NB = 16400 with a run of one value across sorted position 8192 on both sides.  With those
sizes no pair of stores keeps every window of both sweeps within 8192 keys: A's first tile ends inside A's run, which is A's
maximum, so its window is every key of B up to that value; were that at most 8192 keys, B's run -- which holds positions 8191
and 8192 of B -- would lie above A's maximum, and the window of B's first tile would be all 8193 keys of A.  So the variants
cross the switch between them: "overlap" (one range, one run value: the first tile of either side spans more than 8192 keys of
the other, the global path), "above" (every tile of A in LDS, B's first tile global), and a third, "inside", with B cut to 8000
values that all lie inside the window of A's first tile: every window of both sweeps in LDS.

The BIG pair (2 105 349 x 1 against 100 001 x 3) crosses what the others do not reach: side A alone has more than 256 sort tiles
(the second carry step of the sort's scans, with another stride than B's), a second workgroup of k_cmp_bounds, lanes of
k_cmp_reduce that take two tiles and a step chunk of 65.  Its reference is compare_ref.distances_numpy (no Python loop; pinned
to distances() in tests/test_compare_cpu.py) held by compare_ref.check with its rel_w1; mean, sd and ess of a side are the bytes
of rows_summary of that side.  Both columns are built from their pooled order, so that the maxima of D+ lie where the case wants them.
Equal values of D+ at two points need the same remainder of cA NB modulo NA: with gcd(NA, NB) = 3 they lie a multiple of
NA / 3 = 701 783 keys of A (85.7 tiles) apart, so with these sizes no two tiles of one reducer lane (256 tiles apart) can tie.
Column 0 therefore has its three equal maxima in tiles 0, 86 and 171 (three lanes; the lowest position wins), and the lane
that takes two tiles is crossed by column 1, whose only maximum lies in tile 257, behind a lower one in tile 1.  One case holds
both, since a summary of one chain of two million steps costs the library a second, whatever the columns."""
import numpy as np
import pytest

import compare_cases as K
import compare_ref as R
from test_gpu_steptable import same_but_nan
from test_gpu_store_view import run

pytestmark = pytest.mark.gpu

NAN, INF = K.NAN, K.INF


def same_result(a, b):
    return sorted(a) == sorted(b) and all(same_but_nan(a[k], b[k]) for k in a)


def held(got, a, Ta, nca, b, Tb, ncb, iid=False, what=""):
    worst = R.check(got, R.restate(a, Ta, nca, b, Tb, ncb, iid))
    print("%s: largest relative difference of w1 %.3g" % (what, worst))
    return worst


def rows_case(a, Ta, nca, b, Tb, ncb, iid=False, what=""):
    from mcpar_amd import engine as E
    got = E.compare_rows(a, Ta, nca, b, Tb, ncb, iid)
    held(got, a, Ta, nca, b, Tb, ncb, iid, what)
    return got


# ---- 1. ties and shared values ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iid", [False, True])
def test_ties_and_shared_values(iid):
    a, b = K.tie_rows(3, 5, 37, 1), K.tie_rows(3, 9, 11, 2, shift=0.25)
    got = rows_case(a, 37, 5, b, 11, 9, iid, "ties 3 columns")
    assert (got["na"] == 185).all() and (got["nb"] == 99).all() and (got["ks_plus_num"] + got["ks_minus_num"] > 0).all()
    if iid:
        assert (got["ess_a"] == 185).all() and (got["ess_b"] == 99).all()


def test_grouped_columns_give_the_same_bytes(monkeypatch):
    from mcpar_amd import engine as E
    a, b = K.tie_rows(17, 5, 37, 3), K.tie_rows(17, 9, 11, 4, shift=-0.25)
    assert E.debug_compare_geometry(185, 99, 18)["group_cols"] == 18
    whole = rows_case(a, 37, 5, b, 11, 9, what="ties 18 columns")
    monkeypatch.setenv("MCX_COMPARE_GROUP_COLS", "4")
    assert E.debug_compare_geometry(185, 99, 18)["group_cols"] == 4
    assert same_result(E.compare_rows(a, 37, 5, b, 11, 9), whole)


# ---- 2. tile edges -----------------------------------------------------------------------------------------------------------------
def windows(self_col, other_col):
    """the window sizes of the tiles of self in other, as k_cmp_bounds forms them"""
    s, o = np.sort(R.ckey(self_col)), np.sort(R.ckey(other_col))
    last = s[np.minimum(np.arange(K.TILE, s.size + K.TILE, K.TILE), s.size) - 1]
    ob = np.concatenate([[0], np.searchsorted(o, last, "right")])
    return np.diff(ob)


def edge_stores(variant):
    rng = np.random.default_rng([5, len(variant)])
    NA, NB = 8193, 16400
    if variant == "overlap":  # the same range and the same run value on both sides
        xa = K.straddle(NA, 1.0, 8090, 103, rng, 0.0, 2.0)
        xb = K.straddle(NB, 1.0, 8140, 110, rng, 0.0, 2.0)
    elif variant == "above":  # 8000 values of B below A's run, B's run and the rest above it
        xa = K.straddle(NA, 1.0, 8090, 103, rng, 0.0, 2.0)
        xb = np.concatenate([rng.uniform(0.0, 0.99, 8000).astype(np.float32), K.straddle(NB - 8000, 1.5, 140, 110, rng, 1.01, 2.0)])
        xb = rng.permutation(xb)
    else:  # "inside": B cut to 8000 values, all inside A's first tile
        xa = K.straddle(NA, 1.0, 8090, 103, rng, 0.0, 2.0)
        xb = rng.uniform(0.0, 0.99, 8000).astype(np.float32)
        xb[:150] = xa[xa < 0.99][:150]  # shared values
    return K.one_col_rows(xa, rng), K.one_col_rows(xb, rng)


@pytest.mark.parametrize("variant", ["overlap", "above", "inside"])
def test_tile_edges(variant):
    from mcpar_amd import engine as E
    a, b = edge_stores(variant)
    nca, Ta = 3, 2731
    ncb, Tb = (2, 8200) if variant != "inside" else (2, 4000)
    assert a.shape[0] == nca * Ta == 8193 and b.shape[0] == ncb * Tb
    g = E.debug_compare_geometry(a.shape[0], b.shape[0], 2)
    assert (g["tile_keys"], g["tiles_a"], g["tiles_b"]) == (K.TILE, 2, 3 if variant != "inside" else 1)
    wa, wb = windows(a[:, 0], b[:, 0]), windows(b[:, 0], a[:, 0])
    W = g["window_lds_keys"]
    assert len(wa) == g["tiles_a"] and len(wb) == g["tiles_b"]
    if variant == "overlap":
        assert wa[0] > W and wb[0] > W
    elif variant == "above":
        assert (wa <= W).all() and wa[0] == 8000 and wb[0] > W
    else:
        assert (wa <= W).all() and wa[0] == 8000 and (wb <= W).all() and wb[0] > 7000
    sa, sb = np.sort(a[:, 0]), np.sort(b[:, 0])
    assert sa[8191] == sa[8192] == sa[8090] and (variant == "inside" or sb[8191] == sb[8192] == sb[8140])  # the runs straddle
    rows_case(a, Ta, nca, b, Tb, ncb, what="tile edges, " + variant)


# ---- 3. 64-bit products ------------------------------------------------------------------------------------------------------------
def test_products_beyond_32_bits():
    rng = np.random.default_rng(9)
    nc, T = 64, 1100
    N = nc * T
    a = np.stack([rng.uniform(0.0, 1.0, N), -rng.uniform(2.0, 3.0, N)], axis=1).astype(np.float32)
    b = np.stack([rng.uniform(2.0, 3.0, N), -rng.uniform(0.0, 1.0, N)], axis=1).astype(np.float32)
    assert a[:, 0].max() < 1.0 and b[:, 0].min() >= 2.0 and N == 70400
    got = rows_case(a, T, nc, b, T, nc, what="disjoint supports")
    assert N * N > 2 ** 32
    for c in (0, 1):  # every value of A lies below every value of B
        assert got["ks_plus_num"][c] == N * N and got["ks_minus_num"][c] == 0 and got["ks"][c] == 1.0
        want = b[:, c].astype(np.float64).mean() - a[:, c].astype(np.float64).mean()
        assert want > 1.0 and abs(got["w1"][c] - want) <= 1e-10 * want, (c, got["w1"][c], want)


# ---- 4. degenerate -----------------------------------------------------------------------------------------------------------------
def test_the_same_store_on_both_sides():
    a = K.tie_rows(3, 5, 37, 6)
    a[:, 1] = 2.5  # a constant column
    got = rows_case(a, 37, 5, a, 37, 5, what="the same store")
    assert not got["ks_plus_num"].any() and not got["ks_minus_num"].any() and not got["ks"].any() and not got["w1"].any()
    live = [0, 2, 3]
    assert (got["ks_p"][live] == 1.0).all() and (got["z_mean"][live] == 0.0).all()
    assert np.isnan(got["ess_a"][1]) and np.isnan(got["ks_p"][1]) and np.isnan(got["z_mean"][1])
    assert got["ks_plus_x"][1] == 2.5 == got["ks_minus_x"][1]


def test_signed_zeros_are_one_point():
    a = np.full((12, 2), -0.0, np.float32)
    b = np.full((20, 2), 0.0, np.float32)
    got = rows_case(a, 4, 3, b, 5, 4, what="signed zeros")
    assert not got["ks_plus_num"].any() and not got["ks_minus_num"].any() and (got["w1"] == 0.0).all() and (got["ks"] == 0.0).all()
    assert (got["ks_plus_x"] == 0.0).all() and not np.signbit(got["ks_plus_x"]).any()


@pytest.mark.parametrize("Ta, nca, Tb, ncb", [(1, 1, 1, 1), (1, 1, 41, 203), (2, 3, 3, 1), (3, 2, 40, 7)])
def test_short_and_one_row_stores(Ta, nca, Tb, ncb):
    rng = np.random.default_rng([Ta, nca, Tb, ncb])
    a = rng.normal(0, 1, (Ta * nca, 3)).astype(np.float32)
    b = rng.normal(0, 1, (Tb * ncb, 3)).astype(np.float32)
    got = rows_case(a, Ta, nca, b, Tb, ncb, what="%d x %d against %d x %d" % (Ta, nca, Tb, ncb))
    assert (got["ess_a"] == Ta * nca).all()
    if Ta * nca == 1:
        assert np.isnan(got["sd_a"]).all() and np.isnan(got["z_mean"]).all() and np.isfinite(got["ks_p"]).all()


# ---- 5. non-finite -----------------------------------------------------------------------------------------------------------------
def test_non_finite_columns():
    a, b = K.tie_rows(3, 5, 37, 7), K.tie_rows(3, 9, 11, 8)
    a[50, 3] = -INF
    b[17, 0] = NAN
    a[3, 1] = INF
    b[90, 1] = INF
    got = rows_case(a, 37, 5, b, 11, 9, what="non-finite")
    assert got["flags"].tolist() == [R.NONFINITE_B, R.NONFINITE_A | R.NONFINITE_B, 0, R.NONFINITE_A]
    for c in (0, 1, 3):
        for f in R.NAN_WHEN_FLAGGED:
            assert np.isnan(got[f][c]), (c, f)
        assert got["ks"][c] > 0 and got["ks_plus_num"][c] >= 0 and got["ks_minus_num"][c] >= 0
    assert np.isnan(got["mean_b"][0]) and np.isfinite(got["mean_a"][0]) and np.isfinite(got["ess_a"][0])
    assert np.isnan(got["mean_a"][3]) and np.isfinite(got["mean_b"][3])
    assert np.isfinite(got["w1"][2]) and np.isfinite(got["ks_p"][2])
    # (the order defines the KS fields of the flagged columns: held() has compared them with the restatement's, bit for bit)


# ---- 6. the forms agree ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    eg = run(37, 3, 30)
    yield eg
    eg.close()


def swapped(d):
    pairs = dict(ks_plus_num="ks_minus_num", ks_plus_x="ks_minus_x", mean_a="mean_b", sd_a="sd_b", ess_a="ess_b", na="nb")
    pairs.update({v: k for k, v in pairs.items()})
    out = {pairs.get(k, k): v for k, v in d.items()}
    out["flags"] = ((d["flags"] & 1) << 1) | ((d["flags"] & 2) >> 1)
    out["z_mean"] = -d["z_mean"]
    return out


def test_forms_agree(engine):
    from mcpar_amd import engine as E
    eg = engine
    fa, na, fb, nb = 0, 12, 10, 20  # the ranges overlap
    ra, rb = eg.samples_range(fa, na), eg.samples_range(fb, nb)
    got = eg.compare(fa, na, fb, nb)
    held(got, ra, na, 37, rb, nb, 37, what="two ranges of an engine")
    assert same_result(eg.compare(fa, na, fb, nb), got)  # two calls
    assert same_result(E.compare_rows(ra, na, 37, rb, nb, 37), got)
    sa, sb = E.select_chains_rows(ra, na, 37, list(range(37))), E.select_chains_rows(rb, nb, 37, list(range(37)))
    assert same_result(E.compare_stores(sa, sb), got) and same_result(sa.compare(sb), got)
    # against a store of parsed text: the text holds six digits, so B is what the text says
    text = eg.samples_text(fb, nb)
    st, rep = E.store_from_text(text, 37)
    parsed = st.rows()
    assert rep["nrows"] == nb * 37 and parsed.shape == rb.shape
    via_text = eg.compare_store(fa, na, st)
    held(via_text, ra, na, 37, parsed, nb, 37, what="a range against its text")
    assert same_result(E.compare_rows(ra, na, 37, parsed, nb, 37), via_text) and same_result(E.compare_stores(sa, st), via_text)
    # the swap
    back = swapped(E.compare_stores(sb, sa))
    for k in got:
        if k != "w1":
            assert same_but_nan(back[k], got[k]), k
    rel = np.abs(back["w1"] - got["w1"]) / got["w1"]
    print("swap: largest relative difference of w1 %.3g" % rel.max())
    assert (rel <= 1e-10).all()
    for s in (sa, sb, st):
        s.close()


def test_engine_refusals(engine):
    from mcpar_amd import McxError
    eg = engine
    for a in ((0, 12, 25, 6), (-1, 4, 0, 4), (0, 0, 0, 4), (0, 4, 0, 0), (0, 31, 0, 4)):
        with pytest.raises(McxError) as ei:
            eg.compare(*a)
        assert ei.value.code == 1, a
    from mcpar_amd import engine as E
    other = E.select_chains_rows(K.tie_rows(2, 5, 8, 1), 8, 5, [0, 1])
    with pytest.raises(McxError) as ei:
        eg.compare_store(0, 8, other)
    assert ei.value.code == 1 and "columns" in str(ei.value)
    other.close()


# ---- 8. a statement with content ---------------------------------------------------------------------------------------------------
def test_a_statement_with_content():
    a, b, b15 = K.content_rows()
    c = K.CONTENT
    same = rows_case(a, c["T"], c["nc"], b, c["T"], c["nc"], what="iid normal stores")
    scaled = rows_case(a, c["T"], c["nc"], b15, c["T"], c["nc"], what="column 0 of B times 1.5")
    K.check_content(same, scaled)


# ---- 9. a side beyond 256 tiles ----------------------------------------------------------------------------------------------------
BIG_A, BIG_B = (2105349, 1), (100001, 3)  # (T, nc)
BIG_THIRD = (701783, 100001)                # NA / 3, NB / 3: coprime
BIG_VARIANTS = ("tie", "tile 257")          # column 0, column 1 (log L)


def planted_columns(variant, rng):
    """a column of A and one of B, given by their pooled order, position k holding the value (k - 1 200 000) / 1024 (exact in
    float32), each in a shuffle of its own: in every third of A, B runs ahead of A's share (D+ <= 0, and 0 at the end of a third)
    except where values of B are held back: "tie": two of them in every third until A's local key 4000 is past, three equal
    maxima in tiles 0, 86 and 171; "tile 257": one of them until A's key 2 105 345 is past, a maximum of D+ that only tile 257
    holds"""
    (Ta, nca), (Tb, ncb) = BIG_A, BIG_B
    NA, NB, (PA, PB) = Ta * nca, Tb * ncb, BIG_THIRD
    idx = np.arange(NA, dtype=np.int64)
    per, i = idx // PA, idx % PA
    cb = np.minimum(PB, (i + 1) * PB // PA + 1)  # B's values at or before A's local key i
    if variant == "tie":
        at = 4000
        cb = np.where(i <= at, np.minimum(cb, int(cb[at]) - 2), cb)
    else:
        at = 2105345 - 2 * PA
        cb = np.where((per == 2) & (i <= at), np.minimum(cb, int(cb[at]) - 1), cb)
    cB = per * PB + cb
    assert (np.diff(cB) >= 0).all() and cB[-1] == NB
    pos_a = idx + cB
    taken = np.zeros(NA + NB, bool)
    taken[pos_a] = True
    pos_b = np.flatnonzero(~taken)
    assert pos_b.size == NB
    return rng.permutation((pos_a - 1200000) / 1024.0).astype(np.float32), rng.permutation((pos_b - 1200000) / 1024.0).astype(np.float32)


def big_sides():
    rng = np.random.default_rng(20)
    cols = [planted_columns(v, rng) for v in BIG_VARIANTS]
    return np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1)


def big_reference(a, sa, b, sb):
    """compare_ref.restate's dict of a against b, with distances_numpy for the distances and the sides' rows_summary sa, sb"""
    out = {f: [] for f in R.FIELDS}
    for c in range(a.shape[1]):
        r = R.distances_numpy(a[:, c], b[:, c])
        r.update(mean_a=sa["mean"][c], sd_a=sa["sd"][c], ess_a=sa["ess"][c], mean_b=sb["mean"][c], sd_b=sb["sd"][c], ess_b=sb["ess"][c],
                 na=a.shape[0], nb=b.shape[0], flags=0)
        r["z_mean"] = R.z_mean(r["mean_a"], r["sd_a"], r["ess_a"], r["mean_b"], r["sd_b"], r["ess_b"])
        r["ks_neff"], r["ks_p"] = R.ks_prob(r["ks"], r["ess_a"], r["ess_b"])
        for f in R.FIELDS:
            out[f].append(r[f])
    ints = ("ks_plus_num", "ks_minus_num", "na", "nb")
    return {f: np.array(v, np.int64 if f in ints else np.int32 if f == "flags" else np.float64) for f, v in out.items()}


def test_a_side_beyond_256_tiles():
    from mcpar_amd import engine as E
    (Ta, nca), (Tb, ncb) = BIG_A, BIG_B
    NA, NB = Ta * nca, Tb * ncb
    g = E.debug_compare_store_geometry(Ta, nca, Tb, ncb, 2)
    assert (g["tile_keys"], g["block"], g["tiles_a"], g["tiles_b"]) == (K.TILE, 256, 258, 37)
    assert (g["sort_tiles_a"], g["sort_tiles_b"]) == (258, 37) and g["sort_tiles_a"] > 256 >= g["sort_tiles_b"]  # A's scans carry
    assert (g["bounds_workgroups_a"], g["bounds_workgroups_b"]) == (2, 1)
    assert (g["step_chunk_a"], g["step_chunk_b"]) == (65, 64) and (g["grid_y_a"], g["grid_y_b"]) == (-(-Ta // 65), -(-Tb // 64))
    assert g["tiles_a"] > g["block"] >= g["tiles_b"]  # lanes 0 and 1 of k_cmp_reduce take two tiles of A, none two of B
    swapped_g = E.debug_compare_store_geometry(Tb, ncb, Ta, nca, 2)
    assert (swapped_g["tiles_a"], swapped_g["bounds_workgroups_b"], swapped_g["step_chunk_b"]) == (37, 2, 65)
    a, b = big_sides()
    # the reference alone: where the maxima of D+ lie
    plus = []
    for c, variant in enumerate(BIG_VARIANTS):
        ka, kb = np.sort(R.ckey(a[:, c])), np.sort(R.ckey(b[:, c]))
        d = np.arange(1, NA + 1, dtype=np.int64) * NB - np.searchsorted(kb, ka, "right").astype(np.int64) * NA
        top = np.flatnonzero(d == d.max())
        plus.append((int(d.max()), R.key_value(ka[top[:1]])[0]))
        if variant == "tie":
            assert (top // K.TILE).tolist() == [0, 86, 171] and np.diff(top).tolist() == [BIG_THIRD[0]] * 2 and d.max() > 0
            assert len({int(v) % 256 for v in top // K.TILE}) == 3  # three lanes of the reducer
        else:
            assert (top // K.TILE).tolist() == [257] and d[K.TILE:2 * K.TILE].max() < d.max()  # tile 1, the same lane, holds less
    sa, sb = E.rows_summary(a, Ta, nca), E.rows_summary(b, Tb, ncb)
    for x, Tx, ncx, sx, y, Ty, ncy, sy, order in ((a, Ta, nca, sa, b, Tb, ncb, sb, "A, B"), (b, Tb, ncb, sb, a, Ta, nca, sa, "B, A")):
        ref = big_reference(x, sx, y, sy)
        side = "ks_plus" if order == "A, B" else "ks_minus"
        assert [(int(n), v) for n, v in zip(ref[side + "_num"], ref[side + "_x"])] == plus  # the lowest position of the maximum
        got = E.compare_rows(x, Tx, ncx, y, Ty, ncy)
        worst = R.check(got, ref)
        print("beyond 256 tiles, %s: largest relative difference of w1 %.3g" % (order, worst))
        for f, s_, k in (("mean_a", sx, "mean"), ("sd_a", sx, "sd"), ("ess_a", sx, "ess"), ("mean_b", sy, "mean"), ("sd_b", sy, "sd"),
                         ("ess_b", sy, "ess")):
            assert got[f].tobytes() == np.asarray(s_[k], np.float64).tobytes(), (order, f)
