"""mcx_samples_intervals on the GPU against tests/intervals_ref.py on Metropolis-like rows: a chain's row
repeats the step before with probability 0.7.

What is held, by intervals_ref.check: every HDI field bit for bit (index and span included); q bit for bit the summary's;
ess_sd and ess_q within the 1e-4 relative that the summary's tests pin an ESS to, their lags exact; mcse_sd within 2e-4 (that
bound through the root, plus the float rounding of c2); k_lo, k_hi the reference rule on the ess_q returned, with scipy's beta
quantiles; s_lo, s_hi and mcse_q exactly those of numpy's sort.  The launch geometry is asserted before each result.

Shapes: the smallest that cross each switch -- the minimum (1, 2, 4); (3, 5, 8); (17, 37, 24) sorted four columns at a time; and
seven columns of N = three window tiles and 77 more, with spans that stay inside a tile, cross one tile edge and cross two, the
span 0 and the span N - 1, and columns made so that the least window is tied everywhere, lies in the last tile, or is tied between
two tiles.

The HUGE case (one chain of 2 105 349 steps) crosses what those do not reach: 515 window tiles, so that a lane of k_hdi_reduce
takes tiles t, t + 256 and t + 512; 258 sort tiles (the second carry step of the sort's scans); a step chunk of 65.  Its HDI
fields, q, the ranks, s_lo, s_hi and mcse_q are held as above, through intervals_ref.check.  summary_ref on three transformed
columns of that length costs more than the few seconds a test may take, so ess_sd, ess_q, their lags and mcse_sd are held by
intervals_ref.check's tolerances against rows_summary of the transformed columns (float((x - mean)^2) and the indicator x <= q,
built as intervals_ref.restate_column builds them, in one call beside the columns themselves: a summary of one chain of two
million steps costs the library a second, however many columns); mean and sd against numpy's float64 at check's 1e-9."""
import numpy as np
import pytest

import intervals_ref as R
from test_gpu_store_view import run

pytestmark = pytest.mark.gpu

HDI, PROBS = (0.9,), (0.05, 0.5, 0.95)
WT = 4096                    # window starts per workgroup (asserted)
BIG_T, BIG_NC = 5, 2473      # N = 12365 = 3 * 4096 + 77
BIG_N = BIG_T * BIG_NC


def make_rows(np_, nc, T, seed=11, stay=0.7):
    """skewed rows (lognormal parameters, log L below zero), column 1 rounded to one decimal, repeated with probability stay.
    make_rows_loop without its loop over the steps and with the same draws (a Generator fills one [T - 1, nc] request as it
    fills T - 1 requests of nc): a row is the last row at or before it that was not a repeat.  tests/test_intervals_cpu.py pins
    the two to each other"""
    rng = np.random.default_rng([seed, np_, nc, T])
    a = rng.lognormal(0.0, 0.7, (T, nc, np_ + 1)).astype(np.float32)
    a[:, :, -1] = -a[:, :, -1]
    if np_ > 1:
        a[:, :, 1] = np.round(a[:, :, 1], 1)
    rep = np.concatenate([np.zeros((1, nc), bool), rng.random((T - 1, nc)) < stay])
    src = np.maximum.accumulate(np.where(rep, 0, np.arange(T)[:, None]), axis=0)
    return a[src, np.arange(nc)[None, :]].reshape(T * nc, np_ + 1)


def make_rows_loop(np_, nc, T, seed=11, stay=0.7):
    """make_rows step by step: the definition"""
    rng = np.random.default_rng([seed, np_, nc, T])
    a = rng.lognormal(0.0, 0.7, (T, nc, np_ + 1)).astype(np.float32)
    a[:, :, -1] = -a[:, :, -1]
    if np_ > 1:
        a[:, :, 1] = np.round(a[:, :, 1], 1)
    for t in range(1, T):
        rep = rng.random(nc) < stay
        a[t, rep] = a[t - 1, rep]
    return a.reshape(T * nc, np_ + 1)


def span_mass(m, N):
    """a mass whose span is m"""
    return (m + 0.5) / N


BIG_SPANS = (0, 40, 1000, WT + 1500, 2 * WT + 700, BIG_N - 1)


def big_rows():
    """seven columns of BIG_N values, each a fixed shuffle of a sorted column made for the window sweep:
    0 Metropolis-like; 1 an arithmetic progression: every window ties; 2 random gaps, the narrow ones in the last tile; 3 unit gaps
    but two equal runs of quarter gaps, in tiles 0 and 2; 4 constant; 5 a NaN and a +inf; log L: Metropolis-like"""
    N = BIG_N
    rng = np.random.default_rng(17)
    rows = make_rows(6, BIG_NC, BIG_T, seed=13)
    perm = rng.permutation(N)
    rows[perm, 1] = np.arange(N, dtype=np.float32) * np.float32(0.5) - np.float32(100.0)
    gaps = rng.uniform(1.0, 2.0, N)
    gaps[3 * WT + 10:] = rng.uniform(0.01, 0.02, N - 3 * WT - 10)
    rows[rng.permutation(N), 2] = np.cumsum(gaps).astype(np.float32)
    g3 = np.ones(N)
    g3[1000:1000 + 3000] = 0.25
    g3[2 * WT + 500:2 * WT + 3500] = 0.25
    rows[rng.permutation(N), 3] = np.cumsum(g3).astype(np.float32)
    rows[:, 4] = np.float32(2.5)
    rows[N // 3, 5] = np.nan
    rows[N // 2, 5] = np.inf
    return rows


CACHE = {}


def case(key):
    """(rows, T, nc, masses, probs, reference), made once"""
    if key not in CACHE:
        if key == "big":
            rows, T, nc = big_rows(), BIG_T, BIG_NC
            masses = tuple(span_mass(m, BIG_N) for m in BIG_SPANS)
        else:
            np_, nc, T = key
            rows, masses = make_rows(np_, nc, T), HDI
        CACHE[key] = (rows, T, nc, masses, PROBS, R.restate(rows, T, nc, masses, PROBS))
    return CACHE[key]


def held(rows, T, nc, masses, probs, ref):
    """rows_intervals of the rows, held to the reference; q bit for bit the summary's"""
    from mcpar_amd import engine as E
    got = E.rows_intervals(rows, T, nc, masses, probs)
    R.check(got, ref, probs)
    q = E.rows_summary(rows, T, nc, probs)["quantiles"]
    fin = got["flags"] == 0
    assert q[fin].tobytes() == got["quantiles"]["q"][fin].tobytes() and np.isnan(got["quantiles"]["q"][~fin]).all()
    return got


@pytest.mark.parametrize("shape", [(1, 2, 4), (3, 5, 8)])
def test_small_shapes(shape):
    from mcpar_amd import engine as E
    rows, T, nc, masses, probs, ref = case(shape)
    g = E.debug_intervals_geometry(T, nc, shape[0], len(masses), len(probs))
    assert (g["window_tile"], g["window_tiles"], g["sort_tiles"], g["groups"], g["transforms"]) == (WT, 1, 1, 1, 4)
    held(rows, T, nc, masses, probs, ref)


def test_grouped_columns(monkeypatch):
    from mcpar_amd import engine as E
    rows, T, nc, masses, probs, ref = case((17, 37, 24))
    monkeypatch.delenv("MCX_RANK_GROUP_COLS", raising=False)
    whole = E.rows_intervals(rows, T, nc, masses, probs)
    monkeypatch.setenv("MCX_RANK_GROUP_COLS", "4")
    g = E.debug_intervals_geometry(T, nc, 17, len(masses), len(probs))
    assert (g["group_cols"], g["groups"], g["window_tiles"]) == (4, 5, 1)  # (a group of parameters, one across both tile sets' edge)
    got = held(rows, T, nc, masses, probs, ref)
    assert same_bytes(got, whole)


def flat(d):
    out = {k: v for k, v in d.items() if not isinstance(v, dict)}
    for name in ("hdi", "quantiles"):
        out.update({name + "." + k: v for k, v in d[name].items()})
    return out


def same_bytes(a, b):
    a, b = flat(a), flat(b)
    return sorted(a) == sorted(b) and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and
                                          np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f") for k in a)


def test_window_tiles():
    from mcpar_amd import engine as E
    rows, T, nc, masses, probs, ref = case("big")
    g = E.debug_intervals_geometry(T, nc, 6, len(masses), len(probs))
    assert (g["window_tile"], g["window_tiles"], g["sort_tiles"], g["slab_entries"]) == (WT, 4, 2, 4 * len(masses))
    assert BIG_N == 3 * WT + 77 and [h["span"] for h in ref[0]["hdi"]] == list(BIG_SPANS)
    # the reference itself says what each column is for
    idx = lambda c: [h["index"] for h in ref[c]["hdi"]]  # noqa: E731
    assert idx(1) == [0] * 6 and all(h["width"] == 0.5 * m for h, m in zip(ref[1]["hdi"], BIG_SPANS))
    assert idx(2)[1] >= 3 * WT + 10 and 2 * WT <= idx(2)[2] < 3 * WT  # the least window of span 40 starts in the last, ragged tile
    assert idx(3)[1:3] == [999, 999] and [h["width"] for h in ref[3]["hdi"][1:3]] == [10.0, 250.0]  # tied with tile 2: the lower index
    assert idx(4) == [0] * 6 and all(h["width"] == 0.0 and h["lo"] == h["hi"] == np.float32(2.5) for h in ref[4]["hdi"])
    assert ref[5]["flags"] == 1 and idx(5) == [-1] * 6 and not any(ref[c]["flags"] for c in (0, 1, 2, 3, 4, 6))
    got = held(rows, T, nc, masses, probs, ref)
    # a constant column: no spread, so no error of it
    assert got["sd"][4] == 0.0 and np.isnan(got["ess_sd"][4]) and np.isnan(got["mcse_sd"][4])


def test_eight_masses_and_eight_probs_and_none():
    from mcpar_amd import engine as E
    rows, T, nc, _, _, _ = case((3, 5, 8))
    masses = (0.1, 0.25, 0.5, 0.68, 0.8, 0.9, 0.94, 0.99)
    probs = (0.0, 0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)
    g = E.debug_intervals_geometry(T, nc, 3, 8, 8)
    assert (g["slab_entries"], g["reduce_workgroups"], g["pick_ranks"], g["transforms"]) == (8, 8, 16, 9)
    both = E.rows_intervals(rows, T, nc, masses, probs)
    R.check(both, R.restate(rows, T, nc, masses, probs), probs)
    g = E.debug_intervals_geometry(T, nc, 3, 0, 0)
    assert (g["slab_entries"], g["reduce_workgroups"], g["pick_ranks"], g["transforms"]) == (0, 0, 0, 1)
    no_mass, no_probs = E.rows_intervals(rows, T, nc, (), probs), E.rows_intervals(rows, T, nc, masses, ())
    neither = E.rows_intervals(rows, T, nc, (), ())
    assert no_mass["hdi"]["lo"].shape == (4, 0) and no_probs["quantiles"]["q"].shape == (4, 0)
    for part in (no_mass, no_probs, neither):
        for k in ("mean", "sd", "ess_sd", "mcse_sd", "ess_sd_lag", "flags"):
            assert np.array_equal(part[k], both[k], equal_nan=True), k
    assert all(np.array_equal(no_mass["quantiles"][k], both["quantiles"][k], equal_nan=True) for k in both["quantiles"])
    assert all(np.array_equal(no_probs["hdi"][k], both["hdi"][k], equal_nan=True) for k in both["hdi"])


def test_the_three_owners_and_a_second_call_give_the_same_bytes():
    from mcpar_amd import engine as E
    eg = run(37, 17, 30)
    first, nsteps = 3, 24
    rows = eg.samples_range(first, nsteps)
    on_engine = eg.intervals(HDI, PROBS, first_step=first, nsteps=nsteps)
    R.check(on_engine, R.restate(rows, nsteps, eg.nc, HDI, PROBS), PROBS)
    assert same_bytes(eg.intervals(HDI, PROBS, first_step=first, nsteps=nsteps), on_engine)
    assert same_bytes(E.rows_intervals(rows, nsteps, eg.nc, HDI, PROBS), on_engine)
    st = E.select_chains_rows(rows, nsteps, eg.nc, list(range(eg.nc)))
    assert same_bytes(st.intervals(HDI, PROBS), on_engine) and same_bytes(st.intervals(HDI, PROBS), on_engine)
    st.close()
    ms = eg.intervals_times(HDI, PROBS, first_step=first, nsteps=nsteps)
    assert ms.shape == (12,) and (ms >= 0).all() and ms[11] >= ms[:11].sum() * 0.99 > 0
    eg.close()


# ---- more window tiles than lanes of the reducer, more sort tiles than a scan step ------------------------------------------------
HUGE_T = 2105349
HUGE_TILES = (3, 259, 300)  # equal runs of quarter gaps: tiles 3 and 259 are one lane's of k_hdi_reduce, 300 another's
HUGE_SPANS = (40, 1000)
HUGE_PROBS = (0.5,)


def huge_rows():
    """two columns of one chain.  0: a fixed shuffle of a sorted column of unit gaps with 3000 quarter gaps from key 500 of each
    of HUGE_TILES on (every value a multiple of 1 / 4 below 2^22: exact); log L: Metropolis-like"""
    rows = make_rows(1, 1, HUGE_T, seed=13)
    g = np.ones(HUGE_T)
    for t in HUGE_TILES:
        g[t * WT + 500:t * WT + 3500] = 0.25
    rows[np.random.default_rng(19).permutation(HUGE_T), 0] = np.cumsum(g).astype(np.float32)
    return rows


def test_more_window_tiles_than_reducer_lanes():
    from mcpar_amd import engine as E
    T, nc, N = HUGE_T, 1, HUGE_T
    masses = tuple(span_mass(m, N) for m in HUGE_SPANS) + (0.9,)
    g = E.debug_intervals_geometry(T, nc, 1, len(masses), len(HUGE_PROBS))
    assert (g["block"], g["window_tile"], g["window_tiles"], g["sort_tiles"]) == (256, WT, 515, 258)
    assert (g["step_chunk"], g["grid_y"], g["reduce_workgroups"], g["transforms"]) == (65, -(-T // 65), 3, 2)
    assert g["window_tiles"] > 2 * g["block"] and g["sort_tiles"] > 256 and g["groups"] == 1
    rows = huge_rows()
    # the reference alone: the HDI of numpy's sort, and where column 0's narrowest windows tie
    ref = []
    for c in (0, 1):
        srt = R.sorted_values(rows[:, c])
        hd = [dict(zip(("lo", "hi", "width", "index", "span"), R.hdi(srt, p))) for p in masses]
        ref.append(dict(flags=0, sorted=srt, hdi=hd))
    s0 = ref[0]["sorted"].astype(np.float64)
    for h, m in zip(ref[0]["hdi"], HUGE_SPANS):
        w = s0[m:] - s0[:N - m]
        tied = np.flatnonzero(w == w.min())
        assert h["span"] == m and h["width"] == m / 4 == w.min() and h["index"] == tied[0] == HUGE_TILES[0] * WT + 499
        assert sorted(set((tied // WT).tolist())) == list(HUGE_TILES)  # the reference sees the tie: one lane's two tiles, and another's
    assert ref[0]["hdi"][2]["index"] == 0 and ref[0]["hdi"][2]["span"] == int(0.9 * N)  # every window over all three runs ties
    assert ref[1]["hdi"][0]["index"] > 0
    got = E.rows_intervals(rows, T, nc, masses, HUGE_PROBS)
    # the mixing numbers: one rows_summary of the columns and the transformed columns (six series, six lanes' work).  The
    # transforms are restate_column's: about numpy's float64 mean, and at the median, which for an odd N is an order statistic
    x = rows.astype(np.float64)
    assert N % 2 == 1 and HUGE_PROBS == (0.5,)
    q = np.array([float(ref[c]["sorted"][(N - 1) // 2]) for c in (0, 1)])
    c2 = ((x - x.mean(axis=0)[None, :]) ** 2).astype(np.float32)
    ind = (x <= q[None, :]).astype(np.float32)
    st = E.rows_summary(np.concatenate([rows, c2, ind], axis=1), T, nc, HUGE_PROBS)
    assert not st["flags"].any() and st["quantiles"][:2, 0].tolist() == q.tolist()
    for c in (0, 1):
        ref[c].update(mean=x[:, c].mean(), sd=x[:, c].std(ddof=1), ess_sd=st["ess"][2 + c], ess_sd_lag=st["ess_lag"][2 + c],
                      mcse_sd=R.mcse_sd(N, st["mean"][2 + c], st["sd"][2 + c], st["ess"][2 + c]),
                      quantiles=[dict(q=q[c], ess_q=st["ess"][4 + c], ess_q_lag=st["ess_lag"][4 + c])])
        assert np.isfinite(ref[c]["ess_sd"]) and np.isfinite(st["ess"][4 + c])
    R.check(got, ref, HUGE_PROBS)
    assert got["quantiles"]["q"].tobytes() == st["quantiles"][:2].tobytes()
    for c in (0, 1):  # the ranks are decided well clear of the error of u
        assert R.rank_margin(N, HUGE_PROBS[0], float(got["quantiles"]["ess_q"][c, 0])) > 1e-3
