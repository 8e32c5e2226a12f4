"""Pair densities of the sample store on the GPU (include/mcx.h) against the float64 model
tests/density2d_ref.py.  The sweeps add integers, so the slots are compared exactly; the record of a column to 1e-9 relative,
from / to on bits where they are min and max, and z to 1e-10 of its peak after the model is given the grid the call returned
-- so a last-bit difference in sd cannot move a value across a node (test_gpu_density.py's method)."""
import numpy as np
import pytest

import density2d_ref as D
from test_gpu_density import run, synth

pytestmark = pytest.mark.gpu
FIELDS = ("bw", "from", "to", "lo", "up", "mean", "sd")
KEYS = ("bw", "from", "to", "lo", "up", "mean", "sd", "nvalues", "col_flags", "axes", "z", "pairs", "nbinned", "flags")


def same_bytes(a, b, what=""):
    assert sorted(a) == sorted(b) == sorted(KEYS)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


def all_pairs(ncol):
    return [(a, b) for a in range(ncol) for b in range(a + 1, ncol)]


def model_slots(rows, lo, up, G, pairs):
    return np.stack([D.slots(rows[:, a], rows[:, b], lo[a], up[a], lo[b], up[b], G) for a, b in pairs])


def check_model(got, rows, G, pairs, defaults=True, cols=None, check_pairs=None, **kw):
    """the columns `cols` and the pairs `check_pairs` (indices into pairs) of a density2d dict against the model of its rows"""
    N, ncol = rows.shape
    assert got["axes"].shape == (ncol, G) and got["z"].shape == (len(pairs), G, G)
    assert got["pairs"].tolist() == [list(p) for p in pairs]
    used = sorted({c for p in pairs for c in p})
    for c in (used if cols is None else cols):
        ref = D.grid(rows[:, c], is_last_col=c == ncol - 1, **{k: (v if np.isscalar(v) or k == "clip" else v[c]) for k, v in kw.items()})
        for f in FIELDS:
            assert got[f][c] == pytest.approx(ref[f], rel=1e-9, abs=0.0 if ref[f] != 0.0 else 1e-300), (c, f)
        if defaults:
            assert got["from"][c] == float(rows[:, c].min()) and got["to"][c] == float(rows[:, c].max()), c
        assert got["nvalues"][c] == N and got["col_flags"][c] == 0
        g = {f: float(got[f][c]) for f in FIELDS}
        assert got["axes"][c].tobytes() == D.axis(g, G).tobytes(), c
    for p in (range(len(pairs)) if check_pairs is None else check_pairs):
        a, b = pairs[p]
        ga, gb = ({f: float(got[f][c]) for f in FIELDS} for c in (a, b))
        sl = D.slots(rows[:, a], rows[:, b], ga["lo"], ga["up"], gb["lo"], gb["up"], G)
        assert got["nbinned"][p] == int(sl[:, 0].sum()) and got["flags"][p] == 0, p
        if defaults:
            assert got["nbinned"][p] == N, p
        z = D.finish(ga, gb, sl, N, G)
        err = np.abs(got["z"][p] - z).max()
        assert err <= 1e-10 * z.max(), (p, err, z.max())


# ---- the sweeps: exact slots, and the product call on the same rows ---------------------------------------------------------
# (nsteps, nc, np): an odd tile with np % 4 != 0; N = 2, the only pair (p0, LL); two column tiles plus log L, all 153 pairs;
# the widest row with eight named pairs; one step
NAMED = [(0, 256), (255, 256), (256, 3), (0, 1), (31, 32), (100, 200), (200, 100), (128, 255)]
SHAPES = [(7, 37, 5, None), (2, 1, 1, None), (9, 300, 17, None), (5, 64, 256, NAMED), (1, 50, 2, None)]


@pytest.mark.parametrize("G", [8, 37, 64])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s[:3])
def test_slots_are_the_models_integers(shape, G):
    from mcpar_amd import engine as E
    nsteps, nc, np_, named = shape
    rows = synth(nsteps, nc, np_, 10 + np_)
    pairs = named or all_pairs(np_ + 1)
    got = E.rows_density2d(rows, nsteps, nc, g=G, pairs=named)
    slots = E.debug_rows_density2d_bins(rows, nsteps, nc, got["lo"], got["up"], G, pairs=named)
    want = model_slots(rows, got["lo"], got["up"], G, pairs)
    assert slots.shape == want.shape == (len(pairs), (G + 1) ** 2, 4)
    assert np.array_equal(slots, want), np.argwhere(slots != want)[:4]
    assert np.array_equal(got["nbinned"], want[:, :, 0].sum(axis=1).astype(np.int64))
    assert np.all(got["nbinned"] == nsteps * nc)  # from = min, to = max: nothing is dropped
    some = sorted({0, len(pairs) // 2, len(pairs) - 1})
    check_model(got, rows, G, pairs, cols=sorted({c for p in some for c in pairs[p]}), check_pairs=some)


def test_whole_call_clip_adjust_given_values_and_a_swapped_pair():
    from mcpar_amd import engine as E
    rows = synth(50, 100, 5, 99)
    G, pairs = 32, [(0, 1), (1, 0), (4, 5), (5, 2), (2, 5)]
    nan = np.nan
    kw = dict(adjust=0.5, clip=(0.01, 0.99), bw=[nan, 0.0005, nan, nan, nan, 30.0], from_=[-4.0, nan, nan, nan, nan, nan],
              to=[nan, nan, nan, nan, nan, 0.0])
    got = E.rows_density2d(rows, 50, 100, g=G, pairs=pairs, **kw)
    assert got["bw"][1] == 0.0005 and got["bw"][5] == 30.0 and got["from"][0] == -4.0 and got["to"][5] == 0.0
    check_model(got, rows, G, pairs, defaults=False, **kw)
    assert 0 < got["nbinned"][0] < 5000
    # (b, a) is (a, b)'s transpose, bit for bit
    assert got["z"][1].tobytes() == np.ascontiguousarray(got["z"][0].T).tobytes()
    assert got["z"][4].tobytes() == np.ascontiguousarray(got["z"][3].T).tobytes()
    assert got["nbinned"][0] == got["nbinned"][1] and got["nbinned"][3] == got["nbinned"][4]


# ---- carry and contention ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("np_", [1, 2])
def test_carry_and_contention(np_):
    """3 * 2^16 + 5 rows of a pair in one slot with w_a = w_b = 4095: Sab comes within 0.1 % of 2^40 per 2^16 rows, the bound
    the packed word is laid out for, and every workgroup drains into its slab more than once (four chunks, two workgroups
    per pair).  np = 2: the column between the two is spread over its grid"""
    from mcpar_amd import engine as E
    G, N = 64, 3 * (1 << 16) + 5
    v = np.float32(3.0 + 4095.5 / 4096.0)
    assert float(v) == 3.0 + 4095.5 / 4096.0
    rng = np.random.default_rng(7)
    rows = np.full((N, np_ + 1), v, np.float32)
    if np_ == 2:
        rows[:, 1] = rng.uniform(0.0, 63.0, N)
    last = np_
    strag = [5, 70000, 131071, 131072, N - 1]
    rows[strag[0], 0] = 1000.0                    # not on the grid
    rows[strag[1], last] = -2.0                   # not on the grid
    rows[strag[2], 0] = 10.25                     # other slots
    rows[strag[3], last] = 20.5
    rows[strag[4], 0], rows[strag[4], last] = 0.0, 63.0
    # from = 1, to = g - 2, bw = 1/4: lo = 0, up = g - 1, delta = 1
    ncol = np_ + 1
    pairs = [(0, last), (last, 0)] + ([(0, 1), (1, 2)] if np_ == 2 else [])
    got = E.rows_density2d(rows, N, 1, g=G, pairs=pairs, bw=[0.25] * ncol, from_=[1.0] * ncol, to=[G - 2.0] * ncol)
    assert np.all(got["lo"] == 0.0) and np.all(got["up"] == G - 1.0)
    lo, up = got["lo"], got["up"]
    slots = E.debug_rows_density2d_bins(rows, N, 1, lo, up, G, pairs=pairs)
    want = model_slots(rows, lo, up, G, pairs)
    assert np.array_equal(slots, want), np.argwhere(slots != want)[:4]
    one = slots[0].reshape(G + 1, G + 1, 4)[4, 4]
    n = N - len(strag)
    assert one.tolist() == [n, 4095 * n, 4095 * n, 4095 * 4095 * n]
    assert 4095 * 4095 * (1 << 16) > 0.999 * (1 << 40)
    assert slots[1].reshape(G + 1, G + 1, 4)[4, 4].tolist() == one.tolist()
    assert got["nbinned"][0] == N - 2 and got["nbinned"][1] == N - 2
    check_model(got, rows, G, pairs, defaults=False, cols=[], check_pairs=range(len(pairs)))


def test_one_workgroup_walks_every_chunk():
    """1024 pairs leave one workgroup per pair: it walks all four chunks of 3 * 2^16 + 5 rows and drains into its slab four
    times (the geometry gives a pair at most ceil(1024 / npairs) workgroups)"""
    from mcpar_amd import engine as E
    G, N = 8, 3 * (1 << 16) + 5
    rng = np.random.default_rng(12)
    rows = np.stack([rng.normal(0.0, 1.0, N), rng.uniform(-2.0, 2.0, N), -rng.chisquare(3, N)], axis=1).astype(np.float32)
    lo, up = np.array([-2.5, -1.5, -9.0]), np.array([2.5, 2.5, 0.5])  # narrower than the data in every column
    two = [(0, 1), (2, 0)]
    slots = E.debug_rows_density2d_bins(rows, N, 1, lo, up, G, pairs=two * 512)
    want = model_slots(rows, lo, up, G, two)
    assert slots.shape == (1024, 81, 4) and 0 < int(want[0, :, 0].sum()) < N
    assert np.array_equal(slots[:2], want), np.argwhere(slots[:2] != want)[:4]
    assert np.array_equal(slots, np.tile(want, (512, 1, 1)))


# ---- edges ---------------------------------------------------------------------------------------------------------------------
def test_edges():
    """column 0 on lo = 0, up = 7, delta = 1, narrower than its data: its rows off the grid leave its pairs alone"""
    from mcpar_amd import engine as E
    G = 8
    v0 = np.array([-1.5, -1.0, -0.5, 0.0, 3.25, 7.0, 7.5, 7.99, 8.0, 2.0], np.float32)
    N = v0.size
    rows = np.stack([v0, np.linspace(-1.0, 1.0, N).astype(np.float32), np.linspace(5.0, 50.0, N).astype(np.float32)], axis=1)
    nan = np.nan
    pairs = [(0, 1), (0, 2), (1, 2), (2, 0)]
    got = E.rows_density2d(rows, N, 1, g=G, pairs=pairs, bw=[0.25, nan, nan], from_=[1.0, nan, nan], to=[6.0, nan, nan])
    assert got["lo"][0] == 0.0 and got["up"][0] == 7.0
    assert got["nbinned"].tolist() == [N - 2, N - 2, N, N - 2]  # -1.5 and 8.0 are dropped from column 0's pairs only
    check_model(got, rows, G, pairs, defaults=False, bw=[0.25, nan, nan], from_=[1.0, nan, nan], to=[6.0, nan, nan])
    slots = E.debug_rows_density2d_bins(rows, N, 1, got["lo"], got["up"], G, pairs=pairs)
    want = model_slots(rows, got["lo"], got["up"], G, pairs)
    assert np.array_equal(slots, want), np.argwhere(slots != want)[:4]
    s = slots[0].reshape(G + 1, G + 1, 4)
    row = s.sum(axis=1)  # over column 1's slots: (cnt, Sa, .., ..) per slot of column 0
    assert row[0, :2].tolist() == [2, 2048]    # xpos = -1 (w = 0) and -0.5 (w = F / 2): slot 0
    assert row[1, :2].tolist() == [1, 0]       # the value at lo
    assert row[4, :2].tolist() == [1, 1024]    # 3.25
    assert row[8, 0] == 3                      # 7.0, 7.5 and 7.99: xpos in [g - 1, g)
    assert int(row[:, 0].sum()) == N - 2


# ---- non-finite values ---------------------------------------------------------------------------------------------------------
def test_nonfinite_columns():
    from mcpar_amd import engine as E
    nsteps, nc, G = 8, 40, 16
    rows = synth(nsteps, nc, 4, 3)
    rows[17, 0] = np.nan
    rows[200, 2] = np.inf
    got = E.rows_density2d(rows, nsteps, nc, g=G)
    pairs = all_pairs(5)
    clean = [p for p, (a, b) in enumerate(pairs) if a not in (0, 2) and b not in (0, 2)]
    assert [pairs[p] for p in clean] == [(1, 3), (1, 4), (3, 4)]
    for p in range(len(pairs)):
        if p in clean:
            continue
        assert got["flags"][p] == E.SUMMARY_NONFINITE and got["nbinned"][p] == 0 and np.all(np.isnan(got["z"][p])), p
    for c in (0, 2):
        assert got["col_flags"][c] == E.SUMMARY_NONFINITE and got["nvalues"][c] == nsteps * nc
        assert all(np.isnan(got[f][c]) for f in FIELDS) and np.all(np.isnan(got["axes"][c]))
    ref = E.rows_density2d(rows, nsteps, nc, g=G, pairs=[pairs[p] for p in clean])  # without those columns' pairs
    for i, p in enumerate(clean):
        assert got["flags"][p] == 0 and got["nbinned"][p] == ref["nbinned"][i] == nsteps * nc
        assert got["z"][p].tobytes() == ref["z"][i].tobytes(), p
    for c in (1, 3, 4):
        for f in FIELDS + ("axes",):
            assert got[f][c].tobytes() == ref[f][c].tobytes(), (c, f)
    check_model(got, rows, G, pairs, cols=[1, 3, 4], check_pairs=clean)


# ---- the engine's store --------------------------------------------------------------------------------------------------------
def test_engine_sub_range_is_its_rows_and_the_same_on_a_second_call():
    from mcpar_amd import engine as E
    eg = run(5, 333, 100, 40)
    got = eg.density2d(g=24, first_step=3, nsteps=30)
    rows = eg.samples_range(3, 30)
    same_bytes(got, E.rows_density2d(rows, 30, 333, g=24), "rows")
    same_bytes(got, eg.density2d(g=24, first_step=3, nsteps=30), "second call")
    check_model(got, rows, 24, all_pairs(6), check_pairs=[0, 7, 14])
    named = eg.density2d(g=24, pairs=[(5, 0), (2, 3)], first_step=3, nsteps=30)
    assert named["z"][0].tobytes() == np.ascontiguousarray(got["z"][4].T).tobytes()  # (0, 5) is pair 4
    assert named["z"][1].tobytes() == got["z"][all_pairs(6).index((2, 3))].tobytes()
    eg.close()


def test_engine_sample_stride():
    from mcpar_amd import engine as E
    eg = run(5, 512, 100, 150, stride=3)
    kept = eg.samples.shape[0] // eg.nc
    assert kept == 50
    got = eg.density2d(g=16)
    rows = eg.samples_range(0, kept)
    same_bytes(got, E.rows_density2d(rows, kept, 512, g=16), "rows")
    check_model(got, rows, 16, all_pairs(6), check_pairs=[0, 14])
    eg.close()


# ---- a derived store, a clip's store, and their lifetime -----------------------------------------------------------------------
def test_derived_store_rowset_store_and_lifetime():
    import mcpar_amd as M
    from mcpar_amd import engine as E
    d, nc, T = 5, 200, 24
    eg = run(d, nc, 60, T)
    ident = eg.derive(M.derive_linear(np.eye(d, dtype=np.float32), np.zeros(d, np.float32)))
    same_bytes(ident.density2d(g=20, clip=(0.05, 0.95)), eg.density2d(g=20, clip=(0.05, 0.95)), "identity")
    rng = np.random.default_rng(8)
    two = eg.derive(M.derive_linear(rng.standard_normal((2, d)).astype(np.float32), np.array([0.5, -1.0], np.float32)))
    got = two.density2d(g=20)
    rows = two.rows()
    assert rows.shape == (T * nc, 3)
    same_bytes(got, E.rows_density2d(rows, T, nc, g=20), "two outputs")
    check_model(got, rows, 20, all_pairs(3))
    # the rows a clip kept, as a store of pseudo-chains
    rs = eg.clip(0.05, 0.95, ll_hi=np.inf)
    st = rs.store(nc=64)
    t, snc, ncol = st.shape
    assert snc == 64 and ncol == d + 1 and t >= 2
    kept = rs.rows(0, t * 64)
    same_bytes(st.density2d(g=12, pairs=[(0, 5), (3, 1)]), E.rows_density2d(kept, t, 64, g=12, pairs=[(0, 5), (3, 1)]), "clip store")
    # the stores outlive the engine
    eg.close()
    same_bytes(two.density2d(g=20), got, "after the engine")
    for s in (ident, two, st):
        s.close()
    rs.close()
