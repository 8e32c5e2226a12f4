"""Tail-clipped rows of the sample store on the GPU (include/mcx.h) against the float64 restatement
tests/clip_ref.py.  Every comparison is exact: the kernels compare and count, they compute nothing.  Most cases clip
synthetic host rows (clip_rows), so no run is needed.  Shapes are (nsteps, np, nc)."""
import functools
import gc

import numpy as np
import pytest

import clip_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
# 65 rows: one wavefront and a row, everything odd; 272 = 256 + 16 rows, np one past a column tile; the widest row and the
# smallest tile (32 rows); 512 rows: two full tiles, every piece on 16 bytes; one step; 65 537 rows of np = 1: one workgroup
# past what one block of the scan covers (256 workgroups of 256 rows)
SHAPES = [(5, 3, 13), (17, 17, 16), (3, 256, 4), (64, 16, 8), (1, 2, 70), (65537, 1, 1)]


def synth(nsteps, np_, nc, seed):
    """continuous rows [nsteps * nc, np_ + 1]: normal parameters of different location and scale, log L below zero"""
    rng = np.random.default_rng(seed)
    N = nsteps * nc
    rows = rng.normal(0.0, 1.0, (N, np_ + 1)) * (1.0 + 0.25 * (np.arange(np_ + 1) % 7)) + (np.arange(np_ + 1) % 5 - 2.0)
    rows[:, -1] = -rng.chisquare(3, N) * 2.0 - 1e-3
    return rows.astype(np.float32)


@functools.lru_cache(maxsize=None)
def shape_rows(shape):
    rows = synth(*shape, seed=100 + shape[1])
    rows.setflags(write=False)
    return rows


def same_report(a, b):
    assert a.report.tobytes() == b.report.tobytes() and a.nrows == b.nrows and a.nsource == b.nsource and a.ncol == b.ncol


def same_rowset(a, b):
    same_report(a, b)
    assert a.rows().tobytes() == b.rows().tobytes() and a.index().tobytes() == b.index().tobytes()


def same_bytes(a, b, what=""):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (what, k)


# ---- the shapes: default thresholds -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_against_the_restatement(shape):
    from mcpar_amd import engine as E
    nsteps, np_, nc = shape
    rows = shape_rows(shape)
    qlo, qhi = (0.05, 0.95) if nsteps * nc < 1000 else (0.01, 0.99)
    rs = E.clip_rows(rows, nsteps, nc, qlo, qhi)
    assert (rs.nsource, rs.ncol) == (nsteps * nc, np_ + 1) and not rs.report["flags"].any()
    ref = R.check(rs, rows)  # with the thresholds reported
    assert 0 < rs.nrows < rs.nsource or nsteps * nc < 100
    # the reported defaults are the summary's quantiles, bit for bit, and log L's upper threshold is 0
    if nsteps >= 4:
        q = E.rows_summary(rows, nsteps, nc, probs=(qlo, qhi))["quantiles"]
        assert rs.report["lo"].tobytes() == q[:, 0].tobytes() and rs.report["hi"][:-1].tobytes() == q[:-1, 1].tobytes()
    assert rs.report["hi"][-1] == 0.0 and not np.signbit(rs.report["hi"][-1])
    # continuous data: the restatement's own thresholds keep the same rows -- an interpolated threshold lies between two
    # consecutive order statistics with no datum strictly between them, so its last bit cannot move a row
    own = R.clip(rows, qlo, qhi)
    np.testing.assert_allclose(rs.report["lo"], own["lo"], rtol=1e-12)
    np.testing.assert_allclose(rs.report["hi"], own["hi"], rtol=1e-12)
    assert np.array_equal(own["keep"], ref["keep"])
    assert np.array_equal(own["nbelow"], ref["nbelow"]) and np.array_equal(own["nabove"], ref["nabove"])
    # a second call gives the same bytes; count_only the same report and count
    again = E.clip_rows(rows, nsteps, nc, qlo, qhi)
    same_rowset(rs, again)
    same_report(rs, E.clip_rows(rows, nsteps, nc, qlo, qhi, count_only=True))
    rs.close()
    again.close()


# ---- a marker column: which rows go where -----------------------------------------------------------------------------------
def marker(nsteps, np_, nc, keep, seed=5):
    """column 0 = the row number, column 1 = 1 for a row to keep and 0 for one to drop, the rest noise; the bounds that
    clip on column 1 alone"""
    rows = synth(nsteps, np_, nc, seed)
    N = nsteps * nc
    rows[:, 0] = np.arange(N)
    rows[:, 1] = np.asarray(keep, np.float32)
    lo, hi = np.full(np_ + 1, -INF), np.full(np_ + 1, INF)
    lo[1] = 0.5
    return rows, lo, hi


def patterns(N):
    k = np.arange(N)
    yield "first", k == 0
    yield "last", k == N - 1
    yield "every other", k % 2 == 1
    for r in (63, 64, 65):
        yield "runs of %d" % r, (k // r) % 2 == 0
        yield "runs of %d, the others" % r, (k // r) % 2 == 1


@pytest.mark.parametrize("shape", [(40, 3, 25), (9, 16, 64)])  # 1000 rows, pieces off 16 bytes; 576 rows of np = 16
def test_marker_patterns(shape):
    from mcpar_amd import engine as E
    nsteps, np_, nc = shape
    N = nsteps * nc
    for name, keep in patterns(N):
        rows, lo, hi = marker(nsteps, np_, nc, keep)
        rs = E.clip_rows(rows, nsteps, nc, lo=lo, hi=hi, ll_hi=INF)
        assert not rs.report["flags"].any(), name  # no quantile pass ran
        assert rs.nrows == int(keep.sum()), name
        idx, got = rs.index(), rs.rows()
        assert np.array_equal(idx, np.flatnonzero(keep)), name
        assert np.array_equal(got[:, 0], idx.astype(np.float32)), name
        assert got.tobytes() == rows[keep].tobytes(), name
        assert rs.report["nbelow"][1] == N - keep.sum() and rs.report["nbelow"][[0, 2]].sum() == 0 and rs.report["nabove"].sum() == 0, name
        rs.close()


def test_all_kept_and_none_kept():
    from mcpar_amd import McxError
    from mcpar_amd import engine as E
    nsteps, np_, nc = 40, 3, 25
    rows, lo, hi = marker(nsteps, np_, nc, np.ones(nsteps * nc))
    every = E.clip_rows(rows, nsteps, nc, lo=np.full(4, -INF), hi=hi, ll_hi=INF)
    assert every.nrows == 1000 and every.rows().tobytes() == rows.tobytes() and np.array_equal(every.index(), np.arange(1000))
    assert every.report["nbelow"].sum() == 0 and every.report["nabove"].sum() == 0
    lo[1] = INF  # nothing is above +inf
    none = E.clip_rows(rows, nsteps, nc, lo=lo, hi=hi, ll_hi=INF)
    assert none.nrows == 0 and none.nsource == 1000 and none.report["nbelow"][1] == 1000
    assert none.rows().shape == (0, 4) and none.index().shape == (0,)
    assert none.rows(0, 0).shape == (0, 4)
    r0, i0 = none.draw(0, 1)
    assert r0.shape == (0, 4) and i0.shape == (0,)
    with pytest.raises(McxError) as ei:
        none.draw(1, 1)
    assert ei.value.code == 1 and "0 rows" in str(ei.value)
    with pytest.raises(McxError):
        none.store(nc=1, nsteps=1)
    for bad in ((1, 0), (0, 1), (-1, 0)):
        with pytest.raises(McxError):
            none.rows(*bad)
    every.close()
    none.close()


# ---- the tile heights below 256 rows ----------------------------------------------------------------------------------------
# np -> R = derive_rows(np, 0) rows per workgroup.  39 | 40: the two sides of the LDS budget's edge (39 uses all 40 960 bytes)
TILE_NP = {39: 256, 40: 128, 100: 64, 256: 32}


def tile_geometry(np_, N, R):
    """the geometry a reduced-tile case is there for, asserted before any result"""
    from mcpar_amd import engine as E
    g = E.debug_store_geometry(np_, 0, N, 1)
    assert g["clip_rows"] == R and g["clip_mask_words"] == (R + 63) // 64 and g["clip_workgroups"] == 3 - (N == 2 * R), g
    return g


@pytest.mark.parametrize("full", [False, True])  # N = 2 R + 5: a third, ragged workgroup; N = 2 R: two full tiles exactly
@pytest.mark.parametrize("np_", sorted(TILE_NP))
def test_tile_heights_marker_patterns(np_, full):
    """k_clip_mark `if (wave < a.wpw)` and `a.mask[blockIdx.x * a.wpw + wave]`, k_clip_scatter `for (w < wave) pos +=
    popc(mw[w])` and `mw = a.mask + blockIdx.x * a.wpw`: wpw = 2 with wavefronts 2 and 3 idle (R = 128), wpw = 1 with a
    full wavefront (R = 64) and with half of one (R = 32) are run by no other test with more than one workgroup, and so
    never with offs > 0 or a second row of mask words.  The marker column makes every kept row's place visible: a wpw off
    by one or a workgroup reading another's mask words moves or drops rows of the patterns below, whose runs of 63, 64
    and 65 rows put a run's edge at every lane of a mask word and across the tiles of every height."""
    from mcpar_amd import engine as E
    R_ = TILE_NP[np_]
    N = 2 * R_ + (0 if full else 5)
    g = tile_geometry(np_, N, R_)
    assert (g["clip_lds_bytes"] == 40960) == (np_ == 39)
    for name, keep in patterns(N):
        rows, lo, hi = marker(N, np_, 1, keep)
        rs = E.clip_rows(rows, N, 1, lo=lo, hi=hi, ll_hi=INF)
        assert not rs.report["flags"].any(), name  # no quantile pass ran
        assert rs.nrows == int(keep.sum()), name
        idx, got = rs.index(), rs.rows()
        assert np.array_equal(idx, np.flatnonzero(keep)), name
        assert np.array_equal(got[:, 0], idx.astype(np.float32)), name
        assert got.tobytes() == rows[keep].tobytes(), name
        nb, na = rs.report["nbelow"], rs.report["nabove"]
        assert nb[1] == N - keep.sum() and nb.sum() == nb[1] and na.sum() == 0, name
        rs.close()


def correlated(N, np_, seed):
    """synth() with the parameters sharing one factor (plus a tenth of their own noise): the tails of up to 256 columns are
    then mostly the same rows, and a joint clip leaves rows to compact"""
    rng = np.random.default_rng(seed)
    rows = synth(N, np_, 1, seed)
    scale, shift = 1.0 + 0.25 * (np.arange(np_) % 7), np.arange(np_) % 5 - 2.0
    rows[:, :-1] = (rng.normal(0.0, 1.0, (N, 1)) + 0.1 * rng.normal(0.0, 1.0, (N, np_))) * scale + shift
    return rows


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("np_", sorted(TILE_NP))
def test_tile_heights_default_quantiles(np_, full):
    """the same heights with the thresholds of a quantile pass and every column clipping: `atomicAdd(&tails[2 * c], ...)`
    of k_clip_mark counts per column over wpw wavefronts only, and k_clip_scatter's two store paths (16 bytes where a
    workgroup's piece of x' starts on a 16-byte boundary, which depends on offs * np) both run at every height.  Kept rows,
    indices and the per-column counts against the float64 restatement, exact."""
    from mcpar_amd import engine as E
    R_ = TILE_NP[np_]
    N = 2 * R_ + (0 if full else 5)
    tile_geometry(np_, N, R_)
    rows = correlated(N, np_, seed=300 + np_)
    rs = E.clip_rows(rows, N, 1, 0.05, 0.95)
    assert not rs.report["flags"].any()
    ref = R.check(rs, rows)
    own = R.clip(rows, 0.05, 0.95)
    np.testing.assert_allclose(rs.report["lo"], own["lo"], rtol=1e-12)
    np.testing.assert_allclose(rs.report["hi"][:-1], own["hi"][:-1], rtol=1e-12)
    assert np.array_equal(own["keep"], ref["keep"])
    idx = rs.index()
    assert 0 < rs.nrows < N and idx[0] < R_ <= idx[-1], (rs.nrows, idx[:1], idx[-1:])  # a workgroup behind the first has offs > 0
    assert (rs.report["nbelow"] >= 1).all() and (rs.report["nabove"][:-1] >= 1).all()
    assert N - rs.nrows > (rs.report["nbelow"] + rs.report["nabove"]).max()  # the columns' tails are not all the same rows
    same_report(rs, E.clip_rows(rows, N, 1, 0.05, 0.95, count_only=True))
    rs.close()


@pytest.mark.parametrize("np_, nc, R_", [(41, 7, 128), (101, 3, 64), (255, 3, 32)])
def test_tile_heights_from_an_unaligned_store(np_, nc, R_):
    """clip_stage's `((unsigned long)gx & 15ul) == 0`: steps [1, T) of an engine's store with nc * np odd start off a
    16-byte boundary, so derive_tile_copy<true> takes its 4-byte path at this tile height; the same steps given as host rows
    are uploaded to a fresh allocation and take the 16-byte path.  Both must give the same row set, bit for bit."""
    from mcpar_amd import engine as E
    T = 2 + (2 * R_ + nc) // nc
    ns = T - 1
    g = E.debug_store_geometry(np_, 0, ns, nc)
    assert g["clip_rows"] == R_ and g["clip_workgroups"] >= 3 and (nc * np_ * 4) % 16 != 0, g
    eg = run(np_, nc, 30, T)
    rows = eg.samples_range(1, ns)
    # the quantiles of the first and the last parameter (the two ends of a row of the LDS tile) and of log L; a Metropolis
    # store of up to 255 independent parameters has some column's extreme in nearly every row, so the others do not clip
    lo, hi = np.full(np_ + 1, -INF), np.full(np_ + 1, INF)
    lo[[0, np_ - 1, np_]] = hi[[0, np_ - 1]] = NAN
    a = eg.clip(0.1, 0.9, INF, lo, hi, first_step=1, nsteps=ns)
    b = E.clip_rows(rows, ns, nc, 0.1, 0.9, INF, lo, hi)
    q = eg.summary((0.1, 0.9), first_step=1, nsteps=ns)["quantiles"]
    assert a.report["lo"][0] == q[0, 0] and a.report["hi"][np_ - 1] == q[np_ - 1, 1] and a.report["lo"][np_] == q[np_, 0]
    R.check(a, rows)
    same_rowset(a, b)
    assert 0 < a.nrows < a.nsource and a.index()[-1] >= R_
    for r in (a, b):
        r.close()
    eg.close()


# ---- the scan past two carries, the kept rows in their natural 64 MiB chunks ------------------------------------------------
BIG_N = 2 * (1 << 24) + 256 * 300 + 77  # 33 631 309 rows of np = 1: 131 373 workgroups, 514 scan blocks
BIG_LO, BIG_HI = (-1.0, -8.0), (1.5, -0.0009765625)  # float32-representable: the float32 comparison is the float64 rule
BIG_PERIOD = 1000003  # rows of the random block the store repeats; prime: no two workgroups hold the same rows
HOLE = slice(1 << 24, (1 << 24) + (1 << 20))


@pytest.fixture(scope="module", params=[False, True], ids=["dense", "hole"])
def big(request):
    """[BIG_N, 2] float32 -- a normal parameter and log L = -z^2 / 2 of another normal, a block of BIG_PERIOD rows repeated --
    and its clip at (BIG_LO, BIG_HI) by float32 comparisons on the host, made once per kind and left unchanged.
    hole: no row of [2^24, 2^24 + 2^20) is kept (the parameter is 2 there, above its upper bound)."""
    rng = np.random.default_rng(514)
    block = rng.standard_normal((BIG_PERIOD, 2), np.float32)
    block[:, 1] *= np.float32(-0.5) * block[:, 1]
    rows = np.empty((BIG_N, 2), np.float32)
    for i in range(0, BIG_N, BIG_PERIOD):
        rows[i:i + BIG_PERIOD] = block[:BIG_N - i]
    lo, hi = np.array(BIG_LO, np.float32), np.array(BIG_HI, np.float32)
    assert np.array_equal(lo.astype(np.float64), BIG_LO) and np.array_equal(hi.astype(np.float64), BIG_HI)
    # the comparisons of a periodic store are periodic: made on the block, repeated, and made again where the hole is
    above_lo = [np.resize(block[:, c] > lo[c], BIG_N) for c in range(2)]
    below_hi = [np.resize(block[:, c] < hi[c], BIG_N) for c in range(2)]
    if request.param:
        rows[HOLE, 0] = 2.0
        above_lo[0][HOLE], below_hi[0][HOLE] = True, False
    for c in range(2):  # (the repeated comparisons are the comparisons: a stretch across a period's end and the hole)
        for part in (slice(BIG_PERIOD - 1000, BIG_PERIOD + 1000), slice(HOLE.start - 1000, HOLE.start + 1000)):
            assert np.array_equal(above_lo[c][part], rows[part, c] > lo[c]) and np.array_equal(below_hi[c][part], rows[part, c] < hi[c])
    keep = above_lo[0] & below_hi[0] & above_lo[1] & below_hi[1]
    # kept rows per workgroup of 256: none in the hole, some in every other one, so every block sum of the scan counts
    cnt = np.add.reduceat(keep.view(np.uint8), np.arange(0, BIG_N, 256), dtype=np.int64)
    first, n = HOLE.start // 256, (HOLE.stop - HOLE.start) // 256
    assert cnt[:first].all() and cnt[first + n:].all() and (not cnt[first:first + n].any() if request.param else cnt.all())
    rows.setflags(write=False)
    yield dict(hole=request.param, rows=rows, nwg=cnt.size, index=np.flatnonzero(keep), kept=rows.view(np.uint64)[:, 0][keep],
               nbelow=[BIG_N - np.count_nonzero(a) for a in above_lo], nabove=[BIG_N - np.count_nonzero(b) for b in below_hi])


def big_geometry(b, monkeypatch):
    """the geometry the large case is there for, asserted before any result"""
    from mcpar_amd import engine as E
    monkeypatch.delenv("MCX_GATHER_CHUNK_ROWS", raising=False)
    g = E.debug_store_geometry(1, 0, BIG_N, 1)
    assert g["clip_rows"] == 256 and g["clip_scan_blocks"] > 2 * 256 and BIG_N % 256 != 0, g  # a third step of k_clip_scan<1>
    assert g["clip_workgroups"] == b["nwg"] and HOLE.start == 256 * 256 * 256, g  # the hole begins the second step
    K = b["index"].size
    assert 0.7 < K / BIG_N < 0.8 and E.debug_store_geometry(1, 0, K, 1)["gather_chunk_rows"] * 2 < K  # more than two chunks
    return g


def big_report(rs, b):
    assert not rs.report["flags"].any()  # no quantile pass ran
    assert (rs.nrows, rs.nsource, rs.ncol) == (b["index"].size, BIG_N, 2)
    assert rs.report["nbelow"].tolist() == b["nbelow"] and rs.report["nabove"].tolist() == b["nabove"]
    assert rs.report["lo"].tolist() == list(BIG_LO) and rs.report["hi"].tolist() == list(BIG_HI)


def test_scan_past_two_carries_with_natural_gather_chunks(big, monkeypatch):
    """np = 1, one chain, N = 2 * 2^24 + 256 * 300 + 77 rows.
      k_clip_scan<1>, `carry += s[DERIVE_BLOCK - 1]` and `boff[i] = carry + (incl - v)`: 514 scan blocks are three steps of
        CLIP_FAN = 256, two full and one of two blocks (the last workgroup ragged, 77 rows); every other test has at most two
        blocks and never adds a carry.  About three rows in four are kept in every workgroup, so every bsum is non-zero and
        every offset behind block 255 is wrong without the first carry, behind block 511 without the second: the kept rows
        of those workgroups would land on other rows' places, which index() and rows() show.
      hole: no row of [2^24, 2^24 + 2^20) is kept -- bsum is zero for blocks 256 .. 271, the first of the second step, so
        a scan that mishandles empty blocks, or a carry taken from the wrong element, shows as well; k_clip_scatter's
        `if (kw == 0) return` is taken by 4096 workgroups in a row.
      gather_to_host, `for (done = 0; done < n; done += chunk)` with its natural chunk of 64 MiB / 8 bytes = 8 388 608 rows:
        the 25 M kept rows leave in three chunks without MCX_GATHER_CHUNK_ROWS.
    Explicit bounds on both columns: no quantile pass runs.  No row-number marker: row numbers above 2^24 are not floats."""
    from mcpar_amd import engine as E
    big_geometry(big, monkeypatch)
    rs = E.clip_rows(big["rows"], BIG_N, 1, lo=BIG_LO, hi=BIG_HI)
    big_report(rs, big)
    idx = rs.index()
    assert np.array_equal(idx, big["index"]), np.flatnonzero(idx != big["index"])[:4]
    del idx
    assert np.array_equal(rs.rows().view(np.uint64)[:, 0], big["kept"])
    rs.close()


def test_scan_past_two_carries_count_only(big, monkeypatch):
    """the same store with count_only: the total K is `boff[nb] = carry` after the last step of k_clip_scan<1>, the one
    number of the report that depends on every carry"""
    from mcpar_amd import engine as E
    big_geometry(big, monkeypatch)
    rs = E.clip_rows(big["rows"], BIG_N, 1, lo=BIG_LO, hi=BIG_HI, count_only=True)
    assert not rs.h
    big_report(rs, big)


# ---- values on and around a threshold ---------------------------------------------------------------------------------------
def test_ties_on_a_threshold_are_dropped():
    from mcpar_amd import engine as E
    nsteps, np_, nc = 20, 2, 30
    rows = synth(nsteps, np_, nc, 7)
    rng = np.random.default_rng(7)
    rows[:, 0] = rng.integers(0, 5, nsteps * nc)  # quantiles 0.25 and 0.75 are data values: a == b in the type-7 formula
    rs = E.clip_rows(rows, nsteps, nc, 0.25, 0.75, ll_hi=INF)
    lo0, hi0 = rs.report["lo"][0], rs.report["hi"][0]
    assert lo0 in (0.0, 1.0, 2.0) and hi0 in (2.0, 3.0, 4.0) and lo0 < hi0
    R.check(rs, rows)
    assert rs.report["nbelow"][0] == (rows[:, 0] <= lo0).sum() and rs.report["nabove"][0] == (rows[:, 0] >= hi0).sum()
    kept0 = rs.rows()[:, 0]
    assert kept0.size and kept0.min() > lo0 and kept0.max() < hi0
    own = R.clip(rows, 0.25, 0.75, INF)
    assert own["lo"][0] == lo0 and own["hi"][0] == hi0
    rs.close()


def test_negative_zero_against_a_threshold_of_zero():
    from mcpar_amd import engine as E
    rows = synth(10, 1, 10, 8)
    rows[:, 0] = np.where(np.arange(100) % 3 == 0, -0.0, np.where(np.arange(100) % 3 == 1, 0.0, 1.0)).astype(np.float32)
    assert np.signbit(rows[0, 0]) and rows[0, 0] == 0.0
    rs = E.clip_rows(rows, 10, 10, lo=[0.0, -INF], hi=[INF, INF])
    R.check(rs, rows)
    assert rs.nrows == 33 and np.all(rs.rows()[:, 0] == 1.0) and rs.report["nbelow"][0] == 67
    rs2 = E.clip_rows(rows, 10, 10, lo=[-INF, -INF], hi=[-0.0, INF])  # nothing is below -0.0 among 0.0, -0.0 and 1.0
    assert rs2.nrows == 0 and rs2.report["nabove"][0] == 100
    rs.close()
    rs2.close()


def test_nan_values():
    from mcpar_amd import engine as E
    nsteps, np_, nc = 12, 3, 20
    rows = synth(nsteps, np_, nc, 9)
    bad = [0, 64, 65, 239]
    rows[bad, 1] = np.nan
    rs = E.clip_rows(rows, nsteps, nc, 0.05, 0.95)
    assert rs.nrows == 0 and rs.report["flags"].tolist() == [0, 1, 0, 0]
    assert np.isnan(rs.report["lo"][1]) and np.isnan(rs.report["hi"][1])
    assert rs.report["nbelow"][1] == 240 and rs.report["nabove"][1] == 240
    R.check(rs, rows)
    assert rs.rows().shape == (0, 4)
    # both bounds of that column given: only the NaN rows go because of it, and they count on both sides
    lo, hi = np.full(4, NAN), np.full(4, NAN)
    lo[1], hi[1] = -INF, INF
    rs2 = E.clip_rows(rows, nsteps, nc, 0.0, 1.0, ll_hi=INF, lo=[-INF, -INF, -INF, -INF], hi=[INF, INF, INF, INF])
    assert rs2.nrows == 236 and rs2.report["nbelow"].tolist() == [0, 4, 0, 0] and rs2.report["nabove"].tolist() == [0, 4, 0, 0]
    assert np.array_equal(rs2.index(), np.setdiff1d(np.arange(240), bad)) and not rs2.report["flags"].any()
    rs3 = E.clip_rows(rows, nsteps, nc, 0.05, 0.95, lo=lo, hi=hi)  # the other columns by their quantiles
    assert rs3.report["flags"].tolist() == [0, 1, 0, 0] and rs3.report["nbelow"][1] == 4 and rs3.report["nabove"][1] == 4
    ref = R.check(rs3, rows)
    assert 0 < rs3.nrows < 236 and not np.isin(bad, ref["index"]).any()
    own = R.clip(rows, 0.05, 0.95, 0.0, lo, hi)
    assert np.array_equal(own["keep"], ref["keep"])
    for r in (rs, rs2, rs3):
        r.close()


def test_minus_inf_in_log_l():
    from mcpar_amd import engine as E
    nsteps, np_, nc = 12, 2, 20
    rows = synth(nsteps, np_, nc, 10)
    bad = [3, 128]
    rows[bad, -1] = -np.inf
    rs = E.clip_rows(rows, nsteps, nc, 0.05, 0.95)
    assert rs.report["flags"].tolist() == [0, 0, 1]  # flagged by the quantile pass; its quantiles are finite order statistics
    ref = R.check(rs, rows)
    own = R.clip(rows, 0.05, 0.95)
    assert np.array_equal(own["keep"], ref["keep"]) and not np.isin(bad, ref["index"]).any()
    # with both bounds given the -inf rows fail the strict lower comparison alone
    rs2 = E.clip_rows(rows, nsteps, nc, lo=[-INF] * 3, hi=[INF] * 3)
    assert rs2.nrows == 238 and rs2.report["nbelow"].tolist() == [0, 0, 2] and rs2.report["nabove"].tolist() == [0, 0, 0]
    R.check(rs2, rows)
    rs.close()
    rs2.close()


def test_ll_hi_rule():
    from mcpar_amd import engine as E
    rows = synth(10, 1, 9, 11)
    rows[:, -1] = np.tile(np.array([-1.0, 0.0, 1.0], np.float32), 30)
    lo, hi = [-INF, -INF], [INF, NAN]
    zero = E.clip_rows(rows, 10, 9, 0.0, 1.0, 0.0, lo, hi)
    assert zero.nrows == 30 and np.all(zero.rows()[:, -1] == -1.0) and zero.report["hi"][-1] == 0.0 and zero.report["nabove"][-1] == 60
    none = E.clip_rows(rows, 10, 9, 0.0, 1.0, INF, lo, hi)
    assert none.nrows == 90 and none.report["hi"][-1] == INF and none.report["nabove"][-1] == 0
    quant = E.clip_rows(rows, 10, 9, 0.0, 1.0, NAN, lo, hi)  # the qhi quantile: the maximum, 1
    assert quant.nrows == 60 and quant.report["hi"][-1] == 1.0 and np.all(quant.rows()[:, -1] <= 0.0) and quant.report["nabove"][-1] == 30
    over = E.clip_rows(rows, 10, 9, 0.0, 1.0, 0.0, lo, [INF, 0.5])  # hi[ncol - 1] replaces ll_hi
    assert over.nrows == 60 and over.report["hi"][-1] == 0.5
    for r in (zero, none, quant, over):
        R.check(r, rows)
        r.close()


# ---- the row set as an object -----------------------------------------------------------------------------------------------
def test_count_only_allocates_no_row_set():
    from mcpar_amd import engine as E
    rows = shape_rows((17, 17, 16))
    gc.collect()
    before = E.debug_live_resources()
    co = E.clip_rows(rows, 17, 16, 0.05, 0.95, count_only=True)
    assert E.debug_live_resources() == before and not co.h
    rs = E.clip_rows(rows, 17, 16, 0.05, 0.95)
    during = E.debug_live_resources()
    assert during[0] == before[0] + 3 and during[2] == before[2] + 1  # x', ly', the indices; its stream
    same_report(co, rs)
    rs.close()
    assert E.debug_live_resources() == before


def test_draw():
    from mcpar_amd import engine as E
    rows = shape_rows((17, 17, 16))
    rs = E.clip_rows(rows, 17, 16, 0.05, 0.95)
    kept = rs.rows()
    got, idx = rs.draw(300, 4242)
    assert np.array_equal(idx, E.debug_draw_indices(4242, rs.nrows, 0, 300)) and idx.max() < rs.nrows
    assert got.tobytes() == kept[idx].tobytes()
    assert rs.rows(3, 10).tobytes() == kept[3:13].tobytes() and np.array_equal(rs.index(3, 10), rs.index()[3:13])
    rs.close()


def test_store_of_kept_rows():
    from mcpar_amd import McxError
    from mcpar_amd import engine as E
    nsteps, np_, nc = 60, 5, 40
    rows = synth(nsteps, np_, nc, 12)
    rs = E.clip_rows(rows, nsteps, nc, 0.02, 0.98)
    kept = rs.rows()
    K = rs.nrows
    assert 1500 < K < 2400
    st = rs.store(nc=64)
    T = K // 64
    assert st.shape == (T, 64, np_ + 1) and st.dropped == K - T * 64 and rs.dropped == st.dropped
    part = kept[:T * 64]
    assert st.rows().tobytes() == part.tobytes()
    same_bytes(st.summary((0.1, 0.9)), E.rows_summary(part, T, 64, probs=(0.1, 0.9)), "summary")
    same_bytes(st.covariance(), E.rows_covariance(part, T, 64), "covariance")
    same_bytes(st.density(n=64), E.rows_density(part, T, 64, n=64), "density")
    st2 = rs.store(nc=7, first_row=5, nsteps=11)
    assert st2.shape == (11, 7, np_ + 1) and st2.rows().tobytes() == kept[5:5 + 77].tobytes() and st2.dropped == K - 5 - 77
    for args in (dict(nc=64, nsteps=T + 1), dict(nc=0, nsteps=1), dict(nc=1, nsteps=0), dict(nc=1, first_row=K, nsteps=1),
                 dict(nc=1, first_row=-1, nsteps=1)):
        with pytest.raises(McxError) as ei:
            rs.store(**args)
        assert ei.value.code == 1
    rs.close()  # the stores outlive the row set
    assert st.rows().tobytes() == part.tobytes()
    st.close()
    st2.close()


# ---- the engine's store and a derived store ---------------------------------------------------------------------------------
def run(d, n, nburn, nsamp):
    import mcpar_amd as M
    vg, keep = M.make_vlfunc(M.VL_GAUSSIAN, d, np.concatenate([np.linspace(-1.0, 1.0, d), np.linspace(0.5, 2.0, d)]).astype(np.float32))
    eg = M.Engine(d, n, pl=1.0)
    eg.run(nsamp, nburn, O.default_pinit(d, n), vg)
    eg._vl_keep = keep
    return eg


def test_engine_rows_and_derived_store_give_the_same_bytes():
    import mcpar_amd as M
    from mcpar_amd import engine as E
    d, nc, T = 5, 333, 40
    gc.collect()
    before = E.debug_live_resources()
    eg = run(d, nc, 100, T)
    # the whole store, and a sub-range that starts off 16 bytes (one step is 333 * 5 floats)
    for first, nsteps in ((0, None), (1, 30)):
        ns = T - first if nsteps is None else nsteps
        rows = eg.samples_range(first, ns)
        a = eg.clip(0.05, 0.95, first_step=first, nsteps=nsteps)
        assert a.nsource == ns * nc and 0 < a.nrows < a.nsource
        q = eg.summary((0.05, 0.95), first_step=first, nsteps=nsteps)["quantiles"]
        assert a.report["lo"].tobytes() == q[:, 0].tobytes() and a.report["hi"][:-1].tobytes() == q[:-1, 1].tobytes()
        assert a.report["hi"][-1] == 0.0
        R.check(a, rows)
        b = E.clip_rows(rows, ns, nc, 0.05, 0.95)
        same_rowset(a, b)
        same_report(a, eg.clip(0.05, 0.95, first_step=first, nsteps=nsteps, count_only=True))
        a.close()
        b.close()
    ident = eg.derive(M.derive_linear(np.eye(d, dtype=np.float32), np.zeros(d, np.float32)))
    a, c = eg.clip(0.05, 0.95), ident.clip(0.05, 0.95)
    same_rowset(a, c)
    # the row sets outlive the engine and the store they came from
    kept, idx = a.rows(), c.index()
    eg.close()
    ident.close()
    assert a.rows().tobytes() == kept.tobytes() and c.rows().tobytes() == kept.tobytes() and np.array_equal(a.index(), idx)
    got, di = c.draw(50, 7)
    assert got.tobytes() == kept[di].tobytes()
    a.close()
    c.close()
    gc.collect()
    assert E.debug_live_resources() == before


def test_clip_times():
    eg = run(5, 333, 100, 40)
    ms = eg.clip_times(0.05, 0.95)
    assert ms.shape == (5,) and np.all(ms >= 0.0) and ms[4] >= ms[0] and ms[1] > 0.0 and ms[3] > 0.0
    eg.close()


def test_refusals():
    import mcpar_amd as M
    from mcpar_amd import McxError
    eg = M.Engine(4, 64, pl=1.0)
    with pytest.raises(McxError) as ei:
        eg.clip(nsteps=4)
    assert ei.value.code == 1 and "the sample store is empty" in str(ei.value)
    eg.close()
    eg = run(4, 64, 20, 10)
    for first, nsteps in ((0, 11), (8, 3), (-1, 4)):
        with pytest.raises(McxError) as ei:
            eg.clip(first_step=first, nsteps=nsteps)
        assert ei.value.code == 1 and "not in the sample store (10 steps)" in str(ei.value)
    with pytest.raises(McxError) as ei:
        eg.clip(nsteps=0)
    assert ei.value.code == 1 and "at least one step" in str(ei.value)
    with pytest.raises(McxError) as ei:
        eg.clip(0.9, 0.1)
    assert ei.value.code == 1 and "qlo < qhi" in str(ei.value)
    rs = eg.clip()
    for bad in ((0, rs.nrows + 1), (rs.nrows, 1), (-1, 1)):
        with pytest.raises(McxError):
            rs.rows(*bad)
        with pytest.raises(McxError):
            rs.index(*bad)
    with pytest.raises(McxError):
        rs.draw(-1, 0)
    rs.close()
    eg.close()
