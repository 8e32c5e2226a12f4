"""Profile likelihoods of the sample store on the GPU against tests/profile_ref.py.

What must match: cnt, row, row_hat, the counts and flags of a column, nseg and the flags of an interval, and the bits of lmax,
lhat, xat, xhat, from, to and path are equal; pl, plh, the drops and the interval ends agree to 1e-12 relative (the level's drop
goes through a normal quantile that the restatement gets by another route).  Values and log L are made of small integers, so
that ties and exact comparisons mean something."""
import numpy as np
import pytest

import oracle_lib as O
import profile_ref as R

pytestmark = pytest.mark.gpu

RTOL = 1e-12
EXACT = ("cnt", "row", "row_hat", "nvalues", "nbinned", "ndropped", "nempty", "flags")
BITS32 = ("lmax", "xat")
BITS64 = ("from", "to", "lhat", "xhat")
CLOSE = ("pl", "plh")


def int_rows(seed, T, nc, np_, nll=8, span=9):
    """rows [T * nc, np + 1]: values k / 4 with k in [-span, span], log L quantised to nll values: every bin has ties"""
    rng = np.random.default_rng([seed, T, nc, np_])
    rows = np.empty((T * nc, np_ + 1), np.float32)
    rows[:, :np_] = rng.integers(-span, span + 1, (T * nc, np_)) * 0.25
    rows[:, np_] = rng.integers(-nll, 0, T * nc) * 0.5
    return rows


def check(got, ref, what=""):
    for name in EXACT:
        assert np.array_equal(got[name], ref[name]), (what, name)
    for name in BITS32:
        assert np.array_equal(got[name].view(np.uint32), ref[name].view(np.uint32)), (what, name)
    for name in BITS64:
        assert np.array_equal(got[name].view(np.uint64), ref[name].view(np.uint64)), (what, name)
    for name in CLOSE:
        np.testing.assert_allclose(got[name], ref[name], rtol=RTOL, atol=0, equal_nan=True, err_msg="%s %s" % (what, name))
    gi, ri = got["intervals"], ref["intervals"]
    assert gi.shape == ri.shape
    for name in ("nseg", "flags"):
        assert np.array_equal(gi[name], ri[name]), (what, name)
    for name in ("p", "drop", "lo", "hi", "lo_hull", "hi_hull"):
        np.testing.assert_allclose(gi[name], ri[name], rtol=RTOL, atol=0, equal_nan=True, err_msg="%s %s" % (what, name))
    if "path" in got:
        assert np.array_equal(got["path"].view(np.uint32), ref["path"].view(np.uint32)), (what, "path")


def same_bytes(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


# (np, nc, T, n): one-column tile, a partial tile, two tiles, three; one chain, a partial block, a full one, two blocks
CASES = [(1, 1, 2, 2), (1, 37, 67, 7), (3, 37, 67, 7), (3, 300, 2, 512), (9, 256, 1, 512), (9, 1, 67, 2), (17, 300, 2, 7), (17, 37, 1, 512)]


@pytest.mark.parametrize("np_,nc,T,n", CASES)
def test_profile_against_the_restatement(np_, nc, T, n):
    from mcpar_amd import engine as E
    rows = int_rows(1, T, nc, np_)
    got = E.rows_profile(rows, T, nc, n=n, path=True)
    check(got, R.profile(rows, n=n), (np_, nc, T, n))
    assert (got["nbinned"] == T * nc).all() and (got["ndropped"] == 0).all()
    same_bytes(got, E.rows_profile(rows, T, nc, n=n, path=True))  # two calls in a row


@pytest.mark.parametrize("np_,nc", [(1, 300), (9, 37)])
def test_a_range_that_crosses_a_step_chunk(np_, nc):
    """one step more than the chunk the geometry reports: the second chunk's workgroups hold one step each"""
    from mcpar_amd import engine as E
    g = E.debug_profile_geometry(np_, 8, nc, 7)
    T = g["chunk_steps"] + 1
    assert E.debug_profile_geometry(np_, T, nc, 7)["chunks"] == 2 and E.debug_profile_geometry(np_, T - 1, nc, 7)["chunks"] == 1
    rows = int_rows(2, T, nc, np_)
    rows[-1, np_] = 1.0  # the maximum is in the last step: a row of the second chunk
    got = E.rows_profile(rows, T, nc, n=7)
    ref = R.profile(rows, n=7)
    ref.pop("path")
    check(got, ref)
    assert got["row_hat"][0] == T * nc - 1


def test_one_bin_one_log_l_a_million_rows():
    """2^20 values of one column in one bin with one log L: the winner is row 0 and the count is exact (the contention and
    read-before-max case).  Column 0 is constant (to == from: bin 0); column 1 has one other value in the last row"""
    from mcpar_amd import engine as E
    T, nc = 4096, 256
    rows = np.empty((T * nc, 3), np.float32)
    rows[:, 0], rows[:, 1], rows[:, 2] = 1.0, 0.5, 3.0
    rows[-1, 1] = 8.0
    got = E.rows_profile(rows, T, nc, n=2)
    assert got["cnt"].tolist() == [[T * nc, 0], [T * nc - 1, 1]]
    assert got["row"].tolist() == [[0, -1], [0, T * nc - 1]] and (got["row_hat"] == 0).all()
    assert (got["from"][0], got["to"][0], got["nempty"][0], got["ndropped"][0]) == (1.0, 1.0, 1, 0)
    ref = R.profile(rows, n=2)
    ref.pop("path")
    check(got, ref)


def test_log_l_that_is_not_finite():
    from mcpar_amd import engine as E
    T, nc, np_ = 67, 37, 3
    rows = int_rows(3, T, nc, np_)
    ll = rows[:, np_]
    ll[::5] = np.nan
    ll[::7] = -np.inf
    ll[3], ll[4] = -0.0, 0.0  # the largest two: +0 wins although -0 comes first
    got = E.rows_profile(rows, T, nc, n=7, path=True)
    check(got, R.profile(rows, n=7))
    assert (got["row_hat"] == 4).all() and (got["flags"] == 0).all()
    # a bin whose rows all have NaN or -inf: lmax -inf as stored for the first such row, pl -inf, the hull leaves it out
    rows2 = rows.copy()
    rows2[rows2[:, 0] == 0.25, np_] = np.nan
    got = E.rows_profile(rows2, T, nc, n=512, path=True)
    check(got, R.profile(rows2, n=512))
    dead = (got["cnt"][0] > 0) & np.isneginf(got["lmax"][0])
    assert dead.sum() == 1 and np.isneginf(got["pl"][0][dead]).all() and np.isneginf(got["plh"][0][dead]).all()
    # +inf: the maximum is not finite
    rows[11, np_] = np.inf
    got = E.rows_profile(rows, T, nc, n=7, path=True)
    check(got, R.profile(rows, n=7))
    assert (got["flags"] == R.LL_NONFINITE).all() and np.isnan(got["pl"]).all() and np.isnan(got["intervals"]["lo"]).all()
    # every log L a NaN: lhat = -inf, row_hat = 0
    rows[:, np_] = np.nan
    got = E.rows_profile(rows, T, nc, n=7)
    assert (got["row_hat"] == 0).all() and np.isneginf(got["lhat"]).all() and (got["flags"] == R.LL_NONFINITE).all()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_column_that_is_not_finite_is_alone(bad):
    from mcpar_amd import engine as E
    T, nc, np_ = 2, 300, 9
    rows = int_rows(4, T, nc, np_)
    clean = E.rows_profile(rows, T, nc, n=7, path=True)
    rows[123, 8] = bad
    got = E.rows_profile(rows, T, nc, n=7, path=True)
    check(got, R.profile(rows, n=7))
    assert got["flags"].tolist() == [0] * 8 + [1] and got["nbinned"][8] == 0 and np.isnan(got["lhat"][8])
    assert (got["intervals"]["flags"][8] == 1).all() and np.isnan(got["pl"][8]).all()
    for name in ("cnt", "row", "lmax", "xat", "pl", "plh", "intervals"):
        assert got[name][:8].tobytes() == clean[name][:8].tobytes(), name


def test_constant_column_spec_ranges_and_clip():
    from mcpar_amd import engine as E
    T, nc, np_ = 67, 37, 3
    rows = int_rows(5, T, nc, np_)
    rows[:, 1] = -0.75  # a constant column
    nan = np.nan
    for kw in (dict(), dict(from_=[-1.0, nan, nan], to=[1.25, nan, 0.5]),  # inside the data: both ends drop values
               dict(clip=(0.1, 0.9)), dict(clip=(0.05, 0.75), to=[nan, nan, 2.0]), dict(levels=(0.5, 0.9, 0.99)),
               dict(drops=(0.25, 1.0, 3.0, 100.0))):
        for n in (2, 7, 64):
            got = E.rows_profile(rows, T, nc, n=n, path=True, **kw)
            check(got, R.profile(rows, n=n, **kw), (kw, n))
            assert got["cnt"][1, 0] == T * nc and got["nempty"][1] == n - 1
    got = E.rows_profile(rows, T, nc, n=7, from_=[-1.0, nan, nan], to=[1.25, nan, 0.5])
    assert got["ndropped"][0] > 0 and got["ndropped"][2] > 0 and got["ndropped"][1] == 0
    assert got["intervals"]["flags"][1, 0] == R.OPEN_LO | R.OPEN_HI | R.HULL_OPEN_LO | R.HULL_OPEN_HI


def test_the_sweep_alone():
    from mcpar_amd import engine as E
    T, nc, np_, n = 67, 37, 17, 12
    rows = int_rows(6, T, nc, np_)
    f, t = np.full(np_, -2.0), np.full(np_, 1.5)
    keys, cnt, hat = E.debug_rows_profile_bins(rows, T, nc, n, f, t)
    K = R.row_keys(rows[:, np_])
    assert hat == int(K.max())
    for c in range(np_):
        rk, rc = R.max_keys(R.bins_of(rows[:, c], n, -2.0, 1.5, n / 3.5), K, n)
        assert np.array_equal(keys[c], rk) and np.array_equal(cnt[c], rc), c


def run(d, n, nburn, nsamp):
    import mcpar_amd as M
    vg, keep = M.make_vlfunc(M.VL_ROSENBROCK1, d)
    eg = M.Engine(d, n, pl=1.0)
    eg.run(nsamp, nburn, O.default_pinit(d, n), vg)
    eg._vl_keep = keep
    return eg


def test_engine_rows_and_stores_give_the_same_bytes_and_the_engine_s_maximum():
    from mcpar_amd import engine as E
    eg = run(4, 512, 60, 24)
    rows = eg.samples
    T, nc = 24, 512
    assert rows.shape == (T * nc, 5)
    kw = dict(n=64, path=True, clip=(0.01, 0.99))
    a = eg.profile_likelihood(**kw)
    check(a, R.profile(rows, n=64, clip=(0.01, 0.99)))
    same_bytes(a, E.rows_profile(rows, T, nc, **kw))
    same_bytes(a, eg.profile_likelihood(**kw))
    st = eg.select_chains(list(range(nc)))
    assert st.rows().tobytes() == rows.tobytes()
    same_bytes(a, st.profile_likelihood(**kw))
    st.close()
    # a derived store: the profile likelihood of functions of the parameters
    A = np.array([[1.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, -1.0]], np.float32)
    ds = eg.derive(E.derive_linear(A, np.zeros(2, np.float32)))
    check(ds.profile_likelihood(n=33, path=True), R.profile(ds.rows(), n=33))
    ds.close()
    # an inner range
    inner = eg.profile_likelihood(n=7, first_step=3, nsteps=11)
    ref = R.profile(eg.samples_range(3, 11), n=7)
    ref.pop("path")
    check(inner, ref)
    # the engine's own maximum: lhat is mcx_samples_maxlike's lmax bit for bit; where it is attained once, path at row_hat's
    # bin is its params
    lm, params = eg.maxlike()
    ll = rows[:, 4]
    full = eg.profile_likelihood(n=64, path=True)
    assert np.float32(full["lhat"][0]).view(np.uint32) == np.float32(lm).view(np.uint32)
    hits = rows[ll == np.float32(lm)]
    assert hits.shape[0] >= 1
    once = (hits[:, :4] == hits[0, :4]).all()  # attained once, or by one chain that stayed where it was
    for c in range(4):
        j = int(np.flatnonzero(full["row"][c] == full["row_hat"][c])[0])
        assert full["pl"][c, j] == 0.0 and full["path"][c, j].tobytes() == rows[full["row_hat"][c]].tobytes()
        if once:
            assert full["path"][c, j, :4].tobytes() == params.tobytes() and np.float32(full["xhat"][c]) == params[c]
    eg.close()


def test_a_queued_run_is_finished_first():
    import mcpar_amd as M
    from mcpar_amd import engine as E
    vg, keep = M.make_vlfunc(M.VL_ROSENBROCK1, 4)
    eg = M.Engine(4, 512, pl=1.0)
    eg.set_option(E.OPT_ASYNC_RUN, 1)
    eg.run(24, 60, O.default_pinit(4, 512), vg)
    got = eg.profile_likelihood(n=16)
    ref = R.profile(eg.samples, n=16)
    ref.pop("path")
    check(got, ref)
    eg.close()
