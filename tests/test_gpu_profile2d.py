"""Pair profile likelihoods of the sample store on the GPU against tests/profile_ref.py: cnt, row, the
counts, the flags and the level counts equal, the bits of lmax, xat_a, xat_b, lhat, xhat, from and to equal, z to 1e-12 relative.
Values and log L are made of small integers, so that every cell has ties.  The last case has more rows than k_profile_keys
has lanes (4096 workgroups of 256): the rows from 2^20 on are those of a lane's second turn, and some of them are made the only
maximum of their cell, so that their keys show in row and lmax."""
import numpy as np
import pytest

import profile_ref as R
from test_gpu_profile import RTOL, int_rows, same_bytes

pytestmark = pytest.mark.gpu

EXACT = ("pairs", "cnt", "row", "row_hat", "nvalues", "nbinned", "nempty", "flags", "col_flags", "nlevel")
BITS32 = ("lmax", "xat_a", "xat_b")
BITS64 = ("from", "to", "lhat", "xhat")


def check(got, ref, what=""):
    assert sorted(got) == sorted(ref)
    for name in EXACT:
        assert np.array_equal(got[name], ref[name]), (what, name)
    for name in BITS32:
        assert np.array_equal(got[name].view(np.uint32), ref[name].view(np.uint32)), (what, name)
    for name in BITS64:
        assert np.array_equal(got[name].view(np.uint64), ref[name].view(np.uint64)), (what, name)
    np.testing.assert_allclose(got["z"], ref["z"], rtol=RTOL, atol=0, equal_nan=True, err_msg=str(what))


# drops, so that the level counts compare integers with integers' halves
DROPS = (0.5, 1.25, 3.0)


@pytest.mark.parametrize("g", [8, 33, 64])
@pytest.mark.parametrize("np_,nc,T", [(3, 37, 67), (17, 300, 2)])
def test_pairs_against_the_restatement(g, np_, nc, T):
    from mcpar_amd import engine as E
    rows = int_rows(11, T, nc, np_)
    pairs = None if np_ == 3 else [(0, 1), (1, 0), (2, 16), (16, 2), (8, 7), (15, 0)]  # (b, a) next to (a, b); across the tiles
    got = E.rows_profile2d(rows, T, nc, g=g, pairs=pairs, drops=DROPS)
    check(got, R.profile2d(rows, g=g, pairs=pairs, drops=DROPS), (g, np_))
    same_bytes(got, E.rows_profile2d(rows, T, nc, g=g, pairs=pairs, drops=DROPS))  # two calls in a row
    if np_ == 3:
        assert got["pairs"].tolist() == [[0, 1], [0, 2], [1, 2]]  # the default list
        assert (got["nbinned"] == T * nc).all()
    else:
        for p, q in ((0, 1), (2, 3)):  # (b, a) is the transpose of (a, b)
            for name in ("cnt", "row", "lmax", "z"):
                assert np.array_equal(got[name][p].T, got[name][q], equal_nan=True), name
            assert got["xat_a"][p].T.tobytes() == got["xat_b"][q].tobytes()
    # the marginal maximum over ib of a pair's lmax is the 1-D lmax of column a at n = g
    one = E.rows_profile(rows, T, nc, n=g)
    for p, (a, b) in enumerate(got["pairs"]):
        assert np.array_equal(got["lmax"][p].max(axis=1), one["lmax"][a]), (p, a, b)
        assert np.array_equal(got["lmax"][p].max(axis=0), one["lmax"][b]), (p, a, b)
        assert np.array_equal(got["cnt"][p].sum(axis=1), one["cnt"][a])


def test_rows_that_cross_a_pair_chunk_and_default_levels():
    from mcpar_amd import engine as E
    np_, nc = 3, 301
    geo = E.debug_profile_geometry(np_, 8, nc, 7, g=8, npairs=3)
    T = geo["pair_chunk_rows"] // nc + 1  # a little more than one chunk of rows, not a multiple of four
    assert T * nc % 4 != 0 and E.debug_profile_geometry(np_, T, nc, 7, g=8, npairs=3)["pair_chunks"] == 2
    rows = int_rows(12, T, nc, np_)
    rows[-1, np_] = 1.0  # the maximum is the last row
    got = E.rows_profile2d(rows, T, nc, g=8)
    ref = R.profile2d(rows, g=8)
    check(got, ref)
    assert (got["row_hat"] == T * nc - 1).all() and got["nlevel"].shape == (3, 2)


def test_dropped_values_clip_and_log_l_that_is_not_finite():
    from mcpar_amd import engine as E
    T, nc, np_ = 67, 37, 3
    rows = int_rows(13, T, nc, np_)
    nan = np.nan
    kw = dict(from_=[-1.0, nan, nan], to=[1.25, nan, 0.5], drops=DROPS)
    got = E.rows_profile2d(rows, T, nc, g=9, **kw)
    check(got, R.profile2d(rows, g=9, **kw))
    assert (got["nbinned"] < T * nc).all() and (got["nbinned"] > 0).all()
    got = E.rows_profile2d(rows, T, nc, g=16, clip=(0.1, 0.9), levels=(0.5, 0.9))
    check(got, R.profile2d(rows, g=16, clip=(0.1, 0.9), levels=(0.5, 0.9)))
    rows[::5, np_] = nan
    rows[::7, np_] = -np.inf
    got = E.rows_profile2d(rows, T, nc, g=8, drops=DROPS)
    check(got, R.profile2d(rows, g=8, drops=DROPS))
    rows[5, np_] = np.inf
    got = E.rows_profile2d(rows, T, nc, g=8, drops=DROPS)
    check(got, R.profile2d(rows, g=8, drops=DROPS))
    assert (got["flags"] == R.LL_NONFINITE).all() and np.isnan(got["z"]).all() and (got["nlevel"] == 0).all()


def test_a_column_that_is_not_finite_poisons_its_own_pairs_only():
    from mcpar_amd import engine as E
    T, nc, np_ = 2, 300, 9
    rows = int_rows(14, T, nc, np_)
    pairs = [(0, 1), (8, 1), (2, 8), (7, 3)]
    clean = E.rows_profile2d(rows, T, nc, g=12, pairs=pairs, drops=DROPS)
    rows[77, 8] = np.nan
    got = E.rows_profile2d(rows, T, nc, g=12, pairs=pairs, drops=DROPS)
    check(got, R.profile2d(rows, g=12, pairs=pairs, drops=DROPS))
    assert got["flags"].tolist() == [0, 1, 1, 0] and got["col_flags"].tolist() == [0] * 8 + [1]
    assert np.isnan(got["z"][1]).all() and (got["cnt"][2] == 0).all()
    for name in ("cnt", "row", "lmax", "z", "xat_a", "xat_b", "nlevel"):
        for p in (0, 3):
            assert got[name][p].tobytes() == clean[name][p].tobytes(), (name, p)
    # every pair poisoned: nothing goes to the pair sweep
    got = E.rows_profile2d(rows, T, nc, g=12, pairs=[(8, 1)], drops=DROPS)
    check(got, R.profile2d(rows, g=12, pairs=[(8, 1)], drops=DROPS))


def test_engine_rows_and_store_give_the_same_bytes():
    from mcpar_amd import engine as E
    from test_gpu_profile import run
    eg = run(4, 512, 60, 24)
    rows, T, nc = eg.samples, 24, 512
    a = eg.profile_likelihood2d(g=32)
    check(a, R.profile2d(rows, g=32))
    same_bytes(a, E.rows_profile2d(rows, T, nc, g=32))
    same_bytes(a, eg.profile_likelihood2d(g=32))
    st = eg.select_chains(list(range(nc)))
    same_bytes(a, st.profile_likelihood2d(g=32))
    st.close()
    inner = eg.profile_likelihood2d(g=8, pairs=[(3, 0)], first_step=3, nsteps=11)
    check(inner, R.profile2d(eg.samples_range(3, 11), g=8, pairs=[(3, 0)]))
    eg.close()


def test_more_rows_than_lanes_of_the_key_sweep():
    """N = 1 048 833 > 4096 * 256: k_profile_keys walks a grid stride.  The highest log L sits in row N - 5 and, equal, in row
    700 001: the earlier row is the maximum; row N - 5 is the maximum of its own cell, and ten more rows of the second turn are
    their cells' only maxima"""
    from mcpar_amd import engine as E
    np_, nc, T, g = 2, 3, 349611, 8
    N = T * nc
    geo = E.debug_profile_geometry(np_, T, nc, 7, g=g, npairs=1)
    first_turn = geo["keys_max_workgroups"] * geo["block"]
    assert (geo["keys_workgroups"], geo["keys_max_workgroups"], geo["block"]) == (4096, 4096, 256) and N == 1048833 > first_turn
    assert geo["pair_chunks"] == 17
    rows = int_rows(15, T, nc, np_)
    early, late = 700001, N - 5
    assert early < first_turn <= late
    rows[early] = (-2.25, -2.25, 1.0)
    rows[late] = (2.25, 2.25, 1.0)
    second = first_turn + 23 * np.arange(10)  # rows of the second turn: above every row's log L but those two, in ten cells
    rows[second, 0] = -2.25 + 0.5 * np.arange(10).clip(0, 8)
    rows[second, 1] = 2.25 - 0.5 * (np.arange(10) % 3)
    rows[second, 2] = 0.25
    ref = R.profile2d(rows, g=g, pairs=[(0, 1)], drops=DROPS)
    # the reference alone: which row it picks, and that rows of the second turn decide cells
    assert (ref["row_hat"] == early).all() and ref["row"][0, 0, 0] == early and ref["row"][0, g - 1, g - 1] == late
    assert ref["lmax"][0, 0, 0] == ref["lmax"][0, g - 1, g - 1] == 1.0
    won = np.intersect1d(ref["row"][0].reshape(-1), second)
    assert won.size >= 8 and (ref["row"][0] >= first_turn).sum() == won.size + 1 and ref["nbinned"][0] == N
    got = E.rows_profile2d(rows, T, nc, g=g, pairs=[(0, 1)], drops=DROPS)
    check(got, ref, "beyond 2^20 rows")
