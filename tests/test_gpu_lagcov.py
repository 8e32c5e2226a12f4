"""mcx_samples_lagcov on the GPU against tests/lagcov_ref.py on Metropolis-like rows (a chain's row repeats
the step before with probability 0.7) whose column 1 depends on column 0.

What is held:
  G(t)      every entry of every lag within lagcov_ref.bound of the float64 restatement: 4 (N + 16) 2^-53 sqrt(G(0)_ii G(0)_jj);
            exactly 0 where a column is constant; NaN exactly in the rows and columns of a column that is not finite; G(0)
            symmetric in its bits
  section 10   G(0) N / (N - 1) against rows_covariance within twice that bound (times N / (N - 1)); mean bit for bit the summary's
  integers  p, s, k_used, lags_used, the flags: exactly the reference's, on inputs the reference alone says are decisive (every
            log-determinant difference the walk compares above 1e-6 in absolute value, the pivots of Sigma_s within 1e6 of each other)
  floats    Sigma, mess, ess, mcse and the log-determinants within a relative 1e-9 of the reference walk on the RETURNED gamma
            (Sigma: of sqrt(Sigma_ii Sigma_jj)) -- that tests the host walk.  Against the reference's own gamma the G bound b is
            propagated: Sigma is -S(0) + 2 sum of lags_used matrices S(t), each entry of which errs by at most b_ij, so
            |d Sigma_ij| <= (2 lags_used + 1) b_ij =: e_ij (and |d Lambda_ij| <= b_ij N / (N - 1) =: f_ij); to first order
            d log det M = tr(M^-1 dM), so |d log det Sigma| <= sum_ij |Sigma^-1|_ij e_ij, doubled for the higher orders (the
            relative perturbation is below 1e-9), likewise Lambda; mess errs by the sum of the two over p, relatively; ess_j by
            f_jj / Lambda_jj + e_jj / Sigma_jj, mcse_j by half of e_jj / Sigma_jj
  bytes     two calls, the engine and rows_lagcov of its copied rows, and a derived store of them give the same bytes; the lags
            computed on demand give the bytes of a call that computes every lag
  units     more units than workgroups (BIG): a workgroup's second and third unit and the last unit's tail at the windows, the
            same at lag 0, with every tile pair of four tiles; the same bound (it grows with N), the reference on max_lag + 1
            lags only; a NaN in a row that only a second-round unit reads
The launch geometry is asserted before each result."""
import numpy as np
import pytest

import lagcov_ref as R
from test_gpu_store_view import run

pytestmark = pytest.mark.gpu

W, UNIT, WG_MAX = 8, 32, 512
CACHE = {}


def case(shape):
    """(rows, T, nc, the reference on every lag), made once"""
    if shape not in CACHE:
        np_, nc, T = shape
        rows = R.dependent_rows(np_, nc, T)
        CACHE[shape] = (rows, T, nc, R.restate(rows, T, nc))
    return CACHE[shape]


def lags_on_demand(T, L, ref, nlags_out=0):
    """the lags the schedule computes: 1 + W at first (nlags_out at least, also beyond the walk's last lag L), doubled up to L
    while the walk has not stopped"""
    stop_at = None if ref["flags"] & (R.TRUNCATED | R.NOT_PD) else 2 * ref["k_used"] + 4  # lags 0 .. 2 (k_used + 1) + 1
    Lc = max(L, nlags_out - 1)
    have = min(Lc + 1, max(nlags_out, 1 + W))
    have = 1 + -(-(have - 1) // W) * W if have < Lc + 1 else have  # (whole windows)
    have = min(have, Lc + 1)
    while have < L + 1 and (stop_at is None or have < stop_at):
        have = min(L + 1, 1 + 2 * (have - 1))
    return have


def check_geometry(np_, nc, T, nlags):
    from mcpar_amd import engine as E
    g = E.debug_lagcov_geometry(T, nc, np_, nlags)
    N, nt = T * nc, (np_ + 15) // 16
    units = -(-N // UNIT)
    assert (g["window_lags"], g["rows_per_iteration"], g["units"], g["workgroups"]) == (W, UNIT, units, min(units, max(32, WG_MAX // nt ** 2)))
    assert (g["tiles"], g["pairs_lag0"], g["pairs"]) == (nt, nt * (nt + 1) // 2, nt * nt)
    assert g["windows"] == -(-(nlags - 1) // W) and g["launches"] == 1 + g["windows"] and g["lags_computed"] >= nlags
    return g


def check_gamma(got, ref, N, where=""):
    g, r = got["gamma"], ref["gamma"][:got["gamma"].shape[0]]
    bad = (ref["col_flags"] & R.NONFINITE) != 0
    assert np.array_equal(got["col_flags"], ref["col_flags"]), (where, got["col_flags"], ref["col_flags"])
    assert np.isnan(g[:, bad, :]).all() and np.isnan(g[:, :, bad]).all() and np.isnan(got["mean"][bad]).all(), where
    k = np.flatnonzero(~bad)
    g, r = g[:, k][:, :, k], r[:, k][:, :, k]
    assert np.isfinite(g).all(), where
    b = R.bound(ref["gamma"][0][np.ix_(k, k)], N)
    err = np.abs(g - r)
    zero = np.broadcast_to(b == 0, g.shape)
    assert (g[zero] == 0).all(), (where, "entries of a constant column")
    ratio = float((err / np.where(b == 0, 1, b))[~zero].max()) if (~zero).any() else 0.0
    print("%s largest |G - ref| / bound over %d lags: %.3g" % (where, g.shape[0], ratio))
    assert ratio <= 1.0, (where, ratio)
    assert got["gamma"][0].tobytes() == np.ascontiguousarray(got["gamma"][0].T).tobytes(), (where, "G(0) is not symmetric in its bits")
    assert np.array_equal(got["ccf"], R.ccf_of(got["gamma"]), equal_nan=True)
    d = np.flatnonzero(np.diag(got["gamma"][0]) > 0)
    assert (got["ccf"][0, d, d] == 1.0).all()


def check_propagated(got, ref, N, where=""):
    """against the reference's own gamma (the module docstring states the propagation)"""
    idx = np.flatnonzero(~np.isnan(np.diag(ref["sigma"])))
    if idx.size == 0:
        return
    ix = np.ix_(idx, idx)
    b = R.bound(ref["gamma"][0], N)[ix]
    e, f = (2 * ref["lags_used"] + 1) * b, b * N / (N - 1)
    sig, lam = ref["sigma"][ix], ref["gamma"][0][ix] * N / (N - 1)
    assert (np.abs(got["sigma"][ix] - sig) <= e).all(), (where, "sigma")
    t_s, t_l = 2 * np.sum(np.abs(np.linalg.inv(sig)) * e), 2 * np.sum(np.abs(np.linalg.inv(lam)) * f)
    assert abs(got["logdet_sigma"] - ref["logdet_sigma"]) <= t_s and abs(got["logdet_lambda"] - ref["logdet_lambda"]) <= t_l, where
    assert abs(got["mess"] - ref["mess"]) <= 1.01 * ref["mess"] * (t_s + t_l) / idx.size, (where, "mess")
    re, rl = np.diag(e) / np.diag(sig), np.diag(f) / np.diag(lam)
    assert (np.abs(got["ess"][idx] - ref["ess"][idx]) <= 1.01 * ref["ess"][idx] * (re + rl)).all(), (where, "ess")
    assert (np.abs(got["mcse"][idx] - ref["mcse"][idx]) <= 1.01 * ref["mcse"][idx] * re / 2).all(), (where, "mcse")


def held(got, ref, rows, T, nc, with_ll=False, where=""):
    """a call that returned every lag it computed, held to the reference in every way above"""
    from mcpar_amd import engine as E
    N = T * nc
    assert R.decisive(ref), (where, ref["margins"], ref["pivot_ratio"])
    check_gamma(got, ref, N, where)
    R.check_finish(got, ref, rtol=1.0, where=where)  # (the integers and the flags; the floats follow, held more tightly)
    use = R.use_of(ref["col_flags"] & R.NONFINITE, with_ll)
    R.check_finish(got, R.finish(got["gamma"], N, use), rtol=1e-9, where=where + " walk on the returned gamma: ")
    check_propagated(got, ref, N, where)
    assert got["N"] == N and np.array_equal(got["mcse_cov"], got["sigma"] / N, equal_nan=True)
    # section 10 and section 9
    cov = E.rows_covariance(rows, T, nc)
    fin = np.flatnonzero(ref["col_flags"] & R.NONFINITE == 0)
    ix = np.ix_(fin, fin)
    assert (np.abs(got["gamma"][0][ix] * (N / (N - 1)) - cov["cov"][ix]) <= 2 * R.bound(ref["gamma"][0], N)[ix] * (N / (N - 1))).all(), where
    assert got["mean"][fin].tobytes() == cov["mean"][fin].tobytes() == E.rows_summary(rows, T, nc)["mean"][fin].tobytes(), where


def strip(d):
    """what does not depend on how many lags were asked for or computed"""
    return {k: v for k, v in d.items() if k not in ("gamma", "ccf", "lags_computed")}


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_shapes(shape):
    from mcpar_amd import engine as E
    np_, nc, T = shape
    rows, T, nc, ref = case(shape)
    assert ref["s"] == 0 and 0 <= ref["k_used"] <= 4
    g = check_geometry(np_, nc, T, T)
    if shape == (40, 8, 96):
        assert g["launches"] >= 2 and g["tiles"] == 3
    if shape == (3, 7, 5):
        assert g["units"] == 2 and T * nc == UNIT + 3  # tail rows and partners past the range in one unit
    if shape == (3, 5, 16):
        assert nc % 4 != 0  # B's row group straddles A's
    got = E.rows_lagcov(rows, T, nc, nlags=T)
    assert got["lags_computed"] == T == g["lags_computed"] and got["gamma"].shape == (T, np_ + 1, np_ + 1)
    held(got, ref, rows, T, nc, where=str(shape))
    # on demand: the lags the schedule says, the same numbers
    lazy = E.rows_lagcov(rows, T, nc)
    assert lazy["lags_computed"] == lags_on_demand(T, T - 1, ref), (lazy["lags_computed"], ref["k_used"])
    check_geometry(np_, nc, T, lazy["lags_computed"])
    assert R.same(strip(lazy), strip(got))
    if shape == (17, 37, 64):
        # the ordered pairs (0, 1) and (1, 0) differ: column 16 against the others, far beyond the bound
        r1, b = ref["gamma"][1], R.bound(ref["gamma"][0], T * nc)
        assert (np.abs(r1[16, :16] - r1[:16, 16]) > 1e6 * b[16, :16]).any() and abs(r1[0, 1] - r1[1, 0]) > 1e6 * b[0, 1]
        assert abs(got["mess"] / (T * nc) - 0.176) <= 0.05
        print("mess / N = %.4f" % (got["mess"] / (T * nc)))


def test_max_lag_and_some_lags_out():
    from mcpar_amd import engine as E
    rows, T, nc, _ = case((3, 5, 16))
    ref = R.restate(rows, T, nc, max_lag=3)
    got = E.rows_lagcov(rows, T, nc, max_lag=3, nlags=4)
    assert got["flags"] == E.MESS_TRUNCATED == ref["flags"] and got["lags_computed"] == 4 and got["k_used"] == 1
    held(got, ref, rows, T, nc, where="max_lag 3")
    # fewer lags out than the walk computes; more than its first window
    full = E.rows_lagcov(rows, T, nc, nlags=T)
    for nl in (1, 2, 11):
        part = E.rows_lagcov(rows, T, nc, nlags=nl)
        assert part["gamma"].tobytes() == full["gamma"][:nl].tobytes() and R.same(strip(part), strip(full))
        assert part["lags_computed"] == lags_on_demand(T, T - 1, R.restate(rows, T, nc), nl)
    with_ll = E.rows_lagcov(rows, T, nc, nlags=T, with_ll=True)
    assert with_ll["p"] == 4 and with_ll["gamma"].tobytes() == full["gamma"].tobytes()
    held(with_ll, R.restate(rows, T, nc, with_ll=True), rows, T, nc, with_ll=True, where="with log L")


@pytest.mark.parametrize("max_lag,nl", [(3, 10), (3, 64), (9, 30)])
def test_more_lags_out_than_the_walk_may_see(max_lag, nl):
    """nlags > max_lag + 1: the lags asked for are swept and returned, the walk stops at max_lag"""
    from mcpar_amd import engine as E
    rows, T, nc, full_ref = case((17, 37, 64))
    N = T * nc
    ref = R.restate(rows, T, nc, max_lag=max_lag)
    assert R.decisive(ref) and ref["flags"] == R.TRUNCATED and ref["k_used"] == (max_lag - 1) // 2
    want_lags = lags_on_demand(T, max_lag, ref, nl)
    assert nl <= want_lags <= T and check_geometry(17, nc, T, want_lags)["lags_computed"] >= want_lags
    got = E.rows_lagcov(rows, T, nc, max_lag=max_lag, nlags=nl)
    assert got["gamma"].shape[0] == nl and got["lags_computed"] == want_lags
    check_gamma(got, dict(ref, gamma=full_ref["gamma"]), N, "max_lag %d, %d lags out" % (max_lag, nl))
    R.check_finish(got, ref, rtol=1.0)  # (the integers and the flags)
    use = R.use_of(ref["col_flags"] & R.NONFINITE, False)
    R.check_finish(got, R.finish(got["gamma"][:max_lag + 1], N, use), rtol=1e-9, where="walk on the returned gamma: ")
    check_propagated(got, ref, N)
    # the bytes of the call that computes every lag, and of the call that returns max_lag + 1 of them
    assert got["gamma"].tobytes() == E.rows_lagcov(rows, T, nc, nlags=T)["gamma"][:nl].tobytes()
    assert R.same(strip(got), strip(E.rows_lagcov(rows, T, nc, max_lag=max_lag, nlags=max_lag + 1)))


def test_no_column_chosen_stops_at_the_first_window():
    from mcpar_amd import engine as E
    rows, T, nc, _ = case((3, 5, 16))
    rows = rows.copy()
    rows[3, 0] = np.inf
    rows[:, 1] = np.float32(0.75)
    rows[40, 2] = np.nan
    got = E.rows_lagcov(rows, T, nc)
    assert got["p"] == 0 and got["flags"] == E.MESS_NOT_PD and (got["s"], got["k_used"], got["lags_used"]) == (-1, -1, 0)
    assert got["lags_computed"] == 1 + W and got["col_flags"].tolist() == [1, 2, 1, 0] and np.isnan(got["sigma"]).all()
    R.check_finish(got, R.restate(rows, T, nc))


def test_nonfinite_and_constant_columns():
    from mcpar_amd import engine as E
    np_, nc, T = 17, 37, 64
    rows = case((np_, nc, T))[0].copy()
    rows[1234, 3] = np.nan
    rows[77, np_] = -np.inf
    rows[:, 16] = np.float32(-2.5)
    ref = R.restate(rows, T, nc, with_ll=True)
    assert ref["col_flags"].tolist() == [0, 0, 0, 1] + [0] * 12 + [2, 1] and ref["p"] == 15
    got = E.rows_lagcov(rows, T, nc, nlags=T, with_ll=True)
    held(got, ref, rows, T, nc, with_ll=True, where="planted")
    assert got["p"] == 15 and np.isnan(got["ess"][[3, 16, 17]]).all() and np.isnan(got["sigma"][[3, 16, 17]]).all()
    assert (got["gamma"][:, 16, :3] == 0).all() and (got["gamma"][:, :3, 16] == 0).all() and np.isnan(got["ccf"][:, 16, :]).all()
    # every other entry is what it is without those columns
    keep = [c for c in range(np_ + 1) if c not in (3, 16, 17)]
    clean = E.rows_lagcov(case((np_, nc, T))[0], T, nc, nlags=T)
    assert got["gamma"][:, keep][:, :, keep].tobytes() == clean["gamma"][:, keep][:, :, keep].tobytes()


def test_the_three_owners_and_a_second_call_give_the_same_bytes():
    from mcpar_amd import engine as E
    eg = run(37, 17, 30)
    first, nsteps = 3, 24
    rows = eg.samples_range(first, nsteps)
    on_engine = eg.lagcov(nlags=nsteps, first_step=first, nsteps=nsteps)
    ref = R.restate(rows, nsteps, eg.nc)
    check_gamma(on_engine, ref, nsteps * eg.nc, "engine sub-range")
    use = R.use_of(ref["col_flags"] & R.NONFINITE, False)
    R.check_finish(on_engine, R.finish(on_engine["gamma"], nsteps * eg.nc, use), rtol=1e-9, where="engine sub-range: ")
    assert R.same(eg.lagcov(nlags=nsteps, first_step=first, nsteps=nsteps), on_engine)
    assert R.same(E.rows_lagcov(rows, nsteps, eg.nc, nlags=nsteps), on_engine)
    st = E.select_chains_rows(rows, nsteps, eg.nc, list(range(eg.nc)))
    assert R.same(st.lagcov(nlags=nsteps), on_engine) and R.same(st.lagcov(nlags=nsteps), on_engine)
    st.close()
    whole = eg.lagcov(nlags=5)
    assert whole["N"] == 30 * eg.nc and R.same(E.rows_lagcov(eg.samples, 30, eg.nc, nlags=5), whole)
    ms, lags = eg.lagcov_times(first_step=first, nsteps=nsteps)
    assert ms.shape == (5,) and (ms >= 0).all() and ms[4] >= ms[:4].sum() * 0.99 > 0 and 2 <= lags <= nsteps
    eg.close()


# ---- more units than workgroups: the loop of k_lagcov, unit += workgroups, at the windows and at lag 0 ---------------------------
# shape -> (lags computed, units, workgroups, units of lag 0, workgroups of lag 0)
BIG = {(3, 37, 887): (17, 1026, 512, 257, 257),     # workgroups 0 and 1 take three units, the last unit has 19 rows; lag 0 below its cap
       (3, 7, 74917): (9, 16389, 512, 4098, 2048),  # lag 0: workgroups 0 and 1 take three units
       (49, 7, 4701): (17, 1029, 32, 258, 128)}     # four tiles: 16 pairs at the windows, 10 at lag 0, the off-diagonal launches


def big_case(shape, with_ll=False):
    """(rows, the reference on the lags the call computes), made once"""
    np_, nc, T = shape
    if ("rows", shape) not in CACHE:
        CACHE["rows", shape] = R.dependent_rows(np_, nc, T)
    rows = CACHE["rows", shape]
    if (shape, with_ll) not in CACHE:
        CACHE[shape, with_ll] = R.restate(rows, T, nc, max_lag=BIG[shape][0] - 1, with_ll=with_ll)
    return rows, CACHE[shape, with_ll]


def check_big_geometry(shape):
    np_, nc, T = shape
    nl, units, wgs, units0, wgs0 = BIG[shape]
    g = check_geometry(np_, nc, T, nl)
    nt, N = (np_ + 15) // 16, T * nc
    assert (g["units"], g["workgroups"], g["units_lag0"], g["workgroups_lag0"]) == (units, wgs, units0, wgs0)
    assert g["units_lag0"] == -(-N // (4 * UNIT)) and g["workgroups_lag0"] == min(units0, 4 * max(32, WG_MAX // nt ** 2))
    assert g["lags_computed"] == nl and g["launches"] == 1 + -(-(nl - 1) // W)
    return g


@pytest.mark.parametrize("shape", sorted(BIG), ids=str)
def test_more_units_than_workgroups(shape):
    from mcpar_amd import engine as E
    np_, nc, T = shape
    nl = BIG[shape][0]
    g = check_big_geometry(shape)
    if shape == (3, 37, 887):
        assert g["units"] == 2 * g["workgroups"] + 2 and T * nc - (g["units"] - 1) * UNIT == 19 and g["units_lag0"] == g["workgroups_lag0"]
    if shape == (3, 7, 74917):
        assert g["units_lag0"] == 2 * g["workgroups_lag0"] + 2 and g["units"] > 2 * g["workgroups"]
    if shape == (49, 7, 4701):
        assert (g["tiles"], g["pairs"], g["pairs_lag0"]) == (4, 16, 10) and g["units"] > 32 * g["workgroups"]
        assert g["units_lag0"] == 2 * g["workgroups_lag0"] + 2
    for with_ll in ((False, True) if shape == (49, 7, 4701) else (False,)):
        rows, ref = big_case(shape, with_ll)
        assert ref["flags"] == R.TRUNCATED and ref["s"] == 0 and ref["k_used"] == (nl - 2) // 2
        got = E.rows_lagcov(rows, T, nc, max_lag=nl - 1, nlags=nl, with_ll=with_ll)
        assert got["lags_computed"] == nl and got["gamma"].shape == (nl, np_ + 1, np_ + 1) and got["p"] == np_ + with_ll
        held(got, ref, rows, T, nc, with_ll=with_ll, where="%s%s" % (shape, " with log L" if with_ll else ""))


def test_a_nan_in_a_second_round_unit():
    """row 20000 of the first BIG shape lies in unit 625 = 512 + 113, and every unit that reads it as a partner (rows from 20000 -
    16 * 37 on) is a second-round unit too; at lag 0 every unit is a first unit"""
    from mcpar_amd import engine as E
    shape = (3, 37, 887)
    np_, nc, T = shape
    nl = BIG[shape][0]
    g = check_big_geometry(shape)
    row, col = 20000, 1
    first_reader, last_reader = (row - (nl - 1) * nc) // UNIT, row // UNIT
    assert g["workgroups"] <= first_reader and last_reader < 2 * g["workgroups"] and g["units_lag0"] == g["workgroups_lag0"]
    rows, _ = big_case(shape)
    clean = E.rows_lagcov(rows, T, nc, max_lag=nl - 1, nlags=nl)
    bad = rows.copy()
    bad[row, col] = np.nan
    got = E.rows_lagcov(bad, T, nc, max_lag=nl - 1, nlags=nl)
    assert got["col_flags"].tolist() == [0, R.NONFINITE, 0, 0] and got["p"] == 2
    assert np.isnan(got["gamma"][:, col, :]).all() and np.isnan(got["gamma"][:, :, col]).all() and np.isnan(got["mean"][col])
    keep = [0, 2, 3]
    assert np.isfinite(got["gamma"][:, keep][:, :, keep]).all()
    assert got["gamma"][:, keep][:, :, keep].tobytes() == clean["gamma"][:, keep][:, :, keep].tobytes()
    assert got["mean"][keep].tobytes() == clean["mean"][keep].tobytes()
    check_gamma(got, R.restate(bad, T, nc, max_lag=nl - 1), T * nc, "a NaN in unit %d" % last_reader)


def test_the_three_owners_give_the_same_bytes_beyond_one_unit_per_workgroup():
    from mcpar_amd import engine as E
    shape = (3, 37, 887)
    np_, nc, T = shape
    nl = BIG[shape][0]
    check_big_geometry(shape)
    first = 3
    eg = run(nc, np_, first + T)
    rows = eg.samples_range(first, T)
    on_engine = eg.lagcov(max_lag=nl - 1, nlags=nl, first_step=first, nsteps=T)
    ref = R.restate(rows, T, nc, max_lag=nl - 1)
    check_gamma(on_engine, ref, T * nc, "engine sub-range, %s" % (shape,))
    use = R.use_of(ref["col_flags"] & R.NONFINITE, False)
    R.check_finish(on_engine, R.finish(on_engine["gamma"], T * nc, use), rtol=1e-9, where="engine sub-range: ")
    assert R.same(E.rows_lagcov(rows, T, nc, max_lag=nl - 1, nlags=nl), on_engine)
    st = E.select_chains_rows(rows, T, nc, list(range(nc)))
    assert R.same(st.lagcov(max_lag=nl - 1, nlags=nl), on_engine)
    st.close()
    eg.close()
