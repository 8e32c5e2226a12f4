"""Importance weights on a store on the GPU against tests/reweight_ref.py.

Every case first asserts its launch geometry, then holds mcx_debug_reweight_q to within one unit of the float64 restatement of
q (the argument of exp is the same IEEE double on both sides and a 1-ulp exp moves 2^31 exp by at most 2^-21, so only the
rounding can differ) and prints the count of rows that differ; everything else is held to the restatement fed with the
library's own q:
  exactly     n, nzero, sumq, both words of sumq2, tail_m, the flags, min, max and every quantile bit for bit (by key, so that
              any NaN is one value), every resample index and every resampled row
  mean        1e-10 of sum q |x| / Q: the fixed-order bound N 2^-53 with N <= 2^17 in these cases (2^18 in the k-hat anchor,
              whose columns are not what it is about), as in section 20's argument
  sd, mcse    1e-9 relative, plus the mean's bound (an error d of the mean moves either by at most d)
  ess_kish, log_mean_w   1e-14 relative;  khat, tail_sigma   1e-9
The two BIG cases cross what the others do not reach: k_rw_scan lanes that own three and nine tiles and lanes that own none,
k_rw_maxred beyond 256 tiles, a second histogram step chunk, the sort of q beyond 256 sort tiles and k_rw_draw's search over such
an offset table.  They keep the rules above (the mean's 1e-10 too, which is now below N 2^-53 = 2.3e-10 and so asks more)."""
import math

import numpy as np
import pytest

import reweight_ref as R
from test_gpu_store_view import run

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
PROBS = (0.05, 0.5, 0.95)
RS = 1024  # the scan tile; every case asserts it through the geometry entry


def make_rows(nc, np_, T, seed=11):
    """normal rows with ties in column 0 (one decimal, a -0 among them) and log L below zero"""
    rng = np.random.default_rng([seed, nc, np_, T])
    a = rng.normal(0.0, 1.0, (T * nc, np_ + 1)).astype(np.float32)
    a[:, 0] = np.round(a[:, 0], 1)
    a[0, 0] = np.float32(-0.0)
    a[:, -1] = -np.abs(a[:, -1]) * np.float32(3.0) - np.float32(1e-3)
    return a


def spread_logw(N, seed=5):
    """log-weights over some twenty e-folds, with ties"""
    lw = np.random.default_rng([seed, N]).normal(0.0, 3.0, N).astype(np.float32)
    lw[::7] = np.float32(0.25)
    return lw


def same_keys(a, b):
    return np.array_equal(R.okey(np.asarray(a, np.float32)), R.okey(np.asarray(b, np.float32)))


def same_dict(a, b):
    """two results of the library: every byte but the NaN payloads"""
    def flat(d):
        out = {}
        for k, v in d.items():
            if isinstance(v, dict):
                out.update({k + "." + kk: np.asarray(vv) for kk, vv in v.items()})
            else:
                out[k] = np.asarray(v)
        return out
    fa, fb = flat(a), flat(b)
    assert sorted(fa) == sorted(fb)
    for k in fa:
        x, y = fa[k], fb[k]
        assert x.dtype == y.dtype and x.shape == y.shape, k
        if x.dtype.kind == "f":
            assert np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(x[~np.isnan(x)], y[~np.isnan(y)]), (k, x, y)
        else:
            assert np.array_equal(x, y), (k, x, y)


def held(got, ref, what=""):
    """a result of the library against the restatement fed with the library's q"""
    for k in ("n", "nzero", "sumq", "sumq2_hi", "sumq2_lo", "sumq2", "tail_m", "flags"):
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    assert got["lwmax"] == ref["lwmax"], what
    assert abs(got["ess_kish"] - ref["ess_kish"]) <= 1e-14 * ref["ess_kish"], (what, got["ess_kish"], ref["ess_kish"])
    assert abs(got["log_mean_w"] - ref["log_mean_w"]) <= 1e-14 * abs(ref["log_mean_w"]), (what, got["log_mean_w"], ref["log_mean_w"])
    for k in ("khat", "tail_sigma"):
        if math.isnan(ref[k]):
            assert math.isnan(got[k]), (what, k)
        else:
            assert abs(got[k] - ref[k]) <= 1e-9 * max(1.0, abs(ref[k])), (what, k, got[k], ref[k])
    gc, rc = got["cols"], ref["cols"]
    assert np.array_equal(gc["flags"], rc["flags"]), (what, gc["flags"], rc["flags"])
    assert same_keys(gc["min"], rc["min"]) and same_keys(gc["max"], rc["max"]), (what, gc["min"], rc["min"], gc["max"], rc["max"])
    assert got["quantiles"].shape == ref["quantiles"].shape
    assert same_keys(got["quantiles"], ref["quantiles"]), (what, got["quantiles"], ref["quantiles"])
    for c in range(len(rc["flags"])):
        if rc["flags"][c]:
            assert all(math.isnan(gc[k][c]) for k in ("mean", "sd", "mcse_mean")), (what, c)
            continue
        floor = 1e-10 * rc["scale"][c]
        assert abs(gc["mean"][c] - rc["mean"][c]) <= floor, (what, c, gc["mean"][c], rc["mean"][c])
        for k in ("sd", "mcse_mean"):
            assert abs(gc[k][c] - rc[k][c]) <= 1e-9 * rc[k][c] + floor, (what, c, k, gc[k][c], rc[k][c])


def held_q(weights, rows, T, nc, lw, what=""):
    """the library's q and lwmax against the float64 restatement of lw -> q"""
    from mcpar_amd import engine as E
    q, lwmax = E.debug_reweight_q(weights, rows, T, nc)
    want, wmax = R.fixed_point(lw)
    diff = np.abs(q.astype(np.int64) - want.astype(np.int64))
    print("%s: %d of %d rows of q differ from the restatement (by at most %d)" % (what, int((diff > 0).sum()), len(q), int(diff.max())))
    assert lwmax == wmax and diff.max() <= 1, (what, lwmax, wmax, int(diff.max()))
    assert q.max() == 2 ** 31
    return q, lwmax


def resample_held(weights, rows, T, nc, q, K, seed, what=""):
    """a resample of K = 1 x K draws: every index and every row"""
    from mcpar_amd import engine as E
    st, index = E.resample_rows(rows, T, nc, weights, 1, K, seed, with_index=True)
    want, u = R.resample_index(q, seed, K)
    assert st.shape == (1, K, rows.shape[1]) and np.array_equal(index, want), (what, index[:8], want[:8])
    assert np.all(q[index] > 0)
    assert np.all(np.diff(index[np.argsort(u, kind="stable")]) >= 0)  # non-decreasing in u
    got = st.rows()
    st.close()
    assert got.view(np.uint32).tobytes() == rows[index].view(np.uint32).tobytes(), what
    return index


def case(rows, T, nc, weights, lw, probs=PROBS, tiles=None, K=300, what=""):
    from mcpar_amd import engine as E
    N, ncol = rows.shape
    g = E.debug_reweight_geometry(N, ncol, len(probs), K)
    assert g["scan_tile_rows"] == RS and g["scan_tiles"] == (N + RS - 1) // RS and g["draw_workgroups"] == (K + 255) // 256
    if tiles is not None:
        assert g["scan_tiles"] == tiles
    q, lwmax = held_q(weights, rows, T, nc, lw, what)
    got = E.reweight_rows(rows, T, nc, weights, probs)
    held(got, R.restate(rows, q, lwmax, probs), what)
    if K:
        resample_held(weights, rows, T, nc, q, K, 20240611, what)
    return got, q


# ---- shapes ---------------------------------------------------------------------------------------------------------------------
# (nc, np, T): a parameter tile plus a second tile of one column and a ragged chain group; the log L tile crossing 256 chains;
# one row; exact tiles; two scan tiles exactly, and five rows into a third
@pytest.mark.parametrize("nc, np_, T, tiles", [(37, 17, 12, 1), (300, 3, 5, 2), (1, 1, 1, 1), (16, 16, 8, 1), (64, 2, 32, 2), (2053, 2, 1, 3)])
def test_shapes(nc, np_, T, tiles):
    from mcpar_amd import engine as E
    rows = make_rows(nc, np_, T)
    logw = spread_logw(T * nc)
    got, q = case(rows, T, nc, E.weights_host(logw), R.log_weights(logw, 1.0), tiles=tiles, what="%dx%dx%d" % (nc, np_, T))
    if T * nc == 1:
        assert got["flags"] == R.NO_TAIL and got["sumq"] == 2 ** 31 and got["cols"]["sd"][0] == 0.0
        assert got["cols"]["mean"][0] == float(rows[0, 0])


# ---- equal weights --------------------------------------------------------------------------------------------------------------
def test_equal_weights():
    from mcpar_amd import engine as E
    nc, np_, T = 37, 17, 12
    rows = make_rows(nc, np_, T)
    N = T * nc
    w = E.weights_loglike(0.0)
    got, q = case(rows, T, nc, w, R.log_weights(rows[:, -1], 0.0), probs=(0.0, 0.05, 0.31, 0.5, 0.95, 1.0), K=0, what="equal")
    assert N == 444 and np.all(q == 2 ** 31) and got["sumq"] == 444 << 31
    assert got["sumq2"] == 444 << 62 and got["sumq2_hi"] == 111 and got["sumq2_lo"] == 0  # the carry into the high word
    assert got["ess_kish"] == 444.0 and got["log_mean_w"] == 0.0 and got["nzero"] == 0
    assert got["tail_m"] == 64 and got["flags"] == R.NO_TAIL and math.isnan(got["khat"])
    for c in range(np_ + 1):
        want = np.quantile(rows[:, c], (0.0, 0.05, 0.31, 0.5, 0.95, 1.0), method="inverted_cdf")
        assert same_keys(got["quantiles"][c], want), c
        x = rows[:, c].astype(np.float64)
        assert abs(got["cols"]["mean"][c] - x.mean()) <= 1e-10 * np.abs(x).mean()
        assert abs(got["cols"]["sd"][c] - x.std(ddof=0)) <= 1e-9 * x.std(ddof=0)
    # the nested floors agree: the indices are the unweighted draw's of the same seed
    K, seed = 700, 99
    st, index = E.resample_rows(rows, T, nc, w, 7, 100, seed, with_index=True)
    plain = E.select_chains_rows(rows, T, nc, list(range(nc)))
    drawn_rows, drawn = plain.draw(K, seed)
    assert np.array_equal(index, drawn) and np.array_equal(index, E.debug_draw_indices(seed, N, 0, K))
    assert st.shape == (7, 100, np_ + 1) and st.rows().tobytes() == drawn_rows.tobytes()
    st.close()
    plain.close()


def test_three_rows_of_full_weight_in_one_bin():
    """three equal values of full weight in one workgroup: the bin holds 3 * 2^31 > 2^32"""
    from mcpar_amd import engine as E
    rows = np.array([[1, -1], [1, -2], [1, -3], [2, -4], [3, -5], [4, -6], [5, -7], [6, -8]], np.float32)
    logw = np.array([0, 0, 0, -1, -1, -1, -1, -1], np.float32)
    probs = (0.0, 0.3, 0.5, 0.55, 0.69, 1.0)
    got, q = case(rows, 1, 8, E.weights_host(logw), R.log_weights(logw, 1.0), probs=probs, K=40, what="full weight")
    assert list(q[:3]) == [2 ** 31] * 3 and 3 * 2 ** 31 > 2 ** 32
    share = 3 * 2 ** 31 / got["sumq"]  # of the value 1
    assert 0.55 < share < 0.69 and list(got["quantiles"][0]) == [1.0, 1.0, 1.0, 1.0, 2.0, 6.0]


def test_forty_probabilities_on_a_wide_column():
    """a column over sixty orders of magnitude and both signs: more than 32 distinct prefixes from the second pass on, three
    launches of RW_GMAX = 16 prefixes each"""
    from mcpar_amd import engine as E
    nc, np_, T = 50, 2, 40
    rows = make_rows(nc, np_, T)
    rng = np.random.default_rng(3)
    rows[:, 1] = (np.sign(rng.normal(size=T * nc)) * 10.0 ** rng.uniform(-30.0, 30.0, T * nc)).astype(np.float32)
    probs = tuple(np.linspace(0.01, 0.99, 40))
    g = E.debug_reweight_geometry(T * nc, np_ + 1, 40)
    assert g["hist_targets"] == 42 and g["hist_prefixes"] == 16 and g["hist_launches"] == 3 and g["hist_tile_cols"] == 1
    logw = spread_logw(T * nc) * np.float32(0.1)  # mild weights: the forty quantiles are forty values
    got, _ = case(rows, T, nc, E.weights_host(logw), R.log_weights(logw, 1.0), probs=probs, K=0, what="40 probs")
    keys = R.okey(got["quantiles"][1].astype(np.float32))
    assert len(set(keys >> 24)) > 32  # three launches of 16 prefixes from the second pass on


# ---- zero weights ---------------------------------------------------------------------------------------------------------------
def test_zero_weights():
    from mcpar_amd import engine as E
    nc, np_, T = 64, 2, 48  # three scan tiles
    rows = make_rows(nc, np_, T)
    N = T * nc
    logw = np.minimum(spread_logw(N), np.float32(8.0))
    logw[0] = 8.0  # the largest, in the first tile
    logw[5:RS:9] = -INF
    logw[3:RS:11] = np.float32(8.0 + math.log(2.0 ** -33))  # below 2^-32 of the largest weight
    logw[RS:2 * RS] = -INF                                          # a whole tile of zeros between two weighted ones
    # column 1 of the q = 0 rows holds what must never be multiplied in
    rows[5:RS:9, 1] = INF
    rows[RS:2 * RS:3, 1] = NAN
    rows[RS + 1:2 * RS:3, 1] = -INF
    got, q = case(rows, T, nc, E.weights_host(logw), R.log_weights(logw, 1.0), tiles=3, K=2000, what="zeros")
    assert not q[RS:2 * RS].any() and not q[5:RS:9].any() and not q[3:RS:11].any() and got["nzero"] >= RS + 170
    assert not got["cols"]["flags"].any() and np.all(np.isfinite(got["cols"]["mean"])) and np.all(np.isfinite(got["cols"]["sd"]))
    assert np.all(np.isfinite(got["quantiles"]))


def test_all_weight_on_two_rows_across_a_tile_edge():
    from mcpar_amd import engine as E
    nc, np_, T = 64, 2, 48
    rows = make_rows(nc, np_, T)
    logw = np.full(T * nc, -INF, np.float32)
    logw[RS - 1], logw[RS] = 0.0, math.log(0.5)
    got, q = case(rows, T, nc, E.weights_host(logw), R.log_weights(logw, 1.0), tiles=3, K=0, what="two rows")
    assert got["nzero"] == T * nc - 2 and got["sumq"] == 2 ** 31 + int(q[RS]) and abs(int(q[RS]) - 2 ** 30) < 64
    index = resample_held(E.weights_host(logw), rows, T, nc, q, 600, 4, "two rows")
    counts = np.bincount(index, minlength=T * nc)
    assert counts[RS - 1] + counts[RS] == 600 and counts[RS - 1] > counts[RS] > 100
    lo = min(rows[RS - 1, 0], rows[RS, 0])
    assert got["cols"]["min"][0] == lo and got["quantiles"][0][0] == lo


# ---- non-finite values ----------------------------------------------------------------------------------------------------------
def test_non_finite_values_on_weighted_rows():
    from mcpar_amd import engine as E
    nc, np_, T = 37, 4, 12
    rows = make_rows(nc, np_, T)
    logw = spread_logw(T * nc)
    logw[[40, 80, 120, 160]] = 0.0
    rows[40, 0], rows[80, 1], rows[120, 2] = INF, -INF, NAN
    rows[160, 3], rows[161, 3] = INF, -INF
    probs = (0.0, 0.5, 1.0)
    got, q = case(rows, T, nc, E.weights_host(logw), R.log_weights(logw, 1.0), probs=probs, K=0, what="non-finite")
    assert np.all(q[[40, 80, 120, 160]] > 0) and q[161] > 0
    assert list(got["cols"]["flags"]) == [1, 1, 1, 1, 0]
    assert got["cols"]["max"][0] == INF and got["cols"]["min"][1] == -INF and math.isnan(got["cols"]["max"][2])
    assert got["quantiles"][0][2] == INF and got["quantiles"][1][0] == -INF and math.isnan(got["quantiles"][2][2])
    assert np.all(np.isfinite(got["quantiles"][:, 1])) and math.isfinite(got["cols"]["mean"][4])
    # the same values on rows without weight: no flag, finite moments
    logw[[40, 80, 120, 160, 161]] = -INF
    got, q = case(rows, T, nc, E.weights_host(logw), R.log_weights(logw, 1.0), probs=probs, K=0, what="non-finite, q = 0")
    assert not q[[40, 80, 120, 160, 161]].any() and not got["cols"]["flags"].any()
    assert np.all(np.isfinite(got["cols"]["mean"])) and np.all(np.isfinite(got["quantiles"]))


# ---- refused weight sources -----------------------------------------------------------------------------------------------------
def test_refused_weight_sources():
    from mcpar_amd import McxError
    from mcpar_amd import engine as E
    nc, np_, T = 64, 2, 48
    rows = make_rows(nc, np_, T)
    N = T * nc

    def refused(logw, text, scale=1.0):
        w = E.Weights(E.WEIGHT_HOST, logw=logw, scale=scale)
        for call in (lambda: E.reweight_rows(rows, T, nc, w), lambda: E.resample_rows(rows, T, nc, w, 1, 10, 1),
                     lambda: E.debug_reweight_q(w, rows, T, nc)):
            with pytest.raises(McxError) as ei:
                call()
            assert ei.value.code == 1 and text in str(ei.value), str(ei.value)

    logw = spread_logw(N)
    bad = logw.copy()
    bad[[2500, 700, 1030]] = NAN
    refused(bad, "row 700 ")
    bad = logw.copy()
    bad[[3071, 2049]] = INF
    refused(bad, "row 2049 ")
    bad = logw.copy()
    bad[5], bad[4] = INF, NAN
    refused(bad, "row 4 ")
    bad = logw.copy()
    bad[N - 1] = -INF
    refused(bad, "row %d " % (N - 1), scale=-1.0)  # scale * -inf = +inf
    refused(bad, "row %d " % (N - 1), scale=0.0)   # 0 * -inf is NaN
    refused(np.full(N, -INF, np.float32), "of every row is -inf")


# ---- the three kinds and the three forms ----------------------------------------------------------------------------------------
TEMPER = """
__device__ void mcx_user_derive(const float *x, int d, float ly, const float *par, float *out, int nout)
{
  out[0] = par[0] * ly;
}
"""


@pytest.fixture(scope="module")
def engine():
    eg = run(37, 17, 30)
    yield eg
    eg.close()


def test_kinds_and_forms_agree(engine):
    from mcpar_amd import McxError
    from mcpar_amd import engine as E
    first, n, nc = 3, 24, 37
    rows = engine.samples_range(first, n)
    beta = 0.5  # (beta - 1) ly is exact in float: the derived column holds the float of the same double
    ll = E.weights_loglike(beta - 1.0)
    a = engine.reweight(ll, PROBS, first_step=first, nsteps=n)
    q, lwmax = held_q(ll, rows, n, nc, R.log_weights(rows[:, -1], beta - 1.0), "engine range")
    held(a, R.restate(rows, q, lwmax, PROBS), "engine range")
    same_dict(a, engine.reweight(ll, PROBS, first_step=first, nsteps=n))  # two calls
    same_dict(a, E.reweight_rows(rows, n, nc, ll, PROBS))
    same_dict(a, E.reweight_rows(rows, n, nc, E.weights_host((beta - 1.0) * rows[:, -1]), PROBS))
    st = engine.select_chains(list(range(nc)), first_step=first, nsteps=n)
    same_dict(a, st.reweight(ll, PROBS))
    derived = engine.derive(E.derive_source(TEMPER, 1, [beta - 1.0]), first_step=first, nsteps=n)
    assert derived.shape == (n, nc, 2) and derived.rows()[:, 0].tobytes() == ((np.float32(beta - 1.0)) * rows[:, -1]).tobytes()
    for w in (E.weights_column(derived, 0), E.weights_column(derived, 1, beta - 1.0)):  # its own column, and its log L column
        same_dict(a, engine.reweight(w, PROBS, first_step=first, nsteps=n))
        same_dict(a, st.reweight(w, PROBS))
        same_dict(a, E.reweight_rows(rows, n, nc, w, PROBS))
    qs, _ = E.debug_reweight_q(E.weights_column(derived, 0), store=st)
    assert np.array_equal(qs, q)
    # the resample in its three forms, with and without the indices
    want, _ = R.resample_index(q, 8, 500)
    outs = [engine.resample(ll, 5, 100, 8, with_index=True, first_step=first, nsteps=n), st.resample(ll, 5, 100, 8, with_index=True),
            E.resample_rows(rows, n, nc, E.weights_column(derived, 0), 5, 100, 8, with_index=True),
            (engine.resample(E.weights_column(derived, 1, beta - 1.0), 5, 100, 8, first_step=first, nsteps=n), want)]
    for o, index in outs:
        assert o.shape == (5, 100, 18) and np.array_equal(index, want)
        assert o.rows().tobytes() == rows[want].tobytes()
        o.close()
    # a weight store of another shape, a column outside it
    other = engine.select_chains(list(range(nc)), first_step=first, nsteps=n - 1)
    for call in (lambda: engine.reweight(E.weights_column(other, 0), PROBS, first_step=first, nsteps=n),
                 lambda: st.reweight(E.weights_column(other, 0)), lambda: st.resample(E.weights_column(other, 0), 1, 5, 1),
                 lambda: E.reweight_rows(rows, n, nc, E.weights_column(other, 0)),
                 lambda: st.reweight(E.weights_column(derived, 2)), lambda: st.reweight(E.weights_column(derived, -1)),
                 lambda: engine.reweight(ll, PROBS, first_step=first, nsteps=n + 4)):
        with pytest.raises(McxError) as ei:
            call()
        assert ei.value.code == 1
    for s in (st, derived, other):
        s.close()


def test_negative_scale(engine):
    from mcpar_amd import engine as E
    rows = engine.samples_range(0, 30)
    w = E.weights_loglike(-0.75)
    q, lwmax = held_q(w, rows, 30, 37, R.log_weights(rows[:, -1], -0.75), "negative scale")
    got = engine.reweight(w, PROBS)
    held(got, R.restate(rows, q, lwmax, PROBS), "negative scale")
    assert lwmax == -0.75 * float(rows[:, -1].min()) and q[int(np.argmin(rows[:, -1]))] == 2 ** 31


# ---- statistical anchors --------------------------------------------------------------------------------------------------------
def anchor_rows(N=40000, seed=1):
    """x ~ N(0, 1) with log L = -x^2 / 2: under MCX_WEIGHT_LL with scale 1 the target is N(0, 1/2)"""
    x = np.random.default_rng(seed).standard_normal(N)
    rows = np.empty((N, 2), np.float32)
    rows[:, 0] = x
    rows[:, 1] = -0.5 * rows[:, 0].astype(np.float64) ** 2
    return rows


def test_anchor_a_narrower_normal():
    from mcpar_amd import engine as E
    rows, T, nc = anchor_rows(), 200, 200
    w = E.weights_loglike(1.0)
    # the inputs, by the restatement alone
    q0, m0 = R.fixed_point(R.log_weights(rows[:, 1], 1.0))
    r0 = R.restate(rows, q0, m0, PROBS)
    for r in (r0, case(rows, T, nc, w, R.log_weights(rows[:, 1], 1.0), K=0, what="anchor")[0]):
        sd, mean, ess = r["cols"]["sd"][0], r["cols"]["mean"][0], r["ess_kish"]
        print("anchor: sd = %.4f sqrt(1/2), mean = %.4f, ess_kish = %.0f, khat = %.3f" % (sd / math.sqrt(0.5), mean, ess, r["khat"]))
        assert abs(sd / math.sqrt(0.5) - 1.0) < 0.03 and abs(mean) < 0.03 and 30000 < ess < 40000
        assert abs(r["log_mean_w"] - math.log(math.sqrt(0.5))) < 0.01  # the ratio of the normalising constants: sqrt(pi) / sqrt(2 pi)


@pytest.mark.parametrize("s, high", [(1.2, False), (1.5, False), (2.5, True)])
def test_anchor_khat_of_a_wider_normal(s, high):
    """rows from N(0, 1) weighted to N(0, s^2): the weights' tail index is 1 - 1 / s^2"""
    from mcpar_amd import engine as E
    N, T, nc = 200000, 400, 500
    rows = anchor_rows(N, seed=2)
    x = rows[:, 0].astype(np.float64)
    logw = (x * x / 2.0 - x * x / (2.0 * s * s)).astype(np.float32)
    got, _ = case(rows, T, nc, E.weights_host(logw), R.log_weights(logw, 1.0), K=0, what="s = %g" % s)
    print("s = %g: khat = %.3f against 1 - 1/s^2 = %.3f, ess_kish = %.0f" % (s, got["khat"], 1.0 - 1.0 / (s * s), got["ess_kish"]))
    assert got["tail_m"] == 1342
    if high:
        assert got["flags"] & R.KHAT_HIGH and got["khat"] > 0.7
    else:
        assert abs(got["khat"] - (1.0 - 1.0 / (s * s))) < 0.08 and not got["flags"]


def test_resample_then_analyse():
    from mcpar_amd import engine as E
    rows, T, nc = anchor_rows(), 200, 200
    w = E.weights_loglike(1.0)
    q, _ = E.debug_reweight_q(w, rows, T, nc)
    a, index = E.resample_rows(rows, T, nc, w, 100, 200, 1, with_index=True)
    want, _ = R.resample_index(q, 1, 20000)
    assert np.array_equal(np.bincount(index, minlength=len(q)), np.bincount(want, minlength=len(q))) and np.array_equal(index, want)
    s = a.summary(PROBS)
    assert abs(s["sd"][0] / math.sqrt(0.5) - 1.0) < 0.04 and abs(s["mean"][0]) < 0.03
    d = a.density(n=64)
    assert abs(d["sd"][0] / math.sqrt(0.5) - 1.0) < 0.04 and np.all(np.isfinite(d["y"])) and d["y"][0].max() > 0.4
    b = E.resample_rows(rows, T, nc, w, 100, 200, 2)
    c = a.compare(b, iid=True)
    print("two resamples: ks = %.4f, ks_p = %.4f" % (c["ks"][0], c["ks_p"][0]))
    assert c["ks_p"][0] > 0.001
    a.close()
    b.close()


# ---- more scan tiles than lanes, more steps than a histogram chunk, more sort tiles than a scan step -----------------------------
# (nc, np, T) -> scan tiles, tiles per lane of k_rw_scan, the first lane that owns none, histogram step chunks, sort tiles,
# whether rows 2^17 .. 2^17 + 2^18 have q = 0 (256 scan tiles: lanes 43 .. 127 sum to zero), the resample's seed
BIG = {(8, 1, 65537): (513, 3, 171, 2, 65, True, 1), (3, 1, 701783): (2057, 9, 229, 11, 258, False, 1)}
BIG_K = 600


def big_logw(nc, T, zeros):
    logw = spread_logw(T * nc) * np.float32(1.0 / 3.0)
    if zeros:
        logw[2 ** 17:2 ** 17 + 2 ** 18] = -INF
    return logw


def lane_stretches(index, tiles, per):
    """the lanes of k_rw_scan whose tiles the drawn rows lie in, and the last lane that owns a tile"""
    return set((np.asarray(index) // RS // per).tolist()), (tiles - 1) // per


@pytest.mark.parametrize("shape", sorted(BIG), ids=str)
def test_more_tiles_than_lanes(shape):
    from mcpar_amd import engine as E
    nc, np_, T = shape
    tiles, per, idle, chunks, stiles, zeros, seed = BIG[shape]
    N = T * nc
    g = E.debug_reweight_store_geometry(T, nc, np_ + 1, len(PROBS), BIG_K)
    assert (g["block"], g["scan_tile_rows"], g["scan_tiles"], g["scan_tiles_per_lane"]) == (256, RS, tiles, per)
    assert tiles > g["block"] and per == -(-tiles // 256) and idle == -(-tiles // per) and (idle < 256 or tiles - 228 * per == 5)
    assert g["hist_step_chunks"] == chunks == -(-T // 65536) and g["sort_tiles"] == stiles and g["draw_workgroups"] == 3
    if chunks == 2:
        assert T - 65536 == 1  # the second chunk holds one step
    assert g == dict(E.debug_reweight_geometry(N, np_ + 1, len(PROBS), BIG_K), hist_step_chunks=chunks)
    rows = make_rows(nc, np_, T)
    logw = big_logw(nc, T, zeros)
    lw = R.log_weights(logw, 1.0)
    # the reference alone: the draws fall in tiles of the first, a middle and the last lane stretch
    lanes, last = lane_stretches(R.resample_index(R.fixed_point(lw)[0], seed, BIG_K)[0], tiles, per)
    assert 0 in lanes and last in lanes and last == idle - 1 and any(0 < v < last for v in lanes), sorted(lanes)
    w = E.weights_host(logw)
    q, lwmax = held_q(w, rows, T, nc, lw, str(shape))
    if zeros:
        assert not q[2 ** 17:2 ** 17 + 2 ** 18].any() and q[2 ** 17 - 1] > 0 and q[2 ** 17 + 2 ** 18] > 0
    got = E.reweight_rows(rows, T, nc, w, PROBS)
    ref = R.restate(rows, q, lwmax, PROBS)
    assert ref["tail_m"] >= 5 and not math.isnan(ref["khat"]) and ref["nzero"] >= (2 ** 18 if zeros else 0)
    held(got, ref, str(shape))
    index = resample_held(w, rows, T, nc, q, BIG_K, seed, str(shape))
    lanes, last = lane_stretches(index, tiles, per)
    assert 0 in lanes and last in lanes and any(0 < v < last for v in lanes)
