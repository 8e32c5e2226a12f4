"""float64 numpy restatement of mcx_samples_rank_summary, for the tests.

It sits on summary_ref.py: split chains, R-hat, the Geyer ESS and the type-7 quantiles are that file's; what is added is
the pooled average ranks, the normal scores (statistics.NormalDist().inv_cdf is Wichura's PPND16, the algorithm the
device evaluates), the fold about the median and the tail indicators."""
import math
import statistics

import numpy as np

import summary_ref as R

_ND = statistics.NormalDist()
PROBS = (0.05, 0.5, 0.95)
RHAT_PIECES = ("rhat_bulk", "rhat_folded")
ESS_PIECES = ("ess_bulk", "ess_q05", "ess_q95")
FIELDS = ("rhat", "rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "ess_q05", "ess_q95", "q05", "median", "q95")


def ranks(v):
    """average ranks (float64, 1-based) of float32 values among themselves: equal values (-0 == +0) share the mean of
    their positions; NaNs are equal to each other and last"""
    v = np.asarray(v, np.float32).reshape(-1)
    k = R.okey(np.where(v == 0, np.float32(0), v))
    sk = np.sort(k)
    lo = np.searchsorted(sk, k, "left").astype(np.float64)   # values below
    hi = np.searchsorted(sk, k, "right").astype(np.float64)  # values below or equal
    return (lo + hi + 1.0) / 2.0


def ranks_by_sort(v):
    """ranks() from one sort, for millions of values (ranks() searches every value in the sorted column, twice): a value's
    tie run occupies sorted positions [lo, hi), and its rank is (lo + hi + 1) / 2.  tests/test_rank_summary_cpu.py holds it
    equal to ranks()."""
    v = np.asarray(v, np.float32).reshape(-1)
    k = R.okey(np.where(v == 0, np.float32(0), v))
    assert k.size < 1 << 32
    pk = (k.astype(np.uint64) << np.uint64(32)) | np.arange(k.size, dtype=np.uint64)  # (key, position): one plain sort
    pk.sort()
    order, sk = (pk & np.uint64(0xffffffff)).astype(np.int64), (pk >> np.uint64(32)).astype(np.uint32)
    first = np.ones(sk.size, bool)  # the sorted positions at which a tie run begins
    first[1:] = sk[1:] != sk[:-1]
    lo = np.flatnonzero(first)
    hi = np.append(lo[1:], sk.size)
    out = np.empty(sk.size, np.float64)
    out[order] = ((lo + hi + 1) / 2.0)[np.cumsum(first) - 1]
    return out


def normal_scores(r, N):
    """z = float32(PPND16((r - 0.375) / (N + 0.25)))"""
    r = np.asarray(r, np.float64)
    u, inv = np.unique(r, return_inverse=True)
    z = np.array([_ND.inv_cdf(float(p)) for p in (u - 0.375) / (N + 0.25)], np.float64).astype(np.float32)
    return z[inv].reshape(r.shape)


def thresholds(x):
    """(q05, median, q95) of x [T, nc] float32: summary_ref's type-7 quantiles over all values"""
    q, _ = R.quantiles_from_sorted(R.key_sort(x), PROBS)
    return q


def transforms(x):
    """x [T, nc] float32 -> dict of the four transformed columns [T, nc] float32, the ranks behind the first two, and thr"""
    T, nc = x.shape
    N = T * nc
    thr = thresholds(x)
    xd = x.astype(np.float64)
    f = np.abs(xd - thr[1]).astype(np.float32)
    rx, rf = ranks(x).reshape(T, nc), ranks(f).reshape(T, nc)
    return dict(thr=thr, ranks=rx, ranks_folded=rf, z=normal_scores(rx, N), z_folded=normal_scores(rf, N),
                i05=(xd <= thr[0]).astype(np.float32), i95=(xd <= thr[2]).astype(np.float32))


def restate_column(x):
    """x [T, nc] float32: the rank-normalised summary of one column as a dict (plus 'pairs' and 'n' per ESS piece)"""
    nan = float("nan")
    if not np.all(np.isfinite(x)):
        r = {f: nan for f in FIELDS}
        r.update(flags=1, ess_bulk_lag=0, pairs={}, n=x.shape[0] // 2)
        return r
    t = transforms(x)
    parts = {k: R.restate_column(np.ascontiguousarray(t[k]), ()) for k in ("z", "z_folded", "i05", "i95")}
    r = dict(flags=0, q05=t["thr"][0], median=t["thr"][1], q95=t["thr"][2], n=x.shape[0] // 2,
             rhat_bulk=parts["z"]["rhat"], rhat_folded=parts["z_folded"]["rhat"], ess_bulk=parts["z"]["ess"],
             ess_bulk_lag=parts["z"]["ess_lag"], ess_q05=parts["i05"]["ess"], ess_q95=parts["i95"]["ess"],
             pairs=dict(ess_bulk=parts["z"]["pairs"], ess_q05=parts["i05"]["pairs"], ess_q95=parts["i95"]["pairs"]),
             lags=dict(ess_bulk=parts["z"]["ess_lag"], ess_q05=parts["i05"]["ess_lag"], ess_q95=parts["i95"]["ess_lag"]))
    r["rhat"] = nan if math.isnan(r["rhat_bulk"]) or math.isnan(r["rhat_folded"]) else max(r["rhat_bulk"], r["rhat_folded"])
    r["ess_tail"] = nan if math.isnan(r["ess_q05"]) or math.isnan(r["ess_q95"]) else min(r["ess_q05"], r["ess_q95"])
    return r


def restate(rows, nsteps, nc):
    """rows [nsteps * nc, np + 1] (MCout layout): one dict per column"""
    ncol = rows.shape[1]
    x = rows.reshape(nsteps, nc, ncol)
    return [restate_column(np.ascontiguousarray(x[:, :, c])) for c in range(ncol)]


def guard_ok(r, margin=1e-5):
    """summary_ref.check's guard for every ESS piece: the pair sums around the Geyer stop are clear of 0"""
    for f in ESS_PIECES:
        p = r["pairs"].get(f) or []
        if not math.isnan(r[f]) and r["lags"][f] < r["n"] - 5 and not (abs(p[-1]) > margin and abs(p[-2]) > margin):
            return False
    return True


def check(got, ref, abs_rhat=1e-7, rel_ess=1e-4, rel_q=1e-12, margin=1e-5, stats=None):
    """assert the GPU's dict (Engine.rank_summary) against restate()'s list, with summary_ref.check's tolerances.
    stats (a dict) collects the largest ESS relative error and R-hat absolute error seen."""
    refs = dict(enumerate(ref)) if isinstance(ref, list) else ref
    for c, r in sorted(refs.items()):
        where = "column %d" % c
        assert got["flags"][c] == r["flags"], where
        if r["flags"]:
            for f in FIELDS:
                assert math.isnan(got[f][c]), (where, f)
            assert got["ess_bulk_lag"][c] == 0, where
            continue
        for f in ("q05", "median", "q95"):
            np.testing.assert_allclose(got[f][c], r[f], rtol=rel_q, atol=0, err_msg=where + " " + f)
        assert got["ess_bulk_lag"][c] == r["ess_bulk_lag"], (where, got["ess_bulk_lag"][c], r["ess_bulk_lag"])
        for f in RHAT_PIECES:
            if math.isnan(r[f]):
                assert math.isnan(got[f][c]), (where, f)
            else:
                assert abs(got[f][c] - r[f]) < abs_rhat, (where, f, got[f][c], r[f])
                if stats is not None:
                    stats["rhat_abs"] = max(stats.get("rhat_abs", 0.0), abs(got[f][c] - r[f]))
        for f in ESS_PIECES:
            if math.isnan(r[f]):
                assert math.isnan(got[f][c]), (where, f)
            else:
                np.testing.assert_allclose(got[f][c], r[f], rtol=rel_ess, err_msg=where + " " + f)
                if stats is not None:
                    stats["ess_rel"] = max(stats.get("ess_rel", 0.0), abs(got[f][c] - r[f]) / r[f])
        assert guard_ok(r, margin), (where, "a pair sum at the Geyer stop is within %g of 0" % margin)
        # the combined fields are the max / min of the call's own pieces, NaN when either is
        for f, a, b, op in (("rhat", "rhat_bulk", "rhat_folded", max), ("ess_tail", "ess_q05", "ess_q95", min)):
            if math.isnan(got[a][c]) or math.isnan(got[b][c]):
                assert math.isnan(got[f][c]), (where, f)
            else:
                assert got[f][c] == op(got[a][c], got[b][c]), (where, f)
