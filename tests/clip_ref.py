"""float64 numpy restatement of the tail clip (include/mcx.h), for the tests.

thresholds: per column the type-7 quantiles of (qlo, qhi) from the column sorted in float64 (the header's formula, as
summary_ref.quantiles_from_sorted has it; NaN for a column that holds a NaN), the last column's upper threshold ll_hi unless
that is NaN, a non-NaN lo[c] / hi[c] in place of either.  A row is kept iff every column lies strictly between its
thresholds, compared in float64; nbelow / nabove count !(v > lo) / !(v < hi) per column whatever the other columns say."""
import numpy as np

import summary_ref as S


def _given(a, c):
    return a is not None and not np.isnan(a[c])


def column_quantiles(rows, qlo, qhi):
    """q [ncol, 2]: the type-7 quantiles of every column, NaN for a column that holds a NaN"""
    rows = np.asarray(rows, np.float32)
    q = np.full((rows.shape[1], 2), np.nan)
    for c in range(rows.shape[1]):
        col = rows[:, c].astype(np.float64)
        if not np.isnan(col).any():
            q[c] = S.quantiles_from_sorted(np.sort(col), (qlo, qhi))[0]
    return q


def thresholds_from_quantiles(q, ll_hi=0.0, lo=None, hi=None):
    """(lo [ncol], hi [ncol]) from q [ncol, 2] by the LL rule and the overrides"""
    q = np.asarray(q, np.float64).reshape(-1, 2)
    tl, th = q[:, 0].copy(), q[:, 1].copy()
    if not np.isnan(ll_hi):
        th[-1] = ll_hi
    for c in range(q.shape[0]):
        if _given(lo, c):
            tl[c] = lo[c]
        if _given(hi, c):
            th[c] = hi[c]
    return tl, th


def thresholds(rows, qlo=0.01, qhi=0.99, ll_hi=0.0, lo=None, hi=None):
    return thresholds_from_quantiles(column_quantiles(rows, qlo, qhi), ll_hi, lo, hi)


def apply(rows, tl, th):
    """the clip of rows [N, ncol] float32 with thresholds tl, th [ncol]: a dict of keep [N] bool, rows (the kept rows),
    index (their source rows, int64), nbelow and nabove [ncol]"""
    rows = np.asarray(rows, np.float32)
    v = rows.astype(np.float64)
    with np.errstate(invalid="ignore"):
        above_lo, below_hi = v > np.asarray(tl, np.float64), v < np.asarray(th, np.float64)
    keep = (above_lo & below_hi).all(axis=1)
    return dict(keep=keep, rows=rows[keep], index=np.flatnonzero(keep).astype(np.int64), nbelow=(~above_lo).sum(axis=0),
                nabove=(~below_hi).sum(axis=0))


def clip(rows, qlo=0.01, qhi=0.99, ll_hi=0.0, lo=None, hi=None):
    tl, th = thresholds(rows, qlo, qhi, ll_hi, lo, hi)
    out = apply(rows, tl, th)
    out["lo"], out["hi"] = tl, th
    return out


def check(rs, rows, ref=None):
    """assert a RowSet against apply() with the thresholds the RowSet reports (or against ref, a dict of apply / clip):
    counts, kept rows and indices, all exact"""
    rep = rs.report
    ref = ref or apply(rows, rep["lo"], rep["hi"])
    assert rs.nrows == int(ref["keep"].sum()), (rs.nrows, int(ref["keep"].sum()))
    assert np.array_equal(rep["nbelow"], ref["nbelow"]), (rep["nbelow"], ref["nbelow"])
    assert np.array_equal(rep["nabove"], ref["nabove"]), (rep["nabove"], ref["nabove"])
    if rs.h:
        assert np.array_equal(rs.index(), ref["index"])
        assert np.array_equal(rs.rows().view(np.uint32), ref["rows"].view(np.uint32))
    return ref
