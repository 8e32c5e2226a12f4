"""The two ways to a view of a store -- on_store (a step range of an engine's store, in place) and on_rows (the same steps
copied out with samples_range and uploaded to a scratch store) -- run the same kernels with the same grids on the same
layout: Engine.summary / rank_summary / covariance of a range inside the store give the bytes of rows_summary /
rows_rank_summary / rows_covariance of its rows (equal NaN patterns count as equal).  And every engine entry point refuses
a range that is not in the store with the same status and text."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

# (nc, np, steps in the store, first_step, nsteps): first_step > 0 and first_step + nsteps < steps.  At nc = np = 17 the
# parameter tile set has two tiles of 16 columns and two blocks of 16 chains, and log L sits behind 17 columns
SHAPES = {"5x3": (5, 3, 12, 3, 8), "17x17": (17, 17, 16, 2, 12)}


def run(nc, d, nsamp):
    import mcpar_amd as M
    params = np.concatenate([np.linspace(-1.0, 1.0, d), np.linspace(0.5, 2.0, d)]).astype(np.float32)
    vg, keep = M.make_vlfunc(M.VL_GAUSSIAN, d, params)
    eg = M.Engine(d, nc, pl=1.0)
    eg.run(nsamp, 40, O.default_pinit(d, nc), vg)
    eg._vl_keep = keep
    return eg


def assert_same_bytes(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
        same = x.tobytes() == y.tobytes() or (x.dtype.kind == "f" and np.array_equal(np.isnan(x), np.isnan(y)) and
                                              np.array_equal(x[~np.isnan(x)], y[~np.isnan(y)]))
        assert same, (what, k, x, y)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_store_range_agrees_with_its_rows(shape):
    from mcpar_amd import engine as E
    nc, d, steps, first, nsteps = SHAPES[shape]
    eg = run(nc, d, steps)
    assert eg.samples.shape[0] == steps * nc and 0 < first and first + nsteps < steps
    rows = eg.samples_range(first, nsteps)
    probs = (0.01, 0.5, 0.99)
    assert_same_bytes(eg.summary(probs, first_step=first, nsteps=nsteps), E.rows_summary(rows, nsteps, nc, probs), "summary")
    assert_same_bytes(eg.rank_summary(first_step=first, nsteps=nsteps), E.rows_rank_summary(rows, nsteps, nc), "rank_summary")
    assert_same_bytes(eg.covariance(first_step=first, nsteps=nsteps), E.rows_covariance(rows, nsteps, nc), "covariance")


ENTRIES = ("summary", "rank_summary", "rank_summary_times", "covariance", "covariance_times", "summary_windows")


def test_refusals_are_the_same_everywhere():
    import mcpar_amd as M
    nc, d, steps, _first, _nsteps = SHAPES["5x3"]
    fresh = M.Engine(d, nc, pl=1.0)
    eg = run(nc, d, steps)
    cases = ((eg, dict(first_step=-1, nsteps=8), "not in the sample store"),
             (eg, dict(first_step=steps - 7, nsteps=8), "not in the sample store"),  # one step past the end
             (fresh, dict(first_step=0, nsteps=8), "the sample store is empty"))     # no run yet
    for name in ENTRIES:
        for e, kw, text in cases:
            with pytest.raises(M.McxError) as ei:
                getattr(e, name)(**kw)
            assert ei.value.code == 1 and text in str(ei.value), (name, kw, str(ei.value))
        getattr(eg, name)(first_step=steps - 8, nsteps=8)  # the last range that is in the store
