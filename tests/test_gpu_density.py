"""Sample-store densities on the GPU (include/mcx.h) against the float64 model tests/density_ref.py.
The binning sweep adds integers, so its slots are compared exactly; the record of a column to 1e-9 relative (the tolerance
test_gpu_summary.py gives mean and sd), from / to on bits where they are order statistics and to 1e-12 relative where they
are clip quantiles (the project's quantile tolerance), and y to 1e-10 of its peak after the model is given the grid the
call returned -- so a last-bit difference in sd cannot move a value across a bin edge."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import density_ref as D
import oracle_lib as O

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("bw", "from", "to", "lo", "up", "mean", "sd")


def synth(nsteps, nc, np_, seed):
    """rows [nsteps * nc, np_ + 1]: columns of different location, scale and shape, a few values repeated"""
    rng = np.random.default_rng(seed)
    N = nsteps * nc
    rows = np.empty((N, np_ + 1), np.float32)
    for c in range(np_ + 1):
        kind = c % 4
        if kind == 0:
            v = rng.normal(c - 3.0, 0.5 + 0.1 * c, N)
        elif kind == 1:
            v = rng.uniform(-1e-3 * (c + 1), 2e-3, N)
        elif kind == 2:
            v = -rng.chisquare(3, N) * 40.0
        else:
            v = np.round(rng.normal(0.0, 3.0, N))  # heavy ties
        rows[:, c] = v
    return rows


def same_bytes(a, b, what=""):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (what, k)


def model_slots(rows, lo, up):
    return np.stack([D.bins(rows[:, c], lo[c], up[c]) for c in range(rows.shape[1])])


def check_model(got, rows, n=512, clip=(0.0, 1.0), cols=None, adjust=1.0, **kw):
    """every column of a density dict against the model of its rows"""
    ncol = rows.shape[1]
    N = rows.shape[0]
    for c in (range(ncol) if cols is None else cols):
        col = rows[:, c]
        last = c == ncol - 1
        ref = D.grid(col, adjust=adjust, clip=clip, is_last_col=last, **{k: (None if v is None else v[c]) for k, v in kw.items()})
        for f in ("bw", "lo", "up", "mean", "sd"):
            assert got[f][c] == pytest.approx(ref[f], rel=1e-9, abs=0.0 if ref[f] != 0.0 else 1e-300), (c, f)
        if tuple(clip) == (0.0, 1.0) and not kw:
            assert got["from"][c] == float(col.min()) and got["to"][c] == float(col.max()), c
        else:
            assert got["from"][c] == pytest.approx(ref["from"], rel=1e-12), c
            assert got["to"][c] == pytest.approx(ref["to"], rel=1e-12), c
            if last and kw.get("to") is None:
                assert got["to"][c] == float(col.max())
        assert got["nvalues"][c] == N and got["flags"][c] == 0
        g = {f: float(got[f][c]) for f in FIELDS}
        s = D.bins(col, g["lo"], g["up"])
        assert got["nbinned"][c] == int(s[1:, 0].sum()), c
        x, y = D.finish(g, s, N, n)
        assert got["x"][c].tobytes() == x.tobytes(), c
        assert np.abs(got["y"][c] - y).max() <= 1e-10 * y.max(), (c, np.abs(got["y"][c] - y).max(), y.max())


# ---- the sweep: exact slots ------------------------------------------------------------------------------------------------
# (nsteps, nc, np): an odd tile with np % 4 != 0; N = 2; two column tiles plus log L; the widest row; one step (no half-chain)
@pytest.mark.parametrize("shape", [(7, 37, 5), (2, 1, 1), (9, 300, 17), (5, 64, 256), (1, 50, 2)])
def test_slots_are_the_models_integers(shape):
    from mcpar_amd import engine as E
    nsteps, nc, np_ = shape
    rows = synth(nsteps, nc, np_, 10 + np_)
    got = E.rows_density(rows, nsteps, nc)
    slots = E.debug_rows_density_bins(rows, nsteps, nc, got["lo"], got["up"])
    want = model_slots(rows, got["lo"], got["up"])
    assert slots.shape == want.shape == (np_ + 1, 513, 2)
    assert np.array_equal(slots, want), np.argwhere(slots != want)[:4]
    assert np.array_equal(got["nbinned"], want[:, 1:, 0].sum(axis=1).astype(np.int64))
    assert np.all(got["nbinned"] == nsteps * nc)  # from = min, to = max: nothing is dropped
    check_model(got, rows, cols=sorted({0, np_ // 2, np_}))


def test_carry_and_contention():
    """4.48 M values of one column in one slot: more than a 16-, 20- or 24-bit field holds, and more than one workgroup's
    chunk (65 536 values) many times over; the neighbour column is spread over its grid"""
    from mcpar_amd import engine as E
    nsteps, nc = 70001, 64
    rng = np.random.default_rng(7)
    N = nsteps * nc
    rows = np.empty((N, 3), np.float32)
    rows[:, 0] = 3.0
    rows[12345, 0], rows[N - 77, 0] = 2.0, 5.0
    rows[:, 1] = rng.uniform(-1.0, 1.0, N)
    rows[:, 2] = -rng.chisquare(2, N)
    got = E.rows_density(rows, nsteps, nc)
    slots = E.debug_rows_density_bins(rows, nsteps, nc, got["lo"], got["up"])
    want = model_slots(rows, got["lo"], got["up"])
    assert np.array_equal(slots, want), np.argwhere(slots != want)[:4]
    assert int(slots[0, :, 0].max()) == N - 2 and int(slots[0, :, 0].max()) > 1 << 22
    assert np.all(got["nbinned"] == N)
    check_model(got, rows, cols=[0])


def test_edges():
    """lo = 0, up = 511, so delta = 1: the values at and beyond both ends of the grid"""
    from mcpar_amd import engine as E
    vals = np.array([-1.5, -0.5, -0.0, 0.0, 1e-42, 510.25, 511.0, 511.5, 512.0], np.float32)
    assert vals[4] != 0.0  # a denormal float
    rows = np.stack([vals, np.linspace(10.0, 500.0, vals.size).astype(np.float32)], axis=1)
    lo, up = np.zeros(2), np.full(2, 511.0)
    slots = E.debug_rows_density_bins(rows, vals.size, 1, lo, up)
    want = model_slots(rows, lo, up)
    assert np.array_equal(slots, want), np.argwhere(slots != want)[:4]
    s = slots[0]
    assert s[0].tolist() == [1, 1 << 23]               # -0.5: ix = -1, fx = 0.5
    assert s[1, 0] == 3 and s[1, 1] == 0               # -0.0, 0 and the denormal: ix = 0, w = 0
    assert s[511].tolist() == [1, 1 << 22]             # 510.25
    assert s[512].tolist() == [2, 1 << 23]             # 511 (fx = 0) and 511.5
    assert int(s[:, 0].sum()) == vals.size - 2         # -1.5 and 512 are dropped
    rec = np.zeros(1, E.DENSITY_DTYPE)[0]
    g = {"bw": 1.5, "from": 0.0, "to": 511.0, "lo": 0.0, "up": 511.0, "mean": 0.0, "sd": 1.0}
    for f in FIELDS:
        rec[f] = g[f]
    rec["nvalues"] = vals.size
    x, y = E.debug_density_finish(rec, s, 512)
    xr, yr = D.finish(g, want[0], vals.size, 512)
    assert x.tobytes() == xr.tobytes()
    assert np.abs(y - yr).max() <= 1e-10 * yr.max()
    # the edge rules of BinDist: ix = -1 gives only fx to y[0], ix = n_g - 1 only 1 - fx to y[n_g - 1]
    m = D.masses(want[0], vals.size)
    assert m[0] == (3 + 0.5) / vals.size and m[511] == (0.25 + 1.0 + 0.5) / vals.size


def test_nonfinite_columns():
    from mcpar_amd import engine as E
    nsteps, nc = 8, 40
    clean = synth(nsteps, nc, 3, 3)
    rows = clean.copy()
    rows[17, 0] = np.nan
    rows[200, 2] = np.inf
    rows[5, 3] = -np.inf
    got = E.rows_density(rows, nsteps, nc, n=100)
    ref = E.rows_density(clean, nsteps, nc, n=100)
    for c in (0, 2, 3):
        assert got["flags"][c] == E.SUMMARY_NONFINITE and got["nbinned"][c] == 0 and got["nvalues"][c] == nsteps * nc
        assert all(np.isnan(got[f][c]) for f in FIELDS)
        assert np.all(np.isnan(got["x"][c])) and np.all(np.isnan(got["y"][c]))
    assert got["flags"][1] == 0
    for k in got:  # the clean column: the bytes it has without the bad values
        assert got[k][1].tobytes() == ref[k][1].tobytes(), k
    check_model(got, rows, n=100, cols=[1])


# ---- the whole call ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def whole_rows():
    return synth(50, 100, 5, 99)


def test_whole_call_defaults():
    from mcpar_amd import engine as E
    rows = whole_rows()
    check_model(E.rows_density(rows, 50, 100), rows)


def test_whole_call_clip_adjust_and_n():
    from mcpar_amd import engine as E
    rows = whole_rows()
    got = E.rows_density(rows, 50, 100, n=77, adjust=0.5, clip=(0.01, 0.99))
    check_model(got, rows, n=77, adjust=0.5, clip=(0.01, 0.99))
    assert got["x"].shape == (6, 77)
    # (the normal column: its tails beyond the clip quantiles and 4 bw more are dropped)
    assert 4500 < got["nbinned"][0] < 5000 and got["to"][-1] == float(rows[:, -1].max())


def test_whole_call_given_bw_from_to():
    from mcpar_amd import engine as E
    rows = whole_rows()
    nan = np.nan
    bw = [nan, 0.25, nan, nan, nan, 3.0]
    from_ = [-4.0, nan, nan, nan, nan, -100.0]
    to = [nan, nan, nan, 2.0, nan, 0.0]
    got = E.rows_density(rows, 50, 100, adjust=2.0, bw=bw, from_=from_, to=to)
    assert got["bw"][1] == 0.25 and got["bw"][5] == 3.0 and got["from"][0] == -4.0 and got["to"][3] == 2.0
    check_model(got, rows, adjust=2.0, bw=bw, from_=from_, to=to)
    plain = E.rows_density(rows, 50, 100, adjust=2.0)
    for k in got:  # the columns with no entry of their own are untouched
        assert got[k][2].tobytes() == plain[k][2].tobytes() and got[k][4].tobytes() == plain[k][4].tobytes(), k


def test_constant_and_zero_columns():
    from mcpar_amd import engine as E
    rows = np.zeros((60, 3), np.float32)
    rows[:, 0] = -3.5
    rows[:, 2] = np.arange(60)
    got = E.rows_density(rows, 6, 10, n=16)
    assert got["bw"][0] == pytest.approx(0.9 * 3.5 * 60 ** -0.2, rel=1e-15) and got["bw"][1] == pytest.approx(0.9 * 60 ** -0.2, rel=1e-15)
    assert np.all(got["x"][0] == -3.5) and np.all(got["x"][1] == 0.0)
    check_model(got, rows, n=16)


# ---- the engine's store ------------------------------------------------------------------------------------------------------
def run(d, n, nburn, nsamp, stride=1, async_run=False):
    import mcpar_amd as M
    from mcpar_amd import engine as E
    if d % 2 == 0:
        vg, keep = M.make_vlfunc(M.VL_ROSENBROCK1, d)
    else:  # (Rosenbrock1 takes an even number of parameters)
        vg, keep = M.make_vlfunc(M.VL_GAUSSIAN, d, np.concatenate([np.linspace(-1.0, 1.0, d), np.linspace(0.5, 2.0, d)]).astype(np.float32))
    eg = M.Engine(d, n, pl=1.0)
    if stride > 1:
        eg.set_option(E.OPT_SAMPLE_STRIDE, stride)
    if async_run:
        eg.set_option(E.OPT_ASYNC_RUN, 1)
    eg.run(nsamp, nburn, O.default_pinit(d, n), vg)
    eg._vl_keep = keep
    return eg


def test_engine_store_is_its_rows_and_the_model():
    from mcpar_amd import engine as E
    eg = run(16, 4096, 300, 400)
    got = eg.density()
    rows = eg.samples_range(0, 400)
    same_bytes(got, E.rows_density(rows, 400, 4096), "rows")
    same_bytes(got, eg.density(), "second call")
    s = eg.summary((0.25, 0.75))
    assert got["mean"].tobytes() == s["mean"].tobytes() and got["sd"].tobytes() == s["sd"].tobytes()
    assert np.array_equal(got["from"], s["min"].astype(np.float64)) and np.array_equal(got["to"], s["max"].astype(np.float64))
    check_model(got, rows, cols=[0, 7, 15, 16])
    c = eg.density(clip=(0.01, 0.99), n=64)
    q = eg.summary((0.01, 0.99))["quantiles"]
    assert c["from"].tobytes() == q[:, 0].tobytes() and c["to"][:-1].tobytes() == q[:-1, 1].tobytes()
    assert c["to"][-1] == float(s["max"][-1])
    eg.close()


def test_engine_sub_range_np5():
    from mcpar_amd import engine as E
    eg = run(5, 333, 100, 40)
    got = eg.density(first_step=3, nsteps=30, n=50)
    rows = eg.samples_range(3, 30)
    same_bytes(got, E.rows_density(rows, 30, 333, n=50), "rows")
    check_model(got, rows, n=50)
    eg.close()


def test_engine_sample_stride():
    from mcpar_amd import engine as E
    eg = run(16, 512, 100, 150, stride=3)
    kept = eg.samples.shape[0] // eg.nc
    assert kept == 50
    got = eg.density(n=32)
    rows = eg.samples_range(0, kept)
    same_bytes(got, E.rows_density(rows, kept, 512, n=32), "rows")
    check_model(got, rows, n=32, cols=[0, 16])
    eg.close()


def test_async_run_gives_the_synchronous_bytes():
    a = run(16, 2048, 100, 100, async_run=True)
    da = a.density(n=128)  # straight after the queued run
    b = run(16, 2048, 100, 100)
    same_bytes(da, b.density(n=128), "async")
    a.close()
    b.close()


# ---- a derived store -----------------------------------------------------------------------------------------------------------
def test_derived_store():
    import mcpar_amd as M
    from mcpar_amd import engine as E
    d, nc, T = 5, 200, 24
    eg = run(d, nc, 60, T)
    ident = eg.derive(M.derive_linear(np.eye(d, dtype=np.float32), np.zeros(d, np.float32)))
    same_bytes(ident.density(n=40, clip=(0.05, 0.95)), eg.density(n=40, clip=(0.05, 0.95)), "identity")
    rng = np.random.default_rng(8)
    two = eg.derive(M.derive_linear(rng.standard_normal((2, d)).astype(np.float32), np.array([0.5, -1.0], np.float32)))
    got = two.density(n=40)
    rows = two.rows()
    assert rows.shape == (T * nc, 3)
    same_bytes(got, E.rows_density(rows, T, nc, n=40), "two outputs")
    check_model(got, rows, n=40)
    for s in (ident, two):
        s.close()
    eg.close()


# ---- refusals and lifetime ------------------------------------------------------------------------------------------------------
def test_refusals_and_lifetime():
    r = subprocess.run([sys.executable, os.path.join(HERE, "density_worker.py")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=120)
    out = r.stdout.decode(errors="replace")
    if r.returncode != 0:
        print(out)
    assert r.returncode == 0, "the density worker ended with status %d" % r.returncode
    assert "density lifetime: all scenarios done" in out
