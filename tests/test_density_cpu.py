"""The host steps of the sample-store densities against the float64 model tests/density_ref.py:
mcx_debug_density_grid (bw.nrd0, from / to, the grid) to 1e-15 relative -- the same few fp64 operations --, and
mcx_debug_density_finish (grid masses, convolution, interpolation) to 1e-10 of the peak: the plain 1024-term sum's own
bound is 1024 * 2^-53 = 1.1e-13, the margin is for exp() of libm against numpy's.  No GPU."""
import numpy as np
import pytest

import density_ref as D
from mcpar_amd import McxError
from mcpar_amd import engine as E

RTOL = 1e-15
FIELDS = ("bw", "from", "to", "lo", "up", "mean", "sd")


def stats(col):
    """the statistics a density call hands to the grid step, formed as the model forms them"""
    v = np.sort(np.asarray(col, np.float32))
    d = v.astype(np.float64)
    mean = d.sum() / d.size
    sd = float(np.sqrt(((d - mean) ** 2).sum() / (d.size - 1)))
    return dict(N=d.size, mean=mean, sd=sd, min_=float(v[0]), max_=float(v[-1]), q25=D.quantile7(v, 0.25), q75=D.quantile7(v, 0.75)), v


def close(a, b):
    return a == b or abs(a - b) <= RTOL * abs(b)


def check_grid(col, is_last_col=False, column=0, ncol=1, **kw):
    st, v = stats(col)
    clip = kw.get("clip", (0.0, 1.0))
    arr = lambda name: None if kw.get(name) is None else [kw[name] if c == column else np.nan for c in range(ncol)]  # noqa: E731
    spec = E.DensitySpec(adjust=kw.get("adjust", 1.0), clip=clip, bw=arr("bw"), from_=arr("from_"), to=arr("to"))
    qclip = (D.quantile7(v, clip[0]), D.quantile7(v, clip[1])) if tuple(clip) != (0.0, 1.0) else (np.nan, np.nan)
    got = E.debug_density_grid(qclip=qclip, is_last_col=is_last_col, col=column, spec=spec, **st)
    ref = D.grid(col, is_last_col=is_last_col, **kw)
    for f in FIELDS:
        assert close(float(got[f]), ref[f]), (f, float(got[f]), ref[f])
    assert got["nvalues"] == st["N"] and got["nbinned"] == 0 and got["flags"] == 0
    return got, ref


def test_grid_nrd0_normal_sample():
    rng = np.random.default_rng(1)
    col = rng.normal(1.0, 2.0, 20000).astype(np.float32)
    got, ref = check_grid(col)
    assert got["from"] == float(col.min()) and got["to"] == float(col.max())
    assert ref["bw"] == pytest.approx(0.9 * min(ref["sd"], 2 * 0.6745 * 2.0 / 1.34) * 20000 ** -0.2, rel=0.05)


def test_grid_iqr_zero_sd_positive():
    col = np.array([2.0] * 90 + [7.0] * 5 + [-1.0] * 5, np.float32)  # quartiles equal, sd > 0: hi is used
    got, ref = check_grid(col)
    assert ref["bw"] == 0.9 * ref["sd"] * 100 ** -0.2


def test_grid_constant_columns():
    got, ref = check_grid(np.full(50, -3.5, np.float32))  # sd = 0, iqr = 0: |min|
    assert ref["bw"] == 0.9 * 3.5 * 50 ** -0.2 and got["from"] == got["to"] == -3.5
    got, ref = check_grid(np.zeros(50, np.float32))        # and |min| = 0: 1
    assert ref["bw"] == 0.9 * 50 ** -0.2
    assert got["lo"] == -4.0 * ref["bw"] and got["up"] == 4.0 * ref["bw"]


def test_grid_adjust_and_given_values():
    rng = np.random.default_rng(2)
    col = rng.standard_normal(999).astype(np.float32)
    a, _ = check_grid(col)
    b, _ = check_grid(col, adjust=2.5)
    assert close(float(b["bw"]), 2.5 * float(a["bw"]))
    c, _ = check_grid(col, adjust=2.5, bw=0.125, column=2, ncol=4)  # adjust is not applied to a given bandwidth
    assert c["bw"] == 0.125
    d, _ = check_grid(col, from_=-1.0, column=1, ncol=2)
    assert d["from"] == -1.0 and d["to"] == float(col.max())
    e, _ = check_grid(col, from_=-10.0, to=10.0)
    assert e["lo"] == -10.0 - 4.0 * e["bw"] and e["up"] == 10.0 + 4.0 * e["bw"]


def test_grid_clip_pair_and_loglike_exception():
    rng = np.random.default_rng(3)
    col = (-rng.chisquare(4, 5001)).astype(np.float32)
    a, _ = check_grid(col, clip=(0.01, 0.99))
    v = np.sort(col)
    assert a["from"] == D.quantile7(v, 0.01) and a["to"] == D.quantile7(v, 0.99)
    b, _ = check_grid(col, clip=(0.01, 0.99), is_last_col=True)
    assert b["from"] == a["from"] and b["to"] == float(col.max())
    c, _ = check_grid(col, clip=(0.01, 0.99), is_last_col=True, to=0.0)  # a given `to` still overrides
    assert c["to"] == 0.0


def test_grid_nonfinite_statistics_give_a_nan_record():
    got = E.debug_density_grid(100, np.nan, np.nan, 0.0, np.inf, 0.0, 1.0)
    assert got["flags"] == E.SUMMARY_NONFINITE and got["nbinned"] == 0 and got["nvalues"] == 100
    assert all(np.isnan(got[f]) for f in FIELDS)


def test_grid_refusals():
    ok = dict(N=100, mean=0.0, sd=1.0, min_=-2.0, max_=2.0, q25=-0.6, q75=0.6)
    E.debug_density_grid(**ok)
    for spec in (E.DensitySpec(adjust=0.0), E.DensitySpec(adjust=-1.0), E.DensitySpec(adjust=np.inf), E.DensitySpec(adjust=np.nan),
                 E.DensitySpec(clip=(0.5, 0.5)), E.DensitySpec(clip=(-0.1, 0.9)), E.DensitySpec(clip=(0.1, 1.1)),
                 E.DensitySpec(clip=(0.9, 0.1)), E.DensitySpec(bw=[0.0]), E.DensitySpec(bw=[-1.0]), E.DensitySpec(bw=[np.inf]),
                 E.DensitySpec(from_=[3.0]), E.DensitySpec(to=[-3.0]), E.DensitySpec(from_=[1.0], to=[0.5])):
        with pytest.raises(McxError):
            E.debug_density_grid(spec=spec, **ok)
    with pytest.raises(McxError):
        E.debug_density_grid(**dict(ok, N=1))


def test_rows_refusals_need_no_device():
    """the spec is checked before anything touches a device: these raise MCX_ERR_INVALID (1), not MCX_ERR_NO_DEVICE, on a machine without one"""
    rows = np.zeros((8, 3), np.float32)
    for kw in (dict(n=1), dict(n=513), dict(adjust=0.0), dict(adjust=np.nan), dict(clip=(0.6, 0.4)), dict(clip=(0.0, 1.5)),
               dict(bw=[1.0, 0.0, np.nan]), dict(bw=[-2.0, np.nan, np.nan]), dict(from_=[np.nan, 2.0, 0.0], to=[np.nan, 1.0, 0.0])):
        with pytest.raises(McxError) as ei:
            E.rows_density(rows, 4, 2, **kw)
        assert ei.value.code == 1, kw
    with pytest.raises(McxError) as ei:  # N = 1
        E.rows_density(rows[:1], 1, 1)
    assert ei.value.code == 1
    with pytest.raises(ValueError):  # one entry per column
        E.rows_density(rows, 4, 2, bw=[1.0])


def hand_slots(rng, N):
    """slots as the sweep would leave them for N values spread over the grid, both edge slots in use"""
    ix = np.clip(np.round(rng.normal(256, 60, N)), -1, D.NG - 1).astype(np.int64)
    ix[:3] = -1
    ix[3:7] = D.NG - 1
    w = rng.integers(0, 1 << 24, N).astype(np.uint64)
    s = np.zeros((D.NG + 1, 2), np.uint64)
    s[:, 0] = np.bincount(ix + 1, minlength=D.NG + 1).astype(np.uint64)
    np.add.at(s[:, 1], ix + 1, w)
    return s


def record(g, N):
    rec = np.zeros(1, E.DENSITY_DTYPE)
    for f in FIELDS:
        rec[0][f] = g.get(f, 0.0)
    rec[0]["nvalues"] = N
    return rec[0]


@pytest.mark.parametrize("n", [512, 2, 100])
def test_finish_hand_made_slots(n):
    rng = np.random.default_rng(4)
    N = 30000
    s = hand_slots(rng, N)
    g = {"bw": 0.31, "from": -2.0, "to": 5.5, "mean": 0.0, "sd": 1.0}
    g["lo"], g["up"] = g["from"] - 4 * g["bw"], g["to"] + 4 * g["bw"]
    x, y = E.debug_density_finish(record(g, N), s, n)
    xr, yr = D.finish(g, s, N, n)
    assert x.tobytes() == xr.tobytes()
    assert x[0] == g["from"] and x[-1] == g["to"]
    assert np.abs(y - yr).max() <= 1e-10 * yr.max()


def test_model_fft_form_is_the_plain_sum():
    rng = np.random.default_rng(5)
    s = hand_slots(rng, 5000)
    g = {"bw": 0.2, "from": 0.0, "to": 3.0, "lo": -0.8, "up": 3.8}
    a = D.finish_direct(g, s, 5000)
    _, b = D.finish(g, s, 5000)
    xg = g["lo"] + np.arange(D.NG) * ((g["up"] - g["lo"]) / (D.NG - 1))
    assert np.abs(np.interp(np.linspace(0.0, 3.0, D.NG), xg, a) - b).max() <= 1e-13 * a.max()


def test_whole_estimate_on_host_integrates_to_one():
    """200 000 N(1, 2^2) floats: model bins, library finish; the estimate integrates to 1 over [from, to]"""
    rng = np.random.default_rng(6)
    col = rng.normal(1.0, 2.0, 200000).astype(np.float32)
    g, s, xr, yr = D.density(col)
    assert int(s[:, 0].sum()) == col.size
    got, _ = check_grid(col)
    x, y = E.debug_density_finish(got, s, 512)
    assert np.abs(y - yr).max() <= 1e-10 * yr.max()
    integral = float(((y[1:] + y[:-1]) * 0.5 * np.diff(x)).sum())
    assert abs(integral - 1.0) < 2e-5
    true = np.exp(-0.5 * ((x - 1.0) / 2.0) ** 2) / (2.0 * np.sqrt(2 * np.pi))
    assert np.abs(y - true).max() < 0.02 * true.max()


def test_finish_refusals():
    g = {"bw": 0.5, "from": 0.0, "to": 1.0, "lo": -2.0, "up": 3.0}
    s = np.zeros((D.NG + 1, 2), np.uint64)
    E.debug_density_finish(record(g, 10), s, 2)
    for bad, n in ((dict(g, bw=0.0), 16), (dict(g, lo=3.0), 16), (g, 1), (g, 513), (dict(g, to=-1.0), 16)):
        with pytest.raises(McxError):
            E.debug_density_finish(record(bad, 10), s, n)
    with pytest.raises(McxError):
        E.debug_density_finish(record(g, 1), s, 16)
