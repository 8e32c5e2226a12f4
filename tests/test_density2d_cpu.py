"""The host steps of the pair densities against the float64 model tests/density2d_ref.py:
mcx_debug_density2d_grid (bandwidth.nrd / 4, from / to, the grid) to 1e-9 relative, mcx_debug_density2d_finish (node masses,
the separable convolution) to 1e-10 of the peak -- a sum of at most g^2 non-negative terms has a relative error below
2 g 2^-53 = 1.4e-14 at g = 64, the margin is for exp() of libm against numpy's --, every refusal that needs no device, and
the model itself against the direct kde2d sum.  No GPU."""
import numpy as np
import pytest

import density2d_ref as D
import density_ref as D1
from mcpar_amd import McxError
from mcpar_amd import engine as E

FIELDS = ("bw", "from", "to", "lo", "up", "mean", "sd")


def stats(col):
    v = np.sort(np.asarray(col, np.float32))
    d = v.astype(np.float64)
    mean = d.sum() / d.size
    sd = float(np.sqrt(((d - mean) ** 2).sum() / (d.size - 1)))
    return dict(N=d.size, mean=mean, sd=sd, min_=float(v[0]), max_=float(v[-1]), q25=D1.quantile7(v, 0.25), q75=D1.quantile7(v, 0.75)), v


def check_grid(col, is_last_col=False, column=0, ncol=1, **kw):
    st, v = stats(col)
    clip = kw.get("clip", (0.0, 1.0))
    arr = lambda name: None if kw.get(name) is None else [kw[name] if c == column else np.nan for c in range(ncol)]  # noqa: E731
    spec = E.Density2dSpec(adjust=kw.get("adjust", 1.0), clip=clip, bw=arr("bw"), from_=arr("from_"), to=arr("to"))
    qclip = (D1.quantile7(v, clip[0]), D1.quantile7(v, clip[1])) if tuple(clip) != (0.0, 1.0) else (np.nan, np.nan)
    got = E.debug_density2d_grid(qclip=qclip, is_last_col=is_last_col, col=column, spec=spec, **st)
    ref = D.grid(col, is_last_col=is_last_col, **kw)
    for f in FIELDS:
        assert float(got[f]) == pytest.approx(ref[f], rel=1e-9, abs=0.0 if ref[f] != 0.0 else 1e-300), (f, float(got[f]), ref[f])
    assert got["nvalues"] == st["N"] and got["nbinned"] == 0 and got["flags"] == 0
    return got, ref


def record(g, N):
    rec = np.zeros(1, E.DENSITY_DTYPE)
    for f in FIELDS:
        rec[0][f] = g.get(f, 0.0)
    rec[0]["nvalues"] = N
    return rec[0]


def pair(kind, N=2000, seed=11):
    rng = np.random.default_rng(seed)
    if kind == "gauss":  # correlation 0.8
        a = rng.normal(1.0, 2.0, N)
        b = 0.8 * a / 2.0 + 0.6 * rng.normal(0.0, 1.0, N) - 3.0
    else:                # a banana
        a = rng.normal(0.0, 1.0, N)
        b = a * a + 0.3 * rng.normal(0.0, 1.0, N)
    return a.astype(np.float32), b.astype(np.float32)


# ---- the grid ------------------------------------------------------------------------------------------------------------
def test_grid_nrd_normal_sample():
    rng = np.random.default_rng(1)
    col = rng.normal(1.0, 2.0, 20000).astype(np.float32)
    got, ref = check_grid(col)
    assert got["from"] == float(col.min()) and got["to"] == float(col.max())
    # bandwidth.nrd = 4 * 1.06 * min(sd, IQR / 1.34) * N^(-1/5), and kde2d uses a quarter of it
    assert ref["bw"] == pytest.approx(1.06 * min(ref["sd"], 2 * 0.6745 * 2.0 / 1.34) * 20000 ** -0.2, rel=0.05)
    assert got["lo"] == got["from"] - 4.0 * got["bw"] and got["up"] == got["to"] + 4.0 * got["bw"]


def test_grid_fallbacks():
    _, ref = check_grid(np.array([2.0] * 90 + [7.0] * 5 + [-1.0] * 5, np.float32))  # quartiles equal, sd > 0
    assert ref["bw"] == 1.06 * ref["sd"] * 100 ** -0.2
    got, ref = check_grid(np.full(50, -3.5, np.float32))  # sd = 0: |min|
    assert ref["bw"] == 1.06 * 3.5 * 50 ** -0.2 and got["from"] == got["to"] == -3.5
    got, ref = check_grid(np.zeros(50, np.float32))        # and |min| = 0: 1
    assert ref["bw"] == 1.06 * 50 ** -0.2


def test_grid_adjust_given_values_and_clip():
    rng = np.random.default_rng(2)
    col = (-rng.chisquare(4, 5001)).astype(np.float32)
    a, _ = check_grid(col)
    b, _ = check_grid(col, adjust=2.5)
    assert float(b["bw"]) == pytest.approx(2.5 * float(a["bw"]), rel=1e-15)
    c, _ = check_grid(col, adjust=2.5, bw=0.125, column=2, ncol=4)  # adjust is not applied to a given bandwidth
    assert c["bw"] == 0.125
    d, _ = check_grid(col, from_=-30.0, column=1, ncol=2)
    assert d["from"] == -30.0 and d["to"] == float(col.max())
    v = np.sort(col)
    e, _ = check_grid(col, clip=(0.01, 0.99))
    assert e["from"] == D1.quantile7(v, 0.01) and e["to"] == D1.quantile7(v, 0.99)
    f, _ = check_grid(col, clip=(0.01, 0.99), is_last_col=True)  # log L keeps its upper end
    assert f["from"] == e["from"] and f["to"] == float(col.max())


def test_grid_nonfinite_statistics_give_a_nan_record():
    got = E.debug_density2d_grid(100, np.nan, np.nan, 0.0, np.inf, 0.0, 1.0)
    assert got["flags"] == E.SUMMARY_NONFINITE and got["nbinned"] == 0 and got["nvalues"] == 100
    assert all(np.isnan(got[f]) for f in FIELDS)


def test_grid_refusals():
    ok = dict(N=100, mean=0.0, sd=1.0, min_=-2.0, max_=2.0, q25=-0.6, q75=0.6)
    E.debug_density2d_grid(**ok)
    S = E.Density2dSpec
    for spec in (S(adjust=0.0), S(adjust=-1.0), S(adjust=np.inf), S(adjust=np.nan), S(clip=(0.5, 0.5)), S(clip=(-0.1, 0.9)),
                 S(clip=(0.1, 1.1)), S(clip=(0.9, 0.1)), S(bw=[0.0]), S(bw=[-1.0]), S(bw=[np.inf]), S(from_=[3.0]), S(to=[-3.0]),
                 S(from_=[1.0], to=[0.5])):
        with pytest.raises(McxError):
            E.debug_density2d_grid(spec=spec, **ok)
    with pytest.raises(McxError):
        E.debug_density2d_grid(**dict(ok, N=1))


# ---- the refusals of a call, before a device is touched ---------------------------------------------------------------------
def test_rows_refusals_need_no_device():
    """these raise MCX_ERR_INVALID (1), not MCX_ERR_NO_DEVICE, on a machine without a device"""
    rows = np.zeros((8, 3), np.float32)
    for kw in (dict(g=7), dict(g=65), dict(g=0), dict(adjust=0.0), dict(adjust=np.nan), dict(clip=(0.6, 0.4)), dict(clip=(0.0, 1.5)),
               dict(bw=[1.0, 0.0, np.nan]), dict(bw=[-2.0, np.nan, np.nan]), dict(from_=[np.nan, 2.0, 0.0], to=[np.nan, 1.0, 0.0]),
               dict(from_=[np.inf, np.nan, np.nan]), dict(pairs=[(1, 1)]), dict(pairs=[(0, 1), (2, 2)]), dict(pairs=[(0, 3)]),
               dict(pairs=[(-1, 0)]), dict(pairs=[(3, 0)]), dict(pairs=np.zeros((0, 2), np.int32)),
               dict(pairs=[(0, 1)] * 1025)):
        with pytest.raises(McxError) as ei:
            E.rows_density2d(rows, 4, 2, **kw)
        assert ei.value.code == 1, kw
    with pytest.raises(McxError) as ei:  # N = 1
        E.rows_density2d(rows[:1], 1, 1)
    assert ei.value.code == 1
    with pytest.raises(ValueError):  # one entry per column
        E.rows_density2d(rows, 4, 2, bw=[1.0])


def test_default_pairs_of_more_than_45_columns_are_refused():
    rows = np.zeros((4, 47), np.float32)  # 47 columns: 1081 pairs
    with pytest.raises(McxError) as ei:
        E.rows_density2d(rows, 2, 2)
    assert ei.value.code == 1 and "name the pairs" in str(ei.value)
    rows = np.zeros((4, 46), np.float32)  # 46 columns: 1035 pairs
    with pytest.raises(McxError) as ei:
        E.rows_density2d(rows, 2, 2)
    assert ei.value.code == 1 and "name the pairs" in str(ei.value)


def test_two_to_the_31_rows_are_unsupported():
    rows = np.zeros((4, 3), np.float32)  # (refused on nsteps * nc before a row is read)
    with pytest.raises(McxError) as ei:
        E.rows_density2d(rows, 1 << 20, 1 << 11)
    assert ei.value.code == 4


def test_bins_refusals_need_no_device():
    rows = np.zeros((8, 3), np.float32)
    lo, up = np.zeros(3), np.ones(3)
    for kw in (dict(g=7), dict(g=65), dict(g=16, pairs=[(0, 0)]), dict(g=16, pairs=[(0, 3)]), dict(g=16, up=np.zeros(3))):
        kw = dict(dict(lo=lo, up=up), **kw)
        with pytest.raises(McxError) as ei:
            E.debug_rows_density2d_bins(rows, 4, 2, **kw)
        assert ei.value.code == 1, kw


# ---- the finish --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [64, 37, 8])
def test_finish_is_the_model(G):
    a, b = pair("banana", 30000, seed=4)
    ga, gb = D.grid(a, from_=-1.5), D.grid(b, to=4.0)  # both edge slots in use: rows beyond the nodes
    sl = D.slots(a, b, ga["lo"], ga["up"], gb["lo"], gb["up"], G)
    s3 = sl.reshape(G + 1, G + 1, 4)
    assert s3[0, :, 0].sum() > 0 and s3[:, G, 0].sum() > 0 and 0 < int(sl[:, 0].sum()) < a.size
    z = E.debug_density2d_finish(record(ga, a.size), record(gb, a.size), sl, G)
    zr = D.finish(ga, gb, sl, a.size, G)
    assert z.shape == (G, G) and np.abs(z - zr).max() <= 1e-10 * zr.max()
    assert np.all(z >= 0.0)


def test_masses_are_the_bilinear_weights():
    """one row at xpos = (2.25, 5.5) on a grid of delta = 1: its four corners get (1 - fx)(1 - fy), fx (1 - fy), ..."""
    G = 8
    a, b = np.array([2.25, 100.0], np.float32), np.array([5.5, 5.5], np.float32)  # (the second row is off a's grid)
    sl = D.slots(a, b, 0.0, 7.0, 0.0, 7.0, G)
    assert int(sl[:, 0].sum()) == 1 and sl[3 * 9 + 6].tolist() == [1, 1024, 2048, 1024 * 2048]
    m = D.masses(sl, 2, G)
    want = np.zeros((G, G))
    want[2, 5], want[3, 5], want[2, 6], want[3, 6] = 0.75 * 0.5, 0.25 * 0.5, 0.75 * 0.5, 0.25 * 0.5
    assert np.array_equal(m, want / 2.0)


def test_b_a_is_the_transpose():
    """(b, a), summed as the product path sums a pair a > b, is (a, b)'s transpose bit for bit"""
    G = 37
    a, b = pair("gauss", 5000, seed=9)
    ga, gb = D.grid(a), D.grid(b)
    sab = D.slots(a, b, ga["lo"], ga["up"], gb["lo"], gb["up"], G)
    sba = D.slots(b, a, gb["lo"], gb["up"], ga["lo"], ga["up"], G)
    t = sab.reshape(G + 1, G + 1, 4).transpose(1, 0, 2)[..., [0, 2, 1, 3]].reshape(-1, 4)
    assert np.array_equal(sba, t)
    ra, rb = record(ga, a.size), record(gb, a.size)
    zab = E.debug_density2d_finish(ra, rb, sab, G)
    zba = E.debug_density2d_finish(rb, ra, sba, G, b_first=True)
    assert zba.tobytes() == np.ascontiguousarray(zab.T).tobytes()
    # and in the other order of the sums it is the transpose to rounding
    zba0 = E.debug_density2d_finish(rb, ra, sba, G)
    assert np.abs(zba0 - zab.T).max() <= 1e-13 * zab.max()


def test_finish_refusals():
    g = {"bw": 0.5, "from": 0.0, "to": 1.0, "lo": -2.0, "up": 3.0}
    s = np.zeros((81, 4), np.uint64)
    E.debug_density2d_finish(record(g, 10), record(g, 10), s, 8)
    for ra, rb in ((record(dict(g, bw=0.0), 10), record(g, 10)), (record(g, 10), record(dict(g, lo=3.0), 10)),
                   (record(g, 10), record(g, 11)), (record(g, 1), record(g, 1))):
        with pytest.raises(McxError):
            E.debug_density2d_finish(ra, rb, s, 8)
    with pytest.raises(ValueError):
        E.debug_density2d_finish(record(g, 10), record(g, 10), s, 9)


# ---- the model is the estimator it claims to be ---------------------------------------------------------------------------
# The binned estimate against the direct kde2d sum on the same nodes, N = 2000, default bandwidths.  The difference is the
# error of linear binning, a property of the definition of order (delta / h)^2, measured here from the model alone:
#   pair    g   delta / h (a, b)   max |z - direct| / peak
#   gauss   64  0.61, 0.54         0.0111
#   gauss   16  2.56, 2.28         0.0844
#   banana  64  0.61, 1.11         0.0428
#   banana  16  2.56, 4.66         0.646   (the nodes are 4.7 bandwidths apart: 16 nodes do not resolve this kernel)
# The bounds are twice the measured figures.
@pytest.mark.parametrize("kind,G,bound", [("gauss", 64, 0.0222), ("gauss", 16, 0.169), ("banana", 64, 0.0857), ("banana", 16, 1.30)])
def test_model_is_the_direct_kde2d_sum(kind, G, bound):
    a, b = pair(kind)
    ga, gb = D.grid(a), D.grid(b)
    sl = D.slots(a, b, ga["lo"], ga["up"], gb["lo"], gb["up"], G)
    assert int(sl[:, 0].sum()) == a.size
    z, zd = D.finish(ga, gb, sl, a.size, G), D.kde2d_direct(a, b, ga, gb, G)
    err = np.abs(z - zd).max() / zd.max()
    print("%s g = %d: max |z - direct| / peak = %.4g" % (kind, G, err))
    assert err <= bound
    # and the library's finish of the same slots is that model
    zl = E.debug_density2d_finish(record(ga, a.size), record(gb, a.size), sl, G)
    assert np.abs(zl - z).max() <= 1e-10 * z.max()


def test_estimate_integrates_to_one():
    a, b = pair("gauss", 20000, seed=5)
    G = 64
    ga, gb = D.grid(a), D.grid(b)
    sl = D.slots(a, b, ga["lo"], ga["up"], gb["lo"], gb["up"], G)
    z = E.debug_density2d_finish(record(ga, a.size), record(gb, a.size), sl, G)
    cell = ((ga["up"] - ga["lo"]) / (G - 1)) * ((gb["up"] - gb["lo"]) / (G - 1))
    assert abs(z.sum() * cell - 1.0) < 1e-3
