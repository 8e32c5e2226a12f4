"""The step table on the GPU against tests/steptable_ref.py, the definitions restated in float64 numpy.
Every case first asserts, from mcx_debug_steptable_geometry, that its shape lies on the side of the size switch it is there
for.  Tolerances: mean absolute 8 nc 2^-53 max|x| of its (step, column) (a sum of nc terms in any order is off by at most
(nc - 1) 2^-53 sum|x|; 8 covers the division and the tree); sd rtol 1e-9 and quantiles rtol 1e-12 (what
tests/test_gpu_summary.py holds the same numbers to); everything else exactly."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

import chains_ref
import steptable_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAN, INF = float("nan"), float("inf")
PROBS = (0.05, 0.5, 0.95)
EXACT = ("min", "max", "flags", "moved", "ll_max", "ll_max_chain", "step_flags")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_table(a, b):
    return all(same_bits(a[k], b[k]) for k in a)


def same_but_nan(a, b):
    """the same dtype, shape, NaN positions and, elsewhere, bits (a NaN's payload is unspecified)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    n = np.isnan(b)
    return np.array_equal(np.isnan(a), n) and a[~n].tobytes() == b[~n].tobytes()


def make_rows(np_, nc, T, seed=1, stay=0.35):
    """section 16's recipe: normal rows with a log L column; with probability `stay` a chain's row repeats the step before"""
    rng = np.random.default_rng([seed, np_, nc, T])
    a = rng.normal(0.0, 1.0, (T, nc, np_ + 1)).astype(np.float32)
    a[:, :, -1] = -np.abs(a[:, :, -1])
    for t in range(1, T):
        rep = rng.random(nc) < stay
        a[t, rep] = a[t - 1, rep]
    return a.reshape(T * nc, np_ + 1)


def check_table(got, rows, T, nc, probs=PROBS):
    ref = R.table(rows, T, nc, probs)
    ncol = rows.shape[1]
    assert got["mean"].shape == (T, ncol) and got["quantiles"].shape == (T, ncol, len(probs)) and got["moved"].shape == (T,)
    amax = np.abs(rows.reshape(T, nc, ncol).astype(np.float64)).max(axis=1)
    fin = ~np.isnan(ref["mean"])
    assert np.array_equal(~np.isnan(got["mean"]), fin) and np.array_equal(np.isnan(got["sd"]), np.isnan(ref["sd"]))
    if fin.any():
        err, bound = np.abs(got["mean"] - ref["mean"])[fin], (8 * nc * 2.0 ** -53 * amax)[fin]
        print("mean: largest error / bound %.3g" % (err / np.where(bound > 0, bound, 1.0)).max())
        assert (err <= bound).all()
    np.testing.assert_allclose(got["sd"], ref["sd"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(got["quantiles"], ref["quantiles"], rtol=1e-12, atol=0)
    for name in EXACT:
        assert same_but_nan(got[name], ref[name]), (name, got[name], ref[name])
    return ref


# (np, nc, T), nprobs, and what of the geometry the shape is there for
SHAPES = [
    ((1, 1, 1), 3, dict(moments_tile_cols=1, moments_workgroups=2, rows_chunks=1)),     # sd NaN, moved -1, every quantile the value
    ((3, 2, 2), 3, dict(moments_tile_cols=3, moments_stride_chains=85, select_tile_cols=3)),
    ((15, 17, 3), 3, dict(moments_tile_cols=15, moments_col_tiles=1, select_tile_cols=10, select_col_tiles=2)),
    ((16, 17, 3), 3, dict(moments_tile_cols=16, moments_col_tiles=1, moments_stride_chains=16)),
    ((17, 17, 3), 3, dict(moments_col_tiles=2, moments_workgroups=9)),                  # a second parameter tile of one column
    ((16, 15, 3), 3, dict(moments_stride_chains=16)),                                   # nc one short of a stride of 16 columns
    ((16, 16, 3), 3, dict(moments_stride_chains=16)),
    ((2, 255, 2), 3, dict(moments_stride_chains=128, rows_chunks=4)),                   # the log L tile's stride of 256
    ((2, 256, 2), 3, dict(rows_chunks=4)),
    ((2, 257, 2), 3, dict(rows_chunks=5)),
    ((40, 5, 4), 3, dict(rows_lanes_per_chain=64, rows_values_per_lane=1, moments_col_tiles=3)),
    ((256, 3, 3), 3, dict(rows_values_per_lane=5, moments_col_tiles=16)),
    ((64, 5, 3), 3, dict(rows_values_per_lane=2)),
    ((128, 3, 2), 1, dict(rows_values_per_lane=3)),
    ((192, 3, 2), 1, dict(rows_values_per_lane=4)),
    ((2, 1000, 2), 3, dict(rows_chunks=16, moments_stride_chains=128)),                 # many strides per lane
    ((40, 133, 2), 3, dict(rows_chains_per_pass=4, rows_chunks=32)),                    # 34 passes over 32 chunks: a second round
    ((10, 26, 2), 3, dict(select_tile_cols=10, select_col_tiles=1, select_stride_chains=25)),  # the select's narrower tile ...
    ((11, 25, 2), 3, dict(select_tile_cols=10, select_col_tiles=2)),                    # ... and its second tile of one column
    ((16, 9, 2), 1, dict(select_tile_cols=16, select_col_tiles=1, select_lds_bytes=33 * 1024)),
    ((16, 9, 2), 2, dict(select_tile_cols=15, select_col_tiles=2)),
    ((3, 40, 2), 8, dict(select_slots=16, select_tile_cols=3, select_col_tiles=1, select_lds_bytes=49 * 1024)),
    ((4, 40, 2), 8, dict(select_tile_cols=3, select_col_tiles=2)),
    ((5, 300, 3), 0, dict(select_workgroups=0, select_lds_bytes=0)),                    # no select launch, quantiles NULL
]


@pytest.mark.parametrize("shape,nprobs,geo", SHAPES, ids=["%dx%dx%d-q%d" % (s + (n,)) for s, n, _ in SHAPES])
def test_table_against_the_restatement(shape, nprobs, geo):
    from mcpar_amd import engine as E
    np_, nc, T = shape
    g = E.debug_steptable_geometry(np_, T, nc, nprobs)
    assert {k: g[k] for k in geo} == geo
    probs = tuple(np.linspace(0.0, 1.0, nprobs + 2)[1:-1]) if nprobs != 3 else PROBS
    rows = make_rows(np_, nc, T)
    got = E.rows_step_table(rows, T, nc, probs)
    ref = check_table(got, rows, T, nc, probs)
    if nc == 1:
        assert np.isnan(got["sd"]).all() and got["moved"].tolist() == [-1] * T
        assert (got["quantiles"] == rows.reshape(T, np_ + 1).astype(np.float64)[:, :, None]).all()
    assert got["moved"][0] == -1
    if T > 1 and nc >= 15:
        assert (0 < ref["moved"][1:]).all() and (ref["moved"][1:] < nc).all()  # the rows both move and stay
    assert same_table(got, E.rows_step_table(rows, T, nc, probs))  # the same arguments, the same bytes


def test_the_ends_and_unsorted_probabilities():
    from mcpar_amd import engine as E
    np_, nc, T = 3, 37, 3
    rows = make_rows(np_, nc, T, seed=4)
    probs = (1.0, 0.0, 0.5, 0.5, 1.0 / 3.0, 0.999)
    got = E.rows_step_table(rows, T, nc, probs)
    check_table(got, rows, T, nc, probs)
    assert same_bits(got["quantiles"][:, :, 0], got["max"].astype(np.float64))
    assert same_bits(got["quantiles"][:, :, 1], got["min"].astype(np.float64))
    assert same_bits(got["quantiles"][:, :, 2], got["quantiles"][:, :, 3])


def test_radix_select_digits():
    """a column whose values share the top 24 key bits (the last digit decides), one of two values that differ in sign alone"""
    from mcpar_amd import engine as E
    np_, nc, T = 3, 256, 2
    rng = np.random.default_rng(8)
    a = make_rows(np_, nc, T, seed=8).reshape(T, nc, np_ + 1).copy()
    for t in range(T):
        a[t, :, 0] = (np.uint32(0x3f800000) + rng.permutation(256).astype(np.uint32)).view(np.float32)   # 1 + i 2^-23
        a[t, :, 1] = np.where(rng.random(nc) < 0.4, np.float32(-1.5), np.float32(1.5))
        a[t, :, 3] = -(np.uint32(0x41000000) + rng.integers(0, 256, nc).astype(np.uint32)).view(np.float32)  # log L, with ties
    rows = a.reshape(T * nc, np_ + 1)
    probs = (0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 0.996, 1.0)
    got = E.rows_step_table(rows, T, nc, probs)
    ref = check_table(got, rows, T, nc, probs)
    assert same_bits(got["quantiles"][:, 0], ref["quantiles"][:, 0])  # the same two neighbours, 2^-23 apart, and the same formula
    assert set(np.unique(got["quantiles"][:, 1])) <= {-1.5, 1.5}


@pytest.mark.parametrize("np_", [3, 4])
def test_targets_in_sixteen_top_bytes(np_):
    """nprobs = 8 and nc = 16: the 16 target ranks are the 16 values, each in a top key byte of its own -- the most distinct
    prefixes a column can have, from the second digit on"""
    from mcpar_amd import engine as E
    nc, T = 16, 2
    g = E.debug_steptable_geometry(np_, T, nc, 8)
    assert g["select_slots"] == 16 and g["select_tile_cols"] == 3 and g["select_col_tiles"] == (1 if np_ == 3 else 2)
    mags = 2.0 ** np.arange(-40, 40, 10, dtype=np.float64)          # 8 exponents 10 apart: 8 top bytes per sign
    vals = np.concatenate([-mags, mags]).astype(np.float32)
    keys = chains_ref.order_key(vals.view(np.uint32))
    assert np.unique(keys >> 24).size == 16
    rng = np.random.default_rng(5)
    a = np.empty((T, nc, np_ + 1), np.float32)
    for t in range(T):
        for c in range(np_ + 1):
            a[t, :, c] = vals[rng.permutation(nc)] * np.float32(1.0 + 0.25 * c)   # (the same exponents, other mantissas)
    rows = a.reshape(T * nc, np_ + 1)
    probs = tuple((2 * k + 0.5) / 15.0 for k in range(8))           # lo = 2 k, lo + 1 = 2 k + 1: every rank is a target
    got = E.rows_step_table(rows, T, nc, probs)
    check_table(got, rows, T, nc, probs)


def test_constant_column():
    from mcpar_amd import engine as E
    np_, nc, T = 5, 300, 3
    a = make_rows(np_, nc, T, seed=2).reshape(T, nc, np_ + 1).copy()
    a[:, :, 2] = np.float32(0.1)
    a[1, :, 5] = np.float32(-7.25)  # log L of one step: every chain holds the maximum
    rows = a.reshape(T * nc, np_ + 1)
    got = E.rows_step_table(rows, T, nc)
    check_table(got, rows, T, nc)
    assert (got["sd"][:, 2] == 0.0).all() and (got["mean"][:, 2] == np.float64(np.float32(0.1))).all()
    assert (got["quantiles"][:, 2] == np.float64(np.float32(0.1))).all()
    assert got["ll_max"][1] == -7.25 and got["ll_max_chain"][1] == 0 and got["sd"][1, 5] == 0.0


@pytest.mark.parametrize("shape", [(17, 64, 3), (3, 1000, 2)], ids=lambda s: "%dx%dx%d" % s)
def test_offset_data(shape):
    """section 16's 4096 + 2^-6 g: |mean| / sd above 1e5, where a sum of x^2 loses the variance"""
    from mcpar_amd import engine as E
    np_, nc, T = shape
    g = np.random.default_rng(11).standard_normal((T * nc, np_ + 1))
    rows = (4096.0 + 2.0 ** -6 * g).astype(np.float32)
    got = E.rows_step_table(rows, T, nc)
    ref = check_table(got, rows, T, nc)
    assert np.abs(ref["mean"] / ref["sd"]).min() > 1e5


def test_one_inf_touches_its_step_and_column_alone():
    from mcpar_amd import engine as E
    np_, nc, T = 17, 20, 5
    a = make_rows(np_, nc, T, seed=3, stay=0.0).reshape(T, nc, np_ + 1).copy()
    clean = E.rows_step_table(a.reshape(T * nc, np_ + 1), T, nc)
    b = a.copy()
    b[3, 7, 16] = INF
    got = E.rows_step_table(b.reshape(T * nc, np_ + 1), T, nc)
    check_table(got, b.reshape(T * nc, np_ + 1), T, nc)
    m = np.ones((T, np_ + 1), bool)
    m[3, 16] = False
    assert np.isnan(got["mean"][3, 16]) and np.isnan(got["sd"][3, 16]) and got["max"][3, 16] == INF
    for name in ("mean", "sd", "min", "max", "flags", "quantiles"):
        assert same_bits(got[name][m], clean[name][m]), name
    assert got["flags"][3, 16] == 1 and got["flags"].sum() == 1 and got["step_flags"].tolist() == [0, 0, 0, 1, 0]
    for name in ("moved", "ll_max", "ll_max_chain"):
        assert same_bits(got[name], clean[name]), name


def test_log_l_with_a_nan_and_signed_zeros():
    from mcpar_amd import engine as E
    np_, nc, T = 3, 300, 6
    a = make_rows(np_, nc, T, seed=6).reshape(T, nc, np_ + 1).copy()
    a[2, 280, np_] = NAN                                  # a NaN in log L: that step alone
    a[3, :, np_] = -np.abs(a[3, :, np_]) - 1.0
    a[3, 290, np_] = 0.0
    a[3, 5, np_] = -0.0                                   # -0 before +0: chain 290 holds the maximum
    a[4] = a[3]
    a[4, 5, np_] = 0.0                                    # two moves in bits alone: -0 -> +0 ...
    a[4, 290, np_] = -0.0                                 # ... and +0 -> -0; now chain 5 holds the maximum
    a[5] = a[4]
    a[5, 0, 0] = np.array([0x7fc01234], np.uint32).view(np.float32)[0]
    rows = a.reshape(T * nc, np_ + 1)
    got = E.rows_step_table(rows, T, nc)
    check_table(got, rows, T, nc)
    assert np.isnan(got["ll_max"][2]) and got["ll_max_chain"][2] == -1 and got["step_flags"].tolist() == [0, 0, 1, 0, 0, 1]
    assert np.isnan(got["quantiles"][2, np_]).all() and np.isnan(got["min"][2, np_]) and not np.isnan(got["quantiles"][2, :np_]).any()
    assert got["ll_max_chain"][3] == 290 and got["ll_max"][3] == 0.0 and not np.signbit(got["ll_max"][3])
    assert got["moved"][4] == 2 and got["ll_max_chain"][4] == 5
    assert got["moved"][5] == 1
    b = a.copy()
    b[:, 0, 0] = b[5, 0, 0]                               # one NaN pattern repeated is no move of its own
    b[5] = b[4]
    got = E.rows_step_table(b.reshape(T * nc, np_ + 1), T, nc)
    assert got["moved"][5] == 0 and got["flags"][:, 0].all()


def test_against_the_chain_table_and_numpy():
    from mcpar_amd import engine as E
    np_, nc, T = 5, 77, 9
    rows = make_rows(np_, nc, T, seed=12)
    st = E.rows_step_table(rows, T, nc, probs=(0.5,))
    ct = E.rows_chain_table(rows, T, nc)
    assert st["moved"][1:].sum() == ct["moves"].sum() > 0
    assert st["ll_max"].max() == ct["ll_max"].max()
    a = rows.reshape(T, nc, np_ + 1).astype(np.float64)
    np.testing.assert_allclose(st["quantiles"][:, :, 0], np.quantile(a, 0.5, axis=1), rtol=1e-12, atol=0)
    np.testing.assert_allclose(st["mean"], a.mean(axis=1), rtol=0, atol=8 * nc * 2.0 ** -53 * np.abs(a).max())


def test_refusals_allocate_nothing():
    from mcpar_amd import McxError
    from mcpar_amd import engine as E
    nc, T = 7, 6
    rows = make_rows(4, nc, T, seed=5)
    E.rows_step_table(rows, T, nc)
    gc.collect()
    before = E.debug_live_resources()
    for kw, text in ((dict(probs=(0.5, -0.1)), "probs[1] = -0.1"), (dict(probs=(NAN,)), "probs[0] = nan"),
                     (dict(probs=np.linspace(0, 1, 9)), "nprobs = 9")):
        with pytest.raises(McxError) as ei:
            E.rows_step_table(rows, T, nc, **kw)
        assert ei.value.code == 1 and text in str(ei.value)
        assert E.debug_live_resources() == before
    with pytest.raises(McxError) as ei:
        E.rows_step_table(rows, 0, nc)
    assert ei.value.code == 1 and "at least one step" in str(ei.value) and E.debug_live_resources() == before
    st = E.select_chains_rows(rows, T, nc, [1, 2])
    during = E.debug_live_resources()
    with pytest.raises(McxError):
        st.step_table(probs=(2.0,))
    assert E.debug_live_resources() == during
    st.close()
    assert E.debug_live_resources() == before


def test_on_an_engine():
    r = subprocess.run([sys.executable, os.path.join(HERE, "steptable_worker.py")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=120)
    out = r.stdout.decode(errors="replace")
    if r.returncode != 0:
        print(out)
    assert r.returncode == 0, "the step table worker ended with status %d" % r.returncode
    assert "steptable engine: all scenarios done" in out
