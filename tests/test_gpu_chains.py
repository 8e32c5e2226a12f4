"""The chain table and the stores of chosen chains on the GPU against tests/chains_ref.py, the
definitions restated in float64 numpy.  Every case first asserts, from mcx_debug_chains_geometry, that its shape lies on the
side of the size switch it is there for.  Tolerances: mean and sd rtol 1e-9 (what tests/test_gpu_summary.py holds the same two
numbers to); rho1 atol 8 T 2^-53 (sum |c_i c_{i+1}| <= sum c_i^2, so a sequential fp64 sum is off by about T 2^-53 of the
denominator; 8 covers the division and the centring; the device and the restatement centre on the same float64 mean);
everything else exactly."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

import chains_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAN, INF = float("nan"), float("inf")
TABLE_EXACT = ("moves", "longest_stay", "ll_max", "ll_max_step", "flags")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_table(a, b):
    return all(same_bits(a[k], b[k]) for k in a)


def make_rows(np_, nc, T, seed=1, stay=0.35):
    """normal rows with a log L column; with probability `stay` a chain's row repeats the step before (a rejected step)"""
    rng = np.random.default_rng([seed, np_, nc, T])
    a = rng.normal(0.0, 1.0, (T, nc, np_ + 1)).astype(np.float32)
    a[:, :, -1] = -np.abs(a[:, :, -1])
    for t in range(1, T):
        rep = rng.random(nc) < stay
        a[t, rep] = a[t - 1, rep]
    return a.reshape(T * nc, np_ + 1)


def check_table(got, rows, T, nc):
    ref = R.table(rows, T, nc)
    np.testing.assert_allclose(got["mean"], ref["mean"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(got["sd"], ref["sd"], rtol=1e-9, atol=0)
    assert np.array_equal(np.isnan(got["rho1"]), np.isnan(ref["rho1"]))
    if not np.isnan(ref["rho1"]).all():
        err = np.nanmax(np.abs(got["rho1"] - ref["rho1"]))
        print("rho1: max error %.3g of the bound %.3g" % (err, 8 * T * 2.0 ** -53))
        assert err <= 8 * T * 2.0 ** -53
    for name in TABLE_EXACT:
        assert same_bits(got[name], ref[name]) or (name == "ll_max" and np.array_equal(np.isnan(got[name]), np.isnan(ref[name])) and
                                                  np.array_equal(got[name][~np.isnan(ref[name])], ref[name][~np.isnan(ref[name])])), \
            (name, got[name], ref[name])
    return ref


# (np, nc, T) and what of the geometry the shape is there for
SHAPES = [
    ((1, 1, 1), dict(rows_lanes_per_chain=2, series_workgroups=1)),                 # one chain, one step: sd and rho1 NaN
    ((3, 37, 2), dict(rows_lanes_per_chain=4, rows_workgroups=1)),                  # T = 2: one product in rho1
    ((15, 16, 7), dict(series_tile_cols=15, rows_lanes_per_chain=16, rows_workgroups=1)),   # ncol = G = 16, a full workgroup of groups
    ((16, 17, 33), dict(series_tile_cols=16, series_col_tiles=1, series_workgroups=2, rows_lanes_per_chain=32, rows_workgroups=3)),
    ((17, 64, 65), dict(series_col_tiles=2, series_workgroups=8, rows_lanes_per_chain=32, rows_workgroups=8)),
    ((2, 257, 5), dict(series_ll_workgroups=2, series_workgroups=3, rows_lanes_per_chain=4, rows_workgroups=5)),
    ((40, 5, 12), dict(series_col_tiles=3, rows_lanes_per_chain=64, rows_values_per_lane=1)),
    ((256, 3, 9), dict(series_col_tiles=16, rows_values_per_lane=5)),               # the fifth register holds log L alone
    ((31, 9, 5), dict(rows_lanes_per_chain=32, rows_workgroups=2)),                 # ncol = G = 32: the last lane holds log L
    ((32, 5, 5), dict(rows_lanes_per_chain=64, rows_values_per_lane=1, rows_workgroups=2)),  # the first np of a whole wavefront
    ((63, 4, 6), dict(rows_lanes_per_chain=64, rows_values_per_lane=1, rows_workgroups=1)),  # ncol = 64: log L in lane 63
    ((64, 5, 6), dict(rows_values_per_lane=2, rows_workgroups=2)),                  # log L alone in the second register
    ((127, 3, 4), dict(rows_values_per_lane=2)),
    ((128, 3, 4), dict(rows_values_per_lane=3)),
    ((191, 2, 4), dict(rows_values_per_lane=3)),
    ((192, 2, 4), dict(rows_values_per_lane=4)),
    ((255, 2, 3), dict(rows_values_per_lane=4)),
    ((1, 129, 3), dict(rows_lanes_per_chain=2, rows_chains_per_workgroup=128, rows_workgroups=2, series_workgroups=1)),
    ((15, 17, 4), dict(series_tile_chains=17, series_workgroups=1)),                # the last chain of a tile
    ((15, 18, 3), dict(series_tile_chains=17, series_workgroups=2)),                # the first chain of a second tile
]


@pytest.mark.parametrize("shape,geo", SHAPES, ids=["%dx%dx%d" % s for s, _ in SHAPES])
def test_table_against_the_restatement(shape, geo):
    from mcpar_amd import engine as E
    np_, nc, T = shape
    g = E.debug_chains_geometry(np_, T, nc)
    assert {k: g[k] for k in geo} == geo
    rows = make_rows(np_, nc, T)
    got = E.rows_chain_table(rows, T, nc)
    ref = check_table(got, rows, T, nc)
    assert got["mean"].shape == (nc, np_ + 1) and got["moves"].shape == (nc,)
    if T == 1:
        assert np.isnan(got["sd"]).all() and np.isnan(got["rho1"]).all() and got["longest_stay"].tolist() == [1] * nc
    if T > 4:
        assert 0 < ref["moves"].sum() < (T - 1) * nc  # the rows both move and stay
    assert same_table(got, E.rows_chain_table(rows, T, nc))  # the same arguments, the same bytes


@pytest.mark.parametrize("shape", [(17, 64, 65), (3, 37, 33), (2, 5, 1000)], ids=lambda s: "%dx%dx%d" % s)
def test_offset_series(shape):
    """4096 + 2^-6 g: |mean| / sd near 2.6e5, where a sum of x^2 loses the variance (tests/test_chains_cpu.py measures by how
    much); the centred and the shifted forms pass at the same tolerances"""
    from mcpar_amd import engine as E
    np_, nc, T = shape
    g = np.random.default_rng(11).standard_normal((T * nc, np_ + 1))
    rows = (4096.0 + 2.0 ** -6 * g).astype(np.float32)
    got = E.rows_chain_table(rows, T, nc)
    ref = check_table(got, rows, T, nc)
    assert np.abs(ref["mean"] / ref["sd"]).min() > 1e5


def planted(np_, nc=6, T=9, seed=3):
    """rows without repeats, as [T, nc, ncol]"""
    return make_rows(np_, nc, T, seed, stay=0.0).reshape(T, nc, np_ + 1).copy()


@pytest.mark.parametrize("np_", [3, 17, 65])
def test_planted_rows(np_):
    from mcpar_amd import engine as E
    nc, T = 6, 9
    g = E.debug_chains_geometry(np_, T, nc)
    assert g["rows_values_per_lane"] == (2 if np_ == 65 else 1) and g["series_col_tiles"] == (np_ + 15) // 16
    a = planted(np_)
    a[:, 0] = a[0, 0]                                   # chain 0: identical rows
    a[:, 1, :np_] = a[0, 1, :np_]                        # chain 1: changes in log L alone
    a[:, 2] = a[0, 2]
    a[4:, 2, np_ - 1] += 1.0                             # chain 2: one change, in column np - 1 alone
    a[:, 3] = a[0, 3]
    a[::2, 3, 0] = 0.0
    a[1::2, 3, 0] = -0.0                                 # chain 3: -0 / +0 flips in column 0 alone
    a[:, 4] = a[0, 4]
    a[:, 4, np_ - 1] = np.array([0x7fc01234], np.uint32).view(np.float32)[0]  # chain 4: one NaN pattern repeated, nothing else moves
    rows = a.reshape(T * nc, np_ + 1)
    got = E.rows_chain_table(rows, T, nc)
    check_table(got, rows, T, nc)
    assert got["moves"].tolist() == [0, T - 1, 1, T - 1, 0, T - 1]
    assert got["longest_stay"].tolist() == [T, 1, 5, 1, T, 1]
    assert (got["sd"][0] == 0.0).all() and np.isnan(got["rho1"][0]).all() and (got["mean"][0] == a[0, 0].astype(np.float64)).all()
    assert (got["sd"][1, :np_] == 0.0).all() and got["sd"][1, np_] > 0.0
    assert got["flags"].tolist() == [0, 0, 0, 0, 1, 0]
    assert np.isnan(got["mean"][4, np_ - 1]) and np.isnan(got["sd"][4, np_ - 1]) and np.isnan(got["rho1"][4, np_ - 1])
    assert got["mean"][3, 0] == 0.0 and got["sd"][3, 0] == 0.0
    assert got["ll_max_step"][0] == 0 and got["ll_max"][0] == a[0, 0, np_]


def test_one_inf_touches_its_series_and_its_flag_alone():
    from mcpar_amd import engine as E
    np_, nc, T = 17, 20, 9
    a = planted(np_, nc, T)
    clean = E.rows_chain_table(a.reshape(T * nc, np_ + 1), T, nc)
    b = a.copy()
    b[5, 7, 16] = INF
    got = E.rows_chain_table(b.reshape(T * nc, np_ + 1), T, nc)
    check_table(got, b.reshape(T * nc, np_ + 1), T, nc)
    for name in ("mean", "sd", "rho1"):
        assert np.isnan(got[name][7, 16])
        m = np.ones((nc, np_ + 1), bool)
        m[7, 16] = False
        assert same_bits(got[name][m], clean[name][m]), name
    assert got["flags"][7] == 1 and got["flags"].sum() == 1
    for name in ("moves", "longest_stay", "ll_max", "ll_max_step"):
        assert same_bits(got[name], clean[name]), name


def test_log_l_with_a_nan_or_an_inf():
    from mcpar_amd import engine as E
    np_, nc, T = 3, 5, 7
    a = planted(np_, nc, T)
    a[3, 1, np_] = NAN
    a[2, 2, np_] = INF
    a[6, 2, np_] = INF                                   # the first of two holds the maximum
    a[:, 3, np_] = -INF
    a[4, 4, np_] = 0.0
    a[2, 4, np_] = -0.0                                  # -0 before +0
    a[5, 4, np_] = 0.0
    rows = a.reshape(T * nc, np_ + 1)
    got = E.rows_chain_table(rows, T, nc)
    check_table(got, rows, T, nc)
    assert np.isnan(got["ll_max"][1]) and got["ll_max_step"][1] == -1 and got["flags"][1] == 1
    assert got["ll_max"][2] == INF and got["ll_max_step"][2] == 2 and got["flags"][2] == 1
    assert got["ll_max"][3] == -INF and got["ll_max_step"][3] == 0 and got["flags"][3] == 1
    assert got["ll_max"][4] == 0.0 and not np.signbit(got["ll_max"][4]) and got["ll_max_step"][4] == 4 and got["flags"][4] == 0
    assert got["flags"][0] == 0 and got["ll_max"][0] == a[:, 0, np_].max()


# ---- selection -----------------------------------------------------------------------------------------------------------------
def lists(nc):
    return dict(identity=list(range(nc)), reversed=list(range(nc))[::-1], repeats=[2, 2, 0, nc - 1, 2], one=[nc // 2],
                thrice=[(5 * k + 1) % nc for k in range(3 * nc)])


@pytest.mark.parametrize("np_,vec4", [(3, 0), (4, 1)])
@pytest.mark.parametrize("which", ["identity", "reversed", "repeats", "one", "thrice"])
def test_select_rows(np_, vec4, which):
    from mcpar_amd import engine as E
    nc, T = 7, 6
    sel = lists(nc)[which]
    assert E.debug_chains_geometry(np_, T, nc, len(sel))["select_vec4"] == vec4
    rows = make_rows(np_, nc, T, seed=5)
    st = E.select_chains_rows(rows, T, nc, sel)
    assert st.shape == (T, len(sel), np_ + 1)
    got = st.rows()
    want = R.select(rows, T, nc, sel)
    assert same_bits(got, want)
    if which == "identity":
        assert same_bits(got, rows)
    st2 = E.select_chains_rows(rows, T, nc, sel)
    assert same_bits(st2.rows(), got)  # the same arguments, the same bytes
    st2.close()
    # the analyses of the selected store are those of the gathered rows: the same passes on the same shape
    assert same_table(st.chain_table(), E.rows_chain_table(want, T, len(sel)))
    a, b = st.summary(), E.rows_summary(want, T, len(sel))
    assert all(same_bits(a[k], b[k]) for k in a)
    if T * len(sel) >= 2:
        a, b = st.covariance(), E.rows_covariance(want, T, len(sel))
        assert all(same_bits(a[k], b[k]) for k in a)
    st.close()


@pytest.mark.parametrize("np_,vec4", [(8, 1), (6, 0)])
def test_select_over_several_workgroups(np_, vec4):
    from mcpar_amd import engine as E
    nc, T = 40, 9
    sel = np.random.default_rng(2).integers(0, nc, 50)
    g = E.debug_chains_geometry(np_, T, nc, sel.size)
    assert g["select_vec4"] == vec4 and g["select_workgroups"] > 2
    assert g["select_items"] % 256 != 0  # the last workgroup is not full
    rows = make_rows(np_, nc, T, seed=6)
    st = E.select_chains_rows(rows, T, nc, sel)
    assert same_bits(st.rows(), R.select(rows, T, nc, sel))
    again = st.select_chains(np.arange(sel.size)[::-1])  # a store of a store
    assert same_bits(again.rows(), R.select(rows, T, nc, sel[::-1]))
    again.close()
    st.close()


def test_select_refusals_allocate_nothing():
    from mcpar_amd import McxError
    from mcpar_amd import engine as E
    nc, T = 7, 6
    rows = make_rows(4, nc, T, seed=5)
    gc.collect()
    before = E.debug_live_resources()
    for sel, text in (([0, -1], "chains[1] = -1"), ([nc], "chains[0] = %d" % nc), ([], "nsel = 0")):
        with pytest.raises(McxError) as ei:
            E.select_chains_rows(rows, T, nc, sel)
        assert ei.value.code == 1 and text in str(ei.value)
        assert E.debug_live_resources() == before
    st = E.select_chains_rows(rows, T, nc, [1, 2])
    during = E.debug_live_resources()
    assert during[0] == before[0] + 2 and during[2] == before[2] + 1  # x', ly'; its stream
    for sel in ([2], [0, -1]):
        with pytest.raises(McxError) as ei:
            st.select_chains(sel)
        assert ei.value.code == 1 and E.debug_live_resources() == during
    st.close()
    assert E.debug_live_resources() == before


def test_on_an_engine():
    r = subprocess.run([sys.executable, os.path.join(HERE, "chains_worker.py")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=120)
    out = r.stdout.decode(errors="replace")
    if r.returncode != 0:
        print(out)
    assert r.returncode == 0, "the chains worker ended with status %d" % r.returncode
    assert "chains engine: all scenarios done" in out
