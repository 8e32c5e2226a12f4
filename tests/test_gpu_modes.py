"""mcx_samples_modes on the GPU against tests/modes_ref.py.

What is held:
  one pass   (debug_modes_assign) labels and the winner's d2 bit for bit the restatement's: the distance is vector fp64 in a
             stated order without fused multiply-add; n_k exactly; S_k within (n_k + 16) 2^-53 sum |u_ij| of the fsum
  planted    a row between two centres goes to the lower index; identical centres; NaN / inf rows get MODE_NONE and leave no
             trace; a constant column takes no part; a far centre stays empty, keeps its place and sets the flag
  the loop   on the shapes tests/test_modes_cpu.py shows to be decisive: labels, iters, n_changed, flags exactly the
             reference's; centres, means, sds, inertia, ll_mean within a relative 1e-9, entry by entry; ll_max and ll_max_row
             exactly
  many tiles more than 1024 tiles, so that a workgroup takes several: one pass at np = 1 (scalar centre loads) and np = 160 (32-row
             tiles, centres per lane), and the table with the best log L tied across a workgroup's tiles and across workgroups
  integers   visits, hops, dominant, first_label, last_label, trans, occupancy: numpy on the returned labels
  rows       .rows(k) is rows[labels == k] in source order with its indices; the indicator means are the weights
  bytes      two calls, the engine and rows_modes of its copied rows, and a derived store of them give the same bytes
The launch geometry is asserted where a size switches it."""
import ctypes as C
import math

import numpy as np
import pytest

import modes_ref as R
from test_gpu_store_view import run

pytestmark = pytest.mark.gpu

CACHE = {}
RTOL = 1e-9


def case(shape):
    """(rows, the modes of the rows), made once"""
    if shape not in CACHE:
        np_, nc, T, K = shape
        CACHE[shape] = R.make_rows(np_, nc, T, K, seed=100 + np_)
    return CACHE[shape]


def check_pass(rows, T, nc, c, s, where):
    from mcpar_amd import engine as E
    lab, d2, n, S = E.debug_modes_assign(rows, T, nc, c, s)
    rl, rd, rn, rS, _ = R.assign(rows, c, s)
    assert np.array_equal(lab, rl), (where, np.flatnonzero(lab != rl)[:8])
    assert np.array_equal(d2, rd, equal_nan=True), (where, np.flatnonzero(d2 != rd)[:8])
    assert np.array_equal(n, rn), (where, n, rn)
    bound = (rn[:, None] + 16) * R.EPS * R.sum_abs(rows, rl, s, len(c))
    err = np.abs(S - rS)
    ratio = float((err / np.where(bound == 0, 1, bound)).max())
    assert (err <= bound).all(), (where, ratio)
    return lab, ratio


# ---- one pass -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("np_", [1, 15, 16, 17, 64, 256])
def test_one_pass_equals_the_restatement(np_):
    from mcpar_amd import engine as E
    rng = np.random.default_rng(np_)
    Rt = E.debug_modes_geometry(np_, 1, 1, 1)["rows_per_tile"]
    worst = 0.0
    for K in (1, 2, 32):
        for N in (Rt - 1, Rt, Rt + 1):
            g = E.debug_modes_geometry(np_, 1, N, K)
            assert g["tiles"] == (2 if N > Rt else 1) and g["centre_blocks"] == (K + 7) // 8
            rows = (rng.normal(size=(N, np_ + 1)) * 3).astype(np.float32)
            c = rng.normal(size=(K, np_)) * 2
            s = 1.0 / rng.uniform(0.5, 4.0, size=np_)
            _, ratio = check_pass(rows, 1, N, c, s, (np_, K, N))
            worst = max(worst, ratio)
    print("np = %d: largest |S - fsum| / bound %.3g" % (np_, worst))


def test_one_pass_with_257_chains_and_many_tiles():
    rng = np.random.default_rng(257)
    nc, T, np_, K = 257, 9, 5, 7
    rows = (rng.normal(size=(T * nc, np_ + 1)) * 2).astype(np.float32)
    lab, _ = check_pass(rows, T, nc, rng.normal(size=(K, np_)), np.ones(np_), "257 chains")
    assert len(set(lab.tolist())) == K


# ---- more than 1024 tiles: a workgroup takes several --------------------------------------------------------------------------
BIG_N = 2 * 1024 * 256 + 257  # np = 1: 2050 tiles of 256 rows, the last of one row; workgroups 0 and 1 take three tiles, the others two


def big_rows(np_, N, K, seed, sd=1.0):
    """N rows of K well separated clumps (10 apart along every column, of spread sd), the clump of a row at random; log L random"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, K, size=N)
    rows = np.empty((N, np_ + 1), np.float32)
    rows[:, :np_] = sd * rng.normal(size=(N, np_)) + 10.0 * k[:, None]
    rows[:, np_] = -rng.random(N)
    return rows, k


@pytest.mark.parametrize("np_, N, K", [(1, BIG_N, 3), (160, 32 * 1024 + 32 + 1, 9)], ids=["np1", "np160"])
def test_one_pass_over_more_tiles_than_workgroups(np_, N, K):
    from mcpar_amd import engine as E
    g = E.debug_modes_geometry(np_, 1, N, K)
    assert g["workgroups"] == 1024 and g["tiles"] == -(-N // g["rows_per_tile"]) > 1024 + 1 and g["uniform_centres"] == (np_ == 1)
    rows, k = big_rows(np_, N, K, seed=np_)
    rows[[5, N // 2, N - 1], 0] = [np.nan, np.inf, -np.inf]  # a first, a middle and the last tile hold a row that is not finite
    c = 10.0 * np.arange(K)[:, None] * np.ones(np_) + np.random.default_rng(9).normal(size=(K, np_))
    s = np.full(np_, 0.5)
    lab, ratio = check_pass(rows, 1, N, c * s, s, (np_, K, N))
    ok = lab != E.MODE_NONE
    assert (~ok).sum() == 3 and (lab[ok] == k[ok]).mean() > 0.99
    print("np = %d, N = %d: largest |S - fsum| / bound %.3g" % (np_, N, ratio))


def test_table_over_more_tiles_than_workgroups_with_ties_in_the_best_log_l():
    """np = 1, 2050 tiles: the largest log L of a mode planted twice.  Mode 0: in tiles 5 and 1029, both workgroup 5's, which
    keeps the first; mode 1: in tiles 700 and 1030, workgroups 700 and 6, which the host merges by the smaller row; mode 2: twice
    in tile 2048, workgroup 0's third."""
    from mcpar_amd import engine as E
    N, K, nc = BIG_N, 3, 5
    assert N % nc == 0
    rows, k = big_rows(1, N, K, seed=3, sd=0.5)  # (20 spreads between two clumps: the labels are the clumps)

    def plant(mode, places):
        out = []
        for tile, nth in places:
            r = tile * 256 + np.flatnonzero(k[tile * 256:(tile + 1) * 256] == mode)[nth]
            rows[r, 1] = np.float32(0.5 + mode)
            out.append(int(r))
        return min(out)

    first = [plant(0, [(1029, 0), (5, 3)]), plant(1, [(1030, 1), (700, 2)]), plant(2, [(2048, 4), (2048, 1)])]
    centres = np.array([[0.0], [10.0], [20.0]])
    with E.rows_modes(rows, N // nc, nc, K, centres=centres, scale=False) as m:
        ref = R.lloyd(rows, centres, np.ones(1))
        assert min(ref["margins"]) >= 1e-9 and ref["flags"] == R.CONVERGED
        assert np.array_equal(m.labels(), ref["labels"]) and np.array_equal(ref["labels"], k)
        assert (m.result["iters"], m.result["flags"], m.result["n_changed"]) == (ref["iters"], ref["flags"], 0)
        tab = check_table(m, rows, ref, "2050 tiles")
        assert tab["ll_max_row"].tolist() == first and m.table["ll_max"].tolist() == [0.5, 1.5, 2.5]
        ct, rc = m.chain_table(), R.chain_table(ref["labels"], N // nc, nc, K)
        assert all(np.array_equal(ct[f], rc[f]) for f in rc)


# ---- planted rows ---------------------------------------------------------------------------------------------------------------
def test_planted_rows():
    from mcpar_amd import engine as E
    # integer data, centres at -1 and +1, a row at 0: the lower index; then two identical centres
    rows = np.array([[0, 5], [-1, 1], [1, 2], [0, 3], [2, 4], [-3, 0]], np.float32)
    lab, d2, n, S = E.debug_modes_assign(rows, 6, 1, [[-1.0], [1.0]], [1.0])
    assert lab.tolist() == [0, 0, 1, 0, 1, 0] and d2.tolist() == [1, 0, 0, 1, 1, 4] and n.tolist() == [4, 2] and S.ravel().tolist() == [-4, 3]
    lab, _, n, _ = E.debug_modes_assign(rows, 6, 1, [[1.0], [-1.0]], [1.0])
    assert lab.tolist() == [0, 1, 0, 0, 0, 1]
    lab, _, n, S = E.debug_modes_assign(rows, 6, 1, [[1.0], [1.0], [-5.0]], [1.0])
    assert lab.tolist() == [0, 0, 0, 0, 0, 2] and n.tolist() == [5, 0, 1] and S.ravel().tolist() == [2, 0, -3]
    # a NaN or an inf in the first or the last column: MODE_NONE and no trace in any sum
    rng = np.random.default_rng(3)
    base = rng.normal(size=(600, 4)).astype(np.float32)
    base[:300, 0] += 8
    bad = base.copy()
    where = [0, 255, 256, 599]
    bad[0, 0], bad[255, 2], bad[256, 0], bad[599, 2] = np.nan, np.inf, -np.inf, np.nan
    c = np.array([[8.0, 0, 0], [0.0, 0, 0]])
    lab, d2, n, S = E.debug_modes_assign(bad, 600, 1, c, np.ones(3))
    lab0, d20, n0, S0 = E.debug_modes_assign(np.delete(base, where, 0), 596, 1, c, np.ones(3))
    assert (lab[where] == E.MODE_NONE).all() and np.isnan(d2[where]).all() and np.array_equal(np.delete(lab, where), lab0)
    assert np.array_equal(n, n0) and n.sum() == 596 and np.array_equal(np.delete(d2, where), d20)
    rl, _, rn, rS, _ = R.assign(bad, c, np.ones(3))
    assert np.array_equal(lab, rl) and (np.abs(S - rS) <= (rn[:, None] + 16) * R.EPS * R.sum_abs(bad, rl, np.ones(3), 2)).all()
    # a column with s = 0 takes no part whatever the centres hold there (the restatement skips it)
    cz = np.array([[8.0, 1e9, 0.5], [0.0, -3.0, -0.5], [4.0, 7.0, 0.0]])
    check_pass(base, 600, 1, cz, np.array([1.0, 0.0, 0.5]), "a column without scale")
    # a NaN in log L is no reason: the row is labelled
    ll = base.copy()
    ll[5, 3] = np.nan
    assert E.debug_modes_assign(ll, 600, 1, c, np.ones(3))[0][5] != E.MODE_NONE
    # the whole call: the rows are counted, the weights are of the finite rows, the constant column takes no part
    bad[:, 1] = np.float32(2.5)
    with E.rows_modes(bad, 150, 4, 2, centres=[[8.0, 2.5, 0], [0.0, -7, 0]]) as m:
        assert m.result["n_nonfinite"] == 4 and m.result["n"] == 600 and m.result["flags"] == E.MODES_CONVERGED | E.MODES_EMPTY
        # (columns 0 and 2 hold an inf or NaN: section 9's sd is NaN, they take no part either, and nothing is left to tell rows apart)
        assert m.scale.tolist() == [0, 0, 0] and m.table["n"].tolist() == [596, 0]
    fin = np.delete(bad, where, 0)
    with E.rows_modes(fin, 149, 4, 2, centres=[[8.0, 2.5, 0], [0.0, -7, 0]]) as m:
        assert m.scale[1] == 0 and (m.scale[[0, 2]] > 0).all() and np.isnan(m.centres[:, 1]).all() and np.isnan(m.table["sd"][:, 1]).all()
        assert m.table["n"].tolist() == [297, 299] and m.table["weight"].tolist() == [297 / 596, 299 / 596]
        assert np.array_equal(m.labels(), R.lloyd(fin, np.array([[8.0, 2.5, 0], [0.0, -7, 0]]) * m.scale, m.scale)["labels"])
    # a caller's centre far from every row: an empty cluster that keeps its centre, with the flag
    far = [[8.0, 2.5, 0], [0.0, 2.5, 0], [1e6, 2.5, -1e6]]
    with E.rows_modes(fin, 149, 4, 3, centres=far, scale=False) as m:
        assert m.result["flags"] == E.MODES_CONVERGED | E.MODES_EMPTY and m.table["n"].tolist() == [297, 299, 0]
        assert m.centres[2].tolist() == far[2] and m.table["flags"].tolist() == [0, 0, E.MODES_EMPTY]
        assert np.isnan(m.table["mean"][2]).all() and np.isnan(m.table["ll_mean"][2]) and m.table["ll_max_row"][2] == -1
        assert m.table["weight"].tolist() == [297 / 596, 299 / 596, 0.0]


# ---- the loop -------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    """the largest |a - b| / |b|, entry by entry; equal entries (two zeros among them) and NaN in both count as 0"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(np.isnan(b) | (a == b), 0.0, np.abs(a - b) / np.abs(b))
    return float(np.max(r)) if r.size else 0.0


def check_table(m, rows, ref, where=""):
    """a Modes against the reference's labels and centres (a modes_ref.lloyd dict) and the table made of them"""
    s, res = m.scale, m.result
    tab = R.table(rows, ref["labels"], ref["centres"], s)
    with np.errstate(invalid="ignore", divide="ignore"):
        unscaled = np.where(s == 0, np.nan, ref["centres"] / s)
    worst = {"centres_scaled": rel(m.centres_scaled, ref["centres"]), "centres": rel(m.centres, unscaled),
             "mean": rel(m.table["mean"], tab["mean"]), "sd": rel(m.table["sd"], tab["sd"]),
             "inertia": rel(m.table["inertia"], tab["inertia"]), "ll_mean": rel(m.table["ll_mean"], tab["ll_mean"]),
             "total inertia": rel(res["inertia"], math.fsum(tab["inertia"][tab["n"] > 0]))}
    print("%s %d passes; largest relative differences %s" % (where, res["iters"], {k: "%.2g" % v for k, v in worst.items()}))
    assert max(worst.values()) <= RTOL, (where, worst)
    assert np.array_equal(m.table["n"], tab["n"]) and np.array_equal(m.table["weight"], tab["n"] / (len(rows) - ref["n_nonfinite"]))
    assert np.array_equal(m.table["ll_max"], tab["ll_max"], equal_nan=True) and np.array_equal(m.table["ll_max_row"], tab["ll_max_row"])
    return tab


def check_modes(m, rows, K, max_iter=50, where=""):
    """a Modes against the reference loop from the same seeds, with the scale the call returned"""
    s = m.scale
    assert rel(s, R.scale_of(rows)) <= 1e-12, where  # (section 9's sd against the two-pass float64 one)
    idx = R.seed(rows, K, 11, s)
    ref = R.lloyd(rows, R.scaled(rows, s)[idx], s, max_iter)
    lab = m.labels()
    assert np.array_equal(lab, ref["labels"]), (where, int((lab != ref["labels"]).sum()))
    res = m.result
    assert (res["k"], res["iters"], res["n_changed"], res["flags"], res["n"], res["n_nonfinite"]) == \
        (K, ref["iters"], ref["n_changed"], ref["flags"], len(rows), ref["n_nonfinite"]), (where, res)
    check_table(m, rows, ref, where)
    return ref


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_loop_equals_the_reference(shape):
    from mcpar_amd import engine as E
    np_, nc, T, K = shape
    rows, _ = case(shape)
    with E.rows_modes(rows, T, nc, K, seed=11) as m:
        ref = check_modes(m, rows, K, where=str(shape))
        assert ref["flags"] == R.CONVERGED
        # at convergence the mean of a mode's members is its centre
        assert rel(m.table["mean"], m.centres) <= RTOL
    with E.rows_modes(rows, T, nc, K, seed=11, max_iter=1) as m:
        one = check_modes(m, rows, K, max_iter=1, where=str(shape) + " one pass")
        assert one["flags"] == R.NOT_CONVERGED and m.result["iters"] == 1 and m.result["n_changed"] == T * nc
        # the centres are those the labels are the argmin of: the seeds
        assert np.array_equal(m.labels(), R.assign(rows, m.centres_scaled, m.scale)[0])


def test_the_loop_without_scale_and_with_given_centres():
    from mcpar_amd import engine as E
    shape = R.SHAPES[1]
    np_, nc, T, K = shape
    rows, _ = case(shape)
    with E.rows_modes(rows, T, nc, K, seed=11, scale=False) as m:
        assert m.scale.tolist() == [1.0] * np_ and np.array_equal(m.centres, m.centres_scaled)
        idx = R.seed(rows, K, 11, np.ones(np_))
        ref = R.lloyd(rows, rows[idx, :np_].astype(np.float64), np.ones(np_))
        assert np.array_equal(m.labels(), ref["labels"]) and m.result["iters"] == ref["iters"]
        c0 = rows[idx, :np_].astype(np.float64)
    with E.rows_modes(rows, T, nc, K, centres=c0, scale=False) as m2:
        assert np.array_equal(m2.labels(), ref["labels"]) and m2.centres.tobytes() == m.centres.tobytes()
    # a seed sample smaller than the range: the rows of section 12's draw
    with E.rows_modes(rows, T, nc, K, seed=5, seed_rows=200) as m3:
        s = m3.scale
        sample = rows[E.debug_draw_indices(5, len(rows), 0, 200)]
        idx = R.seed(sample, K, 5, s)
        ref3 = R.lloyd(rows, R.scaled(sample, s)[idx], s)  # (decisive: tests/test_modes_cpu.py holds this very input to the margin)
        assert np.array_equal(m3.labels(), ref3["labels"]) and m3.result["iters"] == ref3["iters"] and m3.result["flags"] == ref3["flags"]
        check_table(m3, rows, ref3, "a seed sample of 200 rows")


# ---- chains and steps -----------------------------------------------------------------------------------------------------------
def check_chain_table(m, T, nc, K):
    lab = m.labels()
    got, ref = m.chain_table(), R.chain_table(lab, T, nc, K)
    for name in ("visits", "hops", "dominant", "dominant_steps", "first_label", "last_label", "trans", "occupancy"):
        assert np.array_equal(got[name], ref[name]), (name, got[name], ref[name])
    L = lab.reshape(T, nc)
    valid = L != R.NONE
    assert got["trans"].sum() == (T - 1) * nc - int((~(valid[1:] & valid[:-1])).sum()) if T > 1 else got["trans"].sum() == 0
    assert np.array_equal(got["occupancy"].sum(1) + (~valid).sum(1), np.full(T, nc))
    assert np.array_equal(got["visits"].sum(0), got["occupancy"].sum(0))
    return got


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[2], R.SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
def test_chains_and_steps_are_numpy_on_the_labels(shape):
    from mcpar_amd import engine as E
    np_, nc, T, K = shape
    rows, _ = case(shape)
    with E.rows_modes(rows, T, nc, K, seed=11) as m:
        got = check_chain_table(m, T, nc, K)
        assert got["hops"].sum() > 0 and got["hops"].sum() == got["trans"].sum() - np.trace(got["trans"])


def test_chains_and_steps_with_invalid_labels_one_step_and_257_chains():
    from mcpar_amd import engine as E
    rng = np.random.default_rng(8)
    nc, T = 257, 6
    rows = rng.normal(size=(T * nc, 3)).astype(np.float32)
    rows[rng.random(T * nc) < 0.5, 0] += 9
    rows[rng.choice(T * nc, 60, replace=False), 1] = np.nan
    rows[np.arange(T) * nc + 3, 0] = np.inf  # a chain without one valid label
    with E.rows_modes(rows, T, nc, 2, centres=[[9.0, 0], [0.0, 0]], scale=False) as m:
        got = check_chain_table(m, T, nc, 2)
        assert got["dominant"][3] == E.MODE_NONE and got["dominant_steps"][3] == 0 and got["first_label"][3] == E.MODE_NONE
        assert m.result["n_nonfinite"] == (m.labels() == E.MODE_NONE).sum() >= 60
    with E.rows_modes(rows[:nc], 1, nc, 2, centres=[[9.0, 0], [0.0, 0]], scale=False) as m:  # T = 1
        got = check_chain_table(m, 1, nc, 2)
        assert got["trans"].sum() == 0 and got["hops"].sum() == 0 and np.array_equal(got["first_label"], got["last_label"])


# ---- rows and indicators --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [R.SHAPES[1], R.SHAPES[4], R.SHAPES[5]], ids=lambda s: "x".join(map(str, s)))
def test_rows_of_a_mode_and_the_indicators(shape):
    from mcpar_amd import engine as E
    np_, nc, T, K = shape
    rows, _ = case(shape)
    with E.rows_modes(rows, T, nc, K, seed=11) as m:
        lab = m.labels()
        total = 0
        for k in range(K):
            rs = m.rows(k)
            pick = np.flatnonzero(lab == k)
            assert rs.nrows == len(pick) == m.table["n"][k] and rs.nsource == T * nc
            assert np.array_equal(rs.index(), pick) and rs.rows().tobytes() == rows[pick].tobytes()
            total += rs.nrows
            if k == 0 and rs.nrows >= 2:
                # the analyses of one mode work as they are: the covariance of its rows, through a store of them
                st = rs.store(nc=1)
                a, b = st.covariance(), E.rows_covariance(rows[pick], len(pick), 1)
                assert all(np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes() for f in a)
                st.close()
            rs.close()
        assert total == T * nc - m.result["n_nonfinite"]
        ind = m.indicators()
        x = ind.rows()
        assert ind.shape == (T, nc, K + 1) and (x[:, K] == 0).all()
        assert np.array_equal(x[:, :K], (lab[:, None] == np.arange(K)[None, :]).astype(np.float32))
        ind.close()
        if T >= 4:
            w = m.weights()
            assert np.array_equal(w["mean"], m.table["weight"]) and abs(w["mean"].sum() - 1) < 1e-12
            assert all(w[f].shape == (K,) for f in ("sd", "mcse_mean", "rhat", "ess"))
        # a source of another shape is refused, and a mode that is none of the handle's
        h = C.c_void_p()
        assert m._source(m.h, K, C.byref(h)) == 1 and b"not a mode of the handle" in E.load().mcx_last_error()
        assert E.load().mcx_rows_mode_rows(E._fp(rows), T + 1, nc, np_, m.h, 0, C.byref(h)) == 1
        assert b"but the labels are of" in E.load().mcx_last_error() and not h.value


def test_rows_with_labels_that_are_none():
    from mcpar_amd import engine as E
    rng = np.random.default_rng(2)
    rows = rng.normal(size=(700, 3)).astype(np.float32)
    rows[::2, 0] += 9
    rows[[0, 1, 350, 699], 1] = np.nan
    with E.rows_modes(rows, 70, 10, 2, centres=[[9.0, 0], [0.0, 0]], scale=False) as m:
        lab = m.labels()
        n = 0
        for k in range(2):
            rs = m.rows(k)
            assert np.array_equal(rs.index(), np.flatnonzero(lab == k)) and rs.rows().tobytes() == rows[lab == k].tobytes()
            n += rs.nrows
            rs.close()
        assert n == 696 and m.result["n_nonfinite"] == 4
        ind = m.indicators().rows()
        assert (ind[[0, 1, 350, 699]] == 0).all() and ind[:, :2].sum() == 696


# ---- bytes ----------------------------------------------------------------------------------------------------------------------
def same_modes(a, b):
    if a.result != b.result or not np.array_equal(a.labels(), b.labels()):
        return False
    pairs = [(a.centres, b.centres), (a.centres_scaled, b.centres_scaled), (a.scale, b.scale)] + [(a.table[f], b.table[f]) for f in a.table]
    pairs += [(x, y) for x, y in zip(a.chain_table().values(), b.chain_table().values())]
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in pairs)


def test_the_three_owners_and_a_second_call_give_the_same_bytes():
    from mcpar_amd import engine as E
    eg = run(37, 17, 30)
    first, nsteps, K = 3, 24, 3
    rows = eg.samples_range(first, nsteps)
    on_engine = eg.modes(K, first_step=first, nsteps=nsteps, seed=4)
    assert on_engine.result["n"] == nsteps * eg.nc and on_engine.table["n"].sum() == nsteps * eg.nc
    assert np.array_equal(on_engine.labels(), R.assign(rows, on_engine.centres_scaled, on_engine.scale)[0])
    again = eg.modes(K, first_step=first, nsteps=nsteps, seed=4)
    on_rows = E.rows_modes(rows, nsteps, eg.nc, K, seed=4)
    st = E.select_chains_rows(rows, nsteps, eg.nc, list(range(eg.nc)))
    on_store = st.modes(K, seed=4)
    for other in (again, on_rows, on_store):
        assert same_modes(on_engine, other)
    for k in range(K):
        a, b, c = on_engine.rows(k), on_rows.rows(k), on_store.rows(k)
        assert a.rows().tobytes() == b.rows().tobytes() == c.rows().tobytes() == rows[on_engine.labels() == k].tobytes()
        assert np.array_equal(a.index(), b.index()) and np.array_equal(a.index(), c.index())
        for r in (a, b, c):
            r.close()
    # another seed gives other centres to start from; the labels of the first handle are untouched by the later calls
    before = on_engine.labels().copy()
    other = eg.modes(K, first_step=first, nsteps=nsteps, seed=5, max_iter=1)
    assert not np.array_equal(other.centres, on_engine.centres) and np.array_equal(on_engine.labels(), before)
    import mcpar_amd as M
    for bad in (0, 33, 1 << 30):  # (the timed form sizes its tables before it checks k: a wild k is refused all the same)
        with pytest.raises(M.McxError) as ei:
            eg.modes_times(bad, first_step=first, nsteps=nsteps)
        assert ei.value.code == 1 and "1 to 32 modes" in str(ei.value)
    ms, res = eg.modes_times(K, first_step=first, nsteps=nsteps, seed=4)
    assert ms.shape == (8,) and (ms >= 0).all() and ms[7] > 0 and ms[2] > 0 and ms[4] > 0 and res == on_engine.result
    for m in (on_engine, again, on_rows, on_store, other):
        m.close()
    st.close()
    eg.close()
