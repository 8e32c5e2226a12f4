"""mcx_samples_rank_summary / mcx_rows_rank_summary on the GPU against the float64 restatement of DESIGN.md section 11
(tests/rank_ref.py): the ranks bit for bit and the normal scores within one float ulp on shapes and contents where a radix
sort and a scatter break, the diagnostics with summary_ref.check's tolerances (R-hat 1e-7 absolute, ESS 1e-4 relative,
ess_lag equal), the entry points against each other byte for byte, non-finite and degenerate columns, refusals."""
import math

import numpy as np
import pytest

import oracle_lib as O
import rank_cases as K
import rank_ref as RR
import summary_ref as R

pytestmark = pytest.mark.gpu

ABS_RHAT, REL_ESS, MARGIN = 1e-7, 1e-4, 1e-5  # summary_ref.check's
STATS = {}  # the largest differences seen, printed by the tests that measure them


def same_bytes(a, b):
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def rank_summary(rows, T, nc):
    from mcpar_amd import engine as E
    a = E.rows_rank_summary(rows, T, nc)
    same_bytes(a, E.rows_rank_summary(rows, T, nc))
    return a


def ordered(z):
    """float32 -> integers whose differences count representable floats between two values"""
    i = np.ascontiguousarray(z, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


# ---- 1. ranks exact, z within one float ulp
SHAPES = [(1, 1, 4), (5, 33, 37), (16, 64, 600), (17, 3, 257), (33, 2, 64), (2, 513, 257), (256, 2, 8)]  # np, nc, T
KINDS, content = K.KINDS, K.content  # (shared with tests/test_rank_summary_cpu.py)


@pytest.mark.parametrize("np_,nc,T", SHAPES)
def test_ranks_exact_and_scores_within_an_ulp(np_, nc, T, monkeypatch):
    from mcpar_amd import engine as E
    ncol, N = np_ + 1, T * nc
    rng = np.random.default_rng(1000 + np_ + nc + T)
    if (np_, nc, T) == (17, 3, 257):  # the keys of 4 columns at a time: 5 groups, the last one partial and the log L tile alone
        monkeypatch.setenv("MCX_RANK_GROUP_COLS", "4")
    worst = 0
    for k0 in range(0, len(KINDS), ncol):  # every content in every shape: a narrow shape takes several calls
        cols = [content(KINDS[(k0 + c) % len(KINDS)], T, nc, rng) for c in range(ncol)]
        rows = K.rows_of(cols)
        ref = [RR.transforms(c) for c in cols]
        for what, zk, rk in ((E.RANK_Z, "z", "ranks"), (E.RANK_Z_FOLDED, "z_folded", "ranks_folded")):
            out, ranks = E.debug_rows_rank_transform(rows, T, nc, what, want_ranks=True)
            out, ranks = out.reshape(T, nc, ncol), ranks.reshape(T, nc, ncol)
            for c in range(ncol):
                where = (KINDS[(k0 + c) % len(KINDS)], "column", c, zk)
                assert np.array_equal(ranks[:, :, c], ref[c][rk]), where
                d = np.abs(ordered(out[:, :, c]) - ordered(ref[c][zk])).max()
                worst = max(worst, int(d))
                assert d <= 1, where
        for what, ik in ((E.RANK_I05, "i05"), (E.RANK_I95, "i95")):
            out = E.debug_rows_rank_transform(rows, T, nc, what).reshape(T, nc, ncol)
            for c in range(ncol):
                assert np.array_equal(out[:, :, c], ref[c][ik]), (KINDS[(k0 + c) % len(KINDS)], "column", c, ik)
    STATS["z_ulp"] = max(STATS.get("z_ulp", 0), worst)
    print("largest z difference: %d ulp (N = %d)" % (worst, N))


# ---- 1b. the rank sort past two carries of its scan, and more than 64 steps per workgroup of the sweeps
@pytest.fixture(scope="module")
def big():
    """rank_cases.big_columns() as rows, with the float64 reference of both columns, made once: the average ranks from one
    sort (rank_ref.ranks_by_sort; tests/test_rank_summary_cpu.py holds it equal to rank_ref.ranks and the content to what
    the test below says of it) and the thresholds.  np = 1, nc = 2, T = 2 101 267: the smallest shape past all three size
    switches of mcx_ranks.hip at once."""
    np_, nc, T = K.BIG_SHAPE
    cols = K.big_columns()
    yield dict(T=T, nc=nc, N=T * nc, cols=cols, rows=K.rows_of(cols), ranks=[RR.ranks_by_sort(c) for c in cols],
               thr=[RR.thresholds(c) for c in cols])


def big_geometry(b):
    """the geometry the large case is there for, asserted before any result"""
    from mcpar_amd import engine as E
    g = E.debug_store_geometry(1, 0, b["T"], b["nc"])
    assert g["rank_tiles"] > 2 * 256 and b["N"] % 8192 != 0, g  # a third step of k_rank_scan, a ragged last tile
    assert g["rank_step_chunk"] > 64 and g["rank_grid_y"] == -(-b["T"] // g["rank_step_chunk"]), g
    return g


def test_ranks_past_two_scan_carries_and_a_longer_step_chunk(big, monkeypatch):
    """k_rank_scan, `carry += sh[SB - 1]` at the end of its loop over steps of 256 tiles: 514 tiles are three steps, two full
        and one of two tiles, so the offsets of tiles 256 .. 513 are right only with both carries.  Normal values have every
        low-byte digit in every full tile and their share of each higher digit in every stretch of 256 tiles, so in each of
        the four passes every digit row that holds keys has non-zero counts behind tile 255 and behind tile 511; a wrong
        offset puts keys at wrong places of the sorted column, and a rank is a position in it.
      k_rank_rowsum, `for (i = threadIdx.x; i < nblk; i += SB)`: the same 514 counts, three a thread for threads 0 and 1.
      k_rank_keys / k_rank_transform, `s0 = blockIdx.y * rchunk`: rchunk = 65 here and 64 in every other test.  A step
        left out leaves its key unwritten or its rank and score zero, which is why every value is compared, not a sample.
      The last tile is ragged (38 keys), and tie runs (a value repeats its predecessor in the chain with probability 0.3,
      a rejected step repeating the whole row) lie across tile boundaries: with nc = 2 a run's keys are two apart.
    The average ranks are exact on every value of both columns; the scores are within the one ulp of section 1 on 20 000
    fixed positions (rank_ref.normal_scores is a Python loop over the distinct ranks)."""
    from mcpar_amd import engine as E
    monkeypatch.delenv("MCX_RANK_GROUP_COLS", raising=False)
    g = big_geometry(big)
    T, nc, N = big["T"], big["nc"], big["N"]
    out, ranks = E.debug_rows_rank_transform(big["rows"], T, nc, E.RANK_Z, want_ranks=True)
    pos = np.random.default_rng(5).choice(N, 20000, replace=False)
    worst = 0
    for c, want in enumerate(big["ranks"]):
        assert np.array_equal(ranks[:, c], want), ("ranks, column", c, np.flatnonzero(ranks[:, c] != want)[:8])
        d = np.abs(ordered(out[pos, c]) - ordered(RR.normal_scores(want[pos], N))).max()
        worst = max(worst, int(d))
        assert d <= 1, ("z, column", c)
    print("largest z difference: %d ulp (N = %d, %d tiles, %d steps a workgroup)" % (worst, N, g["rank_tiles"], g["rank_step_chunk"]))


@pytest.mark.parametrize("what, k", [(2, 0), (3, 2)])  # RANK_I05 against q05, RANK_I95 against q95
def test_indicators_with_a_longer_step_chunk(big, what, k):
    """k_rank_transform's indicator branch, `for (s = s0; s < s1; ++s) q[s * t.rs] = p[s * t.rs] <= lim`, with
    s0 = blockIdx.y * rchunk and rchunk = 65: a step left out stays 0 in the transformed store, and about one value in twenty
    (I05) or nineteen in twenty (I95) are 1 everywhere along the chains, so the indicators are exact on every value."""
    from mcpar_amd import engine as E
    big_geometry(big)
    out = E.debug_rows_rank_transform(big["rows"], big["T"], big["nc"], what)
    for c, col in enumerate(big["cols"]):
        want = (col.reshape(-1).astype(np.float64) <= big["thr"][c][k]).astype(np.float32)
        assert 0.04 < want.mean() - (0.0 if k == 0 else 0.9) < 0.06
        assert np.array_equal(out[:, c], want), ("indicator", what, "column", c)


# ---- 2. / 3. diagnostics
def series(T, nc, ncol, kind, seed, phi=0.7, offset=0.0):
    """test_gpu_summary_edges.py's: iid normals, AR(1) or random walks per (chain, column), chains offset by N(0, offset)"""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((T, nc, ncol))
    if kind == "ar":
        for i in range(1, T):
            e[i] += phi * e[i - 1]
    elif kind == "rw":
        e = np.cumsum(e, axis=0)
    return (e + rng.normal(0.0, offset, (nc, ncol)) if offset else e).astype(np.float32)


DIAG = [  # np, nc, T, kind, seed: seeds for which the reference alone clears the guard (checked without a GPU)
    (5, 33, 37, "iid", 31), (16, 64, 600, "ar", 32), (17, 3, 257, "rw", 33), (33, 2, 64, "ar", 34),
    (5, 33, 37, "rw", 35), (17, 3, 257, "iid", 36),
]


def diag_rows(np_, nc, T, kind, seed):
    x = series(T, nc, np_ + 1, kind, seed, offset=0.3 if kind != "rw" else 3.0)
    return np.ascontiguousarray(x.reshape(T * nc, np_ + 1))


def piece(got_rhat, got_ess, got_lag, r, where):
    """one transformed column's R-hat / ESS / lag (None: not reported) against summary_ref.restate_column's dict"""
    if math.isnan(r["rhat"]):  # W = 0
        assert (got_rhat is None or math.isnan(got_rhat)) and (got_ess is None or math.isnan(got_ess)), where
        return
    if got_rhat is not None:
        assert abs(got_rhat - r["rhat"]) < ABS_RHAT, (where, got_rhat, r["rhat"])
    if got_lag is not None:
        assert got_lag == r["ess_lag"], (where, got_lag, r["ess_lag"])
    if got_ess is not None:
        np.testing.assert_allclose(got_ess, r["ess"], rtol=REL_ESS, err_msg=str(where))
        STATS["ess_rel"] = max(STATS.get("ess_rel", 0.0), abs(got_ess - r["ess"]) / r["ess"])
        if r["ess_lag"] < r["n"] - 5:
            assert abs(r["pairs"][-1]) > MARGIN and abs(r["pairs"][-2]) > MARGIN, (where, r["pairs"][-2:])


@pytest.mark.parametrize("np_,nc,T,kind,seed", DIAG[:4])
def test_diagnostics_of_the_devices_own_transform(np_, nc, T, kind, seed):
    """the plumbing alone: the device's transformed rows through summary_ref give the numbers rows_rank_summary reports"""
    from mcpar_amd import engine as E
    rows = diag_rows(np_, nc, T, kind, seed)
    got = rank_summary(rows, T, nc)
    for what, fr, fe, fl in ((E.RANK_Z, "rhat_bulk", "ess_bulk", "ess_bulk_lag"), (E.RANK_Z_FOLDED, "rhat_folded", None, None),
                             (E.RANK_I05, None, "ess_q05", None), (E.RANK_I95, None, "ess_q95", None)):
        ref = R.restate(E.debug_rows_rank_transform(rows, T, nc, what), T, nc, ())
        for c, r in enumerate(ref):
            piece(None if fr is None else got[fr][c], None if fe is None else got[fe][c], None if fl is None else got[fl][c],
                  r, (kind, "column", c, "what", what))
    print("largest ESS relative error so far: %.3g" % STATS.get("ess_rel", 0.0))


@pytest.mark.parametrize("np_,nc,T,kind,seed", DIAG)
def test_end_to_end_against_the_reference(np_, nc, T, kind, seed):
    rows = diag_rows(np_, nc, T, kind, seed)
    RR.check(rank_summary(rows, T, nc), RR.restate(rows, T, nc), stats=STATS)
    print("largest ESS relative error so far: %.3g, R-hat absolute %.3g" % (STATS.get("ess_rel", 0.0), STATS.get("rhat_abs", 0.0)))


def test_demonstration_cases():
    """the two runs the basic summary calls converged, on the GPU's numbers with the thresholds of the CPU test"""
    from mcpar_amd import engine as E
    rows = K.rows_of([K.demo_scale(), K.demo_cauchy()])
    T, nc = K.DEMO_T, K.DEMO_NC
    got, basic = rank_summary(rows, T, nc), E.rows_summary(rows, T, nc, ())
    RR.check(got, RR.restate(rows, T, nc), stats=STATS)
    print("scale: basic rhat %.4f ess %.0f, rhat_folded %.4f ess_tail %.1f | cauchy: basic rhat %.4f ess %.0f, ess_bulk %.1f"
          % (basic["rhat"][0], basic["ess"][0], got["rhat_folded"][0], got["ess_tail"][0], basic["rhat"][1], basic["ess"][1],
             got["ess_bulk"][1]))
    K.check_demo_scale(basic["rhat"][0], basic["ess"][0], got["rhat_folded"][0], got["ess_tail"][0])
    K.check_demo_cauchy(basic["rhat"][1], basic["ess"][1], got["ess_bulk"][1])
    assert got["rhat"][0] == got["rhat_folded"][0] and got["ess_tail"][0] == min(got["ess_q05"][0], got["ess_q95"][0])


# ---- 4. the entry points agree, after real runs
def run(d, n, nburn, nsamp, stride=1):
    import mcpar_amd as M
    from mcpar_amd import engine as E
    vg, keep = M.make_vlfunc(M.VL_ROSENBROCK1, d)
    eg = M.Engine(d, n, pl=1.0)
    if stride > 1:
        eg.set_option(E.OPT_SAMPLE_STRIDE, stride)
    eg.run(nsamp, nburn, O.default_pinit(d, n), vg)
    eg._vl_keep = keep
    return eg


RUNS = {
    "rosen1-16x512": (dict(d=16, n=512, nburn=100, nsamp=200), 0, None),
    "stride-3": (dict(d=16, n=512, nburn=100, nsamp=200, stride=3), 0, None),
    "sub-range": (dict(d=16, n=512, nburn=100, nsamp=200), 37, 101),
    "small-n-8x64": (dict(d=8, n=64, nburn=100, nsamp=200), 0, None),
}


@pytest.mark.parametrize("name", list(RUNS))
def test_entry_points_agree(name):
    from mcpar_amd import engine as E
    cfg, first, nsteps = RUNS[name]
    eg = run(**cfg)
    if nsteps is None:
        nsteps = eg.samples.shape[0] // eg.nc - first
    a = eg.rank_summary(first_step=first, nsteps=nsteps)
    same_bytes(a, eg.rank_summary(first_step=first, nsteps=nsteps))
    rows = eg.samples_range(first, nsteps)
    same_bytes(a, E.rows_rank_summary(rows, nsteps, eg.nc))
    q = eg.summary((0.05, 0.5, 0.95), first_step=first, nsteps=nsteps)["quantiles"]
    for k, f in enumerate(("q05", "median", "q95")):
        assert a[f].tobytes() == np.ascontiguousarray(q[:, k]).tobytes(), f
    assert (a["flags"] == 0).all() and np.isfinite(a["rhat"]).all() and (a["ess_bulk"] > 0).all()
    assert (a["rhat"] >= 0.9).all() and (a["ess_tail"] <= a["ess_q05"]).all()


# ---- 5. non-finite and degenerate columns
def test_nonfinite_columns_are_flagged_and_leave_the_others_alone():
    T, nc, np_ = 61, 9, 5
    rows = diag_rows(np_, nc, T, "ar", 51)
    clean = rank_summary(rows, T, nc)
    bad = rows.copy()
    bad[17 * nc + 4, 2] = np.nan
    bad[::7, np_] = -np.inf  # a log L column of a target with a hard wall
    got = rank_summary(bad, T, nc)
    for c in range(np_ + 1):
        if c in (2, np_):
            assert got["flags"][c] == 1 and got["ess_bulk_lag"][c] == 0, c
            for f in RR.FIELDS:
                assert math.isnan(got[f][c]), (c, f)
        else:
            for f in got:
                assert got[f][c].tobytes() == clean[f][c].tobytes(), (c, f)
    RR.check(got, RR.restate(bad, T, nc))


def test_constant_column_and_a_tied_lower_tail():
    T, nc = 200, 6
    rng = np.random.default_rng(52)
    const = np.full((T, nc), -7.25, np.float32)
    tied = rng.standard_normal((T, nc)).astype(np.float32)
    tied[tied < np.quantile(tied, 0.10)] = np.float32(-1.5)  # the lowest 10 % are one value: q05 is that value
    tied[tied < -1.5] = np.float32(-1.5)
    frozen = np.repeat(rng.standard_normal((1, nc)).astype(np.float32), T, axis=0)  # every chain constant, chains differ
    rows = K.rows_of([const, tied, frozen, rng.standard_normal((T, nc))])
    got = rank_summary(rows, T, nc)
    ref = RR.restate(rows, T, nc)
    assert ref[1]["q05"] == -1.5 and abs(RR.transforms(tied)["i05"].mean() - 0.10) < 0.02  # I05 = (x <= q05) takes the whole tie
    assert not math.isnan(ref[1]["ess_q05"])
    RR.check(got, ref)
    for c in (0, 2):
        assert got["flags"][c] == 0
        for f in ("rhat", "rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "ess_q05", "ess_q95"):
            assert math.isnan(got[f][c]), (c, f)
    assert got["median"][0] == -7.25 and got["q05"][0] == -7.25


# ---- 6. refusals
def test_refusals():
    import mcpar_amd as M
    from mcpar_amd import engine as E
    eg = M.Engine(4, 64)
    with pytest.raises(M.McxError) as ei:  # no run yet
        eg.rank_summary()
    assert ei.value.code == 1
    vg, keep = M.make_vlfunc(M.VL_ROSENBROCK1, 4)
    eg.run(20, 10, O.default_pinit(4, 64), vg)
    for kw in (dict(first_step=0, nsteps=3), dict(first_step=0, nsteps=21), dict(first_step=17, nsteps=4),
               dict(first_step=-1, nsteps=8)):
        with pytest.raises(M.McxError) as ei:
            eg.rank_summary(**kw)
        assert ei.value.code == 1, kw
    assert eg.rank_summary()["rhat"].shape == (5,)
    eg.set_sink(lambda first, nsteps, rows: 0, 5)
    eg.run(20, 0, O.default_pinit(4, 64), vg)
    with pytest.raises(M.McxError) as ei:  # a run into a sink leaves no store
        eg.rank_summary()
    assert ei.value.code == 1
    with pytest.raises(M.McxError) as ei:
        E.rows_rank_summary(np.zeros((6, 3), np.float32), 3, 2)
    assert ei.value.code == 1


# ---- the driver: --rank-summary writes the struct's fields, and moves nothing else
def test_driver_rank_summary(tmp_path):
    import os
    import subprocess
    from mcpar_amd import engine as E
    drv = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mcpar_amd", "drivers", "mcpar-run")
    args = [drv, "--func", "gauss", "--np", "4", "--nc", "256", "--nsamp", "201", "--nburn", "100", "--binary"]
    a = subprocess.run(args + ["--out", "rows.bin", "--summary", "s.txt", "--rank-summary", "r.txt"], cwd=tmp_path,
                       capture_output=True, timeout=300)
    assert a.returncode == 0, a.stderr.decode()
    os.rename(tmp_path / "rows.bin", tmp_path / "rows_r.bin")
    os.rename(tmp_path / "s.txt", tmp_path / "s_r.txt")
    b = subprocess.run(args + ["--out", "rows.bin", "--summary", "s.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert b.returncode == 0, b.stderr.decode()
    assert a.stdout == b.stdout
    assert (tmp_path / "rows_r.bin").read_bytes() == (tmp_path / "rows.bin").read_bytes()
    assert (tmp_path / "s_r.txt").read_bytes() == (tmp_path / "s.txt").read_bytes()
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, 5)
    got = E.rows_rank_summary(rows, 201, 256)
    lines = (tmp_path / "r.txt").read_text().splitlines()
    names = ["rhat", "rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "ess_q05", "ess_q95", "q05", "median", "q95"]
    assert lines[0].split() == ["name"] + names[:7] + ["q05", "q50", "q95", "ess_bulk_lag", "flags"]
    assert [ln.split()[0] for ln in lines[1:]] == ["p0", "p1", "p2", "p3", "LL"]
    for c, ln in enumerate(lines[1:]):
        t = ln.split()[1:]
        assert [float(v) for v in t[:10]] == [got[f][c] for f in names]  # %.17g round-trips a double
        assert [int(v) for v in t[10:]] == [got["ess_bulk_lag"][c], got["flags"][c]]
    c = subprocess.run(args[:-1] + ["--stream-text", "--rank-summary", "r2.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert c.returncode == 2 and b"--rank-summary" in c.stderr
