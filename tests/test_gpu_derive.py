"""Derived columns and bootstrap draws of the sample store on the GPU (include/mcx.h).  Every
comparison is on bits (equal NaN patterns count as equal, as in test_gpu_store_view.py): MCX_DERIVE_LINEAR against a numpy
float32 loop of its stated rule, MCX_DERIVE_SOURCE against LINEAR and against numpy, the derived store's three analyses
against the rows_* entry points on its own rows (and against the engine's for the identity map), non-finite outputs, the
store's independence of its engine, the draws against the stated index rule, and the refusals."""
import functools
import os

import numpy as np
import pytest

from test_gpu_store_view import assert_same_bytes, run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (nc, np, T, nout)
SHAPES = {
    "5x3x13-1": (5, 3, 13, 1),          # N = 65, a wavefront and one row; odd everything
    "17x17x16-17": (17, 17, 16, 17),    # N = 272 = 256 + 16; np and nout one past a tile of 16
    "3x256x4-2": (3, 256, 4, 2),        # the widest input row
    "3x2x4-256": (3, 2, 4, 256),        # the widest output row
    "2x256x4-256": (2, 256, 4, 256),    # the largest LDS case, N = 8
    "64x16x8-4": (64, 16, 8, 4),        # N = 512, exactly two full tiles; the aligned 16-byte path
}
PROBS = (0.01, 0.5, 0.99)


@functools.lru_cache(maxsize=None)
def engine(nc, d, T):
    """one short Gaussian run per (nc, np, T), shared: nothing below changes an engine it did not make itself"""
    return run(nc, d, T)


@functools.lru_cache(maxsize=None)
def linear_map(d, nout):
    rng = np.random.default_rng(1000 * d + nout)
    return rng.standard_normal((nout, d)).astype(np.float32), rng.standard_normal(nout).astype(np.float32)


def linear_ref(rows, A, b):
    """acc = b[j], then acc = acc + A[j][k] * x[k] for k in order, the product and the sum each rounded to float32"""
    x = np.ascontiguousarray(rows[:, :-1].T)
    out = np.empty((rows.shape[0], A.shape[0] + 1), np.float32)
    for j in range(A.shape[0]):
        acc = np.full(rows.shape[0], b[j], np.float32)
        for k in range(A.shape[1]):
            acc = acc + A[j, k] * x[k]
        assert acc.dtype == np.float32
        out[:, j] = acc
    out[:, -1] = rows[:, -1]
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    if a.tobytes() == b.tobytes():
        return True
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32)))


def example(name):
    return open(os.path.join(ROOT, "mcpar_amd", "examples", name)).read()


def need_hiprtc():
    import mcpar_amd as M
    if not M.user_source_available():
        why = M.load().mcx_last_error().decode()
        print("MCX_DERIVE_SOURCE cases skipped:", why)
        pytest.skip("no run-time compilation: " + why)


# ---- 1. LINEAR against numpy -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_linear_is_the_numpy_float32_loop(shape):
    import mcpar_amd as M
    nc, d, T, nout = SHAPES[shape]
    eg = engine(nc, d, T)
    A, b = linear_map(d, nout)
    spec = M.derive_linear(A, b)
    rows = eg.samples_range(0, T)
    st = eg.derive(spec)
    assert st.shape == (T, nc, nout + 1)
    got, want = st.rows(), linear_ref(rows, A, b)
    assert same_bits(got, want), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4]
    assert got[:, -1].tobytes() == rows[:, -1].tobytes()  # log L is the engine's
    assert same_bits(st.rows(1, T - 2), want[nc:(T - 1) * nc])  # a range of the derived store
    assert st.rows(T, 0).shape == (0, nout + 1)
    # a sub-range of the engine's store that does not start at step 0 (np odd: not 16-byte aligned either)
    first, nsteps = 1, T - 2
    sub = eg.derive(spec, first_step=first, nsteps=nsteps)
    assert sub.shape == (nsteps, nc, nout + 1)
    assert same_bits(sub.rows(), want[first * nc:(first + nsteps) * nc])
    # the same store and arguments give the same bytes; host rows go the same way
    assert eg.derive(spec).rows().tobytes() == got.tobytes()
    assert M.derive_rows(rows, T, nc, spec).rows().tobytes() == got.tobytes()
    for s in (st, sub):
        s.close()


# ---- 2. SOURCE against LINEAR and numpy ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["5x3x13-1", "17x17x16-17", "2x256x4-256"])
def test_source_restating_linear_gives_its_bytes(shape):
    import mcpar_amd as M
    need_hiprtc()
    nc, d, T, nout = SHAPES[shape]
    eg = engine(nc, d, T)
    A, b = linear_map(d, nout)
    lin = eg.derive(M.derive_linear(A, b)).rows()
    src = eg.derive(M.derive_source(example("derive_linear.hip"), nout, np.concatenate([A.reshape(-1), b]))).rows()
    assert src.tobytes() == lin.tobytes()
    sub = eg.derive(M.derive_source(example("derive_linear.hip"), nout, np.concatenate([A.reshape(-1), b])), first_step=1, nsteps=2)
    assert sub.rows().tobytes() == lin[nc:3 * nc].tobytes()


def contrast_ref(rows, shift, nout):
    x, d = rows[:, :-1], rows.shape[1] - 1
    out = np.empty((rows.shape[0], nout + 1), np.float32)
    a, z = x[:, 0], x[:, d - 1]
    out[:, 0] = (a - z) + np.float32(shift)
    if nout > 1:
        out[:, 1] = np.abs(a * z)
    if nout > 2:
        out[:, 2] = rows[:, -1]
    for j in range(3, nout):
        out[:, j] = x[:, j % d] * x[:, j % d]
    out[:, -1] = rows[:, -1]
    return out


@pytest.mark.parametrize("shape, nout", [("5x3x13-1", 3), ("17x17x16-17", 3), ("17x17x16-17", 20), ("64x16x8-4", 2)])
def test_nonlinear_source_is_numpy_float32(shape, nout):
    import mcpar_amd as M
    need_hiprtc()
    nc, d, T, _ = SHAPES[shape]
    eg = engine(nc, d, T)
    rows = eg.samples_range(0, T)
    st = eg.derive(M.derive_source(example("derive_contrast.hip"), nout, [0.25]))
    got, want = st.rows(), contrast_ref(rows, 0.25, nout)
    assert same_bits(got, want), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4]
    if nout > 2:
        assert got[:, 2].tobytes() == rows[:, -1].tobytes()  # the output that is ly


# ---- 3. the third way to a view ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["5x3x13-1", "17x17x16-17"])
def test_store_analyses_are_the_rows_analyses(shape):
    import mcpar_amd as M
    from mcpar_amd import engine as E
    nc, d, T, nout = SHAPES[shape]
    eg = engine(nc, d, T)
    A, b = linear_map(d, nout)
    st = eg.derive(M.derive_linear(A, b))
    rows = st.rows()
    assert_same_bytes(st.summary(PROBS), E.rows_summary(rows, T, nc, PROBS), "summary")
    assert_same_bytes(st.rank_summary(), E.rows_rank_summary(rows, T, nc), "rank_summary")
    assert_same_bytes(st.covariance(), E.rows_covariance(rows, T, nc), "covariance")
    # the identity map on a store of finite, non-zero values: the engine's own analyses of the same range
    raw = eg.samples_range(0, T)
    assert np.all(np.isfinite(raw)) and np.all(raw != 0)
    first, nsteps = 2, T - 3
    ident = eg.derive(M.derive_linear(np.eye(d, dtype=np.float32), np.zeros(d, np.float32)), first_step=first, nsteps=nsteps)
    assert ident.rows().tobytes() == eg.samples_range(first, nsteps).tobytes()
    assert_same_bytes(ident.summary(PROBS), eg.summary(PROBS, first_step=first, nsteps=nsteps), "identity summary")
    assert_same_bytes(ident.rank_summary(), eg.rank_summary(first_step=first, nsteps=nsteps), "identity rank_summary")
    assert_same_bytes(ident.covariance(), eg.covariance(first_step=first, nsteps=nsteps), "identity covariance")


# ---- 3b. the tile heights below 256 rows -------------------------------------------------------------------------------------
# (np, nout) -> R = derive_rows(np, nout), the rows a workgroup takes.  The shapes above have R = 256, or R = 32 / 16 with
# fewer rows than one tile.  (20, 19) | (20, 21): the two sides of the LDS budget's edge, (20, 19) using all 40 960 bytes
TILES = {(20, 19): 256, (20, 21): 128, (40, 17): 128, (17, 40): 128, (100, 3): 64, (3, 100): 64, (256, 2): 32, (2, 256): 32,
         (256, 256): 16}


def host_rows(N, d, seed):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((N, d + 1)).astype(np.float32)
    rows[:, -1] = -np.abs(rows[:, -1])
    return rows


@pytest.mark.parametrize("full", [False, True])  # N = 2 R + 5: a third, ragged workgroup; N = 2 R: two full tiles exactly
@pytest.mark.parametrize("d, nout", sorted(TILES))
def test_tile_heights_linear_is_the_numpy_float32_loop(d, nout, full):
    """derive_body's `os = derive_lds + R * sx`, `row0 = blockIdx.x * R`, `mine = tid < rows` and the two
    derive_tile_copy calls with R < 256: lanes R .. 255 have no row but copy, the second workgroup's tiles start at row R
    of x and x', and the last one is ragged.  A workgroup that read or wrote at a stride of 256 rows, or an output tile
    placed for another R, changes rows R .. N - 1, which the bit-for-bit comparison with the numpy loop shows."""
    import mcpar_amd as M
    R_ = TILES[(d, nout)]
    N = 2 * R_ + (0 if full else 5)
    g = M.debug_store_geometry(d, nout, N, 1)
    assert g["derive_rows"] == R_ and g["derive_workgroups"] == (2 if full else 3), g
    assert (g["derive_lds_bytes"] == 40960) == ((d, nout) == (20, 19)), g
    A, b = linear_map(d, nout)
    rows = host_rows(N, d, 7 * d + nout)
    st = M.derive_rows(rows, N, 1, M.derive_linear(A, b))
    assert st.shape == (N, 1, nout + 1)
    got, want = st.rows(), linear_ref(rows, A, b)
    assert same_bits(got, want), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4]
    st.close()


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("d, nout", sorted(TILES))
def test_tile_heights_source_restating_linear(d, nout, full):
    """the same shapes through the run-time build, which gets np and nout as constants: a different kernel per shape, held
    to LINEAR's bytes (which the test above holds to the numpy loop's)"""
    import mcpar_amd as M
    need_hiprtc()
    R_ = TILES[(d, nout)]
    N = 2 * R_ + (0 if full else 5)
    g = M.debug_store_geometry(d, nout, N, 1)
    assert g["derive_rows"] == R_ and g["derive_workgroups"] == (2 if full else 3), g
    A, b = linear_map(d, nout)
    rows = host_rows(N, d, 7 * d + nout)
    lin = M.derive_rows(rows, N, 1, M.derive_linear(A, b))
    src = M.derive_rows(rows, N, 1, M.derive_source(example("derive_linear.hip"), nout, np.concatenate([A.reshape(-1), b])))
    assert src.shape == (N, 1, nout + 1) and src.rows().tobytes() == lin.rows().tobytes()
    lin.close()
    src.close()


@pytest.mark.parametrize("d, nc, nout, R_", [(41, 7, 17, 128), (101, 3, 3, 64), (255, 3, 2, 32)])
def test_tile_heights_from_an_unaligned_store(d, nc, nout, R_):
    """derive_body's `((unsigned long)gx & 15ul) == 0`: steps [1, T) of an engine's store with nc * np odd start off a
    16-byte boundary, so derive_tile_copy<true> takes its 4-byte path at this tile height; the same steps given as host rows
    are uploaded to a fresh allocation and take the 16-byte path.  Both give the numpy loop's bits."""
    import mcpar_amd as M
    T = 2 + (2 * R_ + nc) // nc
    ns = T - 1
    g = M.debug_store_geometry(d, nout, ns, nc)
    assert g["derive_rows"] == R_ and g["derive_workgroups"] >= 3 and (nc * d * 4) % 16 != 0, g
    eg = engine(nc, d, T)
    A, b = linear_map(d, nout)
    spec = M.derive_linear(A, b)
    rows = eg.samples_range(1, ns)
    want = linear_ref(rows, A, b)
    for st in (eg.derive(spec, first_step=1, nsteps=ns), M.derive_rows(rows, ns, nc, spec)):
        assert st.shape == (ns, nc, nout + 1)
        got = st.rows()
        assert same_bits(got, want), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4]
        st.close()


def test_store_analyses_at_a_reduced_tile_height():
    """a store written by workgroups of 64 rows is a store like any other: its summary and covariance are those of its rows"""
    import mcpar_amd as M
    from mcpar_amd import engine as E
    d, nout, T, nc = 100, 3, 19, 7
    g = M.debug_store_geometry(d, nout, T, nc)
    assert g["derive_rows"] == 64 and g["derive_workgroups"] == 3, g
    rows = host_rows(T * nc, d, 64)
    st = M.derive_rows(rows, T, nc, M.derive_linear(*linear_map(d, nout)))
    out = st.rows()
    assert same_bits(out, linear_ref(rows, *linear_map(d, nout)))
    assert_same_bytes(st.summary(PROBS), E.rows_summary(out, T, nc, PROBS), "summary")
    assert_same_bytes(st.covariance(), E.rows_covariance(out, T, nc), "covariance")
    st.close()


# ---- 4. non-finite outputs -------------------------------------------------------------------------------------------------
PLANT = """
// par = (on, x0 of the row that gets par[3] in output 1, x0 of the row that gets par[4] in output 2, NaN, -inf)
__device__ void mcx_user_derive(const float *x, int d, float ly, const float *par, float *out, int nout)
{
  out[0] = x[0] - x[d - 1];
  out[1] = x[0] * x[1];
  out[2] = x[1] + x[d - 1];
  if (par[0] != 0.0f && x[0] == par[1]) out[1] = par[3];
  if (par[0] != 0.0f && x[0] == par[2]) out[2] = par[4];
}
"""


def test_nonfinite_outputs_flag_their_columns_only():
    import mcpar_amd as M
    from mcpar_amd import engine as E
    need_hiprtc()
    nc, d, T, _ = SHAPES["17x17x16-17"]
    eg = engine(nc, d, T)
    rows = eg.samples_range(0, T)
    ra, rb = 3 * nc + 5, 11 * nc + 2
    xa, xb = rows[ra, 0], rows[rb, 0]
    assert xa != xb
    par = np.array([1.0, xa, xb, np.nan, -np.inf], np.float32)
    off = par.copy()
    off[0] = 0.0
    clean, bad = eg.derive(M.derive_source(PLANT, 3, off)), eg.derive(M.derive_source(PLANT, 3, par))
    rc, rbad = clean.rows(), bad.rows()
    assert np.all(np.isfinite(rc))
    hit1, hit2 = rows[:, 0] == xa, rows[:, 0] == xb  # (a rejected step repeats its row: every copy is hit)
    assert hit1[ra] and hit2[rb]
    assert np.all(np.isnan(rbad[hit1, 1])) and np.all(rbad[hit2, 2] == -np.inf)
    keep = np.ones_like(rbad, bool)
    keep[hit1, 1] = False
    keep[hit2, 2] = False
    assert rbad[keep].tobytes() == rc[keep].tobytes()
    s0, s1 = clean.summary(PROBS), bad.summary(PROBS)
    r0, r1 = clean.rank_summary(), bad.rank_summary()
    c0, c1 = clean.covariance(), bad.covariance()
    assert list(s1["flags"]) == [0, E.SUMMARY_NONFINITE, E.SUMMARY_NONFINITE, 0]
    assert list(r1["flags"]) == list(s1["flags"]) and list(c1["flags"]) == list(s1["flags"])
    assert not s0["flags"].any() and not r0["flags"].any() and not c0["flags"].any()
    for name in ("mean", "sd", "rhat", "ess", "mcse_mean"):
        assert np.all(np.isnan(s1[name][1:3])), name
    assert np.isnan(s1["min"][1]) and np.isnan(s1["max"][1]) and np.all(np.isnan(s1["quantiles"][1]))
    assert s1["min"][2] == -np.inf and np.isfinite(s1["max"][2])
    for name in ("rhat", "rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "q05", "median", "q95"):
        assert np.all(np.isnan(r1[name][1:3])), name
    assert np.all(np.isnan(c1["mean"][1:3])) and np.all(np.isnan(c1["cov"][1:3, :])) and np.all(np.isnan(c1["cov"][:, 1:3]))
    fine = [0, 3]  # column 0 and log L: what they are without the planted values
    for a, b, what in ((s0, s1, "summary"), (r0, r1, "rank_summary")):
        assert_same_bytes({k: np.asarray(v)[fine] for k, v in a.items()}, {k: np.asarray(v)[fine] for k, v in b.items()}, what)
    assert c0["mean"][fine].tobytes() == c1["mean"][fine].tobytes()
    assert c0["cov"][np.ix_(fine, fine)].tobytes() == c1["cov"][np.ix_(fine, fine)].tobytes()


# ---- 5. independence of the engine ---------------------------------------------------------------------------------------
def test_store_outlives_its_engine():
    import mcpar_amd as M
    import oracle_lib as O
    nc, d, T, nout = SHAPES["17x17x16-17"]
    eg = run(nc, d, T)  # its own engine: it is run again and destroyed
    A, b = linear_map(d, nout)
    st = eg.derive(M.derive_linear(A, b))
    rows, summ = st.rows(), st.summary(PROBS)
    before = eg.samples_range(0, T)
    vg, keep = M.make_vlfunc(M.VL_GAUSSIAN, d, None)
    eg.run(T, 7, O.default_pinit(d, nc) * np.float32(0.5), vg)
    assert eg.samples_range(0, T).tobytes() != before.tobytes()  # the engine's store has moved on
    assert st.rows().tobytes() == rows.tobytes()
    eg.close()
    assert st.rows().tobytes() == rows.tobytes()
    assert_same_bytes(st.summary(PROBS), summ, "summary after mcx_destroy")
    st.close()
    st.close()  # closing twice is harmless


# ---- 6. draws ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["5x3x13-1", "17x17x16-17"])
@pytest.mark.parametrize("n", [1, 1000])
def test_draws_follow_the_index_rule(shape, n):
    import mcpar_amd as M
    nc, d, T, nout = SHAPES[shape]
    eg = engine(nc, d, T)
    seed, first, nsteps = 4242, 2, T - 3
    rng_rows = eg.samples_range(first, nsteps)
    rows, index = eg.draw(n, seed, first_step=first, nsteps=nsteps)
    want = M.debug_draw_indices(seed, nsteps * nc, 0, n)
    assert index.dtype == np.int64 and np.array_equal(index, want)
    assert rows.tobytes() == rng_rows[index].tobytes()
    if n == 1000:
        assert len(np.unique(index)) < n and index.min() >= 0 and index.max() < nsteps * nc  # with replacement
        assert not np.array_equal(eg.draw(n, seed + 1, first_step=first, nsteps=nsteps)[1], index)
    A, b = linear_map(d, nout)
    st = eg.derive(M.derive_linear(A, b), first_step=first, nsteps=nsteps)
    drows, dindex = st.draw(n, seed)
    assert np.array_equal(dindex, index)
    assert same_bits(drows, linear_ref(rows, A, b))  # the derived draws are f of the draws


def test_gather_in_several_chunks(monkeypatch):
    """the copy to the host goes through one device buffer in chunks (64 MiB; MCX_GATHER_CHUNK_ROWS makes them small): rows
    and indices of every chunk land at their own place, for the draws and for DerivedStore.rows"""
    import mcpar_amd as M
    nc, d, T, nout = SHAPES["17x17x16-17"]
    eg = engine(nc, d, T)
    A, b = linear_map(d, nout)
    st = eg.derive(M.derive_linear(A, b))
    whole = (eg.draw(1000, 99), st.draw(1000, 99), st.rows(), st.rows(3, 9))
    for chunk in (1, 100, 256, 999):  # one row a chunk; not a multiple of the workgroup; exactly one; a last chunk of one
        monkeypatch.setenv("MCX_GATHER_CHUNK_ROWS", str(chunk))
        parts = (eg.draw(1000, 99), st.draw(1000, 99), st.rows(), st.rows(3, 9))
        monkeypatch.delenv("MCX_GATHER_CHUNK_ROWS")
        for (r0, i0), (r1, i1) in zip(whole[:2], parts[:2]):
            assert np.array_equal(i0, i1) and r0.tobytes() == r1.tobytes(), chunk
        assert whole[2].tobytes() == parts[2].tobytes() and whole[3].tobytes() == parts[3].tobytes(), chunk
    rng_rows = eg.samples_range(0, T)
    assert whole[0][0].tobytes() == rng_rows[whole[0][1]].tobytes()
    assert np.array_equal(whole[0][1], M.debug_draw_indices(99, T * nc, 0, 1000))


def test_draw_edges():
    import mcpar_amd as M
    nc, d, T, nout = SHAPES["5x3x13-1"]
    eg = engine(nc, d, T)
    st = eg.derive(M.derive_linear(*linear_map(d, nout)))
    for rows, index in (eg.draw(0, 1), st.draw(0, 1)):
        assert rows.shape[0] == 0 and index.shape == (0,)
    for call in (lambda: eg.draw(-1, 1), lambda: st.draw(-1, 1)):
        with pytest.raises(M.McxError) as ei:
            call()
        assert ei.value.code == 1 and "ndraw" in str(ei.value)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals():
    import mcpar_amd as M
    nc, d, T, nout = SHAPES["5x3x13-1"]
    eg = engine(nc, d, T)
    fresh = M.Engine(d, nc, pl=1.0)
    spec = M.derive_linear(*linear_map(d, nout))
    cases = ((eg, dict(first_step=-1, nsteps=8), "not in the sample store"),
             (eg, dict(first_step=T - 7, nsteps=8), "not in the sample store"),
             (fresh, dict(first_step=0, nsteps=8), "the sample store is empty"))
    for e, kw, text in cases:
        for call in (lambda: e.derive(spec, **kw), lambda: e.draw(3, 1, **kw)):
            with pytest.raises(M.McxError) as ei:
                call()
            assert ei.value.code == 1 and text in str(ei.value), (kw, str(ei.value))
    eg.derive(spec, first_step=T - 8, nsteps=8)  # the last range that is in the store
    with pytest.raises(M.McxError) as ei:
        eg.derive(spec, first_step=0, nsteps=0)
    assert ei.value.code == 1 and "nsteps" in str(ei.value)
    short = eg.derive(spec, first_step=0, nsteps=3)
    for call in (short.summary, short.rank_summary):
        with pytest.raises(M.McxError) as ei:
            call()
        assert ei.value.code == 1 and "needs nsteps >= 4" in str(ei.value)
    short.covariance()  # N = 15 >= 2
    with pytest.raises(M.McxError) as ei:
        short.rows(2, 2)
    assert ei.value.code == 1 and "not in the derived store" in str(ei.value)
    wide = np.zeros((4, 258), np.float32)
    with pytest.raises(M.McxError) as ei:
        M.derive_rows(wide, 4, 1, M.derive_linear(np.ones((1, 257), np.float32), np.zeros(1, np.float32)))
    assert ei.value.code == 1 and "np = 257" in str(ei.value)
