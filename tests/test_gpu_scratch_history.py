"""No analysis of a sample store depends on what its scratch held before the call (DESIGN.md "Scratch and its history").

An engine's analyses share three grow-only buffers, a store's analyses three of their own, and everything allocated per call
holds whatever the allocator hands out.  Every region must therefore be zeroed or written in full by the call that reads it.
Three situations, one table of analyses (table() below, written out), one rule of equality (dtype, shape, NaN positions and
every other byte), one baseline (the rows_* / *_rows result of the same rows with both hooks off):
  1. fresh memory        mcx_debug_fill_allocations: every allocation of a rows_* call or a producer filled with a byte first
  2. persistent scratch  mcx_debug_fill_scratch between two calls of one analysis on six kinds of owner
  3. real residue        every analysis behind every other on one engine and one derived store; every analysis on a whole
                         range and an inner one in both orders on an engine of its own (a regrow in mid-session)
The fill bytes: 0x00, then the residue tests, then 0xFF (all-ones words, NaN doubles, CODE_OFF) and 0x3C (finite, plausible
floats and doubles).  Every engine is created and run before the allocation fill is switched on; a fixture switches it off
behind every test.  No tolerance of its own: the finite baselines are held to the float64 restatements by the check helpers of
the analyses' own test files, at the tolerances those files state in their headers."""
import collections

import numpy as np
import pytest

import chains_ref
import clip_ref
import covariance_ref
import rank_ref
import summary_ref
from test_gpu_chains import check_table as check_chain_table
from test_gpu_density import check_model as check_density
from test_gpu_density2d import check_model as check_density2d
from test_gpu_derive import linear_map, linear_ref
from test_gpu_parse import check_text
from test_gpu_steptable import check_table as check_step_table
from test_gpu_steptable import same_but_nan
from test_gpu_store_view import run

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
FILLS = (0x00, 0xFF, 0x3C)
PROBS, STEP_PROBS = (0.01, 0.5, 0.99), (0.05, 0.5, 0.95)
DENSITY_N, G = 64, 16          # output points of a density (the spec takes 2 to 512); nodes per axis of a pair density
QLO, QHI = 0.02, 0.98          # the clip: about half of 888 rows of 18 columns are kept
SEED, NDRAW = 20240611, 300
ENG_NC, ENG_NP, ENG_STEPS, ENG_FIRST, ENG_INNER = 37, 17, 30, 3, 24  # the engine's store, and the range inside it
CLIP_STORE_NC = 8

# (np, nc, T, non-finite): two parameter column tiles plus the log L tile set, three blocks of 16 chains, N = 888; one tile and
# one block; the first with one NaN in a parameter column and one +inf in log L
VARIANTS = collections.OrderedDict([("17x37x24", (17, 37, 24, False)), ("3x5x8", (3, 5, 8, False)),
                                    ("17x37x24-nonfinite", (17, 37, 24, True))])
FINITE = [k for k, v in VARIANTS.items() if not v[3]]


def make_rows(np_, nc, T, nonfinite, seed=7, stay=0.35):
    """test_gpu_chains.py's recipe -- normal rows, log L below zero, with probability `stay` a chain's row repeats the step
    before -- and ties: column 1 rounded to one decimal"""
    rng = np.random.default_rng([seed, np_, nc, T])
    a = rng.normal(0.0, 1.0, (T, nc, np_ + 1)).astype(np.float32)
    a[:, :, -1] = -np.abs(a[:, :, -1]) - np.float32(1e-3)
    a[:, :, 1] = np.round(a[:, :, 1], 1)
    for t in range(1, T):
        rep = rng.random(nc) < stay
        a[t, rep] = a[t - 1, rep]
    if nonfinite:
        a[T // 2, nc // 3, 2] = NAN
        a[T // 3, nc - 1, np_] = INF
    return a.reshape(T * nc, np_ + 1)


def pairs_of(ncol):
    """four named pairs: one of them swapped, one with log L, one across the two column tiles"""
    return [(0, 1), (1, 0), (2, ncol - 1), (ncol - 2, 0)]


def chains_of(nc):
    """a selection with repeats, out of order"""
    return [2, 2, 0, nc - 1, 2] + list(range(nc - 1, -1, -2))


def linear_of(np_, nout=2):
    from mcpar_amd import engine as E
    return E.derive_linear(*linear_map(np_, nout))


# ---- results as dicts of arrays ------------------------------------------------------------------------------------------------
def as_is(d):
    return {k: np.array(v) for k, v in d.items()}


def rowset_dict(rs):
    d = {name: rs.report[name].copy() for name in rs.report.dtype.names}
    d["nkept"] = np.array([rs.nrows, rs.nsource], np.int64)
    d["rows"], d["index"] = rs.rows(), rs.index()
    rs.close()
    return d


def store_dict(st):
    d = dict(shape=np.array(st.shape, np.int64), rows=st.rows())
    st.close()
    return d


def draw_dict(r):
    return dict(rows=r[0], index=r[1])


def text_result(text, nc):
    """the text, its rows parsed back, and the rows of the store parsed from it"""
    from mcpar_amd import engine as E
    rows, rep = E.parse_text(text, nc)
    st, rep2 = E.store_from_text(text, nc)
    d = dict(text=np.frombuffer(text, np.uint8).copy(), rows=rows, store_rows=st.rows(), shape=np.array(st.shape, np.int64),
             report=np.array([rep[k] for k in sorted(rep)], np.int64), store_report=np.array([rep2[k] for k in sorted(rep2)], np.int64))
    st.close()
    return d


def same_result(a, b):
    """dtype, shape, NaN positions and all other bytes of every array agree"""
    if sorted(a) != sorted(b):
        return False
    return all(same_but_nan(a[k], b[k]) for k in a)


# ---- the float64 restatements, through the analyses' own check helpers (finite rows) ------------------------------------------
def ref_summary(raw, rows, T, nc):
    summary_ref.check(raw, summary_ref.restate(rows, T, nc, PROBS))


def ref_rank(raw, rows, T, nc):
    rank_ref.check(raw, rank_ref.restate(rows, T, nc))


def ref_covariance(raw, rows, T, nc):
    covariance_ref.check(raw, covariance_ref.restate(rows), T * nc)
    assert same_but_nan(raw["corr"], covariance_ref.corr_of(raw["cov"]))


def ref_density(raw, rows, T, nc):
    check_density(raw, rows, n=DENSITY_N)


def ref_density2d(raw, rows, T, nc):
    check_density2d(raw, rows, G, pairs_of(rows.shape[1]))


def ref_clip(raw, rows, T, nc):
    ref = clip_ref.check(raw, rows)  # counts, kept rows and indices with the thresholds reported, all exact
    own = clip_ref.thresholds(rows, QLO, QHI)
    np.testing.assert_allclose(raw.report["lo"], own[0], rtol=1e-12)  # (test_gpu_clip.py's tolerance for a threshold)
    np.testing.assert_allclose(raw.report["hi"], own[1], rtol=1e-12)
    assert 0 < int(ref["keep"].sum()) < T * nc and not raw.report["flags"].any()


def ref_chain_table(raw, rows, T, nc):
    check_chain_table(raw, rows, T, nc)


def ref_step_table(raw, rows, T, nc):
    check_step_table(raw, rows, T, nc, STEP_PROBS)


def ref_select(raw, rows, T, nc):
    sel = chains_of(nc)
    assert raw.shape == (T, len(sel), rows.shape[1])
    assert same_but_nan(raw.rows(), chains_ref.select(rows, T, nc, sel))


def ref_draw(raw, rows, T, nc):
    from mcpar_amd import engine as E
    index = E.debug_draw_indices(SEED, T * nc, 0, NDRAW)  # (the host's statement of the index rule)
    assert same_but_nan(raw[1], index) and same_but_nan(raw[0], rows[index])


def ref_derive(raw, rows, T, nc):
    assert raw.shape == (T, nc, 3)
    assert same_but_nan(raw.rows(), linear_ref(rows, *linear_map(rows.shape[1] - 1, 2)))


def ref_text(raw, rows, T, nc):
    text = raw["text"].tobytes()
    parsed, rep = check_text(text, nc, 0)  # parse_text against parse_ref
    assert same_but_nan(raw["rows"], parsed) and same_but_nan(raw["store_rows"], parsed)
    assert rep["nrows"] == T * nc and rep["ncol"] == rows.shape[1] and raw["shape"].tolist() == [T, nc, rows.shape[1]]


# ---- the one table ------------------------------------------------------------------------------------------------------------
# engine(e, first_step, nsteps) / store(s) / rows(rows, T, nc): how to call the analysis on that owner, None where the owner has
# no such entry point; to_dict: the result as a dict of arrays (it lets go of what the result holds on the device);
# persistent: the analysis uses the owner's three scratch buffers; ref: the check of a finite rows result before to_dict
Analysis = collections.namedtuple("Analysis", "name engine store rows to_dict persistent ref")


def table():
    from mcpar_amd import engine as E
    A = Analysis
    return [
        A("summary", lambda e, f, n: e.summary(PROBS, first_step=f, nsteps=n), lambda s: s.summary(PROBS),
          lambda r, T, nc: E.rows_summary(r, T, nc, PROBS), as_is, True, ref_summary),
        A("rank_summary", lambda e, f, n: e.rank_summary(first_step=f, nsteps=n), lambda s: s.rank_summary(),
          lambda r, T, nc: E.rows_rank_summary(r, T, nc), as_is, True, ref_rank),
        A("covariance", lambda e, f, n: e.covariance(first_step=f, nsteps=n), lambda s: s.covariance(),
          lambda r, T, nc: E.rows_covariance(r, T, nc), as_is, True, ref_covariance),
        A("density", lambda e, f, n: e.density(n=DENSITY_N, first_step=f, nsteps=n), lambda s: s.density(n=DENSITY_N),
          lambda r, T, nc: E.rows_density(r, T, nc, n=DENSITY_N), as_is, True, ref_density),
        A("density2d", lambda e, f, n: e.density2d(g=G, pairs=pairs_of(e.np + 1), first_step=f, nsteps=n),
          lambda s: s.density2d(g=G, pairs=pairs_of(s.shape[2])),
          lambda r, T, nc: E.rows_density2d(r, T, nc, g=G, pairs=pairs_of(r.shape[1])), as_is, True, ref_density2d),
        A("clip", lambda e, f, n: e.clip(QLO, QHI, first_step=f, nsteps=n), lambda s: s.clip(QLO, QHI),
          lambda r, T, nc: E.clip_rows(r, T, nc, QLO, QHI), rowset_dict, True, ref_clip),
        A("chain_table", lambda e, f, n: e.chain_table(first_step=f, nsteps=n), lambda s: s.chain_table(),
          lambda r, T, nc: E.rows_chain_table(r, T, nc), as_is, True, ref_chain_table),
        A("step_table", lambda e, f, n: e.step_table(first_step=f, nsteps=n, probs=STEP_PROBS), lambda s: s.step_table(STEP_PROBS),
          lambda r, T, nc: E.rows_step_table(r, T, nc, STEP_PROBS), as_is, True, ref_step_table),
        A("select_chains", lambda e, f, n: e.select_chains(chains_of(e.nc), first_step=f, nsteps=n),
          lambda s: s.select_chains(chains_of(s.shape[1])),
          lambda r, T, nc: E.select_chains_rows(r, T, nc, chains_of(nc)), store_dict, True, ref_select),
        # (there is no rows_draw: host rows are drawn through the store of all their chains, a gather of its own)
        A("draw", lambda e, f, n: e.draw(NDRAW, SEED, first_step=f, nsteps=n), lambda s: s.draw(NDRAW, SEED),
          lambda r, T, nc: draw_rows(r, T, nc), draw_dict, False, ref_draw),
        # (a DerivedStore has no derive of its own)
        A("derive", lambda e, f, n: e.derive(linear_of(e.np), first_step=f, nsteps=n), None,
          lambda r, T, nc: E.derive_rows(r, T, nc, linear_of(r.shape[1] - 1)), store_dict, False, ref_derive),
        # (a DerivedStore has no text; the text buffers of an engine are not among the three)
        A("text", lambda e, f, n: text_result(e.samples_text(f, n), e.nc), None,
          lambda r, T, nc: text_result(E.format_rows(r), nc), dict, False, ref_text),
        # Engine only; their baselines are made where the engine is (world)
        A("proposal_cov", lambda e, f, n: e.proposal_cov(first_step=f, nsteps=n), None, None, lambda v: dict(incov=np.array(v)), True, None),
        A("summary_windows", lambda e, f, n: e.summary_windows(first_step=f, nsteps=n), None, None,
          lambda v: dict(nwin=np.array([v], np.int64)), True, None),
    ]


def draw_rows(rows, T, nc):
    from mcpar_amd import engine as E
    st = E.select_chains_rows(rows, T, nc, list(range(nc)))
    out = st.draw(NDRAW, SEED)
    st.close()
    return out


NAMES = ["summary", "rank_summary", "covariance", "density", "density2d", "clip", "chain_table", "step_table", "select_chains",
         "draw", "derive", "text", "proposal_cov", "summary_windows"]
ENGINE_NAMES, STORE_NAMES, ROWS_NAMES = NAMES, NAMES[:10], NAMES[:12]  # the entries the table has for each kind of owner
N_ENGINE, N_STORE, N_ROWS = len(ENGINE_NAMES), len(STORE_NAMES), len(ROWS_NAMES)


def entries(kind):
    return [a for a in table() if getattr(a, kind) is not None]


def test_the_table_is_what_it_says():
    assert [a.name for a in table()] == NAMES
    assert [a.name for a in entries("engine")] == ENGINE_NAMES and (N_ENGINE, N_STORE, N_ROWS) == (14, 10, 12)
    assert [a.name for a in entries("store")] == STORE_NAMES    # without derive, text, proposal_cov, summary_windows
    assert [a.name for a in entries("rows")] == ROWS_NAMES      # without proposal_cov, summary_windows
    assert [a.name for a in table() if not a.persistent] == ["draw", "derive", "text"]


# ---- the hooks, and the world the tests share ----------------------------------------------------------------------------------
STATE = dict(fill=-1)


def allocation_fill(byte):
    from mcpar_amd import engine as E
    n = E.debug_fill_allocations(byte)
    STATE["fill"] = byte
    return n


@pytest.fixture(autouse=True)
def allocation_fill_off():
    yield
    allocation_fill(-1)


BASE = {}  # (data key, analysis) -> the baseline dict


def baseline(W, key, a):
    """the rows_* / *_rows result of the rows of `key` with both hooks off, once"""
    if (key, a.name) not in BASE:
        assert STATE["fill"] == -1, "a baseline is made with the allocation fill off"
        rows, T, nc = W["data"][key]
        BASE[key, a.name] = a.to_dict(a.rows(rows, T, nc))
    return BASE[key, a.name]


def engine_baselines(eg, key, first, nsteps, rows):
    """the two analyses only an engine has, on an engine nothing else has touched: the proposal from the rows' covariance, and
    the windows of the engine's first summary"""
    from mcpar_amd import engine as E
    BASE[key, "proposal_cov"] = dict(incov=E.proposal_from_cov(E.rows_covariance(rows, nsteps, eg.nc)["cov"], eg.np))
    BASE[key, "summary_windows"] = dict(nwin=np.array([eg.summary_windows(first_step=first, nsteps=nsteps)], np.int64))


def make_engine():
    eg = run(ENG_NC, ENG_NP, ENG_STEPS)
    assert eg.samples.shape == (ENG_STEPS * ENG_NC, ENG_NP + 1) and 0 < ENG_FIRST and ENG_FIRST + ENG_INNER < ENG_STEPS
    return eg


@pytest.fixture(scope="module")
def world():
    from mcpar_amd import engine as E
    allocation_fill(-1)  # every engine is created and run with the fill off
    W = dict(data={}, owners={})
    for key, (np_, nc, T, nonfinite) in VARIANTS.items():
        W["data"][key] = (make_rows(np_, nc, T, nonfinite), T, nc)
    eg = make_engine()
    W["data"]["engine-whole"] = (eg.samples, ENG_STEPS, ENG_NC)
    W["data"]["engine-inner"] = (eg.samples_range(ENG_FIRST, ENG_INNER), ENG_INNER, ENG_NC)
    twin = make_engine()  # (the same run: for the windows of a first summary of either range)
    assert twin.samples.tobytes() == eg.samples.tobytes()
    engine_baselines(twin, "engine-inner", ENG_FIRST, ENG_INNER, W["data"]["engine-inner"][0])
    twin.close()
    engine_baselines(eg, "engine-whole", 0, ENG_STEPS, W["data"]["engine-whole"][0])
    W["owners"]["engine-whole"] = (eg, 0, ENG_STEPS)
    W["owners"]["engine-inner"] = (eg, ENG_FIRST, ENG_INNER)
    rows, T, nc = W["data"]["17x37x24"]
    rs = E.clip_rows(rows, T, nc, QLO, QHI)
    stores = dict(derived=E.derive_rows(rows, T, nc, linear_of(rows.shape[1] - 1, 17)),
                  selected=E.select_chains_rows(rows, T, nc, chains_of(nc)),
                  text=E.store_from_text(E.format_rows(rows), nc)[0],
                  clipstore=rs.store(nc=CLIP_STORE_NC))
    rs.close()
    for key, st in stores.items():
        t, c, ncol = st.shape
        assert t >= 8 and ncol == 18, (key, st.shape)  # two column tiles and log L; half-chains of four steps at least
        W["data"][key] = (st.rows(), t, c)
        W["owners"][key] = st
    assert stores["clipstore"].shape[1] == CLIP_STORE_NC and stores["derived"].shape == (24, 37, 18)
    yield W
    for st in stores.values():
        st.close()
    eg.close()


def call(W, key, a):
    """analysis a on the owner `key` -> its dict"""
    owner = W["owners"][key]
    if isinstance(owner, tuple):
        eg, first, nsteps = owner
        return a.to_dict(a.engine(eg, first, nsteps))
    return a.to_dict(a.store(owner))


def owner_entries(key):
    return entries("engine" if key.startswith("engine") else "store")


def fill_scratch(W, key, byte):
    from mcpar_amd import engine as E
    owner = W["owners"][key]
    return E.debug_fill_scratch(owner[0] if isinstance(owner, tuple) else owner, byte)


OWNERS = ["engine-whole", "engine-inner", "derived", "selected", "text", "clipstore"]


# ---- 0. the baselines of the finite rows are the restatements' -----------------------------------------------------------------
@pytest.mark.parametrize("variant", FINITE)
def test_baselines_against_the_restatements(world, variant):
    rows, T, nc = world["data"][variant]
    ran = 0
    for a in entries("rows"):
        raw = a.rows(rows, T, nc)
        a.ref(raw, rows, T, nc)
        got = a.to_dict(raw)
        assert same_result(got, baseline(world, variant, a)), a.name  # (made here, or the same bytes as when it was made)
        ran += 1
    assert ran == N_ROWS


# ---- 1. fresh memory -----------------------------------------------------------------------------------------------------------
def fresh_memory(W, byte):
    for key in VARIANTS:
        for a in entries("rows"):
            baseline(W, key, a)
    assert allocation_fill(byte) == 0
    ran = 0
    for key in VARIANTS:
        rows, T, nc = W["data"][key]
        for a in entries("rows"):
            got = a.to_dict(a.rows(rows, T, nc))
            assert same_result(got, BASE[key, a.name]), (key, a.name, "0x%02X" % byte)
            ran += 1
    nfilled = allocation_fill(-1)
    assert nfilled >= ran > 0, nfilled  # every call allocates: had the hook done nothing, the count would say so
    assert ran == len(VARIANTS) * N_ROWS * 1


def test_fresh_memory_of_zeros(world):
    fresh_memory(world, 0x00)


# ---- 2. persistent scratch -----------------------------------------------------------------------------------------------------
def persistent_scratch(W, key, byte):
    ran = 0
    for a in owner_entries(key):
        if a.rows is not None:
            baseline(W, key, a)
        first = call(W, key, a)  # so that the scratch exists
        assert same_result(first, BASE[key, a.name]), (key, a.name, "before the fill")
        nbytes = fill_scratch(W, key, byte)
        assert len(nbytes) == 3 and (sum(nbytes) > 0 or not a.persistent), (key, a.name, nbytes)
        assert same_result(call(W, key, a), BASE[key, a.name]), (key, a.name, "0x%02X" % byte)
        ran += 1
    assert ran == (N_ENGINE if key.startswith("engine") else N_STORE) * 1 * 1


@pytest.mark.parametrize("key", OWNERS)
def test_persistent_scratch_of_zeros(world, key):
    persistent_scratch(world, key, 0x00)


# ---- 3. real residue -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key, before", [("engine-whole", n) for n in ENGINE_NAMES] + [("derived", n) for n in STORE_NAMES])
def test_residue_of_another_analysis(world, key, before):
    """B, then A, for every A != B: A is its baseline"""
    todo = owner_entries(key)
    b = [a for a in todo if a.name == before]
    ran = 0
    for a in todo:
        if a.name == before:
            continue
        if a.rows is not None:
            baseline(world, key, a)
        call(world, key, b[0])
        assert same_result(call(world, key, a), BASE[key, a.name]), (key, before, a.name)
        ran += 1
    assert ran == len(todo) - 1 == (N_ENGINE if key.startswith("engine") else N_STORE) - 1


@pytest.mark.parametrize("name", NAMES)
def test_residue_of_a_larger_and_a_smaller_range(world, name):
    """on an engine of its own: the inner range (its scratch is made), the whole one (it grows), the inner one again (the
    larger call's numbers lie behind its regions), the whole one"""
    a = [x for x in table() if x.name == name][0]
    for key in ("engine-whole", "engine-inner"):
        if a.rows is not None:
            baseline(world, key, a)
    eg = make_engine()
    assert eg.samples.tobytes() == world["data"]["engine-whole"][0].tobytes()  # the run of the shared engine, bit for bit
    for key, first, nsteps in (("engine-inner", ENG_FIRST, ENG_INNER), ("engine-whole", 0, ENG_STEPS)) * 2:
        assert same_result(a.to_dict(a.engine(eg, first, nsteps)), BASE[key, name]), (name, key)
    eg.close()


# ---- 1 and 2 again, with the bytes that are not zero ---------------------------------------------------------------------------
@pytest.mark.parametrize("byte", FILLS[1:], ids=lambda b: "0x%02X" % b)
def test_fresh_memory(world, byte):
    fresh_memory(world, byte)


@pytest.mark.parametrize("byte", FILLS[1:], ids=lambda b: "0x%02X" % b)
@pytest.mark.parametrize("key", OWNERS)
def test_persistent_scratch(world, key, byte):
    persistent_scratch(world, key, byte)
