"""The reweight and the resample of a store do not depend on what their scratch held before (DESIGN.md "Scratch and its
history"): the three situations of tests/test_gpu_scratch_history.py with its rows, fill bytes, owners and rule of equality
(imported, not restated).
  1. fresh memory        every allocation of a rows call filled with a byte first
  2. persistent scratch  the owner's three buffers filled between two calls, on an engine (both ranges) and on two stores
  3. real residue        behind every other analysis of the table on one engine and one store, and behind a larger call of
                         its own on an engine of its own (a regrow in mid-session)
The baseline is the rows call with both hooks off; the finite baselines are held to tests/reweight_ref.py first."""
import numpy as np
import pytest

import reweight_ref as R
import test_gpu_scratch_history as H
from test_gpu_reweight import held

pytestmark = pytest.mark.gpu

PROBS = (0.05, 0.5, 0.95)
SEED, KT, KC = 31, 3, 150  # the resample: 3 x 150 draws, two draw workgroups


def logw_of(rows):
    """log-weights made of the rows (column 0 is finite in every variant): some ten e-folds"""
    return (np.float32(2.0) * rows[:, 0]).astype(np.float32)


def weights_of(rows):
    from mcpar_amd import engine as E
    return E.weights_host(logw_of(rows))


def reweight_dict(d):
    out = {k: np.asarray(v) for k, v in d.items() if k not in ("cols", "sumq2")}
    out.update({"cols." + k: np.asarray(v) for k, v in d["cols"].items()})
    return out


def resample_dict(r):
    st, index = r
    d = dict(shape=np.array(st.shape, np.int64), rows=st.rows(), index=index)
    st.close()
    return d


# name -> (engine(e, first, nsteps, w), store(s, w), rows(rows, T, nc, w), to_dict)
def analyses():
    from mcpar_amd import engine as E
    return {
        "reweight": (lambda e, f, n, w: e.reweight(w, PROBS, first_step=f, nsteps=n), lambda s, w: s.reweight(w, PROBS),
                     lambda r, T, nc, w: E.reweight_rows(r, T, nc, w, PROBS), reweight_dict),
        "resample": (lambda e, f, n, w: e.resample(w, KT, KC, SEED, with_index=True, first_step=f, nsteps=n),
                     lambda s, w: s.resample(w, KT, KC, SEED, with_index=True),
                     lambda r, T, nc, w: E.resample_rows(r, T, nc, w, KT, KC, SEED, with_index=True), resample_dict),
    }


NAMES = ["reweight", "resample"]
BASE = {}


@pytest.fixture(autouse=True)
def allocation_fill_off():
    yield
    H.allocation_fill(-1)


def baseline(rows, T, nc, key, name):
    if (key, name) not in BASE:
        assert H.STATE["fill"] == -1, "a baseline is made with the allocation fill off"
        _, _, on_rows, to_dict = analyses()[name]
        BASE[key, name] = to_dict(on_rows(rows, T, nc, weights_of(rows)))
    return BASE[key, name]


@pytest.fixture(scope="module")
def world():
    from mcpar_amd import engine as E
    H.allocation_fill(-1)
    W = dict(data={}, owners={})
    for key, (np_, nc, T, nonfinite) in H.VARIANTS.items():
        W["data"][key] = (H.make_rows(np_, nc, T, nonfinite), T, nc)
    eg = H.make_engine()
    W["data"]["engine-whole"] = (eg.samples, H.ENG_STEPS, H.ENG_NC)
    W["data"]["engine-inner"] = (eg.samples_range(H.ENG_FIRST, H.ENG_INNER), H.ENG_INNER, H.ENG_NC)
    W["owners"]["engine-whole"] = (eg, 0, H.ENG_STEPS)
    W["owners"]["engine-inner"] = (eg, H.ENG_FIRST, H.ENG_INNER)
    rows, T, nc = W["data"]["17x37x24"]
    stores = dict(selected=E.select_chains_rows(rows, T, nc, H.chains_of(nc)), text=E.store_from_text(E.format_rows(rows), nc)[0])
    for key, st in stores.items():
        t, c, _ = st.shape
        W["data"][key] = (st.rows(), t, c)
        W["owners"][key] = st
    yield W
    for st in stores.values():
        st.close()
    eg.close()


OWNERS = ["engine-whole", "engine-inner", "selected", "text"]


def call(W, key, name):
    owner = W["owners"][key]
    on_engine, on_store, _, to_dict = analyses()[name]
    w = weights_of(W["data"][key][0])
    if isinstance(owner, tuple):
        return to_dict(on_engine(owner[0], owner[1], owner[2], w))
    return to_dict(on_store(owner, w))


def owner_baseline(W, key, name):
    rows, T, nc = W["data"][key]
    return baseline(rows, T, nc, key, name)


# ---- 0. the baselines are the restatement's -------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(H.VARIANTS))
def test_baselines_against_the_restatement(world, variant):
    from mcpar_amd import engine as E
    rows, T, nc = world["data"][variant]
    w = weights_of(rows)
    q, lwmax = E.debug_reweight_q(w, rows, T, nc)
    want, wmax = R.fixed_point(R.log_weights(logw_of(rows), 1.0))
    assert lwmax == wmax and np.abs(q.astype(np.int64) - want.astype(np.int64)).max() <= 1
    got = E.reweight_rows(rows, T, nc, w, PROBS)
    held(got, R.restate(rows, q, lwmax, PROBS), variant)
    assert H.same_result(reweight_dict(got), baseline(rows, T, nc, variant, "reweight"))
    base = baseline(rows, T, nc, variant, "resample")
    index, _ = R.resample_index(q, SEED, KT * KC)
    assert np.array_equal(base["index"], index) and H.same_but_nan(base["rows"], rows[index]) and base["shape"].tolist() == [KT, KC, rows.shape[1]]
    if H.VARIANTS[variant][3]:
        assert got["cols"]["flags"][2] == 1 and got["cols"]["flags"][-1] == 1  # the NaN and the +inf lie on rows with weight


# ---- 1. fresh memory -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", H.FILLS, ids=lambda b: "0x%02X" % b)
def test_fresh_memory(world, byte):
    for key in H.VARIANTS:
        for name in NAMES:
            baseline(*world["data"][key], key, name)
    assert H.allocation_fill(byte) == 0
    ran = 0
    for key in H.VARIANTS:
        rows, T, nc = world["data"][key]
        for name in NAMES:
            _, _, on_rows, to_dict = analyses()[name]
            got = to_dict(on_rows(rows, T, nc, weights_of(rows)))
            assert H.same_result(got, BASE[key, name]), (key, name, "0x%02X" % byte)
            ran += 1
    nfilled = H.allocation_fill(-1)
    assert nfilled >= ran == len(H.VARIANTS) * len(NAMES), nfilled


# ---- 2. persistent scratch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", H.FILLS, ids=lambda b: "0x%02X" % b)
@pytest.mark.parametrize("key", OWNERS)
def test_persistent_scratch(world, key, byte):
    for name in NAMES:
        base = owner_baseline(world, key, name)
        assert H.same_result(call(world, key, name), base), (key, name, "before the fill")
        nbytes = H.fill_scratch(world, key, byte)
        assert len(nbytes) == 3 and (sum(nbytes) > 0 or name == "resample"), (key, name, nbytes)  # (a resample uses per-call scratch alone)
        assert H.same_result(call(world, key, name), base), (key, name, "0x%02X" % byte)


# ---- 3. real residue -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["engine-whole", "selected"])
def test_residue_of_every_other_analysis(world, key):
    """B, then reweight and resample, for every B of the table and for each other: each is its baseline"""
    owner = world["owners"][key]
    kind = "engine" if isinstance(owner, tuple) else "store"
    others = H.entries(kind)
    assert len(others) == (H.N_ENGINE if kind == "engine" else H.N_STORE)
    for name in NAMES:
        base = owner_baseline(world, key, name)
        for b in others:
            b.to_dict(b.engine(*owner) if kind == "engine" else b.store(owner))
            assert H.same_result(call(world, key, name), base), (key, b.name, name)
        for other in NAMES:
            call(world, key, other)
            assert H.same_result(call(world, key, name), base), (key, other, name)


@pytest.mark.parametrize("name", NAMES)
def test_residue_of_a_larger_and_a_smaller_range(world, name):
    """on an engine of its own: the inner range, the whole one (the scratch grows), the inner one again, the whole one"""
    on_engine, _, _, to_dict = analyses()[name]
    for key in ("engine-whole", "engine-inner"):
        owner_baseline(world, key, name)
    eg = H.make_engine()
    assert eg.samples.tobytes() == world["data"]["engine-whole"][0].tobytes()
    for key, first, nsteps in (("engine-inner", H.ENG_FIRST, H.ENG_INNER), ("engine-whole", 0, H.ENG_STEPS)) * 2:
        w = weights_of(world["data"][key][0])
        assert H.same_result(to_dict(on_engine(eg, first, nsteps, w)), BASE[key, name]), (name, key)
    eg.close()
