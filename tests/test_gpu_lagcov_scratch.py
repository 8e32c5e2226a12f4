"""The lagged covariance and the multivariate ESS of a store do not depend on what their scratch held before (DESIGN.md "Scratch and its history"): the
three situations of tests/test_gpu_scratch_history.py with its rows, fill bytes, owners and rule of equality (imported, not
restated).
  1. fresh memory        every allocation of a rows call filled with a byte first
  2. persistent scratch  the owner's three buffers filled between two calls, on an engine (both ranges) and on two stores
  3. real residue        behind every other analysis of the table on one engine and one store, and behind a larger call of
                         its own on an engine of its own (a regrow in mid-session)
The baseline is the rows call with both hooks off; the baselines' G(t) are held to tests/lagcov_ref.py first."""
import numpy as np
import pytest

import lagcov_ref as R
import test_gpu_scratch_history as H
from test_gpu_lagcov import check_gamma

pytestmark = pytest.mark.gpu

NLAGS = 6  # lags returned; the walk computes what it needs beyond them, with log L among the columns
BASE = {}


def to_dict(d):
    return {k: np.asarray(v) for k, v in d.items()}


@pytest.fixture(autouse=True)
def allocation_fill_off():
    yield
    H.allocation_fill(-1)


def baseline(rows, T, nc, key):
    from mcpar_amd import engine as E
    if key not in BASE:
        assert H.STATE["fill"] == -1, "a baseline is made with the allocation fill off"
        BASE[key] = to_dict(E.rows_lagcov(rows, T, nc, nlags=NLAGS, with_ll=True))
    return BASE[key]


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


def call(W, key):
    owner = W["owners"][key]
    if isinstance(owner, tuple):
        return to_dict(owner[0].lagcov(nlags=NLAGS, with_ll=True, first_step=owner[1], nsteps=owner[2]))
    return to_dict(owner.lagcov(nlags=NLAGS, with_ll=True))


def owner_baseline(W, key):
    rows, T, nc = W["data"][key]
    return baseline(rows, T, nc, key)


# ---- 0. the baselines are the restatement's -------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(H.VARIANTS))
def test_baselines_against_the_restatement(world, variant):
    from mcpar_amd import engine as E
    rows, T, nc = world["data"][variant]
    got = E.rows_lagcov(rows, T, nc, nlags=NLAGS, with_ll=True)
    ref = R.restate(rows, T, nc, with_ll=True)
    check_gamma(got, ref, T * nc, variant)
    use = R.use_of(ref["col_flags"] & R.NONFINITE, True)
    if got["lags_computed"] <= NLAGS:  # (every lag the walk saw came back: the walk itself can be held)
        R.check_finish(got, R.finish(got["gamma"][:got["lags_computed"]], T * nc, use), rtol=1e-9, where=variant)
    assert H.same_result(to_dict(got), baseline(rows, T, nc, variant))
    if H.VARIANTS[variant][3]:
        assert got["col_flags"].tolist() == [0, 0, 1] + [0] * 14 + [1]


# ---- 1. fresh memory -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", H.FILLS, ids=lambda b: "0x%02X" % b)
def test_fresh_memory(world, byte):
    from mcpar_amd import engine as E
    for key in H.VARIANTS:
        baseline(*world["data"][key], key)
    assert H.allocation_fill(byte) == 0
    ran = 0
    for key in H.VARIANTS:
        rows, T, nc = world["data"][key]
        assert H.same_result(to_dict(E.rows_lagcov(rows, T, nc, nlags=NLAGS, with_ll=True)), BASE[key]), (key, "0x%02X" % byte)
        ran += 1
    nfilled = H.allocation_fill(-1)
    assert nfilled >= ran == len(H.VARIANTS), nfilled


# ---- 2. persistent scratch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", H.FILLS, ids=lambda b: "0x%02X" % b)
@pytest.mark.parametrize("key", OWNERS)
def test_persistent_scratch(world, key, byte):
    base = owner_baseline(world, key)
    assert H.same_result(call(world, key), base), (key, "before the fill")
    nbytes = H.fill_scratch(world, key, byte)
    assert len(nbytes) == 3 and nbytes[0] > 0, (key, nbytes)  # (a call's sums, partials and reduced slabs are in the owner's doubles)
    assert H.same_result(call(world, key), base), (key, "0x%02X" % byte)


# ---- 3. real residue -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["engine-whole", "selected"])
def test_residue_of_every_other_analysis(world, key):
    """B, then the lagged covariance, for every B of the table: they are their baseline"""
    owner = world["owners"][key]
    kind = "engine" if isinstance(owner, tuple) else "store"
    others = H.entries(kind)
    assert len(others) == (H.N_ENGINE if kind == "engine" else H.N_STORE)
    base = owner_baseline(world, key)
    for b in others:
        b.to_dict(b.engine(*owner) if kind == "engine" else b.store(owner))
        assert H.same_result(call(world, key), base), (key, b.name)


def test_residue_of_a_larger_and_a_smaller_range(world):
    """on an engine of its own: the inner range, the whole one (the scratch grows), the inner one again, the whole one"""
    for key in ("engine-whole", "engine-inner"):
        owner_baseline(world, key)
    eg = H.make_engine()
    assert eg.samples.tobytes() == world["data"]["engine-whole"][0].tobytes()
    for key, first, nsteps in (("engine-inner", H.ENG_FIRST, H.ENG_INNER), ("engine-whole", 0, H.ENG_STEPS)) * 2:
        assert H.same_result(to_dict(eg.lagcov(nlags=NLAGS, with_ll=True, first_step=first, nsteps=nsteps)), BASE[key]), key
    eg.close()
