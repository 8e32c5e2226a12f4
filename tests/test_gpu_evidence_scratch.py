"""The evidence of a store does not depend on what its scratch held before (DESIGN.md "Scratch and its
history"): the three situations of tests/test_gpu_scratch_history.py with its engine, fill bytes and rule of equality
(imported, not restated).
  1. fresh memory        every allocation of a rows call filled with a byte first
  2. persistent scratch  the owner's three buffers filled between two calls, on an engine (both ranges) and on two stores
  3. real residue        behind the summary, the covariance and the modes on one engine and one store, and behind a larger call
                         of its own on an engine of its own (a regrow in mid-session)
The baseline is the rows call with both hooks off; the baselines are held to tests/evidence_ref.py first (the bridge on the l1
and l2 the call itself reports)."""
import numpy as np
import pytest

import evidence_ref as R
import test_gpu_scratch_history as H

pytestmark = pytest.mark.gpu

SPEC = dict(ndraw=500, seed=4)
BASE = {}
RTOL = 1e-9


def likelihood():
    """the Gaussian of test_gpu_store_view.run, which H.make_engine runs"""
    import mcpar_amd as M
    d = H.ENG_NP
    params = np.concatenate([np.linspace(-1.0, 1.0, d), np.linspace(0.5, 2.0, d)]).astype(np.float32)
    return M.make_vlfunc(M.VL_GAUSSIAN, d, params)


def to_dict(res):
    return {k: np.asarray(v) for k, v in res.items()}


@pytest.fixture(autouse=True)
def allocation_fill_off():
    yield
    H.allocation_fill(-1)


@pytest.fixture(scope="module")
def world():
    from mcpar_amd import engine as E
    H.allocation_fill(-1)
    W = dict(data={}, owners={}, vl=likelihood())
    eg = H.make_engine()
    W["data"]["engine-whole"] = (eg.samples, H.ENG_STEPS, H.ENG_NC)
    W["data"]["engine-inner"] = (eg.samples_range(H.ENG_FIRST, H.ENG_INNER), H.ENG_INNER, H.ENG_NC)
    W["owners"]["engine-whole"] = (eg, 0, H.ENG_STEPS)
    W["owners"]["engine-inner"] = (eg, H.ENG_FIRST, H.ENG_INNER)
    rows, T, nc = W["data"]["engine-whole"]
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


def baseline(W, key):
    from mcpar_amd import engine as E
    if key not in BASE:
        assert H.STATE["fill"] == -1, "a baseline is made with the allocation fill off"
        rows, T, nc = W["data"][key]
        BASE[key] = to_dict(E.rows_evidence(rows, T, nc, W["vl"][0], **SPEC))
    return BASE[key]


def call(W, key):
    owner = W["owners"][key]
    if isinstance(owner, tuple):
        return to_dict(owner[0].evidence(first_step=owner[1], nsteps=owner[2], **SPEC))   # (the last run's likelihood)
    return to_dict(owner.evidence(W["vl"][0], **SPEC))


# ---- 0. the baselines are the restatement's -------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", OWNERS)
def test_baselines_against_the_restatement(world, key):
    from mcpar_amd import engine as E
    rows, T, nc = world["data"][key]
    got = baseline(world, key)
    res, l1, l2 = E.debug_evidence_l(rows, T, nc, world["vl"][0], **SPEC)
    assert H.same_result(to_dict(res), got)
    ref = R.bridge(l1, l2, neff=float(got["neff"]), ess_f2=float(got["ess_f2"]))
    assert (got["iters"], got["flags"], got["n1"], got["n2"]) == (ref["iters"], ref["flags"], (T - T // 2) * nc, 500)
    for name in ("lstar", "log_z", "se", "re2_draws", "re2_rows", "log_z_is", "log_z_ris"):
        assert abs(got[name] - ref[name]) <= RTOL * abs(ref[name]), name


# ---- 1. fresh memory -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", H.FILLS, ids=lambda b: "0x%02X" % b)
def test_fresh_memory(world, byte):
    from mcpar_amd import engine as E
    keys = ("engine-whole", "engine-inner", "text")
    for key in keys:
        baseline(world, key)
    assert H.allocation_fill(byte) == 0
    for key in keys:
        rows, T, nc = world["data"][key]
        assert H.same_result(to_dict(E.rows_evidence(rows, T, nc, world["vl"][0], **SPEC)), BASE[key]), (key, "0x%02X" % byte)
    assert H.allocation_fill(-1) >= len(keys)


# ---- 2. persistent scratch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", H.FILLS, ids=lambda b: "0x%02X" % b)
@pytest.mark.parametrize("key", OWNERS)
def test_persistent_scratch(world, key, byte):
    base = baseline(world, key)
    assert H.same_result(call(world, key), base), (key, "before the fill")
    nbytes = H.fill_scratch(world, key, byte)
    assert len(nbytes) == 3 and nbytes[0] > 0, (key, nbytes)   # (the covariance's and the summary's doubles)
    assert H.same_result(call(world, key), base), (key, "0x%02X" % byte)


# ---- 3. real residue -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["engine-whole", "selected"])
def test_residue_of_other_analyses(world, key):
    owner = world["owners"][key]
    base = baseline(world, key)
    if isinstance(owner, tuple):
        others = (lambda: owner[0].summary(), lambda: owner[0].covariance(), lambda: owner[0].rank_summary(),
                  lambda: owner[0].modes(3, seed=1).close(), lambda: owner[0].intervals())
    else:
        others = (owner.summary, owner.covariance, owner.rank_summary, lambda: owner.modes(3, seed=1).close(), owner.intervals)
    for b in others:
        b()
        assert H.same_result(call(world, key), base), key


def test_residue_of_a_larger_and_a_smaller_range(world):
    for key in ("engine-whole", "engine-inner"):
        baseline(world, key)
    eg = H.make_engine()
    assert eg.samples.tobytes() == world["data"]["engine-whole"][0].tobytes()
    for key, first, nsteps in (("engine-inner", H.ENG_FIRST, H.ENG_INNER), ("engine-whole", 0, H.ENG_STEPS)) * 2:
        assert H.same_result(to_dict(eg.evidence(first_step=first, nsteps=nsteps, **SPEC)), BASE[key]), key
    eg.close()
