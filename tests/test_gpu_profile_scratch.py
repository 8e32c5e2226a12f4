"""The profile likelihoods of a store do not depend on what their scratch held before (DESIGN.md "Scratch
and its history"): the three situations of tests/test_gpu_scratch_history.py with its rows, fill bytes, owners and rule of
equality (imported, not restated).
  1. fresh memory        every allocation of a rows call filled with a byte first
  2. persistent scratch  the owner's three buffers filled between two calls, on an engine (both ranges) and on two stores
  3. real residue        behind every other analysis of the table on one engine and one store, and behind a larger call of
                         its own on an engine of its own (a regrow in mid-session)
The baseline is the rows call with both hooks off; the finite baselines are held to tests/profile_ref.py first."""
import numpy as np
import pytest

import profile_ref as R
import test_gpu_scratch_history as H
from test_gpu_profile import check as check1d
from test_gpu_profile2d import check as check2d

pytestmark = pytest.mark.gpu

N1, G2, DROPS = 24, 9, (0.5, 2.0)
BASE = {}


def pairs_of(np_):
    return [(0, 1), (1, 0), (2, 1), (np_ - 1, 0)]


def rows_call(rows, T, nc):
    """both analyses of host rows, as one dict of arrays"""
    from mcpar_amd import engine as E
    np_ = rows.shape[1] - 1
    d = {"p1_" + k: v for k, v in E.rows_profile(rows, T, nc, n=N1, path=True, drops=DROPS).items()}
    d.update({"p2_" + k: v for k, v in E.rows_profile2d(rows, T, nc, g=G2, pairs=pairs_of(np_), drops=DROPS).items()})
    return d


def owner_call(owner):
    if isinstance(owner, tuple):
        eg, first, nsteps = owner
        d = {"p1_" + k: v for k, v in eg.profile_likelihood(n=N1, path=True, drops=DROPS, first_step=first, nsteps=nsteps).items()}
        d.update({"p2_" + k: v for k, v in
                  eg.profile_likelihood2d(g=G2, pairs=pairs_of(eg.np), drops=DROPS, first_step=first, nsteps=nsteps).items()})
        return d
    np_ = owner.shape[2] - 1
    d = {"p1_" + k: v for k, v in owner.profile_likelihood(n=N1, path=True, drops=DROPS).items()}
    d.update({"p2_" + k: v for k, v in owner.profile_likelihood2d(g=G2, pairs=pairs_of(np_), drops=DROPS).items()})
    return d


@pytest.fixture(autouse=True)
def allocation_fill_off():
    yield
    H.allocation_fill(-1)


def baseline(rows, T, nc, key):
    if key not in BASE:
        assert H.STATE["fill"] == -1, "a baseline is made with the allocation fill off"
        BASE[key] = rows_call(rows, T, nc)
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


def owner_baseline(W, key):
    rows, T, nc = W["data"][key]
    return baseline(rows, T, nc, key)


# ---- 0. the baselines are the restatement's -------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(H.VARIANTS))
def test_baselines_against_the_restatement(world, variant):
    rows, T, nc = world["data"][variant]
    got = baseline(rows, T, nc, variant)
    np_ = rows.shape[1] - 1
    check1d({k[3:]: v for k, v in got.items() if k.startswith("p1_")}, R.profile(rows, n=N1, drops=DROPS), variant)
    check2d({k[3:]: v for k, v in got.items() if k.startswith("p2_")}, R.profile2d(rows, g=G2, pairs=pairs_of(np_), drops=DROPS), variant)
    if H.VARIANTS[variant][3]:  # (the column with the NaN; the +inf in log L makes the maximum not finite)
        assert got["p1_flags"][2] == 1 and (np.delete(got["p1_flags"], 2) == R.LL_NONFINITE).all()


# ---- 1. fresh memory -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", H.FILLS, ids=lambda b: "0x%02X" % b)
def test_fresh_memory(world, byte):
    for key in H.VARIANTS:
        baseline(*world["data"][key], key)
    assert H.allocation_fill(byte) == 0
    ran = 0
    for key in H.VARIANTS:
        rows, T, nc = world["data"][key]
        assert H.same_result(rows_call(rows, T, nc), BASE[key]), (key, "0x%02X" % byte)
        ran += 1
    nfilled = H.allocation_fill(-1)
    assert nfilled >= ran == len(H.VARIANTS), nfilled


# ---- 2. persistent scratch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", H.FILLS, ids=lambda b: "0x%02X" % b)
@pytest.mark.parametrize("key", OWNERS)
def test_persistent_scratch(world, key, byte):
    base = owner_baseline(world, key)
    assert H.same_result(owner_call(world["owners"][key]), base), (key, "before the fill")
    nbytes = H.fill_scratch(world, key, byte)
    assert len(nbytes) == 3 and min(nbytes) > 0, (key, nbytes)  # (the grids in the doubles, the keys in the 64-bit words, the values in the 32-bit ones)
    assert H.same_result(owner_call(world["owners"][key]), base), (key, "0x%02X" % byte)


# ---- 3. real residue -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["engine-whole", "selected"])
def test_residue_of_every_other_analysis(world, key):
    """B, then the profiles, for every B of the table: they are their baseline"""
    owner = world["owners"][key]
    kind = "engine" if isinstance(owner, tuple) else "store"
    others = H.entries(kind)
    assert len(others) == (H.N_ENGINE if kind == "engine" else H.N_STORE)
    base = owner_baseline(world, key)
    for b in others:
        b.to_dict(b.engine(*owner) if kind == "engine" else b.store(owner))
        assert H.same_result(owner_call(owner), base), (key, b.name)


def test_residue_of_a_larger_and_a_smaller_range(world):
    """on an engine of its own: the inner range, the whole one (the scratch grows), the inner one again, the whole one"""
    for key in ("engine-whole", "engine-inner"):
        owner_baseline(world, key)
    eg = H.make_engine()
    assert eg.samples.tobytes() == world["data"]["engine-whole"][0].tobytes()
    for key, first, nsteps in (("engine-inner", H.ENG_FIRST, H.ENG_INNER), ("engine-whole", 0, H.ENG_STEPS)) * 2:
        assert H.same_result(owner_call((eg, first, nsteps)), BASE[key]), key
    eg.close()
