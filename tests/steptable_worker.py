"""The engine scenario of tests/test_gpu_steptable.py, in a process of its own (nothing else of the suite is alive here, so
mcx_debug_live_resources starts at zero): Rosenbrock1, np = 4, 64 chains, 20 burn-in + 40 main steps; the step table of a step
range of the engine's store has the bytes of the table of the same rows copied to the host, synchronously and after
MCX_OPT_ASYNC_RUN, on a derived store and on a store of chosen chains; the settle rule on it equals the restatement; with
every store closed the count is (0, 0, 0, 0) again."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import chains_ref  # noqa: E402
import steptable_ref as R  # noqa: E402
import mcpar_amd as M  # noqa: E402
from mcpar_amd import engine as E  # noqa: E402

NP, NC, NBURN, NSAMP, FIRST, T = 4, 64, 20, 40, 5, 30
PROBS = (0.05, 0.5, 0.95)


def pinit(d, n):
    g, i = np.arange(n, dtype=np.float64)[:, None], np.arange(d, dtype=np.float64)[None, :]
    return (0.5 * np.sin(0.37 * (g * d + i))).astype(np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_table(a, b):
    return set(a) == set(b) and all(same_bits(a[k], b[k]) for k in a)


def against_ref(t, rows, nsteps, nc, probs=PROBS):
    ref = R.table(rows, nsteps, nc, probs)
    amax = np.abs(rows.reshape(nsteps, nc, -1).astype(np.float64)).max(axis=1)
    assert (np.abs(t["mean"] - ref["mean"]) <= 8 * nc * 2.0 ** -53 * amax).all()
    np.testing.assert_allclose(t["sd"], ref["sd"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(t["quantiles"], ref["quantiles"], rtol=1e-12, atol=0)
    for name in ("min", "max", "flags", "moved", "ll_max", "ll_max_chain", "step_flags"):
        assert same_bits(t[name], ref[name]), name


def main():
    assert E.debug_live_resources() == (0, 0, 0, 0)
    vl, _keep = M.make_vlfunc(M.VL_ROSENBROCK1, NP)
    e = M.Engine(NP, NC)
    e.set_option(E.OPT_ACCEPT_MASK, 1)
    try:
        e.step_table(first_step=0, nsteps=8)  # no run yet
        raise AssertionError("a table of an empty store was not refused")
    except M.McxError as err:
        assert err.code == 1 and "the sample store is empty" in str(err)
    e.run(NSAMP, NBURN, pinit(NP, NC), vl)
    for first, n in ((0, NSAMP), (FIRST, T), (NSAMP - 1, 1)):
        rows = e.samples_range(first, n)
        t = e.step_table(first, n)
        assert same_table(t, E.rows_step_table(rows, n, NC)), (first, n)
        against_ref(t, rows, n, NC)
        assert t["moved"][0] == -1 and not t["step_flags"].any()
    rows = e.samples_range(FIRST, T)
    t = e.step_table(FIRST, T)
    # a chain moves at most where the main loop accepted: per step, the chains whose row changed against the accept mask
    accepted = e.accept_mask[NBURN + FIRST + 1:NBURN + FIRST + T].astype(np.int64).sum(axis=1)
    assert (t["moved"][1:] <= accepted).all() and t["moved"][1:].sum() > 0
    ct = e.chain_table(FIRST, T)
    assert t["moved"][1:].sum() == ct["moves"].sum() and t["ll_max"].max() == ct["ll_max"].max()
    # the mean over the steps of the step means is the column's mean
    s = e.summary(first_step=FIRST, nsteps=T)
    np.testing.assert_allclose(t["mean"].mean(axis=0), s["mean"], rtol=1e-9, atol=0)
    assert same_table(t, e.step_table(FIRST, T))  # the same arguments, the same bytes
    t0 = e.step_table(FIRST, T, probs=())
    assert t0["quantiles"].shape == (T, NP + 1, 0) and all(same_bits(t0[k], t[k]) for k in t if k != "quantiles")
    # the rule on it
    for kw in (dict(), dict(tol_mean=0.5, tol_sd=0.5), dict(tol_mean=1.0, tol_sd=1.0, ref_frac=0.25), dict(use_col=[0, 0, 0, 0, 1])):
        got, want = E.settle_steps(t, **kw), R.settle(t, **kw)
        assert got[0] == want[0], (kw, got[0], want[0])
        for name in want[1]:
            a, b = got[1][name], want[1][name]
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(b)], b[~np.isnan(b)]), (kw, name)
    # refusals that name the range and the entry
    for call, text in ((lambda: e.step_table(20, 30), "not in the sample store"), (lambda: e.step_table(0, 0), "at least one step"),
                       (lambda: e.step_table(FIRST, T, probs=(0.5, 1.5)), "probs[1] = 1.5")):
        try:
            call()
            raise AssertionError("not refused: " + text)
        except M.McxError as err:
            assert err.code == 1 and text in str(err), str(err)
    ms = e.step_table_times(FIRST, T)
    assert ms.shape == (4,) and (ms > 0).all() and ms[3] >= ms[0] + ms[1] + ms[2]
    ms0 = e.step_table_times(FIRST, T, probs=())
    assert ms0[1] == 0.0 and ms0[0] > 0 and ms0[2] > 0  # no select launch
    # a derived store, and a store of chosen chains in another order: ll_max_chain follows the new indices
    A = np.array([[1, 1, 0, 0], [0, 0, 1, -1], [2, 0, 0, 0]], np.float32)
    ds = e.derive(E.derive_linear(A, np.array([0.5, 0.0, -1.0], np.float32)), first_step=FIRST, nsteps=T)
    td = ds.step_table()
    drows = ds.rows()
    assert td["mean"].shape == (T, 4) and same_table(td, E.rows_step_table(drows, T, NC))
    against_ref(td, drows, T, NC)
    assert same_bits(td["ll_max"], t["ll_max"]) and same_bits(td["ll_max_chain"], t["ll_max_chain"])
    ds.close()
    sel = np.random.default_rng(4).permutation(NC)[:40]
    st = e.select_chains(sel, first_step=FIRST, nsteps=T)
    ts = st.step_table(probs=(0.25, 0.75))
    srows = chains_ref.select(rows, T, NC, sel)
    assert same_table(ts, E.rows_step_table(srows, T, len(sel), probs=(0.25, 0.75)))
    against_ref(ts, srows, T, len(sel), (0.25, 0.75))
    ll = rows.reshape(T, NC, NP + 1)[:, :, NP]
    assert same_bits(ll[np.arange(T), sel[ts["ll_max_chain"]]], ts["ll_max"])
    e.close()
    assert same_table(ts, st.step_table(probs=(0.25, 0.75)))  # the store outlives the engine
    st.close()
    # MCX_OPT_ASYNC_RUN: the table straight after the queued run
    a = M.Engine(NP, NC)
    a.set_option(E.OPT_ASYNC_RUN, 1)
    a.run(NSAMP, NBURN, pinit(NP, NC), vl)
    ta = a.step_table(FIRST, T)
    assert same_table(ta, t)
    a.close()
    assert E.debug_live_resources() == (0, 0, 0, 0), E.debug_live_resources()
    print("steptable engine: all scenarios done")


if __name__ == "__main__":
    main()
