"""The engine scenario of tests/test_gpu_chains.py, in a process of its own (nothing else of the suite is alive here, so
mcx_debug_live_resources starts at zero): Rosenbrock1, np = 4, 64 chains, 20 burn-in + 40 main steps; the chain table of a
step range against tests/chains_ref.py, against the summary and against the accept mask; the store of the kept chains after
the engine is closed; with every store closed the count is (0, 0, 0, 0) again."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import chains_ref as R  # noqa: E402
import mcpar_amd as M  # noqa: E402
from mcpar_amd import engine as E  # noqa: E402

NP, NC, NBURN, NSAMP, FIRST, T = 4, 64, 20, 40, 5, 30


def pinit(d, n):
    g, i = np.arange(n, dtype=np.float64)[:, None], np.arange(d, dtype=np.float64)[None, :]
    return (0.5 * np.sin(0.37 * (g * d + i))).astype(np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def main():
    assert E.debug_live_resources() == (0, 0, 0, 0)
    vl, _keep = M.make_vlfunc(M.VL_ROSENBROCK1, NP)
    e = M.Engine(NP, NC)
    e.set_option(E.OPT_ACCEPT_MASK, 1)
    try:
        e.chain_table(first_step=0, nsteps=8)  # no run yet
        raise AssertionError("a table of an empty store was not refused")
    except M.McxError as err:
        assert err.code == 1 and "the sample store is empty" in str(err)
    e.run(NSAMP, NBURN, pinit(NP, NC), vl)
    rows = e.samples_range(FIRST, T)
    t = e.chain_table(first_step=FIRST, nsteps=T)
    ref = R.table(rows, T, NC)
    np.testing.assert_allclose(t["mean"], ref["mean"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(t["sd"], ref["sd"], rtol=1e-9, atol=0)
    assert np.array_equal(np.isnan(t["rho1"]), np.isnan(ref["rho1"]))
    err = np.nanmax(np.abs(t["rho1"] - ref["rho1"]))
    print("engine: rho1 max error %.3g of %.3g" % (err, 8 * T * 2.0 ** -53))
    assert err <= 8 * T * 2.0 ** -53
    for name in ("moves", "longest_stay", "ll_max", "ll_max_step", "flags"):
        assert same_bits(t[name], ref[name]), name
    assert not t["flags"].any()
    # the mean over the chains of the chain means is the column's mean
    s = e.summary(first_step=FIRST, nsteps=T)
    np.testing.assert_allclose(t["mean"].mean(axis=0), s["mean"], rtol=1e-9, atol=0)
    # a chain moves at most where the main loop accepted
    accepted = e.accept_mask[NBURN:].astype(np.int64).sum(axis=0)
    assert (t["moves"] <= accepted).all() and t["moves"].sum() > 0
    # the same arguments give the same bytes
    t2 = e.chain_table(first_step=FIRST, nsteps=T)
    assert all(same_bits(t[k], t2[k]) for k in t)
    # refusals that name the range and the entry
    for call, text in ((lambda: e.chain_table(first_step=20, nsteps=30), "not in the sample store"),
                       (lambda: e.select_chains([0, NC], FIRST, T), "chains[1] = %d" % NC),
                       (lambda: e.select_chains([-1], FIRST, T), "chains[0] = -1")):
        try:
            call()
            raise AssertionError("not refused: " + text)
        except M.McxError as err:
            assert err.code == 1 and text in str(err), str(err)
    ms = e.chain_table_times(first_step=FIRST, nsteps=T)
    assert ms.shape == (3,) and (ms > 0).all() and ms[2] >= ms[0] + ms[1]
    # keep, select, close the engine: the store lives on
    reasons, centre, kept = E.keep_chains(t, z=5.0, min_moves=1)
    want = R.keep(ref, z=5.0, min_moves=1)
    assert np.array_equal(reasons, want[0]) and np.array_equal(kept, want[2]) and kept.size >= 1
    st = e.select_chains(kept, first_step=FIRST, nsteps=T)
    st_b = e.select_chains(kept, first_step=FIRST, nsteps=T)
    e.close()
    assert st.shape == (T, kept.size, NP + 1)
    got = st.rows()
    assert same_bits(got, R.select(rows, T, NC, kept)) and same_bits(got, st_b.rows())
    st_b.close()
    tk = st.chain_table()
    assert all(same_bits(tk[k], t[k][kept]) for k in ("moves", "longest_stay", "ll_max", "ll_max_step", "flags"))
    assert same_bits(tk["mean"], t["mean"][kept]) and same_bits(tk["rho1"], t["rho1"][kept])  # a series' own operations
    sk = st.summary()
    assert np.isfinite(sk["rhat"]).all()
    sub = st.select_chains([0, 0, kept.size - 1])
    assert same_bits(sub.rows(), R.select(got, T, kept.size, [0, 0, kept.size - 1]))
    sub.close()
    st.close()
    assert E.debug_live_resources() == (0, 0, 0, 0), E.debug_live_resources()
    print("chains engine: all scenarios done")


if __name__ == "__main__":
    main()
