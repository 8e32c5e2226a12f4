"""The lifetime scenario of tests/test_gpu_density.py, in a process of its own (nothing else of the suite is alive here, so
mcx_debug_live_resources starts at zero): every refusal of the density entry points, then one density of an engine's store,
of host rows and of a derived store; with everything closed the count is (0, 0, 0, 0) again."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mcpar_amd as M  # noqa: E402
from mcpar_amd import engine as E  # noqa: E402

NP, NC, NBURN, NSAMP = 4, 64, 8, 20
NAN = float("nan")


def refused(call, text=None, **kw):
    try:
        call(**kw)
    except M.McxError as err:
        assert err.code == 1, (kw, str(err))
        assert text is None or text in str(err), (kw, str(err))
        return
    raise AssertionError("%r was not refused" % (kw,))


def pinit(d, n):
    g, i = np.arange(n, dtype=np.float64)[:, None], np.arange(d, dtype=np.float64)[None, :]
    return (0.5 * np.sin(0.37 * (g * d + i))).astype(np.float32)


def main():
    assert E.debug_live_resources() == (0, 0, 0, 0)
    vl, _keep = M.make_vlfunc(M.VL_GAUSSIAN, NP)
    e = M.Engine(NP, NC)
    refused(e.density, "the sample store is empty", first_step=0, nsteps=8)  # no run yet
    refused(e.density)
    e.run(NSAMP, NBURN, pinit(NP, NC), vl)
    bad = [NAN] * NP
    for kw in (dict(n=1), dict(n=513), dict(adjust=0.0), dict(adjust=-2.0), dict(adjust=float("inf")), dict(adjust=NAN),
               dict(clip=(0.5, 0.5)), dict(clip=(-0.01, 0.99)), dict(clip=(0.01, 1.01)), dict(clip=(0.9, 0.1)),
               dict(bw=bad + [0.0]), dict(bw=[-1.0] + bad), dict(from_=bad + [1.0], to=bad + [0.0]),
               dict(from_=[1e30] + bad)):  # (the last one: above the column's own maximum)
        refused(e.density, **kw)
    for kw in (dict(first_step=0, nsteps=NSAMP + 1), dict(first_step=-1, nsteps=4), dict(first_step=NSAMP - 3, nsteps=4)):
        refused(e.density, "not in the sample store", **kw)
    refused(e.density, first_step=0, nsteps=0)
    one = M.Engine(NP, 1)  # N = 1
    one.run(4, 4, pinit(NP, 1), vl)
    refused(one.density, "nsteps * nc >= 2", first_step=0, nsteps=1)
    assert one.density(first_step=0, nsteps=2)["nvalues"].tolist() == [2] * (NP + 1)
    one.close()

    d = e.density(n=64)
    assert d["y"].shape == (NP + 1, 64) and np.all(d["nbinned"] == NSAMP * NC)
    rows = e.samples
    r = E.rows_density(rows, NSAMP, NC, n=64)
    assert all(d[k].tobytes() == r[k].tobytes() for k in d)
    st = e.derive(M.derive_linear(np.eye(NP, dtype=np.float32), np.zeros(NP, np.float32)))
    s = st.density(n=64)
    assert all(d[k].tobytes() == s[k].tobytes() for k in d)
    for kw in (dict(n=1), dict(adjust=0.0), dict(bw=[0.0] + bad)):
        refused(st.density, **kw)
    for kw in (dict(n=600), dict(clip=(0.7, 0.2))):
        refused(lambda **k: E.rows_density(rows, NSAMP, NC, **k), **kw)
    assert e.density_times(n=64).shape == (4,)
    assert E.debug_live_resources()[0] > 0

    e.set_option(E.OPT_SAMPLES, 0)
    e.run(NSAMP, 0, pinit(NP, NC), vl)
    refused(e.density, "the sample store is empty", first_step=0, nsteps=8)
    refused(e.density)
    st.close()
    e.close()
    assert E.debug_live_resources() == (0, 0, 0, 0), E.debug_live_resources()
    print("density lifetime: all scenarios done")


if __name__ == "__main__":
    main()
