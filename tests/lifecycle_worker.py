"""The scenarios of tests/test_gpu_lifecycle.py, in a process of their own: nothing else of the suite is alive here, so
mcx_debug_live_resources starts at (0, 0, 0, 0) and must be back there whenever every engine and store is closed.
Before a close the category a scenario is about must be above zero -- a scenario that no longer reaches its lazily created
streams and events fails instead of passing.  Every shape is the smallest that still reaches the code."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mcpar_amd as M  # noqa: E402
from mcpar_amd import engine as E  # noqa: E402

DEVICE, PINNED, STREAMS, EVENTS = range(4)
NP, NC, NBURN, NSAMP = 4, 64, 8, 8


def live():
    return E.debug_live_resources()


def all_gone(what):
    assert live() == (0, 0, 0, 0), (what, live())
    print("ok:", what, flush=True)


def refused(call, *args):
    try:
        call(*args)
    except M.McxError:
        return
    raise AssertionError("%s%r was not refused" % (getattr(call, "__name__", call), args))


def pinit(d, n):
    g, i = np.arange(n, dtype=np.float64)[:, None], np.arange(d, dtype=np.float64)[None, :]
    return (0.5 * np.sin(0.37 * (g * d + i))).astype(np.float32)


def gauss(d=NP):
    return M.make_vlfunc(M.VL_GAUSSIAN, d)


def plain_run():
    vl, _keep = gauss()
    e = M.Engine(NP, NC)
    e.run(NSAMP, NBURN, pinit(NP, NC), vl)
    for name in ("state", "loglike", "mean", "var", "musigall", "chol", "accept_counts", "counters", "tuner_trace", "samples"):
        getattr(e, name)
    assert len(e.samples_text(0, NSAMP)) > 0
    e.maxlike()
    e.summary()
    e.rank_summary()
    e.covariance()
    e.draw(10, 1)
    assert live()[DEVICE] > 0 and live()[PINNED] > 0
    e.close()
    all_gone("plain run, every getter")


def async_runs():
    vl, _keep = gauss()
    e = M.Engine(NP, NC, pl=1.0)
    e.set_option(E.OPT_ASYNC_RUN, 1)
    p = pinit(NP, NC)
    e.run(NSAMP, NBURN, p, vl)  # from host memory: kept in pinit_async, the counters come on astream behind run_ev / copy_ev
    e.run(NSAMP, NBURN, p, vl)
    assert live()[STREAMS] > 0 and live()[EVENTS] > 0, live()
    e.close()  # nobody has looked at either run
    all_gone("two asynchronous runs from host pinit, closed unsynchronised")


def sinks():
    vl, _keep = gauss()
    e = M.Engine(NP, NC)
    e.set_option(E.OPT_SINK_TEXT, 1)
    texts = []

    def rows_sink(first, nsteps, rows):
        texts.append(e.sink_text())
        return 0
    e.set_sink(rows_sink, 4)
    e.run(NSAMP, NBURN, pinit(NP, NC), vl)
    assert len(texts) == 2 and all(texts)
    assert live()[STREAMS] >= 2 and live()[EVENTS] > 0 and live()[PINNED] > 0, live()  # cstream, tstream, ev_*, sink_pin
    e.close()
    all_gone("row sink with text")
    e = M.Engine(NP, NC)
    blocks = []
    e.set_text_sink(lambda first, nsteps, text: blocks.append(bytes(text)) or 0, 4)
    e.run(NSAMP, NBURN, pinit(NP, NC), vl)
    assert len(blocks) == 2 and all(blocks)
    assert live()[STREAMS] >= 2 and live()[EVENTS] > 0, live()
    e.close()
    all_gone("text sink")


def murray_run():
    # tests/test_gpu_murray_cull.py's "rosen16" at the fewest chains a pass is cut into column chunks for (OVERLAP_MIN_CHAINS
    # = 8192 in mcx_murray.hip, asked for in screen_pass_dm), a short job
    d, n = 16, 8192
    vl, _keep = M.make_vlfunc(M.VL_ROSENBROCK1, d)
    e = M.Engine(d, n, pl=0.85)
    e.set_option(E.OPT_SAMPLES, 0)
    e.set_option(E.OPT_CULL, 3)
    e.set_option(E.OPT_MURRAY_OVERLAP, 2)
    e.run(30, 60, pinit(d, n), vl)
    c = e.counters
    assert c["remote_steps"] > 0 and c["remote_pairs_evaluated"] < c["remote_pairs"], c  # Murray steps, and the screens ran
    assert live()[STREAMS] > 0 and live()[EVENTS] > 0, live()  # mstream, mev: the chunked sweep
    e.close()
    all_gone("Murray run with screens and the chunked sweep")


def profiled_run():
    vl, _keep = gauss()
    e = M.Engine(NP, NC)
    e.set_option(E.OPT_PROFILE, 1)
    e.run(NSAMP, NBURN, pinit(NP, NC), vl)  # (a run collects its own event pairs when it ends)
    e.gen_local(0, pinit(NP, NC))  # a launch outside a run: its pair waits in evs for profile(), which nobody calls
    assert live()[EVENTS] >= 2, live()
    e.close()
    all_gone("profiled run, profile never read")


def device_vlfunc(tmp):
    """(vlfunc, module handle, hip): the user kernel of tests/test_gpu_device_vlfunc.py"""
    co = os.path.join(tmp, "user.co")
    subprocess.check_call(["hipcc", "--genco", "--offload-arch=gfx950", "-O2", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "cpp", "user_vlfunc_kernel.hip"), "-o", co])
    hip = C.CDLL("libamdhip64.so")
    mod, fn = C.c_void_p(), C.c_void_p()
    assert hip.hipModuleLoad(C.byref(mod), co.encode()) == 0
    assert hip.hipModuleGetFunction(C.byref(fn), mod, b"user_rosenbrock8") == 0
    return M.make_vlfunc(M.VL_DEVICE, 8, device_fn=fn.value), mod, hip


def standalone(tmp):
    lib = M.load()
    rng = np.random.default_rng(7)
    fp = C.POINTER(C.c_float)
    x = rng.normal(size=(5, 4)).astype(np.float32)
    assert np.isfinite(E.vlfunc_eval(M.VL_GAUSSIAN, 4, x)).all()
    refused(E.vlfunc_eval, M.VL_ROSENBROCK1, 3, x[:, :3])  # an odd N
    all_gone("vlfunc_eval, built-in")
    (vd, _keep), mod, hip = device_vlfunc(tmp)
    x8, y8 = rng.normal(size=(5, 8)).astype(np.float32), np.empty(5, np.float32)
    M._lib.check(lib.mcx_vlfunc_eval(C.byref(vd), 5, x8.ctypes.data_as(fp), y8.ctypes.data_as(fp)))
    assert np.isfinite(y8).all()
    bad, _keep2 = M.make_vlfunc(M.VL_DEVICE, 8)  # no kernel
    assert lib.mcx_vlfunc_eval(C.byref(bad), 5, x8.ctypes.data_as(fp), y8.ctypes.data_as(fp)) != 0
    hip.hipModuleUnload(mod)
    all_gone("vlfunc_eval, MCX_VL_DEVICE")
    nc, T = 8, 8
    rows = rng.normal(size=(T * nc, 3)).astype(np.float32)
    E.rows_summary(rows, T, nc)
    refused(E.rows_summary, rows[:3 * nc], 3, nc)  # two half-chains need four steps: refused with the rows uploaded
    all_gone("rows_summary")
    E.rows_rank_summary(rows, T, nc)
    refused(E.rows_rank_summary, rows[:3 * nc], 3, nc)
    all_gone("rows_rank_summary")
    E.rows_covariance(rows, T, nc)
    refused(E.rows_covariance, rows, 0, nc)
    all_gone("rows_covariance")
    assert len(E.format_rows(rows)) > 0
    refused(E.format_rows, np.zeros((2, 0), np.float32))
    all_gone("format_rows")
    spec = E.derive_linear(np.ones((1, 2), np.float32), np.zeros(1, np.float32))
    s = E.derive_rows(rows, T, nc, spec)
    assert s.shape == (T, nc, 2) and live()[DEVICE] > 0 and live()[STREAMS] == 1, live()
    s.rows(); s.summary(); s.rank_summary(); s.covariance(); s.draw(5, 1)
    s.close()
    refused(E.derive_rows, rows, T, nc, None)
    refused(E.derive_rows, rows, 0, nc, spec)
    all_gone("derive_rows with derive_linear")
    w = np.arange(1, 9, dtype=np.uint32)
    assert E.debug_numerics(0, w).shape == w.shape
    assert lib.mcx_debug_numerics(0, 1, None, None) != 0
    assert E.debug_normals(1, 2, 3, 4, 5, 6, 8).shape == (8, 4)
    assert lib.mcx_debug_normals(1, 2, 3, 4, 5, 6, 1, None) != 0
    ms = np.empty((128, 16, 2), np.float32)
    ms[:, :, 0] = rng.normal(0.4, 0.4, (128, 16))
    ms[:, :, 1] = 0.01
    E.debug_murray_screen(ms[:64, :, 0].copy(), ms)
    refused(E.debug_murray_screen, ms[:64, :8, 0].copy(), ms[:, :8])  # np = 8
    all_gone("debug_numerics, debug_normals, debug_murray_screen")


def store_outlives_engine():
    vl, _keep = gauss()
    e = M.Engine(NP, NC)
    e.run(NSAMP, NBURN, pinit(NP, NC), vl)
    s = e.derive(E.derive_linear(np.ones((2, NP), np.float32), np.zeros(2, np.float32)))
    e.close()
    assert live()[DEVICE] > 0 and live()[STREAMS] == 1, live()
    assert s.rows().shape == (NSAMP * NC, 3)
    s.close()
    all_gone("a derived store that outlives its engine")


def create_refused():
    refused(M.Engine, 257, NC)
    refused(M.Engine, NP, 0)
    all_gone("mcx_create refused")


def rccl_exchange():
    if not E.rccl_available():
        print("skipped: no RCCL on this machine", flush=True)
        return
    vl, _keep = gauss()
    e = M.Engine(NP, NC, pl=0.8)
    e.rccl_init(E.rccl_unique_id())
    e.debug_exchange()  # one gather on xstream, between xready and xdone (a run of one shard has none of its own)
    e.run(NSAMP, NBURN, pinit(NP, NC), vl)
    assert live()[STREAMS] > 0 and live()[EVENTS] >= 2, live()
    e.close()
    all_gone("1-rank RCCL exchange")


def main():
    assert live() == (0, 0, 0, 0), live()
    plain_run()
    async_runs()
    sinks()
    murray_run()
    profiled_run()
    with tempfile.TemporaryDirectory() as tmp:
        standalone(tmp)
    store_outlives_engine()
    create_refused()
    rccl_exchange()
    print("lifecycle: all scenarios done", flush=True)


if __name__ == "__main__":
    main()
