"""bench.py --dump-outputs without a GPU: dump_outputs on a stand-in engine writes float32 files, at most 64 MB in all, the
sample rows of the steps and chains it names, and the same bytes every time for the same job."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    saved = dict(os.environ)  # bench.py sets a default in the environment when imported: keep it out of the other tests
    try:
        sys.path.insert(0, ROOT)
        import bench
    finally:
        os.environ.clear()
        os.environ.update(saved)
    return bench


class StandInEngine:
    """what dump_outputs reads of mcpar_amd.Engine; every value says where it came from"""

    def __init__(self, d, n):
        self.d, self.n = d, n
        self.chain = np.arange(n, dtype=np.float32)[:, None]

    @property
    def state(self): return self.chain + np.arange(self.d, dtype=np.float32) / 64
    @property
    def loglike(self): return -self.chain[:, 0]
    @property
    def mean(self): return self.state + 0.5
    @property
    def var(self): return self.state + 0.25

    def samples_range(self, first_step, nsteps):
        assert nsteps == 1
        return (self.chain * 1e-3 + np.float32(first_step)) + np.zeros((1, self.d + 1), np.float32)


@pytest.mark.parametrize("d,n,nsamp", [(16, 65536, 1000), (8, 4096, 1000), (32, 1 << 19, 100)], ids=["c3", "c2", "many-chains"])
def test_dump_fits_the_budget_and_says_what_it_sampled(tmp_path, d, n, nsamp):
    bench = load_bench()
    out = bench.dump_outputs(StandInEngine(d, n), d, n, nsamp, True, str(tmp_path))
    names = sorted(os.listdir(tmp_path))
    assert names == ["loglike.npy", "mean.npy", "samples.npy", "state.npy", "var.npy"]
    assert sum(os.path.getsize(tmp_path / f) for f in names) <= 64 * 10**6
    arrays = {f[:-4]: np.load(tmp_path / f) for f in names}
    assert all(a.dtype == np.float32 for a in arrays.values())
    chains = arrays["loglike"].astype(np.int64) * -1  # the stand-in's loglike is minus the chain index
    assert np.all(np.diff(chains) > 0) and chains[-1] < n
    if out["chains"] == "all":
        assert len(chains) == n
    else:
        assert n * (3 * d + 1) * 4 > bench.DUMP_BYTES // 2 and out["chains"].startswith("%d of %d" % (len(chains), n))
    assert arrays["state"].shape == (len(chains), d) and np.array_equal(arrays["state"][:, 0], chains.astype(np.float32))
    steps = out["sample_steps"]
    assert 1 <= len(steps) <= min(nsamp, bench.DUMP_MAX_STEPS) and steps == sorted(set(steps)) and steps[-1] < nsamp
    s = arrays["samples"]
    assert s.shape == (len(steps), len(chains), d + 1)
    assert np.array_equal(np.rint(s[:, 0, 0]), np.array(steps, np.float32) + np.rint(chains[0] * 1e-3))
    assert out["files"] == {f: list(arrays[f[:-4]].shape) for f in names}


def test_same_job_same_bytes_and_no_rows_without_samples(tmp_path):
    bench = load_bench()
    d, n = 32, 1 << 19
    for sub in ("a", "b"):
        bench.dump_outputs(StandInEngine(d, n), d, n, 100, True, str(tmp_path / sub))
    for f in os.listdir(tmp_path / "a"):
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f
    out = bench.dump_outputs(StandInEngine(d, 64), d, 64, 100, False, str(tmp_path / "c"), "_shard1")
    assert sorted(os.listdir(tmp_path / "c")) == ["loglike_shard1.npy", "mean_shard1.npy", "state_shard1.npy", "var_shard1.npy"]
    assert out["sample_steps"] == [] and out["chains"] == "all"
