"""mcpar-run --reweight / --resampled against the Python binding on the same rows: the file holds the library's numbers, doubles
with 17 significant digits and floats with 9, so the text is compared as text.  The resampled rows are read back by the parser
(DESIGN.md section 18): every one of them is a row of the run, to the six digits of the sample text."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "mcpar_amd", "drivers")
NC, T = 64, 12
ARGS = [os.path.join(DRV, "mcpar-run"), "--func", "gauss", "--np", "4", "--nc", str(NC), "--nsamp", str(T), "--nburn", "40", "--quiet"]
NAMES = ["p0", "p1", "p2", "p3", "LL"]
PROBS = (0.05, 0.5, 0.95)
TEMPER = """
__device__ void mcx_user_derive(const float *x, int d, float ly, const float *par, float *out, int nout)
{
  out[0] = par[0] * ly;
}
"""


def text_of(d):
    lines = [" ".join(["%d" % d["n"], "%d" % d["nzero"], "%.17g" % d["lwmax"], "%d" % d["sumq"], "%d" % d["sumq2_hi"], "%d" % d["sumq2_lo"],
                       "%.17g" % d["ess_kish"], "%.17g" % d["log_mean_w"], "%d" % d["tail_m"], "%.17g" % d["khat"], "%.17g" % d["tail_sigma"],
                       "%d" % d["flags"]])]
    c = d["cols"]
    for k, name in enumerate(NAMES):
        v = [name] + ["%.17g" % c[f][k] for f in ("mean", "sd", "mcse_mean")] + ["%.9g" % c["min"][k], "%.9g" % c["max"][k]]
        v += ["%.17g" % q for q in d["quantiles"][k]] + ["%d" % c["flags"][k]]
        lines.append(" ".join(v))
    return lines


def test_driver_reweight(tmp_path):
    from mcpar_amd import engine as E
    a = subprocess.run(ARGS + ["--binary", "--out", "rows.bin", "--reweight-temper", "0.5", "--reweight", "t.txt"], cwd=tmp_path,
                       capture_output=True, timeout=300)
    assert a.returncode == 0, a.stderr.decode()
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, 5)
    assert rows.shape[0] == T * NC
    want = E.reweight_rows(rows, T, NC, E.weights_loglike(0.5 - 1.0), PROBS)
    assert open(tmp_path / "t.txt").read().splitlines() == text_of(want)
    # the same weights from a derive text, and equal weights from a file of zeros
    (tmp_path / "temper.hip").write_text(TEMPER)
    (tmp_path / "zeros.txt").write_text("0\n" * (T * NC))
    b = subprocess.run(ARGS + ["--reweight-source", "temper.hip", "--derive-par", "-0.5", "--reweight", "s.txt"], cwd=tmp_path,
                       capture_output=True, timeout=300)
    assert b.returncode == 0, b.stderr.decode()
    assert open(tmp_path / "s.txt").read() == open(tmp_path / "t.txt").read()
    c = subprocess.run(ARGS + ["--reweight-logw", "zeros.txt", "--reweight", "z.txt", "--out", "dump.txt", "--resampled", "r.txt",
                               "--resample-n", "500", "--resample-seed", "3", "--resampled-density", "d.txt", "--density-n", "32"],
                       cwd=tmp_path, capture_output=True, timeout=300)
    assert c.returncode == 0, c.stderr.decode()
    equal = E.reweight_rows(rows, T, NC, E.weights_host(np.zeros(T * NC, np.float32)), PROBS)
    assert open(tmp_path / "z.txt").read().splitlines() == text_of(equal)
    assert equal["ess_kish"] == T * NC and equal["sumq"] == (T * NC) << 31
    for k in range(5):
        assert np.array_equal(equal["quantiles"][k], np.quantile(rows[:, k], PROBS, method="inverted_cdf").astype(np.float64))
    # the resampled rows, read back: rows of the run (the text has six digits: compare with the run's own text, parsed)
    dump, _ = E.parse_text(open(tmp_path / "dump.txt", "rb").read(), NC)
    drawn, rep = E.parse_text(open(tmp_path / "r.txt", "rb").read(), 500)
    index = E.debug_draw_indices(3, T * NC, 0, 500)  # equal weights: the unweighted draw's indices
    assert drawn.shape == (500, 5) and drawn.tobytes() == dump[index].tobytes()
    assert len(open(tmp_path / "d.txt").read().splitlines()) == 1 + 5 * 32
    # the same on a file that is read, not run
    d = subprocess.run([ARGS[0], "--read", "dump.txt", "--nc", str(NC), "--quiet", "--reweight-temper", "0.5", "--reweight", "f.txt"],
                       cwd=tmp_path, capture_output=True, timeout=300)
    assert d.returncode == 0, d.stderr.decode()
    assert open(tmp_path / "f.txt").read().splitlines() == text_of(E.reweight_rows(dump, T, NC, E.weights_loglike(-0.5), PROBS))
    # refused by the driver: no source, two sources, draws without a number; by the library: a file of the wrong length
    for extra, word in ((["--reweight", "e.txt"], b"--reweight-temper"),
                        (["--reweight", "e.txt", "--reweight-temper", "0.5", "--reweight-logw", "zeros.txt"], b"exactly one"),
                        (["--reweight-temper", "0.5", "--resampled", "e.txt"], b"--resample-n"),
                        (["--stream-text", "--reweight-temper", "0.5", "--reweight", "e.txt"], b"--reweight")):
        e = subprocess.run(ARGS + extra, cwd=tmp_path, capture_output=True, timeout=300)
        assert e.returncode == 2 and word in e.stderr, (extra, e.stderr)
    (tmp_path / "short.txt").write_text("0\n" * 5)
    f = subprocess.run(ARGS + ["--reweight-logw", "short.txt", "--reweight", "e.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert f.returncode == 2 and b"one per row" in f.stderr
