"""mcpar-run's derive and draw options: one job with --derive-linear, the three --derived-* files and --draws.  The files
parse, name d0 .. d{K-1} and LL, hold what derive_rows(...) of the job's own rows gives at the writers' precision (%.17g
round-trips a double), and the draws are lines of the job's output, the ones the index rule picks."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_driver_derive_and_draws(tmp_path):
    import mcpar_amd as M
    from mcpar_amd import engine as E
    drv = os.path.join(ROOT, "mcpar_amd", "drivers", "mcpar-run")
    d, nc, nsamp, K, ndraw, seed = 3, 16, 40, 2, 25, 77
    A = np.array([[1.0, -1.0, 0.0], [0.5, 0.25, -2.0]], np.float32)
    b = np.array([0.0, 1.5], np.float32)
    (tmp_path / "lin.txt").write_text("\n".join(" ".join(repr(float(v)) for v in list(A[j]) + [b[j]]) for j in range(K)) + "\n")
    r = subprocess.run([drv, "--func", "gauss", "--np", str(d), "--nc", str(nc), "--nsamp", str(nsamp), "--nburn", "60", "--binary",
                        "--out", "rows.bin", "--derive-linear", "lin.txt", "--derived-summary", "ds.txt", "--derived-rank-summary",
                        "dr.txt", "--derived-covariance", "dc.txt", "--draws", "draws.txt", "--ndraw", str(ndraw), "--draw-seed",
                        str(seed)], cwd=tmp_path, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, d + 1)
    assert rows.shape[0] == nsamp * nc
    st = M.derive_rows(rows, nsamp, nc, M.derive_linear(A, b))
    names = ["d0", "d1", "LL"]

    summ = st.summary((0.01, 0.5, 0.99))
    lines = (tmp_path / "ds.txt").read_text().splitlines()
    assert lines[0].split() == ["name", "mean", "sd", "q01", "q50", "q99", "rhat", "ess", "mcse"]
    assert [ln.split()[0] for ln in lines[1:]] == names
    for c, ln in enumerate(lines[1:]):
        t = ln.split()
        assert t[1] == "%.17g" % summ["mean"][c]
        want = [summ["mean"][c], summ["sd"][c]] + list(summ["quantiles"][c]) + [summ["rhat"][c], summ["ess"][c], summ["mcse_mean"][c]]
        assert [float(v) for v in t[1:]] == want

    rank = st.rank_summary()
    lines = (tmp_path / "dr.txt").read_text().splitlines()
    assert [ln.split()[0] for ln in lines[1:]] == names and len(lines[0].split()) == 13
    fields = ["rhat", "rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "ess_q05", "ess_q95", "q05", "median", "q95"]
    for c, ln in enumerate(lines[1:]):
        assert [float(v) for v in ln.split()[1:11]] == [rank[f][c] for f in fields]

    cov = st.covariance()
    lines = (tmp_path / "dc.txt").read_text().splitlines()
    assert lines[0].split() == ["name", "mean"] + names
    assert [ln.split()[0] for ln in lines[1:]] == names
    for c, ln in enumerate(lines[1:]):
        assert [float(v) for v in ln.split()[1:]] == [cov["mean"][c]] + list(cov["cov"][c])

    draws = (tmp_path / "draws.txt").read_bytes()
    index = M.debug_draw_indices(seed, nsamp * nc, 0, ndraw)
    assert draws == E.format_rows(rows[index])
    job_lines = set(E.format_rows(rows).splitlines())
    assert len(draws.splitlines()) == ndraw and all(ln in job_lines for ln in draws.splitlines())

    # a --derived-* file without a function, and the conditions of --summary
    bad = subprocess.run([drv, "--func", "gauss", "--np", "3", "--nc", "16", "--nsamp", "8", "--nburn", "10", "--quiet",
                          "--derived-summary", "x.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert bad.returncode == 2 and b"--derive-source" in bad.stderr
    bad = subprocess.run([drv, "--func", "gauss", "--np", "3", "--nc", "16", "--nsamp", "8", "--nburn", "10", "--stream-text",
                          "--draws", "x.txt", "--ndraw", "3"], cwd=tmp_path, capture_output=True, timeout=300)
    assert bad.returncode == 2 and b"--draws" in bad.stderr
