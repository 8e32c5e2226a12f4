"""mcpar-run --step-table / --step-probs / --settle against the Python binding's step table of the run's own --out rows: the
line counts, the headers and the step column 0 .. T - 1; the doubles come back as the library returned them (17 significant
digits), the floats from 9, the counts as integers; the settle lines are settle_steps' on that table."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "mcpar_amd", "drivers")
NC, T = 64, 12
ARGS = [os.path.join(DRV, "mcpar-run"), "--func", "gauss", "--np", "4", "--nc", str(NC), "--nsamp", str(T), "--nburn", "40", "--binary"]
NAMES = ["p0", "p1", "p2", "p3", "LL"]


def same(a, b):
    """equal, NaN where NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(b)], b[~np.isnan(b)])


def test_driver_step_table(tmp_path):
    from mcpar_amd import engine as E
    probs = (0.1, 0.5, 0.75, 1.0)
    a = subprocess.run(ARGS + ["--out", "rows.bin", "--step-table", "s.txt", "--step-probs", "0.1,0.5,0.75,1", "--settle", "0.5,0.4,0.25"],
                       cwd=tmp_path, capture_output=True, timeout=300)
    assert a.returncode == 0, a.stderr.decode()
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, 5)
    assert rows.shape[0] == T * NC
    ref = E.rows_step_table(rows, T, NC, probs)
    lines = open(tmp_path / "s.txt").read().splitlines()
    assert len(lines) == 1 + T * 5 + 1 + T + 1 + 1 + 5
    assert lines[0].split() == ["step", "column", "mean", "sd", "min", "q0.1", "q0.5", "q0.75", "q1", "max"]
    tok = [ln.split() for ln in lines[1:1 + T * 5]]
    assert [int(t[0]) for t in tok] == [s for s in range(T) for _ in range(5)]   # the iteration mcparam.itercount puts back
    assert [t[1] for t in tok] == NAMES * T and all(len(t) == 10 for t in tok)
    v = np.array([[float(x) for x in t[2:]] for t in tok]).reshape(T, 5, 8)
    assert same(v[:, :, 0], ref["mean"]) and same(v[:, :, 1], ref["sd"])
    assert same(v[:, :, 2].astype(np.float32), ref["min"]) and same(v[:, :, 7].astype(np.float32), ref["max"])
    assert same(v[:, :, 3:7], ref["quantiles"])
    assert same(v[:, :, 6], ref["max"].astype(np.float64))  # p = 1
    k = 1 + T * 5
    assert lines[k].split() == ["step", "moved", "ll_max", "ll_max_chain"]
    tok = [ln.split() for ln in lines[k + 1:k + 1 + T]]
    assert [int(t[0]) for t in tok] == list(range(T)) and [int(t[1]) for t in tok] == ref["moved"].tolist()
    assert same(np.array([float(t[2]) for t in tok], np.float32), ref["ll_max"]) and [int(t[3]) for t in tok] == ref["ll_max_chain"].tolist()
    assert ref["moved"][0] == -1 and (ref["moved"][1:] > 0).all()
    # the rule
    settled, cols = E.settle_steps(ref, tol_mean=0.5, tol_sd=0.4, ref_frac=0.25)
    k += 1 + T
    assert lines[k] == ("settled at step %d of %d" % (settled, T) if settled >= 0 else "not settled")
    assert lines[k + 1].split() == ["column", "m_ref", "s_ref", "last_out", "max_dev_mean", "max_dev_sd"]
    for c, ln in enumerate(lines[k + 2:]):
        t = ln.split()
        assert t[0] == NAMES[c] and int(t[3]) == cols["last_out"][c]
        assert same([float(t[1]), float(t[2]), float(t[4]), float(t[5])],
                    [cols["m_ref"][c], cols["s_ref"][c], cols["max_dev_mean"][c], cols["max_dev_sd"][c]])
    # the default probabilities and no rule: three quantile columns, no settle lines
    b = subprocess.run(ARGS + ["--out", "rows.bin", "--step-table", "s2.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert b.returncode == 0, b.stderr.decode()
    lines = open(tmp_path / "s2.txt").read().splitlines()
    assert len(lines) == 1 + T * 5 + 1 + T and lines[0].split()[5:8] == ["q0.05", "q0.5", "q0.95"]
    # refused: a probability out of range by the library; no rows on the host and a rule without a file by the driver
    c = subprocess.run(ARGS + ["--step-table", "e.txt", "--step-probs", "0.5,1.5"], cwd=tmp_path, capture_output=True, timeout=300)
    assert c.returncode == 2 and b"--step-table" in c.stderr and b"probs[1] = 1.5" in c.stderr
    d = subprocess.run(ARGS[:-1] + ["--stream-text", "--step-table", "f.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert d.returncode == 2 and b"--step-table" in d.stderr
    e = subprocess.run(ARGS + ["--settle", "0.1"], cwd=tmp_path, capture_output=True, timeout=300)
    assert e.returncode == 2 and b"--settle" in e.stderr
