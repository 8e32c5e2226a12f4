"""mcpar-run --read: a run's own --out file read back on the GPU.  The --summary and --step-table files of the file equal those
the Python binding makes of the rows tests/parse_ref.py reads from it (the doubles come back from 17 significant digits); --np,
--read-skip and --read-rows; the refusals exit with 2."""
import os
import subprocess

import numpy as np
import pytest

import parse_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "mcpar_amd", "drivers", "mcpar-run")
NC, T, NP = 64, 12, 4


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(b)], b[~np.isnan(b)])


def summary_file(path):
    lines = open(path).read().splitlines()
    assert lines[0].split() == ["name", "mean", "sd", "q01", "q50", "q99", "rhat", "ess", "mcse"]
    return [ln.split()[0] for ln in lines[1:]], np.array([[float(x) for x in ln.split()[1:]] for ln in lines[1:]])


def test_driver_reads_its_own_dump(tmp_path):
    from mcpar_amd import engine as E
    run = lambda *a: subprocess.run([RUN] + list(a), cwd=tmp_path, capture_output=True, timeout=300)
    a = run("--func", "gauss", "--np", str(NP), "--nc", str(NC), "--nsamp", str(T), "--nburn", "40", "--quiet", "--out", "F.txt",
            "--summary", "S1.txt")
    assert a.returncode == 0, a.stderr.decode()
    text = (tmp_path / "F.txt").read_bytes()
    ref, ncol, _ = R.parse(text, 0, NC)
    rows = ref.view(np.float32)
    assert ncol == NP + 1 and rows.shape == (T * NC, NP + 1)
    b = run("--read", "F.txt", "--nc", str(NC), "--summary", "S2.txt", "--step-table", "T2.txt")
    assert b.returncode == 0, b.stderr.decode()
    assert b"read %d rows of %d columns" % (T * NC, NP + 1) in b.stderr and b"0 tokens through strtof" in b.stderr
    names, v = summary_file(tmp_path / "S2.txt")
    s = E.rows_summary(rows, T, NC)
    assert names == ["p0", "p1", "p2", "p3", "LL"]
    assert same(v[:, 0], s["mean"]) and same(v[:, 1], s["sd"]) and same(v[:, 2:5], s["quantiles"])
    assert same(v[:, 5], s["rhat"]) and same(v[:, 6], s["ess"]) and same(v[:, 7], s["mcse_mean"])
    st = E.rows_step_table(rows, T, NC)
    lines = open(tmp_path / "T2.txt").read().splitlines()
    tok = [ln.split() for ln in lines[1:1 + T * (NP + 1)]]
    assert [int(t[0]) for t in tok] == [k for k in range(T) for _ in range(NP + 1)]
    assert same(np.array([float(t[2]) for t in tok]).reshape(T, NP + 1), st["mean"])
    # --np names the columns, --read-skip / --read-rows frame the rows: a header line and the last two steps left out
    (tmp_path / "G.txt").write_bytes(b"nsamp = 12\n" + text)
    c = run("--read", "G.txt", "--nc", str(NC), "--np", str(NP), "--read-skip", "1", "--read-rows", str((T - 2) * NC), "--summary", "S3.txt")
    assert c.returncode == 0, c.stderr.decode()
    _, v3 = summary_file(tmp_path / "S3.txt")
    s3 = E.rows_summary(rows[:(T - 2) * NC], T - 2, NC)
    assert same(v3[:, 0], s3["mean"]) and same(v3[:, 2:5], s3["quantiles"])
    # refused, exit 2: options of a run, no --nc, the wrong --np, a file that is not there, rows that do not fill the chains
    for extra in (["--nsamp", "5"], ["--nburn", "5"], ["--func", "gauss"], ["--out", "x.txt"], ["--stream-text"]):
        d = run("--read", "F.txt", "--nc", str(NC), *extra)
        assert d.returncode == 2 and b"--read" in d.stderr and extra[0].encode() in d.stderr, extra
    assert run("--read", "F.txt").returncode == 2
    e = run("--read", "F.txt", "--nc", str(NC), "--np", "3")
    assert e.returncode == 2 and b"line 1: 5 fields, expected 4" in e.stderr
    assert run("--read", "none.txt", "--nc", str(NC)).returncode == 2
    f = run("--read", "F.txt", "--nc", "7")
    assert f.returncode == 2 and b"multiple of nc" in f.stderr
    assert run("--nc", "4", "--read-skip", "1").returncode == 2
