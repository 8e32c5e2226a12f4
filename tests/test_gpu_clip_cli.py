"""mcpar-run --clip / --clip-report / --clipped / --clipped-density against the Python binding's clip of the run's own --out
rows: the report's thresholds come back as the doubles the library returned (17 significant digits) and its counts as
integers, the kept text is the formatter's bytes for the kept rows, and the density file is RowSet.store(1024).density() to
the tolerances of tests/test_gpu_density_cli.py."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "mcpar_amd", "drivers")
ARGS = [os.path.join(DRV, "mcpar-run"), "--func", "gauss", "--np", "4", "--nc", "256", "--nsamp", "101", "--nburn", "100", "--binary"]
NAMES = ["p0", "p1", "p2", "p3", "LL"]


def parse_density(path, n):
    lines = open(path).read().splitlines()
    assert lines[0].split() == ["column", "x", "density"] and len(lines) == 1 + n * len(NAMES)
    tok = [ln.split() for ln in lines[1:]]
    assert [t[0] for t in tok] == [nm for nm in NAMES for _ in range(n)]
    v = np.array([[float(t[1]), float(t[2])] for t in tok]).reshape(len(NAMES), n, 2)
    return v[:, :, 0], v[:, :, 1]


def test_driver_clip(tmp_path):
    from mcpar_amd import engine as E
    a = subprocess.run(ARGS + ["--out", "rows.bin", "--clip", "0.05,0.95", "--clip-report", "r.txt", "--clipped", "k.txt",
                               "--clipped-density", "d.txt", "--density-n", "64"], cwd=tmp_path, capture_output=True, timeout=300)
    assert a.returncode == 0, a.stderr.decode()
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, 5)
    assert rows.shape[0] == 101 * 256
    rs = E.clip_rows(rows, 101, 256, 0.05, 0.95)
    K = rs.nrows
    assert 1024 <= K < rows.shape[0]
    # the report
    lines = open(tmp_path / "r.txt").read().splitlines()
    assert lines[0].split() == ["column", "lo", "hi", "nbelow", "nabove"] and len(lines) == 7
    for c, ln in enumerate(lines[1:6]):
        t = ln.split()
        assert t[0] == NAMES[c]
        assert float(t[1]) == rs.report["lo"][c] and float(t[2]) == rs.report["hi"][c]
        assert int(t[3]) == rs.report["nbelow"][c] and int(t[4]) == rs.report["nabove"][c]
    T = K // 1024
    assert lines[6] == "kept %d of %d, density of %d rows (%d x 1024), %d left out" % (K, 101 * 256, T * 1024, T, K - T * 1024)
    # the kept rows' text
    assert open(tmp_path / "k.txt", "rb").read() == E.format_rows(rs.rows())
    # the density of the kept rows
    st = rs.store(1024)
    assert st.dropped == K - T * 1024
    ref = st.density(n=64)
    x, y = parse_density(tmp_path / "d.txt", 64)
    np.testing.assert_allclose(x, ref["x"], rtol=1e-9)
    np.testing.assert_allclose(y, ref["y"], rtol=1e-9, atol=1e-10 * ref["y"].max())
    st.close()
    rs.close()
    # --clip-ll-hi and --clip-nc; a report alone ends with K and N
    b = subprocess.run(ARGS + ["--out", "rows.bin", "--clip", "0.1,0.9", "--clip-ll-hi", "inf", "--clip-report", "r2.txt"], cwd=tmp_path,
                       capture_output=True, timeout=300)
    assert b.returncode == 0, b.stderr.decode()
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, 5)
    rs = E.clip_rows(rows, 101, 256, 0.1, 0.9, float("inf"))
    lines = open(tmp_path / "r2.txt").read().splitlines()
    assert lines[5].split()[2] == "inf" and lines[6] == "kept %d of %d" % (rs.nrows, 101 * 256)
    rs.close()
    # refused: probabilities out of order by the library, no rows on the host by the driver, too few rows for one step
    c = subprocess.run(ARGS + ["--clip", "0.9,0.1", "--clip-report", "e.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert c.returncode == 2 and b"--clip" in c.stderr and b"qlo < qhi" in c.stderr
    d = subprocess.run(ARGS[:-1] + ["--stream-text", "--clipped", "f.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert d.returncode == 2 and b"--clipped" in d.stderr
    e = subprocess.run(ARGS + ["--clipped-density", "g.txt", "--clip-nc", "100000"], cwd=tmp_path, capture_output=True, timeout=300)
    assert e.returncode == 2 and b"--clipped-density" in e.stderr
