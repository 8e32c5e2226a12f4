"""mcpar-run --density / --derived-density: the long-form files (`column x density`, n lines per column) against
rows_density of the run's own --out rows.  The numbers are printed with 17 significant digits, so they come back as the
doubles the library returned; the tolerances are test_driver_summary's (mean and sd 1e-9 relative there, as x and y here)."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "mcpar_amd", "drivers")
ARGS = [os.path.join(DRV, "mcpar-run"), "--func", "gauss", "--np", "4", "--nc", "256", "--nsamp", "101", "--nburn", "100", "--binary"]


def parse(path, names, n):
    lines = open(path).read().splitlines()
    assert lines[0].split() == ["column", "x", "density"]
    assert len(lines) == 1 + n * len(names)
    tok = [ln.split() for ln in lines[1:]]
    assert [t[0] for t in tok] == [nm for nm in names for _ in range(n)]
    v = np.array([[float(t[1]), float(t[2])] for t in tok]).reshape(len(names), n, 2)
    return v[:, :, 0], v[:, :, 1]


def test_driver_density(tmp_path):
    from mcpar_amd import engine as E
    a = subprocess.run(ARGS + ["--out", "rows.bin", "--density", "d.txt", "--density-n", "64"], cwd=tmp_path, capture_output=True, timeout=300)
    assert a.returncode == 0, a.stderr.decode()
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, 5)
    assert rows.shape[0] == 101 * 256
    x, y = parse(tmp_path / "d.txt", ["p0", "p1", "p2", "p3", "LL"], 64)
    ref = E.rows_density(rows, 101, 256, n=64)
    np.testing.assert_allclose(x, ref["x"], rtol=1e-9)
    np.testing.assert_allclose(y, ref["y"], rtol=1e-9, atol=1e-10 * ref["y"].max())
    # the default n and a clip pair
    b = subprocess.run(ARGS + ["--out", "rows.bin", "--density", "c.txt", "--density-clip", "0.01,0.99"], cwd=tmp_path,
                       capture_output=True, timeout=300)
    assert b.returncode == 0, b.stderr.decode()
    x, y = parse(tmp_path / "c.txt", ["p0", "p1", "p2", "p3", "LL"], 512)
    ref = E.rows_density(rows, 101, 256, clip=(0.01, 0.99))
    np.testing.assert_allclose(x, ref["x"], rtol=1e-9)
    np.testing.assert_allclose(y, ref["y"], rtol=1e-9, atol=1e-10 * ref["y"].max())
    assert x[4, -1] == float(rows[:, 4].max())
    # refused: a bad n by the library, no rows on the host by the driver
    c = subprocess.run(ARGS + ["--density", "e.txt", "--density-n", "1"], cwd=tmp_path, capture_output=True, timeout=300)
    assert c.returncode == 2 and b"--density" in c.stderr
    d = subprocess.run(ARGS[:-1] + ["--stream-text", "--density", "f.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert d.returncode == 2 and b"--density" in d.stderr


def test_driver_derived_density(tmp_path):
    import mcpar_amd as M
    from mcpar_amd import engine as E
    A = np.array([[1.0, -1.0, 0.0, 0.5], [0.25, 0.25, 0.25, 0.25]], np.float32)
    bvec = np.array([0.5, -2.0], np.float32)
    (tmp_path / "lin.txt").write_text("\n".join(" ".join(repr(float(v)) for v in list(A[j]) + [bvec[j]]) for j in range(2)) + "\n")
    a = subprocess.run(ARGS + ["--out", "rows.bin", "--derive-linear", "lin.txt", "--derived-density", "dd.txt", "--density-n", "32"],
                       cwd=tmp_path, capture_output=True, timeout=300)
    assert a.returncode == 0, a.stderr.decode()
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, 5)
    x, y = parse(tmp_path / "dd.txt", ["d0", "d1", "LL"], 32)
    st = M.derive_rows(rows, 101, 256, M.derive_linear(A, bvec))
    ref = E.rows_density(st.rows(), 101, 256, n=32)
    st.close()
    np.testing.assert_allclose(x, ref["x"], rtol=1e-9)
    np.testing.assert_allclose(y, ref["y"], rtol=1e-9, atol=1e-10 * ref["y"].max())
    # --derived-density without a derive function
    b = subprocess.run(ARGS + ["--derived-density", "x.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert b.returncode == 2 and b"--derive" in b.stderr
