"""mcpar-run --density2d / --derived-density2d: the long-form files (`a b x y density`, G * G lines per pair) against
rows_density2d of the run's own --out rows.  The numbers are printed with 17 significant digits, so they come back as the
doubles the library returned."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "mcpar_amd", "drivers")
ARGS = [os.path.join(DRV, "mcpar-run"), "--func", "gauss", "--np", "2", "--nc", "256", "--nsamp", "101", "--nburn", "100", "--binary"]


def parse(path, names, G):
    """(x [npairs, G], y [npairs, G], z [npairs, G, G]) of a file whose pairs have these names"""
    lines = open(path).read().splitlines()
    assert lines[0].split() == ["a", "b", "x", "y", "density"]
    assert len(lines) == 1 + G * G * len(names)
    tok = [ln.split() for ln in lines[1:]]
    assert [(t[0], t[1]) for t in tok] == [nm for nm in names for _ in range(G * G)]
    v = np.array([[float(t[2]), float(t[3]), float(t[4])] for t in tok]).reshape(len(names), G, G, 3)
    assert np.all(v[:, :, :, 0] == v[:, :, :1, 0]) and np.all(v[:, :, :, 1] == v[:, :1, :, 1])  # x varies slowest
    return v[:, :, 0, 0], v[:, 0, :, 1], v[:, :, :, 2]


def check(path, names, ref, G):
    x, y, z = parse(path, names, G)
    for p, (a, b) in enumerate(ref["pairs"]):
        assert x[p].tobytes() == ref["axes"][a].tobytes() and y[p].tobytes() == ref["axes"][b].tobytes(), p
    assert z.tobytes() == ref["z"].tobytes()


def test_driver_density2d(tmp_path):
    from mcpar_amd import engine as E
    a = subprocess.run(ARGS + ["--out", "rows.bin", "--density2d", "d.txt", "--density2d-n", "16"], cwd=tmp_path, capture_output=True,
                       timeout=300)
    assert a.returncode == 0, a.stderr.decode()
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, 3)
    assert rows.shape[0] == 101 * 256
    check(tmp_path / "d.txt", [("p0", "p1"), ("p0", "LL"), ("p1", "LL")], E.rows_density2d(rows, 101, 256, g=16), 16)
    # named pairs, the default G and a clip pair
    b = subprocess.run(ARGS + ["--out", "rows.bin", "--density2d", "c.txt", "--density2d-pairs", "2:0,0:1", "--density-clip", "0.01,0.99"],
                       cwd=tmp_path, capture_output=True, timeout=300)
    assert b.returncode == 0, b.stderr.decode()
    ref = E.rows_density2d(rows, 101, 256, pairs=[(2, 0), (0, 1)], clip=(0.01, 0.99))
    check(tmp_path / "c.txt", [("LL", "p0"), ("p0", "p1")], ref, 64)
    assert ref["to"][2] == float(rows[:, 2].max())
    # refused: a bad G and a bad pair by the library, no rows on the host by the driver
    for extra in (["--density2d-n", "7"], ["--density2d-pairs", "1:1"], ["--density2d-pairs", "0:3"]):
        c = subprocess.run(ARGS + ["--density2d", "e.txt"] + extra, cwd=tmp_path, capture_output=True, timeout=300)
        assert c.returncode == 2 and b"--density2d" in c.stderr, extra
    d = subprocess.run(ARGS[:-1] + ["--stream-text", "--density2d", "f.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert d.returncode == 2 and b"--density2d" in d.stderr


def test_driver_derived_density2d(tmp_path):
    import mcpar_amd as M
    A = np.array([[1.0, -1.0], [0.25, 0.75]], np.float32)
    bvec = np.array([0.5, -2.0], np.float32)
    (tmp_path / "lin.txt").write_text("\n".join(" ".join(repr(float(v)) for v in list(A[j]) + [bvec[j]]) for j in range(2)) + "\n")
    a = subprocess.run(ARGS + ["--out", "rows.bin", "--derive-linear", "lin.txt", "--derived-density2d", "dd.txt", "--density2d-n", "12",
                               "--density2d-pairs", "0:1,2:1"], cwd=tmp_path, capture_output=True, timeout=300)
    assert a.returncode == 0, a.stderr.decode()
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, 3)
    st = M.derive_rows(rows, 101, 256, M.derive_linear(A, bvec))
    ref = st.density2d(g=12, pairs=[(0, 1), (2, 1)])
    st.close()
    check(tmp_path / "dd.txt", [("d0", "d1"), ("LL", "d1")], ref, 12)
    # --derived-density2d without a derive function
    b = subprocess.run(ARGS + ["--derived-density2d", "x.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert b.returncode == 2 and b"--derive" in b.stderr
