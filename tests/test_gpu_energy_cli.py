"""mcpar-run --energy / --compare-to / --energy-halves against the Python binding on the same rows: the file holds the
library's numbers, doubles with 17 significant digits, so the text is compared as text."""
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
FIELDS = ("e", "h", "mean_ab", "mean_aa", "mean_bb", "p_value")
COUNTS = ("nge", "n_a", "n_b", "nperm", "nused", "na_rows", "nb_rows")


def text_of(d):
    lines = [" ".join(FIELDS + COUNTS), " ".join(["%.17g" % d[f] for f in FIELDS] + ["%d" % d[f] for f in COUNTS]), "name scale flags"]
    return lines + ["%s %.17g %d" % (name, d["scale"][c], d["flags"][c]) for c, name in enumerate(NAMES)]


def test_driver_energy(tmp_path):
    from mcpar_amd import engine as E
    a = subprocess.run(ARGS + ["--binary", "--out", "rows.bin", "--energy-halves", "h.txt", "--energy-perm", "49"], cwd=tmp_path,
                       capture_output=True, timeout=300)
    assert a.returncode == 0, a.stderr.decode()
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, 5)
    assert rows.shape[0] == T * NC
    h = T // 2
    want = E.energy_rows(rows[:h * NC], h, NC, rows[h * NC:], T - h, NC, nperm=49)
    assert (want["n_a"], want["n_b"], want["nused"]) == (h * NC, (T - h) * NC, 4)
    assert open(tmp_path / "h.txt").read().splitlines() == text_of(want)
    # the run against its own text, every option given
    b = subprocess.run(ARGS + ["--out", "dump.txt", "--energy", "c.txt", "--compare-to", "dump.txt", "--energy-n", "100,-1", "--energy-perm", "33",
                               "--energy-seed", "4000000000", "--energy-with-ll", "--energy-raw"], cwd=tmp_path, capture_output=True, timeout=300)
    assert b.returncode == 0, b.stderr.decode()
    parsed, rep = E.parse_text(open(tmp_path / "dump.txt", "rb").read(), NC)
    assert parsed.shape == rows.shape
    want = E.energy_rows(rows, T, NC, parsed, T, NC, n_a=100, n_b=-1, nperm=33, seed=4000000000, with_ll=True, raw=True)
    assert (want["n_a"], want["n_b"], want["nused"]) == (100, T * NC, 5)
    assert open(tmp_path / "c.txt").read().splitlines() == text_of(want)
    # refused by the driver: --energy without --compare-to, options without a file, no rows on the host; by the library: sizes
    d = subprocess.run(ARGS + ["--energy", "e.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert d.returncode == 2 and b"--compare-to" in d.stderr
    d = subprocess.run(ARGS + ["--energy-perm", "5"], cwd=tmp_path, capture_output=True, timeout=300)
    assert d.returncode == 2 and b"--energy-halves" in d.stderr
    e = subprocess.run(ARGS + ["--stream-text", "--energy-halves", "f.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert e.returncode == 2 and b"--energy" in e.stderr
    f = subprocess.run(ARGS + ["--energy-halves", "g.txt", "--energy-n", "1"], cwd=tmp_path, capture_output=True, timeout=300)
    assert f.returncode == 2 and b"--energy-halves: " in f.stderr and b"1 rows of side a" in f.stderr
