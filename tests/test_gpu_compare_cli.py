"""mcpar-run --compare / --compare-to / --compare-halves against the Python binding on the same rows: the files hold the
library's numbers, doubles with 17 significant digits, so the text is compared as text.

A run against its own --out text: the text holds six significant digits, so B is the run's rows rounded to six digits and the
distances are those of that rounding, not zero -- the file is compare_rows' of the run's rows against the parsed text, and w1 is at
most the largest move of a value, 5e-6 of the column's largest magnitude.  The dump against itself (--read) gives all-zero
distances and ks_p = 1."""
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
HEADER = ("name ks ks_plus_num ks_plus_x ks_minus_num ks_minus_x w1 mean_a sd_a ess_a mean_b sd_b ess_b z_mean ks_neff ks_p na nb "
          "flags")


def text_of(d):
    lines = [HEADER]
    for c, name in enumerate(NAMES):
        v = [name, "%.17g" % d["ks"][c], "%d" % d["ks_plus_num"][c], "%.17g" % d["ks_plus_x"][c], "%d" % d["ks_minus_num"][c],
             "%.17g" % d["ks_minus_x"][c]]
        v += ["%.17g" % d[f][c] for f in ("w1", "mean_a", "sd_a", "ess_a", "mean_b", "sd_b", "ess_b", "z_mean", "ks_neff", "ks_p")]
        v += ["%d" % d["na"][c], "%d" % d["nb"][c], "%d" % d["flags"][c]]
        lines.append(" ".join(v))
    return lines


def test_driver_compare(tmp_path):
    from mcpar_amd import engine as E
    a = subprocess.run(ARGS + ["--binary", "--out", "rows.bin", "--compare-halves", "h.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert a.returncode == 0, a.stderr.decode()
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, 5)
    assert rows.shape[0] == T * NC
    h = T // 2
    want = E.compare_rows(rows[:h * NC], h, NC, rows[h * NC:], T - h, NC)
    assert open(tmp_path / "h.txt").read().splitlines() == text_of(want)
    # the run against its own text
    b = subprocess.run(ARGS + ["--out", "dump.txt", "--compare", "c.txt", "--compare-to", "dump.txt", "--compare-iid"], cwd=tmp_path,
                       capture_output=True, timeout=300)
    assert b.returncode == 0, b.stderr.decode()
    parsed, rep = E.parse_text(open(tmp_path / "dump.txt", "rb").read(), NC)
    assert parsed.shape == rows.shape and np.allclose(parsed, rows, rtol=1e-5, atol=0)
    want = E.compare_rows(rows, T, NC, parsed, T, NC, iid=True)
    assert open(tmp_path / "c.txt").read().splitlines() == text_of(want)
    assert (want["w1"] <= 5e-6 * np.abs(rows).max(axis=0)).all() and (want["ess_a"] == T * NC).all()
    # the dump against itself
    c = subprocess.run([ARGS[0], "--read", "dump.txt", "--nc", str(NC), "--quiet", "--compare", "z.txt", "--compare-to", "dump.txt"],
                       cwd=tmp_path, capture_output=True, timeout=300)
    assert c.returncode == 0, c.stderr.decode()
    lines = open(tmp_path / "z.txt").read().splitlines()
    assert lines[0] == HEADER and [ln.split()[0] for ln in lines[1:]] == NAMES
    for ln in lines[1:]:
        t = ln.split()
        assert (float(t[1]), int(t[2]), int(t[4]), float(t[6]), float(t[13]), float(t[15])) == (0.0, 0, 0, 0.0, 0.0, 1.0), ln
        assert t[16:] == [str(T * NC), str(T * NC), "0"]
    # refused by the driver: one of the pair alone, no rows on the host; by the library: another number of columns
    d = subprocess.run(ARGS + ["--compare", "e.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert d.returncode == 2 and b"--compare-to" in d.stderr
    e = subprocess.run(ARGS + ["--stream-text", "--compare-halves", "f.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert e.returncode == 2 and b"--compare" in e.stderr
    (tmp_path / "three.txt").write_text("1 2 3\n" * NC)
    f = subprocess.run(ARGS + ["--compare", "g.txt", "--compare-to", "three.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert f.returncode == 2 and b"--compare-to three.txt" in f.stderr
