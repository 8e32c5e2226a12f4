"""mcpar-run --mess / --ccf against the Python binding on the same rows, after a run and after --read.  The files hold the
library's numbers, doubles with 17 significant digits, so the text is compared as text.  The sample text of a run keeps six digits,
so the file that is read back here is the run's binary rows written with nine: the same floats, and so the same files."""
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
RESULT = ("N", "p", "s", "k_used", "lags_used", "lags_computed", "flags")


def mess_text(d):
    lines = ["name mean ess mcse flags"]
    for c, name in enumerate(NAMES):
        lines.append(" ".join([name] + ["%.17g" % d[f][c] for f in ("mean", "ess", "mcse")] + ["%d" % d["col_flags"][c]]))
    lines += ["%s %d" % (f, d[f]) for f in RESULT] + ["%s %.17g" % (f, d[f]) for f in ("mess", "logdet_lambda", "logdet_sigma")]
    return lines + ["sigma"] + [" ".join("%.17g" % v for v in row) for row in d["sigma"]]


def ccf_text(d):
    lines = ["lag i j ccf gamma"]
    for t in range(d["gamma"].shape[0]):
        for i, a in enumerate(NAMES):
            for j, b in enumerate(NAMES):
                lines.append("%d %s %s %.17g %.17g" % (t, a, b, d["ccf"][t, i, j], d["gamma"][t, i, j]))
    return lines


def test_driver_mess_and_ccf(tmp_path):
    from mcpar_amd import engine as E
    a = subprocess.run(ARGS + ["--binary", "--out", "rows.bin", "--mess", "a.txt", "--ccf", "a_ccf.txt", "--ccf-lags", "3"], cwd=tmp_path,
                       capture_output=True, timeout=300)
    assert a.returncode == 0, a.stderr.decode()
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, 5)
    assert rows.shape[0] == T * NC
    want = E.rows_lagcov(rows, T, NC, nlags=3)
    assert open(tmp_path / "a.txt").read().splitlines() == mess_text(want)
    assert open(tmp_path / "a_ccf.txt").read().splitlines() == ccf_text(want)
    assert want["p"] == 4 and want["k_used"] >= 0 and np.isnan(want["sigma"][4]).all()
    # the same rows as a file that is read, not run
    with open(tmp_path / "full.txt", "w") as f:
        for r in rows:
            f.write("  ".join("%.9g" % v for v in r) + "  \n")
    back, _ = E.parse_text(open(tmp_path / "full.txt", "rb").read(), NC)
    assert back.tobytes() == rows.tobytes()
    b = subprocess.run([ARGS[0], "--read", "full.txt", "--nc", str(NC), "--quiet", "--mess", "b.txt", "--ccf", "b_ccf.txt", "--ccf-lags", "3"],
                       cwd=tmp_path, capture_output=True, timeout=300)
    assert b.returncode == 0, b.stderr.decode()
    assert open(tmp_path / "b.txt").read() == open(tmp_path / "a.txt").read()
    assert open(tmp_path / "b_ccf.txt").read() == open(tmp_path / "a_ccf.txt").read()
    # a shorter walk with log L, the mess alone
    c = subprocess.run([ARGS[0], "--read", "full.txt", "--nc", str(NC), "--quiet", "--mess", "c.txt", "--mess-max-lag", "3", "--mess-with-ll"],
                       cwd=tmp_path, capture_output=True, timeout=300)
    assert c.returncode == 0, c.stderr.decode()
    short = E.rows_lagcov(rows, T, NC, max_lag=3, with_ll=True)
    assert open(tmp_path / "c.txt").read().splitlines() == mess_text(short) and short["p"] == 5 and short["lags_computed"] == 4
    assert not os.path.exists(tmp_path / "c_ccf.txt")
    # more lags in the ccf file than the walk may see
    d = subprocess.run([ARGS[0], "--read", "full.txt", "--nc", str(NC), "--quiet", "--mess", "d.txt", "--mess-max-lag", "3", "--ccf", "d_ccf.txt",
                        "--ccf-lags", "10"], cwd=tmp_path, capture_output=True, timeout=300)
    assert d.returncode == 0, d.stderr.decode()
    long = E.rows_lagcov(rows, T, NC, max_lag=3, nlags=10)
    assert open(tmp_path / "d.txt").read().splitlines() == mess_text(long) and long["k_used"] <= 1 and long["lags_computed"] == 10
    assert open(tmp_path / "d_ccf.txt").read().splitlines() == ccf_text(long)
    assert long["gamma"].tobytes() == E.rows_lagcov(rows, T, NC, nlags=T)["gamma"][:10].tobytes()
    # refused by the library, and by the driver
    for extra, word in ((["--ccf", "e.txt", "--ccf-lags", "13"], b"nlags_out"), (["--ccf", "e.txt"], b"--ccf-lags"),
                        (["--mess", "e.txt", "--stream-text"], b"--mess")):
        e = subprocess.run(ARGS + extra, cwd=tmp_path, capture_output=True, timeout=300)
        assert e.returncode == 2 and word in e.stderr, (extra, e.stderr)
