"""mcpar-run --intervals against the Python binding on the same rows, after a run and after --read.  The file holds the library's
numbers, doubles with 17 significant digits and floats with 9, so the text is compared as text.  The sample text of a run keeps
six digits, so the file that is read back here is the run's binary rows written with nine: the same floats, and so the same
file of intervals."""
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


def text_of(d, masses, probs):
    head = ["name", "mean", "sd", "mcse_sd", "ess_sd"] + [w % ("%g" % m) for m in masses for w in ("hdi%s_lo", "hdi%s_hi")]
    head += [w % ("%g" % p) for p in probs for w in ("q%s", "mcse_q%s", "ess_q%s")] + ["flags"]
    lines = [" ".join(head)]
    for c, name in enumerate(NAMES):
        v = [name] + ["%.17g" % d[f][c] for f in ("mean", "sd", "mcse_sd", "ess_sd")]
        for j in range(len(masses)):
            v += ["%.9g" % d["hdi"]["lo"][c, j], "%.9g" % d["hdi"]["hi"][c, j]]
        for k in range(len(probs)):
            v += ["%.17g" % d["quantiles"][f][c, k] for f in ("q", "mcse_q", "ess_q")]
        lines.append(" ".join(v + ["%d" % d["flags"][c]]))
    return lines


def test_driver_intervals(tmp_path):
    from mcpar_amd import engine as E
    a = subprocess.run(ARGS + ["--binary", "--out", "rows.bin", "--intervals", "a.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert a.returncode == 0, a.stderr.decode()
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, 5)
    assert rows.shape[0] == T * NC
    want = text_of(E.rows_intervals(rows, T, NC, (0.9,), (0.05, 0.5, 0.95)), (0.9,), (0.05, 0.5, 0.95))
    assert open(tmp_path / "a.txt").read().splitlines() == want
    assert want[0] == "name mean sd mcse_sd ess_sd hdi0.9_lo hdi0.9_hi q0.05 mcse_q0.05 ess_q0.05 q0.5 mcse_q0.5 ess_q0.5 q0.95 mcse_q0.95 ess_q0.95 flags"
    # the same rows as a file that is read, not run
    with open(tmp_path / "full.txt", "w") as f:
        for r in rows:
            f.write("  ".join("%.9g" % v for v in r) + "  \n")
    back, _ = E.parse_text(open(tmp_path / "full.txt", "rb").read(), NC)
    assert back.tobytes() == rows.tobytes()
    b = subprocess.run([ARGS[0], "--read", "full.txt", "--nc", str(NC), "--quiet", "--intervals", "b.txt"], cwd=tmp_path,
                       capture_output=True, timeout=300)
    assert b.returncode == 0, b.stderr.decode()
    assert open(tmp_path / "b.txt").read() == open(tmp_path / "a.txt").read()
    # other masses and probabilities, and none
    masses, probs = (0.5, 0.94), (0.25, 0.75)
    c = subprocess.run([ARGS[0], "--read", "full.txt", "--nc", str(NC), "--quiet", "--intervals", "c.txt", "--hdi", "0.5,0.94",
                        "--interval-probs", "0.25,0.75"], cwd=tmp_path, capture_output=True, timeout=300)
    assert c.returncode == 0, c.stderr.decode()
    assert open(tmp_path / "c.txt").read().splitlines() == text_of(E.rows_intervals(rows, T, NC, masses, probs), masses, probs)
    # refused by the library, and by the driver
    for extra, word in ((["--intervals", "e.txt", "--hdi", "1.5"], b"mass[0]"), (["--intervals", "e.txt", "--interval-probs", "0.5,-1"], b"probs[1]"),
                        (["--intervals", "e.txt", "--stream-text"], b"--intervals")):
        e = subprocess.run(ARGS + extra, cwd=tmp_path, capture_output=True, timeout=300)
        assert e.returncode == 2 and word in e.stderr, (extra, e.stderr)
