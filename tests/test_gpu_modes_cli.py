"""mcpar-run --modes and the --mode-* files against the Python binding on the same rows, after a small run on the Gaussian
mixture (--func mix) and after --read.  The files hold the library's numbers, doubles with 17 significant digits, so the text is
compared as text.  The sample text of a run keeps six digits, so the file that is read back here is the run's binary rows
written with nine: the same floats, and so the same files."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "mcpar_amd", "drivers")
NC, T, NP, K = 64, 12, 4, 3
ARGS = [os.path.join(DRV, "mcpar-run"), "--func", "mix", "--ncomp", "3", "--np", str(NP), "--nc", str(NC), "--nsamp", str(T), "--nburn", "40",
        "--quiet"]
MODES = ["--modes-k", str(K), "--modes-seed", "9"]
FILES = ["--modes", "modes.txt", "--mode-weights", "weights.txt", "--mode-chains", "chains.txt", "--mode-occupancy", "occ.txt"]


def modes_text(m):
    r, t = m.result, m.table
    lines = ["%s %d" % (f, r[f]) for f in ("k", "iters", "flags", "n", "n_nonfinite", "n_changed")] + ["inertia %.17g" % r["inertia"]]
    lines.append("mode n weight inertia ll_mean ll_max ll_max_row flags")
    for k in range(m.k):
        lines.append("%d %d %.17g %.17g %.17g %.9g %d %d" % (k, t["n"][k], t["weight"][k], t["inertia"][k], t["ll_mean"][k], t["ll_max"][k],
                                                            t["ll_max_row"][k], t["flags"][k]))
    mat = lambda a: [" ".join("%.17g" % v for v in row) for row in a]  # noqa: E731
    return lines + ["scale"] + mat([m.scale]) + ["centres"] + mat(m.centres) + ["means"] + mat(t["mean"]) + ["sds"] + mat(t["sd"])


def weights_text(m):
    w = m.weights()
    return ["mode weight sd mcse_mean rhat ess"] + ["%d %s" % (k, " ".join("%.17g" % w[f][k] for f in ("mean", "sd", "mcse_mean", "rhat", "ess")))
                                                   for k in range(m.k)]


def chains_text(m):
    c = m.chain_table()
    lines = ["chain hops dominant dominant_steps first_label last_label visits"]
    for i in range(m.nc):
        lines.append(" ".join(str(int(v)) for v in [i, c["hops"][i], c["dominant"][i], c["dominant_steps"][i], c["first_label"][i],
                                                    c["last_label"][i]] + list(c["visits"][i])))
    return lines + ["trans"] + [" ".join(str(int(v)) for v in row) for row in c["trans"]], \
        [" ".join(str(int(v)) for v in [t] + list(row)) for t, row in enumerate(c["occupancy"])]


def run(args, cwd):
    r = subprocess.run(args, cwd=cwd, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()


def read(path):
    return open(path).read().splitlines()


def test_driver_modes(tmp_path):
    from mcpar_amd import engine as E
    run(ARGS + ["--binary", "--out", "rows.bin"] + MODES + FILES, tmp_path)
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, NP + 1)
    assert rows.shape[0] == T * NC
    with E.rows_modes(rows, T, NC, K, seed=9) as m:
        assert read(tmp_path / "modes.txt") == modes_text(m)
        assert read(tmp_path / "weights.txt") == weights_text(m)
        ch, occ = chains_text(m)
        assert read(tmp_path / "chains.txt") == ch and read(tmp_path / "occ.txt") == occ
        n = m.table["n"].copy()
    # the files parse, and the weights sum to 1
    w = np.loadtxt(tmp_path / "weights.txt", skiprows=1)
    assert w.shape == (K, 6) and abs(w[:, 1].sum() - 1) < 1e-12 and (w[:, 1] > 0).all()
    occ = np.loadtxt(tmp_path / "occ.txt", dtype=np.int64)
    assert occ.shape == (T, K + 1) and (occ[:, 1:].sum(1) == NC).all() and np.array_equal(occ[:, 1:].sum(0), n)
    # the same rows as a file that is read, not run: the same files
    with open(tmp_path / "full.txt", "w") as f:
        for r in rows:
            f.write("  ".join("%.9g" % v for v in r) + "  \n")
    back, _ = E.parse_text(open(tmp_path / "full.txt", "rb").read(), NC)
    assert back.tobytes() == rows.tobytes()
    rd = [ARGS[0], "--read", "full.txt", "--nc", str(NC), "--quiet"]
    run(rd + MODES + ["--modes", "b.txt", "--mode-weights", "b_w.txt", "--mode-chains", "b_c.txt", "--mode-occupancy", "b_o.txt"], tmp_path)
    for a, b in (("modes.txt", "b.txt"), ("weights.txt", "b_w.txt"), ("chains.txt", "b_c.txt"), ("occ.txt", "b_o.txt")):
        assert open(tmp_path / a).read() == open(tmp_path / b).read(), a
    # the rows of a mode and their summary; the summary of the rows read back as one chain is the same file when the text
    # holds the floats: six digits do not, so the rows go through nine again
    big = int(np.argmax(n))
    run(rd + MODES + ["--mode-rows", "%d,mode_rows.txt" % big, "--mode-summary", "%d,mode_summary.txt" % big], tmp_path)
    with E.rows_modes(rows, T, NC, K, seed=9) as m:
        mine = rows[m.labels() == big]
    assert open(tmp_path / "mode_rows.txt", "rb").read() == E.format_rows(mine) and len(mine) == n[big] >= 4
    with open(tmp_path / "mode_full.txt", "w") as f:
        for r in mine:
            f.write("  ".join("%.9g" % v for v in r) + "  \n")
    run([ARGS[0], "--read", "mode_full.txt", "--nc", "1", "--quiet", "--summary", "mode_summary_again.txt"], tmp_path)
    assert open(tmp_path / "mode_summary.txt").read() == open(tmp_path / "mode_summary_again.txt").read()
    # --summary of the six-digit --mode-rows file itself: the same table within what six digits keep.  A value moves by at most
    # 5e-6 of itself; a mean and an interpolated quantile by no more than the largest move, an sd by sqrt(N / (N - 1)) < 2 times it
    run([ARGS[0], "--read", "mode_rows.txt", "--nc", "1", "--quiet", "--summary", "mode_summary_text.txt"], tmp_path)
    a, b = (np.loadtxt(tmp_path / f, skiprows=1, usecols=(1, 2, 3, 4)) for f in ("mode_summary.txt", "mode_summary_text.txt"))
    assert a.shape == b.shape == (NP + 1, 4) and np.allclose(a, b, rtol=0, atol=1e-5 * np.abs(mine).max())
    # given centres, raw columns, one pass
    np.savetxt(tmp_path / "centres.txt", np.array([[0.0] * NP, [2.5] * NP, [5.0] * NP]))
    run(rd + ["--modes-k", "3", "--modes-centres", "centres.txt", "--modes-raw", "--modes-iter", "1", "--modes", "c.txt"], tmp_path)
    with E.rows_modes(rows, T, NC, 3, centres=[[0.0] * NP, [2.5] * NP, [5.0] * NP], scale=False, max_iter=1) as m:
        assert read(tmp_path / "c.txt") == modes_text(m) and m.result["flags"] & E.MODES_NOT_CONVERGED
    # refused by the library, and by the driver
    for extra, word in ((["--modes", "e.txt", "--modes-k", "33"], b"1 to 32 modes"), (["--modes", "e.txt"], b"--modes-k"),
                        (["--mode-rows", "e.txt", "--modes-k", "2"], b"K,FILE"), (["--mode-rows", "7,e.txt", "--modes-k", "2"], b"not a mode"),
                        (["--modes", "e.txt", "--modes-k", "2", "--stream-text"], b"--modes")):
        e = subprocess.run(ARGS + extra, cwd=tmp_path, capture_output=True, timeout=300)
        assert e.returncode == 2 and word in e.stderr, (extra, e.stderr)
