"""mcpar-run --evidence against the Python binding on the same rows, after a small run on the Gaussian mixture (--func mix) and
after --read with the likelihood flags.  The file holds the library's numbers, doubles with 17 significant digits, so the text is
compared as text.  The sample text of a run keeps six digits, so the file that is read back here is the run's binary rows
written with nine: the same floats, and so the same file."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "mcpar_amd", "drivers")
NC, T, NP, NCOMP = 64, 32, 4, 3
FUNC = ["--func", "mix", "--ncomp", str(NCOMP)]
ARGS = [os.path.join(DRV, "mcpar-run")] + FUNC + ["--np", str(NP), "--nc", str(NC), "--nsamp", str(T), "--nburn", "40", "--quiet"]
FIELDS = ("n1", "n2", "k", "fit_steps", "neff", "lstar", "log_z", "se", "re2_draws", "re2_rows", "ess_f2", "log_z_is", "log_z_ris",
          "ndraw_zero", "iters", "flags")


def evidence_text(res):
    return ["%s %s" % (f, "%.17g" % res[f] if isinstance(res[f], float) else "%d" % res[f]) for f in FIELDS]


def mixture():
    """the driver's --func mix: means 5 k / (K - 1) in every coordinate, weights (5, 1, ..., 1)"""
    import mcpar_amd as M
    means = np.repeat(5.0 * np.arange(NCOMP) / (NCOMP - 1), NP)
    return M.make_vlfunc(M.VL_GAUSSMIX, NP, np.concatenate([means, [5.0] + [1.0] * (NCOMP - 1)]).astype(np.float32), NCOMP)


def run(args, cwd):
    r = subprocess.run(args, cwd=cwd, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()


def read(path):
    return open(path).read().splitlines()


def test_driver_evidence(tmp_path):
    from mcpar_amd import engine as E
    run(ARGS + ["--binary", "--out", "rows.bin", "--evidence", "ev.txt"], tmp_path)
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, NP + 1)
    assert rows.shape[0] == T * NC
    vl, _keep = mixture()
    res = E.rows_evidence(rows, T, NC, vl, fit_steps=T // 2)
    assert read(tmp_path / "ev.txt") == evidence_text(res)
    assert res["k"] == 1 and res["n1"] == res["n2"] == (T - T // 2) * NC and np.isfinite(res["log_z"])
    # the same rows as a file that is read, not run, with the likelihood flags: the same file
    with open(tmp_path / "full.txt", "w") as f:
        for r in rows:
            f.write("  ".join("%.9g" % v for v in r) + "  \n")
    rd = [ARGS[0], "--read", "full.txt", "--nc", str(NC), "--quiet"] + FUNC
    run(rd + ["--evidence", "b.txt"], tmp_path)
    assert open(tmp_path / "ev.txt").read() == open(tmp_path / "b.txt").read()
    # every option: the modes of the fitting steps as the proposal
    fit, K, scale = 12, 2, 1.25
    run(rd + ["--evidence", "c.txt", "--evidence-draws", "777", "--evidence-seed", "5", "--evidence-fit-steps", str(fit),
              "--evidence-modes", str(K), "--evidence-scale", str(scale)], tmp_path)
    with E.rows_modes(rows[:fit * NC], fit, NC, K, seed=0) as m:
        p = E.proposal_from_modes(m, scale=scale)
    got = E.rows_evidence(rows, T, NC, vl, p, ndraw=777, seed=5, fit_steps=fit)
    assert read(tmp_path / "c.txt") == evidence_text(got) and got["k"] == K and got["n2"] == 777 and got["fit_steps"] == fit
    # refused by the library, and by the driver
    for extra, word in ((["--evidence", "e.txt", "--evidence-fit-steps", str(T)], b"fit_steps"),
                        (["--evidence", "e.txt", "--evidence-modes", "9"], b"1 to 8 modes"),
                        (["--evidence", "e.txt", "--evidence-scale", "0"], b"scale"),
                        (["--evidence-draws", "5"], b"belong to --evidence"),
                        (["--evidence", "e.txt", "--stream-text"], b"--evidence")):
        e = subprocess.run(ARGS + extra, cwd=tmp_path, capture_output=True, timeout=300)
        assert e.returncode == 2 and word in e.stderr, (extra, e.stderr)
    e = subprocess.run([ARGS[0], "--read", "full.txt", "--nc", str(NC), "--quiet"] + FUNC, cwd=tmp_path, capture_output=True, timeout=300)
    assert e.returncode == 2 and b"not with --func" in e.stderr   # without --evidence the likelihood flags still start a run
