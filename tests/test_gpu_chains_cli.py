"""mcpar-run --chain-table / --chain-keep / --kept-chains / --kept-summary against the Python binding's table, rule and
selection of the run's own --out rows.  The job plants one frozen chain through a user likelihood: the driver starts chain 0,
and no other, at x[0] = 0 exactly, and the likelihood puts a value there that no proposal reaches."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "mcpar_amd", "drivers")
NP, NC, NSAMP = 4, 256, 101
NAMES = ["p0", "p1", "p2", "p3", "LL"]
FROZEN = """__device__ float mcx_user_loglike(const float *x, int d, const float *par)
{
  if (x[0] == 0.0f) return 1.0e6f;
  float acc = 0.0f;
  for (int k = 0; k < d; ++k) acc = acc + x[k] * x[k];
  return -0.5f * acc;
}
"""
MPIEXEC = "/opt/conda/bin/mpiexec"


def args(tmp_path):
    src = tmp_path / "frozen.hip"
    src.write_text(FROZEN)
    return [os.path.join(DRV, "mcpar-run"), "--func-source", str(src), "--np", str(NP), "--nc", str(NC), "--nsamp", str(NSAMP), "--nburn",
            "100", "--binary"]


def numbers(tokens):
    return np.array([float(t) for t in tokens])


def same_numbers(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def test_driver_chain_files(tmp_path):
    from mcpar_amd import engine as E
    a = subprocess.run(args(tmp_path) + ["--out", "rows.bin", "--chain-table", "t.txt", "--chain-keep", "4,1,50", "--kept-chains", "k.txt",
                                         "--kept-summary", "s.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert a.returncode == 0, a.stderr.decode()
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, NP + 1)
    assert rows.shape[0] == NSAMP * NC
    t = E.rows_chain_table(rows, NSAMP, NC)
    assert t["moves"][0] == 0 and t["longest_stay"][0] == NSAMP and t["ll_max"][0] == 1.0e6 and (t["moves"][1:] > 0).all()
    # the table: 17 significant digits bring the doubles back, 9 the float
    lines = open(tmp_path / "t.txt").read().splitlines()
    assert lines[0].split() == ["chain", "moves", "longest_stay", "ll_max", "ll_max_step", "flags"] + \
        ["%s_%s" % (n, s) for n in NAMES for s in ("mean", "sd", "rho1")]
    assert len(lines) == 1 + NC
    tok = [ln.split() for ln in lines[1:]]
    assert [int(k[0]) for k in tok] == list(range(NC))
    for j, name in ((1, "moves"), (2, "longest_stay"), (4, "ll_max_step"), (5, "flags")):
        assert [int(k[j]) for k in tok] == t[name].tolist(), name
    assert same_numbers(np.array([float(k[3]) for k in tok], np.float32), t["ll_max"])
    body = np.array([numbers(k[6:]) for k in tok]).reshape(NC, NP + 1, 3)
    for j, name in enumerate(("mean", "sd", "rho1")):
        assert same_numbers(body[:, :, j], t[name]), name
    # the verdicts are keep_chains' on the same rows
    reasons, _, kept = E.keep_chains(t, z=4.0, min_moves=1, max_stay=50)
    assert reasons[0] & E.CHAIN_STUCK and 0 not in kept and 1 <= kept.size < NC
    lines = open(tmp_path / "k.txt").read().splitlines()
    assert lines[0].split() == ["chain", "reasons"] and len(lines) == NC + 2
    assert [[int(v) for v in ln.split()] for ln in lines[1:-1]] == [[k, int(r)] for k, r in enumerate(reasons)]
    assert lines[-1] == "kept %d of %d" % (kept.size, NC)
    # the summary of the kept chains is --summary's file for the kept rows
    st = E.select_chains_rows(rows, NSAMP, NC, kept)
    ref = st.summary()
    st.close()
    lines = open(tmp_path / "s.txt").read().splitlines()
    assert lines[0].split() == ["name", "mean", "sd", "q01", "q50", "q99", "rhat", "ess", "mcse"] and len(lines) == NP + 2
    for c, ln in enumerate(lines[1:]):
        k = ln.split()
        assert k[0] == NAMES[c]
        want = [ref["mean"][c], ref["sd"][c], ref["quantiles"][c, 0], ref["quantiles"][c, 1], ref["quantiles"][c, 2], ref["rhat"][c],
                ref["ess"][c], ref["mcse_mean"][c]]
        assert same_numbers(numbers(k[1:]), want), (ln, want)
    assert float(lines[-1].split()[1]) < 0.0  # log L without the frozen chain's 1e6
    # the default rule, and a table alone
    b = subprocess.run(args(tmp_path) + ["--out", "rows.bin", "--kept-chains", "k2.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert b.returncode == 0, b.stderr.decode()
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, NP + 1)
    reasons, _, kept = E.keep_chains(E.rows_chain_table(rows, NSAMP, NC))
    lines = open(tmp_path / "k2.txt").read().splitlines()
    assert [int(ln.split()[1]) for ln in lines[1:-1]] == reasons.tolist() and lines[-1] == "kept %d of %d" % (kept.size, NC)


def test_driver_chain_refusals(tmp_path):
    base = args(tmp_path)
    c = subprocess.run(base + ["--chain-keep", "0", "--kept-chains", "e.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert c.returncode == 2 and b"--chain-keep" in c.stderr and b"z = 0" in c.stderr
    d = subprocess.run(base[:-1] + ["--stream-text", "--chain-table", "f.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert d.returncode == 2 and b"--chain-table, --kept-chains and --kept-summary need the rows on the host of a single rank" in d.stderr
    e = subprocess.run(base + ["--chain-keep", "x"], cwd=tmp_path, capture_output=True, timeout=300)
    assert e.returncode == 2 and b"--chain-keep takes Z" in e.stderr


def test_several_ranks_are_refused(tmp_path):
    """before anything runs: every flag of the four needs the rows on the host of one rank"""
    r = subprocess.run(["make", "-C", DRV, "mpi"], capture_output=True, text=True)
    assert r.returncode == 0, "the MPI build of the drivers: " + r.stderr[-300:]
    for flag in ("--chain-table", "--kept-chains", "--kept-summary"):
        m = subprocess.run([MPIEXEC, "-n", "2", os.path.join(DRV, "mcpar-run-mpi"), "--func", "gauss", "--np", "4", "--nc", "64", "--nsamp",
                            "8", "--nburn", "8", "--quiet", flag, "x.txt"], cwd=tmp_path, capture_output=True, timeout=300)
        assert m.returncode != 0, flag
        assert m.stderr.count(b"--chain-table, --kept-chains and --kept-summary need the rows on the host of a single rank: not with "
                              b"more than one rank") == 1, m.stderr.decode()
        assert not (tmp_path / "x.txt").exists()
