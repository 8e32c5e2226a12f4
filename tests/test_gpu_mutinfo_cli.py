"""mcpar-run --mutual-info against the Python binding on the same rows, after a run and after --read: the file holds the
library's numbers, doubles with 17 significant digits, so the text is compared as text."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "mcpar_amd", "drivers")
NC, T = 64, 12
RUN = [os.path.join(DRV, "mcpar-run"), "--func", "gauss", "--np", "4", "--nc", str(NC), "--nsamp", str(T), "--nburn", "40", "--quiet"]
NAMES = ["p0", "p1", "p2", "p3", "LL"]
COUNTS = ("n_rows", "n_sel", "ndup", "m", "k", "npairs", "nperm", "nused")
FIELDS = ("mi", "r_info", "pearson", "perm_mean", "perm_sd", "p_value")


def text_of(d, names=NAMES):
    lines = [" ".join(COUNTS), " ".join("%d" % d[f] for f in COUNTS), "a b mi r_info pearson perm_mean perm_sd p_value nge nzero flags"]
    return lines + ["%s %s %s %d %d %d" % (names[o["a"]], names[o["b"]], " ".join("%.17g" % o[f] for f in FIELDS), o["nge"], o["nzero"],
                                           o["flags"]) for o in d["pairs"]]


def test_driver_mutual_info(tmp_path):
    from mcpar_amd import engine as E
    a = subprocess.run(RUN + ["--binary", "--out", "rows.bin", "--mutual-info", "mi.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert a.returncode == 0, a.stderr.decode()
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, 5)
    assert rows.shape[0] == T * NC
    want = E.rows_mutual_info(rows, T, NC)
    assert (want["n_sel"], want["npairs"], want["k"], want["nperm"]) == (T * NC, 6, 3, 0) and want["m"] + want["ndup"] == T * NC
    assert open(tmp_path / "mi.txt").read().splitlines() == text_of(want)
    # a short run repeats its rows: the warning says so exactly when more than a tenth of the rows taken were dropped
    assert (b"repeat an earlier one" in a.stderr) == (want["ndup"] * 10 > want["n_sel"])
    # every option given, text out; then the same analysis of the text read back
    opts = ["--mi-n", "300", "--mi-k", "2", "--mi-perm", "9", "--mi-seed", "4000000000", "--mi-pairs", "0:1,4:2,3:0", "--mi-with-ll", "--mi-raw"]
    kw = dict(n=300, k=2, nperm=9, seed=4000000000, pairs=[(0, 1), (4, 2), (3, 0)], with_ll=True, raw=True)
    b = subprocess.run(RUN + ["--out", "dump.txt", "--mutual-info", "named.txt"] + opts, cwd=tmp_path, capture_output=True, timeout=300)
    assert b.returncode == 0, b.stderr.decode()
    want = E.rows_mutual_info(rows, T, NC, **kw)
    assert (want["n_sel"], want["npairs"], want["nused"]) == (300, 3, 5)
    assert open(tmp_path / "named.txt").read().splitlines() == text_of(want)
    c = subprocess.run([RUN[0], "--read", "dump.txt", "--nc", str(NC), "--quiet", "--mutual-info", "read.txt"] + opts, cwd=tmp_path,
                       capture_output=True, timeout=300)
    assert c.returncode == 0, c.stderr.decode()
    parsed, rep = E.parse_text(open(tmp_path / "dump.txt", "rb").read(), NC)
    assert parsed.shape == rows.shape
    assert open(tmp_path / "read.txt").read().splitlines() == text_of(E.rows_mutual_info(parsed, T, NC, **kw))
    # refused by the driver: options without a file, no rows on the host; by the library: its own message
    d = subprocess.run(RUN + ["--mi-perm", "5"], cwd=tmp_path, capture_output=True, timeout=300)
    assert d.returncode == 2 and b"--mutual-info" in d.stderr
    d = subprocess.run(RUN + ["--stream-text", "--mutual-info", "f.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert d.returncode == 2 and b"--mutual-info" in d.stderr
    d = subprocess.run(RUN + ["--mutual-info", "g.txt", "--mi-pairs", "0:1,2"], cwd=tmp_path, capture_output=True, timeout=300)
    assert d.returncode == 2 and b"--mi-pairs takes" in d.stderr
    d = subprocess.run(RUN + ["--mutual-info", "g.txt", "--mi-k", "9"], cwd=tmp_path, capture_output=True, timeout=300)
    assert d.returncode == 2 and b"--mutual-info: " in d.stderr and b"spec.k = 9" in d.stderr


def test_driver_warns_of_ties(tmp_path):
    """an indicator column read back from text: the pair has ties and the driver says so"""
    from mcpar_amd import engine as E
    rng = np.random.default_rng(5)
    rows = np.stack([rng.integers(0, 2, 256).astype(np.float32), rng.integers(0, 2, 256).astype(np.float32),
                     -rng.random(256).astype(np.float32)], axis=1)
    with open(tmp_path / "ind.txt", "w") as f:
        for r in rows:
            f.write("%.9g %.9g %.9g\n" % tuple(r))
    c = subprocess.run([RUN[0], "--read", "ind.txt", "--nc", "4", "--quiet", "--mutual-info", "ind_mi.txt", "--mi-n", "-1", "--mi-with-ll"],
                       cwd=tmp_path, capture_output=True, timeout=300)
    assert c.returncode == 0, c.stderr.decode()
    want = E.rows_mutual_info(rows, 64, 4, n=-1, with_ll=True)
    assert want["ndup"] == 0 and want["pairs"][0]["flags"] == E.MUTINFO_PAIR_TIES and want["pairs"][0]["nzero"] > 0
    assert open(tmp_path / "ind_mi.txt").read().splitlines() == text_of(want, ("p0", "p1", "LL"))
    assert b"pairs have points whose k nearest neighbours are at distance 0" in c.stderr and b"repeat an earlier one" not in c.stderr
