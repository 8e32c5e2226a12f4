"""mcpar-run --profile / --profile-intervals / --profile-path / --profile2d against the Python binding on the same rows, after a
small run and after --read.  The files hold the library's numbers, doubles with 17 and floats with 9 significant digits, so the
text is compared as text.  The sample text of a run keeps six digits, so the file that is read back here is the run's binary
rows written with nine: the same floats, and so the same files."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "mcpar_amd", "drivers")
NC, T, NP = 64, 32, 4
ARGS = [os.path.join(DRV, "mcpar-run"), "--func", "mix", "--ncomp", "3", "--np", str(NP), "--nc", str(NC), "--nsamp", str(T), "--nburn", "40", "--quiet"]
N1, G2, LEVELS, CLIP, PATH_COL = 12, 9, (0.5, 0.9), (0.02, 0.98), 2
OPTS = ["--profile-n", str(N1), "--profile-levels", ",".join(str(p) for p in LEVELS), "--profile-clip", "%g,%g" % CLIP]
FILES = ["--profile", "pl.txt", "--profile-intervals", "iv.txt", "--profile-path", "%d,path.txt" % PATH_COL,
         "--profile2d", "p2.txt", "--profile2d-n", str(G2), "--profile2d-pairs", "0:1,3:0"]


def name(c):
    return "p%d" % c if c < NP else "LL"


def run(args, cwd):
    r = subprocess.run(args, cwd=cwd, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()


def read(path):
    return open(path).read().splitlines()


def curve_text(o):
    out = ["column bin cnt row xat lmax pl plh"]
    for c in range(NP):
        for j in range(N1):
            out.append("%s %d %d %d %.9g %.9g %.17g %.17g" % (name(c), j, o["cnt"][c, j], o["row"][c, j], o["xat"][c, j], o["lmax"][c, j],
                                                             o["pl"][c, j], o["plh"][c, j]))
    return out


def interval_text(o):
    out = ["column p drop lo hi lo_hull hi_hull nseg flags"]
    for c in range(NP):
        for v in o["intervals"][c]:
            out.append("%s %.17g %.17g %.17g %.17g %.17g %.17g %d %d" % (name(c), v["p"], v["drop"], v["lo"], v["hi"], v["lo_hull"],
                                                                        v["hi_hull"], v["nseg"], v["flags"]))
    return out


def path_text(o):
    out = ["bin " + " ".join(name(c) for c in range(NP + 1))]
    for j in range(N1):
        if o["row"][PATH_COL, j] >= 0:
            out.append("%d " % j + " ".join("%.9g" % v for v in o["path"][PATH_COL, j]))
    return out


def pair_text(o, g=G2):
    out = ["a b ia ib cnt row xat_a xat_b lmax z"]
    for p, (a, b) in enumerate(o["pairs"]):
        for j in range(g):
            for k in range(g):
                out.append("%s %s %d %d %d %d %.9g %.9g %.9g %.17g" % (name(a), name(b), j, k, o["cnt"][p, j, k], o["row"][p, j, k],
                                                                      o["xat_a"][p, j, k], o["xat_b"][p, j, k], o["lmax"][p, j, k], o["z"][p, j, k]))
    return out


def same_lines(got, want):
    """the C library prints nan, inf and -inf as Python does, but for the sign of a NaN"""
    assert [l.replace("-nan", "nan") for l in got] == want


def test_driver_profiles(tmp_path):
    from mcpar_amd import engine as E
    run(ARGS + ["--binary", "--out", "rows.bin"] + OPTS + FILES, tmp_path)
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, NP + 1)
    assert rows.shape[0] == T * NC
    o = E.rows_profile(rows, T, NC, n=N1, levels=LEVELS, clip=CLIP, path=True)
    same_lines(read(tmp_path / "pl.txt"), curve_text(o))
    same_lines(read(tmp_path / "iv.txt"), interval_text(o))
    same_lines(read(tmp_path / "path.txt"), path_text(o))
    o2 = E.rows_profile2d(rows, T, NC, g=G2, pairs=[(0, 1), (3, 0)], levels=LEVELS, clip=CLIP)
    same_lines(read(tmp_path / "p2.txt"), pair_text(o2))
    assert len(read(tmp_path / "pl.txt")) == 1 + NP * N1 and len(read(tmp_path / "p2.txt")) == 1 + 2 * G2 * G2
    # the same rows as a file that is read, not run: the same files
    with open(tmp_path / "full.txt", "w") as f:
        for r in rows:
            f.write("  ".join("%.9g" % v for v in r) + "  \n")
    sub = tmp_path / "read"
    sub.mkdir()
    run([ARGS[0], "--read", "../full.txt", "--nc", str(NC), "--quiet"] + OPTS + FILES, sub)
    for fn in ("pl.txt", "iv.txt", "path.txt", "p2.txt"):
        assert open(tmp_path / fn).read() == open(sub / fn).read(), fn
    # the defaults: 64 bins, the levels 0.6827 and 0.9545, every pair at 32 nodes
    run([ARGS[0], "--read", "../full.txt", "--nc", str(NC), "--quiet", "--profile-intervals", "iv0.txt", "--profile2d", "p20.txt"], sub)
    same_lines(read(sub / "iv0.txt"), interval_text(E.rows_profile(rows, T, NC)))
    same_lines(read(sub / "p20.txt"), pair_text(E.rows_profile2d(rows, T, NC), 32))
    # refused by the library, and by the driver
    for extra, word in ((["--profile", "e.txt", "--profile-n", "1"], b"bins per column"),
                        (["--profile", "e.txt", "--profile-levels", "0.5,1.5"], b"levels[1]"),
                        (["--profile2d", "e.txt", "--profile2d-pairs", "0:0"], b"pair 0"),
                        (["--profile-path", "9,e.txt"], b"C is a parameter"),
                        (["--profile-path", "e.txt"], b"C,FILE"),
                        (["--profile", "e.txt", "--stream-text"], b"--profile")):
        e = subprocess.run(ARGS + extra, cwd=tmp_path, capture_output=True, timeout=300)
        assert e.returncode == 2 and word in e.stderr, (extra, e.stderr)
