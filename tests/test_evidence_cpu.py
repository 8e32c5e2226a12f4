"""The evidence of a store without a GPU: the entry points and the ABI, the refusals of every entry point
(all before a device is touched), mcx_evidence_proposal against numpy, mcx_evidence_iterate against tests/evidence_ref.py, the
launch geometry, the header as C99, the host half alone, plain and under sanitizers -- and the proof that the inputs of the GPU
test of the whole call (tests/test_gpu_evidence.py) are decisive by the reference alone.

Decisive: the target is MCX_VL_GAUSSMIX with d = 3, centres (0, 0, 0) and (6, 6, 6) and weights 0.3 and 0.7, so log Z = 1.5 log
2 pi.  4096 iid float rows in 16 "chains", the first half for fitting, 2048 draws from the engine's normals (the oracle's
mcxo_normal4), seeds 0 to 4, proposals K = 1 (fitted) and K = 2 (moments per true component): in all ten cases
|log_z_ref - truth| <= 3 se_ref and the loop converges in under 50 passes.  No case is left out."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import evidence_ref as R
from mcpar_amd import McxError
from mcpar_amd import engine as E
from mcpar_amd._lib import EvidenceGeometry, EvidenceMixtureC, EvidenceResultC, EvidenceSpecC, VLFunc, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mcx_samples_evidence", "mcx_rows_evidence", "mcx_store_evidence", "mcx_evidence_proposal", "mcx_evidence_iterate",
                "mcx_debug_evidence_logg", "mcx_debug_evidence_draws", "mcx_debug_evidence_l", "mcx_debug_evidence_geometry",
                "mcx_debug_evidence_times")
RTOL = 1e-9


def test_entry_points_are_declared_and_exported_and_the_abi_is_5():
    L = load()
    header = open(os.path.join(ROOT, "include", "mcx.h")).read()
    for name in ENTRY_POINTS:
        assert getattr(L, name).argtypes is not None, name
        assert "int %s(" % name in header, name
    for name in ("mcx_evidence_mixture", "mcx_evidence_spec", "mcx_evidence_result", "mcx_evidence_geometry"):
        assert "} %s;" % name in header, name
    assert L.mcx_abi_version() == 5 and "#define MCX_ABI_VERSION 5" in header
    assert C.sizeof(EvidenceMixtureC) == 40 and C.sizeof(EvidenceSpecC) == 40 and C.sizeof(EvidenceResultC) == 112
    assert C.sizeof(EvidenceGeometry) == 15 * 8
    assert (E.EVIDENCE_MAX_K, E.EVIDENCE_STREAM) == (R.MAX_K, R.STREAM) == (8, 8)
    assert (E.EVIDENCE_NOT_CONVERGED, E.EVIDENCE_NO_ESS) == (R.NOT_CONVERGED, R.NO_ESS) == (1, 2)
    text = open(os.path.join(ROOT, "mcpar_amd", "csrc", "mcx_evidence_host.hpp")).read()
    assert "ST_EVIDENCE = 8" in text and "hip" not in text.replace("__HIPCC__", "").replace("mcx_evidence.hip", "").replace("no HIP", "")


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_arguments_refused_before_a_device_is_touched():
    """MCX_ERR_INVALID (1) or MCX_ERR_UNSUPPORTED (4), never MCX_ERR_NO_DEVICE (2)"""
    L = load()
    err = L.mcx_last_error
    d, T, nc = 2, 8, 4
    rows = np.zeros((T * nc, d + 1), np.float32)
    fp = rows.ctypes.data_as(C.POINTER(C.c_float))
    vl = VLFunc(E.VL_GAUSSIAN, d, 0, None)
    res = EvidenceResultC()
    good = E.Proposal([1.0, 2.0], np.zeros((2, d)), [np.eye(d)] * 2)

    def spec(**kw):
        return C.byref(E._evidence_spec(**kw))

    def call(r=fp, a=(T, nc), np_=d, v=vl, s=None, p=None, rs=res, null_spec=False):
        return L.mcx_rows_evidence(r, a[0], a[1], np_, None if v is None else C.byref(v), None if null_spec else (s or spec()),
                                   None if p is None else C.byref(p.c), None if rs is None else C.byref(rs))

    assert call(r=None) == 1 and b"rows is NULL" in err()
    assert call(null_spec=True) == 1 and b"spec is NULL" in err()
    assert call(rs=None) == 1 and b"res is NULL" in err()
    assert call(v=None) == 1 and b"L is NULL" in err()
    for k in (0, -1, 9):
        p = E.Proposal(np.ones(max(k, 1)), np.zeros((max(k, 1), d)), [np.eye(d)] * max(k, 1))
        p.c.k = k
        assert call(p=p) == 1 and b"1 to 8 components" in err(), k
    for w in (0.0, -1.0, np.nan, np.inf):
        assert call(p=E.Proposal([1.0, w], np.zeros((2, d)), [np.eye(d)] * 2)) == 1 and b"weights[1]" in err()
    for sc in (0.0, -2.0, np.inf, np.nan):
        assert call(p=E.Proposal([1.0], np.zeros((1, d)), [np.eye(d)], scale=sc)) == 1 and b"scale" in err()
        assert call(s=spec(scale=sc)) == 1 and b"scale" in err()
    assert call(p=E.Proposal([1.0], [[0.0, np.nan]], [np.eye(d)])) == 1 and b"centres[0][1] is not finite" in err()
    for f in (-2, T, T + 5):
        assert call(s=spec(fit_steps=f)) == 1 and b"fit_steps" in err()
        assert call(s=spec(fit_steps=f), p=good) == 1 and b"fit_steps" in err()
    assert call(s=spec(fit_steps=0)) == 1 and b"a fitted proposal needs steps to fit on" in err()
    assert call(a=(1, nc)) == 1 and b"fit" in err()                       # one step: its default, nsteps / 2, is 0
    assert call(a=(2, 1), s=spec(fit_steps=1)) == 1 and b">= 2 rows" in err()
    assert call(v=VLFunc(E.VL_GAUSSIAN, d + 1, 0, None)) == 1 and b"L->d = 3 but the rows have np = 2" in err()
    for tol in (-1e-300, -1.0, np.nan):
        assert call(s=spec(tol=tol)) == 1 and b"tol" in err()
    assert call(s=spec(max_iter=-1)) == 1 and b"max_iter" in err()
    assert call(s=spec(ndraw=-1)) == 1 and b"ndraw" in err()
    assert call(np_=0) == 1 and b"np = 0" in err() and call(np_=257, v=VLFunc(E.VL_GAUSSIAN, 257, 0, None)) == 1 and b"np = 257" in err()
    assert call(a=(0, nc)) == 1 and call(a=(T, 0)) == 1 and b"at least one step" in err()
    assert call(s=spec(ndraw=1 << 31)) == 4 and b"fewer than 2^31" in err()
    assert call(a=(1 << 20, 1 << 12), s=spec(fit_steps=1, ndraw=16)) == 4 and b"fewer than 2^31" in err()
    sing = E.Proposal([1.0, 1.0], np.zeros((2, d)), [np.eye(d), np.array([[1.0, 0.0], [0.0, 0.0]])])
    assert call(p=sing) == 1 and b"component 1" in err() and b"pivot 1 = 0" in err()
    # the store and engine forms, the debug entries
    sp = spec()
    assert L.mcx_store_evidence(None, C.byref(vl), sp, None, C.byref(res)) == 1 and b"store s is NULL" in err()
    assert L.mcx_samples_evidence(None, 0, 8, None, sp, None, C.byref(res)) == 1 and b"engine is NULL" in err()
    assert L.mcx_debug_evidence_times(None, 0, 8, None, sp, None, C.byref(res), (C.c_double * 8)()) == 1 and b"engine is NULL" in err()
    dp = C.POINTER(C.c_double)
    out = np.zeros(64)
    assert L.mcx_debug_evidence_l(fp, T, nc, d, C.byref(vl), sp, None, C.byref(res), None, out.ctypes.data_as(dp)) == 1 and b"NULL" in err()
    assert L.mcx_debug_evidence_logg(None, 4, d, C.byref(good.c), out.ctypes.data_as(dp)) == 1
    assert L.mcx_debug_evidence_logg(fp, 4, d, None, out.ctypes.data_as(dp)) == 1 and b"proposal m is NULL" in err()
    assert L.mcx_debug_evidence_logg(fp, 0, d, C.byref(good.c), out.ctypes.data_as(dp)) == 1 and b"n = 0" in err()
    assert L.mcx_debug_evidence_logg(fp, 1 << 31, d, C.byref(good.c), out.ctypes.data_as(dp)) == 4
    assert L.mcx_debug_evidence_draws(d, C.byref(good.c), None, 0, 0, None, None, None, None) == 1 and b"ndraw = 0" in err()
    assert L.mcx_debug_evidence_draws(d, None, None, 0, 4, None, None, None, None) == 1
    assert L.mcx_debug_evidence_draws(d, C.byref(good.c), None, 0, 4, None, None, None, fp) == 1 and b"L is NULL" in err()
    assert L.mcx_debug_evidence_draws(d, C.byref(sing.c), None, 0, 4, None, None, None, None) == 1 and b"pivot" in err()
    assert L.mcx_evidence_proposal(d, None, None, None, out.ctypes.data_as(dp)) == 1
    assert L.mcx_evidence_proposal(d, C.byref(good.c), None, None, None) == 1 and b"lc is NULL" in err()
    g = EvidenceGeometry()
    assert L.mcx_debug_evidence_geometry(d, 10, 10, 1, None) == 1 and L.mcx_debug_evidence_geometry(0, 10, 10, 1, C.byref(g)) == 1
    assert L.mcx_debug_evidence_geometry(d, 10, 10, 9, C.byref(g)) == 1 and L.mcx_debug_evidence_geometry(d, 0, 10, 1, C.byref(g)) == 1
    assert L.mcx_debug_evidence_geometry(d, 1 << 31, 10, 1, C.byref(g)) == 4
    with pytest.raises(McxError) as ei:
        E.rows_evidence(rows, T, nc, vl, E.Proposal(np.ones(9), np.zeros((9, d)), [np.eye(d)] * 9))
    assert ei.value.code == 1 and "1 to 8 components" in str(ei.value)


# ---- the proposal's factors -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("np_", [1, 3, 16, 64, 256])
@pytest.mark.parametrize("K", [1, 8])
def test_proposal_factors_against_numpy(np_, K):
    rng = np.random.default_rng(np_ * 10 + K)
    covs = np.empty((K, np_, np_))
    for k in range(K):
        A = rng.normal(size=(np_, np_))
        covs[k] = A @ A.T / np_ + np.diag(rng.uniform(0.1, 2.0, np_))
    w, c, scale = rng.uniform(0.1, 3.0, K), rng.normal(size=(K, np_)), 1.7
    Cf, W, lc = E.evidence_proposal(E.Proposal(w, c, covs, scale))
    _, _, rlc = R.proposal(w, c, covs, scale)
    assert np.abs(lc - rlc).max() <= 1e-12 * np.abs(rlc).max() and (np.abs(lc - rlc) <= 1e-12 * np.abs(rlc)).all()
    for k in range(K):
        assert (np.triu(Cf[k], 1) == 0).all() and (np.triu(W[k], 1) == 0).all() and (np.diag(Cf[k]) > 0).all()
        tol = 64 * np_ * R.EPS * np.linalg.norm(Cf[k]) * np.linalg.norm(W[k])
        assert np.abs(W[k] @ Cf[k] - np.eye(np_)).max() <= tol
        assert np.abs(Cf[k] @ Cf[k].T - scale * scale * covs[k]).max() <= tol


def test_a_singular_covariance_is_refused_and_names_its_pivot():
    rng = np.random.default_rng(1)
    x = rng.normal(size=(100, 4))
    x[:, 2] = 1.5   # a constant column
    with pytest.raises(McxError) as ei:
        E.evidence_proposal(E.Proposal([1.0, 1.0], np.zeros((2, 4)), [np.eye(4), np.cov(x.T)]))
    assert ei.value.code == 1 and "component 1" in str(ei.value) and "pivot 2 = 0 is not positive and finite" in str(ei.value)
    with pytest.raises(McxError) as ei:
        E.evidence_proposal(E.Proposal([1.0], np.zeros((1, 2)), [[[1.0, 2.0], [2.0, 1.0]]]))
    assert "component 0" in str(ei.value) and "pivot 1 = -3" in str(ei.value)
    with pytest.raises(McxError) as ei:
        E.evidence_proposal(E.Proposal([1.0], np.zeros((1, 2)), [[[np.nan, 0.0], [0.0, 1.0]]]))
    assert "pivot 0 = nan" in str(ei.value)


# ---- the estimator on host arrays -------------------------------------------------------------------------------------------------
def check_iterate(l1, l2, **kw):
    got, ref = E.evidence_iterate(l1, l2, **kw), R.bridge(l1, l2, **kw)
    assert (got["iters"], got["flags"], got["ndraw_zero"], got["n1"], got["n2"]) == (ref["iters"], ref["flags"], ref["ndraw_zero"],
                                                                                     ref["n1"], ref["n2"])
    assert got["neff"] == ref["neff"] and got["ess_f2"] == ref["ess_f2"] == len(l1)
    for name in ("lstar", "log_z", "se", "re2_draws", "re2_rows", "log_z_is", "log_z_ris"):
        assert abs(got[name] - ref[name]) <= RTOL * abs(ref[name]), (name, got[name], ref[name])
    return got


def test_iterate_equals_the_restatement():
    rng = np.random.default_rng(5)
    for n1, n2, sd, neff in ((1000, 400, 0.5, None), (257, 1023, 2.0, 100.0), (64, 64, 5.0, 1e9), (2, 1, 1.0, None), (1, 2, 1.0, None)):
        l1, l2 = 3.0 + sd * rng.normal(size=n1) + 0.5 * sd * sd, 3.0 + sd * rng.normal(size=n2) - 0.5 * sd * sd
        got = check_iterate(l1, l2, neff=neff)
        assert got["flags"] == 0 and np.isfinite(got["log_z"])
    l2[0] = -np.inf
    assert check_iterate(l1, l2)["ndraw_zero"] == 1


def test_iterate_on_its_edges():
    # l constant: that constant exactly, after one pass
    for c in (0.0, 3.25, -1234.5678, 700.0):
        got = check_iterate(np.full(100, c), np.full(40, c))
        assert got["log_z"] == c and got["iters"] == 1 and got["flags"] == 0 and got["se"] == 0.0
        assert got["log_z_is"] == c and got["log_z_ris"] == c
    # a range of +-700 about l*: no overflow, a finite result
    l1, l2 = np.linspace(-700.0, 700.0, 101), np.linspace(700.0, -700.0, 41)
    with np.errstate(over="raise", invalid="raise"):
        got = check_iterate(l1, l2)
    assert all(np.isfinite(got[k]) for k in ("log_z", "se", "log_z_is", "log_z_ris")) and abs(got["lstar"]) < 1e-9
    # one pass allowed: the flag
    rng = np.random.default_rng(2)
    l1, l2 = rng.normal(size=50) + 1.0, rng.normal(size=50) - 1.0
    got = check_iterate(l1, l2, max_iter=1)
    assert got["iters"] == 1 and got["flags"] == E.EVIDENCE_NOT_CONVERGED
    assert check_iterate(l1, l2)["flags"] == 0
    # refusals
    for bad1, bad2, text in ((l1, np.full(50, -np.inf), "every one of the 50 draws has L = 0"),
                             (l1, np.where(np.arange(50) == 7, np.inf, l2), "draw 7"),
                             (l1, np.where(np.arange(50) == 8, np.nan, l2), "draw 8"),
                             (np.where(np.arange(50) == 9, -np.inf, l1), l2, "row 9"),
                             (np.where(np.arange(50) >= 11, np.nan, l1), l2, "row 11")):
        with pytest.raises(McxError) as ei:
            E.evidence_iterate(bad1, bad2)
        assert ei.value.code == 1 and text in str(ei.value)
    for kw, text in ((dict(tol=-1.0), "tol"), (dict(max_iter=-1), "max_iter"), (dict(neff=0.0), "neff"), (dict(neff=np.nan), "neff")):
        with pytest.raises(McxError) as ei:
            E.evidence_iterate(l1, l2, **kw)
        assert ei.value.code == 1 and text in str(ei.value)
    L, res = load(), EvidenceResultC()
    dp = C.POINTER(C.c_double)
    assert L.mcx_evidence_iterate(None, 5, l2.ctypes.data_as(dp), 5, 5.0, 1e-10, 10, C.byref(res)) == 1
    assert L.mcx_evidence_iterate(l1.ctypes.data_as(dp), 0, l2.ctypes.data_as(dp), 5, 5.0, 1e-10, 10, C.byref(res)) == 1
    assert L.mcx_evidence_iterate(l1.ctypes.data_as(dp), 5, l2.ctypes.data_as(dp), 1 << 31, 5.0, 1e-10, 10, C.byref(res)) == 4


# ---- the decisive inputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2], ids=["fitted", "two-components"])
@pytest.mark.parametrize("seed", R.DEC_SEEDS)
def test_decisive_inputs_by_the_reference_alone(seed, K):
    ref, l1, l2 = R.decisive_case(seed, K)
    err = abs(ref["log_z"] - R.DEC_TRUTH)
    print("seed %d, K = %d: |err| / se = %.3g, se = %.3g, %d passes" % (seed, K, err / ref["se"], ref["se"], ref["iters"]))
    assert err <= 3 * ref["se"] and ref["iters"] < 50 and ref["flags"] == 0
    check_iterate(l1, l2)   # and the library's host loop on the same arrays


def test_the_draws_restatement_uses_the_engines_streams():
    """the component's uniform is section 25's form on block (j, 0, 1, 0) of stream 8, and one component draws z itself"""
    x, comp = R.draws([1.0], np.zeros((1, 5)), np.eye(5)[None], 3, 4)
    assert (comp == 0).all()
    for j in range(4):
        assert np.array_equal(x[j], R.normals(3, j, 5)[:5])
    u = [R.uniform(3, j) for j in range(2000)]
    assert 0 <= min(u) and max(u) < 1 and abs(np.mean(u) - 0.5) < 0.03
    _, comp = R.draws([1.0, 3.0], np.zeros((2, 1)), np.ones((2, 1, 1)), 3, 2000)
    assert np.array_equal(comp, (np.array(u) * 4.0 >= 1.0).astype(np.int32))


# ---- the launch geometry ----------------------------------------------------------------------------------------------------------
def test_geometry():
    for np_, Rt in ((1, 64), (128, 64), (129, 32), (256, 32)):
        g = E.debug_evidence_geometry(np_, 100000, 5000, 8)
        assert g["tile_rows"] == Rt and g["slices"] == 256 // Rt and g["use_mfma"] == 0 and g["block"] == 256
        assert g["sweep_tiles"] == -(-100000 // Rt) and g["sweep_workgroups"] == min(g["sweep_tiles"], 4096)
        assert g["sweep_lds_bytes"] == (256 + 8 * 64 + 2048 + 256) * 8 + 256 * 4 + Rt * (np_ | 1) * 4 <= 64 * 1024
        assert g["w_chunk_rows"] == {1: 1, 128: 16, 129: 8, 256: 8}[np_]
        assert g["draw_rows"] == max(16, 256 // np_) and g["draw_workgroups"] == -(-5000 // g["draw_rows"])
        assert g["draw_lds_bytes"] <= 64 * 1024
        assert (g["terms_workgroups_rows"], g["terms_workgroups_draws"]) == (98, 5)
    g = E.debug_evidence_geometry(16, (1 << 31) - 1, (1 << 31) - 1, 1)
    assert g["sweep_workgroups"] == 4096 and g["terms_workgroups_rows"] == 1024 and g["draw_workgroups"] == -(-((1 << 31) - 1) // 16)


# ---- the header and the host half on their own ------------------------------------------------------------------------------------
def test_header_is_plain_c99_with_the_evidence_declarations(tmp_path):
    src = tmp_path / "evidence_cabi.c"
    src.write_text('#include "mcx.h"\n'
                   'int main(void){ double w[1] = {1.0}, c[2] = {0.0, 0.0}, cov[4] = {4.0, 0.0, 0.0, 9.0}, Cf[4], W[4], lc[1];\n'
                   ' double l1[3] = {1.0, 1.0, 1.0}, l2[2] = {1.0, 1.0}; float rows[6] = {0};\n'
                   ' mcx_evidence_mixture m = {1, 0, 0, 0, 0, 1.0}; mcx_evidence_spec sp = {0, 0u, -1, 1, 0, 1e-10, 1.0};\n'
                   ' mcx_evidence_result r; mcx_evidence_geometry g; mcx_vlfunc L = {MCX_VL_GAUSSIAN, 2, 0, 0, 0, 0};\n'
                   ' m.weights = w; m.centres = c; m.covs = cov;\n'
                   ' if (mcx_evidence_proposal(2, &m, Cf, W, lc) != MCX_OK || Cf[0] != 2.0 || Cf[3] != 3.0 || W[0] != 0.5 || W[1] != 0.0) return 2;\n'
                   ' if (mcx_evidence_iterate(l1, 3, l2, 2, 3.0, 1e-10, 0, &r) != MCX_OK || r.log_z != 1.0 || r.iters != 1) return 3;\n'
                   ' if (mcx_debug_evidence_geometry(256, 100, 100, 8, &g) != MCX_OK || g.tile_rows != 32 || g.use_mfma != 0) return 4;\n'
                   ' if (mcx_rows_evidence(0, 2, 1, 2, &L, &sp, &m, &r) != MCX_ERR_INVALID) return 5;\n'
                   ' if (mcx_store_evidence(0, &L, &sp, &m, &r) != MCX_ERR_INVALID) return 6;\n'
                   ' if (mcx_samples_evidence(0, 0, 2, &L, &sp, &m, &r) != MCX_ERR_INVALID) return 7;\n'
                   ' if (mcx_debug_evidence_logg(rows, 0, 2, &m, l1) != MCX_ERR_INVALID) return 8;\n'
                   ' if (sizeof(mcx_evidence_mixture) != 40 || sizeof(mcx_evidence_spec) != 40 || sizeof(r) != 112 || sizeof(g) != 120) return 9;\n'
                   ' if (MCX_EVIDENCE_MAX_K != 8 || MCX_EVIDENCE_NOT_CONVERGED != 1 || MCX_EVIDENCE_NO_ESS != 2 || MCX_EVIDENCE_TIMES != 8) return 10;\n'
                   ' return mcx_abi_version() == MCX_ABI_VERSION && MCX_ABI_VERSION == 5 ? 0 : 1; }\n')
    exe = tmp_path / "evidence_cabi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", os.path.join(ROOT, "mcpar_amd"), "-lmcx",
                           "-Wl,-rpath," + os.path.join(ROOT, "mcpar_amd")])
    assert subprocess.call([str(exe)]) == 0


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_host_code_alone(tmp_path, flags):
    """tests/cpp/evidence_host_check.cc: the host half (csrc/mcx_evidence_host.hpp: the factors, the refusals, the terms, the loop)
    as a stand-alone program, plain and under AddressSanitizer and UBSan"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "evidence_host_check"
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror"] + flags +
                   ["-I", ROOT, os.path.join(ROOT, "tests", "cpp", "evidence_host_check.cc"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
