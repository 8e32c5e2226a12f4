"""mcx_proposal_from_cov -- the host step from a covariance to the incov of the next run -- against numpy, the float64
restatement tests/covariance_ref.py against np.cov, and the new declarations of include/mcx.h as C99.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import covariance_ref as R
from mcpar_amd import McxError
from mcpar_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_spd(rng, d, cond):
    """a symmetric positive definite matrix with eigenvalues log-spaced over a factor cond"""
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    ev = np.logspace(0, -np.log10(cond), d) * rng.uniform(0.5, 2.0)
    c = (q * ev) @ q.T
    return (c + c.T) / 2


def test_default_scale_rounding_and_symmetry():
    rng = np.random.default_rng(1)
    for d in (1, 2, 5, 16, 33):
        c = random_spd(rng, d, 1e3)
        p = E.proposal_from_cov(c, d)
        assert p.dtype == np.float32 and p.shape == (d, d)
        assert np.array_equal(p, p.T)
        want = np.float32((2.38 * 2.38 / d) * c)
        assert np.array_equal(np.triu(p), np.triu(want))
        assert np.array_equal(p, R.proposal(c, d)[0])
        p3 = E.proposal_from_cov(c, d, scale=3.0)
        assert np.array_equal(np.triu(p3), np.triu(np.float32(3.0 * c)))
        assert np.array_equal(E.proposal_from_cov(c, d, scale=-1.0), p)  # scale <= 0: the default


def test_leading_dimension_skips_log_l():
    rng = np.random.default_rng(2)
    d = 6
    full = random_spd(rng, d + 1, 1e2)
    full[d, :] = full[:, d] = np.nan  # the log L row and column are never read
    p = E.proposal_from_cov(full, d)
    assert np.array_equal(p, E.proposal_from_cov(np.ascontiguousarray(full[:d, :d]), d))


def test_rejects_nan_zero_variance_and_indefinite():
    rng = np.random.default_rng(3)
    d = 5
    c = random_spd(rng, d, 10.0)
    bad = c.copy()
    bad[1, 3] = bad[3, 1] = np.nan
    with pytest.raises(McxError) as ei:
        E.proposal_from_cov(bad, d)
    assert ei.value.code == 1 and "not finite" in str(ei.value)
    bad = c.copy()
    bad[2, :] = bad[:, 2] = 0.0  # a constant column
    with pytest.raises(McxError) as ei:
        E.proposal_from_cov(bad, d)
    assert "pivot 2" in str(ei.value)
    bad = c.copy()
    bad[0, 1] = bad[1, 0] = 10.0 * max(c[0, 0], c[1, 1])  # |cov_01| > sqrt(cov_00 cov_11)
    with pytest.raises(McxError) as ei:
        E.proposal_from_cov(bad, d)
    assert "pivot 1" in str(ei.value)
    with pytest.raises(McxError):
        E.proposal_from_cov(c * 1e60, d)  # overflows float
    for args in ((0,), (257,)):
        with pytest.raises((McxError, ValueError)):
            E.proposal_from_cov(np.eye(300), *args)


def test_accepts_exactly_what_the_float_cholesky_accepts():
    """a seeded batch of SPD and near-singular matrices: accepted <=> the float Cholesky restated in numpy succeeds"""
    rng = np.random.default_rng(4)
    verdicts = []
    for k in range(160):
        d = int(rng.integers(2, 13))
        c = random_spd(rng, d, 10.0 ** rng.uniform(0, 9))
        if k % 4 == 1:  # rank-deficient up to rounding
            v = rng.standard_normal((d, d - 1))
            c = v @ v.T
        if k % 4 == 2:  # two nearly collinear columns
            c[:, 1] = c[:, 0] * (1 + 1e-7 * rng.standard_normal())
            c[1, :] = c[:, 1]
            c[1, 1] = c[0, 0] * (1 + 2e-7 * rng.standard_normal())
        want, rc = R.proposal(c, d)
        try:
            got = E.proposal_from_cov(c, d)
            assert rc == 0, (k, d, rc)
            assert np.array_equal(got, want), k
            verdicts.append(True)
        except McxError as e:
            assert rc > 0 and "pivot %d" % (rc - 1) in str(e), (k, d, rc, str(e))
            verdicts.append(False)
    assert 20 < sum(verdicts) < 140, sum(verdicts)  # the batch holds both kinds


def test_fmaf_restatement_is_correctly_rounded():
    """the float fma the Cholesky restatement is built on, against exact rational arithmetic"""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a = rng.standard_normal(400).astype(np.float32)
    b = rng.standard_normal(400).astype(np.float32)
    c = (-(a.astype(np.float64) * b) * (1 + rng.standard_normal(400) * 10.0 ** rng.integers(-9, 1, 400))).astype(np.float32)
    for x, y, z in zip(a, b, c):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        got = R.fmaf(x, y, z)
        lo, hi = np.nextafter(got, np.float32(-np.inf)), np.nextafter(got, np.float32(np.inf))
        err = abs(Fraction(float(got)) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), (x, y, z, got)


@pytest.mark.parametrize("N,ncol,seed", [(2, 3, 1), (1000, 5, 2), (4097, 17, 3), (300, 41, 4)])
def test_reference_matches_np_cov(N, ncol, seed):
    rng = np.random.default_rng(seed)
    rows = (rng.standard_normal((N, ncol)) * rng.uniform(0.1, 30, ncol) + rng.uniform(-100, 100, ncol)).astype(np.float32)
    r = R.restate(rows)
    want = np.cov(rows.astype(np.float64), rowvar=False).reshape(ncol, ncol)
    assert (np.abs(r["cov"] - want) <= R.bound(want, N)).all()
    np.testing.assert_allclose(r["mean"], rows.astype(np.float64).mean(axis=0), rtol=1e-13)
    assert not r["flags"].any() and np.array_equal(r["cov"], r["cov"].T)
    c = R.corr_of(r["cov"])
    assert (np.diag(c) == 1).all() and np.abs(c).max() <= 1 + 1e-12


def test_reference_nonfinite_and_constant_columns():
    rng = np.random.default_rng(6)
    rows = rng.standard_normal((200, 5)).astype(np.float32)
    clean = R.restate(np.delete(rows, 2, axis=1))
    rows[17, 2] = np.inf
    rows[:, 4] = 0.75
    r = R.restate(rows)
    assert r["flags"].tolist() == [0, 0, 1, 0, 0] and np.isnan(r["mean"][2])
    assert np.isnan(r["cov"][2]).all() and np.isnan(r["cov"][:, 2]).all()
    keep = [0, 1, 3, 4]
    clean_rows = R.restate(np.delete(rows, 2, axis=1))
    assert np.array_equal(r["cov"][np.ix_(keep, keep)], clean_rows["cov"])
    assert np.array_equal(r["cov"][np.ix_([0, 1, 3], [0, 1, 3])], clean["cov"][np.ix_([0, 1, 2], [0, 1, 2])])
    assert (r["cov"][4, keep] == 0).all() and r["mean"][4] == 0.75
    c = R.corr_of(r["cov"])
    assert np.isnan(c[4]).all() and np.isnan(c[2]).all() and c[0, 0] == 1 and c[3, 3] == 1


def test_covariance_refuses_bad_arguments_without_a_device():
    rows = np.zeros((1, 3), np.float32)
    with pytest.raises(McxError) as ei:
        E.rows_covariance(rows, 1, 1)  # N = 1
    assert ei.value.code == 1
    with pytest.raises(McxError) as ei:
        E.rows_covariance(np.zeros((0, 3), np.float32), 0, 4)  # nsteps = 0
    assert ei.value.code == 1


def test_new_declarations_are_plain_c99(tmp_path):
    """include/mcx.h with the covariance entry points used must compile as C99 and link against libmcx.so"""
    src = tmp_path / "cov.c"
    src.write_text('#include "mcx.h"\n'
                   'int main(void){ double cov[9] = {2.0, 0.5, 9.0, 0.5, 1.0, 9.0, 9.0, 9.0, 9.0}; float incov[4];\n'
                   ' double mean[3]; int flags[3]; float rows[3] = {0.0f, 0.0f, 0.0f};\n'
                   ' int (*fs)(mcx_engine *, int, int, double *, double *, int *) = mcx_samples_covariance;\n'
                   ' if (!fs) return 5;\n'
                   ' if (mcx_proposal_from_cov(2, cov, 3, 0.0, incov) != MCX_OK) return 2;\n'
                   ' if (incov[1] != incov[2] || incov[0] != (float)(2.38 * 2.38 / 2 * 2.0)) return 3;\n'
                   ' cov[4] = 0.0;\n'
                   ' if (mcx_proposal_from_cov(2, cov, 3, 1.0, incov) != MCX_ERR_INVALID) return 4;\n'
                   ' if (mcx_rows_covariance(rows, 1, 1, 2, mean, cov, flags) != MCX_ERR_INVALID) return 6;\n'
                   ' return mcx_abi_version() == MCX_ABI_VERSION && MCX_ABI_VERSION == 5 ? 0 : 1; }\n')
    exe = tmp_path / "cov"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", os.path.join(ROOT, "mcpar_amd"), "-lmcx",
                           "-Wl,-rpath," + os.path.join(ROOT, "mcpar_amd")])
    assert subprocess.call([str(exe)]) == 0
