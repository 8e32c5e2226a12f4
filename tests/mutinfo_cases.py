"""Rows shared by the tests of the mutual information between columns.  Every generator gives MCout rows
[n, np + 1] in float32: the parameters, then a log L below zero."""
import numpy as np

NAN, INF = float("nan"), float("inf")
# fixed with tests/mutinfo_ref.py alone (test_mutinfo_cpu.py runs that check again)
NORMAL_SEEDS = (1, 2, 3)
CURVED_SEED, CURVED_NULL_SEED = 5, 6


def with_ll(x):
    x = np.asarray(x, np.float64)
    return np.concatenate([x, -0.5 * (x ** 2).sum(axis=1, keepdims=True) - 1e-3], axis=1).astype(np.float32)


def normal_rows(n, np_, seed):
    """n rows of np_ independent normal parameters"""
    return with_ll(np.random.default_rng([seed, n, np_]).normal(0.0, 1.0, (n, np_)))


def normal_pair(n, rho, seed):
    """a bivariate normal with correlation rho: mi = -log(1 - rho^2) / 2"""
    g = np.random.default_rng([seed, n, 77]).normal(0.0, 1.0, (n, 2))
    g[:, 1] = rho * g[:, 0] + np.sqrt(1.0 - rho * rho) * g[:, 1]
    return with_ll(g)


def curved_pair(n, seed):
    """b = a^2 + 0.1 noise, a ~ N(0, 0.7): almost no correlation, an almost deterministic relation"""
    rng = np.random.default_rng([seed, n, 78])
    a = rng.normal(0.0, 0.7, n)
    return with_ll(np.stack([a, a * a + 0.1 * rng.normal(0.0, 1.0, n)], axis=1))


def integer_rows(n, np_, seed, span=6):
    """integer-valued floats in [0, span): many distances tie exactly at eps, and some points have all k neighbours at 0"""
    x = np.random.default_rng([seed, n, np_, 79]).integers(0, span, (n, np_)).astype(np.float64)
    return with_ll(x)


def one_column_ties(n, seed):
    """column 0 takes three values only, column 1 is continuous: a query's k nearest in column 0 are all at distance 0 there"""
    rng = np.random.default_rng([seed, n, 80])
    return with_ll(np.stack([rng.integers(0, 3, n).astype(np.float64), rng.normal(0.0, 1.0, n)], axis=1))


def repeated_rows(n, np_, seed, every=3):
    """rows of which all but every `every`-th repeat the row before, as rejected Metropolis steps do"""
    a = normal_rows(n, np_, seed)
    for i in range(1, n):
        if i % every:
            a[i] = a[i - 1]
    return a
