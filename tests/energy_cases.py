"""Rows shared by the tests of the joint comparison."""
import numpy as np

NAN, INF = float("nan"), float("inf")
FINDING = dict(na=448, nb=320, rho=0.9, nperm=199, seed=0, rng=100)  # the numpy seed was chosen with tests/energy_ref.py alone


def normal_rows(n, np_, seed, shift=0.0):
    """n rows of np_ normal parameters and a log L below zero"""
    rng = np.random.default_rng([seed, n, np_])
    a = rng.normal(0.0, 1.0, (n, np_ + 1)).astype(np.float32)
    a[:, :np_] += np.float32(shift)
    a[:, -1] = -np.abs(a[:, -1]) - np.float32(1e-3)
    return a


def finding_rows(k=None):
    """A, B of the same law (two iid N(0, 1) columns) and B' with correlation rho between its columns: equal marginals"""
    c = FINDING
    rng = np.random.default_rng(c["rng"] if k is None else k)
    a = rng.normal(0.0, 1.0, (c["na"], 2))
    b = rng.normal(0.0, 1.0, (c["nb"], 2))
    bc = b.copy()
    bc[:, 1] = c["rho"] * b[:, 0] + np.sqrt(1.0 - c["rho"] ** 2) * b[:, 1]
    ll = lambda x: np.concatenate([x, -0.5 * (x ** 2).sum(axis=1, keepdims=True)], axis=1).astype(np.float32)
    return ll(a), ll(b), ll(bc)
