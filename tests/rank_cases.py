"""Inputs the rank-summary tests share (tests/test_rank_summary_cpu.py, tests/test_gpu_rank_summary.py): the two
demonstration cases that basic R-hat / ESS call converged, and rows built from columns."""
import numpy as np

DEMO_T, DEMO_NC = 1000, 4
SCALE_SEED, CAUCHY_SEED = 12, 14  # chosen on the float64 reference: every threshold below holds with room to spare


def demo_scale(seed=SCALE_SEED):
    """four iid normal chains, one with 3 x the scale: x [T, nc] float32"""
    x = np.random.default_rng(seed).standard_normal((DEMO_T, DEMO_NC))
    x[:, 3] *= 3.0
    return x.astype(np.float32)


def demo_cauchy(seed=CAUCHY_SEED):
    """four Cauchy chains, one shifted by 1: x [T, nc] float32"""
    x = np.random.default_rng(seed).standard_cauchy((DEMO_T, DEMO_NC))
    x[:, 3] += 1.0
    return x.astype(np.float32)


def check_demo_scale(basic_rhat, basic_ess, rhat_folded, ess_tail):
    assert basic_rhat <= 1.01, basic_rhat
    assert rhat_folded >= 1.05, rhat_folded
    assert ess_tail < basic_ess / 20, (ess_tail, basic_ess)


def check_demo_cauchy(basic_rhat, basic_ess, ess_bulk):
    assert basic_rhat <= 1.01, basic_rhat
    assert ess_bulk < basic_ess / 10, (ess_bulk, basic_ess)


def rows_of(cols):
    """columns [T, nc] -> rows [T * nc, ncol] float32 (MCout layout)"""
    x = np.stack([np.asarray(c, np.float32) for c in cols], axis=2)
    T, nc, ncol = x.shape
    return np.ascontiguousarray(x.reshape(T * nc, ncol))
