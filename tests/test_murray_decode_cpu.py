"""decode_pass (mcx_murray.hip), the host's reading of the counter block a Murray kernel turn sends home, on hand-built
blocks: which half of word 0 holds the survivors, what a turn over candidates stood for, and which cells are the min-arg
screen's and which the sum screens'.  Host logic only: no GPU.  The layout is include/mcx.h's (mcx_debug_murray_decode)."""
import numpy as np
import pytest

from mcpar_amd import engine as E

CELLS, MULTI_K, WORDS = 64, 4, 132
W_MIN, W_SUMS, W_TRIED = 1, 1 + CELLS, 1 + 2 * CELLS + 1
N = 1000


def block(low=0, high=0, tried=(0, 0, 0, 0), cells_min=None, cells_sums=None):
    w = np.zeros(WORDS, np.uint64)
    w[0] = np.uint64(low | (high << 32))
    if cells_min is not None:
        w[W_MIN:W_MIN + CELLS] = cells_min
    if cells_sums is not None:
        w[W_SUMS:W_SUMS + CELLS] = cells_sums
    w[W_TRIED:W_TRIED + MULTI_K // 2] = np.asarray(tried, np.uint32).view(np.uint64)
    return w


@pytest.mark.parametrize("it,expect", [(0, 17), (1, 23), (2, 17), (5, 23)])
def test_survivors_come_from_the_half_of_the_turn(it, expect):
    survivors, passes, pairs, kmin, ksums = E.murray_decode(block(low=17, high=23), it, False, False, 40, N)
    assert survivors == expect
    assert (passes, pairs, kmin, ksums) == (1, 40 * N, 0, 0)


def test_candidates_two_tried_nobody_left():
    survivors, passes, pairs, _, _ = E.murray_decode(block(low=0, high=9, tried=(5, 3, 0, 0)), 2, True, False, 5, N)
    assert (survivors, passes, pairs) == (0, 2, 8 * N)


def test_candidates_survivors_tried_them_all():
    survivors, passes, pairs, _, _ = E.murray_decode(block(low=9, high=1, tried=(5, 3, 2, 1)), 3, True, False, 5, N)
    assert (survivors, passes, pairs) == (1, MULTI_K, 11 * N)
    # (and whatever tried[] says: a survivor has been through all of them)
    survivors, passes, pairs, _, _ = E.murray_decode(block(low=2, tried=(5, 3, 0, 0)), 0, True, False, 5, N)
    assert (survivors, passes, pairs) == (2, MULTI_K, 8 * N)


def test_candidates_nothing_tried_nobody_left_is_no_pass():
    """(cannot happen with chains in the turn; pinned as it is)"""
    survivors, passes, pairs, _, _ = E.murray_decode(block(), 1, True, False, 5, N)
    assert (survivors, passes, pairs) == (0, 0, 0)


@pytest.mark.parametrize("multi", [False, True])
def test_kept_pairs_min_and_sums_apart(multi):
    cmin = np.arange(1, CELLS + 1, dtype=np.uint64)                   # sum 2080
    csums = np.arange(1, CELLS + 1, dtype=np.uint64) * np.uint64(1 << 33) + np.uint64(7)  # past 32 bits: whole words are added
    w = block(low=3, tried=(4, 0, 0, 0), cells_min=cmin, cells_sums=csums)
    out = E.murray_decode(w, 0, multi, True, 4, N)
    assert out[3] == 2080 and out[4] == 2080 * (1 << 33) + 7 * CELLS
    # the first and the last cell of either kind count, the words around them do not
    for lo, hi, which in ((W_MIN, W_SUMS, 3), (W_SUMS, W_SUMS + CELLS, 4)):
        w = block()
        w[lo], w[hi - 1] = 11, 13
        out = E.murray_decode(w, 0, multi, True, 4, N)
        assert out[which] == 24 and out[7 - which] == 0
    w = block()
    w[W_SUMS + CELLS] = 99  # the kernels' own word behind the cells
    assert E.murray_decode(w, 0, multi, True, 4, N)[3:] == (0, 0)
    # no screen can have run: nothing is read
    w = block(low=3, cells_min=cmin, cells_sums=csums)
    assert E.murray_decode(w, 0, multi, False, 4, N)[3:] == (0, 0)


def test_short_block_is_refused():
    import mcpar_amd as M
    with pytest.raises(M.McxError):
        E.murray_decode(np.zeros(WORDS - 1, np.uint64), 0, False, False, 1, N)
