"""mcx_debug_live_resources needs no device, and a call that fails its argument checks holds nothing afterwards: the
count is the same before and after (with or without a GPU in the machine)."""
import ctypes as C

import numpy as np
import pytest


def test_calls_that_fail_their_argument_checks_leave_the_count_unchanged():
    import mcpar_amd as M
    from mcpar_amd import engine as E
    lib = M.load()
    before = E.debug_live_resources()
    assert len(before) == 4
    with pytest.raises(M.McxError):
        M.Engine(0, 64)
    assert E.debug_live_resources() == before
    cols = np.zeros(3, E.SUMMARY_DTYPE)
    assert lib.mcx_rows_summary(None, 8, 8, 2, None, 0, cols.ctypes.data_as(C.c_void_p), None) != 0
    assert E.debug_live_resources() == before
    with pytest.raises(M.McxError):
        E.format_rows(np.zeros((2, 0), np.float32))
    assert E.debug_live_resources() == before


def test_a_null_out_is_refused():
    import mcpar_amd as M
    assert M.load().mcx_debug_live_resources(None) != 0
    assert "NULL" in M.load().mcx_last_error().decode()
