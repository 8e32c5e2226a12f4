"""The comparison of two stores does not depend on what its scratch held before the call: the three
situations of tests/test_gpu_scratch_history.py -- fresh memory under mcx_debug_fill_allocations, the owner's persistent scratch
under mcx_debug_fill_scratch, real residue behind a rank summary and a step table -- with that file's fill bytes and its rule of
equality (dtype, shape, NaN positions and every other byte).  The baseline is compare_rows of the same rows with both hooks off,
held to tests/compare_ref.py once."""
import pytest

import compare_cases as K
import compare_ref as R
from test_gpu_scratch_history import FILLS, allocation_fill, allocation_fill_off, same_result  # noqa: F401 (the fixture is autouse)
from test_gpu_store_view import run

pytestmark = pytest.mark.gpu

NC, NP, STEPS = 37, 17, 30
FA, NA, FB, NB = 0, 12, 10, 20


@pytest.fixture(scope="module")
def world():
    from mcpar_amd import engine as E
    allocation_fill(-1)
    eg = run(NC, NP, STEPS)
    ra, rb = eg.samples_range(FA, NA), eg.samples_range(FB, NB)
    ta, tb = K.tie_rows(3, 5, 37, 1), K.tie_rows(3, 9, 11, 2, shift=0.25)
    ta[7, 2] = K.NAN
    W = dict(eg=eg, ra=ra, rb=rb, ta=ta, tb=tb, sa=E.select_chains_rows(ra, NA, NC, list(range(NC))),
             sb=E.select_chains_rows(rb, NB, NC, list(range(NC))))
    W["base"] = E.compare_rows(ra, NA, NC, rb, NB, NC)
    W["base_ties"] = E.compare_rows(ta, 37, 5, tb, 11, 9)
    R.check(W["base"], R.restate(ra, NA, NC, rb, NB, NC))
    R.check(W["base_ties"], R.restate(ta, 37, 5, tb, 11, 9))
    yield W
    W["sa"].close()
    W["sb"].close()
    eg.close()


@pytest.mark.parametrize("byte", FILLS, ids=lambda b: "0x%02X" % b)
def test_fresh_memory(world, byte):
    from mcpar_amd import engine as E
    W = world
    assert allocation_fill(byte) == 0
    assert same_result(E.compare_rows(W["ra"], NA, NC, W["rb"], NB, NC), W["base"])
    assert same_result(E.compare_rows(W["ta"], 37, 5, W["tb"], 11, 9), W["base_ties"])
    assert same_result(W["eg"].compare(FA, NA, FB, NB), W["base"])
    assert same_result(E.compare_stores(W["sa"], W["sb"]), W["base"])
    assert allocation_fill(-1) >= 4  # every call allocates its scratch: had the hook done nothing, the count would say so


@pytest.mark.parametrize("byte", FILLS, ids=lambda b: "0x%02X" % b)
def test_persistent_scratch(world, byte):
    from mcpar_amd import engine as E
    W = world
    calls = ((W["eg"], lambda: W["eg"].compare(FA, NA, FB, NB)), (W["sa"], lambda: E.compare_stores(W["sa"], W["sb"])),
             (W["eg"], lambda: W["eg"].compare_store(FA, NA, W["sb"])))
    for owner, call in calls:
        assert same_result(call(), W["base"])  # so that the scratch exists
        nbytes = E.debug_fill_scratch(owner, byte)
        assert len(nbytes) == 3 and sum(nbytes) > 0
        assert same_result(call(), W["base"]), "0x%02X" % byte


@pytest.mark.parametrize("before", ["rank_summary", "step_table", "compare_larger"])
def test_residue_of_another_analysis(world, before):
    from mcpar_amd import engine as E
    W = world
    eg, sa, sb = W["eg"], W["sa"], W["sb"]
    residue = dict(rank_summary=(lambda: eg.rank_summary(), lambda: sa.rank_summary()),
                   step_table=(lambda: eg.step_table(), lambda: sa.step_table()),
                   compare_larger=(lambda: eg.compare(0, STEPS, 0, STEPS), lambda: E.compare_stores(sb, sb)))[before]
    residue[0]()
    assert same_result(eg.compare(FA, NA, FB, NB), W["base"])
    residue[0]()
    assert same_result(eg.compare_store(FA, NA, sb), W["base"])
    residue[1]()
    assert same_result(E.compare_stores(sa, sb), W["base"])
