"""The joint comparison of two stores does not depend on what its scratch held before the call: the three
situations of tests/test_gpu_scratch_history.py -- fresh memory under mcx_debug_fill_allocations, the owner's persistent scratch
under mcx_debug_fill_scratch, real residue behind other analyses and a larger call of its own -- with that file's fill bytes and
its rule of equality (dtype, shape, NaN positions and every other byte).  The baseline is energy_rows of the same rows with both
hooks off, held to tests/energy_ref.py once."""
import pytest

import energy_cases as K
import energy_ref as R
from test_gpu_scratch_history import FILLS, allocation_fill, allocation_fill_off, same_result  # noqa: F401 (the fixture is autouse)
from test_gpu_store_view import run

pytestmark = pytest.mark.gpu

NC, NP, STEPS = 37, 17, 30
FA, NA, FB, NB = 0, 12, 10, 20
KW = dict(n_a=-1, n_b=-1, nperm=17, seed=3)       # every row: 444 against 740, two label blocks
KW_DRAW = dict(n_a=70, n_b=0, nperm=15, seed=3, with_ll=True)
KW_DROP = dict(n_a=-1, n_b=-1, nperm=16, seed=4)  # rows with a constant and a non-finite column


@pytest.fixture(scope="module")
def world():
    from mcpar_amd import engine as E
    allocation_fill(-1)
    eg = run(NC, NP, STEPS)
    ra, rb = eg.samples_range(FA, NA), eg.samples_range(FB, NB)
    ta, tb = K.normal_rows(37, 4, 1), K.normal_rows(29, 4, 2, shift=0.25)
    ta[:, 1] = tb[:, 1] = 0.5
    ta[7, 2] = K.NAN
    W = dict(eg=eg, ra=ra, rb=rb, ta=ta, tb=tb, sa=E.select_chains_rows(ra, NA, NC, list(range(NC))),
             sb=E.select_chains_rows(rb, NB, NC, list(range(NC))))
    W["base"] = E.energy_rows(ra, NA, NC, rb, NB, NC, **KW)
    W["base_draw"] = E.energy_rows(ra, NA, NC, rb, NB, NC, **KW_DRAW)
    W["base_drop"] = E.energy_rows(ta, 37, 1, tb, 29, 1, **KW_DROP)
    R.check(W["base"], R.restate(ra, rb, **KW), NP + 1, E.debug_energy_sums(ra, NA, NC, rb, NB, NC, **KW))
    R.check(W["base_draw"], R.restate(ra, rb, **KW_DRAW), NP + 1)
    R.check(W["base_drop"], R.restate(ta, tb, **KW_DROP), 5)
    yield W
    W["sa"].close()
    W["sb"].close()
    eg.close()


@pytest.mark.parametrize("byte", FILLS, ids=lambda b: "0x%02X" % b)
def test_fresh_memory(world, byte):
    from mcpar_amd import engine as E
    W = world
    assert allocation_fill(byte) == 0
    assert same_result(E.energy_rows(W["ra"], NA, NC, W["rb"], NB, NC, **KW), W["base"])
    assert same_result(E.energy_rows(W["ra"], NA, NC, W["rb"], NB, NC, **KW_DRAW), W["base_draw"])
    assert same_result(E.energy_rows(W["ta"], 37, 1, W["tb"], 29, 1, **KW_DROP), W["base_drop"])
    assert same_result(W["eg"].energy(FA, NA, FB, NB, **KW), W["base"])
    assert same_result(E.energy_stores(W["sa"], W["sb"], **KW), W["base"])
    assert allocation_fill(-1) >= 5 * 4  # every call allocates its scratch: had the hook done nothing, the count would say so


@pytest.mark.parametrize("byte", FILLS, ids=lambda b: "0x%02X" % b)
def test_persistent_scratch(world, byte):
    from mcpar_amd import engine as E
    W = world
    calls = ((W["eg"], lambda: W["eg"].energy(FA, NA, FB, NB, **KW)), (W["sa"], lambda: E.energy_stores(W["sa"], W["sb"], **KW)),
             (W["eg"], lambda: W["eg"].energy_store(FA, NA, W["sb"], **KW)))
    for owner, call in calls:
        W["eg"].rank_summary()      # so that the owners' scratch exists: this unit keeps none of its own
        W["sa"].rank_summary()
        nbytes = E.debug_fill_scratch(owner, byte)
        assert len(nbytes) == 3 and sum(nbytes) > 0
        assert same_result(call(), W["base"]), "0x%02X" % byte


@pytest.mark.parametrize("before", ["rank_summary", "compare", "energy_larger"])
def test_residue_of_another_analysis(world, before):
    from mcpar_amd import engine as E
    W = world
    eg, sa, sb = W["eg"], W["sa"], W["sb"]
    big = dict(n_a=-1, n_b=-1, nperm=300, seed=1, with_ll=True)
    residue = dict(rank_summary=(lambda: eg.rank_summary(), lambda: sa.rank_summary()),
                   compare=(lambda: eg.compare(0, STEPS, 0, STEPS), lambda: E.compare_stores(sb, sb)),
                   energy_larger=(lambda: eg.energy(0, STEPS, 0, STEPS, **big), lambda: E.energy_stores(sb, sb, **big)))[before]
    residue[0]()
    assert same_result(eg.energy(FA, NA, FB, NB, **KW), W["base"])
    residue[0]()
    assert same_result(eg.energy_store(FA, NA, sb, **KW), W["base"])
    residue[1]()
    assert same_result(E.energy_stores(sa, sb, **KW), W["base"])
    assert same_result(E.energy_stores(sa, sb, **KW_DRAW), W["base_draw"])
