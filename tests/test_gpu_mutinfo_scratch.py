"""The mutual information between columns does not depend on what its scratch held before the call: the
three situations of tests/test_gpu_scratch_history.py -- fresh memory under mcx_debug_fill_allocations, the owner's persistent
scratch under mcx_debug_fill_scratch, real residue behind other analyses and a larger call of its own -- with that file's fill
bytes and its rule of equality (dtype, shape, NaN positions and every other byte).  The baseline is rows_mutual_info of the same
rows with both hooks off, held to tests/mutinfo_ref.py once."""
import pytest

import mutinfo_cases as K
import mutinfo_ref as R
from test_gpu_scratch_history import FILLS, allocation_fill, allocation_fill_off, same_result  # noqa: F401 (the fixture is autouse)
from test_gpu_store_view import run

pytestmark = pytest.mark.gpu

NC, NP, STEPS = 37, 17, 30
KW = dict(n=-1, nperm=5, seed=3, pairs=[(0, 1), (16, 2), (3, 17), (9, 4)], with_ll=True)   # every row of the run: several tiles
KW_SPACED = dict(n=150, k=2, nperm=2, seed=3, pairs=[(0, 1), (5, 6)])
KW_DROP = dict(n=-1, nperm=3, seed=4)                                                    # a constant and a non-finite column


def flat(call):
    return R.flat(call)


@pytest.fixture(scope="module")
def world():
    from mcpar_amd import engine as E
    allocation_fill(-1)
    eg = run(NC, NP, STEPS)
    rows = eg.samples_range(0, STEPS)
    t = K.normal_rows(70, 4, 1)
    t[:, 1] = 0.5
    t[7, 2] = K.NAN
    W = dict(eg=eg, rows=rows, t=t, st=E.select_chains_rows(rows, STEPS, NC, list(range(NC))))
    for name, r, nc, kw in (("base", rows, NC, KW), ("base_spaced", rows, NC, KW_SPACED), ("base_drop", t, 1, KW_DROP)):
        got = E.rows_mutual_info(r, len(r) // nc, nc, **kw)
        R.check(got, R.restate(r, scale=got["scale"], **kw))
        W[name] = flat(got)
    yield W
    W["st"].close()
    eg.close()


@pytest.mark.parametrize("byte", FILLS, ids=lambda b: "0x%02X" % b)
def test_fresh_memory(world, byte):
    from mcpar_amd import engine as E
    W = world
    assert allocation_fill(byte) == 0
    assert same_result(flat(E.rows_mutual_info(W["rows"], STEPS, NC, **KW)), W["base"])
    assert same_result(flat(E.rows_mutual_info(W["rows"], STEPS, NC, **KW_SPACED)), W["base_spaced"])
    assert same_result(flat(E.rows_mutual_info(W["t"], 70, 1, **KW_DROP)), W["base_drop"])
    assert same_result(flat(W["eg"].mutual_info(**KW)), W["base"])
    assert same_result(flat(W["st"].mutual_info(**KW)), W["base"])
    assert allocation_fill(-1) >= 5 * 4  # every call allocates its scratch: had the hook done nothing, the count would say so


@pytest.mark.parametrize("byte", FILLS, ids=lambda b: "0x%02X" % b)
def test_persistent_scratch(world, byte):
    from mcpar_amd import engine as E
    W = world
    for owner, call in ((W["eg"], lambda: W["eg"].mutual_info(**KW)), (W["st"], lambda: W["st"].mutual_info(**KW))):
        W["eg"].rank_summary()      # so that the owners' scratch exists: this unit keeps none of its own
        W["st"].rank_summary()
        nbytes = E.debug_fill_scratch(owner, byte)
        assert len(nbytes) == 3 and sum(nbytes) > 0
        assert same_result(flat(call()), W["base"]), "0x%02X" % byte


@pytest.mark.parametrize("before", ["rank_summary", "energy", "mutual_info_larger"])
def test_residue_of_another_analysis(world, before):
    W = world
    eg, st = W["eg"], W["st"]
    big = dict(n=-1, k=8, nperm=40, seed=1, with_ll=True, pairs=[(a, a + 1) for a in range(17)])
    residue = dict(rank_summary=(lambda: eg.rank_summary(), lambda: st.rank_summary()),
                   energy=(lambda: eg.energy(0, STEPS, 0, STEPS, nperm=30), lambda: st.energy(st, nperm=30)),
                   mutual_info_larger=(lambda: eg.mutual_info(**big), lambda: st.mutual_info(**big)))[before]
    residue[0]()
    assert same_result(flat(eg.mutual_info(**KW)), W["base"])
    residue[1]()
    assert same_result(flat(st.mutual_info(**KW)), W["base"])
    assert same_result(flat(st.mutual_info(**KW_SPACED)), W["base_spaced"])
