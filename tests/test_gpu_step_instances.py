"""Every compiled step-kernel instance (engine.step_instance_list()) reached on purpose, at the smallest shape where it can
go wrong, and compared with the oracle bit for bit: the recipes of step_instances.py, one test per (family, likelihood).
What a run launched is asked of the library's ledger (Engine.step_instances, formed from the launchers' template
arguments), not inferred from the options: a dispatcher that falls back to another instance fails here by name."""
import numpy as np
import pytest

import step_instances as S

pytestmark = pytest.mark.gpu

SEEN = set()     # records the recipes' runs launched
STARTED = set()  # the (group, likelihood) cases this session ran


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run_recipe(r, ncu):
    import mcpar_amd as M
    from mcpar_amd import engine as E
    eo, p, n = S.oracle_run(r, ncu, threads=8 if n_big(r, ncu) else 1)
    kind, params, ncomp = S.lik_spec(r)
    vg, keep = M.make_vlfunc(kind, r.d, params, ncomp)
    eg = M.Engine(r.d, n, pl=S.PL, sync=S.SYNC)
    for name, value in r.opts.items():
        eg.set_option(getattr(E, name), value)
    eg.set_option(E.OPT_SAMPLES, r.samples)
    eg.set_option(E.OPT_SAMPLE_STRIDE, r.stride)
    eg.run(S.NSAMP, S.NBURN, p, vg, S.incov(r))
    c = eg.counters
    assert c["meet_timeouts"] == 0, (r.name, c)
    got, want = set(eg.step_instances), set(r.expect)
    SEEN.update(got)
    assert got == want, "%s (n = %d) launched %s, the recipe is for %s" % (r.name, n, S.names(got), S.names(want))
    assert (c["naccept_burn"], c["naccept_main"]) == (eo.naccept_burn, eo.naccept_main), r.name
    assert np.array_equal(eg.accept_counts, eo.accept_counts), r.name
    assert np.array_equal(bits(eg.tuner_trace), bits(eo.tuner_trace)), r.name
    for name in ("state", "loglike", "chol", "mean", "var", "musigall"):
        assert np.array_equal(bits(getattr(eg, name)), bits(getattr(eo, name))), (r.name, name)
    if r.samples:
        a, b = eg.samples, eo.samples  # (the oracle keeps every stride-th step too: set_record)
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), (r.name, "samples")
    if r.opts["OPT_ACCEPT_MASK"]:
        assert np.array_equal(eg.accept_mask, eo.accept_mask), (r.name, "accept mask")
    eg.close()
    eo.close()


def n_big(r, ncu):
    return S.chains(r, ncu) >= 1000


@pytest.mark.parametrize("group,lik", S.GROUPS, ids=["%s-%s" % (g, k[4:].lower()) for g, k in S.GROUPS])
def test_recipes_launch_their_instances_and_match_the_oracle(group, lik):
    from mcpar_amd import engine as E
    ncu = E.device_info()[1]
    todo = [r for r in S.RECIPES if (r.group, r.lik) == (group, lik)]
    assert todo
    STARTED.add((group, lik))
    for r in todo:
        run_recipe(r, ncu)


def test_every_listed_instance_was_reached():
    """the union of what the recipes' runs launched, plus the exemptions, is the library's list -- nothing compiled that no
    test ran.  (Defined last: it needs every case above to have run in this session; a case that failed leaves its
    instances out and fails this test too.)"""
    from mcpar_amd import engine as E
    if STARTED != set(S.GROUPS):
        pytest.skip("only %d of the %d recipe cases ran in this session: the union is not whole" % (len(STARTED), len(S.GROUPS)))
    listed = set(E.step_instance_list())
    reached = SEEN | set(S.EXEMPT)
    assert SEEN and not (SEEN & set(S.EXEMPT)), S.names(SEEN & set(S.EXEMPT))
    assert reached == listed, "listed, never launched: %s; launched, not listed: %s" % (S.names(listed - reached), S.names(reached - listed))
    print("%d of %d listed instances launched, %d exempt" % (len(SEEN), len(listed), len(S.EXEMPT)))
