"""The compiled step-kernel instances as a checked fact, without a GPU: the library's own list (the launchers' switches
run dry, mcx_debug_step_instance_list) against the matrix spelt out here, the recipes of step_instances.py against the
list, the id's encode / decode / name, and every recipe's oracle run alone -- a recipe in which the accept rule never
takes one of its branches could not show a wrong kernel."""
import itertools

import numpy as np
import pytest

import step_instances as S
from mcpar_amd import engine as E

Inst = E.StepInstance
P2 = (1, 2, 4, 8)
BURN_MAIN = (False, True)


def matrix():
    """DESIGN.md section 5's table, as products"""
    fast = {Inst("fast", lpc, 1, lik, main, emit, False) for lpc, lik in itertools.product(P2, S.LIKS_ALL)
            for main, emit in ((False, "EMIT_NONE"), (True, "EMIT_NONE"), (True, "EMIT_EVERY"), (True, "EMIT_THIN"))}
    fastb = {Inst("fastb", lpc2, bpl, lik, main, "", False) for (lpc2, bpl), lik, main in
             itertools.product(((1, 2), (2, 2), (4, 2), (1, 4), (2, 4)), S.LIKS_FAST, BURN_MAIN)}
    fast_full = {Inst("fast_full", lpc, 1, lik, main, "", False) for lpc, lik, main in itertools.product(P2, S.LIKS_FAST, BURN_MAIN)}
    fastb_full = {Inst("fastb_full", lpc2, 2, lik, main, "", False) for lpc2, lik, main in itertools.product((2, 4), S.LIKS_FAST, BURN_MAIN)}
    pregen = {Inst("pregen", lpc, 1, lik, main, "", False) for lpc, lik, main in itertools.product(P2, S.LIKS_FAST, BURN_MAIN)}
    gen = {Inst("gen_normals", lpc, 1, "", False, "", False) for lpc in P2}
    generic = {Inst("generic", lpc, 1, lik, main, "", False) for lpc, lik, main in
               itertools.product((1, 2, 4, 8, 16, 32, 64), S.LIKS_ALL, BURN_MAIN)}
    persist = {Inst("persist", lpc2, bpl, lik, False, "", rec) for (lpc2, bpl), lik, rec in
               itertools.product(((1, 1), (2, 1), (4, 1), (8, 1), (1, 2), (2, 2), (4, 2), (1, 4), (2, 4)), S.LIKS_FAST, BURN_MAIN)}
    parts = dict(fast=fast, fastb=fastb, fast_full=fast_full, fastb_full=fastb_full, pregen=pregen, gen_normals=gen,
                 generic=generic, persist=persist)
    assert {k: len(v) for k, v in parts.items()} == dict(fast=64, fastb=30, fast_full=24, fastb_full=12, pregen=24, gen_normals=4,
                                                         generic=56, persist=54)
    return set().union(*parts.values())


@pytest.fixture(scope="module")
def listed():
    return E.step_instance_list()


def test_library_list_is_the_matrix(listed):
    want, got = matrix(), set(listed)
    assert len(listed) == len(got), "the list repeats an instance"
    assert got == want, "listed but not in the matrix: %s; in the matrix but not listed: %s" % (S.names(got - want), S.names(want - got))
    assert len(listed) == 268


def test_every_listed_instance_has_a_recipe_or_an_exemption(listed):
    got = set(listed)
    by_recipe = {}
    for r in S.RECIPES:
        for rec in r.expect:
            by_recipe.setdefault(rec, []).append(r.name)
    assert len({r.name for r in S.RECIPES}) == len(S.RECIPES)
    assert not set(by_recipe) - got, "recipes expect instances the library does not list: %s" % S.names(set(by_recipe) - got)
    assert not set(S.EXEMPT) - got, "exempted but not listed: %s" % S.names(set(S.EXEMPT) - got)
    both = set(by_recipe) & set(S.EXEMPT)
    assert not both, "a recipe and an exemption: %s" % S.names(both)
    orphans = got - set(by_recipe) - set(S.EXEMPT)
    assert not orphans, "neither recipe nor exemption: %s" % S.names(orphans)
    assert all(reason and "\n" not in reason for reason in S.EXEMPT.values())
    assert len(S.EXEMPT) == 15  # k_run_small<..., BPL >= 2, ..., REC = true>: 5 (LPC2, BPL) pairs x 3 likelihoods


def test_recipes_pin_every_option_and_use_the_stated_shapes():
    for r in S.RECIPES:
        assert set(r.opts) == {"OPT_PERSIST", "OPT_SPLIT_RNG", "OPT_BLOCKS_PER_LANE", "OPT_FUSE", "OPT_ACCEPT_MASK"}, r.name
        assert r.opts["OPT_PERSIST"] in (0, 1) and r.opts["OPT_SPLIT_RNG"] in (0, 1) and r.opts["OPT_BLOCKS_PER_LANE"] in (1, 2, 4), r.name
        assert r.lik != "LIK_ROSEN1" or r.d % 2 == 0, r.name
        n = S.chains(r, S.NCU_MI355X)
        lanes = n * r.lanes
        if r.two_owners:  # one owner wavefront more than CUs, the last one partial, the last lane group too
            assert (lanes + 63) // 64 == S.NCU_MI355X + 1 and lanes % 64 and n <= 16448, r.name
        else:  # more than one 256-thread workgroup, a partial last wavefront (64 lanes per chain: a chain is a wavefront)
            assert lanes > 512 and (lanes % 64 or r.lanes == 64), r.name
        if r.group.startswith("persist"):
            bpl = r.opts["OPT_BLOCKS_PER_LANE"]
            assert r.d % (4 * bpl) == 0 and bpl * r.lanes == max(1, 1 << ((r.d + 3) // 4 - 1).bit_length()), r.name
    emits = {rec.emit for r in S.RECIPES for rec in r.expect if rec.family == "fast" and rec.main}
    assert emits == {"EMIT_NONE", "EMIT_EVERY", "EMIT_THIN"}


def test_id_round_trip_and_names(listed):
    seen = set()
    for rec in listed:
        word = E.step_instance_encode(rec)
        assert E.step_instance_decode(word) == rec
        name = E.step_instance_name(rec)
        assert name not in seen, name  # the name tells instances apart
        seen.add(name)
    assert E.step_instance_name(Inst("fastb", 2, 4, "LIK_MIX", True, "", False)) == "k_fused_fastb<2,4,true,LIK_MIX>"
    assert E.step_instance_name(Inst("fast", 1, 1, "LIK_MIX", True, "EMIT_THIN", False)) == "k_fused_fast<1,true,LIK_MIX,false,false,EMIT_THIN>"
    assert E.step_instance_name(Inst("generic", 64, 1, "LIK_ROSEN2F", True, "", False)) == "k_fused_steps<64,LIK_ROSEN2F,true>"
    assert E.step_instance_name(Inst("persist", 8, 1, "LIK_GAUSS", False, "", False)) == "k_run_small<8,1,LIK_GAUSS,false>"
    assert "user" in E.step_instance_name(E.step_instance_decode(9 | 4 << 4 | 1 << 11 | 7 << 14))


@pytest.mark.parametrize("group", sorted({r.group for r in S.RECIPES}))
def test_oracle_alone_takes_both_branches_of_the_accept_rule(group):
    for r in (r for r in S.RECIPES if r.group == group):
        eo, p, n = S.oracle_run(r, threads=4)
        m = eo.accept_mask
        nb, nm = int(m[:S.NBURN].sum()), int(m[S.NBURN:].sum())
        assert (nb, nm) == (eo.naccept_burn, eo.naccept_main), r.name
        assert 0 < nb < n * S.NBURN and 0 < nm < n * S.NSAMP, (r.name, nb, nm)
        assert m[:S.NBURN].any(axis=0).sum() > n // 2 and m[S.NBURN:].any(axis=0).sum() > n // 2, r.name  # (most chains move in either loop)
        assert m.any(axis=0).all(), "%s: chains stuck for the whole run: %s" % (r.name, np.flatnonzero(~m.any(axis=0))[:5])
        kept = (S.NSAMP + r.stride - 1) // r.stride
        assert eo.samples.shape == (kept * n, r.d + 1), r.name
        eo.close()
