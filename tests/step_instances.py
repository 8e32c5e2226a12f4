"""Recipes: for every step-kernel template instance the launchers of mcpar_amd/csrc/mcx_k_*.hip can launch
(engine.step_instance_list()), the smallest job that makes mcx_run launch it -- or the reason, taken from the
dispatcher's code, why no job can.  Plain data and host logic: importing this needs no GPU.

Shapes.  d: the ragged size of the lane count where the family allows one (LPC 4 -> 12, LPC 8 -> 20: a lane without
parameters), and the full one beside it.  n: a grid of more than one 256-thread workgroup that ends in a partial wavefront
and a partial lane group, n = 2 (256 / L) + 64 / L + 3 for L lanes per chain.  Steps: nburn = 110 (two tuner events and a
tail), nsamp = 37 with sync = 10 (snapshots inside a launch), pl = 1 -- 147 steps are several 16/20/32-step phases of the
one-launch kernel and a partial last one.  Every recipe pins OPT_PERSIST, OPT_SPLIT_RNG, OPT_BLOCKS_PER_LANE, OPT_FUSE and
OPT_ACCEPT_MASK: no instance is reached by an automatic choice alone."""
import collections

import numpy as np

from mcpar_amd import engine as E

NBURN, NSAMP, SYNC, PL = 110, 37, 10, 1.0
NCU_MI355X = 256  # what the CPU tests size the two-owner recipes of k_run_small with (the GPU tests ask device_info)

LIKS_FAST = ("LIK_ROSEN1", "LIK_GAUSS", "LIK_MIX")
LIKS_ALL = LIKS_FAST + ("LIK_ROSEN2F",)
D_OF_LPC = {1: (4,), 2: (8,), 4: (12, 16), 8: (20, 32)}
# generic kernel: one d per lane count, none a multiple of 4 (even: Rosenbrock1), LPC 64 at d = 130
D_GENERIC = {1: 2, 2: 6, 4: 14, 8: 22, 16: 50, 32: 102, 64: 130}

Recipe = collections.namedtuple("Recipe", "name group lik ncomp d lanes two_owners fullcov opts samples stride expect")
Inst = E.StepInstance


def seg_n(lanes):
    """chains of a per-segment kernel's recipe: three workgroups, the last with a partial wavefront and lane group"""
    return 2 * (256 // lanes) + 64 // lanes + 3


def chains(r, ncu):
    """k_run_small without recorders and one block per lane needs two owner wavefronts in some workgroup: one wavefront
    more than the device has CUs, 257 * 64 / LPC2 chains on 256 CUs, less three (a partial lane group)"""
    return (ncu + 1) * 64 // r.lanes - 3 if r.two_owners else seg_n(r.lanes)


def options(persist, split, bpl, mask=0, fuse=1):
    return {"OPT_PERSIST": persist, "OPT_SPLIT_RNG": split, "OPT_BLOCKS_PER_LANE": bpl, "OPT_FUSE": fuse, "OPT_ACCEPT_MASK": mask}


def lik_spec(r):
    """(kind, params, ncomp) of a recipe's likelihood: the same numbers for oracle_lib.make_vlfunc and mcpar_amd.make_vlfunc"""
    d = r.d
    if r.lik == "LIK_ROSEN1":
        return E.VL_ROSENBROCK1, None, 0
    if r.lik == "LIK_ROSEN2F":
        return E.VL_ROSENBROCK2_FIXED, None, 0
    if r.lik == "LIK_GAUSS":
        return E.VL_GAUSSIAN, np.concatenate([np.linspace(-1, 1, d), np.linspace(0.5, 2.0, d)]).astype(np.float32), 0
    K = r.ncomp  # K unit-variance components, means 5 k / (K - 1), weights (5, 1, ..., 1)
    means = np.stack([np.full(d, 5.0 * k / (K - 1)) for k in range(K)]).astype(np.float32)
    return E.VL_GAUSSMIX, np.concatenate([means.ravel(), [5] + [1] * (K - 1)]).astype(np.float32), K


def incov(r):
    if not r.fullcov:
        return None
    a = np.random.default_rng(5 + r.d).normal(size=(r.d, r.d))
    return (0.02 * (np.eye(r.d) + 0.5 * a @ a.T / r.d)).astype(np.float32)


def _recipes():
    out = []

    def add(group, lik, d, lanes, opts, expect, samples=1, stride=1, ncomp=0, two_owners=False, fullcov=False, tag=""):
        ncomp = ncomp or (8 if lik == "LIK_MIX" else 0)
        name = "%s-%s-L%d-b%d-d%d-s%d%s%s" % (group, lik[4:].lower(), lanes, opts["OPT_BLOCKS_PER_LANE"], d, stride if samples else 0,
                                              "-" if tag else "", tag)
        out.append(Recipe(name, group, lik, ncomp, d, lanes, two_owners, fullcov, opts, samples, stride, tuple(expect)))

    # k_fused_fast<LPC, MAIN, LIK, false, false, EMIT>: the per-segment modes and several blocks per lane off
    for lpc, ds in D_OF_LPC.items():
        for lik in LIKS_ALL:
            for d in ds:
                for samples, stride, emit in ((0, 1, "EMIT_NONE"), (1, 1, "EMIT_EVERY"), (1, 3, "EMIT_THIN")):
                    add("fast", lik, d, lpc, options(0, 0, 1),
                        [Inst("fast", lpc, 1, lik, False, "EMIT_NONE", False), Inst("fast", lpc, 1, lik, True, emit, False)], samples, stride)
    # k_fused_fastb<LPC2, BPL, MAIN, LIK>: fused_choice takes the forced bpl while bpl <= lpc; ragged chains are legal here
    for lpc, ds in D_OF_LPC.items():
        for bpl in (2, 4):
            if bpl > lpc:
                continue
            for lik in LIKS_FAST:
                for d, stride in zip(ds, (1, 3)) if len(ds) > 1 else ((ds[0], 1), (ds[0], 3)):
                    add("fastb", lik, d, lpc // bpl, options(0, 0, bpl),
                        [Inst("fastb", lpc // bpl, bpl, lik, m, "", False) for m in (False, True)], 1, stride)
    # full covariance: k_fused_fast<LPC, MAIN, LIK, false, true> with one block per lane forced, the mirrored k_fused_fastb
    # <LPC2, 2, MAIN, LIK, true> with two (lpc 4 or 8 only: fused_choice's `mirrored`)
    for lpc, ds in D_OF_LPC.items():
        for lik in LIKS_FAST:
            for d, stride in zip(ds, (1, 3)) if len(ds) > 1 else ((ds[0], 1), (ds[0], 3)):
                add("fast_full", lik, d, lpc, options(0, 0, 1), [Inst("fast_full", lpc, 1, lik, m, "", False) for m in (False, True)],
                    1, stride, fullcov=True)
                if lpc >= 4:
                    add("fastb_full", lik, d, lpc // 2, options(0, 0, 2),
                        [Inst("fastb_full", lpc // 2, 2, lik, m, "", False) for m in (False, True)], 1, stride, fullcov=True)
    # small-n mode with pre-generated normals: k_gen_normals<LPC> and k_fused_fast<LPC, MAIN, LIK, true> in turn
    for lpc, ds in D_OF_LPC.items():
        for lik in LIKS_FAST:
            for d, stride in zip(ds, (1, 3)) if len(ds) > 1 else ((ds[0], 1), (ds[0], 3)):
                add("pregen", lik, d, lpc, options(0, 1, 1),
                    [Inst("pregen", lpc, 1, lik, m, "", False) for m in (False, True)] + [Inst("gen_normals", lpc, 1, "", False, "", False)],
                    1, stride)
    # k_fused_steps<LPC, LIK, MAIN>: d not a multiple of 4 with the accept mask on; the hot path's own sizes with the mask
    # alone (thinned); the mixture with more components than the hot path takes, mask off
    for lpc, d in D_GENERIC.items():
        for lik in LIKS_ALL:
            add("generic", lik, d, lpc, options(0, 0, 1, mask=1), [Inst("generic", lpc, 1, lik, m, "", False) for m in (False, True)])
    for lpc, ds in D_OF_LPC.items():
        for lik in LIKS_ALL:
            add("generic", lik, ds[-1], lpc, options(0, 0, 1, mask=1),
                [Inst("generic", lpc, 1, lik, m, "", False) for m in (False, True)], 1, 3, tag="mask")
    add("generic", "LIK_MIX", 16, 4, options(0, 0, 1), [Inst("generic", 4, 1, "LIK_MIX", m, "", False) for m in (False, True)],
        ncomp=11, tag="ncomp11")
    # k_run_small<LPC2, BPL, LIK, REC>: one launch for the whole run.  Recorders (mcxk_persist_recorders: own * bpl <= 1): one
    # block per lane and one owner wavefront per workgroup; without them at one block per lane: two owners in some workgroup
    for lpc, ds in D_OF_LPC.items():
        for lik in LIKS_FAST:
            for d, stride in zip(ds, (1, 3)) if len(ds) > 1 else ((ds[0], 1), (ds[0], 3)):
                add("persist_rec", lik, d, lpc, options(1, 0, 1), [Inst("persist", lpc, 1, lik, False, "", True)], 1, stride)
            add("persist_two_owners", lik, ds[0], lpc, options(1, 0, 1), [Inst("persist", lpc, 1, lik, False, "", False)], 1,
                3 if lpc == 2 else 1, two_owners=True)
    # several blocks per lane (mcxk_persist_bpl: bpl <= lpc and d % (4 bpl) == 0): never with recorders
    for lpc2, bpl, ds in ((1, 2, (8,)), (2, 2, (16,)), (4, 2, (24, 32)), (1, 4, (16,)), (2, 4, (32,))):
        for lik in LIKS_FAST:
            for d, stride in zip(ds, (1, 3)) if len(ds) > 1 else ((ds[0], 1), (ds[0], 3)):
                add("persist_blocks", lik, d, lpc2, options(1, 0, bpl), [Inst("persist", lpc2, bpl, lik, False, "", False)], 1, stride)
    return out


RECIPES = _recipes()

# instances no job reaches, with the dispatcher's reason
EXEMPT = {
    Inst("persist", lpc2, bpl, lik, False, "", True):
        "mcxk_persist_recorders: own * bpl <= 1 is false for bpl >= 2; only the MCX_PERSIST_REC tuning variable selects it"
    for lpc2, bpl in ((1, 2), (2, 2), (4, 2), (1, 4), (2, 4)) for lik in LIKS_FAST
}

GROUPS = sorted({(r.group, r.lik) for r in RECIPES})


def names(records):
    return sorted(E.step_instance_name(r) for r in records)


def oracle_run(r, ncu=NCU_MI355X, threads=1):
    """the recipe on the CPU oracle: (engine, pinit, n).  The accept mask is always recorded: the CPU test asks it whether
    both branches of the accept rule occurred"""
    import oracle_lib as O
    n = chains(r, ncu)
    kind, params, ncomp = lik_spec(r)
    p = O.default_pinit(r.d, n)
    vo, keep = O.make_vlfunc(kind, r.d, params, ncomp)
    eo = O.Engine(r.d, n, pl=PL, sync=SYNC, threads=threads)
    eo.set_record(samples=True, mask=True, stride=r.stride)
    eo.run(NSAMP, NBURN, p, vo, incov(r))
    return eo, p, n
