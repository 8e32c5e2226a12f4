"""Runs whose chains start where the log-likelihood is -inf or NaN, or with an infinite or NaN coordinate: the shared case
builder of tests/test_nonfinite_cpu.py (the oracle alone) and tests/test_gpu_nonfinite.py (the engine).

The contract is DESIGN.md section 3, "Non-finite values": the local test is `log1(u24) < ly' - ly` with IEEE comparisons, so
  - a difference that is NaN (a NaN on either side, or -inf - -inf) rejects whatever the draw,
  - a chain at ly = -inf takes the first proposal whose ly' is finite (the difference is +inf; log1(u24) < 0, -inf at u24 = 0),
  - a chain at a finite ly never takes a proposal with ly' = -inf or NaN (-inf < -inf is false also at u24 = 0),
and a chain is a lane group of its own: what it holds reaches no other chain at pl = 1.
check_semantics below replays exactly these three rules from the rows of a run; it consults neither the oracle's nor the
kernels' acceptance code."""
import numpy as np

from test_gpu_step_ref import CASES, SEED, default_pinit, params_of, spd   # noqa: F401  (shapes and options: one table)
import step_ref as R

# the kernel families (tests/test_gpu_step_ref.py says at each case which kernel it reaches and why)
FAMILIES = ("generic_6d", "small_n_16d", "hot_16d", "hot_32d_257", "pregen_16d", "fullcov_8d", "fullcov_32d_mirrored",
            "mixture_32d", "two_blocks_per_lane_16d", "unfused_16d", "gauss_33d")

# the poisoned starts: name -> (coordinates replaced: "all", "mid", "first" or "last"; value)
POISONS = (("all_1e12", "all", 1e12), ("one_nan", "mid", np.nan), ("x0_plus_inf", "first", np.inf), ("all_3e38", "all", 3e38),
           ("last_minus_inf", "last", -np.inf), ("all_nan", "all", np.nan))
MIX_POISON = ("all_1e20", "all", 1e20)   # the mixture: sum (x - m)^2 overflows in every component


def chains_per_wavefront(d, blocks_per_lane=1):
    """the hot-path kernels hold a chain in lpc / blocks_per_lane lanes, lpc = the 4-parameter blocks rounded up to a power of two"""
    lpc = 1
    while lpc < (d + 3) // 4:
        lpc <<= 1
    return max(1, 64 * blocks_per_lane // lpc)


def placements(n, cpw):
    """chain 0; an adjacent pair; both sides of a wavefront boundary of the hot-path layout (cpw chains) and of one chain per
    lane (64); one chain in the middle; the last chain (of a ragged wavefront wherever n is no multiple of cpw)"""
    want = [0, cpw + 2, cpw + 3, cpw - 1, cpw, n // 2, n - 1, 63, 64]
    out = []
    for j in want:
        if 0 <= j < n and j not in out:
            out.append(j)
    return out


def poisoned_start(name):
    """the case `name` of CASES with its poisoned chains: dict of everything a run needs"""
    kind, d, n, nburn, nsamp, pl, sync, ncomp, full, mask, opts, ran = CASES[name]
    kinds = list(POISONS) + ([MIX_POISON] if kind == R.VL_GAUSSMIX else [])
    clean = default_pinit(d, n)
    pinit = clean.copy()
    where = {}
    for i, j in enumerate(placements(n, chains_per_wavefront(d, opts.get("OPT_BLOCKS_PER_LANE", 1)))):
        pname, coords, value = kinds[i % len(kinds)]
        k = {"all": slice(None), "mid": d // 2, "first": 0, "last": d - 1}[coords]
        pinit[j, k] = np.float32(value)
        where[j] = pname
    healthy = np.array([j for j in range(n) if j not in where])
    return dict(name=name, kind=kind, d=d, n=n, nburn=nburn, nsamp=nsamp, pl=pl, sync=sync, ncomp=ncomp, mask=mask, opts=opts, ran=ran,
                params=params_of(kind, d, ncomp), incov=spd(d, 5) if full else None, clean=clean, pinit=pinit, where=where,
                poisoned=np.array(sorted(where)), healthy=healthy)


# ------------------------------------------------------------------------------------------------------------------
# comparisons: bits on everything that is not NaN, NaN exactly where the other side has one (x86 and gfx950 produce
# different default NaNs: neither sign nor payload is compared)
# ------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    bad = np.argwhere(na != nb)
    assert bad.size == 0, "%s: NaN on one side only, first at %s" % (what, bad[:3].tolist())
    bad = np.argwhere((bits(a) != bits(b)) & ~na)
    assert bad.size == 0, "%s: bits differ first at %s: %r != %r" % (what, bad[:3].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


def row_of_start(pinit, ly0):
    return np.concatenate([np.asarray(pinit, np.float32), np.asarray(ly0, np.float32)[:, None]], 1)


# ------------------------------------------------------------------------------------------------------------------
# the semantics, replayed from the rows of a run with nburn = 0 and pl = 1
# ------------------------------------------------------------------------------------------------------------------
def check_semantics(start, rows, mask, propose, loglike, label=""):
    """start[n, d + 1] = (pinit, ly of pinit); rows[nsteps, n, d + 1] the sample rows; mask[nsteps, n] or None.
    propose(t, x) -> the local proposals of step t from the states x (genLocal of the engine under test, itself checked
    against the float64 model elsewhere); loglike(x) -> ly'.  For every step and chain:
      a row either stays or becomes the proposal (x', ly'), and the mask, where there is one, says which;
      ly' - ly NaN or -inf: it stays; +inf: it moves -- whatever the draw.
    Returns what the run exercised: counts of (stayed at NaN, stayed at -inf, left -inf, refused a non-finite proposal)."""
    nsteps, n, d1 = rows.shape
    prev = start
    seen = dict(nan_stays=0, minf_stays=0, minf_leaves=0, finite_refuses=0)
    for t in range(nsteps):
        now = rows[t]
        xp = propose(t, prev[:, :d1 - 1])
        lyp = loglike(xp)
        prop = row_of_start(xp, lyp)
        ly = prev[:, d1 - 1]
        with np.errstate(invalid="ignore", over="ignore"):
            diff = (lyp.astype(np.float32) - ly.astype(np.float32)).astype(np.float32)
        same_prev = np.all((bits(now) == bits(prev)) | (np.isnan(now) & np.isnan(prev)), 1)
        same_prop = np.all((bits(now) == bits(prop)) | (np.isnan(now) & np.isnan(prop)), 1)
        bad = np.flatnonzero(~(same_prev | same_prop))
        assert bad.size == 0, "%s step %d: chain %d holds neither its last row nor its proposal" % (label, t, bad[0])
        moved = same_prop & ~same_prev
        if mask is not None:
            took = mask[t].astype(bool)
            bad = np.flatnonzero((took & ~same_prop) | (~took & ~same_prev))
            assert bad.size == 0, "%s step %d: the mask of chain %d contradicts its row" % (label, t, bad[0])
            moved = took
        must_stay = np.isnan(diff) | (diff == -np.inf)
        must_move = diff == np.inf
        bad = np.flatnonzero(must_stay & (moved | ~same_prev))
        assert bad.size == 0, "%s step %d: chain %d moved from ly = %r to ly' = %r" % (label, t, bad[0], ly[bad[0]], lyp[bad[0]])
        bad = np.flatnonzero(must_move & ~(same_prop if mask is None else moved))
        assert bad.size == 0, "%s step %d: chain %d at ly = %r refused ly' = %r" % (label, t, bad[0], ly[bad[0]], lyp[bad[0]])
        seen["nan_stays"] += int(np.sum(np.isnan(ly)))
        seen["minf_stays"] += int(np.sum((ly == -np.inf) & must_stay))
        seen["minf_leaves"] += int(np.sum((ly == -np.inf) & must_move))
        seen["finite_refuses"] += int(np.sum(np.isfinite(ly) & must_stay))
        # the third rule as the rows alone show it: a finite ly never becomes anything else
        bad = np.flatnonzero(np.isfinite(ly) & ~np.isfinite(now[:, d1 - 1]))
        assert bad.size == 0, "%s step %d: chain %d went from a finite ly to %r" % (label, t, bad[0], now[bad[0], d1 - 1])
        prev = now
    return seen


# ------------------------------------------------------------------------------------------------------------------
# the draw u24 = 0: log1(u24) = -inf there, so a chain takes ANY proposal with ly' - ly > -inf, however deep the drop
# ------------------------------------------------------------------------------------------------------------------
U0_SEED, U0_CHAIN = 83073, 59   # found by search: the acceptance draw of (seed, step 0, chain 59) is 0x00000061 >> 8 = 0


def u0_draw_is_zero():
    w = R.philox4x32(0, U0_CHAIN, 0, 0, U0_SEED, R.ST_ACCEPT)[0]
    return int(w) >> 8 == 0 and float(R.accept_u(U0_SEED, 0, np.array([U0_CHAIN]))[0]) == 0.0


# ------------------------------------------------------------------------------------------------------------------
# a box prior: log L = -inf where any |x_k| > 0.6, a Gaussian inside.  Three statements of the same float32 operations
# in the same order (squares added left to right from 0 within blocks of four parameters, the block sums added in turn;
# d = 8: two blocks), so that the numpy functor and both source forms return the same bits.
# ------------------------------------------------------------------------------------------------------------------
BOX_D, BOX_PAR = 8, np.array([4.0, 0.6], np.float32)   # par = (1 / sigma^2, the half-width of the box)


def box_numpy(x):
    x = np.asarray(x, np.float32)
    w, edge = BOX_PAR
    tot = None
    for q in range(0, x.shape[1], 4):
        acc = np.zeros(x.shape[0], np.float32)
        for k in range(q, min(q + 4, x.shape[1])):
            acc = acc + x[:, k] * x[:, k]
        tot = acc if tot is None else tot + acc
    with np.errstate(invalid="ignore"):
        out = np.any(np.abs(x) > edge, 1)
    tot = np.where(out, np.float32(np.inf), tot).astype(np.float32)
    return ((np.float32(-0.5) * w) * tot).astype(np.float32)


BOX_BLOCK_FORM = """
#define MCX_USER_BLOCK_FORM
__device__ float mcx_user_block(const float xb[4], int nv, int k0, int d, const float *par)
{
  float acc = 0.0f;
  bool out = false;
  for (int k = 0; k < nv; ++k) {
    acc = acc + xb[k] * xb[k];
    out = out || __builtin_fabsf(xb[k]) > par[1];
  }
  return out ? __builtin_inff() : acc;
}
#define MCX_USER_FINISH
__device__ float mcx_user_finish(float sum, int d, const float *par) { return (-0.5f * par[0]) * sum; }
"""

BOX_WHOLE_FORM = """
__device__ float mcx_user_loglike(const float *x, int d, const float *par)
{
  float tot = 0.0f;
  bool out = false;
  for (int q = 0; q < d; q += 4) {
    float acc = 0.0f;
    for (int k = q; k < d && k < q + 4; ++k) {
      acc = acc + x[k] * x[k];
      out = out || __builtin_fabsf(x[k]) > par[1];
    }
    tot = q == 0 ? acc : tot + acc;
  }
  return (-0.5f * par[0]) * (out ? __builtin_inff() : tot);
}
"""

BOX_N, BOX_NBURN, BOX_NSAMP = 128, 110, 100
BOX_OUTSIDE = (3, 70)


def box_pinit():
    """0.5 sin(...) lies inside the box; chain 3 starts just outside in one coordinate, chain 70 outside in all"""
    p = default_pinit(BOX_D, BOX_N)
    p[BOX_OUTSIDE[0], 0] = np.float32(0.61)
    p[BOX_OUTSIDE[1], :] = np.float32(0.9)
    return p


# ------------------------------------------------------------------------------------------------------------------
# Murray steps with non-finite likelihoods.  Before the loop of a Murray call was bounded some of
# these never returned: the oracle runs every one of them in a process of its own under a time limit, and the GPU tests
# run a case only after the oracle has ended on it.
# ------------------------------------------------------------------------------------------------------------------
# name: (d, chains per shard, shards, nburn, nsamp, pl, {chain: value of every coordinate, or (coordinate, value)}, likelihood)
MURRAY_JOBS = {
    # four chains at ly = -inf with finite coordinates: Murray proposals rescue them
    "minf_16d": (16, 128, 1, 60, 100, 0.8, {5: 1e12, 6: 1e12, 64: 3e38, 127: -1e15}, "rosenbrock1"),
    "minf_36d": (36, 100, 1, 60, 100, 0.8, {5: 1e12, 6: 1e12, 64: 3e38, 99: -1e15}, "rosenbrock1"),   # np > 32: the chain vector in memory
    # NaN moments: the call must fail at the first Murray step
    "nan_16d": (16, 128, 1, 60, 40, 0.8, {37: (3, np.nan)}, "rosenbrock1"),
    "inf_16d": (16, 128, 1, 60, 40, 0.8, {37: (0, np.inf)}, "rosenbrock1"),   # delta = inf: the Welford sum is inf - inf
    "nan_sharded": (16, 64, 2, 60, 40, 0.8, {64 + 9: (3, np.nan)}, "rosenbrock1"),   # global chain 73: shard 1's chain 9
    # nothing poisoned: for the lowered cap
    "healthy_2d": (2, 200, 1, 110, 100, 0.8, {}, "rosenbrock1"),   # (2-D: Murray calls of tens of passes)
    "box_pl08": (BOX_D, BOX_N, 1, BOX_NBURN, BOX_NSAMP, 0.8, None, "box"),
    "box_pl1": (BOX_D, BOX_N, 1, BOX_NBURN, BOX_NSAMP, 1.0, None, "box"),   # (no Murray step: for the comparison with the engine)
}


def murray_pinit(name):
    d, n, nshards, nburn, nsamp, pl, poison, lik = MURRAY_JOBS[name]
    if lik == "box":
        return box_pinit()
    p = default_pinit(d, n * nshards)
    for j, v in poison.items():
        if isinstance(v, tuple):
            p[j, v[0]] = np.float32(v[1])
        else:
            p[j, :] = np.float32(v)
    return p


def first_murray_step(name, seed=SEED):
    """(isamp, t) of the run's first Murray step: the first main-loop step at or after SYNCSTEP = 10 whose coin exceeds pl"""
    d, n, nshards, nburn, nsamp, pl, poison, lik = MURRAY_JOBS[name]
    for isamp in range(nsamp):
        if R.is_remote(seed, nburn + isamp, isamp, 10, pl):
            return isamp, nburn + isamp
    return None


def run_oracle_job(name, max_passes=0):
    """the job on the oracle, in this process: dict of arrays (per shard where there are several: leading axis)"""
    import oracle_lib as O
    d, n, nshards, nburn, nsamp, pl, poison, lik = MURRAY_JOBS[name]
    pinit = murray_pinit(name)
    if lik == "box":
        def tramp(ctx, npset, x, y):
            np.ctypeslib.as_array(y, shape=(npset,))[:] = box_numpy(np.ctypeslib.as_array(x, shape=(npset, d)))
            return 0
        cb = O.HOSTFN(tramp)
        vo, keep = O.make_vlfunc(O.VL_HOST, d, fn=cb)
    else:
        vo, keep = O.make_vlfunc(O.VL_ROSENBROCK1, d)
    engs = [O.Engine(d, n, nshards=nshards, shard=s, pl=pl, threads=4) for s in range(nshards)]
    for e in engs:
        e.set_murray_max_passes(max_passes)
    status, error = 0, ""
    try:
        if nshards == 1:
            engs[0].run(nsamp, nburn, pinit, vo)
        else:
            O.run_all(engs, nsamp, nburn, [pinit[s * n:(s + 1) * n] for s in range(nshards)], vo)
    except O.OracleError as ex:
        status, error = ex.status, "|".join(e.last_error for e in engs)
    out = dict(status=status, error=error,
               remote_steps=[e.remote_steps for e in engs], remote_passes=[e.remote_passes for e in engs],
               remote_passes_max=[e.remote_passes_max for e in engs],
               naccept_burn=[e.naccept_burn for e in engs], naccept_main=[e.naccept_main for e in engs])
    for what in ("state", "loglike", "mean", "var", "musigall", "samples", "accept_mask", "accept_counts", "tuner_trace"):
        out[what] = np.stack([getattr(e, what) for e in engs])
    for e in engs:
        e.close()
    return out


def oracle_job_in_child(name, max_passes=0, timeout=120):
    """the same in a child process under a time limit (subprocess.TimeoutExpired: the oracle did not end)"""
    import os
    import subprocess
    import sys
    import tempfile
    here = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "job.npz")
        code = "import sys; sys.path.insert(0, %r); import numpy as np, nonfinite_cases as N; np.savez(%r, **N.run_oracle_job(%r, %d))" % (
            here, path, name, max_passes)
        subprocess.run([sys.executable, "-c", code], check=True, timeout=timeout, cwd=here)
        with np.load(path) as z:
            out = {k: z[k] for k in z.files}
    out["status"], out["error"] = int(out["status"]), str(out["error"])
    return out
