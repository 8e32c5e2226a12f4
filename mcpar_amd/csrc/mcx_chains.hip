// mcx_chains.hip -- the per-chain table of a sample store, the rule that names the chains to keep and the store of chosen
// chains: mcx_*_chain_table, mcx_chains_keep, mcx_*_select_chains.  The one analysis whose unit is the
// chain.
//
// The table is two sweeps, each walking all T steps of a chain in one lane as k_sum_moments does:
//   k_chain_series   one lane per (chain, column) series on the tiles of k_sum_moments (up to 16 adjacent columns x 16 chains,
//                    log L a tile set of its own): pass 1 the sum -> mean, pass 2 the centred sums c_i^2 and c_i c_{i+1}, fp64,
//                    in step order -> cols[chain][column] = (mean, sd, rho1)
//   k_chain_rows     G = min(64, pow2ceil(ncol)) lanes per chain, lane j holding columns j, j + G, ... of the previous row in
//                    V = ceil(ncol / G) <= 5 registers as u32; per step the lanes' "my share changed" bits are one ballot, and
//                    the group's bits of it say whether the row moved.  The lane that holds log L (lane np % G, register
//                    V - 1) keeps the counters and the log L maximum and writes the chain's four words
// The store of chosen chains is one gather sweep, k_chain_select: one lane per 16 bytes of x' (np % 4 == 0 and aligned bases)
// or per float, then one per value of log L; a row's lanes are adjacent, so loads and stores are coalesced along the row.
// No atomics of any kind and no LDS: every number has one writer and a fixed order, the bytes do not depend on scheduling.
#include "mcx_store.hpp"

#include "mcx_chains_host.hpp"

#include <chrono>
#include <cstring>
#include <memory>

namespace {

constexpr int CHAIN_WORDS = 4;  // u64 words of a chain from k_chain_rows: moves, longest_stay, ll_max bits | step << 32, flags

// ---- the series sweep.  grid = nbc * ntiles of the tile set; out[chain][ncol][3]
__global__ void __launch_bounds__(SB) k_chain_series(TileSet t, int nc, int ncol, int64_t T, double *out)
{
  const int tile = blockIdx.x % t.ntiles, bc = blockIdx.x / t.ntiles;
  const Lane l = lane_of(t, tile, bc, nc);
  if (!l.ok) return;
  const float *p = t.src + (size_t)l.chain * t.cs + l.lcol;
  double s = 0.0;
#pragma unroll 8
  for (int64_t i = 0; i < T; ++i) s += (double)p[i * t.rs];
  const double mean = s / (double)T;
  double cp = (double)p[0] - mean, ss = cp * cp, sc = 0.0;
#pragma unroll 8
  for (int64_t i = 1; i < T; ++i) {
    const double c = (double)p[i * t.rs] - mean;
    ss += c * c;
    sc += cp * c;
    cp = c;
  }
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const bool fin = isfinite(s);  // (finite floats cannot overflow an fp64 sum: an inf or NaN in the series, and only that)
  double *o = out + ((size_t)l.chain * ncol + (t.col0 + l.lcol)) * 3;
  o[0] = fin ? mean : qnan;
  o[1] = fin ? sqrt(ss / (double)(T - 1)) : qnan;  // (T = 1: 0 / 0)
  o[2] = fin && T >= 2 && ss > 0.0 ? sc / ss : qnan;
}

// ---- the row sweep
struct ChainRowArgs {
  const float *x, *ly;      // x[T][nc][np], ly[T][nc]
  unsigned long long *out;  // [nc][CHAIN_WORDS]
  int nc, np, lg;           // G = 1 << lg lanes per chain
  int64_t T;
};

__device__ __forceinline__ bool chain_nonfinite_bits(uint32_t b) { return (b & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ bool chain_nan_bits(uint32_t b) { return (b & 0x7fffffffu) > 0x7f800000u; }
// ascending in float order: -inf < finite < +inf, -0 before +0
__device__ __forceinline__ uint32_t chain_order_key(uint32_t b) { return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u); }

// grid = ceil(nc / (SB >> lg)).  Every lane of a wavefront walks all T steps (no early return: the ballots are the
// wavefront's); a lane without a chain or without a column contributes "unchanged" and "finite".
template <int V> __global__ void __launch_bounds__(SB) k_chain_rows(const ChainRowArgs a)
{
  const int G = 1 << a.lg, tid = (int)threadIdx.x, j = tid & (G - 1), np = a.np;
  const int chain = (int)blockIdx.x * (SB >> a.lg) + (tid >> a.lg);
  const bool ok = chain < a.nc;
  const int first = (tid & 63) & ~(G - 1);  // the group's first lane in its wavefront
  const unsigned long long gmask = (G == 64 ? ~0ull : (1ull << G) - 1ull) << first;
  const float *p[V];
  size_t rs[V];
  bool has[V];
  uint32_t prev[V];
  bool nf = false;
#pragma unroll
  for (int r = 0; r < V; ++r) {
    const int c = j + r * G;
    has[r] = ok && c <= np;
    const bool par = c < np;
    p[r] = has[r] ? (par ? a.x + (size_t)chain * np + c : a.ly + chain) : a.x;
    rs[r] = par ? (size_t)a.nc * np : (size_t)a.nc;
    prev[r] = has[r] ? __float_as_uint(p[r][0]) : 0u;
    nf = nf || chain_nonfinite_bits(prev[r]);
  }
  // what the lane of log L keeps (the others compute the same from a register that is not log L and write nothing)
  const bool leader = ok && j == (np & (G - 1));
  long long moves = 0, run = 1, longest = 1;
  uint32_t best = prev[V - 1], best_key = chain_order_key(best);
  int best_step = 0;
  bool llnan = chain_nan_bits(best);  // (an inf alone leaves ll_max what float order says)
  for (int64_t t = 1; t < a.T; ++t) {
    bool ch = false;
#pragma unroll
    for (int r = 0; r < V; ++r) {
      const uint32_t cur = has[r] ? __float_as_uint(p[r][(size_t)t * rs[r]]) : 0u;
      ch = ch || cur != prev[r];
      nf = nf || chain_nonfinite_bits(cur);
      prev[r] = cur;
    }
    const bool moved = (__ballot(ch) & gmask) != 0ull;
    if (moved) {
      ++moves;
      run = 1;
    } else if (++run > longest) longest = run;
    const uint32_t key = chain_order_key(prev[V - 1]);
    llnan = llnan || chain_nan_bits(prev[V - 1]);
    if (key > best_key) {
      best_key = key;
      best = prev[V - 1];
      best_step = (int)t;
    }
  }
  const bool nfany = (__ballot(nf) & gmask) != 0ull;
  if (leader) {
    unsigned long long *o = a.out + (size_t)chain * CHAIN_WORDS;
    o[0] = (unsigned long long)moves;
    o[1] = (unsigned long long)longest;
    o[2] = llnan ? (0x7fc00000ull | (0xffffffffull << 32)) : ((unsigned long long)best | ((unsigned long long)(uint32_t)best_step << 32));
    o[3] = nfany ? (unsigned long long)MCX_SUMMARY_NONFINITE : 0ull;
  }
}

// ---- the gather sweep
struct ChainSelectArgs {
  const float *x, *ly;  // x[T][nc][np], ly[T][nc]
  float *xo, *lyo;      // x'[T][nsel][np], ly'[T][nsel]
  const uint32_t *sel;  // [nsel], each < nc
  uint64_t nx, nrows;   // items of x' (quads or floats), rows T * nsel
  int nc, np, nsel, ipr;  // ipr: items per row, np / 4 or np
};

// grid = ceil((nx + nrows) / SB): item i < nx is quad or float i of x', item nx + r the log L of row r
template <bool VEC4> __global__ void __launch_bounds__(SB) k_chain_select(const ChainSelectArgs a)
{
  const uint64_t i = (uint64_t)blockIdx.x * SB + threadIdx.x;
  if (i >= a.nx + a.nrows) return;
  const bool isx = i < a.nx;
  const uint64_t row = isx ? i / (uint64_t)a.ipr : i - a.nx;
  const uint64_t t = row / (uint64_t)a.nsel;
  const uint32_t k = (uint32_t)(row - t * (uint64_t)a.nsel);
  const uint64_t src = t * (uint64_t)a.nc + a.sel[k];
  if (!isx) {
    a.lyo[row] = a.ly[src];
    return;
  }
  const uint64_t q = i - row * (uint64_t)a.ipr;
  if (VEC4) reinterpret_cast<float4 *>(a.xo)[i] = reinterpret_cast<const float4 *>(a.x + src * (uint64_t)a.np)[q];
  else a.xo[i] = a.x[src * (uint64_t)a.np + q];
}

// ---- launch geometry: what the launches below use and mcx_debug_chains_geometry reports (rows_geometry: the row sweep's
// grouping, in mcx_summary_kernels.hpp, which the step table's row sweep shares)
struct SelectGeometry {
  bool vec4;  // when the bases are 16-byte aligned
  int ipr;
  uint64_t nx, nrows, nwg;
};
SelectGeometry select_geometry(int np, int64_t T, int nsel, bool aligned)
{
  SelectGeometry g;
  g.vec4 = aligned && np % 4 == 0;
  g.ipr = g.vec4 ? np / 4 : np;
  g.nrows = (uint64_t)T * (uint64_t)nsel;
  g.nx = g.nrows * (uint64_t)g.ipr;
  g.nwg = (g.nx + g.nrows + SB - 1) / SB;
  return g;
}

int launch_rows(hipStream_t st, const RowsGeometry &g, const ChainRowArgs &a)
{
  switch (g.V) {
  case 1: hipLaunchKernelGGL(k_chain_rows<1>, dim3(g.nwg), dim3(SB), 0, st, a); break;
  case 2: hipLaunchKernelGGL(k_chain_rows<2>, dim3(g.nwg), dim3(SB), 0, st, a); break;
  case 3: hipLaunchKernelGGL(k_chain_rows<3>, dim3(g.nwg), dim3(SB), 0, st, a); break;
  case 4: hipLaunchKernelGGL(k_chain_rows<4>, dim3(g.nwg), dim3(SB), 0, st, a); break;
  case 5: hipLaunchKernelGGL(k_chain_rows<5>, dim3(g.nwg), dim3(SB), 0, st, a); break;
  default: return fail(MCX_ERR_INVALID, "np = %d: a chain table takes rows of 1 to 256 parameters", a.np);
  }
  HIPCHK(hipGetLastError());
  return MCX_OK;
}

// what a table call refuses before a device is touched
int table_args(int nsteps, const mcx_chain_col *cols, const mcx_chain_row *chains)
{
  if (!cols || !chains) return fail(MCX_ERR_INVALID, "cols or chains is NULL");
  if (nsteps < 1) return fail(MCX_ERR_INVALID, "nsteps = %d: a range of at least one step", nsteps);
  return MCX_OK;
}

// ms (mcx_debug_chain_table_times, else NULL): ms[0] the series sweep, ms[1] the row sweep (HIP events), ms[2] the whole call
// (wall clock)
int chains_span(hipStream_t st, Bufs B, const StoreView &v, mcx_chain_col *cols, mcx_chain_row *chains, double *ms = nullptr)
{
  using clk = std::chrono::steady_clock;
  const clk::time_point t_call = clk::now();
  StageTimer tm{st, ms, 3, {}};
  const int nc = v.nc, np = v.np, ncol = v.ncol;
  if (np < 1 || np > 256) return fail(MCX_ERR_INVALID, "np = %d: a chain table takes rows of 1 to 256 parameters", np);
  const RowsGeometry rg = rows_geometry(np, nc);
  const size_t nd = (size_t)nc * ncol * 3, nh = (size_t)nc * CHAIN_WORDS;
  MCXCHK(B.d->alloc(nd));
  MCXCHK(B.h->alloc(nh));
  ChainRowArgs a{v.x, v.ly, B.h->p, nc, np, rg.lg, v.T};
  std::vector<unsigned long long> words(nh);
  static_assert(sizeof(mcx_chain_col) == 3 * sizeof(double), "cols[nc][ncol] is the device's out[nc][ncol][3]");
  auto run = [&]() -> int {
    MCXCHK(tm.run(0, [&]() -> int {
      for (const TileSet *t : {&v.tx, &v.tl}) {
        hipLaunchKernelGGL(k_chain_series, dim3((unsigned)(t->nbc * t->ntiles)), dim3(SB), 0, st, *t, nc, ncol, v.T, B.d->p);
        HIPCHK(hipGetLastError());
      }
      return MCX_OK;
    }));
    MCXCHK(tm.run(1, [&]() -> int { return launch_rows(st, rg, a); }));
    HIPCHK(hipMemcpyAsync(cols, B.d->p, nd * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(words.data(), B.h->p, nh * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MCX_OK;
  };
  const int rc = run();
  if (rc != MCX_OK) (void)hipStreamSynchronize(st);  // (cols and words are the copies' until here)
  MCXCHK(rc);
  for (int k = 0; k < nc; ++k) {
    const unsigned long long *w = words.data() + (size_t)k * CHAIN_WORDS;
    const uint32_t bits = (uint32_t)w[2];
    mcx_chain_row &r = chains[k];
    r.moves = (long long)w[0];
    r.longest_stay = (long long)w[1];
    memcpy(&r.ll_max, &bits, sizeof bits);
    r.ll_max_step = (int)(uint32_t)(w[2] >> 32);
    r.flags = (int)w[3];
  }
  MCXCHK(tm.collect());
  if (ms) ms[2] = std::chrono::duration<double, std::milli>(clk::now() - t_call).count();
  return MCX_OK;
}

// what a selection refuses before a device is touched: nothing is allocated for a list it does not take
int select_args(int nsteps, int nc, const int *chains, int nsel, mcx_store **out)
{
  if (nsel < 1) return fail(MCX_ERR_INVALID, "nsel = %d: a store of at least one chain", nsel);
  if (!chains || !out) return fail(MCX_ERR_INVALID, "chains or out is NULL");
  if (nsteps < 1) return fail(MCX_ERR_INVALID, "nsteps = %d: a range of at least one step", nsteps);
  for (int k = 0; k < nsel; ++k)
    if (chains[k] < 0 || chains[k] >= nc)
      return fail(MCX_ERR_INVALID, "chains[%d] = %d is not a chain of the source (0 to %d)", k, chains[k], nc - 1);
  return MCX_OK;
}

int select_span(hipStream_t st, Bufs B, const StoreSpan &s, const int *chains, int nsel, mcx_store **out)
{
  const int np = s.np;
  if (np < 1 || np > 256) return fail(MCX_ERR_INVALID, "np = %d: a selection takes rows of 1 to 256 parameters", np);
  std::unique_ptr<mcx_store> o(new mcx_store);
  HIPCHK(hipGetDevice(&o->device));
  o->nc = nsel; o->nout = np; o->T = (int)s.T;
  const size_t n = o->rows();
  MCXCHK(o->st.ensure(hipStreamNonBlocking));
  MCXCHK(o->x.alloc(n * np));
  MCXCHK(o->ly.alloc(n));
  MCXCHK(B.u->alloc((size_t)nsel));
  const bool aligned = (((unsigned long)s.x | (unsigned long)o->x.p) & 15ul) == 0;
  const SelectGeometry g = select_geometry(np, s.T, nsel, aligned);
  if (g.nwg > 0x7fffffffull)
    return fail(MCX_ERR_UNSUPPORTED, "select: %llu rows of %d parameters are more workgroups than a grid holds",
                (unsigned long long)g.nrows, np);
  const std::vector<uint32_t> sel(chains, chains + nsel);  // (checked: each in [0, nc))
  ChainSelectArgs a{s.x, s.ly, o->x.p, o->ly.p, B.u->p, g.nx, g.nrows, s.nc, np, nsel, g.ipr};
  auto run = [&]() -> int {
    HIPCHK(hipMemcpyAsync(B.u->p, sel.data(), sel.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (g.vec4) hipLaunchKernelGGL(k_chain_select<true>, dim3((unsigned)g.nwg), dim3(SB), 0, st, a);
    else hipLaunchKernelGGL(k_chain_select<false>, dim3((unsigned)g.nwg), dim3(SB), 0, st, a);
    HIPCHK(hipGetLastError());
    return MCX_OK;
  };
  const int rc = run();
  const hipError_t es = hipStreamSynchronize(st);  // (before sel, or the new store, may go)
  MCXCHK(rc);
  HIPCHK(es);
  *out = o.release();  // (the unique_ptr's: the store is the caller's now)
  return MCX_OK;
}

}  // namespace

extern "C" int mcx_samples_chain_table(mcx_engine *e, int first_step, int nsteps, mcx_chain_col *cols, mcx_chain_row *chains)
{
  return on_store(
      e, first_step, nsteps, [&] { return table_args(nsteps, cols, chains); },
      [&](hipStream_t st, Bufs B, const StoreView &v) { return chains_span(st, B, v, cols, chains); });
}

// mcx_samples_chain_table with its sweeps timed, for tools/chains_bench.py; the table is let go
extern "C" int mcx_debug_chain_table_times(mcx_engine *e, int first_step, int nsteps, double *ms)
{
  std::vector<mcx_chain_col> cols;
  std::vector<mcx_chain_row> chains;
  return on_store(
      e, first_step, nsteps,
      [&] {
        if (!ms) return fail(MCX_ERR_INVALID, "ms is NULL");
        chains.resize((size_t)e->nchain);
        cols.resize(chains.size() * ((size_t)e->nparam + 1));
        return table_args(nsteps, cols.data(), chains.data());
      },
      [&](hipStream_t st, Bufs B, const StoreView &v) { return chains_span(st, B, v, cols.data(), chains.data(), ms); });
}

extern "C" int mcx_rows_chain_table(const float *rows, int nsteps, int nc, int np, mcx_chain_col *cols, mcx_chain_row *chains)
{
  MCXCHK(table_args(nsteps, cols, chains));
  return on_rows(rows, nsteps, nc, np,
                 [&](hipStream_t st, Bufs B, const StoreView &v) { return chains_span(st, B, v, cols, chains); });
}

extern "C" int mcx_store_chain_table(mcx_store *s, mcx_chain_col *cols, mcx_chain_row *chains)
{
  if (!s) return fail(MCX_ERR_INVALID, "the store s is NULL");
  MCXCHK(table_args(s->T, cols, chains));
  HIPCHK(hipSetDevice(s->device));
  return chains_span(s->st, s->bufs(), StoreView(s->span()), cols, chains);
}

// host only
extern "C" int mcx_chains_keep(int nc, int ncol, const mcx_chain_col *cols, const mcx_chain_row *chains, const mcx_chain_rule *rule,
                               int *reasons, double *centre, int *nkept)
{
  char msg[160];
  const int rc = mcx_chains_host::keep(nc, ncol, cols, chains, rule, reasons, centre, nkept, msg, sizeof msg);
  return rc == MCX_OK ? MCX_OK : fail(rc, "%s", msg);
}

extern "C" int mcx_samples_select_chains(mcx_engine *e, int first_step, int nsteps, const int *chains, int nsel, mcx_store **out)
{
  return on_store(
      e, first_step, nsteps, [&] { return select_args(nsteps, e->nchain, chains, nsel, out); },
      [&](hipStream_t st, Bufs B, const StoreView &v) { return select_span(st, B, v, chains, nsel, out); });
}

extern "C" int mcx_rows_select_chains(const float *rows, int nsteps, int nc, int np, const int *chains, int nsel, mcx_store **out)
{
  MCXCHK(select_args(nsteps, nc, chains, nsel, out));
  return on_rows(rows, nsteps, nc, np,
                 [&](hipStream_t st, Bufs B, const StoreView &v) { return select_span(st, B, v, chains, nsel, out); });
}

extern "C" int mcx_store_select_chains(mcx_store *s, const int *chains, int nsel, mcx_store **out)
{
  if (!s) return fail(MCX_ERR_INVALID, "the store s is NULL");
  MCXCHK(select_args(s->T, s->nc, chains, nsel, out));
  HIPCHK(hipSetDevice(s->device));
  return select_span(s->st, s->bufs(), s->span(), chains, nsel, out);
}

// host only
extern "C" int mcx_debug_chains_geometry(int np, int nsteps, int nc, int nsel, mcx_chains_geometry *g)
{
  if (!g) return fail(MCX_ERR_INVALID, "g is NULL");
  if (np < 1 || np > 256) return fail(MCX_ERR_INVALID, "np = %d: 1 to 256 parameters", np);
  if (nsteps < 1 || nc < 1 || nsel < 1)
    return fail(MCX_ERR_INVALID, "nsteps = %d, nc = %d, nsel = %d: at least one step of one chain, one chain chosen", nsteps, nc, nsel);
  const TileSet tx = tiles_x(nullptr, nc, np), tl = tiles_l(nullptr, nc, np);
  const RowsGeometry r = rows_geometry(np, nc);
  const SelectGeometry s = select_geometry(np, nsteps, nsel, true);
  g->block = SB;
  g->lds_bytes = 0;
  g->series_tile_cols = tx.ct;
  g->series_tile_chains = tx.cg;
  g->series_col_tiles = tx.ntiles;
  g->series_workgroups = (long long)tx.nbc * tx.ntiles;
  g->series_ll_workgroups = (long long)tl.nbc * tl.ntiles;
  g->rows_lanes_per_chain = r.G;
  g->rows_values_per_lane = r.V;
  g->rows_chains_per_workgroup = r.cpw;
  g->rows_workgroups = r.nwg;
  g->select_vec4 = s.vec4 ? 1 : 0;
  g->select_items = (long long)(s.nx + s.nrows);
  g->select_workgroups = (long long)s.nwg;
  return MCX_OK;
}
