// mcx_clip.hip -- mcx_samples_clip / mcx_rows_clip / mcx_store_clip and the row set they make (the
// reference's mcparam.clip.tails, src/anly/mcpar-analysis.R:60-78): every row that lies in the tail of any column is dropped,
// jointly, and the kept rows are compacted on the device in source order.
//
// One call:
//   1. summary_thresholds (mcx_summary.hip)   the (qlo, qhi) quantiles of every column, where some column takes a default
//   2. mcx_debug_clip_thresholds              host (mcx_clip_host.hpp): the quantiles and the spec -> lo[ncol], hi[ncol]
//   3. k_clip_mark      a workgroup stages R consecutive rows in LDS (section 12's tile copy), lane r < R tests its row:
//                       per column the wavefront's ballots feed two LDS counters (-> one integer atomic per non-zero counter
//                       per workgroup), the keep ballot is the wavefront's mask word, the kept count is cnt[wg]
//   4. k_clip_scan      cnt -> exclusive u64 offsets, two levels of 256, a fixed order; the total is K
//   5. k_clip_scatter   a workgroup stages its rows again, turns its mask words into the list of its kept rows in LDS and
//                       stores them as one contiguous piece of x', with ly' and the source row indices
// Only integers are added, every kept row has one position: the bytes do not depend on scheduling.  No float atomics, no
// waits between workgroups.
#include "mcx_derive.hpp"
#include "mcx_store.hpp"

#include "mcx_clip_host.hpp"

#include <chrono>
#include <limits>

struct mcx_rowset {
  int device = 0, np = 0;
  long long K = 0, N = 0;  // kept rows, rows of the source
  DevBuf<float> x, ly;     // x'[K][np], ly'[K]
  DevBuf<long long> idx;   // [K]: the source row of every kept row, ascending
  DevStream st;
  StoreSpan span() const { return StoreSpan{x.p, ly.p, 1, np, (int64_t)K}; }  // (a gather does not care about chains)
  ~mcx_rowset()
  {
    if (st) (void)hipStreamSynchronize(st);  // (before the members go)
  }
};

namespace {

constexpr int CLIP_FAN = DERIVE_BLOCK;  // counts per scan block, and scan blocks per step of the top level

struct ClipArgs {
  const float *x, *ly;             // x[N][np], ly[N]
  const double *thr;               // lo[ncol], then hi[ncol]
  unsigned long long *counts;      // [ncol][2]: nbelow, nabove
  unsigned long long *mask;        // [nwg][wpw]: bit l of word w = row w * 64 + l of the workgroup is kept
  uint32_t *cnt;                   // [nwg]: kept rows of the workgroup
  const unsigned long long *offs;  // [nwg]: kept rows of the workgroups before it (k_clip_scatter)
  float *xo, *lyo;                 // x'[K][np], ly'[K]
  long long *idx;                  // [K]
  uint64_t N;
  int np, R, wpw;  // R = derive_rows(np, 0) rows per workgroup (256 down to 32 at np = 256), wpw = ceil(R / 64) mask words
};

// the workgroup's rows into LDS: xs[r * (np | 1) + c], lys[r]; returns how many rows it has (the last workgroup: fewer)
__device__ __forceinline__ int clip_stage(const ClipArgs &a, float *xs, float *lys, uint64_t row0)
{
  const uint64_t left = a.N - row0;  // > 0: the grid is ceil(N / R)
  const int rows = left < (uint64_t)a.R ? (int)left : a.R, tid = (int)threadIdx.x;
  const float *gx = a.x + row0 * (uint64_t)a.np;
  if (tid < rows) lys[tid] = a.ly[row0 + tid];
  derive_tile_copy<true>(xs, a.np | 1, const_cast<float *>(gx), a.np, rows * a.np, ((unsigned long)gx & 15ul) == 0);
  return rows;
}

__global__ void __launch_bounds__(DERIVE_BLOCK) k_clip_mark(const ClipArgs a)
{
  extern __shared__ float clip_lds[];
  __shared__ unsigned tails[2 * (DERIVE_MAXW + 1)], wkept[DERIVE_BLOCK / 64];
  const int np = a.np, ncol = np + 1, sx = np | 1, tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float *xs = clip_lds, *lys = clip_lds + a.R * sx;
  for (int i = tid; i < 2 * ncol; i += DERIVE_BLOCK) tails[i] = 0u;
  const uint64_t row0 = (uint64_t)blockIdx.x * (uint64_t)a.R;
  const int rows = clip_stage(a, xs, lys, row0);
  __syncthreads();
  const bool mine = tid < rows;  // (a lane without a row contributes nothing)
  if (wave < a.wpw) {
    bool keep = mine;
    const float *xr = xs + (mine ? tid : 0) * sx;
    for (int c = 0; c < ncol; ++c) {
      const double lo = a.thr[c], hi = a.thr[ncol + c];  // (wave-uniform addresses)
      const double v = (double)(c < np ? xr[c] : lys[mine ? tid : 0]);
      const bool below = mine && !(v > lo), above = mine && !(v < hi);
      keep = keep && !below && !above;
      const unsigned long long bb = __ballot(below), ba = __ballot(above);
      if (lane == 0) {
        if (bb) atomicAdd(&tails[2 * c], (unsigned)__popcll(bb));
        if (ba) atomicAdd(&tails[2 * c + 1], (unsigned)__popcll(ba));
      }
    }
    const unsigned long long kb = __ballot(keep);
    if (lane == 0) {
      a.mask[(uint64_t)blockIdx.x * a.wpw + wave] = kb;
      wkept[wave] = (unsigned)__popcll(kb);
    }
  } else if (lane == 0) wkept[wave] = 0u;
  __syncthreads();
  if (tid == 0) {
    unsigned k = 0;
    for (int w = 0; w < DERIVE_BLOCK / 64; ++w) k += wkept[w];
    a.cnt[blockIdx.x] = k;
  }
  for (int i = tid; i < 2 * ncol; i += DERIVE_BLOCK)
    if (tails[i]) atomicAdd(&a.counts[i], (unsigned long long)tails[i]);
}

// inclusive scan of one value per thread over the workgroup, in s[DERIVE_BLOCK] (left holding the scan)
__device__ __forceinline__ unsigned long long clip_block_scan(unsigned long long v, unsigned long long *s)
{
  const int tid = (int)threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (int d = 1; d < DERIVE_BLOCK; d <<= 1) {
    const unsigned long long t = tid >= d ? s[tid - d] : 0ull;
    __syncthreads();
    s[tid] += t;
    __syncthreads();
  }
  return s[tid];
}

// cnt[nwg] -> offs[nwg], the kept rows before each workgroup, and boff[nb] = the total K.  nb = ceil(nwg / CLIP_FAN) blocks.
//   PHASE 0 (grid nb): bsum[b] = the sum of block b's counts
//   PHASE 1 (grid 1):  boff[b] = the sum of bsum before b, in steps of CLIP_FAN blocks with a carry; boff[nb] = the total
//   PHASE 2 (grid nb): offs[i] = boff[block of i] + the counts of its block before i
template <int PHASE>
__global__ void __launch_bounds__(DERIVE_BLOCK) k_clip_scan(const uint32_t *cnt, uint64_t nwg, uint64_t nb, unsigned long long *bsum,
                                                            unsigned long long *boff, unsigned long long *offs)
{
  __shared__ unsigned long long s[DERIVE_BLOCK];
  const int tid = (int)threadIdx.x;
  if (PHASE == 1) {
    unsigned long long carry = 0ull;
    for (uint64_t base = 0; base < nb; base += CLIP_FAN) {
      const uint64_t i = base + tid;
      const unsigned long long v = i < nb ? bsum[i] : 0ull;
      const unsigned long long incl = clip_block_scan(v, s);
      if (i < nb) boff[i] = carry + (incl - v);
      carry += s[DERIVE_BLOCK - 1];
      __syncthreads();  // (before the next step overwrites s)
    }
    if (tid == 0) boff[nb] = carry;
  } else {
    const uint64_t i = (uint64_t)blockIdx.x * CLIP_FAN + tid;
    const unsigned long long v = i < nwg ? (unsigned long long)cnt[i] : 0ull;
    const unsigned long long incl = clip_block_scan(v, s);
    if (PHASE == 0 && tid == DERIVE_BLOCK - 1) bsum[blockIdx.x] = incl;
    if (PHASE == 2 && i < nwg) offs[i] = boff[blockIdx.x] + (incl - v);
  }
}

__global__ void __launch_bounds__(DERIVE_BLOCK) k_clip_scatter(const ClipArgs a)
{
  extern __shared__ float clip_lds[];
  __shared__ int src[DERIVE_BLOCK];  // src[p] = the row of the tile that is the workgroup's p-th kept row
  const int kw = (int)a.cnt[blockIdx.x];
  if (kw == 0) return;
  const uint64_t off = a.offs[blockIdx.x];
  const int np = a.np, sx = np | 1, tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float *xs = clip_lds, *lys = clip_lds + a.R * sx;
  const uint64_t row0 = (uint64_t)blockIdx.x * (uint64_t)a.R;
  clip_stage(a, xs, lys, row0);
  if (wave < a.wpw) {
    const unsigned long long *mw = a.mask + (uint64_t)blockIdx.x * a.wpw;
    const unsigned long long m = mw[wave];
    int pos = __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += __popcll(mw[w]);
    if ((m >> lane) & 1ull) src[pos] = tid;  // (a bit is set for lanes with a row only)
  }
  __syncthreads();
  // the kw * np floats are one contiguous piece of x': element e is column e % np of kept row e / np
  const int total = kw * np;
  float *go = a.xo + off * (uint64_t)np;
  int head = 0;
  if (((unsigned long)go & 15ul) == 0) {
    const int nq = total >> 2, step = DERIVE_BLOCK * 4;
    const int dp = step / np, dc = step - dp * np;
    int e = tid * 4, p = e / np, c = e - p * np;
    for (int q = tid; q < nq; q += DERIVE_BLOCK) {
      float v[4];
      int pp = p, cc = c;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[k] = xs[src[pp] * sx + cc];
        if (++cc == np) { cc = 0; ++pp; }
      }
      reinterpret_cast<float4 *>(go)[q] = make_float4(v[0], v[1], v[2], v[3]);
      p += dp; c += dc;
      if (c >= np) { c -= np; ++p; }
    }
    head = nq << 2;
  }
  // the 4-byte path: everything when the piece is not 16-byte aligned, else the up to three floats behind the last quad
  {
    const int dp = DERIVE_BLOCK / np, dc = DERIVE_BLOCK - dp * np;
    int e = head + tid, p = e / np, c = e - p * np;
    for (; e < total; e += DERIVE_BLOCK) {
      go[e] = xs[src[p] * sx + c];
      p += dp; c += dc;
      if (c >= np) { c -= np; ++p; }
    }
  }
  if (tid < kw) {
    const int r = src[tid];
    a.lyo[off + tid] = lys[r];
    a.idx[off + tid] = (long long)(row0 + (uint64_t)r);
  }
}

int clip_fail(int rc, const char *msg) { return rc == MCX_OK ? MCX_OK : fail(rc, "%s", msg); }

// what can be refused before a device is touched
int clip_args(const mcx_clip_spec *spec, const mcx_col_clip *cols, const long long *nkept, int nsteps)
{
  char msg[160];
  MCXCHK(clip_fail(mcx_clip_host::spec_check(spec, cols, nkept, msg, sizeof msg), msg));
  if (nsteps < 1) return fail(MCX_ERR_INVALID, "nsteps = %d: a range of at least one step", nsteps);
  return MCX_OK;
}

// ms (mcx_debug_clip_times, else NULL): ms[0] the thresholds (wall clock), ms[1] mark, ms[2] scan, ms[3] scatter (HIP
// events), ms[4] the whole call (wall clock)
int clip_span(hipStream_t st, Bufs B, const StoreSpan &s, const mcx_clip_spec *spec, mcx_col_clip *cols, long long *nkept,
              mcx_rowset **out, double *ms = nullptr)
{
  using clk = std::chrono::steady_clock;
  auto since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
  const clk::time_point t_call = clk::now();
  StageTimer tm{st, ms, 5, {}};
  const int np = s.np, ncol = np + 1;
  const uint64_t N = (uint64_t)s.T * (uint64_t)s.nc;
  if (np < 1 || np > DERIVE_MAXW) return fail(MCX_ERR_INVALID, "np = %d: a clip takes rows of 1 to %d parameters", np, DERIVE_MAXW);
  ClipArgs a{};
  const ClipGeometry geo = clip_geometry(np, N);
  a.x = s.x; a.ly = s.ly; a.N = N; a.np = np; a.R = geo.R; a.wpw = geo.wpw;
  const uint64_t nwg = geo.nwg, nb = geo.nb;
  if (nwg > 0x7fffffffull)
    return fail(MCX_ERR_UNSUPPORTED, "clip: %llu rows in tiles of %d are more workgroups than a grid holds", (unsigned long long)N, a.R);

  // ---- 1, 2. the thresholds
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  std::vector<mcx_col_summary> sc(ncol);
  std::vector<double> q((size_t)ncol * 2, qnan), thr((size_t)ncol * 2);
  const bool quant = mcx_clip_host::needs_quantiles(spec, ncol);
  if (quant) {
    const double probs[2] = {spec->qlo, spec->qhi};
    MCXCHK(summary_thresholds(st, B, s, probs, 2, sc.data(), q.data()));
  }
  MCXCHK(mcx_debug_clip_thresholds(ncol, q.data(), spec, thr.data(), thr.data() + ncol));
  const double ms_thr = since(t_call);

  // ---- 3, 4. mark and scan.  u64 scratch: counts[ncol][2] | mask[nwg][wpw] | offs[nwg] | bsum[nb] | boff[nb + 1]
  const size_t o_mask = (size_t)ncol * 2, o_offs = o_mask + (size_t)nwg * a.wpw, o_bsum = o_offs + nwg, o_boff = o_bsum + nb;
  MCXCHK(B.d->alloc(thr.size()));
  MCXCHK(B.h->alloc(o_boff + nb + 1));
  MCXCHK(B.u->alloc(nwg));
  unsigned long long *H = B.h->p;
  a.thr = B.d->p; a.counts = H; a.mask = H + o_mask; a.cnt = B.u->p; a.offs = H + o_offs;
  const size_t lds = geo.lds_bytes;
  const RowMask rm{a.mask, a.cnt, H + o_offs};  // (offs | bsum | boff: rowset_scan's order)
  std::vector<unsigned long long> counts((size_t)ncol * 2);
  unsigned long long total = 0;
  auto run = [&]() -> int {
    HIPCHK(hipMemcpyAsync(B.d->p, thr.data(), thr.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(H, 0, counts.size() * sizeof(unsigned long long), st));
    MCXCHK(tm.run(1, [&]() -> int {
      hipLaunchKernelGGL(k_clip_mark, dim3((unsigned)nwg), dim3(DERIVE_BLOCK), lds, st, a);
      HIPCHK(hipGetLastError());
      return MCX_OK;
    }));
    MCXCHK(tm.run(2, [&]() -> int { return rowset_scan(st, rm, geo); }));
    HIPCHK(hipMemcpyAsync(counts.data(), H, counts.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&total, H + o_boff + nb, sizeof total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return MCX_OK;
  };
  int rc = run();
  if (rc != MCX_OK) (void)hipStreamSynchronize(st);  // (thr and the host words are the copies' until here)
  MCXCHK(rc);
  for (int c = 0; c < ncol; ++c) {
    cols[c].lo = thr[c];
    cols[c].hi = thr[ncol + c];
    cols[c].nbelow = (long long)counts[2 * c];
    cols[c].nabove = (long long)counts[2 * c + 1];
    cols[c].flags = quant ? sc[c].flags : 0;
  }
  *nkept = (long long)total;

  // ---- 5. the row set
  std::unique_ptr<mcx_rowset> o;
  if (out) {
    MCXCHK(rowset_new(np, total, N, o));
    if (total > 0) {
      rc = tm.run(3, [&]() -> int { return rowset_scatter(st, s, rm, geo, *o); });
      const hipError_t es = hipStreamSynchronize(st);  // (before the new row set may go)
      MCXCHK(rc);
      HIPCHK(es);
    }
  }
  MCXCHK(tm.collect());
  if (ms) {
    ms[0] = ms_thr;
    ms[4] = since(t_call);
  }
  if (out) *out = o.release();  // (the unique_ptr's: the row set is the caller's now)
  return MCX_OK;
}

int rowset_enter(const mcx_rowset *r)
{
  if (!r) return fail(MCX_ERR_INVALID, "the row set r is NULL");
  HIPCHK(hipSetDevice(r->device));
  return MCX_OK;
}

int rowset_range(const mcx_rowset *r, long long first_row, long long nrows)
{
  if (first_row < 0 || nrows < 0 || first_row > r->K || nrows > r->K - first_row)
    return fail(MCX_ERR_INVALID, "rows [%lld,%lld) not in the row set (%lld rows)", first_row, first_row + nrows, r->K);
  return MCX_OK;
}

}  // namespace

ClipGeometry clip_geometry(int np, uint64_t N)
{
  ClipGeometry g;
  g.R = derive_rows(np, 0);
  g.wpw = (g.R + 63) / 64;
  g.lds_bytes = (size_t)derive_lds_floats(np, 0, g.R) * sizeof(float);
  g.nwg = sweep_tiles(N, g.R);
  g.nb = (g.nwg + CLIP_FAN - 1) / CLIP_FAN;
  return g;
}

int rowset_scan(hipStream_t st, const RowMask &m, const ClipGeometry &g)
{
  const uint64_t nwg = g.nwg, nb = g.nb;
  unsigned long long *offs = m.scan, *bsum = offs + nwg, *boff = bsum + nb;
  hipLaunchKernelGGL(k_clip_scan<0>, dim3((unsigned)nb), dim3(DERIVE_BLOCK), 0, st, m.cnt, nwg, nb, bsum, boff, offs);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_clip_scan<1>, dim3(1), dim3(DERIVE_BLOCK), 0, st, m.cnt, nwg, nb, bsum, boff, offs);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_clip_scan<2>, dim3((unsigned)nb), dim3(DERIVE_BLOCK), 0, st, m.cnt, nwg, nb, bsum, boff, offs);
  HIPCHK(hipGetLastError());
  return MCX_OK;
}

int rowset_new(int np, unsigned long long total, uint64_t N, std::unique_ptr<mcx_rowset> &o)
{
  o.reset(new mcx_rowset);
  HIPCHK(hipGetDevice(&o->device));
  o->np = np; o->K = (long long)total; o->N = (long long)N;
  MCXCHK(o->st.ensure(hipStreamNonBlocking));
  MCXCHK(o->x.alloc((size_t)total * np));
  MCXCHK(o->ly.alloc((size_t)total));
  MCXCHK(o->idx.alloc((size_t)total));
  return MCX_OK;
}

int rowset_scatter(hipStream_t st, const StoreSpan &s, const RowMask &m, const ClipGeometry &g, mcx_rowset &o)
{
  ClipArgs a{};
  a.x = s.x; a.ly = s.ly; a.N = (uint64_t)s.T * (uint64_t)s.nc; a.np = s.np; a.R = g.R; a.wpw = g.wpw;
  a.mask = const_cast<unsigned long long *>(m.mask); a.cnt = const_cast<uint32_t *>(m.cnt); a.offs = m.scan;
  a.xo = o.x.p; a.lyo = o.ly.p; a.idx = o.idx.p;
  hipLaunchKernelGGL(k_clip_scatter, dim3((unsigned)g.nwg), dim3(DERIVE_BLOCK), g.lds_bytes, st, a);
  HIPCHK(hipGetLastError());
  return MCX_OK;
}

int rowset_from_mask(hipStream_t st, const StoreSpan &s, const RowMask &m, const ClipGeometry &g, mcx_rowset **out)
{
  unsigned long long total = 0;
  auto scan = [&]() -> int {
    MCXCHK(rowset_scan(st, m, g));
    HIPCHK(hipMemcpyAsync(&total, m.scan + g.nwg + 2 * g.nb, sizeof total, hipMemcpyDeviceToHost, st));
    return MCX_OK;
  };
  int rc = scan();
  const hipError_t e0 = hipStreamSynchronize(st);  // (total is the copy's until here)
  MCXCHK(rc);
  HIPCHK(e0);
  std::unique_ptr<mcx_rowset> o;
  MCXCHK(rowset_new(s.np, total, (uint64_t)s.T * (uint64_t)s.nc, o));
  if (total > 0) {
    rc = rowset_scatter(st, s, m, g, *o);
    const hipError_t es = hipStreamSynchronize(st);  // (before the new row set may go)
    MCXCHK(rc);
    HIPCHK(es);
  }
  *out = o.release();
  return MCX_OK;
}

extern "C" int mcx_samples_clip(mcx_engine *e, int first_step, int nsteps, const mcx_clip_spec *spec, mcx_col_clip *cols,
                                long long *nkept, mcx_rowset **out)
{
  return on_store(
      e, first_step, nsteps, [&] { return clip_args(spec, cols, nkept, nsteps); },
      [&](hipStream_t st, Bufs B, const StoreView &v) { return clip_span(st, B, v, spec, cols, nkept, out); });
}

// mcx_samples_clip with its stages timed, for tools/clip_bench.py; the row set is let go
extern "C" int mcx_debug_clip_times(mcx_engine *e, int first_step, int nsteps, const mcx_clip_spec *spec, double *ms)
{
  mcx_rowset *o = nullptr;
  std::vector<mcx_col_clip> cols;
  long long nkept = 0;
  const int rc = on_store(
      e, first_step, nsteps,
      [&] {
        if (!ms) return fail(MCX_ERR_INVALID, "ms is NULL");
        cols.resize((size_t)e->nparam + 1);
        return clip_args(spec, cols.data(), &nkept, nsteps);
      },
      [&](hipStream_t st, Bufs B, const StoreView &v) { return clip_span(st, B, v, spec, cols.data(), &nkept, &o, ms); });
  delete o;
  return rc;
}

extern "C" int mcx_rows_clip(const float *rows, int nsteps, int nc, int np, const mcx_clip_spec *spec, mcx_col_clip *cols,
                             long long *nkept, mcx_rowset **out)
{
  MCXCHK(clip_args(spec, cols, nkept, nsteps));
  return on_rows(rows, nsteps, nc, np,
                 [&](hipStream_t st, Bufs B, const StoreView &v) { return clip_span(st, B, v, spec, cols, nkept, out); });
}

extern "C" int mcx_store_clip(mcx_store *s, const mcx_clip_spec *spec, mcx_col_clip *cols, long long *nkept, mcx_rowset **out)
{
  if (!s) return fail(MCX_ERR_INVALID, "the store s is NULL");
  MCXCHK(clip_args(spec, cols, nkept, s->T));
  HIPCHK(hipSetDevice(s->device));
  return clip_span(s->st, s->bufs(), s->span(), spec, cols, nkept, out);
}

extern "C" int mcx_rowset_destroy(mcx_rowset *r)
{
  if (!r) return MCX_OK;
  (void)hipSetDevice(r->device);
  delete r;
  return MCX_OK;
}

extern "C" int mcx_rowset_shape(const mcx_rowset *r, long long *nrows, int *ncol, long long *nsource)
{
  if (!r) return fail(MCX_ERR_INVALID, "the row set r is NULL");
  if (nrows) *nrows = r->K;
  if (ncol) *ncol = r->np + 1;
  if (nsource) *nsource = r->N;
  return MCX_OK;
}

extern "C" int mcx_rowset_copy(mcx_rowset *r, long long first_row, long long nrows, float *rows)
{
  MCXCHK(rowset_enter(r));
  MCXCHK(rowset_range(r, first_row, nrows));
  if (nrows > 0 && !rows) return fail(MCX_ERR_INVALID, "rows is NULL with nrows = %lld", nrows);
  return gather_span(r->st, r->span(), false, 0u, (uint64_t)first_row, (uint64_t)nrows, rows, nullptr);
}

extern "C" int mcx_rowset_index(mcx_rowset *r, long long first_row, long long nrows, long long *index)
{
  MCXCHK(rowset_enter(r));
  MCXCHK(rowset_range(r, first_row, nrows));
  if (nrows == 0) return MCX_OK;
  if (!index) return fail(MCX_ERR_INVALID, "index is NULL with nrows = %lld", nrows);
  HIPCHK(hipMemcpyAsync(index, r->idx.p + first_row, (size_t)nrows * sizeof(long long), hipMemcpyDeviceToHost, r->st));
  HIPCHK(hipStreamSynchronize(r->st));
  return MCX_OK;
}

extern "C" int mcx_rowset_draw(mcx_rowset *r, uint32_t seed, int64_t ndraw, float *rows, int64_t *index)
{
  MCXCHK(rowset_enter(r));
  if (ndraw < 0) return fail(MCX_ERR_INVALID, "ndraw = %lld is negative", (long long)ndraw);
  if (ndraw > 0 && !rows) return fail(MCX_ERR_INVALID, "rows is NULL with ndraw = %lld", (long long)ndraw);
  if (ndraw > 0 && r->K == 0) return fail(MCX_ERR_INVALID, "ndraw = %lld from a row set of 0 rows", (long long)ndraw);
  return gather_span(r->st, r->span(), true, seed, 0, (uint64_t)ndraw, rows, index);
}

extern "C" int mcx_rowset_store(mcx_rowset *r, long long first_row, int nsteps, int nc, mcx_store **out)
{
  MCXCHK(rowset_enter(r));
  if (!out) return fail(MCX_ERR_INVALID, "out is NULL");
  if (nsteps < 1 || nc < 1) return fail(MCX_ERR_INVALID, "nsteps = %d, nc = %d: a store of at least one step of one chain", nsteps, nc);
  const long long n = (long long)nsteps * nc;
  MCXCHK(rowset_range(r, first_row, n));
  std::unique_ptr<mcx_store> o(new mcx_store);
  o->device = r->device; o->nc = nc; o->nout = r->np; o->T = nsteps;
  MCXCHK(o->st.ensure(hipStreamNonBlocking));
  MCXCHK(o->x.alloc((size_t)n * r->np));
  MCXCHK(o->ly.alloc((size_t)n));
  // the flat layouts are identical: x and ly are one copy each
  hipError_t e1 = hipMemcpyAsync(o->x.p, r->x.p + (size_t)first_row * r->np, (size_t)n * r->np * sizeof(float), hipMemcpyDeviceToDevice, r->st);
  hipError_t e2 = hipMemcpyAsync(o->ly.p, r->ly.p + first_row, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, r->st);
  hipError_t e3 = hipStreamSynchronize(r->st);  // (before the new store may go)
  HIPCHK(e1);
  HIPCHK(e2);
  HIPCHK(e3);
  *out = o.release();
  return MCX_OK;
}

// host only
extern "C" int mcx_debug_clip_thresholds(int ncol, const double *q, const mcx_clip_spec *spec, double *lo, double *hi)
{
  char msg[160];
  return clip_fail(mcx_clip_host::thresholds(ncol, q, spec, lo, hi, msg, sizeof msg), msg);
}
