// mcx_sort_kernels.hpp -- the segmented LSD radix sort of DESIGN.md section 11, for the units that sort every column's keys:
// mcx_ranks.hip (the pooled ranks of a store) and mcx_compare.hip (section 20: two stores, column by column).  The key of a
// value, the four kernels of a pass and the four-pass loop; each unit that includes it gets its own copy of the kernels.
// Internal, as everything under csrc/ is.
//   4 x { k_rank_hist, k_rank_rowsum, k_rank_scan, k_rank_scatter }
//                        LSD radix sort of every column's keys, 8 bits per pass, the column a grid dimension: digit counts
//                        of each tile of RTILE keys, their exclusive scan in (digit, tile) order, a stable scatter.
//                        Every kernel is a launch of its own and none waits for another workgroup: the order between the
//                        steps of a pass is the stream's.  Counting uses integer LDS atomics only.
#pragma once
#include "mcx_summary_kernels.hpp"

namespace {

constexpr int RKPT = 32;             // keys per thread of a sort tile
constexpr int RTILE = SB * RKPT;     // keys per workgroup of a sort pass
constexpr int RWAVES = SB / 64;      // a wavefront takes RTILE / RWAVES consecutive keys of the tile
static_assert(SB == 256, "a sort workgroup has one thread per digit value");

// mcx_summary.hip's key with -0 canonicalised to +0: equal floats have equal keys, every NaN sorts last
__device__ __forceinline__ uint32_t rkey(float v)
{
  uint32_t u = __float_as_uint(v);
  if (v != v) return 0xffffffffu;
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the lanes of this wavefront that are valid and hold the same 8-bit digit as this lane
__device__ __forceinline__ unsigned long long match8(uint32_t d, bool valid)
{
  unsigned long long m = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (d >> b) & 1u;
    const unsigned long long bm = __ballot(bit);
    m &= bit ? bm : ~bm;
  }
  return m;
}

// 2a. digit counts of one tile.  grid = (tiles, columns); hist[(column * 256 + digit) * nblk + tile]
__global__ void __launch_bounds__(SB) k_rank_hist(const uint32_t *keys, int64_t N, int shift, uint32_t nblk, uint32_t *hist)
{
  __shared__ uint32_t cnt[256];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t *k = keys + (size_t)blockIdx.y * (size_t)N;
  const int64_t base = (int64_t)blockIdx.x * RTILE;
  const int lane = threadIdx.x & 63;
  for (int j = 0; j < RKPT; ++j) {
    const int64_t i = base + (int64_t)j * SB + threadIdx.x;
    const bool valid = i < N;
    const uint32_t d = valid ? (k[i] >> shift) & 255u : 0u;
    const unsigned long long peers = match8(d, valid);
    // one add per digit and wavefront: most keys of a pass share their digit
    if (valid && lane == __ffsll((long long)peers) - 1) atomicAdd(&cnt[d], (uint32_t)__popcll(peers));
  }
  __syncthreads();
  hist[((size_t)blockIdx.y * 256 + threadIdx.x) * nblk + blockIdx.x] = cnt[threadIdx.x];
}

// 2b. the keys of one (column, digit) over all tiles.  grid = (256, columns)
__global__ void __launch_bounds__(SB) k_rank_rowsum(const uint32_t *hist, uint32_t nblk, uint32_t *rowsum)
{
  __shared__ uint32_t red[SB];
  const size_t r = (size_t)blockIdx.y * 256 + blockIdx.x;
  const uint32_t *row = hist + r * nblk;
  uint32_t s = 0;
  for (uint32_t i = threadIdx.x; i < nblk; i += SB) s += row[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = SB / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) rowsum[r] = red[0];
}

// 2c. hist -> where each tile's keys of each digit start in the column: the exclusive scan in (digit, tile) order.
// grid = (256, columns): workgroup (digit, column) starts at the count of the smaller digits and scans its own row
__global__ void __launch_bounds__(SB) k_rank_scan(uint32_t *hist, uint32_t nblk, const uint32_t *rowsum)
{
  __shared__ uint32_t sh[SB];
  const int tid = threadIdx.x;
  sh[tid] = tid < (int)blockIdx.x ? rowsum[(size_t)blockIdx.y * 256 + tid] : 0u;
  __syncthreads();
  for (int w = SB / 2; w > 0; w >>= 1) {
    if (tid < w) sh[tid] += sh[tid + w];
    __syncthreads();
  }
  uint32_t carry = sh[0];
  __syncthreads();
  uint32_t *row = hist + ((size_t)blockIdx.y * 256 + blockIdx.x) * nblk;
  for (uint32_t b0 = 0; b0 < nblk; b0 += SB) {
    const uint32_t i = b0 + tid;
    const uint32_t v = i < nblk ? row[i] : 0u;
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < SB; off <<= 1) {
      const uint32_t a = tid >= off ? sh[tid - off] : 0u;
      __syncthreads();
      sh[tid] += a;
      __syncthreads();
    }
    if (i < nblk) row[i] = carry + sh[tid] - v;
    carry += sh[SB - 1];
    __syncthreads();
  }
}

// 2d. the stable scatter of one tile.  grid = (tiles, columns).  Wavefront w holds keys [w, w + 1) * RTILE / RWAVES of the
// tile, 64 consecutive keys a round: (wavefront, round, lane) is index order, and so is the order within a digit
__global__ void __launch_bounds__(SB) k_rank_scatter(const uint32_t *in, uint32_t *out, int64_t N, int shift, uint32_t nblk,
                                                     const uint32_t *hist)
{
  __shared__ uint32_t woff[RWAVES][256];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  in += (size_t)blockIdx.y * (size_t)N;
  out += (size_t)blockIdx.y * (size_t)N;
  for (int i = tid; i < RWAVES * 256; i += SB) (&woff[0][0])[i] = 0u;
  __syncthreads();
  const int64_t wbase = (int64_t)blockIdx.x * RTILE + (int64_t)w * (RTILE / RWAVES);
  uint32_t key[RKPT], local[RKPT];  // local: the key's place among its wavefront's keys of the same digit
#pragma unroll
  for (int j = 0; j < RKPT; ++j) {
    const int64_t i = wbase + j * 64 + lane;
    const bool valid = i < N;
    key[j] = valid ? in[i] : 0xffffffffu;
    const uint32_t d = (key[j] >> shift) & 255u;
    const unsigned long long peers = match8(d, valid);
    const int leader = valid ? __ffsll((long long)peers) - 1 : lane;
    uint32_t old = 0u;
    if (valid && lane == leader) old = atomicAdd(&woff[w][d], (uint32_t)__popcll(peers));
    old = __shfl(old, leader);
    local[j] = old + (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
  }
  __syncthreads();
  {  // thread = digit: where each wavefront's keys of the digit start in the column
    uint32_t run = hist[((size_t)blockIdx.y * 256 + tid) * nblk + blockIdx.x];
    for (int v = 0; v < RWAVES; ++v) {
      const uint32_t c = woff[v][tid];
      woff[v][tid] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < RKPT; ++j) {
    const int64_t i = wbase + j * 64 + lane;
    if (i < N) out[woff[w][(key[j] >> shift) & 255u] + local[j]] = key[j];
  }
}

// The LSD radix sort of ncols columns of N keys each, a[column][N]: four passes alternating between a and b, after which the
// sorted keys are back in a.  hist[ncols * 256 * nblk] and rowsum[ncols * 256] are the counts, nblk = ceil(N / RTILE) the sort
// tiles per column.  run(pass, f) runs the launches f of one pass (a unit's stage timer, or f() alone)
template <class Run>
int sort_columns(hipStream_t st, uint32_t *a, uint32_t *b, uint32_t *hist, uint32_t *rowsum, int64_t N, unsigned ncols, uint32_t nblk,
                 Run run)
{
  uint32_t *src = a, *dst = b;
  for (int pass = 0; pass < 4; ++pass) {
    MCXCHK(run(pass, [&]() -> int {
      const int shift = 8 * pass;
      hipLaunchKernelGGL(k_rank_hist, dim3(nblk, ncols), dim3(SB), 0, st, (const uint32_t *)src, N, shift, nblk, hist);
      HIPCHK(hipGetLastError());
      hipLaunchKernelGGL(k_rank_rowsum, dim3(256, ncols), dim3(SB), 0, st, (const uint32_t *)hist, nblk, rowsum);
      HIPCHK(hipGetLastError());
      hipLaunchKernelGGL(k_rank_scan, dim3(256, ncols), dim3(SB), 0, st, hist, nblk, (const uint32_t *)rowsum);
      HIPCHK(hipGetLastError());
      hipLaunchKernelGGL(k_rank_scatter, dim3(nblk, ncols), dim3(SB), 0, st, (const uint32_t *)src, dst, N, shift, nblk,
                         (const uint32_t *)hist);
      HIPCHK(hipGetLastError());
      return MCX_OK;
    }));
    std::swap(src, dst);
  }
  return MCX_OK;
}

}  // namespace
