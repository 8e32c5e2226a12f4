// mcx_summary_kernels.hpp -- what mcx_summary.hip, mcx_covariance.hip and mcx_ranks.hip need: the column tiles of the sample store,
// pass 1 of every summary (k_sum_moments: per-series fp64 sums), the fixed-order reducer k_sum_rows that every cross-chain
// or cross-workgroup sum goes through, and the upload of host rows to a scratch store (on_rows).  Internal to those three
// translation units (each gets its own copy of the kernels); nothing here is part of the library's interface.
#pragma once
#include "mcx_engine_internal.hpp"

// mcx_summary.hip's device passes for mcx_ranks.hip: summary_device with the parts (SUMM_*) a pass needs
enum { SUMM_OSTAT = 1, SUMM_ACOV = 2 };
MCXI int summary_device_parts(hipStream_t st, DevBuf<double> *d, DevBuf<unsigned long long> *h, DevBuf<uint32_t> *u,
                              const float *x, const float *ly, int nc, int np, int64_t T, const double *probs, int nprobs,
                              mcx_col_summary *cols, double *quantiles, int parts);

namespace {

constexpr int SB = 256;     // threads per workgroup of every summary kernel
constexpr int CTX = 16;     // columns per parameter tile

// where a tile set lives: x (ncs = np columns, chain stride np) or ly (ncs = 1, chain stride 1)
struct TileSet {
  const float *src;  // step 0 of the range
  size_t rs;         // floats per step
  int cs;            // floats per chain
  int ncs;           // columns in this array
  int col0;          // global column of its first column
  int ct, cg, ntiles, nbc;
};

struct Lane {
  int chain, lcol, j;
  bool ok;
};
__device__ __forceinline__ Lane lane_of(const TileSet &t, int tile, int bc, int nc)
{
  Lane l;
  const int k = threadIdx.x / t.ct;
  l.j = threadIdx.x - k * t.ct;
  l.chain = bc * t.cg + k;
  l.lcol = tile * t.ct + l.j;
  l.ok = k < t.cg && l.chain < nc && l.lcol < t.ncs;
  return l;
}

// pass 1: half-chain means and series sums.  grid = nbc * ntiles
__global__ void __launch_bounds__(SB) k_sum_moments(TileSet t, int nc, int64_t T, int64_t n, double *hm, double *tot)
{
  const int tile = blockIdx.x % t.ntiles, bc = blockIdx.x / t.ntiles;
  const Lane l = lane_of(t, tile, bc, nc);
  if (!l.ok) return;
  const float *p = t.src + (size_t)l.chain * t.cs + l.lcol;
  double s0 = 0.0, s1 = 0.0, sm = 0.0;
#pragma unroll 8
  for (int64_t s = 0; s < n; ++s) s0 += (double)p[s * t.rs];
#pragma unroll 8
  for (int64_t s = T - n; s < T; ++s) s1 += (double)p[s * t.rs];
  if (T - 2 * n == 1) sm = (double)p[n * t.rs];
  const int col = t.col0 + l.lcol;
  hm[((size_t)col * 2 + 0) * nc + l.chain] = s0 / (double)n;
  hm[((size_t)col * 2 + 1) * nc + l.chain] = s1 / (double)n;
  tot[(size_t)col * nc + l.chain] = (s0 + sm) + s1;
}

// out[r] = sum over l < len of in[r * stride + l], or of (in - center[col] * cscale)^2; len = lenx for a parameter column,
// lenl for log L (col = (r / qper) % ncol).  One workgroup per row, fixed order: per-thread strided sums, then a tree.
__global__ void __launch_bounds__(SB) k_sum_rows(const double *in, size_t stride, int qper, int ncol, int np, size_t lenx,
                                                 size_t lenl, const double *center, double cscale, double *out)
{
  __shared__ double red[SB];
  const size_t r = blockIdx.x;
  const int col = (int)((r / qper) % ncol);
  const size_t len = col < np ? lenx : lenl;
  const double c = center ? center[col] * cscale : 0.0;
  const double *p = in + r * stride;
  double s = 0.0;
  for (size_t i = threadIdx.x; i < len; i += SB) {
    const double v = p[i];
    s += center ? (v - c) * (v - c) : v;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = SB / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[r] = red[0];
}

__global__ void k_sum_deinterleave(const float *rows, size_t nrows, int np, float *x, float *ly)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t ncol = (size_t)np + 1;
  if (i >= nrows * ncol) return;
  const size_t r = i / ncol;
  const int c = (int)(i - r * ncol);
  if (c < np) x[r * np + c] = rows[i];
  else ly[r] = rows[i];
}

inline TileSet tiles_x(const float *x, int nc, int np)
{
  TileSet t;
  t.src = x; t.rs = (size_t)nc * np; t.cs = np; t.ncs = np; t.col0 = 0;
  t.ct = std::min(np, CTX); t.cg = SB / t.ct; t.ntiles = (np + t.ct - 1) / t.ct; t.nbc = (nc + t.cg - 1) / t.cg;
  return t;
}
inline TileSet tiles_l(const float *ly, int nc, int np)
{
  TileSet t;
  t.src = ly; t.rs = (size_t)nc; t.cs = 1; t.ncs = 1; t.col0 = np;
  t.ct = 1; t.cg = SB; t.ntiles = 1; t.nbc = (nc + SB - 1) / SB;
  return t;
}

struct Bufs {
  DevBuf<double> *d;
  DevBuf<unsigned long long> *h;
  DevBuf<uint32_t> *u;
};

// rows [nsteps * nc][np + 1] on the host (MCout layout) uploaded to a scratch store x, ly on a stream of its own:
// f(st, bufs, x, ly) runs the device passes there
template <class F> int on_rows(const float *rows, int nsteps, int nc, int np, F f)
{
  if (!rows || nc < 1 || np < 1 || np > 256) return fail(MCX_ERR_INVALID, "bad arguments");
  MCXCHK(need_device());
  const size_t nr = (size_t)nsteps * nc;
  DevBuf<float> rd, x, ly;
  DevBuf<double> d;
  DevBuf<unsigned long long> h;
  DevBuf<uint32_t> u;
  hipStream_t st = nullptr;
  auto run = [&]() -> int {
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    MCXCHK(rd.alloc(nr * (np + 1)));
    MCXCHK(x.alloc(nr * np));
    MCXCHK(ly.alloc(nr));
    HIPCHK(hipMemcpyAsync(rd.p, rows, nr * (np + 1) * sizeof(float), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_sum_deinterleave, dim3(nblocks(nr * (np + 1))), dim3(BLOCK), 0, st, rd.p, nr, np, x.p, ly.p);
    HIPCHK(hipGetLastError());
    return f(st, Bufs{&d, &h, &u}, x.p, ly.p);
  };
  const int rc = run();
  if (st) {
    (void)hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
  }
  rd.release(); x.release(); ly.release(); d.release(); h.release(); u.release();
  return rc;
}

}  // namespace
