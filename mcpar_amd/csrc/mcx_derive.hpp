// mcx_derive.hpp -- the derive sweep: a function f of one row (x[0..np-1], ly) -> nout floats, applied
// to every row of a step range of a sample store.  The store is x[T][nc][np] plus ly[T][nc], i.e. N = T * nc rows of np
// contiguous floats; the result is a store of the same shape, x'[N][nout] and ly' = ly.
//
// One body template over the functor: instantiated for MCX_DERIVE_LINEAR in mcx_derive.hip, and compiled around a user's
// mcx_user_derive at run time (hiprtc; this header travels inside libmcx.so as a string, so it includes nothing but
// mcx_numerics.hpp).  A workgroup of DERIVE_BLOCK threads takes R consecutive rows, one row per lane of its first R threads:
//   1. the R * np floats of its rows are one contiguous piece of x: loaded coalesced (16 bytes per lane where the piece
//      starts on a 16-byte boundary) into an LDS tile of row stride np | 1
//   2. lane r < R calls f(its LDS row, np, ly[row], par, its row of an LDS output tile of stride nout | 1, nout)
//   3. the R * nout floats are one contiguous piece of x': stored coalesced from the output tile; ly' = ly by the lanes
// The odd strides put the 32 lanes of an LDS access group on 32 banks when every lane walks its own row.  Every output
// word is written by one thread from values of its own workgroup: no atomics, no waits across workgroups, and the bytes do
// not depend on scheduling.
#pragma once
#include "mcx_numerics.hpp"

namespace mcx {

constexpr int DERIVE_BLOCK = 256;         // threads per workgroup
constexpr int DERIVE_LDS_BUDGET = 40960;  // bytes of LDS a workgroup's two tiles may take: four workgroups per CU
constexpr int DERIVE_MAXW = 256;          // np and nout at most

struct DeriveArgs {
  const float *x, *ly;  // x[N][np], ly[N]
  float *xo, *lyo;      // x'[N][nout], ly'[N]
  const float *par;
  uint64_t N;
  int np, nout, R;      // R = derive_rows(np, nout)
};

// LDS floats of a tile of R rows
MCX_HD int derive_lds_floats(int np, int nout, int R) { return R * ((np | 1) + (nout | 1)); }

// Rows per workgroup, a function of np and nout alone: 256 where the two tiles fit the budget, else the largest power of
// two that does (16 at np = nout = 256, where a row takes 2 056 bytes)
MCX_HD int derive_rows(int np, int nout)
{
  int R = DERIVE_BLOCK;
  while (R > 1 && derive_lds_floats(np, nout, R) * 4 > DERIVE_LDS_BUDGET) R >>= 1;
  return R;
}

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
// tile[r * stride + c] <-> g[r * w + c] for the cnt = rows * w floats of a workgroup's rows.  (r, c) of a thread's element
// advance by the workgroup's stride without a division per element.
template <bool LOAD>
__device__ __forceinline__ void derive_tile_copy(float *tile, int stride, float *g, int w, int cnt, bool vec4)
{
  const int tid = (int)threadIdx.x;
  int head = 0;
  if (vec4) {
    const int nq = cnt >> 2, step = DERIVE_BLOCK * 4;
    const int dr = step / w, dc = step - dr * w;
    int e = tid * 4, r = e / w, c = e - r * w;
    for (int q = tid; q < nq; q += DERIVE_BLOCK) {
      float4 *gp = reinterpret_cast<float4 *>(g) + q;
      float v[4];
      if (LOAD) {
        const float4 t = *gp;
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      }
      int rr = r, cc = c;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (LOAD) tile[rr * stride + cc] = v[k];
        else v[k] = tile[rr * stride + cc];
        if (++cc == w) { cc = 0; ++rr; }
      }
      if (!LOAD) *gp = make_float4(v[0], v[1], v[2], v[3]);
      r += dr; c += dc;
      if (c >= w) { c -= w; ++r; }
    }
    head = nq << 2;
  }
  // the scalar path: everything when the piece is not 16-byte aligned, else the up to three floats behind the last quad
  {
    const int dr = DERIVE_BLOCK / w, dc = DERIVE_BLOCK - dr * w;
    int e = head + tid, r = e / w, c = e - r * w;
    for (; e < cnt; e += DERIVE_BLOCK) {
      if (LOAD) tile[r * stride + c] = g[e];
      else g[e] = tile[r * stride + c];
      r += dr; c += dc;
      if (c >= w) { c -= w; ++r; }
    }
  }
}

// The body.  f(const float *x, int np, float ly, const float *par, float *out, int nout) is called for rows of the range
// only, never for a lane without a row.  np, nout: a.np, a.nout, passed apart so that a run-time build hands constants in.
template <class F> __device__ __forceinline__ void derive_body(const DeriveArgs &a, const int np, const int nout, F f)
{
  extern __shared__ float derive_lds[];
  const int R = a.R, sx = np | 1, so = nout | 1;
  float *xs = derive_lds, *os = derive_lds + R * sx;
  const uint64_t row0 = (uint64_t)blockIdx.x * (uint64_t)R;
  const uint64_t left = a.N - row0;  // > 0: the grid is ceil(N / R)
  const int rows = left < (uint64_t)R ? (int)left : R;
  const float *gx = a.x + row0 * (uint64_t)np;
  float *go = a.xo + row0 * (uint64_t)nout;
  const int tid = (int)threadIdx.x;
  const bool mine = tid < rows;
  float ly = 0.0f;
  if (mine) ly = a.ly[row0 + tid];
  derive_tile_copy<true>(xs, sx, const_cast<float *>(gx), np, rows * np, ((unsigned long)gx & 15ul) == 0);
  __syncthreads();
  if (mine) {
    f(xs + tid * sx, np, ly, a.par, os + tid * so, nout);
    a.lyo[row0 + tid] = ly;
  }
  __syncthreads();
  derive_tile_copy<false>(os, so, go, nout, rows * nout, ((unsigned long)go & 15ul) == 0);
}

// MCX_DERIVE_LINEAR: par = A[nout][np] row-major, then b[nout].  out[j]: acc = b[j], then for k = 0 .. np-1 in that order
// acc = acc + A[j][k] * x[k], the product and the sum each rounded to float (built with -ffp-contract=off: not an fma
// chain).  Four outputs share one read of x[k]; each output's own sequence of operations is the stated one.
struct DeriveLinear {
  __device__ __forceinline__ void operator()(const float *x, int np, float, const float *par, float *out, int nout) const
  {
    const float *A = par, *b = par + (size_t)nout * np;
    int j = 0;
    for (; j + 4 <= nout; j += 4) {
      const float *a0 = A + (size_t)j * np, *a1 = a0 + np, *a2 = a1 + np, *a3 = a2 + np;
      float c0 = b[j], c1 = b[j + 1], c2 = b[j + 2], c3 = b[j + 3];
      for (int k = 0; k < np; ++k) {
        const float xk = x[k];
        c0 = c0 + a0[k] * xk;
        c1 = c1 + a1[k] * xk;
        c2 = c2 + a2[k] * xk;
        c3 = c3 + a3[k] * xk;
      }
      out[j] = c0; out[j + 1] = c1; out[j + 2] = c2; out[j + 3] = c3;
    }
    for (; j < nout; ++j) {
      const float *aj = A + (size_t)j * np;
      float c = b[j];
      for (int k = 0; k < np; ++k) c = c + aj[k] * x[k];
      out[j] = c;
    }
  }
};
#endif

}  // namespace mcx
