// mcx_block.hpp -- the numeric contract of DESIGN.md §3 for ONE 4-parameter block in packed form, stated once for the
// three hand-tuned step kernels: k_fused_fast (mcx_device.hpp), k_fused_fastb (mcx_fastb.hpp), k_run_small
// (mcx_persist.hpp).  A block (x0, x1, x2, x3) is held as the pairs e = (x0, x2) and o = (x1, x3): the operands of the
// packed (v_pk_*_f32) instructions.  Plain functions on values: the kernels keep their own registers, loops and pins.
// (The scalar statement of the same contract, for every other kernel, is in the Lik<> structs of mcx_device.hpp.)
#pragma once
#include "mcx_numerics.hpp"

namespace mcx {

template <int LPC>
__device__ __forceinline__ float group_sum(float p);  // the butterfly over the lanes of a chain (mcx_device.hpp)

// ---- (e, o) pairs to and from the row-major float4 of the chain-state matrices ---------------------------------
__device__ __forceinline__ float4 pk_float4(f32x2 e, f32x2 o) { return make_float4(e.x, o.x, e.y, o.y); }
__device__ __forceinline__ void pk_pairs(const float4 f, f32x2 &e, f32x2 &o) { e = f32x2{f.x, f.z}; o = f32x2{f.y, f.w}; }
__device__ __forceinline__ void pk_load(const float *p, f32x2 &e, f32x2 &o) { pk_pairs(*reinterpret_cast<const float4 *>(p), e, o); }
__device__ __forceinline__ void pk_store(float *p, f32x2 e, f32x2 o) { *reinterpret_cast<float4 *>(p) = pk_float4(e, o); }
// a block's mean and sum of squares (both loads are issued before either is unpacked)
__device__ __forceinline__ void pk_load_moments(const float *mu, const float *psum2, size_t off, f32x2 &me, f32x2 &mo, f32x2 &se, f32x2 &so)
{
  const float4 m = *reinterpret_cast<const float4 *>(mu + off);
  const float4 p = *reinterpret_cast<const float4 *>(psum2 + off);
  pk_pairs(m, me, mo);
  pk_pairs(p, se, so);
}

// the block's entries k0 .. k0 + 3 of the diagonal of the factor T[d][d] (diagonal proposals, src/mcpar.cc:302-312)
__device__ __forceinline__ void pk_load_tdiag(const float *T, int d, int k0, f32x2 &te, f32x2 &to)
{
  te = f32x2{T[(k0 + 0) * d + k0 + 0], T[(k0 + 2) * d + k0 + 2]};
  to = f32x2{T[(k0 + 1) * d + k0 + 1], T[(k0 + 3) * d + k0 + 3]};
}

// diagonal Gaussian: the block's means and 1/sigma^2 (lik = mu[d], s2inv[d])
__device__ __forceinline__ void pk_load_gauss(const float *lik, int d, int k0, f32x2 &gme, f32x2 &gmo, float (&gs)[4])
{
  gme = f32x2{lik[k0 + 0], lik[k0 + 2]}; gmo = f32x2{lik[k0 + 1], lik[k0 + 3]};
  gs[0] = lik[d + k0 + 0]; gs[1] = lik[d + k0 + 1]; gs[2] = lik[d + k0 + 2]; gs[3] = lik[d + k0 + 3];
}

// ---- likelihood partials of one block: the SUM, which the caller reduces over the chain and negates (or not) ----
// Rosenbrock1 (src/rosenbrock.cc:4-21) on the pairs (x0,x1), (x2,x3): 100 (x1 - x0^2)^2 + (1 - x0)^2 each
__device__ __forceinline__ float pk_rosen1(f32x2 pe, f32x2 po, bool live)
{
  const f32x2 t1 = splat2(1.0f) - pe;
  const f32x2 t2 = fma2(-pe, pe, po);
  const f32x2 term = fma2(splat2(100.0f) * t2, t2, t1 * t1);
  float acc = 0.0f;
  if (live) acc = term.x + term.y;  // == (0 + term.x) + term.y: the terms are >= +0
  return acc;
}

// diagonal Gaussian (src/rosenbrock.cc:44-61): acc = fma((0.5 a) a, 1/sigma^2, acc) for k = 0..3 in order, a = x - mu
__device__ __forceinline__ float pk_gauss(f32x2 pe, f32x2 po, f32x2 gme, f32x2 gmo, const float (&gs)[4], bool live)
{
  const f32x2 ae = pe - gme, ao = po - gmo;
  const f32x2 he = (splat2(0.5f) * ae) * ae, ho = (splat2(0.5f) * ao) * ao;
  float acc = 0.0f;
  if (live) {
    acc = __builtin_fmaf(he.x, gs[0], 0.0f);
    acc = __builtin_fmaf(ho.x, gs[1], acc);
    acc = __builtin_fmaf(he.y, gs[2], acc);
    acc = __builtin_fmaf(ho.y, gs[3], acc);
  }
  return acc;
}

// mixture of unit Gaussians (DualGaussian: src/rosenbrock.cc:63-78): |x - m_c|^2 of one block, k = 0..3 in order;
// `means` = the component's means of this block (16-byte aligned, LDS)
__device__ __forceinline__ float pk_mix_dist2(f32x2 pe, f32x2 po, const float *means, bool live)
{
  float s2 = 0.0f;
  if (live) {
    const float4 m = *reinterpret_cast<const float4 *>(means);
    const f32x2 ae = pe - f32x2{m.x, m.z}, ao = po - f32x2{m.y, m.w};
    s2 = __builtin_fmaf(ae.x, ae.x, 0.0f);
    s2 = __builtin_fmaf(ao.x, ao.x, s2);
    s2 = __builtin_fmaf(ae.y, ae.y, s2);
    s2 = __builtin_fmaf(ao.y, ao.y, s2);
  }
  return s2;
}

// ... and its tail: log sum_c w_c exp(-|x - m_c|^2 / 2) as a log-sum-exp over e[c] = fma(-0.5, |x - m_c|^2, log w_c),
// c < K <= 8 (e[c] = 0 beyond): the components' exponentials two at a time, added in component order
__device__ __forceinline__ float mix_logsumexp(const float (&e)[8], int K)
{
  float emax = e[0];
#pragma unroll
  for (int c = 1; c < 8; ++c)
    if (c < K) emax = e[c] > emax ? e[c] : emax;
  float ssum = 0.0f;
#pragma unroll
  for (int c = 0; c < 8; c += 2) {
    if (c < K) {
      const f32x2 ex = expf_v2x2(f32x2{e[c] - emax, e[c + 1] - emax});
      ssum = ssum + ex.x;
      if (c + 1 < K) ssum = ssum + ex.y;
    }
  }
  return emax + logf_v1(ssum);
}

// the first log2(BPL) stages of the butterfly over the block index for the BPL CONSECUTIVE blocks of a
// lane -- they pair blocks of one lane: plain adds -- and the lane group's butterfly for the rest
template <int LPC2, int BPL>
__device__ __forceinline__ float blocks_sum(const float (&p)[BPL])
{
  static_assert(BPL == 1 || BPL == 2 || BPL == 4, "one, two or four blocks per lane");
  if (BPL == 1) return group_sum<LPC2>(p[0]);
  if (BPL == 2) return group_sum<LPC2>(p[0] + p[BPL > 1 ? 1 : 0]);
  return group_sum<LPC2>((p[0] + p[BPL > 1 ? 1 : 0]) + (p[BPL == 4 ? 2 : 0] + p[BPL == 4 ? 3 : 0]));
}

// ---- staging in LDS by the NT threads of a workgroup (the caller places the barrier) ----------------------------
// mixture: component means [ncomp][d] and log-weights [ncomp] (every lane group reads the same rows)
template <int NT>
__device__ __forceinline__ void stage_mixture(float *lds_means, float *lds_logw, const float *lik, int ncomp, int d)
{
  const int kd = ncomp * d;
  for (int i = threadIdx.x; i < kd; i += NT) lds_means[i] = lik[i];
  if (threadIdx.x < (unsigned)ncomp) lds_logw[threadIdx.x] = lik[kd + threadIdx.x];
}

// full factor by column for chains of NB blocks: slot [(qq * 4 + c) * NB + qv] = column 4 qq + c of the four rows of
// block qv, as (row 0, row 2, row 1, row 3): the two halves are the packed operands of the block's (x0, x2) / (x1, x3)
// accumulators; zero beyond the matrix
template <int NB, int NT>
__device__ __forceinline__ void stage_factor_columns(float4 *lds_T, const float *T, int dd)
{
  for (int i = threadIdx.x; i < 16 * NB * NB; i += NT) {
    const int h = i & 3, qv = (i >> 2) % NB, c = ((i >> 2) / NB) & 3, qq = (i >> 2) / (4 * NB);
    const int row = 4 * qv + (h == 0 ? 0 : (h == 1 ? 2 : (h == 2 ? 1 : 3))), col = 4 * qq + c;
    reinterpret_cast<float *>(lds_T)[i] = (row < dd && col < dd) ? T[row * dd + col] : 0.0f;
  }
}

// ---- moments -----------------------------------------------------------------------------------------------------
// Welford update of one block's mean and sum of squares from the post-step state (src/mcpar.cc:199-202);
// w2 = 1/pwgt of the step in both halves (:186-187)
__device__ __forceinline__ void pk_welford(f32x2 xe, f32x2 xo, f32x2 w2, f32x2 &me, f32x2 &mo, f32x2 &se, f32x2 &so)
{
  const f32x2 de = xe - me, dO = xo - mo;
  me = fma2(de, w2, me);
  mo = fma2(dO, w2, mo);
  se = fma2(de, xe - me, se);
  so = fma2(dO, xo - mo, so);
}

// snapshot of one block for the next exchange (src/mcpar.cc:202-208): (mean, variance = psum2 / pwgt) interleaved into
// the shard's slot `musig` at the block's offset `off` in the chain-state matrix; `sig`, where not null: the variances as
// mcx_get_var returns them (the run's last step; k_variance otherwise).  (The parameters are in the order in which the
// kernels' text first named them: a lambda's captures are laid out by first mention, and the registers follow.)
__device__ __forceinline__ void pk_snapshot(f32x2 se, f32x2 so, f32x2 w2, float *musig, float *sig, size_t off, f32x2 me, f32x2 mo)
{
  const f32x2 ve = se * w2, vo = so * w2;
  float4 *slot = reinterpret_cast<float4 *>(musig + 2 * off);
  slot[0] = make_float4(me.x, ve.x, mo.x, vo.x);
  slot[1] = make_float4(me.y, ve.y, mo.y, vo.y);
  if (sig) pk_store(sig + off, ve, vo);
}

// ---- acceptance draws (k_fused_fast, k_fused_fastb) ----------------------------------------------------------------
// Philox block (t >> 2) of the ACCEPT stream serves steps 4b .. 4b + 3.  The LPC lanes of a chain split the work: lane q
// draws block b for b % LPC == q, and the four logs are taken here, once per 4 * LPC steps per lane
template <int LPC>
__device__ __forceinline__ void accept_refresh(uint32_t blk, int q, uint32_t g, uint32_t seed, uint32_t &ablk, f32x2 &al01, f32x2 &al23)
{
  if ((blk & ~(uint32_t)(LPC - 1)) != ablk) {
    ablk = blk & ~(uint32_t)(LPC - 1);
    const u32x4 aw = philox4x32_10(ablk + (uint32_t)q, g, 0u, 0u, seed, ST_ACCEPT);
    al01 = accept_lu_x2(aw.x, aw.y);
    al23 = accept_lu_x2(aw.z, aw.w);
  }
}
// word wi = t & 3 of the lane's current block.  (By address: wi is wave-uniform, the word is chosen by scalar branches and
// only that word is read; handed over by value all four are read first and the choice becomes selects -- another step loop.)
__device__ __forceinline__ float accept_word(const f32x2 *al01, const f32x2 *al23, uint32_t wi)
{
  return wi == 0u ? al01->x : (wi == 1u ? al01->y : (wi == 2u ? al23->x : al23->y));
}

}  // namespace mcx
