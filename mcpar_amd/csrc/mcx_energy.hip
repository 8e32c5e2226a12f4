// mcx_energy.hip -- mcx_*_energy: two sample stores compared as clouds of points: the energy distance
// between rows drawn from each store and its permutation law.  The work is every pairwise distance of the N pooled rows, each
// multiplied into nperm + 2 label vectors: a dense fp64 contraction on the matrix cores.
//   1. gather_span         section 12's k_gather_rows: each side's drawn (or all) rows to the host
//   2. host                scale and flags per column in fp64, z = x / scale with the dropped columns removed; the label vectors
//                          (mcx_energy_host.hpp), bit-packed: lab[block][row] holds label columns 16 block ... 16 block + 15 of
//                          a row.  Column 0 is all ones, column 1 is l_0, column 1 + p is l_p
//   3. k_energy_pairs      grid = (tiles of 64 rows i, slabs of rows j, chunks of label blocks).  A wavefront owns 16 rows i.
//                          For 64 rows j at a time the lane (i = lane & 15, jj = lane >> 4) forms d_ij of rows j = jj + 4 u,
//                          u < 16, on the vector unit from z staged in LDS (EKC columns at a time): that double is the A
//                          operand of v_mfma_f64_16x16x4_f64, A[i = lane & 15][k = lane >> 4].  B[k = lane >> 4][q = lane & 15]
//                          is the label bit of row j = 4 u + (lane >> 4) as 0.0 or 1.0, and acc[block] += d L for every block
//                          of the chunk.  D[i = (lane >> 4) + 4 reg][q = lane & 15] = sum_j d_ij L_jq; the workgroup's
//                          sum_i D[i][q] is its part of S_A(q) (d is symmetric bit for bit: sum_i sum_j d_ij L_jq = sum_j L_jq r_j)
//                          and sum_i L_iq D[i][q] its part of S_AA(q) -> part[slab][tile][2][label column]
//   4. k_energy_reduce     one thread per (sum, label column) walks the slabs and tiles in order
// The full matrix is computed, not a triangle: d_ij = d_ji is used only to read S_A off the same accumulators.  No float
// atomics and no global atomics; every word of the scratch that is read was uploaded or written earlier in the same call.
#include "mcx_store.hpp"

#include "mcx_energy_host.hpp"

#include <atomic>
#include <chrono>
#include <exception>
#include <limits>
#include <thread>

namespace {

namespace EH = mcx_energy_host;

typedef double en_f64x4 __attribute__((ext_vector_type(4)));

constexpr int EB = 256;       // threads of a k_energy_pairs workgroup: four wavefronts
constexpr int ETI = 64;       // rows i of a workgroup, 16 a wavefront
constexpr int EJB = 64;       // rows j staged at a time: 16 MFMA steps of 4
constexpr int EKC = 32;       // columns of z staged at a time
constexpr int EKP = EKC + 1;  // the staged rows' stride in doubles: odd, so that 16 rows i lie in 16 different bank pairs
constexpr int ECH = 16;       // label blocks of a chunk at most: 16 accumulators of 4 doubles, 128 registers
constexpr int ESLAB = 16384;  // rows j of a slab (MCX_ENERGY_SLAB_ROWS lowers it)
enum { ET_GATHER = 0, ET_SCALE, ET_LABELS, ET_UPLOAD, ET_PAIRS, ET_REDUCE, ET_TOTAL, ET_N };

struct EnergyArgs {
  const double *z;      // [N][K]
  const uint16_t *lab;  // [PB][Np], Np = N rounded up to EJB, rows from N on are 0
  int N, Np, K, PB, tiles, slab_rows;
  double *part;  // [slab][tile][2][PB * 16]
};

// 3. grid = (tiles, slabs, chunks).  NB: the label blocks of a chunk, a power of two (energy_geometry); a last chunk of fewer
// blocks stages zeros for the rest, whose sums are not written
template <int NB>
__global__ void __launch_bounds__(EB) k_energy_pairs(const EnergyArgs a)
{
  constexpr int LW = NB < 2 ? 1 : NB / 2;  // 32-bit words of a staged row's labels: blocks 2 k (low half) and 2 k + 1
  __shared__ double zi[ETI * EKP], zj[EJB * EKP];
  __shared__ __attribute__((aligned(16))) uint32_t lj[EJB * LW];
  __shared__ double red[2][16][16];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int N = a.N, K = a.K;
  const int i0 = (int)blockIdx.x * ETI;
  const int js0 = (int)blockIdx.y * a.slab_rows, js1 = min(N, js0 + a.slab_rows);
  const int pb0 = (int)blockIdx.z * NB, npb = min(NB, a.PB - pb0);
  const bool one_chunk = K <= EKC;
  en_f64x4 acc[NB];
#pragma unroll
  for (int v = 0; v < NB; ++v) acc[v] = en_f64x4{0.0, 0.0, 0.0, 0.0};
  // rows i of columns [kc, kc + kw) -> zi; rows past N are zeros (their sums are left out at the end)
  auto stage_i = [&](int kc, int kw) {
    for (int e = tid; e < ETI * kw; e += EB) {
      const int r = e / kw, c = e - r * kw, row = i0 + r;
      zi[r * EKP + c] = row < N ? a.z[(size_t)row * K + kc + c] : 0.0;
    }
  };
  if (one_chunk) stage_i(0, K);
  const double *myi = zi + (wave * 16 + li) * EKP;
  for (int jb = js0; jb < js1; jb += EJB) {
    double ss[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) ss[u] = 0.0;
    for (int kc = 0; kc < K; kc += EKC) {
      const int kw = min(EKC, K - kc);
      __syncthreads();  // (the block before is read)
      if (!one_chunk) stage_i(kc, kw);
      for (int e = tid; e < EJB * kw; e += EB) {
        const int r = e / kw, c = e - r * kw, row = jb + r;
        zj[r * EKP + c] = row < js1 ? a.z[(size_t)row * K + kc + c] : 0.0;  // (past the slab: the labels staged are 0)
      }
      if (kc == 0)
        for (int e = tid; e < LW * EJB; e += EB) {
          const int k = e / EJB, r = e - k * EJB;
          const bool in = jb + r < js1;
          const uint32_t lo = in && 2 * k < npb ? a.lab[(size_t)(pb0 + 2 * k) * a.Np + jb + r] : 0u;
          const uint32_t hi = in && 2 * k + 1 < npb ? a.lab[(size_t)(pb0 + 2 * k + 1) * a.Np + jb + r] : 0u;
          lj[r * LW + k] = lo | hi << 16;
        }
      __syncthreads();
      for (int c = 0; c < kw; ++c) {
        const double x = myi[c];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const double t = x - zj[(4 * u + lg) * EKP + c];
          ss[u] = fma(t, t, ss[u]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const double d = sqrt(ss[u]);
      // the row's label words in one go, then a B operand of its own per block: nothing waits between the MFMAs
      uint32_t w[LW];
      const uint32_t *lw = lj + (4 * u + lg) * LW;
#pragma unroll
      for (int k = 0; k < LW; ++k) w[k] = lw[k];
      double b[NB];
#pragma unroll
      for (int v = 0; v < NB; ++v) b[v] = __hiloint2double((int)(0u - ((w[v >> 1] >> ((v & 1) * 16 + li)) & 1u)) & 0x3ff00000, 0);
#pragma unroll
      for (int v = 0; v < NB; ++v) acc[v] = __builtin_amdgcn_mfma_f64_16x16x4f64(d, b[v], acc[v], 0, 0, 0);
    }
  }
  // acc[v][reg] = D[i = lg + 4 reg][q = li] of the wavefront's 16 rows.  Per block: the 16 (wavefront, lane group) parts of
  // each label column in red, added in that order
  double *out = a.part + ((size_t)blockIdx.y * a.tiles + blockIdx.x) * 2 * ((size_t)a.PB * 16);
#pragma unroll
  for (int v = 0; v < NB; ++v) {
    if (v < npb) {  // (the same for every lane of the workgroup)
      double sa = 0.0, saa = 0.0;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = i0 + wave * 16 + lg + 4 * reg;
        if (row < N) {
          const double t = acc[v][reg];
          sa += t;
          if ((a.lab[(size_t)(pb0 + v) * a.Np + row] >> li) & 1) saa += t;
        }
      }
      __syncthreads();  // (red of the block before is read)
      red[0][wave * 4 + lg][li] = sa;
      red[1][wave * 4 + lg][li] = saa;
      __syncthreads();
      if (tid < 32) {
        const int which = tid >> 4, q = tid & 15;
        double s = 0.0;
        for (int k = 0; k < 16; ++k) s += red[which][k][q];
        out[(size_t)which * a.PB * 16 + (size_t)(pb0 + v) * 16 + q] = s;
      }
    }
  }
}

// 4. sums[which][q] = the parts of (which, q) over the slabs and tiles in order.  grid = ceil(2 nq / SB)
__global__ void __launch_bounds__(SB) k_energy_reduce(const double *part, int nparts, int nq, double *sums)
{
  const int t = (int)(blockIdx.x * SB + threadIdx.x);
  if (t >= 2 * nq) return;
  double s = 0.0;
  for (int k = 0; k < nparts; ++k) s += part[(size_t)k * 2 * nq + t];
  sums[t] = s;
}

// ---- launch geometry: what the launch below uses and mcx_debug_energy_geometry reports
struct EnergyGeometry {
  int N, Np, tiles, slab_rows, slabs, nq, PB, NB, chunks;
  size_t scratch_bytes;
};
EnergyGeometry energy_geometry(int n_a, int n_b, int nused, int nperm)
{
  EnergyGeometry g;
  g.N = n_a + n_b;
  g.Np = (g.N + EJB - 1) / EJB * EJB;
  g.tiles = (g.N + ETI - 1) / ETI;
  g.slab_rows = ESLAB;
  // (a test knob, as MCX_COMPARE_GROUP_COLS is: rows per slab, rounded down to whole staged blocks)
  if (const char *cap = std::getenv("MCX_ENERGY_SLAB_ROWS")) g.slab_rows = std::max(EJB, std::min(ESLAB, std::atoi(cap) / EJB * EJB));
  g.slabs = (g.N + g.slab_rows - 1) / g.slab_rows;
  g.nq = nperm + 2;
  g.PB = (g.nq + 15) / 16;
  g.NB = 1;  // the label blocks of a chunk: the power of two that holds them all, at most ECH
  while (g.NB < g.PB && g.NB < ECH) g.NB *= 2;
  g.chunks = (g.PB + g.NB - 1) / g.NB;
  const size_t nqp = (size_t)g.PB * 16;
  g.scratch_bytes = (size_t)g.N * (size_t)std::max(nused, 1) * sizeof(double) + (size_t)g.PB * g.Np * sizeof(uint16_t) +
                    (size_t)g.slabs * g.tiles * 2 * nqp * sizeof(double) + 2 * nqp * sizeof(double);
  return g;
}

int energy_spec(const mcx_energy_spec *spec, mcx_energy_spec *s)
{
  *s = spec ? *spec : mcx_energy_spec{0, 0, 999, 0u, 0u};
  if (s->flags & ~(unsigned)(MCX_ENERGY_WITH_LL | MCX_ENERGY_RAW))
    return fail(MCX_ERR_INVALID, "spec.flags = %u: MCX_ENERGY_WITH_LL (1), MCX_ENERGY_RAW (2) or 0", s->flags);
  if (s->nperm < 0 || s->nperm > MCX_ENERGY_MAX_PERM)
    return fail(MCX_ERR_INVALID, "spec.nperm = %d: 0 to %d permutations", s->nperm, (int)MCX_ENERGY_MAX_PERM);
  return MCX_OK;
}

// the rows a side gives: spec's n resolved against the side's rows
int energy_side_n(const char *side, int n, int64_t rows, int *out)
{
  if (n < -1) return fail(MCX_ERR_INVALID, "spec.n_%s = %d: a number of draws, 0 (min(rows, 2048) draws) or -1 (every row)", side, n);
  const int64_t k = n > 0 ? (int64_t)n : n == 0 ? std::min<int64_t>(rows, 2048) : rows;
  if (k < 2 || k > MCX_ENERGY_MAX_SIDE)
    return fail(MCX_ERR_INVALID, "energy: %lld rows of side %s (spec.n_%s = %d of %lld rows), 2 to %d are supported", (long long)k, side, side,
                n, (long long)rows, (int)MCX_ENERGY_MAX_SIDE);
  *out = (int)k;
  return MCX_OK;
}

// what every entry refuses of its two sides before anything is allocated; *n_a and *n_b: the rows each side gives
int energy_sides(int ncol_a, int64_t rows_a, int ncol_b, int64_t rows_b, const mcx_energy_spec &s, int *n_a, int *n_b)
{
  if (ncol_a != ncol_b) return fail(MCX_ERR_INVALID, "energy: A has %d columns and B %d", ncol_a, ncol_b);
  if (rows_a < 1 || rows_b < 1) return fail(MCX_ERR_INVALID, "energy: %lld and %lld rows, at least one each", (long long)rows_a, (long long)rows_b);
  MCXCHK(energy_side_n("a", s.n_a, rows_a, n_a));
  return energy_side_n("b", s.n_b, rows_b, n_b);
}

double ms_since(std::chrono::steady_clock::time_point t0)
{
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// the comparison of two views on stream st (B's memory is ready: its stream is idle, or it is st).  cols, perm_e, sums
// (3 + 2 nperm doubles), ms (ET_N doubles) may each be NULL
int energy_device(hipStream_t st, const StoreView &va, const StoreView &vb, const mcx_energy_spec &s, mcx_energy_result *res,
                  mcx_energy_col *cols, double *perm_e, double *sums_out, double *ms)
{
  const auto t_total = std::chrono::steady_clock::now();
  int n_a = 0, n_b = 0;
  MCXCHK(energy_sides(va.ncol, va.N, vb.ncol, vb.N, s, &n_a, &n_b));
  const int ncol = va.ncol, N = n_a + n_b, P = s.nperm;
  const bool raw = s.flags & MCX_ENERGY_RAW, with_ll = s.flags & MCX_ENERGY_WITH_LL;
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  double host_ms[ET_N] = {};
  StageTimer tm{st, ms, ET_N, {}};
  // 1. the rows
  std::vector<float> rows((size_t)N * ncol);
  MCXCHK(tm.run(ET_GATHER, [&]() -> int {
    MCXCHK(gather_span(st, va, s.n_a >= 0, s.seed, 0, (uint64_t)n_a, rows.data(), nullptr));
    return gather_span(st, vb, s.n_b >= 0, s.seed, s.n_b >= 0 ? (uint64_t)n_a : 0, (uint64_t)n_b, rows.data() + (size_t)n_a * ncol, nullptr);
  }));
  // 2. scale, flags and z
  auto t0 = std::chrono::steady_clock::now();
  std::vector<mcx_energy_col> hc((size_t)ncol);
  std::vector<int> used;
  for (int c = 0; c < ncol; ++c) {
    mcx_energy_col &o = hc[(size_t)c];
    o = mcx_energy_col{qnan, 0};
    if (c == ncol - 1 && !with_ll) {
      o.flags = MCX_ENERGY_COL_UNUSED;
      continue;
    }
    bool finite = true;
    const double sd = EH::column_scale(rows.data() + c, (size_t)N, (size_t)ncol, &finite);
    o.scale = !finite ? qnan : raw ? 1.0 : sd;
    if (!finite) o.flags = MCX_ENERGY_COL_NONFINITE;
    else if (!raw && !(sd > 0.0)) o.flags = MCX_ENERGY_COL_CONSTANT;
    if (!o.flags) used.push_back(c);
  }
  const int K = (int)used.size();
  std::vector<double> z((size_t)N * (size_t)std::max(K, 1));
  for (int i = 0; i < N; ++i)
    for (int k = 0; k < K; ++k) z[(size_t)i * K + k] = (double)rows[(size_t)i * ncol + used[(size_t)k]] / hc[(size_t)used[(size_t)k]].scale;
  host_ms[ET_SCALE] = ms_since(t0);
  *res = mcx_energy_result{};
  res->n_a = n_a;
  res->n_b = n_b;
  res->nperm = P;
  res->nused = K;
  res->na_rows = va.N;
  res->nb_rows = vb.N;
  if (cols) std::copy(hc.begin(), hc.end(), cols);
  std::vector<double> sums(3 + 2 * (size_t)P, qnan);
  if (K > 0) {
    const EnergyGeometry g = energy_geometry(n_a, n_b, K, P);
    const size_t nqp = (size_t)g.PB * 16;
    // the label vectors, bit-packed
    t0 = std::chrono::steady_clock::now();
    std::vector<uint16_t> lab((size_t)g.PB * g.Np, (uint16_t)0);
    {
      // a block of 16 label columns is one piece of work and one stretch of lab: the vectors are functions of (seed, p) alone,
      // so the threads share nothing but the counter
      // Every vector is sized before a thread starts and the threads are joined by a guard: work() allocates nothing
      const int nth = (int)std::max(1u, std::min({std::thread::hardware_concurrency(), 16u, (unsigned)g.PB}));
      std::vector<std::vector<uint8_t>> ls((size_t)nth, std::vector<uint8_t>((size_t)N));
      std::vector<std::vector<uint32_t>> idxs((size_t)nth, std::vector<uint32_t>((size_t)N));
      std::atomic<int> next{0};
      auto work = [&](int t) {
        std::vector<uint8_t> &l = ls[(size_t)t];
        std::vector<uint32_t> &idx = idxs[(size_t)t];
        for (int pb = next.fetch_add(1); pb < g.PB; pb = next.fetch_add(1)) {
          uint16_t *w = lab.data() + (size_t)pb * g.Np;
          for (int q = pb * 16; q < std::min(g.nq, pb * 16 + 16); ++q) {
            const uint16_t bit = (uint16_t)(1u << (q & 15));
            if (q == 0) {  // column 0: ones
              for (int i = 0; i < N; ++i) w[i] |= bit;
              continue;
            }
            EH::labels(s.seed, n_a, n_b, q - 1, l.data(), idx);
            for (int i = 0; i < N; ++i)
              if (l[(size_t)i]) w[i] |= bit;
          }
        }
      };
      struct Joined {
        std::vector<std::thread> th;
        ~Joined()
        {
          for (std::thread &t : th) t.join();
        }
      } J;
      J.th.reserve((size_t)nth);
      try {
        for (int t = 1; t < nth; ++t) J.th.emplace_back(work, t);
      } catch (const std::exception &) {
      }  // (no more threads to be had: those there are share the work)
      work(0);
    }
    host_ms[ET_LABELS] = ms_since(t0);
    DevBuf<double> dz, dpart, dsums;
    DevBuf<uint16_t> dlab;
    std::vector<double> hs(2 * nqp);
    auto run = [&]() -> int {
      MCXCHK(dz.alloc(z.size()));
      MCXCHK(dlab.alloc(lab.size()));
      MCXCHK(dpart.alloc((size_t)g.slabs * g.tiles * 2 * nqp));
      MCXCHK(dsums.alloc(2 * nqp));
      MCXCHK(tm.run(ET_UPLOAD, [&]() -> int {
        HIPCHK(hipMemcpyAsync(dz.p, z.data(), z.size() * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dlab.p, lab.data(), lab.size() * sizeof(uint16_t), hipMemcpyHostToDevice, st));
        return MCX_OK;
      }));
      const EnergyArgs ea{dz.p, dlab.p, N, g.Np, K, g.PB, g.tiles, g.slab_rows, dpart.p};
      MCXCHK(tm.run(ET_PAIRS, [&]() -> int {
        const dim3 grid((unsigned)g.tiles, (unsigned)g.slabs, (unsigned)g.chunks);
        switch (g.NB) {
        case 1: hipLaunchKernelGGL(k_energy_pairs<1>, grid, dim3(EB), 0, st, ea); break;
        case 2: hipLaunchKernelGGL(k_energy_pairs<2>, grid, dim3(EB), 0, st, ea); break;
        case 4: hipLaunchKernelGGL(k_energy_pairs<4>, grid, dim3(EB), 0, st, ea); break;
        case 8: hipLaunchKernelGGL(k_energy_pairs<8>, grid, dim3(EB), 0, st, ea); break;
        default: hipLaunchKernelGGL(k_energy_pairs<ECH>, grid, dim3(EB), 0, st, ea); break;
        }
        HIPCHK(hipGetLastError());
        return MCX_OK;
      }));
      MCXCHK(tm.run(ET_REDUCE, [&]() -> int {
        hipLaunchKernelGGL(k_energy_reduce, dim3((unsigned)((2 * nqp + SB - 1) / SB)), dim3(SB), 0, st, (const double *)dpart.p,
                           g.slabs * g.tiles, (int)nqp, dsums.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hs.data(), dsums.p, hs.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        return MCX_OK;
      }));
      HIPCHK(hipStreamSynchronize(st));
      return MCX_OK;
    };
    const int rc = run();
    if (rc != MCX_OK) (void)hipStreamSynchronize(st);  // (z, lab, hs and the scratch are the stream's until here)
    MCXCHK(rc);
    sums[0] = hs[0];  // S_A of the column of ones
    for (int p = 0; p <= P; ++p) {
      sums[1 + 2 * (size_t)p] = hs[(size_t)p + 1];
      sums[2 + 2 * (size_t)p] = hs[nqp + (size_t)p + 1];
    }
  }
  // (no column left: finish() gives NaN everywhere, perm_e included)
  const EH::Finish f = EH::finish(K > 0 ? sums.data() : nullptr, n_a, n_b, P, perm_e);
  res->e = f.e; res->h = f.h; res->mean_ab = f.mean_ab; res->mean_aa = f.mean_aa; res->mean_bb = f.mean_bb;
  res->p_value = f.p_value;
  res->nge = f.nge;
  if (sums_out) std::copy(sums.begin(), sums.end(), sums_out);
  MCXCHK(tm.collect());
  if (ms) {
    ms[ET_SCALE] = host_ms[ET_SCALE];
    ms[ET_LABELS] = host_ms[ET_LABELS];
    ms[ET_TOTAL] = ms_since(t_total);
  }
  return MCX_OK;
}

int engine_range(const mcx_engine *e, int first, int nsteps, const char *side)
{
  if (first < 0 || (int64_t)first + nsteps > e->samp_steps)
    return fail(MCX_ERR_INVALID, "%s: steps [%d,%lld) not in the sample store (%d steps)", side, first, (long long)first + nsteps,
                e->samp_steps);
  return MCX_OK;
}

int samples_energy(mcx_engine *e, int first_a, int nsteps_a, int first_b, int nsteps_b, const mcx_energy_spec *spec,
                   mcx_energy_result *res, mcx_energy_col *cols, double *perm_e, double *ms)
{
  mcx_energy_spec s;
  return on_store(
      e, first_a, nsteps_a,
      [&]() -> int {
        if (!res) return fail(MCX_ERR_INVALID, "res is NULL");
        MCXCHK(energy_spec(spec, &s));
        if (nsteps_a < 1 || nsteps_b < 1)
          return fail(MCX_ERR_INVALID, "nsteps_a = %d, nsteps_b = %d: ranges of at least one step", nsteps_a, nsteps_b);
        int n_a, n_b;
        return energy_sides(e->nparam + 1, (int64_t)nsteps_a * e->nchain, e->nparam + 1, (int64_t)nsteps_b * e->nchain, s, &n_a, &n_b);
      },
      [&](hipStream_t st, Bufs, const StoreView &va) {
        MCXCHK(engine_range(e, first_b, nsteps_b, "B"));
        const size_t nc = (size_t)e->nchain, np = (size_t)e->nparam;
        const StoreView vb(StoreSpan{e->samp_x.p + (size_t)first_b * nc * np, e->samp_ly.p + (size_t)first_b * nc, (int)nc, (int)np, nsteps_b});
        return energy_device(st, va, vb, s, res, cols, perm_e, nullptr, ms);
      });
}

int rows_energy(const float *rows_a, int nsteps_a, int nc_a, const float *rows_b, int nsteps_b, int nc_b, int np,
                const mcx_energy_spec *spec, mcx_energy_result *res, mcx_energy_col *cols, double *perm_e, double *sums)
{
  if (!rows_a || !rows_b) return fail(MCX_ERR_INVALID, "rows_%s is NULL", rows_a ? "b" : "a");
  if (!res) return fail(MCX_ERR_INVALID, "res is NULL");
  mcx_energy_spec s;
  MCXCHK(energy_spec(spec, &s));
  if (np < 1 || np > 256) return fail(MCX_ERR_INVALID, "np = %d: 1 to 256 parameters", np);
  if (nsteps_a < 1 || nc_a < 1 || nsteps_b < 1 || nc_b < 1)
    return fail(MCX_ERR_INVALID, "A is %d steps of %d chains, B %d of %d: at least one step of one chain each", nsteps_a, nc_a, nsteps_b, nc_b);
  int n_a, n_b;
  MCXCHK(energy_sides(np + 1, (int64_t)nsteps_a * nc_a, np + 1, (int64_t)nsteps_b * nc_b, s, &n_a, &n_b));
  return on_rows(rows_a, nsteps_a, nc_a, np, [&](hipStream_t st, Bufs, const StoreView &va) {
    return on_rows(rows_b, nsteps_b, nc_b, np, [&](hipStream_t stb, Bufs, const StoreView &vb) {
      HIPCHK(hipStreamSynchronize(stb));  // B's upload
      return energy_device(st, va, vb, s, res, cols, perm_e, sums, nullptr);
    });
  });
}

}  // namespace

extern "C" int mcx_store_energy(mcx_store *a, mcx_store *b, const mcx_energy_spec *spec, mcx_energy_result *res, mcx_energy_col *cols,
                                double *perm_e)
{
  if (!a || !b) return fail(MCX_ERR_INVALID, "the store %s is NULL", a ? "b" : "a");
  if (!res) return fail(MCX_ERR_INVALID, "res is NULL");
  mcx_energy_spec s;
  MCXCHK(energy_spec(spec, &s));
  int n_a, n_b;
  MCXCHK(energy_sides(a->nout + 1, (int64_t)a->T * a->nc, b->nout + 1, (int64_t)b->T * b->nc, s, &n_a, &n_b));
  if (a->device != b->device) return fail(MCX_ERR_INVALID, "energy: A is on device %d and B on device %d", a->device, b->device);
  HIPCHK(hipSetDevice(a->device));
  if (b != a && b->st) HIPCHK(hipStreamSynchronize(b->st));
  return energy_device(a->st, StoreView(a->span()), StoreView(b->span()), s, res, cols, perm_e, nullptr, nullptr);
}

extern "C" int mcx_rows_energy(const float *rows_a, int nsteps_a, int nc_a, const float *rows_b, int nsteps_b, int nc_b, int np,
                               const mcx_energy_spec *spec, mcx_energy_result *res, mcx_energy_col *cols, double *perm_e)
{
  return rows_energy(rows_a, nsteps_a, nc_a, rows_b, nsteps_b, nc_b, np, spec, res, cols, perm_e, nullptr);
}

extern "C" int mcx_debug_energy_sums(const float *rows_a, int nsteps_a, int nc_a, const float *rows_b, int nsteps_b, int nc_b, int np,
                                     const mcx_energy_spec *spec, double *sums)
{
  if (!sums) return fail(MCX_ERR_INVALID, "sums is NULL");
  mcx_energy_result res;
  return rows_energy(rows_a, nsteps_a, nc_a, rows_b, nsteps_b, nc_b, np, spec, &res, nullptr, nullptr, sums);
}

extern "C" int mcx_samples_energy(mcx_engine *e, int first_a, int nsteps_a, int first_b, int nsteps_b, const mcx_energy_spec *spec,
                                  mcx_energy_result *res, mcx_energy_col *cols, double *perm_e)
{
  return samples_energy(e, first_a, nsteps_a, first_b, nsteps_b, spec, res, cols, perm_e, nullptr);
}

extern "C" int mcx_debug_energy_times(mcx_engine *e, int first_a, int nsteps_a, int first_b, int nsteps_b, const mcx_energy_spec *spec,
                                      double *ms)
{
  if (!ms) return fail(MCX_ERR_INVALID, "ms is NULL");
  mcx_energy_result res;
  return samples_energy(e, first_a, nsteps_a, first_b, nsteps_b, spec, &res, nullptr, nullptr, ms);
}

extern "C" int mcx_samples_energy_store(mcx_engine *e, int first_step, int nsteps, mcx_store *b, const mcx_energy_spec *spec,
                                        mcx_energy_result *res, mcx_energy_col *cols, double *perm_e)
{
  mcx_energy_spec s;
  return on_store(
      e, first_step, nsteps,
      [&]() -> int {
        if (!b) return fail(MCX_ERR_INVALID, "the store b is NULL");
        if (!res) return fail(MCX_ERR_INVALID, "res is NULL");
        MCXCHK(energy_spec(spec, &s));
        if (nsteps < 1) return fail(MCX_ERR_INVALID, "nsteps = %d: a range of at least one step", nsteps);
        int n_a, n_b;
        MCXCHK(energy_sides(e->nparam + 1, (int64_t)nsteps * e->nchain, b->nout + 1, (int64_t)b->T * b->nc, s, &n_a, &n_b));
        if (e->device != b->device) return fail(MCX_ERR_INVALID, "energy: the engine is on device %d and B on device %d", e->device, b->device);
        return MCX_OK;
      },
      [&](hipStream_t st, Bufs, const StoreView &va) {
        if (b->st) HIPCHK(hipStreamSynchronize(b->st));
        return energy_device(st, va, StoreView(b->span()), s, res, cols, perm_e, nullptr, nullptr);
      });
}

// host only
extern "C" int mcx_debug_energy_labels(uint32_t seed, int n_a, int n_b, int p, uint8_t *labels)
{
  if (!labels) return fail(MCX_ERR_INVALID, "labels is NULL");
  if (n_a < 1 || n_b < 1 || n_a > MCX_ENERGY_MAX_SIDE || n_b > MCX_ENERGY_MAX_SIDE)
    return fail(MCX_ERR_INVALID, "n_a = %d, n_b = %d: 1 to %d rows a side", n_a, n_b, (int)MCX_ENERGY_MAX_SIDE);
  if (p < 0 || p > MCX_ENERGY_MAX_PERM) return fail(MCX_ERR_INVALID, "p = %d: 0 to %d", p, (int)MCX_ENERGY_MAX_PERM);
  std::vector<uint32_t> idx;
  EH::labels(seed, n_a, n_b, p, labels, idx);
  return MCX_OK;
}

// host only
extern "C" int mcx_debug_energy_geometry(int n_a, int n_b, int nused, int nperm, mcx_energy_geometry *g)
{
  if (!g) return fail(MCX_ERR_INVALID, "g is NULL");
  if (n_a < 2 || n_b < 2 || n_a > MCX_ENERGY_MAX_SIDE || n_b > MCX_ENERGY_MAX_SIDE)
    return fail(MCX_ERR_INVALID, "n_a = %d, n_b = %d: 2 to %d rows a side", n_a, n_b, (int)MCX_ENERGY_MAX_SIDE);
  if (nused < 1 || nused > 257) return fail(MCX_ERR_INVALID, "nused = %d: 1 to 257 columns", nused);
  if (nperm < 0 || nperm > MCX_ENERGY_MAX_PERM) return fail(MCX_ERR_INVALID, "nperm = %d: 0 to %d permutations", nperm, (int)MCX_ENERGY_MAX_PERM);
  const EnergyGeometry c = energy_geometry(n_a, n_b, nused, nperm);
  g->block = EB;
  g->tile_rows = ETI;
  g->tiles = c.tiles;
  g->slab_rows = c.slab_rows;
  g->slabs = c.slabs;
  g->label_cols = c.nq;
  g->label_blocks = c.PB;
  g->chunk_blocks = c.NB;
  g->chunks = c.chunks;
  g->col_chunk = EKC;
  g->workgroups = (long long)c.tiles * c.slabs * c.chunks;
  g->lds_bytes = (long long)((ETI + EJB) * EKP * sizeof(double) + std::max(c.NB / 2, 1) * EJB * sizeof(uint32_t) + 2 * 16 * 16 * sizeof(double));
  g->scratch_bytes = (long long)c.scratch_bytes;
  return MCX_OK;
}
