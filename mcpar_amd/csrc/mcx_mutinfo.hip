// mcx_mutinfo.hip -- mcx_*_mutinfo: the mutual information of every column pair of a store by the k-nearest-neighbour estimator
// of Kraskov, Stoegbauer and Grassberger, with a permutation null.  The work is every pairwise distance of
// the m points, twice, per column pair and per permutation: plain fp64 subtract, maximum and compare on the vector unit.
//   1. gather_spaced       the n evenly spaced rows to the host (mcx_derive.hip)
//   2. host                scale and flags per column, the repeated rows dropped, z = x / scale column-major [c][m]; the
//                          permutations pi_1 ... pi_nperm as 16-bit indices; the table psi(1) ... psi(m) (mcx_mutinfo_host.hpp)
//   3. k_mi_pairs          grid = (tiles of MTI queries, pairs, 1 + nperm).  A lane owns MQ queries (u_i, v_i).  The m points
//                          (u_j, v_j), v gathered through pi_p, go through LDS a stage at a time; every lane reads the same
//                          point (a broadcast) and serves its MQ queries from it.  Sweep 1 keeps the k smallest joint distances
//                          of each query in registers, sweep 2 counts na and nb below the k-th; psi from the table, the
//                          workgroup's sum in a fixed tree -> part[perm][pair][tile][2] (the sum, and #{eps = 0})
//   4. k_mi_reduce         one thread per (perm, pair, which) walks the tiles in order
// No atomics; every word of the scratch that is read was uploaded or written earlier in the same call.
#include "mcx_store.hpp"

#include "mcx_mutinfo_host.hpp"

#include <atomic>
#include <chrono>
#include <exception>
#include <limits>
#include <thread>

namespace {

namespace MH = mcx_mutinfo_host;

static_assert((int)MH::COL_NONFINITE == (int)MCX_MUTINFO_COL_NONFINITE && (int)MH::COL_CONSTANT == (int)MCX_MUTINFO_COL_CONSTANT &&
                  (int)MH::COL_UNUSED == (int)MCX_MUTINFO_COL_UNUSED && (int)MH::PAIR_UNUSED == (int)MCX_MUTINFO_PAIR_UNUSED &&
                  (int)MH::PAIR_FEW == (int)MCX_MUTINFO_PAIR_FEW && (int)MH::PAIR_TIES == (int)MCX_MUTINFO_PAIR_TIES,
              "mcx_mutinfo_host.hpp restates include/mcx.h's flags");

constexpr int MB = 256;        // threads of a k_mi_pairs workgroup: four wavefronts
constexpr int MQ = 2;          // queries of a lane: a staged point is read once and serves both
constexpr int MTI = MB * MQ;   // queries of a workgroup
constexpr int MST = 1024;      // points staged at a time (MCX_MUTINFO_STAGE_ROWS lowers it): 16 KiB
constexpr int MAXCOLS = 45;    // used columns up to which the default is every pair (section 15's rule)
enum { MT_GATHER = 0, MT_POINTS, MT_PERMS, MT_UPLOAD, MT_PAIRS, MT_REDUCE, MT_FINISH, MT_TOTAL, MT_N };

struct MiArgs {
  const double *z;       // [ncol][m], column-major
  const uint16_t *perm;  // [nperm][m]: pi_1 ... pi_nperm (pi_0 is the identity and is not stored)
  const int *pairs;      // [pairs][2]: the columns of the pairs that are computed
  const double *psi;     // [m]: psi[q] = psi(q + 1)
  int m, npairs, tiles, stage_rows;
  int pair0, p0;         // added to blockIdx.y and .z: mcx_debug_mutinfo_counts launches one (pair, permutation)
  double *part;          // [1 + nperm][pairs][tiles][2], or NULL
  double *eps;           // [m] each or NULL: the kernel's own integers, for the tests
  int *na, *nb;
};

// one stage of points against the lane's queries.  CHECK: the stage holds points of this workgroup's own tile, so j = i is
// looked for (by index, not by distance); the other stages run without that compare.  SWEEP 1: best[q] holds the K smallest
// joint distances so far, ascending; a new one goes in behind one compare against the K-th.  SWEEP 2: counts below eps[q]
template <int K, int SWEEP, bool CHECK>
__device__ __forceinline__ void mi_point(const double2 pt, int j, const int (&qi)[MQ], const double (&qu)[MQ], const double (&qv)[MQ],
                                         double (&best)[MQ][K], int (&ca)[MQ], int (&cb)[MQ])
{
#pragma unroll
  for (int q = 0; q < MQ; ++q) {
    const double da = fabs(qu[q] - pt.x), db = fabs(qv[q] - pt.y);
    const bool other = !CHECK || j != qi[q];
    if (SWEEP == 1) {
      const double d = fmax(da, db);
      if (other && d < best[q][K - 1]) {
        best[q][K - 1] = d;
#pragma unroll
        for (int t = K - 1; t > 0; --t) {
          const double lo = fmin(best[q][t - 1], best[q][t]), hi = fmax(best[q][t - 1], best[q][t]);
          best[q][t - 1] = lo;
          best[q][t] = hi;
        }
      }
    } else {
      const double e = best[q][K - 1];
      ca[q] += (other && da < e) ? 1 : 0;
      cb[q] += (other && db < e) ? 1 : 0;
    }
  }
}
// (MU points are read before the first is used, so that a wavefront does not wait for every read in turn)
template <int K, int SWEEP, bool CHECK>
__device__ __forceinline__ void mi_visit(const double2 *pts, int j0, int cnt, const int (&qi)[MQ], const double (&qu)[MQ],
                                         const double (&qv)[MQ], double (&best)[MQ][K], int (&ca)[MQ], int (&cb)[MQ])
{
  constexpr int MU = 4;
  int jj = 0;
  for (; jj + MU <= cnt; jj += MU) {
    double2 pt[MU];
#pragma unroll
    for (int u = 0; u < MU; ++u) pt[u] = pts[jj + u];
#pragma unroll
    for (int u = 0; u < MU; ++u) mi_point<K, SWEEP, CHECK>(pt[u], j0 + jj + u, qi, qu, qv, best, ca, cb);
  }
  for (; jj < cnt; ++jj) mi_point<K, SWEEP, CHECK>(pts[jj], j0 + jj, qi, qu, qv, best, ca, cb);
}

// 3. grid = (tiles, pairs, 1 + nperm); with a.eps one (pair, permutation): grid = (tiles, 1, 1)
template <int K>
__global__ void __launch_bounds__(MB) k_mi_pairs(const MiArgs a)
{
  __shared__ double2 pts[MST];
  __shared__ double red[2][MB];
  const int tid = (int)threadIdx.x, m = a.m;
  const int tile = (int)blockIdx.x, pair = a.pair0 + (int)blockIdx.y, p = a.p0 + (int)blockIdx.z;
  const double *za = a.z + (size_t)a.pairs[2 * pair] * (size_t)m, *zb = a.z + (size_t)a.pairs[2 * pair + 1] * (size_t)m;
  const uint16_t *pi = p > 0 ? a.perm + (size_t)(p - 1) * (size_t)m : nullptr;
  const int i0 = tile * MTI;
  int qi[MQ], ca[MQ], cb[MQ];
  double qu[MQ], qv[MQ], best[MQ][K];
#pragma unroll
  for (int q = 0; q < MQ; ++q) {
    qi[q] = i0 + q * MB + tid;
    const int i = min(qi[q], m - 1);  // (a query past m reads the last point; nothing of it is kept)
    qu[q] = za[i];
    qv[q] = zb[pi ? (int)pi[i] : i];
    ca[q] = cb[q] = 0;
#pragma unroll
    for (int t = 0; t < K; ++t) best[q][t] = __builtin_inf();
  }
  const int S = a.stage_rows;
  const bool one_stage = m <= S;
  auto stage = [&](int j0, int cnt) {
    __syncthreads();  // (the stage before is read)
    for (int e = tid; e < cnt; e += MB) {
      const int j = j0 + e;
      pts[e] = double2{za[j], zb[pi ? (int)pi[j] : j]};
    }
    __syncthreads();
  };
  for (int j0 = 0; j0 < m; j0 += S) {
    const int cnt = min(S, m - j0);
    stage(j0, cnt);
    if (j0 < i0 + MTI && j0 + cnt > i0) mi_visit<K, 1, true>(pts, j0, cnt, qi, qu, qv, best, ca, cb);
    else mi_visit<K, 1, false>(pts, j0, cnt, qi, qu, qv, best, ca, cb);
  }
  for (int j0 = 0; j0 < m; j0 += S) {
    const int cnt = min(S, m - j0);
    if (!one_stage) stage(j0, cnt);  // (one stage: it is still there)
    if (j0 < i0 + MTI && j0 + cnt > i0) mi_visit<K, 2, true>(pts, j0, cnt, qi, qu, qv, best, ca, cb);
    else mi_visit<K, 2, false>(pts, j0, cnt, qi, qu, qv, best, ca, cb);
  }
  double s = 0.0, nz = 0.0;
#pragma unroll
  for (int q = 0; q < MQ; ++q)
    if (qi[q] < m) {
      s += a.psi[ca[q]] + a.psi[cb[q]];  // ca, cb <= m - 1
      if (best[q][K - 1] == 0.0) nz += 1.0;
      if (a.eps) {
        a.eps[qi[q]] = best[q][K - 1];
        a.na[qi[q]] = ca[q];
        a.nb[qi[q]] = cb[q];
      }
    }
  if (!a.part) return;  // (the same for every lane)
  red[0][tid] = s;
  red[1][tid] = nz;
  __syncthreads();
  for (int w = MB / 2; w > 0; w >>= 1) {
    if (tid < w) {
      red[0][tid] += red[0][tid + w];
      red[1][tid] += red[1][tid + w];
    }
    __syncthreads();
  }
  if (tid < 2) a.part[(((size_t)p * a.npairs + pair) * a.tiles + tile) * 2 + tid] = red[tid][0];
}

// 4. sums[(perm, pair)][which] = the parts of its tiles in order.  grid = ceil(2 nq / SB)
__global__ void __launch_bounds__(SB) k_mi_reduce(const double *part, int tiles, int nq, double *sums)
{
  const int t = (int)(blockIdx.x * SB + threadIdx.x);
  if (t >= 2 * nq) return;
  const size_t r = (size_t)(t >> 1);
  double s = 0.0;
  for (int k = 0; k < tiles; ++k) s += part[(r * tiles + k) * 2 + (t & 1)];
  sums[t] = s;
}

template <int K> void launch_pairs(dim3 grid, hipStream_t st, const MiArgs &a) { hipLaunchKernelGGL(k_mi_pairs<K>, grid, dim3(MB), 0, st, a); }

// ---- launch geometry: what the launch below uses and mcx_debug_mutinfo_geometry reports
struct MiGeometry {
  int tiles, stage_rows, stages;
  size_t scratch_bytes;
};
MiGeometry mutinfo_geometry(int m, int npairs, int nperm)
{
  MiGeometry g;
  g.tiles = (m + MTI - 1) / MTI;
  g.stage_rows = MST;
  // (a test knob, as MCX_ENERGY_SLAB_ROWS is: points per stage, rounded down to whole wavefronts)
  if (const char *cap = std::getenv("MCX_MUTINFO_STAGE_ROWS")) g.stage_rows = std::max(64, std::min(MST, std::atoi(cap) / 64 * 64));
  g.stages = (m + g.stage_rows - 1) / g.stage_rows;
  const size_t nq = (size_t)(1 + nperm) * (size_t)npairs;
  g.scratch_bytes = (size_t)nperm * m * sizeof(uint16_t) + (size_t)m * sizeof(double) + (size_t)npairs * 2 * sizeof(int) +
                    nq * g.tiles * 2 * sizeof(double) + nq * 2 * sizeof(double);
  return g;
}

// ---- what every entry refuses before anything is allocated
int mutinfo_spec(const mcx_mutinfo_spec *spec, mcx_mutinfo_spec *s)
{
  *s = spec ? *spec : mcx_mutinfo_spec{0, 0, 0, 0u, 0u, 0, nullptr};
  if (s->flags & ~(unsigned)(MCX_MUTINFO_WITH_LL | MCX_MUTINFO_RAW))
    return fail(MCX_ERR_INVALID, "spec.flags = %u: MCX_MUTINFO_WITH_LL (1), MCX_MUTINFO_RAW (2) or 0", s->flags);
  if (s->k < 0 || s->k > MCX_MUTINFO_MAX_K) return fail(MCX_ERR_INVALID, "spec.k = %d: 1 to %d neighbours, or 0 for 3", s->k, (int)MCX_MUTINFO_MAX_K);
  if (s->k == 0) s->k = 3;
  if (s->nperm < 0 || s->nperm > MCX_MUTINFO_MAX_PERM)
    return fail(MCX_ERR_INVALID, "spec.nperm = %d: 0 to %d permutations", s->nperm, (int)MCX_MUTINFO_MAX_PERM);
  return MCX_OK;
}

// spec.n resolved against the N rows of the view
int mutinfo_rows_n(int n, int64_t N, int *out)
{
  if (n < -1) return fail(MCX_ERR_INVALID, "spec.n = %d: a number of rows, 0 (min(rows, 4096)) or -1 (every row)", n);
  const int64_t k = n > 0 ? (int64_t)n : n == 0 ? std::min<int64_t>(N, 4096) : N;
  if (k < 2 || k > MCX_MUTINFO_MAX_ROWS || k > N)
    return fail(MCX_ERR_INVALID, "mutual information: %lld rows (spec.n = %d of %lld rows), 2 to %d of the store's are supported", (long long)k, n,
                (long long)N, (int)MCX_MUTINFO_MAX_ROWS);
  *out = (int)k;
  return MCX_OK;
}

// the pairs of a call over ncol columns: *npairs, and with list the pairs themselves
int mutinfo_pairs(const mcx_mutinfo_spec &s, int ncol, int *npairs, std::vector<int> *list)
{
  const int U = ncol - ((s.flags & MCX_MUTINFO_WITH_LL) ? 0 : 1);  // the used columns are 0 ... U - 1
  if (!s.pairs) {
    if (s.npairs != 0) return fail(MCX_ERR_INVALID, "spec.npairs = %d with spec.pairs NULL", s.npairs);
    if (U < 2) return fail(MCX_ERR_INVALID, "mutual information: %d used column, a pair takes two (MCX_MUTINFO_WITH_LL adds log L)", U);
    if (U > MAXCOLS)
      return fail(MCX_ERR_INVALID, "mutual information: %d used columns, every pair is the default up to %d: name the pairs (spec.pairs)", U, MAXCOLS);
    *npairs = U * (U - 1) / 2;
    if (list) {
      list->clear();
      for (int a = 0; a < U; ++a)
        for (int b = a + 1; b < U; ++b) {
          list->push_back(a);
          list->push_back(b);
        }
    }
    return MCX_OK;
  }
  if (s.npairs < 1 || s.npairs > MCX_MUTINFO_MAX_PAIRS)
    return fail(MCX_ERR_INVALID, "spec.npairs = %d: 1 to %d pairs", s.npairs, (int)MCX_MUTINFO_MAX_PAIRS);
  for (int i = 0; i < s.npairs; ++i) {
    const int a = s.pairs[2 * i], b = s.pairs[2 * i + 1];
    if (a < 0 || b < 0 || a >= U || b >= U || a == b)
      return fail(MCX_ERR_INVALID, "spec.pairs[%d] = (%d, %d): two different columns of the %d used", i, a, b, U);
  }
  *npairs = s.npairs;
  if (list) list->assign(s.pairs, s.pairs + 2 * (size_t)s.npairs);
  return MCX_OK;
}

// all of it for a view of ncol columns and N rows; *n and *npairs as the call will have them
int mutinfo_args(const mcx_mutinfo_spec *spec, mcx_mutinfo_spec *s, int ncol, int64_t N, int *n, int *npairs)
{
  MCXCHK(mutinfo_spec(spec, s));
  MCXCHK(mutinfo_rows_n(s->n, N, n));
  return mutinfo_pairs(*s, ncol, npairs, nullptr);
}

double ms_since(std::chrono::steady_clock::time_point t0)
{
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// the m kept points' permutations pi_1 ... pi_nperm -> perm[nperm][m]: functions of (seed, p) alone, so the threads share
// nothing but the counter.  Everything is sized before a thread starts and the threads are joined by a guard
void make_perms(uint32_t seed, int m, int nperm, uint16_t *perm)
{
  if (nperm < 1) return;
  const int nth = (int)std::max(1u, std::min({std::thread::hardware_concurrency(), 16u, (unsigned)((nperm + 7) / 8)}));
  std::atomic<int> next{1};
  auto work = [&]() {
    for (int p = next.fetch_add(1); p <= nperm; p = next.fetch_add(1)) MH::permutation(seed, m, p, perm + (size_t)(p - 1) * (size_t)m);
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
    for (int t = 1; t < nth; ++t) J.th.emplace_back(work);
  } catch (const std::exception &) {
  }  // (no more threads to be had: those there are share the work)
  work();
}

// the selected rows of a host array: what gather_spaced gives from the device
void select_rows(const float *rows, int64_t N, int ncol, int n, float *sel, long long *index)
{
  for (int i = 0; i < n; ++i) {
    const int64_t r = MH::row_index(N, n, i);
    if (index) index[i] = (long long)r;
    if (sel) std::copy(rows + (size_t)r * ncol, rows + (size_t)(r + 1) * ncol, sel + (size_t)i * ncol);
  }
}

struct MiDebug {
  int pair, p;
  double *eps;
  int *na, *nb;
};

// the analysis of a view on stream st.  cols, perm_mi, ms (MT_N doubles) may be NULL; dbg: mcx_debug_mutinfo_counts' one
// (pair, permutation), whose eps, na, nb are written and nothing else
int mutinfo_device(hipStream_t st, const StoreView &v, const mcx_mutinfo_spec &s, mcx_mutinfo_result *res, mcx_mutinfo_col *cols,
                   mcx_mutinfo_pair *pairs_out, double *perm_mi, const MiDebug *dbg, double *ms)
{
  const auto t_total = std::chrono::steady_clock::now();
  int n = 0, npairs = 0;
  std::vector<int> list;
  MCXCHK(mutinfo_rows_n(s.n, v.N, &n));
  MCXCHK(mutinfo_pairs(s, v.ncol, &npairs, &list));
  const int ncol = v.ncol, P = s.nperm, k = s.k;
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  double host_ms[MT_N] = {};
  StageTimer tm{st, ms, MT_N, {}};
  // 1. the rows
  std::vector<float> sel((size_t)n * ncol);
  MCXCHK(tm.run(MT_GATHER, [&]() -> int { return gather_spaced(st, v, (uint64_t)n, sel.data()); }));
  // 2. scale, flags, repeats and z
  auto t0 = std::chrono::steady_clock::now();
  MH::Points pt;
  MH::points(sel.data(), n, ncol, s.flags & MCX_MUTINFO_WITH_LL, s.flags & MCX_MUTINFO_RAW, pt);
  host_ms[MT_POINTS] = ms_since(t0);
  const int m = pt.m;
  *res = mcx_mutinfo_result{(long long)v.N, n, pt.ndup, m, k, npairs, P, pt.nused};
  if (cols)
    for (int c = 0; c < ncol; ++c) cols[c] = mcx_mutinfo_col{pt.scale[(size_t)c], pt.flags[(size_t)c]};
  // the pairs that are computed, in the order of the call's list
  std::vector<int> act, act_of((size_t)npairs, -1);
  for (int i = 0; i < npairs; ++i) {
    const int a = list[2 * (size_t)i], b = list[2 * (size_t)i + 1];
    mcx_mutinfo_pair &o = pairs_out[i];
    o = mcx_mutinfo_pair{a, b, qnan, qnan, qnan, qnan, qnan, qnan, 0, 0, 0};
    if (pt.flags[(size_t)a] || pt.flags[(size_t)b]) o.flags |= MCX_MUTINFO_PAIR_UNUSED;
    if (m <= k) o.flags |= MCX_MUTINFO_PAIR_FEW;
    if (!o.flags) {
      act_of[(size_t)i] = (int)act.size() / 2;
      act.push_back(a);
      act.push_back(b);
    }
  }
  if (perm_mi) std::fill(perm_mi, perm_mi + (size_t)npairs * P, qnan);
  const int nact = (int)act.size() / 2;
  if (dbg && (dbg->pair < 0 || dbg->pair >= npairs || act_of[(size_t)dbg->pair] < 0))
    return fail(MCX_ERR_INVALID, "pair = %d: a pair of the call's %d that is computed (no flagged column, m = %d > k = %d)", dbg->pair, npairs, m, k);
  if (nact > 0) {
    const MiGeometry g = mutinfo_geometry(m, nact, P);
    const size_t nq = (size_t)(1 + P) * (size_t)nact;
    t0 = std::chrono::steady_clock::now();
    std::vector<uint16_t> perm((size_t)P * (size_t)m);
    make_perms(s.seed, m, P, perm.data());
    std::vector<double> table((size_t)m);
    MH::psi_table(m, table.data());
    host_ms[MT_PERMS] = ms_since(t0);
    DevBuf<double> dz, dpsi, dpart, dsums, deps;
    DevBuf<uint16_t> dperm;
    DevBuf<int> dpairs, dna, dnb;
    std::vector<double> hs(2 * nq);
    auto run = [&]() -> int {
      MCXCHK(dz.alloc(pt.z.size()));
      MCXCHK(dpsi.alloc(table.size()));
      MCXCHK(dpairs.alloc(act.size()));
      if (P > 0) MCXCHK(dperm.alloc(perm.size()));
      if (dbg) {
        MCXCHK(deps.alloc((size_t)m));
        MCXCHK(dna.alloc((size_t)m));
        MCXCHK(dnb.alloc((size_t)m));
      } else {
        MCXCHK(dpart.alloc(nq * g.tiles * 2));
        MCXCHK(dsums.alloc(2 * nq));
      }
      MCXCHK(tm.run(MT_UPLOAD, [&]() -> int {
        HIPCHK(hipMemcpyAsync(dz.p, pt.z.data(), pt.z.size() * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dpsi.p, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dpairs.p, act.data(), act.size() * sizeof(int), hipMemcpyHostToDevice, st));
        if (P > 0) HIPCHK(hipMemcpyAsync(dperm.p, perm.data(), perm.size() * sizeof(uint16_t), hipMemcpyHostToDevice, st));
        return MCX_OK;
      }));
      MiArgs ma{dz.p, dperm.p, dpairs.p, dpsi.p, m, nact, g.tiles, g.stage_rows, 0, 0, dpart.p, nullptr, nullptr, nullptr};
      dim3 grid((unsigned)g.tiles, (unsigned)nact, (unsigned)(1 + P));
      if (dbg) {
        ma.pair0 = act_of[(size_t)dbg->pair];
        ma.p0 = dbg->p;
        ma.part = nullptr;
        ma.eps = deps.p;
        ma.na = dna.p;
        ma.nb = dnb.p;
        grid = dim3((unsigned)g.tiles, 1u, 1u);
      }
      MCXCHK(tm.run(MT_PAIRS, [&]() -> int {
        switch (k) {
        case 1: launch_pairs<1>(grid, st, ma); break;
        case 2: launch_pairs<2>(grid, st, ma); break;
        case 3: launch_pairs<3>(grid, st, ma); break;
        case 4: launch_pairs<4>(grid, st, ma); break;
        case 5: launch_pairs<5>(grid, st, ma); break;
        case 6: launch_pairs<6>(grid, st, ma); break;
        case 7: launch_pairs<7>(grid, st, ma); break;
        default: launch_pairs<8>(grid, st, ma); break;
        }
        HIPCHK(hipGetLastError());
        return MCX_OK;
      }));
      if (dbg) {
        HIPCHK(hipMemcpyAsync(dbg->eps, deps.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(dbg->na, dna.p, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(dbg->nb, dnb.p, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, st));
      } else {
        MCXCHK(tm.run(MT_REDUCE, [&]() -> int {
          hipLaunchKernelGGL(k_mi_reduce, dim3((unsigned)((2 * nq + SB - 1) / SB)), dim3(SB), 0, st, (const double *)dpart.p, g.tiles, (int)nq,
                             dsums.p);
          HIPCHK(hipGetLastError());
          HIPCHK(hipMemcpyAsync(hs.data(), dsums.p, hs.size() * sizeof(double), hipMemcpyDeviceToHost, st));
          return MCX_OK;
        }));
      }
      HIPCHK(hipStreamSynchronize(st));
      return MCX_OK;
    };
    const int rc = run();
    if (rc != MCX_OK) (void)hipStreamSynchronize(st);  // (the host vectors and the scratch are the stream's until here)
    MCXCHK(rc);
    if (dbg) return MCX_OK;
    // mi, the null, pearson
    t0 = std::chrono::steady_clock::now();
    std::vector<double> pm((size_t)P);
    for (int i = 0; i < npairs; ++i) {
      const int ia = act_of[(size_t)i];
      if (ia < 0) continue;
      mcx_mutinfo_pair &o = pairs_out[i];
      o.mi = MH::mi_of_sum(hs[2 * (size_t)ia], m, k, table.data());
      o.nzero = (long long)hs[2 * (size_t)ia + 1];
      if (o.nzero > 0) o.flags |= MCX_MUTINFO_PAIR_TIES;
      o.r_info = MH::r_info(o.mi);
      o.pearson = MH::pearson(pt.z.data() + (size_t)o.a * m, pt.z.data() + (size_t)o.b * m, m);
      for (int p = 1; p <= P; ++p) pm[(size_t)p - 1] = MH::mi_of_sum(hs[2 * ((size_t)p * nact + ia)], m, k, table.data());
      if (perm_mi) std::copy(pm.begin(), pm.end(), perm_mi + (size_t)i * P);
      const MH::Null nl = MH::null_of(o.mi, pm.data(), P);
      o.perm_mean = nl.mean;
      o.perm_sd = nl.sd;
      o.p_value = nl.p_value;
      o.nge = nl.nge;
    }
    host_ms[MT_FINISH] = ms_since(t0);
  }
  MCXCHK(tm.collect());
  if (ms) {
    ms[MT_POINTS] = host_ms[MT_POINTS];
    ms[MT_PERMS] = host_ms[MT_PERMS];
    ms[MT_FINISH] = host_ms[MT_FINISH];
    ms[MT_TOTAL] = ms_since(t_total);
  }
  return MCX_OK;
}

int samples_mutinfo(mcx_engine *e, int first_step, int nsteps, const mcx_mutinfo_spec *spec, mcx_mutinfo_result *res, mcx_mutinfo_col *cols,
                    mcx_mutinfo_pair *pairs, double *perm_mi, double *ms)
{
  mcx_mutinfo_spec s;
  return on_store(
      e, first_step, nsteps,
      [&]() -> int {
        if (!res) return fail(MCX_ERR_INVALID, "res is NULL");
        if (!pairs) return fail(MCX_ERR_INVALID, "pairs is NULL");
        if (nsteps < 1) return fail(MCX_ERR_INVALID, "nsteps = %d: a range of at least one step", nsteps);
        int n, np;
        return mutinfo_args(spec, &s, e->nparam + 1, (int64_t)nsteps * e->nchain, &n, &np);
      },
      [&](hipStream_t st, Bufs, const StoreView &v) { return mutinfo_device(st, v, s, res, cols, pairs, perm_mi, nullptr, ms); });
}

// what the host-row entries refuse before a device is touched
int rows_args(const float *rows, int nsteps, int nc, int np, const mcx_mutinfo_spec *spec, mcx_mutinfo_spec *s, int *n, int *npairs)
{
  if (!rows) return fail(MCX_ERR_INVALID, "rows is NULL");
  if (np < 1 || np > 256) return fail(MCX_ERR_INVALID, "np = %d: 1 to 256 parameters", np);
  if (nsteps < 1 || nc < 1) return fail(MCX_ERR_INVALID, "%d steps of %d chains: at least one step of one chain", nsteps, nc);
  return mutinfo_args(spec, s, np + 1, (int64_t)nsteps * nc, n, npairs);
}

}  // namespace

extern "C" int mcx_store_mutinfo(mcx_store *a, const mcx_mutinfo_spec *spec, mcx_mutinfo_result *res, mcx_mutinfo_col *cols,
                                 mcx_mutinfo_pair *pairs, double *perm_mi)
{
  if (!a) return fail(MCX_ERR_INVALID, "the store s is NULL");
  if (!res) return fail(MCX_ERR_INVALID, "res is NULL");
  if (!pairs) return fail(MCX_ERR_INVALID, "pairs is NULL");
  mcx_mutinfo_spec s;
  int n, np;
  MCXCHK(mutinfo_args(spec, &s, a->nout + 1, (int64_t)a->T * a->nc, &n, &np));
  HIPCHK(hipSetDevice(a->device));
  return mutinfo_device(a->st, StoreView(a->span()), s, res, cols, pairs, perm_mi, nullptr, nullptr);
}

extern "C" int mcx_rows_mutinfo(const float *rows, int nsteps, int nc, int np, const mcx_mutinfo_spec *spec, mcx_mutinfo_result *res,
                                mcx_mutinfo_col *cols, mcx_mutinfo_pair *pairs, double *perm_mi)
{
  if (!res) return fail(MCX_ERR_INVALID, "res is NULL");
  if (!pairs) return fail(MCX_ERR_INVALID, "pairs is NULL");
  mcx_mutinfo_spec s;
  int n, npairs;
  MCXCHK(rows_args(rows, nsteps, nc, np, spec, &s, &n, &npairs));
  return on_rows(rows, nsteps, nc, np,
                 [&](hipStream_t st, Bufs, const StoreView &v) { return mutinfo_device(st, v, s, res, cols, pairs, perm_mi, nullptr, nullptr); });
}

extern "C" int mcx_samples_mutinfo(mcx_engine *e, int first_step, int nsteps, const mcx_mutinfo_spec *spec, mcx_mutinfo_result *res,
                                   mcx_mutinfo_col *cols, mcx_mutinfo_pair *pairs, double *perm_mi)
{
  return samples_mutinfo(e, first_step, nsteps, spec, res, cols, pairs, perm_mi, nullptr);
}

extern "C" int mcx_debug_mutinfo_times(mcx_engine *e, int first_step, int nsteps, const mcx_mutinfo_spec *spec, double *ms)
{
  if (!ms) return fail(MCX_ERR_INVALID, "ms is NULL");
  if (!e) return fail(MCX_ERR_INVALID, "engine is NULL");
  mcx_mutinfo_spec s;
  int n, npairs;
  if (nsteps < 1) return fail(MCX_ERR_INVALID, "nsteps = %d: a range of at least one step", nsteps);
  MCXCHK(mutinfo_args(spec, &s, e->nparam + 1, (int64_t)nsteps * e->nchain, &n, &npairs));
  mcx_mutinfo_result res;
  std::vector<mcx_mutinfo_pair> pairs((size_t)npairs);
  return samples_mutinfo(e, first_step, nsteps, spec, &res, nullptr, pairs.data(), nullptr, ms);
}

extern "C" int mcx_debug_mutinfo_counts(const float *rows, int nsteps, int nc, int np, const mcx_mutinfo_spec *spec, int pair, int p,
                                        double *eps, int *na, int *nb)
{
  if (!eps || !na || !nb) return fail(MCX_ERR_INVALID, "eps, na or nb is NULL");
  mcx_mutinfo_spec s;
  int n, npairs;
  MCXCHK(rows_args(rows, nsteps, nc, np, spec, &s, &n, &npairs));
  if (pair < 0 || pair >= npairs) return fail(MCX_ERR_INVALID, "pair = %d: 0 to %d", pair, npairs - 1);
  if (p < 0 || p > s.nperm) return fail(MCX_ERR_INVALID, "p = %d: 0 to spec.nperm = %d", p, s.nperm);
  mcx_mutinfo_result res;
  std::vector<mcx_mutinfo_pair> pairs((size_t)npairs);
  const MiDebug dbg{pair, p, eps, na, nb};
  return on_rows(rows, nsteps, nc, np,
                 [&](hipStream_t st, Bufs, const StoreView &v) { return mutinfo_device(st, v, s, &res, nullptr, pairs.data(), nullptr, &dbg, nullptr); });
}

// host only
extern "C" int mcx_debug_mutinfo_rows(long long N, int n, long long *index)
{
  if (!index) return fail(MCX_ERR_INVALID, "index is NULL");
  if (n < 1 || n > MCX_MUTINFO_MAX_ROWS || (long long)n > N) return fail(MCX_ERR_INVALID, "n = %d of N = %lld: 1 to min(N, %d) rows", n, N, (int)MCX_MUTINFO_MAX_ROWS);
  if (N >= (1LL << 49)) return fail(MCX_ERR_INVALID, "N = %lld: below 2^49", N);
  for (int i = 0; i < n; ++i) index[i] = (long long)MH::row_index(N, n, i);
  return MCX_OK;
}

// host only
extern "C" int mcx_debug_mutinfo_perm(uint32_t seed, int m, int p, int *perm)
{
  if (!perm) return fail(MCX_ERR_INVALID, "perm is NULL");
  if (m < 1 || m > MCX_MUTINFO_MAX_ROWS) return fail(MCX_ERR_INVALID, "m = %d: 1 to %d points", m, (int)MCX_MUTINFO_MAX_ROWS);
  if (p < 0 || p > MCX_MUTINFO_MAX_PERM) return fail(MCX_ERR_INVALID, "p = %d: 0 to %d", p, (int)MCX_MUTINFO_MAX_PERM);
  MH::permutation(seed, m, p, perm);
  return MCX_OK;
}

// host only
extern "C" int mcx_debug_mutinfo_psi(int q_max, double *table)
{
  if (!table) return fail(MCX_ERR_INVALID, "table is NULL");
  if (q_max < 1 || q_max > MCX_MUTINFO_MAX_ROWS) return fail(MCX_ERR_INVALID, "q_max = %d: 1 to %d", q_max, (int)MCX_MUTINFO_MAX_ROWS);
  MH::psi_table(q_max, table);
  return MCX_OK;
}

// host only
extern "C" int mcx_mutinfo_finish(const double *eps, const int *na, const int *nb, int m, int k, double *mi, long long *nzero)
{
  if (!eps || !na || !nb || !mi) return fail(MCX_ERR_INVALID, "eps, na, nb or mi is NULL");
  if (k < 1 || k > MCX_MUTINFO_MAX_K) return fail(MCX_ERR_INVALID, "k = %d: 1 to %d", k, (int)MCX_MUTINFO_MAX_K);
  if (m <= k || m > MCX_MUTINFO_MAX_ROWS) return fail(MCX_ERR_INVALID, "m = %d: k + 1 = %d to %d points", m, k + 1, (int)MCX_MUTINFO_MAX_ROWS);
  for (int i = 0; i < m; ++i)
    if (na[i] < 0 || na[i] >= m || nb[i] < 0 || nb[i] >= m) return fail(MCX_ERR_INVALID, "na[%d] = %d, nb[%d] = %d: 0 to m - 1 = %d", i, na[i], i, nb[i], m - 1);
  std::vector<double> table((size_t)m);
  MH::psi_table(m, table.data());
  *mi = MH::finish_pair(eps, na, nb, m, k, table.data(), nzero);
  return MCX_OK;
}

// host only
extern "C" int mcx_debug_mutinfo_points(const float *rows, int nsteps, int nc, int np, const mcx_mutinfo_spec *spec, mcx_mutinfo_result *res,
                                        long long *index, unsigned char *kept, mcx_mutinfo_col *cols, double *z)
{
  mcx_mutinfo_spec s;
  int n, npairs;
  MCXCHK(rows_args(rows, nsteps, nc, np, spec, &s, &n, &npairs));
  const int ncol = np + 1;
  const int64_t N = (int64_t)nsteps * nc;
  std::vector<float> sel((size_t)n * ncol);
  select_rows(rows, N, ncol, n, sel.data(), index);
  MH::Points pt;
  MH::points(sel.data(), n, ncol, s.flags & MCX_MUTINFO_WITH_LL, s.flags & MCX_MUTINFO_RAW, pt);
  if (res) *res = mcx_mutinfo_result{(long long)N, n, pt.ndup, pt.m, s.k, npairs, s.nperm, pt.nused};
  if (kept) std::copy(pt.kept.begin(), pt.kept.end(), kept);
  if (cols)
    for (int c = 0; c < ncol; ++c) cols[c] = mcx_mutinfo_col{pt.scale[(size_t)c], pt.flags[(size_t)c]};
  if (z) std::copy(pt.z.begin(), pt.z.end(), z);
  return MCX_OK;
}

// host only
extern "C" int mcx_debug_mutinfo_geometry(int m, int npairs, int nperm, int k, mcx_mutinfo_geometry *g)
{
  if (!g) return fail(MCX_ERR_INVALID, "g is NULL");
  if (k < 1 || k > MCX_MUTINFO_MAX_K) return fail(MCX_ERR_INVALID, "k = %d: 1 to %d", k, (int)MCX_MUTINFO_MAX_K);
  if (m <= k || m > MCX_MUTINFO_MAX_ROWS) return fail(MCX_ERR_INVALID, "m = %d: k + 1 = %d to %d points", m, k + 1, (int)MCX_MUTINFO_MAX_ROWS);
  if (npairs < 1 || npairs > MCX_MUTINFO_MAX_PAIRS) return fail(MCX_ERR_INVALID, "npairs = %d: 1 to %d", npairs, (int)MCX_MUTINFO_MAX_PAIRS);
  if (nperm < 0 || nperm > MCX_MUTINFO_MAX_PERM) return fail(MCX_ERR_INVALID, "nperm = %d: 0 to %d permutations", nperm, (int)MCX_MUTINFO_MAX_PERM);
  const MiGeometry c = mutinfo_geometry(m, npairs, nperm);
  g->block = MB;
  g->queries_per_lane = MQ;
  g->tile_rows = MTI;
  g->stage_rows = c.stage_rows;
  g->stages = c.stages;
  g->tiles = c.tiles;
  g->workgroups = (long long)c.tiles * npairs * (1 + nperm);
  g->lds_bytes = (long long)(MST * sizeof(double2) + 2 * MB * sizeof(double));
  g->scratch_bytes = (long long)c.scratch_bytes;
  return MCX_OK;
}
