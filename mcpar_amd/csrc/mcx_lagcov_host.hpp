// mcx_lagcov_host.hpp -- the host half of mcx_*_lagcov and the whole of mcx_mess_finish: from the lagged
// covariance matrices G(0), G(1), ... of a store to the multivariate initial sequence estimator Sigma of Dai & Jones (2017), the
// multivariate effective sample size of Vats, Flegal & Jones (2019) and the per-column numbers made of Sigma.  No HIP and no
// library state: tests/cpp/lagcov_host_check.cc compiles it alone.
//
// cholesky_lower is the one factorisation: it says whether a matrix is positive definite (every pivot > 0) and leaves the factor
// whose diagonal gives the log-determinant.  It is mcx_engine.hip's float cholesky_lower operation by operation, in double: the
// float one cannot hold a log-determinant to the nine digits section 24 states.
#pragma once
#include <cmath>
#include <cstddef>
#include <limits>
#include <vector>

namespace mcx_lagcov_host {

enum { MESS_NOT_PD = 1, MESS_TRUNCATED = 2, MESS_LAMBDA_SINGULAR = 4 };  // include/mcx.h MCX_MESS_*
enum { COL_NONFINITE = 1, COL_CONSTANT = 2 };                            // MCX_SUMMARY_NONFINITE, MCX_LAGCOV_CONSTANT

// lower Cholesky factor of the row-major d x d matrix a, in place, strict upper triangle zeroed.  0, or 1 + the index of the
// first pivot that is not > 0 (a NaN pivot is not)
inline int cholesky_lower(int d, double *a)
{
  for (int i = 0; i < d; ++i) {
    for (int j = 0; j <= i; ++j) {
      double s = a[(size_t)i * d + j];
      for (int k = 0; k < j; ++k) s = std::fma(-a[(size_t)i * d + k], a[(size_t)j * d + k], s);
      if (i == j) {
        if (!(s > 0.0)) return i + 1;
        a[(size_t)i * d + i] = std::sqrt(s);
      } else {
        a[(size_t)i * d + j] = s / a[(size_t)j * d + j];
      }
    }
    for (int j = i + 1; j < d; ++j) a[(size_t)i * d + j] = 0.0;
  }
  return 0;
}

// log det of a symmetric d x d matrix m through cholesky_lower on a copy (work, d * d doubles); false when m is not positive
// definite
inline bool logdet_pd(int d, const double *m, std::vector<double> &work, double *logdet)
{
  work.assign(m, m + (size_t)d * d);
  if (cholesky_lower(d, work.data()) != 0) return false;
  double s = 0.0;
  for (int i = 0; i < d; ++i) s += std::log(work[(size_t)i * d + i]);
  *logdet = 2.0 * s;
  return true;
}

struct Result {
  long long N;
  int p, s, k_used, lags_used, flags;
  double mess, logdet_lambda, logdet_sigma;
};

// The walk.  gamma[nlags][ncol][ncol]: G(0) .. G(nlags - 1); use[ncol]: the chosen columns (a column with G(0)_jj = 0 is taken
// out here and flagged in col_flags[ncol]); N: the rows behind G.  Outputs: res; ess[ncol], mcse[ncol] (NaN outside the chosen
// columns); sigma[ncol][ncol] (NaN outside them).  Returns true when the walk stopped at a test that failed -- then more lags
// change nothing --, false when it ran out of lags (MESS_TRUNCATED) or found no positive definite partial sum (MESS_NOT_PD).
inline bool finish(int ncol, int nlags, long long N, const double *gamma, const unsigned char *use, Result *res, int *col_flags,
                   double *ess, double *mcse, double *sigma)
{
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  const size_t nn = (size_t)ncol * ncol;
  std::vector<int> idx;
  for (int c = 0; c < ncol; ++c) {
    const double v = gamma[(size_t)c * ncol + c];
    col_flags[c] = v == 0.0 ? COL_CONSTANT : 0;
    ess[c] = mcse[c] = qnan;
    if (use[c] && v > 0.0) idx.push_back(c);  // (v is NaN for a column that is not finite: the caller leaves it out of use)
  }
  for (size_t i = 0; i < nn; ++i) sigma[i] = qnan;
  const int p = (int)idx.size();
  res->N = N;
  res->p = p;
  res->s = res->k_used = -1;
  res->lags_used = 0;
  res->flags = 0;
  res->mess = res->logdet_lambda = res->logdet_sigma = qnan;
  const int K = (nlags - 2) / 2;  // the last k with lags 2k and 2k + 1 below nlags
  if (p == 0 || nlags < 2) {
    res->flags |= MESS_NOT_PD;
    return false;
  }
  const size_t pp = (size_t)p * p;
  // S(t) on the chosen columns
  auto sym = [&](int t, int a, int b) {
    const double *g = gamma + (size_t)t * nn;
    return 0.5 * (g[(size_t)idx[a] * ncol + idx[b]] + g[(size_t)idx[b] * ncol + idx[a]]);
  };
  std::vector<double> cur(pp), best(pp), work, lam(pp);
  for (int a = 0; a < p; ++a)
    for (int b = 0; b < p; ++b) {
      const double s0 = sym(0, a, b);
      cur[(size_t)a * p + b] = -s0;
      lam[(size_t)a * p + b] = s0 * ((double)N / (double)(N - 1));
    }
  double ld_best = 0.0;
  bool stopped = false;
  for (int k = 0; k <= K; ++k) {
    for (int a = 0; a < p; ++a)
      for (int b = 0; b < p; ++b) cur[(size_t)a * p + b] += 2.0 * (sym(2 * k, a, b) + sym(2 * k + 1, a, b));
    double ld = 0.0;
    const bool pd = logdet_pd(p, cur.data(), work, &ld);
    if (res->s < 0) {
      if (!pd) continue;
      res->s = k;
    } else if (!pd || !(ld > ld_best)) {
      stopped = true;
      break;
    }
    res->k_used = k;
    ld_best = ld;
    best = cur;
  }
  if (res->s < 0) {
    res->flags |= MESS_NOT_PD;
    return false;
  }
  if (!stopped) res->flags |= MESS_TRUNCATED;
  res->lags_used = 2 * res->k_used + 2;
  res->logdet_sigma = ld_best;
  double ldl = 0.0;
  if (logdet_pd(p, lam.data(), work, &ldl)) {
    res->logdet_lambda = ldl;
    res->mess = (double)N * std::exp((ldl - ld_best) / (double)p);
  } else {
    res->flags |= MESS_LAMBDA_SINGULAR;
  }
  for (int a = 0; a < p; ++a) {
    for (int b = 0; b < p; ++b) sigma[(size_t)idx[a] * ncol + idx[b]] = best[(size_t)a * p + b];
    const double saa = best[(size_t)a * p + a];
    ess[idx[a]] = (double)N * lam[(size_t)a * p + a] / saa;
    mcse[idx[a]] = std::sqrt(saa / (double)N);
  }
  return stopped;
}

}  // namespace mcx_lagcov_host
