// The host half of the lagged covariance (mcpar_amd/csrc/mcx_lagcov_host.hpp: the Cholesky factorisation, the walk of the
// multivariate initial sequence estimator, its flags and the numbers made of Sigma) as a stand-alone program: built plain and
// with -fsanitize=address,undefined by tests/test_lagcov_cpu.py.  It needs no HIP and no library.
#include "mcpar_amd/csrc/mcx_lagcov_host.hpp"

#include <cstdio>

namespace H = mcx_lagcov_host;

static int fails = 0;
#define EXPECT(c)                                                \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("line %d: %s\n", __LINE__, #c);                \
      ++fails;                                                   \
    }                                                            \
  } while (0)

static bool close_to(double a, double b) { return std::fabs(a - b) <= 1e-12 * std::fabs(b); }

// G(t) of a stationary AR(1) column of variance v and coefficient phi, ncol = 1, lags 0 .. nlags - 1
static std::vector<double> ar1(double v, double phi, int nlags)
{
  std::vector<double> g(nlags);
  for (int t = 0; t < nlags; ++t) g[t] = v * std::pow(phi, t);
  return g;
}

struct Out {
  H::Result r{};
  std::vector<int> fl;
  std::vector<double> ess, mcse, sigma;
  bool stopped = false;
};
static Out run(int ncol, int nlags, long long N, const std::vector<double> &g, std::vector<unsigned char> use = {})
{
  Out o;
  if (use.empty()) use.assign(ncol, 1);
  o.fl.resize(ncol);
  o.ess.resize(ncol);
  o.mcse.resize(ncol);
  o.sigma.resize((size_t)ncol * ncol);
  o.stopped = H::finish(ncol, nlags, N, g.data(), use.data(), &o.r, o.fl.data(), o.ess.data(), o.mcse.data(), o.sigma.data());
  return o;
}

int main()
{
  // the factorisation: a known factor, the failing pivot, a NaN
  double a[9] = {4, 2, 2, 2, 5, 3, 2, 3, 6};
  EXPECT(H::cholesky_lower(3, a) == 0 && a[0] == 2 && a[3] == 1 && a[4] == 2 && a[6] == 1 && a[7] == 1 && a[8] == 2 && a[1] == 0 &&
         a[2] == 0 && a[5] == 0);
  double b[4] = {1, 2, 2, 1};
  EXPECT(H::cholesky_lower(2, b) == 2);
  double c[1] = {NAN};
  EXPECT(H::cholesky_lower(1, c) == 1);
  std::vector<double> work;
  double ld = 0.0;
  const double m[4] = {2, 1, 1, 2};
  EXPECT(H::logdet_pd(2, m, work, &ld) && close_to(ld, std::log(3.0)));

  // one column, AR(1) with phi = 0.5 and exact autocovariances: P(k) = v phi^2k (1 + phi) decreases, Sigma_k grows for ever, so
  // the walk runs to K and says so.  Sigma_K = v (-1 + 2 (1 + phi) (1 - phi^(2K + 2)) / (1 - phi^2))
  {
    const int nlags = 12, K = 5;
    Out o = run(1, nlags, 1000, ar1(2.0, 0.5, nlags));
    EXPECT(!o.stopped && o.r.s == 0 && o.r.k_used == K && o.r.lags_used == 12 && o.r.flags == H::MESS_TRUNCATED && o.r.p == 1);
    const double want = 2.0 * (-1.0 + 2.0 * 1.5 * (1.0 - std::pow(0.5, 2 * K + 2)) / 0.75);
    EXPECT(close_to(o.sigma[0], want) && close_to(o.r.logdet_sigma, std::log(want)));
    EXPECT(close_to(o.r.logdet_lambda, std::log(2.0 * 1000 / 999.0)));
    EXPECT(close_to(o.r.mess, 1000 * (2.0 * 1000 / 999.0) / want) && close_to(o.ess[0], o.r.mess) &&
           close_to(o.mcse[0], std::sqrt(want / 1000)));
  }
  // noise in the tail ends the walk: P(2) < 0 makes log det fall, k_used = 1, not truncated
  {
    std::vector<double> g = {1.0, 0.5, 0.25, 0.125, -0.05, -0.05, 0.3, 0.3};
    Out o = run(1, 8, 100, g);
    EXPECT(o.stopped && o.r.s == 0 && o.r.k_used == 1 && o.r.lags_used == 4 && o.r.flags == 0);
    EXPECT(close_to(o.sigma[0], -1.0 + 2.0 * (1.0 + 0.5 + 0.25 + 0.125)));
  }
  // an antithetic column, phi = -0.9: Sigma_k = v (-1 + 0.2 (1 - 0.81^(k + 1)) / 0.19) turns positive only at k = 14
  {
    const int nlags = 96;
    Out o = run(1, nlags, 4000, ar1(1.0, -0.9, nlags));
    EXPECT(o.r.s == 14 && o.r.k_used == (nlags - 2) / 2 && (o.r.flags & H::MESS_TRUNCATED));
    Out early = run(1, 20, 4000, ar1(1.0, -0.9, 20));
    EXPECT(!early.stopped && early.r.s == -1 && early.r.k_used == -1 && early.r.flags == H::MESS_NOT_PD && std::isnan(early.r.mess) &&
           std::isnan(early.sigma[0]) && std::isnan(early.ess[0]) && std::isnan(early.mcse[0]) && early.r.lags_used == 0);
  }
  // two columns with a cross term that is not symmetric, one unused, one constant, one not finite
  {
    const int ncol = 5, nlags = 4;
    const size_t nn = 25;
    std::vector<double> g(nlags * nn, 0.0);
    auto at = [&](int t, int i, int j) -> double & { return g[t * nn + (size_t)i * ncol + j]; };
    for (int t = 0; t < nlags; ++t) {
      const double f = std::pow(0.5, t);
      at(t, 0, 0) = 2.0 * f;
      at(t, 1, 1) = 1.0 * f;
      at(t, 0, 1) = 0.6 * f;
      at(t, 1, 0) = t == 0 ? 0.6 : 0.2 * f;
      at(t, 2, 2) = 3.0 * f;
      for (int j = 0; j < ncol; ++j) at(t, 4, j) = at(t, j, 4) = NAN;
    }
    Out o = run(ncol, nlags, 50, g, {1, 1, 0, 1, 0});
    EXPECT(o.r.p == 2 && o.r.s == 0 && o.r.k_used == 1 && (o.r.flags & H::MESS_TRUNCATED));
    EXPECT(o.fl[3] == H::COL_CONSTANT && o.fl[0] == 0 && o.fl[2] == 0);
    // Sigma_01 = -0.6 + 2 (0.6 + 0.2 + 0.1 + 0.05) with S(t)_01 = (0.6 + 0.2) / 2 f for t > 0
    EXPECT(close_to(o.sigma[1], -0.6 + 2.0 * (0.6 + 0.4 * (0.5 + 0.25 + 0.125))) && o.sigma[1] == o.sigma[5]);
    EXPECT(std::isnan(o.sigma[2]) && std::isnan(o.sigma[12]) && std::isnan(o.sigma[18]) && std::isnan(o.sigma[24]));
    EXPECT(std::isnan(o.ess[2]) && std::isnan(o.ess[3]) && std::isnan(o.ess[4]) && o.ess[0] > 0 && o.ess[1] > 0);
    const double dl = (2.0 * 1.0 - 0.36) * (50.0 / 49.0) * (50.0 / 49.0);
    EXPECT(close_to(o.r.logdet_lambda, std::log(dl)));
    const double ds = o.sigma[0] * o.sigma[6] - o.sigma[1] * o.sigma[5];
    EXPECT(close_to(o.r.mess, 50.0 * std::sqrt(dl / ds)));
    // nothing chosen
    Out none = run(ncol, nlags, 50, g, {0, 0, 0, 1, 1});
    EXPECT(none.r.p == 0 && none.r.flags == H::MESS_NOT_PD && none.r.k_used == -1);
  }
  // two collinear columns: Lambda is singular, Sigma is not positive definite at any k
  {
    std::vector<double> g(2 * 4);  // (Sigma_0 = 4 everywhere: the second pivot is 4 - 2 * 2, exactly 0)
    for (int t = 0; t < 2; ++t)
      for (int e = 0; e < 4; ++e) g[t * 4 + e] = 2.0 * std::pow(0.5, t);
    Out o = run(2, 2, 10, g);
    EXPECT(o.r.flags == H::MESS_NOT_PD && o.r.p == 2);
  }
  std::printf(fails ? "%d checks failed\n" : "lagcov host checks ok\n", fails);
  return fails ? 1 : 0;
}
