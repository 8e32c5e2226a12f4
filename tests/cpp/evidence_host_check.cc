// The host half of the evidence of a store (mcpar_amd/csrc/mcx_evidence_host.hpp) as a stand-alone
// program: the proposal's factors, the refusals with their messages, the component pick, the terms at the ends of their
// range and the whole estimator on host arrays.  tests/test_evidence_cpu.py builds it plain and under AddressSanitizer and
// UBSan and runs it; it exits 0 or prints the line that failed.
#include "mcpar_amd/csrc/mcx_evidence_host.hpp"

#include <cstdlib>
#include <cstring>

namespace H = mcx_evidence_host;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("%s:%d: %s\n", __FILE__, __LINE__, #c);         \
      return 1;                                                   \
    }                                                             \
  } while (0)

static bool close_to(double a, double b, double rtol) { return std::fabs(a - b) <= rtol * std::fabs(b); }

int main()
{
  char msg[256];
  // ---- the factors of two components of three parameters
  const int np = 3, K = 2;
  const double w[K] = {1.0, 3.0};
  const double c[K * np] = {0.0, 1.0, -1.0, 6.0, 6.0, 6.0};
  const double cov[K * np * np] = {4.0, 2.0, 0.6, 2.0, 2.0, 0.5, 0.6, 0.5, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  std::vector<double> Cf(K * np * np), W(K * np * np), lc(K);
  CHECK(H::proposal(np, K, w, c, cov, 1.5, Cf.data(), W.data(), lc.data(), msg, sizeof msg) == H::OK);
  for (int k = 0; k < K; ++k)
    for (int i = 0; i < np; ++i)
      for (int j = 0; j < np; ++j) {
        double cc = 0.0, wc = 0.0;
        for (int l = 0; l < np; ++l) {
          cc += Cf[(k * np + i) * np + l] * Cf[(k * np + j) * np + l];
          wc += W[(k * np + i) * np + l] * Cf[(k * np + l) * np + j];
        }
        CHECK(std::fabs(cc - 2.25 * cov[(k * np + i) * np + j]) < 1e-14);
        CHECK(std::fabs(wc - (i == j ? 1.0 : 0.0)) < 1e-14);
        if (j > i) CHECK(Cf[(k * np + i) * np + j] == 0.0 && W[(k * np + i) * np + j] == 0.0);
      }
  CHECK(close_to(lc[1], std::log(0.75) - 3.0 * std::log(1.5) - 1.5 * H::LOG_2PI, 1e-14));
  // a row at a centre has log g = lc when it is the only component
  const float at[np] = {6.0f, 6.0f, 6.0f};
  const double one = 1.0;
  double lc1 = 0.0;
  CHECK(H::proposal(np, 1, &one, c + np, cov + np * np, 1.0, Cf.data(), W.data(), &lc1, msg, sizeof msg) == H::OK);
  CHECK(H::logg_row(np, 1, c + np, W.data(), &lc1, at) == lc1);
  const float nanrow[np] = {6.0f, std::numeric_limits<float>::quiet_NaN(), 6.0f};
  const double lgn = H::logg_row(np, 1, c + np, W.data(), &lc1, nanrow);
  CHECK(lgn != lgn);

  // ---- the refusals
  CHECK(H::proposal(0, K, w, c, cov, 1.0, Cf.data(), W.data(), lc.data(), msg, sizeof msg) == H::ERR_INVALID && std::strstr(msg, "np = 0"));
  CHECK(H::proposal(np, 9, w, c, cov, 1.0, Cf.data(), W.data(), lc.data(), msg, sizeof msg) == H::ERR_INVALID && std::strstr(msg, "1 to 8"));
  CHECK(H::proposal(np, K, nullptr, c, cov, 1.0, Cf.data(), W.data(), lc.data(), msg, sizeof msg) == H::ERR_INVALID && std::strstr(msg, "NULL"));
  const double wbad[K] = {1.0, 0.0};
  CHECK(H::proposal(np, K, wbad, c, cov, 1.0, Cf.data(), W.data(), lc.data(), msg, sizeof msg) == H::ERR_INVALID && std::strstr(msg, "weights[1]"));
  for (double s : {0.0, -1.0, std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN()})
    CHECK(H::proposal(np, K, w, c, cov, s, Cf.data(), W.data(), lc.data(), msg, sizeof msg) == H::ERR_INVALID && std::strstr(msg, "scale"));
  double sing[K * np * np];
  std::memcpy(sing, cov, sizeof sing);
  for (int i = 0; i < np; ++i) sing[np * np + i * np + 1] = sing[np * np + 1 * np + i] = 0.0;  // a constant column in component 1
  CHECK(H::proposal(np, K, w, c, sing, 1.0, Cf.data(), W.data(), lc.data(), msg, sizeof msg) == H::ERR_INVALID);
  CHECK(std::strstr(msg, "component 1") && std::strstr(msg, "pivot 1 = 0"));

  // ---- the component pick and the uniform
  const double cum[3] = {1.0, 1.0 + 2.0, 1.0 + 2.0 + 1.0};
  CHECK(H::pick_component(0.0, cum, 3) == 0 && H::pick_component(0.25, cum, 3) == 1 && H::pick_component(0.7499, cum, 3) == 1);
  CHECK(H::pick_component(0.75, cum, 3) == 2 && H::pick_component(0.999999, cum, 3) == 2 && H::pick_component(0.5, cum, 1) == 0);
  for (uint32_t j = 0; j < 64; ++j) {
    const double u = H::draw_uniform(7u, j);
    CHECK(u >= 0.0 && u < 1.0);
  }
  CHECK(H::uniform53(0xffffffffu, 0xffffffffu) < 1.0 && H::uniform53(0u, 0x7ffu) == 0.0 && H::uniform53(0u, 0x800u) == 0x1p-53);

  // ---- the terms at the ends of their range: no overflow, no NaN
  const double ninf = -std::numeric_limits<double>::infinity();
  for (double a : {-745.0, -700.0, -1.0, 0.0, 1.0, 700.0, 745.0}) {
    for (double r : {1e-300, 1.0, 1e300}) {
      CHECK(std::isfinite(H::term_num(a, r, 0.25, 0.75)) && std::isfinite(H::term_den(a, r, 0.25, 0.75)));
      CHECK(H::term_num(a, r, 0.25, 0.75) >= 0.0 && H::term_den(a, r, 0.25, 0.75) >= 0.0);
    }
    CHECK(std::isfinite(H::term_f1(a, 0.25, 0.75)) && std::isfinite(H::term_f2(a, 0.25, 0.75)));
  }
  CHECK(H::term_num(ninf, 1.0, 0.25, 0.75) == 0.0 && H::term_f1(ninf, 0.25, 0.75) == 0.0);
  CHECK(close_to(H::term_num(1e-9, 2.0, 0.25, 0.75), H::term_num(-1e-9, 2.0, 0.25, 0.75), 1e-8));  // the branches meet
  CHECK(close_to(H::term_den(1e-9, 2.0, 0.25, 0.75), H::term_den(-1e-9, 2.0, 0.25, 0.75), 1e-8));

  // ---- the whole estimator: l constant gives that constant after one pass (a second one sees no change)
  H::IterateResult o;
  std::vector<double> l1(100, 3.25), l2(40, 3.25);
  CHECK(H::iterate(l1.data(), 100, l2.data(), 40, 100.0, 100.0, 1e-10, 1000, &o, msg, sizeof msg) == H::OK);
  CHECK(o.log_z == 3.25 && o.iters <= 2 && o.flags == 0 && o.se == 0.0 && o.log_z_is == 3.25 && o.log_z_ris == 3.25 && o.ndraw_zero == 0);
  // a range of +-700 about l*: finite
  for (int i = 0; i < 100; ++i) l1[i] = -700.0 + 14.0 * i + 7.0;
  for (int j = 0; j < 40; ++j) l2[j] = 700.0 - 35.0 * j - 17.5;
  CHECK(H::iterate(l1.data(), 100, l2.data(), 40, 100.0, 100.0, 1e-10, 1000, &o, msg, sizeof msg) == H::OK);
  CHECK(std::isfinite(o.log_z) && std::isfinite(o.se) && std::isfinite(o.log_z_is) && std::isfinite(o.log_z_ris));
  // one pass allowed: the flag
  CHECK(H::iterate(l1.data(), 100, l2.data(), 40, 100.0, 100.0, 1e-10, 1, &o, msg, sizeof msg) == H::OK);
  CHECK(o.iters == 1 && (o.flags & H::F_NOT_CONVERGED));
  // draws with L = 0: counted, and refused when they are all there is
  l2[3] = l2[17] = ninf;
  CHECK(H::iterate(l1.data(), 100, l2.data(), 40, 100.0, 100.0, 1e-10, 1000, &o, msg, sizeof msg) == H::OK && o.ndraw_zero == 2);
  for (double &v : l2) v = ninf;
  CHECK(H::iterate(l1.data(), 100, l2.data(), 40, 100.0, 100.0, 1e-10, 1000, &o, msg, sizeof msg) == H::ERR_INVALID && std::strstr(msg, "L = 0"));
  l2[5] = std::numeric_limits<double>::infinity();
  CHECK(H::iterate(l1.data(), 100, l2.data(), 40, 100.0, 100.0, 1e-10, 1000, &o, msg, sizeof msg) == H::ERR_INVALID && std::strstr(msg, "draw 5"));
  l1[42] = std::numeric_limits<double>::quiet_NaN();
  l1[77] = ninf;
  CHECK(H::iterate(l1.data(), 100, l2.data(), 40, 100.0, 100.0, 1e-10, 1000, &o, msg, sizeof msg) == H::ERR_INVALID && std::strstr(msg, "row 42"));

  // ---- the lower median
  std::vector<double> v = {5.0, 1.0, 4.0, 2.0};
  CHECK(H::lower_median(v) == 2.0);
  v = {3.0, 9.0, 1.0};
  CHECK(H::lower_median(v) == 3.0);
  v = {3.0, std::numeric_limits<double>::quiet_NaN()};
  const double m = H::lower_median(v);
  CHECK(m != m);
  std::printf("ok\n");
  return 0;
}
