// parse_check -- mcpar_amd/csrc/parse_g.hpp against the C library: the float of a token as glibc's strtof gives it in the
// "C" locale (the program never calls setlocale).
//   parse_check quick      every 1009th bit pattern through fmt_g6's text and through %.9g; 10^6 random tokens of 1-19 digits;
//                          10^5 midpoints of adjacent floats and their neighbours one unit in the last digit away; the
//                          specials, the refused and the tokens that need the host
//   parse_check all        all 2^32 bit patterns through both texts, and the count of floats x with
//                          fmt(parse(fmt(x))) != fmt(x) (minutes; OpenMP)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../mcpar_amd/csrc/parse_g.hpp"

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()
{
  uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

static uint32_t bits_of(float f)
{
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}
static bool is_nan(uint32_t b) { return (b & 0x7fffffffu) > 0x7f800000u; }
static bool same_bits(uint32_t a, uint32_t b) { return a == b || (is_nan(a) && is_nan(b)); }

// parse_g against strtof on one token of the exact domain
static void check_token(const char *tok, long *bad)
{
  uint32_t got = 0;
  const int st = parseg::parse(tok, strlen(tok), &got);
  char *end;
  const uint32_t want = bits_of(strtof(tok, &end));
  if (st != parseg::OK || *end || !same_bits(got, want)) {
    if (++*bad <= 10) fprintf(stderr, "token '%s': status %d, parse_g %08x, strtof %08x\n", tok, st, got, want);
  }
}

// the two texts of one float: what fmt_g6 writes must parse as strtof parses it, what %.9g writes must give the float back
static void check_float(uint32_t b, long *bad, long *roundtrip)
{
  float f;
  memcpy(&f, &b, 4);
  char t6[32], t9[64];
  *fmtg6::append(t6, f) = 0;
  check_token(t6, bad);
  snprintf(t9, sizeof t9, "%.9g", (double)f);
  uint32_t got = 0;
  const int st = parseg::parse(t9, strlen(t9), &got);
  if (st != parseg::OK || !same_bits(got, b)) {
    if (++*bad <= 10) fprintf(stderr, "bits %08x as '%s': status %d, parse_g %08x\n", b, t9, st, got);
  }
  if (roundtrip) {
    uint32_t back = 0;
    char again[32];
    if (parseg::parse(t6, strlen(t6), &back) == parseg::OK) {
      float g;
      memcpy(&g, &back, 4);
      *fmtg6::append(again, g) = 0;
      if (strcmp(again, t6) != 0) ++*roundtrip;
    }
  }
}

// digits (no sign) with a point somewhere and an exponent, in one of the spellings the grammar allows
static std::string spell(const std::string &digits, int q)
{
  std::string s;
  const int r = (int)(rnd() % 8);
  if (r == 0) s += '+';
  else if (r < 3) s += '-';
  for (int z = (int)(rnd() % 4); z > 1; --z) s += '0';  // leading zeros, sometimes
  const int n = (int)digits.size(), pt = (int)(rnd() % (n + 2));  // digits before the point; n + 1: no point at all
  int e = q;
  if (pt <= n) {
    if (pt == 0 && (rnd() & 1)) s += '0';
    s += digits.substr(0, pt) + "." + digits.substr(pt);
    e = q + (n - pt);
    if (pt == 0 && n == 0) s += '0';
  } else s += digits;
  if (e != 0 || (rnd() & 1)) {
    s += (rnd() & 1) ? 'e' : 'E';
    if (e < 0) s += '-';
    else if (rnd() & 1) s += '+';
    char buf[16];
    snprintf(buf, sizeof buf, (rnd() & 1) ? "%02d" : "%d", e < 0 ? -e : e);
    s += buf;
  }
  return s;
}

static void random_tokens(long count, long *bad, long *n)
{
  for (long k = 0; k < count; ++k) {
    const int nd = 1 + (int)(rnd() % 19);
    std::string d;
    for (int i = 0; i < nd; ++i) d += (char)('0' + rnd() % 10);
    if (rnd() % 4 == 0)  // trailing zeros (they count among the 19)
      for (int i = nd - 1, z = (int)(rnd() % nd); z > 0 && i > 0; --z, --i) d[i] = '0';
    const int q = (int)(rnd() % 116) - 70;  // -70 .. 45
    const std::string t = spell(d, q);
    check_token(t.c_str(), bad);
    ++*n;
  }
}

// midpoints of adjacent floats with at most 19 digits, and the decimals one unit in the last digit to either side
static void midpoints(long count, long *bad, long *n)
{
  for (long k = 0; k < count; ++k) {
    const uint32_t m = 0x800000u | (uint32_t)(rnd() & 0x7fffffu);
    const uint64_t odd = 2ull * m + 1ull;  // midpoint = odd 2^(e - 1), value = m 2^e
    const int h = (int)(rnd() % 55) - 16;  // e - 1: -16 .. 38
    uint64_t W;
    int q;
    if (h >= 0) {
      if (h > 38) continue;
      W = odd << h;  // < 2^25 2^38 < 10^19
      q = 0;
    } else {
      W = odd;
      for (int i = 0; i < -h; ++i) W *= 5u;  // odd 5^k < 2^25 5^16 < 10^19
      q = h;
    }
    for (int o = -1; o <= 1; ++o) {
      char buf[32];
      snprintf(buf, sizeof buf, "%llu", (unsigned long long)(W + (uint64_t)o));
      const std::string t = spell(buf, q);
      check_token(t.c_str(), bad);
      ++*n;
    }
  }
}

static void expect(const char *tok, uint32_t want, long *bad)
{
  uint32_t got = 0;
  const int st = parseg::parse(tok, strlen(tok), &got);
  if (st != parseg::OK || !same_bits(got, want)) {
    if (++*bad <= 10) fprintf(stderr, "special '%s': status %d, parse_g %08x, expected %08x\n", tok, st, got, want);
  }
  if (!is_nan(want)) check_token(tok, bad);
}

static void expect_status(const char *tok, int want, long *bad)
{
  uint32_t got = 0;
  const int st = parseg::parse(tok, strlen(tok), &got);
  if (st != want && ++*bad <= 10) fprintf(stderr, "token '%s': status %d, expected %d\n", tok, st, want);
}

static void specials(long *bad, long *n)
{
  const struct { const char *t; uint32_t b; } sp[] = {
      {"9.99999e+07", 0x4cbebc14u}, {"7.00649e-46", 0u}, {"7.0065e-46", 1u}, {"3.40282e+38", 0x7f7fffeeu},
      {"3.40283e+38", 0x7f800000u}, {"1e39", 0x7f800000u}, {"-1e39", 0xff800000u}, {"-0", 0x80000000u}, {"0", 0u},
      {".5", 0x3f000000u}, {"5.", 0x40a00000u}, {"+1e+2", 0x42c80000u}, {"16777217", 0x4b800000u}, {"16777219", 0x4b800002u},
      {"inf", 0x7f800000u}, {"-inf", 0xff800000u}, {"+INF", 0x7f800000u}, {"Infinity", 0x7f800000u}, {"-iNfInItY", 0xff800000u},
      {"nan", 0x7fc00000u}, {"-NaN", 0xffc00000u}, {"+nan", 0x7fc00000u}, {"0e999", 0u}, {"-0.000e-999", 0x80000000u},
      {"1e-99999", 0u}, {"1e99999", 0x7f800000u}, {"1.17549435e-38", 0x00800000u}, {"1.17549e-38", 0x007fffe1u},
      {"1.4013e-45", 1u}, {"0000000000000000000000000000000000001.5", 0x3fc00000u}, {"1E0", 0x3f800000u},
      {"0.0000000000000000000000000000000001", 0x0704ec3du},
  };
  for (const auto &s : sp) { expect(s.t, s.b, bad); ++*n; }
  for (const char *t : {"0x10", "1e", "NA", "1.2.3", "--1", "e5", "nan(1)", "", "+", "-", ".", "1e+", "1e-", "e", "1f", "infinit",
                        "in", "na", "1 ", "+-1", "1e5.0", "0x1p3", "1d5", "-.e1"}) {
    expect_status(t, parseg::BAD, bad);
    ++*n;
  }
  // of the grammar, outside the exact domain: 20 digits, 41 bytes; and refused before that is asked
  for (const char *t : {"12345678901234567890", "1.2345678901234567890e5", "00000000000000000000000000000000000000001",
                        "0.000000000000000000000000000000000000001"}) {
    expect_status(t, parseg::NEEDS_HOST, bad);
    ++*n;
  }
  expect_status("12345678901234567890x", parseg::BAD, bad);
  expect_status("1234567890123456789", parseg::OK, bad);   // 19 digits
  expect_status("0001234567890123456789", parseg::OK, bad);  // leading zeros are not counted
  *n += 3;
}

int main(int argc, char **argv)
{
  const std::string mode = argc > 1 ? argv[1] : "quick";
  long bad = 0, n = 0, roundtrip = 0;
  if (mode == "all") {
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : bad, n, roundtrip)
    for (long hi = 0; hi < 65536; ++hi)
      for (uint32_t lo = 0; lo < 65536u; ++lo) {
        long b = 0, r = 0;
        check_float(((uint32_t)hi << 16) | lo, &b, &r);
        bad += b;
        roundtrip += r;
        ++n;
      }
    printf("%ld floats whose fmt_g6 text does not parse back to a float of the same text\n", roundtrip);
  } else {
    for (uint64_t b = 0; b < (1ull << 32); b += 1009) { check_float((uint32_t)b, &bad, nullptr); ++n; }
    for (uint32_t b = 0; b < 4096; ++b) {
      check_float(b, &bad, nullptr);
      check_float(0x80000000u + b, &bad, nullptr);
      check_float(0x7f7ff000u + b, &bad, nullptr);
      check_float(0x7f800000u + b * 2048u, &bad, nullptr);
      n += 4;
    }
    random_tokens(1000000, &bad, &n);
    midpoints(100000, &bad, &n);
    specials(&bad, &n);
  }
  printf("%ld values, %ld differences\n", n, bad);
  return bad != 0;
}
