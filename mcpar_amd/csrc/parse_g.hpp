// parse_g.hpp -- one token of sample text -> the float glibc's strtof gives for it in the "C" locale: the inverse of
// fmt_g6.hpp, built the same way.  Correctly rounded, ties to even, in integer arithmetic (one fp64 quotient is an estimate
// that an exact comparison then settles, as in fmt_g6.hpp), by one routine that compiles for the host and for gfx950:
// same bits everywhere, no libm, no locale.
//
//   token    [+-]? ( D+ ( . D* )? | . D+ ) ( [eE] [+-]? D+ )?   |   [+-]? inf | infinity | nan, in any letter case
//   value    the digits without their leading zeros are w, the point and the exponent give q: value = w 10^q.
//   domain   at most MAX_BYTES = 40 bytes and MAX_DIGITS = 19 digits from the first non-zero one on: w < 10^19 < 2^64.  A
//            token of the grammar outside that domain is not converted: NEEDS_HOST, and the caller takes strtof to it.
//   range    w = 0: +-0.  q > 38: w 10^q >= 10^39 > FLT_MAX: +-inf.  q < -65: w 10^q < 10^-46 < 2^-150: +-0.
//   q >= 0   N = w 10^q < 2^64 10^38 < 2^191, an integer in 256 bits; its top 64 bits and "any bit below them set" round it.
//   q < 0    D = 10^-q <= 10^65 < 2^216.  With s = 25 + bits(D) - bits(w) the quotient Q = floor(w 2^s / D) lies in
//            [2^24, 2^26): s >= 0: num = w 2^s < 2^(25 + 216), den = D; s < 0: num = w, den = D 2^-s < 2^64.  Q is estimated
//            in fp64 from the limbs and corrected on the exact product Q den against num; value = (Q + f) 2^-s, 0 <= f < 1,
//            f != 0 iff the remainder is not 0.
//   round    value = (Q + f) 2^-s with Q >= 2^24 or f = 0.  ulp exponent u = max(floor(log2 value) - 23, -149), m = value / 2^u
//            rounded on the bits of Q below 2^(s + u), the tie broken to even with f as the sticky bit; bits = ((u + 149) << 23)
//            + m serves denormals (u = -149, m < 2^23), normals and the carry m = 2^24 alike; >= 0x7f800000: inf.
//   q in [-11, 19] with N or num in 64 bits -- every field fmt_g6 writes for 1e-6 <= |value| < 1e6 -- needs no 256-bit limb:
//            parse_small does those, and the callers on the GPU keep parse_big out of line.
#pragma once
#include "fmt_g6.hpp"

#if defined(__HIPCC__)
#define PARSEG_HD __host__ __device__ inline
#else
#define PARSEG_HD inline
#endif

namespace parseg {

enum { OK = 0, BAD = 1, NEEDS_HOST = 2 };
enum { MAX_BYTES = 40, MAX_DIGITS = 19 };

using fmtg6::Big;

PARSEG_HD int bits64(uint64_t v)  // bit length, 0 for 0
{
  int n = 0;
  if (v >> 32) { n += 32; v >>= 32; }
  if (v >> 16) { n += 16; v >>= 16; }
  if (v >> 8) { n += 8; v >>= 8; }
  if (v >> 4) { n += 4; v >>= 4; }
  if (v >> 2) { n += 2; v >>= 2; }
  if (v >> 1) { n += 1; v >>= 1; }
  return n + (int)v;
}

// (Q + f) 2^-s, sticky = (f != 0), to float bits without the sign; Q != 0, and Q >= 2^24 wherever sticky is set
PARSEG_HD uint32_t round_to_float(uint64_t Q, int s, bool sticky)
{
  const int ev = bits64(Q) - 1 - s;
  const int u = ev - 23 > -149 ? ev - 23 : -149;
  if (u + 149 >= 255) return 0x7f800000u;
  const int r = s + u;  // m = value 2^-u = (Q + f) 2^-r
  uint64_t m;
  if (r <= 0) m = Q << -r;  // (exact: -r <= 23 and Q < 2^24 here)
  else if (r > 64) m = 0;   // value < ulp / 2
  else {
    m = r == 64 ? 0 : Q >> r;
    const uint64_t half = (Q >> (r - 1)) & 1u;
    const bool low = (r >= 2 && (Q & ((1ull << (r - 1)) - 1ull)) != 0) || sticky;
    if (half && (low || (m & 1u))) ++m;
  }
  const uint64_t b = ((uint64_t)(u + 149) << 23) + m;
  return b >= 0x7f800000ull ? 0x7f800000u : (uint32_t)b;
}

// a <<= s, 0 <= s < 256, with every limb index a constant: whole limbs by three conditional moves, then the bits
PARSEG_HD void big_shl_static(Big &a, int s)
{
  const int ws = s >> 5, bs = s & 31;
  if (ws & 4) {
    for (int i = 7; i >= 4; --i) a.w[i] = a.w[i - 4];
    for (int i = 3; i >= 0; --i) a.w[i] = 0u;
  }
  if (ws & 2) {
    for (int i = 7; i >= 2; --i) a.w[i] = a.w[i - 2];
    a.w[1] = a.w[0] = 0u;
  }
  if (ws & 1) {
    for (int i = 7; i >= 1; --i) a.w[i] = a.w[i - 1];
    a.w[0] = 0u;
  }
  if (bs) {
    for (int i = 7; i >= 1; --i) a.w[i] = (a.w[i] << bs) | (a.w[i - 1] >> (32 - bs));
    a.w[0] <<= bs;
  }
}

PARSEG_HD int big_bits(const Big &a)
{
  int n = 0;
  for (int i = 0; i < 8; ++i)
    if (a.w[i]) n = 32 * i + bits64(a.w[i]);
  return n;
}

PARSEG_HD void big_set64(Big &a, uint64_t v)
{
  fmtg6::big_set(a, (uint32_t)v);
  a.w[1] = (uint32_t)(v >> 32);
}

PARSEG_HD uint64_t pow10_u64(int p)  // p <= 19
{
  uint64_t d = 1;
  for (int i = 0; i < p; ++i) d *= 10u;
  return d;
}

PARSEG_HD uint64_t mulhi64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// w 10^q, w != 0, where 64 bits hold it: true and the bits, else false
PARSEG_HD bool parse_small(uint64_t w, int q, uint32_t *bits)
{
  if (q >= 0) {
    if (q > 19) return false;
    const uint64_t d = pow10_u64(q);
    if (mulhi64(w, d)) return false;
    *bits = round_to_float(w * d, 0, false);
    return true;
  }
  if (q < -11) return false;  // bits(10^11) = 37: 25 + 37 <= 64
  const uint64_t D = pow10_u64(-q);
  const int s = 25 + bits64(D) - bits64(w);
  const uint64_t num = s >= 0 ? w << s : w, den = s >= 0 ? D : D << -s;
  const uint64_t Q = num / den;
  *bits = round_to_float(Q, s, num - Q * den != 0);
  return true;
}

// w 10^q, w != 0, -65 <= q <= 38, in 256-bit limbs
PARSEG_HD uint32_t parse_big(uint64_t w, int q)
{
  Big num;
  big_set64(num, w);
  if (q >= 0) {
    fmtg6::big_mul_pow10(num, q);
    const int L = big_bits(num);
    if (L <= 64) return round_to_float((uint64_t)num.w[0] | ((uint64_t)num.w[1] << 32), 0, false);
    big_shl_static(num, 256 - L);  // the top bit to bit 255
    bool sticky = false;
    for (int i = 0; i < 6; ++i) sticky = sticky || num.w[i] != 0u;
    return round_to_float((uint64_t)num.w[6] | ((uint64_t)num.w[7] << 32), 64 - L, sticky);
  }
  Big den;
  fmtg6::big_set(den, 1u);
  fmtg6::big_mul_pow10(den, -q);
  const int s = 25 + big_bits(den) - bits64(w);
  if (s >= 0) big_shl_static(num, s);
  else big_shl_static(den, -s);
  double dn = 0.0, dd = 0.0;
  for (int i = 7; i >= 0; --i) {
    dn = dn * 4294967296.0 + (double)num.w[i];
    dd = dd * 4294967296.0 + (double)den.w[i];
  }
  uint32_t n = (uint32_t)(dn / dd);  // < 2^26, off by one at the most
  Big prod = den;
  fmtg6::big_mul_small(prod, n);
  while (fmtg6::big_cmp(prod, num) > 0) {  // n too large
    --n;
    fmtg6::big_sub(prod, den);
  }
  Big rem = num;
  fmtg6::big_sub(rem, prod);
  while (fmtg6::big_cmp(rem, den) >= 0) {  // n too small
    ++n;
    fmtg6::big_sub(rem, den);
  }
  bool sticky = false;
  for (int i = 0; i < 8; ++i) sticky = sticky || rem.w[i] != 0u;
  return round_to_float(n, s, sticky);
}

PARSEG_HD char lower(char c) { return c >= 'A' && c <= 'Z' ? (char)(c + 32) : c; }

PARSEG_HD bool word_is(const char *s, size_t at, size_t len, const char *word, size_t wlen)
{
  if (len != wlen) return false;
  for (size_t i = 0; i < len; ++i)
    if (lower((char)s[at + i]) != word[i]) return false;
  return true;
}

// What the grammar makes of a token: OK and (neg, w, q) of a number, or word = 1 inf / 2 nan; BAD; NEEDS_HOST for a token of
// the grammar outside the exact domain (w and q are then not meant)
struct Scan {
  uint64_t w;
  int q, word;
  bool neg;
};

PARSEG_HD int scan(const char *s, size_t len, Scan &o)
{
  o.w = 0;
  o.q = 0;
  o.word = 0;
  o.neg = false;
  size_t i = 0;
  if (i < len && ((char)s[i] == '+' || (char)s[i] == '-')) o.neg = (char)s[i++] == '-';
  if (i >= len) return BAD;
  const char c0 = lower((char)s[i]);
  if (c0 == 'i' || c0 == 'n') {
    if (word_is(s, i, len - i, "inf", 3) || word_is(s, i, len - i, "infinity", 8)) o.word = 1;
    else if (word_is(s, i, len - i, "nan", 3)) o.word = 2;
    else return BAD;
    return OK;
  }
  int nd = 0, nsig = 0, nfrac = 0;  // digits of the mantissa, those from the first non-zero one on, those behind the point
  bool point = false;
  for (; i < len; ++i) {
    const char c = (char)s[i];
    if (c == '.') {
      if (point) return BAD;
      point = true;
      continue;
    }
    if (c < '0' || c > '9') break;
    ++nd;
    if (nsig || c != '0') {
      if (nsig < MAX_DIGITS) o.w = o.w * 10u + (uint64_t)(c - '0');
      if (nsig <= MAX_DIGITS) ++nsig;
    }
    if (point && nfrac < (1 << 28)) ++nfrac;
  }
  if (nd == 0) return BAD;
  int ex = 0;
  if (i < len) {
    if ((char)s[i] != 'e' && (char)s[i] != 'E') return BAD;
    ++i;
    bool eneg = false;
    if (i < len && ((char)s[i] == '+' || (char)s[i] == '-')) eneg = (char)s[i++] == '-';
    if (i >= len) return BAD;
    for (; i < len; ++i) {
      const char c = (char)s[i];
      if (c < '0' || c > '9') return BAD;
      if (ex < 100000) ex = ex * 10 + (c - '0');
    }
    if (eneg) ex = -ex;
  }
  if (nsig > MAX_DIGITS || len > (size_t)MAX_BYTES) return NEEDS_HOST;
  o.q = ex - nfrac;  // (len <= 40 here: no overflow)
  return OK;
}

PARSEG_HD uint32_t word_bits(const Scan &t) { return (t.neg ? 0x80000000u : 0u) | (t.word == 1 ? 0x7f800000u : 0x7fc00000u); }

// The routine.  *bits is written with OK only.
PARSEG_HD int parse(const char *s, size_t len, uint32_t *bits)
{
  Scan t;
  const int st = scan(s, len, t);
  if (st != OK) return st;
  const uint32_t sign = t.neg ? 0x80000000u : 0u;
  if (t.word) {
    *bits = word_bits(t);
    return OK;
  }
  uint32_t b;
  if (t.w == 0 || t.q < -65) b = 0u;
  else if (t.q > 38) b = 0x7f800000u;
  else if (!parse_small(t.w, t.q, &b)) b = parse_big(t.w, t.q);
  *bits = sign | b;
  return OK;
}

}  // namespace parseg
