// mcx_parse.hip -- sample text read back on the GPU: mcx_text_store, mcx_text_rows, mcx_file_store.
// The reference's read.mc.data (src/anly/mcpar-analysis.R: read.table(filename)) for the text MCout::output prints, which
// mcx_samples_text and fmt_g6.hpp write; one token becomes one float by parse_g.hpp, the routine the host uses too.
//
// The host cuts the text into pieces at line ends, ends the last line with a newline if it has none, and pads a piece with
// blanks to whole 16-byte words.  Per piece, on 4 KiB tiles of 256 lanes x 16 bytes:
//   k_mark      every lane classifies its 16 bytes (separator, newline, other) in registers; a token starts where a
//               non-separator follows a separator or the piece's start; per-workgroup counts of token starts and of
//               newlines, packed into one u64, are all that reaches HBM
//   k_text_scan (mcx_text.hpp) the counts become offsets, the last word the piece's totals
//   k_scatter   the marks again; every token start writes its byte offset at its token index: the starts, compacted
//   k_parse     one lane per token: the token's end, its float (parse_g), a plain store at the place of (row, column) =
//               (index / ncol, index % ncol); then the separators behind the token: a newline is among them if and only if
//               the token is the last of its row, else the lowest such token index is kept (atomicMin).  A token outside the
//               grammar: the lowest index likewise.  A token parse_g leaves to the host: (byte offset, token index) into a list
//               of MCX_TEXT_FALLBACK_CAPACITY entries; the host converts those with strtof and k_poke stores them; a piece with
//               more of them is tokenised again on the host.
// A row's place does not depend on the number of rows (x'[row][ncol - 1], ly'[row]), so the store is allocated once for an
// upper bound of the rows -- the lines of the text, counted on the host before the first piece -- and the text crosses to
// the device once.  Integer atomics only, every float has one writer: the same text and arguments give the same bytes.
#include "mcx_store.hpp"

#include "mcx_text.hpp"
#include "parse_g.hpp"

#include <climits>
#include <locale.h>

namespace {

constexpr int PB = 256;                  // lanes per workgroup of the sweeps
constexpr size_t PIECE_DEFAULT = 32u << 20, PIECE_MAX = 1u << 30;
constexpr uint32_t FALLBACK_CAP = MCX_TEXT_FALLBACK_CAPACITY;
constexpr unsigned long long NONE = ~0ull;

__host__ __device__ inline bool is_sep(unsigned c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; }

struct PieceArgs {
  const char *text;
  uint32_t n;                         // bytes, a multiple of 16
  unsigned long long *counts;         // [nwg + 1]: token starts | newlines << 32 per workgroup; scanned: offsets, then the totals
  uint32_t nwg;
  uint32_t *starts;                   // [tokens of the piece]
  float *x, *ly;                      // x'[rows][ncol - 1], ly'[rows]
  uint64_t tok0, tok_end;             // token index of the piece's first token; tokens from tok_end on are not looked at
  uint32_t ncol;
  unsigned long long *words;          // [0] lowest token that breaks the structure, [1] lowest token outside the grammar, [2] tokens for the host
  uint2 *list;                        // [FALLBACK_CAP]: (byte offset, token index within the piece)
};

// bit j: byte j of the lane's 16 starts a token / is a newline
__device__ __forceinline__ void marks_of(const PieceArgs &a, uint32_t chunk, uint32_t &start, uint32_t &nl)
{
  start = nl = 0u;
  if (chunk >= a.n / 16u) return;
  const uint4 v = reinterpret_cast<const uint4 *>(a.text)[chunk];
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t sep = 0u;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const unsigned c = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
    sep |= (is_sep(c) ? 1u : 0u) << j;
    nl |= (c == '\n' ? 1u : 0u) << j;
  }
  const uint32_t prev = chunk == 0u || is_sep((unsigned char)a.text[(size_t)chunk * 16u - 1u]) ? 1u : 0u;
  start = ~sep & ((sep << 1) | prev) & 0xffffu;
}

__global__ void __launch_bounds__(PB) k_mark(const PieceArgs a)
{
  __shared__ unsigned long long part[PB / 64];
  uint32_t start, nl;
  marks_of(a, blockIdx.x * PB + threadIdx.x, start, nl);
  unsigned long long v = (unsigned long long)__popc(start) | ((unsigned long long)__popc(nl) << 32);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
#pragma unroll
    for (int w = 0; w < PB / 64; ++w) t += part[w];
    a.counts[blockIdx.x] = t;
  }
}

__global__ void __launch_bounds__(PB) k_scatter(const PieceArgs a)
{
  __shared__ uint32_t wave_sum[PB / 64];
  uint32_t start, nl;
  const uint32_t chunk = blockIdx.x * PB + threadIdx.x;
  marks_of(a, chunk, start, nl);
  const uint32_t mine = (uint32_t)__popc(start), lane = threadIdx.x & 63u;
  uint32_t incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(incl, o);
    if (lane >= (uint32_t)o) incl += v;
  }
  if (lane == 63u) wave_sum[threadIdx.x >> 6] = incl;
  __syncthreads();
  uint32_t k = (uint32_t)a.counts[blockIdx.x] + (incl - mine);
  for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) k += wave_sum[w];
  while (start) {  // (k < the piece's token starts <= n / 2 + 1, the size of starts)
    const int j = __ffs((int)start) - 1;
    start &= start - 1u;
    a.starts[k++] = chunk * 16u + (uint32_t)j;
  }
}

// 256-bit limbs: out of line, so that the lanes whose tokens parse_small takes do not carry their registers
__device__ __noinline__ uint32_t parse_big_device(uint64_t w, int q) { return parseg::parse_big(w, q); }

__device__ __forceinline__ int parse_device(const char *s, uint32_t len, uint32_t *bits)
{
  parseg::Scan t;
  const int st = parseg::scan(s, len, t);
  if (st != parseg::OK) return st;
  uint32_t b;
  if (t.word) {
    *bits = parseg::word_bits(t);
    return parseg::OK;
  }
  if (t.w == 0 || t.q < -65) b = 0u;
  else if (t.q > 38) b = 0x7f800000u;
  else if (!parseg::parse_small(t.w, t.q, &b)) b = parse_big_device(t.w, t.q);
  *bits = (t.neg ? 0x80000000u : 0u) | b;
  return parseg::OK;
}

// the float of token index kg (counted from the text's first kept token) goes to (row, column) = (kg / ncol, kg % ncol)
__device__ __forceinline__ void put_value(float *x, float *ly, uint64_t row, uint32_t col, uint32_t ncol, uint32_t bits)
{
  if (col + 1u < ncol) x[row * (uint64_t)(ncol - 1u) + col] = __uint_as_float(bits);
  else ly[row] = __uint_as_float(bits);
}

__global__ void __launch_bounds__(PB) k_parse(const PieceArgs a)
{
  const uint32_t k = blockIdx.x * PB + threadIdx.x;
  if (k >= (uint32_t)a.counts[a.nwg]) return;
  const uint64_t kg = a.tok0 + k;
  if (kg >= a.tok_end) return;
  const uint32_t b = a.starts[k];
  uint32_t e = b + 1u;
  while (e < a.n && !is_sep((unsigned char)a.text[e])) ++e;
  bool nl = false;
  for (uint32_t g = e; g < a.n; ++g) {
    const unsigned c = (unsigned char)a.text[g];
    if (!is_sep(c)) break;
    if (c == '\n') {
      nl = true;
      break;
    }
  }
  const uint32_t rowl = k / a.ncol, col = k - rowl * a.ncol;
  if (nl != (col + 1u == a.ncol)) atomicMin(&a.words[0], (unsigned long long)kg);
  uint32_t bits = 0u;
  const int st = parse_device(a.text + b, e - b, &bits);
  if (st == parseg::OK) put_value(a.x, a.ly, a.tok0 / a.ncol + rowl, col, a.ncol, bits);
  else if (st == parseg::BAD) atomicMin(&a.words[1], (unsigned long long)kg);
  else {
    const unsigned long long slot = atomicAdd(&a.words[2], 1ull);
    if (slot < FALLBACK_CAP) a.list[slot] = make_uint2(b, k);
  }
}

// the values the host converted: token index kg[i] gets bits[i]
__global__ void __launch_bounds__(PB) k_poke(const unsigned long long *kg, const uint32_t *bits, uint32_t n, float *x, float *ly,
                                             uint32_t ncol)
{
  const uint32_t i = blockIdx.x * PB + threadIdx.x;
  if (i >= n) return;
  const uint64_t row = kg[i] / ncol;
  put_value(x, ly, row, (uint32_t)(kg[i] - row * ncol), ncol, bits[i]);
}

// ---- the host side

uint32_t strtof_bits(const char *tok, size_t len)
{
  static const locale_t c_locale = newlocale(LC_ALL_MASK, "C", (locale_t)0);
  const std::string z(tok, len);
  const float f = c_locale ? strtof_l(z.c_str(), nullptr, c_locale) : strtof(z.c_str(), nullptr);
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}

// parse_g on the host, and strtof where it asks for the host: OK / BAD, *fallback set when strtof was taken
int host_token(const char *tok, size_t len, uint32_t *bits, bool *fallback)
{
  *fallback = false;
  const int st = parseg::parse(tok, len, bits);
  if (st != parseg::NEEDS_HOST) return st;
  *bits = strtof_bits(tok, len);
  *fallback = true;
  return parseg::OK;
}

// where the text comes from: memory, or a file read in pieces
struct Source {
  const char *mem = nullptr;
  size_t n = 0, pos = 0;
  FILE *f = nullptr;
  size_t read(char *dst, size_t want)
  {
    if (f) return fread(dst, 1, want, f);
    const size_t got = std::min(want, n - pos);
    memcpy(dst, mem + pos, got);
    pos += got;
    return got;
  }
  bool at_end()
  {
    if (!f) return pos == n;
    const int c = fgetc(f);
    if (c == EOF) return true;
    ungetc(c, f);
    return false;
  }
  int seek(size_t off)
  {
    if (!f) {
      pos = off;
      return MCX_OK;
    }
    return fseeko(f, (off_t)off, SEEK_SET) == 0 ? MCX_OK : fail(MCX_ERR_INVALID, "cannot seek in the file: %s", strerror(errno));
  }
};

// newlines among n bytes: 64 byte-wide counters for 255 rounds at a time, a loop the compiler turns into byte compares
// (std::count widens every byte first: a fifth of the speed)
uint64_t count_newlines(const char *p, size_t n)
{
  uint64_t total = 0;
  size_t i = 0;
  while (i + 64 <= n) {
    uint8_t acc[64] = {0};
    for (int round = 0; round < 255 && i + 64 <= n; ++round, i += 64)
      for (int j = 0; j < 64; ++j) acc[j] += (uint8_t)(p[i + j] == '\n');
    for (int j = 0; j < 64; ++j) total += acc[j];
  }
  for (; i < n; ++i) total += p[i] == '\n';
  return total;
}

// the pass before the first piece, on the host: where the kept text begins, an upper bound of its rows (its lines), and
// the fields of its first line that holds any
struct Prescan {
  int64_t skip;            // lines still to skip
  size_t start = 0;        // bytes skipped
  uint64_t lines = 0;      // newlines of the kept text
  bool tail = false;       // the kept text does not end with a newline
  int first = 0;           // fields of the first kept line that has any
  bool first_done = false, in_token = false;
  void feed(const char *p, size_t n)
  {
    size_t i = 0;
    while (skip > 0 && i < n) {
      const char *q = (const char *)memchr(p + i, '\n', n - i);
      if (!q) {
        start += n - i;
        return;
      }
      start += (size_t)(q - (p + i)) + 1;
      i = (size_t)(q - p) + 1;
      --skip;
    }
    if (i >= n) return;
    for (size_t j = i; j < n && !first_done; ++j) {
      const unsigned c = (unsigned char)p[j];
      if (!is_sep(c)) {
        if (!in_token) ++first;
        in_token = true;
      } else {
        in_token = false;
        if (c == '\n' && first) first_done = true;
      }
    }
    lines += count_newlines(p + i, n - i);
    tail = p[n - 1] != '\n';
  }
};

int prescan(Source &src, Prescan &ps)
{
  if (!src.f) {
    ps.feed(src.mem, src.n);
    return MCX_OK;
  }
  std::vector<char> buf(4u << 20);
  for (size_t got; (got = fread(buf.data(), 1, buf.size(), src.f)) > 0;) ps.feed(buf.data(), got);
  if (ferror(src.f)) return fail(MCX_ERR_INVALID, "reading the file failed: %s", strerror(errno));
  return MCX_OK;
}

// The first thing wrong with a piece, as parse_ref (tests/parse_ref.py) names it: lines in order; a line with fields but not
// ncol of them: "line L: K fields, expected ncol"; else its first field outside the grammar: "line L, field F".  line0 = lines
// before the piece, rows_left = rows still wanted.  MCX_OK when nothing is wrong.
int diagnose(const char *p, size_t n, uint64_t line0, uint32_t ncol, uint64_t rows_left)
{
  uint64_t line = line0;
  for (size_t i = 0; i < n && rows_left > 0;) {
    const char *q = (const char *)memchr(p + i, '\n', n - i);
    const size_t end = q ? (size_t)(q - p) : n;
    ++line;
    uint32_t fields = 0, badfield = 0;
    for (size_t j = i; j < end;) {
      while (j < end && is_sep((unsigned char)p[j])) ++j;
      if (j >= end) break;
      size_t e = j;
      while (e < end && !is_sep((unsigned char)p[e])) ++e;
      ++fields;
      uint32_t bits;
      bool fb;
      if (!badfield && fields <= ncol && host_token(p + j, e - j, &bits, &fb) == parseg::BAD) badfield = fields;
      j = e;
    }
    if (fields) {
      if (fields != ncol)
        return fail(MCX_ERR_INVALID, "line %llu: %u fields, expected %u", (unsigned long long)line, fields, ncol);
      if (badfield) return fail(MCX_ERR_INVALID, "line %llu, field %u is not a number", (unsigned long long)line, badfield);
      --rows_left;
    }
    i = end + 1;
  }
  return MCX_OK;
}

struct TextJob {
  const mcx_text_spec *spec;
  mcx_text_report *rep;
  mcx_store **out;        // mcx_text_store / mcx_file_store
  float *rows;            // mcx_text_rows
  int64_t capacity_rows;
  bool want_rows;
  double *ms;             // mcx_debug_text_times, else NULL
};

int spec_args(const mcx_text_spec *spec)
{
  if (!spec) return fail(MCX_ERR_INVALID, "spec is NULL");
  if (spec->ncol != 0 && (spec->ncol < 2 || spec->ncol > 257))
    return fail(MCX_ERR_INVALID, "ncol = %d: 2 to 257 columns per line, or 0 for those of the first line", spec->ncol);
  if (spec->nc < 1) return fail(MCX_ERR_INVALID, "nc = %d: at least one chain", spec->nc);
  if (spec->skip_lines < 0) return fail(MCX_ERR_INVALID, "skip_lines = %lld is negative", (long long)spec->skip_lines);
  if (spec->piece_bytes != 0 && (spec->piece_bytes < 64 || spec->piece_bytes > PIECE_MAX))
    return fail(MCX_ERR_INVALID, "piece_bytes = %zu: 0 for the default, else 64 to %zu", spec->piece_bytes, PIECE_MAX);
  return MCX_OK;
}

int parse_source(Source &src, const TextJob &job)
{
  using clk = std::chrono::steady_clock;
  const clk::time_point t_call = clk::now();
  const mcx_text_spec &sp = *job.spec;
  Prescan ps;
  ps.skip = sp.skip_lines;
  MCXCHK(prescan(src, ps));
  const double ms_prescan = std::chrono::duration<double, std::milli>(clk::now() - t_call).count();
  const int ncoli = sp.ncol ? sp.ncol : ps.first;
  if (ncoli < 2 || ncoli > 257)
    return fail(MCX_ERR_INVALID, "the first line has %d fields: 2 to 257 columns per line", ncoli);
  const uint32_t ncol = (uint32_t)ncoli;
  uint64_t rows_cap = ps.lines + (ps.tail ? 1u : 0u);
  if (sp.max_rows >= 0) rows_cap = std::min<uint64_t>(rows_cap, (uint64_t)sp.max_rows);
  if (rows_cap == 0) return fail(MCX_ERR_INVALID, "the text holds no rows");
  MCXCHK(src.seek(ps.start));
  MCXCHK(need_device());

  const size_t piece = sp.piece_bytes ? sp.piece_bytes : PIECE_DEFAULT;
  const size_t cap_dev = (piece + 1 + 15) / 16 * 16;  // a piece, the newline its last line may lack, whole 16-byte words
  const uint32_t nwg_max = (uint32_t)((cap_dev / 16 + PB - 1) / PB);
  const size_t ntok_max = cap_dev / 2 + 2;
  std::unique_ptr<mcx_store> o(new mcx_store);
  HIPCHK(hipGetDevice(&o->device));
  DevBuf<char> dtext;
  DevBuf<unsigned long long> counts, words, pk;
  DevBuf<uint32_t> starts, pb;
  DevBuf<uint2> list;
  PinBuf<char> stage[2];
  PinBuf<unsigned long long> hw;   // the piece's totals, then its three words
  PinBuf<uint2> hlist;
  const size_t need = (size_t)rows_cap * ncol * sizeof(float) + cap_dev + (nwg_max + 1 + 3) * sizeof(unsigned long long) +
                      ntok_max * sizeof(uint32_t) + FALLBACK_CAP * sizeof(uint2);
  auto allocs = [&]() -> int {
    MCXCHK(o->st.ensure(hipStreamNonBlocking));
    MCXCHK(o->x.alloc((size_t)rows_cap * (ncol - 1)));
    MCXCHK(o->ly.alloc((size_t)rows_cap));
    MCXCHK(dtext.alloc(cap_dev));
    MCXCHK(counts.alloc(nwg_max + 1));
    MCXCHK(words.alloc(3));
    MCXCHK(starts.alloc(ntok_max));
    MCXCHK(list.alloc(FALLBACK_CAP));
    MCXCHK(stage[0].alloc(cap_dev));
    MCXCHK(stage[1].alloc(cap_dev));
    MCXCHK(hw.alloc(4));
    MCXCHK(hlist.alloc(FALLBACK_CAP));
    return MCX_OK;
  };
  const int arc = allocs();
  if (arc == MCX_ERR_ALLOC)
    return fail(MCX_ERR_ALLOC, "text store: %zu bytes of device memory are needed (%llu rows of %u columns, pieces of %zu bytes; DESIGN.md section 18)",
                need, (unsigned long long)rows_cap, ncol, piece);
  MCXCHK(arc);
  hipStream_t st = o->st;
  StageTimer tm{st, job.ms, 5, {}};
  double ms_stage = 0.0;

  const uint64_t tok_end = rows_cap * ncol;
  uint64_t tok0 = 0, line0 = (uint64_t)sp.skip_lines - (uint64_t)ps.skip, nfallback = 0, npieces = 0;
  size_t have = 0;
  int cur = 0;
  std::vector<unsigned long long> fix_kg;
  std::vector<uint32_t> fix_bits;
  auto piece_loop = [&]() -> int {
    for (;;) {
      if (sp.max_rows >= 0 && tok0 >= tok_end) break;
      const clk::time_point t_stage = clk::now();
      char *buf = stage[cur].p;
      have += src.read(buf + have, piece - have);
      if (src.f && ferror(src.f)) return fail(MCX_ERR_INVALID, "reading the file failed: %s", strerror(errno));
      if (have == 0) break;
      size_t cut = have;
      if (!(have <= piece && src.at_end())) {
        const char *q = (const char *)memrchr(buf, '\n', have);
        if (!q) return fail(MCX_ERR_INVALID, "line %llu is longer than a piece of %zu bytes", (unsigned long long)(line0 + 1), piece);
        cut = (size_t)(q - buf) + 1;
      }
      const size_t carry = have - cut;
      if (carry) memcpy(stage[cur ^ 1].p, buf + cut, carry);  // the next piece's beginning
      size_t n = cut;
      if (buf[n - 1] != '\n') buf[n++] = '\n';  // (the text's last line)
      while (n % 16) buf[n++] = ' ';
      ms_stage += std::chrono::duration<double, std::milli>(clk::now() - t_stage).count();

      PieceArgs a{dtext.p, (uint32_t)n, counts.p, (uint32_t)((n / 16 + PB - 1) / PB), starts.p, o->x.p, o->ly.p, tok0, tok_end, ncol,
                  words.p, list.p};
      hw.p[1] = hw.p[2] = NONE;
      hw.p[3] = 0;
      MCXCHK(tm.run(0, [&]() -> int {
        HIPCHK(hipMemcpyAsync(dtext.p, buf, n, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(words.p, hw.p + 1, 3 * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
        return MCX_OK;
      }));
      MCXCHK(tm.run(1, [&]() -> int {
        hipLaunchKernelGGL(k_mark, dim3(a.nwg), dim3(PB), 0, st, a);
        HIPCHK(hipGetLastError());
        return MCX_OK;
      }));
      MCXCHK(tm.run(2, [&]() -> int {
        hipLaunchKernelGGL(k_text_scan, dim3(1), dim3(1024), 0, st, counts.p, (size_t)a.nwg);
        HIPCHK(hipGetLastError());
        return MCX_OK;
      }));
      MCXCHK(tm.run(3, [&]() -> int {
        hipLaunchKernelGGL(k_scatter, dim3(a.nwg), dim3(PB), 0, st, a);
        HIPCHK(hipGetLastError());
        return MCX_OK;
      }));
      MCXCHK(tm.run(4, [&]() -> int {  // (a grid for the most tokens n bytes can hold: the lanes past the count leave at once)
        hipLaunchKernelGGL(k_parse, dim3((unsigned)((n / 2 + 1 + PB - 1) / PB)), dim3(PB), 0, st, a);
        HIPCHK(hipGetLastError());
        return MCX_OK;
      }));
      HIPCHK(hipMemcpyAsync(hw.p, counts.p + a.nwg, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(hw.p + 1, words.p, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      const uint64_t ntok = hw.p[0] & 0xffffffffull, nlines = hw.p[0] >> 32;
      const uint64_t nproc = std::min<uint64_t>(ntok, tok_end - tok0), nhost = hw.p[3];
      bool wrong = hw.p[1] != NONE || hw.p[2] != NONE;
      fix_kg.clear();
      fix_bits.clear();
      auto host_fix = [&](uint32_t ofs, uint32_t k) {
        size_t e = ofs;
        while (e < n && !is_sep((unsigned char)buf[e])) ++e;
        uint32_t bits = 0;
        bool fb;
        if (host_token(buf + ofs, e - ofs, &bits, &fb) != parseg::OK) {
          wrong = true;
          return;
        }
        if (!fb) return;  // (the device has stored it)
        ++nfallback;
        fix_kg.push_back(tok0 + k);
        fix_bits.push_back(bits);
      };
      if (!wrong && nhost > FALLBACK_CAP) {  // the list did not hold them: every token of the piece again, on the host
        uint32_t k = 0;
        for (size_t i = 0; i < n && k < nproc;) {
          while (i < n && is_sep((unsigned char)buf[i])) ++i;
          if (i >= n) break;
          host_fix((uint32_t)i, k++);
          while (i < n && !is_sep((unsigned char)buf[i])) ++i;
        }
      } else if (!wrong && nhost) {
        HIPCHK(hipMemcpy(hlist.p, list.p, nhost * sizeof(uint2), hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < nhost; ++i) host_fix(hlist.p[i].x, hlist.p[i].y);
      }
      if (wrong) {
        MCXCHK(diagnose(buf, cut, line0, ncol, (tok_end - tok0) / ncol));
        return fail(MCX_ERR_HIP, "the device refused a piece in which the host finds nothing wrong (tokens %llu, %llu)",
                    (unsigned long long)hw.p[1], (unsigned long long)hw.p[2]);
      }
      if (!fix_kg.empty()) {
        const uint32_t nf = (uint32_t)fix_kg.size();
        MCXCHK(pk.alloc(nf));
        MCXCHK(pb.alloc(nf));
        HIPCHK(hipMemcpyAsync(pk.p, fix_kg.data(), nf * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(pb.p, fix_bits.data(), nf * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_poke, dim3((nf + PB - 1) / PB), dim3(PB), 0, st, pk.p, pb.p, nf, o->x.p, o->ly.p, ncol);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
      }
      tok0 += nproc;
      line0 += nlines;
      ++npieces;
      have = carry;
      cur ^= 1;
    }
    return MCX_OK;
  };
  const int rc = piece_loop();
  if (rc != MCX_OK) (void)hipStreamSynchronize(st);  // (before the buffers go)
  MCXCHK(rc);

  const uint64_t nrows = tok0 / ncol;
  if (nrows == 0) return fail(MCX_ERR_INVALID, "the text holds no rows");
  if (nrows % (uint64_t)sp.nc)
    return fail(MCX_ERR_INVALID, "%llu rows are not a multiple of nc = %d", (unsigned long long)nrows, sp.nc);
  if (nrows / (uint64_t)sp.nc > (uint64_t)INT_MAX)
    return fail(MCX_ERR_UNSUPPORTED, "%llu rows of %d chains are more steps than a store counts", (unsigned long long)nrows, sp.nc);
  o->nc = sp.nc;
  o->nout = (int)ncol - 1;
  o->T = (int)(nrows / (uint64_t)sp.nc);
  if (job.want_rows && job.rows) {
    if ((uint64_t)std::max<int64_t>(job.capacity_rows, 0) < nrows)
      return fail(MCX_ERR_INVALID, "capacity_rows = %lld, the text holds %llu rows", (long long)job.capacity_rows, (unsigned long long)nrows);
    MCXCHK(gather_span(st, o->span(), false, 0u, 0, nrows, job.rows, nullptr));
  }
  MCXCHK(tm.collect());
  if (job.ms) {
    job.ms[5] = ms_prescan;
    job.ms[6] = ms_stage;
    job.ms[7] = std::chrono::duration<double, std::milli>(clk::now() - t_call).count();
  }
  if (job.rep) {
    job.rep->nrows = (int64_t)nrows;
    job.rep->nlines = (int64_t)line0;
    job.rep->ntokens = (int64_t)tok0;
    job.rep->nfallback = (int64_t)nfallback;
    job.rep->npieces = (int64_t)npieces;
    job.rep->ncol = (int)ncol;
  }
  if (job.out) *job.out = o.release();  // (the unique_ptr's: the store is the caller's now)
  return MCX_OK;
}

int memory_job(const char *text, size_t nbytes, const TextJob &job)
{
  if (job.out) *job.out = nullptr;
  if (!text) return fail(MCX_ERR_INVALID, "text is NULL");
  MCXCHK(spec_args(job.spec));
  Source src;
  src.mem = text;
  src.n = nbytes;
  return parse_source(src, job);
}

}  // namespace

extern "C" int mcx_text_store(const char *text, size_t nbytes, const mcx_text_spec *spec, mcx_store **out, mcx_text_report *rep)
{
  if (!out) return fail(MCX_ERR_INVALID, "out is NULL");
  return memory_job(text, nbytes, TextJob{spec, rep, out, nullptr, 0, false, nullptr});
}

extern "C" int mcx_text_rows(const char *text, size_t nbytes, const mcx_text_spec *spec, float *rows, int64_t capacity_rows,
                             mcx_text_report *rep)
{
  if (!rows && !rep) return fail(MCX_ERR_INVALID, "rows and rep are both NULL");
  return memory_job(text, nbytes, TextJob{spec, rep, nullptr, rows, capacity_rows, true, nullptr});
}

extern "C" int mcx_file_store(const char *path, const mcx_text_spec *spec, mcx_store **out, mcx_text_report *rep)
{
  if (!out) return fail(MCX_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (!path) return fail(MCX_ERR_INVALID, "path is NULL");
  MCXCHK(spec_args(spec));
  std::unique_ptr<FILE, int (*)(FILE *)> f(fopen(path, "rb"), fclose);
  if (!f) return fail(MCX_ERR_INVALID, "cannot open %s: %s", path, strerror(errno));
  Source src;
  src.f = f.get();
  return parse_source(src, TextJob{spec, rep, out, nullptr, 0, false, nullptr});
}

// mcx_text_store with its stages timed, for tools/parse_bench.py; the store is let go.  ms[8]: upload, mark, scan, scatter,
// parse (HIP events, summed over the pieces), the host's line count, its staging of the pieces, the whole call (wall clock)
extern "C" int mcx_debug_text_times(const char *text, size_t nbytes, const mcx_text_spec *spec, mcx_text_report *rep, double *ms)
{
  if (!ms) return fail(MCX_ERR_INVALID, "ms is NULL");
  return memory_job(text, nbytes, TextJob{spec, rep, nullptr, nullptr, 0, false, ms});
}

// host only
extern "C" int mcx_debug_parse_token(const char *tok, size_t len, uint32_t *bits, int *status)
{
  if (!tok || !bits || !status) return fail(MCX_ERR_INVALID, "tok, bits or status is NULL");
  *bits = 0u;
  *status = parseg::parse(tok, len, bits);
  if (*status == parseg::NEEDS_HOST) *bits = strtof_bits(tok, len);
  return MCX_OK;
}
