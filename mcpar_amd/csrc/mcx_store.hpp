// mcx_store.hpp -- the derived store as the units that make one see it: mcx_derive.hip (a derive sweep writes one, and the
// mcx_store_* entry points live there) and mcx_clip.hip (mcx_rowset_store copies kept rows into one).
// Internal, as everything under csrc/ is.
#pragma once
#include "mcx_summary_kernels.hpp"

struct mcx_store {
  int device = 0, nc = 0, nout = 0, T = 0;
  DevBuf<float> x, ly;  // x'[T][nc][nout], ly'[T][nc]
  DevBuf<double> d;     // the analyses' scratch, as on_rows has it
  DevBuf<unsigned long long> h;
  DevBuf<uint32_t> u;
  DevStream st;
  StoreSpan span() const { return StoreSpan{x.p, ly.p, nc, nout, (int64_t)T}; }
  Bufs bufs() { return Bufs{&d, &h, &u}; }
  size_t rows() const { return (size_t)T * nc; }
  ~mcx_store()
  {
    if (st) (void)hipStreamSynchronize(st);  // (before the members go)
  }
};

// mcx_derive.hip's gather (k_gather_rows in chunks through one device buffer) for a span of any unit: n rows from row i0 on,
// or with draw the rows of draws i0 .. i0 + n - 1 of seed among the span's T * nc rows and their indices (index may be NULL),
// to the host in MCout layout
MCXI int gather_span(hipStream_t st, const StoreSpan &s, bool draw, uint32_t seed, uint64_t i0, uint64_t n, float *rows, int64_t *index);
// gather_span's sibling for section 28: the n <= 2^14 rows floor(k N / n), k < n, of the span's N = T * nc rows (n <= N), evenly
// spaced in store order, to the host in MCout layout; one chunk (mcx_derive.hip)
MCXI int gather_spaced(hipStream_t st, const StoreSpan &s, uint64_t n, float *rows);
// the rows of one chunk of that gather when n rows of ncol floats are asked for (mcx_derive.hip)
MCXI uint64_t gather_chunk_rows(uint64_t n, uint64_t ncol);

// Launch geometry, one function per sweep so that mcx_debug_store_geometry (mcx_derive.hip) reports what is launched.
// Workgroups of a sweep that gives each R consecutive rows of N (the derive and clip sweeps):
inline uint64_t sweep_tiles(uint64_t N, int R) { return (N + (uint64_t)R - 1) / (uint64_t)R; }
// the clip of N rows of np parameters (mcx_clip.hip)
struct ClipGeometry {
  int R, wpw;        // rows per workgroup, derive_rows(np, 0); mask words per workgroup
  size_t lds_bytes;  // of a workgroup's tile
  uint64_t nwg, nb;  // workgroups of the mark and scatter sweeps; scan blocks
};
MCXI ClipGeometry clip_geometry(int np, uint64_t N);

// Section 14's scan and scatter for any unit that has a keep mask in the clip's geometry g = clip_geometry(s.np, N) (mcx_clip.hip
// has them; section 25's rows of a mode come through here): mask[g.nwg][g.wpw], bit l of word w = row w * 64 + l of the
// workgroup is kept; cnt[g.nwg] the kept rows of each; scan[rowset_scan_words(g)] u64 words of scratch, all on the device
struct RowMask {
  const unsigned long long *mask;
  const uint32_t *cnt;
  unsigned long long *scan;  // offs[nwg] | bsum[nb] | boff[nb + 1]: boff[nb] is the total
};
inline size_t rowset_scan_words(const ClipGeometry &g) { return (size_t)g.nwg + 2 * (size_t)g.nb + 1; }
// the three scan launches: nothing is waited for
MCXI int rowset_scan(hipStream_t st, const RowMask &m, const ClipGeometry &g);
// a new row set of total rows of np parameters out of N, allocated with a stream of its own; then the one launch that scatters
// the rows the mask keeps (total as rowset_scan left it in boff[nb], read by the caller) into it: nothing is waited for
MCXI int rowset_new(int np, unsigned long long total, uint64_t N, std::unique_ptr<mcx_rowset> &o);
MCXI int rowset_scatter(hipStream_t st, const StoreSpan &s, const RowMask &m, const ClipGeometry &g, mcx_rowset &o);
// scan, the total, a new row set, scatter; waited for
MCXI int rowset_from_mask(hipStream_t st, const StoreSpan &s, const RowMask &m, const ClipGeometry &g, mcx_rowset **out);
