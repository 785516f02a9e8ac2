// gtok_decode_csr.hpp — what the two row decoders (gtok_sent_decode.hip, gtok_ibtt_decode.hip) share around their parsers: how a
// row is found and read, the slice of the output arrays a row claims, the row-pointer scan, what pass 2 reports in `info`, and
// the launchers' common start.  Everything is a template over the caller's own argument struct: no kernel-argument layout is
// decided here.
//
// gtok_csr_built.info after pass 2 (int32 [8], cleared by the launcher, accumulated by lane 0 of every wave):
//   [0] rows skipped: the recount of a row did not match the slice node_ptr / edge_ptr claim for it, or that slice does not lie
//       inside the arrays the two pointer arrays describe ("rows changed between the two passes") - nothing of the row is written
//   [1] the largest degree   [2] the largest node count   [3] the largest entry count   (of the rows that were built)
//   [4] [5] the largest claimed node / entry sum of an aligned group of 64 graphs (GraphBatch.chunk_nodes / chunk_edges)
//   [6] rows of status 1 (malformed: an empty graph)
//   [7] 1 when some row's entry list is not row-sorted as it stands (eorder is then not the identity)
#pragma once
#include "gtok_common.hpp"
#include "gtok_decode_args.hpp"

namespace gtok {

// ---- a row of ids.  A: a struct with ids, row_start, len, eb (bytes per id), ld
template <class A>
__device__ __forceinline__ int load_id(const A &a, int64_t at) {
  if (a.eb == 1) return (int)static_cast<const uint8_t *>(a.ids)[at];
  if (a.eb == 2) return (int)static_cast<const uint16_t *>(a.ids)[at];
  return static_cast<const int32_t *>(a.ids)[at];      // (as sent_decode_kernel reads them: a negative id is malformed wherever it stands)
}

// first element and token count of row r; a negative start or an empty row: L = 0 (status 1)
template <class A>
__device__ __forceinline__ void row_span(const A &a, int r, int64_t &base, int &L) {
  base = a.row_start ? sload(a.row_start, r) : (int64_t)r * a.ld;
  L = min(sload(a.len, r), a.ld);
  if (base < 0 || L < 0) L = 0;
}

// ---- pass 2: the per-wave accumulators of info[0..7] (above), reported once by lane 0
struct DecodeInfo {
  int bad = 0, max_deg = 0, max_n = 0, max_e = 0, chunk_n = 0, chunk_e = 0, malformed = 0, unsorted = 0;
  __device__ __forceinline__ void built(int n, int e) { max_n = max(max_n, n); max_e = max(max_e, e); }
  __device__ __forceinline__ void report(int32_t *info) const {
    if (lane_id() != 0) return;
    if (bad) atomicAdd(info + 0, bad);
    info_max(info + 1, max_deg); info_max(info + 2, max_n); info_max(info + 3, max_e);
    info_max(info + 4, chunk_n); info_max(info + 5, chunk_e);
    if (malformed) atomicAdd(info + 6, malformed);
    info_max(info + 7, unsorted);
  }
};

// ---- pass 2: the slice of the output arrays that node_ptr / edge_ptr claim for row r (all wave-uniform)
struct DecodeSlice {
  int nb; int64_t e0;   // first node, first entry
  bool ok;              // the slice lies inside the arrays the two pointer arrays describe; anything else is a row to skip
  int ncl, ecl;         // claimed nodes / entries (0, 0 when not ok)
};
struct DecodeTotals {
  int rows, ntot; int64_t etot;
  __device__ __forceinline__ DecodeTotals(const gtok_csr_built &out, int num_rows)
      : rows(num_rows), ntot(sload(out.node_ptr, num_rows)), etot(sload(out.edge_ptr, num_rows)) {}
};
// ... and, from the first row of an aligned group of 64 graphs, the group's claimed sums into info[4] / info[5]
__device__ __forceinline__ DecodeSlice claim_slice(const gtok_csr_built &out, const DecodeTotals &t, int r, int maxn, DecodeInfo &acc) {
  DecodeSlice s;
  s.nb = sload(out.node_ptr, r); s.e0 = sload(out.edge_ptr, r);
  const int ne = sload(out.node_ptr, r + 1);
  const int64_t e1 = sload(out.edge_ptr, r + 1);
  if ((r & 63) == 0) {
    const int rl = min(r + 64, t.rows);
    const int64_t cn = (int64_t)sload(out.node_ptr, rl) - s.nb, ce = sload(out.edge_ptr, rl) - s.e0;
    acc.chunk_n = max(acc.chunk_n, (int)min(max(cn, (int64_t)0), (int64_t)0x7FFFFFFF));
    acc.chunk_e = max(acc.chunk_e, (int)min(max(ce, (int64_t)0), (int64_t)0x7FFFFFFF));
  }
  s.ok = s.nb >= 0 && ne >= s.nb && ne <= t.ntot && ne - s.nb <= maxn && s.e0 >= 0 && e1 >= s.e0 && e1 <= t.etot && e1 - s.e0 <= 0x7FFFFFFF;
  s.ncl = s.ok ? ne - s.nb : 0; s.ecl = s.ok ? (int)(e1 - s.e0) : 0;
  return s;
}

// ---- pass 2: row pointers.  deg[0..n): the degrees of the row's n nodes (LDS); their exclusive scan goes to rowptr[0..n) and
// back into deg (the counters become the rows' cursors), rowptr[n] = e.  Returns the largest degree (in every lane).
__device__ __forceinline__ int scan_rowptr(int32_t *rowptr, int *deg, int n, int e) {
  const int lane = lane_id();
  int carry = 0, dmax = 0;
  for (int u0 = 0; u0 < n; u0 += kWave) {
    const int u = u0 + lane;
    const int d = u < n ? deg[u] : 0;
    const int incl = wave_incl_scan(d);
    if (u < n) { rowptr[u] = carry + incl - d; deg[u] = carry + incl - d; }
    dmax = max(dmax, d);
    carry += __builtin_amdgcn_readlane(incl, kWave - 1);
  }
  if (lane == 0) rowptr[n] = e;
  return wave_max(dmax);
}

// ---- the launchers' common start.  rows_check: the answer of *_decode_check_rows; outs_ok: the outputs are all there; out: pass
// 2's arrays (its info is cleared on the stream), nullptr for pass 1.  launch(dev, stream) runs with the stream's device current.
template <class Launch>
int decode_launch(int rows_check, bool outs_ok, const gtok_csr_built *out, void *stream, Launch launch) {
  if (rows_check) return rows_check < 0 ? rows_check : GTOK_OK;
  if (!outs_ok) return GTOK_E_INVAL;
  hipStream_t s = (hipStream_t)stream;
  DeviceScope device_scope(s);   // the stream's device, not the thread's current one
  if (!device_scope.ok()) return GTOK_E_NO_DEVICE;
  if (out && hipMemsetAsync(out->info, 0, 8 * sizeof(int32_t), s) != hipSuccess) return GTOK_E_LAUNCH;
  return launch(device_scope.dev, s);
}

}  // namespace gtok
