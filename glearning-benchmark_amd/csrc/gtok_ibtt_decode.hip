// gtok_ibtt_decode.hip — IBTT rows back to a batched CSR (include/gtok.h: gtok_ibtt_decode_sizes / gtok_ibtt_decode_csr).
//
// One wave per row.  Both grammars are positional (a header, fixed-stride records, a fixed tail), so the parse runs on the
// VECTOR side: a lane takes one record per step, loads its tokens (1 / 2 / 4 bytes, widened in registers), bounds-checks
// the id and looks its class up in `inv`; a ballot over "this record is not valid" gives the end of a region.  What is left
// after the last record (at most four tokens) is judged once, wave-uniformly.  No token is taken one at a time.
//
// row_shape() finds a row's status, node count, entry count and record count; for_entries() then hands the entries to a
// functor 64 slots at a time, in list order (molecules: a slot per direction of a bond, 32 bonds to a step; the second slot
// of a self loop is idle).  Pass 2 runs it twice: degrees into LDS counters (4 bytes per node of max_num_nodes), then -
// row pointers scanned, the counters now row cursors - the scatter.  The scatter is STABLE: inside a step an entry's slot is
// its row's cursor plus the number of earlier lanes of the step with the same row (found with one ballot per bit of the row
// index), so a row lists its entries in list order (GraphBatch.from_coo).  Nothing is staged: the tokens are read again.
// Everything around the parse and the scatter - the slice a row claims, the row-pointer scan, `info` - is
// gtok_decode_csr.hpp's, shared with gtok_sent_decode.hip.
#include "gtok_common.hpp"
#include "gtok_decode_args.hpp"
#include "gtok_decode_csr.hpp"

namespace {
using namespace gtok;

enum { kZinc = GTOK_IBTT_GRAMMAR_ZINC, kSynth = GTOK_IBTT_GRAMMAR_SYNTH };

struct RowArgs {
  const void *ids; const int64_t *row_start; const int32_t *len; const int32_t *inv;
  int eb, ld, rows, inv_len, maxn;
};

// class (LUT slot) of the row's token i; -1 for an id outside the vocab, an id no slot owns, or a position outside [0, L)
__device__ __forceinline__ int cls_at(const RowArgs &a, int64_t base, int64_t i, int64_t L) {
  if (i < 0 || i >= L) return -1;
  const int id = load_id(a, base + i);
  return (unsigned)id < (unsigned)a.inv_len ? a.inv[id] : -1;
}
__device__ __forceinline__ int ucls_at(const RowArgs &a, int64_t base, int64_t i, int64_t L) { return uni(cls_at(a, base, i, L)); }

// lanes below the first set bit of `stop` (all of them when none is set)
__device__ __forceinline__ uint64_t below_first(uint64_t stop) { return stop ? (1ull << __builtin_ctzll(stop)) - 1ull : ~0ull; }

// What a row holds.  Everything is wave-uniform.  st 1: n = e = recs = 0.
struct Shape {
  int st, n, e;        // status (0, 1, 3), nodes, entries
  int recs;            // bond / edge records
  int64_t first;       // position of record 0
  int64_t L;           // tokens the records were judged inside (molecules: without a dropped <eos>)
  int nq; int64_t q;   // (graph-token rows, st 0) the ids after <q> and the position of <q>
};

template <int GR>
__device__ __forceinline__ Shape row_shape(const RowArgs &a, int64_t base, int L);

template <>
__device__ __forceinline__ Shape row_shape<kZinc>(const RowArgs &a, int64_t base, int L) {
  const int lane = lane_id();
  Shape s{1, 0, 0, 0, 0, 0, 0, 0};
  if (L < 1) return s;
  const bool dropped = ucls_at(a, base, L - 1, L) == GTOK_ZLUT_EOS;
  const int64_t Lp = L - (dropped ? 1 : 0);
  s.L = Lp;
  if (Lp == 0) { s.st = 3; return s; }
  if (ucls_at(a, base, 0, Lp) != GTOK_ZLUT_BOS) return s;
  int A = 0;
  for (int k0 = 0;; k0 += kWave) {                       // (ends: a record past Lp is not valid)
    const int64_t at = 1 + 2 * (int64_t)(k0 + lane);
    const int c0 = cls_at(a, base, at, Lp), c1 = cls_at(a, base, at + 1, Lp);
    const bool ok = c0 == GTOK_ZLUT_ATOM && c1 >= GTOK_ZLUT_ATOM0 && c1 <= GTOK_ZLUT_ATOM0 + 9;
    const uint64_t stop = __ballot(!ok);
    if (stop) { A = k0 + (int)__builtin_ctzll(stop); break; }
  }
  const int64_t p = 1 + 2 * (int64_t)A;
  int B = 0, loops = 0;
  for (int k0 = 0;; k0 += kWave) {
    const int64_t at = p + 4 * (int64_t)(k0 + lane);
    const int c0 = cls_at(a, base, at, Lp), c1 = cls_at(a, base, at + 1, Lp);
    const int u = cls_at(a, base, at + 2, Lp) - GTOK_ZLUT_NODE0, v = cls_at(a, base, at + 3, Lp) - GTOK_ZLUT_NODE0;
    const bool ok = c0 == GTOK_ZLUT_BOND && c1 >= GTOK_ZLUT_BOND0 && c1 <= GTOK_ZLUT_BOND0 + 4 && u >= 0 && u < A && v >= 0 && v < A;
    const uint64_t stop = __ballot(!ok);
    loops += (int)__popcll(__ballot(ok && u == v) & below_first(stop));
    if (stop) { B = k0 + (int)__builtin_ctzll(stop); break; }
  }
  const int64_t t = p + 4 * (int64_t)B, R = Lp - t;
  const int r0 = ucls_at(a, base, t, Lp), r1 = ucls_at(a, base, t + 1, Lp), r2 = ucls_at(a, base, t + 2, Lp);
  const bool bond_type = r1 >= GTOK_ZLUT_BOND0 && r1 <= GTOK_ZLUT_BOND0 + 4;
  const bool node = r2 >= GTOK_ZLUT_NODE0 && r2 - GTOK_ZLUT_NODE0 < A;
  int st = 1;
  if (R == 3 && r0 == GTOK_ZLUT_Q && r1 == GTOK_ZLUT_REGRESSION && r2 == GTOK_ZLUT_P) st = dropped ? 1 : 0;
  else if (R == 0 || (R == 1 && r0 == GTOK_ZLUT_Q) || (R == 2 && r0 == GTOK_ZLUT_Q && r1 == GTOK_ZLUT_REGRESSION)) st = 3;
  else if (R <= 3 && r0 == GTOK_ZLUT_BOND && (R < 2 || bond_type) && (R < 3 || node)) st = 3;
  else if (R == 1 && B == 0 && r0 == GTOK_ZLUT_ATOM) st = 3;
  if (A > a.maxn) st = 1;
  if (st == 1) return s;
  s.st = st; s.n = A; s.recs = B; s.e = 2 * B - loops; s.first = p;
  return s;
}

template <>
__device__ __forceinline__ Shape row_shape<kSynth>(const RowArgs &a, int64_t base, int L) {
  const int lane = lane_id();
  Shape s{1, 0, 0, 0, 1, L, 0, 0};
  if (L < 1) return s;
  if (ucls_at(a, base, 0, L) != GTOK_SLUT_BOS) return s;
  int M = 0, top = -1;                                   // records, their largest endpoint (per lane, then of the row)
  for (int k0 = 0;; k0 += kWave) {
    const int64_t at = 1 + 3 * (int64_t)(k0 + lane);
    const int u = cls_at(a, base, at, L) - GTOK_SLUT_NODE0, v = cls_at(a, base, at + 1, L) - GTOK_SLUT_NODE0;
    const bool ok = u >= 0 && v >= 0 && cls_at(a, base, at + 2, L) == GTOK_SLUT_E;
    const uint64_t stop = __ballot(!ok);
    if (ok && ((below_first(stop) >> lane) & 1ull)) top = max(top, max(u, v));
    if (stop) { M = k0 + (int)__builtin_ctzll(stop); break; }
  }
  top = wave_max(top);
  const int64_t p = 1 + 3 * (int64_t)M;
  int st = 1, S = 0, nq = 0;
  int64_t q = 0;
  bool q_seen = false;
  if (p == L) st = 3;
  else {
    const int cp = ucls_at(a, base, p, L);
    if (cp != GTOK_SLUT_N) {                             // one or two endpoints of a record that was cut
      const int64_t R = L - p;
      const bool n0 = cp >= GTOK_SLUT_NODE0, n1 = ucls_at(a, base, p + 1, L) >= GTOK_SLUT_NODE0;
      st = ((R == 1 && n0) || (R == 2 && n0 && n1)) ? 3 : 1;
    } else {
      for (int k0 = 0;; k0 += kWave) {
        const int k = k0 + lane;
        const bool ok = (int64_t)cls_at(a, base, p + 1 + k, L) == (int64_t)GTOK_SLUT_NODE0 + k;
        const uint64_t stop = __ballot(!ok);
        if (stop) { S = k0 + (int)__builtin_ctzll(stop); break; }
      }
      q = p + 1 + S;
      if (q == L) st = 3;
      else if (ucls_at(a, base, q, L) == GTOK_SLUT_Q) {
        q_seen = true;
        const int64_t rem = L - q - 1;                   // tokens after <q>
        if (rem >= 1 && rem <= 4 && ucls_at(a, base, L - 1, L) == GTOK_SLUT_P) { st = 0; nq = (int)rem - 1; }
        else if (rem <= 3) st = 3;
      }
    }
  }
  int n = S;
  if (q_seen) { if (top >= S) st = 1; }
  else n = max(S, top + 1);
  if (n > a.maxn) st = 1;
  if (st == 1) return s;
  s.st = st; s.n = n; s.recs = M; s.e = M; s.nq = nq; s.q = q;
  return s;
}

// The entries of a row whose shape is known (st != 1), a step of 64 slots at a time in list order: f(src, dst, type, active,
// inrow) - `inrow` lanes hold a slot of the list (an idle one included: the second direction of a self loop, src as its twin's).
template <int GR, class F>
__device__ __forceinline__ void for_entries(const RowArgs &a, int64_t base, const Shape &s, F &f) {
  const int lane = lane_id();
  const int per = GR == kZinc ? kWave / 2 : kWave;       // records per step
  for (int k0 = 0; k0 < s.recs; k0 += per) {
    const int k = k0 + (GR == kZinc ? lane >> 1 : lane);
    const bool inrow = k < s.recs;
    int src = 0, dst = 0, ty = 0;
    bool active = inrow;
    if (GR == kZinc) {
      const int64_t at = s.first + 4 * (int64_t)k;
      const int t = cls_at(a, base, at + 1, inrow ? s.L : 0) - GTOK_ZLUT_BOND0;
      const int u = cls_at(a, base, at + 2, inrow ? s.L : 0) - GTOK_ZLUT_NODE0, v = cls_at(a, base, at + 3, inrow ? s.L : 0) - GTOK_ZLUT_NODE0;
      const bool back = lane & 1;
      src = back ? v : u; dst = back ? u : v; ty = t;
      active = inrow && !(back && u == v);
    } else {
      const int64_t at = s.first + 3 * (int64_t)k;
      src = cls_at(a, base, at, inrow ? s.L : 0) - GTOK_SLUT_NODE0; dst = cls_at(a, base, at + 1, inrow ? s.L : 0) - GTOK_SLUT_NODE0;
    }
    f(src, dst, ty, active, inrow);
  }
}

// ---- pass 1: sizes ------------------------------------------------------------------------------------------------
struct SizesArgs {
  RowArgs r;
  int32_t *num_nodes, *num_entries, *status, *query;
  int units, upb;
};

template <int GR>
__global__ void __launch_bounds__(256) ibtt_decode_sizes_kernel(const SizesArgs a) {
  const int wave = wave_id(), wpb = (int)(blockDim.x >> 6), lane = lane_id();
  const int vb = virtual_block();
  const int u0 = vb * a.upb, u1 = min(a.units, u0 + a.upb);
  for (int unit = u0; unit < u1; ++unit) {
    const int r = unit * wpb + wave;
    if (r >= a.r.rows) break;
    int64_t base; int L;
    row_span(a.r, r, base, L);
    const Shape s = row_shape<GR>(a.r, base, L);
    if (lane == 0) {
      a.num_nodes[r] = s.n;
      a.num_entries[r] = s.e;
      a.status[r] = s.st;
    }
    if (GR == kSynth && a.query && lane < 4) {           // gtok_ibtt_synth's input, read back from a complete row
      int v = 0;
      if (s.st == 0) v = lane == 0 ? s.nq : (lane <= s.nq ? load_id(a.r, base + s.q + lane) : 0);
      a.query[4 * (int64_t)r + lane] = v;
    }
  }
}

// ---- pass 2: the CSR ----------------------------------------------------------------------------------------------
// degrees into the LDS counters; whether the list is row-sorted as it stands
struct DegreeStep {
  int *deg; int n;
  int last = 0, unsorted = 0;
  __device__ __forceinline__ void operator()(int src, int, int, bool active, bool inrow) {
    if (active && (unsigned)src < (unsigned)n) atomicAdd(&deg[src], 1);
    const int sx = inrow ? src : 0x7FFFFFFF;
    int prev = __shfl_up(sx, 1);
    if (lane_id() == 0) prev = last;
    if (__ballot(inrow && sx < prev)) unsorted = 1;
    last = __builtin_amdgcn_readlane(sx, kWave - 1);
  }
};

// the entries to their slots
template <int GR>
struct ScatterStep {
  int32_t *col, *eorder; uint8_t *eattr;    // the row's slices
  int *cursor; int n, e, bits;               // bits: of the largest row index
  int done = 0;
  __device__ __forceinline__ void operator()(int src, int dst, int ty, bool active, bool) {
    active = active && (unsigned)src < (unsigned)n;
    const uint64_t act = __ballot(active);
    const int cur = active ? cursor[src] : 0;
    uint64_t same = act;                     // the active lanes with this lane's row
    for (int b = 0; b < bits; ++b) {
      const bool bit = (src >> b) & 1;
      const uint64_t set = __ballot(active && bit);
      same &= bit ? set : ~set;
    }
    const int rank = (int)__popcll(same & lanemask_lt()), group = (int)__popcll(same);
    const int slot = cur + rank;
    if (active && (unsigned)slot < (unsigned)e) {
      col[slot] = dst;
      eorder[slot] = done + (int)__popcll(act & lanemask_lt());
      if (GR == kZinc) eattr[slot] = (uint8_t)ty;
    }
    if (active && rank == group - 1) cursor[src] = cur + group;     // the row's last lane moves its cursor on
    wave_sync();
    done += (int)__popcll(act);
  }
};

struct CsrArgs {
  RowArgs r;
  gtok_csr_built out;
  int stride;          // LDS bytes per wave: the counters
  int units, upb;
};

template <int GR>
__global__ void __launch_bounds__(256) ibtt_decode_csr_kernel(const CsrArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id();
  const int wave = wave_id(), wpb = (int)(blockDim.x >> 6);
  int *deg = reinterpret_cast<int *>(smem + (size_t)wave * a.stride);
  const DecodeTotals tot(a.out, a.r.rows);
  DecodeInfo acc;                                  // info[0..7]: gtok_decode_csr.hpp
  const int vb = virtual_block();
  const int u0 = vb * a.upb, u1 = min(a.units, u0 + a.upb);
  for (int unit = u0; unit < u1; ++unit) {
    const int r = unit * wpb + wave;
    if (r >= tot.rows) break;
    const DecodeSlice sl = claim_slice(a.out, tot, r, a.r.maxn, acc);
    const int nb = sl.nb;
    const int64_t e0 = sl.e0;
    int64_t base; int L;
    row_span(a.r, r, base, L);
    const Shape s = row_shape<GR>(a.r, base, L);
    const int n = s.n, e = s.e;
    if (s.st == 1) ++acc.malformed;
    if (!sl.ok || n != sl.ncl || e != sl.ecl) { ++acc.bad; continue; }
    acc.built(n, e);
    for (int u = lane; u < n; u += kWave) deg[u] = 0;            // (n <= maxn: inside this wave's counters)
    wave_sync();
    DegreeStep ds;
    ds.deg = deg; ds.n = n;
    for_entries<GR>(a.r, base, s, ds);
    wave_sync();
    acc.unsorted |= ds.unsorted;
    acc.max_deg = max(acc.max_deg, scan_rowptr(a.out.rowptr + nb + r, deg, n, e));   // the counters become the rows' cursors
    if (n == 0) continue;
    wave_sync();
    if (GR == kZinc)                                             // atom k's symbol is token 2 + 2 k
      for (int u = lane; u < n; u += kWave) {
        const int t = cls_at(a.r, base, 2 + 2 * (int64_t)u, s.L) - GTOK_ZLUT_ATOM0;
        a.out.nattr[nb + u] = (uint8_t)(t == 9 ? 255 : t);
      }
    ScatterStep<GR> ss;
    ss.col = a.out.col + e0; ss.eorder = a.out.eorder + e0; ss.eattr = GR == kZinc ? a.out.eattr + e0 : nullptr;
    ss.cursor = deg; ss.n = n; ss.e = e; ss.bits = n > 1 ? 32 - __builtin_clz(n - 1) : 0;
    for_entries<GR>(a.r, base, s, ss);
  }
  acc.report(a.out.info);
}

RowArgs row_args(const void *ids, int32_t elem_bytes, const int64_t *row_start, int32_t ld, const int32_t *len, int32_t num_rows,
                 const int32_t *inv, int32_t inv_len, int32_t max_num_nodes) {
  RowArgs r;
  r.ids = ids; r.row_start = row_start; r.len = len; r.inv = inv; r.eb = elem_bytes; r.ld = ld; r.rows = num_rows; r.inv_len = inv_len;
  r.maxn = max_num_nodes;
  return r;
}

}  // namespace

extern "C" int gtok_ibtt_decode_sizes(const void *ids, int32_t elem_bytes, const int64_t *row_start, int32_t ld, const int32_t *len,
                                      int32_t num_rows, int32_t grammar, const int32_t *inv, int32_t inv_len, int32_t max_num_nodes,
                                      int32_t *num_nodes, int32_t *num_entries, int32_t *status, int32_t *query, void *stream) {
  const int c = ibtt_decode_check_rows(ids, elem_bytes, ld, len, num_rows, grammar, inv, inv_len, max_num_nodes);
  return decode_launch(c, num_nodes && num_entries && status, nullptr, stream, [&](int dev, hipStream_t s) {
    SizesArgs a;
    a.r = row_args(ids, elem_bytes, row_start, ld, len, num_rows, inv, inv_len, max_num_nodes);
    a.num_nodes = num_nodes; a.num_entries = num_entries; a.status = status; a.query = query;
    return grammar == kZinc ? launch_wave_per_item(ibtt_decode_sizes_kernel<kZinc>, a, num_rows, 4, 0, dev, s)
                            : launch_wave_per_item(ibtt_decode_sizes_kernel<kSynth>, a, num_rows, 4, 0, dev, s);
  });
}

extern "C" int gtok_ibtt_decode_csr(const void *ids, int32_t elem_bytes, const int64_t *row_start, int32_t ld, const int32_t *len,
                                    int32_t num_rows, int32_t grammar, const int32_t *inv, int32_t inv_len, int32_t max_num_nodes,
                                    const gtok_csr_built *out, void *stream) {
  const int c = ibtt_decode_check_rows(ids, elem_bytes, ld, len, num_rows, grammar, inv, inv_len, max_num_nodes);
  return decode_launch(c, ibtt_decode_check_out(out, grammar) == GTOK_OK, out, stream, [&](int dev, hipStream_t s) {
    CsrArgs a;
    a.r = row_args(ids, elem_bytes, row_start, ld, len, num_rows, inv, inv_len, max_num_nodes);
    a.out = *out;
    a.stride = align_up((max_num_nodes > 0 ? max_num_nodes : 1) * 4, 16);
    return grammar == kZinc ? launch_wave_per_item(ibtt_decode_csr_kernel<kZinc>, a, num_rows, 4, a.stride, dev, s)
                            : launch_wave_per_item(ibtt_decode_csr_kernel<kSynth>, a, num_rows, 4, a.stride, dev, s);
  });
}
