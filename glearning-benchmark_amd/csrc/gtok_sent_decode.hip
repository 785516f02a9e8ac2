// gtok_sent_decode.hip — SENT rows back to a batched CSR (include/gtok.h: gtok_sent_decode_sizes / gtok_sent_decode_csr).
//
// One wave per row.  The grammar is sequential, so the parse runs on the SCALAR side: the wave loads 64 tokens per step
// (coalesced, widened from 1 / 2 / 4 bytes in registers, the next chunk in flight while this one is parsed) and a
// wave-uniform state machine takes them one at a time with v_readlane.  Its tests are those of sent_decode_kernel
// (gtok_sent.hip) in the same order, cut into one-token steps - status, node count and edge list are that decoder's.
// What the parse finds (an adjacency entry, a node type) is dropped into the next free lane of a register (a select on the
// lane id); the vector side takes the entries 64 at a time.
//
// Pass 2 parses a row to count the degrees (LDS, 4 bytes per node of max_num_nodes) and to check the recount against the
// row's node_ptr / edge_ptr slice, staging the entries in LDS while they fit (up to 2,048); then - row pointers scanned,
// the counters now row cursors - it scatters the entries, from the stage or, for a longer row, from a second parse.  The
// scatter is STABLE: inside a batch an entry's slot is its row's cursor plus the number of earlier lanes of the batch with
// the same row, so a row lists its entries in stream order (GraphBatch.from_coo).  Everything around the parse and the
// scatter - the slice a row claims, the row-pointer scan, `info` - is gtok_decode_csr.hpp's, shared with gtok_ibtt_decode.hip.
//
// ZINC-remapped rows (gtok_sent_decode_zinc_sizes / gtok_sent_decode_zinc_csr, gtok_unremap_zinc): instantiations of the same two
// kernels that UNFOLD every chunk on the vector side before the state machine reads it (ZincUnfold), and a kernel that writes
// the unfolded chunks out.
#include "gtok_common.hpp"
#include "gtok_decode_args.hpp"
#include "gtok_decode_csr.hpp"
#include "gtok_zinc_unremap.hpp"

namespace {
using namespace gtok;

struct RowArgs {
  const void *ids; const int64_t *row_start; const int32_t *len;
  int eb, ld, rows, idx_off, node_off, edge_off, maxn;
};

// v with the wave-uniform value s in lane `at` (v_writelane's effect)
__device__ __forceinline__ int put_lane(int s, int at, int v) { return lane_id() == at ? s : v; }

__device__ __forceinline__ int type_u8(int t) { return (unsigned)t < 255u ? t : 255; }   // csr.py: _to_u8

// ZINC-remapped rows (include/gtok.h: the rule): one 64-token chunk UNFOLDED in registers, on the vector side.  Every lane takes the
// preimage of its id; the folded id is told apart by the id behind it (the neighbouring lane's, or lane 0's of the next chunk,
// which is already in flight) and by the flag `open`.  The flag is a two-state automaton over the folded ids of a row - one with an
// edge type behind it toggles it, any other clears it - so the flag in front of a lane is the parity of the toggles below it since
// the last clear below it (or since the chunk's start, plus the carry): two ballots and a popcount, no token taken by itself.
struct ZincUnfold {
  int maxn, ntypes, edge_off;
  int open;                      // (wave-uniform) the flag in front of the next chunk
  __device__ __forceinline__ ZincUnfold(const RowArgs &a) : maxn(a.maxn), ntypes(a.edge_off - a.node_off), edge_off(a.edge_off), open(0) {}
  // the toggles of `tog` that count for a token with the folded ids `cb` of the clearing kind below it, and whether the carry does
  static __device__ __forceinline__ int flag(uint64_t tog, uint64_t cb, int carry) {
    const uint64_t since = cb ? (~0ull << (63 - __builtin_clzll(cb))) << 1 : ~0ull;     // the bits above the last clear
    return ((int)__popcll(tog & since) + (cb ? 0 : carry)) & 1;
  }
  // v: the chunk's ids (lane l: token l of the `left` >= 1 ids the row still has), vn: the next chunk's.  Returns the unfolded ids
  // (lanes at or beyond `left`: undefined) and moves `open` on.
  __device__ __forceinline__ int chunk(int v, int vn, int left) {
    const int lane = lane_id();
    const bool in = lane < left;
    const int p = zinc_pre(v, maxn, ntypes);
    const uint64_t xs = __ballot(in && v == kZincFolded);
    uint64_t es = __ballot(in && p >= edge_off) >> 1;                                   // bit l: an edge type stands behind token l
    if (left > kWave && zinc_pre(__builtin_amdgcn_readfirstlane(vn), maxn, ntypes) >= edge_off) es |= 1ull << 63;
    const uint64_t tog = xs & es, clr = xs & ~es, below = lanemask_lt();
    const int open_here = flag(tog & below, clr & below, open);
    open = flag(tog, clr, open);
    if ((xs >> lane) & 1ull) return open_here ? GTOK_SENT_RADJ : ((es >> lane) & 1ull) ? GTOK_SENT_LADJ : GTOK_SENT_RESET;
    return p != kZincNone ? p : GTOK_SENT_PAD;                                          // (PAD: no state of the parse accepts it)
  }
};

struct NoUnfold {                // un-remapped rows: the ids as they stand
  __device__ __forceinline__ NoUnfold(const RowArgs &) {}
  __device__ __forceinline__ int chunk(int v, int, int) const { return v; }
};

// The state machine.  sink.node(type) is called once per node in first-visit order (type -1: none / cut), sink.edge(a, b,
// type) once per decoded edge in stream order; everything here is wave-uniform.  Returns the status (0, 1 or 3).  ZINC: the rows are
// ZINC-remapped - every chunk is unfolded before the state machine reads it, whose tests stay as they are.
enum { kMain = 0, kBracket = 1, kBracketPos = 2, kNodeType = 3 };
template <bool LAB, bool ZINC, class Sink>
__device__ __forceinline__ int parse_row(const RowArgs &a, int64_t base, int L, Sink &sink, int &num_nodes) {
  const int lane = lane_id();
  num_nodes = 0;
  if (L < 1) return 1;
  int st = 3, state = kMain, prev = -1, nseen = 0, pending = -1, k = 0, btype = -1;
  int v = lane < L ? load_id(a, base + lane) : 0;
  std::conditional_t<ZINC, ZincUnfold, NoUnfold> zu(a);
  for (int c0 = 0; c0 < L && st == 3; c0 += kWave) {
    const int nx = c0 + kWave + lane;
    const int vn = nx < L ? load_id(a, base + nx) : 0;
    const int cn = min(kWave, L - c0);
    const int cur = zu.chunk(v, vn, L - c0);
    int j = 0;
    if (c0 == 0) {
      if (__builtin_amdgcn_readlane(cur, 0) != GTOK_SENT_SOS) st = 1;
      j = 1;
    }
    for (; j < cn && st == 3; ++j) {
      const int tk = __builtin_amdgcn_readlane(cur, j);
      bool new_node = false, new_edge = false;
      int ntype = -1, ea = 0, eb = 0, et = -1;
      if (state == kMain) {
        if (tk == GTOK_SENT_EOS) st = 0;
        else if (tk == GTOK_SENT_RESET) { prev = -1; pending = -1; }
        else if (tk == GTOK_SENT_LADJ) { if (prev < 0) st = 1; else state = kBracket; }
        else if (!(tk >= a.idx_off && tk < a.node_off)) {
          if (LAB && tk >= a.edge_off) pending = tk - a.edge_off;       // edge type ahead of a trail step
          else st = 1;
        } else {
          k = tk - a.idx_off;
          if (k > nseen) st = 1;
          else if (LAB && k == nseen) state = kNodeType;                // first visit: its type token follows
          else {
            new_node = k == nseen;
            new_edge = prev >= 0; ea = prev; eb = k; et = pending;
            pending = -1; prev = k;
          }
        }
      } else if (state == kNodeType) {
        ntype = tk - a.node_off;
        if (ntype < 0) st = 1;
        else {
          new_node = true;
          new_edge = prev >= 0; ea = prev; eb = k; et = pending;
          pending = -1; prev = k; state = kMain;
        }
      } else if (state == kBracket && tk == GTOK_SENT_RADJ) {
        state = kMain;
      } else if (LAB && state == kBracket) {
        btype = tk - a.edge_off;
        if (btype < 0) st = 1; else state = kBracketPos;
      } else {                                                           // a bracket member's position
        const int b = tk - a.idx_off;
        if (b < 0 || b >= nseen) st = 1;
        else { new_edge = true; ea = prev; eb = b; et = LAB ? btype : -1; state = kBracket; }
      }
      if (new_node) { sink.node(ntype); ++nseen; }
      if (new_edge) sink.edge(ea, eb, et);
    }
    v = vn;
  }
  if (st == 3 && state == kNodeType) { sink.node(-1); ++nseen; }         // cut between a position and its type
  num_nodes = nseen;
  return st;
}

// ---- pass 1: sizes ------------------------------------------------------------------------------------------------
struct CountSink {
  int entries = 0;
  __device__ __forceinline__ void node(int) {}
  __device__ __forceinline__ void edge(int a, int b, int) { entries += a == b ? 1 : 2; }
};

struct SizesArgs {
  RowArgs r;
  int32_t *num_nodes, *num_entries, *status;
  int units, upb;
};

template <bool LAB, bool ZINC = false>
__global__ void __launch_bounds__(256) sent_decode_sizes_kernel(const SizesArgs a) {
  const int wave = wave_id(), wpb = (int)(blockDim.x >> 6);
  const int vb = virtual_block();
  const int u0 = vb * a.upb, u1 = min(a.units, u0 + a.upb);
  for (int unit = u0; unit < u1; ++unit) {
    const int r = unit * wpb + wave;
    if (r >= a.r.rows) break;
    int64_t base; int L, n;
    row_span(a.r, r, base, L);
    CountSink sink;
    const int st = parse_row<LAB, ZINC>(a.r, base, L, sink, n);
    if (lane_id() == 0) {
      a.num_nodes[r] = st == 1 ? 0 : n;
      a.num_entries[r] = st == 1 ? 0 : sink.entries;
      a.status[r] = st;
    }
  }
}

// ---- pass 2: the CSR ----------------------------------------------------------------------------------------------
// first parse: degrees into LDS, the recount, whether the interleaved list is row-sorted as it stands.  While they fit, the
// entries (row | column << 16, type) and the node types are also STAGED in LDS in stream order: the scatter then reads them
// back instead of parsing the row a second time.
template <bool LAB>
struct DegreeSink {
  int *deg; int ncl;             // LDS counters of the row's claimed nodes
  int *stage_pk; uint8_t *stage_t, *stage_nt; int cap, ncap;   // LDS stage: `cap` entries, `ncap` node types (0: none)
  int entries = 0, last = 0, unsorted = 0, cnt = 0, ncnt = 0, ndone = 0;
  int vpk = 0, vt = 0, vnt = 0;  // (vector) the batch's entries, its node types
  __device__ __forceinline__ void flush_nodes() {
    const int u = ndone + lane_id();
    if (lane_id() < ncnt && u < ncap) stage_nt[u] = (uint8_t)vnt;
    ndone += ncnt; ncnt = 0;
  }
  __device__ __forceinline__ void node(int type) {
    if (!LAB) return;
    vnt = put_lane(type_u8(type), ncnt, vnt);
    if (++ncnt == kWave) flush_nodes();
  }
  __device__ __forceinline__ void flush() {
    const int lane = lane_id(), src = vpk & 0xFFFF, p = entries - cnt + lane;
    if (lane < cnt) {
      if ((unsigned)src < (unsigned)ncl) atomicAdd(&deg[src], 1);
      if (p < cap) { stage_pk[p] = vpk; if (LAB) stage_t[p] = (uint8_t)vt; }
    }
    cnt = 0;
  }
  __device__ __forceinline__ void put(int s, int d, int t) {
    if (s < last) unsorted = 1;
    last = s; ++entries;
    vpk = put_lane(s | (d << 16), cnt, vpk);
    if (LAB) vt = put_lane(t, cnt, vt);
    if (++cnt == kWave) flush();
  }
  __device__ __forceinline__ void edge(int a, int b, int t) {
    const int t8 = type_u8(t);
    put(a, b, t8);
    if (a != b) put(b, a, t8);
  }
};

// the entries to their slots, the node types: fed by a second parse, or batch by batch from the stage
template <bool LAB>
struct ScatterSink {
  int32_t *col, *eorder; uint8_t *eattr, *nattr;   // the row's slices
  int *cursor; int n, e;
  int cnt = 0, done = 0, ncnt = 0, ndone = 0;
  int vpk = 0, vt = 0, vnt = 0;                    // (vector) row | column << 16, edge type, node type of the batch
  __device__ __forceinline__ void flush_nodes() {
    const int u = ndone + lane_id();
    if (lane_id() < ncnt && u < n) nattr[u] = (uint8_t)vnt;
    ndone += ncnt; ncnt = 0;
  }
  __device__ __forceinline__ void node(int type) {
    if (!LAB) return;
    vnt = put_lane(type_u8(type), ncnt, vnt);
    if (++ncnt == kWave) flush_nodes();
  }
  __device__ __forceinline__ void flush() {
    const int lane = lane_id();
    const int src = vpk & 0xFFFF, dst = (int)((unsigned)vpk >> 16);
    const bool active = lane < cnt && src < n;
    const int cur = active ? cursor[src] : 0;
    int rank = 0, group = 0;
    uint64_t todo = __ballot(active);
    while (todo) {                                  // once per distinct row of the batch
      const int leader = (int)__builtin_ctzll(todo);
      const int row = __builtin_amdgcn_readlane(src, leader);
      const uint64_t same = __ballot(active && src == row);
      if (src == row) { rank = (int)__popcll(same & lanemask_lt()); group = (int)__popcll(same); }
      todo &= ~same;
    }
    const int slot = cur + rank;
    if (active && (unsigned)slot < (unsigned)e) {
      col[slot] = dst;
      eorder[slot] = done + lane;
      if (LAB) eattr[slot] = (uint8_t)vt;
    }
    if (active && rank == group - 1) cursor[src] = cur + group;     // the row's last lane moves its cursor on
    wave_sync();
    done += cnt; cnt = 0;
  }
  __device__ __forceinline__ void put(int s, int d, int t) {
    vpk = put_lane(s | (d << 16), cnt, vpk);
    if (LAB) vt = put_lane(t, cnt, vt);
    if (++cnt == kWave) flush();
  }
  __device__ __forceinline__ void edge(int a, int b, int t) {
    const int t8 = type_u8(t);
    put(a, b, t8);
    if (a != b) put(b, a, t8);
  }
};

struct CsrArgs {
  RowArgs r;
  gtok_csr_built out;
  int stride;          // LDS bytes per wave: the counters, then the stage (entries, their types, the node types)
  int deg_bytes, cap;  // bytes of the counters; entries the stage holds (a multiple of 64; 0: no stage, always two parses)
  int units, upb;
};

template <bool LAB, bool ZINC = false>
__global__ void __launch_bounds__(256) sent_decode_csr_kernel(const CsrArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id();
  const int wave = wave_id(), wpb = (int)(blockDim.x >> 6);
  unsigned char *mine = smem + (size_t)wave * a.stride;
  int *deg = reinterpret_cast<int *>(mine);
  int *stage_pk = reinterpret_cast<int *>(mine + a.deg_bytes);
  uint8_t *stage_t = reinterpret_cast<uint8_t *>(stage_pk + a.cap), *stage_nt = stage_t + a.cap;
  const int ncap = LAB && a.cap ? a.r.maxn : 0;
  const DecodeTotals tot(a.out, a.r.rows);
  DecodeInfo acc;                                  // info[0..7]: gtok_decode_csr.hpp
  const int vb = virtual_block();
  const int u0 = vb * a.upb, u1 = min(a.units, u0 + a.upb);
  for (int unit = u0; unit < u1; ++unit) {
    const int r = unit * wpb + wave;
    if (r >= tot.rows) break;
    const DecodeSlice sl = claim_slice(a.out, tot, r, a.r.maxn, acc);
    const int nb = sl.nb, ncl = sl.ncl;
    const int64_t e0 = sl.e0;
    for (int u = lane; u < ncl; u += kWave) deg[u] = 0;
    wave_sync();
    int64_t base; int L, n;
    row_span(a.r, r, base, L);
    DegreeSink<LAB> ds;
    ds.deg = deg; ds.ncl = ncl;
    ds.stage_pk = stage_pk; ds.stage_t = stage_t; ds.stage_nt = stage_nt; ds.cap = a.cap; ds.ncap = ncap;
    const int st = parse_row<LAB, ZINC>(a.r, base, L, ds, n);
    ds.flush();
    if (LAB) ds.flush_nodes();
    wave_sync();
    int e = ds.entries;
    if (st == 1) { n = 0; e = 0; ++acc.malformed; }
    if (!sl.ok || n != ncl || e != sl.ecl) { ++acc.bad; continue; }
    acc.unsorted |= st == 1 ? 0 : ds.unsorted;
    acc.built(n, e);
    acc.max_deg = max(acc.max_deg, scan_rowptr(a.out.rowptr + nb + r, deg, n, e));   // the counters become the rows' cursors
    if (st == 1 || n == 0) continue;
    wave_sync();
    ScatterSink<LAB> ss;
    ss.col = a.out.col + e0; ss.eorder = a.out.eorder + e0;
    ss.eattr = LAB ? a.out.eattr + e0 : nullptr; ss.nattr = LAB ? a.out.nattr + nb : nullptr;
    ss.cursor = deg; ss.n = n; ss.e = e;
    if (a.cap && e <= a.cap) {                     // there is a stage and it holds everything: no second parse
      for (int p0 = 0; p0 < e; p0 += kWave) {
        ss.cnt = min(kWave, e - p0);
        if (lane < ss.cnt) { ss.vpk = stage_pk[p0 + lane]; if (LAB) ss.vt = stage_t[p0 + lane]; }
        ss.flush();
      }
      if (LAB)
        for (int u = lane; u < n; u += kWave) ss.nattr[u] = stage_nt[u];
    } else {
      int n2;
      (void)parse_row<LAB, ZINC>(a.r, base, L, ss, n2);
      ss.flush();
      if (LAB) ss.flush_nodes();
    }
  }
  acc.report(a.out.info);
}

// ---- gtok_unremap_zinc: the unfolded ids of every row as an int32 slab, `pad` behind them --------------------------------------
struct UnremapArgs {
  RowArgs r;
  int32_t *out;
  int pad;
  int units, upb;
};

__global__ void __launch_bounds__(256) unremap_zinc_kernel(const UnremapArgs a) {
  const int lane = lane_id();
  const int wave = wave_id(), wpb = (int)(blockDim.x >> 6);
  const int vb = virtual_block();
  const int u0 = vb * a.upb, u1 = min(a.units, u0 + a.upb);
  for (int unit = u0; unit < u1; ++unit) {
    const int r = unit * wpb + wave;
    if (r >= a.r.rows) break;
    int64_t base; int L;
    row_span(a.r, r, base, L);
    int32_t *row = a.out + (int64_t)r * a.r.ld;
    ZincUnfold zu(a.r);
    int v = lane < L ? load_id(a.r, base + lane) : 0;
    for (int64_t c0 = 0; c0 < a.r.ld; c0 += kWave) {          // (64-bit: c0 + 64 may pass 2^31 where ld is close to it)
      const int64_t i = c0 + lane;
      int vn = 0, u = a.pad;
      if (c0 < L) {
        vn = i + kWave < L ? load_id(a.r, base + i + kWave) : 0;
        u = zu.chunk(v, vn, L - (int)c0);
        if (i >= L) u = a.pad;
      }
      if (i < a.r.ld) row[i] = u;
      v = vn;
    }
  }
}

RowArgs row_args(const void *ids, int32_t elem_bytes, const int64_t *row_start, int32_t ld, const int32_t *len, int32_t num_rows,
                 int32_t max_num_nodes, int32_t num_node_types) {
  RowArgs r;
  r.ids = ids; r.row_start = row_start; r.len = len; r.eb = elem_bytes; r.ld = ld; r.rows = num_rows; r.maxn = max_num_nodes;
  r.idx_off = GTOK_SENT_IDX_OFFSET; r.node_off = r.idx_off + max_num_nodes; r.edge_off = r.node_off + num_node_types;
  return r;
}

// the kernel of a row kind: ZINC-remapped rows (always labelled), labelled, unlabelled
template <class K> K pick(bool zinc, bool labeled, K z, K l, K u) { return zinc ? z : labeled ? l : u; }

int decode_sizes(const void *ids, int32_t elem_bytes, const int64_t *row_start, int32_t ld, const int32_t *len, int32_t num_rows,
                 int32_t max_num_nodes, bool labeled, bool zinc, int32_t num_node_types, int32_t *num_nodes, int32_t *num_entries,
                 int32_t *status, void *stream) {
  const int c = sent_decode_check_rows(ids, elem_bytes, ld, len, num_rows, max_num_nodes, num_node_types);
  return decode_launch(c, num_nodes && num_entries && status, nullptr, stream, [&](int dev, hipStream_t s) {
    SizesArgs a;
    a.r = row_args(ids, elem_bytes, row_start, ld, len, num_rows, max_num_nodes, num_node_types);
    a.num_nodes = num_nodes; a.num_entries = num_entries; a.status = status;
    const auto kern = pick(zinc, labeled, sent_decode_sizes_kernel<true, true>, sent_decode_sizes_kernel<true>, sent_decode_sizes_kernel<false>);
    return launch_wave_per_item(kern, a, num_rows, 4, 0, dev, s);
  });
}

int decode_csr(const void *ids, int32_t elem_bytes, const int64_t *row_start, int32_t ld, const int32_t *len, int32_t num_rows,
               int32_t max_num_nodes, bool labeled, bool zinc, int32_t num_node_types, const gtok_csr_built *out, void *stream) {
  const int c = sent_decode_check_rows(ids, elem_bytes, ld, len, num_rows, max_num_nodes, num_node_types);
  return decode_launch(c, (zinc ? sent_decode_zinc_check_out(out) : sent_decode_check_out(out, labeled)) == GTOK_OK, out, stream, [&](int dev, hipStream_t s) {
    CsrArgs a;
    a.r = row_args(ids, elem_bytes, row_start, ld, len, num_rows, max_num_nodes, num_node_types);
    a.out = *out;
    a.deg_bytes = align_up((max_num_nodes > 0 ? max_num_nodes : 1) * 4, 16);
    // the stage: a row of L tokens decodes to fewer than 2 L entries; 2,048 of them at the most (10 KB), and none where counters
    // and stage together would pass what a workgroup has without the opt-in - every row is then parsed a second time, as rows of
    // more entries than the stage holds always are
    a.cap = align_up(ld < 1024 ? 2 * ld : 2048, 64);
    int stage_bytes = a.cap * 4 + (labeled ? a.cap + align_up(max_num_nodes, 16) : 0);
    if (a.deg_bytes + stage_bytes > kLdsWithoutOptIn) { a.cap = 0; stage_bytes = 0; }
    a.stride = a.deg_bytes + stage_bytes;
    const auto kern = pick(zinc, labeled, sent_decode_csr_kernel<true, true>, sent_decode_csr_kernel<true>, sent_decode_csr_kernel<false>);
    return launch_wave_per_item(kern, a, num_rows, 4, a.stride, dev, s);
  });
}

}  // namespace

extern "C" int gtok_sent_decode_sizes(const void *ids, int32_t elem_bytes, const int64_t *row_start, int32_t ld, const int32_t *len,
                                      int32_t num_rows, int32_t max_num_nodes, int32_t labeled, int32_t num_node_types,
                                      int32_t *num_nodes, int32_t *num_entries, int32_t *status, void *stream) {
  return decode_sizes(ids, elem_bytes, row_start, ld, len, num_rows, max_num_nodes, labeled != 0, false, num_node_types, num_nodes, num_entries,
                      status, stream);
}

extern "C" int gtok_sent_decode_csr(const void *ids, int32_t elem_bytes, const int64_t *row_start, int32_t ld, const int32_t *len,
                                    int32_t num_rows, int32_t max_num_nodes, int32_t labeled, int32_t num_node_types,
                                    const gtok_csr_built *out, void *stream) {
  return decode_csr(ids, elem_bytes, row_start, ld, len, num_rows, max_num_nodes, labeled != 0, false, num_node_types, out, stream);
}

// ---- ZINC-remapped rows (include/gtok.h)
extern "C" int gtok_sent_decode_zinc_sizes(const void *ids, int32_t elem_bytes, const int64_t *row_start, int32_t ld, const int32_t *len,
                                           int32_t num_rows, int32_t max_num_nodes, int32_t num_node_types, int32_t *num_nodes,
                                           int32_t *num_entries, int32_t *status, void *stream) {
  return decode_sizes(ids, elem_bytes, row_start, ld, len, num_rows, max_num_nodes, true, true, num_node_types, num_nodes, num_entries, status,
                      stream);
}

extern "C" int gtok_sent_decode_zinc_csr(const void *ids, int32_t elem_bytes, const int64_t *row_start, int32_t ld, const int32_t *len,
                                         int32_t num_rows, int32_t max_num_nodes, int32_t num_node_types, const gtok_csr_built *out,
                                         void *stream) {
  return decode_csr(ids, elem_bytes, row_start, ld, len, num_rows, max_num_nodes, true, true, num_node_types, out, stream);
}

extern "C" int gtok_unremap_zinc(const void *ids, int32_t elem_bytes, const int64_t *row_start, int32_t ld, const int32_t *len,
                                 int32_t num_rows, int32_t max_num_nodes, int32_t num_node_types, int32_t pad_id, int32_t *out_ids,
                                 void *stream) {
  const int c = unremap_zinc_check(ids, elem_bytes, ld, len, num_rows, max_num_nodes, num_node_types, out_ids);
  return decode_launch(c, true, nullptr, stream, [&](int dev, hipStream_t s) {
    UnremapArgs a;
    a.r = row_args(ids, elem_bytes, row_start, ld, len, num_rows, max_num_nodes, num_node_types);
    a.out = out_ids; a.pad = pad_id;
    return launch_wave_per_item(unremap_zinc_kernel, a, num_rows, 4, 0, dev, s);
  });
}
