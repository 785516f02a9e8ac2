// gtok_graph_keys.hip — a 128-bit key per graph of a batched CSR (include/gtok.h: gtok_graph_keys; the arithmetic:
// gtok_graph_keys_hash.hpp), gfx950.
//
// One wave per graph, the waves of a workgroup independent, each with its own slice of the dynamic LDS (gtok_common.hpp) - the
// conventions of gtok_graph_tasks.hip.  A key is a sum of mixed words over the graph's terms: every lane adds the terms it meets into
// two 64-bit sums, wave_sum64 folds them, lane 0 finishes and writes keys[2 g], keys[2 g + 1] with vector stores.
//   keys_stream_kernel<Attrs, Upper>   LISTED keys of any batch (and CLOSURE keys beyond 512 nodes: Upper keeps the entries with
//                         u < v of a GTOK_CSR_SIMPLE_SYMMETRIC batch).  64 rows per step: lane l reads row v0 + l's bounds from
//                         rowptr (coalesced); the entries of those rows are one run of col, which the wave reads 64 consecutive
//                         entries at a time (coalesced; eattr likewise), each lane finding the row of its entry by a six-step search
//                         over the 64 row starts (__shfl).  A row of more than 64 entries is thereby read by the whole wave (the
//                         centre of a 16,383-leaf star is 256 coalesced steps, not one lane's loop).  No LDS.
//   keys_reg_kernel       CLOSURE, <= 64 nodes: lane v holds closure row v as one 64-bit register, OR-ed together in 512 bytes of LDS
//                         from the listed entries, both directions, the diagonal kept apart; lane v's terms are the set bits b > v.
//   keys_lds_kernel<W>    CLOSURE, <= 512 nodes: the same over the bit matrix in LDS, word-major (word w of node v at w * max_nodes
//                         + v), lane l owning nodes l + 64 j and enumerating the set bits b > v of words j .. W - 1 of each.
// The two closure-row builders restate those of tasks_reg_kernel / tasks_lds_kernel (gtok_graph_tasks.hip) instead of sharing a
// header with them: profiles/graph_keys/kernel_resources.md says why.
// Everything read through is range-checked first (graph_slice, row_range, the columns).
#include "gtok_common.hpp"
#include "gtok_graph_keys_args.hpp"
#include "gtok_graph_keys_hash.hpp"

namespace {
using namespace gtok;

struct KeyArgs {
  gtok_csr g;
  const int32_t *labels;      // [G] or nullptr
  uint64_t *keys;             // [G, 2]
  int32_t *info;
  int stride;                 // LDS bytes per wave
  int units, upb;
};

constexpr int kDamaged = 2;   // info[0]

struct Acc {                  // what a wave adds to info[] when it retires
  int status = 0, damaged = 0;
};

struct Slice {
  int n, e;                   // 0 / 0 for a damaged slice
  bool ok;
  const int32_t *rp, *col;
  const uint8_t *na, *ea;     // the slice's attribute bytes (read with GTOK_KEYS_ATTRS only)
};

// graph r's slices, checked against the totals of the pointer arrays and the host-known bounds the LDS tables are sized by
__device__ __forceinline__ Slice graph_slice(const KeyArgs &a, int r, int ntot, int64_t etot) {
  const int nb = sload(a.g.node_ptr, r), ne = sload(a.g.node_ptr, r + 1);
  const int64_t e0 = sload(a.g.edge_ptr, r), e1 = sload(a.g.edge_ptr, r + 1);
  const bool ok = nb >= 0 && ne >= nb && ne <= ntot && ne - nb <= a.g.max_nodes && e0 >= 0 && e1 >= e0 && e1 <= etot &&
                  e1 - e0 <= (int64_t)a.g.max_edges;
  Slice s;
  s.ok = ok;
  s.n = ok ? ne - nb : 0;
  s.e = ok ? (int)(e1 - e0) : 0;
  s.rp = a.g.rowptr + (ok ? (int64_t)nb + r : 0);
  s.col = a.g.col + (ok ? e0 : 0);
  s.na = a.g.nattr ? a.g.nattr + (ok ? nb : 0) : nullptr;
  s.ea = a.g.eattr ? a.g.eattr + (ok ? e0 : 0) : nullptr;
  return s;
}

// row v of the slice (v < n): [x, y) inside [0, e], or empty and `bad` raised
__device__ __forceinline__ void row_range(const Slice &s, int v, int &x, int &y, int &bad) {
  x = s.rp[v]; y = s.rp[v + 1];
  if (x < 0 || y < x || y > s.e) { bad = 1; x = y = 0; }
}

// the wave's sums -> the graph's key, written by lane 0; the damage of this graph -> acc
__device__ __forceinline__ void write_key(const KeyArgs &a, int r, const Slice &s, const KeySums &mine, int terms, int bad, Acc &acc, int lane) {
  KeySums all;
  all.s0 = (uint64_t)wave_sum64((int64_t)mine.s0);
  all.s1 = (uint64_t)wave_sum64((int64_t)mine.s1);
  const int total = wave_sum(terms);
  if (!s.ok || __ballot(bad != 0)) { acc.status |= kDamaged; ++acc.damaged; }
  const int label = a.labels ? sload(a.labels, r) : 0;
  uint64_t k[2];
  keys_finish(all, (uint32_t)s.n, (uint32_t)total, label, k);
  if (lane == 0) {
    a.keys[2 * (int64_t)r] = k[0];
    a.keys[2 * (int64_t)r + 1] = k[1];
  }
}

__device__ __forceinline__ void retire(const KeyArgs &a, const Acc &acc, int lane) {
  if (lane != 0 || !acc.status) return;
  atomicOr(a.info + 0, acc.status);
  atomicAdd(a.info + 1, acc.damaged);
}

// ---- the stream over rowptr / col: LISTED keys, and CLOSURE keys of simple symmetric batches (Upper) --------------------------------
template <bool Attrs, bool Upper>
__device__ __forceinline__ void take_entry(const Slice &s, int u, int k, KeySums &sum, int &terms, int &bad) {
  const int c = s.col[k];                                            // (k inside [0, e): the row bounds were checked)
  if ((unsigned)c >= (unsigned)s.n) { bad = 1; return; }
  if (Upper && c <= u) return;
  sum.add(keys_entry_word((uint32_t)u, (uint32_t)c, Attrs ? (uint32_t)s.ea[k] : 0u));
  ++terms;
}

template <bool Attrs, bool Upper>
__global__ void __launch_bounds__(256) keys_stream_kernel(const KeyArgs a) {
  const int lane = lane_id(), wave = wave_id(), wpb = (int)(blockDim.x >> 6);
  const int G = a.g.num_graphs;
  const int ntot = sload(a.g.node_ptr, G);
  const int64_t etot = sload(a.g.edge_ptr, G);
  Acc acc;
  const int vb = virtual_block();
  const int u0 = vb * a.upb, u1 = min(a.units, u0 + a.upb);
  for (int unit = u0; unit < u1; ++unit) {
    const int r = unit * wpb + wave;
    if (r >= G) break;
    const Slice s = graph_slice(a, r, ntot, etot);
    KeySums sum;
    int terms = 0, bad = 0;
    for (int v0 = 0; v0 < s.n; v0 += kWave) {
      const int v = v0 + lane;
      int x = 0x7FFFFFFF, y = 0x7FFFFFFF, rowbad = 0;                   // (a lane beyond the graph never wins the search below)
      if (v < s.n) {
        x = s.rp[v]; y = s.rp[v + 1];
        rowbad = (x < 0 || y < x || y > s.e) ? 1 : 0;
        if (Attrs) { sum.add(keys_node_word((uint32_t)v, (uint32_t)s.na[v])); ++terms; }
      }
      if (!__ballot(rowbad != 0)) {
        // sound row pointers (0 <= x <= y <= e in every lane, and y of a row is x of the next: the same array): the entries of these
        // rows are ONE run [X0, X1) of col, read 64 consecutive entries per step; entry k belongs to the last row that starts at or
        // before k - six steps of a search over the row starts, one per lane.  A long row is thereby read by the whole wave.
        const int cnt = min(kWave, s.n - v0);
        const int X0 = __builtin_amdgcn_readlane(x, 0), X1 = __builtin_amdgcn_readlane(y, cnt - 1);
        for (int k0 = X0; k0 < X1; k0 += kWave) {
          const int k = k0 + lane;
          int l = 0;
#pragma unroll
          for (int step = 32; step; step >>= 1) {
            const int xc = __shfl(x, l + step);                          // (l + step <= 63)
            if (xc <= k) l += step;
          }
          if (k < X1) take_entry<Attrs, Upper>(s, v0 + l, k, sum, terms, bad);
        }
      } else {
        // damaged row pointers: the sound rows one by one, a lane each; the others are skipped
        bad = 1;
        if (v < s.n && !rowbad)
          for (int k = x; k < y; ++k) take_entry<Attrs, Upper>(s, v, k, sum, terms, bad);
      }
    }
    write_key(a, r, s, sum, terms, bad, acc, lane);
  }
  retire(a, acc, lane);
}

// the terms of closure row v held as words: the set bits b > v of word `w` (bits 64 w .. 64 w + 63)
__device__ __forceinline__ void take_row_word(int v, int w, uint64_t word, KeySums &sum, int &terms) {
  if (w == (v >> 6)) word &= ~((2ull << (v & 63)) - 1ull);            // (bit 63: 2 << 63 wraps to 0, the mask to nothing)
  while (word) {
    const int b = 64 * w + (int)__builtin_ctzll(word);
    word &= word - 1;
    sum.add(keys_entry_word((uint32_t)v, (uint32_t)b, 0u));
    ++terms;
  }
}

// ---- CLOSURE, <= 64 nodes: closure rows in registers ------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) keys_reg_kernel(const KeyArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id(), wave = wave_id(), wpb = (int)(blockDim.x >> 6);
  unsigned long long *rows = reinterpret_cast<unsigned long long *>(smem + (size_t)wave * a.stride);
  const int G = a.g.num_graphs;
  const int ntot = sload(a.g.node_ptr, G);
  const int64_t etot = sload(a.g.edge_ptr, G);
  Acc acc;
  const int vb = virtual_block();
  const int u0 = vb * a.upb, u1 = min(a.units, u0 + a.upb);
  for (int unit = u0; unit < u1; ++unit) {
    const int r = unit * wpb + wave;
    if (r >= G) break;
    const Slice s = graph_slice(a, r, ntot, etot);                      // (s.n <= max_nodes <= 64)
    wave_sync();
    rows[lane] = 0;
    wave_sync();
    uint64_t mine = 0;
    int diag = 0, bad = 0;
    if (lane < s.n) {
      int x, y;
      row_range(s, lane, x, y, bad);
      for (int k = x; k < y; ++k) {
        const int c = s.col[k];
        if ((unsigned)c >= (unsigned)s.n) { bad = 1; continue; }
        if (c == lane) { diag = 1; continue; }
        mine |= 1ull << c;
        atomicOr(rows + c, 1ull << lane);
      }
    }
    wave_sync();
    KeySums sum;
    int terms = 0;
    take_row_word(lane, 0, mine | rows[lane], sum, terms);
    if (diag) { sum.add(keys_entry_word((uint32_t)lane, (uint32_t)lane, 0u)); ++terms; }
    write_key(a, r, s, sum, terms, bad, acc, lane);
  }
  retire(a, acc, lane);
}

// ---- CLOSURE, <= 512 nodes: the bit matrix in LDS ---------------------------------------------------------------------------------
template <int W>
__global__ void __launch_bounds__(256) keys_lds_kernel(const KeyArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id(), wave = wave_id(), wpb = (int)(blockDim.x >> 6);
  unsigned long long *mat = reinterpret_cast<unsigned long long *>(smem + (size_t)wave * a.stride);
  const int G = a.g.num_graphs, np = max(a.g.max_nodes, 1);
  const int ntot = sload(a.g.node_ptr, G);
  const int64_t etot = sload(a.g.edge_ptr, G);
  Acc acc;
  const int vb = virtual_block();
  const int u0 = vb * a.upb, u1 = min(a.units, u0 + a.upb);
  for (int unit = u0; unit < u1; ++unit) {
    const int r = unit * wpb + wave;
    if (r >= G) break;
    const Slice s = graph_slice(a, r, ntot, etot);                      // (s.n <= max_nodes <= 64 W: every word index below is < W)
    wave_sync();
#pragma unroll
    for (int w = 0; w < W; ++w)
      for (int v = lane; v < s.n; v += kWave) mat[w * np + v] = 0;
    wave_sync();
    unsigned diag = 0;                                                  // bit j: node lane + 64 j has a loop
    int bad = 0;
    for (int v = lane; v < s.n; v += kWave) {
      int x, y;
      row_range(s, v, x, y, bad);
      for (int k = x; k < y; ++k) {
        const int c = s.col[k];
        if ((unsigned)c >= (unsigned)s.n) { bad = 1; continue; }
        if (c == v) { diag |= 1u << (v >> 6); continue; }
        atomicOr(mat + (c >> 6) * np + v, 1ull << (c & 63));
        atomicOr(mat + (v >> 6) * np + c, 1ull << (v & 63));
      }
    }
    wave_sync();
    KeySums sum;
    int terms = 0;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const int v = lane + 64 * j;
      if (v < s.n) {
#pragma unroll
        for (int w = j; w < W; ++w) take_row_word(v, w, mat[w * np + v], sum, terms);
        if ((diag >> j) & 1u) { sum.add(keys_entry_word((uint32_t)v, (uint32_t)v, 0u)); ++terms; }
      }
    }
    write_key(a, r, s, sum, terms, bad, acc, lane);
  }
  retire(a, acc, lane);
}

}  // namespace

extern "C" int gtok_graph_keys(const gtok_csr *g, const int32_t *labels, int32_t flags, uint64_t *keys, int32_t *info, void *stream) {
  const int forced = gtok::graph_keys_forced(std::getenv("GTOK_KEYS_KERNEL"));
  const int c = gtok::graph_keys_check(g, labels, flags, keys, info, forced);
  if (c < gtok::kKeysPathBase) return c < 0 ? c : GTOK_OK;
  const int path = c - gtok::kKeysPathBase;
  gtok::DeviceScope device_scope((hipStream_t)stream);   // the stream's device, not the thread's current one
  if (!device_scope.ok()) return GTOK_E_NO_DEVICE;
  hipStream_t s = (hipStream_t)stream;
  KeyArgs a;
  a.g = *g; a.labels = labels; a.keys = keys; a.info = info;
  a.stride = gtok::graph_keys_lds_bytes(path, g->max_nodes);
  a.units = a.upb = 0;
  const int G = g->num_graphs, dev = device_scope.dev;
  if (path == gtok::kKeysListed)
    return (flags & GTOK_KEYS_ATTRS) ? launch_wave_per_item(keys_stream_kernel<true, false>, a, G, 4, 0, dev, s)
                                     : launch_wave_per_item(keys_stream_kernel<false, false>, a, G, 4, 0, dev, s);
  if (path == gtok::kKeysCsr) return launch_wave_per_item(keys_stream_kernel<false, true>, a, G, 4, 0, dev, s);
  if (path == gtok::kKeysReg) return launch_wave_per_item(keys_reg_kernel, a, G, 4, a.stride, dev, s);
  switch (gtok::graph_tasks_lds_words(g->max_nodes)) {
    case 2: return launch_wave_per_item(keys_lds_kernel<2>, a, G, 4, a.stride, dev, s);
    case 4: return launch_wave_per_item(keys_lds_kernel<4>, a, G, 4, a.stride, dev, s);
    default: return launch_wave_per_item(keys_lds_kernel<8>, a, G, 4, a.stride, dev, s);
  }
}
