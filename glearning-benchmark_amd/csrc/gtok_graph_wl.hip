// gtok_graph_wl.hip — a 128-bit key per graph of a batched CSR that does not depend on the numbering: Weisfeiler-Lehman colour
// refinement (include/gtok.h: gtok_graph_wl; the arithmetic: gtok_graph_wl_hash.hpp), gfx950.
//
// One wave per graph, the waves of a workgroup independent, each with its own slice of the dynamic LDS (gtok_common.hpp) - the
// conventions of gtok_graph_tasks.hip / gtok_graph_keys.hip.  A round is a pull: every node sums one mixed word per neighbour and
// mixes the sum into its own colour.  Structure-only terms depend on the neighbour alone, so a round first writes every node's term
// wl_term(c[u], 0) into a table and then every node sums the table entries of its neighbours.
//   wl_reg_kernel        <= 64 nodes, any listing: lane v holds closure row v as one 64-bit register (built as keys_reg_kernel builds
//                        it, the diagonal kept apart) and its colour; the 64-entry term table is in LDS, lane v sums the entries of its
//                        set bits.
//   wl_lds_kernel<W>     <= 512 nodes, any listing: the bit matrix in LDS as keys_lds_kernel<W> builds it, word-major, plus the term
//                        table (8 bytes per node); lane l owns nodes l + 64 j, their colours in W registers.
//   wl_csr_kernel<Attrs, Global>   GTOK_CSR_SIMPLE_SYMMETRIC batches: every row is the node's complete neighbour list, deg = the row's
//                        length, no loops.  Lane l owns nodes l + 64 j.  Two 8-byte tables per node: colours and terms (structure
//                        only), or this round's and the next round's colours (Attrs: a term carries the entry's own eattr byte).  The
//                        tables are in LDS up to 4,096 nodes; beyond (Global) in the caller's workspace, one slice per wave, a one-wave
//                        workgroup per slice, wave w taking graphs w, w + waves, ...; slice_sync drains a round's stores before the
//                        next round's loads.
// A hub's row is one lane's loop on all three paths.  Everything read through is range-checked first (the slice, the row bounds, the
// columns); a table is only ever indexed by a checked node id below the max_nodes it is sized by.
#include "gtok_common.hpp"
#include "gtok_graph_wl_args.hpp"
#include "gtok_graph_wl_hash.hpp"

namespace {
using namespace gtok;

struct WlArgs {
  gtok_csr g;
  const int32_t *labels;      // [G] or nullptr
  uint64_t *keys;             // [G, 2]
  uint64_t *colors;           // [node_ptr[G]] or nullptr
  int32_t *info;
  int rounds;
  int stride;                 // LDS bytes per wave
  int units, upb;
  unsigned char *ws;          // Global: one slice of 16 * max(max_nodes, 1) bytes per wave
};

constexpr int kDamaged = 2;   // info[0]

struct Acc {                  // what a wave adds to info[] when it retires
  int status = 0, damaged = 0;
};

struct Slice {
  int n, e, nb;               // 0 / 0 / 0 for a damaged slice
  bool ok;
  const int32_t *rp, *col;
  const uint8_t *na, *ea;     // the slice's attribute bytes (read with GTOK_WL_ATTRS only)
};

// graph r's slices, checked against the totals of the pointer arrays and the host-known bounds the tables are sized by
__device__ __forceinline__ Slice graph_slice(const WlArgs &a, int r, int ntot, int64_t etot) {
  const int nb = sload(a.g.node_ptr, r), ne = sload(a.g.node_ptr, r + 1);
  const int64_t e0 = sload(a.g.edge_ptr, r), e1 = sload(a.g.edge_ptr, r + 1);
  const bool ok = nb >= 0 && ne >= nb && ne <= ntot && ne - nb <= a.g.max_nodes && e0 >= 0 && e1 >= e0 && e1 <= etot &&
                  e1 - e0 <= (int64_t)a.g.max_edges;
  Slice s;
  s.ok = ok;
  s.n = ok ? ne - nb : 0;
  s.e = ok ? (int)(e1 - e0) : 0;
  s.nb = ok ? nb : 0;
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

// the wave's sums over the final colours -> the graph's key, written by lane 0; the damage of this graph -> acc
__device__ __forceinline__ void write_key(const WlArgs &a, int r, const Slice &s, const WlSums &mine, int bad, Acc &acc, int lane) {
  WlSums all;
  all.s0 = (uint64_t)wave_sum64((int64_t)mine.s0);
  all.s1 = (uint64_t)wave_sum64((int64_t)mine.s1);
  if (!s.ok || __ballot(bad != 0)) { acc.status |= kDamaged; ++acc.damaged; }
  const int label = a.labels ? sload(a.labels, r) : 0;
  uint64_t k[2];
  wl_finish(all, (uint32_t)s.n, wl_rounds_run(a.rounds, s.n), label, k);
  if (lane == 0) {
    a.keys[2 * (int64_t)r] = k[0];
    a.keys[2 * (int64_t)r + 1] = k[1];
  }
}

__device__ __forceinline__ void retire(const WlArgs &a, const Acc &acc, int lane) {
  if (lane != 0 || !acc.status) return;
  atomicOr(a.info + 0, acc.status);
  atomicAdd(a.info + 1, acc.damaged);
}

// ---- <= 64 nodes: closure rows in registers, the term table in LDS -----------------------------------------------------------------
__global__ void __launch_bounds__(256) wl_reg_kernel(const WlArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id(), wave = wave_id(), wpb = (int)(blockDim.x >> 6);
  unsigned long long *rows = reinterpret_cast<unsigned long long *>(smem + (size_t)wave * a.stride);
  unsigned long long *term = rows + 64;
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
    const uint64_t row = mine | rows[lane];                             // (bits below s.n only: both ends were checked)
    uint64_t c = wl_init((uint32_t)__popcll(row), (uint32_t)diag, 0u);
    const int R = (int)wl_rounds_run(a.rounds, s.n);
    for (int it = 0; it < R; ++it) {
      term[lane] = wl_term(c, 0u);
      wave_sync();
      uint64_t sum = 0;
      for (uint64_t w = row; w; w &= w - 1) sum += term[__builtin_ctzll(w)];
      wave_sync();                                                      // (every lane has read before the next round's terms land)
      c = wl_next(c, sum);
    }
    WlSums sums;
    if (lane < s.n) {
      sums.add(c);
      if (a.colors) a.colors[(int64_t)s.nb + lane] = c;
    }
    write_key(a, r, s, sums, bad, acc, lane);
  }
  retire(a, acc, lane);
}

// ---- <= 512 nodes: the bit matrix and the term table in LDS -------------------------------------------------------------------------
template <int W>
__global__ void __launch_bounds__(256) wl_lds_kernel(const WlArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id(), wave = wave_id(), wpb = (int)(blockDim.x >> 6);
  unsigned long long *mat = reinterpret_cast<unsigned long long *>(smem + (size_t)wave * a.stride);
  const int G = a.g.num_graphs, np = max(a.g.max_nodes, 1);
  unsigned long long *term = mat + W * np;                              // [np]
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
    uint64_t c[W];
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const int v = lane + 64 * j;
      int deg = 0;
      if (v < s.n) {
#pragma unroll
        for (int w = 0; w < W; ++w) deg += (int)__popcll(mat[w * np + v]);
      }
      c[j] = wl_init((uint32_t)deg, (diag >> j) & 1u, 0u);
    }
    const int R = (int)wl_rounds_run(a.rounds, s.n);
    for (int it = 0; it < R; ++it) {
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const int v = lane + 64 * j;
        if (v < s.n) term[v] = wl_term(c[j], 0u);
      }
      wave_sync();
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const int v = lane + 64 * j;
        if (v < s.n) {
          uint64_t sum = 0;
#pragma unroll
          for (int w = 0; w < W; ++w)
            for (uint64_t word = mat[w * np + v]; word; word &= word - 1) sum += term[64 * w + (int)__builtin_ctzll(word)];
          c[j] = wl_next(c[j], sum);
        }
      }
      wave_sync();
    }
    WlSums sums;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const int v = lane + 64 * j;
      if (v < s.n) {
        sums.add(c[j]);
        if (a.colors) a.colors[(int64_t)s.nb + v] = c[j];
      }
    }
    write_key(a, r, s, sums, bad, acc, lane);
  }
  retire(a, acc, lane);
}

// ---- GTOK_CSR_SIMPLE_SYMMETRIC batches: a pull over the CSR rows ---------------------------------------------------------------------
// stores to a table drained before another lane of the wave loads them: LDS ops of a wave execute in issue order (wave_sync); the
// workspace slice is written with plain stores and read back behind a workgroup-scope fence (the workgroup is this one wave)
template <bool Global>
__device__ __forceinline__ void table_sync() {
  if (Global) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  } else {
    wave_sync();
  }
}

template <bool Attrs, bool Global>
__device__ __forceinline__ void wl_csr_graph(const WlArgs &a, int r, int ntot, int64_t etot, unsigned long long *ta, unsigned long long *tb,
                                             Acc &acc, int lane) {
  const Slice s = graph_slice(a, r, ntot, etot);                        // (s.n <= max_nodes: the tables hold max(max_nodes, 1) words)
  int bad = 0;
  table_sync<Global>();                                                 // (the graph before this one has been read to its end)
  for (int v = lane; v < s.n; v += kWave) {
    int x, y;
    row_range(s, v, x, y, bad);
    const uint64_t c = wl_init((uint32_t)(y - x), 0u, Attrs ? 1u + (uint32_t)s.na[v] : 0u);
    ta[v] = c;
    if (!Attrs) tb[v] = wl_term(c, 0u);
  }
  table_sync<Global>();
  const int R = (int)wl_rounds_run(a.rounds, s.n);
  for (int it = 0; it < R; ++it) {
    for (int v = lane; v < s.n; v += kWave) {
      int x, y, rowbad = 0;
      row_range(s, v, x, y, rowbad);
      uint64_t sum = 0;
      for (int k = x; k < y; ++k) {
        const int u = s.col[k];
        if ((unsigned)u >= (unsigned)s.n) { bad = 1; continue; }
        sum += Attrs ? wl_term(ta[u], 1u + (uint32_t)s.ea[k]) : tb[u];
      }
      // structure only: colour v is read and written by its owner alone, in place; Attrs: into the other table
      (Attrs ? tb : ta)[v] = wl_next(ta[v], sum);
    }
    table_sync<Global>();
    if (Attrs) {
      unsigned long long *t = ta; ta = tb; tb = t;
    } else if (it + 1 < R) {
      for (int v = lane; v < s.n; v += kWave) tb[v] = wl_term(ta[v], 0u);
      table_sync<Global>();
    }
  }
  WlSums sums;
  for (int v = lane; v < s.n; v += kWave) {
    const uint64_t c = ta[v];
    sums.add(c);
    if (a.colors) a.colors[(int64_t)s.nb + v] = c;
  }
  write_key(a, r, s, sums, bad, acc, lane);
}

template <bool Attrs, bool Global>
__global__ void __launch_bounds__(Global ? 64 : 256) wl_csr_kernel(const WlArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id();
  const int G = a.g.num_graphs, np = max(a.g.max_nodes, 1);
  const int ntot = sload(a.g.node_ptr, G);
  const int64_t etot = sload(a.g.edge_ptr, G);
  Acc acc;
  if (Global) {
    unsigned long long *ta = reinterpret_cast<unsigned long long *>(a.ws + (size_t)blockIdx.x * 16u * (size_t)np);
    for (int r = (int)blockIdx.x; r < G; r += (int)gridDim.x) wl_csr_graph<Attrs, true>(a, r, ntot, etot, ta, ta + np, acc, lane);
  } else {
    const int wave = wave_id(), wpb = (int)(blockDim.x >> 6);
    unsigned long long *ta = reinterpret_cast<unsigned long long *>(smem + (size_t)wave * a.stride);
    const int vb = virtual_block();
    const int u0 = vb * a.upb, u1 = min(a.units, u0 + a.upb);
    for (int unit = u0; unit < u1; ++unit) {
      const int r = unit * wpb + wave;
      if (r >= G) break;
      wl_csr_graph<Attrs, false>(a, r, ntot, etot, ta, ta + np, acc, lane);
    }
  }
  retire(a, acc, lane);
}

template <bool Attrs>
int launch_csr_global(WlArgs &a, hipStream_t s) {
  const int waves = gtok::graph_wl_waves(a.g.num_graphs);
  hipLaunchKernelGGL((wl_csr_kernel<Attrs, true>), dim3(waves), dim3(64), 0, s, a);
  return hipGetLastError() == hipSuccess ? GTOK_OK : GTOK_E_LAUNCH;
}

}  // namespace

extern "C" int64_t gtok_graph_wl_workspace(int32_t max_nodes, int32_t num_graphs) { return gtok::graph_wl_workspace(max_nodes, num_graphs); }

extern "C" int gtok_graph_wl(const gtok_csr *g, const int32_t *labels, int32_t rounds, int32_t flags, uint64_t *keys, uint64_t *node_colors,
                             int32_t *info, void *workspace, int64_t workspace_bytes, void *stream) {
  const int forced = gtok::graph_wl_forced(std::getenv("GTOK_WL_KERNEL"));
  const int c = gtok::graph_wl_check(g, labels, rounds, flags, keys, node_colors, info, workspace, workspace_bytes, forced);
  if (c < gtok::kWlPathBase) return c < 0 ? c : GTOK_OK;
  const int path = c - gtok::kWlPathBase;
  gtok::DeviceScope device_scope((hipStream_t)stream);   // the stream's device, not the thread's current one
  if (!device_scope.ok()) return GTOK_E_NO_DEVICE;
  hipStream_t s = (hipStream_t)stream;
  WlArgs a;
  a.g = *g; a.labels = labels; a.keys = keys; a.colors = node_colors; a.info = info; a.rounds = rounds;
  a.stride = gtok::graph_wl_lds_bytes(path, g->max_nodes);
  a.units = a.upb = 0;
  a.ws = static_cast<unsigned char *>(workspace);
  const int G = g->num_graphs, dev = device_scope.dev;
  const bool attrs = (flags & GTOK_WL_ATTRS) != 0;
  if (path == gtok::kWlReg) return launch_wave_per_item(wl_reg_kernel, a, G, 4, a.stride, dev, s);
  if (path == gtok::kWlLds) {
    switch (gtok::graph_tasks_lds_words(g->max_nodes)) {
      case 2: return launch_wave_per_item(wl_lds_kernel<2>, a, G, 4, a.stride, dev, s);
      case 4: return launch_wave_per_item(wl_lds_kernel<4>, a, G, 4, a.stride, dev, s);
      default: return launch_wave_per_item(wl_lds_kernel<8>, a, G, 4, a.stride, dev, s);
    }
  }
  if (g->max_nodes > gtok::kWlCsrLdsMaxNodes) return attrs ? launch_csr_global<true>(a, s) : launch_csr_global<false>(a, s);
  return attrs ? launch_wave_per_item(wl_csr_kernel<true, false>, a, G, 4, a.stride, dev, s)
               : launch_wave_per_item(wl_csr_kernel<false, false>, a, G, 4, a.stride, dev, s);
}
