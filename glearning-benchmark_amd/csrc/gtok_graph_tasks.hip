// gtok_graph_tasks.hip — the task answers of a batched CSR: cycle check, components, shortest-path distances (include/gtok.h:
// gtok_graph_tasks), gfx950.
//
// One wave per graph, the waves of a workgroup independent, each with its own slice of the dynamic LDS (gtok_common.hpp).  The graph
// is the simple undirected closure of the listed entries; three searches, one per size class of the BATCH (g->max_nodes):
//   tasks_reg_kernel      <= 64 nodes: lane v holds closure row v as one 64-bit register.  The rows are OR-ed together in 512 bytes
//                         of LDS from the listed entries, both directions, the diagonal kept apart.  The closure is symmetric, so a
//                         level is PULLED: next = ballot((row & F) != 0) & ~V - no atomics, no set-bit enumeration, no queue.
//   tasks_lds_kernel<W>   <= 512 nodes: the same over a bit matrix in LDS, stored word-major (word w of node v at w * max_nodes + v: the
//                         64 lanes of a read touch consecutive 8-byte words), lane l owning nodes l + 64 j; F and V are W scalar
//                         words, a level is W ballots.  Visited nodes and empty frontier words are not read for.
//   tasks_csr_kernel      <= 16,384 nodes, simple symmetric batches: a push search over the CSR.  LDS: a visited bit per node, a
//                         16-bit level and a 16-bit FIFO slot per node.  64 nodes are popped per step, never beyond the end of the
//                         level being expanded (two lanes of levels L and L + 1 racing for a node would give it L + 2); a node is
//                         claimed by the old value of the LDS OR-atomic; appends are wave-aggregated (ballot + popcount prefix); a
//                         row of more than 64 entries is read by the whole wave, 64 entries per step.
// Components: the search is repeated from the lowest unvisited node, the visited set carried over.  A graph's queries are answered
// one after another on the resident graph; a search is RESUMABLE (frontier, visited set and the levels reached so far are kept), so
// consecutive queries with the same source continue one search instead of starting over, and a query stops at its target's level.
// Everything read through is range-checked first (graph_slice, row_range, the columns, the query endpoints); outputs are written by
// lane 0 with vector stores.
#include "gtok_common.hpp"
#include "gtok_graph_tasks_args.hpp"

namespace {
using namespace gtok;

struct TaskArgs {
  gtok_csr g;
  const int32_t *qn;          // [Q, 2] or nullptr
  const int64_t *qptr;        // [G + 1] or nullptr: one query per graph
  int64_t nq;
  int32_t *cyc, *comp, *dist, *info;
  int stride;                 // LDS bytes per wave
  int units, upb;
};

constexpr int kBadQuery = 1, kDamaged = 2;   // info[0]

struct Acc {                  // what a wave adds to info[] when it retires
  int status = 0, maxd = 0, unreach = 0, cycles = 0;
};

struct Slice {
  int n, e;                   // 0 / 0 for a damaged slice
  const int32_t *rp, *col;
  int64_t q0, q1;
};

// graph r's slices, checked against the totals of the pointer arrays and the host-known bounds the LDS tables are sized by
__device__ __forceinline__ Slice graph_slice(const TaskArgs &a, int r, int ntot, int64_t etot, Acc &acc) {
  const int nb = sload(a.g.node_ptr, r), ne = sload(a.g.node_ptr, r + 1);
  const int64_t e0 = sload(a.g.edge_ptr, r), e1 = sload(a.g.edge_ptr, r + 1);
  const bool ok = nb >= 0 && ne >= nb && ne <= ntot && ne - nb <= a.g.max_nodes && e0 >= 0 && e1 >= e0 && e1 <= etot &&
                  e1 - e0 <= (int64_t)a.g.max_edges;
  Slice s;
  s.n = ok ? ne - nb : 0;
  s.e = ok ? (int)(e1 - e0) : 0;
  s.rp = a.g.rowptr + (ok ? (int64_t)nb + r : 0);
  s.col = a.g.col + (ok ? e0 : 0);
  s.q0 = s.q1 = 0;
  if (!ok) acc.status |= kDamaged;
  if (a.qn) {
    const int64_t q0 = a.qptr ? sload(a.qptr, r) : (int64_t)r, q1 = a.qptr ? sload(a.qptr, r + 1) : (int64_t)r + 1;
    if (q0 >= 0 && q1 >= q0 && q1 <= a.nq) { s.q0 = q0; s.q1 = q1; } else acc.status |= kDamaged;
  }
  return s;
}

// row v of the slice (v < n): [x, y) inside [0, e], or empty and `bad` raised
__device__ __forceinline__ void row_range(const Slice &s, int v, int &x, int &y, int &bad) {
  x = s.rp[v]; y = s.rp[v + 1];
  if (x < 0 || y < x || y > s.e) { bad = 1; x = y = 0; }
}

// The queries of one graph on a resident search B: start(u), level_of(v) (-1: not reached yet), done() (nothing left to expand), step().
template <class B>
__device__ __forceinline__ void answer_queries(const TaskArgs &a, const Slice &s, B &bfs, Acc &acc, int lane) {
  int src = -1;
  for (int64_t q = s.q0; q < s.q1; ++q) {
    const int u = sload(a.qn, 2 * q), v = sload(a.qn, 2 * q + 1);
    int d;
    if ((unsigned)u >= (unsigned)s.n || (unsigned)v >= (unsigned)s.n) {
      d = -2; acc.status |= kBadQuery;
    } else if (u == v) {
      d = 0;
    } else {
      if (u != src) { bfs.start(u); src = u; }
      while ((d = bfs.level_of(v)) < 0 && !bfs.done()) bfs.step();
      if (d < 0) ++acc.unreach; else acc.maxd = max(acc.maxd, d);
    }
    if (lane == 0) a.dist[q] = d;
  }
}

__device__ __forceinline__ void write_graph(const TaskArgs &a, int r, int n, int m, int loops, int comp, Acc &acc, int lane) {
  const int cyc = (loops > 0 || m > n - comp) ? 1 : 0;
  acc.cycles += cyc;
  if (lane == 0) {
    if (a.cyc) a.cyc[r] = cyc;
    if (a.comp) a.comp[r] = comp;
  }
}

__device__ __forceinline__ void retire(const TaskArgs &a, const Acc &acc, int lane) {
  if (lane != 0) return;
  if (acc.status) atomicOr(a.info + 0, acc.status);
  info_max(a.info + 1, acc.maxd);
  if (acc.unreach) atomicAdd(a.info + 2, acc.unreach);
  if (acc.cycles) atomicAdd(a.info + 3, acc.cycles);
}

// ---- <= 64 nodes: closure rows in registers --------------------------------------------------------------------------------------
struct RegBfs {
  uint64_t row, F, V;
  int lane, d, lev;
  __device__ __forceinline__ void start(int u) { F = V = 1ull << u; d = 0; lev = lane == u ? 0 : -1; }
  __device__ __forceinline__ bool done() const { return F == 0; }
  __device__ __forceinline__ void step() {
    const uint64_t nx = __ballot((row & F) != 0) & ~V;
    ++d;
    if ((nx >> lane) & 1ull) lev = d;
    V |= nx; F = nx;
  }
  __device__ __forceinline__ int level_of(int v) const { return __builtin_amdgcn_readlane(lev, v); }
};

__global__ void __launch_bounds__(256) tasks_reg_kernel(const TaskArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id(), wave = wave_id(), wpb = (int)(blockDim.x >> 6);
  unsigned long long *rows = reinterpret_cast<unsigned long long *>(smem + (size_t)wave * a.stride);
  const int G = a.g.num_graphs;
  const int ntot = sload(a.g.node_ptr, G);
  const int64_t etot = sload(a.g.edge_ptr, G);
  const bool want_cc = a.cyc != nullptr || a.comp != nullptr;
  Acc acc;
  const int vb = virtual_block();
  const int u0 = vb * a.upb, u1 = min(a.units, u0 + a.upb);
  for (int unit = u0; unit < u1; ++unit) {
    const int r = unit * wpb + wave;
    if (r >= G) break;
    const Slice s = graph_slice(a, r, ntot, etot, acc);
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
    RegBfs b;
    b.lane = lane;
    b.row = mine | rows[lane];
    if (__ballot(bad != 0)) acc.status |= kDamaged;
    if (want_cc) {
      const int m = uni(wave_sum((int)__popcll(b.row))) >> 1;
      const int loops = __ballot(diag != 0) != 0 ? 1 : 0;
      const uint64_t nodes = s.n >= 64 ? ~0ull : ((1ull << s.n) - 1ull);
      uint64_t V = 0;
      int comp = 0;
      while (nodes & ~V) {
        uint64_t F = 1ull << __builtin_ctzll(nodes & ~V);
        V |= F;
        while (F) {
          F = __ballot((b.row & F) != 0) & ~V;
          V |= F;
        }
        ++comp;
      }
      write_graph(a, r, s.n, m, loops, comp, acc, lane);
    }
    answer_queries(a, s, b, acc, lane);
  }
  retire(a, acc, lane);
}

// ---- <= 512 nodes: the bit matrix in LDS -----------------------------------------------------------------------------------------
template <int W>
struct LdsBfs {
  const unsigned long long *mat;   // word w of node v at w * np + v
  int np, n, lane, d;
  uint64_t F[W], V[W];
  int lev[W];
  // V |= the neighbours of F outside V; F = those (Lev: they are given level d)
  template <bool Lev>
  __device__ __forceinline__ void expand() {
    uint64_t nx[W];
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const int v = lane + 64 * j;
      bool hit = false;
      if (v < n && !((V[j] >> lane) & 1ull)) {
#pragma unroll
        for (int w = 0; w < W; ++w)
          if (F[w]) hit |= (mat[w * np + v] & F[w]) != 0;
      }
      nx[j] = __ballot(hit);
      if (Lev && hit) lev[j] = d;
    }
#pragma unroll
    for (int j = 0; j < W; ++j) { V[j] |= nx[j]; F[j] = nx[j]; }
  }
  __device__ __forceinline__ void seed(int u) {      // F = {u}, V |= {u}
#pragma unroll
    for (int w = 0; w < W; ++w) {
      F[w] = w == (u >> 6) ? 1ull << (u & 63) : 0ull;
      V[w] |= F[w];
    }
  }
  __device__ __forceinline__ void start(int u) {
#pragma unroll
    for (int w = 0; w < W; ++w) { V[w] = 0; lev[w] = lane + 64 * w == u ? 0 : -1; }
    seed(u);
    d = 0;
  }
  __device__ __forceinline__ bool done() const {
    uint64_t any = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) any |= F[w];
    return any == 0;
  }
  __device__ __forceinline__ void step() { ++d; expand<true>(); }
  __device__ __forceinline__ int level_of(int v) const {
    int x = -1;
#pragma unroll
    for (int j = 0; j < W; ++j)
      if (j == (v >> 6)) x = lev[j];
    return __builtin_amdgcn_readlane(x, v & 63);
  }
};

template <int W>
__global__ void __launch_bounds__(256) tasks_lds_kernel(const TaskArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id(), wave = wave_id(), wpb = (int)(blockDim.x >> 6);
  unsigned long long *mat = reinterpret_cast<unsigned long long *>(smem + (size_t)wave * a.stride);
  const int G = a.g.num_graphs, np = max(a.g.max_nodes, 1);
  const int ntot = sload(a.g.node_ptr, G);
  const int64_t etot = sload(a.g.edge_ptr, G);
  const bool want_cc = a.cyc != nullptr || a.comp != nullptr;
  Acc acc;
  const int vb = virtual_block();
  const int u0 = vb * a.upb, u1 = min(a.units, u0 + a.upb);
  for (int unit = u0; unit < u1; ++unit) {
    const int r = unit * wpb + wave;
    if (r >= G) break;
    const Slice s = graph_slice(a, r, ntot, etot, acc);      // (s.n <= max_nodes <= 64 W: every word index below is < W)
    wave_sync();
#pragma unroll
    for (int w = 0; w < W; ++w)
      for (int v = lane; v < s.n; v += kWave) mat[w * np + v] = 0;
    wave_sync();
    int diag = 0, bad = 0;
    for (int v = lane; v < s.n; v += kWave) {
      int x, y;
      row_range(s, v, x, y, bad);
      for (int k = x; k < y; ++k) {
        const int c = s.col[k];
        if ((unsigned)c >= (unsigned)s.n) { bad = 1; continue; }
        if (c == v) { diag = 1; continue; }
        atomicOr(mat + (c >> 6) * np + v, 1ull << (c & 63));
        atomicOr(mat + (v >> 6) * np + c, 1ull << (v & 63));
      }
    }
    wave_sync();
    if (__ballot(bad != 0)) acc.status |= kDamaged;
    LdsBfs<W> b;
    b.mat = mat; b.np = np; b.n = s.n; b.lane = lane; b.d = 0;
    if (want_cc) {
      int bits = 0;
#pragma unroll
      for (int w = 0; w < W; ++w)
        for (int v = lane; v < s.n; v += kWave) bits += (int)__popcll(mat[w * np + v]);
      const int m = uni(wave_sum(bits)) >> 1;
      const int loops = __ballot(diag != 0) != 0 ? 1 : 0;
#pragma unroll
      for (int w = 0; w < W; ++w) { b.V[w] = 0; b.lev[w] = -1; }
      int comp = 0;
      for (;;) {
        int start = -1;
#pragma unroll
        for (int w = W - 1; w >= 0; --w) {
          const int left = s.n - 64 * w;       // nodes of word w
          const uint64_t nodes = left >= 64 ? ~0ull : left > 0 ? ((1ull << left) - 1ull) : 0ull;
          const uint64_t open = nodes & ~b.V[w];
          if (open) start = 64 * w + (int)__builtin_ctzll(open);
        }
        if (start < 0) break;
        b.seed(start);
        while (!b.done()) b.template expand<false>();
        ++comp;
      }
      write_graph(a, r, s.n, m, loops, comp, acc, lane);
    }
    answer_queries(a, s, b, acc, lane);
  }
  retire(a, acc, lane);
}

// ---- <= 16,384 nodes, simple symmetric: the push search over the CSR -------------------------------------------------------------
struct CsrBfs {
  uint32_t *vis;              // one bit per node
  uint16_t *lvl, *fifo;       // level of every claimed node; the claimed nodes in claim order
  Slice s;
  int lane, nw;               // words of vis in use
  int head, tail, lend, level;   // fifo[head .. lend) = what is left of level `level`, fifo[lend .. tail) = level + 1 so far
  int bad;
  __device__ __forceinline__ void clear() {
    wave_sync();
    for (int i = lane; i < nw; i += kWave) vis[i] = 0;
    wave_sync();
  }
  __device__ __forceinline__ void seed(int u) {      // a search from u on the visited set as it stands (u not in it)
    if (lane == 0) {
      vis[u >> 5] |= 1u << (u & 31);
      lvl[u] = 0;
      fifo[0] = (uint16_t)u;
    }
    head = 0; tail = 1; lend = 1; level = 0;
    wave_sync();
  }
  __device__ __forceinline__ void start(int u) { clear(); seed(u); }
  __device__ __forceinline__ bool done() const { return head >= tail; }
  // the lanes with `active` try to claim their column; the winners append themselves behind `tail`
  __device__ __forceinline__ void claim(int c, bool active) {
    bool won = false;
    if (active) {
      if ((unsigned)c < (unsigned)s.n) {
        const uint32_t bit = 1u << (c & 31);
        won = !(atomicOr(vis + (c >> 5), bit) & bit);
      } else {
        bad = 1;
      }
    }
    const uint64_t b = __ballot(won);
    if (won) {
      const int pos = tail + (int)__popcll(b & lanemask_lt());     // (every node is claimed once: pos < n)
      fifo[pos] = (uint16_t)c;
      lvl[c] = (uint16_t)(level + 1);
    }
    tail += (int)__popcll(b);
  }
  __device__ __forceinline__ void step() {
    const int cnt = min(kWave, lend - head);                        // never beyond the level's end
    int rs = 0, dg = 0;
    if (lane < cnt) {
      const int x = (int)fifo[head + lane];
      int y;
      row_range(s, x, rs, y, bad);
      dg = y - rs;
    }
    head += cnt;
    const int shortest = uni(wave_max(dg <= kWave ? dg : 0));
    for (int i = 0; i < shortest; ++i) {                            // rows of up to 64 entries: a lane each
      const bool on = dg <= kWave && i < dg;
      claim(on ? s.col[rs + i] : 0, on);
    }
    uint64_t todo = __ballot(dg > kWave);                           // longer rows: the whole wave on each
    while (todo) {
      const int L = (int)__builtin_ctzll(todo);
      todo &= todo - 1;
      const int urs = __builtin_amdgcn_readlane(rs, L), ud = __builtin_amdgcn_readlane(dg, L);
      for (int k0 = 0; k0 < ud; k0 += kWave) {
        const int k = k0 + lane;
        claim(k < ud ? s.col[urs + k] : 0, k < ud);
      }
    }
    wave_sync();
    if (head == lend) { ++level; lend = tail; }
  }
  __device__ __forceinline__ int level_of(int v) const {            // v uniform: a broadcast read
    const uint32_t w = vis[v >> 5];
    const int x = (w >> (v & 31)) & 1u ? (int)lvl[v] : -1;
    return uni(x);
  }
  // lowest node outside the visited set at or behind word `cursor` (which it moves up to that node's word); -1: none
  __device__ __forceinline__ int lowest_open(int &cursor) {
    const int nwn = (s.n + 31) >> 5;
    for (int w0 = cursor; w0 < nwn; w0 += kWave) {
      const int w = w0 + lane;
      uint32_t open = 0;
      if (w < nwn) {
        open = ~vis[w];
        if (w == nwn - 1 && (s.n & 31)) open &= (1u << (s.n & 31)) - 1u;
      }
      const uint64_t b = __ballot(open != 0);
      if (b) {
        const int L = (int)__builtin_ctzll(b);
        const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)open, L);
        cursor = w0 + L;
        return (w0 + L) * 32 + (int)__builtin_ctz(word);
      }
    }
    cursor = nwn;
    return -1;
  }
};

__global__ void __launch_bounds__(256) tasks_csr_kernel(const TaskArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id(), wave = wave_id(), wpb = (int)(blockDim.x >> 6);
  unsigned char *mine = smem + (size_t)wave * a.stride;
  const int np = max(a.g.max_nodes, 1);
  const int off_lvl = ((np + 31) / 32 * 4 + 15) & ~15, off_fifo = off_lvl + ((np * 2 + 15) & ~15);   // graph_tasks_lds_bytes' layout
  const int G = a.g.num_graphs;
  const int ntot = sload(a.g.node_ptr, G);
  const int64_t etot = sload(a.g.edge_ptr, G);
  const bool want_cc = a.cyc != nullptr || a.comp != nullptr;
  Acc acc;
  const int vb = virtual_block();
  const int u0 = vb * a.upb, u1 = min(a.units, u0 + a.upb);
  for (int unit = u0; unit < u1; ++unit) {
    const int r = unit * wpb + wave;
    if (r >= G) break;
    CsrBfs b;
    b.vis = reinterpret_cast<uint32_t *>(mine);
    b.lvl = reinterpret_cast<uint16_t *>(mine + off_lvl);
    b.fifo = reinterpret_cast<uint16_t *>(mine + off_fifo);
    b.s = graph_slice(a, r, ntot, etot, acc);
    b.lane = lane; b.nw = (b.s.n + 31) >> 5; b.bad = 0;
    b.head = b.tail = b.lend = b.level = 0;
    if (want_cc) {
      b.clear();
      int comp = 0, cursor = 0;
      for (;;) {
        const int start = b.lowest_open(cursor);
        if (start < 0) break;
        b.seed(start);
        while (!b.done()) b.step();
        ++comp;
      }
      write_graph(a, r, b.s.n, b.s.e >> 1, 0, comp, acc, lane);      // simple and symmetric: m = E / 2, no loops
    }
    answer_queries(a, b.s, b, acc, lane);
    if (__ballot(b.bad != 0)) acc.status |= kDamaged;
  }
  retire(a, acc, lane);
}

}  // namespace

extern "C" int gtok_graph_tasks(const gtok_csr *g, const int32_t *query_nodes, const int64_t *query_ptr, int64_t num_queries,
                                int32_t *has_cycle, int32_t *num_components, int32_t *dist, int32_t *info, void *stream) {
  const int forced = gtok::graph_tasks_forced(std::getenv("GTOK_TASKS_KERNEL"));
  const int c = gtok::graph_tasks_check(g, query_nodes, query_ptr, num_queries, has_cycle, num_components, dist, info, forced);
  if (c < gtok::kTasksPathBase) return c < 0 ? c : GTOK_OK;
  const int path = c - gtok::kTasksPathBase;
  gtok::DeviceScope device_scope((hipStream_t)stream);   // the stream's device, not the thread's current one
  if (!device_scope.ok()) return GTOK_E_NO_DEVICE;
  hipStream_t s = (hipStream_t)stream;
  TaskArgs a;
  a.g = *g; a.qn = query_nodes; a.qptr = query_ptr; a.nq = num_queries;
  a.cyc = has_cycle; a.comp = num_components; a.dist = dist; a.info = info;
  a.stride = gtok::graph_tasks_lds_bytes(path, g->max_nodes);
  a.units = a.upb = 0;
  const int G = g->num_graphs, dev = device_scope.dev;
  if (path == gtok::kTasksReg) return launch_wave_per_item(tasks_reg_kernel, a, G, 4, a.stride, dev, s);
  if (path == gtok::kTasksCsr) return launch_wave_per_item(tasks_csr_kernel, a, G, 4, a.stride, dev, s);
  switch (gtok::graph_tasks_lds_words(g->max_nodes)) {
    case 2: return launch_wave_per_item(tasks_lds_kernel<2>, a, G, 4, a.stride, dev, s);
    case 4: return launch_wave_per_item(tasks_lds_kernel<4>, a, G, 4, a.stride, dev, s);
    default: return launch_wave_per_item(tasks_lds_kernel<8>, a, G, 4, a.stride, dev, s);
  }
}
