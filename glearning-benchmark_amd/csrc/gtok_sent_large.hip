// gtok_sent_large.hip — SENT trail walk for graphs of up to GTOK_SENT_LARGE_MAX_NODES nodes, gfx950.
//
// Same spec, same tokens and same output convention as gtok_sent (bit-exact checker
// oracle/gtok_oracle.c:oracle_sent), for the batches gtok_sent refuses: its kernels hold a graph as an N x N bit
// matrix (registers, a mirror, or LDS), which ends at 512 nodes.  This kernel keeps NO per-edge state:
//   after visit(v) every edge between two visited nodes is covered, so the uncovered edges of a visited node are exactly
//   its entries - listed in either direction - whose other end is unvisited.
// One wave walks one (graph, epoch) pair; wave w of the launch takes pairs w, w + waves, ... (static).  Per wave:
//   LDS     four N-bit sets (visited; live = visited nodes that still own uncovered edges; a node-space and a visit-space
//           scratch set), the node -> visit index table (16 bits per node) and a window of the token row
//   slice   (caller's workspace, one per wave) cnt[N]: entries of a visited node whose other end is unvisited; key[N]: per
//           visit index, the entry that decides a bracket member's edge type; the IN-lists of the graph (for every node the
//           entries w -> u that name it, with their CSR positions) for batches without GTOK_CSR_SIMPLE_SYMMETRIC
// cnt / key are only ever touched with agent-scope atomics (they are updated by atomics at L2: a plain load could hit a
// stale L1 line); the in-lists are written once per pair with plain stores and read back behind a workgroup-scope fence.
// Nothing of the slice is read through a const __restrict__ pointer (the scalar cache would return stale bytes): only the
// caller's immutable CSR arrays go that way.
// Separate translation unit: the register allocation of gtok_sent.hip's kernels is untouched by it.
// gtok_sent_large_order runs the same walk through instantiations of their own (ORD = 1: rows and the visit order, ORD = 2: the
// order alone, no token leaves the wave): when a walk ends the wave copies its node -> visit index table from LDS to the caller's
// array.  The ORD = 0 instantiations are gtok_sent_large's, compiled as before (profiles/sent_order/kernel_resources.md).
#include "gtok_common.hpp"
#include "gtok.h"
#include "gtok_sent_reg.hpp"

namespace gtok {

constexpr int kLargeWin = 512;        // ids of the token window in LDS (one reserve() asks for 66 at the most)
constexpr int kLargeLimit = 0x70000000;   // token positions are counted in 31 bits: max_len beyond this reads as this

struct LargeArgs {
  gtok_csr g;
  gtok_sent_params p;
  int32_t *out;
  int ld;
  int32_t *out_len;
  unsigned char *ws;      // one slice per wave
  int64_t slice;          // bytes
  int64_t off_key, off_inptr, off_insrc, off_inpos;   // cnt at 0
  int maxn, maxe;         // the batch's claims: a graph beyond them is clamped to them (the slice and the LDS tables are sized by them)
  int nw;                 // 32-bit words of a set in LDS
  int pairs;              // (graph, epoch) pairs, epoch-major
  int32_t *visit_index;   // gtok_sent_large_order only: [K, order_stride], epoch-major
  int64_t order_stride;   // elements
};

__device__ __forceinline__ void slice_sync() {   // stores to the slice drained before another lane loads them
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ int aload(int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void astore(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int aadd(int *p, int v) { return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void amin(unsigned *p, unsigned v) { (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ unsigned wave_umin(unsigned x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x = min(x, (unsigned)__shfl_xor((int)x, o));
  return uni(x);
}

// k-th (0-based, ascending) member of the set whose 32-bit word i is word_at(i), i in [wlo, whi); -1 when the set has
// k members or fewer (a batch flagged or sized wrongly: the callers fall back, nothing is indexed with it)
template <class F>
__device__ __forceinline__ int select_kth(F word_at, int wlo, int whi, int k) {
  const int lane = lane_id();
  int base = 0;
  for (int w0 = wlo; w0 < whi; w0 += kWave) {
    const int i = w0 + lane;
    const uint32_t word = i < whi ? word_at(i) : 0u;
    const int c = __popc(word);
    const int incl = wave_incl_scan(c);
    const int total = __builtin_amdgcn_readlane(incl, 63);
    if (k < base + total) {
      const int kk = k - base;
      const int L = __builtin_ctzll((uint64_t)__ballot(incl > kk));
      const uint32_t wd = (uint32_t)__builtin_amdgcn_readlane((int)word, L);
      const int ex = __builtin_amdgcn_readlane(incl - c, L);
      return (w0 + L) * 32 + kth_bit_reg((uint64_t)wd, kk - ex);
    }
    base += total;
  }
  return -1;
}

// ORD: 0 = the rows (gtok_sent_large), 1 = the rows and the visit order, 2 = the visit order alone (tokens are counted, not stored,
// and no type is looked up)
template <bool LAB, int ORD = 0>
__global__ void __launch_bounds__(64) sent_large_kernel(const LargeArgs a) {
  constexpr bool TOK = ORD != 2;          // rows are written
  constexpr bool TY = LAB && TOK;         // ... with their type tokens
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id();
  const bool is0 = lane == 0;
  const int nw = a.nw;
  uint32_t *vis = reinterpret_cast<uint32_t *>(smem);
  uint32_t *live = vis + nw;
  uint32_t *scr = live + nw;      // node space: the unvisited neighbours of the current node
  uint32_t *vscr = scr + nw;      // visit-index space: the members of a bracket
  int32_t *win = reinterpret_cast<int32_t *>(vscr + nw);
  uint16_t *vidx = reinterpret_cast<uint16_t *>(win + kLargeWin);   // node -> visit index, 0xFFFF = unvisited

  unsigned char *slice = a.ws + (int64_t)blockIdx.x * a.slice;
  int *cnt = reinterpret_cast<int *>(slice);
  int *key = reinterpret_cast<int *>(slice + a.off_key);
  int *inptr = reinterpret_cast<int *>(slice + a.off_inptr);
  int *insrc = reinterpret_cast<int *>(slice + a.off_insrc);
  int *inpos = reinterpret_cast<int *>(slice + a.off_inpos);

  const int lim = min(a.p.max_len, kLargeLimit);
  const int cap = min(lim, a.ld);
  const int idx_off = GTOK_SENT_IDX_OFFSET;
  const int node_off = idx_off + a.p.max_num_nodes;
  const int edge_off = node_off + a.p.num_node_types;
  const uint32_t k0 = (uint32_t)a.p.seed, k1 = (uint32_t)(a.p.seed >> 32), epoch0 = (uint32_t)a.p.epoch;
  const bool remap = a.p.remap_zinc != 0;
  const bool u16 = (a.p.flags & GTOK_SENT_U16) != 0;
  const bool sym = (a.g.flags & GTOK_CSR_SIMPLE_SYMMETRIC) != 0;   // every row is the node's whole neighbour list: no in-lists
  constexpr int per = LAB ? 2 : 1;
  const int G = a.g.num_graphs;

  for (int gv = (int)blockIdx.x; gv < a.pairs; gv += (int)gridDim.x) {
    const int g = gv % G;
    const uint32_t epoch = epoch0 + (uint32_t)(gv / G);
    const int nb0 = sload(a.g.node_ptr, g);
    const int nfull = sload(a.g.node_ptr, g + 1) - nb0;
    const int n = max(0, min(nfull, a.maxn));                       // (a graph beyond the batch's claims is clamped to them)
    const int64_t e0 = sload(a.g.edge_ptr, g);
    const int64_t efull = sload(a.g.edge_ptr, g + 1) - e0;
    const int e = (int)max((int64_t)0, min(efull, (int64_t)a.maxe));
    const int32_t *__restrict__ rpg = a.g.rowptr + nb0 + g;
    const int32_t *__restrict__ colg = a.g.col + e0;
    const uint64_t gid = (uint64_t)(a.p.graph_base + g);
    const uint32_t gid_lo = (uint32_t)gid, gid_hi = (uint32_t)(gid >> 32);
    const int nwn = (n + 31) >> 5;                                  // words of this graph's sets
    int32_t *row32 = a.out + (int64_t)gv * a.ld;
    uint16_t *row16 = reinterpret_cast<uint16_t *>(a.out) + (int64_t)gv * a.ld;

    // row u's entries, as positions [rs, re) inside [0, e) whatever the row pointers say
    auto row_bounds = [&](int u, int &rs, int &re) {
      rs = min(max(rpg[u], 0), e);
      re = min(max(rpg[u + 1], rs), e);
    };

    // ---- a wave's LDS and slice hold the previous walk: everything is set again
    wave_sync();
    for (int i = lane; i < nw; i += kWave) { vis[i] = 0; live[i] = 0; scr[i] = 0; vscr[i] = 0; }
    for (int i = lane; i < n; i += kWave) vidx[i] = 0xFFFFu;
    bool has_in = false;
    if (!sym && e > 0 && n > 0) {   // in-lists: in-degrees (key[] serves as counter, then as cursor), a scan, a scatter
      has_in = true;
      for (int i = lane; i < n; i += kWave) astore(key + i, 0);
      slice_sync();
      for (int u = lane; u < n; u += kWave) {
        int rs, re;
        row_bounds(u, rs, re);
        for (int k = rs; k < re; ++k) {
          const int w = colg[k];
          if ((unsigned)w < (unsigned)n && w != u) (void)aadd(key + w, 1);   // (a self loop is an out-entry only)
        }
      }
      slice_sync();
      int carry = 0;
      for (int b = 0; b < n; b += kWave) {
        const int i = b + lane;
        const int c = i < n ? aload(key + i) : 0;
        const int incl = wave_incl_scan(c);
        if (i < n) { inptr[i] = carry + incl - c; astore(key + i, carry + incl - c); }
        carry += __builtin_amdgcn_readlane(incl, 63);
      }
      if (is0) inptr[n] = carry;
      slice_sync();
      for (int u = lane; u < n; u += kWave) {
        int rs, re;
        row_bounds(u, rs, re);
        for (int k = rs; k < re; ++k) {
          const int w = colg[k];
          if ((unsigned)w < (unsigned)n && w != u) {
            const int q = aadd(key + w, 1);
            if ((unsigned)q < (unsigned)e) { insrc[q] = u; inpos[q] = k; }
          }
        }
      }
      slice_sync();
    }
    for (int i = lane; i < n; i += kWave) astore(key + i, -1);
    slice_sync();

    // every incident entry of v, 64 per round: f(valid, w, dir, pos) with w the other end, dir 0 = listed v -> w (row v),
    // 1 = listed w -> v (in-list of v), pos = the entry's CSR position inside the graph.  All lanes call f.
    auto for_entries = [&](int v, auto f) {
      int rs, re;
      row_bounds(v, rs, re);
      rs = uni(rs); re = uni(re);
      int is = 0, ie = 0;
      if (has_in) {
        is = uni(min(max(inptr[v], 0), e));
        ie = uni(min(max(inptr[v + 1], is), e));
      }
      const int dout = re - rs, total = dout + (ie - is);
      for (int t0 = 0; t0 < total; t0 += kWave) {
        const int t = t0 + lane;
        int w = -1, dir = 0, pos = 0;
        if (t < dout) { pos = rs + t; w = colg[pos]; }
        else if (t < total) { const int j = is + (t - dout); w = insrc[j]; pos = min(max(inpos[j], 0), e - 1); dir = 1; }
        f((unsigned)w < (unsigned)n, w, dir, pos);
      }
    };

    // ---- decisions: lane j holds the word of decision d0 + j (decision-major Philox block, 64 per refill)
    auto draws = [&](int d0) -> uint32_t {
      uint32_t o[4];
      philox4x32_10((uint32_t)((d0 + lane) >> 2), epoch, gid_lo, gid_hi, k0, k1, o);
      const int w = lane & 3;
      uint32_t x = o[3];
      x = w == 2 ? o[2] : x;
      x = w == 1 ? o[1] : x;
      x = w == 0 ? o[0] : x;
      return x;
    };
    uint32_t R = draws(0);
    int d = 0;
    auto below = [&](uint32_t nchoices) -> uint32_t {
      const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)R, d & 63);
      ++d;
      if ((d & 63) == 0) R = draws(d);
      return __umulhi(x, nchoices);
    };

    // ---- tokens: a window of the row in LDS, flushed with coalesced stores; positions beyond min(max_len, ld) are counted only
    int pos = 0, wbase = 0;
    auto flush = [&]() {
      wave_sync();
      const int count = pos - wbase;
      for (int i = lane; TOK && i < count; i += kWave) {
        const int q = wbase + i;
        if (q < cap) {
          int t = win[i];
          if (remap) t = remap_zinc_token(t, idx_off, node_off, edge_off);
          if (u16) row16[q] = (uint16_t)t; else row32[q] = t;
        }
      }
      wave_sync();
      wbase = pos;
    };
    auto reserve = [&](int k) { if (pos - wbase + k > kLargeWin) flush(); };   // k <= 66
    auto emit1 = [&](int t) { reserve(1); if (is0) win[pos - wbase] = t; pos += 1; };

    int nvis = 0, nlive = 0, cur = 0;

    // first visit of v; pred >= 0: reached over the trail edge (pred, v) whose type token is et
    auto visit = [&](int v, int pred, int et) {
      const int kv = nvis;
      if (is0) { vidx[v] = (uint16_t)kv; vis[v >> 5] |= 1u << (v & 31); }
      wave_sync();
      int cntv = 0, dead = 0, klo = 0x7FFFFFFF, khi = -1;
      for_entries(v, [&](bool valid, int w, int dir, int p) {
        if (!valid) return;
        int kw;
        if (w == v) kw = kv;                   // a self loop: v is a member of its own bracket
        else {
          kw = vidx[w];
          if (kw == 0xFFFF) { ++cntv; return; }
          if (aadd(cnt + w, -1) == 1) { atomicAnd(live + (w >> 5), ~(1u << (w & 31))); ++dead; }
          if (w == pred) return;
        }
        atomicOr(vscr + (kw >> 5), 1u << (kw & 31));
        klo = min(klo, kw); khi = max(khi, kw);
        if (TY) amin(reinterpret_cast<unsigned *>(key + kw), ((unsigned)dir << 31) | (unsigned)p);
      });
      cntv = uni(wave_sum(cntv)); dead = uni(wave_sum(dead)); klo = uni(wave_min(klo)); khi = uni(wave_max(khi));
      nlive -= dead;
      wave_sync();
      if (is0) {
        astore(cnt + v, cntv);
        if (cntv > 0) live[v >> 5] |= 1u << (v & 31);
      }
      nlive += cntv > 0 ? 1 : 0;
      slice_sync();

      reserve(3);
      {
        const int o = pos - wbase;
        if (LAB) {
          const int ty = TY ? node_off + a.g.nattr[nb0 + v] : 0;
          if (pred >= 0) {
            if (lane < 3) win[o + lane] = lane == 0 ? et : lane == 1 ? idx_off + kv : ty;
            pos += 3;
          } else {
            if (lane < 2) win[o + lane] = lane == 0 ? idx_off + kv : ty;
            pos += 2;
          }
        } else {
          if (is0) win[o] = idx_off + kv;
          pos += 1;
        }
      }
      if (khi >= 0) {   // the bracket: members in ascending visit index
        emit1(GTOK_SENT_LADJ);
        const int wlo = klo >> 5, whi = (khi >> 5) + 1;
        for (int w0 = wlo; w0 < whi; w0 += kWave) {
          const int i = w0 + lane;
          uint32_t word = 0;
          if (i < whi) { word = vscr[i]; if (word) vscr[i] = 0; }
          uint64_t nz = __ballot(word != 0);
          while (nz) {
            const int L = __builtin_ctzll(nz);
            nz &= nz - 1;
            const uint32_t wd = (uint32_t)__builtin_amdgcn_readlane((int)word, L);
            const int m = __popc(wd);
            reserve(per * m);
            if (lane < 32 && ((wd >> lane) & 1u)) {
              const int kk = (w0 + L) * 32 + lane;
              const int q = pos - wbase + per * __popc(wd & ((1u << lane) - 1u));
              if (TY) {
                const unsigned kx = (unsigned)aload(key + kk);
                astore(key + kk, -1);
                const int ty = kx == 0xFFFFFFFFu ? 0 : (int)a.g.eattr[e0 + (int)(kx & 0x7FFFFFFFu)];
                win[q] = edge_off + ty;
                win[q + 1] = idx_off + kk;
              } else {
                win[q] = idx_off + kk;
              }
            }
            pos += per * m;
          }
        }
        emit1(GTOK_SENT_RADJ);
      }
      ++nvis;
      slice_sync();
    };

    emit1(GTOK_SENT_SOS);
    if (n > 0) {
      cur = (int)below((uint32_t)n);
      visit(cur, -1, 0);
      while (pos < lim) {
        {   // extend the trail over an uncovered edge: the below(cnt)-th unvisited neighbour in ascending node id
          int lo = 0x7FFFFFFF, hi = -1;
          for_entries(cur, [&](bool valid, int w, int, int) {
            if (valid && w != cur && vidx[w] == 0xFFFF) {
              atomicOr(scr + (w >> 5), 1u << (w & 31));
              lo = min(lo, w); hi = max(hi, w);
            }
          });
          lo = uni(wave_min(lo)); hi = uni(wave_max(hi));
          wave_sync();
          if (hi >= 0) {
            const int wlo = lo >> 5, whi = (hi >> 5) + 1;
            int c = 0;
            for (int i = wlo + lane; i < whi; i += kWave) c += __popc(scr[i]);
            c = uni(wave_sum(c));
            const int nxt = select_kth([&](int i) { return scr[i]; }, wlo, whi, (int)below((uint32_t)c));
            for (int i = wlo + lane; i < whi; i += kWave) scr[i] = 0;
            wave_sync();
            if ((unsigned)nxt >= (unsigned)n) break;     // (never: c counts the very set the pick selects from)
            int et = 0;
            if (TY) {   // first listed cur -> nxt, else first listed nxt -> cur
              unsigned kx = 0xFFFFFFFFu;
              for_entries(cur, [&](bool valid, int w, int dir, int p) {
                if (valid && w == nxt) kx = min(kx, ((unsigned)dir << 31) | (unsigned)p);
              });
              kx = wave_umin(kx);
              et = edge_off + (kx == 0xFFFFFFFFu ? 0 : (int)a.g.eattr[e0 + (int)(kx & 0x7FFFFFFFu)]);
            }
            visit(nxt, cur, et);
            cur = nxt;
            continue;
          }
          // a dead end.  (cur is not live then; where a batch flagged wrongly left it so, it is retired here - no node is
          // picked twice without a visit in between, so the walk ends whatever the input)
          int was = 0;
          if (is0 && (live[cur >> 5] >> (cur & 31) & 1u)) { live[cur >> 5] &= ~(1u << (cur & 31)); was = 1; }
          nlive -= uni(was);
          wave_sync();
        }
        if (nlive > 0) {   // restart from a visited node that still owns uncovered edges, ascending node id
          const int c = select_kth([&](int i) { return live[i]; }, 0, nwn, (int)below((uint32_t)nlive));
          if ((unsigned)c >= (unsigned)n) { nlive = 0; continue; }
          cur = c;
          reserve(2);
          if (lane < 2) win[pos - wbase + lane] = lane == 0 ? GTOK_SENT_RESET : idx_off + (int)vidx[cur];
          pos += 2;
          continue;
        }
        if (nvis < n) {   // another component or an isolated node: the below(left)-th unvisited node
          const int c = select_kth([&](int i) { return ~vis[i] & ((i + 1) * 32 <= n ? ~0u : ((1u << (n & 31)) - 1u)); }, 0, nwn,
                                   (int)below((uint32_t)(n - nvis)));
          if ((unsigned)c >= (unsigned)n) break;
          cur = c;
          emit1(GTOK_SENT_RESET);
          visit(cur, -1, 0);
          continue;
        }
        break;
      }
    }
    emit1(GTOK_SENT_EOS);
    flush();

    if (ORD) {   // the visit order: the wave's table as it stands, 0xFFFF (never visited) widened to -1; nodes the batch's max_nodes
                 // clamped away were never visited either.  Coalesced 32-bit vector stores inside the graph's own slice of the epoch's block.
      wave_sync();
      int32_t *ord = a.visit_index + (int64_t)(gv / G) * a.order_stride + nb0;
      const int nout = nb0 < 0 ? 0 : (int)max((int64_t)0, min((int64_t)nfull, a.order_stride - nb0));
      for (int i = lane; i < nout; i += kWave) {
        const int k = i < n ? (int)vidx[i] : 0xFFFF;
        ord[i] = k == 0xFFFF ? -1 : k;
      }
    }
    if (!TOK) continue;

    // ---- row end: query ids (original node ids, not remapped), pad tail, true length
    const int ltrail = min(pos, lim);
    int len = ltrail;
    if (a.p.query) {   // trainer/train_agtt.py:257-267
      if (lane < 3 && ltrail + lane < a.ld) {
        const int t = idx_off + (lane == 0 ? nfull : a.p.query[2 * (int64_t)g + lane - 1]);
        if (u16) row16[ltrail + lane] = (uint16_t)t; else row32[ltrail + lane] = t;
      }
      len = ltrail + 3;
    }
    if (!(a.p.flags & GTOK_SENT_NO_PAD)) {
      for (int i = min(len, a.ld) + lane; i < a.ld; i += kWave) {
        if (u16) row16[i] = (uint16_t)a.p.pad_id; else row32[i] = a.p.pad_id;
      }
    }
    if (is0) a.out_len[gv] = len;
  }
}

static inline int64_t up16(int64_t v) { return (v + 15) / 16 * 16; }

// the slice of one wave: cnt[n], key[n], inptr[n + 1], insrc[e], inpos[e]
struct LargeSlice { int64_t key, inptr, insrc, inpos, bytes; };
static LargeSlice large_slice(int maxn, int maxe) {
  LargeSlice s;
  int64_t off = up16(4 * (int64_t)maxn);
  s.key = off; off += up16(4 * (int64_t)maxn);
  s.inptr = off; off += up16(4 * ((int64_t)maxn + 1));
  s.insrc = off; off += up16(4 * (int64_t)maxe);
  s.inpos = off; off += up16(4 * (int64_t)maxe);
  s.bytes = off;
  return s;
}

}  // namespace gtok

using namespace gtok;

extern "C" int64_t gtok_sent_large_workspace(int32_t max_nodes, int32_t max_edges, int64_t walks) {
  if (max_nodes < 0 || max_edges < 0 || walks < 0) return GTOK_E_INVAL;
  if (max_nodes > GTOK_SENT_LARGE_MAX_NODES) return GTOK_E_TOO_LARGE;
  const int64_t waves = walks < GTOK_SENT_LARGE_WAVES ? walks : GTOK_SENT_LARGE_WAVES;
  return waves * large_slice(max_nodes > 0 ? max_nodes : 1, max_edges > 0 ? max_edges : 1).bytes;
}

// the argument rules the two entry points share (include/gtok.h); `rows`: out_ids / out_len are used.  GTOK_OK, a GTOK_E_* code,
// or 1: an empty batch, nothing to do.  Pure host arithmetic: no device is asked for anything.
static int large_check(const gtok_csr *g, const gtok_sent_params *p, bool rows, const int32_t *out_ids, int32_t ld, const int32_t *out_len,
                       const void *workspace, int64_t workspace_bytes) {
  if (!g || !p || (rows && ld <= 0) || g->num_graphs < 0 || g->max_nodes < 0 || g->max_edges < 0) return GTOK_E_INVAL;
  if (g->num_graphs == 0) return 1;   // an empty batch is a no-op
  if (rows && (!out_ids || !out_len)) return GTOK_E_INVAL;
  if (!g->node_ptr || !g->edge_ptr || !g->rowptr || (g->max_edges > 0 && !g->col)) return GTOK_E_INVAL;
  if (g->graph_ids || g->unit_ptr || g->unit_info) return GTOK_E_INVAL;      // a batch in dataset order only
  if (p->max_len < 0 || p->max_num_nodes < 0 || p->epoch_count < 0 || p->reserved != 0) return GTOK_E_INVAL;
  if (p->flags & ~(GTOK_SENT_NO_PAD | GTOK_SENT_U16)) return GTOK_E_INVAL;   // (GTOK_SENT_PACK_ONLY / _PACK_U8: gtok_sent_packed's)
  const bool u16 = rows && (p->flags & GTOK_SENT_U16) != 0;
  if (u16 && (p->pad_id < 0 || p->pad_id > 65535)) return GTOK_E_INVAL;
  const int K = p->epoch_count > 1 ? p->epoch_count : 1;
  if ((int64_t)g->num_graphs * K > 0x7FFFFFFF / 2) return GTOK_E_TOO_LARGE;  // rows of the [K, G, ld] slab are counted in 32 bits
  if (p->labeled && (!g->nattr || !g->eattr)) return GTOK_E_INVAL;
  if (g->max_nodes > GTOK_SENT_LARGE_MAX_NODES) return GTOK_E_TOO_LARGE;
  // gtok_sent's id-space rule: every id of the row must fit 16 bits
  if (u16 && (int64_t)GTOK_SENT_IDX_OFFSET + p->max_num_nodes + p->num_node_types + 512 > 65535) return GTOK_E_TOO_LARGE;
  const int64_t need = gtok_sent_large_workspace(g->max_nodes, g->max_edges, (int64_t)g->num_graphs * K);
  if (need < 0) return (int)need;
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u) || workspace_bytes < need) return GTOK_E_INVAL;
  return GTOK_OK;
}

// ord: 0 = gtok_sent_large, 1 = rows and order, 2 = order only (LargeArgs.out / ld are not used)
static int large_launch(const gtok_csr *g, const gtok_sent_params *p, int32_t *out_ids, int32_t ld, int32_t *out_len, int ord,
                        int32_t *visit_index, int64_t order_stride, void *workspace, hipStream_t stream) {
  const int K = p->epoch_count > 1 ? p->epoch_count : 1;
  const int pairs = g->num_graphs * K;
  LargeArgs a;
  a.g = *g; a.p = *p; a.out = out_ids; a.ld = ld; a.out_len = out_len;
  a.maxn = g->max_nodes; a.maxe = g->max_edges;
  const int tabn = g->max_nodes > 0 ? g->max_nodes : 1;
  const LargeSlice s = large_slice(tabn, g->max_edges > 0 ? g->max_edges : 1);
  a.ws = static_cast<unsigned char *>(workspace); a.slice = s.bytes;
  a.off_key = s.key; a.off_inptr = s.inptr; a.off_insrc = s.insrc; a.off_inpos = s.inpos;
  a.nw = ((tabn + 31) / 32 + 3) & ~3;                      // (whole 16-byte pieces: the window behind the sets stays aligned)
  a.pairs = pairs;
  a.visit_index = visit_index; a.order_stride = order_stride;
  // LDS by the batch's max_nodes: four sets, the window, 16 bits per node - 43 KB at 16,384 nodes (three waves per CU)
  const size_t lds = (size_t)4 * a.nw * 4 + (size_t)kLargeWin * 4 + (((size_t)tabn * 2 + 15) & ~(size_t)15);
  const int nb = pairs < GTOK_SENT_LARGE_WAVES ? pairs : GTOK_SENT_LARGE_WAVES;
  typedef void (*Kern)(const LargeArgs);
  const bool lab = p->labeled != 0;
  const Kern kern = ord == 0 ? (lab ? (Kern)sent_large_kernel<true> : (Kern)sent_large_kernel<false>)
                  : ord == 1 ? (lab ? (Kern)sent_large_kernel<true, 1> : (Kern)sent_large_kernel<false, 1>)
                             : (lab ? (Kern)sent_large_kernel<true, 2> : (Kern)sent_large_kernel<false, 2>);
  hipLaunchKernelGGL(kern, dim3(nb), dim3(64), lds, stream, a);
  return hipGetLastError() == hipSuccess ? GTOK_OK : GTOK_E_LAUNCH;
}

extern "C" int gtok_sent_large(const gtok_csr *g, const gtok_sent_params *p, int32_t *out_ids, int32_t ld, int32_t *out_len,
                               void *workspace, int64_t workspace_bytes, void *stream) {
  gtok::DeviceScope device_scope((hipStream_t)stream);   // the stream's device, not the thread's current one
  if (!device_scope.ok()) return GTOK_E_NO_DEVICE;
  const int c = large_check(g, p, true, out_ids, ld, out_len, workspace, workspace_bytes);
  if (c) return c < 0 ? c : GTOK_OK;
  return large_launch(g, p, out_ids, ld, out_len, 0, nullptr, 0, workspace, (hipStream_t)stream);
}

extern "C" int gtok_sent_large_order(const gtok_csr *g, const gtok_sent_params *p, int32_t *out_ids, int32_t ld, int32_t *out_len,
                                     int32_t *visit_index, int64_t order_stride, void *workspace, int64_t workspace_bytes, void *stream) {
  // every argument error before any device is asked for
  if ((out_ids == nullptr) != (out_len == nullptr)) return GTOK_E_INVAL;
  const bool rows = out_ids != nullptr;
  if (!visit_index || order_stride < 0) return GTOK_E_INVAL;
  const int c = large_check(g, p, rows, out_ids, ld, out_len, workspace, workspace_bytes);
  if (c) return c < 0 ? c : GTOK_OK;
  gtok::DeviceScope device_scope((hipStream_t)stream);
  if (!device_scope.ok()) return GTOK_E_NO_DEVICE;
  if (rows) return large_launch(g, p, out_ids, ld, out_len, 1, visit_index, order_stride, workspace, (hipStream_t)stream);
  gtok_sent_params q = *p;              // order only: nothing of a row is written, whatever the row flags say
  q.flags = GTOK_SENT_NO_PAD; q.query = nullptr;
  return large_launch(g, &q, nullptr, 0, nullptr, 2, visit_index, order_stride, workspace, (hipStream_t)stream);
}
