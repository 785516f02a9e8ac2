// gtok_csr_relabel.hip — a batched CSR renumbered through a per-graph node map (include/gtok.h: gtok_csr_relabel), gfx950.
//
// One wave per graph, in the style of the two decode kernels (gtok_sent_decode.hip, gtok_ibtt_decode.hip).  Per wave, in LDS:
//   tab   old node -> new node, 16 bits per node of the batch's max_nodes (0xFFFF: not named by the map)
//   set   one bit per node of max(max_nodes, target_max_nodes): first the old nodes the map has named (the bijection is checked on
//         it: a bit found set is a second naming, and the named nodes must count N_old), then - per long row - the row's new columns
//   pre   per 32-bit word of `set`, the number of members below it (a long row's ranks: pre[word] + the popcount below the bit)
// Everything the caller's arrays claim is checked before it is used as an index: the slices against the pointer arrays' totals and
// the host-known bounds, the row pointers (from 0 to E_g, never decreasing), every column, the map.  A graph that fails is skipped.
// Rows are built in NEW order, 64 target nodes per step: their old rows' degrees are scanned into the new row starts (coalesced
// stores of rowptr and nattr), then every non-empty row is put in column order by the whole wave:
//   up to 64 entries  a lane per entry; its rank is the number of entries (new column, input position) below its own, counted with
//                     one v_readlane per entry of the row - stable, duplicates and all
//   longer rows       the new columns are dropped into `set`; without a duplicate the rank of a column is the number of members
//                     below it (a scan of the words the row touched); with one, the stable count above, entries read back from memory
// so a simple graph costs O(N + E) lane steps plus, per long row, the words between its smallest and largest new column (at most
// N / 32, eight wave steps at 16,384 nodes); only a long row that holds duplicates pays d steps per 64 entries.
#include "gtok_common.hpp"
#include "gtok_csr_relabel_args.hpp"

namespace {
using namespace gtok;

struct RelabelArgs {
  gtok_csr g;
  const int32_t *tptr;        // the target's node_ptr
  const int32_t *oon;         // old_of_new
  gtok_csr_built out;
  int32_t *status;
  unsigned long long *groups; // [ceil(G / 64)][2]: summed target nodes, entries of the built graphs
  int maxn_t;                 // target_max_nodes
  int stride, off_set, off_pre, nw;   // LDS bytes per wave, offsets of set / pre, words of set
  int units, upb;
};

__global__ void __launch_bounds__(256) csr_relabel_kernel(const RelabelArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id();
  const int wave = wave_id(), wpb = (int)(blockDim.x >> 6);
  unsigned char *mine = smem + (size_t)wave * a.stride;
  uint16_t *tab = reinterpret_cast<uint16_t *>(mine);
  uint32_t *set = reinterpret_cast<uint32_t *>(mine + a.off_set);
  int *pre = reinterpret_cast<int *>(mine + a.off_pre);
  const int G = a.g.num_graphs;
  const int ntot = sload(a.g.node_ptr, G), ttot = sload(a.tptr, G);
  const int64_t etot = sload(a.g.edge_ptr, G);
  const bool has_n = a.g.nattr != nullptr, has_e = a.g.eattr != nullptr;
  int skipped = 0, nonsimple = 0, max_deg = 0, max_n = 0, max_e = 0;
  const int vb = virtual_block();
  const int u0 = vb * a.upb, u1 = min(a.units, u0 + a.upb);
  for (int unit = u0; unit < u1; ++unit) {
    const int r = unit * wpb + wave;
    if (r >= G) break;
    const int nb = sload(a.g.node_ptr, r), ne = sload(a.g.node_ptr, r + 1);
    const int tb = sload(a.tptr, r), te = sload(a.tptr, r + 1);
    const int64_t e0 = sload(a.g.edge_ptr, r), e1 = sload(a.g.edge_ptr, r + 1);
    // slices that lie inside the arrays the pointer arrays describe and inside the host-known bounds the LDS tables are sized by
    bool ok = nb >= 0 && ne >= nb && ne <= ntot && ne - nb <= a.g.max_nodes && tb >= 0 && te >= tb && te <= ttot && te - tb <= a.maxn_t &&
              ne - nb <= te - tb && e0 >= 0 && e1 >= e0 && e1 <= etot && e1 - e0 <= (int64_t)a.g.max_edges;
    const int n = ok ? ne - nb : 0, nt = ok ? te - tb : 0, e = ok ? (int)(e1 - e0) : 0;
    const int32_t *rp = a.g.rowptr + nb + r;          // (only dereferenced below an index < n + 1, n > 0 only when the slice is ok)
    const int32_t *colg = a.g.col + e0;
    const int32_t *oon = a.oon + tb;
    int bad = 0;
    if (ok) {
      // ---- the map: every old node named exactly once
      wave_sync();
      for (int i = lane; i < a.nw; i += kWave) set[i] = 0;
      for (int i = lane; i < n; i += kWave) tab[i] = 0xFFFFu;
      wave_sync();
      int named = 0;
      for (int t = lane; t < nt; t += kWave) {
        const int o = oon[t];
        if ((unsigned)o < (unsigned)n) {
          const uint32_t bit = 1u << (o & 31);
          if (atomicOr(set + (o >> 5), bit) & bit) bad = 1;     // named twice
          tab[o] = (uint16_t)t;
          ++named;
        }
      }
      named = uni(wave_sum(named));
      if (named != n) bad = 1;
      wave_sync();
      for (int i = lane; i < ((n + 31) >> 5); i += kWave) set[i] = 0;
      // ---- the old graph: row pointers from 0 to E_g that never decrease, columns inside [0, N_old)
      for (int i = lane; i < n; i += kWave) {
        const int x = rp[i], y = rp[i + 1];
        if (x < 0 || y < x || y > e) bad = 1;
      }
      if (lane == 0) {
        if (n > 0 ? (rp[0] != 0 || rp[n] != e) : e != 0) bad = 1;
      }
      bad = __ballot(bad != 0) != 0 ? 1 : 0;
      if (!bad) {     // (the columns only under row pointers that were found sound: e is what they sum to)
        for (int k = lane; k < e; k += kWave)
          if ((unsigned)colg[k] >= (unsigned)n) bad = 1;
        bad = __ballot(bad != 0) != 0 ? 1 : 0;
      }
      wave_sync();
    }
    if (!ok || bad) {
      ++skipped;
      if (lane == 0) a.status[r] = 1;
      continue;
    }

    int32_t *orow = a.out.rowptr + tb + r;
    int32_t *ocol = a.out.col + e0, *oord = a.out.eorder + e0;
    uint8_t *oea = has_e ? a.out.eattr + e0 : nullptr;
    const uint8_t *iea = has_e ? a.g.eattr + e0 : nullptr;
    int flag = 0, dmax = 0, run = 0;       // flag: a duplicate or a self loop was met (per lane until the end)
    for (int t0 = 0; t0 < nt; t0 += kWave) {
      // ---- 64 target nodes: their old rows, the scan of the degrees, row pointers and node types
      const int t = t0 + lane;
      int o = -1, rs = 0, d = 0;
      if (t < nt) {
        o = oon[t];
        if ((unsigned)o < (unsigned)n) { rs = rp[o]; d = rp[o + 1] - rs; } else o = -1;
      }
      const int incl = wave_incl_scan(d);
      const int start = run + incl - d;
      if (t < nt) {
        orow[t] = start;
        if (has_n) a.out.nattr[tb + t] = o >= 0 ? a.g.nattr[nb + o] : (uint8_t)255;
      }
      run += __builtin_amdgcn_readlane(incl, kWave - 1);
      dmax = max(dmax, d);
      // ---- the non-empty rows of the 64, one after another, the whole wave on each
      uint64_t todo = __ballot(d > 0);
      while (todo) {
        const int L = (int)__builtin_ctzll(todo);
        todo &= todo - 1;
        const int u = __builtin_amdgcn_readlane(o, L), urs = __builtin_amdgcn_readlane(rs, L);
        const int ud = __builtin_amdgcn_readlane(d, L), ust = __builtin_amdgcn_readlane(start, L);
        auto put = [&](int k, int cn, int rank) {       // entry k of the old row (0-based inside it) to its slot
          const int slot = ust + rank;
          if ((unsigned)slot < (unsigned)e) {
            ocol[slot] = cn;
            oord[slot] = urs + k;
            if (has_e) oea[slot] = iea[urs + k];
          }
        };
        if (ud <= kWave) {
          int c = -1, cn = 0x7FFFFFFF;
          if (lane < ud) { c = colg[urs + lane]; cn = (int)tab[c]; }
          if (c == u) flag = 1;
          int rank = 0;
          for (int j = 0; j < ud; ++j) {
            const int x = __builtin_amdgcn_readlane(cn, j);
            rank += (x < cn || (x == cn && j < lane)) ? 1 : 0;
            if (x == cn && j != lane) flag = 1;
          }
          if (lane < ud) put(lane, cn, rank);
          continue;
        }
        // a long row: its new columns into the set
        int dup = 0, lo = 0x7FFFFFFF, hi = -1;
        for (int k = lane; k < ud; k += kWave) {
          const int c = colg[urs + k];
          const int cn = (int)tab[c];
          if (c == u) flag = 1;
          const uint32_t bit = 1u << (cn & 31);
          if (atomicOr(set + (cn >> 5), bit) & bit) dup = 1;
          lo = min(lo, cn >> 5); hi = max(hi, cn >> 5);
        }
        dup = __ballot(dup != 0) != 0 ? 1 : 0;
        lo = uni(wave_min(lo)); hi = uni(wave_max(hi));
        wave_sync();
        if (!dup) {
          int carry = 0;
          for (int w0 = lo; w0 <= hi; w0 += kWave) {
            const int w = w0 + lane;
            const int c = w <= hi ? __popc(set[w]) : 0;
            const int in = wave_incl_scan(c);
            if (w <= hi) pre[w] = carry + in - c;
            carry += __builtin_amdgcn_readlane(in, kWave - 1);
          }
          wave_sync();
          for (int k = lane; k < ud; k += kWave) {
            const int cn = (int)tab[colg[urs + k]];
            put(k, cn, pre[cn >> 5] + __popc(set[cn >> 5] & ((1u << (cn & 31)) - 1u)));
          }
        } else {
          flag = 1;
          for (int k0 = 0; k0 < ud; k0 += kWave) {    // the stable count, every entry of the row against the lane's own
            const int k = k0 + lane;
            const int cn = k < ud ? (int)tab[colg[urs + k]] : 0x7FFFFFFF;
            int rank = 0;
            for (int j = 0; j < ud; ++j) {
              const int x = (int)tab[colg[urs + j]];
              rank += (x < cn || (x == cn && j < k)) ? 1 : 0;
            }
            if (k < ud) put(k, cn, rank);
          }
        }
        wave_sync();
        for (int w = lo + lane; w <= hi; w += kWave) set[w] = 0;
        wave_sync();
      }
    }
    flag = __ballot(flag != 0) != 0 ? 1 : 0;
    if (lane == 0) {
      orow[nt] = e;
      a.status[r] = flag ? 2 : 0;
      atomicAdd(a.groups + 2 * (size_t)(r >> 6), (unsigned long long)nt);
      atomicAdd(a.groups + 2 * (size_t)(r >> 6) + 1, (unsigned long long)e);
    }
    nonsimple += flag;
    max_deg = max(max_deg, uni(wave_max(dmax))); max_n = max(max_n, nt); max_e = max(max_e, e);
  }
  if (lane == 0) {
    int32_t *info = a.out.info;
    if (skipped) atomicAdd(info + 0, skipped);
    info_max(info + 1, max_deg); info_max(info + 2, max_n); info_max(info + 3, max_e);
    if (nonsimple) atomicAdd(info + 6, nonsimple);
  }
}

// info[4] / info[5]: the largest group sums, behind the build on the same stream
__global__ void __launch_bounds__(64) csr_relabel_chunks_kernel(const unsigned long long *groups, int ngroups, int32_t *info) {
  const int lane = lane_id();
  int cn = 0, ce = 0;
  for (int i = lane; i < ngroups; i += kWave) {
    const unsigned long long x = groups[2 * (size_t)i], y = groups[2 * (size_t)i + 1];
    cn = max(cn, (int)(x < 0x7FFFFFFFull ? x : 0x7FFFFFFFull));
    ce = max(ce, (int)(y < 0x7FFFFFFFull ? y : 0x7FFFFFFFull));
  }
  cn = uni(wave_max(cn)); ce = uni(wave_max(ce));
  if (lane == 0) { info[4] = cn; info[5] = ce; }
}

}  // namespace

extern "C" int64_t gtok_csr_relabel_workspace(int32_t num_graphs, int64_t num_entries) {
  return gtok::csr_relabel_workspace_bytes(num_graphs, num_entries);
}

extern "C" int gtok_csr_relabel(const gtok_csr *g, const int32_t *target_node_ptr, int32_t target_max_nodes, const int32_t *old_of_new,
                                const gtok_csr_built *out, int32_t *status, void *workspace, int64_t workspace_bytes, void *stream) {
  const int c = gtok::csr_relabel_check(g, target_node_ptr, target_max_nodes, old_of_new, out, status, workspace, workspace_bytes);
  if (c) return c < 0 ? c : GTOK_OK;
  gtok::DeviceScope device_scope((hipStream_t)stream);   // the stream's device, not the thread's current one
  if (!device_scope.ok()) return GTOK_E_NO_DEVICE;
  hipStream_t s = (hipStream_t)stream;
  const int G = g->num_graphs, ngroups = (G + 63) / 64;
  if (hipMemsetAsync(out->info, 0, 8 * sizeof(int32_t), s) != hipSuccess) return GTOK_E_LAUNCH;
  if (hipMemsetAsync(workspace, 0, (size_t)ngroups * 16, s) != hipSuccess) return GTOK_E_LAUNCH;
  RelabelArgs a;
  a.g = *g; a.tptr = target_node_ptr ? target_node_ptr : g->node_ptr; a.oon = old_of_new; a.out = *out; a.status = status;
  a.groups = static_cast<unsigned long long *>(workspace);
  a.maxn_t = target_max_nodes;
  const int setn = g->max_nodes > target_max_nodes ? g->max_nodes : target_max_nodes;
  a.nw = ((setn > 0 ? setn : 1) + 31) / 32;
  a.off_set = align_up((g->max_nodes > 0 ? g->max_nodes : 1) * 2, 16);
  a.off_pre = a.off_set + align_up(a.nw * 4, 16);
  a.stride = a.off_pre + align_up(a.nw * 4, 16);     // 36 KB at 16,384 nodes: inside kLdsWithoutOptIn, one wave per workgroup
  const int rc = launch_wave_per_item(csr_relabel_kernel, a, G, 4, a.stride, device_scope.dev, s);
  if (rc != GTOK_OK) return rc;
  hipLaunchKernelGGL(csr_relabel_chunks_kernel, dim3(1), dim3(64), 0, s, (const unsigned long long *)a.groups, ngroups, out->info);
  return hipGetLastError() == hipSuccess ? GTOK_OK : GTOK_E_LAUNCH;
}
