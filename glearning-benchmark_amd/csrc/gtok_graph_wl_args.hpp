// gtok_graph_wl_args.hpp - the host-side argument checks, the kernel choice and the LDS / workspace arithmetic of gtok_graph_wl, in a
// header of their own (no HIP in it) so that a plain C++ program can exercise them under the host sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>

#include "gtok.h"
#include "gtok_graph_tasks_args.hpp"

namespace gtok {

// The kernels (include/gtok.h, gtok_graph_wl), with gtok_graph_tasks' size classes.  Structure-only keys of any listing: closure rows
// in registers (<= 64 nodes), the bit matrix in LDS (<= 512 nodes).  A pull over the CSR rows for GTOK_CSR_SIMPLE_SYMMETRIC batches of
// any size, which is also the only path of GTOK_WL_ATTRS.
enum GraphWlPath { kWlReg = 0, kWlLds = 1, kWlCsr = 2 };
constexpr int32_t kWlKnownFlags = GTOK_WL_ATTRS;
constexpr int kWlCsrLdsMaxNodes = 4096;      // the csr path keeps its two tables in LDS up to here, in the caller's workspace beyond

// GTOK_WL_KERNEL=reg|lds|csr (a test hook): -1 when unset, empty or anything else
inline int graph_wl_forced(const char *env) {
  if (!env) return -1;
  if (!strcmp(env, "reg")) return kWlReg;
  if (!strcmp(env, "lds")) return kWlLds;
  if (!strcmp(env, "csr")) return kWlCsr;
  return -1;
}

// The path a batch takes: by max_nodes (csr with GTOK_WL_ATTRS), or the forced one where it can hold the batch - a forced path that
// cannot (graphs beyond its node limit, attributes on reg / lds, csr on an unflagged batch) is GTOK_E_UNSUPPORTED, never a quiet
// change of path.  rounds == 0 runs N_g rounds and stops at 512 nodes.
inline int graph_wl_path(int32_t max_nodes, int32_t csr_flags, int32_t flags, int32_t rounds, int forced) {
  if (max_nodes < 0 || (flags & ~kWlKnownFlags) || rounds < 0 || rounds > GTOK_WL_MAX_ROUNDS) return GTOK_E_INVAL;
  if (max_nodes > GTOK_SENT_LARGE_MAX_NODES) return GTOK_E_TOO_LARGE;
  const bool sym = (csr_flags & GTOK_CSR_SIMPLE_SYMMETRIC) != 0, attrs = (flags & GTOK_WL_ATTRS) != 0;
  int path = attrs ? kWlCsr : max_nodes <= kTasksRegMaxNodes ? kWlReg : max_nodes <= kTasksLdsMaxNodes ? kWlLds : kWlCsr;
  if (forced >= 0) {
    if (forced < path) return GTOK_E_UNSUPPORTED;
    path = forced;
  }
  if (path == kWlCsr && !sym) return GTOK_E_UNSUPPORTED;
  if (rounds == 0 && max_nodes > kTasksLdsMaxNodes) return GTOK_E_UNSUPPORTED;
  return path;
}

// LDS bytes one wave needs on `path` (a multiple of 16).  reg: 64 closure rows and 64 terms.  lds: W words for every node,
// word-major, and a term for every node (36 KB at 512 nodes).  csr: two 8-byte tables up to kWlCsrLdsMaxNodes nodes (64 KB there),
// nothing beyond (the tables are in the workspace).
inline int graph_wl_lds_bytes(int path, int32_t max_nodes) {
  const int n = max_nodes > 0 ? max_nodes : 1;
  if (path == kWlReg) return 2 * 64 * 8;
  if (path == kWlLds) return ((graph_tasks_lds_words(max_nodes) + 1) * n * 8 + 15) / 16 * 16;
  return max_nodes <= kWlCsrLdsMaxNodes ? 16 * n : 0;
}

// waves of the launch whose tables are in the workspace: wave w takes graphs w, w + waves, ...
inline int graph_wl_waves(int32_t num_graphs) { return num_graphs < GTOK_WL_LARGE_WAVES ? num_graphs : GTOK_WL_LARGE_WAVES; }

// gtok_graph_wl_workspace: 0 up to kWlCsrLdsMaxNodes nodes, else 16 bytes per node of max_nodes for every wave
inline int64_t graph_wl_workspace(int32_t max_nodes, int32_t num_graphs) {
  if (max_nodes < 0 || num_graphs < 0) return GTOK_E_INVAL;
  if (max_nodes > GTOK_SENT_LARGE_MAX_NODES) return GTOK_E_TOO_LARGE;
  if (max_nodes <= kWlCsrLdsMaxNodes) return 0;
  return (int64_t)graph_wl_waves(num_graphs) * 16 * max_nodes;
}

// Nothing is launched or written before this passes.  Returns a GTOK_E_* code, the path (>= 0) offset by 16, or 1: nothing to do
// (no graphs).
constexpr int kWlPathBase = 16;
inline int graph_wl_check(const gtok_csr *g, const int32_t *labels, int32_t rounds, int32_t flags, const uint64_t *keys,
                          const uint64_t *node_colors, const int32_t *info, const void *workspace, int64_t workspace_bytes, int forced) {
  (void)labels; (void)node_colors;                                            // NULL = no labels / no colours asked for
  if (!g || g->num_graphs < 0 || g->max_nodes < 0 || g->max_edges < 0 || workspace_bytes < 0) return GTOK_E_INVAL;
  if (g->graph_ids || g->unit_ptr || g->unit_info) return GTOK_E_INVAL;       // a batch in dataset order only
  if (flags & ~kWlKnownFlags) return GTOK_E_INVAL;
  if (rounds < 0 || rounds > GTOK_WL_MAX_ROUNDS) return GTOK_E_INVAL;
  if (!info) return GTOK_E_INVAL;
  if (g->max_nodes > GTOK_SENT_LARGE_MAX_NODES) return GTOK_E_TOO_LARGE;
  if (g->num_graphs == 0) return 1;
  if (!keys) return GTOK_E_INVAL;
  if (!g->node_ptr || !g->edge_ptr || !g->rowptr || (g->max_edges > 0 && !g->col)) return GTOK_E_INVAL;
  if ((flags & GTOK_WL_ATTRS) && ((g->max_nodes > 0 && !g->nattr) || (g->max_edges > 0 && !g->eattr))) return GTOK_E_INVAL;
  const int path = graph_wl_path(g->max_nodes, g->flags, flags, rounds, forced);
  if (path < 0) return path;
  if (path == kWlCsr) {
    const int64_t need = graph_wl_workspace(g->max_nodes, g->num_graphs);
    if (need > 0 && (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u) || workspace_bytes < need)) return GTOK_E_INVAL;
  }
  return kWlPathBase + path;
}

}  // namespace gtok
