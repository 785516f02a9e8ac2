// gtok_graph_tasks_args.hpp - the host-side argument checks and the kernel choice of gtok_graph_tasks, in a header of their own
// (no HIP in it) so that a plain C++ program can exercise them under the host sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>

#include "gtok.h"

namespace gtok {

// The three searches (include/gtok.h, gtok_graph_tasks): closure rows in registers (<= 64 nodes), a bit matrix in LDS (<= 512
// nodes), a push search over the CSR (<= GTOK_SENT_LARGE_MAX_NODES nodes, GTOK_CSR_SIMPLE_SYMMETRIC batches only).
enum GraphTasksPath { kTasksReg = 0, kTasksLds = 1, kTasksCsr = 2 };
constexpr int kTasksRegMaxNodes = 64, kTasksLdsMaxNodes = 512;

// GTOK_TASKS_KERNEL=reg|lds|csr (a test hook): -1 when unset, empty or anything else
inline int graph_tasks_forced(const char *env) {
  if (!env) return -1;
  if (!strcmp(env, "reg")) return kTasksReg;
  if (!strcmp(env, "lds")) return kTasksLds;
  if (!strcmp(env, "csr")) return kTasksCsr;
  return -1;
}

// The path a batch takes: by max_nodes, or the forced one where it can hold the batch (a forced path that cannot - graphs beyond its
// node limit, the CSR search on an unflagged batch - is GTOK_E_UNSUPPORTED, never a quiet change of path).
inline int graph_tasks_path(int32_t max_nodes, int32_t flags, int forced) {
  if (max_nodes < 0) return GTOK_E_INVAL;
  if (max_nodes > GTOK_SENT_LARGE_MAX_NODES) return GTOK_E_TOO_LARGE;
  const bool sym = (flags & GTOK_CSR_SIMPLE_SYMMETRIC) != 0;
  int path = max_nodes <= kTasksRegMaxNodes ? kTasksReg : max_nodes <= kTasksLdsMaxNodes ? kTasksLds : kTasksCsr;
  if (forced >= 0) {
    if (forced < path) return GTOK_E_UNSUPPORTED;
    path = forced;
  }
  if (path == kTasksCsr && !sym) return GTOK_E_UNSUPPORTED;
  return path;
}

// 64-bit words of a bit-matrix row on the LDS path: 2, 4 or 8
inline int graph_tasks_lds_words(int32_t max_nodes) { return max_nodes <= 128 ? 2 : max_nodes <= 256 ? 4 : 8; }

// LDS bytes one wave needs on `path` (a multiple of 16).  reg: 64 closure rows.  lds: W words for every node, word-major.
// csr: a visited bit per node, a 16-bit distance and a 16-bit FIFO slot per node (66 KB at 16,384 nodes: one wave per workgroup).
inline int graph_tasks_lds_bytes(int path, int32_t max_nodes) {
  const int n = max_nodes > 0 ? max_nodes : 1;
  const auto up16 = [](int v) { return (v + 15) / 16 * 16; };
  if (path == kTasksReg) return 64 * 8;
  if (path == kTasksLds) return up16(graph_tasks_lds_words(max_nodes) * n * 8);
  return up16((n + 31) / 32 * 4) + 2 * up16(n * 2);
}

// Nothing is launched or written before this passes.  Returns a GTOK_E_* code, the path (>= 0) offset by 16, or 1: nothing to do
// (no graphs, or no output asked for).
constexpr int kTasksPathBase = 16;
inline int graph_tasks_check(const gtok_csr *g, const int32_t *query_nodes, const int64_t *query_ptr, int64_t num_queries,
                             const int32_t *has_cycle, const int32_t *num_components, const int32_t *dist, const int32_t *info, int forced) {
  if (!g || g->num_graphs < 0 || g->max_nodes < 0 || g->max_edges < 0 || num_queries < 0) return GTOK_E_INVAL;
  if (g->graph_ids || g->unit_ptr || g->unit_info) return GTOK_E_INVAL;      // a batch in dataset order only
  if ((query_nodes != nullptr) != (dist != nullptr)) return GTOK_E_INVAL;    // dist is required iff there are queries
  if (!query_nodes && (query_ptr || num_queries != 0)) return GTOK_E_INVAL;
  if (query_nodes && !query_ptr && num_queries != (int64_t)g->num_graphs) return GTOK_E_INVAL;   // NULL = exactly one per graph
  if (g->num_graphs == 0 && num_queries != 0) return GTOK_E_INVAL;           // queries of no graph
  if (g->max_nodes > GTOK_SENT_LARGE_MAX_NODES) return GTOK_E_TOO_LARGE;
  if (!info) return GTOK_E_INVAL;
  if (g->num_graphs == 0) return 1;
  if (!has_cycle && !num_components && !query_nodes) return 1;
  if (!g->node_ptr || !g->edge_ptr || !g->rowptr || (g->max_edges > 0 && !g->col)) return GTOK_E_INVAL;
  const int path = graph_tasks_path(g->max_nodes, g->flags, forced);
  return path < 0 ? path : kTasksPathBase + path;
}

}  // namespace gtok
