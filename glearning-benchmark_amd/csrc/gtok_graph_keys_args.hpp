// gtok_graph_keys_args.hpp - the host-side argument checks and the kernel choice of gtok_graph_keys, in a header of their own
// (no HIP in it) so that a plain C++ program can exercise them under the host sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>

#include "gtok.h"
#include "gtok_graph_tasks_args.hpp"

namespace gtok {

// The kernels (include/gtok.h, gtok_graph_keys).  LISTED keys stream the CSR whatever the batch holds.  CLOSURE keys take the graph
// as gtok_graph_tasks does, with its three size classes and its LDS layouts (graph_tasks_lds_words / graph_tasks_lds_bytes): closure
// rows in registers (<= 64 nodes), the bit matrix in LDS (<= 512 nodes), and beyond that the listed stream over a
// GTOK_CSR_SIMPLE_SYMMETRIC batch, keeping the entries with u < v.
enum GraphKeysPath { kKeysListed = 0, kKeysReg = 1, kKeysLds = 2, kKeysCsr = 3 };
constexpr int32_t kKeysKnownFlags = GTOK_KEYS_CLOSURE | GTOK_KEYS_ATTRS;

// GTOK_KEYS_KERNEL=reg|lds|csr (a test hook for the closure kernels): -1 when unset, empty or anything else
inline int graph_keys_forced(const char *env) {
  if (!env) return -1;
  if (!strcmp(env, "reg")) return kKeysReg;
  if (!strcmp(env, "lds")) return kKeysLds;
  if (!strcmp(env, "csr")) return kKeysCsr;
  return -1;
}

// The path a batch takes.  LISTED: the stream, the hook ignored.  CLOSURE: by max_nodes, or the forced one where it can hold the
// batch (a forced path that cannot - graphs beyond its node limit, the stream on an unflagged batch - is GTOK_E_UNSUPPORTED, never a
// quiet change of path).
inline int graph_keys_path(int32_t max_nodes, int32_t csr_flags, int32_t flags, int forced) {
  if (max_nodes < 0 || (flags & ~kKeysKnownFlags)) return GTOK_E_INVAL;
  if ((flags & GTOK_KEYS_CLOSURE) && (flags & GTOK_KEYS_ATTRS)) return GTOK_E_INVAL;     // closure keys are structure only
  if (max_nodes > GTOK_SENT_LARGE_MAX_NODES) return GTOK_E_TOO_LARGE;
  if (!(flags & GTOK_KEYS_CLOSURE)) return kKeysListed;
  const bool sym = (csr_flags & GTOK_CSR_SIMPLE_SYMMETRIC) != 0;
  int path = max_nodes <= kTasksRegMaxNodes ? kKeysReg : max_nodes <= kTasksLdsMaxNodes ? kKeysLds : kKeysCsr;
  if (forced >= 0) {
    if (forced < path) return GTOK_E_UNSUPPORTED;
    path = forced;
  }
  if (path == kKeysCsr && !sym) return GTOK_E_UNSUPPORTED;
  return path;
}

// LDS bytes one wave needs on `path` (a multiple of 16; the streams need none)
inline int graph_keys_lds_bytes(int path, int32_t max_nodes) {
  if (path == kKeysReg) return graph_tasks_lds_bytes(kTasksReg, max_nodes);
  if (path == kKeysLds) return graph_tasks_lds_bytes(kTasksLds, max_nodes);
  return 0;
}

// Nothing is launched or written before this passes.  Returns a GTOK_E_* code, the path (>= 0) offset by 16, or 1: nothing to do
// (no graphs).
constexpr int kKeysPathBase = 16;
inline int graph_keys_check(const gtok_csr *g, const int32_t *labels, int32_t flags, const uint64_t *keys, const int32_t *info, int forced) {
  (void)labels;                                                               // NULL = no labels
  if (!g || g->num_graphs < 0 || g->max_nodes < 0 || g->max_edges < 0) return GTOK_E_INVAL;
  if (g->graph_ids || g->unit_ptr || g->unit_info) return GTOK_E_INVAL;       // a batch in dataset order only
  if (flags & ~kKeysKnownFlags) return GTOK_E_INVAL;
  if ((flags & GTOK_KEYS_CLOSURE) && (flags & GTOK_KEYS_ATTRS)) return GTOK_E_INVAL;
  if (!info) return GTOK_E_INVAL;
  if (g->max_nodes > GTOK_SENT_LARGE_MAX_NODES) return GTOK_E_TOO_LARGE;
  if (g->num_graphs == 0) return 1;
  if (!keys) return GTOK_E_INVAL;
  if (!g->node_ptr || !g->edge_ptr || !g->rowptr || (g->max_edges > 0 && !g->col)) return GTOK_E_INVAL;
  if ((flags & GTOK_KEYS_ATTRS) && ((g->max_nodes > 0 && !g->nattr) || (g->max_edges > 0 && !g->eattr))) return GTOK_E_INVAL;
  const int path = graph_keys_path(g->max_nodes, g->flags, flags, forced);
  return path < 0 ? path : kKeysPathBase + path;
}

}  // namespace gtok
