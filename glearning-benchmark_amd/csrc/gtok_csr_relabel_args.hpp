// gtok_csr_relabel_args.hpp - the host-side argument checks and workspace arithmetic of gtok_csr_relabel, in a header of their
// own (no HIP in it) so that a plain C++ program can exercise them under the host sanitizers.
#pragma once
#include <stdint.h>

#include "gtok.h"

namespace gtok {

// The workspace holds, per aligned group of 64 graphs, the summed target node counts and entry counts of the graphs that were
// built (two 64-bit sums: info[4] / info[5] are their maxima).  num_entries is part of the signature for builds that keep
// per-entry temporaries; this one keeps none.  A multiple of 16, 0 for an empty batch; GTOK_E_INVAL for a negative argument.
inline int64_t csr_relabel_workspace_bytes(int32_t num_graphs, int64_t num_entries) {
  if (num_graphs < 0 || num_entries < 0) return GTOK_E_INVAL;
  const int64_t groups = ((int64_t)num_graphs + 63) / 64;
  return groups * 16;
}

// Nothing is launched or written before this passes.  Returns a GTOK_E_* code, GTOK_OK, or 1: no graphs, nothing to do.
inline int csr_relabel_check(const gtok_csr *g, const int32_t *target_node_ptr, int32_t target_max_nodes, const int32_t *old_of_new,
                             const gtok_csr_built *out, const int32_t *status, const void *workspace, int64_t workspace_bytes) {
  (void)target_node_ptr;                      // NULL = g->node_ptr
  if (!g || g->num_graphs < 0 || g->max_nodes < 0 || g->max_edges < 0 || target_max_nodes < 0 || workspace_bytes < 0) return GTOK_E_INVAL;
  if (g->graph_ids || g->unit_ptr || g->unit_info) return GTOK_E_INVAL;      // a batch in dataset order only
  if (g->max_nodes > GTOK_SENT_LARGE_MAX_NODES || target_max_nodes > GTOK_SENT_LARGE_MAX_NODES) return GTOK_E_TOO_LARGE;
  if (g->num_graphs == 0) return 1;
  if (!g->node_ptr || !g->edge_ptr || !g->rowptr || (g->max_edges > 0 && !g->col)) return GTOK_E_INVAL;
  if (!old_of_new || !status) return GTOK_E_INVAL;
  if (!out || !out->rowptr || !out->col || !out->eorder || !out->info) return GTOK_E_INVAL;
  if ((g->nattr && !out->nattr) || (g->eattr && !out->eattr)) return GTOK_E_INVAL;
  const int64_t need = csr_relabel_workspace_bytes(g->num_graphs, 0);
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u) || workspace_bytes < need) return GTOK_E_INVAL;
  return GTOK_OK;
}

}  // namespace gtok
