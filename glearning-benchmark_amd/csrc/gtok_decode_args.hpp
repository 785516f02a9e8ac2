// gtok_decode_args.hpp - the host-side argument checks of the row decoders (gtok_sent_decode_sizes / gtok_sent_decode_csr,
// gtok_ibtt_decode_sizes / gtok_ibtt_decode_csr, gtok_unremap_zinc and the gtok_sent_decode_zinc_* pair), in a header of their own (no HIP in it) so that a plain C++ program can
// exercise them under the host sanitizers.
#pragma once
#include <stdint.h>

#include "gtok.h"

namespace gtok {

// What both decoders ask of their rows, in the order the codes take precedence: bad scalars (`scalars_ok`: the caller's own as
// well), a node bound the kernels have no counters for, no rows (1: nothing to do), a missing array (`arrays_ok`: likewise).
inline int decode_check_rows(bool scalars_ok, bool arrays_ok, const void *ids, int32_t elem_bytes, int32_t ld, const int32_t *len,
                             int32_t num_rows, int32_t max_num_nodes) {
  if (!scalars_ok || num_rows < 0 || ld <= 0 || max_num_nodes < 0) return GTOK_E_INVAL;
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) return GTOK_E_INVAL;
  if (max_num_nodes > GTOK_SENT_LARGE_MAX_NODES) return GTOK_E_TOO_LARGE;
  if (num_rows == 0) return 1;
  if (!arrays_ok || !ids || !len) return GTOK_E_INVAL;
  return GTOK_OK;
}

// the outputs pass 2 needs (`typed` rows: the two type arrays as well)
inline int decode_check_out(const gtok_csr_built *out, bool typed) {
  if (!out || !out->node_ptr || !out->edge_ptr || !out->rowptr || !out->col || !out->eorder || !out->info) return GTOK_E_INVAL;
  if (typed && (!out->nattr || !out->eattr)) return GTOK_E_INVAL;
  return GTOK_OK;
}

// Nothing is launched or written before these pass.  Returns a GTOK_E_* code, GTOK_OK, or 1: no rows, nothing to do.
inline int sent_decode_check_rows(const void *ids, int32_t elem_bytes, int32_t ld, const int32_t *len, int32_t num_rows,
                                  int32_t max_num_nodes, int32_t num_node_types) {
  return decode_check_rows(num_node_types >= 0, true, ids, elem_bytes, ld, len, num_rows, max_num_nodes);
}
inline int ibtt_decode_check_rows(const void *ids, int32_t elem_bytes, int32_t ld, const int32_t *len, int32_t num_rows, int32_t grammar,
                                  const int32_t *inv, int32_t inv_len, int32_t max_num_nodes) {
  const bool grammar_ok = grammar == GTOK_IBTT_GRAMMAR_ZINC || grammar == GTOK_IBTT_GRAMMAR_SYNTH;
  return decode_check_rows(inv_len > 0 && grammar_ok, inv != nullptr, ids, elem_bytes, ld, len, num_rows, max_num_nodes);
}

// labelled SENT rows and molecule IBTT rows carry types
inline int sent_decode_check_out(const gtok_csr_built *out, int32_t labeled) { return decode_check_out(out, labeled != 0); }
inline int ibtt_decode_check_out(const gtok_csr_built *out, int32_t grammar) { return decode_check_out(out, grammar == GTOK_IBTT_GRAMMAR_ZINC); }

// ZINC-remapped SENT rows (gtok_unremap_zinc, gtok_sent_decode_zinc_sizes / gtok_sent_decode_zinc_csr): the rows are checked as the
// un-remapped decoders check theirs, the rows are always labelled, and gtok_unremap_zinc needs its output slab.
inline int sent_decode_zinc_check_out(const gtok_csr_built *out) { return decode_check_out(out, true); }
inline int unremap_zinc_check(const void *ids, int32_t elem_bytes, int32_t ld, const int32_t *len, int32_t num_rows, int32_t max_num_nodes,
                              int32_t num_node_types, const int32_t *out_ids) {
  const int c = sent_decode_check_rows(ids, elem_bytes, ld, len, num_rows, max_num_nodes, num_node_types);
  if (c) return c;
  return out_ids ? GTOK_OK : GTOK_E_INVAL;
}

}  // namespace gtok
