// gtok_ibtt_decode_args.hpp - the host-side argument checks of gtok_ibtt_decode_sizes / gtok_ibtt_decode_csr, in a header of
// their own (no HIP in it) so that a plain C++ program can exercise them under the host sanitizers.
#pragma once
#include <stdint.h>

#include "gtok.h"

namespace gtok {

// Nothing is launched or written before these pass.  Returns a GTOK_E_* code, GTOK_OK, or 1: no rows, nothing to do.
inline int ibtt_decode_check_rows(const void *ids, int32_t elem_bytes, int32_t ld, const int32_t *len, int32_t num_rows, int32_t grammar,
                                  const int32_t *inv, int32_t inv_len, int32_t max_num_nodes) {
  if (num_rows < 0 || ld <= 0 || max_num_nodes < 0 || inv_len <= 0) return GTOK_E_INVAL;
  if (grammar != GTOK_IBTT_GRAMMAR_ZINC && grammar != GTOK_IBTT_GRAMMAR_SYNTH) return GTOK_E_INVAL;
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) return GTOK_E_INVAL;
  if (max_num_nodes > GTOK_SENT_LARGE_MAX_NODES) return GTOK_E_TOO_LARGE;
  if (num_rows == 0) return 1;
  if (!ids || !len || !inv) return GTOK_E_INVAL;
  return GTOK_OK;
}

// the outputs pass 2 needs (molecule rows: the two type arrays as well)
inline int ibtt_decode_check_out(const gtok_csr_built *out, int32_t grammar) {
  if (!out || !out->node_ptr || !out->edge_ptr || !out->rowptr || !out->col || !out->eorder || !out->info) return GTOK_E_INVAL;
  if (grammar == GTOK_IBTT_GRAMMAR_ZINC && (!out->nattr || !out->eattr)) return GTOK_E_INVAL;
  return GTOK_OK;
}

}  // namespace gtok
