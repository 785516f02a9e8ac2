// gtok_zinc_unremap.hpp - the ZINC remap of SENT ids (trainer/train_agtt.py:171-244; the kernels' own statement of it is
// remap_zinc_token, gtok_common.hpp) restated beside its INVERSE, in a header of their own (no HIP in it) usable from host and
// device: a plain C++ program can sweep the pair under the host sanitizers, and the decoders of remapped rows (gtok_unremap_zinc,
// gtok_sent_decode_zinc_sizes / gtok_sent_decode_zinc_csr: gtok_sent_decode.hip) use zinc_pre().  The rule is include/gtok.h's.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GTOK_HD __host__ __device__
#else
#define GTOK_HD
#endif

namespace gtok {

constexpr int kZincFolded = 2;    // the id RESET (1), LADJ (2), RADJ (3) - and PAD (5) - fold into
constexpr int kZincNone = -1;     // zinc_pre: the id has no preimage

// The forward map on a raw id t, branch order preserved: idx_off = 6, node_off = idx_off + max_num_nodes, edge_off = node_off +
// num_node_types.
GTOK_HD inline int zinc_remap(int t, int idx_off, int node_off, int edge_off) {
  if (t == 0) return 0;                                   // SOS
  if (t >= 1 && t <= 3) return kZincFolded;               // RESET, LADJ, RADJ
  if (t == 4) return 1;                                   // EOS
  if (t == 5) return kZincFolded;                         // PAD
  if (node_off <= t && t < edge_off) {                    // a node type: the nine atoms, or the fallback
    const int a = t - node_off;
    return a < 9 ? 8 + a : 22 + t;
  }
  if (t >= edge_off) {                                    // an edge type: the four bonds, or the fallback
    const int b = t - edge_off + 1;
    return b <= 4 ? 16 + b : 22 + t;
  }
  if (idx_off <= t && t < node_off) return 22 + (t - idx_off);   // a position
  return 22 + t;
}

// The inverse.  zinc_remap is injective on raw ids t >= 0 outside {1, 2, 3, 5}: zinc_pre(id) is the one such t with
// zinc_remap(t) == id, or kZincNone - for kZincFolded, for 3..7 and 21, for a negative id, and for a candidate whose remap is
// another id (8 + a with a >= num_node_types; 22 + t where t is an atom or a bond that has an id of its own).
GTOK_HD inline int zinc_pre(int id, int max_num_nodes, int num_node_types) {
  const int idx_off = 6, node_off = idx_off + max_num_nodes;
  if (id == 0) return 0;
  if (id == 1) return 4;
  if (id >= 8 && id <= 16) return id - 8 < num_node_types ? node_off + (id - 8) : kZincNone;
  if (id >= 17 && id <= 20) return node_off + num_node_types + (id - 17);
  if (id >= 22 && id - 22 < max_num_nodes) return idx_off + (id - 22);
  if (id >= 22 + node_off) {
    const int a = id - 22 - node_off;                     // (the candidate id - 22 lies at or behind node_off)
    if (a < num_node_types) return a >= 9 ? id - 22 : kZincNone;
    return a - num_node_types >= 4 ? id - 22 : kZincNone;
  }
  return kZincNone;
}

}  // namespace gtok
