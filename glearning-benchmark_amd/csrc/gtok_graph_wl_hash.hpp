// gtok_graph_wl_hash.hpp - the arithmetic of gtok_graph_wl (include/gtok.h): a 128-bit key of a graph that does NOT depend on its
// numbering - Weisfeiler-Lehman colour refinement over 64-bit words, in a header of its own (no HIP in it) usable from host and
// device: the kernels (gtok_graph_wl.hip) and a plain C++ program under the host sanitizers (tests/host/graph_wl_args_main.cpp)
// compute the same words; tests/_graph_wl_ref.py restates it in numpy.  The form is frozen in DESIGN.md section 5c; the mixer and the
// four constants are those of gtok_graph_keys_hash.hpp.  All sums are mod 2^64.
//
// The graph of a CSR slice is the simple undirected closure gtok_graph_tasks defines: A(v) = the distinct neighbours u != v with
// (u, v) or (v, u) listed, loop_v = 1 iff (v, v) is listed, deg_v = |A(v)|.
//   a_v      = 0                  structure only;   1 + nattr[v]                                        with GTOK_WL_ATTRS
//   t_vu     = 0                  structure only;   1 + eattr of the entry (v, u) as row v lists it      with GTOK_WL_ATTRS
//   c_0[v]   = mix((deg_v | loop_v << 15 | a_v << 16) ^ C0)
//   c_r+1[v] = mix((c_r[v] + sum over u in A(v) of mix(c_r[u] ^ C1 ^ (t_vu * D1))) ^ D0)
//   S_j      = sum over v of mix(c_R[v] ^ C_j)                                                          j = 0, 1
//   key_j    = mix(S_j + mix((N | R << 32) ^ C_j) + mix((uint32)label ^ D_j))
// R = the rounds actually run: `rounds` when rounds >= 1, N when rounds == 0 (the colouring is stable by then).
// A sum does not depend on the order of its terms and no term names a node id: isomorphic graphs always share the key.  Graphs that
// are not isomorphic share it when R rounds of colour refinement cannot tell them apart (regular graphs of equal degree: C6 and two
// triangles), or by a collision of 64-bit words.  Structure-only terms depend on the neighbour alone: wl_term(c[u], 0) is computed
// once per node and round, and a node sums table entries.
#pragma once
#include <stdint.h>

#include "gtok_graph_keys_hash.hpp"

namespace gtok {

GTOK_HD inline uint64_t wl_init(uint32_t deg, uint32_t loop, uint32_t a) {
  return keys_mix(((uint64_t)deg | (uint64_t)loop << 15 | (uint64_t)a << 16) ^ kKeysC0);
}
// what neighbour u adds to node v's sum (t = t_vu)
GTOK_HD inline uint64_t wl_term(uint64_t cu, uint32_t t) { return keys_mix(cu ^ kKeysC1 ^ ((uint64_t)t * kKeysD1)); }
GTOK_HD inline uint64_t wl_next(uint64_t cv, uint64_t sum) { return keys_mix((cv + sum) ^ kKeysD0); }

// R of a graph of n nodes
GTOK_HD inline uint32_t wl_rounds_run(int32_t rounds, int32_t n) { return (uint32_t)(rounds >= 1 ? rounds : n); }

// the two sums over the final colours, one node at a time
struct WlSums {
  uint64_t s0 = 0, s1 = 0;
  GTOK_HD inline void add(uint64_t c) { s0 += keys_mix(c ^ kKeysC0); s1 += keys_mix(c ^ kKeysC1); }
};

GTOK_HD inline void wl_finish(const WlSums &s, uint32_t num_nodes, uint32_t rounds_run, int32_t label, uint64_t out[2]) {
  out[0] = keys_final(s.s0, num_nodes, rounds_run, label, kKeysC0, kKeysD0);      // (the same closing form as a graph key's, R in the
  out[1] = keys_final(s.s1, num_nodes, rounds_run, label, kKeysC1, kKeysD1);      // place of the term count)
}

}  // namespace gtok
