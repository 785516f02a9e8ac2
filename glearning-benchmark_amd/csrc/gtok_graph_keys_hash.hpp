// gtok_graph_keys_hash.hpp - the arithmetic of gtok_graph_keys (include/gtok.h): a 128-bit keyed multiset digest of a NUMBERED
// graph, in a header of its own (no HIP in it) usable from host and device - the kernels (gtok_graph_keys.hip) and a plain C++
// program under the host sanitizers (tests/host/graph_keys_args_main.cpp) compute the same words; tests/_graph_keys_ref.py restates
// it in numpy.  The form and the constants are frozen in DESIGN.md ("graph keys"): a key is an identity that may be stored.
//
//   entry word   a | b << 14 | t << 28      a = min(u, v), b = max(u, v) (ids below 16,384: 14 bits each), t = the entry's eattr
//                                           byte with GTOK_KEYS_ATTRS, else 0
//   node word    u | nattr[u] << 14 | 1 << 40                              (GTOK_KEYS_ATTRS only; bit 40 keeps it apart from entries)
//   S_j          sum over the graph's terms of mix(word ^ C_j), mod 2^64   (j = 0, 1: two sums under two keys)
//   key_j        mix(S_j + mix((N | terms << 32) ^ C_j) + mix(label ^ D_j))   label = the caller's int32 as its 32-bit pattern, or 0
//
// A sum does not depend on the order of its terms, an entry word not on the entry's orientation: the key is that of the MULTISET of
// folded entries, which is what the reference's tuple key (test/train_performance_test.py:70-74: num_nodes, the sorted list of
// sorted endpoint pairs, the label) identifies.  It identifies a graph in ITS numbering - two isomorphic graphs numbered differently
// get different keys, as they get different tuples there.  Equal keys of different graphs are possible in principle (128 bits).
#pragma once
#include <stdint.h>

#ifndef GTOK_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define GTOK_HD __host__ __device__
#else
#define GTOK_HD
#endif
#endif

namespace gtok {

// C_0, C_1: the 64-bit golden ratio and xxHash64's PRIME64_2; D_0, D_1: xxHash64's PRIME64_3 and PRIME64_4.
constexpr uint64_t kKeysC0 = 0x9E3779B97F4A7C15ull, kKeysC1 = 0xC2B2AE3D27D4EB4Full;
constexpr uint64_t kKeysD0 = 0x165667B19E3779F9ull, kKeysD1 = 0x85EBCA77C2B2AE63ull;

// the splitmix64 finaliser (Steele, Lea & Flood 2014)
GTOK_HD inline uint64_t keys_mix(uint64_t z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

GTOK_HD inline uint64_t keys_entry_word(uint32_t u, uint32_t v, uint32_t t) {
  const uint32_t a = u < v ? u : v, b = u < v ? v : u;
  return (uint64_t)a | (uint64_t)b << 14 | (uint64_t)t << 28;
}
GTOK_HD inline uint64_t keys_node_word(uint32_t u, uint32_t x) { return (uint64_t)u | (uint64_t)x << 14 | 1ull << 40; }

// the two sums of a graph, one term at a time
struct KeySums {
  uint64_t s0 = 0, s1 = 0;
  GTOK_HD inline void add(uint64_t word) { s0 += keys_mix(word ^ kKeysC0); s1 += keys_mix(word ^ kKeysC1); }
};

GTOK_HD inline uint64_t keys_final(uint64_t S, uint32_t num_nodes, uint32_t terms, int32_t label, uint64_t C, uint64_t D) {
  return keys_mix(S + keys_mix(((uint64_t)num_nodes | (uint64_t)terms << 32) ^ C) + keys_mix((uint64_t)(uint32_t)label ^ D));
}
GTOK_HD inline void keys_finish(const KeySums &s, uint32_t num_nodes, uint32_t terms, int32_t label, uint64_t out[2]) {
  out[0] = keys_final(s.s0, num_nodes, terms, label, kKeysC0, kKeysD0);
  out[1] = keys_final(s.s1, num_nodes, terms, label, kKeysC1, kKeysD1);
}

}  // namespace gtok
