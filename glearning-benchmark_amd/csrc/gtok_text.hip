// gtok_text.hip — the gfx950 kernels that read raw text bytes, one wavefront per text, lane = byte: vocab_stats_text_kernel (corpus pass
// of build_vocab_from_texts), text_ids_kernel (data_loader.py:465-484, any grammar: text -> vocab ids), count_edge_tokens_kernel /
// parse_edge_zone_kernel / parse_graph_text_kernel (graph-token text -> edge lists).  Bit-exact checkers: oracle/gtok_oracle.c.
#include <cassert>
#include <cstdlib>

#include "gtok_common.hpp"   // (and gtok.h)

namespace gtok {

// ---------------------------------------------------------------------------------------------
// TokenDataset on raw text
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool py_isspace(uint32_t c) {
  return c == 32u || (c >= 9u && c <= 13u) || (c >= 28u && c <= 31u);
}

// ---------------------------------------------------------------------------------------------
// corpus pass of build_vocab_from_texts (data_loader.py:451-463) / the ZINC dynamic-token scan
// (trainer/train_ibtt.py:361-372) over ARBITRARY texts: occurrence count and first position of every
// distinct whitespace-separated token.  Wave per text; lane = byte; a token's start lane hashes it (two
// independent 32-bit FNV-1a streams = a 64-bit identity, the token's length is compared as well) and adds it
// to the wave's own LDS table; the table is merged into the global one once per wave (a hot token such as
// `<e>` would otherwise be one global atomic per occurrence).  first = byte offset of the token's earliest
// occurrence in the corpus blob: the blob is the texts in order, so offsets order occurrences exactly as
// Counter's first-insertion order does, and blob[first : first + len] is the token string itself.
// ---------------------------------------------------------------------------------------------
struct VocabTextArgs {
  const uint8_t *bytes; const int64_t *text_ptr; int num_texts;
  int64_t base_offset;
  int capacity;                                    // global table slots (power of two)
  unsigned long long *key, *count, *first; int32_t *len, *status;
  int lslots;                                      // per-wave LDS slots (power of two)
  int units, upb;
};

// Two tokens are the same token when their BYTES agree, not merely their 64-bit identity and length: every merge of an
// occurrence into a slot compares the occurrence with the slot's recorded first occurrence, byte for byte, wherever that
// one lies inside the blob of THIS launch (a `first` left by another shard's launch cannot be read here).  A mismatch -
// a hash collision - raises status bit 2 (value 4): the table would have dropped a token silently.
__device__ __forceinline__ bool vocab_text_same(const VocabTextArgs &a, unsigned long long p, unsigned long long q, unsigned int ln) {
  const unsigned long long lo = (unsigned long long)a.base_offset, hi = lo + (unsigned long long)a.text_ptr[a.num_texts];
  if (p == q || p < lo || p >= hi || q < lo || q >= hi) return true;
  const uint8_t *x = a.bytes + (p - lo), *y = a.bytes + (q - lo);
  for (unsigned int i = 0; i < ln; ++i)
    if (x[i] != y[i]) return false;
  return true;
}

__device__ __forceinline__ void vocab_text_global_add(const VocabTextArgs &a, unsigned long long k, unsigned int ln,
                                                      unsigned long long cnt, unsigned long long fst) {
  const unsigned int mask = (unsigned int)a.capacity - 1u;
  unsigned int slot = (unsigned int)(k ^ (k >> 29)) & mask;
  for (unsigned int probes = 0; probes <= mask; ++probes, slot = (slot + 1) & mask) {
    unsigned long long old = atomicCAS(a.key + slot, 0ull, k);
    if (old == 0ull) {                              // claimed an empty slot: publish the length
      __hip_atomic_store(a.len + slot, (int)ln, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      old = k;
    }
    if (old == k) {
      // same 64-bit identity: the lengths must agree too (the claimant's store may not have landed yet: 0 = not yet)
      int l2 = __hip_atomic_load(a.len + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (int spin = 0; l2 == 0 && spin < 1000000; ++spin) l2 = __hip_atomic_load(a.len + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (l2 == 0) { atomicOr(a.status, 2); return; }   // never seen in practice: the claimant's length did not arrive
      if (l2 == (int)ln) {
        atomicAdd(a.count + slot, cnt);
        const unsigned long long seen = atomicMin(a.first + slot, fst);
        if (seen != ~0ull && seen != 0x7FFFFFFFFFFFFFFFull && !vocab_text_same(a, seen, fst, ln)) atomicOr(a.status, 4);
        return;
      }
    }
  }
  atomicOr(a.status, 1);                            // table full: the caller enlarges it and runs again
}

__global__ void __launch_bounds__(256) vocab_stats_text_kernel(const VocabTextArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id();
  const int wave = wave_id(), wpb = (int)(blockDim.x >> 6);
  const int S = a.lslots;
  unsigned char *wb = smem + (size_t)wave * ((size_t)S * 24);
  unsigned long long *lkey = reinterpret_cast<unsigned long long *>(wb);
  unsigned long long *lfirst = lkey + S;
  unsigned int *lcount = reinterpret_cast<unsigned int *>(lfirst + S);
  unsigned int *llen = lcount + S;
  for (int i = lane; i < S; i += kWave) { lkey[i] = 0ull; lfirst[i] = ~0ull; lcount[i] = 0u; llen[i] = 0u; }
  wave_sync();
  const unsigned int lmask = (unsigned int)S - 1u;

  const int vb = virtual_block();
  const int u0 = vb * a.upb, u1 = min(a.units, u0 + a.upb);
  for (int unit = u0; unit < u1; ++unit) {
    const int g = unit * wpb + wave;
    if (g >= a.num_texts) break;
    const int64_t t0 = a.text_ptr[g];
    const uint8_t *__restrict__ s = a.bytes + t0;
    const int64_t n = a.text_ptr[g + 1] - t0;
    bool prev_sp = true;                            // a text starts a token: texts are not separated in the blob
    for (int64_t b0 = 0; b0 < n; b0 += kWave) {
      const int64_t i = b0 + lane;
      const uint32_t c = i < n ? s[i] : 32u;
      const bool sp = py_isspace(c);
      const uint64_t spm = __ballot(sp);
      const bool before = lane == 0 ? prev_sp : ((spm >> (lane - 1)) & 1ull);
      prev_sp = (spm >> 63) & 1ull;
      if (!sp && before) {
        uint32_t h1 = 2166136261u, h2 = 0x9747b28cu;
        unsigned int ln = 0;
        for (int64_t j = i; j < n; ++j) {
          const uint32_t cj = s[j];
          if (py_isspace(cj)) break;
          h1 = (h1 ^ cj) * 16777619u;
          h2 = (h2 ^ (cj + 0x9e3779b9u)) * 0x85ebca6bu; h2 ^= h2 >> 13;
          ++ln;
        }
        unsigned long long k = ((unsigned long long)h2 << 32) | h1;
        if (k == 0ull) k = 1ull;                    // 0 marks an empty slot
        const unsigned long long pos = (unsigned long long)(a.base_offset + t0 + i);
        bool placed = false;
        unsigned int slot = (unsigned int)(k ^ (k >> 29)) & lmask;
        for (unsigned int probes = 0; probes < 16u && !placed; ++probes, slot = (slot + 1) & lmask) {
          unsigned long long old = atomicCAS(lkey + slot, 0ull, k);
          if (old == 0ull) { atomicExch(llen + slot, ln); old = k; }
          if (old == k) {
            unsigned int l2 = __hip_atomic_load(llen + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            for (int spin = 0; l2 == 0u && spin < 100000; ++spin) l2 = __hip_atomic_load(llen + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            if (l2 == ln) {
              atomicAdd(lcount + slot, 1u);
              const unsigned long long seen = atomicMin(lfirst + slot, pos);
              if (seen != ~0ull && !vocab_text_same(a, seen, pos, ln)) atomicOr(a.status, 4);
              placed = true;
            }
          }
        }
        if (!placed) vocab_text_global_add(a, k, ln, 1ull, pos);   // crowded neighbourhood of the small table: straight to the global one
      }
    }
  }
  wave_sync();
  for (int i = lane; i < S; i += kWave)
    if (lkey[i] != 0ull) vocab_text_global_add(a, lkey[i], llen[i], (unsigned long long)lcount[i], lfirst[i]);
}

struct TextArgs {
  const uint8_t *bytes; const int64_t *text_ptr; int num_texts;
  gtok_vocab_table v;
  int strip_label, cap, max_len, pad_id;
  int32_t *out; int ld; int32_t *out_len;
  int units, upb;
  int off_vocab, off_wave, ring_off, tok_off, wave_stride;   // LDS: [vocab slots (VLDS)] then per wave: text ring, tokens
  int off_short;   // VLDS: second table, the keys of up to 7 bytes as {key lo, key hi, id, used} (one 16-byte read per probe)
  int sidx_off;    // per wave: the token starts of one 256-byte step, compacted (128 x int32)
  int short_slots; // its size (a power of two, >= capacity: the sparser it is, the shorter the probe chains the 64 lanes wait for)
};

// The text of one graph is read ONCE, 16 bytes per lane and load, into a 2 KB LDS ring (the chunk being split and
// the next one, so a token may run up to 1 KB past its chunk; beyond that bytes come from global), the chunk after
// that is requested before the current one is processed, and - VLDS - the vocab table is copied into LDS once per
// workgroup as 24-byte slots {id, length, first 19 key bytes} (longer keys finish their compare in global memory).
// The previous version read the text a byte per lane and hashed / probed straight from global memory: ~10
// dependent round trips per 64 bytes of text.
constexpr int kTextChunk = 1024, kTextRing = 2 * kTextChunk, kSlotBytes = 24, kSlotKey = 19;

struct __attribute__((aligned(16))) U32x4a { uint32_t x, y, z, w; };
constexpr uint32_t kSlotBusy = 0xFFFFFFFFu;   // short-key slot: claimed, its key not written yet (so a vocab id of -2 stays out of the table, like -1)
__device__ __forceinline__ uint32_t short_key_hash(uint32_t klo, uint32_t khi) {   // (the first 8 bytes: a key's third word only tells it apart in its slot)
  const uint32_t h = (klo ^ __builtin_amdgcn_alignbit(khi, khi, 19)) * 0x9E3779B1u;
  return h ^ (h >> 15);
}

template <bool VLDS>
__global__ void __launch_bounds__(512, 6) text_ids_kernel(const TextArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id();
  const int wave = wave_id(), wpb = (int)(blockDim.x >> 6);
  unsigned char *vs = smem + a.off_vocab;
  unsigned char *wbase = smem + a.off_wave + (size_t)wave * a.wave_stride;
  uint8_t *ring = wbase + a.ring_off;
  const int cap = a.cap;
  const uint32_t mask = (uint32_t)a.v.capacity - 1u;
  const int64_t total = a.text_ptr[a.num_texts];

  // four scratch words in front of the short-key table: [0] bytes readable at key_bytes (= the end of the last key: the ABI
  // carries no length, and the vector loads below must not leave the array), [1] some short key was left OUT of the short-key
  // table, [2] short keys offered so far, [3] short keys in the table (it grows while the texts are split, see `adopt`)
  int *scratch = reinterpret_cast<int *>(smem + a.off_short - 16);
  if (threadIdx.x == 0) { scratch[0] = 0; scratch[1] = 0; scratch[2] = 0; scratch[3] = 0; }
  __syncthreads();
  if (VLDS) {   // (only the 16-byte loads of the slot copy below need it: a key's own bytes are inside the array by definition)
    int my_end = 0;
    for (int sl = (int)threadIdx.x; sl < a.v.capacity; sl += (int)blockDim.x) {
      const int off = a.v.key_off[sl];
      if (off >= 0) my_end = max(my_end, off + a.v.key_len[sl]);
    }
    atomicMax(scratch, my_end);
  }
  __syncthreads();
  const int kb_total = VLDS ? scratch[0] : 0x7FFFFFFF;
  if (VLDS) {   // slot s: id (4 B), length (1 B; 255 = empty), key bytes (one unaligned 16-byte load + 3 bytes)
    for (int sl = (int)threadIdx.x; sl < a.v.capacity; sl += (int)blockDim.x) {
      unsigned char *d = vs + (size_t)sl * kSlotBytes;
      const int off = a.v.key_off[sl], len = off < 0 ? 255 : min(a.v.key_len[sl], 254);
      uint32_t w[5] = {0, 0, 0, 0, 0};
      if (off >= 0) {
        if (off + 20 <= kb_total) {
          const U8x16 x = *reinterpret_cast<const U8x16 *>(a.v.key_bytes + off);
          w[0] = x.a; w[1] = x.b; w[2] = x.c; w[3] = x.d;
          w[4] = (uint32_t)a.v.key_bytes[off + 16] | ((uint32_t)a.v.key_bytes[off + 17] << 8) | ((uint32_t)a.v.key_bytes[off + 18] << 16);
        } else {
          for (int j = 0; j < kSlotKey && off + j < kb_total; ++j) w[j >> 2] |= (uint32_t)a.v.key_bytes[off + j] << (8 * (j & 3));
        }
      }
      *reinterpret_cast<int32_t *>(d) = a.v.id[sl];
      d[4] = (unsigned char)len;
      for (int j = 0; j < kSlotKey; ++j) d[5 + j] = (unsigned char)((j < len) ? (w[j >> 2] >> (8 * (j & 3))) & 255u : 0u);
    }
  }
  // the short-key table (both modes: also a vocab too large for LDS - ZINC's, with its thousands of label tokens - has only a
  // few dozen keys that ever occur in a text): the tokens of a graph-token or molecule text are a few bytes long (node ids,
  // <e>, <bond>, aromatic, regression), so keys of up to 11 bytes are matched as ONE 96-bit value - slot = {lo, mid, hi, id + 1},
  // 0 = empty - instead of a hash loop and a compare loop over their bytes.  Keys of up to 7 bytes go in first, then those of
  // 8 .. 11, while the table is less than a quarter full (they are label tokens, one per text at most: not worth longer probe chains for
  // every other token); whatever is left out (and a key whose id is -1) makes a miss non-final: such a
  // token takes the byte loops.
  uint32_t *st = reinterpret_cast<uint32_t *>(smem + a.off_short);
  const uint32_t smask_b = (uint32_t)a.short_slots - 1u;
  for (int sl = (int)threadIdx.x; sl < a.short_slots; sl += (int)blockDim.x) *reinterpret_cast<U32x4a *>(st + sl * 4) = U32x4a{0u, 0u, 0u, 0u};
  __syncthreads();
  for (int pass = 0; pass < 2; ++pass) {
    for (int sl = (int)threadIdx.x; sl < a.v.capacity; sl += (int)blockDim.x) {
      const int off = a.v.key_off[sl];
      const int len = off < 0 ? 0 : a.v.key_len[sl];
      if (len < (pass ? 8 : 1) || len > (pass ? 11 : 7)) continue;
      const uint32_t idp1 = (uint32_t)a.v.id[sl] + 1u;
      if (idp1 == 0u || idp1 == kSlotBusy || atomicAdd(&scratch[2], 1) >= (pass ? a.short_slots / 4 : a.short_slots / 2)) { scratch[1] = 1; continue; }
      atomicAdd(&scratch[3], 1);
      uint32_t k[3] = {0u, 0u, 0u};
      for (int j = 0; j < len && off + j < kb_total; ++j) k[j >> 2] |= (uint32_t)a.v.key_bytes[off + j] << (8 * (j & 3));
      uint32_t idx = short_key_hash(k[0], k[1]) & smask_b;
      while (atomicCAS(&st[idx * 4 + 3], 0u, idp1) != 0u) idx = (idx + 1) & smask_b;
      st[idx * 4 + 0] = k[0]; st[idx * 4 + 1] = k[1]; st[idx * 4 + 2] = k[2];
    }
    __syncthreads();   // (the second one is the last workgroup barrier: before any wave can leave)
  }
  const bool has_m1 = scratch[1] != 0;   // a short-table miss is not final
  auto load16 = [&](int64_t abs) -> U8x16 {   // never touches bytes past the end of the blob
    if (abs + 16 <= total) return *reinterpret_cast<const U8x16 *>(a.bytes + abs);
    uint32_t w[4] = {0x20202020u, 0x20202020u, 0x20202020u, 0x20202020u};
    for (int b = 0; b < 16; ++b)
      if (abs + b < total) w[b >> 2] = (w[b >> 2] & ~(0xFFu << (8 * (b & 3)))) | ((uint32_t)a.bytes[abs + b] << (8 * (b & 3)));
    return U8x16{w[0], w[1], w[2], w[3]};
  };
  U8x16a *ring16 = reinterpret_cast<U8x16a *>(ring);

  const int vb = virtual_block();
  const int u0 = vb * a.upb, u1 = min(a.units, u0 + a.upb);
  for (int unit = u0; unit < u1; ++unit) {
    const int g = unit * wpb + wave;
    if (g >= a.num_texts) break;
    const int64_t t0 = a.text_ptr[g];
    const uint8_t *__restrict__ s = a.bytes + t0;
    const int64_t n = a.text_ptr[g + 1] - t0;
    // ring <- chunks 0 and 1
    wave_sync();
    {
      const U8x16 x0 = load16(t0 + lane * 16), x1 = load16(t0 + kTextChunk + lane * 16);
      ring16[lane] = U8x16a{x0.a, x0.b, x0.c, x0.d};
      ring16[64 + lane] = U8x16a{x1.a, x1.b, x1.c, x1.d};
    }
    wave_sync();
    int32_t *__restrict__ orow = a.out + (int64_t)g * a.ld;
    int count = 0;
    bool prev_sp = true;  // carry: was the byte before this chunk whitespace
    bool done = false;
    for (int64_t c0 = 0; c0 < n && count < a.max_len && !done; c0 += kTextChunk) {
      const int64_t have = c0 + kTextRing;                       // bytes below this offset are in the ring
      const U8x16 nxt = load16(t0 + c0 + kTextRing + lane * 16);   // chunk +2: in flight while this one is split
      auto byte_at = [&](int64_t j) -> uint32_t { return j < have ? ring[j & (kTextRing - 1)] : s[j]; };
      // one token: its id (pad_id when it is not in the vocab, as TokenDataset's vocab.get(tok, vocab['<pad>'])) and whether it is "<p>"
      auto lookup = [&](const int64_t i, int &id, bool &is_p) __attribute__((always_inline)) {
        id = a.pad_id; is_p = false;
#ifdef GTOK_ABLATE_TEXT_LOOKUP   // (profiling builds: no vocab look-up - wrong ids, the time difference is the look-ups')
        id = (int)(i & 7); return;
#endif
        bool fast = false, keyed = false, hit = false;
        uint32_t klo = 0u, khi = 0u, kx = 0u;
        {
          // tokens of up to 11 bytes: the 12 bytes at i (all in the ring; what lies behind the end of the text reads as
          // spaces) as one 96-bit value, cut at their first whitespace - found with the zero-byte trick on "byte < 33"
          // (ASCII: exact for the lowest flag) - and looked up in the short-key table.  Anything else (longer, a control
          // character that is not whitespace, a vocab id of -1) takes the byte loops below.
          const uint32_t *ring32 = reinterpret_cast<const uint32_t *>(ring);
          const uint32_t o = (uint32_t)i & (kTextRing - 1), sh = o & 3u, q = o >> 2;
          constexpr uint32_t RM = kTextRing / 4 - 1;
          const uint32_t w0 = ring32[q], w1 = ring32[(q + 1) & RM], w2 = ring32[(q + 2) & RM];
          klo = __builtin_amdgcn_alignbyte(w1, w0, sh); khi = __builtin_amdgcn_alignbyte(w2, w1, sh);
          const int rem = (int)min((int64_t)12, n - i);                 // bytes of the text at i (>= 1)
          if (rem < 8) {                                                // (the last token or two of a text)
            const uint32_t keep_lo = rem >= 4 ? ~0u : (1u << (8 * rem)) - 1u, keep_hi = rem <= 4 ? 0u : (1u << (8 * (rem - 4))) - 1u;
            klo = (klo & keep_lo) | (0x20202020u & ~keep_lo);
            khi = (khi & keep_hi) | (0x20202020u & ~keep_hi);
          }
          const uint32_t flo = (klo - 0x21212121u) & ~klo & 0x80808080u, fhi = (khi - 0x21212121u) & ~khi & 0x80808080u;
          int len = -1;
          uint32_t delim = 0u;
          if (flo | fhi) {                                              // the token ends inside its first 8 bytes
            len = flo ? (__builtin_ctz(flo) >> 3) : 4 + (__builtin_ctz(fhi) >> 3);
            delim = ((flo ? klo : khi) >> (8 * (len & 3))) & 255u;
            const uint32_t part = (1u << (8 * (len & 3))) - 1u;          // bytes of the token in its last, partial word
            klo = len >= 4 ? klo : klo & part;
            khi = len <= 4 ? 0u : khi & part;
          } else {                                                      // 8 .. 11 bytes: one more word (few lanes, few steps)
            kx = __builtin_amdgcn_alignbyte(ring32[(q + 3) & RM], w2, sh);
            if (rem < 12) { const uint32_t keep = (1u << (8 * (rem - 8))) - 1u; kx = (kx & keep) | (0x20202020u & ~keep); }
            const uint32_t fx = (kx - 0x21212121u) & ~kx & 0x80808080u;
            if (fx) {
              len = 8 + (__builtin_ctz(fx) >> 3);
              delim = (kx >> (8 * (len & 3))) & 255u;
              kx = kx & ((1u << (8 * (len & 3))) - 1u);
            }
          }
          if (len >= 1 && (VLDS || klo != 0u) && py_isspace(delim)) {    // (klo != 0: a key can never look like a slot being written)
            const uint32_t smask = (uint32_t)a.short_slots - 1u;
            const U32x4a *stab = reinterpret_cast<const U32x4a *>(smem + a.off_short);
            for (uint32_t slot = short_key_hash(klo, khi) & smask;; slot = (slot + 1) & smask) {
              const U32x4a e = stab[slot];
              if (e.w == 0u || (!VLDS && e.w == kSlotBusy)) break;      // not among the short keys (yet)
              if (e.x == klo && e.y == khi && e.z == kx) { id = (int)(e.w - 1u); hit = true; break; }
            }
            is_p = len == 3 && klo == 0x003E703Cu;                      // "<p>"
            keyed = true;
            fast = hit || !has_m1;                                      // (a miss is final when every short key of the vocab is in the table)
          }
        }
        if (!fast) {
        // hash the token (FNV-1a), then probe the open-addressing table
        uint32_t h = 2166136261u;
        int len = 0;
        for (int64_t j = i; j < n; ++j) {
          const uint32_t cj = byte_at(j);
          if (py_isspace(cj)) break;
          h = (h ^ cj) * 16777619u;
          ++len;
        }
        is_p = (len == 3) && byte_at(i) == '<' && byte_at(i + 1) == 'p' && byte_at(i + 2) == '>';
        for (uint32_t slot = h & mask, probes = 0; probes <= mask; slot = (slot + 1) & mask, ++probes) {
          if (VLDS) {
            const unsigned char *d = vs + (size_t)slot * kSlotBytes;
            const int kl = d[4];
            if (kl == 255) break;
            if (kl != min(len, 254)) continue;
            bool eq = true;
            for (int j = 0; j < min(len, kSlotKey) && eq; ++j) eq = d[5 + j] == byte_at(i + j);
            if (eq && len > kSlotKey) {   // long key: the rest (and keys of 254+ bytes: everything) from global
              const int off = a.v.key_off[slot];
              eq = a.v.key_len[slot] == len;
              for (int j = kSlotKey; j < len && eq; ++j) eq = a.v.key_bytes[off + j] == byte_at(i + j);
            }
            if (eq) { id = *reinterpret_cast<const int32_t *>(d); hit = true; break; }
          } else {
            const int off = a.v.key_off[slot];
            if (off < 0) break;
            if (a.v.key_len[slot] != len) continue;
            bool eq = true;
            for (int j = 0; j < len && eq; ++j) eq = a.v.key_bytes[off + j] == byte_at(i + j);
            if (eq) { id = a.v.id[slot]; hit = true; break; }
          }
        }
        // a short key that was left out of the table at set-up and does occur in the texts ("regression" behind three
        // thousand val_* label tokens) is ADOPTED: its next look-up is one LDS read instead of these byte loops over global
        // memory (only there: a vocab small enough for LDS has its byte loops in LDS).  The slot is claimed (its id word -> busy), the key written, then the id: a reader that meets a busy slot,
        // or the words of a slot mid-write (zeros: no key is zero), just misses and comes here.
        if (!VLDS && keyed && hit) {
          const uint32_t idp1 = (uint32_t)id + 1u, smask = (uint32_t)a.short_slots - 1u;
          uint32_t *stw = reinterpret_cast<uint32_t *>(smem + a.off_short);
          if (idp1 != 0u && idp1 != kSlotBusy && atomicAdd(&scratch[3], 1) < a.short_slots / 2) {
            for (uint32_t slot = short_key_hash(klo, khi) & smask;; slot = (slot + 1) & smask) {
              const uint32_t was = atomicCAS(&stw[slot * 4 + 3], 0u, kSlotBusy);
              if (was == 0u) {
                stw[slot * 4 + 0] = klo; stw[slot * 4 + 1] = khi; stw[slot * 4 + 2] = kx;
                __threadfence_block();
                __hip_atomic_store(&stw[slot * 4 + 3], idp1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                break;
              }
              if (was == kSlotBusy) break;                              // another wave is writing here - perhaps this very key
              if (stw[slot * 4 + 0] == klo && stw[slot * 4 + 1] == khi && stw[slot * 4 + 2] == kx) break;   // adopted meanwhile
            }
          }
        }
        }
      };
      // 256 bytes per step, FOUR per lane (one aligned dword of the ring): whitespace flags of the lane's bytes, token starts
      // among them (a token is at least one byte and one separator: at most two starts per dword), token numbers from two
      // ballots.  With a byte per lane a 64-byte piece of a molecule text holds ~13 token starts: four fifths of the lanes sat
      // out the look-ups, which are what the kernel's time is made of.
      const uint32_t *ring32w = reinterpret_cast<const uint32_t *>(ring);
      int32_t *sidx = reinterpret_cast<int32_t *>(wbase + a.sidx_off);
      for (int sub = 0; sub < kTextChunk / (4 * kWave) && count < a.max_len && !done; ++sub) {
        const int64_t b0 = c0 + sub * (4 * kWave);
        if (b0 >= n) break;
        const int64_t i0 = b0 + 4 * lane;
        uint32_t w = ring32w[((uint32_t)i0 & (kTextRing - 1)) >> 2];
        const int64_t left = n - i0;                                  // bytes of the text in this dword; the rest reads as spaces
        if (left < 4) w = left <= 0 ? 0x20202020u : ((w & ((1u << (8 * (int)left)) - 1u)) | (0x20202020u << (8 * (int)left)));
        // Python's ASCII whitespace - 9..13, 28..32 - for the four bytes at once, flags in bit 7 of each byte: "byte >= c" is bit 7
        // of (byte & 0x7F) + (0x80 - c), exact per byte (no carry leaves a byte), bytes >= 0x80 are never whitespace
        const uint32_t lo7 = w & 0x7F7F7F7Fu;
        const uint32_t ge9 = lo7 + 0x77777777u, ge14 = lo7 + 0x72727272u, ge28 = lo7 + 0x64646464u, ge33 = lo7 + 0x5F5F5F5Fu;
        const uint32_t sp4 = ((ge9 & ~ge14) | (ge28 & ~ge33)) & ~w & 0x80808080u;
        const uint64_t lastsp = __ballot((sp4 >> 31) != 0u);
        const uint32_t before0 = lane == 0 ? (prev_sp ? 0x80u : 0u) : (uint32_t)((lastsp >> (lane - 1)) & 1ull) << 7;
        prev_sp = (lastsp >> 63) & 1ull;
        const uint32_t st4 = ~sp4 & ((sp4 << 8) | before0) & 0x80808080u;     // bit 7 of byte b: byte b starts a token
        const int nst = __popc(st4);
        const uint64_t m1 = __ballot(nst >= 1), m2 = __ballot(nst >= 2);
        if (m1 == 0) continue;
        const int pre = __popcll(m1 & lanemask_lt()) + __popcll(m2 & lanemask_lt());   // token starts in the lanes below
        const int T = __popcll(m1) + __popcll(m2);                                     // token starts of this step (<= 128)
        // the starts are compacted through LDS so that the look-ups - two dependent LDS round trips each - run on FULL lanes:
        // one dense pass for a molecule text's ~52 tokens per step instead of a first-start pass and a sparse second-start pass
        if (nst >= 1) sidx[pre] = (int32_t)(i0 - b0) + (__builtin_ctz(st4) >> 3);
        if (nst >= 2) sidx[pre + 1] = (int32_t)(i0 - b0) + (__builtin_ctz(st4 & (st4 - 1u)) >> 3);
        wave_sync();
        int first_p = 1 << 30;
        for (int q0 = 0; q0 < T; q0 += kWave) {
          const int q = q0 + lane, t = count + q;
          bool isp = false;
          int id = a.pad_id;
          bool mine = q < T && t < a.max_len;
          const int64_t ti = mine ? b0 + sidx[q] : 0;
          if (a.strip_label) {
            // "<p>" is found BEFORE the look-ups: what follows it - the label, <eos> - is cut (data_loader.py:479-481), and a
            // label token is the one kind a large vocab's short-key table may not hold (thousands of val_* keys)
            if (mine && ti + 3 <= n) {
              const uint32_t o = (uint32_t)ti & (kTextRing - 1), q4 = o >> 2;
              const uint32_t k = __builtin_amdgcn_alignbyte(ring32w[(q4 + 1) & (kTextRing / 4 - 1)], ring32w[q4], o & 3u);
              isp = (k & 0x00FFFFFFu) == 0x003E703Cu && (ti + 3 == n || py_isspace(k >> 24));
            }
            const uint64_t pm = __ballot(isp);
            if (pm) first_p = q0 + __ffsll((unsigned long long)pm) - 1;
            mine = mine && q <= first_p;
          }
          bool isp2;
          if (mine) lookup(ti, id, isp2);
          // ids go straight to the row: lane q holds token count + q, so a pass is one coalesced run of stores (no staging
          // in LDS, no second pass over the row); nothing behind the first "<p>" is written
          if (mine && t < cap && q <= first_p) orow[t] = id;
          if (first_p != (1 << 30) || count + q0 + kWave >= a.max_len) break;
        }
        wave_sync();                                                  // sidx is rewritten by the next step
        if (first_p != (1 << 30)) {  // data_loader.py:479-481: keep up to and including the first <p>
          count += first_p + 1;
          done = true;
        } else {
          count += T;
        }
      }
      wave_sync();   // every lane is done with chunk c0: its half of the ring takes chunk +2
      ring16[((c0 / kTextChunk) & 1) * 64 + lane] = U8x16a{nxt.a, nxt.b, nxt.c, nxt.d};
      wave_sync();
    }
    wave_sync();
    const int len = min(count, a.max_len);
#ifndef GTOK_ABLATE_TEXT_WRITE
    for (int i = min(len, cap) + lane; i < a.ld; i += kWave) orow[i] = a.pad_id;      // the tokens are in place: only the tail is left
#endif
    if (lane == 0) a.out_len[g] = len;
    wave_sync();
  }
}

// ---------------------------------------------------------------------------------------------
// graph-token text -> edge list (graph_token_dataset_autograph.py:14-158), canonical texts
// ---------------------------------------------------------------------------------------------
// `<bos> (INT INT <e>)* <n> INT* [<q> WORD [INT INT]] [<p> WORD] ...`: for a text in this form the reference's
// left-to-right scan takes exactly the `INT INT <e>` triples before `<n>` as edges, the integers after `<n>` as the
// node list, the two integers after `<q> shortest_distance` as the query and the word after `<p>` as the label.
// Token k (k >= 1) of the edge zone is the source (k % 3 == 1) or target (k % 3 == 2) of edge (k - 1) / 3, so every
// token lane writes its own value: no sequential scan.  Anything else - a token out of place, an integer of more
// than 9 digits, a second <n>/<q>/<p> - sets status 1 and the host parser takes that record (the reference's scan has
// corner semantics, int() included, that are not worth a kernel).  Wave per text, 64 bytes per step, lane = byte.
enum { T_INT = 0, T_BOS, T_E, T_N, T_Q, T_P, T_EOS, T_OTHER };
constexpr int32_t kNoLabel = INT32_MIN;
// ---------------------------------------------------------------------------------------------
// number of `<e>` tokens per text = the number of edges of a text in the canonical graph-token form: the sizing pass
// of gtok_parse_graph_text without the parse.  Streaming: every lane looks at 16 bytes (plus two after) and counts the
// positions where the three bytes `<e>` begin - one byte-aligned dword and one compare per position.  What stands around the
// three bytes is not looked at: the count is exact for canonical texts and never BELOW the number of `<e>` tokens of any text,
// which is what a sizing pass owes (a text with `x<e>` in a word gets a slot too many; gtok.ops squeezes such ranges).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) count_edge_tokens_kernel(const uint8_t *__restrict__ bytes, const int64_t *__restrict__ text_ptr,
                                                                int num_texts, int32_t *__restrict__ num_edges) {
  const int lane = lane_id();
  const int g = (int)blockIdx.x * (int)(blockDim.x >> 6) + wave_id();
  if (g >= num_texts) return;
  const int64_t t0 = text_ptr[g], n = text_ptr[g + 1] - t0;
  const uint8_t *__restrict__ s = bytes + t0;
  int cnt = 0;
  auto load = [&](int64_t b0, uint32_t (&w)[5]) __attribute__((always_inline)) {   // bytes b0 .. b0+19; outside the text = space
    if (b0 + 20 <= n) {
      const U8x16 x = *reinterpret_cast<const U8x16 *>(s + b0);
      w[0] = x.a; w[1] = x.b; w[2] = x.c; w[3] = x.d;
      __builtin_memcpy(&w[4], s + b0 + 16, 4);
    } else {
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int64_t i = b0 + 4 * k + j; v |= (i < n ? (uint32_t)s[i] : 32u) << (8 * j); }
        w[k] = v;
      }
    }
  };
  constexpr uint32_t kTag = ((uint32_t)'<' << 8) | ((uint32_t)'e' << 16) | ((uint32_t)'>' << 24);   // the three bytes, shifted up by one
  auto tags = [&](const uint32_t (&w)[5]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint32_t x = (j & 3) ? __builtin_amdgcn_alignbyte(w[(j >> 2) + 1], w[j >> 2], (uint32_t)(j & 3)) : w[j >> 2];   // bytes b0+j .. b0+j+3
      cnt += ((x << 8) == kTag) ? 1 : 0;
    }
  };
  for (int64_t b0 = (int64_t)lane * 16; b0 < n; b0 += 2 * kWave * 16) {   // two 1 KB steps per turn: both loads are out before the first is looked at
    uint32_t w0[5], w1[5];
    load(b0, w0);
    load(b0 + kWave * 16, w1);                                             // (wholly behind the text: reads as spaces)
    tags(w0);
    tags(w1);
  }
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  if (lane == 0) num_edges[g] = cnt;
}

struct ParseArgs {
  const uint8_t *bytes; const int64_t *text_ptr; int num_texts;
  const int64_t *edge_ptr; int32_t *src, *dst;   // pass 2 only (NULL in pass 1)
  int32_t *num_edges, *num_nodes, *query, *label, *status;
  int units, upb;
};

// ---------------------------------------------------------------------------------------------
// graph-token text -> edge list, phase 1: the edge zone, streamed (wave per text, 1 KB per step, registers only: a light
// kernel with many waves per SIMD, so that the loads of one wave travel behind the work of the others)
// ---------------------------------------------------------------------------------------------
// `INT INT <e>` triples are nearly all of a text.  The stream walks TAGS, not bytes (round 4; the byte walk it replaces -
// value / length / all-digits carried over 32 bytes per lane, eight token slots - cost ~750 vector instructions per step):
//   * every lane classes its 16 bytes with three masks - spaces, digits, bytes of a `<e>` (one byte-aligned dword compare per
//     position, as the sizing pass does) - and the window passes only if every byte is one of the three (plus `<bos> ` at the
//     very start of the text);
//   * for each `<e>` that STARTS in its bytes (at most two: a triple is >= 8 bytes) the lane reads backwards
//     `> u v <e> ` - a space, v (1-4 digits), a space, u (1-4 digits, at most 7 with v), a space, and the `>` that ends the tag
//     before (or <bos>) - out of the 12 bytes in front of the tag, with 4-byte SWAR arithmetic for the two numbers; so the
//     bytes between two consecutive tags are exactly one edge, single spaces, and the edge's index is the tag's rank.
// The first window in which anything fails - another token, a tab, a double space, a 5-digit id, a tag out of place - and
// everything behind it go through parse_graph_text_kernel's general loop, which starts right behind the last tag the stream
// took with the token count where the stream left it: same results, byte for byte.  Integers behind a window's last tag are
// not taken here; their tag takes them (next window) or the general loop does.
__global__ void __launch_bounds__(256) parse_edge_zone_kernel(const ParseArgs a) {
  const int lane = lane_id();
  const int g = (int)blockIdx.x * (int)(blockDim.x >> 6) + wave_id();
  if (g >= a.num_texts) return;
  const bool fill = a.edge_ptr != nullptr;
  const uint8_t *__restrict__ s = a.bytes + a.text_ptr[g];
  const int64_t n = a.text_ptr[g + 1] - a.text_ptr[g];
  const int64_t ebase = fill ? a.edge_ptr[g] : 0;
  const int64_t ecap = fill ? a.edge_ptr[g + 1] - ebase : 0;
  auto spaces4 = [](uint32_t x) __attribute__((always_inline)) -> uint32_t {   // 0x80 in every byte that is a space
    const uint32_t y = x ^ 0x20202020u;
    return ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u;
  };
  auto nondig4 = [](uint32_t x) __attribute__((always_inline)) -> uint32_t {   // 0x80 in every byte that is NOT a digit
    const uint32_t t = x ^ 0x30303030u;
    return (((t & 0x7F7F7F7Fu) + 0x76767676u) | t) & 0x80808080u;
  };
  auto nib = [](uint32_t m) __attribute__((always_inline)) -> uint32_t { return (((m >> 7) * 0x00204081u) >> 21) & 15u; };   // 0x80-per-byte -> 4 bits
  auto atoi4 = [](uint32_t d) __attribute__((always_inline)) -> uint32_t {   // up to four digits, first digit in the lowest byte, bytes in front zeroed
    d &= 0x0F0F0F0Fu;
    const uint32_t t = (d * 10u + (d >> 8)) & 0x00FF00FFu;
    return (t * 100u + (t >> 16)) & 0xFFFFu;
  };
  int64_t handover = 0;
  int tags = 0, max_end = -1;
  for (int64_t wb = 0; wb < n; wb += 1024) {
    const int64_t o = wb + 16 * lane;
    uint32_t w[9];                                              // bytes o - 16 .. o + 19; outside the text: spaces
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int64_t rel = o - 16 + 16 * half;
      if (rel >= 0 && rel + 16 <= n) {
        const U8x16 x = *reinterpret_cast<const U8x16 *>(s + rel);
        w[4 * half] = x.a; w[4 * half + 1] = x.b; w[4 * half + 2] = x.c; w[4 * half + 3] = x.d;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          uint32_t v = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) { const int64_t i = rel + 4 * k + j; v |= ((i >= 0 && i < n) ? (uint32_t)s[i] : 32u) << (8 * j); }
          w[4 * half + k] = v;
        }
      }
    }
    if (o + 20 <= n) {
      __builtin_memcpy(&w[8], s + o + 16, 4);
    } else {
      uint32_t v = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { const int64_t i = o + 16 + j; v |= (i < n ? (uint32_t)s[i] : 32u) << (8 * j); }
      w[8] = v;
    }
    // ---- byte classes of the lane's 16 bytes (sp: and of the four behind them)
    const uint32_t sp = nib(spaces4(w[4])) | (nib(spaces4(w[5])) << 4) | (nib(spaces4(w[6])) << 8) | (nib(spaces4(w[7])) << 12) |
                        (nib(spaces4(w[8])) << 16);
    const uint32_t nd = nib(nondig4(w[4])) | (nib(nondig4(w[5])) << 4) | (nib(nondig4(w[6])) << 8) | (nib(nondig4(w[7])) << 12);
    constexpr uint32_t kTag = ((uint32_t)'<' << 8) | ((uint32_t)'e' << 16) | ((uint32_t)'>' << 24);   // the three bytes, shifted up by one
    uint32_t tall = 0;                                          // bit j + 2: `<e>` starts at byte o + j, j = -2 .. 15
#pragma unroll
    for (int j = -2; j < 16; ++j) {
      const int b = 16 + j;
      const uint32_t x = (b & 3) ? __builtin_amdgcn_alignbyte(w[(b >> 2) + 1], w[b >> 2], (uint32_t)(b & 3)) : w[b >> 2];
      tall |= ((x << 8) == kTag ? 1u : 0u) << (j + 2);
    }
    const uint32_t town = tall >> 2;                            // tags that start in this lane's bytes
    uint32_t cover = (sp & 0xFFFFu) | (~nd & 0xFFFFu) | (((tall | (tall << 1) | (tall << 2)) >> 2) & 0xFFFFu);
    bool wrong = false;
    if (wb == 0) {                                              // the text opens with `<bos> ` (or is `<bos>`)
      const bool bos = w[4] == 0x736F623Cu && (w[5] & 0xFFFFu) == 0x203Eu;
      if (lane == 0) { wrong = !bos; cover |= 0x1Fu; }
    }
    wrong = wrong || cover != 0xFFFFu || __popc(town) > 2;
    // ---- the (at most two) tags that start here: `> u v <e> ` read backwards
    uint32_t eu[2] = {0u, 0u}, ev[2] = {0u, 0u};
    uint32_t tm = town;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const bool has = tm != 0u;
      const int j = has ? (int)__builtin_ctz(tm) : 0;
      tm &= tm - 1u;
      const int b = (j + 4) >> 2;                               // w[b] holds byte o + j - 12
      const uint32_t sh = (uint32_t)(j & 3);
      const bool b1 = b == 1, b2 = b == 2, b3 = b == 3;
      const uint32_t y0 = b1 ? w[1] : (b2 ? w[2] : (b3 ? w[3] : w[4]));
      const uint32_t y1 = b1 ? w[2] : (b2 ? w[3] : (b3 ? w[4] : w[5]));
      const uint32_t y2 = b1 ? w[3] : (b2 ? w[4] : (b3 ? w[5] : w[6]));
      const uint32_t y3 = b1 ? w[4] : (b2 ? w[5] : (b3 ? w[6] : w[7]));
      const uint32_t x0 = __builtin_amdgcn_alignbyte(y1, y0, sh);   // bytes j - 12 .. j - 9
      const uint32_t x1 = __builtin_amdgcn_alignbyte(y2, y1, sh);   //       j -  8 .. j - 5
      const uint32_t x2 = __builtin_amdgcn_alignbyte(y3, y2, sh);   //       j -  4 .. j - 1
      bool ok = ((sp >> (j + 3)) & 1u) != 0u && (x2 >> 24) == 32u;   // a space (or the text's end) behind the tag, a space in front
      // v: the digits that end at byte j - 2
      const uint32_t v4 = __builtin_amdgcn_alignbyte(x2, x1, 3u);   // bytes j - 5 .. j - 2
      const uint32_t vs = spaces4(v4) & 0x00808080u;
      const int lv = vs ? 3 - (int)((31u - (uint32_t)__builtin_clz(vs)) >> 3) : 4;
      const uint32_t vkeep = 0xFFFFFFFFu << (8 * (4 - lv));
      ok = ok && (nondig4(v4) & vkeep) == 0u && (lv < 4 || ((x1 >> 16) & 255u) == 32u);
      // u: the digits that end at byte j - 3 - lv
      const uint32_t u4 = lv <= 2 ? __builtin_amdgcn_alignbyte(x2, x1, (uint32_t)(2 - lv)) : __builtin_amdgcn_alignbyte(x1, x0, (uint32_t)(6 - lv));
      const uint32_t us = spaces4(u4) & 0x00808080u;
      const int lu = us ? 3 - (int)((31u - (uint32_t)__builtin_clz(us)) >> 3) : 4;
      const uint32_t ukeep = 0xFFFFFFFFu << (8 * (4 - lu));
      ok = ok && (nondig4(u4) & ukeep) == 0u && lv + lu <= 7;
      // `> ` in front of u: bytes j - 4 - lv - lu, j - 3 - lv - lu
      const int pq = 8 - lv - lu;                               // their offset behind byte j - 12: 1 .. 6 when lv + lu <= 7
      const uint32_t pp = pq < 4 ? __builtin_amdgcn_alignbyte(x1, x0, (uint32_t)(pq & 3)) : __builtin_amdgcn_alignbyte(x2, x1, (uint32_t)(pq & 3));
      ok = ok && (pp & 0xFFFFu) == 0x203Eu;
      wrong = wrong || (has && !ok);
      ev[q] = atoi4(v4 & vkeep);
      eu[q] = atoi4(u4 & ukeep);
    }
    const int nt = __popc(town);
    int incl = nt;
#pragma unroll
    for (int dsh = 1; dsh < kWave; dsh <<= 1) { const int up = __shfl_up(incl, dsh); if (lane >= dsh) incl += up; }
    if (__ballot(wrong) != 0) break;
    {
      const int64_t k0 = (int64_t)tags + incl - nt;
#pragma unroll
      for (int q = 0; q < 2; ++q)
        if (q < nt) {
          max_end = max(max_end, (int)max(eu[q], ev[q]));
          if (fill && k0 + q < ecap) { a.src[ebase + k0 + q] = (int)eu[q]; a.dst[ebase + k0 + q] = (int)ev[q]; }
        }
    }
    tags += __builtin_amdgcn_readlane(incl, 63);
    const uint64_t holders = __ballot(town != 0u);
    if (holders) {
      const int l = 63 - __builtin_clzll(holders);
      handover = wb + 16 * l + (31 - __builtin_clz((uint32_t)__builtin_amdgcn_readlane((int)town, l))) + 3;
    }
  }
  for (int off = 32; off > 0; off >>= 1) max_end = max(max_end, __shfl_xor(max_end, off));
  if (lane == 0) {   // state for parse_graph_text_kernel (which overwrites these slots with the text's results)
    a.num_edges[g] = tags ? 1 + 3 * tags : 0;                   // tokens taken: <bos> and the triples
    a.num_nodes[g] = max_end;
    a.query[2 * (int64_t)g] = (int32_t)(uint32_t)handover;
    a.query[2 * (int64_t)g + 1] = (int32_t)(handover >> 32);
  }
}

__global__ void __launch_bounds__(256) parse_graph_text_kernel(const ParseArgs a) {
  // the text travels through a 2 KB LDS ring per wave, 16 bytes per lane and load, the chunk after next in flight while
  // the current one is split (a byte per lane straight from HBM, one piece ahead, left the waves waiting for memory half
  // of the time)
  __shared__ __align__(16) uint8_t ring_all[4][kTextRing];
  const int lane = lane_id();
  const int wave = wave_id(), wpb = (int)(blockDim.x >> 6);
  uint8_t *ring = ring_all[wave];
  U8x16a *ring16 = reinterpret_cast<U8x16a *>(ring);
  const int64_t total = a.text_ptr[a.num_texts];
  auto load16 = [&](int64_t abs) -> U8x16 {   // never touches bytes past the end of the blob
    if (abs + 16 <= total) return *reinterpret_cast<const U8x16 *>(a.bytes + abs);
    uint32_t w[4] = {0x20202020u, 0x20202020u, 0x20202020u, 0x20202020u};
    for (int b = 0; b < 16; ++b)
      if (abs + b < total) w[b >> 2] = (w[b >> 2] & ~(0xFFu << (8 * (b & 3)))) | ((uint32_t)a.bytes[abs + b] << (8 * (b & 3)));
    return U8x16{w[0], w[1], w[2], w[3]};
  };
  const bool fill = a.edge_ptr != nullptr;
  const int vb = virtual_block();
  const int u0 = vb * a.upb, u1 = min(a.units, u0 + a.upb);
  for (int unit = u0; unit < u1; ++unit) {
    const int g = unit * wpb + wave;
    if (g >= a.num_texts) break;
    const uint8_t *__restrict__ s = a.bytes + a.text_ptr[g];
    int64_t n = a.text_ptr[g + 1] - a.text_ptr[g];
    const int64_t ebase = fill ? a.edge_ptr[g] : 0;
    const int64_t ecap = fill ? a.edge_ptr[g + 1] - ebase : 0;
    // a token's bytes, read again (tags, label words): out of the ring when they lie in the chunk being split or the one
    // behind it - a byte from HBM per step of these compare loops made them the kernel's time: ~100 dependent loads per text
    int64_t ring_lo = 0;                                          // first byte (of the text as this loop sees it) the ring holds
    auto tb = [&](int64_t i) __attribute__((always_inline)) -> uint32_t { return i >= ring_lo ? (uint32_t)ring[i & (kTextRing - 1)] : (uint32_t)s[i]; };
    auto lit = [&](int64_t i, int len, const char *w, int wl) -> bool {   // token == literal (upper-cased text)
      if (len != wl) return false;
      for (int j = 0; j < wl; ++j) {
        uint32_t c = tb(i + j);
        if (c >= 'a' && c <= 'z') c -= 32;
        if (c != (uint32_t)w[j]) return false;
      }
      return true;
    };
    int count = 0, tn = -1, tq = -1, q_t = -1, p_t = -1, cnt_n = 0, cnt_q = 0, cnt_p = 0;
    int max_end = -1, max_node = -1, nnodes = 0, bad = 0;
    int sd = 0, qu = -1, qv = -1, qu_ok = 0, qv_ok = 0, label = kNoLabel;
    bool prev_sp = true;
    // the token that runs into this piece: decimal value so far, length, "digits only so far"
    uint32_t carry_val = 0; int carry_len = 0; bool carry_dig = true;
    // ---- the edge zone has been streamed by parse_edge_zone_kernel: it left, in this text's output slots, the token count
    // and largest endpoint it reached and the byte where this loop takes over (the first window that holds anything but
    // `INT INT <e>` triples starts there, right behind the last token the stream took)
    count = a.num_edges[g];
    max_end = a.num_nodes[g];
    const int64_t handover = (int64_t)(uint32_t)a.query[2 * (int64_t)g] | ((int64_t)a.query[2 * (int64_t)g + 1] << 32);
    s += handover;                                                  // the general loop sees the rest as a text of its own
    n -= handover;
    const int64_t t0 = a.text_ptr[g] + handover;
    wave_sync();                                                  // the previous text's last reads of the ring are done
    {
      const U8x16 x0 = load16(t0 + lane * 16), x1 = load16(t0 + kTextChunk + lane * 16);
      ring16[lane] = U8x16a{x0.a, x0.b, x0.c, x0.d};
      ring16[64 + lane] = U8x16a{x1.a, x1.b, x1.c, x1.d};
    }
    wave_sync();
    U8x16 nxt = load16(t0 + kTextRing + lane * 16);               // chunk 2: lands while chunk 0 is split
    for (int64_t b0 = 0; b0 < n; b0 += kWave) {
      if (b0 && (b0 & (kTextChunk - 1)) == 0) {                   // chunk b0/1024 - 1 is done: its half takes chunk + 1
        const int64_t cdone = b0 / kTextChunk - 1;
        wave_sync();
        ring16[(cdone & 1) * 64 + lane] = U8x16a{nxt.a, nxt.b, nxt.c, nxt.d};
        wave_sync();
        ring_lo = b0;                                             // chunk cdone is gone from the ring
        nxt = load16(t0 + (cdone + 3) * kTextChunk + lane * 16);
      }
      const int64_t i = b0 + lane;
      const uint32_t c = i < n ? ring[i & (kTextRing - 1)] : 32u;
      const uint32_t cnext = (i + kWave < n) ? ring[(i + kWave) & (kTextRing - 1)] : 32u;   // (lane 0's value: the byte after this piece)
      const bool sp = py_isspace(c);
      const uint64_t spm = __ballot(sp);
      const bool before = lane == 0 ? prev_sp : ((spm >> (lane - 1)) & 1ull);
      const bool after = lane == 63 ? py_isspace((uint32_t)__builtin_amdgcn_readlane((int)cnext, 0)) : ((spm >> (lane + 1)) & 1ull);
      const uint64_t sm = __ballot(!sp && before), em = __ballot(!sp && after);   // token starts / ends
      prev_sp = (spm >> 63) & 1ull;
      if ((~spm) == 0) continue;
      // Integer tokens without a loop per token.  Node ids have at most three digits: the value of the digits of a token
      // that lie in this piece, up to this lane, comes from this byte and the two before it (wave shifts).  A longer run
      // of digits anywhere in the piece (rare) takes the general route: x -> 10 x + digit is an affine map, affine maps
      // compose associatively, so one segmented scan over the lanes (segments = tokens) leaves every token's value at
      // its last byte.  "All digits" is a mask test over the token's lanes.
      const uint64_t le = (2ull << lane) - 1ull;
      const int seg_lo = (sm & le) ? 63 - __builtin_clzll(sm & le) : 0;
      const bool cont = !(sm & le);                                 // began in an earlier piece
      const bool isdig = c >= '0' && c <= '9';
      const uint64_t ndm = __ballot(!sp && !isdig);
      // the two bytes before this one (tags are three bytes long)
      const uint32_t p1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)c, 0x138, 0xf, 0xf, false);    // wave_shr:1
      const uint32_t p2 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)p1, 0x138, 0xf, 0xf, false);
      int len = lane - seg_lo + 1;
      bool alldig = (ndm & le & ~((1ull << seg_lo) - 1ull)) == 0;
      uint32_t m, h;
      if (__ballot(!sp && alldig && len > 3) == 0) {
        const uint32_t d0 = c - '0', d1 = p1 - '0', d2 = p2 - '0';
        h = isdig ? d0 : 0u;
        h += len >= 2 ? 10u * d1 : 0u;
        h += len >= 3 ? 100u * d2 : 0u;
        m = len >= 3 ? 1000u : (len == 2 ? 100u : 10u);
      } else {
        m = 10u; h = isdig ? c - '0' : 0u;
#pragma unroll
        for (int dsh = 1; dsh < kWave; dsh <<= 1) {
          const uint32_t pm = (uint32_t)__builtin_amdgcn_ds_bpermute((lane - dsh) << 2, (int)m);
          const uint32_t ph = (uint32_t)__builtin_amdgcn_ds_bpermute((lane - dsh) << 2, (int)h);
          if (!sp && lane - dsh >= seg_lo) { h = ph * m + h; m = pm * m; }
        }
      }
      if (cont) { h = carry_val * m + h; len += carry_len; alldig = alldig && carry_dig; }
      const bool open = !((spm >> 63) & 1ull) && !((em >> 63) & 1ull);
      carry_val = 0u; carry_len = 0; carry_dig = true;
      if (open) {
        carry_val = (uint32_t)__builtin_amdgcn_readlane((int)h, 63);
        carry_len = __builtin_amdgcn_readlane(len, 63);
        carry_dig = (bool)__builtin_amdgcn_readlane((int)alldig, 63);
      }
      if (em == 0) continue;
      const bool start = (em >> lane) & 1ull;                       // (a token END: the structure code below keys on it)
      const int t = count + __popcll(em & lanemask_lt());
      // ---- the bulk of a text: pieces that lie wholly in the edge zone and hold nothing but integers and <e> tags
      // (whole inside the piece).  One ballot decides; then only the triple check and the two stores remain.
      if (tn < 0) {
        const bool is_e = len == 3 && lane >= 2 && p2 == '<' && p1 == 'e' && c == '>';
        const bool plain = !start || (alldig && len <= 9) || is_e;
        if (__ballot(!plain) == 0 && count > 0) {                  // (token 0 must be <bos>: never plain)
          if (start) {
            const int r = (t - 1) % 3;
            if (is_e != (r == 2)) bad = 1;
            else if (r != 2) {
              max_end = max(max_end, (int)h);
              const int64_t k = (t - 1) / 3;
              if (fill && k < ecap) { if (r == 0) a.src[ebase + k] = (int)h; else a.dst[ebase + k] = (int)h; }
            }
          }
          count += __popcll(em);
          continue;
        }
      }
      // ---- likewise the node list behind <n>: pieces that hold nothing but integers (the list's end - the first token that
      // is not one - is still ahead, so neither <q> nor <p> has been seen)
      if (tn >= 0 && tq < 0 && count > tn) {
        const bool plain = !start || (alldig && len <= 9);
        if (__ballot(!plain) == 0) {
          if (start) { max_node = max(max_node, (int)h); ++nnodes; }
          count += __popcll(em);
          continue;
        }
      }
      int type = T_OTHER, val = (int)h, lab = kNoLabel;
      bool is_sd = false;
      if (start) {
        const int64_t ts = i - len + 1;                             // the token's first byte
        if (alldig) { type = T_INT; if (len > 9) bad = 1; }
        else if (len == 3 && lane >= 2) {                           // a tag inside this piece: bytes are in registers
          if (p2 == '<' && c == '>') type = p1 == 'e' ? T_E : p1 == 'n' ? T_N : p1 == 'q' ? T_Q : p1 == 'p' ? T_P : T_OTHER;
        } else if (tb(ts) == '<') {                                  // <bos> / <eos>, or a tag across two pieces
          if (lit(ts, len, "<E>", 3)) type = T_E;
          else if (lit(ts, len, "<N>", 3)) type = T_N;
          else if (lit(ts, len, "<Q>", 3)) type = T_Q;
          else if (lit(ts, len, "<P>", 3)) type = T_P;
          else if (lit(ts, len, "<BOS>", 5)) type = T_BOS;
          else if (lit(ts, len, "<EOS>", 5)) type = T_EOS;
          // the reference compares these tags case-sensitively: an upper-case variant is not a tag
          if (type != T_OTHER) for (int j = 1; j < len - 1; ++j) if (tb(ts + j) < 'a') type = T_OTHER;
        }
        if (type == T_OTHER && !alldig) {
          is_sd = len == 17;
          if (is_sd) { const char *w = "shortest_distance"; for (int j = 0; j < 17; ++j) is_sd = is_sd && tb(ts + j) == (uint32_t)(uint8_t)w[j]; }
          // label words (reference :80-113, upper-cased): YES / NO / LENk / INF / INFINITY
          if (lit(ts, len, "YES", 3)) lab = 1;
          else if (lit(ts, len, "NO", 2)) lab = 0;
          else if (len > 3 && len <= 12 && lit(ts, 3, "LEN", 3)) {
            int k = 0; bool ok = true;
            for (int j = 3; j < len; ++j) { const uint32_t cj = tb(ts + j); ok = ok && cj >= '0' && cj <= '9'; k = k * 10 + (int)(cj - '0'); }
            if (ok) lab = k - 1; else lab = kNoLabel + 1;     // LEN<junk>: the reference tries the next <p>: not canonical
          }
        }
      }
      const uint64_t sm_tok = em;   // tokens are indexed in END order below
      // ---- structure (token indices are uniform values, token lanes report through ballots / readlane)
      auto first_t = [&](uint64_t m) -> int { return count + __popcll(sm_tok & ((1ull << __builtin_ctzll(m)) - 1ull)); };
      auto lane_of = [&](int tt) -> int {   // start lane of token tt if it starts in this piece, else -1
        const int k = tt - count;
        if (k < 0 || k >= (int)__popcll(sm_tok)) return -1;
        uint64_t m = sm_tok;
        for (int q = 0; q < k; ++q) m &= m - 1;
        return __builtin_ctzll(m);
      };
      const uint64_t nm = __ballot(start && type == T_N), qm = __ballot(start && type == T_Q), pm = __ballot(start && type == T_P);
      cnt_n += __popcll(nm); cnt_q += __popcll(qm); cnt_p += __popcll(pm);
      if (tn < 0 && nm) tn = first_t(nm);
      if (p_t < 0 && pm) p_t = first_t(pm);
      if (tn >= 0 && tq < 0) {
        const uint64_t em = __ballot(start && t > tn && type != T_INT);
        if (em) tq = first_t(em);
      }
      if (start) {
        if (t == 0) { if (type != T_BOS) bad = 1; }
        else if (tn < 0 || t < tn) {                       // edge zone: (INT INT <e>)*
          const int r = (t - 1) % 3;
          if (type != (r == 2 ? T_E : T_INT)) bad = 1;
          else if (r != 2) {
            max_end = max(max_end, val);
            const int64_t k = (t - 1) / 3;
            if (fill && k < ecap) { if (r == 0) a.src[ebase + k] = val; else a.dst[ebase + k] = val; }
          }
        } else if (t > tn && (tq < 0 || t < tq)) {         // node list
          max_node = max(max_node, val); ++nnodes;
        } else if (t == tq) {
          if (type != T_Q && type != T_P && type != T_EOS) bad = 1;
        }
      }
      if (q_t < 0 && qm) q_t = first_t(qm);
      if (q_t >= 0) {                                       // <q> WORD [INT INT]
        int l;
        if ((l = lane_of(q_t + 1)) >= 0) sd = __builtin_amdgcn_readlane((int)is_sd, l);
        if ((l = lane_of(q_t + 2)) >= 0) { qu_ok = __builtin_amdgcn_readlane((int)(type == T_INT), l); qu = __builtin_amdgcn_readlane(val, l); }
        if ((l = lane_of(q_t + 3)) >= 0) { qv_ok = __builtin_amdgcn_readlane((int)(type == T_INT), l); qv = __builtin_amdgcn_readlane(val, l); }
      }
      if (p_t >= 0) {
        const int l = lane_of(p_t + 1);
        if (l >= 0) label = __builtin_amdgcn_readlane(lab, l);
      }
      count += __popcll(sm_tok);
    }
    // wave-wide results
    const uint64_t anybad = __ballot(bad != 0);
    int me = max_end, mn = max_node, nn = nnodes;
    for (int off = 32; off > 0; off >>= 1) {
      me = max(me, __shfl_xor(me, off)); mn = max(mn, __shfl_xor(mn, off)); nn += __shfl_xor(nn, off);
    }
    int status = anybad ? 1 : 0;
    if (tn < 0 || cnt_n != 1 || cnt_q > 1 || cnt_p > 1) status = 1;
    if (tn >= 0 && (tn - 1) % 3 != 0) status = 1;           // an unfinished triple before <n>
    if (q_t >= 0 && q_t != tq) status = 1;                  // <q> somewhere else than right after the node list
    if (label == kNoLabel + 1) status = 1;
    if (lane == 0) {
      const int ne = tn >= 0 ? (tn - 1) / 3 : 0;
      a.num_edges[g] = ne;
      a.num_nodes[g] = nn > 0 ? mn + 1 : (ne > 0 ? me + 1 : 0);
      const bool has_q = q_t >= 0 && sd && qu_ok && qv_ok;
      a.query[2 * (int64_t)g] = has_q ? qu : -1;
      a.query[2 * (int64_t)g + 1] = has_q ? qv : -1;
      a.label[g] = label;
      a.status[g] = status;
    }
  }
}

}  // namespace gtok

using namespace gtok;

extern "C" int gtok_vocab_stats_text(const uint8_t *bytes, const int64_t *text_ptr, int32_t num_texts, int64_t base_offset,
                                     int32_t capacity, uint64_t *key, int64_t *count, int64_t *first, int32_t *len,
                                     int32_t *status, void *stream) {
  gtok::DeviceScope device_scope((hipStream_t)stream);   // the stream's device, not the thread's current one
  if (!device_scope.ok()) return GTOK_E_NO_DEVICE;
  if (num_texts < 0 || capacity < 16 || (capacity & (capacity - 1)) != 0) return GTOK_E_INVAL;
  if (num_texts == 0) return GTOK_OK;
  if (!bytes || !text_ptr || !key || !count || !first || !len || !status) return GTOK_E_INVAL;
  VocabTextArgs a;
  a.bytes = bytes; a.text_ptr = text_ptr; a.num_texts = num_texts; a.base_offset = base_offset; a.capacity = capacity;
  a.key = reinterpret_cast<unsigned long long *>(key); a.count = reinterpret_cast<unsigned long long *>(count);
  a.first = reinterpret_cast<unsigned long long *>(first); a.len = len; a.status = status;
  a.lslots = 512;      // 24 bytes each: four waves per workgroup
  return launch_wave_per_item(vocab_stats_text_kernel, a, num_texts, 4, a.lslots * 24, device_scope.dev, (hipStream_t)stream);
}

extern "C" int gtok_text_to_ids(const uint8_t *bytes, const int64_t *text_ptr, int32_t num_texts,
                                const gtok_vocab_table *vocab, int32_t strip_label, int32_t max_len,
                                int32_t *out_ids, int32_t ld, int32_t *out_len, void *stream) {
  gtok::DeviceScope device_scope((hipStream_t)stream);   // the stream's device, not the thread's current one
  if (!device_scope.ok()) return GTOK_E_NO_DEVICE;
  if (!vocab || num_texts < 0 || max_len < 0 || ld <= 0) return GTOK_E_INVAL;
  if (vocab->capacity <= 0 || (vocab->capacity & (vocab->capacity - 1)) || !vocab->key_off ||
      !vocab->key_len || !vocab->id || !vocab->key_bytes)
    return GTOK_E_INVAL;
  if (num_texts == 0) return GTOK_OK;
  if (!bytes || !text_ptr || !out_ids || !out_len) return GTOK_E_INVAL;
  TextArgs a;
  a.bytes = bytes; a.text_ptr = text_ptr; a.num_texts = num_texts; a.v = *vocab;
  a.strip_label = strip_label; a.pad_id = vocab->pad_id; a.max_len = max_len;
  a.cap = max_len < ld ? max_len : ld;
  const bool vlds = vocab->capacity <= 1024;   // 24 KB of slots per workgroup
  a.off_vocab = 0;
  a.off_short = (vlds ? align_up(vocab->capacity * kSlotBytes, 16) : 0) + 16;   // + scratch words for the staging passes
  // the short-key table is made sparser than the vocab table while the workgroup's LDS stays under 40 KB of tables: a token's
  // look-up is a chain of dependent LDS reads, and a wave waits for the longest chain among its lanes.  A vocab too large for
  // LDS still gets a short-key table (2048 slots: its first thousand short keys)
  a.short_slots = vlds ? vocab->capacity : 2048;
  while (vlds && a.short_slots < 2048 && a.short_slots < 8 * vocab->capacity && a.off_short + 2 * a.short_slots * 16 <= 40 * 1024) a.short_slots *= 2;
  a.off_wave = a.off_short + a.short_slots * 16;
  a.ring_off = 0;
  a.tok_off = kTextRing;
  a.sidx_off = kTextRing;                     // (ids go straight to the output row: no token staging in LDS)
  a.wave_stride = a.sidx_off + 512;
  const int wpb = 8;        // the LDS tables are per workgroup: more waves share one copy (and one set-up)
  // The workgroup stays under 64 KB whatever the vocab (no opt-in, no size to refuse): off_wave <= 1024 * 24 + 16 + 1024 * 16 = 40,976 for a vocab in
  // LDS (its short-key table is doubled only while it ends by 40 KB) and 16 + 2048 * 16 for one outside
  const size_t lds = (size_t)a.off_wave + (size_t)wpb * a.wave_stride;
  assert(lds <= 61456);   // 40,976 + 8 x (kTextRing + 512)
  typedef void (*K)(const TextArgs);
  K kern = vlds ? (K)text_ids_kernel<true> : (K)text_ids_kernel<false>;
  const Grid G = plan_grid(reinterpret_cast<const void *>(kern), device_scope.dev, num_texts, wpb, lds, Resident::Blocks);
  a.out = out_ids; a.ld = ld; a.out_len = out_len; a.units = G.units; a.upb = G.upb;
  hipLaunchKernelGGL(kern, dim3(G.nb), dim3(wpb * 64), lds, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? GTOK_OK : GTOK_E_LAUNCH;
}

extern "C" int gtok_count_edge_tokens(const uint8_t *bytes, const int64_t *text_ptr, int32_t num_texts, int32_t *num_edges,
                                      void *stream) {
  gtok::DeviceScope device_scope((hipStream_t)stream);   // the stream's device, not the thread's current one
  if (!device_scope.ok()) return GTOK_E_NO_DEVICE;
  if (num_texts < 0) return GTOK_E_INVAL;
  if (num_texts == 0) return GTOK_OK;
  if (!bytes || !text_ptr || !num_edges) return GTOK_E_INVAL;
  hipLaunchKernelGGL(count_edge_tokens_kernel, dim3((num_texts + 3) / 4), dim3(256), 0, (hipStream_t)stream, bytes, text_ptr, num_texts, num_edges);
  return hipGetLastError() == hipSuccess ? GTOK_OK : GTOK_E_LAUNCH;
}

extern "C" int gtok_parse_graph_text(const uint8_t *bytes, const int64_t *text_ptr, int32_t num_texts,
                                     const int64_t *edge_ptr, int32_t *src, int32_t *dst, int32_t *num_edges,
                                     int32_t *num_nodes, int32_t *query_nodes, int32_t *label, int32_t *status,
                                     void *stream) {
  gtok::DeviceScope device_scope((hipStream_t)stream);   // the stream's device, not the thread's current one
  if (!device_scope.ok()) return GTOK_E_NO_DEVICE;
  if (num_texts < 0) return GTOK_E_INVAL;
  if (num_texts == 0) return GTOK_OK;
  if (!bytes || !text_ptr || !num_edges || !num_nodes || !query_nodes || !label || !status) return GTOK_E_INVAL;
  if (edge_ptr && (!src || !dst)) return GTOK_E_INVAL;
  ParseArgs a;
  a.bytes = bytes; a.text_ptr = text_ptr; a.num_texts = num_texts; a.edge_ptr = edge_ptr; a.src = src; a.dst = dst;
  a.num_edges = num_edges; a.num_nodes = num_nodes; a.query = query_nodes; a.label = label; a.status = status;
  const Grid G = plan_grid(reinterpret_cast<const void *>(parse_graph_text_kernel), device_scope.dev, num_texts, 4, 0, Resident::Blocks);
  a.units = G.units; a.upb = G.upb;
  hipLaunchKernelGGL(parse_edge_zone_kernel, dim3((num_texts + 3) / 4), dim3(256), 0, (hipStream_t)stream, a);
  if (hipGetLastError() != hipSuccess) return GTOK_E_LAUNCH;
  hipLaunchKernelGGL(parse_graph_text_kernel, dim3(G.nb), dim3(256), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? GTOK_OK : GTOK_E_LAUNCH;
}
