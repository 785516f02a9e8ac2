// gtok_ibtt.hip — index-based serialisers (IBTT) for gfx950.
//
//   ibtt_zinc_kernel   graph_data_loader/zinc_dataset_indexbase.py:143-227 fused with
//                      graph_data_loader/data_loader.py:465-484: CSR -> vocab ids, no strings
//   ibtt_synth_kernel  docs/synthetic_data.md:46-68 grammar + data_loader.py:479-482
//   vocab_stats_synth_kernel  the node-id token statistics of the synthetic grammar's texts, from the CSR
// (everything that reads text: gtok_text.hip; remap / collate / find over a slab: gtok_rows.hip)
//
// One wavefront per graph (ibtt_zinc_lane_kernel: a lane, ibtt_zinc_quad_kernel: 8 or 16 lanes), LDS-staged, closed-form
// token positions so every lane writes its own tokens; rows leave through write_row() as 16-byte
// stores.  Bit-exact checkers: oracle/gtok_oracle.c.  The launchers are at the end: one function per gtok_ibtt_zinc kernel.
#include <cstdlib>

#include "gtok_common.hpp"   // (and gtok.h)

namespace gtok {

// largest u in [0, n) with rp[u] <= k (rp in LDS, rp[n] > k guaranteed)
__device__ __forceinline__ int row_of(const int32_t *rp, int n, int k) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rp[mid] <= k) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---------------------------------------------------------------------------------------------
// IBTT molecular serialiser
// ---------------------------------------------------------------------------------------------
struct ZincLds { int rp, cc, co, ou, ov, oa, tok, stride; };
struct ZincArgs {
  gtok_csr g;
  const int32_t *lut;
  int lut_len, max_len, pad_id, maxn, maxe, tcap;
  ZincLds l;
  int32_t *out; int ld; int32_t *out_len;
  int units, upb;
};

__global__ void __launch_bounds__(256) ibtt_zinc_kernel(const ZincArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id();
  const int wave = wave_id(), wpb = (int)(blockDim.x >> 6);
  unsigned char *base = smem + (size_t)wave * a.l.stride;
  int32_t *rp = reinterpret_cast<int32_t *>(base + a.l.rp);
  uint16_t *cc = reinterpret_cast<uint16_t *>(base + a.l.cc);  // col, CSR position
  uint16_t *co = reinterpret_cast<uint16_t *>(base + a.l.co);  // original position, CSR position
  uint16_t *ou = reinterpret_cast<uint16_t *>(base + a.l.ou);  // src by original position
  uint16_t *ov = reinterpret_cast<uint16_t *>(base + a.l.ov);  // dst by original position
  uint8_t *oa = base + a.l.oa;                                  // edge_attr by original position
  int32_t *tok = reinterpret_cast<int32_t *>(base + a.l.tok);
  const int32_t *__restrict__ lut = a.lut;
  const int pad = a.pad_id, tcap = a.tcap;
  const bool has_order = a.g.eorder != nullptr, has_ea = a.g.eattr != nullptr, has_na = a.g.nattr != nullptr;

  auto put = [&](int q, int v) { if (q < tcap) tok[q] = v; };
  auto node_id = [&](int i) { return (GTOK_ZLUT_NODE0 + i < a.lut_len) ? lut[GTOK_ZLUT_NODE0 + i] : pad; };

  // Software pipeline (the kernel is latency-bound: ~570 instructions per molecule behind four dependent
  // memory round trips): scalar pointers of graph i+2 and the per-lane head of graph i+1 — first 64 row
  // pointers / node types, first 128 entries — are requested before graph i is serialised.
  struct Ptrs { int n0, n1; int64_t e0, e1; };
  struct Data { int rp, x, c0, c1, p0, p1, a0, a1; };
  auto load_ptrs = [&](int g) -> Ptrs {
    Ptrs p;
    p.n0 = sload(a.g.node_ptr, g); p.n1 = sload(a.g.node_ptr, g + 1);
    p.e0 = sload(a.g.edge_ptr, g); p.e1 = sload(a.g.edge_ptr, g + 1);
    return p;
  };
  auto load_data = [&](int g, const Ptrs &p) -> Data {
    Data q = {0, 255, 0, 0, 0, 0, 0, 0};
    const int pn = p.n1 - p.n0, pe = (int)(p.e1 - p.e0);
    if (lane <= pn) q.rp = a.g.rowptr[p.n0 + g + lane];
    if (has_na && lane < pn) q.x = a.g.nattr[p.n0 + lane];
    if (lane < pe) {
      q.c0 = a.g.col[p.e0 + lane];
      q.p0 = has_order ? a.g.eorder[p.e0 + lane] : lane;
      if (has_ea) q.a0 = a.g.eattr[p.e0 + lane];
    }
    if (lane + 64 < pe) {
      q.c1 = a.g.col[p.e0 + lane + 64];
      q.p1 = has_order ? a.g.eorder[p.e0 + lane + 64] : lane + 64;
      if (has_ea) q.a1 = a.g.eattr[p.e0 + lane + 64];
    }
    return q;
  };

  const int vb = virtual_block();
  const int u0 = vb * a.upb, u1 = min(a.units, u0 + a.upb);
  const int G = a.g.num_graphs;
  int g = u0 * wpb + wave;
  if (u0 >= u1 || g >= G) return;
  Ptrs pc = load_ptrs(g);
  Data dc = load_data(g, pc);
  bool has_next = (u0 + 1 < u1) && (g + wpb < G);
  Ptrs pn = pc;
  if (has_next) pn = load_ptrs(g + wpb);
  for (int unit = u0;; ++unit) {
    Data dn = dc;
    if (has_next) dn = load_data(g + wpb, pn);
    const bool has_next2 = (unit + 2 < u1) && (g + 2 * wpb < G);
    Ptrs pnn = pn;
    if (has_next2) pnn = load_ptrs(g + 2 * wpb);

    const int nb0 = pc.n0;
    const int n = min(pc.n1 - pc.n0, a.maxn);
    const int64_t e0 = pc.e0;
    const int e = min((int)(pc.e1 - pc.e0), a.maxe);
    const int32_t *__restrict__ rpg = a.g.rowptr + nb0 + g;

    if (lane <= n) rp[lane] = dc.rp;
    for (int i = lane + kWave; i <= n; i += kWave) rp[i] = rpg[i];   // more than 63 nodes: the rest, not prefetched
    wave_sync();
    // CSR entry k = (u, v, attr) listed at original position p: scatter back to COO order
    auto scatter = [&](int k, int v, int p, int at) {
      const int u = row_of(rp, n, k);
      cc[k] = (uint16_t)v; co[k] = (uint16_t)p;
      if ((unsigned)p < (unsigned)e) { ou[p] = (uint16_t)u; ov[p] = (uint16_t)v; oa[p] = (uint8_t)at; }
    };
    if (lane < e) scatter(lane, dc.c0, dc.p0, dc.a0);
    if (lane + 64 < e) scatter(lane + 64, dc.c1, dc.p1, dc.a1);
    for (int k = lane + 128; k < e; k += kWave)
      scatter(k, a.g.col[e0 + k], has_order ? a.g.eorder[e0 + k] : k, has_ea ? a.g.eattr[e0 + k] : 0);
    wave_sync();
    // zinc_dataset_indexbase.py:176-184: keep entry p iff no earlier entry joins the same {u,v}
    int kept = 0;
    for (int b0 = 0; b0 < e; b0 += kWave) {
      const int p = b0 + lane;
      bool keep = false;
      int u = 0, v = 0, at = 0;
      if (p < e) {
        u = ou[p]; v = ov[p]; at = oa[p];
        keep = true;
        if (u < n && v < n) {
          for (int j = rp[u], je = rp[u + 1]; j < je; ++j) keep = keep && !(cc[j] == v && co[j] < p);
          for (int j = rp[v], je = rp[v + 1]; j < je; ++j) keep = keep && !(cc[j] == u && co[j] < p);
        }
      }
      const uint64_t m = __ballot(keep);
      if (keep) {
        const int q = 1 + 2 * n + 4 * (kept + __popcll(m & lanemask_lt()));
        put(q, lut[GTOK_ZLUT_BOND]);
        put(q + 1, lut[GTOK_ZLUT_BOND0 + ((at >= 1 && at <= 4) ? at : 0)]);
        put(q + 2, node_id(u));
        put(q + 3, node_id(v));
      }
      kept += __popcll(m);
    }
    auto put_atom = [&](int i, int x) {   // :168-169, 'X' for x outside 0..8 (:104)
      put(1 + 2 * i, lut[GTOK_ZLUT_ATOM]);
      put(2 + 2 * i, lut[GTOK_ZLUT_ATOM0 + (x <= 8 ? x : 9)]);
    };
    if (lane < n) put_atom(lane, dc.x);
    for (int i = lane + kWave; i < n; i += kWave) put_atom(i, has_na ? a.g.nattr[nb0 + i] : 255);
    const int64_t T = 6 + 2 * (int64_t)n + 4 * (int64_t)kept;  // text tokens incl. label and <eos>
    if (lane == 0) {
      put(0, lut[GTOK_ZLUT_BOS]);
      const int q = 1 + 2 * n + 4 * kept;
      put(q, lut[GTOK_ZLUT_Q]); put(q + 1, lut[GTOK_ZLUT_REGRESSION]); put(q + 2, lut[GTOK_ZLUT_P]);
    }
    wave_sync();
    int len;
    if (T <= (int64_t)a.max_len + 1) {
      len = (int)(T - 2);  // everything up to and including <p> (data_loader.py:479-481)
    } else {               // :217-221 tokens[:max_len-1] + ['<eos>'], <p> was cut off
      len = a.max_len;
      if (lane == 0 && a.max_len >= 1) put(a.max_len - 1, lut[GTOK_ZLUT_EOS]);
      wave_sync();
    }
    write_row(a.out + (int64_t)g * a.ld, a.ld, min(len, min(a.ld, tcap)), pad, [=](int i) -> int { return tok[i]; });
    if (lane == 0) a.out_len[g] = len;
    wave_sync();
    if (!has_next) break;
    g += wpb;
    pc = pn; dc = dn; pn = pnn;
    has_next = has_next2;
  }
}

// ---------------------------------------------------------------------------------------------
// IBTT molecular serialiser, LANE per graph (64 molecules per wave)
// ---------------------------------------------------------------------------------------------
// For batches the host verified as simple + symmetric (GTOK_CSR_SIMPLE_SYMMETRIC) whose entries are already
// in edge_index order (eorder == NULL): the pair {u,v} is listed exactly twice, u->v in row u and v->u in row
// v, and row order is list order, so "first occurrence wins" (zinc_dataset_indexbase.py:176-184) keeps exactly
// the entries with u <= v.  Each lane then streams its own molecule: <bos>, 2 tokens per atom, one 16-byte
// store per kept bond (<bond> TYPE u v), the 3-token tail — ~40 instructions per molecule instead of ~570.
// The wave's 64 molecules are one contiguous CSR chunk, staged in LDS with 16-byte loads (as in
// gtok_sent_lane.hpp); the LUT sits in LDS too.  Bond types are staged as NIBBLES (min(type, 15): the grammar
// only tells types 1..4 from "anything else"), which brings a ZINC wave to <= 10 KB of LDS = 16 waves per CU =
// 4096 resident waves, more than ZINC-full's 3898 units: the whole corpus runs in ONE round (the kernel is
// bound by per-unit latency, so a second, 2 %-full round used to double its time).  Units beyond the resident
// waves are drawn from the ticket queues.  Same ids as ibtt_zinc_kernel, same oracle.
struct ZincLaneArgs {
  gtok_csr g;
  const int32_t *lut;
  int lut_len, max_len, pad_id;
  int off_rp, off_col, off_eat, off_nat, off_lut, lds;   // byte offsets of the wave's staging areas
  int cap_r, cap_n, cap_e;
  int32_t *out; int ld; int32_t *out_len;
  int units;
  int *queue;   // ticket counter block (gtok_common.hpp: Tickets)
};

// 4 type bytes -> 4 nibbles (16 bits), each min(byte, 15)
__device__ __forceinline__ uint32_t nibbles4(uint32_t x) {
  uint32_t hi = x & 0xF0F0F0F0u;
  hi |= hi >> 1; hi |= hi >> 2;                       // any high bit set -> whole high nibble set
  uint32_t y = (x | (hi >> 4)) & 0x0F0F0F0Fu;           // saturate
  y = (y | (y >> 4)) & 0x00FF00FFu;
  return (y | (y >> 8)) & 0xFFFFu;
}

// <= 128 VGPRs: 4 waves per SIMD, so that LDS (<= 10 KB) and not registers sets the 16 waves per CU
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) ibtt_zinc_lane_kernel(const ZincLaneArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id();
  const bool lane0 = lane == 0;
  uint8_t *srp = smem + a.off_rp, *scol = smem + a.off_col, *seat = smem + a.off_eat, *snat = smem + a.off_nat;
  int32_t *slut = reinterpret_cast<int32_t *>(smem + a.off_lut);
  const int ld = a.ld, cap = min(a.max_len, ld), pad = a.pad_id, G = a.g.num_graphs;
  const bool has_ea = a.g.eattr != nullptr, has_na = a.g.nattr != nullptr;

  for (int i = lane; i < a.lut_len; i += kWave) slut[i] = a.lut[i];
  Tickets tickets;
  tickets.init(a.queue, (int)blockIdx.x, (int)gridDim.x, a.units);
  int unit = (int)blockIdx.x;
  while (unit < a.units) {
    const int ticket = tickets.draw(lane0);
    const int g0 = unit * 64, g = g0 + lane, gl = min(g0 + 64, G);
    const bool valid = g < G;
    const int N0 = sload(a.g.node_ptr, g0), N1 = sload(a.g.node_ptr, gl);
    const int64_t E0 = sload(a.g.edge_ptr, g0), E1 = sload(a.g.edge_ptr, gl);
    int nb0 = N0, n = 0, e = 0;
    int64_t e0 = E0;
    if (valid) {
      nb0 = a.g.node_ptr[g]; n = a.g.node_ptr[g + 1] - nb0;
      e0 = a.g.edge_ptr[g]; e = (int)(a.g.edge_ptr[g + 1] - e0);
    }
    __builtin_amdgcn_wave_barrier();   // the previous unit's lanes are done reading the staging areas
    {  // stage the chunk: 16 bytes per lane and load, every first-pass load issued before the first wait
      const int cr = min((N1 - N0) + (gl - g0), a.cap_r);
      const int ce = (int)min(E1 - E0, (int64_t)a.cap_e);
      const int cn = min(N1 - N0, a.cap_n);
      const int32_t *__restrict__ rpc = a.g.rowptr + N0 + g0;
      const int32_t *__restrict__ cc = a.g.col + E0;
      const uint8_t *__restrict__ ec = has_ea ? a.g.eattr + E0 : nullptr;
      const uint8_t *__restrict__ nc = has_na ? a.g.nattr + N0 : nullptr;
      const I32x4 *rpv = reinterpret_cast<const I32x4 *>(rpc), *ccv = reinterpret_cast<const I32x4 *>(cc);
      const U8x16 *ecv = reinterpret_cast<const U8x16 *>(ec), *ncv = reinterpret_cast<const U8x16 *>(nc);
      uint32_t *srp4 = reinterpret_cast<uint32_t *>(srp), *scol4 = reinterpret_cast<uint32_t *>(scol);
      uint2 *seat8 = reinterpret_cast<uint2 *>(seat);
      U8x16a *snat16 = reinterpret_cast<U8x16a *>(snat);
      const int nrv = cr >> 2, ncv4 = ce >> 2, nev = ce >> 4, nnv = cn >> 4;
      auto pack4 = [](const I32x4 &v) -> uint32_t {
        return ((uint32_t)v.x & 255u) | (((uint32_t)v.y & 255u) << 8) | (((uint32_t)v.z & 255u) << 16) | ((uint32_t)v.w << 24);
      };
      auto nib16 = [](const U8x16 &x) -> uint2 {
        return make_uint2(nibbles4(x.a) | (nibbles4(x.b) << 16), nibbles4(x.c) | (nibbles4(x.d) << 16));
      };
      constexpr int UR = 4, UC = 8, UE = 4, UN = 2;   // vectors in flight per lane
      I32x4 rv[UR], cv[UC];
      U8x16 ev[UE], nv[UN];
#pragma unroll
      for (int j = 0; j < UR; ++j) { const int t = lane + j * kWave; rv[j] = t < nrv ? rpv[t] : I32x4{0, 0, 0, 0}; }
#pragma unroll
      for (int j = 0; j < UE; ++j) { const int t = lane + j * kWave; ev[j] = (has_ea && t < nev) ? ecv[t] : U8x16{0, 0, 0, 0}; }
#pragma unroll
      for (int j = 0; j < UN; ++j) { const int t = lane + j * kWave; nv[j] = (has_na && t < nnv) ? ncv[t] : U8x16{~0u, ~0u, ~0u, ~0u}; }
#pragma unroll
      for (int j = 0; j < UC; ++j) { const int t = lane + j * kWave; cv[j] = t < ncv4 ? ccv[t] : I32x4{0, 0, 0, 0}; }
#pragma unroll
      for (int j = 0; j < UR; ++j) { const int t = lane + j * kWave; if (t < nrv) srp4[t] = pack4(rv[j]); }
#pragma unroll
      for (int j = 0; j < UE; ++j) { const int t = lane + j * kWave; if (t < nev) seat8[t] = nib16(ev[j]); }
#pragma unroll
      for (int j = 0; j < UN; ++j) { const int t = lane + j * kWave; if (t < nnv) snat16[t] = U8x16a{nv[j].a, nv[j].b, nv[j].c, nv[j].d}; }
#pragma unroll
      for (int j = 0; j < UC; ++j) { const int t = lane + j * kWave; if (t < ncv4) scol4[t] = pack4(cv[j]); }
      // chunks longer than the vectors in flight (not molecules), then the last < 4 / < 16 elements of each array
      for (int t = lane + UR * kWave; t < nrv; t += kWave) srp4[t] = pack4(rpv[t]);
      for (int t = lane + UC * kWave; t < ncv4; t += kWave) scol4[t] = pack4(ccv[t]);
      for (int t = lane + UE * kWave; t < nev; t += kWave) seat8[t] = has_ea ? nib16(ecv[t]) : make_uint2(0u, 0u);
      for (int t = lane + UN * kWave; t < nnv; t += kWave) {
        const U8x16 x = has_na ? ncv[t] : U8x16{~0u, ~0u, ~0u, ~0u};
        snat16[t] = U8x16a{x.a, x.b, x.c, x.d};
      }
      if (lane < (cr & 3)) srp[(nrv << 2) + lane] = (uint8_t)rpc[(nrv << 2) + lane];
      if (lane < (ce & 3)) scol[(ncv4 << 2) + lane] = (uint8_t)cc[(ncv4 << 2) + lane];
      if (lane < (cn & 15)) snat[(nnv << 4) + lane] = has_na ? nc[(nnv << 4) + lane] : (uint8_t)255;
      {  // last < 16 bond types: one per lane, even lanes pair theirs with the right neighbour's
        const int rest = ce & 15;
        uint32_t x = (has_ea && lane < rest) ? (uint32_t)ec[(nev << 4) + lane] : 0u;
        x = x > 15u ? 15u : x;
        const uint32_t right = (uint32_t)__shfl_down((int)x, 1);
        if (lane < rest && !(lane & 1)) seat[(nev << 3) + (lane >> 1)] = (uint8_t)(x | (right << 4));
      }
    }
    wave_sync();
    const uint8_t *rpl = srp + (nb0 - N0) + lane, *cl = scol + (int)(e0 - E0), *nl = snat + (nb0 - N0);
    const int eo = (int)(e0 - E0);   // this lane's first entry inside the chunk (nibble index)
    int32_t *__restrict__ orow = a.out + (int64_t)g * ld;
    auto node_id = [&](int i) { return (GTOK_ZLUT_NODE0 + i < a.lut_len) ? slut[GTOK_ZLUT_NODE0 + i] : pad; };

    int pos = 0, len = 0;
    if (valid) {
      if (pos < cap) orow[pos] = slut[GTOK_ZLUT_BOS];
      pos = 1;
      const int t_atom = slut[GTOK_ZLUT_ATOM];
      for (int i = 0; i < n; ++i) {   // :168-169, 'X' for x outside 0..8 (:104)
        const int x = nl[i];
        if (pos < cap) orow[pos] = t_atom;
        if (pos + 1 < cap) orow[pos + 1] = slut[GTOK_ZLUT_ATOM0 + (x <= 8 ? x : 9)];
        pos += 2;
      }
      const int t_bond = slut[GTOK_ZLUT_BOND];
      int u = 0, row_end = n > 0 ? (int)rpl[1] : 0;
      for (int k = 0; k < e; ++k) {
        while (k >= row_end && u + 1 < n) { ++u; row_end = rpl[u + 1]; }
        const int v = cl[k];
        if (u <= v) {   // first occurrence of {u,v}: zinc_dataset_indexbase.py:176-184
          const int at = (seat[(eo + k) >> 1] >> (((eo + k) & 1) << 2)) & 15;
          const int t1 = slut[GTOK_ZLUT_BOND0 + ((at >= 1 && at <= 4) ? at : 0)], t2 = node_id(u), t3 = node_id(v);
          if (pos + 3 < cap) {
            *reinterpret_cast<int4 *>(orow + pos) = make_int4(t_bond, t1, t2, t3);   // dword-aligned 16-byte store
          } else {
            if (pos < cap) orow[pos] = t_bond;
            if (pos + 1 < cap) orow[pos + 1] = t1;
            if (pos + 2 < cap) orow[pos + 2] = t2;
          }
          pos += 4;
        }
      }
      if (pos < cap) orow[pos] = slut[GTOK_ZLUT_Q];
      if (pos + 1 < cap) orow[pos + 1] = slut[GTOK_ZLUT_REGRESSION];
      if (pos + 2 < cap) orow[pos + 2] = slut[GTOK_ZLUT_P];
      const int64_t T = (int64_t)pos + 5;   // text tokens incl. label and <eos>
      if (T <= (int64_t)a.max_len + 1) {
        len = (int)(T - 2);
      } else {                               // :217-221 tokens[:max_len-1] + ['<eos>']
        len = a.max_len;
        if (a.max_len >= 1 && a.max_len - 1 < ld) orow[a.max_len - 1] = slut[GTOK_ZLUT_EOS];
      }
      a.out_len[g] = len;
    }
    {  // pad the tails of the unit's 64 rows: four rows per pass, 16 lanes x 16-byte stores on each
      const int lw = min(len, ld), q = lane & 15;
      for (int it = 0; it < 16; ++it) {
        const int r = it * 4 + (lane >> 4);
        const int lr = __builtin_amdgcn_ds_bpermute(r << 2, lw);
        if (g0 + it * 4 >= G) break;
        if (g0 + r < G) {
          int32_t *__restrict__ row = a.out + (int64_t)(g0 + r) * ld + lr;
          const int nrem = ld - lr, nvec = nrem >> 2;
          for (int t = q; t < nvec; t += 16) reinterpret_cast<I32x4 *>(row)[t] = I32x4{pad, pad, pad, pad};
          if (q < (nrem & 3)) row[(nvec << 2) + q] = pad;
        }
      }
    }
    unit = tickets.settle(ticket, lane0);
  }
  tickets.retire(lane0, lane, (int)gridDim.x);
}

// ---------------------------------------------------------------------------------------------
// IBTT molecular serialiser, SIXTEEN LANES per graph (4 molecules per wave)
// ---------------------------------------------------------------------------------------------
// Same precondition as the lane kernel (GTOK_CSR_SIMPLE_SYMMETRIC, list order: keep iff u <= v), but a DPP row of
// 16 lanes shares one molecule, so every memory access is coalesced and no CSR data is staged at all:
//   rows     lane = node: row pointers straight from global; each node writes its id over its entry range
//            of a small LDS buffer (the entry -> row map; molecules have <= 4 entries per row)
//   atoms    lane = node: one 8-byte store (<atom> TYPE); 16 lanes = 128 contiguous bytes
//   bonds    lane = entry: neighbour id and bond type straight from global (64 / 16 contiguous bytes per
//            group), row from the LDS map, kept entries ranked with one wave ballot, one 16-byte store each
//   tail/pad the group's first lane writes the 3-token tail; all 16 pad the row with 16-byte stores
// A unit (4 molecules) is ~300 instructions and a few microseconds, so the grid is thousands of units deep and
// neither round quantisation nor per-unit latency matters (the lane kernel's unit is 64 molecules and ~100 us).
struct ZincQuadArgs {
  gtok_csr g;
  const int32_t *lut;
  int lut_len, max_len, pad_id;
  int off_map, off_lut, off_row, lds;   // LDS: entry -> row map u16 [4][maxe], LUT, (ROWS) int32 [4][ld]
  int maxe;
  int32_t *out; int ld; int32_t *out_len;
  int units, upb;
};

// ROWS: the unit's four rows are assembled in LDS and leave as whole 16-byte-per-lane, 1 KB-per-instruction
// stores with the padding merged in (the rows are adjacent in the slab): every line is written once, in full.
// Without it (slabs too wide for LDS) tokens and padding go out as they are produced, in 100-250 byte pieces,
// and the store stream is twice as expensive (measured 0.068 vs 0.035 ms for ZINC-full's 240 MB slab).
// GS = lanes per molecule (16 or 8): 64 / GS molecules per wave.  Eight lanes halve the instructions per molecule
// (a molecule's ~50 entries fill 7 passes of 8 lanes instead of 4 passes of 16 with a third of the lanes idle) as
// long as the molecules are small; NP / EP = node / entry passes whose loads travel through the register pipeline.
// PK: row pointers and neighbour ids come from the batch's byte mirror (gtok_csr.rowptr8 / col8): a quarter of the index bytes
template <bool ROWS, int GS, bool PK>
__global__ void __launch_bounds__(64) ibtt_zinc_quad_kernel(const ZincQuadArgs a) {
  constexpr int NG = kWave / GS, NP = GS == 16 ? 4 : 6, EP = GS == 16 ? 8 : 12;
  constexpr uint32_t kGroupBits = (1u << GS) - 1u;
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id(), grp = lane / GS, ql = lane % GS;
  uint16_t *rmap = reinterpret_cast<uint16_t *>(smem + a.off_map) + grp * a.maxe;
  int32_t *slut = reinterpret_cast<int32_t *>(smem + a.off_lut);
  int32_t *srow = reinterpret_cast<int32_t *>(smem + a.off_row);
  const int ld = a.ld, cap = min(a.max_len, ld), pad = a.pad_id, G = a.g.num_graphs;
  const bool has_ea = a.g.eattr != nullptr, has_na = a.g.nattr != nullptr;
  for (int i = lane; i < a.lut_len; i += kWave) slut[i] = a.lut[i];
  wave_sync();
  const int t_atom = slut[GTOK_ZLUT_ATOM], t_bond = slut[GTOK_ZLUT_BOND];
  auto node_id = [&](int i) { return (GTOK_ZLUT_NODE0 + i < a.lut_len) ? slut[GTOK_ZLUT_NODE0 + i] : pad; };

  // Software pipeline over the block's units: a unit's loads form a chain header -> (row pointers, types,
  // neighbour ids), and vmcnt retires in order, so loads issued behind the previous unit's row stores wait for
  // them.  The header of unit+2 and the data of unit+1 are therefore requested BEFORE unit's rows are stored;
  // in steady state a unit finds everything it needs in registers.  The first 64 atoms / 128 entries of a
  // molecule travel this way (unconditional loads at clamped, always-valid indices: one basic block, all in
  // flight together); longer molecules finish with plain loops.
  const int64_t Etot = sload(a.g.edge_ptr, G);
  const int Ntot = sload(a.g.node_ptr, G);
  const bool ld_na = has_na && Ntot > 0, ld_ea = has_ea && Etot > 0, ld_col = Etot > 0;
  struct Hdr { int nb0, n, e; int64_t e0; };
  struct Dat { int rs[NP], re[NP], x[NP], v[EP], at[EP]; };
  const int vb = virtual_block();
  const int u0 = vb * a.upb, u1 = min(a.units, u0 + a.upb);
  auto load_hdr = [&](int unit) -> Hdr {
    Hdr h{0, 0, 0, 0};
    const int g = unit * NG + grp;
    if (unit < u1 && g < G) {
      h.nb0 = a.g.node_ptr[g]; h.n = a.g.node_ptr[g + 1] - h.nb0;
      h.e0 = a.g.edge_ptr[g]; h.e = min((int)(a.g.edge_ptr[g + 1] - h.e0), a.maxe);
    }
    return h;
  };
  auto load_dat = [&](int unit, const Hdr &h) -> Dat {
    Dat d;
    const bool live = unit < u1 && unit * NG + grp < G;
    const int g = live ? unit * NG + grp : 0;                                  // idle groups read graph 0's first words
    // every address is a wave-uniform base (scalar registers) + an unsigned 32-bit lane offset: one or two vector
    // instructions per load instead of a 64-bit clamp and add (the unit's groups are consecutive graphs, so their
    // entry ranges start within 2^31 of the first group's)
    const uint32_t rb = (uint32_t)(h.nb0 + g);                                  // this group's row pointers (node_ptr + graph index)
    const uint32_t nlast = (uint32_t)max(h.nb0 + h.n - 1, 0);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int i = ql + GS * j;
      const uint32_t i0 = rb + (uint32_t)min(i, h.n), i1 = rb + (uint32_t)min(i + 1, h.n);
      d.rs[j] = PK ? (int)a.g.rowptr8[i0] : a.g.rowptr[i0];
      d.re[j] = PK ? (int)a.g.rowptr8[i1] : a.g.rowptr[i1];
      d.x[j] = ld_na ? (int)a.g.nattr[min(min((uint32_t)h.nb0 + (uint32_t)i, nlast), (uint32_t)(Ntot - 1))] : 255;
    }
    const int64_t ebase = max(min((int64_t)uni((uint64_t)h.e0), Etot - 1), (int64_t)0);   // group 0's first entry, inside the array (0 for an idle unit)
    const uint32_t ehi = (uint32_t)min(Etot - 1 - ebase, (int64_t)0x7fffffff);  // last readable entry behind the base
    const uint8_t *__restrict__ c8 = PK ? a.g.col8 + ebase : nullptr;
    const int32_t *__restrict__ c32 = a.g.col + ebase;
    const uint8_t *__restrict__ ea = a.g.eattr + ebase;
    const int erel = live ? (int)(h.e0 - ebase) : 0;
#pragma unroll
    for (int j = 0; j < EP; ++j) {
      const uint32_t k = min((uint32_t)max(erel + min(ql + GS * j, h.e - 1), 0), ehi);
      d.v[j] = ld_col ? (PK ? (int)c8[k] : c32[k]) : 0;
      d.at[j] = ld_ea ? (int)ea[k] : 0;
    }
    return d;
  };
  Hdr hdr = load_hdr(u0);
  Dat dat = load_dat(u0, hdr);
  Hdr hdr_next = load_hdr(u0 + 1);
  for (int unit = u0; unit < u1; ++unit) {
    const int g = unit * NG + grp;
    const bool valid = g < G;
    const int nb0 = hdr.nb0, n = hdr.n, e = hdr.e;
    const int64_t e0 = hdr.e0;
    // the group's row: in LDS (ROWS) or in the slab
    int32_t *__restrict__ orow = ROWS ? srow + grp * ld : a.out + (int64_t)g * ld;
    auto put = [&](int p, int t) { if (p < cap) orow[p] = t; };
    const int32_t *__restrict__ rpg = a.g.rowptr + nb0 + g;
    // ---- lane = node: entry -> row map, <atom> TYPE pairs
    wave_sync();   // the previous unit's map and rows are no longer read
    if (valid && ql == 0) put(0, slut[GTOK_ZLUT_BOS]);
    auto node_step = [&](int i, int rs, int re, int x) {   // :168-169, 'X' for x outside 0..8 (:104)
      re = min(re, e);
      for (int k = rs; k < re; ++k) rmap[k] = (uint16_t)i;
      const int p = 1 + 2 * i, id = slut[GTOK_ZLUT_ATOM0 + (x <= 8 ? x : 9)];
      if (p + 1 < cap) *reinterpret_cast<I32x2 *>(orow + p) = I32x2{t_atom, id};   // dword-aligned 8-byte store
      else put(p, t_atom);
    };
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int i = ql + GS * j;
      if (i < n) node_step(i, dat.rs[j], dat.re[j], dat.x[j]);
    }
    for (int i = ql + GS * NP; i < n; i += GS) node_step(i, rpg[i], rpg[i + 1], has_na ? (int)a.g.nattr[nb0 + i] : 255);
    wave_sync();
    // ---- lane = entry: keep u <= v (first occurrence of {u,v}: zinc_dataset_indexbase.py:176-184)
    int pos = 1 + 2 * n;
    int emax = 0;
#pragma unroll
    for (int q = 0; q < NG; ++q) emax = max(emax, __builtin_amdgcn_readlane(e, q * GS));
    auto entry_step = [&](int k, int v, int at) {
      const bool in = k < e;
      const int u = in ? (int)rmap[k] : 0;
      const bool keep = in && u <= v;
      const uint32_t kept = (uint32_t)((uint64_t)__ballot(keep) >> (grp * GS)) & kGroupBits;   // this group's lanes
      if (keep) {
        const int p = pos + 4 * __popc(kept & ((1u << ql) - 1u));
        const int t1 = slut[GTOK_ZLUT_BOND0 + ((at >= 1 && at <= 4) ? at : 0)], t2 = node_id(u), t3 = node_id(v);
        if (p + 3 < cap) {
          *reinterpret_cast<I32x4 *>(orow + p) = I32x4{t_bond, t1, t2, t3};   // dword-aligned 16-byte store
        } else {
          put(p, t_bond); put(p + 1, t1); put(p + 2, t2);
        }
      }
      pos += 4 * __popc(kept);
    };
#pragma unroll
    for (int j = 0; j < EP; ++j)
      if (GS * j < emax) entry_step(ql + GS * j, dat.v[j], dat.at[j]);
    for (int k0 = GS * EP; k0 < emax; k0 += GS) {
      const int k = k0 + ql;
      entry_step(k, k < e ? a.g.col[e0 + k] : 0, (k < e && has_ea) ? (int)a.g.eattr[e0 + k] : 0);
    }
    // ---- next units' requests go out ahead of this unit's row stores
    hdr = hdr_next;
    dat = load_dat(unit + 1, hdr);
    hdr_next = load_hdr(unit + 2);
    // ---- tail, length
    int len = 0;
    if (valid) {
      if (ql == 0) {
        put(pos, slut[GTOK_ZLUT_Q]);
        put(pos + 1, slut[GTOK_ZLUT_REGRESSION]);
        put(pos + 2, slut[GTOK_ZLUT_P]);
      }
      const int64_t T = (int64_t)pos + 5;   // text tokens incl. label and <eos>
      if (T <= (int64_t)a.max_len + 1) {
        len = (int)(T - 2);
      } else {                               // :217-221 tokens[:max_len-1] + ['<eos>']
        len = a.max_len;
        if (ql == 0 && a.max_len >= 1 && a.max_len - 1 < ld) {
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // after the other lanes' stores to that slot
          orow[a.max_len - 1] = slut[GTOK_ZLUT_EOS];
        }
      }
      if (ql == 0) a.out_len[g] = len;
    }
    if (ROWS) {
      // ---- the four rows leave together: ld is a multiple of 4 here, so a 16-byte vector never spans two rows
      wave_sync();
      const int g0 = unit * NG, rows = min(NG, G - g0), vpr = ld >> 2;
      I32x4 *__restrict__ dst = reinterpret_cast<I32x4 *>(a.out + (int64_t)g0 * ld);
      const U8x16a *src = reinterpret_cast<const U8x16a *>(srow);
      int rl[NG];
#pragma unroll
      for (int q = 0; q < NG; ++q) rl[q] = min(__builtin_amdgcn_readlane(len, q * GS), ld);
      int r = 0, c = lane;                      // vector t = lane + 64 j of the unit sits in row r, column 4c
      while (c >= vpr) { c -= vpr; ++r; }
      while (r < rows) {
        int lr = rl[0];
#pragma unroll
        for (int q = 1; q < NG; ++q) lr = r == q ? rl[q] : lr;
        const U8x16a w = src[r * vpr + c];
        const int c4 = c << 2;
        dst[r * vpr + c] = I32x4{c4 + 0 < lr ? (int)w.a : pad, c4 + 1 < lr ? (int)w.b : pad,
                                 c4 + 2 < lr ? (int)w.c : pad, c4 + 3 < lr ? (int)w.d : pad};
        c += kWave;
        while (c >= vpr) { c -= vpr; ++r; }
      }
    } else if (valid) {
      const int lr = min(len, ld), nrem = ld - lr, nvec = nrem >> 2;
      int32_t *__restrict__ tail = orow + lr;
      for (int t = ql; t < nvec; t += GS) reinterpret_cast<I32x4 *>(tail)[t] = I32x4{pad, pad, pad, pad};
      if (ql < (nrem & 3)) tail[(nvec << 2) + ql] = pad;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// graph-token grammar from the edge list
// ---------------------------------------------------------------------------------------------
struct SynthLds { int rp, tok, lut, stride; };
struct SynthArgs {
  gtok_csr g;
  const int32_t *lut; const int32_t *query;
  int lut_len, max_len, pad_id, maxn, tcap;
  SynthLds l;
  int32_t *out; int ld; int32_t *out_len;
  int units, upb;
};

__global__ void __launch_bounds__(256) ibtt_synth_kernel(const SynthArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id();
  const int wave = wave_id(), wpb = (int)(blockDim.x >> 6);
  unsigned char *base = smem + (size_t)wave * a.l.stride;
  int32_t *rp = reinterpret_cast<int32_t *>(base + a.l.rp);
  int32_t *tok = reinterpret_cast<int32_t *>(base + a.l.tok);
  int32_t *lut = reinterpret_cast<int32_t *>(base + a.l.lut);   // the wave's own copy: no workgroup barrier anywhere
  const int pad = a.pad_id, tcap = a.tcap, G = a.g.num_graphs;
  const bool has_order = a.g.eorder != nullptr;
  for (int i = lane; i < a.lut_len; i += kWave) lut[i] = a.lut[i];
  wave_sync();
  auto put = [&](int64_t q, int v) { if (q < tcap) tok[q] = v; };
  auto node_id = [&](int i) { return (GTOK_SLUT_NODE0 + i < a.lut_len) ? lut[GTOK_SLUT_NODE0 + i] : pad; };

  // Software pipeline over the wave's graphs: a graph's loads form the chain header -> (row pointers, the entries that
  // survive the cut), and vmcnt retires in order, so loads issued behind the previous row's 2.4 KB of stores wait for
  // HBM to take them.  Graph +2's header (scalar loads) and graph +1's first 320 row pointers / 256 entries are
  // therefore requested before graph's row is stored; longer graphs finish with plain loops.
  struct Hdr { int nb0, nfull, n, e, elim; int64_t e0; };
  struct Dat { int rp[5], col[4], ord[4]; };
  const int64_t Etot = sload(a.g.edge_ptr, G);
  const int vb = virtual_block();
  const int u0 = vb * a.upb, u1 = min(a.units, u0 + a.upb);
  auto load_hdr = [&](int unit) -> Hdr {
    Hdr h{0, 0, 0, 0, 0, 0};
    const int g = unit * wpb + wave;
    if (unit < u1 && g < G) {
      h.nb0 = sload(a.g.node_ptr, g);
      h.nfull = sload(a.g.node_ptr, g + 1) - h.nb0;
      h.n = min(h.nfull, a.maxn);
      h.e0 = sload(a.g.edge_ptr, g);
      h.e = (int)(sload(a.g.edge_ptr, g + 1) - h.e0);
      // "u v <e>" at 1+3p for the edge at original position p; only entries whose tokens survive the cut are
      // touched when the order is the identity
      h.elim = has_order ? h.e : min(h.e, (tcap + 1) / 3 + 1);
    }
    return h;
  };
  auto load_dat = [&](int unit, const Hdr &h) -> Dat {
    Dat d;
    const int g = (unit < u1 && unit * wpb + wave < G) ? unit * wpb + wave : 0;   // past the end: graph 0's first words
    const int32_t *__restrict__ rpg = a.g.rowptr + h.nb0 + g;
#pragma unroll
    for (int j = 0; j < 5; ++j) d.rp[j] = rpg[(uint32_t)min(lane + kWave * j, h.n)];
    // a graph's entries are [e0, e0 + e) of the arrays, so the clamp is needed only where there are none (an empty graph, a unit
    // past the end: entry 0 of the array then): the base is wave-uniform - scalar registers - and the lane adds an unsigned
    // 32-bit offset, two vector instructions per load instead of a 64-bit add and two 64-bit clamps
    const int64_t ebase = h.e > 0 ? h.e0 : 0;
    const int32_t *__restrict__ cb = a.g.col + ebase;
    const int32_t *__restrict__ ob = has_order ? a.g.eorder + ebase : nullptr;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t k = (uint32_t)max(min(lane + kWave * j, h.elim - 1), 0);
      d.col[j] = Etot > 0 ? cb[k] : 0;
      d.ord[j] = (has_order && Etot > 0) ? ob[k] : lane + kWave * j;
    }
    return d;
  };
  Hdr hdr = load_hdr(u0);
  Dat dat = load_dat(u0, hdr);
  Hdr hdr_next = load_hdr(u0 + 1);
  for (int unit = u0; unit < u1; ++unit) {
    const int g = unit * wpb + wave;
    if (g >= G) break;
    const int nb0 = hdr.nb0, nfull = hdr.nfull, n = hdr.n, e = hdr.e, elim = hdr.elim;
    const int64_t e0 = hdr.e0;
    const int32_t *__restrict__ rpg = a.g.rowptr + nb0 + g;

#pragma unroll
    for (int j = 0; j < 5; ++j) { const int i = lane + kWave * j; if (i <= n) rp[i] = dat.rp[j]; }
    for (int i = lane + 5 * kWave; i <= n; i += kWave) rp[i] = rpg[i];
    wave_sync();
    // only rows that start before the cut can own a surviving entry (row pointers never decrease): the search for an
    // entry's row runs over those, ~16 rows of a 150-node graph instead of all of them
    int nrow = 0;
    for (int b = 0; b < n; b += kWave) nrow += __popcll(__ballot(b + lane < n && rp[b + lane] < elim));
    nrow = max(nrow, 1);
    auto entry = [&](int k, int v, int p) {
      const int64_t q = 1 + 3 * (int64_t)p;
      if (q < tcap) {
        const int u = row_of(rp, nrow, k);
        put(q, node_id(u)); put(q + 1, node_id(v)); put(q + 2, lut[GTOK_SLUT_E]);
      }
    };
#pragma unroll
    for (int j = 0; j < 4; ++j) { const int k = lane + kWave * j; if (k < elim) entry(k, dat.col[j], dat.ord[j]); }
    for (int k = lane + 4 * kWave; k < elim; k += kWave) entry(k, a.g.col[e0 + k], has_order ? a.g.eorder[e0 + k] : k);
    const int64_t qn = 1 + 3 * (int64_t)e;
    for (int i = lane; i < nfull; i += kWave) put(qn + 1 + i, node_id(i));
    int nq = 0;
    if (a.query) nq = min(max(a.query[4 * (int64_t)g], 0), 3);
    if (lane == 0) {
      put(0, lut[GTOK_SLUT_BOS]);
      put(qn, lut[GTOK_SLUT_N]);
      const int64_t qq = qn + 1 + nfull;
      put(qq, lut[GTOK_SLUT_Q]);
      for (int i = 0; i < nq; ++i) put(qq + 1 + i, a.query[4 * (int64_t)g + 1 + i]);
      put(qq + 1 + nq, lut[GTOK_SLUT_P]);
    }
    // ---- the next graphs' requests go out ahead of this row's stores
    hdr = hdr_next;
    dat = load_dat(unit + 1, hdr);
    hdr_next = load_hdr(unit + 2);
    wave_sync();
    const int64_t T = 1 + 3 * (int64_t)e + 1 + nfull + 1 + nq + 1;
    const int len = (int)min(T, (int64_t)a.max_len);
    write_row(a.out + (int64_t)g * a.ld, a.ld, min(len, tcap), pad, [=](int i) -> int { return tok[i]; });
    if (lane == 0) a.out_len[g] = len;
    wave_sync();
  }
}

// ---------------------------------------------------------------------------------------------
// node-id token statistics of the graph-token texts (corpus pass of build_vocab_from_texts)
// ---------------------------------------------------------------------------------------------
// Wave per graph over a contiguous range; the wave keeps a private histogram / first-position table in LDS
// (every graph hits the same few hundred ids: global atomics would serialise) and merges it into the global
// tables once, when its range is done.  Lane = row for the `u` side (a row's endpoints share u: one add of the
// degree), lane = entry for the `v` side, lane = node for the <n> list.
struct VocabArgs {
  gtok_csr g;
  const int32_t *query_nodes;
  int64_t graph_base;
  int num_ids, stride;   // LDS bytes per wave
  unsigned long long *count, *first;
  int units, upb;
};

__global__ void __launch_bounds__(256) vocab_stats_synth_kernel(const VocabArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = lane_id();
  const int wave = wave_id(), wpb = (int)(blockDim.x >> 6);
  unsigned long long *fst = reinterpret_cast<unsigned long long *>(smem + (size_t)wave * a.stride);
  unsigned int *cnt = reinterpret_cast<unsigned int *>(fst + a.num_ids);
  const int K = a.num_ids, G = a.g.num_graphs;
  const bool has_order = a.g.eorder != nullptr;
  for (int i = lane; i < K; i += kWave) { fst[i] = ~0ull >> 1; cnt[i] = 0; }
  wave_sync();
  // A wave walks its graphs in increasing index, and a graph's <n> list names every id below its node count:
  // once a graph with N nodes is done, ids < N already hold a first position from an earlier (smaller) graph
  // key, so later graphs with <= N nodes only count (half the LDS atomics of the pass).
  int seen_n = 0;
  const int vb = virtual_block();
  const int u0 = vb * a.upb, u1 = min(a.units, u0 + a.upb);
  for (int unit = u0; unit < u1; ++unit) {
    const int g = unit * wpb + wave;
    if (g >= G) break;
    const int nb0 = sload(a.g.node_ptr, g), n = sload(a.g.node_ptr, g + 1) - nb0;
    const int64_t e0 = sload(a.g.edge_ptr, g);
    const int e = (int)(sload(a.g.edge_ptr, g + 1) - e0);
    const int32_t *__restrict__ rpg = a.g.rowptr + nb0 + g;
    const unsigned long long gkey = (unsigned long long)(a.graph_base + g) << 32;
    const bool fresh = n > seen_n;   // some id of this graph may not have been seen yet
    auto hit = [&](int id, unsigned int times, unsigned long long key) {
      if ((unsigned)id < (unsigned)K) {
        atomicAdd(&cnt[id], times);
        if (fresh || id >= seen_n) atomicMin(&fst[id], key);
      }
    };
    for (int u = lane; u < n; u += kWave) {   // "u v <e>" of the edge at list position p: u at 1+3p, v at 2+3p
      const int rs = rpg[u], re = min(rpg[u + 1], e);
      if (re > rs) {
        int pmin = rs;                        // identity order: the row's first entry is its first listed one
        if (has_order && fresh) { pmin = a.g.eorder[e0 + rs]; for (int k = rs + 1; k < re; ++k) pmin = min(pmin, a.g.eorder[e0 + k]); }
        hit(u, (unsigned)(re - rs), gkey | (unsigned long long)(1 + 3 * (int64_t)pmin));
      }
      hit(u, 1u, gkey | (unsigned long long)(2 + 3 * (int64_t)e + u));   // the <n> list: node u at 1+3E+1+u
    }
    for (int k0 = 0; k0 < e; k0 += 8 * kWave) {   // 8 loads in flight per lane (clamped, unconditional: one basic block)
      int v[8], p[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = min(k0 + lane + kWave * j, e - 1);
        v[j] = a.g.col[e0 + k];
        p[j] = (has_order && fresh) ? a.g.eorder[e0 + k] : k;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (k0 + lane + kWave * j < e) hit(v[j], 1u, gkey | (unsigned long long)(2 + 3 * (int64_t)p[j]));
    }
    if (a.query_nodes && lane < 2) {          // "<q> TASK qu qv": after the <n> list (1+3E+1+N), <q> and TASK
      const int qn = a.query_nodes[2 * (int64_t)g + lane];
      if (qn >= 0) hit(qn, 1u, gkey | (unsigned long long)(4 + 3 * (int64_t)e + n + lane));
    }
    wave_sync();   // this graph's positions are in before a later graph may skip them
    seen_n = max(seen_n, n);
  }
  wave_sync();
  for (int i = lane; i < K; i += kWave)
    if (cnt[i]) { atomicAdd(&a.count[i], (unsigned long long)cnt[i]); atomicMin(&a.first[i], fst[i]); }
}

// tokens a wave stages for a row: the longest row of the batch (tmax) under max_len and the slab's width, at least 4
static int token_cap(int64_t tmax, int max_len, int ld) {
  int64_t tcap = max_len < ld ? max_len : ld;
  if (tmax < tcap) tcap = tmax;
  return (int)(tcap < 4 ? 4 : tcap);
}

static bool csr_ok(const gtok_csr *g) {
  return g && g->num_graphs >= 0 && g->node_ptr && g->edge_ptr && g->rowptr && (g->max_edges <= 0 || g->col) &&
         !g->graph_ids && !g->unit_ptr;   // (a batch reordered for the lane-per-graph SENT kernel is for gtok_sent alone)
}

}  // namespace gtok

using namespace gtok;

namespace {

// Wave = wave per graph (any batch), Lane = lane per graph, Quad = 8 or 16 lanes per graph.  Lane and Quad need simple symmetric
// batches in list order; Quad is the default for them, GTOK_IBTT_KERNEL=lane|quad|wave pins a kernel (tests run all)
enum class ZincKernel { Wave, Lane, Quad };

ZincKernel ibtt_zinc_choose(const gtok_csr *g) {
  const char *pin = std::getenv("GTOK_IBTT_KERNEL");
  const bool list_ok = (g->flags & GTOK_CSR_SIMPLE_SYMMETRIC) && !g->eorder;
  const bool lane_ok = list_ok && g->max_nodes <= 255 && g->max_edges <= 255;
  const bool quad_ok = list_ok && g->max_nodes <= 65535 && g->max_edges <= 6000;   // 4 x maxe u16 of LDS
  ZincKernel k = quad_ok && g->num_graphs >= 1024 ? ZincKernel::Quad : ZincKernel::Wave;
  if (pin && pin[0] == 'l' && lane_ok) k = ZincKernel::Lane;
  if (pin && pin[0] == 'q' && quad_ok) k = ZincKernel::Quad;
  if (pin && pin[0] == 'w') k = ZincKernel::Wave;
  return k;
}

// one gtok_ibtt_zinc call that passed the argument checks
struct ZincCall {
  const gtok_csr *g; const int32_t *lut; int32_t lut_len, max_len, pad_id;
  int32_t *out; int32_t ld; int32_t *out_len;
  hipStream_t stream; int dev;   // (the stream's device: DeviceScope)
};

// ---- ibtt_zinc_quad_kernel: 8 or 16 lanes per molecule, one-wave workgroups
typedef void (*QuadKernel)(const ZincQuadArgs);

QuadKernel quad_kernel(bool rows, bool gs8, bool pk) {
  return with_flag(rows, [=](auto rows_) {
    return with_flag(gs8, [=](auto gs8_) {
      return with_flag(pk, [](auto pk_) -> QuadKernel {
        return ibtt_zinc_quad_kernel<decltype(rows_)::value, decltype(gs8_)::value ? 8 : 16, decltype(pk_)::value>;
      });
    });
  });
}

int launch_zinc_quad(const ZincCall &c) {
  const gtok_csr *g = c.g;
  ZincQuadArgs q;
  q.g = *g; q.lut = c.lut; q.lut_len = c.lut_len; q.max_len = c.max_len; q.pad_id = c.pad_id;
  q.maxe = g->max_edges > 0 ? g->max_edges : 1;
  // 8 lanes per molecule while molecules are small (the register pipeline covers 48 nodes / 96 entries), else 16
  const char *gs_pin = std::getenv("GTOK_IBTT_GROUP");
  int gs = (g->max_nodes <= 48 && g->max_edges <= 96) ? 8 : 16;
  if (gs_pin && (gs_pin[0] == '8')) gs = 8;
  if (gs_pin && (gs_pin[0] == '1')) gs = 16;
  const int ng = 64 / gs;
  int off = 0;
  q.off_map = off; off += align_up(ng * q.maxe * 2, 16);
  q.off_lut = off; off += align_up(c.lut_len * 4, 16);
  // rows assembled in LDS when the unit's rows fit next to the map (and 16-byte vectors do not span rows)
  const bool rows = (c.ld % 4) == 0 && off + 4 * ng * (int64_t)c.ld <= 16 * 1024;
  q.off_row = off;
  if (rows) off += 4 * ng * c.ld;
  q.lds = off;
  const QuadKernel kern = quad_kernel(rows, gs == 8, g->rowptr8 && g->col8);
  // a unit = the ng molecules of one wave.  ~60 SGPRs: 8 waves per SIMD are resident (measured: 24 -> 32 waves per CU still pays)
  const Grid G = plan_grid(reinterpret_cast<const void *>(kern), c.dev, (g->num_graphs + ng - 1) / ng, 1, (size_t)q.lds, Resident::Cap32);
  q.units = G.units; q.upb = G.upb;
  q.out = c.out; q.ld = c.ld; q.out_len = c.out_len;
  hipLaunchKernelGGL(kern, dim3(G.nb), dim3(64), (size_t)q.lds, c.stream, q);
  return hipGetLastError() == hipSuccess ? GTOK_OK : GTOK_E_LAUNCH;
}

// ---- ibtt_zinc_lane_kernel: a 64-graph unit staged in the LDS of a one-wave workgroup, units drawn from tickets.
// Returns whether it launched (*rc: the outcome); else the caller launches the wave-per-graph kernel.
bool launch_zinc_lane(const ZincCall &c, int *rc) {
  const gtok_csr *g = c.g;
  ZincLaneArgs z;
  z.g = *g; z.lut = c.lut; z.lut_len = c.lut_len; z.max_len = c.max_len; z.pad_id = c.pad_id;
  z.cap_n = g->chunk_nodes > 0 ? g->chunk_nodes : 64 * g->max_nodes;
  z.cap_e = g->chunk_edges > 0 ? g->chunk_edges : 64 * g->max_edges;
  z.cap_r = z.cap_n + 64;
  int off = 0;
  z.off_rp = off; off += align_up(z.cap_r + 4, 16);
  z.off_col = off; off += align_up(z.cap_e + 4, 16);
  z.off_eat = off; off += align_up((z.cap_e + 1) / 2 + 8, 16);   // nibbles
  z.off_nat = off; off += align_up(z.cap_n + 4, 16);
  z.off_lut = off; off += align_up(c.lut_len * 4, 16);
  z.lds = off;
  // a pinned lane kernel whose unit does not fit: the wave kernel runs (gtok_ibtt_zinc_kernel_name, which is not told lut_len, still says lane)
  if (z.lds > 64 * 1024) return false;
  const void *kern = reinterpret_cast<const void *>(ibtt_zinc_lane_kernel);
  const Grid G = plan_grid(kern, c.dev, (g->num_graphs + 63) / 64, 1, (size_t)z.lds, Resident::Tickets);
  z.units = G.units;
  const QueueSlot slot = take_queue_slot(c.dev, c.stream);   // (nothing is taken before the LDS test has passed)
  z.queue = slot.counters;
  if (!z.queue) { *rc = slot.graph_pool_empty ? GTOK_E_GRAPH_SLOTS : GTOK_E_LAUNCH; return true; }
  z.out = c.out; z.ld = c.ld; z.out_len = c.out_len;
  hipLaunchKernelGGL(ibtt_zinc_lane_kernel, dim3(G.nb), dim3(64), (size_t)z.lds, c.stream, z);
  mark_queue_slot(slot, c.stream);
  *rc = hipGetLastError() == hipSuccess ? GTOK_OK : GTOK_E_LAUNCH;
  return true;
}

// ---- ibtt_zinc_kernel: wave per graph
int launch_zinc_wave(const ZincCall &c) {
  const gtok_csr *g = c.g;
  ZincArgs a;
  a.g = *g; a.lut = c.lut; a.lut_len = c.lut_len; a.max_len = c.max_len; a.pad_id = c.pad_id;
  a.maxn = g->max_nodes > 0 ? g->max_nodes : 1;
  a.maxe = g->max_edges > 0 ? g->max_edges : 0;
  a.tcap = token_cap(6 + 2 * (int64_t)a.maxn + 4 * (int64_t)a.maxe, c.max_len, c.ld);
  const int me = a.maxe > 0 ? a.maxe : 1;
  int off = 0;
  a.l.rp = off; off += align_up((a.maxn + 1) * 4, 8);
  a.l.cc = off; off += align_up(me * 2, 8);
  a.l.co = off; off += align_up(me * 2, 8);
  a.l.ou = off; off += align_up(me * 2, 8);
  a.l.ov = off; off += align_up(me * 2, 8);
  a.l.oa = off; off += align_up(me, 8);
  a.l.tok = off; off += align_up(a.tcap * 4, 16);
  a.l.stride = align_up(off, 16);
  if (a.l.stride > 160 * 1024) return GTOK_E_TOO_LARGE;
  a.out = c.out; a.ld = c.ld; a.out_len = c.out_len;
  return launch_wave_per_item(ibtt_zinc_kernel, a, g->num_graphs, 4, a.l.stride, c.dev, c.stream);
}

}  // namespace

extern "C" const char *gtok_ibtt_zinc_kernel_name(const gtok_csr *g) {
  static const char *names[] = {"ibtt_zinc_kernel", "ibtt_zinc_lane_kernel", "ibtt_zinc_quad_kernel"};   // in ZincKernel's order
  return !g ? "" : names[(int)ibtt_zinc_choose(g)];
}

extern "C" int gtok_ibtt_zinc(const gtok_csr *g, const int32_t *lut, int32_t lut_len, int32_t max_len,
                              int32_t pad_id, int32_t *out_ids, int32_t ld, int32_t *out_len,
                              void *stream) {
  gtok::DeviceScope device_scope((hipStream_t)stream);   // the stream's device, not the thread's current one
  if (!device_scope.ok()) return GTOK_E_NO_DEVICE;
  if (!g || g->num_graphs < 0 || max_len < 0 || ld <= 0) return GTOK_E_INVAL;
  if (g->num_graphs == 0) return GTOK_OK;   // an empty batch is a no-op
  if (!csr_ok(g) || !lut || lut_len < GTOK_ZLUT_NODE0 || !out_ids || !out_len) return GTOK_E_INVAL;
  if (g->max_nodes > 65535 || g->max_edges > 65535) return GTOK_E_TOO_LARGE;
  const ZincCall c{g, lut, lut_len, max_len, pad_id, out_ids, ld, out_len, (hipStream_t)stream, device_scope.dev};
  const ZincKernel which = ibtt_zinc_choose(g);
  if (which == ZincKernel::Quad) return launch_zinc_quad(c);
  int rc = GTOK_E_LAUNCH;
  if (which == ZincKernel::Lane && launch_zinc_lane(c, &rc)) return rc;
  return launch_zinc_wave(c);
}

extern "C" int gtok_ibtt_synth(const gtok_csr *g, const int32_t *lut, int32_t lut_len,
                               const int32_t *query, int32_t max_len, int32_t pad_id,
                               int32_t *out_ids, int32_t ld, int32_t *out_len, void *stream) {
  gtok::DeviceScope device_scope((hipStream_t)stream);   // the stream's device, not the thread's current one
  if (!device_scope.ok()) return GTOK_E_NO_DEVICE;
  if (!g || g->num_graphs < 0 || max_len < 0 || ld <= 0) return GTOK_E_INVAL;
  if (g->num_graphs == 0) return GTOK_OK;
  if (!csr_ok(g) || !lut || lut_len < GTOK_SLUT_NODE0 || !out_ids || !out_len) return GTOK_E_INVAL;
  SynthArgs a;
  a.g = *g; a.lut = lut; a.query = query; a.lut_len = lut_len; a.max_len = max_len; a.pad_id = pad_id;
  a.maxn = g->max_nodes > 0 ? g->max_nodes : 1;
  a.tcap = token_cap(1 + 3 * (int64_t)(g->max_edges > 0 ? g->max_edges : 0) + 1 + a.maxn + 5, max_len, ld);
  int off = 0;
  a.l.rp = off; off += align_up((a.maxn + 1) * 4, 16);
  a.l.tok = off; off += align_up(a.tcap * 4, 16);
  a.l.lut = off; off += align_up(lut_len * 4, 16);
  a.l.stride = align_up(off, 16);
  if (a.l.stride > 160 * 1024) return GTOK_E_TOO_LARGE;
  a.out = out_ids; a.ld = ld; a.out_len = out_len;
  return launch_wave_per_item(ibtt_synth_kernel, a, g->num_graphs, 4, a.l.stride, device_scope.dev, (hipStream_t)stream);
}

extern "C" int gtok_vocab_stats_synth(const gtok_csr *g, const int32_t *query_nodes, int64_t graph_base,
                                      int32_t num_ids, int64_t *count, int64_t *first, void *stream) {
  gtok::DeviceScope device_scope((hipStream_t)stream);   // the stream's device, not the thread's current one
  if (!device_scope.ok()) return GTOK_E_NO_DEVICE;
  if (!g || g->num_graphs < 0 || num_ids <= 0) return GTOK_E_INVAL;
  if (g->num_graphs == 0) return GTOK_OK;
  if (!csr_ok(g) || !count || !first) return GTOK_E_INVAL;
  if (num_ids > 1024) return GTOK_E_TOO_LARGE;
  VocabArgs a;
  a.g = *g; a.query_nodes = query_nodes; a.graph_base = graph_base; a.num_ids = num_ids;
  a.stride = align_up(num_ids * 12, 16);
  a.count = reinterpret_cast<unsigned long long *>(count);
  a.first = reinterpret_cast<unsigned long long *>(first);
  // (four waves per workgroup: at most 1024 ids x 12 bytes each)
  return launch_wave_per_item(vocab_stats_synth_kernel, a, g->num_graphs, 4, a.stride, device_scope.dev, (hipStream_t)stream);
}

extern "C" int gtok_version(void) { return GTOK_ABI_VERSION; }
extern "C" const char *gtok_target(void) { return "gfx950"; }
