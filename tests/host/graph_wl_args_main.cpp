// Stand-alone program over the host-side argument checks, the kernel choice and the LDS / workspace arithmetic of gtok_graph_wl
// (csrc/gtok_graph_wl_args.hpp) and over the key arithmetic (csrc/gtok_graph_wl_hash.hpp), to be run under the host sanitizers on a
// machine without a GPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Iglearning-benchmark_amd/csrc \
//       tests/host/graph_wl_args_main.cpp -o /tmp/graph_wl_args && /tmp/graph_wl_args
// Exit status 0 and "0 failures": every check answered as include/gtok.h documents, the key has the properties DESIGN.md states and
// no sanitizer spoke.  `graph_wl_args key N ROUNDS v0 u0 v1 u1 ... [label L] [attrs a_0 .. a_N-1 t_0 .. t_E-1]` prints the key of one
// graph, entry i being (v_i, u_i) as row v_i lists it (the host tests hold the numpy restatement against it).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "gtok_graph_wl_args.hpp"
#include "gtok_graph_wl_hash.hpp"

static int failures = 0;
#define EXPECT(expr, want)                                                        \
  do {                                                                            \
    const long long got_ = (long long)(expr);                                     \
    if (got_ != (long long)(want)) { std::printf("%s: %lld, expected %lld\n", #expr, got_, (long long)(want)); ++failures; } \
  } while (0)

typedef std::vector<std::pair<int, int>> Edges;

// the definition, node by node: the closure of the entries; with attributes the bytes of the entry (v, u) as listed
static void wl_key(int n, const Edges &e, int rounds, int label, const std::vector<int> *na, const std::vector<int> *ea, uint64_t out[2]) {
  std::vector<std::set<int>> A(n);
  std::vector<int> loop(n, 0);
  for (const auto &p : e) {
    if (p.first == p.second) { loop[p.first] = 1; continue; }
    A[p.first].insert(p.second); A[p.second].insert(p.first);
  }
  auto t_of = [&](int v, int u) -> uint32_t {
    if (!ea) return 0;
    for (size_t i = 0; i < e.size(); ++i)
      if (e[i].first == v && e[i].second == u) return 1u + (uint32_t)(*ea)[i];
    return 0;
  };
  std::vector<uint64_t> c(n), d(n);
  for (int v = 0; v < n; ++v) c[v] = gtok::wl_init((uint32_t)A[v].size(), (uint32_t)loop[v], na ? 1u + (uint32_t)(*na)[v] : 0u);
  const uint32_t R = gtok::wl_rounds_run(rounds, n);
  for (uint32_t r = 0; r < R; ++r) {
    for (int v = 0; v < n; ++v) {
      uint64_t sum = 0;
      for (int u : A[v]) sum += gtok::wl_term(c[u], t_of(v, u));
      d[v] = gtok::wl_next(c[v], sum);
    }
    c.swap(d);
  }
  gtok::WlSums s;
  for (int v = 0; v < n; ++v) s.add(c[v]);
  gtok::wl_finish(s, (uint32_t)n, R, label, out);
}
static void wl_key(int n, const Edges &e, int rounds, int label, uint64_t out[2]) { wl_key(n, e, rounds, label, nullptr, nullptr, out); }
static bool same(const uint64_t a[2], const uint64_t b[2]) { return a[0] == b[0] && a[1] == b[1]; }

int main(int argc, char **argv) {
  using namespace gtok;
  if (argc >= 4 && !strcmp(argv[1], "key")) {
    const int n = std::atoi(argv[2]), rounds = std::atoi(argv[3]);
    Edges e;
    int label = 0, i = 4;
    for (; i + 1 < argc && strcmp(argv[i], "label") && strcmp(argv[i], "attrs"); i += 2) e.push_back({std::atoi(argv[i]), std::atoi(argv[i + 1])});
    if (i + 1 < argc && !strcmp(argv[i], "label")) { label = std::atoi(argv[i + 1]); i += 2; }
    std::vector<int> na, ea;
    const bool attrs = i < argc && !strcmp(argv[i], "attrs");
    if (attrs) {
      ++i;
      if (argc - i != n + (int)e.size()) { std::printf("attrs: %d node bytes and %d entry bytes\n", n, (int)e.size()); return 2; }
      for (int k = 0; k < n; ++k) na.push_back(std::atoi(argv[i++]));
      for (size_t k = 0; k < e.size(); ++k) ea.push_back(std::atoi(argv[i++]));
    }
    for (const auto &p : e)
      if (p.first < 0 || p.first >= n || p.second < 0 || p.second >= n) { std::printf("an endpoint outside the graph\n"); return 2; }
    uint64_t k[2];
    wl_key(n, e, rounds, label, attrs ? &na : nullptr, attrs ? &ea : nullptr, k);
    std::printf("%016llx %016llx\n", (unsigned long long)k[0], (unsigned long long)k[1]);
    return 0;
  }
  const int SYM = GTOK_CSR_SIMPLE_SYMMETRIC, BIG = GTOK_SENT_LARGE_MAX_NODES, A = GTOK_WL_ATTRS;
  // ---- the arithmetic: the worked examples of DESIGN.md section 5c, and what changes a key
  {
    uint64_t a[2], b[2];
    wl_key(3, {{2, 1}, {0, 1}}, 2, 0, a);
    EXPECT(a[0] == 0x370B3D1306912C14ull && a[1] == 0x2ED56162F3BE8ABBull, 1);
    wl_key(3, {{0, 2}, {2, 1}, {1, 2}}, 2, 0, b);             // the same path renumbered, one edge listed twice
    EXPECT(same(a, b), 1);
    const std::vector<int> na = {0, 1, 0}, ea = {1, 2, 1, 2};
    wl_key(3, {{2, 1}, {0, 1}, {1, 2}, {1, 0}}, 2, -1, &na, &ea, b);
    EXPECT(b[0] == 0xF57092ED9F8FA531ull && b[1] == 0x314F65BE727FB3C7ull, 1);
    const std::vector<int> na2 = {0, 0, 1}, ea2 = {2, 1, 2, 1};   // renumbered 0 -> 1, 1 -> 2, 2 -> 0: entries (0,2), (1,2), (2,0), (2,1)
    uint64_t c[2];
    wl_key(3, {{1, 2}, {0, 2}, {2, 1}, {2, 0}}, 2, -1, &na2, &ea2, c);
    EXPECT(same(b, c), 1);
    const std::vector<int> na3 = {0, 2, 0}, ea3 = {1, 3, 1, 2};
    wl_key(3, {{2, 1}, {0, 1}, {1, 2}, {1, 0}}, 2, -1, &na3, &ea, c);
    EXPECT(same(b, c), 0);                                    // one node byte changed
    wl_key(3, {{2, 1}, {0, 1}, {1, 2}, {1, 0}}, 2, -1, &na, &ea3, c);
    EXPECT(same(b, c), 0);                                    // one edge byte changed
    wl_key(3, {{2, 1}, {0, 1}}, 3, 0, b);
    EXPECT(same(a, b), 0);                                    // another round count
    wl_key(3, {{2, 1}, {0, 1}}, 0, 0, c);
    EXPECT(same(b, c), 1);                                    // rounds == 0 is N rounds
    wl_key(3, {{2, 1}, {0, 1}}, 2, 1, b);
    EXPECT(same(a, b), 0);                                    // another label
    wl_key(4, {{2, 1}, {0, 1}}, 2, 0, b);
    EXPECT(same(a, b), 0);                                    // one node more
    wl_key(3, {{2, 1}, {0, 1}, {1, 1}}, 2, 0, b);
    EXPECT(same(a, b), 0);                                    // a loop
    wl_key(3, {{2, 1}, {0, 1}, {0, 2}}, 2, 0, b);
    EXPECT(same(a, b), 0);                                    // one edge more
    // the documented limit: a 6-cycle and two triangles, 2-regular both, share the key at every round count
    const Edges c6 = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {5, 0}}, tt = {{0, 1}, {1, 2}, {2, 0}, {3, 4}, {4, 5}, {5, 3}};
    for (int r : {0, 1, 2, 3, 7, 512}) {
      wl_key(6, c6, r, 0, a);
      wl_key(6, tt, r, 0, b);
      EXPECT(same(a, b), 1);
    }
    // ... and a 6-path and a triangle with a tail part ways
    wl_key(6, {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}}, 3, 0, a);
    wl_key(6, {{0, 1}, {1, 2}, {2, 0}, {2, 3}, {3, 4}}, 3, 0, b);
    EXPECT(same(a, b), 0);
    wl_key(0, {}, 3, 0, a);
    wl_key(1, {}, 3, 0, b);
    EXPECT(same(a, b), 0);
    EXPECT(wl_rounds_run(0, 17), 17);
    EXPECT(wl_rounds_run(5, 17), 5);
    EXPECT(wl_init(3, 0, 0) != wl_init(3, 1, 0) && wl_init(3, 0, 0) != wl_init(3, 0, 1) && wl_init(16383, 1, 256) == keys_mix((16383ull | 1ull << 15 | 256ull << 16) ^ kKeysC0), 1);
    EXPECT(wl_term(5, 0) != wl_term(5, 1), 1);
  }
  // ---- the hook
  EXPECT(graph_wl_forced(nullptr), -1);
  EXPECT(graph_wl_forced(""), -1);
  EXPECT(graph_wl_forced("reg"), kWlReg);
  EXPECT(graph_wl_forced("lds"), kWlLds);
  EXPECT(graph_wl_forced("csr"), kWlCsr);
  EXPECT(graph_wl_forced("CSR"), -1);
  // ---- the path: by max_nodes, at every threshold; attributes pull over the CSR
  for (int r : {0, 1, 3, 512}) {
    for (int n : {0, 1, 2, 63, 64}) EXPECT(graph_wl_path(n, 0, 0, r, -1), kWlReg);
    for (int n : {65, 128, 129, 256, 257, 511, 512}) EXPECT(graph_wl_path(n, SYM, 0, r, -1), kWlLds);
  }
  for (int n : {513, 4096, 4097, BIG}) {
    EXPECT(graph_wl_path(n, SYM, 0, 3, -1), kWlCsr);
    EXPECT(graph_wl_path(n, SYM, A, 3, -1), kWlCsr);
    EXPECT(graph_wl_path(n, 0, 0, 3, -1), GTOK_E_UNSUPPORTED);            // the flag rule
    EXPECT(graph_wl_path(n, 0, A, 3, -1), GTOK_E_UNSUPPORTED);
    EXPECT(graph_wl_path(n, SYM, 0, 0, -1), GTOK_E_UNSUPPORTED);          // rounds == 0 ends at 512 nodes
    EXPECT(graph_wl_path(n, SYM, 0, 3, kWlReg), GTOK_E_UNSUPPORTED);      // a forced kernel that cannot hold the batch
    EXPECT(graph_wl_path(n, SYM, 0, 3, kWlLds), GTOK_E_UNSUPPORTED);
    EXPECT(graph_wl_path(n, SYM, 0, 3, kWlCsr), kWlCsr);
  }
  EXPECT(graph_wl_path(512, SYM, 0, 0, kWlCsr), kWlCsr);
  EXPECT(graph_wl_path(40, SYM, A, 3, -1), kWlCsr);
  EXPECT(graph_wl_path(40, 0, A, 3, -1), GTOK_E_UNSUPPORTED);             // attributes on an unflagged batch
  EXPECT(graph_wl_path(40, SYM, A, 3, kWlReg), GTOK_E_UNSUPPORTED);       // attributes are the csr kernel's alone
  EXPECT(graph_wl_path(40, SYM, A, 3, kWlLds), GTOK_E_UNSUPPORTED);
  EXPECT(graph_wl_path(40, SYM, A, 0, kWlCsr), kWlCsr);
  EXPECT(graph_wl_path(40, 0, 0, 3, kWlLds), kWlLds);                     // small graphs through the larger kernels
  EXPECT(graph_wl_path(40, 0, 0, 3, kWlCsr), GTOK_E_UNSUPPORTED);
  EXPECT(graph_wl_path(40, SYM, 0, 3, kWlCsr), kWlCsr);
  EXPECT(graph_wl_path(65, 0, 0, 3, kWlReg), GTOK_E_UNSUPPORTED);
  EXPECT(graph_wl_path(BIG + 1, SYM, 0, 3, -1), GTOK_E_TOO_LARGE);
  EXPECT(graph_wl_path(-1, 0, 0, 3, -1), GTOK_E_INVAL);
  EXPECT(graph_wl_path(40, 0, 1, 3, -1), GTOK_E_INVAL);                   // unknown flag bits
  EXPECT(graph_wl_path(40, 0, 4, 3, -1), GTOK_E_INVAL);
  EXPECT(graph_wl_path(40, 0, 0, -1, -1), GTOK_E_INVAL);
  EXPECT(graph_wl_path(40, 0, 0, 513, -1), GTOK_E_INVAL);
  // ---- LDS per wave
  EXPECT(graph_wl_lds_bytes(kWlReg, 0), 1024);
  EXPECT(graph_wl_lds_bytes(kWlReg, 64), 1024);
  EXPECT(graph_wl_lds_bytes(kWlLds, 66), 3 * 66 * 8);
  EXPECT(graph_wl_lds_bytes(kWlLds, 129), (5 * 129 * 8 + 15) / 16 * 16);
  EXPECT(graph_wl_lds_bytes(kWlLds, 512), 36 * 1024);
  EXPECT(graph_wl_lds_bytes(kWlCsr, 23), 16 * 23);
  EXPECT(graph_wl_lds_bytes(kWlCsr, 0), 16);
  EXPECT(graph_wl_lds_bytes(kWlCsr, 4096), 64 * 1024);
  EXPECT(graph_wl_lds_bytes(kWlCsr, 4097), 0);
  EXPECT(graph_wl_lds_bytes(kWlCsr, BIG), 0);
  for (int n : {0, 1, 63, 64, 65, 129, 257, 511, 512})
    for (int p : {(int)kWlReg, (int)kWlLds, (int)kWlCsr}) EXPECT(graph_wl_lds_bytes(p, n) % 16, 0);
  // ---- the workspace: nothing up to 4,096 nodes, then 16 bytes per node for every wave
  EXPECT(graph_wl_workspace(0, 0), 0);
  EXPECT(graph_wl_workspace(4096, 100000), 0);
  EXPECT(graph_wl_workspace(4097, 0), 0);
  EXPECT(graph_wl_workspace(4097, 1), 16 * 4097);
  EXPECT(graph_wl_workspace(4097, 3), 3 * 16 * 4097);
  EXPECT(graph_wl_workspace(BIG, GTOK_WL_LARGE_WAVES), 1024ll * 16 * BIG);
  EXPECT(graph_wl_workspace(BIG, 2000000000), 1024ll * 16 * BIG);          // 256 MiB at the most
  EXPECT(graph_wl_workspace(BIG + 1, 1), GTOK_E_TOO_LARGE);
  EXPECT(graph_wl_workspace(-1, 1), GTOK_E_INVAL);
  EXPECT(graph_wl_workspace(1, -1), GTOK_E_INVAL);
  EXPECT(graph_wl_waves(5), 5);
  EXPECT(graph_wl_waves(1024), 1024);
  EXPECT(graph_wl_waves(1025), 1024);

  // ---- the argument checks
  std::vector<int32_t> i32(64, 0);
  std::vector<int64_t> i64(8, 0);
  std::vector<uint64_t> u64(64, 0);
  std::vector<uint8_t> u8(64, 0);
  alignas(16) static unsigned char wsbuf[64];
  gtok_csr g;
  std::memset(&g, 0, sizeof g);
  g.num_graphs = 3; g.max_nodes = 9; g.max_edges = 20;
  g.node_ptr = i32.data(); g.edge_ptr = i64.data(); g.rowptr = i32.data(); g.col = i32.data();
  const int32_t *lab = i32.data(), *info = i32.data();
  const uint64_t *keys = u64.data(), *colors = u64.data();
  const int REG = kWlPathBase + kWlReg, LDS = kWlPathBase + kWlLds, CSR = kWlPathBase + kWlCsr;
  EXPECT(graph_wl_check(&g, lab, 3, 0, keys, colors, info, nullptr, 0, -1), REG);
  EXPECT(graph_wl_check(&g, nullptr, 3, 0, keys, nullptr, info, nullptr, 0, -1), REG);          // no labels, no colours
  EXPECT(graph_wl_check(&g, lab, 0, 0, keys, colors, info, nullptr, 0, -1), REG);
  EXPECT(graph_wl_check(&g, lab, 512, 0, keys, colors, info, nullptr, 0, -1), REG);
  EXPECT(graph_wl_check(&g, lab, 513, 0, keys, colors, info, nullptr, 0, -1), GTOK_E_INVAL);
  EXPECT(graph_wl_check(&g, lab, -1, 0, keys, colors, info, nullptr, 0, -1), GTOK_E_INVAL);
  EXPECT(graph_wl_check(nullptr, lab, 3, 0, keys, colors, info, nullptr, 0, -1), GTOK_E_INVAL);
  EXPECT(graph_wl_check(&g, lab, 3, 0, nullptr, colors, info, nullptr, 0, -1), GTOK_E_INVAL);
  EXPECT(graph_wl_check(&g, lab, 3, 0, keys, colors, nullptr, nullptr, 0, -1), GTOK_E_INVAL);
  EXPECT(graph_wl_check(&g, lab, 3, 0, keys, colors, info, nullptr, -1, -1), GTOK_E_INVAL);     // a negative size
  EXPECT(graph_wl_check(&g, lab, 3, 1, keys, colors, info, nullptr, 0, -1), GTOK_E_INVAL);      // unknown flag bits
  EXPECT(graph_wl_check(&g, lab, 3, 4, keys, colors, info, nullptr, 0, -1), GTOK_E_INVAL);
  EXPECT(graph_wl_check(&g, lab, 3, A, keys, colors, info, nullptr, 0, -1), GTOK_E_INVAL);      // attributes asked for, none there
  {
    gtok_csr h = g;
    h.nattr = u8.data();
    EXPECT(graph_wl_check(&h, lab, 3, A, keys, colors, info, nullptr, 0, -1), GTOK_E_INVAL);    // ... only one of the two
    h.eattr = u8.data();
    EXPECT(graph_wl_check(&h, lab, 3, A, keys, colors, info, nullptr, 0, -1), GTOK_E_UNSUPPORTED);   // both, but no flag
    h.flags = SYM;
    EXPECT(graph_wl_check(&h, lab, 3, A, keys, colors, info, nullptr, 0, -1), CSR);
    EXPECT(graph_wl_check(&h, lab, 0, A, keys, colors, info, nullptr, 0, -1), CSR);
    EXPECT(graph_wl_check(&h, lab, 3, A, keys, colors, info, nullptr, 0, kWlReg), GTOK_E_UNSUPPORTED);
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, 0, -1), REG);
    h = g; h.num_graphs = 0;                                                                    // no graphs: a no-op, keys may be NULL
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, 0, -1), 1);
    EXPECT(graph_wl_check(&h, nullptr, 3, 0, nullptr, nullptr, info, nullptr, 0, -1), 1);
    EXPECT(graph_wl_check(&h, nullptr, 3, 0, nullptr, nullptr, nullptr, nullptr, 0, -1), GTOK_E_INVAL);
    EXPECT(graph_wl_check(&h, nullptr, 600, 0, nullptr, nullptr, info, nullptr, 0, -1), GTOK_E_INVAL);
    h.node_ptr = nullptr; h.edge_ptr = nullptr; h.rowptr = nullptr; h.col = nullptr;
    EXPECT(graph_wl_check(&h, nullptr, 3, 0, nullptr, nullptr, info, nullptr, 0, -1), 1);
    h = g; h.num_graphs = -1;
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, 0, -1), GTOK_E_INVAL);
    h = g; h.max_nodes = -1;
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, 0, -1), GTOK_E_INVAL);
    h = g; h.max_edges = -1;
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, 0, -1), GTOK_E_INVAL);
    h = g; h.graph_ids = i32.data();                                                            // a reordered batch
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, 0, -1), GTOK_E_INVAL);
    h = g; h.unit_ptr = i32.data();
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, 0, -1), GTOK_E_INVAL);
    h = g; h.unit_info = i32.data();
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, 0, -1), GTOK_E_INVAL);
    h = g; h.node_ptr = nullptr;
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, 0, -1), GTOK_E_INVAL);
    h = g; h.edge_ptr = nullptr;
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, 0, -1), GTOK_E_INVAL);
    h = g; h.rowptr = nullptr;
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, 0, -1), GTOK_E_INVAL);
    h = g; h.col = nullptr;
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, 0, -1), GTOK_E_INVAL);
    // graph size limits, the flag rule, rounds == 0
    h = g; h.max_nodes = 64;
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, 0, -1), REG);
    h.max_nodes = 65;
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, 0, -1), LDS);
    h.max_nodes = 512;
    EXPECT(graph_wl_check(&h, lab, 0, 0, keys, colors, info, nullptr, 0, -1), LDS);
    h.max_nodes = 513;
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, 0, -1), GTOK_E_UNSUPPORTED);
    h.flags = SYM;
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, 0, -1), CSR);
    EXPECT(graph_wl_check(&h, lab, 0, 0, keys, colors, info, nullptr, 0, -1), GTOK_E_UNSUPPORTED);
    h.max_nodes = 4096;
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, 0, -1), CSR);            // no workspace up to here
    // the workspace: 3 graphs of up to 4,097 nodes
    h.max_nodes = 4097;
    const int64_t need = graph_wl_workspace(4097, 3);
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, 0, -1), GTOK_E_INVAL);
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, need, -1), GTOK_E_INVAL);
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, wsbuf, need - 1, -1), GTOK_E_INVAL);        // short
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, wsbuf + 8, need, -1), GTOK_E_INVAL);        // misaligned
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, wsbuf, need, -1), CSR);                     // (the check reads no byte of it)
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, wsbuf, need + 16, -1), CSR);
    h.max_nodes = BIG + 1;
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, wsbuf, need, -1), GTOK_E_TOO_LARGE);
    EXPECT(graph_wl_check(&h, lab, 3, 4, keys, colors, info, wsbuf, need, -1), GTOK_E_INVAL);            // a bad flag wins over the size
    // the hook
    h = g;
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, 0, kWlLds), LDS);
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, 0, kWlCsr), GTOK_E_UNSUPPORTED);
    h.flags = SYM;
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, 0, kWlCsr), CSR);
    h.max_nodes = 100;
    EXPECT(graph_wl_check(&h, lab, 3, 0, keys, colors, info, nullptr, 0, kWlReg), GTOK_E_UNSUPPORTED);
  }
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
