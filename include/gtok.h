/*
 * gtok.h — C ABI of libgtok.so, the MI355X (gfx950) graph->sequence tokenizer.
 *
 * Every entry point replaces one piece of the reference's Python hot path
 * (paths relative to the reference checkout):
 *
 *   gtok_ibtt_zinc     graph_data_loader/zinc_dataset_indexbase.py:143-227
 *                      (tokenize_molecule + __getitem__ truncation) fused with
 *                      graph_data_loader/data_loader.py:465-484 (TokenDataset:
 *                      strip after <p>, vocab lookup, [:max_len])
 *   gtok_text_to_ids   graph_data_loader/data_loader.py:465-484 (TokenDataset on
 *                      arbitrary whitespace-tokenised text, any grammar)
 *   gtok_ibtt_synth    the graph-token index-based grammar
 *                      (docs/synthetic_data.md:46-68) emitted straight from the
 *                      edge list, then data_loader.py:479-482
 *   gtok_sent          autograph Graph2TrailTokenizer.__call__ as called at
 *                      trainer/train_agtt.py:250 (SENT walk; spec in DESIGN.md,
 *                      upstream parity unpinned), optionally fused with
 *                      remap_zinc_tokens (:171-244) and the query append (:257-267)
 *   gtok_sent_large    gtok_sent for batches it refuses: graphs of up to GTOK_SENT_LARGE_MAX_NODES nodes (the protein graphs and
 *                      point clouds of the model family), any edge list, with a caller-given workspace - same tokens
 *   gtok_sent_packed   gtok_sent whose walk also appends every row to a packed buffer (the payload of the all-gather behind the
 *                      val / test loaders, trainer/train_agtt.py:602-607, and of the D2H copy behind :246-273) - no second pass
 *   gtok_sent_decode   the SENT spec read backwards (token rows -> graphs in visit-index space)
 *   gtok_sent_decode_sizes / gtok_sent_decode_csr   the same, from int32 / 16-bit slabs or packed rows, a wave per row, into a
 *                      batched CSR (gtok_csr's arrays): what a generative model's sequences are turned back into
 *   gtok_unremap_zinc / gtok_sent_decode_zinc_sizes / gtok_sent_decode_zinc_csr   the way back from ZINC-REMAPPED labelled rows (what
 *                      every ZINC run trains on): the raw ids of the same walk, and the decoders above over them
 *   gtok_remap_zinc    trainer/train_agtt.py:171-244 on an existing token slab
 *   gtok_collate       data_loader.py:488-497 and trainer/train_agtt.py:276-302
 *                      (gather rows of a batch, pad to the batch max, bool mask)
 *   gtok_parse_graph_text  graph_token_dataset_autograph.py:14-158 (text -> edges, query, label)
 *   gtok_find_token    the `<q>` search of trainer/train_ibtt.py:88-103 on a collated batch
 *   gtok_row_offsets / gtok_pack_rows / gtok_pack_rows_u16 / gtok_pack_rows_scan / gtok_unpack_rows / gtok_unpack_rows_checked / gtok_unpack_rows_u16 / gtok_unpack_rows_at / gtok_collate_packed
 *                      (no reference counterpart) the packed form of a token slab - rows back to back, 16 or 32
 *                      bits per id - for the copies that leave the GPU: the all-gather that reassembles the rows of
 *                      every rank in dataset order (val/test loaders, trainer/train_agtt.py:602-607) and the D2H
 *                      copy behind TokenizedGraphDataset.__getitem__ (trainer/train_agtt.py:246-273); the readers also
 *                      take a [rows, ld] slab of 16-bit ids in place (row_ptr NULL): the per-batch collate of
 *                      trainer/train_agtt.py:276-302 straight over GTOK_SENT_U16 rows
 *   gtok_collate_epoch_plan / gtok_collate_epoch   trainer/train_agtt.py:276-302 for every batch of an epoch at once
 *   gtok_collate_batch  the same for one batch whose row list is a host array (what torch's DataLoader hands over)
 *   gtok_ids_to_text   graph_data_loader/zinc_dataset_indexbase.py:143-227, the STRING form (ids rendered through a string table)
 *   gtok_zinc_text_tails   zinc_dataset_indexbase.py:186-195, :217-221 (label token + <eos> / the max_len cut, per molecule)
 *   gtok_csr_check     (no reference counterpart; the property torch_geometric's coalesced undirected graphs have by construction -
 *                      zinc_dataset_autograph.py:51-73 passes them through) verifies GTOK_CSR_SIMPLE_SYMMETRIC on the device and
 *                      measures max_nodes / max_edges / max_degree
 *   gtok_csr_lane_sort (no reference counterpart) the reordered copy of a small-graph batch that the lane-per-graph SENT kernel
 *                      walks fastest (graph_ids / unit_ptr / unit_info + the permuted arrays and their byte mirror), built on
 *                      the device: what a caller of trainer/train_agtt.py:246-250's tokenizer prepares once per split
 *   gtok_csr_from_coo  the batched CSR from PyG collated storage (edge_index + slices['x'] / slices['edge_index'] + an optional
 *                      subset, graph_token_dataset_autograph.py:336-348, zinc_dataset_autograph.py:51-73) built on the device:
 *                      what GraphBatch.from_coo does on the host
 *   gtok_csr_pack8     (no reference counterpart) byte-packed mirror of the CSR index arrays of small-graph batches
 *   gtok_csr_adjbits   (no reference counterpart) adjacency bit-matrix mirror of batches of graphs with <= 256 nodes
 *   gtok_vocab_stats_text   the corpus pass of build_vocab_from_texts / the ZINC dynamic-token scan over arbitrary texts
 *   gtok_vocab_stats_synth  the corpus pass of build_vocab_from_texts
 *                      (data_loader.py:451-463) for graph-token corpora held as
 *                      CSR: per node-id token, occurrence count and first position
 *
 * Conventions: all pointers are DEVICE pointers borrowed from the caller
 * (never freed or retained), `stream` is a hipStream_t passed as void*, the
 * call only enqueues work on that stream (no synchronisation; the only allocation
 * is a small per-device block of work-queue counters on a device's FIRST launch,
 * so warm up once before capturing a hipGraph), outputs are caller-allocated.  Return value is
 * 0 or a negative GTOK_E_* code; nothing throws across the ABI.  Re-entrant.
 *
 * Output convention of every tokenizer entry point: out_ids is a row-major
 * [rows, ld] int32 slab; row g receives its first min(out_len[g], ld) ids and
 * pad_id after them; out_len[g] is the TRUE sequence length (already cut at
 * max_len as the reference does), so out_len[g] > ld tells the caller that
 * the slab was too narrow for that row.  gtok_sent only (ABI v4): epoch_count = K
 * makes that K slabs back to back ([K, G, ld], out_len [K, G]); GTOK_SENT_U16
 * makes the ids 16 bits wide; GTOK_SENT_NO_PAD leaves the pad tails unwritten.
 *
 * Batched CSR layout (gtok_csr), G graphs, graph g has N_g nodes and E_g
 * directed adjacency entries exactly as the source edge_index lists them:
 *   node_ptr[G+1]  int32  prefix sum of N_g
 *   edge_ptr[G+1]  int64  prefix sum of E_g
 *   rowptr[sum(N_g)+G] int32  graph g's N_g+1 LOCAL row pointers start at
 *                             node_ptr[g]+g; entry k of row u lives at
 *                             edge_ptr[g] + rowptr_g[u] + k
 *   col[sum E_g]   int32  local neighbour id
 *   eorder[sum E_g] int32 position of the entry in the graph's original COO
 *                         edge list (NULL = identity, i.e. edge_index was
 *                         already row-sorted); IBTT's first-occurrence rule
 *                         needs it
 *   nattr[sum N_g] uint8  node type (x); NULL for unlabelled graphs
 *   eattr[sum E_g] uint8  edge type (edge_attr); NULL for unlabelled graphs
 */
#ifndef GTOK_H
#define GTOK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GTOK_OK 0
#define GTOK_E_INVAL (-1)     /* null pointer / negative size / bad flag        */
#define GTOK_E_TOO_LARGE (-2) /* a graph exceeds the LDS-resident limits        */
#define GTOK_E_LAUNCH (-3)    /* hipLaunchKernel reported an error              */
#define GTOK_E_NO_DEVICE (-4) /* no gfx950 device visible                       */
#define GTOK_E_GRAPH_SLOTS (-5) /* a launch captured into a hipGraph needed a reserved block of work-queue counters and all 64
                                   per device are held by LIVE graphs: the ticket-scheduled kernels ("sent_lds_kernel",
                                   "sent_blane_kernel", "ibtt_zinc_lane_kernel", gtok_pack_rows_scan) keep one per captured launch for as long as the capturing graph
                                   (and the executable graphs made from it) exist - destroying a graph returns its blocks   */

#define GTOK_E_UNSUPPORTED (-6) /* the request is valid but not for the kernel this batch runs: gtok_sent_packed on a batch that
                                   gtok_sent_kernel_name() answers neither "sent_lane_kernel" nor "sent_blane_kernel<W=..>" for,
                                   or a "sent_blane_kernel" batch of fewer than 20,000 walks (graphs x epochs), with
                                   GTOK_SENT_PACK_U8, or with ld > 2040 (1020 at 32 bits).  Nothing was launched or written:
                                   use the two-call route (gtok_sent + gtok_pack_rows_scan).  Still ABI version 8: callers
                                   learn what a library packs in the walk from this code                                       */

#define GTOK_MAX_NODES 512 /* SENT adjacency bit-matrix rows per wave (LDS): gtok_sent / gtok_sent_packed only - gtok_sent_large walks larger graphs */

/* flags: properties the CALLER has verified for the whole batch (on the host, or with gtok_csr_check on the device) */
#define GTOK_CSR_SIMPLE_SYMMETRIC 1 /* simple undirected graphs, both directions stored: no self-loop, no entry
                                       listed twice, and (v,u) is listed whenever (u,v) is - every row is the
                                       node's complete neighbour list (PyG-coalesced molecules).  A batch flagged
                                       wrongly gets wrong tokens (never an out-of-bounds access).                */

typedef struct gtok_csr {
  int32_t num_graphs;
  int32_t max_nodes; /* max N_g over the batch (host-known)                 */
  int32_t max_edges; /* max E_g over the batch (host-known)                 */
  int32_t flags;     /* GTOK_CSR_* (0 = nothing known)                      */
  const int32_t *node_ptr;
  const int64_t *edge_ptr;
  const int32_t *rowptr;
  const int32_t *col;
  const int32_t *eorder;
  const uint8_t *nattr;
  const uint8_t *eattr;
  int32_t chunk_nodes; /* max over 64-graph groups [64i, 64i+64) of sum N_g; 0 = unknown (64*max_nodes assumed) */
  int32_t chunk_edges; /* same for sum E_g                                                                      */
  int32_t max_degree;  /* longest CSR row of the batch (upper bound accepted); 0 = unknown                       */
  int32_t reserved;    /* must be 0                                                                              */
  /* Byte-packed mirror of rowptr / col for batches of small graphs (max_edges <= 255, max_nodes <= 256), written
   * once per resident batch by gtok_csr_pack8 (same indexing as the int32 arrays); NULL = absent.  The
   * lane-per-graph SENT kernel stages its 64-graph chunks from these (a quarter of the index bytes).            */
  const uint8_t *rowptr8;
  const uint8_t *col8;
  /* Adjacency bit-matrix mirror for UNLABELLED batches of graphs with <= 256 nodes, written once per resident batch by
   * gtok_csr_adjbits; NULL = absent.  adj_rows[(node_ptr[g] + u) * adj_words + w] = word w of node u's row in the
   * symmetric closure of graph g's entries (self loops kept); adj_planes[(g * 8 + p) * adj_words + w] = bit p of the
   * degrees of nodes 64 w .. 64 w + 63; adj_max_degree = the largest degree (must be <= 255).  lane_order (optional):
   * the graphs in the order the lane-per-graph kernel deals them to lanes (64 per wave) - a permutation of 0..G-1
   * grouping walks of similar length; NULL = dataset order.  The SENT walk of such a batch reads one row per step.   */
  const uint64_t *adj_rows;
  const uint64_t *adj_planes;
  const int32_t *lane_order;
  int32_t adj_words;      /* 1, 2 or 4 = ceil(max_nodes / 64) rounded up to a power of two */
  int32_t adj_max_degree;
  /* A batch REORDERED for the lane-per-graph SENT kernel (optional; NULL / 0 = the batch is in dataset order).
   * graph_ids[s] = the dataset index of the graph stored at slot s: the row of the output slab, the entries of out_len
   * and `query`, and the RNG identity (graph_base + graph_ids[s]) follow it, so the result is that of the batch in
   * dataset order.  unit_ptr[num_units + 1] = the slots dealt to each wave (<= 64 per unit; chunk_nodes / chunk_edges
   * = the largest unit's sums).  Storing the graphs by descending walk length lets the 64 walks of a wave end together
   * (a wave lasts as long as its longest walk).  Only gtok_sent's lane-per-graph kernel accepts such a batch
   * (GTOK_E_INVAL from every other entry point and when another SENT kernel would be chosen).                      */
  const int32_t *graph_ids;
  const int32_t *unit_ptr;
  int32_t num_units;
  int32_t reserved2;
  /* Optional (NULL = derived from unit_ptr / node_ptr / edge_ptr by the kernel; ABI v4): one 32-byte record per unit of a
   * reordered batch, unit_info[8 u ..] = { unit_ptr[u], unit_ptr[u + 1], node_ptr[g0], node_ptr[gl], edge_ptr[g0] (low,
   * high word), edge_ptr[gl] (low, high) } - everything a wave needs to request its unit's chunk arrives in ONE scalar
   * load instead of a chain of two (a unit's staging is a chain of dependent HBM round trips: ~2 us each at launch start,
   * when every resident wave stages at once).                                                                      */
  const int32_t *unit_info;
} gtok_csr;

/* LUT layout for gtok_ibtt_zinc (int32 vocab ids; an absent token holds pad_id
 * exactly as TokenDataset's vocab.get(tok, vocab['<pad>']) would give):
 *   [0] <bos> [1] <eos> [2] <atom> [3] <bond> [4] <q> [5] regression [6] <p>
 *   [7..16]  atom symbols C N O F P S Cl Br I, then 'X'   (x outside 0..8)
 *   [17..21] 'unknown', single, double, triple, aromatic  (index = attr if 1..4 else 0)
 *   [22..22+n) decimal strings "0".."n-1"                  (node indices) */
#define GTOK_ZLUT_BOS 0
#define GTOK_ZLUT_EOS 1
#define GTOK_ZLUT_ATOM 2
#define GTOK_ZLUT_BOND 3
#define GTOK_ZLUT_Q 4
#define GTOK_ZLUT_REGRESSION 5
#define GTOK_ZLUT_P 6
#define GTOK_ZLUT_ATOM0 7
#define GTOK_ZLUT_BOND0 17
#define GTOK_ZLUT_NODE0 22

/* rowptr8[i] = (uint8_t)rowptr[i], col8[i] = (uint8_t)col[i] for the whole batch (sum N + G and sum E elements).
 * GTOK_E_TOO_LARGE when max_edges > 255 or max_nodes > 256 (values would not fit).  No reference counterpart: a
 * data-layout step, done once when a batch becomes resident, like the CSR build itself.                       */
int gtok_csr_pack8(const gtok_csr *g, int64_t num_rowptr, int64_t num_col, uint8_t *rowptr8, uint8_t *col8, void *stream);

/* What GTOK_CSR_SIMPLE_SYMMETRIC claims, verified on the device (ABI v5), and the batch maxima a caller may not know:
 * info = int32[8] in device memory (zeroed by the call), after the stream has run it holds
 *   [0] violations: 0 <=> every graph is simple and stored in both directions (no self loop, no (u,v) listed twice, (v,u)
 *       listed whenever (u,v) is) AND the arrays are well-formed (sizes >= 0, row pointers start at 0, never decrease and end
 *       at E_g, neighbour ids inside [0, N_g)) - only then may flags carry GTOK_CSR_SIMPLE_SYMMETRIC;
 *   [1] the longest row (max_degree)   [2] max N_g (max_nodes)   [3] max E_g (max_edges)   [4..7] 0.
 * Of *g only num_graphs and the five array pointers are read (col may be NULL when max_edges == 0 is claimed: the entry
 * checks are then skipped); a batch in dataset order only (graph_ids / unit_ptr set: GTOK_E_INVAL).  Nothing is read through an
 * offset that has not been range-checked first, so a damaged batch yields violations, never a fault - PROVIDED node_ptr /
 * edge_ptr hold num_graphs + 1 entries and rowptr / col as many elements as those two say.                                */
int gtok_csr_check(const gtok_csr *g, int32_t *info, void *stream);

/* The reordered copy of a batch of small graphs (max_nodes <= 64, max_edges <= 255: GTOK_E_TOO_LARGE otherwise) that
 * gtok_sent's lane-per-graph kernel walks fastest, built on the device in a dozen small launches and no host round trip
 * (ABI v5).  Graphs are stored by descending (nodes + rows of length 1) - the expected walk length: a walk restarts once per
 * dead end - ties in dataset order, and cut greedily into units of <= 64 graphs whose node and entry sums fit `lds_budget`
 * bytes of LDS per wave (0 = 10224: 16 resident waves per CU share its 160 KB), the budget being split between the two in
 * the corpus' own proportion.  Outputs (device memory, caller-allocated, G = num_graphs, N / E = the batch's node / entry
 * totals):
 *   graph_ids int32[G]        dataset index of the graph at every stored slot
 *   node_ptr  int32[G + 1], edge_ptr int64[G + 1], rowptr int32[N + G], col int32[E], nattr / eattr uint8[N] / [E] (only
 *                             when the batch has them): the batch in stored order, same layout as gtok_csr
 *   rowptr8   uint8[N + G + 16], col8 uint8[E + 16]   (optional, NULL = skip) the byte mirror of the two (gtok_csr_pack8)
 *   unit_ptr  int32[G + 1]    first slot of every unit, num_units + 1 entries used
 *   unit_info int32[8 G]      one record per unit (gtok_csr.unit_info), 8 num_units entries used
 *   info      int32[8]        as gtok_csr_check ([0] only when check != 0, else 0) + [4] num_units, [5] chunk_nodes,
 *                             [6] chunk_edges (the largest unit's node and entry sums)
 * The caller reads `info` back once (the only host read of the whole preparation), fills a gtok_csr with the new arrays,
 * flags (GTOK_CSR_SIMPLE_SYMMETRIC if verified), max_degree = info[1], chunk_nodes / chunk_edges, graph_ids, unit_ptr,
 * num_units, unit_info, rowptr8 / col8, and passes that to gtok_sent.  `workspace`: gtok_csr_lane_sort_workspace(G) bytes of
 * device memory, 16-byte aligned, free again when the stream has run the call.                                            */
typedef struct gtok_csr_sorted {
  int32_t *graph_ids;
  int32_t *node_ptr;
  int64_t *edge_ptr;
  int32_t *rowptr;
  int32_t *col;
  uint8_t *nattr;
  uint8_t *eattr;
  uint8_t *rowptr8;
  uint8_t *col8;
  int32_t *unit_ptr;
  int32_t *unit_info;
  int32_t *info;
} gtok_csr_sorted;
int64_t gtok_csr_lane_sort_workspace(int32_t num_graphs);
int gtok_csr_lane_sort(const gtok_csr *g, int32_t lds_budget, int32_t check, const gtok_csr_sorted *out, void *workspace,
                       int64_t workspace_bytes, void *stream);

/* The batched CSR (gtok_csr's arrays) built on the device from PyG collated storage (ABI v7): `edge_index` int64 [2, sum E]
 * with LOCAL node ids, slices['x'] / slices['edge_index'], optional x / edge_attr, optional subset `indices`
 * (dataset._indices) - what graph_token_dataset_autograph.py:336-348 and zinc_dataset_autograph.py:51-73 hold.  Inputs
 * (device memory, S = num_source_graphs, G = num_graphs):                                                              */
typedef struct gtok_coo {
  int32_t num_graphs;          /* G: graphs of the batch to build                                                  */
  int32_t num_source_graphs;   /* S: graphs in the storage (must equal G when indices == NULL)                    */
  int64_t num_nodes;           /* sum N of the batch to build (host-known: x.shape[0], slices[-1], the counts)     */
  int64_t num_entries;         /* sum E of the batch to build                                                      */
  const int64_t *node_slices;  /* [S + 1] slices['x']: graph s holds storage nodes [node_slices[s], node_slices[s+1]) */
  const int64_t *edge_slices;  /* [S + 1] slices['edge_index']: likewise for the entries                           */
  const int64_t *indices;      /* [G] storage graph of batch graph i; NULL = 0 .. S - 1                             */
  const int64_t *src;          /* edge_index[0]: local row of every storage entry                                   */
  const int64_t *dst;          /* edge_index[1]: local column                                                      */
  const int64_t *x;            /* node type of storage node v at x[v * x_stride] (x[:, 0]); NULL = no node types    */
  int64_t x_stride;            /* in elements, >= 1                                                                 */
  const int64_t *edge_attr;    /* edge type of storage entry t at edge_attr[t * edge_attr_stride]; NULL = none      */
  int64_t edge_attr_stride;
} gtok_coo;
/* Outputs (device memory, caller-allocated, N / E = num_nodes / num_entries):
 *   node_ptr int32[G + 1], edge_ptr int64[G + 1], rowptr int32[N + G], col int32[E]: gtok_csr's layout; entries are
 *       ordered by row with a STABLE sort (a row lists its entries in edge_index order), rowptr holds each graph's local row
 *       starts and then E_g
 *   eorder   int32[E]   always written: every entry's position in its graph's own edge list (the identity for a graph whose
 *                       entries were already row-sorted; pass it as gtok_csr.eorder only when info[7] != 0)
 *   nattr    uint8[N], eattr uint8[E]   when x / edge_attr are given: values 0..254 kept, everything else 255
 *   info     int32[8]   [0] violations as gtok_csr_check counts them (0 <=> every graph simple and stored in both
 *                       directions; 0 when check == 0), [1] max_degree, [2] max_nodes, [3] max_edges, [4] chunk_nodes,
 *                       [5] chunk_edges (maxima over aligned groups of 64 graphs of the summed counts), [6] input status:
 *                       GTOK_COO_* bits below, [7] 1 when some graph had to be sorted (eorder is not the identity)
 * A damaged input raises bits of info[6] and never faults: the slices and indices are validated before anything is read
 * through them and the scanned totals are compared with num_nodes / num_entries before anything is written with them
 * (their bits leave every output but info undefined), PROVIDED the arrays hold as many elements as their slices say.
 * An endpoint outside [0, N_g) leaves that graph's arrays undefined.  An unsorted graph of more than GTOK_COO_SORT_NODES
 * nodes (its row cursors live in LDS; its entry count is not bounded) raises GTOK_COO_SORT_TOO_LARGE and its arrays are
 * undefined.  The symmetry check uses a bit matrix in LDS for graphs of up to 256 nodes and gtok_csr_check's row scan for
 * larger ones.  Everything is enqueued on `stream` (four launches) with no allocation and no host synchronisation, so the
 * call can be captured into a hipGraph; the caller reads `info` back once.  `workspace`: gtok_csr_from_coo_workspace(G, S)
 * bytes of device memory, 16-byte aligned, free again when the stream has run the call.                              */
#define GTOK_COO_BAD_ENDPOINT   1   /* an endpoint outside [0, N_g)                                           */
#define GTOK_COO_BAD_SLICES     2   /* slices that decrease, do not start at 0, or a graph of >= 2^31 entries */
#define GTOK_COO_BAD_TOTALS     4   /* the scanned totals differ from num_nodes / num_entries                 */
#define GTOK_COO_BAD_INDEX      8   /* an index outside [0, S)                                                 */
#define GTOK_COO_SORT_TOO_LARGE 16  /* an unsorted graph of more than GTOK_COO_SORT_NODES nodes               */
#define GTOK_COO_SORT_NODES 4096
typedef struct gtok_csr_built {
  int32_t *node_ptr;
  int64_t *edge_ptr;
  int32_t *rowptr;
  int32_t *col;
  int32_t *eorder;
  uint8_t *nattr;
  uint8_t *eattr;
  int32_t *info;
} gtok_csr_built;
int64_t gtok_csr_from_coo_workspace(int32_t num_graphs, int32_t num_source_graphs);
int gtok_csr_from_coo(const gtok_coo *in, int32_t check, const gtok_csr_built *out, void *workspace, int64_t workspace_bytes,
                      void *stream);

/* Adjacency bit-matrix mirror (see gtok_csr.adj_rows): rows = [sum N_g][words] uint64, planes = [G][8][words] uint64,
 * info = int32[1], zeroed by the caller, receives the largest closure degree.  words = 1, 2 or 4 with 64 * words >=
 * max_nodes (GTOK_E_TOO_LARGE otherwise).  Works on any edge list (one or both directions, duplicates, self loops).
 * A data-layout step like gtok_csr_pack8: done once when a batch becomes resident, not per epoch.                    */
int gtok_csr_adjbits(const gtok_csr *g, int32_t words, uint64_t *rows, uint64_t *planes, int32_t *info, void *stream);

/* IBTT molecular serialiser -> ids.
 * lut_len = 22 + number of node-index entries (must cover max_nodes).      */
int gtok_ibtt_zinc(const gtok_csr *g, const int32_t *lut, int32_t lut_len,
                   int32_t max_len, int32_t pad_id, int32_t *out_ids,
                   int32_t ld, int32_t *out_len, void *stream);

/* LUT layout for gtok_ibtt_synth:
 *   [0] <bos> [1] <e> [2] <n> [3] <q> [4] <p>  [5..5+n) "0".."n-1"           */
#define GTOK_SLUT_BOS 0
#define GTOK_SLUT_E 1
#define GTOK_SLUT_N 2
#define GTOK_SLUT_Q 3
#define GTOK_SLUT_P 4
#define GTOK_SLUT_NODE0 5

/* graph-token grammar "<bos> u v <e> ... <n> 0 1 .. N-1 <q> q0 [q1 q2] <p>":
 * edges in ORIGINAL order (needs eorder unless identity), query[g*4+0] =
 * number of query ids (0..3), query[g*4+1..3] = the vocab ids after <q>.     */
int gtok_ibtt_synth(const gtok_csr *g, const int32_t *lut, int32_t lut_len,
                    const int32_t *query, int32_t max_len, int32_t pad_id,
                    int32_t *out_ids, int32_t ld, int32_t *out_len,
                    void *stream);

/* Open-addressing vocab table for gtok_text_to_ids, built on the host by
 * the Python mirror (capacity a power of two): slot s holds key_off[s] (byte
 * offset of the token string in key_bytes, -1 = empty), key_len[s], id[s].
 * Hash = 32-bit FNV-1a of the token bytes; probe linearly.                   */
typedef struct gtok_vocab_table {
  int32_t capacity;
  int32_t pad_id;
  const int32_t *key_off;
  const int32_t *key_len;
  const int32_t *id;
  const uint8_t *key_bytes;
} gtok_vocab_table;

/* TokenDataset: texts are concatenated ASCII bytes, text g = bytes
 * [text_ptr[g], text_ptr[g+1]).  Splits on Python str.split() ASCII
 * whitespace, keeps tokens up to and including the first "<p>" when
 * strip_label != 0, maps through the table (miss -> pad_id), cuts at
 * max_len.                                                                   */
int gtok_text_to_ids(const uint8_t *bytes, const int64_t *text_ptr,
                     int32_t num_texts, const gtok_vocab_table *vocab,
                     int32_t strip_label, int32_t max_len, int32_t *out_ids,
                     int32_t ld, int32_t *out_len, void *stream);

#define GTOK_SENT_SOS 0
#define GTOK_SENT_RESET 1
#define GTOK_SENT_LADJ 2
#define GTOK_SENT_RADJ 3
#define GTOK_SENT_EOS 4
#define GTOK_SENT_PAD 5
#define GTOK_SENT_IDX_OFFSET 6

/* gtok_sent_params.flags */
#define GTOK_SENT_NO_PAD 1 /* rows are only guaranteed up to out_len[g] (rounded up to a multiple of 16 ids); the pad tails -
                              56 % of a ZINC slab - may be left unwritten.  For callers that read rows through out_len
                              anyway (gtok_collate pads per batch, as both reference collates do).                  */
#define GTOK_SENT_U16 2    /* out_ids points at uint16_t storage: a [rows, ld] slab of 16-bit ids (ld still counts ids).  Every
                              SENT id fits (gtok_sent checks the id space and pad_id against 65535): the walk kernels hold
                              tokens 16 bits each anyway, so the rows leave as they are - half the bytes of the int32 slab,
                              no unpacking.  The reference never materialises a padded corpus slab (it pads per batch,
                              trainer/train_agtt.py:276-302); readers: gtok_collate_packed / gtok_unpack_rows with
                              row_ptr == NULL (the slab read in place) and gtok_pack_rows_u16.  The int32 slab stays the
                              documented default.                                                                   */

typedef struct gtok_sent_params {
  int32_t max_num_nodes;  /* tokenizer.set_num_nodes()                      */
  int32_t labeled;        /* labeled_graph: emit node/edge type tokens      */
  int32_t num_node_types; /* set_num_node_and_edge_types()                  */
  int32_t num_edge_types;
  int32_t max_len;        /* max_length == truncation_length                */
  int32_t remap_zinc;     /* fuse TokenizedGraphDataset.remap_zinc_tokens   */
  int32_t pad_id;         /* slab fill (Graph2TrailTokenizer.pad = 5)       */
  int32_t flags;          /* GTOK_SENT_* (0 = the documented output convention) */
  uint64_t seed;          /* Philox key                                     */
  uint64_t epoch;         /* a new trail every epoch                        */
  int64_t graph_base;     /* global index of graph 0 (shard-invariant RNG)  */
  const int32_t *query;   /* NULL, or [G,2] (query_u, query_v): appends
                             idx_off+N, idx_off+u, idx_off+v after the trail */
  int32_t epoch_count;    /* K epochs in ONE launch (0 and 1 both mean one): epoch slice e = 0..K-1 holds the trails of
                             epoch `epoch + e` - out_ids is [K, G, ld], out_len [K, G], `query` is shared.  The trainer
                             re-tokenizes the same split every epoch (trainer/train_agtt.py:246-250, epoch loop :676-680)
                             and a trail is a pure function of (seed, epoch, graph_base + g): K epochs of a small split
                             fill the chip where one epoch cannot (ABI v4).                                        */
  int32_t reserved;       /* must be 0                                      */
} gtok_sent_params;

/* SENT trail walk -> ids.  out_len[g] = min(trail, max_len) (+3 if query).  With epoch_count = K > 1 the result is
 * that of K calls with epoch, epoch + 1, ... written to consecutive [G, ld] slices.                               */
int gtok_sent(const gtok_csr *g, const gtok_sent_params *p, int32_t *out_ids,
              int32_t ld, int32_t *out_len, void *stream);

/* ---- the constants mirror of a reordered batch: what the lane-per-graph walk would otherwise recompute in every epoch ---------
 * A labelled walk with the ZINC remap turns every attribute byte it visits into a token, and the result depends only on the byte
 * and on (max_num_nodes, num_node_types, num_edge_types) - settings a tokenizer fixes for the life of a dataset.  The mirror
 * holds those tokens, computed once per resident batch and settings:
 *   ntok8[N]  the token of every node type:  gtok_sent's remapped node-type token of nattr[i]
 *   etok8[E]  the token of every entry type: gtok_sent's remapped edge-type token of eattr[i]
 * indexed as nattr / eattr of the SAME (reordered) batch; the kernel stages them in place of the attribute bytes and emits a
 * byte as it stands (no range compare, no add per token).  gtok_sent_lane_consts builds the two arrays (device memory,
 * caller-allocated: num_nodes / num_entries bytes, the batch's node and entry totals) with a thread per byte and zeroes *status
 * (int32, device memory) first; bit 0 of it is set when a token does not fit a byte (an attribute of 255, a large
 * max_num_nodes): the mirror must then not be used.  The caller reads the status back once, at build time.  The builder reads
 * nattr / eattr below the two totals only, and nothing through an offset.  GTOK_E_INVAL: null pointers, negative totals, a
 * batch without graph_ids / unit_ptr or without attributes, p not labelled with remap_zinc.  (Added without an ABI version
 * step: no struct changes - a library may lack the two entry points.)
 * gtok_sent_prepared is gtok_sent with the mirror: consts == NULL is gtok_sent itself; otherwise GTOK_E_INVAL unless the batch
 * runs the lane-per-graph kernel from its byte mirror (graph_ids, unit_ptr, rowptr8, col8), p is labelled with remap_zinc and
 * p's three settings equal the recorded ones.  The arrays are only ever read as token VALUES, at the offsets nattr / eattr are
 * read at: a stale mirror gives wrong tokens and never widens what the kernel addresses.                                     */
typedef struct gtok_sent_consts {
  const uint8_t *ntok8;
  const uint8_t *etok8;
  int32_t max_num_nodes;  /* the settings the mirror was built for */
  int32_t num_node_types;
  int32_t num_edge_types;
  int32_t reserved;       /* must be 0 */
} gtok_sent_consts;
int gtok_sent_lane_consts(const gtok_csr *g, const gtok_sent_params *p, int64_t num_nodes, int64_t num_entries, uint8_t *ntok8,
                          uint8_t *etok8, int32_t *status, void *stream);
int gtok_sent_prepared(const gtok_csr *g, const gtok_sent_params *p, const gtok_sent_consts *consts, int32_t *out_ids,
                       int32_t ld, int32_t *out_len, void *stream);

/* ---- gtok_sent_large: the SENT walk for graphs of more than GTOK_MAX_NODES nodes -------------------------------------------
 * Same spec, same tokens, same output convention as gtok_sent (bit-exact against oracle_sent), for ANY batch in dataset order
 * whose largest graph has at most GTOK_SENT_LARGE_MAX_NODES nodes - small graphs included, so a caller need not split a
 * batch.  Any edge list: one direction or both (the walk forms the symmetric closure itself - the graph-token datasets list
 * every edge once, graph_token_dataset_autograph.py:336-348), duplicates, self loops, unsorted rows; with or without
 * GTOK_CSR_SIMPLE_SYMMETRIC (with it the walk skips building the lists of entries that name a node from other rows), labelled
 * or not.  Honours remap_zinc, query, graph_base, epoch_count = K ([K, G, ld], epoch-major), GTOK_SENT_NO_PAD and GTOK_SENT_U16
 * (GTOK_E_TOO_LARGE when an id cannot fit 16 bits, gtok_sent's rule: 6 + max_num_nodes + num_node_types + 512 <= 65535).
 * out_len is the true length cut at max_len (max_len beyond 0x70000000 reads as that): the walk keeps counting past ld.
 * One wave walks one (graph, epoch) pair; a launch has at most GTOK_SENT_LARGE_WAVES waves and wave w takes pairs w,
 * w + waves, ... - `workspace` holds one slice per wave (12 bytes per node + 8 per entry of the batch's maxima):
 * gtok_sent_large_workspace(max_nodes, max_edges, num_graphs x epochs) bytes of device memory, 16-byte aligned, contents
 * unspecified before and after, free again when the stream has run the call.  The call only enqueues on `stream`: no
 * allocation, no host synchronisation, no library-owned counters.
 * Errors, all before anything is launched: GTOK_E_INVAL for null pointers / bad sizes, a reordered batch (graph_ids / unit_ptr
 * set), labelled without attributes, GTOK_SENT_PACK_ONLY / GTOK_SENT_PACK_U8, a workspace that is misaligned or smaller than
 * gtok_sent_large_workspace() says; GTOK_E_TOO_LARGE for max_nodes beyond GTOK_SENT_LARGE_MAX_NODES.  An entry with an endpoint
 * outside [0, N_g) is skipped (as the oracle does); a graph whose real N or E exceeds the batch's max_nodes / max_edges is
 * clamped to them: wrong tokens, never an access outside its slice or its row.  Packed rows of such batches come from
 * gtok_pack_rows_scan over the slab.  (Added without an ABI version step, like GTOK_E_UNSUPPORTED: no struct changes - a
 * binding learns that a library has it from the symbol.)
 * gtok_sent_large_workspace: pure host arithmetic (no device, no pointer is touched); a multiple of 16; GTOK_E_INVAL for a
 * negative argument, GTOK_E_TOO_LARGE beyond GTOK_SENT_LARGE_MAX_NODES.                                                     */
#define GTOK_SENT_LARGE_MAX_NODES 16384 /* largest graph gtok_sent_large walks */
#define GTOK_SENT_LARGE_WAVES 1024      /* most walks in flight in one launch: the workspace holds one slice per wave */
int64_t gtok_sent_large_workspace(int32_t max_nodes, int32_t max_edges, int64_t walks);
int gtok_sent_large(const gtok_csr *g, const gtok_sent_params *p, int32_t *out_ids, int32_t ld, int32_t *out_len,
                    void *workspace, int64_t workspace_bytes, void *stream);

/* gtok_sent_large's walk that also - or only - exports its VISIT ORDER: what maps a decoded SENT graph (visit-index space,
 * gtok_sent_decode_csr) back to the input's node ids.
 *   visit_index[e * order_stride + node_ptr[g] + u] = k: node u of graph g was the k-th node first visited by the walk of epoch
 *   p->epoch + e; the position token GTOK_SENT_IDX_OFFSET + k names it.  -1: the walk had not visited u when it stopped (a row cut
 *   at max_len; a node beyond a clamped max_nodes).
 * The walk stops at the first loop test with pos >= max_len, so a visit that BEGAN below max_len is recorded even when its position
 * token falls just behind the cut: a reader that pairs the order with a decoded, cut row treats an index >= the decoded node count
 * as absent (gtok_csr_relabel does).  order_stride (elements) >= the batch's node total node_ptr[G], which the host knows; the array
 * holds K * order_stride int32, K = max(epoch_count, 1); elements of a block beyond the node total are not touched.
 * Every SENT kernel emits the same tokens for the same (seed, epoch, graph_base + g), so this is the order of the rows of gtok_sent
 * and gtok_sent_packed as well, whichever kernel wrote them: any batch in dataset order is accepted, small graphs included.  The
 * visit index of a node depends on (seed, epoch, graph_base + g) and the edge list only - not on labeled, remap_zinc, query or the
 * row width; how far a cut walk got depends on max_len and, through the tokens a visit costs, on labeled: pass the max_len and
 * labeled the rows were written with.
 * out_ids / out_len: both set - rows and lengths bit for bit gtok_sent_large's, from the same launch; both NULL - an order-only call:
 * no token is stored, ld, query, GTOK_SENT_U16 and GTOK_SENT_NO_PAD are ignored; one of the two NULL: GTOK_E_INVAL.  Everything else -
 * batch rules, errors, the workspace (gtok_sent_large_workspace), one wave per (graph, epoch) pair, at most GTOK_SENT_LARGE_WAVES
 * waves - is gtok_sent_large's; also GTOK_E_INVAL: visit_index NULL, order_stride < 0.  Argument errors are answered before any
 * device is asked for.  The export is one coalesced 32-bit store per node when a walk ends.  (Added without an ABI version step.)  */
int gtok_sent_large_order(const gtok_csr *g, const gtok_sent_params *p, int32_t *out_ids, int32_t ld, int32_t *out_len,
                          int32_t *visit_index, int64_t order_stride, void *workspace, int64_t workspace_bytes, void *stream);

/* gtok_sent whose walk ALSO appends every row to a packed buffer (ABI v6): the payload of the compact all-gather and of the
 * per-epoch D2H copy without a second pass over the rows.  `packed` holds `capacity` ids of the slab's width (16-bit with
 * GTOK_SENT_U16, else 32-bit; one byte per id with GTOK_SENT_PACK_U8, below).  The library cuts it into R <= GTOK_PACK_REGIONS equal regions of (capacity / R rounded down to a
 * multiple of 8) ids, each with a fill mark of its own - one mark for all 64-graph units costs as much as the walk - and deals
 * the units to the regions so that they fill evenly (R = the largest power of two that leaves every region >= 64 (unit, epoch)
 * pairs; a ZINC-full epoch: 32 regions that end within 1 % of each other): size `capacity` as the expected total + a few
 * per cent.  state (int64 [GTOK_PACK_STATE_WORDS], ZEROED BY THE CALLER before every launch): [0] collects status bits (bit 1:
 * a unit's rows did not fit its region; they are skipped and their row_start is -1), [GTOK_PACK_STATE_FILL + GTOK_PACK_STATE_STRIDE * r]
 * is region r's fill mark in ids (it counts skipped units too).  row_start[e * G + g] (int64 [K * G]) = first id of that row in
 * `packed`: rows start on 16-byte boundaries and lie in the order in which the units finished, NOT in dataset order - readers go
 * through row_start (gtok_unpack_rows_at, gtok_collate_packed with row_ptr = row_start).  Row r holds min(out_len[r], ld) ids;
 * the slab itself is written as gtok_sent writes it (pass GTOK_SENT_NO_PAD when nobody reads its pad tails).  Needs ld % 8 == 0
 * (% 4 for 32-bit ids), 16-byte aligned out_ids / packed (else GTOK_E_INVAL), and a batch that runs one of the two lane-per-graph
 * kernels: the molecule kernel (sent_lane_kernel; ld <= 2040 / 1020, wider: GTOK_E_TOO_LARGE), or the bit-matrix kernel
 * (sent_blane_kernel: unlabelled graphs of up to 256 nodes, all of config 5) when ALL of these hold:
 *   - num_graphs x epochs >= 20,000 walks, whether the kernel was chosen or pinned (fewer pairs than that do not fill regions),
 *   - no GTOK_SENT_PACK_U8 (position ids reach 6 + 255 in its batches: 8-bit rows of such batches come from gtok_pack_rows_scan,
 *     which raises status bit 0 where an id does not fit),
 *   - ld <= 2040 at 16 bits / 1020 at 32 bits (a row's 16-byte pieces are counted in 8 bits).
 * Everything else answers GTOK_E_UNSUPPORTED before anything is launched or written: call gtok_sent + gtok_pack_rows_scan.   */
#define GTOK_SENT_PACK_ONLY 4 /* gtok_sent_params.flags, gtok_sent_packed only: the caller reads the PACKED rows alone - out_ids is then staging
                                space of gtok_sent_pack_scratch_rows() rows x ld ids (contents unspecified afterwards) instead of a
                                [K, G, ld] slab: every resident wave reuses its 64 rows for all of its units, the row stores stay in
                                the caches and K epochs need 92 MB of staging on an MI355X instead of K slabs.  Implies
                                GTOK_SENT_NO_PAD.                                                                              */
#define GTOK_SENT_PACK_U8 8   /* gtok_sent_params.flags, gtok_sent_packed only and only together with GTOK_SENT_U16 (ABI v8): `packed` holds
                                `capacity` ONE-byte ids (the slab, or the GTOK_SENT_PACK_ONLY staging rows, stay 16-bit).  row_start, the
                                fill marks and capacity count ids = bytes; rows start on 16-byte boundaries = multiples of 16 ids, a
                                region is (capacity / R rounded down to a multiple of 16) ids, the bytes between a row's end and the
                                next boundary are zeros.  An id that does not fit 8 bits raises bit 0 (value 1) of state[0]: the
                                buffer is not to be used, walk again with 16-bit packed rows (type attributes are passed through
                                un-clamped, so the id space is a property of the data, not of the parameters).  Needs ld % 16 == 0
                                (a staged row is a whole number of PAIRS of 16-byte pieces; GTOK_E_INVAL otherwise); ld <= 2040 as
                                for 16-bit rows.  gtok_sent refuses the flag (GTOK_E_INVAL).                                       */
#define GTOK_PACK_REGIONS 64
#define GTOK_PACK_STATE_FILL 16    /* the fill marks start one cache line behind the status word ... */
#define GTOK_PACK_STATE_STRIDE 16  /* ... and keep a cache line each                                   */
#define GTOK_PACK_STATE_WORDS (GTOK_PACK_STATE_FILL + GTOK_PACK_STATE_STRIDE * GTOK_PACK_REGIONS)
int gtok_sent_packed(const gtok_csr *g, const gtok_sent_params *p, int32_t *out_ids, int32_t ld, int32_t *out_len,
                     void *packed, int64_t capacity, int64_t *row_start, int64_t *state, void *stream);
/* rows of staging space a GTOK_SENT_PACK_ONLY launch on the stream's device needs (64 per wave the device can hold: 262,144 on an
 * MI355X), or a negative GTOK_E_* code                                                                                          */
int64_t gtok_sent_pack_scratch_rows(void *stream);

/* remap_zinc_tokens over the first len[g] ids of every row, in place or not. */
int gtok_remap_zinc(const int32_t *in_ids, int32_t *out_ids, int32_t ld,
                    const int32_t *len, int32_t num_rows, int32_t idx_offset,
                    int32_t node_idx_offset, int32_t edge_idx_offset,
                    void *stream);

/* Batch collate: rows index[b] of the [*, ld] slab -> X[B, out_ld] int64
 * (pad_id beyond the row length; columns >= the batch max stay pad) and
 * attn[B, out_ld] uint8 (bool).  batch_max[0] receives max length.          */
int gtok_collate(const int32_t *ids, int32_t ld, const int32_t *len,
                 const int64_t *index, int32_t batch, int32_t pad_id,
                 int64_t *out_x, uint8_t *out_attn, int32_t out_ld,
                 int32_t *batch_max, void *stream);

/* graph-token text -> edge list: parse_graph_from_text / parse_query_nodes_from_text /
 * parse_label_from_text (graph_token_dataset_autograph.py:14-113) and the num_nodes rule of
 * parse_graph_from_json (:116-158) for texts in the canonical form
 *   <bos> (INT INT <e>)* <n> INT* [<q> WORD [INT INT]] [<p> WORD] ...
 * Texts as for gtok_text_to_ids.  Two passes: with edge_ptr == NULL only the per-text results are
 * written (num_edges[g], num_nodes[g], query_nodes[2g..] = (u, v) or (-1, -1), label[g] = 1/0 for
 * yes/no, K-1 for lenK, INT32_MIN for none, status[g]); the caller prefix-sums num_edges into
 * edge_ptr[G+1] and calls again with src/dst to receive the edges in text order.  status 1 marks a
 * text that is not in that form (token out of place, integer of more than 9 digits, several
 * <n>/<q>/<p>, `len` + junk): its other outputs are undefined and the host parser must take it. */
/* Sizing pass for gtok_parse_graph_text without the parse: num_edges[g] = the number of places in text g where the three
 * bytes `<e>` stand (for a text in the canonical form: its number of `<e>` tokens = its number of edges; for any text: never
 * less than its `<e>` tokens, so a range sized by it holds whatever the parse writes).  A streaming kernel, against one full
 * parse per pass of gtok_parse_graph_text: prefix-sum it into edge_ptr and make ONE parsing call with src / dst; a text's
 * edges are its first num_edges[g] slots as that call reports them (squeeze the ranges where the two counts differ).        */
int gtok_count_edge_tokens(const uint8_t *bytes, const int64_t *text_ptr, int32_t num_texts, int32_t *num_edges,
                           void *stream);
int gtok_parse_graph_text(const uint8_t *bytes, const int64_t *text_ptr, int32_t num_texts,
                          const int64_t *edge_ptr, int32_t *src, int32_t *dst, int32_t *num_edges,
                          int32_t *num_nodes, int32_t *query_nodes, int32_t *label, int32_t *status,
                          void *stream);

/* ---- packed (ragged) rows -------------------------------------------------------------------------------------
 * The padded slab is the documented output of every tokenizer entry point; more than half of a ZINC slab is padding
 * and every id fits 16 bits (8 bits for ZINC molecules).  The packed form holds row r's n_r = min(len[r], ld) ids contiguously,
 * `elem_bytes` (1, 2 or 4; 1 since ABI v8, accepted by every entry point of this block) bytes each, from element row_ptr[r] of
 * `packed`.
 *
 * gtok_row_offsets: row_ptr[0] = 0, row_ptr[r + 1] = row_ptr[r] + round_up(n_r, align) for r < num_rows (int64
 * [num_rows + 1], align a power of two: 8 keeps every row start 16-byte aligned at 2 bytes per id, 16 at 1 byte per id - the
 * fast path of pack / unpack - 1 packs tightly).  Three small launches, no workspace.
 * gtok_pack_rows: slab -> packed, a buffer of `capacity` elements.  status[0] (zeroed by the caller) gets bit 0 when
 * an id does not fit the packed width - elem_bytes == 2 and an id beyond 16 bits of an int32 slab, or elem_bytes == 1 and an id
 * beyond 8 bits of either slab: the buffer is not to be used, pack again one width up -, bit 1 when capacity <
 * row_ptr[num_rows] (rows that do not fit are skipped, nothing is written out of bounds).
 * gtok_unpack_rows: packed -> [num_rows, ld] slab, pad_id behind every row.  segment_rows > 0: the packed buffer is
 * the concatenation of equally sized segments - what an all-gather of per-rank buffers of segment_stride elements
 * gives - rows [s * segment_rows, (s + 1) * segment_rows) live in segment s: row r starts at
 * s * segment_stride + row_ptr[r] - row_ptr[s * segment_rows], with row_ptr = gtok_row_offsets over the gathered
 * lengths (same align).
 * gtok_collate_packed: gtok_collate reading the packed form (unsegmented) instead of the slab; a row whose row_ptr entry is
 * negative (row_start -1: a row that did not fit its packed buffer) is collated as empty - gtok_collate_batch and
 * gtok_collate_epoch do the same.
 * row_ptr == NULL (gtok_unpack_rows with segment_rows == 0, gtok_collate_packed): the STRIDED form - row r starts at
 * element r * ld of `packed` - i.e. a GTOK_SENT_U16 slab (or any [rows, ld] slab of 16- / 32-bit ids) read in place.
 * gtok_unpack_rows never reads beyond a segment: with segment_rows > 0 a row whose ids would end past segment_stride
 * (a rank whose rows did not fit the caller-given capacity skipped them in gtok_pack_rows, status bit 1) is written as
 * all pad and, when `status` is not NULL, flagged there (bit 1) - gtok_unpack_rows_checked is gtok_unpack_rows with that
 * status word and the total number of elements `packed` holds (0 = unknown) as further bounds.
 * gtok_pack_rows_u16: gtok_pack_rows reading a GTOK_SENT_U16 slab; elem_bytes 1, 2, 4 or 8 (8: int64 ids, the dtype the
 * reference's tensors have - the D2H copy behind TokenizedGraphDataset.__getitem__ needs no widening pass).           */
int gtok_row_offsets(const int32_t *len, int64_t num_rows, int32_t ld, int32_t align, int64_t *row_ptr, void *stream);
int gtok_pack_rows(const int32_t *ids, int32_t ld, const int32_t *len, int64_t num_rows, const int64_t *row_ptr,
                   int32_t elem_bytes, void *packed, int64_t capacity, int32_t *status, void *stream);
int gtok_unpack_rows(const void *packed, int32_t elem_bytes, const int64_t *row_ptr, const int32_t *len,
                     int64_t num_rows, int32_t segment_rows, int64_t segment_stride, int32_t pad_id,
                     int32_t *out_ids, int32_t ld, void *stream);
int gtok_collate_packed(const void *packed, int32_t elem_bytes, const int64_t *row_ptr, const int32_t *len,
                        int32_t ld, const int64_t *index, int32_t batch, int32_t pad_id, int64_t *out_x,
                        uint8_t *out_attn, int32_t out_ld, void *stream);
int gtok_unpack_rows_checked(const void *packed, int32_t elem_bytes, const int64_t *row_ptr, const int32_t *len,
                             int64_t num_rows, int32_t segment_rows, int64_t segment_stride, int64_t packed_elems,
                             int32_t pad_id, int32_t *out_ids, int32_t ld, int32_t *status, void *stream);
int gtok_pack_rows_u16(const uint16_t *ids16, int32_t ld, const int32_t *len, int64_t num_rows, const int64_t *row_ptr,
                       int32_t elem_bytes, void *packed, int64_t capacity, int32_t *status, void *stream);
/* gtok_unpack_rows_checked into a slab of 16-BIT ids (ABI v5; what GTOK_SENT_U16 writes and gtok_collate_packed reads in
 * place): the re-padding pass that ends a compact all-gather of 16-bit rows writes half the bytes.  ids keep their low 16
 * bits; 0 <= pad_id <= 65535.                                                                                             */
int gtok_unpack_rows_u16(const void *packed, int32_t elem_bytes, const int64_t *row_ptr, const int32_t *len,
                         int64_t num_rows, int32_t segment_rows, int64_t segment_stride, int64_t packed_elems,
                         int32_t pad_id, uint16_t *out_ids16, int32_t ld, int32_t *status, void *stream);
/* gtok_unpack_rows_checked / _u16 for rows with EXPLICIT starts (ABI v6; what gtok_sent_packed writes): row r's ids start at
 * element (r / segment_rows) * segment_stride + row_start[r] of `packed` (segment_rows == 0: at row_start[r]); a negative start,
 * or a row that would end beyond its segment / packed_elems (> 0), comes out as all pad and is flagged in status (bit 1).
 * out_bytes: 4 = an int32 slab, 2 = a slab of 16-bit ids.                                                                  */
int gtok_unpack_rows_at(const void *packed, int32_t elem_bytes, const int64_t *row_start, const int32_t *len, int64_t num_rows,
                        int32_t segment_rows, int64_t segment_stride, int64_t packed_elems, int32_t pad_id, void *out_ids,
                        int32_t out_bytes, int32_t ld, int32_t *status, void *stream);
/* gtok_row_offsets + gtok_pack_rows (src_bytes 4: an int32 slab) / gtok_pack_rows_u16 (src_bytes 2: a GTOK_SENT_U16 slab) in
 * ONE pass (ABI v5): row_ptr (int64 [num_rows + 1], OUT) and the packed rows are written by the same kernel - tiles of 256
 * rows, each tile learning its start from the tiles before it (single-pass prefix sum, the tile's closing row_ptr slot is its
 * status word) - for callers that know a capacity before they know the sizes (the compact all-gather with a caller-given
 * bound, a per-epoch D2H staging buffer): the lengths are read once, the ids once, and two launches replace four.  Same
 * results, same status bits - except that status is SET by this call, not accumulated into (bit 1 = rows that did not
 * fit `capacity` were skipped).                                                                                              */
int gtok_pack_rows_scan(const void *ids, int32_t src_bytes, int32_t ld, const int32_t *len, int64_t num_rows, int32_t align,
                        int32_t elem_bytes, void *packed, int64_t capacity, int64_t *row_ptr, int32_t *status, void *stream);

/* gtok_collate_packed for ONE batch whose row list is on the HOST (ABI v5; the stock torch DataLoader hands a dataset its index
 * list as Python ints - trainer/train_agtt.py:599-607): host_index[batch] (rows of the slab / packed form, each in [0, num_rows):
 * checked on the host, GTOK_E_INVAL otherwise) travels in the kernel's arguments - no upload, nothing to synchronise - and the
 * labels are gathered by the same launch: out_y[b] = y[host_index[b]] for elements of y_bytes (4: float32 / int32, 8: int64)
 * bytes each, y == NULL = none.  num_rows must fit 31 bits.  Outputs as gtok_collate_packed.                                  */
int gtok_collate_batch(const void *packed, int32_t elem_bytes, const int64_t *row_ptr, const int32_t *len, int32_t ld,
                       const int64_t *host_index, int32_t batch, int64_t num_rows, int32_t pad_id, int64_t *out_x, uint8_t *out_attn,
                       int32_t out_ld, const void *y, int32_t y_bytes, void *out_y, void *stream);

/* A whole EPOCH's batches collated by one call (ABI v5; trainer/train_agtt.py:599-607 builds the loader, :276-302 is the collate
 * it replaces): the rows order[0 .. n) of the slab / packed rows (as gtok_collate_packed reads them) are cut into batches of
 * batch_size consecutive entries of `order` (the last one may be short).  gtok_collate_epoch_plan writes batch_lmax[b] = the
 * longest row of batch b (min(len, ld) each; int32 [nb], nb = ceil(n / batch_size)) and batch_off[b] = the element at which
 * batch b starts in the arenas, batch_off[nb] = their size (int64 [nb + 1]).  gtok_collate_epoch then fills out_x (int64) and
 * out_attn (bool bytes): batch b is the row-major [B_b, batch_lmax[b]] block at batch_off[b] of both - exactly what
 * gtok_collate_packed gives for index = order[b * batch_size ..] and out_ld = batch_lmax[b].  arena_elems = the elements the
 * arenas hold: an upper bound such as n * ld needs no read-back before the fill (a row that would end beyond it is skipped).
 * A batch then costs its consumer no launch, no allocation and no synchronisation: the host reads batch_lmax / batch_off once
 * per epoch and takes views.                                                                                                  */
int gtok_collate_epoch_plan(const int32_t *len, int32_t ld, const int64_t *order, int64_t n, int32_t batch_size,
                            int32_t *batch_lmax, int64_t *batch_off, void *stream);
int gtok_collate_epoch(const void *packed, int32_t elem_bytes, const int64_t *row_ptr, const int32_t *len, int32_t ld,
                       const int64_t *order, int64_t n, int32_t batch_size, int32_t pad_id, const int32_t *batch_lmax,
                       const int64_t *batch_off, int64_t *out_x, uint8_t *out_attn, int64_t arena_elems, void *stream);

/* Rows of ids -> TEXT: the strings ZINCTokenizationDataset.__getitem__ returns (zinc_dataset_indexbase.py:143-227: the
 * trainer builds its vocab from them, trainer/train_ibtt.py:229-235, :361-372) rendered for a whole split at once.  Row
 * r's text = the strings of its first take[r] ids (string t = tab_bytes[tab_ptr[t] .. tab_ptr[t+1]), t < num_strings; ids
 * outside the table render as empty strings) joined by single spaces, followed VERBATIM by the row's suffix bytes
 * suf_bytes[suf_ptr[r] .. suf_ptr[r+1]) (suf_ptr NULL = none; the label token and <eos>, which differ per molecule, travel
 * here).  Two passes like gtok_parse_graph_text: out_bytes == NULL writes text_len[r]; the caller prefix-sums it into
 * text_ptr[num_rows+1] and calls again with out_bytes (capacity text_ptr[num_rows]).                                       */
int gtok_ids_to_text(const int32_t *ids, int32_t ld, const int32_t *take, int64_t num_rows, const uint8_t *tab_bytes,
                     const int32_t *tab_ptr, int32_t num_strings, const uint8_t *suf_bytes, const int64_t *suf_ptr,
                     const int64_t *text_ptr, uint8_t *out_bytes, int64_t *text_len, void *stream);

/* The per-molecule TAIL of a ZINC text, for gtok_ids_to_text's suffixes: zinc_dataset_indexbase.py:186-195 (`... <p> val_X_XX
 * <eos>`, the label token being f"val_{label:.2f}" with '.' -> '_' and '-' -> 'neg', :192) and :217-221 (a text of more than
 * max_len tokens keeps its first max_len - 1 tokens and `<eos>`).  len[r] = the ids row r holds (gtok_ibtt_zinc's length: up
 * to and including `<p>`), y[r] = the molecule's float32 label.  With cut = len[r] + 2 > max_len: take[r] = cut ? max_len - 1 :
 * len[r]; suffix r = [" " if take[r] > 0] + (cut ? "" : label token + " ") + "<eos>" (at most 56 bytes).  The label is "%.2f" of
 * the float's exact value with ties to even, as Python formats the double that holds it: the sign bit alone decides `neg`
 * (-0.001 -> val_neg0_00), values of any magnitude print in full, nan / inf / -inf -> val_nan / val_inf / val_neginf.
 * Two passes like gtok_ids_to_text: suf_bytes == NULL writes take[r] and suf_len[r]; the caller prefix-sums suf_len into
 * suf_ptr[num_rows+1] and calls again with suf_bytes (capacity suf_ptr[num_rows]).  max_len >= 1.                              */
int gtok_zinc_text_tails(const float *y, const int32_t *len, int64_t num_rows, int32_t max_len, int32_t *take,
                         const int64_t *suf_ptr, uint8_t *suf_bytes, int64_t *suf_len, void *stream);

/* First position of `token` in every row of an int64 [rows, ld] batch (what gtok_collate
 * returns): pos[r] = the smallest i with x[r, i] == token, -1 if there is none.  This is the
 * per-sample `<q>` search of trainer/train_ibtt.py:88-103 and trainer/train_agtt.py:78-114 (the
 * query nodes sit at pos + 2 and pos + 3) as one launch.                                      */
int gtok_find_token(const int64_t *x, int32_t rows, int32_t ld, int64_t token, int32_t *pos,
                    void *stream);

/* Node-id token statistics of the graph-token texts this batch stands for
 * (`<bos> u v <e> ... <n> 0 .. N-1 <q> TASK [qu qv] <p> LABEL <eos>`,
 * graph_token_dataset_autograph.py / docs/synthetic_data.md:46-68) - the corpus
 * pass of build_vocab_from_texts (data_loader.py:451-463) without the texts:
 * for every id i < num_ids,
 *   count[i] += occurrences of the token str(i): edge endpoints (list order),
 *               the <n> list, the two query arguments (query_nodes[g] = (u, v),
 *               NULL or negative entries = none);
 *   first[i]  = min(first[i], (graph_base + g) << 32 | token position in the text
 *               of graph g) over those occurrences.
 * The caller initialises count to 0 and first to INT64_MAX; calls ACCUMULATE, so
 * shards, ranks and epochs can be summed / min-reduced.  num_ids <= 1024.      */
int gtok_vocab_stats_synth(const gtok_csr *g, const int32_t *query_nodes,
                           int64_t graph_base, int32_t num_ids, int64_t *count,
                           int64_t *first, void *stream);

/* The same corpus pass over ARBITRARY texts (any grammar: graph-token tasks, the ZINC strings whose unseen
 * tokens become the dynamic vocab of trainer/train_ibtt.py:361-372): every distinct whitespace-separated token
 * (str.split() rules) gets one slot of an open-addressing table of `capacity` slots (a power of two):
 *   key[s]   64-bit identity of the token (two 32-bit hash streams; 0 = empty slot)
 *   count[s] occurrences            first[s] base_offset + byte offset of the earliest occurrence in `bytes`
 *   len[s]   token length in bytes  -> the token string is bytes[first - base_offset : .. + len]
 * The caller zeroes key / count / len and sets first to INT64_MAX; calls ACCUMULATE (shards: pass the shard's
 * offset in the whole corpus as base_offset so that `first` keeps ordering occurrences corpus-wide).  status
 * (zeroed by the caller) gets bit 0 when the table overflowed: enlarge and repeat; bit 2 (value 4) when two DIFFERENT
 * tokens met in one slot (same 64-bit identity and length, different bytes: every merge compares the occurrence with
 * the slot's first occurrence byte for byte) - the table is then not a token table and must be discarded.  The byte
 * check reaches occurrences inside the blob of the call at hand only: when shards are accumulated by several calls,
 * a collision between tokens of two different shards goes unseen, and reading the strings back needs the whole corpus
 * (a slot's `first` may lie in another shard).  Counter.most_common order =
 * count descending, then `first` ascending.                                                                    */
int gtok_vocab_stats_text(const uint8_t *bytes, const int64_t *text_ptr, int32_t num_texts, int64_t base_offset,
                          int32_t capacity, uint64_t *key, int64_t *count, int64_t *first, int32_t *len,
                          int32_t *status, void *stream);

/* SENT decoder: un-remapped token rows (gtok_sent with remap_zinc = 0) -> graphs in visit-index space: node
 * k is the k-th node the trail visited.  Per row: num_nodes, num_edges, the edges in stream order - edge_a =
 * the node the edge was written from, edge_b = the other end, edge_type = its type token minus the edge offset
 * (-1 unlabelled) - in [rows, edge_cap] arrays, node types in [rows, node_cap], and status: 0 complete (EOS
 * reached), 1 malformed, 2 a capacity exceeded (the row is still read to its end: num_nodes / num_edges are those of
 * the whole row, entries beyond a capacity are dropped - edge_cap = node_cap = 0 is a count-only pass), 3 well-formed but
 * cut before EOS (a row truncated at max_len).  The reverse of the spec in DESIGN.md section 5; with the trail's visit order it gives back
 * the input graph exactly (oracle_sent_roundtrip checks that for every row).                                      */
int gtok_sent_decode(const int32_t *ids, int32_t ld, const int32_t *len, int32_t num_rows,
                     int32_t max_num_nodes, int32_t labeled, int32_t num_node_types,
                     int32_t *num_nodes, int32_t *num_edges, int32_t *edge_a, int32_t *edge_b,
                     int32_t *edge_type, int32_t edge_cap, int32_t *node_type, int32_t node_cap,
                     int32_t *status, void *stream);

/* ---- SENT rows back to a batched CSR (gtok_csr's arrays, what GraphBatch.from_coo builds), in two passes like
 * gtok_parse_graph_text / gtok_ids_to_text ------------------------------------------------------------------------------------
 * Rows: row r = the first min(len[r], ld) ids at element row_start[r] of `ids` (row_start NULL: at r * ld - a [rows, ld] slab
 * read in place), elem_bytes 1, 2 or 4 bytes each: an int32 slab, a GTOK_SENT_U16 slab, or packed rows (gtok_pack_rows_scan's
 * row_ptr, gtok_sent_packed's row_start); a negative row_start = an empty row.  Un-remapped SENT ids only (remap_zinc folds
 * RESET, LADJ and RADJ into one id: gtok_sent_decode_zinc_sizes / gtok_sent_decode_zinc_csr below read those).  4-byte ids are read as int32, as gtok_sent_decode reads them.
 * One row becomes one graph, in visit-index space.  status[r], the node count and the edge list are those of gtok_sent_decode's
 * state machine with unlimited capacities (status 2 cannot occur).  A status-1 row (malformed, len < 1, a negative start) is an
 * EMPTY graph (N = 0, E = 0): rows and graphs stay index-aligned.  A status-3 row (cut before EOS) gives the part of the graph
 * that was read; a node whose type token was cut has type 255.
 * Entries: every decoded edge (a, b, t), in stream order, contributes the entry a -> b and then b -> a (a self loop: one entry);
 * num_entries[r] = 2 x edges - self loops.  The CSR is what GraphBatch.from_coo builds from that list: rows ordered by source
 * with a STABLE sort (a row lists its entries in stream order); eorder (always written) = an entry's position in its graph's
 * interleaved list; nattr / eattr only when labelled: values 0..254 kept, everything else (a missing type included) 255.
 * Duplicates in a stream stay duplicates: the decoder judges grammar, gtok_csr_check judges simplicity.
 * gtok_sent_decode_sizes writes num_nodes / num_entries / status (int32 [num_rows]).  The caller prefix-sums the two counts
 * into node_ptr int32 [num_rows + 1] / edge_ptr int64 [num_rows + 1] and allocates; gtok_sent_decode_csr READS out->node_ptr /
 * out->edge_ptr and writes rowptr, col, eorder, nattr / eattr (labelled) and info int32 [8], which it zeroes first, laid out as
 * gtok_csr_from_coo's where the meanings coincide:
 *   [0] rows whose recount disagrees with their node_ptr / edge_ptr slice (or whose slice does not lie inside [0, node_ptr[rows]]
 *       / [0, edge_ptr[rows]]): such a row is skipped, its arrays stay undefined - nothing is written outside the row's own slice
 *       whatever the two arrays hold;
 *   [1] max_degree, [2] max_nodes, [3] max_edges (of the rows that were built), [4] chunk_nodes, [5] chunk_edges (maxima over
 *       aligned groups of 64 graphs of the slices' sums), [6] the number of status-1 rows, [7] 1 when some graph's interleaved list
 *       was not already row-sorted (eorder is not the identity).
 * One wave per row; the degree counters / row cursors of a row live in LDS, 4 bytes per node of max_num_nodes (and up to 2,048 of
 * its entries, staged between the two halves of pass 2; a longer row is parsed once more instead).  Errors, all
 * before anything is launched or written: GTOK_E_INVAL for null pointers, negative sizes, elem_bytes outside {1, 2, 4}, ld <= 0;
 * GTOK_E_TOO_LARGE for max_num_nodes > GTOK_SENT_LARGE_MAX_NODES; num_rows == 0 is a no-op.  The calls only enqueue on `stream`:
 * no allocation, no host synchronisation, no library-owned counters (they can be captured into a hipGraph).  (Added without an
 * ABI version step, like gtok_sent_large: no struct changes - a binding learns that a library has them from the symbols.)       */
int gtok_sent_decode_sizes(const void *ids, int32_t elem_bytes, const int64_t *row_start, int32_t ld, const int32_t *len,
                           int32_t num_rows, int32_t max_num_nodes, int32_t labeled, int32_t num_node_types,
                           int32_t *num_nodes, int32_t *num_entries, int32_t *status, void *stream);
int gtok_sent_decode_csr(const void *ids, int32_t elem_bytes, const int64_t *row_start, int32_t ld, const int32_t *len,
                         int32_t num_rows, int32_t max_num_nodes, int32_t labeled, int32_t num_node_types,
                         const gtok_csr_built *out, void *stream);

/* ---- ZINC-remapped SENT rows back to raw ids and to a batched CSR ---------------------------------------------------------------
 * gtok_sent with remap_zinc = 1 (every ZINC run of the reference: trainer/train_agtt.py:171-244) folds RESET, LADJ and RADJ into
 * one id.  For LABELLED rows - the only ones the remap is used on - the fold is undone with one id of look-ahead and one bit of
 * state: every trail step and every bracket member starts with an edge-type id, and a RESET is always followed by a position.
 * Parameters (the walk's own): M = max_num_nodes, T = num_node_types, idx_off = 6, node_off = 6 + M, edge_off = node_off + T.
 * Preimage.  The remap (remap_zinc_token; csrc/gtok_zinc_unremap.hpp restates it beside this inverse) is injective on raw ids
 * t >= 0 outside {1, 2, 3, 5}; pre(id) is the one such t whose remap is id, or "none":
 *   0 -> SOS (0), 1 -> EOS (4); 8..16 -> node_off + (id - 8); 17..20 -> edge_off + (id - 17); 22..22+M-1 -> idx_off + (id - 22);
 *   id >= 22 + node_off -> id - 22; a candidate counts only if remapping it gives id back (8 + a with a >= T has none, nor has
 *   22 + t for an atom or bond t that has an id of its own); 3..7, 21, negative ids and everything else: none.  2 is the folded id X.
 * Unfold.  The first min(len, ld) ids of a row, left to right, with a flag open = 0:
 *   at an X with open set: RADJ (3), open cleared; else, when a next id exists inside the row and its preimage is >= edge_off:
 *   LADJ (2), open set; else RESET (1).  Any other id becomes its preimage; an id without one becomes PAD (5), which no state of
 *   the decoder accepts.
 * Decode.  decode_zinc(row) = the labelled decoder of gtok_sent_decode_sizes / gtok_sent_decode_csr over unfold(row): status, node
 * count, edge list, types and the CSR are thereby defined for every input, damaged rows included.  Consequences:
 *   - unfolding a remapped row gives the raw row of the same walk id for id, except that a row which a cut leaves ENDING in X gets
 *     RESET there where the walk may have written LADJ - nothing decodable differs;
 *   - ids behind EOS (a query tail) are unfolded but never parsed, as in the un-remapped decoders;
 *   - UNLABELLED remapped rows are ambiguous (position X position) and have no entry point.
 * gtok_unremap_zinc: rows read exactly as gtok_sent_decode_csr reads them (elem_bytes 1 / 2 / 4, row_start, ld, len; a negative start
 * or len < 1: an empty row); out_ids int32 [num_rows, ld] (must not overlap ids): row r = its unfolded ids, then pad_id to the end of
 * the row.  A wave per row on the vector side: 64 ids per step, the look-ahead from the neighbouring lane (or lane 0 of the next
 * chunk), the flag - a two-state automaton over the X's: one with an edge type behind it toggles it, any other clears it - from two
 * ballots, one bit carried between chunks.
 * gtok_sent_decode_zinc_sizes / gtok_sent_decode_zinc_csr: gtok_sent_decode_sizes / gtok_sent_decode_csr without `labeled` (always
 * 1: out->nattr / out->eattr are needed); outputs, info[8], the slice checks and the errors are theirs.  Every 64-id chunk is
 * unfolded in registers before the state machine reads it.
 * Errors, before anything is launched or written: those of gtok_sent_decode_csr (GTOK_E_TOO_LARGE for max_num_nodes >
 * GTOK_SENT_LARGE_MAX_NODES included), GTOK_E_INVAL for a NULL out_ids; num_rows == 0 is a no-op.  The calls only enqueue on
 * `stream` (capturable).  (Added without an ABI version step: no struct changes.)                                                  */
int gtok_unremap_zinc(const void *ids, int32_t elem_bytes, const int64_t *row_start, int32_t ld, const int32_t *len, int32_t num_rows,
                      int32_t max_num_nodes, int32_t num_node_types, int32_t pad_id, int32_t *out_ids, void *stream);
int gtok_sent_decode_zinc_sizes(const void *ids, int32_t elem_bytes, const int64_t *row_start, int32_t ld, const int32_t *len,
                                int32_t num_rows, int32_t max_num_nodes, int32_t num_node_types,
                                int32_t *num_nodes, int32_t *num_entries, int32_t *status, void *stream);
int gtok_sent_decode_zinc_csr(const void *ids, int32_t elem_bytes, const int64_t *row_start, int32_t ld, const int32_t *len,
                              int32_t num_rows, int32_t max_num_nodes, int32_t num_node_types,
                              const gtok_csr_built *out, void *stream);

/* ---- IBTT rows back to a batched CSR: the same two passes, outputs and row formats as the SENT pair above ---------------------
 * Rows: exactly as gtok_sent_decode_csr reads them (row_start / ld / len / elem_bytes; a negative start or fewer than one id:
 * status 1).  `grammar` says which serialiser wrote them.  The vocab is an input: inv[id], 0 <= id < inv_len, is the LUT slot of
 * that id (GTOK_ZLUT_* / GTOK_SLUT_*; a slot >= *_NODE0 is node index slot - NODE0) or -1; the caller builds it on the host from
 * the LUT it tokenized with, an id that two slots share (pad_id, when a token is absent from the vocab) gets -1.  An id outside
 * [0, inv_len) or with inv[id] < 0 has class -1 and matches nothing.  c[i] below = the class of token i, L = the row's ids.
 * IBTT lists node indices in the input's own numbering and edges in the input's own order: a decoded row is the input graph.
 * status[r]: 0 complete, 1 malformed (an EMPTY graph, N = 0, E = 0: rows and graphs stay index-aligned), 3 a well-formed prefix
 * (the part that was read is built); 2 does not occur.
 * GTOK_IBTT_GRAMMAR_ZINC  "<bos> (<atom> sym)* (<bond> type u v)* <q> regression <p>":
 *   a last token of class EOS is dropped and remembered (L' = L - 1: the max_len cut writes <eos> over the last kept token); L' == 0
 *   then: status 3, empty.  c[0] must be BOS.  A = the longest run of atom records (c[1+2k] == ATOM, c[2+2k] in [ATOM0, ATOM0+9],
 *   both inside L'); N = A, node type slot - ATOM0, 255 for 'X'.  B = the longest run of bond records from p = 1 + 2A (c[p+4k] ==
 *   BOND, c[p+4k+1] in [BOND0, BOND0+4], the next two node slots of index < N, all four inside L'); type slot - BOND0.  The rest
 *   c[p+4B .. L'): [Q, REGRESSION, P] is status 0 (status 1 when an EOS was dropped); a proper prefix of that, a proper prefix of a
 *   bond record valid so far, or - when B == 0 - a lone ATOM is status 3; anything else status 1.  N > max_num_nodes: status 1.
 *   Entries: bond k = (u, v, t) contributes u -> v and then v -> u (a self loop: one entry): num_entries = 2B - self loops.
 * GTOK_IBTT_GRAMMAR_SYNTH "<bos> (u v <e>)* <n> 0 1 .. N-1 <q> [q0 [q1 [q2]]] <p>":
 *   c[0] must be BOS.  M = the longest run of edge records (c[1+3k], c[2+3k] node slots, c[3+3k] == E, inside L); p = 1 + 3M.
 *   p == L: status 3.  c[p] != N: status 3 when c[p..L) is one or two node slots, else 1.  Otherwise S = the longest run with
 *   c[p+1+k] == NODE0 + k, q = p + 1 + S; q == L: status 3; c[q] != Q: status 1; c[L-1] == P with nq = L - q - 2 in 0..3: status
 *   0; else L - q - 1 <= 3: status 3 (cut inside the query); else status 1.  Once Q was seen N = S and an endpoint >= S is
 *   status 1; before it N = max(S, 1 + the largest endpoint of the M records).  N > max_num_nodes: status 1.
 *   Entries: one entry u -> v per edge record, in list order (what gtok_csr keeps of a graph-token edge list).
 *   query (int32 [num_rows, 4], NULL = skip; sizes pass): gtok_ibtt_synth's input read back from a status-0 row - query[4r] = nq,
 *   query[4r+1 ..] = the raw ids after <q>, unused slots 0; all 0 for any other row.
 * The CSR, info[8], the skipping of a row whose recount disagrees with its slice and the errors are gtok_sent_decode_csr's; ZINC
 * writes (and needs) nattr / eattr, SYNTH neither.  Also GTOK_E_INVAL: a grammar outside {0, 1}, inv NULL, inv_len <= 0.  One wave
 * per row, a lane per record; the degree counters / row cursors live in LDS, 4 bytes per node of max_num_nodes (hence
 * max_num_nodes <= GTOK_SENT_LARGE_MAX_NODES); nothing is staged, pass 2 reads a row's tokens three times.  Nothing is read through
 * an index that has not been range-checked; row_start and len are trusted, as by every packed-row reader.  The calls only enqueue
 * on `stream`: no allocation, no host synchronisation, no library-owned counters.  (Added without an ABI version step.)            */
#define GTOK_IBTT_GRAMMAR_ZINC  0   /* gtok_ibtt_zinc's rows  */
#define GTOK_IBTT_GRAMMAR_SYNTH 1   /* gtok_ibtt_synth's rows */
int gtok_ibtt_decode_sizes(const void *ids, int32_t elem_bytes, const int64_t *row_start, int32_t ld, const int32_t *len,
                           int32_t num_rows, int32_t grammar, const int32_t *inv, int32_t inv_len, int32_t max_num_nodes,
                           int32_t *num_nodes, int32_t *num_entries, int32_t *status, int32_t *query, void *stream);
int gtok_ibtt_decode_csr(const void *ids, int32_t elem_bytes, const int64_t *row_start, int32_t ld, const int32_t *len,
                         int32_t num_rows, int32_t grammar, const int32_t *inv, int32_t inv_len, int32_t max_num_nodes,
                         const gtok_csr_built *out, void *stream);

/* ---- gtok_csr_relabel: a batched CSR renumbered through a per-graph node map, in a canonical entry order ---------------------
 * g: the graphs to renumber ("old" ids), dataset order.  target_node_ptr int32 [G + 1]: node_ptr of the TARGET numbering (NULL =
 * g->node_ptr); target_max_nodes: a host-known bound on the target node counts.  old_of_new int32 [target_node_ptr[G]]: the old id
 * of target node t of graph g at target_node_ptr[g] + t; a value outside [0, N_old) = absent.  It is exactly a visit_index slice
 * (gtok_sent_large_order) when g is a decoded batch and the target is the batch that was tokenized.
 * Per graph (N_old = g's node count, N_t = the target's, E_g unchanged): the map must name every old node exactly once (N_old <=
 * N_t; the entries of old_of_new inside [0, N_old) are a bijection onto it).  Target nodes with an absent entry become isolated
 * nodes of type 255.  Row t of the output lists old row old_of_new[t]'s entries with their columns renumbered, in ascending new
 * column; entries of equal column (duplicates) keep their input order (a stable sort); a self loop stays a self loop.  Two graphs
 * are equal iff their relabelled arrays are, provided neither lists an edge twice.
 * out: rowptr int32 [target total + G] (gtok_csr's layout over the target's node_ptr), col int32 [E] the renumbered columns, eorder
 * int32 [E] always written: the entry's local index in the old graph's entry list (a gather map for whatever else the caller keeps
 * per entry), nattr uint8 [target total] / eattr uint8 [E] only when g has them (they follow their node / entry); out->node_ptr /
 * out->edge_ptr are not touched (they would equal target_node_ptr / g->edge_ptr).
 * status int32 [G]: 0 built; 2 built, but some row holds a duplicate or a self loop (the graph is not simple); 1 skipped: the map
 * is not such a bijection, N_old > N_t, N_t > target_max_nodes (or N_old > g->max_nodes, E_g > g->max_edges: the other host-known
 * bounds), a slice outside the totals of its pointer array, a column outside [0, N_old), row pointers that decrease or do not run
 * from 0 to E_g.  A skipped graph's arrays are undefined; nothing is ever written outside the graph's own slices, whatever the
 * inputs hold, and nothing is read through an index that was not range-checked first - given that the arrays are as long as their
 * pointer arrays say.
 * out->info int32 [8], zeroed by the call: [0] skipped graphs, [1] max_degree, [2] max_nodes (target counts), [3] max_edges of the
 * built graphs, [4] chunk_nodes, [5] chunk_edges (gtok_csr_from_coo's meaning: maxima over aligned groups of 64 graphs of the
 * built graphs' summed counts), [6] status-2 graphs, [7] 0.
 * One wave per graph; the old -> new table lives in LDS, 16 bits per node (36 KB per wave at 16,384 nodes with the set the
 * bijection is checked on).  Rows of up to 64 entries are ranked in registers; longer ones through an N-bit set with popcount
 * ranks (rows with duplicates: a stable count, d steps per 64 entries): a simple graph costs O(N + E) lane steps plus N / 2,048
 * wave steps per row of more than 64 entries.
 * workspace: gtok_csr_relabel_workspace(G, E) bytes of device memory (pure host arithmetic; a multiple of 16, 0 for an empty batch;
 * GTOK_E_INVAL for a negative argument), 16-byte aligned, free again when the stream has run the call.
 * Errors, all before any device is asked for: GTOK_E_INVAL for null pointers, negative sizes, a reordered batch (graph_ids /
 * unit_ptr set), g with attributes and out without, a misaligned or short workspace; GTOK_E_TOO_LARGE for target_max_nodes or
 * g->max_nodes beyond GTOK_SENT_LARGE_MAX_NODES; num_graphs == 0 is a no-op.  The call only enqueues on `stream` (two memsets, two
 * launches): no allocation, no host synchronisation, no library-owned counters - it can be captured into a hipGraph.  (Added
 * without an ABI version step, like the decoders: no struct changes.)                                                         */
int64_t gtok_csr_relabel_workspace(int32_t num_graphs, int64_t num_entries);
int gtok_csr_relabel(const gtok_csr *g, const int32_t *target_node_ptr, int32_t target_max_nodes, const int32_t *old_of_new,
                     const gtok_csr_built *out, int32_t *status, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- the task answers of a batch: cycle check and shortest-path distances ----------------------------------------------------
 * The graph-token corpora are built for two tasks (graph_data_loader/data_loader.py:57-110: `has_cycle ... <p> yes|no` and
 * `shortest_distance u v ... <p> lenK|INF`; :90-91 also accepts `connected` / `reachable` answer words;
 * configs/agtt_graph_token.yaml and configs/ibtt_graph_token.yaml train on exactly these).  gtok_graph_tasks answers both for every
 * graph of a batched CSR - a parsed corpus, a device-built one, a decoded batch - without leaving the device.
 * Definitions.  The graph of a CSR slice is the SIMPLE UNDIRECTED CLOSURE of its listed entries: nodes 0..N-1, {u,v} an edge iff
 * (u,v) or (v,u) is listed, u != v; duplicates collapse; self loops are counted apart (`loops`).  One-direction lists, both-direction
 * lists, duplicates and loops are all legal input (on the paths up to 512 nodes).
 *   num_components[g]  connected components of the closure, isolated nodes included; 0 for N = 0
 *   has_cycle[g]       1 iff loops > 0 || m > N - num_components, m = distinct undirected non-loop edges (the graph is no forest:
 *                      what test/data_distribution_test.py:136-140 asks networkx), else 0
 *   dist[q]            for the query (u, v) of graph g: the hop count of a shortest path in the closure; 0 when u == v; -1 when
 *                      unreachable; -2 when an endpoint is outside [0, N_g) - that also raises bit 0 of info[0], and nothing is read
 *                      through such an endpoint
 * The reference's label conventions are host arithmetic on top (lenK <-> label K - 1, INF = the item is dropped).
 * query_nodes int32 [Q, 2] local ids, or NULL (no distances: then query_ptr must be NULL and num_queries 0).  query_ptr int64 [G + 1]:
 * the queries of graph g are query_ptr[g] .. query_ptr[g + 1]; NULL = exactly one per graph (Q == G), the form gtok_sent's `query`
 * has.  Consecutive queries of one graph with the same source share one search.  has_cycle / num_components int32 [G] or NULL each;
 * dist int32 [Q], required iff query_nodes is given.  A call that asks for nothing is a no-op.
 * info int32 [4], zeroed by the CALLER (several calls may accumulate into one): [0] status bits - 1: a query endpoint outside its
 * graph, 2: damaged arrays (a slice outside the totals of its pointer array or beyond max_nodes / max_edges: the graph counts as
 * empty; a row pointer outside [0, E_g] or decreasing: the row counts as empty; a column outside [0, N_g): the entry is skipped;
 * query_ptr outside [0, Q] or decreasing: the graph's queries are not answered) - nothing is read or written through an index that
 * was not range-checked, given that the arrays are as long as their pointer arrays say; [1] the largest dist; [2] queries answered
 * -1; [3] graphs with a cycle (counted when has_cycle or num_components is asked for).
 * One wave per graph; the search is chosen for the whole batch by g->max_nodes:
 *   <= 64 nodes    lane v holds closure row v in a 64-bit register (built through 512 bytes of LDS); the closure is symmetric, so
 *                  the search PULLS: next = ballot((row & frontier) != 0) & ~visited - one ballot per level, no atomics, no queue
 *   <= 512 nodes   the same over an immutable bit matrix in LDS, W = 2, 4 or 8 words per node (at most 32 KB per wave), lane l
 *                  owning nodes l + 64 j; frontier and visited are W scalar words, W ballots per level
 *   <= GTOK_SENT_LARGE_MAX_NODES   GTOK_CSR_SIMPLE_SYMMETRIC batches only (m = E / 2, loops = 0 follow from the flag): a push search
 *                  over the CSR with a visited bit set, a 16-bit distance table and a 16-bit FIFO in LDS (66 KB per wave at 16,384
 *                  nodes: one wave per workgroup); 64 nodes are popped per step, never across a level boundary; rows of more than
 *                  64 entries are read by the whole wave
 * GTOK_TASKS_KERNEL=reg|lds|csr forces a search (tests); one that cannot hold the batch is GTOK_E_UNSUPPORTED.
 * Errors, all before any device is asked for: GTOK_E_INVAL for null pointers / negative sizes / a reordered batch / query_nodes
 * and dist not both given or both NULL / query_ptr == NULL with num_queries != G / queries with no graphs; GTOK_E_TOO_LARGE for
 * max_nodes beyond GTOK_SENT_LARGE_MAX_NODES; GTOK_E_UNSUPPORTED for more than 512 nodes without GTOK_CSR_SIMPLE_SYMMETRIC.  The
 * call only enqueues one launch on `stream` (whose device is used): no allocation, no host read-back, no library-owned counters -
 * it can be captured into a hipGraph.  (Added without an ABI version step, like the decoders: no struct changes.)              */
int gtok_graph_tasks(const gtok_csr *g, const int32_t *query_nodes, const int64_t *query_ptr, int64_t num_queries, int32_t *has_cycle,
                     int32_t *num_components, int32_t *dist, int32_t *info, void *stream);

/* ---- a key per graph: duplicate graphs and split leakage ------------------------------------------------------------------------
 * The reference checks a corpus for leaked test graphs (test/train_performance_test.py:70-74 compute_graph_hash, :146-207
 * test_data_leakage): every graph gets the key (num_nodes, the sorted list of its listed edges with each edge's endpoints sorted,
 * label), and the splits' key sets are intersected.  gtok_graph_keys gives every graph of a batched CSR a 128-bit digest of exactly
 * that key in one pass over the CSR, keys[2 g], keys[2 g + 1]; grouping equal keys (and confirming them exactly) is torch plumbing
 * on top (ops.duplicate_graphs, ops.split_leakage).  The digest is a keyed multiset sum - it does not depend on the order of the
 * entries or on their orientation; its arithmetic is csrc/gtok_graph_keys_hash.hpp, frozen in DESIGN.md.
 * A key identifies a NUMBERED graph, as the reference's tuple does: isomorphic graphs numbered differently get different keys.  It
 * is no isomorphism class and no canonical form.  Equal keys of different graphs are possible in principle (128 bits).
 * flags = a mode, optionally | GTOK_KEYS_ATTRS:
 *   GTOK_KEYS_LISTED   the reference's key.  The terms are ALL listed entries, folded to a <= b: duplicates count, self loops count -
 *                      a graph listed once and the same graph listed in both directions get different keys, as there.  With
 *                      GTOK_KEYS_ATTRS every entry carries its eattr byte and every node adds a term with its nattr byte (ZINC;
 *                      needs g->nattr and g->eattr).
 *   GTOK_KEYS_CLOSURE  the key of the graph as gtok_graph_tasks defines it: the simple undirected closure of the entries - every
 *                      distinct edge {u, v}, u != v, counts once and every node with a self loop counts once.  By definition it
 *                      equals the LISTED key of that graph listed once and simple (each edge once in either orientation, each looped
 *                      node's loop once): a once-listed, a both-directions and a messy listing of one graph share it.  Structure
 *                      only: with GTOK_KEYS_ATTRS it is GTOK_E_INVAL.
 * labels int32 [G] or NULL (label 0 for every graph).  keys uint64 [G, 2].  info int32 [4], zeroed by the CALLER: [0] status bits -
 * 2: damaged arrays (a slice outside the totals of its pointer array or beyond max_nodes / max_edges: the graph counts as empty; a
 * row pointer outside [0, E_g] or decreasing: the row is skipped; a column outside [0, N_g): the entry is skipped) - nothing is read
 * through an index that was not range-checked; [1] the graphs with such damage; [2], [3] are not written.  Nothing is written outside
 * keys[2 g .. 2 g + 1] and info.
 * One wave per graph (independent waves, gtok_graph_tasks' conventions):
 *   LISTED   any batch up to GTOK_SENT_LARGE_MAX_NODES nodes: a stream over rowptr / col (/ eattr / nattr) with coalesced reads - the
 *            bounds of 64 rows, then their entries 64 consecutive ones per step, each lane finding its entry's row among the 64 row
 *            starts; a row of more than 64 entries is thereby read by the whole wave
 *   CLOSURE  chosen for the whole batch by g->max_nodes: <= 64 nodes closure rows in registers; <= 512 nodes the bit matrix in LDS,
 *            each lane enumerating the set bits b > v of the rows it owns (the diagonal kept apart for loops); beyond 512 nodes
 *            GTOK_CSR_SIMPLE_SYMMETRIC batches only - the listed stream keeping the entries with u < v - GTOK_E_UNSUPPORTED without the
 *            flag.  GTOK_KEYS_KERNEL=reg|lds|csr forces one (tests); one that cannot hold the batch is GTOK_E_UNSUPPORTED.
 * Errors, all before any device is asked for: GTOK_E_INVAL for null pointers / negative sizes / a reordered batch / unknown flag bits /
 * GTOK_KEYS_ATTRS with GTOK_KEYS_CLOSURE or without the attribute arrays; GTOK_E_TOO_LARGE for max_nodes beyond
 * GTOK_SENT_LARGE_MAX_NODES; num_graphs == 0 is a no-op.  The call only enqueues one launch on `stream` (whose device is used): no
 * allocation, no host read-back, no library-owned counters - it can be captured into a hipGraph.  (Added without an ABI version step:
 * no struct changes.)                                                                                                          */
#define GTOK_KEYS_LISTED 0
#define GTOK_KEYS_CLOSURE 1
#define GTOK_KEYS_ATTRS 2
int gtok_graph_keys(const gtok_csr *g, const int32_t *labels, int32_t flags, uint64_t *keys, int32_t *info, void *stream);

/* ---- a key per graph that does not depend on the numbering: Weisfeiler-Lehman colour refinement ---------------------------------
 * gtok_graph_keys identifies a NUMBERED graph, and every graph the SENT decoders return is numbered in visit-index space: the same
 * molecule tokenized in two epochs decodes to two numberings and two keys, and a generated sequence has no input numbering to go
 * back to.  gtok_graph_wl gives every graph of a batched CSR a 128-bit key that is an INVARIANT: isomorphic graphs always share it,
 * however they are numbered, listed or oriented.  It is no isomorphism class and no canonical form either - graphs that are not
 * isomorphic share it when `rounds` rounds of colour refinement cannot tell them apart (regular graphs of equal degree: a 6-cycle
 * and two triangles), or by a collision of 64-bit words.  Grouping, confirming and the uniqueness / novelty counts of a sampled batch
 * are torch plumbing on top (ops.isomorphic_duplicates, ops.unique_novel).  The arithmetic is csrc/gtok_graph_wl_hash.hpp, frozen in
 * DESIGN.md section 5c.
 * The graph of a CSR slice is the simple undirected closure gtok_graph_tasks defines (distinct neighbours, a loop flag per node).
 * Every node starts with a colour made of its degree and loop flag; a round gives it the mix of its colour and the keyed sum of its
 * neighbours' colours; the key digests the multiset of final colours, N, the rounds run and the label.  rounds in [0,
 * GTOK_WL_MAX_ROUNDS]: 0 = N_g rounds for every graph (the colouring is stable by then; <= 512 nodes only).  A path of N nodes needs
 * about N / 2 rounds to tell its nodes apart; 3 separates what molecules and the graph-token corpora hold.
 * flags = 0 or GTOK_WL_ATTRS: the node attribute bytes enter the first colours and the byte of the entry (v, u), as row v lists it,
 * enters what u adds to v (needs g->nattr, g->eattr and a GTOK_CSR_SIMPLE_SYMMETRIC batch; the flag is trusted: each direction's own
 * byte is read).
 * labels int32 [G] or NULL (label 0).  keys uint64 [G, 2].  node_colors uint64 [node_ptr[G]] or NULL: the final colour of node v of
 * graph g at node_ptr[g] + v - equal colours in two graphs of equal key pair up nodes no round could tell apart; a graph with N
 * distinct colours is numbered canonically by their ranks.  info int32 [4], zeroed by the CALLER, as gtok_graph_keys': [0] bit value
 * 2 = damaged arrays (a bad slice: the graph counts as empty and gets no colours; a bad row is skipped; a bad column is skipped),
 * [1] the graphs with such damage.  Nothing is read through an unchecked index; nothing is written outside keys[2 g .. 2 g + 1], the
 * graph's own node_colors slice, info and the workspace.
 * One wave per graph (independent waves), the kernel chosen for the whole batch:
 *   reg   max_nodes <= 64, structure only, any listing: closure rows in a 64-bit register per lane, a 64-entry term table in LDS
 *   lds   <= 512, structure only, any listing: the bit matrix in LDS plus a term table of 8 bytes per node (36 KB per wave at most)
 *   csr   GTOK_CSR_SIMPLE_SYMMETRIC batches of any size up to GTOK_SENT_LARGE_MAX_NODES, and every GTOK_WL_ATTRS call: a pull over
 *         the CSR rows, lane l owning nodes l + 64 j, two 8-byte tables per node - in LDS up to 4,096 nodes (64 KB, one wave per
 *         workgroup there), beyond that in `workspace`: 16 bytes per node of max_nodes for each of min(G, GTOK_WL_LARGE_WAVES) waves,
 *         wave w taking graphs w, w + waves, ...
 * A hub's row is one lane's loop on all three.  GTOK_WL_KERNEL=reg|lds|csr forces one (tests); one that cannot hold the batch is
 * GTOK_E_UNSUPPORTED.  gtok_graph_wl_workspace: pure host arithmetic, the bytes `workspace` must have (16-byte aligned; 0, and
 * workspace may be NULL, up to 4,096 nodes); GTOK_E_INVAL for a negative argument, GTOK_E_TOO_LARGE beyond GTOK_SENT_LARGE_MAX_NODES.
 * Errors, all before any device is asked for: GTOK_E_INVAL for null pointers / negative sizes / a reordered batch / unknown flag bits /
 * rounds outside [0, GTOK_WL_MAX_ROUNDS] / GTOK_WL_ATTRS without both attribute arrays / a short or misaligned workspace;
 * GTOK_E_TOO_LARGE for max_nodes beyond GTOK_SENT_LARGE_MAX_NODES; GTOK_E_UNSUPPORTED for an unflagged batch beyond 512 nodes,
 * GTOK_WL_ATTRS on an unflagged batch, rounds == 0 beyond 512 nodes, a forced kernel that cannot hold the batch; num_graphs == 0 is a
 * no-op.  The call only enqueues one launch on `stream` (whose device is used): no allocation, no host read-back, no library-owned
 * counters - it can be captured into a hipGraph.  (Added without an ABI version step: no struct changes.)                        */
#define GTOK_WL_ATTRS 2            /* flags: node and edge attribute bytes enter the colours */
#define GTOK_WL_MAX_ROUNDS 512
#define GTOK_WL_LARGE_WAVES 1024
int64_t gtok_graph_wl_workspace(int32_t max_nodes, int32_t num_graphs);
int gtok_graph_wl(const gtok_csr *g, const int32_t *labels, int32_t rounds, int32_t flags, uint64_t *keys, uint64_t *node_colors,
                  int32_t *info, void *workspace, int64_t workspace_bytes, void *stream);

/* Which SENT kernel gtok_sent() will run for this batch ("sent_lane_kernel": lane per graph over the CSR, needs
 * GTOK_CSR_SIMPLE_SYMMETRIC, <= 64 nodes and a large batch; "sent_blane_kernel<W=..>": lane per graph over the
 * adjacency bit-matrix mirror, unlabelled, <= 256 nodes; "sent_reg_kernel": wave per graph, <= 64 nodes;
 * "sent_lds_kernel<W=..>": wave per graph, up to 512 nodes).  All emit the same tokens.                      */
const char *gtok_sent_kernel_name(const gtok_csr *g, const gtok_sent_params *p);
/* Same for gtok_ibtt_zinc(): "ibtt_zinc_quad_kernel" (8 or 16 lanes per molecule: GTOK_CSR_SIMPLE_SYMMETRIC
 * batches in list order - the default for ZINC), "ibtt_zinc_lane_kernel" (lane per graph, GTOK_IBTT_KERNEL=lane
 * only) or "ibtt_zinc_kernel" (wave per graph: any batch).  All emit the same tokens.                          */
const char *gtok_ibtt_zinc_kernel_name(const gtok_csr *g);

/* ABI version (GTOK_ABI_VERSION of the header the library was built from: 2 since gtok_csr carries the optional
 * mirrors - a binding checks it before passing structs; 3 adds the packed-row entry points; 4: gtok_sent_params carries
 * epoch_count, GTOK_SENT_U16, the strided / checked packed-row readers; 5 adds gtok_csr_check / gtok_csr_lane_sort -
 * structs unchanged; 6 adds gtok_sent_packed / GTOK_SENT_PACK_ONLY / gtok_unpack_rows_at / GTOK_E_UNSUPPORTED - structs
 * unchanged; 7 adds gtok_csr_from_coo - structs unchanged; 8 adds elem_bytes == 1 to the packed-row entry points and
 * GTOK_SENT_PACK_U8 - structs unchanged) and build target string ("gfx950").                                        */
#define GTOK_ABI_VERSION 8
int gtok_version(void);
const char *gtok_target(void);

#ifdef __cplusplus
}
#endif
#endif /* GTOK_H */
