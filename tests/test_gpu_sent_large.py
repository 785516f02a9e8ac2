"""gtok_sent_large (include/gtok.h): the SENT trail walk for graphs of more than 512 nodes.  The reference of every comparison is
the C oracle (oracle_sent), bit for bit; where gtok_sent runs the same batch its rows are compared too."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from _util import PygDataLike, PygInMemoryLike, both, edge_case_graphs, gtok, orc, unpad

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THREADS = 16
_lib = gtok._lib
MAXN, WAVES = _lib.SENT_LARGE_MAX_NODES, _lib.SENT_LARGE_WAVES
LAB = dict(labeled=True, num_node_types=28, num_edge_types=6)
RESET, LADJ, RADJ = 1, 2, 3


def _kw(labeled):
    return dict(LAB) if labeled else dict(labeled=False)


def _cmp(ids, ln, ref_ids, ref_ln, what):
    ids, ln = ids.cpu().numpy(), ln.cpu().numpy()
    assert np.array_equal(ln, ref_ln), f"{what}: lengths differ at {np.nonzero(ln != ref_ln)[0][:5]}: {ln[ln != ref_ln][:5]} vs {ref_ln[ln != ref_ln][:5]}"
    bad = np.nonzero((ids != ref_ids).any(1))[0]
    if bad.size:
        r = bad[0]
        c = int(np.nonzero(ids[r] != ref_ids[r])[0][0])
        lo = max(0, c - 12)
        raise AssertionError(f"{what}: {bad.size} rows differ, first row {r} col {c}: {ids[r, lo:c + 8].tolist()} vs {ref_ids[r, lo:c + 8].tolist()}")


# ------------------------------------------------------------------------------------------------ generators
def _ring_pairs(n, chords, rng):
    """the undirected edges (a < b) of a ring on n nodes + `chords` random chords"""
    pairs = {(min(i, (i + 1) % n), max(i, (i + 1) % n)) for i in range(n)} if n > 2 else set()
    while len(pairs) < min((n if n > 2 else 0) + chords, n * (n - 1) // 2) and n > 3:
        a, b = sorted(rng.integers(0, n, 2).tolist())
        if a != b:
            pairs.add((a, b))
    return np.array(sorted(pairs), np.int64).reshape(-1, 2)


def _graphs(edge_lists, sizes, rng, listing, dup=False):
    """A batch dict of graphs given as undirected pair arrays, listed as `listing` says:
    both: both directions, row-sorted;  shuffled: both directions in random order;  oneway: a < b only, as given.
    Types: x random in [0, 28); the two directions of an edge carry DIFFERENT types ((a + b) % 3 forward, 3 + (a + b) % 2 backward);
    dup: a duplicate of every tenth entry is appended with a third type (5)."""
    srcs, dsts, eas, ecs = [], [], [], []
    for e in edge_lists:
        a, b = e[:, 0], e[:, 1]
        if listing == "oneway":
            s, t, ty = a, b, (a + b) % 3
        else:
            s, t = np.concatenate([a, b]), np.concatenate([b, a])
            ty = np.concatenate([(a + b) % 3, 3 + (a + b) % 2])
            o = rng.permutation(s.size) if listing == "shuffled" else np.lexsort((t, s))
            s, t, ty = s[o], t[o], ty[o]
        if dup:
            s, t, ty = np.concatenate([s, s[::10]]), np.concatenate([t, t[::10]]), np.concatenate([ty, np.full(s[::10].size, 5)])
        srcs.append(s); dsts.append(t); eas.append(ty); ecs.append(s.size)
    cat = lambda l: np.concatenate(l).astype(np.int64) if l else np.zeros(0, np.int64)
    return dict(node_counts=np.asarray(sizes, np.int64), edge_counts=np.asarray(ecs, np.int64), src=cat(srcs), dst=cat(dsts),
                x=rng.integers(0, 28, int(np.sum(sizes))).astype(np.int64), edge_attr=cat(eas))


def _concat(*ds):
    keys = ("node_counts", "edge_counts", "src", "dst", "x", "edge_attr")
    return {k: np.concatenate([np.asarray(d[k], np.int64) for d in ds]) for k in keys}


BORDER_SIZES = (513, 514, 575, 576, 577, 640, 1024, 1025, 2050)
LISTINGS = ("flagged", "cleared", "shuffled", "oneway")


@functools.lru_cache(maxsize=None)
def _border(listing, labeled):
    """Item 3's batch in one listing: (host batch, oracle Coo).  `flagged` = both directions, row-sorted, GTOK_CSR_SIMPLE_SYMMETRIC
    set; `cleared` = the same lists with the flag cleared (the in-list path).  The labelled runs carry a duplicate of every tenth
    entry - except the flagged listing, which claims that no entry is listed twice."""
    rng = np.random.default_rng(31)
    el = [_ring_pairs(n, 300, rng) for n in BORDER_SIZES]
    d = _graphs(el, BORDER_SIZES, np.random.default_rng(32), "both" if listing in ("flagged", "cleared") else listing,
                dup=labeled and listing != "flagged")
    x, ea = (d["x"], d["edge_attr"]) if labeled else (None, None)
    batch = gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], x, ea, check_symmetric=listing == "flagged")
    assert bool(batch.flags & 1) == (listing == "flagged")
    return batch, orc.Coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], x, ea)


@functools.lru_cache(maxsize=None)
def _border_ref(listing, labeled, max_len):
    batch, coo = _border(listing, labeled)
    ld = gtok.ops.sent_safe_ld(batch, labeled, max_len)
    return orc.sent(coo, 2050, max_len, 7, 1, ld=ld, nthreads=THREADS, **_kw(labeled))


def _lossless(coo, ids, ln, max_num_nodes, max_len, seed, epoch, labeled):
    """item 7: every untruncated row decodes back to its input graph, and the device decoder equals the oracle's"""
    ids_h, ln_h = ids.cpu().numpy(), ln.cpu().numpy()
    nt = 28 if labeled else 0
    st = orc.sent_roundtrip(coo, ids_h, ln_h, max_num_nodes, max_len, seed, epoch, labeled=labeled, num_node_types=nt, nthreads=THREADS)
    whole = ln_h < max_len
    assert whole.any() and (st[whole] == 0).all(), st
    cap = int(ids.shape[1])
    got = gtok.ops.sent_decode(ids, ln, max_num_nodes, labeled, nt, edge_cap=cap, node_cap=max_num_nodes)
    want = orc.sent_decode_rows(ids_h, ln_h, max_num_nodes, labeled, nt, edge_cap=cap, node_cap=max_num_nodes)
    for k in ("num_nodes", "num_edges", "status"):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    for g in range(ids_h.shape[0]):
        m, nn = int(want["num_edges"][g]), int(want["num_nodes"][g])
        for k in ("edge_a", "edge_b", "edge_type"):
            assert np.array_equal(got[k][g, :m].cpu().numpy(), want[k][g, :m]), (k, g)
        assert np.array_equal(got["node_type"][g, :nn].cpu().numpy(), want["node_type"][g, :nn]), g


# ------------------------------------------------------------------------------------------------ 1. hand-made graphs
@pytest.mark.parametrize("labeled", [True, False])
def test_hand_made_graphs(labeled):
    """empty graph, single node, isolated nodes, self loops, duplicates, reversed-first entries with different types, two components"""
    batch, coo = both(edge_case_graphs(), labeled)
    dev = batch.to(DEV)
    for flags in (batch.flags, 0):
        dev.flags = flags
        for max_len in (4096, 100, 5, 1):
            ids, ln = gtok.ops.sent_large(dev, 8, max_len, 3, 2, **_kw(labeled))
            ref, rln = orc.sent(coo, 8, max_len, 3, 2, ld=ids.shape[1], **_kw(labeled))
            _cmp(ids, ln, ref, rln, f"hand-made labeled={labeled} max_len={max_len}")
    assert gtok.ops.last_sent_kernel() == "sent_large_kernel"


# ------------------------------------------------------------------------------------------------ 2. where gtok_sent runs too
def test_same_tokens_as_gtok_sent_on_molecules_and_graph_token_graphs():
    d = gtok.synth.zinc_like(300, seed=21)
    batch, coo = both(d)
    dev = batch.to(DEV)
    kw = dict(labeled=True, num_node_types=28, num_edge_types=4, remap_zinc=True)
    ids, ln = gtok.ops.sent_large(dev, 37, 1024, 5, 3, **kw)
    ref, rln = orc.sent(coo, 37, 1024, 5, 3, ld=ids.shape[1], nthreads=THREADS, **kw)
    _cmp(ids, ln, ref, rln, "zinc_like, remapped")
    ids2, ln2 = gtok.ops.sent(dev, 37, 1024, 5, 3, **kw)
    assert torch.equal(ids, ids2) and torch.equal(ln, ln2)

    d = gtok.synth.graph_token_like(200, seed=22, task="shortest_path", with_text=False)
    batch, coo = both(d, False)
    dev = batch.to(DEV)
    q = np.asarray(d["queries"], np.int32)
    kw = dict(graph_base=1000, query=torch.from_numpy(q))
    ids, ln = gtok.ops.sent_large(dev, 49, 600, 6, 1, **kw)
    ref, rln = orc.sent(coo, 49, 600, 6, 1, ld=ids.shape[1], graph_base=1000, query=q, nthreads=THREADS)
    _cmp(ids, ln, ref, rln, "graph_token_like with query")
    ids2, ln2 = gtok.ops.sent(dev, 49, 600, 6, 1, **kw)
    assert torch.equal(ids, ids2) and torch.equal(ln, ln2)


# ------------------------------------------------------------------------------------------------ 3. set-word borders, the 512 limit
@pytest.mark.parametrize("labeled", [True, False])
@pytest.mark.parametrize("listing", LISTINGS)
def test_rings_with_chords_across_the_word_borders(listing, labeled):
    """513 .. 2050 nodes: one node past gtok_sent's limit, both sides of multiples of 32 and 64 words' worth of nodes, a set of
    more than one 64-word round (2050 nodes = 65 words) - listed in both directions with and without the flag, shuffled, and in
    one direction only (the walk forms the symmetric closure)."""
    batch, coo = _border(listing, labeled)
    dev = batch.to(DEV)
    for max_len in (1 << 20, 600):
        ids, ln = gtok.ops.sent_large(dev, 2050, max_len, 7, 1, **_kw(labeled))
        ref, rln = _border_ref(listing, labeled, max_len)
        _cmp(ids, ln, ref, rln, f"rings {listing} labeled={labeled} max_len={max_len}")
        if max_len == 1 << 20:
            _lossless(coo, ids, ln, 2050, max_len, 7, 1, labeled)


# ------------------------------------------------------------------------------------------------ 4. long rows, brackets, dead ends
@functools.lru_cache(maxsize=None)
def _hard_shapes():
    rng = np.random.default_rng(41)
    star = np.stack([np.zeros(2999, np.int64), np.arange(1, 3000)], 1)                       # centre -> leaf only
    iu, iv = np.triu_indices(130, 1)
    path = np.stack([np.arange(2999), np.arange(1, 3000)], 1)
    sparse = rng.integers(0, 800, (2000, 2))                                                 # nodes 800 .. 1499 stay isolated
    sparse = sparse[sparse[:, 0] != sparse[:, 1]]
    ring = _ring_pairs(5000, 2000, rng)
    one = _graphs([star, path, sparse, ring], [3000, 3000, 1500, 5000], np.random.default_rng(42), "oneway")
    k130 = _graphs([np.stack([iu, iv], 1)], [130], np.random.default_rng(43), "both")        # rows of 129 entries
    return _concat(one, k130)


@pytest.mark.parametrize("labeled", [True, False])
def test_long_rows_long_brackets_many_dead_ends(labeled):
    d = _hard_shapes()
    batch, coo = both(d, labeled)
    assert batch.flags == 0
    ids, ln = gtok.ops.sent_large(batch.to(DEV), 5000, 1 << 20, 11, 0, **_kw(labeled))
    ref, rln = orc.sent(coo, 5000, 1 << 20, 11, 0, ld=ids.shape[1], nthreads=THREADS, **_kw(labeled))
    # the oracle's rows exercise the hard paths: a dead end per leaf of the star, a bracket of more than 64 members in K130
    assert int((ref[0, :rln[0]] == RESET).sum()) >= 2000
    row = ref[4, :rln[4]]
    opens, closes = np.nonzero(row == LADJ)[0], np.nonzero(row == RADJ)[0]
    assert int((closes - opens - 1).max()) // (2 if labeled else 1) > 64
    _cmp(ids, ln, ref, rln, f"hard shapes labeled={labeled}")
    _lossless(coo, ids, ln, 5000, 1 << 20, 11, 0, labeled)


def test_a_ring_of_the_largest_size_cut_at_600_tokens():
    n = MAXN
    a = np.arange(n, dtype=np.int64)
    d = dict(node_counts=np.array([n]), edge_counts=np.array([n]), src=a, dst=(a + 1) % n)
    batch, coo = both(d, False)
    assert batch.max_nodes == MAXN
    ids, ln = gtok.ops.sent_large(batch.to(DEV), n, 600, 13, 0)
    ref, rln = orc.sent(coo, n, 600, 13, 0, ld=ids.shape[1])
    assert rln[0] == 600
    _cmp(ids, ln, ref, rln, "largest ring")


# ------------------------------------------------------------------------------------------------ 5. output convention
def test_output_convention_narrow_slab_no_pad_u16_epochs():
    batch, coo = _border("oneway", False)
    dev = batch.to(DEV)
    G = batch.num_graphs
    full, fln = _border_ref("oneway", False, 600)
    # ld < max_len: the true length, beyond ld; rows hold the first 64 ids
    ids, ln = gtok.ops.sent_large(dev, 2050, 600, 7, 1, ld=64)
    assert np.array_equal(ln.cpu().numpy(), fln) and (fln > 64).all()
    assert np.array_equal(ids.cpu().numpy(), full[:, :64])
    # pad=False: compared through out_len
    out = (torch.full((G, full.shape[1]), -7, dtype=torch.int32, device=DEV), torch.empty(G, dtype=torch.int32, device=DEV))
    ids, ln = gtok.ops.sent_large(dev, 2050, 600, 7, 1, ld=full.shape[1], out=out, pad=False)
    assert np.array_equal(ln.cpu().numpy(), fln) and unpad(ids.cpu().numpy(), fln) == unpad(full, fln)
    # rows of 16-bit ids
    ids, ln = gtok.ops.sent_large(dev, 2050, 600, 7, 1, ld=full.shape[1], u16=True)
    assert ids.dtype == torch.int16
    _cmp(torch.from_numpy(ids.cpu().numpy().view(np.uint16).astype(np.int32)), ln, full, fln, "u16")
    # three epochs in one launch against three oracle calls
    ids, ln = gtok.ops.sent_large(dev, 2050, 600, 7, 4, ld=full.shape[1], epochs=3)
    assert tuple(ids.shape) == (3, G, full.shape[1]) and tuple(ln.shape) == (3, G)
    for e in range(3):
        ref, rln = orc.sent(coo, 2050, 600, 7, 4 + e, ld=full.shape[1], nthreads=THREADS)
        _cmp(ids[e], ln[e], ref, rln, f"epoch slice {e}")
    # an id space that cannot fit 16 bits
    with pytest.raises(gtok.GtokError, match="GTOK_E_TOO_LARGE"):
        gtok.ops.sent_large(dev, 65530, 600, 7, 1, u16=True)


# ------------------------------------------------------------------------------------------------ 6. several pairs per wave
@pytest.mark.parametrize("big_first", [False, True])
def test_a_wave_takes_several_pairs_and_reuses_its_slice(big_first):
    d = gtok.synth.zinc_like(WAVES + 900, seed=61)
    if big_first:   # a large walk followed by small ones in the same slice (and the same LDS)
        ring = _graphs([_ring_pairs(700, 100, np.random.default_rng(62))], [700], np.random.default_rng(63), "both")
        ring["edge_attr"] %= 4
        d = _concat(ring, d)
    x, ea = d["x"], d["edge_attr"]
    batch = gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], x, ea, check_symmetric=False)
    coo = orc.Coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], x, ea)
    assert batch.flags == 0 and batch.num_graphs > WAVES
    dev = batch.to(DEV)
    nn = 700 if big_first else 37
    kw = dict(labeled=True, num_node_types=28, num_edge_types=4)
    ids, ln = gtok.ops.sent_large(dev, nn, 1024, 9, 0, ld=256 if not big_first else None, **kw)
    ref, rln = orc.sent(coo, nn, 1024, 9, 0, ld=ids.shape[1], nthreads=THREADS, **kw)
    _cmp(ids, ln, ref, rln, "one epoch")
    ids, ln = gtok.ops.sent_large(dev, nn, 1024, 9, 0, ld=ids.shape[1], epochs=3, **kw)
    for e in range(3):
        ref, rln = orc.sent(coo, nn, 1024, 9, e, ld=ids.shape[2], nthreads=THREADS, **kw)
        _cmp(ids[e], ln[e], ref, rln, f"epoch {e} of 3")


# ------------------------------------------------------------------------------------------------ 8. damaged input
@pytest.mark.parametrize("labeled", [True, False])
def test_entries_with_an_endpoint_outside_the_graph_are_skipped(labeled):
    rng = np.random.default_rng(81)
    sizes = (600, 40)
    d = _graphs([_ring_pairs(n, 60, rng) for n in sizes], sizes, np.random.default_rng(82), "both")      # row-sorted: col == dst
    x, ea = (d["x"], d["edge_attr"]) if labeled else (None, None)
    batch = gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], x, ea, check_symmetric=False)
    assert batch.eorder is None and np.array_equal(batch.col.numpy(), d["dst"])
    dev = batch.to(DEV)
    dst = d["dst"].copy()
    hit = np.array([0, 1, 7, 300, 655, 1000, int(d["edge_counts"][0]) - 1, int(d["edge_counts"][0]) + 3])
    dst[hit] = np.where(np.arange(hit.size) % 2 == 0, 605, -1)                                          # N + 5 and -1
    dev.col[torch.from_numpy(hit).to(DEV)] = torch.from_numpy(dst[hit].astype(np.int32)).to(DEV)
    coo = orc.Coo(d["node_counts"], d["edge_counts"], d["src"], dst, x, ea)
    ids, ln = gtok.ops.sent_large(dev, 600, 1 << 20, 4, 0, **_kw(labeled))
    ref, rln = orc.sent(coo, 600, 1 << 20, 4, 0, ld=ids.shape[1], **_kw(labeled))
    _cmp(ids, ln, ref, rln, f"damaged labeled={labeled}")


def test_a_graph_beyond_the_claimed_maxima_is_clamped():
    rng = np.random.default_rng(83)
    d = _graphs([_ring_pairs(n, 60, rng) for n in (600, 30)], (600, 30), np.random.default_rng(84), "both")
    b, _ = both(d, False)
    b = b.to(DEV)
    for claim_n, claim_e in ((520, b.max_edges), (520, 700), (600, 100)):
        low = gtok.GraphBatch(b.num_graphs, claim_n, claim_e, b.node_ptr, b.edge_ptr, b.rowptr, b.col, None, None, None)
        ids, ln = gtok.ops.sent_large(low, 600, 4096, 1, 0, ld=4096)
        ln = ln.cpu().numpy()
        assert ((ln >= 0) & (ln <= 4096)).all()


# ------------------------------------------------------------------------------------------------ 9. error codes, bare ctypes
def test_error_codes_through_ctypes():
    L = _lib.lib()
    batch, _ = _border("oneway", False)
    b = batch.to(DEV)
    G = b.num_graphs
    cs = b.c_struct()
    ids = torch.empty((G, 64), dtype=torch.int32, device=DEV); ln = torch.empty(G, dtype=torch.int32, device=DEV)
    need = int(L.gtok_sent_large_workspace(b.max_nodes, b.max_edges, G))
    ws = torch.empty(need + 32, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 16 == 0
    P = lambda flags=0: _lib.GtokSentParams(2050, 0, 0, 0, 64, 0, 5, flags, 1, 0, 0, None, 1, 0)
    call = lambda cs_, p, w, nbytes, out=ids: L.gtok_sent_large(ctypes.byref(cs_), ctypes.byref(p), out.data_ptr() if out is not None else None,
                                                                64, ln.data_ptr(), w, nbytes, None)
    assert call(cs, P(), ws.data_ptr(), need) == 0
    assert call(cs, P(), ws.data_ptr(), need - 1) == -1                     # one byte short
    assert call(cs, P(), ws.data_ptr() + 8, need) == -1                     # misaligned
    assert call(cs, P(), None, need) == -1
    assert call(cs, P(), ws.data_ptr(), need, out=None) == -1
    assert call(cs, P(_lib.SENT_PACK_ONLY), ws.data_ptr(), need) == -1 and call(cs, P(_lib.SENT_U16 | _lib.SENT_PACK_U8), ws.data_ptr(), need) == -1
    order = torch.arange(G, dtype=torch.int32, device=DEV); units = torch.tensor([0, G], dtype=torch.int32, device=DEV)
    re = _lib.GtokCsr.from_buffer_copy(cs)
    re.graph_ids, re.unit_ptr, re.num_units = order.data_ptr(), units.data_ptr(), 1
    assert call(re, P(), ws.data_ptr(), need) == -1                         # a reordered batch
    lab = _lib.GtokSentParams(2050, 1, 28, 6, 64, 0, 5, 0, 1, 0, 0, None, 1, 0)
    assert call(cs, lab, ws.data_ptr(), need) == -1                         # labelled without attributes
    big = _lib.GtokCsr.from_buffer_copy(cs)
    big.max_nodes = MAXN + 1
    assert call(big, P(), ws.data_ptr(), ws.numel()) == -2                  # GTOK_E_TOO_LARGE
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 10. the call sites
def test_tokenizer_dataset_and_torch_op_take_large_graphs():
    batch, coo = _border("oneway", False)
    dev = batch.to(DEV)
    tok = gtok.Graph2TrailTokenizer(dataset_names=[], max_length=600, truncation_length=600, labeled_graph=False, seed=7, device=DEV)
    tok.set_num_nodes(2050)
    ids, ln = tok.tokenize_batch(dev, epoch=1)
    ref, rln = _border_ref("oneway", False, 600)
    _cmp(ids, ln, ref, rln, "tokenize_batch")
    assert gtok.ops.last_sent_kernel() == "sent_large_kernel"
    # torch.ops.gtok.sent_large == ops.sent_large
    tids, tln = torch.ops.gtok.sent_large(dev.node_ptr, dev.edge_ptr, dev.rowptr, dev.col, None, None, None, dev.max_nodes, dev.max_edges,
                                          2050, 600, int(ids.shape[1]), 7, 1, False, 0, 0, False, 5, 0)
    assert torch.equal(tids, ids) and torch.equal(tln, ln)
    # ops.sent keeps refusing what it refused
    small, _ = both(_graphs([_ring_pairs(513, 3, np.random.default_rng(1))], [513], np.random.default_rng(2), "both"), False)
    with pytest.raises(gtok.GtokError):
        gtok.ops.sent(small.to(DEV), 513, 64, 0)

    # tokenizer(data) for one 700-node item
    d1 = _graphs([_ring_pairs(700, 50, np.random.default_rng(3))], [700], np.random.default_rng(4), "oneway")
    item = PygDataLike(x=torch.from_numpy(d1["x"]).view(-1, 1), edge_index=torch.from_numpy(np.stack([d1["src"], d1["dst"]])),
                       edge_attr=torch.from_numpy(d1["edge_attr"]), y=torch.tensor([0.5]))
    tok1 = gtok.Graph2TrailTokenizer(dataset_names=[], max_length=1 << 16, labeled_graph=False, seed=7, device=DEV)
    tok1.set_num_nodes(700)
    row = tok1(item)
    _, c1 = both(d1, False)
    ref1, rln1 = orc.sent(c1, 700, 1 << 16, 7, 0, ld=8192)
    assert row.dtype == torch.long and row.tolist() == ref1[0, :rln1[0]].tolist()

    # a 40-graph split of 513 - 900-node graphs through the dataset class
    rng = np.random.default_rng(5)
    sizes = [513, 900] + rng.integers(513, 901, 38).tolist()
    d40 = _graphs([_ring_pairs(n, 40, rng) for n in sizes], sizes, np.random.default_rng(6), "oneway")
    d40["y"] = np.arange(40, dtype=np.float32)
    tok2 = gtok.Graph2TrailTokenizer(dataset_names=[], max_length=4096, truncation_length=4096, labeled_graph=True, seed=3, device=DEV)
    tok2.set_num_nodes(900); tok2.set_num_node_and_edge_types(28, 6)
    ds = gtok.agtt.TokenizedGraphDataset(PygInMemoryLike(d40), tok2, task="zinc", device=DEV)
    ids, ln = ds.tokenize_epoch(0)
    _, c40 = both(d40, True)
    ref, rln = orc.sent(c40, 900, 4096, 3, 0, ld=ids.shape[1], nthreads=THREADS, **LAB)
    _cmp(ids, ln, ref, rln, "TokenizedGraphDataset.tokenize_epoch")
    ids16, ln16 = ds.tokenize_epoch_u16(0)
    assert np.array_equal(ln16.cpu().numpy(), rln)
    t, m, y, _ = gtok.agtt.TokenizedGraphDataset(PygInMemoryLike(d40), tok2, task="zinc", device=DEV)[3]      # a first fetch: epoch 0
    assert t.tolist() == ref[3, :rln[3]].tolist() and bool(m.all()) and y == 3.0
