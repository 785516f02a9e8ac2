"""gtok_sent_decode_sizes / gtok_sent_decode_csr (include/gtok.h): SENT rows back to a batched CSR on the device.

The expected result of every test is built the same way: the C oracle's decoder (oracle_sent_decode, the state machine the
kernel restates) with capacities nothing can exceed, its edges interleaved (a -> b, then b -> a; a self loop once; a status-1
row an empty graph), and the HOST GraphBatch.from_coo over that list.  Everything is compared exactly."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from _util import both, edge_case_graphs, gtok, orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THREADS = 16
_lib = gtok._lib
MAXN = _lib.SENT_LARGE_MAX_NODES
LAB = dict(labeled=True, num_node_types=28, num_edge_types=6)
SOS, RESET, LADJ, RADJ, EOS, PAD, IDX = 0, 1, 2, 3, 4, 5, 6


def _kw(labeled):
    return dict(LAB) if labeled else dict(labeled=False)


# ------------------------------------------------------------------------------------------------ the expected batch
def _interleave(a, b, t):
    """edges (a, b, t) in stream order -> entries a -> b, b -> a (a self loop: one entry)"""
    keep = np.ones((a.size, 2), bool)
    keep[:, 1] = a != b
    src = np.stack([a, b], 1)[keep]; dst = np.stack([b, a], 1)[keep]; ty = np.stack([t, t], 1)[keep]
    return src.astype(np.int64), dst.astype(np.int64), ty.astype(np.int64)


def expected(ids, ln, max_num_nodes, labeled, nt):
    """ids int32 [G, ld], ln [G] on the host -> dict(status, batch = host GraphBatch, src, dst: the interleaved lists per graph)"""
    ids = np.ascontiguousarray(ids, np.int32); ln = np.asarray(ln, np.int32)
    G, ld = ids.shape
    dec = orc.sent_decode_rows(ids, ln, max_num_nodes, labeled, nt, edge_cap=ld, node_cap=max(1, max_num_nodes))
    st = dec["status"]
    assert not (st == 2).any()
    ncs, ecs, srcs, dsts, tys, xs, lists = [], [], [], [], [], [], []
    for g in range(G):
        n, m = (0, 0) if st[g] == 1 else (int(dec["num_nodes"][g]), int(dec["num_edges"][g]))
        s, d, ty = _interleave(dec["edge_a"][g, :m], dec["edge_b"][g, :m], dec["edge_type"][g, :m])
        ncs.append(n); ecs.append(s.size); srcs.append(s); dsts.append(d); tys.append(ty); xs.append(dec["node_type"][g, :n].astype(np.int64))
        lists.append((s, d, ty, xs[-1]))
    cat = lambda l: np.concatenate(l) if l else np.zeros(0, np.int64)
    batch = gtok.GraphBatch.from_coo(np.array(ncs, np.int64), np.array(ecs, np.int64), cat(srcs), cat(dsts),
                                     cat(xs) if labeled else None, cat(tys) if labeled else None, check_symmetric=False)
    return dict(status=st, batch=batch, lists=lists, node_counts=np.array(ncs, np.int64), edge_counts=np.array(ecs, np.int64),
                src=cat(srcs), dst=cat(dsts), x=cat(xs), edge_attr=cat(tys))


def _identity_order(edge_ptr):
    ep = edge_ptr.cpu().numpy()
    E = int(ep[-1])
    return (np.arange(E) - np.repeat(ep[:-1], np.diff(ep))).astype(np.int32)


def same_batch(got, want, what):
    """two GraphBatches (device or host) hold the same arrays and maxima"""
    h = lambda t: None if t is None else t.cpu().numpy()
    assert got.num_graphs == want.num_graphs, what
    for k in ("node_ptr", "edge_ptr", "rowptr", "col", "nattr", "eattr"):
        a, b = h(getattr(got, k)), h(getattr(want, k))
        assert (a is None) == (b is None), (what, k)
        if a is not None:
            assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
            bad = np.nonzero(a != b)[0]
            assert bad.size == 0, f"{what}: {k} differs at {bad[:8]}: {a[bad[:8]]} vs {b[bad[:8]]}"
    eo = lambda x: _identity_order(x.edge_ptr) if x.eorder is None else h(x.eorder)
    assert np.array_equal(eo(got), eo(want)), (what, "eorder")
    for k in ("max_degree", "max_nodes", "max_edges", "chunk_nodes", "chunk_edges"):       # info[1..5]
        assert getattr(got, k) == getattr(want, k), (what, k, getattr(got, k), getattr(want, k))


def check(got, status, exp, what):
    st = status.cpu().numpy()
    bad = np.nonzero(st != exp["status"])[0]
    assert bad.size == 0, f"{what}: status differs at rows {bad[:8]}: {st[bad[:8]]} vs {exp['status'][bad[:8]]}"
    same_batch(got, exp["batch"], what)


def decode_and_check(ids, ln, max_num_nodes, labeled, what):
    nt = 28 if labeled else 0
    got, st = gtok.ops.sent_decode_csr(ids, ln, max_num_nodes, labeled, nt)
    h = ids.cpu().numpy()
    if h.dtype == np.int16:
        h = h.view(np.uint16).astype(np.int32)
    exp = expected(h, ln.cpu().numpy(), max_num_nodes, labeled, nt)
    check(got, st, exp, what)
    return got, st, exp


# ------------------------------------------------------------------------------------------------ 1. hand-made graphs
@pytest.mark.parametrize("labeled", [True, False])
def test_hand_made_graphs_whole_and_cut(labeled):
    """empty graph, one node, isolated nodes, self loops, duplicates, types 200 / 254 / 77; max_len 9, 5 and 1 cut inside a bracket
    and between a position and its type"""
    batch, _ = both(edge_case_graphs(), labeled)
    dev = batch.to(DEV)
    seen = set()
    for max_len in (4096, 9, 5, 1):
        ids, ln = gtok.ops.sent(dev, 8, max_len, 3, 2, **_kw(labeled))
        _, st, exp = decode_and_check(ids, ln, 8, labeled, f"hand-made labeled={labeled} max_len={max_len}")
        seen |= set(exp["status"].tolist())
        if max_len == 4096:
            assert (exp["status"] == 0).all()
            assert np.array_equal(np.sort(exp["node_counts"]), np.sort(edge_case_graphs()["node_counts"]))
    assert seen == {0, 3}


# ------------------------------------------------------------------------------------------------ 2. molecules, every row format
@functools.lru_cache(maxsize=None)
def _molecules(max_len):
    d = gtok.synth.zinc_like(300, seed=21)
    batch, coo = both(d)
    dev = batch.to(DEV)
    kw = dict(labeled=True, num_node_types=28, num_edge_types=4)
    ids, ln = gtok.ops.sent(dev, 37, max_len, 5, 3, **kw)
    exp = expected(ids.cpu().numpy(), ln.cpu().numpy(), 37, True, 28)
    return batch, ids, ln, exp


@pytest.mark.parametrize("max_len", [4096, 50])
def test_molecules_as_slab_u16_slab_and_packed_rows(max_len):
    batch, ids, ln, exp = _molecules(max_len)
    dev = batch.to(DEV)
    got, st = gtok.ops.sent_decode_csr(ids, ln, 37, True, 28)
    check(got, st, exp, f"int32 slab max_len={max_len}")
    ln_h = ln.cpu().numpy()                                           # (a row of exactly max_len tokens may still end in EOS)
    assert (exp["status"][ln_h < max_len] == 0).all() and (ln_h[exp["status"] == 3] == max_len).all()
    assert max_len != 50 or (exp["status"] == 3).sum() > 100
    ld = int(ids.shape[1])
    # the same rows as a slab of 16-bit ids (written by the walk)
    i16, l16 = gtok.ops.sent(dev, 37, max_len, 5, 3, labeled=True, num_node_types=28, num_edge_types=4, u16=True, ld=ld)
    assert i16.dtype == torch.int16 and torch.equal(l16, ln)
    g16, s16 = gtok.ops.sent_decode_csr(i16, l16, 37, True, 28)
    assert torch.equal(s16, st)
    same_batch(g16, got, "16-bit slab")
    # packed rows at 1, 2 and 4 bytes per id
    for eb, align in ((1, 16), (2, 8), (4, 1)):
        packed, row_ptr, pst = gtok.ops.pack_rows_scan(ids, ln, eb, 300 * ld, align)
        assert int(pst.item()) == 0 and packed.element_size() == eb
        gp, sp = gtok.ops.sent_decode_csr(packed, ln, 37, True, 28, row_start=row_ptr[:-1].contiguous(), ld=ld)
        assert torch.equal(sp, st)
        same_batch(gp, got, f"packed rows, {eb} bytes per id")
    # a row that did not fit its packed buffer (row_start -1) is an empty graph, status 1
    starts = row_ptr[:-1].clone()
    starts[7] = -1
    gm, sm = gtok.ops.sent_decode_csr(packed, ln, 37, True, 28, row_start=starts, ld=ld)
    ln0 = ln.cpu().numpy().copy(); ln0[7] = 0
    check(gm, sm, expected(ids.cpu().numpy(), ln0, 37, True, 28), "row_start -1")
    assert int(sm[7]) == 1 and int(gm.node_ptr[8] - gm.node_ptr[7]) == 0
    if max_len == 4096:
        # uncut molecules come back simple and symmetric, with the input's degree sequences
        assert (exp["status"] == 0).all()
        gf, _ = gtok.ops.sent_decode_csr(ids, ln, 37, True, 28, check_symmetric=True)
        assert gf.flags & _lib.CSR_SIMPLE_SYMMETRIC and gf.checked
        assert not (got.flags & _lib.CSR_SIMPLE_SYMMETRIC)
        same_batch(gf, got, "check_symmetric")
        rp, np_ = got.rowptr.cpu().numpy(), got.node_ptr.cpu().numpy()
        irp, inp = batch.rowptr.numpy(), batch.node_ptr.numpy()
        assert np.array_equal(np_, inp)
        for g in range(300):
            deg = np.diff(rp[np_[g] + g:np_[g + 1] + g + 1]); ideg = np.diff(irp[inp[g] + g:inp[g + 1] + g + 1])
            assert np.array_equal(np.sort(deg), np.sort(ideg)), g


# ------------------------------------------------------------------------------------------------ 3. long brackets, chunk borders
def _complete(n):
    iu, iv = np.triu_indices(n, 1)
    return np.concatenate([iu, iv]), np.concatenate([iv, iu])


def test_brackets_longer_than_a_chunk_and_rows_that_end_at_chunk_borders():
    parts = [_complete(40), _complete(70), (np.array([0, 1, 1, 2]), np.array([1, 0, 2, 1]))]
    d = dict(node_counts=np.array([40, 70, 3]), edge_counts=np.array([p[0].size for p in parts]),
             src=np.concatenate([p[0] for p in parts]).astype(np.int64), dst=np.concatenate([p[1] for p in parts]).astype(np.int64))
    batch, _ = both(d, False)
    ids, ln = gtok.ops.sent(batch.to(DEV), 70, 1 << 20, 9, 0)
    row = ids[1, :int(ln[1])].cpu().numpy()
    opens, closes = np.nonzero(row == LADJ)[0], np.nonzero(row == RADJ)[0]
    assert int((closes - opens - 1).max()) > 64                      # a bracket of more than one 64-token chunk
    _, _, exp = decode_and_check(ids, ln, 70, False, "complete graphs, whole")
    assert (exp["status"] == 0).all() and exp["edge_counts"].tolist() == [40 * 39, 70 * 69, 4]
    for cut in (63, 64, 65, 128, 129):
        _, _, exp = decode_and_check(ids, torch.clamp(ln, max=cut), 70, False, f"complete graphs cut at {cut}")
        assert exp["status"].tolist() == [3, 3, 0]


# ------------------------------------------------------------------------------------------------ 4. large graphs
def _ring_pairs(n, chords, rng):
    pairs = {(i, i + 1) for i in range(n - 1)} | {(0, n - 1)}
    while len(pairs) < n + chords:
        a, b = sorted(rng.integers(0, n, 2).tolist())
        if a != b:
            pairs.add((a, b))
    return np.array(sorted(pairs), np.int64)


@pytest.mark.parametrize("labeled", [True, False])
def test_rings_with_chords_of_513_to_2050_nodes(labeled):
    """labelled with both directions listed, unlabelled with one direction listed; rows from gtok_sent_large"""
    rng = np.random.default_rng(41)
    sizes = (513, 1025, 2050)
    srcs, dsts = [], []
    for n in sizes:
        e = _ring_pairs(n, 300, rng)
        a, b = e[:, 0], e[:, 1]
        if labeled:
            s, t = np.concatenate([a, b]), np.concatenate([b, a])
            o = np.lexsort((t, s))
            a, b = s[o], t[o]
        srcs.append(a); dsts.append(b)
    d = dict(node_counts=np.array(sizes), edge_counts=np.array([s.size for s in srcs]), src=np.concatenate(srcs), dst=np.concatenate(dsts))
    d["x"] = rng.integers(0, 28, int(sum(sizes))); d["edge_attr"] = (d["src"] + d["dst"]) % 5
    batch, _ = both(d, labeled)
    ids, ln = gtok.ops.sent_large(batch.to(DEV), 2050, 1 << 20, 7, 1, **_kw(labeled))
    _, _, exp = decode_and_check(ids, ln, 2050, labeled, f"rings labeled={labeled}")
    assert (exp["status"] == 0).all() and exp["node_counts"].tolist() == list(sizes)
    assert exp["edge_counts"].tolist() == [2 * (n + 300) for n in sizes]
    _, _, exp = decode_and_check(ids, torch.clamp(ln, max=1000), 2050, labeled, f"rings labeled={labeled}, cut at 1000")
    assert (exp["status"] == 3).all()


def test_a_ring_of_the_largest_size_beside_a_triangle():
    """16,384 nodes: the upper bound of the row cursors in LDS (64 KB, one wave per workgroup)"""
    a = np.arange(MAXN, dtype=np.int64)
    d = dict(node_counts=np.array([MAXN, 3]), edge_counts=np.array([MAXN, 3]), src=np.concatenate([a, [0, 1, 2]]),
             dst=np.concatenate([(a + 1) % MAXN, [1, 2, 0]]))
    batch, _ = both(d, False)
    ids, ln = gtok.ops.sent_large(batch.to(DEV), MAXN, 1 << 20, 13, 0)
    got, _, exp = decode_and_check(ids, ln, MAXN, False, "largest ring")
    assert exp["status"].tolist() == [0, 0] and exp["node_counts"].tolist() == [MAXN, 3] and exp["edge_counts"].tolist() == [2 * MAXN, 6]
    assert got.max_degree == 2


def test_labelled_rows_at_the_largest_max_num_nodes_where_no_entry_is_staged():
    """Labelled rows decoded with max_num_nodes = 16,384: the row cursors fill the workgroup's LDS, the launcher drops the stage
    of the first parse, and every row - a single node, isolated nodes (no entry at all), self loops, edges, a 300-node ring
    whose node types come in more than one batch of 64 - gets its entries AND its node types from the second parse.  max_len 2
    cuts every row between its first position and that node's type (type 255)."""
    hand = edge_case_graphs()
    e = _ring_pairs(300, 40, np.random.default_rng(45))
    s, t = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
    o = np.lexsort((t, s))
    ring = dict(node_counts=np.array([300]), edge_counts=np.array([s.size]), src=s[o], dst=t[o],
                x=1 + np.arange(300) % 27, edge_attr=1 + (s[o] + t[o]) % 5)
    d = {k: np.concatenate([np.asarray(hand[k], np.int64), np.asarray(ring[k], np.int64)]) for k in hand}
    batch, _ = both(d, True)
    dev = batch.to(DEV)
    for max_len in (4096, 9, 5, 2, 1):
        ids, ln = gtok.ops.sent(dev, MAXN, max_len, 3, 2, **LAB)
        got, _, exp = decode_and_check(ids, ln, MAXN, True, f"labelled, max_num_nodes {MAXN}, max_len {max_len}")
        if max_len == 4096:
            assert (exp["status"] == 0).all() and exp["node_counts"].tolist() == d["node_counts"].tolist()
            assert exp["edge_counts"][1] == 0 and exp["edge_counts"][2] == 0          # one node; five isolated nodes
            x = got.nattr.cpu().numpy()
            assert x[0] == 3 and sorted(x[1:6].tolist()) == [0, 1, 2, 9, 27] and (x[-300:] > 0).all()      # (visit order permutes them)
        if max_len == 2:
            whole = d["node_counts"] == 0                                             # (the empty graph's row is SOS EOS)
            assert exp["node_counts"].tolist() == (1 - whole).tolist() and (exp["status"][~whole] == 3).all()
            assert (got.nattr.cpu().numpy() == 255).all() and got.num_edges_total == 0


# ------------------------------------------------------------------------------------------------ 5. grid tails
@pytest.mark.parametrize("rows", [1000, 1])
def test_grid_tails(rows):
    d = gtok.synth.zinc_like(rows, seed=51)
    batch, _ = both(d)
    ids, ln = gtok.ops.sent(batch.to(DEV), 37, 1024, 2, 0, labeled=True, num_node_types=28, num_edge_types=4)
    _, _, exp = decode_and_check(ids, ln, 37, True, f"{rows} rows")
    assert (exp["status"] == 0).all()


# ------------------------------------------------------------------------------------------------ raw calls (7, 9, num_rows = 0)
GUARD = 4096
FILL32, FILL8 = -77, 0xAB


class Raw:
    """caller-side arrays of gtok_sent_decode_csr with 4,096-element guard regions on both sides of every output"""

    def __init__(self, rows, N, E, labeled):
        self.sizes = dict(rowptr=N + rows, col=E, eorder=E, nattr=N if labeled else 0, eattr=E if labeled else 0, info=8)
        self.buf = {}
        for k, n in self.sizes.items():
            u8 = k in ("nattr", "eattr")
            self.buf[k] = torch.full((GUARD + n + GUARD,), FILL8 if u8 else FILL32, dtype=torch.uint8 if u8 else torch.int32, device=DEV)
        self.labeled = labeled

    def view(self, k):
        return self.buf[k][GUARD:GUARD + self.sizes[k]]

    def struct(self, node_ptr, edge_ptr):
        p = lambda k: self.buf[k].data_ptr() + GUARD * self.buf[k].element_size()
        typed = lambda k: p(k) if (self.labeled or k not in ("nattr", "eattr")) else None
        return _lib.GtokCsrBuilt(node_ptr.data_ptr(), edge_ptr.data_ptr(), p("rowptr"), p("col"), p("eorder"), typed("nattr"), typed("eattr"), p("info"))

    def guards_untouched(self):
        for k, b in self.buf.items():
            fill = FILL8 if b.dtype == torch.uint8 else FILL32
            assert bool((b[:GUARD] == fill).all()) and bool((b[GUARD + self.sizes[k]:] == fill).all()), k

    def untouched(self):
        self.guards_untouched()
        for k, b in self.buf.items():
            assert bool((b == (FILL8 if b.dtype == torch.uint8 else FILL32)).all()), k


def _call_csr(ids, eb, ld, ln, rows, maxn, labeled, nt, cout):
    return _lib.lib().gtok_sent_decode_csr(None if ids is None else ids.data_ptr(), eb, None, ld, None if ln is None else ln.data_ptr(), rows, maxn,
                                           int(labeled), nt, ctypes.byref(cout), None)


def test_slices_that_do_not_match_are_skipped_and_nothing_is_written_outside():
    batch, ids, ln, exp = _molecules(4096)
    want = exp["batch"]
    rows, ld = int(ids.shape[0]), int(ids.shape[1])
    nc, ec = exp["node_counts"].copy(), exp["edge_counts"].copy()
    ec[11] -= 1                      # one entry too few for row 11
    nc[200] -= 1                     # one node too few for row 200
    node_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(nc)]).astype(np.int32)).to(DEV)
    edge_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(ec)]).astype(np.int64)).to(DEV)
    N, E = int(nc.sum()), int(ec.sum())
    raw = Raw(rows, N, E, True)
    assert _call_csr(ids, 4, ld, ln, rows, 37, True, 28, raw.struct(node_ptr, edge_ptr)) == 0
    torch.cuda.synchronize()
    raw.guards_untouched()
    info = raw.view("info").cpu().numpy()
    assert info[0] == 2 and info[6] == 0
    # every other graph is exact, inside its own (shifted) slice
    g_np, g_ep = node_ptr.cpu().numpy(), edge_ptr.cpu().numpy()
    w_np, w_ep = want.node_ptr.numpy(), want.edge_ptr.numpy()
    out = {k: raw.view(k).cpu().numpy() for k in ("rowptr", "col", "eorder", "nattr", "eattr")}
    w_eo = _identity_order(want.edge_ptr) if want.eorder is None else want.eorder.numpy()
    for g in range(rows):
        if g in (11, 200):
            continue
        n, e = int(nc[g]), int(ec[g])
        assert np.array_equal(out["rowptr"][g_np[g] + g:g_np[g] + g + n + 1], want.rowptr.numpy()[w_np[g] + g:w_np[g] + g + n + 1]), g
        assert np.array_equal(out["col"][g_ep[g]:g_ep[g] + e], want.col.numpy()[w_ep[g]:w_ep[g] + e]), g
        assert np.array_equal(out["eorder"][g_ep[g]:g_ep[g] + e], w_eo[w_ep[g]:w_ep[g] + e]), g
        assert np.array_equal(out["nattr"][g_np[g]:g_np[g] + n], want.nattr.numpy()[w_np[g]:w_np[g] + n]), g
        assert np.array_equal(out["eattr"][g_ep[g]:g_ep[g] + e], want.eattr.numpy()[w_ep[g]:w_ep[g] + e]), g
    # the two skipped rows' slices were left alone
    assert (out["col"][g_ep[11]:g_ep[12]] == FILL32).all() and (out["nattr"][g_np[200]:g_np[201]] == FILL8).all()


def test_error_codes_and_no_rows_leave_the_outputs_untouched():
    batch, ids, ln, exp = _molecules(4096)
    rows, ld = int(ids.shape[0]), int(ids.shape[1])
    want = exp["batch"]
    node_ptr, edge_ptr = want.node_ptr.to(DEV), want.edge_ptr.to(DEV)
    raw = Raw(rows, want.num_nodes_total, want.num_edges_total, True)
    cout = raw.struct(node_ptr, edge_ptr)
    assert _call_csr(ids, 3, ld, ln, rows, 37, True, 28, cout) == -1                  # elem_bytes 3: GTOK_E_INVAL
    assert _call_csr(ids, 4, ld, ln, rows, MAXN + 1, True, 28, cout) == -2            # GTOK_E_TOO_LARGE
    assert _call_csr(ids, 4, ld, None, rows, 37, True, 28, cout) == -1                # null len
    assert _call_csr(ids, 4, 0, ln, rows, 37, True, 28, cout) == -1                   # ld <= 0
    assert _call_csr(ids, 4, ld, ln, -1, 37, True, 28, cout) == -1
    assert _call_csr(ids, 4, ld, ln, 0, 37, True, 28, cout) == 0                      # no rows: a no-op
    assert _call_csr(None, 4, ld, None, 0, 37, True, 28, cout) == 0
    sizes = [torch.full((rows,), FILL32, dtype=torch.int32, device=DEV) for _ in range(3)]
    call_sizes = lambda eb, ln_, n, maxn: _lib.lib().gtok_sent_decode_sizes(ids.data_ptr(), eb, None, ld, None if ln_ is None else ln_.data_ptr(), n, maxn,
                                                                           1, 28, *[t.data_ptr() for t in sizes], None)
    assert call_sizes(3, ln, rows, 37) == -1 and call_sizes(4, ln, rows, MAXN + 1) == -2 and call_sizes(4, None, rows, 37) == -1
    assert call_sizes(4, ln, 0, 37) == 0
    torch.cuda.synchronize()
    raw.untouched()
    assert all(bool((t == FILL32).all()) for t in sizes)
    with pytest.raises(gtok.GtokError, match="GTOK_E_TOO_LARGE"):
        gtok.ops.sent_decode_csr(ids, ln, MAXN + 1, True, 28)
    empty, st = gtok.ops.sent_decode_csr(ids[:0], ln[:0], 37, True, 28)
    assert empty.num_graphs == 0 and st.numel() == 0 and empty.col.numel() == 0 and empty.rowptr.numel() == 0


# ------------------------------------------------------------------------------------------------ 6. damaged rows
def _damage(ids, ln, maxn, labeled, nt, copies, rng):
    """`copies` copies of random rows of a valid slab, each with one or two changes"""
    node_off, edge_off = IDX + maxn, IDX + maxn + nt
    R, ld = ids.shape
    out = np.full((copies, ld), PAD, np.int32); oln = np.empty(copies, np.int32)
    for c in range(copies):
        r = int(rng.integers(0, R))
        L = int(min(ln[r], ld))
        row = ids[r, :L].tolist()
        for _ in range(int(rng.integers(1, 3))):
            L = len(row)
            if L == 0:
                break
            kind = int(rng.integers(0, 6))
            i = int(rng.integers(1, L)) if L > 1 else 0
            if kind == 0:
                row[i] = int(rng.integers(0, 6))                                        # a special id
            elif kind == 1:
                seen = len({t for t in row[:i] if IDX <= t < node_off})
                row[i] = IDX + int(rng.integers(seen, maxn)) if seen < maxn else PAD    # a position >= the nodes seen
            elif kind == 2:
                t = row[i]                                                              # an id below the range its slot needs
                row[i] = edge_off - 1 - int(rng.integers(0, 4)) if t >= edge_off else node_off - 1 if t >= node_off else PAD
            elif kind == 3:
                del row[i]                                                              # a deleted token
            elif kind == 4:
                row = row[:int(rng.integers(1, L + 1))]                                 # a shorter len
            else:
                row = row[1:]                                                           # SOS removed
        out[c, :len(row)] = row; oln[c] = len(row)
    return out, oln


def test_damaged_rows_get_the_oracles_status_and_graphs():
    rng = np.random.default_rng(6)
    counts = np.zeros(4, np.int64)
    for labeled in (True, False):
        d = gtok.synth.zinc_like(200, seed=61 + labeled)
        batch, _ = both(d, labeled)
        kw = dict(labeled=True, num_node_types=28, num_edge_types=4) if labeled else dict(labeled=False)
        ids, ln = gtok.ops.sent(batch.to(DEV), 37, 1024, 8, 0, **kw)
        bad_ids, bad_ln = _damage(ids.cpu().numpy(), ln.cpu().numpy(), 37, labeled, 28 if labeled else 0, 1000, rng)
        got, st, exp = decode_and_check(torch.from_numpy(bad_ids).to(DEV), torch.from_numpy(bad_ln).to(DEV), 37, labeled, f"damaged labeled={labeled}")
        counts += np.bincount(exp["status"], minlength=4)
        # info[6]: the status-1 rows (every one an empty graph)
        nt = 28 if labeled else 0
        nn, ne, s2 = gtok.ops.sent_decode_sizes(torch.from_numpy(bad_ids).to(DEV), torch.from_numpy(bad_ln).to(DEV), 37, labeled, nt)
        o = gtok.ops._decode_csr_launch(torch.from_numpy(bad_ids).to(DEV), torch.from_numpy(bad_ln).to(DEV), None, None, 37, labeled, nt,
                                        got.node_ptr, got.edge_ptr, got.num_nodes_total, got.num_edges_total)
        info = o["info"].cpu().numpy()
        assert info[0] == 0 and info[6] == int((exp["status"] == 1).sum())
        assert torch.equal(s2, st) and bool((nn[st == 1] == 0).all()) and bool((ne[st == 1] == 0).all())
    assert counts[0] >= 100 and counts[1] >= 100 and counts[3] >= 100 and counts[2] == 0, counts


# ------------------------------------------------------------------------------------------------ 8. through the interface
def test_tokenizer_and_torch_op_and_the_round_trip_of_the_format():
    batch, ids, ln, exp = _molecules(4096)
    dev = batch.to(DEV)
    tok = gtok.Graph2TrailTokenizer(dataset_names=[], max_length=4096, truncation_length=4096, labeled_graph=True, seed=5, device=DEV)
    tok.set_num_nodes(37); tok.set_num_node_and_edge_types(28, 4)
    tids, tln = tok.tokenize_batch(dev, epoch=3)
    assert torch.equal(tids, ids) and torch.equal(tln, ln)
    want, wst = gtok.ops.sent_decode_csr(ids, ln, 37, True, 28)
    got, st = tok.decode_batch(tids, tln)
    assert torch.equal(st, wst)
    same_batch(got, want, "decode_batch")
    for r in (0, 17, 299):
        one = tok.decode(ids[r, :int(ln[r])].to(torch.long).cpu())
        s, d, ty, x = exp["lists"][r]
        assert one["status"] == 0 and one["num_nodes"] == x.size
        assert np.array_equal(one["edge_index"].numpy(), np.stack([s, d])) and np.array_equal(one["edge_attr"].numpy(), np.minimum(ty, 255))
        assert np.array_equal(one["x"].numpy(), x)
    # torch.ops.gtok.sent_decode_sizes / sent_decode_csr == ops
    nn, ne, s3 = torch.ops.gtok.sent_decode_sizes(ids, ln, 37, True, 28)
    assert torch.equal(s3, wst) and torch.equal(torch.cumsum(nn, 0), want.node_ptr[1:].to(torch.int64))
    rowptr, col, eorder, nattr, eattr, info = torch.ops.gtok.sent_decode_csr(ids, ln, 37, True, 28, want.node_ptr, want.edge_ptr,
                                                                             want.num_nodes_total, want.num_edges_total)
    assert torch.equal(rowptr, want.rowptr) and torch.equal(col, want.col) and torch.equal(nattr, want.nattr) and torch.equal(eattr, want.eattr)
    v = info.tolist()
    assert v[0] == 0 and v[1:6] == [want.max_degree, want.max_nodes, want.max_edges, want.chunk_nodes, want.chunk_edges] and v[6] == 0
    assert np.array_equal(eorder.cpu().numpy(), _identity_order(want.edge_ptr) if want.eorder is None else want.eorder.cpu().numpy())
    # the decoded batch is a batch like any other: walked again, its rows decode to the decoded graphs
    flagged, _ = gtok.ops.sent_decode_csr(ids, ln, 37, True, 28, check_symmetric=True)
    assert flagged.flags & _lib.CSR_SIMPLE_SYMMETRIC
    ids2, ln2 = gtok.ops.sent(flagged, 37, 4096, 11, 0, labeled=True, num_node_types=28, num_edge_types=4)
    coo = orc.Coo(exp["node_counts"], exp["edge_counts"], exp["src"], exp["dst"], exp["x"], exp["edge_attr"])
    rt = orc.sent_roundtrip(coo, ids2.cpu().numpy(), ln2.cpu().numpy(), 37, 4096, 11, 0, labeled=True, num_node_types=28, nthreads=THREADS)
    assert (rt == 0).all(), rt
