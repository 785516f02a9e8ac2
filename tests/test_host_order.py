"""gtok_sent_large_order / gtok_csr_relabel, the parts that need no GPU: the two host references the GPU tests measure against
(tests/_sent_walk_ref.py pinned to the C oracle token for token, tests/_relabel_ref.py on graphs whose answer is known), the
binding, the host-side argument errors, the torch ops' meta kernels and the tokenizer's signature."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import _relabel_ref as rref
import _sent_walk_ref as wref
from _util import gtok, orc

_lib = gtok._lib
NAMES = ("gtok_sent_large_order", "gtok_csr_relabel_workspace", "gtok_csr_relabel")


def random_multigraphs(count, seed, max_n=13, max_e=30):
    """multigraphs of 0 .. max_n nodes with self loops and duplicates, typed"""
    rng = np.random.default_rng(seed)
    nc = rng.integers(0, max_n + 1, count)
    ec = np.where(nc > 0, rng.integers(0, max_e + 1, count), 0)
    src = np.concatenate([rng.integers(0, max(n, 1), e) for n, e in zip(nc, ec)]).astype(np.int64)
    dst = np.concatenate([rng.integers(0, max(n, 1), e) for n, e in zip(nc, ec)]).astype(np.int64)
    return dict(node_counts=nc, edge_counts=ec, src=src, dst=dst, x=rng.integers(0, 9, int(nc.sum())), edge_attr=rng.integers(0, 5, int(ec.sum())))


@pytest.mark.parametrize("labeled", [True, False])
@pytest.mark.parametrize("max_len", [4096, 17])
def test_the_python_walk_equals_the_oracle_token_for_token(labeled, max_len):
    """300 graphs per case, 1,200 rows in all: tokens and lengths are oracle.sent's; the visit order the helper returns alongside is
    the one those tokens name: position ids handed out in first-visit order, -1 for the nodes the walk never reached - at most the
    last visit's id fell behind the cut"""
    d = random_multigraphs(300, 11)
    coo = orc.Coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], d["x"] if labeled else None, d["edge_attr"] if labeled else None)
    kw = dict(labeled=True, num_node_types=9, num_edge_types=5) if labeled else {}
    ids, ln = orc.sent(coo, 13, max_len, 77, epoch=3, graph_base=1000, ld=max_len, **kw)
    toks, vis = wref.walk_batch(orc, d["node_counts"], d["edge_counts"], d["src"], d["dst"], max_len, 77, epoch=3, graph_base=1000,
                                labeled=labeled, x=d["x"], edge_attr=d["edge_attr"], max_num_nodes=13, num_node_types=9 if labeled else 0)
    nptr = np.concatenate([[0], np.cumsum(d["node_counts"])])
    cut = 0
    for g, t in enumerate(toks):
        assert t.size == ln[g] and np.array_equal(t, ids[g, :ln[g]]), g
        v = vis[nptr[g]:nptr[g + 1]]
        seen = np.sort(v[v >= 0])
        assert np.array_equal(seen, np.arange(seen.size)), g                       # a prefix of 0, 1, 2, ... handed out once each
        if t[-1] == wref.EOS and ln[g] < max_len:
            assert seen.size == v.size, g                                          # a complete row visits every node
        else:
            cut += 1
        named = t[(t >= 6) & (t < 6 + 13)] - 6                                     # the position ids the row holds
        assert named.size == 0 or named.max() <= seen.size - 1, g
        assert seen.size - (named.max() + 1 if named.size else 0) <= 1, g          # at most the last visit's id fell behind the cut
    assert cut == 0 if max_len == 4096 else cut > 100            # (17 tokens cut most of these rows: graphs of up to 13 nodes)


def _batch_arrays(d, labeled=True):
    b = gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], d["x"] if labeled else None,
                                 d["edge_attr"] if labeled else None, check_symmetric=False)
    h = lambda t: None if t is None else t.numpy()
    return b, (h(b.node_ptr), h(b.edge_ptr), h(b.rowptr), h(b.col), h(b.nattr), h(b.eattr), b.max_nodes, b.max_edges)


def test_the_relabel_reference_on_graphs_whose_answer_is_known():
    d = random_multigraphs(40, 5)
    b, arrays = _batch_arrays(d)
    N = int(b.node_ptr[-1])
    nptr = b.node_ptr.numpy()
    ident = (np.arange(N) - np.repeat(nptr[:-1], np.diff(nptr))).astype(np.int32)
    o = rref.relabel(*arrays, ident)
    assert (o["status"] != 1).all() and o["info"][0] == 0
    assert np.array_equal(o["rowptr"], b.rowptr.numpy()) and np.array_equal(o["nattr"], b.nattr.numpy())
    ep = b.edge_ptr.numpy()
    for g in range(b.num_graphs):                        # the canonical form: every row in ascending column, duplicates in input order
        rp = o["rowptr"][nptr[g] + g:nptr[g + 1] + g + 1]
        c, eo = o["col"][ep[g]:ep[g + 1]], o["eorder"][ep[g]:ep[g + 1]]
        assert np.array_equal(b.col.numpy()[ep[g]:ep[g + 1]][eo], c)
        for u in range(rp.size - 1):
            row, pos = c[rp[u]:rp[u + 1]], eo[rp[u]:rp[u + 1]]
            assert (np.diff(row) >= 0).all() and (np.diff(pos)[np.diff(row) == 0] > 0).all()
    # a permutation and its inverse give the canonical form back
    rng = np.random.default_rng(2)
    perm = np.concatenate([rng.permutation(n) for n in np.diff(nptr)]).astype(np.int32)        # old id of new node t
    p1 = rref.relabel(*arrays, perm)
    inv = np.empty_like(perm)
    for g in range(b.num_graphs):
        s = slice(nptr[g], nptr[g + 1])
        inv[s][perm[s]] = np.arange(nptr[g + 1] - nptr[g])
    back = rref.relabel(nptr, ep, p1["rowptr"], p1["col"], p1["nattr"], p1["eattr"], b.max_nodes, b.max_edges, inv)
    for k in ("rowptr", "col", "nattr", "eattr", "status"):
        assert np.array_equal(back[k], o[k]), k
    assert np.array_equal(o["info"][1:6], [b.max_degree, b.max_nodes, b.max_edges, b.chunk_nodes, b.chunk_edges])
    bad = perm.copy(); bad[nptr[3]] = bad[nptr[3] + 1] if nptr[4] - nptr[3] > 1 else -1
    assert rref.relabel(*arrays, bad)["status"][3] == (1 if nptr[4] - nptr[3] > 0 else 0)


def test_the_entry_points_are_bound_by_symbol_with_their_arity():
    L = _lib.lib()
    for n in NAMES:
        assert n in _lib.SYMBOLS and hasattr(L, n), n
    assert len(L.gtok_sent_large_order.argtypes) == 10 and len(L.gtok_csr_relabel.argtypes) == 9 and len(L.gtok_csr_relabel_workspace.argtypes) == 2
    assert L.gtok_csr_relabel.argtypes[4] == ctypes.POINTER(_lib.GtokCsrBuilt) and L.gtok_csr_relabel_workspace.restype == ctypes.c_int64
    assert set(_lib.ORDER_SYMBOLS) == set(NAMES) and not set(NAMES) & set(_lib.OPTIONAL_SYMBOLS)
    assert _lib.ABI_VERSION == 8 and L.gtok_version() == 8                      # no ABI version step
    assert "gtok_csr_relabel.hip" in [s.rsplit("/", 1)[-1] for s in _lib.SOURCES]


def test_workspace_arithmetic():
    W = _lib.lib().gtok_csr_relabel_workspace
    assert W(0, 0) == 0 and W(1, 0) == 16 and W(64, 10 ** 9) == 16 and W(65, 0) == 32
    assert all(W(g, 7) % 16 == 0 for g in (0, 1, 63, 64, 65, 4096, 32768))
    assert W(-1, 0) == -1 and W(4, -1) == -1


def test_host_side_argument_errors_come_before_any_device_is_asked_for():
    L = _lib.lib()
    buf = (ctypes.c_int32 * 256)()
    base = ctypes.addressof(buf)
    p = (base + 15) // 16 * 16                                               # a 16-byte aligned address inside buf
    cs = lambda **kw: _lib.GtokCsr(**{**dict(num_graphs=2, max_nodes=8, max_edges=16, node_ptr=p, edge_ptr=p, rowptr=p, col=p), **kw})
    sp = lambda **kw: _lib.GtokSentParams(**{**dict(max_num_nodes=8, max_len=64, pad_id=5, epoch_count=1), **kw})
    need = L.gtok_sent_large_workspace(8, 16, 2)
    order = lambda g, q, ids=p, ld=32, ln=p, vis=p, stride=16, ws=p, wb=None: L.gtok_sent_large_order(
        ctypes.byref(g), ctypes.byref(q), ids, ld, ln, vis, stride, ws, need if wb is None else wb, None)
    assert order(cs(), sp(), ids=None) == -1 and order(cs(), sp(), ln=None) == -1          # one of the two outputs NULL
    assert order(cs(), sp(), vis=None) == -1 and order(cs(), sp(), stride=-1) == -1
    assert order(cs(), sp(), ld=0) == -1                                                   # rows asked for: ld counts
    assert order(cs(), sp(), ids=None, ln=None, ld=0, ws=None) == -1                       # order only: ld is ignored, the workspace is not
    assert order(cs(), sp(), ws=p + 4) == -1 and order(cs(), sp(), wb=need - 1) == -1
    assert order(cs(graph_ids=p), sp()) == -1 and order(cs(unit_ptr=p), sp()) == -1        # dataset order only
    assert order(cs(), sp(labeled=1)) == -1                                                # labelled without attributes
    assert order(cs(), sp(flags=4)) == -1 and order(cs(), sp(max_len=-1)) == -1
    assert order(cs(max_nodes=_lib.SENT_LARGE_MAX_NODES + 1), sp()) == -2
    assert order(cs(num_graphs=0), sp()) == 0                                              # an empty batch: a no-op
    assert L.gtok_sent_large_order(None, ctypes.byref(sp()), p, 32, p, p, 16, p, need, None) == -1

    out = lambda **kw: _lib.GtokCsrBuilt(**{**dict(rowptr=p, col=p, eorder=p, info=p), **kw})
    rel = lambda g, t=p, tmax=8, m=p, o=None, st=p, ws=p, wb=16: L.gtok_csr_relabel(ctypes.byref(g), t, tmax, m, ctypes.byref(o or out()), st, ws, wb, None)
    assert rel(cs(), m=None) == -1 and rel(cs(), st=None) == -1 and rel(cs(), ws=None) == -1
    assert rel(cs(), ws=p + 8) == -1 and rel(cs(), wb=15) == -1 and rel(cs(), tmax=-1) == -1
    assert rel(cs(graph_ids=p)) == -1 and rel(cs(unit_ptr=p)) == -1
    assert rel(cs(rowptr=None)) == -1 and rel(cs(), o=out(col=None)) == -1 and rel(cs(), o=out(info=None)) == -1
    assert rel(cs(nattr=p)) == -1 and rel(cs(eattr=p)) == -1                               # attributes in, nowhere to put them
    assert rel(cs(), tmax=_lib.SENT_LARGE_MAX_NODES + 1) == -2 and rel(cs(max_nodes=_lib.SENT_LARGE_MAX_NODES + 1)) == -2
    assert rel(cs(num_graphs=0), m=None, st=None, ws=None, wb=0) == 0                      # no graphs: a no-op
    assert L.gtok_csr_relabel(None, p, 8, p, ctypes.byref(out()), p, p, 16, None) == -1
    assert list(buf) == [0] * 256                                                          # nothing was written


def test_torch_ops_are_cuda_only_and_their_meta_kernels_give_the_documented_shapes():
    assert hasattr(torch.ops.gtok, "sent_order") and hasattr(torch.ops.gtok, "csr_relabel")
    G, N, E, T = 5, 40, 90, 55
    node_ptr, edge_ptr = torch.zeros(G + 1, dtype=torch.int32), torch.zeros(G + 1, dtype=torch.int64)
    rowptr, col = torch.zeros(N + G, dtype=torch.int32), torch.zeros(E, dtype=torch.int32)
    nattr, eattr = torch.zeros(N, dtype=torch.uint8), torch.zeros(E, dtype=torch.uint8)
    oon, tptr = torch.zeros(T, dtype=torch.int32), torch.zeros(G + 1, dtype=torch.int32)
    with pytest.raises((NotImplementedError, RuntimeError)):        # no CPU kernel exists
        torch.ops.gtok.csr_relabel(node_ptr, edge_ptr, rowptr, col, None, None, 8, 18, oon, tptr, 11)
    m = lambda t: None if t is None else t.to("meta")
    for epochs in (0, 1, 3):
        v = torch.ops.gtok.sent_order(m(node_ptr), m(edge_ptr), m(rowptr), m(col), None, None, 8, 18, N, 8, 64, 1, 0, epochs, False, 0, 0)
        assert tuple(v.shape) == (max(1, epochs), N) and v.dtype == torch.int32
    for na, ea in ((None, None), (nattr, eattr)):
        out = torch.ops.gtok.csr_relabel(m(node_ptr), m(edge_ptr), m(rowptr), m(col), m(na), m(ea), 8, 18, m(oon), m(tptr), 11)
        want = [(T + G,), (E,), (E,), (T,) if na is not None else (0,), (E,) if ea is not None else (0,), (8,), (G,)]
        assert [tuple(t.shape) for t in out] == want
        assert [t.dtype for t in out] == [torch.int32] * 3 + [torch.uint8] * 2 + [torch.int32] * 2


def test_python_layer_and_the_tokenizer():
    assert list(inspect.signature(gtok.ops.sent_order).parameters)[:8] == ["batch", "max_len", "seed", "epoch", "epochs", "graph_base", "with_rows",
                                                                          "max_num_nodes"]
    assert list(inspect.signature(gtok.ops.csr_relabel).parameters) == ["batch", "old_of_new", "target_node_ptr", "target_max_nodes"]
    assert list(inspect.signature(gtok.ops.graphs_equal).parameters) == ["a", "b"]
    d = random_multigraphs(4, 1)
    b, _ = _batch_arrays(d)
    with pytest.raises(gtok.GtokError):               # host batches: refused, never walked or renumbered on the CPU
        gtok.ops.sent_order(b, 64, 1)
    with pytest.raises(gtok.GtokError):
        gtok.ops.csr_relabel(b, torch.zeros(int(b.node_ptr[-1]), dtype=torch.int32))
    Tok = gtok.autograph.datamodules.data.tokenizer.Graph2TrailTokenizer
    assert list(inspect.signature(Tok.visit_order).parameters) == ["self", "batch", "epoch", "epochs", "graph_base"]
    assert list(inspect.signature(Tok.decode_batch_like).parameters) == ["self", "ids", "ln", "like", "order", "row_start", "check_symmetric"]
    assert list(inspect.signature(Tok.decode_batch).parameters) == ["self", "ids", "ln", "row_start", "check_symmetric"]      # as before
    # graphs_equal is plain torch: it runs wherever the batches live
    same = gtok.ops.graphs_equal(b, b)
    assert same.dtype == torch.bool and bool(same.all())
    d2 = {k: v.copy() for k, v in d.items()}
    g = int(np.nonzero(d["edge_counts"] > 0)[0][0])
    e0 = int(np.cumsum(d["edge_counts"])[g] - 1)
    d2["edge_attr"][e0] = (d2["edge_attr"][e0] + 1) % 5
    b2, _ = _batch_arrays(d2)
    assert gtok.ops.graphs_equal(b, b2).tolist() == [i != g for i in range(4)]
