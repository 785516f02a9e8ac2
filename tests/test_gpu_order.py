"""gtok_sent_large_order / gtok_csr_relabel (include/gtok.h) on the device: the visit order against the Python walk of
tests/_sent_walk_ref.py (pinned to the C oracle by tests/test_host_order.py), the renumbering against tests/_relabel_ref.py, and
the route they close: rows of any SENT kernel -> sent_decode_csr -> csr_relabel -> graphs_equal(the input)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _relabel_ref as rref
import _sent_walk_ref as wref
from _util import both, edge_case_graphs, gtok, orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_lib = gtok._lib
MAXN = _lib.SENT_LARGE_MAX_NODES
Tokenizer = gtok.autograph.datamodules.data.tokenizer.Graph2TrailTokenizer
GUARD = 16


# ------------------------------------------------------------------------------------------------ batches
def _ring_pairs(n, chords, rng):
    pairs = {(min(i, (i + 1) % n), max(i, (i + 1) % n)) for i in range(n)}
    while len(pairs) < n + chords:
        a, b = sorted(rng.integers(0, n, 2).tolist())
        if a != b:
            pairs.add((a, b))
    return np.array(sorted(pairs), np.int64)


def _both_ways(pairs):
    s, t = np.concatenate([pairs[:, 0], pairs[:, 1]]), np.concatenate([pairs[:, 1], pairs[:, 0]])
    o = np.lexsort((t, s))
    return s[o], t[o]


def _from_lists(sizes, lists):
    return dict(node_counts=np.asarray(sizes, np.int64), edge_counts=np.asarray([s.size for s, _ in lists], np.int64),
                src=np.concatenate([s for s, _ in lists]).astype(np.int64), dst=np.concatenate([t for _, t in lists]).astype(np.int64))


@functools.lru_cache(maxsize=None)
def _corpus(name):
    """-> (dict in COO form, labelled?, max_num_nodes, a max_len that cuts most rows)"""
    if name == "molecules":
        return gtok.synth.zinc_like(300, seed=21), True, 37, 50
    if name == "graph_token":                       # every edge listed once, unlabelled
        d = gtok.synth.graph_token_like(198, seed=7, task=None, with_text=False)
        return {k: d[k] for k in ("node_counts", "edge_counts", "src", "dst")}, False, 49, 40
    if name == "hand_made":                         # empty graph, one node, isolated nodes, self loops, two components, duplicates
        return edge_case_graphs(), True, 8, 9
    assert name == "large"
    rng = np.random.default_rng(3)
    star = np.stack([np.zeros(512, np.int64), np.arange(1, 513)], 1)
    path = np.stack([np.arange(16383), np.arange(1, 16384)], 1)
    lists = [_both_ways(_ring_pairs(65, 40, rng)), (star[:, 0], star[:, 1]), _both_ways(_ring_pairs(4097, 300, rng)), _both_ways(path)]
    return _from_lists([65, 513, 4097, 16384], lists), False, MAXN, 1000


def _kw(labeled):
    return dict(labeled=True, num_node_types=28, num_edge_types=6) if labeled else dict(labeled=False)


def _host_batch(d, labeled):
    return gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], d.get("x") if labeled else None,
                                    d.get("edge_attr") if labeled else None, check_symmetric=False)


@functools.lru_cache(maxsize=None)
def _expected_order(name, max_len, epoch, graph_base):
    d, labeled, mnn, _ = _corpus(name)
    _, vis = wref.walk_batch(orc, d["node_counts"], d["edge_counts"], d["src"], d["dst"], max_len, 5, epoch=epoch, graph_base=graph_base,
                             labeled=labeled, x=d.get("x"), edge_attr=d.get("edge_attr"), max_num_nodes=mnn, num_node_types=28 if labeled else 0)
    vis.setflags(write=False)
    return vis


def _order_call(batch, p, rows, ld, u16, K, stride, fill=-99):
    """gtok_sent_large_order through the binding with a visit_index block of `stride` elements per epoch, pre-filled with `fill`"""
    dev = batch.device
    G = batch.num_graphs
    vis = torch.full((K, stride), fill, dtype=torch.int32, device=dev)
    ids = torch.full((K * G, ld), -3, dtype=torch.int16 if u16 else torch.int32, device=dev) if rows else None
    ln = torch.full((K * G,), -3, dtype=torch.int32, device=dev) if rows else None
    need = int(_lib.lib().gtok_sent_large_workspace(batch.max_nodes, batch.max_edges, G * K))
    ws = torch.empty(max(16, need), dtype=torch.uint8, device=dev)
    cs = batch.c_struct()
    rc = _lib.lib().gtok_sent_large_order(ctypes.byref(cs), ctypes.byref(p), None if ids is None else ids.data_ptr(), ld,
                                          None if ln is None else ln.data_ptr(), vis.data_ptr(), stride, ws.data_ptr(), ws.numel(),
                                          ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return vis, ids, ln


# ------------------------------------------------------------------------------------------------ 1. the visit order
@pytest.mark.parametrize("name", ["molecules", "graph_token", "hand_made", "large"])
def test_visit_index_equals_the_reference_walk(name):
    d, labeled, mnn, cut_len = _corpus(name)
    batch = _host_batch(d, labeled).to(DEV)
    N, G = batch.num_nodes_total, batch.num_graphs
    kw = _kw(labeled)
    for max_len, epoch, epochs, base in ((1 << 20, 0, 1, 0), (1 << 20, 2, 3, 1000), (cut_len, 1, 1, 7)):
        what = f"{name} max_len={max_len} epoch={epoch} epochs={epochs} graph_base={base}"
        want = np.stack([_expected_order(name, max_len, epoch + e, base) for e in range(epochs)])
        ld = gtok.ops.sent_safe_ld(batch, labeled, max_len)
        vis, ids, ln = gtok.ops.sent_order(batch, max_len, 5, epoch, epochs=epochs, graph_base=base, with_rows=True, max_num_nodes=mnn, ld=ld, **kw)
        got = vis.cpu().numpy()
        assert got.shape == (epochs, N) and got.dtype == np.int32
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{what}: visit_index differs at {bad[:6].tolist()}: {got[got != want][:6]} vs {want[got != want][:6]}"
        if max_len == cut_len:
            cut_rows = (ln.cpu().numpy().reshape(-1) >= max_len).mean()
            assert cut_rows > 0.5 and (want == -1).any(), (what, cut_rows)
        else:
            assert (want >= 0).all()
        # the rows of the same launch are gtok_sent_large's, bit for bit - int32 and 16-bit
        ref_ids, ref_ln = gtok.ops.sent_large(batch, mnn, max_len, 5, epoch, epochs=epochs, graph_base=base, ld=ld, **kw)
        assert torch.equal(ids, ref_ids) and torch.equal(ln, ref_ln), what
        if mnn + 28 + 512 + 6 <= 65535:
            v16, i16, l16 = gtok.ops.sent_order(batch, max_len, 5, epoch, epochs=epochs, graph_base=base, with_rows=True, max_num_nodes=mnn, ld=ld,
                                                u16=True, **kw)
            r16, rl16 = gtok.ops.sent_large(batch, mnn, max_len, 5, epoch, epochs=epochs, graph_base=base, ld=ld, u16=True, **kw)
            assert i16.dtype == torch.int16 and torch.equal(i16, r16) and torch.equal(l16, rl16) and torch.equal(v16, vis), what
        # order only: the same index, nothing else written
        only = gtok.ops.sent_order(batch, max_len, 5, epoch, epochs=epochs, graph_base=base, max_num_nodes=mnn, **kw)
        assert torch.equal(only, vis), what
        # a stride beyond the node total: the gap keeps its guard values, with rows and without
        p = gtok.ops._sent_params(mnn, max_len, labeled, kw.get("num_node_types", 0), kw.get("num_edge_types", 0), False, 5, 0, 5, epoch, base, None, epochs)
        for rows in (True, False):
            wide, wi, wl = _order_call(batch, p, rows, ld, False, epochs, N + 37)
            assert torch.equal(wide[:, :N], vis) and bool((wide[:, N:] == -99).all()), (what, rows)
            if rows:
                assert torch.equal(wi.view_as(ids), ids) and torch.equal(wl.view_as(ln), ln), what


# ------------------------------------------------------------------------------------------------ 2. the fast kernels' rows
def _tiled(batch, K):
    """K copies of a device batch, one after another (what K epochs of it decode to)"""
    counts = lambda ptr: (ptr[1:] - ptr[:-1]).repeat(K)
    node_ptr = torch.zeros(K * batch.num_graphs + 1, dtype=torch.int32, device=batch.device)
    torch.cumsum(counts(batch.node_ptr), 0, dtype=torch.int32, out=node_ptr[1:])
    edge_ptr = torch.zeros(K * batch.num_graphs + 1, dtype=torch.int64, device=batch.device)
    torch.cumsum(counts(batch.edge_ptr), 0, out=edge_ptr[1:])
    rep = lambda t: None if t is None else t.repeat(K)
    return gtok.GraphBatch(K * batch.num_graphs, batch.max_nodes, batch.max_edges, node_ptr, edge_ptr, rep(batch.rowptr), rep(batch.col), None,
                           rep(batch.nattr), rep(batch.eattr))


def test_the_order_pairs_with_the_rows_of_the_lane_kernel():
    """4,096 molecules x 8 epochs through ops.sent: 32,768 walks, every decoded and renumbered graph equals its input"""
    K = 8
    d = gtok.synth.zinc_like(4096, seed=9)
    batch, _ = both(d)
    dev = batch.to(DEV)
    kw = dict(labeled=True, num_node_types=28, num_edge_types=4)
    ids, ln = gtok.ops.sent(dev, 37, 4096, 11, 3, epochs=K, graph_base=50, **kw)
    kernel = gtok.ops.last_sent_kernel()
    dec, st = gtok.ops.sent_decode_csr(ids.view(K * 4096, -1), ln.view(-1), 37, True, 28)
    assert int((st != 0).sum()) == 0
    vis = gtok.ops.sent_order(dev, 4096, 11, 3, epochs=K, graph_base=50, max_num_nodes=37, **kw)
    want = _tiled(dev, K)
    out, rst = gtok.ops.csr_relabel(dec, vis.view(-1), want.node_ptr, dev.max_nodes)
    assert int((rst != 0).sum()) == 0
    same = gtok.ops.graphs_equal(out, want)
    assert tuple(same.shape) == (K * 4096,) and bool(same.all()), f"{int((~same).sum())} of {K * 4096} rows of {kernel} do not decode to their input"
    # (the input is its own canonical form: coalesced molecules list every row in ascending column)
    ident, ist = gtok.ops.csr_relabel(dev, (torch.arange(dev.num_nodes_total, device=DEV) - torch.repeat_interleave(
        dev.node_ptr[:-1].to(torch.int64), dev.node_counts().to(torch.int64))).to(torch.int32))
    assert bool(gtok.ops.graphs_equal(ident, dev).all()) and int(ist.sum()) == 0
    assert "sent_lane_kernel" in kernel, f"ops.sent ran {kernel} for 32,768 walks (the round trip above passed on its rows)"


# ------------------------------------------------------------------------------------------------ 3. csr_relabel against the reference
def _guarded(n, dtype, fill):
    t = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return t, t[GUARD:GUARD + n]


def _run_relabel(arrays, oon, tptr, tmax):
    """gtok_csr_relabel through the binding, every output between guard words -> (dict of host arrays, guards intact?)"""
    node_ptr, edge_ptr, rowptr, col, nattr, eattr, maxn, maxe = arrays
    G, T, E = node_ptr.size - 1, int(tptr[-1]), int(edge_ptr[-1])
    up = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)
    pad = lambda t: t if t is None or t.numel() else torch.zeros(1, dtype=t.dtype, device=DEV)      # (an empty tensor has no address)
    b = gtok.GraphBatch(G, maxn, maxe, up(node_ptr, torch.int32), up(edge_ptr, torch.int64), pad(up(rowptr, torch.int32)), pad(up(col, torch.int32)),
                        None, pad(up(nattr, torch.uint8)), pad(up(eattr, torch.uint8)))
    shapes = dict(rowptr=(T + G, torch.int32, -7), col=(E, torch.int32, -7), eorder=(E, torch.int32, -7), info=(8, torch.int32, -7), status=(G, torch.int32, -7))
    if nattr is not None:
        shapes["nattr"] = (T, torch.uint8, 249)
    if eattr is not None:
        shapes["eattr"] = (E, torch.uint8, 249)
    full, view = {}, {}
    for k, (n, dt, fill) in shapes.items():
        full[k], view[k] = _guarded(n, dt, fill)
    ptr = lambda k: view[k].data_ptr() if k in view else None
    cout = _lib.GtokCsrBuilt(None, None, ptr("rowptr"), ptr("col"), ptr("eorder"), ptr("nattr"), ptr("eattr"), ptr("info"))
    need = int(_lib.lib().gtok_csr_relabel_workspace(G, E))
    ws_t = torch.empty(max(16, need) + 16, dtype=torch.uint8, device=DEV)
    off = (-ws_t.data_ptr()) % 16
    t_oon, t_ptr = pad(up(oon, torch.int32)), up(tptr, torch.int32)
    cs = b.c_struct()
    rc = _lib.lib().gtok_csr_relabel(ctypes.byref(cs), t_ptr.data_ptr(), int(tmax), t_oon.data_ptr(), ctypes.byref(cout), view["status"].data_ptr(),
                                     ws_t.data_ptr() + off, need, ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    intact = all(bool((full[k][:GUARD] == fill).all()) and bool((full[k][GUARD + n:] == fill).all()) for k, (n, dt, fill) in shapes.items())
    return {k: v.cpu().numpy() for k, v in view.items()}, intact


def _arrays(d, labeled):
    b = _host_batch(d, labeled)
    h = lambda t: None if t is None else t.numpy().copy()
    return [h(b.node_ptr), h(b.edge_ptr), h(b.rowptr), h(b.col), h(b.nattr), h(b.eattr), b.max_nodes, b.max_edges]


def _multigraphs(count, seed, max_n, max_e, min_n=0):
    rng = np.random.default_rng(seed)
    nc = rng.integers(min_n, max_n + 1, count)
    ec = np.where(nc > 0, rng.integers(0, max_e + 1, count), 0)
    draw = lambda: np.concatenate([rng.integers(0, max(n, 1), e) for n, e in zip(nc, ec)]).astype(np.int64)
    src, dst = draw(), draw()
    return dict(node_counts=nc, edge_counts=ec, src=src, dst=dst, x=rng.integers(0, 256, int(nc.sum())), edge_attr=rng.integers(0, 256, int(ec.sum())))


def _perms(node_ptr, rng):
    return np.concatenate([rng.permutation(n) for n in np.diff(node_ptr)] + [np.zeros(0, np.int64)]).astype(np.int32)


def _identity(node_ptr):
    return (np.arange(node_ptr[-1]) - np.repeat(node_ptr[:-1], np.diff(node_ptr))).astype(np.int32)


def _case(name):
    """-> (arrays, old_of_new, target node_ptr, target_max_nodes, statuses that must occur)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name in ("attrs", "no_attrs", "non_injective", "old_gt_target", "col_out_of_range", "bad_rowptr"):
        a = _arrays(_multigraphs(150, 4, 40, 120, min_n=1 if name != "attrs" else 0), name != "no_attrs")
        nptr = a[0].astype(np.int64)
        oon, tptr = _perms(nptr, rng), nptr.copy()
        hit = [g for g in range(150) if nptr[g + 1] - nptr[g] >= 3 and a[1][g + 1] > a[1][g]][::7]
        if name == "non_injective":
            for g in hit:
                oon[nptr[g]] = oon[nptr[g] + 1]
        if name == "old_gt_target":                 # the target has one node fewer than the old graph in some graphs
            keep = np.ones(oon.size, bool)
            keep[[nptr[g] for g in hit]] = False
            tcounts = np.diff(nptr); tcounts[hit] -= 1
            oon, tptr = oon[keep], np.concatenate([[0], np.cumsum(tcounts)])
        if name == "col_out_of_range":
            for i, g in enumerate(hit):
                a[3][a[1][g]] = (nptr[g + 1] - nptr[g]) if i % 2 else -1
        if name == "bad_rowptr":
            for i, g in enumerate(hit):
                rp = a[2][nptr[g] + g:nptr[g + 1] + g + 1]
                if i % 3 == 0:
                    rp[1], rp[2] = max(rp[1], rp[2]) + 1, min(rp[1], rp[2])          # decreasing
                elif i % 3 == 1:
                    rp[-1] += 1                                                      # does not end at E_g
                else:
                    rp[0] = 1 if rp[1] >= 1 else -1                                  # does not start at 0
        must = {0, 2} if name in ("attrs", "no_attrs") else {0, 1, 2}
        return a, oon, tptr, int(np.diff(tptr).max()), must
    if name == "empty_graphs":                      # every third graph has no node, others no entry
        r = np.random.default_rng(8)
        nc = r.integers(0, 6, 70); nc[::3] = 0
        ec = np.where(nc > 0, r.integers(0, 10, 70), 0)
        draw = lambda: np.concatenate([r.integers(0, max(n, 1), e) for n, e in zip(nc, ec)]).astype(np.int64)
        d = dict(node_counts=nc, edge_counts=ec, src=draw(), dst=draw(), x=r.integers(0, 9, int(nc.sum())), edge_attr=r.integers(0, 5, int(ec.sum())))
        a = _arrays(d, True)
        return a, _perms(a[0].astype(np.int64), rng), a[0].astype(np.int64), 5, {0, 2}
    if name == "absent_targets":                    # N_t > N_old: extra target nodes with -1 / out-of-range entries, anywhere in the graph
        a = _arrays(_multigraphs(120, 9, 30, 80), True)
        nptr = a[0].astype(np.int64)
        extra = rng.integers(0, 6, 120)
        parts = []
        for g in range(120):
            n = int(nptr[g + 1] - nptr[g])
            m = np.concatenate([rng.permutation(n), rng.choice([-1, n, n + 5, -2 ** 31, 2 ** 31 - 1], int(extra[g]))])
            parts.append(m[rng.permutation(m.size)])
        tptr = np.concatenate([[0], np.cumsum(np.diff(nptr) + extra)])
        return a, np.concatenate(parts).astype(np.int32), tptr, int(np.diff(tptr).max()), {0, 2}
    if name == "identity_unsorted":                 # rows in random column order: the identity map gives the canonical form
        d = _multigraphs(100, 12, 25, 90)
        a = _arrays(d, True)
        return a, _identity(a[0].astype(np.int64)), a[0].astype(np.int64), 25, {0, 2}
    if name == "long_rows":                         # rows of more than 64 entries full of duplicates: the stable count
        r = np.random.default_rng(13)
        nc, ec = r.integers(2, 7, 12), r.integers(300, 700, 12)
        draw = lambda: np.concatenate([r.integers(0, n, e) for n, e in zip(nc, ec)]).astype(np.int64)
        a = _arrays(dict(node_counts=nc, edge_counts=ec, src=draw(), dst=draw(), x=r.integers(0, 256, int(nc.sum())), edge_attr=r.integers(0, 256, int(ec.sum()))), True)
        return a, _perms(a[0].astype(np.int64), rng), a[0].astype(np.int64), 6, {2}
    if name == "star_16384":
        leaves = np.arange(1, MAXN)
        s, t = np.concatenate([np.zeros(MAXN - 1, np.int64), leaves]), np.concatenate([leaves, np.zeros(MAXN - 1, np.int64)])
        d = dict(node_counts=np.array([MAXN]), edge_counts=np.array([s.size]), src=s, dst=t, x=rng.integers(0, 200, MAXN), edge_attr=rng.integers(0, 200, s.size))
        a = _arrays(d, True)
        return a, _perms(a[0].astype(np.int64), rng), a[0].astype(np.int64), MAXN, {0}
    assert name == "complete_512"                   # + a complete graph on 100 nodes with self loops: long rows, no duplicate, status 2
    iu = np.array([(i, j) for i in range(512) for j in range(512) if i != j], np.int64)
    il = np.array([(i, j) for i in range(100) for j in range(100)], np.int64)
    d = dict(node_counts=np.array([512, 100]), edge_counts=np.array([iu.shape[0], il.shape[0]]), src=np.concatenate([iu[:, 0], il[:, 0]]),
             dst=np.concatenate([iu[:, 1], il[:, 1]]), x=rng.integers(0, 9, 612), edge_attr=rng.integers(0, 250, iu.shape[0] + il.shape[0]))
    a = _arrays(d, True)
    return a, _perms(a[0].astype(np.int64), rng), a[0].astype(np.int64), 512, {0, 2}


CASES = ["attrs", "no_attrs", "empty_graphs", "absent_targets", "identity_unsorted", "non_injective", "old_gt_target", "col_out_of_range",
         "bad_rowptr", "long_rows", "star_16384", "complete_512"]


@pytest.mark.parametrize("name", CASES)
def test_csr_relabel_equals_the_reference(name):
    a, oon, tptr, tmax, must = _case(name)
    if name == "identity_unsorted":                 # shuffle every row's entries (and their types with them)
        rng = np.random.default_rng(1)
        nptr, ep = a[0].astype(np.int64), a[1]
        for g in range(nptr.size - 1):
            rp = a[2][nptr[g] + g:nptr[g + 1] + g + 1]
            for u in range(rp.size - 1):
                o = rng.permutation(rp[u + 1] - rp[u]) + ep[g] + rp[u]
                a[3][ep[g] + rp[u]:ep[g] + rp[u + 1]] = a[3][o]
                a[5][ep[g] + rp[u]:ep[g] + rp[u + 1]] = a[5][o]
    want = rref.relabel(*a, oon, tptr, tmax)
    got, intact = _run_relabel(a, oon, tptr, tmax)
    assert intact, f"{name}: a guard word around an output array was overwritten"
    assert np.array_equal(got["status"], want["status"]), (name, np.nonzero(got["status"] != want["status"])[0][:8])
    assert set(want["status"].tolist()) == must, (name, set(want["status"].tolist()))
    assert np.array_equal(got["info"], want["info"]), (name, got["info"], want["info"])
    node_ptr, edge_ptr = a[0].astype(np.int64), a[1]
    for g in np.nonzero(want["status"] != 1)[0]:
        for k, lo, hi in (("rowptr", tptr[g] + g, tptr[g + 1] + g + 1), ("col", edge_ptr[g], edge_ptr[g + 1]), ("eorder", edge_ptr[g], edge_ptr[g + 1]),
                          ("nattr", tptr[g], tptr[g + 1]), ("eattr", edge_ptr[g], edge_ptr[g + 1])):
            if want[k] is None:
                assert k not in got
                continue
            x, y = got[k][lo:hi], want[k][lo:hi]
            assert np.array_equal(x, y), f"{name}: graph {g} {k} differs at {np.nonzero(x != y)[0][:6]}: {x[x != y][:6]} vs {y[x != y][:6]}"


def test_csr_relabel_python_layer_carries_info():
    a, oon, tptr, tmax, _ = _case("absent_targets")
    d = _multigraphs(120, 9, 30, 80)
    dev = _host_batch(d, True).to(DEV)
    out, st = gtok.ops.csr_relabel(dev, torch.from_numpy(oon), torch.from_numpy(tptr.astype(np.int32)))
    want = rref.relabel(*a, oon, tptr, tmax)
    assert np.array_equal(st.cpu().numpy(), want["status"])
    assert [out.max_degree, out.max_nodes, out.max_edges, out.chunk_nodes, out.chunk_edges] == want["info"][1:6].tolist()
    assert out.num_graphs == 120 and out.num_nodes_total == int(tptr[-1]) and out.eorder is not None
    assert np.array_equal(out.col.cpu().numpy(), want["col"]) and np.array_equal(out.nattr.cpu().numpy(), want["nattr"])


# ------------------------------------------------------------------------------------------------ 4. cut rows
def test_round_trip_of_cut_rows():
    """max_len 40 cuts most molecules: what decode_batch_like(like=, order=) returns is a part of the input - every entry an entry of the
    input with its type, none twice; the input's node types for decoded nodes, 255 for the rest"""
    d = gtok.synth.zinc_like(300, seed=33)
    batch, _ = both(d)
    dev = batch.to(DEV)
    tok = Tokenizer(max_length=40, labeled_graph=True, seed=17, device=DEV)
    tok.set_num_nodes(37); tok.set_num_node_and_edge_types(28, 4)
    K = 2
    ids, ln = tok.tokenize_batch(dev, epoch=4, graph_base=9, epochs=K)
    order = tok.visit_order(dev, epoch=4, epochs=K, graph_base=9)
    out, st = tok.decode_batch_like(ids.view(K * 300, -1), ln.view(-1), like=dev, order=order)
    raw, _ = tok.decode_batch(ids.view(K * 300, -1), ln.view(-1))
    st = st.cpu().numpy()
    assert (st == 3).mean() > 0.5 and not (st == 1).any()
    assert out.num_graphs == K * 300 and torch.equal(out.node_ptr.cpu(), torch.cat([batch.node_ptr[:-1], batch.node_ptr + batch.node_ptr[-1]]))
    h = lambda t: t.cpu().numpy()
    nptr, eptr, rowptr, col, na, ea = h(out.node_ptr), h(out.edge_ptr), h(out.rowptr), h(out.col), h(out.nattr), h(out.eattr)
    decoded = np.diff(h(raw.node_ptr))
    order_h = h(order)
    inp = {}
    bn, be, brp, bc, bna, bea = h(batch.node_ptr), h(batch.edge_ptr), h(batch.rowptr), h(batch.col), h(batch.nattr), h(batch.eattr)
    entries = 0
    for r in range(K * 300):
        g, e = r % 300, r // 300
        n = bn[g + 1] - bn[g]
        rp = brp[bn[g] + g:bn[g + 1] + g + 1]
        src = np.repeat(np.arange(n), np.diff(rp))
        types = {(int(s), int(c)): int(t) for s, c, t in zip(src, bc[be[g]:be[g + 1]], bea[be[g]:be[g + 1]])}
        orp = rowptr[nptr[r] + r:nptr[r + 1] + r + 1]
        assert nptr[r + 1] - nptr[r] == n and orp[0] == 0 and orp[-1] == eptr[r + 1] - eptr[r]
        osrc = np.repeat(np.arange(n), np.diff(orp))
        got = list(zip(osrc.tolist(), col[eptr[r]:eptr[r + 1]].tolist()))
        assert len(set(got)) == len(got), r                                                    # never twice
        for (s, c), t in zip(got, ea[eptr[r]:eptr[r + 1]].tolist()):
            assert types.get((s, c)) == t, (r, s, c, t)                                        # an entry of the input, with its type
        entries += len(got)
        k = order_h[e, bn[g]:bn[g + 1]]
        present = (k >= 0) & (k < decoded[r])
        x = na[nptr[r]:nptr[r + 1]]
        assert (x[~present] == 255).all(), r
        typed = present & ~((st[r] == 3) & (k == decoded[r] - 1) & (x == 255))                 # (the last node's type token may be cut)
        assert np.array_equal(x[typed], bna[bn[g]:bn[g + 1]][typed]), r
        assert present.sum() - typed.sum() <= 1
    assert entries > 0


# ------------------------------------------------------------------------------------------------ 5. one-direction input
def test_one_direction_input_decodes_to_its_symmetric_closure():
    d, _, mnn, _ = _corpus("graph_token")
    batch = _host_batch(d, False).to(DEV)
    tok = Tokenizer(max_length=-1, labeled_graph=False, seed=23, device=DEV)
    tok.set_num_nodes(mnn)
    ids, ln = tok.tokenize_batch(batch, epoch=1)
    out, st = tok.decode_batch_like(ids, ln, like=batch, order=tok.visit_order(batch, epoch=1))
    assert int((st != 0).sum()) == 0
    ptr = np.concatenate([[0], np.cumsum(d["edge_counts"])])
    lists = []
    for g in range(len(d["node_counts"])):
        a, b = d["src"][ptr[g]:ptr[g + 1]], d["dst"][ptr[g]:ptr[g + 1]]
        lists.append(_both_ways(np.stack([a, b], 1)))
    closure = _host_batch(_from_lists(d["node_counts"], lists), False).to(DEV)
    same = gtok.ops.graphs_equal(out, closure)
    assert bool(same.all()), f"{int((~same).sum())} graphs differ from the symmetric closure of their input"
    assert not bool(gtok.ops.graphs_equal(out, batch).all())              # ... not from the one-direction lists themselves
