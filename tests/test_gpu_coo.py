"""gtok_csr_from_coo: the batched CSR built on the device from collated COO storage (edge_index + slices), against the host
builder GraphBatch.from_coo and the torch chain of GraphBatch.from_coo_device."""
import ctypes

import numpy as np
import pytest
import torch

from _util import both, edge_case_graphs, gtok, orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ZKW = dict(labeled=True, num_node_types=9, num_edge_types=4, remap_zinc=True)
ARRAYS = ("node_ptr", "edge_ptr", "rowptr", "col", "eorder", "nattr", "eattr")
META = ("num_graphs", "max_nodes", "max_edges", "flags", "chunk_nodes", "chunk_edges", "max_degree")


def _rings_with_chords(sizes, chords, seed):
    """Simple symmetric graphs (ring + random chords), both directions listed, row-sorted, typed."""
    rng = np.random.default_rng(seed)
    ncs, ecs, srcs, dsts = [], [], [], []
    for n in sizes:
        pairs = {(i, (i + 1) % n) if i < (i + 1) % n else ((i + 1) % n, i) for i in range(n)} if n > 2 else set()
        while len(pairs) < min((n if n > 2 else 0) + chords, n * (n - 1) // 2) and n > 3:
            a, b = sorted(rng.integers(0, n, 2).tolist())
            if a != b:
                pairs.add((a, b))
        e = np.array(sorted(pairs), np.int64).reshape(-1, 2)
        s = np.concatenate([e[:, 0], e[:, 1]]); t = np.concatenate([e[:, 1], e[:, 0]])
        o = np.lexsort((t, s))
        ncs.append(n); ecs.append(s.size); srcs.append(s[o]); dsts.append(t[o])
    src, dst = np.concatenate(srcs), np.concatenate(dsts)
    N = int(np.sum(ncs))
    return dict(node_counts=np.array(ncs), edge_counts=np.array(ecs), src=src, dst=dst,
                x=rng.integers(0, 30, N), edge_attr=np.minimum(src, dst) % 7)


def _shuffled(d, seed):
    """The same graphs with every graph's entry list in a random order (not row-sorted)."""
    rng = np.random.default_rng(seed)
    ep = np.concatenate([[0], np.cumsum(d["edge_counts"])])
    perm = np.concatenate([ep[g] + rng.permutation(int(d["edge_counts"][g])) for g in range(len(d["edge_counts"]))]).astype(np.int64)
    out = dict(d)
    out["src"], out["dst"] = d["src"][perm], d["dst"][perm]
    if d.get("edge_attr") is not None:
        out["edge_attr"] = np.asarray(d["edge_attr"])[perm]
    return out


def _slices(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int64)


def _dev(a):
    return None if a is None else torch.as_tensor(np.asarray(a, np.int64)).to(DEV)


def _assert_same(h, g, what=""):
    assert tuple(getattr(g, m) for m in META) == tuple(getattr(h, m) for m in META), (what, [(m, getattr(g, m), getattr(h, m)) for m in META])
    for name in ARRAYS:
        a, b = getattr(h, name), getattr(g, name)
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            assert a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu()), (what, name)


def _build(d, labeled=True, check=True):
    x, ea = (d.get("x"), d.get("edge_attr")) if labeled else (None, None)
    return gtok.ops.csr_from_coo(_dev(d["src"]), _dev(d["dst"]), _dev(_slices(d["node_counts"])), _dev(_slices(d["edge_counts"])),
                                 _dev(x), _dev(ea), check_symmetric=check)


def _host(d, labeled=True):
    x, ea = (d.get("x"), d.get("edge_attr")) if labeled else (None, None)
    return gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], x, ea)


def _info(d, check=True, labeled=False):
    """info of torch.ops.gtok.csr_from_coo (no read-back inside the op)."""
    N, E = int(np.sum(d["node_counts"])), int(np.sum(d["edge_counts"]))
    x, ea = (d.get("x"), d.get("edge_attr")) if labeled else (None, None)
    out = torch.ops.gtok.csr_from_coo(_dev(d["src"]), _dev(d["dst"]), _dev(_slices(d["node_counts"])), _dev(_slices(d["edge_counts"])),
                                      _dev(x), _dev(ea), None, N, E, check)
    return out[-1].tolist()


def test_csr_from_coo_equals_the_host_builder():
    """Every array, flags, maxima, chunk maxima and max_degree, and eorder is None exactly when the host builder's is: sorted and
    unsorted edge lists, typed and untyped, the hand-made edge cases, rings with chords, graphs of 300-600 nodes (the check's
    large-graph path)."""
    cases = [(gtok.synth.zinc_like(5000, seed=41), True), (gtok.synth.zinc_like(1500, seed=42, coalesced=False), True),
             (gtok.synth.graph_token_like(400, seed=43, with_text=False), False),
             (gtok.synth.er_batch(50, seed=44, min_nodes=10, max_nodes=200), False), (edge_case_graphs(), True),
             (_rings_with_chords([64, 63, 5, 1, 0], 20, seed=3), True),
             (_rings_with_chords([300, 450, 600, 257, 256, 12], 400, seed=5), True),
             (_shuffled(_rings_with_chords([600, 300, 7], 300, seed=6), seed=7), True)]
    for k, (d, labeled) in enumerate(cases):
        _assert_same(_host(d, labeled), _build(d, labeled), k)
        _assert_same(_host(d, labeled), gtok.GraphBatch.from_coo_device(
            d["node_counts"], d["edge_counts"], d["src"], d["dst"], d.get("x") if labeled else None,
            d.get("edge_attr") if labeled else None, device=DEV), k)
    untyped = _build(cases[0][0], labeled=False, check=False)
    assert untyped.nattr is None and untyped.eattr is None and untyped.flags == 0 and not untyped.checked
    # x as [N, 3] int64 with the type in column 0 (read in place with stride 3; a non-contiguous view with stride 6; a transposed one
    # with stride 1), edge_attr as [E, 2]; types -1, 255, 256 and 2**40 become 255 as in the host builder
    d = gtok.synth.zinc_like(700, seed=45)
    N, E = int(np.sum(d["node_counts"])), int(np.sum(d["edge_counts"]))
    rng = np.random.default_rng(46)
    odd = np.array([-1, 255, 256, 2 ** 40], np.int64)
    xt, et = np.asarray(d["x"], np.int64).copy(), np.asarray(d["edge_attr"], np.int64).copy()
    xt[rng.permutation(N)[:40]] = np.resize(odd, 40)
    et[rng.permutation(E)[:40]] = np.resize(odd, 40)
    h = gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], xt, et)
    assert int((h.nattr == 255).sum()) >= 40 and int((h.eattr == 255).sum()) >= 40
    x3 = _dev(np.stack([xt, rng.integers(0, 9, N), rng.integers(-7, 7, N)], 1))
    x6 = torch.cat([_dev(rng.integers(0, 300, (N, 3))), x3], 1)[:, 3:]
    xT = x3.t().contiguous().t()
    e2 = _dev(np.stack([et, rng.integers(0, 4, E)], 1))
    assert x3.stride() == (3, 1) and x6.stride() == (6, 1) and not x6.is_contiguous() and xT.stride() == (1, N)
    for xs, what in ((x3, "x [N, 3]"), (x6, "x [N, 3] view of [N, 6]"), (xT, "x [N, 3] transposed")):
        g = gtok.ops.csr_from_coo(_dev(d["src"]), _dev(d["dst"]), _dev(_slices(d["node_counts"])), _dev(_slices(d["edge_counts"])), xs, e2)
        _assert_same(h, g, what)


def test_the_device_sort_bound():
    """An unsorted graph of COO_SORT_NODES nodes is sorted on the device; one node more raises its status bit, and
    from_coo_device still gives the host builder's arrays (through the torch chain)."""
    bound = gtok._lib.COO_SORT_NODES
    under = _shuffled(_rings_with_chords([bound, 9], 3000, seed=11), seed=12)
    over = _shuffled(_rings_with_chords([bound + 1, 9], 3000, seed=13), seed=14)
    b = _build(under)
    assert b.eorder is not None
    _assert_same(_host(under), b)
    with pytest.raises(gtok.ops.CooInputError) as err:
        _build(over)
    assert err.value.status == gtok._lib.COO_SORT_TOO_LARGE
    _assert_same(_host(over), gtok.GraphBatch.from_coo_device(over["node_counts"], over["edge_counts"], over["src"], over["dst"],
                                                              over["x"], over["edge_attr"], device=DEV))


def test_csr_from_coo_with_indices_equals_the_host_subset():
    """Collated storage in HBM and a shuffled subset with repeated indices: from_collated on the device (never through the
    host) and ops.csr_from_coo equal the host from_collated(..., indices=...)."""
    for d, labeled in ((gtok.synth.zinc_like(3000, seed=21, coalesced=False), True), (gtok.synth.er_batch(120, seed=22, max_nodes=90), False)):
        S = len(d["node_counts"])
        rng = np.random.default_rng(23)
        idx = np.concatenate([rng.permutation(S)[: S // 3], rng.integers(0, S, 40), [0, S - 1, S - 1]]).astype(np.int64)
        ei = np.stack([d["src"], d["dst"]])
        x, ea = (d["x"], d["edge_attr"]) if labeled else (None, None)
        h = gtok.GraphBatch.from_collated(torch.as_tensor(d["node_counts"]), torch.as_tensor(ei), torch.as_tensor(_slices(d["edge_counts"])),
                                          None if x is None else torch.as_tensor(x)[:, None], None if ea is None else torch.as_tensor(ea),
                                          indices=idx.tolist())
        g = gtok.GraphBatch.from_collated(_dev(d["node_counts"]), _dev(ei), _dev(_slices(d["edge_counts"])),
                                          None if x is None else _dev(x)[:, None], _dev(ea), indices=_dev(idx))
        assert g.col.device.type == "cuda"
        _assert_same(h, g)
        o = gtok.ops.csr_from_coo(_dev(d["src"]), _dev(d["dst"]), _dev(_slices(d["node_counts"])), _dev(_slices(d["edge_counts"])),
                                  _dev(x), _dev(ea), indices=_dev(idx))
        _assert_same(h, o)
    g2 = gtok.GraphBatch.from_collated(_dev(d["node_counts"]), _dev(ei), _dev(_slices(d["edge_counts"])))      # all graphs, device storage
    _assert_same(_host(d, False), g2)


def test_symmetry_verdicts_match_the_host_check():
    """info[0] > 0 exactly when the host builder clears GTOK_CSR_SIMPLE_SYMMETRIC: clean corpora, a self loop, a missing
    reverse entry, a duplicate (small graphs: the LDS bit matrix; 300+ nodes: the row scan), one-direction synth_er graphs."""
    def damaged(d, how, g):
        d = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
        ep = _slices(d["edge_counts"])
        s, t = d["src"].tolist(), d["dst"].tolist()
        a, b = int(ep[g]), int(ep[g + 1])
        gs, gt = s[a:b], t[a:b]
        if how == "self":
            gs.append(0); gt.append(0)
        elif how == "missing":
            gs.pop(); gt.pop()
        elif how == "dup":
            gs.append(gs[0]); gt.append(gt[0])
        order = np.argsort(np.array(gs), kind="stable")
        gs, gt = list(np.array(gs)[order]), list(np.array(gt)[order])
        d["src"] = np.array(s[:a] + gs + s[b:], np.int64); d["dst"] = np.array(t[:a] + gt + t[b:], np.int64)
        d["edge_counts"] = d["edge_counts"].copy(); d["edge_counts"][g] = len(gs)
        return d
    small, large = _rings_with_chords([30, 12, 40], 20, seed=31), _rings_with_chords([12, 400, 520], 300, seed=32)
    cases = [small, large, gtok.synth.zinc_like(800, seed=33), gtok.synth.er_batch(60, seed=34, max_nodes=200)]
    for base, g in ((small, 1), (large, 1), (large, 2)):
        cases += [damaged(base, how, g) for how in ("self", "missing", "dup")]
    for k, d in enumerate(cases):
        h = _host(d, labeled=False)
        v = _info(d)
        assert v[6] == 0 and (v[0] > 0) == (not (h.flags & gtok._lib.CSR_SIMPLE_SYMMETRIC)), (k, v, h.flags)
        assert _info(d, check=False)[0] == 0


def test_damaged_input_sets_status_bits_not_faults():
    """Endpoints of -1 and N_g, decreasing slices, wrong totals, an index outside the storage: status bits; through
    from_coo_device the same exception as builder="torch"."""
    d = gtok.synth.zinc_like(200, seed=51)
    ns, es = _slices(d["node_counts"]), _slices(d["edge_counts"])
    def status(src=d["src"], dst=d["dst"], nsl=ns, esl=es, indices=None, N=None, E=None):
        with pytest.raises(gtok.ops.CooInputError) as err:
            gtok.ops.csr_from_coo(_dev(src), _dev(dst), _dev(nsl), _dev(esl), indices=_dev(indices), num_nodes=N, num_entries=E)
        return err.value.status
    lb = gtok._lib
    s1 = d["src"].copy(); s1[7] = -1
    d1 = d["dst"].copy(); d1[int(es[5]) + 2] = int(d["node_counts"][5])
    assert status(src=s1) == lb.COO_BAD_ENDPOINT and status(dst=d1) == lb.COO_BAD_ENDPOINT
    s2 = d["src"].copy(); s2[9] = 2 ** 32 + 1                       # endpoints that would wrap to a valid node in 32 bits
    d2 = d["dst"].copy(); d2[int(es[7]) + 1] = -(2 ** 32)
    assert status(src=s2) == lb.COO_BAD_ENDPOINT and status(dst=d2) == lb.COO_BAD_ENDPOINT
    bad_sl = es.copy(); bad_sl[10] = bad_sl[11] + 3
    assert status(esl=bad_sl) & lb.COO_BAD_SLICES
    assert status(N=int(ns[-1]) + 1) == lb.COO_BAD_TOTALS and status(E=int(es[-1]) - 1) == lb.COO_BAD_TOTALS
    assert status(indices=np.array([0, 5, 200, 3])) == lb.COO_BAD_INDEX and status(indices=np.array([-1])) == lb.COO_BAD_INDEX
    bad_nc = d["node_counts"].copy(); bad_nc[3] = -bad_nc[3]
    bad_ec = d["edge_counts"].copy(); bad_ec[4] += 1
    for args in ((d["node_counts"], d["edge_counts"], s1, d["dst"]), (d["node_counts"], d["edge_counts"], d["src"], d1),
                 (d["node_counts"], d["edge_counts"], s2, d["dst"]), (d["node_counts"], d["edge_counts"], d["src"], d2),
                 (bad_nc, d["edge_counts"], d["src"], d["dst"]), (d["node_counts"], bad_ec, d["src"], d["dst"])):
        errs = []
        for builder in ("torch", "auto"):
            with pytest.raises(Exception) as err:
                gtok.GraphBatch.from_coo_device(*args, device=DEV, builder=builder)
            errs.append((type(err.value), str(err.value)))
        assert errs[0] == errs[1], errs
    torch.cuda.synchronize()


def test_csr_from_coo_op_captures_into_a_cuda_graph():
    """torch.ops.gtok.csr_from_coo enqueues without a host sync: captured after one warm-up call, replayed on a second
    corpus of the same totals copied into the captured inputs, it gives the host builder's arrays."""
    a = gtok.synth.zinc_like(1000, seed=61)
    b = _shuffled(a, seed=62)
    b["x"] = (np.asarray(a["x"]) + 3) % 9
    N, E = int(np.sum(a["node_counts"])), int(np.sum(a["edge_counts"]))
    ins = [_dev(a["src"]), _dev(a["dst"]), _dev(_slices(a["node_counts"])), _dev(_slices(a["edge_counts"])), _dev(a["x"]), _dev(a["edge_attr"])]
    torch.ops.gtok.csr_from_coo(*ins, None, N, E, True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = torch.ops.gtok.csr_from_coo(*ins, None, N, E, True)
    for t, v in zip(ins, (b["src"], b["dst"], _slices(b["node_counts"]), _slices(b["edge_counts"]), b["x"], b["edge_attr"])):
        t.copy_(_dev(v))
    graph.replay()
    torch.cuda.synchronize()
    h = _host(b)
    v = out[7].tolist()
    assert v[6] == 0 and v[7] == 1
    got = gtok.ops._coo_batch(dict(zip(ARRAYS + ("info",), out)), v, h.num_graphs, N, E, True)
    _assert_same(h, got)


def test_coo_to_sent_through_bare_ctypes_without_ops_py():
    """A C caller's route: collated COO in HBM -> gtok_csr_from_coo -> one 32-byte read-back -> gtok_csr_lane_sort ->
    gtok_sent; the rows equal the oracle's."""
    L, lb = gtok.lib(), gtok._lib
    G = 30000
    d = gtok.synth.zinc_like(G, seed=71)
    _, coo = both(d)
    dev = torch.device(DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    z = lambda n, dt: torch.empty(n, dtype=dt, device=dev)
    t = {k: torch.as_tensor(np.asarray(v, np.int64)).to(dev) for k, v in
         dict(src=d["src"], dst=d["dst"], x=d["x"], ea=d["edge_attr"], ns=_slices(d["node_counts"]), es=_slices(d["edge_counts"])).items()}
    N, E = int(t["ns"][-1]), int(t["es"][-1])
    b = dict(node_ptr=z(G + 1, torch.int32), edge_ptr=z(G + 1, torch.int64), rowptr=z(N + G, torch.int32), col=z(E, torch.int32),
             eorder=z(E, torch.int32), nattr=z(N, torch.uint8), eattr=z(E, torch.uint8), info=z(8, torch.int32))
    cin = lb.GtokCoo(G, G, N, E, t["ns"].data_ptr(), t["es"].data_ptr(), None, t["src"].data_ptr(), t["dst"].data_ptr(),
                     t["x"].data_ptr(), 1, t["ea"].data_ptr(), 1)
    cout = lb.GtokCsrBuilt(*[b[n].data_ptr() for n, _ in lb.GtokCsrBuilt._fields_])
    ws = z(int(L.gtok_csr_from_coo_workspace(G, G)), torch.uint8)
    assert L.gtok_csr_from_coo(ctypes.byref(cin), 1, ctypes.byref(cout), ws.data_ptr(), ws.numel(), stream) == 0
    viol, maxdeg, maxn, maxe, chunk_n, chunk_e, status, unsorted = b["info"].tolist()
    assert viol == 0 and status == 0 and unsorted == 0
    csr = lb.GtokCsr(G, maxn, maxe, lb.CSR_SIMPLE_SYMMETRIC, b["node_ptr"].data_ptr(), b["edge_ptr"].data_ptr(), b["rowptr"].data_ptr(),
                     b["col"].data_ptr(), None, b["nattr"].data_ptr(), b["eattr"].data_ptr(), chunk_n, chunk_e, maxdeg, 0,
                     None, None, None, None, None, 0, 0, None, None, 0, 0, None)
    o = dict(graph_ids=z(G, torch.int32), node_ptr=z(G + 1, torch.int32), edge_ptr=z(G + 1, torch.int64), rowptr=z(N + G, torch.int32), col=z(E, torch.int32),
             nattr=z(N, torch.uint8), eattr=z(E, torch.uint8), rowptr8=z(N + G + 16, torch.uint8), col8=z(E + 16, torch.uint8),
             unit_ptr=z(G + 1, torch.int32), unit_info=z(8 * G, torch.int32), info=z(8, torch.int32))
    ws2 = z(int(L.gtok_csr_lane_sort_workspace(G)), torch.uint8)
    outs = lb.GtokCsrSorted(*[o[n].data_ptr() for n, _ in lb.GtokCsrSorted._fields_])
    assert L.gtok_csr_lane_sort(ctypes.byref(csr), 0, 0, ctypes.byref(outs), ws2.data_ptr(), ws2.numel(), stream) == 0
    _, _, _, _, units, cn2, ce2, _ = o["info"].tolist()
    srt = lb.GtokCsr(G, maxn, maxe, lb.CSR_SIMPLE_SYMMETRIC, o["node_ptr"].data_ptr(), o["edge_ptr"].data_ptr(), o["rowptr"].data_ptr(),
                     o["col"].data_ptr(), None, o["nattr"].data_ptr(), o["eattr"].data_ptr(), cn2, ce2, maxdeg, 0, o["rowptr8"].data_ptr(),
                     o["col8"].data_ptr(), None, None, None, 0, 0, o["graph_ids"].data_ptr(), o["unit_ptr"].data_ptr(), units, 0, o["unit_info"].data_ptr())
    p = lb.GtokSentParams(maxn, 1, 9, 4, 1024, 1, 5, 0, 42, 9, 0, None, 1, 0)
    ids, ln = z((G, 176), torch.int32), z(G, torch.int32)
    assert L.gtok_sent(ctypes.byref(srt), ctypes.byref(p), ids.data_ptr(), 176, ln.data_ptr(), stream) == 0
    ref, rln = orc.sent(coo, maxn, 1024, 42, 9, ld=176, **ZKW)
    assert np.array_equal(ln.cpu().numpy(), rln) and np.array_equal(ids.cpu().numpy(), ref)
    assert L.gtok_csr_from_coo(ctypes.byref(cin), 1, ctypes.byref(cout), ws.data_ptr(), 16, stream) == -1      # workspace too small
    assert L.gtok_csr_from_coo(None, 1, ctypes.byref(cout), ws.data_ptr(), ws.numel(), stream) == -1


def test_full_size_corpora_hip_builder_equals_the_torch_chain():
    """ZINC-full's shape (249,456 molecules) and a 20 k-graph share of the config-5 mix, inputs already in HBM: the HIP
    builder gives the torch chain's arrays, flags and maxima."""
    z = gtok.synth.zinc_like(249456, seed=81)
    m = gtok.synth.mix_batch_device(20000, DEV, seed=82)
    for d, labeled in ((z, True), (m, False)):
        args = [_dev(d[k]) for k in ("node_counts", "edge_counts", "src", "dst")]
        ty = [_dev(d["x"]), _dev(d["edge_attr"])] if labeled else [None, None]
        a = gtok.GraphBatch.from_coo_device(*args, *ty, device=DEV, builder="torch")
        b = gtok.GraphBatch.from_coo_device(*args, *ty, device=DEV)
        _assert_same(a, b)
        assert a.checked == b.checked
