"""gtok_graph_tasks (include/gtok.h) on the device: cycle check, components and shortest-path distances of every search - closure
rows in registers, the bit matrix in LDS (W = 2, 4, 8), the push search over the CSR - against the numpy restatement of the
definitions (tests/_graph_tasks_ref.py).  Every comparison is exact; every launch of this file writes into guarded arrays."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _graph_tasks_ref as ref
from _util import GOLDEN_DIR, edge_case_graphs, gtok

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_lib = gtok._lib
SYM = _lib.CSR_SIMPLE_SYMMETRIC
GUARD, SENTINEL = 64, -77
SIZES = (0, 1, 2, 63, 64, 65, 128, 129, 256, 511, 512)
FAMILIES = ("path", "ring", "star", "complete", "two_components", "isolated", "tree_chord")
LISTINGS = ("once", "both", "messy")


# ------------------------------------------------------------------------------------------------ graphs
def family_edges(family, n, rng):
    """[(u, v)] with u < v, every edge once"""
    a = np.arange(max(n - 1, 0))
    path = lambda lo, hi: [(i, i + 1) for i in range(lo, hi - 1)]
    if family == "path":
        return path(0, n)
    if family == "ring":
        return path(0, n) + ([(0, n - 1)] if n >= 3 else [])
    if family == "star":
        return [(0, int(i) + 1) for i in a]
    if family == "complete":
        iu, iv = np.triu_indices(n, 1)
        return list(zip(iu.tolist(), iv.tolist()))
    if family == "two_components":          # a path on the first half, a ring on the second
        h = n // 2
        return path(0, h) + path(h, n) + ([(h, n - 1)] if n - h >= 3 else [])
    if family == "isolated":
        return []
    if family == "tree_chord":              # a random tree and one edge more
        e = {(int(rng.integers(0, i)), i) for i in range(1, n)}
        for u in range(n):
            v = next((v for v in range(u + 1, n) if (u, v) not in e), None)
            if v is not None:
                e.add((u, v))
                break
        return sorted(e)
    raise ValueError(family)


def listed(edges, n, listing, rng, loops):
    """the edge list as the batch stores it: once, in both directions, or with duplicates, reversed copies (and self loops)"""
    e = list(edges)
    if listing == "both":
        e = e + [(v, u) for u, v in e]
    elif listing == "messy":
        if e:
            take = rng.integers(0, len(e), len(e) // 3 + 1)
            e = e + [e[i] for i in take[::2]] + [(e[i][1], e[i][0]) for i in take[1::2]]
        if loops and n:
            e = e + [(int(v), int(v)) for v in rng.integers(0, n, 2)]
        e = [e[i] for i in rng.permutation(len(e))]
    return e


def graph_queries(n, k):
    """the queries of case k on n nodes: both ends of the numbering (a path's N - 1 levels), u == v, repeated sources, a change of
    source and back, endpoints outside the graph on every fifth case, none at all on every seventh"""
    if k % 7 == 3:
        return []
    if n == 0:
        return [(0, 0)] if k % 2 else []
    q = [(0, n - 1), (n - 1, 0), (n // 2, n // 2), (0, n // 2), (0, min(1, n - 1)), (n - 1, n // 3), (0, n - 1), (n // 2, n - 1)]
    if k % 5 == 0:
        q += [(-1, 0), (0, n), (2 ** 31 - 1, 0), (0, -(2 ** 31)), (n, n)]
    return q


class Cases:
    """a list of graphs with their queries -> batched COO, query arrays and (once) the reference answers"""

    def __init__(self, graphs):
        self.n = np.array([g[0] for g in graphs], np.int64)
        self.ec = np.array([len(g[1]) for g in graphs], np.int64)
        self.src = np.array([u for g in graphs for u, _ in g[1]], np.int64)
        self.dst = np.array([v for g in graphs for _, v in g[1]], np.int64)
        self.queries = np.array([q for g in graphs for q in g[2]], np.int64).reshape(-1, 2).astype(np.int32)
        self.qptr = np.concatenate([[0], np.cumsum([len(g[2]) for g in graphs])]).astype(np.int64)
        self._want = None

    def subset(self, keep):
        eptr = np.concatenate([[0], np.cumsum(self.ec)])
        return Cases([(int(self.n[g]), list(zip(self.src[eptr[g]:eptr[g + 1]].tolist(), self.dst[eptr[g]:eptr[g + 1]].tolist())),
                       [tuple(q) for q in self.queries[self.qptr[g]:self.qptr[g + 1]].tolist()]) for g in keep])

    @property
    def want(self):
        if self._want is None:
            self._want = ref.batch_answers(self.n, self.ec, self.src, self.dst, self.queries, self.qptr)
        return self._want

    def batch(self):
        return gtok.GraphBatch.from_coo(self.n, self.ec, self.src, self.dst).to(DEV)


_CASES = {}


def boundary_cases(listing):
    """every family at every size, listed one way (kept for the session: the reference runs once)"""
    if listing not in _CASES:
        rng = np.random.default_rng(LISTINGS.index(listing))
        graphs = []
        for n in SIZES:
            for f in FAMILIES:
                k = len(graphs)
                graphs.append((n, listed(family_edges(f, n, rng), n, listing, rng, loops=k % 2 == 0), graph_queries(n, k)))
        if listing == "messy":
            d = edge_case_graphs()
            eptr = np.concatenate([[0], np.cumsum(d["edge_counts"])])
            for g, n in enumerate(d["node_counts"]):
                graphs.append((int(n), list(zip(d["src"][eptr[g]:eptr[g + 1]].tolist(), d["dst"][eptr[g]:eptr[g + 1]].tolist())),
                               graph_queries(int(n), len(graphs))))
        _CASES[listing] = Cases(graphs)
    return _CASES[listing]


# ------------------------------------------------------------------------------------------------ guarded launches
class Guarded:
    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        self.view = self.buf[GUARD:GUARD + n]

    def ptr(self):
        return self.view.data_ptr()

    def check(self, what):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + self.n:] == SENTINEL).all(), f"{what}: a guard region was written"
        return b[GUARD:GUARD + self.n]


def raw_call(batch, queries=None, qptr=None, cyc=True, comp=True, dist=True, kernel=None, nq=None):
    """gtok_graph_tasks through ctypes alone, every output between guard regions -> (rc, dict of host arrays)"""
    G = batch.num_graphs
    out = {}
    if cyc:
        out["has_cycle"] = Guarded(G)
    if comp:
        out["num_components"] = Guarded(G)
    qt = pt = None
    Q = 0
    if queries is not None:
        qt = torch.from_numpy(np.ascontiguousarray(queries, np.int32).reshape(-1, 2)).to(DEV)
        Q = qt.shape[0] if nq is None else nq
        if qt.numel() == 0:
            qt = torch.zeros((1, 2), dtype=torch.int32, device=DEV)
        if qptr is not None:
            pt = torch.from_numpy(np.ascontiguousarray(qptr, np.int64)).to(DEV)
        if dist:
            out["dist"] = Guarded(max(Q, 0))
    info = Guarded(4)
    info.view.zero_()
    out["info"] = info
    p = lambda k: out[k].ptr() if k in out else None
    old = os.environ.pop("GTOK_TASKS_KERNEL", None)
    if kernel:
        os.environ["GTOK_TASKS_KERNEL"] = kernel
    try:
        cs = batch.c_struct()
        rc = _lib.lib().gtok_graph_tasks(ctypes.byref(cs), None if qt is None else qt.data_ptr(), None if pt is None else pt.data_ptr(), Q,
                                         p("has_cycle"), p("num_components"), p("dist"), info.ptr(), None)
        torch.cuda.synchronize()
    finally:
        os.environ.pop("GTOK_TASKS_KERNEL", None)
        if old is not None:
            os.environ["GTOK_TASKS_KERNEL"] = old
    return rc, {k: v.check(f"{k} (kernel={kernel})") for k, v in out.items()}


def assert_answers(cases, batch, kernel, what):
    rc, got = raw_call(batch, cases.queries, cases.qptr, kernel=kernel)
    assert rc == 0, (what, rc)
    want = cases.want
    for k in ("num_components", "has_cycle", "dist", "info"):
        bad = np.nonzero(got[k] != want[k])[0]
        assert bad.size == 0, f"{what}: {k} differs at {bad[:8]}: got {got[k][bad[:8]]}, want {want[k][bad[:8]]}"


# ------------------------------------------------------------------------------------------------ each search at its sizes
SLICES = {"reg": (0, 64), "lds2": (65, 128), "lds4": (129, 256), "lds8": (257, 512)}


@pytest.mark.parametrize("listing", LISTINGS)
@pytest.mark.parametrize("cls", sorted(SLICES))
def test_each_search_at_its_own_sizes(listing, cls):
    """a batch whose max_nodes selects the search: <= 64 registers, <= 128 / 256 / 512 the LDS matrix with W = 2 / 4 / 8"""
    full = boundary_cases(listing)
    lo, hi = SLICES[cls]
    c = full.subset([g for g in range(full.n.size) if lo <= full.n[g] <= hi])
    b = c.batch()
    assert lo <= b.max_nodes <= hi
    if listing == "both":
        assert b.flags & SYM
    want = c.want
    assert want["info"][0] == 1 and (want["dist"] == -1).any() and (want["dist"] == 0).any() and 0 < want["has_cycle"].sum() < c.n.size
    assert_answers(c, b, None, f"{cls} {listing}")
    if cls != "reg":
        assert want["dist"].max() == hi - 1, "both ends of the longest path: N - 1 levels"


@pytest.mark.parametrize("listing", LISTINGS)
def test_small_graphs_through_the_larger_searches(listing):
    """the whole size sweep as ONE batch runs the W = 8 matrix on graphs of 0 .. 512 nodes; the <= 64-node graphs also through
    W = 2 by the hook; both-direction lists (simple and symmetric) through the CSR search as well"""
    full = boundary_cases(listing)
    b = full.batch()
    assert b.max_nodes == 512
    assert_answers(full, b, None, f"all sizes {listing}")
    small = full.subset([g for g in range(full.n.size) if full.n[g] <= 64])
    sb = small.batch()
    assert_answers(small, sb, "lds", f"small graphs, lds forced, {listing}")
    assert_answers(small, sb, "reg", f"small graphs, reg forced, {listing}")
    if listing == "both":
        assert (b.flags & SYM) and (sb.flags & SYM)
        assert_answers(full, b, "csr", "all sizes, csr forced")
        assert_answers(small, sb, "csr", "small graphs, csr forced")
    else:
        assert not (b.flags & SYM)
        assert raw_call(b, full.queries, full.qptr, kernel="csr")[0] == _lib.E_UNSUPPORTED
    assert raw_call(b, full.queries, full.qptr, kernel="reg")[0] == _lib.E_UNSUPPORTED      # 512 nodes do not fit the registers


def test_one_query_per_graph_without_query_ptr_and_outputs_null_in_turn():
    full = boundary_cases("messy")
    b = full.batch()
    G = full.n.size
    q = np.stack([np.zeros(G, np.int64), np.maximum(full.n - 1, 0)], 1)
    q[::9] = [[3, -1]]
    want = ref.batch_answers(full.n, full.ec, full.src, full.dst, q)
    rc, got = raw_call(b, q)
    assert rc == 0 and all(np.array_equal(got[k], want[k]) for k in want)
    # every output NULL in turn; has_cycle only; the distances only
    for cyc, comp, dist in ((False, True, True), (True, False, True), (True, True, False), (True, False, False), (False, True, False),
                            (False, False, True)):
        rc, got = raw_call(b, q if dist else None, cyc=cyc, comp=comp, dist=dist)
        assert rc == 0 and set(got) == {k for k, on in (("has_cycle", cyc), ("num_components", comp), ("dist", dist)) if on} | {"info"}
        for k in got:
            if k != "info":
                assert np.array_equal(got[k], want[k]), (k, cyc, comp, dist)
        assert got["info"][3] == (want["info"][3] if cyc or comp else 0)
        assert got["info"][:3].tolist() == (want["info"][:3].tolist() if dist else [0, 0, 0])
    rc, got = raw_call(b, None, cyc=False, comp=False, dist=False)
    assert rc == 0 and got["info"].tolist() == [0, 0, 0, 0]                  # nothing asked for
    # the argument rules, through the library
    assert raw_call(b, q[:-1])[0] == -1                                        # query_ptr == NULL and Q != G
    assert raw_call(b, q, dist=False)[0] == -1                                 # queries without dist
    assert raw_call(b, full.queries, full.qptr, nq=-1, dist=False)[0] == -1
    # damaged query_ptr: beyond Q / decreasing - those graphs' queries are not answered, status bit 1, nothing else is touched
    ptr = full.qptr.copy()
    ptr[5] = full.queries.shape[0] + 1
    rc, got = raw_call(b, full.queries, ptr)
    assert rc == 0 and got["info"][0] & 2
    keep = np.ones(full.queries.shape[0], bool)
    keep[full.qptr[4]:full.qptr[6]] = False
    assert np.array_equal(got["dist"][keep], full.want["dist"][keep]) and (got["dist"][~keep] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ the CSR search at its sizes
def _both(edges):
    return edges + [(v, u) for u, v in edges]


_LARGE = None


def large_cases():
    global _LARGE
    if _LARGE is None:
        N = _lib.SENT_LARGE_MAX_NODES
        ring = [(i, (i + 1) % 4097) for i in range(4097)] + [(i, (i + 1500) % 4097) for i in range(0, 4097, 400)]
        two = [(i, i + 1) for i in range(255)] + [(i, i + 1) for i in range(256, 512)] + [(256, 512)]
        graphs = [
            (N, _both([(i, i + 1) for i in range(N - 1)]), [(0, N - 1), (N - 1, 0), (0, 1), (0, N // 2), (N // 2, N // 2), (0, N)]),
            (3, _both([(0, 1), (1, 2), (0, 2)]), [(0, 2)]),
            (N, _both([(0, i) for i in range(1, N)]), [(1, N - 1), (N - 1, 0), (0, 77), (5, 6), (5, 5)]),
            (4097, _both(ring), [(0, 2048), (0, 4096), (0, 1500), (1234, 3210), (1234, 1), (4096, 2047)]),
            (513, _both(two), [(0, 255), (0, 256), (256, 512), (257, 512), (511, 0), (512, 257)]),
            (600, [], [(0, 599), (7, 7)]),
        ]
        _LARGE = Cases(graphs)
    return _LARGE


def test_csr_search_on_large_flagged_graphs():
    """the 16,384-node path (distance 16,383, one node per level), a 16,384-node star (a row of 16,383 entries read by the whole wave,
    leaf to leaf = 2), a 4,097-node ring with chords, a 513-node graph of two components, 600 isolated nodes"""
    c = large_cases()
    b = c.batch()
    assert b.max_nodes == _lib.SENT_LARGE_MAX_NODES and (b.flags & SYM)
    want = c.want
    assert want["dist"][:2].tolist() == [16383, 16383] and want["dist"][7] == 2 and want["num_components"].tolist() == [1, 1, 1, 1, 2, 600]
    assert want["has_cycle"].tolist() == [0, 1, 0, 1, 1, 0]
    assert_answers(c, b, None, "large graphs")


def test_size_and_flag_limits():
    c = large_cases()
    one = c.subset([4])                                             # 513 nodes
    eh = one.src < one.dst
    once = gtok.GraphBatch.from_coo(one.n, [int(eh.sum())], one.src[eh], one.dst[eh]).to(DEV)
    assert once.max_nodes == 513 and not (once.flags & SYM)
    assert raw_call(once, one.queries, one.qptr)[0] == _lib.E_UNSUPPORTED
    with pytest.raises(_lib.GtokError, match="GTOK_CSR_SIMPLE_SYMMETRIC"):
        gtok.ops.graph_tasks(once)
    N = _lib.SENT_LARGE_MAX_NODES + 1
    big = gtok.GraphBatch.from_coo([N], [2], [0, 1], [1, 0]).to(DEV)
    assert big.flags & SYM
    assert raw_call(big, [[0, 1]])[0] == -2                         # GTOK_E_TOO_LARGE
    with pytest.raises(_lib.GtokError, match="TOO_LARGE"):
        gtok.ops.graph_tasks(big)
    # damaged arrays: a slice beyond max_nodes counts as an empty graph, a column outside its graph is skipped - status bit 1
    good = c.subset([1, 1, 1])
    b = good.batch()
    b.max_nodes = 2
    rc, got = raw_call(b, good.queries, good.qptr)
    assert rc == 0 and got["info"].tolist()[0] == 3 and got["num_components"].tolist() == [0, 0, 0] and got["dist"].tolist() == [-2, -2, -2]
    b = good.batch()
    b.col[7] = 3
    b.col[14] = -1
    for kernel in ("reg", "lds", "csr"):
        rc, got = raw_call(b, good.queries, good.qptr, kernel=kernel)
        assert rc == 0 and got["info"][0] == 2 and got["num_components"].tolist() == [1, 1, 1] and got["dist"].tolist()[0] == 1, kernel


# ------------------------------------------------------------------------------------------------ the Python surfaces
def test_ops_and_torch_op_equal_the_raw_call():
    full = boundary_cases("both")
    b = full.batch()
    q, p = torch.from_numpy(full.queries).to(DEV), torch.from_numpy(full.qptr).to(DEV)
    r = gtok.ops.graph_tasks(b, q, p)
    want = full.want
    assert np.array_equal(r.has_cycle.cpu().numpy(), want["has_cycle"]) and np.array_equal(r.num_components.cpu().numpy(), want["num_components"])
    assert np.array_equal(r.dist.cpu().numpy(), want["dist"]) and r.info.cpu().tolist() == want["info"].tolist()
    assert r.status() == dict(status=1, max_dist=int(want["info"][1]), unreachable=int(want["info"][2]), cycles=int(want["info"][3]))
    only = gtok.ops.graph_tasks(b, num_components=False)
    assert only.num_components is None and only.dist is None and torch.equal(only.has_cycle, r.has_cycle)
    t = torch.ops.gtok.graph_tasks(b.node_ptr, b.edge_ptr, b.rowptr, b.col, b.max_nodes, b.max_edges, b.flags, q, p)
    for got, exp in zip(t, (r.has_cycle, r.num_components, r.dist, r.info)):
        assert got.dtype == torch.int32 and torch.equal(got, exp)
    t0 = torch.ops.gtok.graph_tasks(b.node_ptr, b.edge_ptr, b.rowptr, b.col, b.max_nodes, b.max_edges, 0, None, None)
    assert torch.equal(t0[0], r.has_cycle) and t0[2].numel() == 0
    # the fake kernel: shapes without a launch
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode(allow_non_fake_inputs=False) as mode:
        f = lambda x: mode.from_tensor(x)
        ft = torch.ops.gtok.graph_tasks(f(b.node_ptr), f(b.edge_ptr), f(b.rowptr), f(b.col), b.max_nodes, b.max_edges, b.flags, f(q), f(p))
        f0 = torch.ops.gtok.graph_tasks(f(b.node_ptr), f(b.edge_ptr), f(b.rowptr), f(b.col), b.max_nodes, b.max_edges, b.flags, None, None)
    assert [tuple(x.shape) for x in ft] == [(b.num_graphs,), (b.num_graphs,), (q.shape[0],), (4,)] and all(x.dtype == torch.int32 for x in ft)
    assert tuple(f0[2].shape) == (0,)


def _golden_records(task):
    with open(os.path.join(GOLDEN_DIR, "reference_vectors.json")) as fh:
        return [e["text"] for e in json.load(fh)[f"synth_{task}_examples"]]


@pytest.mark.parametrize("task", ("cycle_check", "shortest_path"))
def test_golden_text_records_are_consistent_and_tampering_is_found(task):
    """parse on the device -> CSR on the device -> check_task_labels: the reference's records agree with their graphs; a flipped
    label / a lenK moved by one is reported, and nothing else"""
    texts = _golden_records(task)
    tb, tp = gtok.ops.pack_texts(texts)
    r = gtok.ops.parse_graph_texts(tb.to(DEV), tp)
    assert int((r["status"] != 0).sum()) == 0
    b = gtok.GraphBatch.from_coo_device(r["num_nodes"], r["num_edges"], r["src"], r["dst"], device=DEV)
    labelled = (r["label"] != gtok.ops.NO_LABEL).cpu().numpy()
    assert labelled.sum() >= 10
    q = r["query"] if task == "shortest_path" else None
    bad = gtok.ops.check_task_labels(b, task, r["label"], q)
    assert bad.dtype == torch.bool and int(bad.sum()) == 0
    lab = r["label"].clone()
    hit = np.nonzero(labelled)[0][[0, 3, 7]]
    lab[hit[0]] = (1 - lab[hit[0]]) if task == "cycle_check" else lab[hit[0]] + 1
    lab[hit[1]] = (1 - lab[hit[1]]) if task == "cycle_check" else lab[hit[1]] - 1
    bad = gtok.ops.check_task_labels(b, task, lab, q)
    assert np.nonzero(bad.cpu().numpy())[0].tolist() == sorted(hit[:2].tolist())
    none = torch.full_like(lab, gtok.ops.NO_LABEL)
    assert int(gtok.ops.check_task_labels(b, task, none, q).sum()) == 0            # no label: never a disagreement
    if task == "shortest_path":
        assert int(gtok.ops.check_task_labels(b, task, lab, torch.full_like(q, -1)).sum()) == 0      # no query neither
        # and the labels themselves: lenK <-> K - 1 (gtok_parse_graph_text) == dist - 1
        d = gtok.ops.graph_tasks(b, q, has_cycle=False, num_components=False).dist
        assert torch.equal((d - 1)[torch.from_numpy(labelled).to(DEV)], r["label"][torch.from_numpy(labelled).to(DEV)])


_CORPORA = {}


def _corpus(kind):
    if kind not in _CORPORA:
        d = (gtok.synth.er_batch_device if kind == "er" else gtok.synth.mix_batch_device)(2000, DEV, seed=3)
        _CORPORA[kind] = (d, gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"]).to(DEV))
    return _CORPORA[kind]


@pytest.mark.parametrize("kind", ("er", "mix"))
def test_label_batch_device_on_device_built_corpora(kind):
    d, b = _corpus(kind)
    G = b.num_graphs
    cyc = gtok.synth.label_batch_device(b, "cycle_check", seed=5)["labels"]
    sp = gtok.synth.label_batch_device(b, "shortest_path", seed=5)
    q = sp["queries"].cpu().numpy()
    n = d["node_counts"]
    assert sp["queries"].dtype == torch.int32 and q.shape == (G, 2) and (q >= 0).all() and (q < n[:, None]).all() and (q[:, 0] != q[:, 1]).all()
    assert sp["graph_index"].tolist() == list(range(G))
    want = ref.batch_answers(n, d["edge_counts"], d["src"], d["dst"], q)
    assert np.array_equal(cyc.cpu().numpy(), want["has_cycle"]) and np.array_equal(sp["dist"].cpu().numpy(), want["dist"])
    assert torch.equal(sp["labels"], sp["dist"] - 1) and torch.equal(sp["keep"], sp["dist"] > 0)
    again = gtok.synth.label_batch_device(b, "shortest_path", seed=5)
    other = gtok.synth.label_batch_device(b, "shortest_path", seed=6)
    assert torch.equal(again["queries"], sp["queries"]) and not torch.equal(other["queries"], sp["queries"])
    # several pairs per graph, graph by graph
    sp3 = gtok.synth.label_batch_device(b, "shortest_path", seed=9, pairs_per_graph=3)
    q3 = sp3["queries"].cpu().numpy()
    assert sp3["graph_index"].tolist() == np.repeat(np.arange(G), 3).tolist() and sp3["query_ptr"].tolist() == list(range(0, 3 * G + 1, 3))
    want3 = ref.batch_answers(n, d["edge_counts"], d["src"], d["dst"], q3, sp3["query_ptr"].cpu().numpy())
    assert np.array_equal(sp3["dist"].cpu().numpy(), want3["dist"])
    # ops.sent(query=queries) appends exactly those nodes: [6 + N, 6 + u, 6 + v] behind the trail, found the way the trainer finds <q>
    ids, ln = gtok.ops.sent(b, 256, 600, seed=1, query=sp["queries"])
    X, _ = gtok.ops.collate(ids, ln, torch.arange(G), gtok.ops.SENT_PAD, int(ln.max()))
    Xh, lh = X.cpu().numpy(), ln.cpu().numpy()
    for nodes in np.unique(n):
        rows = np.nonzero(n == nodes)[0]
        pos = gtok.ops.find_token(X, gtok.ops.SENT_IDX_OFFSET + int(nodes)).cpu().numpy()[rows]
        assert np.array_equal(pos, lh[rows] - 3)
        assert np.array_equal(Xh[rows, pos + 1], 6 + q[rows, 0]) and np.array_equal(Xh[rows, pos + 2], 6 + q[rows, 1])


def test_graphs_of_fewer_than_two_nodes_get_no_pair():
    b = gtok.GraphBatch.from_coo([1, 0, 2, 5], [0, 0, 1, 2], [0, 0, 3], [1, 1, 4]).to(DEV)
    sp = gtok.synth.label_batch_device(b, "shortest_path", seed=0, pairs_per_graph=2)
    assert sp["queries"][:4].tolist() == [[-1, -1]] * 4 and sp["keep"][:4].tolist() == [False] * 4
    assert sorted(sp["queries"][4].tolist()) == [0, 1] and sp["dist"][4:6].tolist() == [1, 1] and sp["keep"][4:6].tolist() == [True, True]
    assert gtok.synth.label_batch_device(b, "cycle_check", 0)["labels"].tolist() == [0, 0, 0, 0]


def test_ibtt_round_trip_keeps_the_answers():
    """rows of ops.ibtt_synth -> ops.ibtt_decode_csr -> graph_tasks: the decoded batch answers as the input batch does"""
    d = gtok.synth.graph_token_like(400, seed=8, task=None, with_text=False)
    b = gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"]).to(DEV)
    vocab = {t: i for i, t in enumerate(["<pad>", "<bos>", "<eos>", "<e>", "<n>", "<q>", "<p>", "yes", "no"] + [str(i) for i in range(64)])}
    lut = gtok.ops.synth_lut(vocab, 64)
    ids, ln = gtok.ops.ibtt_synth(b, lut, None, 4096, vocab["<pad>"])
    inv = gtok.ops.ibtt_inverse_lut(lut, len(vocab), vocab["<pad>"])
    back, status, _ = gtok.ops.ibtt_decode_csr(ids, ln, "synth", inv, 64)
    assert int((status != 0).sum()) == 0 and back.num_graphs == b.num_graphs
    sp = gtok.synth.label_batch_device(b, "shortest_path", seed=2)
    one, two = gtok.ops.graph_tasks(b, sp["queries"]), gtok.ops.graph_tasks(back, sp["queries"])
    for k in ("has_cycle", "num_components", "dist", "info"):
        assert torch.equal(getattr(one, k), getattr(two, k)), k
    want = ref.batch_answers(d["node_counts"], d["edge_counts"], d["src"], d["dst"], sp["queries"].cpu().numpy())
    assert np.array_equal(one.has_cycle.cpu().numpy(), want["has_cycle"]) and np.array_equal(one.dist.cpu().numpy(), want["dist"])
    assert 0 < int(one.has_cycle.sum()) < b.num_graphs
