"""gtok_graph_keys (include/gtok.h) on the device: the keys of every kernel - the stream over the CSR (listed keys, with and without
attributes; closure keys beyond 512 nodes), closure rows in registers, the bit matrix in LDS (W = 2, 4, 8) - against the numpy
restatement of the digest (tests/_graph_keys_ref.py), and ops.duplicate_graphs / ops.split_leakage against Python sets of the
reference's tuple keys (test/train_performance_test.py:70-74, :146-207).  Every comparison is exact; every raw launch of this file
writes its keys and its info between guard regions."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _graph_keys_ref as ref
from _util import gtok
from test_gpu_graph_tasks import FAMILIES, LISTINGS, SIZES, family_edges, listed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_lib = gtok._lib
SYM = _lib.CSR_SIMPLE_SYMMETRIC
LISTED, CLOSURE, ATTRS = _lib.KEYS_LISTED, _lib.KEYS_CLOSURE, _lib.KEYS_ATTRS
MODES = {"listed": LISTED, "closure": CLOSURE}
GUARD, SENTINEL = 64, -77


# ------------------------------------------------------------------------------------------------ graphs
class Cases:
    """a list of (n, [(u, v)], label[, x, edge bytes]) -> batched COO, the batch, and (once per mode) the reference keys"""

    def __init__(self, graphs):
        self.graphs = graphs
        self.n = np.array([g[0] for g in graphs], np.int64)
        self.ec = np.array([len(g[1]) for g in graphs], np.int64)
        self.src = np.array([u for g in graphs for u, _ in g[1]], np.int64)
        self.dst = np.array([v for g in graphs for _, v in g[1]], np.int64)
        self.labels = np.array([g[2] for g in graphs], np.int32)
        self.attrs = len(graphs) > 0 and len(graphs[0]) > 3
        self.x = np.array([t for g in graphs for t in g[3]], np.int64) if self.attrs else None
        self.ea = np.array([t for g in graphs for t in g[4]], np.int64) if self.attrs else None
        self._want = {}

    def subset(self, keep):
        return Cases([self.graphs[g] for g in keep])

    def want(self, mode, attrs=False):
        k = (mode, attrs)
        if k not in self._want:
            self._want[k] = ref.batch_keys(self.n, self.ec, self.src, self.dst, self.labels, mode, self.x if attrs else None,
                                           self.ea if attrs else None)
        return self._want[k]

    def batch(self):
        return gtok.GraphBatch.from_coo(self.n, self.ec, self.src, self.dst, self.x, self.ea).to(DEV)


_CASES = {}


def boundary_cases(listing):
    """every family at every size, listed one way, labels -1 .. 3 (kept for the session: the reference runs once)"""
    if listing not in _CASES:
        rng, same_trees = np.random.default_rng(10 + LISTINGS.index(listing)), np.random.default_rng(9)
        graphs = []
        for n in SIZES:
            for f in FAMILIES:
                k = len(graphs)
                graphs.append((n, listed(family_edges(f, n, same_trees), n, listing, rng, loops=k % 2 == 0), k % 5 - 1))
        _CASES[listing] = Cases(graphs)
    return _CASES[listing]


# ------------------------------------------------------------------------------------------------ guarded launches
class Guarded:
    def __init__(self, n, dtype):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
        self.view = self.buf[GUARD:GUARD + n]

    def check(self, what):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + self.n:] == SENTINEL).all(), f"{what}: a guard region was written"
        return b[GUARD:GUARD + self.n]


def raw_call(batch, labels, flags, kernel=None):
    """gtok_graph_keys through ctypes alone, keys and info between guard regions -> (rc, keys uint64 [G, 2], info [4])"""
    G = batch.num_graphs
    keys, info = Guarded(2 * G, torch.int64), Guarded(4, torch.int32)
    info.view.zero_()
    lt = None if labels is None else torch.from_numpy(np.ascontiguousarray(labels, np.int32)).to(DEV)
    old = os.environ.pop("GTOK_KEYS_KERNEL", None)
    if kernel:
        os.environ["GTOK_KEYS_KERNEL"] = kernel
    try:
        cs = batch.c_struct()
        rc = _lib.lib().gtok_graph_keys(ctypes.byref(cs), None if lt is None else lt.data_ptr(), flags, keys.view.data_ptr(),
                                        info.view.data_ptr(), None)
        torch.cuda.synchronize()
    finally:
        os.environ.pop("GTOK_KEYS_KERNEL", None)
        if old is not None:
            os.environ["GTOK_KEYS_KERNEL"] = old
    return rc, keys.check(f"keys (kernel={kernel})").view(np.uint64).reshape(G, 2), info.check("info")


def assert_keys(cases, batch, mode, what, kernel=None, attrs=False):
    rc, got, info = raw_call(batch, cases.labels, MODES[mode] | (ATTRS if attrs else 0), kernel)
    assert rc == 0, (what, rc)
    want = cases.want(mode, attrs)
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, f"{what}: keys differ at graphs {bad[:8]} (nodes {cases.n[bad[:8]]})"
    assert info.tolist() == [0, 0, 0, 0], what
    return got


# ------------------------------------------------------------------------------------------------ each kernel at its sizes
SLICES = {"reg": (0, 64), "lds2": (65, 128), "lds4": (129, 256), "lds8": (257, 512)}


@pytest.mark.parametrize("listing", LISTINGS)
@pytest.mark.parametrize("cls", sorted(SLICES))
def test_keys_equal_the_numpy_digest_at_each_closure_kernels_sizes(listing, cls):
    """a batch whose max_nodes selects the closure kernel (<= 64 registers, <= 128 / 256 / 512 the LDS matrix with W = 2 / 4 / 8): its
    closure keys and its listed keys"""
    full = boundary_cases(listing)
    lo, hi = SLICES[cls]
    c = full.subset([g for g in range(full.n.size) if lo <= full.n[g] <= hi])
    b = c.batch()
    assert lo <= b.max_nodes <= hi and (bool(b.flags & SYM) == (listing == "both"))
    got_c = assert_keys(c, b, "closure", f"closure {cls} {listing}")
    got_l = assert_keys(c, b, "listed", f"listed {cls} {listing}")
    simple_once = np.array([ref.simple_once_listing([u for u, _ in e], [v for _, v in e])[0].size == len(e) for _, e, _ in c.graphs])
    assert np.array_equal((got_c == got_l).all(1), simple_once), "both keys are one exactly where the listing is simple and lists every edge once"
    assert simple_once.all() == (listing == "once")


@pytest.mark.parametrize("listing", LISTINGS)
def test_one_batch_of_all_sizes_and_the_forced_kernels(listing):
    """the whole size sweep as ONE batch (W = 8 on graphs of 0 .. 512 nodes); the closure keys of the graphs of at most 64 nodes
    bit-identical through reg, lds and - listed in both directions, flagged - csr; the three listings of a graph share its closure key"""
    full = boundary_cases(listing)
    b = full.batch()
    assert b.max_nodes == 512
    got = assert_keys(full, b, "closure", f"all sizes {listing}")
    assert_keys(full, b, "listed", f"all sizes {listing}, listed")
    ids = [g for g in range(full.n.size) if full.n[g] <= 64]
    small = full.subset(ids)
    sb = small.batch()
    for kernel in ("reg", "lds"):
        again = assert_keys(small, sb, "closure", f"small graphs, {kernel} forced, {listing}", kernel)
        assert np.array_equal(again, got[ids])
    if listing == "both":
        assert (b.flags & SYM) and (sb.flags & SYM)
        assert np.array_equal(assert_keys(small, sb, "closure", "small graphs, csr forced", "csr"), got[ids])
        assert np.array_equal(assert_keys(full, b, "closure", "all sizes, csr forced", "csr"), got)
        assert np.array_equal(assert_keys(full, b, "listed", "listed keys ignore the hook", "csr"), full.want("listed"))
    else:
        assert raw_call(b, full.labels, CLOSURE, "csr")[0] == _lib.E_UNSUPPORTED
    assert raw_call(b, full.labels, CLOSURE, "reg")[0] == _lib.E_UNSUPPORTED      # 512 nodes do not fit the registers
    if listing != "messy":          # (the messy listing adds loops the other two do not have)
        other = boundary_cases("both" if listing == "once" else "once")
        assert np.array_equal(other.want("closure"), full.want("closure"))


# ------------------------------------------------------------------------------------------------ attributes
_ZINC = {}


def zinc_cases():
    if not _ZINC:
        d = gtok.synth.zinc_like(3000, seed=4)
        d["x"][::17] = 300                         # stored as byte 255 ("other")
        d["edge_attr"][::23] = 255
        d["edge_attr"][5::29] = 254
        _ZINC["d"] = d
        nptr, eptr = np.concatenate([[0], np.cumsum(d["node_counts"])]), np.concatenate([[0], np.cumsum(d["edge_counts"])])
        _ZINC["c"] = Cases([(int(d["node_counts"][g]), list(zip(d["src"][eptr[g]:eptr[g + 1]].tolist(), d["dst"][eptr[g]:eptr[g + 1]].tolist())),
                             g % 3, d["x"][nptr[g]:nptr[g + 1]].tolist(), d["edge_attr"][eptr[g]:eptr[g + 1]].tolist()) for g in range(3000)])
    return _ZINC["c"]


def test_listed_keys_with_attributes_on_molecules():
    c = zinc_cases()
    b = c.batch()
    assert (b.flags & SYM) and int((b.nattr == 255).sum()) > 100 and int((b.eattr == 255).sum()) > 100
    with_a = assert_keys(c, b, "listed", "zinc, attributes", attrs=True)
    without = assert_keys(c, b, "listed", "zinc, structure only")
    assert not (with_a == without).all(1).any()
    assert_keys(c, b, "closure", "zinc, closure (csr would do too)")
    assert raw_call(b, c.labels, CLOSURE | ATTRS)[0] == -1
    plain = gtok.GraphBatch.from_coo(c.n, c.ec, c.src, c.dst).to(DEV)
    assert raw_call(plain, c.labels, LISTED | ATTRS)[0] == -1                   # no arrays


# ------------------------------------------------------------------------------------------------ invariance and sensitivity
def _keys_of(graphs, mode="listed", attrs=False):
    c = Cases(graphs)
    return assert_keys(c, c.batch(), mode, "variants", attrs=attrs)


def test_what_changes_a_key_and_what_does_not():
    rng = np.random.default_rng(8)
    base = []
    for f, n in (("tree_chord", 129), ("complete", 65), ("star", 64), ("ring", 300), ("path", 7), ("two_components", 40)):
        e = family_edges(f, n, rng)
        base.append((n, e, 2, rng.integers(0, 9, n).tolist(), rng.integers(0, 5, len(e)).tolist()))
    k0 = _keys_of(base, attrs=True)
    s0 = _keys_of([g[:3] for g in base])

    def variant(fn):
        return [fn(n, list(e), lab, list(x), list(a)) for n, e, lab, x, a in base]

    def permuted(n, e, lab, x, a):
        p = rng.permutation(len(e))
        return (n, [e[i] for i in p], lab, x, [a[i] for i in p])

    def flipped(n, e, lab, x, a):
        return (n, [(v, u) if i % 2 else (u, v) for i, (u, v) in enumerate(e)], lab, x, a)

    assert np.array_equal(_keys_of(variant(permuted), attrs=True), k0), "the order of the entries does not count"
    assert np.array_equal(_keys_of(variant(flipped), attrs=True), k0), "nor their orientation"
    assert np.array_equal(_keys_of([g[:3] for g in variant(flipped)]), s0)
    changes = {
        "one edge changed": lambda n, e, lab, x, a: (n, e[:-1] + [(e[-1][0], (e[-1][1] + 1) % n if (e[-1][1] + 1) % n != e[-1][0] else (e[-1][1] + 2) % n)], lab, x, a),
        "one node more": lambda n, e, lab, x, a: (n + 1, e, lab, x + [x[0]], a),
        "another label": lambda n, e, lab, x, a: (n, e, lab + 1, x, a),
        "one edge byte changed": lambda n, e, lab, x, a: (n, e, lab, x, [a[0] + 1] + a[1:]),
        "one node byte changed": lambda n, e, lab, x, a: (n, e, lab, x[:-1] + [x[-1] + 1], a),
    }
    for what, fn in changes.items():
        k = _keys_of(variant(fn), attrs=True)
        assert (k != k0).any(1).all(), what
        both_words = (k[:, 0] != k0[:, 0]) & (k[:, 1] != k0[:, 1])
        assert both_words.all(), what
    # renumbered (every id moved up by one, the attributes with their nodes and edges): another numbered graph, another key - unless the
    # rotation maps the edge set onto itself, as it does for the complete graph and the ring
    turned = variant(lambda n, e, lab, x, a: (n, [((u + 1) % n, (v + 1) % n) for u, v in e], lab, x[-1:] + x[:-1], a))
    assert (_keys_of([g[:3] for g in turned]) != s0).any(1).tolist() == [True, False, True, False, True, True]
    assert (_keys_of(turned, attrs=True) != k0).any(1).all(), "with attributes the rotated complete graph and ring are other graphs too"
    for what in ("one edge changed", "one node more", "another label"):
        assert (_keys_of([g[:3] for g in variant(changes[what])]) != s0).any(1).all(), what
        assert (_keys_of([g[:3] for g in variant(changes[what])], "closure") != _keys_of([g[:3] for g in base], "closure")).any(1).all(), what


# ------------------------------------------------------------------------------------------------ large graphs
_LARGE = {}


def large_cases():
    if not _LARGE:
        N = _lib.SENT_LARGE_MAX_NODES
        star = [(0, i) for i in range(1, N)]                                          # 16,383 leaves: the centre's row is the whole list
        ring = [(i, i + 1) for i in range(N - 1)] + [(0, N - 1)] + [(i, i + 5000) for i in range(0, N - 5000, 700)]
        mid = [(i, (i + 1) % 700) if i + 1 < 700 else (0, 699) for i in range(700)] + [(i, i + 300) for i in range(0, 400, 50)]
        graphs = [(N, star, 1), (3, [(0, 1), (1, 2), (0, 2)], 0), (N, ring, -7), (700, mid, 4), (600, [], 0)]
        _LARGE["once"] = Cases(graphs)
        _LARGE["both"] = Cases([(n, e + [(v, u) for u, v in e], lab) for n, e, lab in graphs])
    return _LARGE["once"], _LARGE["both"]


def test_large_graphs_flagged_and_not():
    once, both = large_cases()
    bo, bb = once.batch(), both.batch()
    assert bo.max_nodes == bb.max_nodes == _lib.SENT_LARGE_MAX_NODES and not (bo.flags & SYM) and (bb.flags & SYM)
    assert bo.max_degree == _lib.SENT_LARGE_MAX_NODES - 1
    lo = assert_keys(once, bo, "listed", "large graphs listed once")
    assert_keys(both, bb, "listed", "large graphs, both directions")
    cb = assert_keys(both, bb, "closure", "large graphs, closure over the flagged CSR")
    assert np.array_equal(cb, lo), "the closure key is the listed key of the graph listed once"
    assert raw_call(bo, once.labels, CLOSURE)[0] == _lib.E_UNSUPPORTED
    with pytest.raises(_lib.GtokError, match="GTOK_CSR_SIMPLE_SYMMETRIC"):
        gtok.ops.graph_keys(bo, mode="closure")
    # the 700-node graph alone
    m_once, m_both = once.subset([3]), both.subset([3])
    assert raw_call(m_once.batch(), m_once.labels, CLOSURE)[0] == _lib.E_UNSUPPORTED
    assert raw_call(m_both.batch(), m_both.labels, CLOSURE, "lds")[0] == _lib.E_UNSUPPORTED
    assert np.array_equal(assert_keys(m_both, m_both.batch(), "closure", "700 nodes, flagged"), assert_keys(m_once, m_once.batch(), "listed", "700 nodes"))
    big = gtok.GraphBatch.from_coo([_lib.SENT_LARGE_MAX_NODES + 1], [2], [0, 1], [1, 0]).to(DEV)
    assert raw_call(big, None, LISTED)[0] == -2                                     # GTOK_E_TOO_LARGE
    with pytest.raises(_lib.GtokError, match="TOO_LARGE"):
        gtok.ops.graph_keys(big)


# ------------------------------------------------------------------------------------------------ batch shapes, damaged arrays
@pytest.mark.parametrize("G", (1, 3, 5, 257))
def test_batch_shapes(G):
    rng = np.random.default_rng(G)
    graphs = []
    for g in range(G):
        n = int(rng.integers(1, 90))
        k = int(rng.integers(0, 3 * n))
        graphs.append((n, list(zip(rng.integers(0, n, k).tolist(), rng.integers(0, n, k).tolist())), int(rng.integers(-3, 4))))
    graphs[-1] = (0, [], 1)                                                         # the last graph is empty
    c = Cases(graphs)
    b = c.batch()
    for mode in ("listed", "closure"):
        assert_keys(c, b, mode, f"G = {G}, {mode}")
    rc, got, _ = raw_call(b, None, LISTED)                                          # no labels = label 0
    assert rc == 0 and np.array_equal(got, ref.batch_keys(c.n, c.ec, c.src, c.dst))
    small = c.subset([g for g in range(G) if c.n[g] <= 64])
    assert_keys(small, small.batch(), "closure", f"G = {small.n.size}, registers")


def test_damaged_arrays_raise_bit_2_and_touch_nothing_else():
    tri = (3, [(0, 1), (1, 0), (1, 2), (2, 1), (0, 2), (2, 0)], 1)
    good = Cases([tri, (4, [(0, 1), (1, 0), (2, 3), (3, 2)], 2), tri])
    want = {m: good.want(m) for m in MODES}
    empty = ref.batch_keys([0, 0, 0], [0, 0, 0], [], [], good.labels)
    kernels = (("listed", None), ("closure", "reg"), ("closure", "lds"), ("closure", "csr"))
    # a slice beyond max_nodes counts as an empty graph
    b = good.batch()
    assert b.flags & SYM
    b.max_nodes = 2
    for mode, kernel in kernels:
        rc, got, info = raw_call(b, good.labels, MODES[mode], kernel)
        assert rc == 0 and info.tolist() == [2, 3, 0, 0] and np.array_equal(got, empty), (mode, kernel)
    # columns outside the graph are skipped: graph 1 loses (1, 0) and (3, 2)
    b = good.batch()
    b.col[7] = 4
    b.col[9] = -1
    less = Cases([tri, (4, [(0, 1), (2, 3)], 2), tri])
    for mode, kernel in kernels:
        rc, got, info = raw_call(b, good.labels, MODES[mode], kernel)
        assert rc == 0 and info.tolist() == [2, 1, 0, 0], (mode, kernel)
        assert np.array_equal(got[[0, 2]], want[mode][[0, 2]]), "the other graphs' keys are unchanged"
        if kernel != "csr":                 # (the stream over a flagged CSR keeps u < v: (0, 1) and (2, 3) are what is left anyway)
            assert np.array_equal(got[1], less.want(mode)[1]), (mode, kernel)
        else:
            assert np.array_equal(got[1], want[mode][1])
    # a decreasing row pointer: the rows it bounds are skipped
    b = good.batch()
    b.rowptr[4 + 2] = 9                     # graph 1 (rowptr slice starts at 3 + 1): row 1 ends at 9 > E, row 2 starts there
    for mode, kernel in kernels:
        rc, got, info = raw_call(b, good.labels, MODES[mode], kernel)
        assert rc == 0 and info.tolist() == [2, 1, 0, 0], (mode, kernel)
        assert np.array_equal(got[[0, 2]], want[mode][[0, 2]])
        if mode == "listed":                # rows 0 and 3 are left: (0, 1) and (3, 2)
            assert np.array_equal(got[1], less.want("listed")[1])
        if kernel == "csr":                 # ... of which u < v keeps (0, 1)
            assert np.array_equal(got[1], ref.listed_key(4, [0], [1], 2))
    # a damaged edge_ptr: graph 1 is empty, its neighbours are not touched
    b = good.batch()
    b.edge_ptr[2] = 5
    rc, got, info = raw_call(b, good.labels, LISTED)
    assert rc == 0 and info[0] == 2 and info[1] >= 1 and np.array_equal(got[0], want["listed"][0])


# ------------------------------------------------------------------------------------------------ duplicates and leakage
def _dev_batches(sp, names):
    bl = [gtok.GraphBatch.from_coo(sp[s]["node_counts"], sp[s]["edge_counts"], sp[s]["src"], sp[s]["dst"]).to(DEV) for s in names]
    return bl, [torch.from_numpy(sp[s]["labels"]).to(DEV) for s in names]


def _check_against_sets(dup, tups, names=None):
    want = ref.classes([t for ts in tups for t in ts])
    assert np.array_equal(dup.group.cpu().numpy(), want)
    assert np.array_equal(dup.is_first.cpu().numpy(), want == np.arange(want.size))
    uniq, ov = ref.set_report(tups)
    assert dup.unique_per_split().tolist() == uniq and dup.overlap().tolist() == ov
    return uniq, ov


@pytest.mark.parametrize("mode", ("listed", "closure"))
def test_duplicates_and_leakage_of_a_graph_token_train_test_pair(mode):
    sp = ref.tree_splits(gtok.synth.graph_token_tree(40, seed=11, min_nodes=10, max_nodes=30))
    names = ("train", "test")
    bl, labels = _dev_batches(sp, names)
    tups = [ref.batch_tuples(sp[s]["node_counts"], sp[s]["edge_counts"], sp[s]["src"], sp[s]["dst"], sp[s]["labels"], mode, fast=True) for s in names]
    dup = gtok.ops.duplicate_graphs(bl, labels, mode=mode)
    assert dup.group.device == bl[0].device and dup.split.device == bl[0].device
    uniq, ov = _check_against_sets(dup, tups)
    assert ov[0][1] > 0
    quick = gtok.ops.duplicate_graphs(bl, labels, mode=mode, confirm=False)
    assert torch.equal(quick.group, dup.group), "no collision among a few hundred 128-bit keys"
    leaked = dup.leaked(0, 1).cpu().numpy()
    in_train = set(tups[0])
    assert leaked.tolist() == [i for i, t in enumerate(tups[1]) if t in in_train]
    assert set(np.array(sp["test"]["family"])[leaked]) == {"path", "star", "complete"}
    rep = gtok.ops.split_leakage({"train": (bl[0], labels[0]), "test": (bl[1], labels[1])}, mode=mode)
    assert rep["leakage"] and rep["total"] == {"train": 240, "test": 240} and rep["unique"] == {"train": uniq[0], "test": uniq[1]}
    assert rep["overlap"] == {("train", "test"): ov[0][1]}
    ia, ib = rep["example"][("train", "test")]
    assert tups[0][ia] == tups[1][ib] and ib == leaked[0]
    # without labels the same graphs still meet; with every test label moved, nothing leaks
    clean = gtok.ops.split_leakage({"train": (bl[0], labels[0]), "test": (bl[1], labels[1] + 2)}, mode=mode)
    assert not clean["leakage"] and clean["example"] == {("train", "test"): None} and clean["overlap"] == {("train", "test"): 0}
    three = gtok.ops.split_leakage({"train": bl[0], "val": bl[1], "test": bl[0]}, mode=mode)
    assert list(three["overlap"]) == [("train", "val"), ("train", "test"), ("val", "test")]
    assert three["overlap"][("train", "test")] == three["unique"]["train"] == three["unique"]["test"]


_MIX = {}


def _mix():
    if not _MIX:
        d = gtok.synth.mix_batch_device(2000, DEV, seed=3)
        eptr = np.concatenate([[0], np.cumsum(d["edge_counts"])])
        halves = []
        for lo, hi in ((0, 1000), (1000, 2000)):
            halves.append(dict(node_counts=d["node_counts"][lo:hi], edge_counts=d["edge_counts"][lo:hi], src=d["src"][eptr[lo]:eptr[hi]],
                               dst=d["dst"][eptr[lo]:eptr[hi]], family=d["family"][lo:hi]))
        _MIX["halves"] = halves
    return _MIX["halves"]


@pytest.mark.parametrize("mode", ("listed", "closure"))
def test_duplicates_of_a_device_built_mix_split_in_two(mode):
    halves = _mix()
    bl = [gtok.GraphBatch.from_coo(h["node_counts"], h["edge_counts"], h["src"], h["dst"]).to(DEV) for h in halves]
    tups = [ref.batch_tuples(h["node_counts"], h["edge_counts"], h["src"], h["dst"], None, mode, fast=True) for h in halves]
    dup = gtok.ops.duplicate_graphs(bl, mode=mode, budget_bytes=8 << 20)
    uniq, ov = _check_against_sets(dup, tups)
    assert ov[0][1] > 50 and uniq[0] < 1000
    fam = np.array(gtok.synth.MIX_FAMILIES)[halves[1]["family"][dup.leaked(0, 1).cpu().numpy()]]
    assert set(fam) == {"path", "star", "complete"}, "one graph per node count in these families"
    rep = gtok.ops.split_leakage({"a": bl[0], "b": bl[1]}, mode=mode)
    assert rep["overlap"] == {("a", "b"): ov[0][1]} and rep["unique"] == {"a": uniq[0], "b": uniq[1]}
    # keys that say nothing: the confirm path alone still finds the classes of the first half
    sub = bl[0].shard(0, 120)
    same = torch.zeros((120, 2), dtype=torch.int64, device=DEV)
    exact = gtok.ops.duplicate_graphs(sub, mode=mode, keys=same)
    assert np.array_equal(exact.group.cpu().numpy(), ref.classes(tups[0][:120]))


# ------------------------------------------------------------------------------------------------ the Python surfaces
def test_ops_torch_op_and_graph_capture_equal_the_raw_call():
    c = zinc_cases()
    b = c.batch()
    lt = torch.from_numpy(c.labels).to(DEV)
    want = torch.from_numpy(c.want("listed", True).view(np.int64)).to(DEV)
    info = torch.zeros(4, dtype=torch.int32, device=DEV)
    k = gtok.ops.graph_keys(b, lt, attrs=True, info=info)
    assert k.dtype == torch.int64 and tuple(k.shape) == (3000, 2) and torch.equal(k, want) and info.tolist() == [0, 0, 0, 0]
    args = (b.node_ptr, b.edge_ptr, b.rowptr, b.col, b.nattr, b.eattr, b.max_nodes, b.max_edges, b.flags)
    assert torch.equal(torch.ops.gtok.graph_keys(*args, lt, LISTED, True), want)
    wc = torch.from_numpy(c.want("closure").view(np.int64)).to(DEV)
    assert torch.equal(torch.ops.gtok.graph_keys(*args[:4], None, None, *args[6:], lt, CLOSURE, False), wc)
    assert torch.equal(gtok.ops.graph_keys(b, lt, mode="closure"), wc)
    none = torch.ops.gtok.graph_keys(*args, None, LISTED, True)
    assert torch.equal(none, torch.from_numpy(ref.batch_keys(c.n, c.ec, c.src, c.dst, None, "listed", c.x, c.ea).view(np.int64)).to(DEV))
    empty = gtok.GraphBatch.from_coo([], [], [], []).to(DEV)
    assert tuple(gtok.ops.graph_keys(empty).shape) == (0, 2)
    # one launch, nothing read back: captured, then replayed on other labels
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = torch.ops.gtok.graph_keys(*args, lt, LISTED, True)
    lt.copy_(torch.zeros_like(lt))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, none)
    # the fake kernel: shapes without a launch
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode(allow_non_fake_inputs=False) as mode:
        f = lambda x: mode.from_tensor(x)
        ft = torch.ops.gtok.graph_keys(*[f(a) for a in args[:6]], *args[6:], f(lt), LISTED, True)
    assert tuple(ft.shape) == (3000, 2) and ft.dtype == torch.int64


def test_one_ctypes_only_call():
    """the C ABI as a foreign caller uses it: a gtok_csr filled by hand, raw device pointers, the stream NULL"""
    c = Cases([(4, [(0, 1), (1, 2), (2, 3), (3, 0), (1, 1)], 9), (2, [(1, 0)], -1)])
    b = c.batch()
    cs = _lib.GtokCsr()
    cs.num_graphs, cs.max_nodes, cs.max_edges, cs.flags = 2, 4, 5, 0
    cs.node_ptr, cs.edge_ptr, cs.rowptr, cs.col = b.node_ptr.data_ptr(), b.edge_ptr.data_ptr(), b.rowptr.data_ptr(), b.col.data_ptr()
    labels = torch.tensor([9, -1], dtype=torch.int32, device=DEV)
    keys = torch.zeros((2, 2), dtype=torch.int64, device=DEV)
    info = torch.zeros(4, dtype=torch.int32, device=DEV)
    L = ctypes.CDLL(_lib.LIB_PATH)
    L.gtok_graph_keys.restype = ctypes.c_int
    L.gtok_graph_keys.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    for flags, mode in ((0, "listed"), (1, "closure")):
        assert L.gtok_graph_keys(ctypes.addressof(cs), labels.data_ptr(), flags, keys.data_ptr(), info.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(keys.cpu().numpy().view(np.uint64), c.want(mode)) and info.tolist() == [0, 0, 0, 0]
