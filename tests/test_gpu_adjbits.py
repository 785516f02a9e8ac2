"""gtok_csr_adjbits and gtok_csr_pack8 through the bare C ABI, against their statements in include/gtok.h: the adjacency bit-matrix
mirror bit for bit against tests/_degree_graphs.py:adjbits_reference (Python integers and sets, itself checked on the host by
test_host_degree.py), the byte mirror byte for byte against numpy.  Every output sits between 4,096-element guard regions."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _degree_graphs as dg
from _util import both, gtok, orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_lib = gtok._lib
GUARD = 4096
FILL = {torch.int64: 0x5A5A5A5A5A5A5A5A, torch.int32: -77, torch.uint8: 0xAB}
OK, E_INVAL, E_TOO_LARGE = 0, -1, -2


class Guarded:
    """n elements of an output between two guard regions of GUARD elements, all filled with the dtype's FILL value"""

    def __init__(self, n, dtype):
        self.n, self.fill = max(int(n), 0), FILL[dtype]
        self.buf = torch.full((GUARD + self.n + GUARD,), self.fill, dtype=dtype, device=DEV)

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD * self.buf.element_size()

    @property
    def inner(self):
        return self.buf[GUARD:GUARD + self.n]

    def guards_intact(self):
        return bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


def _dev(a, dtype):
    """a host array on the device, never empty (an empty tensor has no address to pass)"""
    a = np.ascontiguousarray(a)
    if a.size == 0:
        a = np.zeros(1, a.dtype)
    return torch.from_numpy(a).to(DEV, dtype=dtype)


class Mirror:
    """One gtok_csr_adjbits call on a batch given in COO form: the CSR is built here entry for entry (columns unchecked, rows as
    unsorted as the list), max_nodes / max_edges are the true maxima unless given."""

    def __init__(self, d, words, max_nodes=None, **fields):
        nc, ec = np.asarray(d["node_counts"], np.int64), np.asarray(d["edge_counts"], np.int64)
        node_ptr, edge_ptr, rowptr, col = dg.csr_arrays(nc, ec, d["src"], d["dst"])
        self.G, self.N, self.W = nc.size, int(nc.sum()), words
        self.keep = [_dev(node_ptr, torch.int32), _dev(edge_ptr, torch.int64), _dev(rowptr, torch.int32), _dev(col, torch.int32)]
        self.rows, self.planes, self.info = Guarded(self.N * words, torch.int64), Guarded(self.G * 8 * words, torch.int64), Guarded(1, torch.int32)
        self.info.inner.zero_()                          # (zeroed by the caller)
        self.cs = _lib.GtokCsr(num_graphs=self.G, max_nodes=int(nc.max()) if max_nodes is None and nc.size else int(max_nodes or 0),
                               max_edges=int(ec.max()) if ec.size else 0, node_ptr=self.keep[0].data_ptr(), edge_ptr=self.keep[1].data_ptr(),
                               rowptr=self.keep[2].data_ptr(), col=self.keep[3].data_ptr())
        for k, v in fields.items():
            setattr(self.cs, k, v)

    def call(self, rows=True, planes=True, info=True):
        p = lambda g, on: g.ptr if on else None
        rc = gtok.lib().gtok_csr_adjbits(ctypes.byref(self.cs), self.W, p(self.rows, rows), p(self.planes, planes), p(self.info, info), None)
        torch.cuda.synchronize()
        return rc

    def guards_intact(self):
        return self.rows.guards_intact() and self.planes.guards_intact() and self.info.guards_intact()

    def outputs_untouched(self):
        return self.rows.untouched() and self.planes.untouched() and self.info.guards_intact() and int(self.info.inner[0]) == 0

    def result(self):
        u64 = lambda g, *shape: g.inner.cpu().numpy().view(np.uint64).reshape(*shape)
        return u64(self.rows, self.N, self.W), u64(self.planes, self.G, 8, self.W), int(self.info.inner[0])


def _check(d, words, what=""):
    """call, compare rows / planes / info[0] with the reference bit for bit, guards intact; returns (rows, planes, max_degree)"""
    m = Mirror(d, words)
    assert m.call() == OK, what
    rows, planes, maxdeg = m.result()
    ref_rows, ref_planes, ref_deg = dg.adjbits_reference(d["node_counts"], d["edge_counts"], d["src"], d["dst"], words)
    assert m.guards_intact(), what
    bad = np.nonzero((rows != ref_rows).any(1))[0]
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first at node {bad[0]}: {rows[bad[0]].tolist()} vs {ref_rows[bad[0]].tolist()}"
    badp = np.argwhere(planes != ref_planes)
    assert badp.size == 0, f"{what}: planes differ first at (graph, plane, word) {badp[0].tolist()}"
    assert maxdeg == ref_deg, what
    return rows, planes, maxdeg


def _relisted(g, how, seed=0):
    """one graph in another listing: `both` / `one` as built, `dup` = every third entry listed again (once as it is, once reversed),
    `shuffled` = the entries in random order (rows unsorted)"""
    rng = np.random.default_rng(seed)
    s, t = g["src"], g["dst"]
    if how == "dup":
        s, t = np.concatenate([s, s[::3], t[1::3]]), np.concatenate([t, t[::3], s[1::3]])
    elif how == "shuffled":
        o = rng.permutation(s.size)
        s, t = s[o], t[o]
    z = np.zeros(s.size, np.int64)
    return dict(g, src=s, dst=t, edge_attr=z, edge_counts=np.array([s.size], np.int64))


# ------------------------------------------------------------------------------------------------ word counts and node limits
@pytest.mark.parametrize("words,top", [(1, 64), (2, 64), (2, 65), (2, 128), (4, 128), (4, 129), (4, 256), (4, 65), (1, 10), (2, 10), (4, 10)])
def test_word_counts_and_node_limits(words, top):
    """batches whose largest graph has exactly `top` nodes - at a word boundary, one past it, and far below what `words` could hold
    (the header allows more words than needed) - with graphs of 0, 1 and 2 nodes between the large ones"""
    small = [dg.empty(0), dg.empty(1), dg.path(2), dg.path(2, True), dg.empty(2)]
    big = [dg.complete(top, True), dg.star(top, top - 1), _relisted(dg.wheel(top, True), "shuffled", 1), dg.sparse(top) if top >= 16 else dg.ring(top),
           _relisted(dg.bipartite(top // 2, top - top // 2), "dup"), dg.path(top - 1), dg.with_self_loop(dg.star(top, 0, True), top - 1)]
    gs = []
    for i, g in enumerate(big):
        gs += [g, small[i % len(small)], small[(i + 2) % len(small)]]
    d = dg.batch_of(*gs)
    assert int(d["node_counts"].max()) == top and d["degree"] == top - 1
    _, _, maxdeg = _check(d, words, f"W={words} top={top}")
    assert maxdeg == top - 1


# ------------------------------------------------------------------------------------------------ listings
@pytest.mark.parametrize("words,n,loops", [(1, 64, (0, 63)), (2, 128, (0, 63, 64, 127)), (4, 256, (0, 63, 64, 255))])
def test_listings_give_one_mirror(words, n, loops):
    """One graph (a wheel with the chords of `sparse`) listed in one direction, in both, with duplicated entries, with unsorted rows and
    with entries whose column lies outside [0, N): the same rows and planes every time.  Self loops on the first and the last node of a
    word set that node's own bit and add one to its degree, nothing else."""
    base = dg.wheel(n)
    extra = dg.sparse(n)
    one = dict(base, src=np.concatenate([base["src"], extra["src"]]), dst=np.concatenate([base["dst"], extra["dst"]]))
    one["edge_counts"] = np.array([one["src"].size], np.int64); one["edge_attr"] = np.zeros(one["src"].size, np.int64)
    both_dirs = dict(one, src=np.concatenate([one["src"], one["dst"]]), dst=np.concatenate([one["dst"], one["src"]]))
    both_dirs["edge_counts"] = np.array([both_dirs["src"].size], np.int64); both_dirs["edge_attr"] = np.zeros(both_dirs["src"].size, np.int64)
    # columns outside the graph: just past the end, far past it, negative - on rows of the first, a middle and the last node
    bad_src = np.array([0, 0, n // 2, n - 1, n - 1, n - 1], np.int64)
    bad_dst = np.array([n, -1, 64 * words, n, 1 << 20, -(1 << 31)], np.int64)
    outside = dict(one, src=np.concatenate([bad_src[:3], one["src"], bad_src[3:]]), dst=np.concatenate([bad_dst[:3], one["dst"], bad_dst[3:]]))
    outside["edge_counts"] = np.array([outside["src"].size], np.int64); outside["edge_attr"] = np.zeros(outside["src"].size, np.int64)
    listings = [one, both_dirs, _relisted(one, "dup"), _relisted(both_dirs, "shuffled", 3), _relisted(one, "shuffled", 4), outside,
                _relisted(outside, "shuffled", 5)]
    d = dg.batch_of(*listings)
    rows, planes, _ = _check(d, words, f"listings W={words}")
    for i in range(1, len(listings)):
        assert np.array_equal(rows[i * n:(i + 1) * n], rows[:n]) and np.array_equal(planes[i], planes[0]), i
    looped = one
    for v in loops:
        looped = dg.with_self_loop(looped, v)
    looped = dg.with_self_loop(looped, loops[0])                       # (listed twice: still one bit, still one more neighbour)
    lr, lp, _ = _check(dg.batch_of(dg.empty(3), looped, dg.path(2)), words, f"self loops W={words}")
    want = rows[:n].copy()
    for v in loops:
        want[v, v >> 6] |= np.uint64(1) << np.uint64(v & 63)
    assert np.array_equal(lr[3:3 + n], want)
    deg = lambda pl, v: sum(((int(pl[p, v >> 6]) >> (v & 63)) & 1) << p for p in range(8))
    for v in range(n):
        assert deg(lp[1], v) == (deg(planes[0], v) + (v in loops)) % 256, v          # (the 256-node wheel's hub: 255 + 1 reads 0)


# ------------------------------------------------------------------------------------------------ LDS reuse
def test_a_wave_takes_k256_then_a_path_then_k200_then_an_empty_graph():
    """A wave keeps one matrix in LDS and zeroes n x W words per graph.  At W = 4 a workgroup has 2 waves and the grid stops at 2,048
    workgroups, so wave 0 of workgroup 0 takes graphs 0, 4096, 8192 and 12288: K256, a 3-node path, K200 and an empty graph sit there,
    the 12,285 graphs between them have 1 or 2 nodes (what a stale word of K256 would show up in)."""
    stride = 2048 * 2
    fill = [dg.empty(1), dg.path(2), dg.path(2, True), dg.with_self_loop(dg.empty(1), 0)]
    gs = [fill[i % 4] for i in range(3 * stride + 1)]
    gs[0], gs[stride], gs[2 * stride], gs[3 * stride] = dg.complete(256), dg.path(3), dg.complete(200, True), dg.empty(0)
    gs[1], gs[stride + 1] = dg.complete(256, True), dg.empty(2)          # (the neighbouring wave: K256, then two isolated nodes)
    d = dg.batch_of(*gs)
    assert d["node_counts"].size == 12289
    rows, planes, maxdeg = _check(d, 4, "K256 / P3 / K200 / empty on one wave")
    assert maxdeg == 255
    nptr = np.concatenate([[0], np.cumsum(d["node_counts"])])
    p3 = rows[nptr[stride]:nptr[stride] + 3]
    assert p3.tolist() == [[2, 0, 0, 0], [5, 0, 0, 0], [2, 0, 0, 0]] and planes[stride, :, :].tolist() == [[0b101, 0, 0, 0], [0b010, 0, 0, 0]] + [[0] * 4] * 6
    assert not planes[3 * stride].any() and not rows[nptr[stride + 1]:nptr[stride + 1] + 2].any()


@functools.lru_cache(maxsize=None)
def _second_round_batch():
    full = [dg.complete(8), dg.complete(8, True), dg.complete(12), dg.complete(5, True)]
    one = lambda n, a, b: dict(dg.empty(n), edge_counts=np.array([1], np.int64), src=np.array([a], np.int64), dst=np.array([b], np.int64),
                               edge_attr=np.zeros(1, np.int64), degree=1)
    single = [one(8, 7, 0), one(12, 3, 11), one(5, 4, 4), one(2, 0, 1), one(9, 8, 2)]
    return dg.batch_of(*([full[i % 4] for i in range(8192)] + [single[i % 5] for i in range(640)]))


@pytest.mark.parametrize("words", [1, 2])
def test_every_wave_takes_a_second_graph(words):
    """8,832 tiny graphs at 4 waves per workgroup and 2,048 workgroups: graphs 8192 .. 8831 are second graphs of waves whose first had
    full rows (K5, K8, K12); they have one edge each, in graphs smaller than, as large as and larger than the wave's first."""
    d = _second_round_batch()
    rows, planes, maxdeg = _check(d, words, f"second round W={words}")
    assert maxdeg == 11
    n0 = int(d["node_counts"][:8192].sum())
    bits = np.array([bin(int(w)).count("1") for w in rows[n0:, 0]])
    assert bits.sum() == 2 * 640 - 128 and not rows[n0:, 1:].any()         # (every fifth is a self loop: one bit)


# ------------------------------------------------------------------------------------------------ degrees at the plane edges
def _hub_graph(n, hub, degree):
    """n nodes, `hub` joined to the first `degree` other nodes (entries listed from the lower id)"""
    others = [v for v in range(n) if v != hub][:degree]
    g = dg.star(n, hub)
    keep = np.isin(g["src"], others) | np.isin(g["dst"], others)
    return dict(g, src=g["src"][keep], dst=g["dst"][keep], edge_attr=g["edge_attr"][keep], edge_counts=np.array([int(keep.sum())], np.int64),
                degree=degree)


@pytest.mark.parametrize("words,n,degrees,hubs", [(1, 64, (15, 16, 63), (0, 31, 63)), (2, 128, (15, 16, 127), (0, 63, 64, 127)),
                                                    (4, 256, (15, 16, 127, 128, 255), (0, 63, 64, 255))])
def test_hub_degrees_at_the_plane_edges(words, n, degrees, hubs):
    """hubs of degree 15 | 16 (4 planes | more), 127 | 128 (plane 7) and 255 (every plane), sitting at the first node, at either side of
    a word boundary and at the last node: plane p holds bit p of the hub's degree at the hub's bit of the hub's word, the leaves hold 1"""
    cases = [(h, k) for k in degrees for h in hubs]
    d = dg.batch_of(*[_hub_graph(n, h, k) for h, k in cases])
    assert d["degree"] == max(degrees)
    rows, planes, maxdeg = _check(d, words, f"hubs W={words}")
    assert maxdeg == max(degrees)
    for g, (h, k) in enumerate(cases):
        leaves = [v for v in range(n) if v != h][:k]
        for p in range(8):
            want = [0] * words
            if (k >> p) & 1:
                want[h >> 6] |= 1 << (h & 63)
            if p == 0:
                for v in leaves:
                    want[v >> 6] |= 1 << (v & 63)
            assert planes[g, p].tolist() == want, (h, k, p)
        assert bin(int.from_bytes(rows[g * n + h].tobytes(), "little")).count("1") == k


def test_degree_256_is_reported_and_refused(monkeypatch):
    """K256 with a self loop: info[0] == 256, the rows are the reference's, the planes hold the degree modulo 256 (as the reference
    states).  ops.adjbits answers False for the batch; ops.sent marks it adj_unusable, walks it with another kernel, and the tokens
    are the oracle's."""
    for both_dirs in (False, True):
        d = dg.batch_of(dg.path(4), dg.LIMIT_GRAPHS["K256_loop"][0](both_dirs), dg.ring(5))
        assert d["degree"] == 256
        rows, planes, maxdeg = _check(d, 4, "K256 + self loop")
        assert maxdeg == 256
        deg = [sum(((int(planes[1, p, v >> 6]) >> (v & 63)) & 1) << p for p in range(8)) for v in range(256)]
        assert deg == [255] * 255 + [0] and int(rows[4 + 255, 3]) >> 63 == 1
    # (listed once: both directions of K256 are 65,280 entries, more than gtok_sent stages)
    batch, coo = both(dg.batch_of(dg.path(4), dg.LIMIT_GRAPHS["K256_loop"][0](False), dg.ring(5)), False)
    b = batch.to(DEV)
    assert gtok.ops.adjbits(b) is False and b.adj_rows is None and b.adj_planes is None
    monkeypatch.setenv("GTOK_SENT_KERNEL", "blane")
    for max_len in (4096, 100):
        fresh = batch.to(DEV)
        ids, ln = gtok.ops.sent(fresh, 256, max_len, 7, 1)
        assert fresh.adj_unusable and fresh.adj_rows is None and gtok.ops.last_sent_kernel() == "sent_lds_kernel<W=4>", gtok.ops.last_sent_kernel()
        ref, rln = orc.sent(coo, 256, max_len, 7, 1, ld=ids.shape[1])
        assert np.array_equal(ln.cpu().numpy(), rln) and np.array_equal(ids.cpu().numpy(), ref)
        assert rln[1] == max_len
        again, _ = gtok.ops.sent(fresh, 256, max_len, 7, 1)              # (not tried again: still no mirror, same rows)
        assert fresh.adj_rows is None and torch.equal(again, ids)


# ------------------------------------------------------------------------------------------------ error codes
def test_adjbits_error_codes_beyond_the_abi_test():
    d = dg.batch_of(dg.star(65, 64), dg.path(3))
    m = Mirror(d, 1)
    assert m.call() == E_TOO_LARGE and m.outputs_untouched()                        # max_nodes 65 > 64 x 1
    for words, maxn in ((1, 65), (2, 129), (4, 257)):
        m = Mirror(d, words, max_nodes=maxn)
        assert m.call() == E_TOO_LARGE and m.outputs_untouched(), words
    spare = torch.zeros(8, dtype=torch.int32, device=DEV)
    for field in ("graph_ids", "unit_ptr"):                                         # a reordered batch
        m = Mirror(d, 2, **{field: spare.data_ptr()})
        assert m.call() == E_INVAL and m.outputs_untouched(), field
    m = Mirror(d, 2)
    m.cs.num_graphs = 0                                                             # no graphs: OK, nothing written
    assert m.call() == OK and m.outputs_untouched()
    assert m.call(rows=False, planes=False, info=False) == OK
    m.cs.num_graphs = -1
    assert m.call() == E_INVAL and m.outputs_untouched()
    for off in ("rows", "planes", "info"):                                          # a NULL output with graphs present
        m = Mirror(d, 2)
        assert m.call(**{off: False}) == E_INVAL and m.outputs_untouched(), off
    for field in ("node_ptr", "edge_ptr", "rowptr", "col"):                         # a NULL input
        m = Mirror(d, 2, **{field: None})
        assert m.call() == E_INVAL and m.outputs_untouched(), field
    m = Mirror(d, 2)
    assert m.call() == OK and m.guards_intact() and m.result()[2] == 64             # (the same batch is fine as it stands)


# ------------------------------------------------------------------------------------------------ gtok_csr_pack8
def _pack8(rowptr, col, num_rowptr, num_col, max_nodes=256, max_edges=255, null_inputs=False, null_outputs=False):
    r_in, c_in = _dev(rowptr, torch.int32), _dev(col, torch.int32)
    r8, c8 = Guarded(num_rowptr, torch.uint8), Guarded(num_col, torch.uint8)
    cs = _lib.GtokCsr(num_graphs=1, max_nodes=max_nodes, max_edges=max_edges, rowptr=None if null_inputs else r_in.data_ptr(),
                      col=None if null_inputs else c_in.data_ptr())
    rc = gtok.lib().gtok_csr_pack8(ctypes.byref(cs), num_rowptr, num_col, None if null_outputs else r8.ptr, None if null_outputs else c8.ptr, None)
    torch.cuda.synchronize()
    return rc, r8, c8


def _values(n, seed):
    """n int32 values in 0 .. 255 with both ends present wherever there is room"""
    v = np.random.default_rng(seed).integers(0, 256, n).astype(np.int32)
    if n >= 1:
        v[-1] = 255
    if n >= 2:
        v[0] = 0
    if n >= 6:
        v[n - 5:n - 1] = [255, 254, 128, 127]
    return v


TAILS = [(nr, nc) for nr in (0, 1, 2, 3, 4, 5, 6, 7) for nc in (0, 1, 2, 3, 4)] + \
        [(1024 + k, 2052 - k) for k in range(4)] + [(5, 4 * 256 * 4096 + 4 + 3), (4 * 256 * 4096 + 8 + 1, 2)]


@pytest.mark.parametrize("nr,nc", TAILS)
def test_pack8_every_tail_of_both_arrays(nr, nc):
    """n & 3 = 0 .. 3 for the two arrays independently, none at all, more than one workgroup, and more 16-byte pieces than the
    4,096-workgroup grid has threads (the grid-stride loop): every byte is the low byte of its int32, nothing around them is touched"""
    rowptr, col = _values(nr, 1), _values(nc, 2)
    rc, r8, c8 = _pack8(rowptr, col, nr, nc)
    assert rc == OK
    assert np.array_equal(r8.inner.cpu().numpy(), rowptr.astype(np.uint8)) and np.array_equal(c8.inner.cpu().numpy(), col.astype(np.uint8))
    assert r8.guards_intact() and c8.guards_intact()


def test_pack8_null_pointers_sizes_and_limits():
    rc, r8, c8 = _pack8(np.zeros(0, np.int32), np.zeros(0, np.int32), 0, 0, null_inputs=True, null_outputs=True)
    assert rc == OK                                                                  # nothing to pack: NULL pointers are allowed
    v = _values(9, 3)
    rc, r8, c8 = _pack8(v, v, 9, 0, null_outputs=False)
    assert rc == OK and np.array_equal(r8.inner.cpu().numpy(), v.astype(np.uint8)) and c8.untouched()
    for kw in (dict(max_edges=256), dict(max_nodes=257), dict(max_edges=256, max_nodes=257)):
        rc, r8, c8 = _pack8(v, v, 9, 9, **kw)
        assert rc == E_TOO_LARGE and r8.untouched() and c8.untouched(), kw           # before anything is written
    rc, r8, c8 = _pack8(v, v, 9, 9, max_edges=255, max_nodes=256)
    assert rc == OK and r8.guards_intact() and c8.guards_intact()
    for kw in (dict(null_inputs=True), dict(null_outputs=True)):
        rc, r8, c8 = _pack8(v, v, 9, 9, **kw)
        assert rc == E_INVAL and r8.untouched() and c8.untouched(), kw
    rc, r8, c8 = _pack8(v, v, -1, 9)
    assert rc == E_INVAL and c8.untouched()
