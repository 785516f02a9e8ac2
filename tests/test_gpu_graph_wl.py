"""gtok_graph_wl (include/gtok.h) on the device: keys AND node colours of every kernel - closure rows in registers, the bit matrix in
LDS (W = 2, 4, 8), the pull over the CSR rows with its tables in LDS and in the workspace, with and without attributes - bit-equal to
the numpy restatement (tests/_graph_wl_ref.py), which tests/test_host_graph_wl.py holds against an exact refinement and networkx.
Then what the key is for: the graphs decoded from the token rows of several epochs keep the keys of the graphs that were walked,
while their numbered keys do not, and ops.unique_novel finds exactly the edited graphs of a decoded batch.  Every comparison is
exact; every raw launch of this file writes its keys, colours, info and workspace between guard regions."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _graph_wl_ref as ref
from _util import gtok
from test_gpu_graph_tasks import FAMILIES, LISTINGS, family_edges, listed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_lib = gtok._lib
SYM, ATTRS = _lib.CSR_SIMPLE_SYMMETRIC, _lib.WL_ATTRS
GUARD, SENTINEL = 64, -77
SIZES = (0, 1, 2, 63, 64, 65, 128, 129, 256, 257, 512)          # both sides of every kernel's limits
R = 3


# ------------------------------------------------------------------------------------------------ graphs
class Cases:
    """a list of (n, [(u, v)], label[, x, entry bytes]) -> batched COO, the batch, and (once per rounds / attrs) the reference"""

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
        self.nptr = np.concatenate([[0], np.cumsum(self.n)])
        self._want = {}

    def subset(self, keep):
        c = Cases([self.graphs[g] for g in keep])
        for k, (keys, colors) in self._want.items():               # the reference runs once
            c._want[k] = (keys[keep], np.concatenate([colors[self.nptr[g]:self.nptr[g + 1]] for g in keep] + [np.zeros(0, np.uint64)]))
        return c

    def want(self, rounds=R, attrs=False):
        k = (rounds, attrs)
        if k not in self._want:
            self._want[k] = ref.batch_wl(self.n, self.ec, self.src, self.dst, rounds, self.labels, self.x if attrs else None,
                                         self.ea if attrs else None)
        return self._want[k]

    def batch(self):
        return gtok.GraphBatch.from_coo(self.n, self.ec, self.src, self.dst, self.x, self.ea).to(DEV)


_CASES = {}


def boundary_cases(listing):
    """every family at every size (the complete graph up to 256 nodes), listed one way, labels -1 .. 3 (kept for the session)"""
    if listing not in _CASES:
        rng, same_trees = np.random.default_rng(10 + LISTINGS.index(listing)), np.random.default_rng(9)
        graphs = []
        for n in SIZES:
            for f in FAMILIES:
                if f == "complete" and n > 256:
                    continue
                k = len(graphs)
                graphs.append((n, listed(family_edges(f, n, same_trees), n, listing, rng, loops=k % 2 == 0), k % 5 - 1))
        _CASES[listing] = Cases(graphs)
    return _CASES[listing]


# ------------------------------------------------------------------------------------------------ guarded launches
class Guarded:
    def __init__(self, n, dtype, fill=SENTINEL):
        self.n, self.fill = n, fill
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        self.view = self.buf[GUARD:GUARD + n]

    def check(self, what):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == self.fill).all() and (b[GUARD + self.n:] == self.fill).all(), f"{what}: a guard region was written"
        return b[GUARD:GUARD + self.n]


def raw_call(batch, labels, rounds, flags=0, kernel=None, colors=True):
    """gtok_graph_wl through ctypes alone, everything it writes between guard regions -> (rc, keys uint64 [G, 2], colours uint64 [N]
    (SENTINEL where nothing was written), info [4])"""
    G, N = batch.num_graphs, batch.num_nodes_total
    keys, col, info = Guarded(2 * G, torch.int64), Guarded(N, torch.int64), Guarded(4, torch.int32)
    info.view.zero_()
    need = int(_lib.lib().gtok_graph_wl_workspace(min(batch.max_nodes, _lib.SENT_LARGE_MAX_NODES), G))
    ws = Guarded(need, torch.uint8, 0x5A) if need > 0 else None     # (16-byte aligned: the allocation is, and GUARD is 64 bytes)
    lt = None if labels is None else torch.from_numpy(np.ascontiguousarray(labels, np.int32)).to(DEV)
    old = os.environ.pop("GTOK_WL_KERNEL", None)
    if kernel:
        os.environ["GTOK_WL_KERNEL"] = kernel
    try:
        cs = batch.c_struct()
        rc = _lib.lib().gtok_graph_wl(ctypes.byref(cs), None if lt is None else lt.data_ptr(), rounds, flags, keys.view.data_ptr(),
                                      col.view.data_ptr() if colors else None, info.view.data_ptr(), None if ws is None else ws.view.data_ptr(),
                                      need, None)
        torch.cuda.synchronize()
    finally:
        os.environ.pop("GTOK_WL_KERNEL", None)
        if old is not None:
            os.environ["GTOK_WL_KERNEL"] = old
    if ws is not None:
        ws.check("workspace")
    return rc, keys.check(f"keys (kernel={kernel})").view(np.uint64).reshape(G, 2), col.check("colours").view(np.uint64), info.check("info")


def assert_wl(cases, batch, what, rounds=R, attrs=False, kernel=None):
    rc, keys, colors, info = raw_call(batch, cases.labels, rounds, ATTRS if attrs else 0, kernel)
    assert rc == 0, (what, rc)
    wk, wc = cases.want(rounds, attrs)
    bad = np.nonzero((keys != wk).any(1))[0]
    assert bad.size == 0, f"{what}: keys differ at graphs {bad[:8]} (nodes {cases.n[bad[:8]]})"
    badc = np.nonzero(colors != wc)[0]
    assert badc.size == 0, f"{what}: colours differ at nodes {badc[:8]}"
    assert info.tolist() == [0, 0, 0, 0], what
    return keys, colors


# ------------------------------------------------------------------------------------------------ reg and lds at their sizes
SLICES = {"reg": (0, 64), "lds2": (65, 128), "lds4": (129, 256), "lds8": (257, 512)}


@pytest.mark.parametrize("listing", LISTINGS)
@pytest.mark.parametrize("cls", sorted(SLICES))
def test_keys_and_colours_equal_the_restatement_at_each_kernels_sizes(listing, cls):
    """a batch whose max_nodes selects the kernel (<= 64 registers, <= 128 / 256 / 512 the LDS matrix with W = 2 / 4 / 8)"""
    full = boundary_cases(listing)
    full.want()
    lo, hi = SLICES[cls]
    c = full.subset([g for g in range(full.n.size) if lo <= full.n[g] <= hi])
    b = c.batch()
    assert lo <= b.max_nodes <= hi and set(c.n.tolist()) == {n for n in SIZES if lo <= n <= hi}
    assert_wl(c, b, f"{cls} {listing}")
    rc, keys, colors, _ = raw_call(b, None, R, colors=False)               # no labels = label 0, no colours asked for
    lab0 = c.labels == 0
    assert rc == 0 and np.array_equal(keys[lab0], c.want()[0][lab0]) and (keys[~lab0] != c.want()[0][~lab0]).all()
    assert (colors.view(np.int64) == SENTINEL).all()


@pytest.mark.parametrize("listing", LISTINGS)
def test_one_mixed_batch_under_every_kernel_that_can_hold_it(listing):
    """the whole size sweep as ONE batch (W = 8 on graphs of 0 .. 512 nodes); the graphs of at most 64 nodes through reg, lds and -
    listed in both directions, flagged - csr: one answer; a forced kernel that cannot hold the batch answers GTOK_E_UNSUPPORTED"""
    full = boundary_cases(listing)
    b = full.batch()
    assert b.max_nodes == 512
    keys, colors = assert_wl(full, b, f"all sizes {listing}")
    assert np.array_equal(assert_wl(full, b, "lds forced", kernel="lds")[0], keys)
    ids = [g for g in range(full.n.size) if full.n[g] <= 64]
    small = full.subset(ids)
    sb = small.batch()
    for kernel in ("reg", "lds"):
        assert np.array_equal(assert_wl(small, sb, f"small graphs, {kernel} forced, {listing}", kernel=kernel)[0], keys[ids])
    if listing == "both":
        assert (b.flags & SYM) and (sb.flags & SYM)
        assert np.array_equal(assert_wl(small, sb, "small graphs, csr forced", kernel="csr")[0], keys[ids])
        k2, c2 = assert_wl(full, b, "all sizes, csr forced", kernel="csr")
        assert np.array_equal(k2, keys) and np.array_equal(c2, colors)
    else:
        assert raw_call(b, full.labels, R, kernel="csr")[0] == _lib.E_UNSUPPORTED
        assert raw_call(sb, small.labels, R, kernel="csr")[0] == _lib.E_UNSUPPORTED
    rc, k, c, info = raw_call(b, full.labels, R, kernel="reg")                 # 512 nodes do not fit the registers
    assert rc == _lib.E_UNSUPPORTED and (k.view(np.int64) == SENTINEL).all() and (c.view(np.int64) == SENTINEL).all() and not info.any()


def test_the_listings_of_a_graph_share_its_key_and_a_loop_changes_it():
    once, both, messy = (boundary_cases(l) for l in LISTINGS)
    assert np.array_equal(once.want()[0], both.want()[0]) and np.array_equal(once.want()[1], both.want()[1])
    rng = np.random.default_rng(2)
    graphs = []
    for n, f in ((40, "tree_chord"), (64, "ring"), (100, "tree_chord"), (300, "two_components")):
        e = family_edges(f, n, rng)
        dup = [e[i] for i in rng.integers(0, len(e), 9)]
        graphs += [(n, e, 1), (n, e + [(v, u) for u, v in e], 1), (n, [(v, u) for u, v in dup] + e[::-1] + dup, 1), (n, e + [(n // 2, n // 2)], 1)]
    for keep in (range(8), range(16)):                                      # max_nodes 64: reg; 300: lds
        c = Cases([graphs[i] for i in keep])
        keys, colors = assert_wl(c, c.batch(), "listings")
        for g in range(0, len(c.graphs), 4):
            assert np.array_equal(keys[g], keys[g + 1]) and np.array_equal(keys[g], keys[g + 2]), "once, both directions, messy"
            assert (keys[g + 3] != keys[g]).all(), "a loop changes the key"
            n0, n1 = c.nptr[g], c.nptr[g + 1]
            assert np.array_equal(colors[n0:n1], colors[n1:2 * n1 - n0])


# ------------------------------------------------------------------------------------------------ the pull over the CSR rows
def _both(e):
    return e + [(v, u) for u, v in e]


def _ring_chords(n, step):
    return [(i, i + 1) for i in range(n - 1)] + [(0, n - 1)] + [(i, i + n // 3) for i in range(0, n - n // 3, step)]


_LARGE = {}


def large_cases(n):
    """a path, a star (the centre's row is the whole list), a ring with a few chords and a small graph, flagged, with attribute bytes"""
    if n not in _LARGE:
        rng = np.random.default_rng(n)
        graphs = []
        for k, e in enumerate(([(i, i + 1) for i in range(n - 1)], [(0, i) for i in range(1, n)], _ring_chords(n, n // 7), [(0, 1), (1, 2), (0, 2)])):
            nn = 3 if k == 3 else n
            und = rng.integers(0, 4, len(e)).tolist()
            graphs.append((nn, _both(e), k - 1, rng.integers(0, 5, nn).tolist(), und + [(t + k) % 4 for t in und]))
        _LARGE[n] = Cases(graphs)
    return _LARGE[n]


@pytest.mark.parametrize("n", (513, 4096, 4097))
def test_csr_path_with_its_tables_in_lds_and_in_the_workspace(n):
    """513 and 4,096 nodes: two 8-byte tables per node in LDS (64 KB at 4,096: one wave per workgroup); 4,097: in the workspace, whose
    guard regions stay as they were.  Structure only and with attributes (each direction's own byte)."""
    c = large_cases(n)
    b = c.batch()
    assert b.max_nodes == n and (b.flags & SYM) and b.max_degree == n - 1
    assert (_lib.lib().gtok_graph_wl_workspace(n, 4) > 0) == (n > 4096)
    plain, _ = assert_wl(c, b, f"{n} nodes, structure only")
    with_a, _ = assert_wl(c, b, f"{n} nodes, attributes", attrs=True)
    assert (plain != with_a).all()
    assert raw_call(b, c.labels, R, kernel="lds")[0] == _lib.E_UNSUPPORTED
    unflagged = gtok.GraphBatch.from_coo(c.n, c.ec, c.src, c.dst, c.x, c.ea, check_symmetric=False).to(DEV)
    for flags in (0, ATTRS):
        assert raw_call(unflagged, c.labels, R, flags)[0] == _lib.E_UNSUPPORTED
    with pytest.raises(_lib.GtokError, match="GTOK_CSR_SIMPLE_SYMMETRIC"):
        gtok.ops.graph_wl_keys(unflagged)


def test_one_graph_of_16384_nodes():
    N = _lib.SENT_LARGE_MAX_NODES
    c = Cases([(N, _both(_ring_chords(N, 1500)), 5)])
    b = c.batch()
    assert b.max_nodes == N and (b.flags & SYM)
    assert_wl(c, b, "16,384 nodes")
    k, col = gtok.ops.graph_wl_keys(b, R, torch.tensor([5], dtype=torch.int32, device=DEV), with_colors=True)      # the module's workspace
    assert np.array_equal(k.cpu().numpy().view(np.uint64), c.want()[0]) and np.array_equal(col.cpu().numpy().view(np.uint64), c.want()[1])
    big = gtok.GraphBatch.from_coo([N + 1], [2], [0, 1], [1, 0]).to(DEV)
    assert raw_call(big, None, R)[0] == -2                                        # GTOK_E_TOO_LARGE
    with pytest.raises(_lib.GtokError, match="TOO_LARGE"):
        gtok.ops.graph_wl_keys(big)


# ------------------------------------------------------------------------------------------------ renumbering
def test_a_renumbered_copy_has_the_key_and_the_colours_follow_the_nodes():
    rng = np.random.default_rng(12)
    base = [(30, "tree_chord"), (64, "two_components"), (100, "tree_chord"), (300, "ring"), (257, "star"), (129, "tree_chord")]
    graphs, perms = [], []
    for n, f in base:
        e = family_edges(f, n, rng)
        perm, s2, d2, _, _ = ref.renumbered(rng, n, [u for u, _ in e], [v for _, v in e])
        graphs += [(n, e, 0), (n, list(zip(s2.tolist(), d2.tolist())), 0)]
        perms.append(perm)
    for keep, what in ((range(4), "reg"), (range(12), "lds")):
        c = Cases([graphs[i] for i in keep])
        keys, colors = assert_wl(c, c.batch(), what)
        for g in range(0, len(c.graphs), 2):
            assert np.array_equal(keys[g], keys[g + 1]), (what, g)
            a, p = colors[c.nptr[g]:c.nptr[g + 1]], colors[c.nptr[g + 1]:c.nptr[g + 2]]
            assert np.array_equal(p[perms[g // 2]], a), "colors_perm[perm[v]] == colors[v]"
    # the same through the pull over the rows: both directions listed, flagged
    c = Cases([(n, _both(e), lab) for n, e, lab in graphs])
    b = c.batch()
    assert b.flags & SYM
    keys, _ = assert_wl(c, b, "csr", kernel="csr")
    assert np.array_equal(keys[0::2], keys[1::2])


# ------------------------------------------------------------------------------------------------ attributes
_ZINC = {}


def zinc_cases(G=600, seed=4):
    if (G, seed) not in _ZINC:
        d = gtok.synth.zinc_like(G, seed=seed)
        d["x"][::17] = 300                         # stored as byte 255 ("other")
        d["edge_attr"][5::29] = 254
        nptr, eptr = np.concatenate([[0], np.cumsum(d["node_counts"])]), np.concatenate([[0], np.cumsum(d["edge_counts"])])
        _ZINC[(G, seed)] = (d, Cases([(int(d["node_counts"][g]), list(zip(d["src"][eptr[g]:eptr[g + 1]].tolist(), d["dst"][eptr[g]:eptr[g + 1]].tolist())),
                                       g % 3, d["x"][nptr[g]:nptr[g + 1]].tolist(), d["edge_attr"][eptr[g]:eptr[g + 1]].tolist()) for g in range(G)]))
    return _ZINC[(G, seed)]


def test_attributes_on_molecules_and_what_one_byte_changes():
    d, c = zinc_cases()
    b = c.batch()
    assert (b.flags & SYM) and int((b.nattr == 255).sum()) > 20
    with_a, _ = assert_wl(c, b, "zinc, attributes", attrs=True)
    plain, _ = assert_wl(c, b, "zinc, structure only (reg)")
    assert np.array_equal(assert_wl(c, b, "zinc, structure only (csr)", kernel="csr")[0], plain)
    assert not (with_a == plain).all(1).any()
    assert raw_call(b, c.labels, R, ATTRS, kernel="reg")[0] == _lib.E_UNSUPPORTED
    bare = gtok.GraphBatch.from_coo(c.n, c.ec, c.src, c.dst).to(DEV)
    assert raw_call(bare, c.labels, R, ATTRS)[0] == -1                                # no arrays
    # one node byte, then one entry byte, of every third molecule
    nptr, eptr = b.node_ptr.cpu().numpy(), b.edge_ptr.cpu().numpy()
    hit = np.arange(0, 600, 3)
    for arr, ptr in ((b.nattr, nptr), (b.eattr, eptr)):
        saved = arr.clone()
        arr[torch.from_numpy(ptr[hit]).to(DEV)] += 1
        b.nattr = b.nattr                                                             # (drops the cached C struct)
        rc, keys, _, info = raw_call(b, c.labels, R, ATTRS)
        changed = (keys != with_a).all(1)
        assert rc == 0 and not info.any() and changed[hit].all() and not changed[np.setdiff1d(np.arange(600), hit)].any()
        arr.copy_(saved)
    assert np.array_equal(raw_call(b, c.labels, R, ATTRS)[1], with_a)


# ------------------------------------------------------------------------------------------------ the point of the feature
def _int64(keys):
    return torch.from_numpy(np.ascontiguousarray(keys).view(np.int64)).to(DEV)


def test_decoded_graphs_keep_the_wl_key_of_the_graphs_that_were_walked():
    """K = 3 epochs of SENT walks, decoded: every decoded graph is numbered in visit-index space, another numbering every epoch - its WL
    key is its input graph's all the same (structure; with attributes for the molecules), its numbered key is not; nothing of a decoded
    batch is novel against its input, and of a batch with a few edited graphs exactly those are"""
    kw = dict(labeled=True, num_node_types=28, num_edge_types=4)
    d = gtok.synth.zinc_like(120, seed=31)
    mols = gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], d["x"], d["edge_attr"]).to(DEV)
    t = gtok.synth.graph_token_like(60, seed=32, min_nodes=10, max_nodes=40, task=None, with_text=False)
    toks = gtok.GraphBatch.from_coo(t["node_counts"], t["edge_counts"], t["src"], t["dst"]).to(DEV)
    want_m, want_ma = gtok.ops.graph_wl_keys(mols, R), gtok.ops.graph_wl_keys(mols, R, attrs=True)
    want_t = gtok.ops.graph_wl_keys(toks, R)
    num_m, num_t = gtok.ops.graph_keys(mols, mode="closure"), gtok.ops.graph_keys(toks, mode="closure")
    moved_m = moved_t = 0
    for epoch in range(3):
        ids, ln = gtok.ops.sent(mols, 37, 4096, 5, epoch, remap_zinc=True, **kw)
        dec, st = gtok.ops.sent_decode_zinc_csr(ids, ln, 37, 28, check_symmetric=True)
        assert not st.any() and (dec.flags & SYM) and torch.equal(dec.node_ptr, mols.node_ptr)
        assert torch.equal(gtok.ops.graph_wl_keys(dec, R), want_m), epoch
        assert torch.equal(gtok.ops.graph_wl_keys(dec, R, attrs=True), want_ma), epoch
        moved_m += int((gtok.ops.graph_keys(dec, mode="closure") != num_m).any(1).sum())
        ids, ln = gtok.ops.sent(toks, 40, 1 << 16, 5, epoch)
        dect, st = gtok.ops.sent_decode_csr(ids, ln, 40)
        assert not st.any() and torch.equal(dect.node_ptr, toks.node_ptr)
        assert torch.equal(gtok.ops.graph_wl_keys(dect, R), want_t), epoch
        moved_t += int((gtok.ops.graph_keys(dect, mode="closure") != num_t).any(1).sum())
    assert moved_m > 100 and moved_t > 50, "the numbered keys of decoded graphs are not their input graphs'"
    for attrs in (False, True):
        out = gtok.ops.unique_novel(dec, [mols], rounds=0, attrs=attrs)
        assert out["novel"].device.type == "cuda" and int(out["num_novel"]) == 0 and not out["novel"].any()
    assert int(gtok.ops.unique_novel(dect, toks)["num_novel"]) == 0
    # a few edited molecules: another atom type on one node
    edited = [3, 40, 41, 119]
    saved = dec.nattr.clone()
    dec.nattr[dec.node_ptr[torch.tensor(edited, device=DEV)].long()] = 27
    dec.nattr = dec.nattr
    assert not bool((saved[dec.node_ptr[torch.tensor(edited, device=DEV)].long()] == 27).any())
    out = gtok.ops.unique_novel(dec, [mols], rounds=0, attrs=True)
    assert out["novel"].nonzero().reshape(-1).tolist() == edited and int(out["num_novel"]) == 4
    assert int(gtok.ops.unique_novel(dec, [mols], rounds=0)["num_novel"]) == 0, "structure only: the edit does not show"
    # uniqueness is that of the decoded batch alone
    alone = gtok.ops.isomorphic_duplicates(dec, rounds=0, attrs=True)
    assert torch.equal(out["unique"], alone.is_first) and int(out["num_unique"]) == int(alone.is_first.sum())


# ------------------------------------------------------------------------------------------------ rounds
def test_rounds_zero_is_as_many_rounds_as_the_graph_has_nodes():
    rng = np.random.default_rng(14)
    graphs = [(n, family_edges(f, n, rng), 0) for n, f in ((0, "path"), (1, "path"), (7, "path"), (40, "tree_chord"), (64, "ring"), (33, "star"))]
    for keep, what in ((range(6), "reg"), (None, "lds")):
        gs = [graphs[i] for i in keep] if keep is not None else graphs + [(130, family_edges("path", 130, rng), 0), (512, family_edges("path", 512, rng), 0)]
        c = Cases(gs)
        b = c.batch()
        k0, c0 = assert_wl(c, b, f"rounds = 0, {what}", rounds=0)
        for g, (n, _, _) in enumerate(gs):
            if n == 0:
                continue
            rc, kn, cn, _ = raw_call(b, c.labels, n)
            assert rc == 0 and np.array_equal(kn[g], k0[g]) and np.array_equal(cn[c.nptr[g]:c.nptr[g + 1]], c0[c.nptr[g]:c.nptr[g + 1]]), (what, n)
    # a 512-node path is told apart end to end only after ~N / 2 rounds
    path = Cases([(512, family_edges("path", 512, rng), 0)])
    _, c3 = assert_wl(path, path.batch(), "path, 3 rounds")
    _, call = assert_wl(path, path.batch(), "path, N rounds", rounds=0)
    assert np.unique(c3).size == 5 and np.unique(call).size == 256
    # flagged small graphs through the csr kernel
    sym = Cases([(n, _both(e), lab) for n, e, lab in graphs])
    assert_wl(sym, sym.batch(), "rounds = 0, csr", rounds=0, kernel="csr")


def test_rounds_outside_their_range_write_nothing():
    c = large_cases(513)
    b = c.batch()
    for rounds, flags, want in ((0, 0, _lib.E_UNSUPPORTED), (0, ATTRS, _lib.E_UNSUPPORTED), (513, 0, -1), (-1, 0, -1)):
        rc, keys, colors, info = raw_call(b, c.labels, rounds, flags)
        assert rc == want and (keys.view(np.int64) == SENTINEL).all() and (colors.view(np.int64) == SENTINEL).all() and not info.any(), rounds
    with pytest.raises(_lib.GtokError, match="rounds=0"):
        gtok.ops.graph_wl_keys(b, 0)
    with pytest.raises(ValueError, match="rounds"):
        gtok.ops.graph_wl_keys(b, 513)
    small = boundary_cases("once").subset([8, 9])
    assert raw_call(small.batch(), small.labels, 512)[0] == 0                     # the largest round count


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
    assert_wl(c, c.batch(), f"G = {G}, lds")
    small = c.subset([g for g in range(G) if c.n[g] <= 64])
    assert_wl(small, small.batch(), f"G = {small.n.size}, registers")
    sym = Cases([(n, _both(sorted({(min(u, v), max(u, v)) for u, v in e if u != v})), lab) for n, e, lab in graphs])
    sb = sym.batch()
    if sb.flags & SYM:
        assert_wl(sym, sb, f"G = {G}, csr", kernel="csr")


def test_damaged_arrays_raise_bit_2_and_touch_nothing_else():
    tri = (3, [(0, 1), (1, 0), (1, 2), (2, 1), (0, 2), (2, 0)], 1)
    good = Cases([tri, (4, [(0, 1), (1, 0), (2, 3), (3, 2)], 2), tri])
    wk, wc = good.want()
    empty = ref.batch_wl([0, 0, 0], [0, 0, 0], [], [], R, good.labels)[0]
    kernels = ("reg", "lds", "csr")
    # a slice beyond max_nodes counts as an empty graph and gets no colours
    b = good.batch()
    assert b.flags & SYM
    b.max_nodes = 2
    for kernel in kernels:
        rc, keys, colors, info = raw_call(b, good.labels, R, kernel=kernel)
        assert rc == 0 and info.tolist() == [2, 3, 0, 0] and np.array_equal(keys, empty) and (colors.view(np.int64) == SENTINEL).all(), kernel
    # columns outside the graph are skipped: graph 1 loses (1, 0) and (3, 2)
    b = good.batch()
    b.col[7] = 4
    b.col[9] = -1
    less = Cases([tri, (4, [(0, 1), (2, 3)], 2), tri])
    for kernel in kernels:
        rc, keys, colors, info = raw_call(b, good.labels, R, kernel=kernel)
        assert rc == 0 and info.tolist() == [2, 1, 0, 0], kernel
        assert np.array_equal(keys[[0, 2]], wk[[0, 2]]) and np.array_equal(colors[:3], wc[:3]) and np.array_equal(colors[7:], wc[7:])
        if kernel != "csr":                 # (the closure of what is left is the same graph; the pull reads each row as it stands)
            assert np.array_equal(keys[1], less.want()[0][1]) and np.array_equal(keys[1], wk[1]), kernel
    # a decreasing row pointer: the rows it bounds are skipped
    b = good.batch()
    b.rowptr[4 + 2] = 9                     # graph 1 (rowptr slice starts at 3 + 1): row 1 ends at 9 > E, row 2 starts there
    for kernel in kernels:
        rc, keys, colors, info = raw_call(b, good.labels, R, kernel=kernel)
        assert rc == 0 and info.tolist() == [2, 1, 0, 0], kernel
        assert np.array_equal(keys[[0, 2]], wk[[0, 2]]) and np.array_equal(colors[:3], wc[:3]) and np.array_equal(colors[7:], wc[7:])
        if kernel != "csr":                 # rows 0 and 3 are left: (0, 1) and (3, 2), the same closure again
            assert np.array_equal(keys[1], wk[1])
    # a damaged edge_ptr: graph 1 is empty, its neighbours are not touched
    b = good.batch()
    b.edge_ptr[2] = 5
    rc, keys, colors, info = raw_call(b, good.labels, R)
    assert rc == 0 and info[0] == 2 and info[1] >= 1 and np.array_equal(keys[0], wk[0]) and np.array_equal(colors[:3], wc[:3])
    # attributes, a damaged column: the byte of a skipped entry is not read either
    d, zc = zinc_cases()
    zb = zc.batch()
    zb.col[0] = 1 << 20
    rc, keys, _, info = raw_call(zb, zc.labels, R, ATTRS)
    assert rc == 0 and info.tolist() == [2, 1, 0, 0] and np.array_equal(keys[1:], zc.want(R, True)[0][1:])


# ------------------------------------------------------------------------------------------------ the Python surfaces
def test_ops_torch_op_and_graph_capture_equal_the_raw_call():
    d, c = zinc_cases()
    b = c.batch()
    lt = torch.from_numpy(c.labels).to(DEV)
    wk, wc = (_int64(a) for a in c.want(R, True))
    info = torch.zeros(4, dtype=torch.int32, device=DEV)
    k, col = gtok.ops.graph_wl_keys(b, R, lt, attrs=True, with_colors=True, info=info)
    assert k.dtype == col.dtype == torch.int64 and tuple(k.shape) == (600, 2) and torch.equal(k, wk) and torch.equal(col, wc) and info.tolist() == [0, 0, 0, 0]
    assert torch.equal(gtok.ops.graph_wl_keys(b, R, lt, attrs=True), wk)
    args = (b.node_ptr, b.edge_ptr, b.rowptr, b.col, b.nattr, b.eattr, b.max_nodes, b.max_edges, b.flags)
    tk, tc = torch.ops.gtok.graph_wl_keys(*args, lt, R, True)
    assert torch.equal(tk, wk) and torch.equal(tc, wc)
    sk, sc = (_int64(a) for a in c.want())
    tk, tc = torch.ops.gtok.graph_wl_keys(*args[:4], None, None, *args[6:], lt, R, False)
    assert torch.equal(tk, sk) and torch.equal(tc, sc) and torch.equal(gtok.ops.graph_wl_keys(b, labels=lt), sk)
    none = torch.ops.gtok.graph_wl_keys(*args, None, R, True)[0]
    assert torch.equal(none, _int64(ref.batch_wl(c.n, c.ec, c.src, c.dst, R, None, c.x, c.ea)[0]))
    empty = gtok.GraphBatch.from_coo([], [], [], []).to(DEV)
    assert tuple(gtok.ops.graph_wl_keys(empty).shape) == (0, 2)
    # one launch, nothing read back: captured, then replayed on other labels
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, outc = torch.ops.gtok.graph_wl_keys(*args, lt, R, True)
    lt.copy_(torch.zeros_like(lt))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, none) and torch.equal(outc, wc)
    # the fake kernel: shapes without a launch
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode(allow_non_fake_inputs=False) as mode:
        f = lambda x: mode.from_tensor(x)
        fk, fc = torch.ops.gtok.graph_wl_keys(*[f(a) for a in args[:6]], *args[6:], f(lt), R, True)
    assert tuple(fk.shape) == (600, 2) and tuple(fc.shape) == (b.num_nodes_total,) and fk.dtype == fc.dtype == torch.int64
    # the classes of a batch beside a renumbered copy of itself, on the device: what isomorphic_duplicates adds on top
    dup = gtok.ops.isomorphic_duplicates([b, b], rounds=0, attrs=True)
    first = ref.classes([tuple(r) for r in ref.batch_wl(c.n, c.ec, c.src, c.dst, 0, None, c.x, c.ea)[0].tolist()])
    assert np.array_equal(dup.group.cpu().numpy(), np.concatenate([first, first])) and dup.proven.device.type == "cuda"
    assert dup.overlap().tolist() == [[len(set(first.tolist()))] * 2] * 2 and 0 < int(dup.proven[600:].sum()) < 600


def test_one_ctypes_only_call():
    """the C ABI as a foreign caller uses it: a gtok_csr filled by hand, raw device pointers, the stream NULL"""
    c = Cases([(4, [(0, 1), (1, 2), (2, 3), (3, 0), (1, 1)], 9), (2, [(1, 0)], -1)])
    b = c.batch()
    cs = _lib.GtokCsr()
    cs.num_graphs, cs.max_nodes, cs.max_edges, cs.flags = 2, 4, 5, 0
    cs.node_ptr, cs.edge_ptr, cs.rowptr, cs.col = b.node_ptr.data_ptr(), b.edge_ptr.data_ptr(), b.rowptr.data_ptr(), b.col.data_ptr()
    labels = torch.tensor([9, -1], dtype=torch.int32, device=DEV)
    keys = torch.zeros((2, 2), dtype=torch.int64, device=DEV)
    colors = torch.zeros(6, dtype=torch.int64, device=DEV)
    info = torch.zeros(4, dtype=torch.int32, device=DEV)
    L = ctypes.CDLL(_lib.LIB_PATH)
    L.gtok_graph_wl.restype = ctypes.c_int
    L.gtok_graph_wl.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    L.gtok_graph_wl_workspace.restype = ctypes.c_int64
    L.gtok_graph_wl_workspace.argtypes = [ctypes.c_int32, ctypes.c_int32]
    assert L.gtok_graph_wl_workspace(4, 2) == 0
    for rounds in (R, 0):
        assert L.gtok_graph_wl(ctypes.addressof(cs), labels.data_ptr(), rounds, 0, keys.data_ptr(), colors.data_ptr(), info.data_ptr(), None, 0, None) == 0
        torch.cuda.synchronize()
        wk, wc = c.want(rounds)
        assert np.array_equal(keys.cpu().numpy().view(np.uint64), wk) and np.array_equal(colors.cpu().numpy().view(np.uint64), wc) and info.tolist() == [0, 0, 0, 0]
