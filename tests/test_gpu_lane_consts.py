"""The constants mirror of sent_lane_kernel (gtok_sent_lane_consts / gtok_sent_prepared): the device builder against the numpy
restatement of tests/test_host_lane_consts.py, and the walk that stages the mirror (type bytes emitted as tokens) against the walk
without it (GTOK_NO_LANE_CONSTS=1) and against the oracle - molecules whose types take all three remap ranges, dense graphs
on the 32- and the 64-bit node sets with the sizes and degrees at which the kernel switches paths - through every row flavour,
the fallbacks (a token beyond a byte, an unlabelled or un-remapped call), a second settings key, and the C entry point's refusals."""
import ctypes

import numpy as np
import pytest
import torch

from _util import both, gtok, orc
from test_host_lane_consts import tok8_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KW = dict(labeled=True, num_node_types=9, num_edge_types=4, remap_zinc=True)


def _ring_chords(n, chord_frac, rng):
    pairs = {(min(i, (i + 1) % n), max(i, (i + 1) % n)) for i in range(n)} if n > 2 else ({(0, 1)} if n == 2 else set())
    want = min(n + int(chord_frac * n), 127, n * (n - 1) // 2)
    while len(pairs) < want:
        a, b = sorted(rng.integers(0, n, 2).tolist())
        if a != b:
            pairs.add((a, b))
    return pairs


def _corpus(graphs, seed):
    """[(nodes, set of undirected pairs)] -> symmetric, row-sorted, typed COO (node types 0..27, entry types 0..4: every remap range)."""
    rng = np.random.default_rng(seed)
    ncs, ecs, srcs, dsts = [], [], [], []
    for n, pairs in graphs:
        e = np.array(sorted(pairs), np.int64).reshape(-1, 2)
        s = np.concatenate([e[:, 0], e[:, 1]]); t = np.concatenate([e[:, 1], e[:, 0]])
        o = np.lexsort((t, s))
        ncs.append(n); ecs.append(s.size); srcs.append(s[o]); dsts.append(t[o])
    src, dst = np.concatenate(srcs), np.concatenate(dsts)
    return dict(node_counts=np.array(ncs), edge_counts=np.array(ecs), src=src, dst=dst,
                x=rng.integers(0, 28, int(np.sum(ncs))), edge_attr=(np.minimum(src, dst) + np.maximum(src, dst)) % 5)


def _star(leaves):
    return leaves + 1, {(0, i) for i in range(1, leaves + 1)}


def _dense32():
    rng = np.random.default_rng(52)
    g = [(n, _ring_chords(n, 1.5, rng)) for n in [30, 32, 28, 31] * 16 + [20, 18, 24, 16] * 16]
    # exactly 32 nodes (above), one node, an isolated node beside a ring, a row of degree 15 (the last one 4 counter planes hold)
    g += [(1, set()), (11, _ring_chords(10, 0.0, rng)), _star(15)]
    return _corpus(g, 53)


def _dense64():
    rng = np.random.default_rng(62)
    g = [(n, _ring_chords(n, 0.9, rng)) for n in [64, 60, 50, 40] * 12 + [36, 34, 40, 33] * 12 + [20, 12, 25, 8] * 12]
    g += [(33, _ring_chords(33, 0.5, rng)), (64, _ring_chords(64, 0.2, rng)), (1, set()), (7, _ring_chords(6, 0.5, rng)), _star(16)]   # degree 16: six planes
    return _corpus(g, 63)


CORPORA = {
    "zinc": (lambda: gtok.synth.zinc_like(3000, seed=41), 37),
    "dense32": (_dense32, 32),
    "dense64": (_dense64, 64),
}
_made = {}


def _get(name):
    """(device batch, oracle corpus, max_num_nodes) of a corpus, made once and shared by the tests (read only)."""
    if name not in _made:
        gen, nn = CORPORA[name]
        batch, coo = both(gen(), True)
        _made[name] = (batch.to(DEV), coo, nn)
    return _made[name]


def _rows(ids, ln):
    ids, ln = ids.cpu(), ln.cpu().numpy()
    if ids.dtype == torch.int16:
        ids = ids.to(torch.int32) & 0xFFFF
    return ids.numpy(), ln


def _cmp(got, ref, what, upto_len=False):
    (ids, ln), (rids, rln) = got, ref
    assert np.array_equal(ln, rln), f"{what}: lengths differ at {np.nonzero(ln != rln)[0][:5]}"
    if upto_len:       # rows written up to their length only
        inside = np.arange(ids.shape[-1])[None, :] < np.minimum(ln, ids.shape[-1])[:, None]
        ids, rids = np.where(inside, ids, 0), np.where(inside, rids, 0)
    bad = np.nonzero((ids != rids).any(-1))[0]
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[0]}: {ids[bad[0], :40].tolist()} vs {rids[bad[0], :40].tolist()}"


def _walk(b, nn, max_len, consts, monkeypatch, **kw):
    """ops.sent with or without the mirror; asserts that the launch says which one ran."""
    if consts:
        monkeypatch.delenv("GTOK_NO_LANE_CONSTS", raising=False)
    else:
        monkeypatch.setenv("GTOK_NO_LANE_CONSTS", "1")
    args = dict(KW); args.update(kw)
    ids, ln = gtok.ops.sent(b, nn, max_len, 5, 2, **args)
    assert gtok.ops.last_sent_kernel() == "sent_lane_kernel" and gtok.ops.last_sent_consts() == consts, \
        (gtok.ops.last_sent_kernel(), gtok.ops.last_sent_consts())
    return ids, ln


@pytest.mark.parametrize("name", list(CORPORA))
def test_builder_equals_the_restatement(name, monkeypatch):
    monkeypatch.setenv("GTOK_SENT_KERNEL", "lane")
    b, _, nn = _get(name)
    sb = gtok.ops.lane_sorted(b)
    assert sb is not None and sb.graph_ids is not None
    nat, eat = sb.nattr.cpu().numpy(), sb.eattr.cpu().numpy()
    assert nat.max() == 27 and eat.max() == 4 and nat.min() == 0 and eat.min() == 0      # all three ranges of both formulas
    for key in ((nn, 9, 4), (64, 28, 5), (200, 9, 4), (201, 9, 4)):
        kc = gtok.ops.lane_consts(sb, *key)
        ntok, etok, st = tok8_reference(nat, eat, *key)
        assert kc["status"] == st and (kc["consts"] is None) == bool(st), key
        assert np.array_equal(kc["ntok8"].cpu().numpy(), (ntok & 255).astype(np.uint8)), key
        assert np.array_equal(kc["etok8"].cpu().numpy(), (etok & 255).astype(np.uint8)), key
    # the edge of a byte on this corpus: node type 27 under max_num_nodes 200 is token 255, under 201 it is 256
    assert gtok.ops.lane_consts(sb, 200, 9, 4)["status"] == 0 and gtok.ops.lane_consts(sb, 201, 9, 4)["status"] == 1
    assert gtok.ops.lane_consts(sb, nn, 9, 4) is gtok.ops.lane_consts(sb, nn, 9, 4)       # one per key, kept on the batch
    assert gtok.ops.lane_consts(b, nn, 9, 4) is None                                      # the batch in dataset order has none


@pytest.mark.parametrize("name", list(CORPORA))
def test_walk_with_constants_equals_walk_without_and_the_oracle(name, monkeypatch):
    monkeypatch.setenv("GTOK_SENT_KERNEL", "lane")
    b, coo, nn = _get(name)
    G = b.num_graphs
    for max_len in (4096, 61, 30):
        ref = None
        for consts in (True, False):
            ids, ln = _walk(b, nn, max_len, consts, monkeypatch)
            if ref is None:
                ref = orc.sent(coo, nn, max_len, 5, 2, ld=ids.shape[1], **KW)
            _cmp(_rows(ids, ln), ref, f"{name} max_len={max_len} consts={consts}")
    sb = b.lane_sorted
    sizes = (sb.node_ptr[1:] - sb.node_ptr[:-1]).cpu().numpy()
    units = (sb.unit_ptr[1:] - sb.unit_ptr[:-1]).cpu().numpy()
    assert units[-1] < 64 and units.size >= 2                      # a last unit of fewer than 64 graphs
    if name == "dense32":
        assert sizes.max() == 32 and sizes.min() == 1 and sb.max_degree == 15        # 32-bit node sets throughout, four counter planes
    if name == "dense64":
        assert {33, 64, 1} <= set(sizes.tolist()) and sb.max_degree == 16            # six counter planes
    keys = set(sb.lane_consts)
    ld = gtok.ops.sent_safe_ld(b, True, 4096)
    # two epochs in one launch; rows of 16-bit ids; rows without padding; a query tail - each with and without the mirror
    refs2 = [orc.sent(coo, nn, 4096, 5, 2 + e, ld=ld, **KW) for e in range(2)]
    rng = np.random.default_rng(7)
    nc = np.maximum(coo.node_counts, 1)
    q = np.stack([rng.integers(0, nc), rng.integers(0, nc)], 1).astype(np.int32)
    refq = orc.sent(coo, nn, 4096, 5, 2, ld=ld + 3, query=q, **KW)
    for consts in (True, False):
        i2, l2 = _walk(b, nn, 4096, consts, monkeypatch, epochs=2, ld=ld)
        u2, m2 = _walk(b, nn, 4096, consts, monkeypatch, epochs=2, u16=True, ld=ld)
        for e in range(2):
            _cmp(_rows(i2[e], l2[e]), refs2[e], f"{name} epoch slice {e} consts={consts}")
            _cmp(_rows(u2[e], m2[e]), refs2[e], f"{name} 16-bit rows, epoch slice {e} consts={consts}")
        out = (torch.full((G, ld), -7, dtype=torch.int32, device=DEV), torch.empty(G, dtype=torch.int32, device=DEV))
        _walk(b, nn, 4096, consts, monkeypatch, pad=False, ld=ld, out=out)
        _cmp(_rows(*out), refs2[0], f"{name} pad=False consts={consts}", upto_len=True)
        iq, lq = _walk(b, nn, 4096, consts, monkeypatch, query=torch.from_numpy(q), ld=ld + 3)
        _cmp(_rows(iq, lq), refq, f"{name} query tail consts={consts}")
    assert set(sb.lane_consts) == keys and (nn, 9, 4) in keys          # every flavour through the ONE set of its settings


def test_fallbacks_run_without_constants_and_say_so(monkeypatch):
    monkeypatch.setenv("GTOK_SENT_KERNEL", "lane")
    monkeypatch.delenv("GTOK_NO_LANE_CONSTS", raising=False)
    b, coo, nn = _get("zinc")

    def run(batch, c, mnn, used, **kw):
        args = dict(KW); args.update(kw)
        ids, ln = gtok.ops.sent(batch, mnn, 1024, 5, 2, **args)
        assert gtok.ops.last_sent_kernel() == "sent_lane_kernel" and gtok.ops.last_sent_consts() == used, (mnn, kw, gtok.ops.last_sent_consts())
        _cmp(_rows(ids, ln), orc.sent(c, mnn, 1024, 5, 2, ld=ids.shape[1], **args), f"max_num_nodes={mnn} {kw}")

    # an attribute byte of 255: its token does not fit a byte
    d = gtok.synth.zinc_like(3000, seed=41)
    d["x"] = np.array(d["x"]).copy(); d["x"][17] = 255
    b255, coo255 = both(d, True)
    b255 = b255.to(DEV)
    run(b255, coo255, 37, False)
    assert b255.lane_sorted.lane_consts[(37, 9, 4)]["status"] == 1
    # max_num_nodes = 200: node type 27 is token 255 - the largest that fits, the mirror is used; at 201 it is 256 and the walk goes without
    run(b, coo, 200, True)
    run(b, coo, 201, False)
    # an unlabelled call (the batch carries attributes, the call ignores them), and a labelled one without the remap
    run(b, coo, 37, False, labeled=False, num_node_types=0, num_edge_types=0, remap_zinc=False)
    run(b, coo, 37, False, remap_zinc=False)
    run(b, coo, 37, True)


def test_second_settings_key_and_the_c_entry_point(monkeypatch):
    monkeypatch.setenv("GTOK_SENT_KERNEL", "lane")
    monkeypatch.delenv("GTOK_NO_LANE_CONSTS", raising=False)
    d = gtok.synth.zinc_like(3000, seed=41)
    batch, coo = both(d, True)
    b = batch.to(DEV)
    for nnt in (9, 28):
        kw = dict(KW, num_node_types=nnt)
        ids, ln = gtok.ops.sent(b, 37, 1024, 5, 2, **kw)
        assert gtok.ops.last_sent_consts()
        _cmp(_rows(ids, ln), orc.sent(coo, 37, 1024, 5, 2, ld=ids.shape[1], **kw), f"num_node_types={nnt}")
    sb = b.lane_sorted
    assert set(sb.lane_consts) == {(37, 9, 4), (37, 28, 4)}
    # ---- the C ABI alone: build a mirror, walk with it, and the launcher's refusals
    L, _lib = gtok.lib(), gtok._lib
    N, E, G = sb.num_nodes_total, sb.num_edges_total, sb.num_graphs
    nt, et = torch.zeros(N + 16, dtype=torch.uint8, device=DEV), torch.zeros(E + 16, dtype=torch.uint8, device=DEV)
    st = torch.full((1,), 99, dtype=torch.int32, device=DEV)
    cs, plain = sb.c_struct(), b.c_struct()
    p = gtok.ops._sent_params(37, 1024, True, 9, 4, True, seed=5, epoch=2)
    assert L.gtok_sent_lane_consts(ctypes.byref(cs), ctypes.byref(p), N, E, nt.data_ptr(), et.data_ptr(), st.data_ptr(), None) == 0
    assert int(st.item()) == 0 and torch.equal(nt[:N], sb.lane_consts[(37, 9, 4)]["ntok8"]) and torch.equal(et[:E], sb.lane_consts[(37, 9, 4)]["etok8"])
    assert L.gtok_sent_lane_consts(ctypes.byref(plain), ctypes.byref(p), N, E, nt.data_ptr(), et.data_ptr(), st.data_ptr(), None) == -1   # not a reordered batch
    ld = ids.shape[1]
    out, oln = torch.empty((G, ld), dtype=torch.int32, device=DEV), torch.empty(G, dtype=torch.int32, device=DEV)
    call = lambda c_, p_, k_: L.gtok_sent_prepared(ctypes.byref(c_), ctypes.byref(p_), None if k_ is None else ctypes.byref(k_),
                                                   out.data_ptr(), ld, oln.data_ptr(), None)
    k = _lib.GtokSentConsts(nt.data_ptr(), et.data_ptr(), 37, 9, 4, 0)
    ref = orc.sent(coo, 37, 1024, 5, 2, ld=ld, **KW)
    for kk in (k, None):          # consts == NULL is gtok_sent
        out.fill_(-1)
        assert call(cs, p, kk) == 0
        _cmp(_rows(out, oln), ref, "gtok_sent_prepared" + ("" if kk is not None else " (no constants)"))
    out.fill_(-3)
    for mnn, nnt, net in ((38, 9, 4), (37, 28, 4), (37, 9, 5)):      # recorded settings that differ from p
        assert call(cs, p, _lib.GtokSentConsts(nt.data_ptr(), et.data_ptr(), mnn, nnt, net, 0)) == -1
    assert call(cs, p, _lib.GtokSentConsts(None, et.data_ptr(), 37, 9, 4, 0)) == -1
    assert call(cs, p, _lib.GtokSentConsts(nt.data_ptr(), et.data_ptr(), 37, 9, 4, 1)) == -1
    assert call(plain, p, k) == -1                                                             # not the lane kernel's reordered batch
    assert call(cs, gtok.ops._sent_params(37, 1024, True, 9, 4, False, seed=5, epoch=2), k) == -1    # no remap: nothing to look up
    assert call(cs, gtok.ops._sent_params(37, 1024, False, 9, 4, False, seed=5, epoch=2), k) == -1
    torch.cuda.synchronize()
    assert bool((out == -3).all())                                                             # a refusal launches nothing
