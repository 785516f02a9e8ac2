"""sent_lane_kernel's two step-body fast paths against the oracle, each next to its general fallback: the bracket list (every
lane of the wave with at most one member: one append; a second member anywhere: the min-search loop) and the pick (every
active lane's choice set with <= 4 bits: clear-lowest steps; more anywhere: the prefix-popcount search).  Molecules take the
fast paths nearly always; dense ring-and-chord graphs of <= 32 and of 33-64 nodes (the 32- and 64-bit node sets) force
brackets of two, three, four and more members and large choice sets, in the same launches as steps that stay on the fast paths."""
import numpy as np
import pytest
import torch

from _util import both, gtok, orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDX, LADJ, RADJ = 6, 2, 3      # include/gtok.h: GTOK_SENT_IDX_OFFSET, GTOK_SENT_LADJ, GTOK_SENT_RADJ


def _dense(sizes, chord_frac, seed):
    """Symmetric ring + chords graphs (both directions listed, row-sorted, typed), <= 254 entries each."""
    rng = np.random.default_rng(seed)
    ncs, ecs, srcs, dsts = [], [], [], []
    for n in sizes:
        pairs = {(min(i, (i + 1) % n), max(i, (i + 1) % n)) for i in range(n)}
        want = min(n + int(chord_frac * n), 127, n * (n - 1) // 2)
        while len(pairs) < want:
            a, b = sorted(rng.integers(0, n, 2).tolist())
            if a != b:
                pairs.add((a, b))
        e = np.array(sorted(pairs), np.int64).reshape(-1, 2)
        s = np.concatenate([e[:, 0], e[:, 1]]); t = np.concatenate([e[:, 1], e[:, 0]])
        o = np.lexsort((t, s))
        ncs.append(n); ecs.append(s.size); srcs.append(s[o]); dsts.append(t[o])
    src, dst = np.concatenate(srcs), np.concatenate(dsts)
    return dict(node_counts=np.array(ncs), edge_counts=np.array(ecs), src=src, dst=dst,
                x=rng.integers(0, 9, int(np.sum(ncs))), edge_attr=np.minimum(src, dst) % 4)


def _bracket_sizes(ids, ln, num_nodes):
    """Members of every bracket in unremapped rows (position tokens between LADJ and RADJ)."""
    out = []
    for r in range(ids.shape[0]):
        row, k = ids[r, :ln[r]], None
        for t in row.tolist():
            if t == LADJ:
                k = 0
            elif t == RADJ and k is not None:
                out.append(k); k = None
            elif k is not None and IDX <= t < IDX + num_nodes:
                k += 1
    return np.array(out)


def _cmp(ids, ln, ref, rln, what):
    ids, ln = ids.cpu().numpy(), ln.cpu().numpy()
    assert np.array_equal(ln, rln), f"{what}: lengths differ at {np.nonzero(ln != rln)[0][:5]}"
    bad = np.nonzero((ids != ref).any(1))[0]
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[0]}: {ids[bad[0], :40].tolist()} vs {ref[bad[0], :40].tolist()}"


CORPORA = [
    ("zinc", lambda: gtok.synth.zinc_like(3000, seed=41), 37, 1),
    # 32-bit node sets: a unit of dense graphs every fourth unit, molecule-sized sparse ones between
    ("dense32", lambda: _dense(([30, 32, 28, 31] * 16 + [20, 18, 24, 16] * 48) * 3, 1.5, seed=42), 32, 4),
    # 64-bit node sets: 33-64 nodes, dense and sparse units
    ("dense64", lambda: _dense(([64, 60, 50, 40] * 16 + [36, 34, 40, 33] * 16) * 3, 0.9, seed=43), 64, 4),
]


@pytest.mark.parametrize("pin", ["lane", "lane-int32", "lane-unsorted"])
@pytest.mark.parametrize("name,gen,nn,min_big", CORPORA, ids=[c[0] for c in CORPORA])
def test_lane_bracket_and_pick_fast_paths_against_the_oracle(pin, name, gen, nn, min_big, monkeypatch):
    monkeypatch.setenv("GTOK_SENT_KERNEL", "lane")
    for var, on in (("GTOK_NO_PACK8", pin == "lane-int32"), ("GTOK_NO_LANE_SORT", pin == "lane-unsorted")):
        if on:
            monkeypatch.setenv(var, "1")
        else:
            monkeypatch.delenv(var, raising=False)
    d = gen()
    for labeled in (True, False):
        batch, coo = both(d, labeled)
        kw = dict(labeled=labeled, num_node_types=9 if labeled else 0, num_edge_types=4 if labeled else 0)
        # the corpus takes both sides of the bracket test: brackets of 2 and 3 members, and of 4 or more where min_big > 1
        raw, rraw = orc.sent(coo, nn, 4096, 5, 2, ld=None, **kw)
        sizes = _bracket_sizes(raw, rraw, nn)
        assert (sizes >= 2).any() and (sizes == 3).any()
        if min_big > 1:
            assert (sizes >= min_big).sum() > 20, np.bincount(sizes)
        b = batch.to(DEV)
        for remap in ((False, True) if labeled else (False,)):
            for max_len in (4096, 61, 30):
                ids, ln = gtok.ops.sent(b, nn, max_len, 5, 2, remap_zinc=remap, **kw)
                assert gtok.ops.last_sent_kernel() == "sent_lane_kernel", gtok.ops.last_sent_kernel()
                ref, rln = orc.sent(coo, nn, max_len, 5, 2, ld=ids.shape[1], remap_zinc=remap, **kw)
                _cmp(ids, ln, ref, rln, f"{name} [{pin}] labeled={labeled} remap={remap} max_len={max_len}")
        # rows of 16-bit ids, two epochs per launch (the U16 instantiations share the body)
        i16, l16 = gtok.ops.sent(b, nn, 4096, 5, 0, epochs=2, u16=True, **kw)
        for e in range(2):
            ref, rln = orc.sent(coo, nn, 4096, 5, e, ld=i16.shape[2], **kw)
            _cmp(i16[e].to(torch.int32) & 0xFFFF, l16[e], ref, rln, f"{name} [{pin}] u16 epoch {e} labeled={labeled}")
