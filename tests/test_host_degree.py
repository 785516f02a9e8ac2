"""The yardsticks of the degree-limit tests, established without a GPU: on every graph family instance that test_gpu_degree.py and
test_gpu_adjbits.py use, the C oracle equals the plain-Python walk of DESIGN.md §5 (tests/_sent_walk_ref.py) token for token, the
uncut lengths are the recorded ones, the builders' stated degrees are the true ones, and the numpy statement of the adjacency
bit-matrix mirror (tests/_degree_graphs.py: adjbits_reference) agrees with the closure computed independently."""
import functools

import numpy as np
import pytest

import _degree_graphs as dg
import _sent_walk_ref as wref
from _util import gtok, orc

UNCUT = 1 << 17          # beyond the longest walk here (K256 with a self loop: 33,152 tokens unlabelled, about twice that labelled)
LAB = dict(labeled=True, num_node_types=dg.NODE_TYPES, num_edge_types=dg.EDGE_TYPES)


def _instances():
    out = {}
    for name, (mk, _) in dg.LIMIT_GRAPHS.items():
        for both in (False, True):
            out[f"{name}-{'both' if both else 'one'}"] = functools.partial(mk, both)
    for leaves in (15, 16):
        for big in (0, 128, 256):
            out[f"plane{leaves}-big{big}-one"] = functools.partial(dg.plane_batch, leaves, False, big)
        out[f"plane{leaves}-big0-both"] = functools.partial(dg.plane_batch, leaves, True, 0)
    return out


INSTANCES = _instances()


def _closure(d):
    """per graph: the neighbour sets of the symmetric closure, straight from the lists"""
    eptr = np.concatenate([[0], np.cumsum(d["edge_counts"])])
    out = []
    for g, n in enumerate(d["node_counts"]):
        pairs = list(zip(d["src"][eptr[g]:eptr[g + 1]].tolist(), d["dst"][eptr[g]:eptr[g + 1]].tolist()))
        out.append([{b for a, b in pairs if a == u} | {a for a, b in pairs if b == u} for u in range(int(n))])
    return out


@pytest.mark.parametrize("name", list(INSTANCES))
def test_the_stated_degree_is_the_true_one_and_the_listing_is_what_it_says(name):
    d = INSTANCES[name]()
    nb = _closure(d)
    assert d["degree"] == max([len(s) for g in nb for s in g], default=0)
    batch = gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"])
    loops = bool((d["src"] == d["dst"]).any())
    assert bool(batch.flags & gtok._lib.CSR_SIMPLE_SYMMETRIC) == (name.endswith("-both") and not loops)
    if name.endswith("-both"):
        assert batch.eorder is None                                         # row-sorted
        assert batch.max_degree == d["degree"]                              # the longest CSR row is the largest degree
    else:
        assert not np.any((d["src"] > d["dst"]))                            # every edge once, a <= b


@pytest.mark.parametrize("name", list(INSTANCES))
@pytest.mark.parametrize("labeled", [False, True])
def test_the_oracle_equals_the_python_walk_on_every_instance(name, labeled):
    """token for token, uncut and cut at 100, at both (seed, epoch, graph_base) triples of the GPU tests"""
    d = INSTANCES[name]()
    x, ea = (d["x"], d["edge_attr"]) if labeled else (None, None)
    coo = orc.Coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], x, ea)
    kw = dict(LAB) if labeled else {}
    for max_len in (UNCUT, 100):
        for seed, epoch, base in ((7, 1, 0), (12345678901234567, 3, 10 ** 10)):
            if max_len == UNCUT and base and int(d["edge_counts"].max()) > 20000:
                continue                                                    # (the 33 k-token Python walks of K256: once per labelling)
            ids, ln = orc.sent(coo, 256, max_len, seed, epoch, graph_base=base, ld=max_len, **kw)
            toks, _ = wref.walk_batch(orc, d["node_counts"], d["edge_counts"], d["src"], d["dst"], max_len, seed, epoch, graph_base=base,
                                      labeled=labeled, x=x, edge_attr=ea, max_num_nodes=256, num_node_types=dg.NODE_TYPES if labeled else 0)
            for g, t in enumerate(toks):
                assert t.size == ln[g] and np.array_equal(t, ids[g, :ln[g]]), (g, max_len, seed)
            if max_len == UNCUT:
                assert (ln < UNCUT).all()


@pytest.mark.parametrize("name", list(dg.LIMIT_GRAPHS))
@pytest.mark.parametrize("both", [False, True])
def test_the_uncut_lengths_are_the_recorded_ones(name, both):
    """seed 7, epoch 1, graph_base 0, unlabelled, every graph a batch of its own: a change of a fixture shows here"""
    mk, want = dg.LIMIT_GRAPHS[name]
    d = mk(both)
    coo = orc.Coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"])
    _, ln = orc.sent(coo, 256, UNCUT, dg.LENGTH_SEED, dg.LENGTH_EPOCH, ld=16)
    assert ln.tolist() == [want]


def test_the_degrees_the_instances_sit_on():
    deg = {k: mk(False)["degree"] for k, (mk, _) in dg.LIMIT_GRAPHS.items()}
    assert deg == dict(star16=15, star17=16, star64_hub0=63, star64_hub63=63, K64=63, star256_hub0=255, star256_hub64=255,
                       star256_hub255=255, wheel256=255, K8_248=248, K256=255, K256_loop=256)
    for big in (0, 128, 256):
        assert dg.plane_batch(15, False, big)["degree"] == 15 and dg.plane_batch(16, False, big)["degree"] == 16
        assert int(dg.plane_batch(15, False, big)["node_counts"].max()) == max(big, 30)
    assert dg.plane_batch(15, True)["degree"] == 15 and dg.plane_batch(16, True)["degree"] == 16


@pytest.mark.parametrize("name", list(INSTANCES))
def test_the_mirror_reference_agrees_with_the_closure(name):
    d = INSTANCES[name]()
    W = 1 if d["node_counts"].max() <= 64 else 2 if d["node_counts"].max() <= 128 else 4
    rows, planes, maxdeg = dg.adjbits_reference(d["node_counts"], d["edge_counts"], d["src"], d["dst"], W)
    nb = _closure(d)
    assert maxdeg == d["degree"]
    nptr = np.concatenate([[0], np.cumsum(d["node_counts"])])
    eptr = np.concatenate([[0], np.cumsum(d["edge_counts"])])
    bit = lambda r, v: (int(rows[r, v >> 6]) >> (v & 63)) & 1
    for g, sets in enumerate(nb):
        n = len(sets)
        loops = {a for a, b in zip(d["src"][eptr[g]:eptr[g + 1]].tolist(), d["dst"][eptr[g]:eptr[g + 1]].tolist()) if a == b}
        for u in range(n):
            r = int(nptr[g]) + u
            assert sum(bin(int(w)).count("1") for w in rows[r]) == len(sets[u])            # the row holds the degree's worth of bits
            in_planes = sum(((int(planes[g, p, u >> 6]) >> (u & 63)) & 1) << p for p in range(8))
            assert in_planes == len(sets[u]) % 256
            assert bit(r, u) == (u in loops)                                                 # the diagonal: exactly the listed self loops
        for u in range(n):
            for v in sets[u]:
                assert bit(int(nptr[g]) + u, v) and bit(int(nptr[g]) + v, u)                 # symmetric
        for p in range(8):                                                                   # nodes at or beyond N_g contribute 0
            for w in range(W):
                lo = max(0, min(64, n - 64 * w))
                assert int(planes[g, p, w]) >> lo == 0


def test_the_mirror_reference_on_a_hand_made_listing():
    """duplicates, a reversed duplicate, a self loop, columns outside the graph: 4 nodes, words = 2 (more than needed)"""
    rows, planes, maxdeg = dg.adjbits_reference([4, 0, 1], [8, 0, 1], [0, 0, 1, 2, 2, 3, 3, 0, 0], [1, 1, 0, 2, 4, -1, 300, 3, 0], 2)
    assert rows.tolist() == [[0b1010, 0], [0b0001, 0], [0b0100, 0], [0b0001, 0], [0b1, 0]] and maxdeg == 2
    assert planes[0].tolist() == [[0b1110, 0], [0b0001, 0]] + [[0, 0]] * 6 and not planes[1].any()
    assert planes[2].tolist() == [[1, 0]] + [[0, 0]] * 7
