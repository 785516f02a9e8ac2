"""SENT walks at the degree limits, bit-exact against the C oracle in ids and lengths (test_host_degree.py pins the oracle to the
plain-Python walk on these very graphs): batches whose largest degree is exactly 15 and exactly 16 - where the launchers switch the
number of counter planes (sent_blane_kernel 4 | 8 by adj_max_degree, sent_lane_kernel 4 | 6 by max_degree) - and the largest hubs
and densest graphs each kernel accepts.  Every walk runs pinned (GTOK_SENT_KERNEL) and asserts, from the very struct the launch
got, that the intended kernel and plane count ran: a pin is only honoured where the kernel accepts the batch."""
import functools

import numpy as np
import pytest
import torch

import _degree_graphs as dg
from _util import both, gtok, orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NN = 256                                                         # max_num_nodes of every call here
RUNS = ((7, 1, 0), (12345678901234567, 3, 10 ** 10))             # (seed, epoch, graph_base)
UNCUT = 1 << 16                                                  # beyond every uncut walk here but K256's, which is cut at 4,096
LAB = dict(labeled=True, num_node_types=dg.NODE_TYPES, num_edge_types=dg.EDGE_TYPES)


def _kw(labeled):
    return dict(LAB) if labeled else {}


def _pin(monkeypatch, pin):
    """GTOK_SENT_KERNEL pin; "lane-int32" = the lane kernel staging from the int32 CSR (no byte mirror), "lane-unsorted" = the lane
    kernel on the batch as stored instead of its copy reordered by walk length"""
    monkeypatch.setenv("GTOK_SENT_KERNEL", pin.split("-")[0])
    for var, on in (("GTOK_NO_PACK8", pin == "lane-int32"), ("GTOK_NO_LANE_SORT", pin == "lane-unsorted")):
        if on:
            monkeypatch.setenv(var, "1")
        else:
            monkeypatch.delenv(var, raising=False)
    for var in ("GTOK_NO_ADJBITS", "GTOK_BLANE_ORDER"):
        monkeypatch.delenv(var, raising=False)


def _launched():
    """(kernel name, max_degree, adj_max_degree) of the struct the last ops.sent call launched"""
    cs, _ = gtok.ops._LAST_SENT
    return gtok.ops.last_sent_kernel(), int(cs.max_degree), int(cs.adj_max_degree)


def _cmp(ids, ln, ref_ids, ref_ln, what):
    ids, ln = ids.cpu().numpy(), ln.cpu().numpy()
    assert np.array_equal(ln, ref_ln), f"{what}: lengths {ln.tolist()[:8]} vs {ref_ln.tolist()[:8]}"
    bad = np.nonzero((ids != ref_ids).any(1))[0]
    if bad.size:
        r = bad[0]
        c = int(np.nonzero(ids[r] != ref_ids[r])[0][0])
        lo = max(0, c - 12)
        raise AssertionError(f"{what}: {bad.size} rows differ, first row {r} col {c}: {ids[r, lo:c + 8].tolist()} vs {ref_ids[r, lo:c + 8].tolist()}")


# ------------------------------------------------------------------------------------------------ batches and their references
@functools.lru_cache(maxsize=None)
def _data(name):
    """plane<leaves>-<big>-<one|both>: the plane-switch batch; <limit graph>-<one|both>: that graph between a path and a ring"""
    head, listing = name.rsplit("-", 1)
    both_dirs = listing == "both"
    if head.startswith("plane"):
        leaves, big = head[5:].split("-")
        d = dg.plane_batch(int(leaves), both_dirs, int(big))
    else:
        d = dg.batch_of(dg.path(4, both_dirs), dg.LIMIT_GRAPHS[head][0](both_dirs), dg.ring(5, both_dirs))
    return d


@functools.lru_cache(maxsize=None)
def _host(name, labeled):
    return both(_data(name), labeled)


@functools.lru_cache(maxsize=None)
def _ref(name, labeled, max_len, run):
    batch, coo = _host(name, labeled)
    seed, epoch, base = RUNS[run]
    ld = gtok.ops.sent_safe_ld(batch, labeled, max_len)
    return orc.sent(coo, NN, max_len, seed, epoch, graph_base=base, ld=ld, nthreads=4, **_kw(labeled))


def _walk_all(name, labeled, max_lens, kernel, prepare=None, check=None):
    """every (seed, epoch, graph_base) x max_len on a fresh device batch: rows and lengths are the oracle's, `kernel` ran"""
    batch, _ = _host(name, labeled)
    for max_len in max_lens:
        for run, (seed, epoch, base) in enumerate(RUNS):
            b = batch.to(DEV)
            if prepare:
                prepare(b)
            ids, ln = gtok.ops.sent(b, NN, max_len, seed, epoch, graph_base=base, **_kw(labeled))
            got = _launched()
            assert got[0] == kernel, (got, kernel)
            if check:
                check(b, got)
            ref, rln = _ref(name, labeled, max_len, run)
            _cmp(ids, ln, ref, rln, f"{name} labeled={labeled} max_len={max_len} run={run} [{kernel}]")


def _words(name):
    n = int(_data(name)["node_counts"].max())
    return 1 if n <= 64 else 2 if n <= 128 else 4


# ------------------------------------------------------------------------------------------------ plane switch: sent_blane_kernel
@pytest.mark.parametrize("big", [0, 128, 256])
@pytest.mark.parametrize("leaves", [15, 16])
def test_blane_plane_switch(leaves, big, monkeypatch):
    """unlabelled, one-direction listings: a 16-node star beside paths and small rings has closure degree exactly 15 - the 4-plane
    instantiation; one more leaf - the 8-plane one; a sparse graph of 128 | 256 nodes moves both to W = 2 | 4"""
    name = f"plane{leaves}-{big}-one"
    assert _data(name)["degree"] == leaves and not (_host(name, False)[0].flags & 1)
    _pin(monkeypatch, "blane")

    def check(b, got):
        assert b.adj_max_degree == leaves and got[2] == leaves and b.adj_words == _words(name)
        assert (got[2] <= 15) == (leaves == 15)                      # launch_blane's rule: 4 planes iff adj_max_degree <= 15
    _walk_all(name, False, (UNCUT, 100), f"sent_blane_kernel<W={_words(name)}>", check=check)


# ------------------------------------------------------------------------------------------------ plane switch: sent_lane_kernel
@pytest.mark.parametrize("pin", ["lane", "lane-int32", "lane-unsorted"])
@pytest.mark.parametrize("labeled", [False, True])
@pytest.mark.parametrize("leaves", [15, 16])
def test_lane_plane_switch(leaves, labeled, pin, monkeypatch):
    """both-direction listings: max_degree exactly 15 runs P = 4, exactly 16 runs P = 6 (launch_lane: 4 planes iff 0 < max_degree
    <= 15)"""
    name = f"plane{leaves}-0-both"
    batch, _ = _host(name, labeled)
    assert batch.max_degree == leaves == _data(name)["degree"] and batch.flags & 1
    _pin(monkeypatch, pin)

    def check(b, got):
        assert got[1] == leaves
    _walk_all(name, labeled, (UNCUT, 100), "sent_lane_kernel", check=check)


@pytest.mark.parametrize("pin", ["lane", "lane-int32", "lane-unsorted"])
@pytest.mark.parametrize("labeled", [False, True])
@pytest.mark.parametrize("claim", [0, 40])
def test_lane_degree_15_batch_with_an_unknown_and_a_loose_max_degree(claim, labeled, pin, monkeypatch):
    """the degree-15 batch again with max_degree 0 (unknown) and 40 (an accepted upper bound) on the batch object: the same tokens from
    the 6-plane instantiation - except that the reordered copy of a batch that does not know its max_degree carries the measured one, 15,
    and so runs 4 planes again; the batch as stored ("lane-unsorted") launches with 0."""
    name = "plane15-0-both"
    _pin(monkeypatch, pin)

    def prepare(b):
        b.max_degree = claim

    def check(b, got):
        assert got[1] == (claim if claim or pin == "lane-unsorted" else 15), got
    _walk_all(name, labeled, (UNCUT, 100), "sent_lane_kernel", prepare=prepare, check=check)


# ------------------------------------------------------------------------------------------------ the largest degrees each kernel accepts
def _limit_cases():
    out = []
    for g in ("star64_hub0", "star64_hub63"):
        for labeled in (False, True):
            out += [(g, "both", labeled, p) for p in ("lane", "lane-int32", "lane-unsorted", "reg", "lds")]
        out += [(g, "both", False, "blane"), (g, "one", False, "blane"), (g, "one", True, "reg"), (g, "one", False, "lds")]
    for labeled in (False, True):
        out += [("K64", "both", labeled, p) for p in ("reg", "lds")] + [("K64", "one", labeled, p) for p in ("reg", "lds")]
    out += [("K64", "both", False, "blane"), ("K64", "one", False, "blane")]
    for g in ("star256_hub0", "star256_hub64", "star256_hub255", "wheel256", "K8_248"):
        for listing in ("one", "both"):
            out += [(g, listing, False, "lds"), (g, listing, True, "lds"), (g, listing, False, "blane")]
    # K256 listed in both directions has 65,280 entries, beyond what gtok_sent stages (60,000): one direction here, both through sent_large
    out += [("K256", "one", False, "lds"), ("K256", "one", True, "lds"), ("K256", "one", False, "blane")]
    return out


def _max_lens(graph):
    return (4096, 100) if graph.startswith("K256") else (UNCUT, 100)


@pytest.mark.parametrize("graph,listing,labeled,pin", _limit_cases())
def test_largest_degrees_on_every_kernel_that_accepts_them(graph, listing, labeled, pin, monkeypatch):
    """hubs of degree 63 (at node 0 and node 63) and K64 on the 64-node kernels; hubs of degree 255 at node 0, 64 and 255, a wheel,
    K(8,248) and K256 on sent_lds_kernel and sent_blane_kernel: a k-th-neighbour pick over rows with hundreds of set bits in four
    words, brackets of up to 255 members, a `live` set that is one hub for 250 restarts"""
    name = f"{graph}-{listing}"
    d = _data(name)
    W = _words(name)
    assert d["degree"] == {"s": 63 if W == 1 else 255, "w": 255, "K": {"K64": 63, "K8_248": 248, "K256": 255}.get(graph)}[graph[0]]
    _pin(monkeypatch, pin)
    kernel = {"lane": "sent_lane_kernel", "reg": "sent_reg_kernel", "lds": f"sent_lds_kernel<W={W}>", "blane": f"sent_blane_kernel<W={W}>"}[pin.split("-")[0]]

    def check(b, got):
        if pin == "blane":
            assert b.adj_max_degree == d["degree"] == got[2] and got[2] > 15        # 8 planes
        if pin.startswith("lane"):
            assert got[1] == d["degree"]                                              # 6 planes
    _walk_all(name, labeled, _max_lens(graph), kernel, check=check)


@pytest.mark.parametrize("labeled", [False, True])
@pytest.mark.parametrize("listing", ["one", "both"])
@pytest.mark.parametrize("graph", list(dg.LIMIT_GRAPHS))
def test_largest_degrees_through_sent_large(graph, listing, labeled):
    """the same graphs (K256 in both listings, and with its self loop: degree 256) through gtok_sent_large"""
    name = f"{graph}-{listing}"
    batch, _ = _host(name, labeled)
    b = batch.to(DEV)
    for max_len in _max_lens(graph):
        for run, (seed, epoch, base) in enumerate(RUNS):
            ids, ln = gtok.ops.sent_large(b, NN, max_len, seed, epoch, graph_base=base, **_kw(labeled))
            assert gtok.ops.last_sent_kernel() == "sent_large_kernel"
            ref, rln = _ref(name, labeled, max_len, run)
            _cmp(ids, ln, ref, rln, f"sent_large {name} labeled={labeled} max_len={max_len} run={run}")
