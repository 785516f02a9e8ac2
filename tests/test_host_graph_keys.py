"""gtok_graph_keys without a GPU: the numpy restatement of the key (tests/_graph_keys_ref.py) against a key worked out with plain
Python integers and against the DEFINITION it digests - the reference's tuple key, test/train_performance_test.py:70-74: a graph's
identity is (its node count, the sorted list of its listed edges after each edge's two endpoints were put in ascending order, its
label), so two graphs are the same exactly when they have as many nodes, the same label and the same multiset of unordered listed
pairs, whatever order and orientation the list has; :146-207 intersects the splits' sets of such tuples.  Then the grouping of
ops.duplicate_graphs on CPU tensors against Python sets, the confirm path under keys that say nothing, the host-side argument checks
(csrc/gtok_graph_keys_args.hpp and the hash header through tests/host/graph_keys_args_main.cpp), the binding and the errors the
Python layer raises before any device is touched."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import _graph_keys_ref as ref
from _util import ROOT, edge_case_graphs, gtok

_lib = gtok._lib
M = (1 << 64) - 1


def _mix(z):
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9 & M
    z = (z ^ (z >> 27)) * 0x94D049BB133111EB & M
    return z ^ (z >> 31)


def _key_by_hand(n, edges, label, C, D):
    S = sum(_mix((min(u, v) | max(u, v) << 14) ^ C) for u, v in edges) & M
    return _mix((S + _mix((n | len(edges) << 32) ^ C) + _mix((label & 0xFFFFFFFF) ^ D)) & M)


def test_numpy_digest_equals_a_key_worked_out_by_hand():
    """3 nodes, the entries (2, 0) and (0, 1), label 1: the words are 0 | 2 << 14 and 0 | 1 << 14, two terms"""
    assert _mix(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF, "splitmix64, seed 0, first output"
    want = [_key_by_hand(3, [(2, 0), (0, 1)], 1, ref.C[j], ref.D[j]) for j in range(2)]
    assert want == [0x3F390493A2540768, 0xD150091ECB30AFDF], "the constants of DESIGN.md"
    assert ref.listed_key(3, [2, 0], [0, 1], 1).tolist() == want
    assert ref.listed_key(3, [1, 0], [0, 2], 1).tolist() == want, "order and orientation do not count"
    assert ref.listed_key(3, [2, 0], [0, 1], -1).tolist() == [_key_by_hand(3, [(2, 0), (0, 1)], -1, ref.C[j], ref.D[j]) for j in range(2)]
    assert int(ref.mix(np.array([0x9E3779B97F4A7C15], np.uint64))[0]) == 0xE220A8397B1DCDAF
    # with attributes: edge bytes in bits 28.., a node term per node
    w = ref.words(2, [1], [0], x=[7, 300], edge_attr=[3])
    assert w.tolist() == [0 | 1 << 14 | 3 << 28, 0 | 7 << 14 | 1 << 40, 1 | 255 << 14 | 1 << 40]


def _splits(num=12):
    return ref.tree_splits(gtok.synth.graph_token_tree(num, seed=7, min_nodes=10, max_nodes=20))


def _keys_agree_with_tuples(d, labels, mode, x=None, ea=None):
    keys = ref.batch_keys(d["node_counts"], d["edge_counts"], d["src"], d["dst"], labels, mode, x, ea)
    tup = ref.batch_tuples(d["node_counts"], d["edge_counts"], d["src"], d["dst"], labels, mode, x, ea)
    by_key = ref.classes([tuple(k) for k in keys.tolist()])
    assert np.array_equal(by_key, ref.classes(tup)), mode
    fast = ref.batch_tuples(d["node_counts"], d["edge_counts"], d["src"], d["dst"], labels, mode, x, ea, fast=True)
    assert np.array_equal(by_key, ref.classes(fast)), "the quick form of the tuples (the GPU tests' yardstick) makes the same classes"
    return keys, tup


def test_equal_keys_are_equal_tuples_on_the_hand_made_graphs_and_on_corpus_splits():
    d = edge_case_graphs()
    for mode in ("listed", "closure"):
        _keys_agree_with_tuples(d, None, mode)
    _keys_agree_with_tuples(d, None, "listed", d["x"], d["edge_attr"])
    # twice the same graphs, one copy with every entry flipped and the order reversed: each graph meets itself
    two = dict(edge_counts=np.concatenate([d["edge_counts"], d["edge_counts"][::-1]]))
    eptr = np.concatenate([[0], np.cumsum(d["edge_counts"])])
    rs = np.concatenate([d["dst"][eptr[g]:eptr[g + 1]][::-1] for g in range(9, -1, -1)])
    rd = np.concatenate([d["src"][eptr[g]:eptr[g + 1]][::-1] for g in range(9, -1, -1)])
    two["node_counts"] = np.concatenate([d["node_counts"], d["node_counts"][::-1]])
    two["src"], two["dst"] = np.concatenate([d["src"], rs]), np.concatenate([d["dst"], rd])
    keys, tup = _keys_agree_with_tuples(two, None, "listed")
    assert all(tup[g] == tup[19 - g] for g in range(10)) and np.array_equal(keys[:10], keys[10:][::-1])
    sp = _splits()
    for mode in ("listed", "closure"):
        alls = {k: np.concatenate([sp[s][k] for s in ("train", "test")]) for k in ("node_counts", "edge_counts", "src", "dst", "labels")}
        keys, tup = _keys_agree_with_tuples(alls, alls["labels"], mode)
        assert len(set(tup)) < len(tup), "the corpus repeats its path, star and complete graphs"
        flipped = 1 - alls["labels"]
        assert not (ref.batch_keys(alls["node_counts"], alls["edge_counts"], alls["src"], alls["dst"], flipped, mode) == keys).all(1).any()


def _messy(rng, n):
    k = int(rng.integers(0, 3 * n + 1)) if n else 0
    src, dst = rng.integers(0, max(n, 1), k), rng.integers(0, max(n, 1), k)
    take = rng.integers(0, max(k, 1), k // 2)
    return np.concatenate([src, dst[take]]), np.concatenate([dst, src[take]])


def test_closure_key_of_a_messy_listing_is_the_listed_key_of_the_graph_listed_once():
    rng = np.random.default_rng(5)
    seen_loop = seen_dup = 0
    for t in range(200):
        n = int(rng.integers(0, 30))
        src, dst = _messy(rng, n)
        a, b = ref.simple_once_listing(src, dst)
        assert (a <= b).all() and len(set(zip(a.tolist(), b.tolist()))) == a.size
        want = ref.listed_key(n, a, b, t)
        assert np.array_equal(ref.closure_key(n, src, dst, t), want)
        assert np.array_equal(ref.closure_key(n, np.concatenate([a, b]), np.concatenate([b, a]), t), want), "both directions"
        assert np.array_equal(ref.closure_key(n, b, a, t), want)
        seen_loop += int((a == b).any()); seen_dup += int(src.size > a.size)
        if src.size > a.size:
            assert not np.array_equal(ref.listed_key(n, src, dst, t), want), "the listed key counts duplicates"
    assert seen_loop > 20 and seen_dup > 100


def _host_batches(sp, names=("train", "test")):
    return [gtok.GraphBatch.from_coo(sp[s]["node_counts"], sp[s]["edge_counts"], sp[s]["src"], sp[s]["dst"]) for s in names]


def _t(keys):
    return torch.from_numpy(np.ascontiguousarray(keys).view(np.int64))


@pytest.mark.parametrize("mode", ("listed", "closure"))
@pytest.mark.parametrize("confirm", (False, True))
def test_grouping_and_overlap_on_cpu_tensors_equal_python_sets(mode, confirm):
    sp = _splits()
    names = ("train", "test")
    bl = _host_batches(sp, names)
    labels = [torch.from_numpy(sp[s]["labels"]) for s in names]
    keys = [_t(ref.batch_keys(sp[s]["node_counts"], sp[s]["edge_counts"], sp[s]["src"], sp[s]["dst"], sp[s]["labels"], mode)) for s in names]
    tups = [ref.batch_tuples(sp[s]["node_counts"], sp[s]["edge_counts"], sp[s]["src"], sp[s]["dst"], sp[s]["labels"], mode) for s in names]
    dup = gtok.ops.duplicate_graphs(bl, labels, mode=mode, confirm=confirm, keys=keys)
    assert dup.group.dtype == torch.int64 and dup.split_ptr == [0, bl[0].num_graphs, bl[0].num_graphs + bl[1].num_graphs]
    assert np.array_equal(dup.group.numpy(), ref.classes(tups[0] + tups[1]))
    assert np.array_equal(dup.is_first.numpy(), dup.group.numpy() == np.arange(dup.group.numel()))
    assert dup.split.tolist() == [0] * bl[0].num_graphs + [1] * bl[1].num_graphs
    uniq, ov = ref.set_report(tups)
    assert dup.unique_per_split().tolist() == uniq and dup.overlap().tolist() == ov and ov[0][1] > 0
    in_train = set(tups[0])
    assert dup.leaked(0, 1).tolist() == [i for i, t in enumerate(tups[1]) if t in in_train]
    fam = np.array(sp["test"]["family"])[dup.leaked(0, 1).numpy()]
    assert set(fam) == {"path", "star", "complete"}, "one graph per node count in these families: they repeat across splits"
    # one batch alone, keys as one tensor
    one = gtok.ops.duplicate_graphs(bl[0], labels[0], mode=mode, confirm=confirm, keys=keys[0])
    assert np.array_equal(one.group.numpy(), ref.classes(tups[0])) and one.overlap().tolist() == [[uniq[0]]]


@pytest.mark.parametrize("mode,attrs", (("listed", False), ("closure", False), ("listed", True)))
def test_keys_that_say_nothing_still_give_the_exact_classes(mode, attrs):
    """every graph under ONE key: the confirm path alone finds the classes, round after round; a small byte budget cuts it into chunks"""
    d = edge_case_graphs()
    # the hand-made graphs three times: as they are, every entry flipped, and with one attribute byte / one label changed
    nc, ec = np.tile(d["node_counts"], 3), np.tile(d["edge_counts"], 3)
    src, dst = np.concatenate([d["src"], d["dst"], d["src"]]), np.concatenate([d["dst"], d["src"], d["dst"]])
    x, ea = np.tile(d["x"], 3), np.tile(d["edge_attr"], 3)
    labels = np.zeros(30, np.int64)
    labels[27] = 5
    x[-1] += 1                     # the last node of the last K8
    ea[d["edge_attr"].size * 2 + 4] += 1      # an entry of the third copy of Mol B
    b = gtok.GraphBatch.from_coo(nc, ec, src, dst, x if attrs else None, ea if attrs else None)
    tup = ref.batch_tuples(nc, ec, src, dst, labels, mode, x if attrs else None, ea if attrs else None)
    want = ref.classes(tup)
    assert 10 <= len(set(want.tolist())) < 30
    same = torch.zeros((30, 2), dtype=torch.int64)
    for budget in (256 << 20, 64 * 40):
        dup = gtok.ops.duplicate_graphs(b, torch.from_numpy(labels), mode=mode, attrs=attrs, keys=same, budget_bytes=budget)
        assert np.array_equal(dup.group.numpy(), want), (mode, attrs, budget)
    merged = gtok.ops.duplicate_graphs(b, torch.from_numpy(labels), mode=mode, attrs=attrs, keys=same, confirm=False)
    assert merged.group.tolist() == [0] * 30, "without confirm the keys are trusted"
    # two splits of it: the classes of the concatenation
    both = gtok.ops.duplicate_graphs([b, b], [torch.from_numpy(labels)] * 2, mode=mode, attrs=attrs, keys=[same, same])
    assert np.array_equal(both.group.numpy(), ref.classes(tup + tup)) and both.overlap().tolist() == [[len(set(tup))] * 2] * 2


def test_argument_checks_program():
    """tests/host/graph_keys_args_main.cpp sweeps the host-side checks, the kernel choice and the hash header; built here as plain
    C++ (the sanitizer build is the command at the top of that file).  Its `key` mode prints the key the C++ header computes."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "graph_keys_args")
        subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "glearning-benchmark_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host", "graph_keys_args_main.cpp"), "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True)
        k = subprocess.run([exe, "key", "3", "2", "0", "0", "1", "label", "1"], capture_output=True, text=True)
        d = edge_case_graphs()
        e0, e1 = int(d["edge_counts"][:9].sum()), int(d["edge_counts"].sum())
        flat = [str(v) for p in zip(d["src"][e0:e1].tolist(), d["dst"][e0:e1].tolist()) for v in p]
        k8 = subprocess.run([exe, "key", "8"] + flat + ["label", "-3"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failures"), r.stdout + r.stderr
    assert k.stdout.split() == ["3f390493a2540768", "d150091ecb30afdf"]
    assert k8.stdout.split() == ["%016x" % int(v) for v in ref.listed_key(8, d["src"][e0:e1], d["dst"][e0:e1], -3)]


def test_binding_and_python_errors():
    assert "gtok_graph_keys" in _lib.SYMBOLS and _lib.GRAPH_KEYS_SYMBOLS == ("gtok_graph_keys",)
    assert set(_lib.GRAPH_KEYS_SYMBOLS) <= _lib._MAY_BE_MISSING
    assert any(s.endswith("gtok_graph_keys.hip") for s in _lib.SOURCES)
    assert all(any(h.endswith(n) for h in _lib.HEADERS) for n in ("gtok_graph_keys_args.hpp", "gtok_graph_keys_hash.hpp"))
    assert (_lib.KEYS_LISTED, _lib.KEYS_CLOSURE, _lib.KEYS_ATTRS) == (0, 1, 2)
    assert hasattr(_lib.lib(), "gtok_graph_keys"), "the built library exports the entry point"
    assert hasattr(torch.ops.gtok, "graph_keys")
    d = edge_case_graphs()
    host = gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"])
    attr = gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], d["x"], d["edge_attr"])
    with pytest.raises(_lib.GtokError, match="GPU"):
        gtok.ops.graph_keys(host)
    with pytest.raises(_lib.GtokError, match="GPU"):
        gtok.ops.duplicate_graphs(host)
    with pytest.raises(_lib.GtokError, match="GPU"):
        gtok.ops.split_leakage({"train": (host, None), "test": host})
    with pytest.raises(ValueError, match="mode"):
        gtok.ops.graph_keys(host, mode="isomorphic")
    with pytest.raises(ValueError, match="structure only"):
        gtok.ops.graph_keys(attr, mode="closure", attrs=True)
    with pytest.raises(ValueError, match="attributes"):
        gtok.ops.graph_keys(host, attrs=True)
    with pytest.raises(ValueError, match="keys must be"):
        gtok.ops.duplicate_graphs(host, keys=torch.zeros((3, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="one label"):
        gtok.ops.duplicate_graphs(host, torch.zeros(3), keys=torch.zeros((10, 2), dtype=torch.int64))
    with pytest.raises(ValueError):
        gtok.ops.duplicate_graphs([host, host], [None], keys=torch.zeros((20, 2), dtype=torch.int64))
    # the library refuses bad arguments before it asks for a device
    L = _lib.lib()
    cs = host.c_struct()
    keys, info = torch.zeros((10, 2), dtype=torch.int64), torch.zeros(4, dtype=torch.int32)
    assert L.gtok_graph_keys(None, None, 0, keys.data_ptr(), info.data_ptr(), None) == -1
    assert L.gtok_graph_keys(ctypes.byref(cs), None, 0, None, info.data_ptr(), None) == -1
    assert L.gtok_graph_keys(ctypes.byref(cs), None, 0, keys.data_ptr(), None, None) == -1
    assert L.gtok_graph_keys(ctypes.byref(cs), None, 4, keys.data_ptr(), info.data_ptr(), None) == -1             # an unknown flag bit
    assert L.gtok_graph_keys(ctypes.byref(cs), None, 3, keys.data_ptr(), info.data_ptr(), None) == -1             # CLOSURE | ATTRS
    assert L.gtok_graph_keys(ctypes.byref(cs), None, 2, keys.data_ptr(), info.data_ptr(), None) == -1             # ATTRS, no arrays
    empty = gtok.GraphBatch.from_coo([], [], [], [])
    assert L.gtok_graph_keys(ctypes.byref(empty.c_struct()), None, 0, None, info.data_ptr(), None) == 0           # no graphs: a no-op
    big = gtok.GraphBatch.from_coo([_lib.SENT_LARGE_MAX_NODES + 1], [0], [], [])
    assert L.gtok_graph_keys(ctypes.byref(big.c_struct()), None, 0, keys.data_ptr(), info.data_ptr(), None) == -2
    mid = gtok.GraphBatch.from_coo([513], [1], [0], [1])
    assert L.gtok_graph_keys(ctypes.byref(mid.c_struct()), None, 1, keys.data_ptr(), info.data_ptr(), None) == _lib.E_UNSUPPORTED
    assert keys.abs().sum() == 0 and info.tolist() == [0, 0, 0, 0]
