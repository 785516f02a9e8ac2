"""gtok_graph_tasks without a GPU: the numpy restatement of its definitions (tests/_graph_tasks_ref.py) pinned to the host loops it
replaces (synth._has_cycle / synth._bfs_dist) and to networkx, the host-side argument checks (csrc/gtok_graph_tasks_args.hpp through
tests/host/graph_tasks_args_main.cpp), the binding and the errors the Python layer raises before any device is touched."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _graph_tasks_ref as ref
from _util import ROOT, edge_case_graphs, gtok

_lib = gtok._lib


def test_reference_equals_the_host_loops_on_simple_once_listed_graphs():
    """graph_token_like lists every edge once and simple: there synth._has_cycle is the cycle check and synth._bfs_dist the
    distances (every source of every graph)."""
    d = gtok.synth.graph_token_like(300, task=None, with_text=False)
    eptr = np.concatenate([[0], np.cumsum(d["edge_counts"])])
    cycles = 0
    for g, n in enumerate(d["node_counts"]):
        e = np.stack([d["src"][eptr[g]:eptr[g + 1]], d["dst"][eptr[g]:eptr[g + 1]]], 1)
        c = ref.Closure(n, e[:, 0], e[:, 1])
        assert c.loops == 0 and c.m == e.shape[0]
        assert c.has_cycle() == int(gtok.synth._has_cycle(int(n), e)), g
        cycles += c.has_cycle()
        for s in range(0, int(n), 7):
            assert np.array_equal(c.levels(s), gtok.synth._bfs_dist(int(n), e, s)), (g, s)
    assert 0 < cycles < 300, "both answers occur"


def _random_multigraph(rng, n):
    k = int(rng.integers(0, 3 * n + 1)) if n else 0
    src, dst = rng.integers(0, max(n, 1), k), rng.integers(0, max(n, 1), k)
    if k and rng.random() < 0.5:                       # duplicates and reversed copies
        take = rng.integers(0, k, k // 2 + 1)
        src, dst = np.concatenate([src, dst[take]]), np.concatenate([dst, src[take]])
    if k and rng.random() < 0.5:                       # no loops in this one
        keep = src != dst
        src, dst = src[keep], dst[keep]
    return src, dst


def test_reference_equals_networkx_on_multigraphs_with_loops_and_duplicates():
    nx = pytest.importorskip("networkx")
    rng = np.random.default_rng(20261019)
    seen = set()
    for t in range(300):
        n = int(rng.integers(1, 41))
        src, dst = _random_multigraph(rng, n)
        G = nx.Graph()
        G.add_nodes_from(range(n))
        G.add_edges_from(zip(src.tolist(), dst.tolist()))
        for dense in (True, False):
            c = ref.Closure(n, src, dst, dense=dense)
            comp = c.num_components()
            assert comp == nx.number_connected_components(G), t
            assert c.has_cycle(comp) == int(not nx.is_forest(G)), t
            H = G.copy()
            H.remove_edges_from(nx.selfloop_edges(G))
            want = np.full((n, n), -1, np.int64)
            for u, row in nx.all_pairs_shortest_path_length(H):
                for v, dd in row.items():
                    want[u, v] = dd
            got = np.stack([c.levels(s) for s in range(n)])
            assert np.array_equal(got, want), t
        seen.add((c.has_cycle(comp), c.loops > 0, comp > 1))
    assert len(seen) >= 6, "cyclic and acyclic, with and without loops, connected and not"


def test_reference_on_the_empty_graph_and_the_hand_made_ones():
    c = ref.Closure(0, [], [])
    assert (c.num_components(), c.has_cycle(), c.dist(0, 0)) == (0, 0, ref.BAD_QUERY)
    d = edge_case_graphs()
    r = ref.batch_answers(d["node_counts"], d["edge_counts"], d["src"], d["dst"])
    #            empty 1 node 5 isolated MolB(loop) MolA(path) loops two triangles 7-ring one edge K8
    assert r["num_components"].tolist() == [0, 1, 5, 1, 1, 3, 2, 1, 1, 1]
    assert r["has_cycle"].tolist() == [0, 0, 0, 1, 0, 1, 1, 1, 0, 1]
    q = np.array([[0, 0], [0, 0], [0, 4], [0, 1], [0, 3], [0, 3], [0, 3], [0, 4], [1, 0], [7, 7]])
    r = ref.batch_answers(d["node_counts"], d["edge_counts"], d["src"], d["dst"], q)
    assert r["dist"].tolist() == [-2, 0, -1, 2, 3, -1, -1, 3, 1, 0] and r["info"].tolist() == [1, 3, 3, 5]
    both = ref.batch_answers([4], [6], [0, 1, 1, 2, 2, 3], [1, 0, 2, 1, 3, 2], [[0, 3], [3, 0], [1, 1], [5, 0]], [0, 4])
    assert both["has_cycle"].tolist() == [0] and both["dist"].tolist() == [3, 3, 0, -2]     # a both-directions list is no cycle


def test_dense_and_sparse_closures_agree_on_a_large_ring_with_chords():
    n = 700
    a = np.arange(n)
    src, dst = np.concatenate([a, a[::50]]), np.concatenate([(a + 1) % n, (a[::50] + 300) % n])
    cd, cs = ref.Closure(n, src, dst, dense=True), ref.Closure(n, src, dst, dense=False)
    assert cd.m == cs.m == n + 14 and cd.num_components() == cs.num_components() == 1
    for s in (0, 1, 349, 699):
        assert np.array_equal(cd.levels(s), cs.levels(s))


def test_argument_checks_program():
    """tests/host/graph_tasks_args_main.cpp sweeps the host-side checks and the kernel choice; built here as plain C++ (the sanitizer
    build is the command at the top of that file)."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "graph_tasks_args")
        subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "glearning-benchmark_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host", "graph_tasks_args_main.cpp"), "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failures"), r.stdout + r.stderr


def test_binding_and_python_errors():
    assert "gtok_graph_tasks" in _lib.SYMBOLS and _lib.GRAPH_TASKS_SYMBOLS == ("gtok_graph_tasks",)
    assert set(_lib.GRAPH_TASKS_SYMBOLS) <= _lib._MAY_BE_MISSING
    assert any(s.endswith("gtok_graph_tasks.hip") for s in _lib.SOURCES) and any(h.endswith("gtok_graph_tasks_args.hpp") for h in _lib.HEADERS)
    assert hasattr(_lib.lib(), "gtok_graph_tasks"), "the built library exports the entry point"
    d = edge_case_graphs()
    host = gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"])
    with pytest.raises(_lib.GtokError, match="GPU"):
        gtok.ops.graph_tasks(host)
    with pytest.raises(_lib.GtokError, match="GPU"):
        gtok.ops.check_task_labels(host, "cycle_check", torch.zeros(host.num_graphs, dtype=torch.int32))
    with pytest.raises(ValueError):
        gtok.ops.check_task_labels(host, "connected", torch.zeros(host.num_graphs, dtype=torch.int32))
    with pytest.raises(ValueError):
        gtok.synth.label_batch_device(host, "triangles", 0)
    # NULL arguments are refused by the library before it asks for a device
    L = _lib.lib()
    cs = host.c_struct()
    import ctypes
    assert L.gtok_graph_tasks(None, None, None, 0, None, None, None, None, None) == -1
    assert L.gtok_graph_tasks(ctypes.byref(cs), None, None, 0, None, None, None, None, None) == -1          # no info
    info = torch.zeros(4, dtype=torch.int32)
    assert L.gtok_graph_tasks(ctypes.byref(cs), None, None, 0, None, None, None, info.data_ptr(), None) == 0   # nothing asked for
    assert L.gtok_graph_tasks(ctypes.byref(cs), None, None, 3, None, None, None, info.data_ptr(), None) == -1
    big = gtok.GraphBatch.from_coo([_lib.SENT_LARGE_MAX_NODES + 1], [0], [], [])
    assert L.gtok_graph_tasks(ctypes.byref(big.c_struct()), None, None, 0, info.data_ptr(), None, None, info.data_ptr(), None) == -2
    mid = gtok.GraphBatch.from_coo([513], [1], [0], [1])
    assert L.gtok_graph_tasks(ctypes.byref(mid.c_struct()), None, None, 0, info.data_ptr(), None, None, info.data_ptr(), None) == _lib.E_UNSUPPORTED
