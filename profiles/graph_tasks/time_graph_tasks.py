"""Timing of ops.graph_tasks / synth.label_batch_device with HIP events: the 125 k-graph config-5 ER share (10-256 nodes, one query
per graph) and 100 k default graph-token graphs (10-49 nodes), against the host loops (synth._has_cycle / _bfs_dist) and the numpy
reference of the tests on a sample of the same graphs.  `python profiles/graph_tasks/time_graph_tasks.py OUT_DIR` writes OUT_DIR/time_graph_tasks.json (the figures of timing.md)."""
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
gtok = importlib.import_module("glearning-benchmark_amd")
DEV = "cuda:0"


def events(fn, warmup=3, reps=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts = np.array(ts)
    return dict(ms_median=float(np.median(ts)), ms_min=float(ts.min()), ms_max=float(ts.max()), reps=reps)


def host_loops(d, sample, queries):
    eptr = np.concatenate([[0], np.cumsum(d["edge_counts"])])
    t = time.perf_counter()
    for g in sample:
        e = np.stack([d["src"][eptr[g]:eptr[g + 1]], d["dst"][eptr[g]:eptr[g + 1]]], 1)
        n = int(d["node_counts"][g])
        gtok.synth._has_cycle(n, e)
        gtok.synth._bfs_dist(n, e, int(queries[g, 0]))
    return (time.perf_counter() - t) / len(sample)


def numpy_ref(d, sample, queries):
    import _graph_tasks_ref as ref
    eptr = np.concatenate([[0], np.cumsum(d["edge_counts"])])
    t = time.perf_counter()
    for g in sample:
        c = ref.Closure(d["node_counts"][g], d["src"][eptr[g]:eptr[g + 1]], d["dst"][eptr[g]:eptr[g + 1]])
        c.has_cycle()
        c.dist(int(queries[g, 0]), int(queries[g, 1]))
    return (time.perf_counter() - t) / len(sample)


def one(name, d):
    b = gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"]).to(DEV)
    sp = gtok.synth.label_batch_device(b, "shortest_path", seed=0)
    q = sp["queries"]
    G = b.num_graphs
    out = dict(graphs=G, nodes=b.num_nodes_total, entries=b.num_edges_total, max_nodes=b.max_nodes)
    out["all_answers"] = events(lambda: gtok.ops.graph_tasks(b, q))
    out["cycle_only"] = events(lambda: gtok.ops.graph_tasks(b, num_components=False))
    out["dist_only"] = events(lambda: gtok.ops.graph_tasks(b, q, has_cycle=False, num_components=False))
    out["label_batch_device_shortest_path"] = events(lambda: gtok.synth.label_batch_device(b, "shortest_path", seed=0), reps=10)
    byts = b.algorithmic_read_bytes(False, False) + 8 * G + 4 * (G + 1) + 12 * G          # CSR + queries + pointers read, three answers written
    out["algorithmic_bytes"] = int(byts)
    out["bytes_per_s_all_answers"] = byts / (out["all_answers"]["ms_median"] * 1e-3)
    st = gtok.ops.graph_tasks(b, q).status()
    out["status"] = st
    sample = np.random.default_rng(0).choice(G, 500, replace=False)
    qh = q.cpu().numpy()
    per_host, per_ref = host_loops(d, sample, qh), numpy_ref(d, sample, qh)
    out["host_loops_s_per_graph_sample500"] = per_host
    out["host_loops_s_extrapolated"] = per_host * G
    out["numpy_reference_s_per_graph_sample500"] = per_ref
    out["numpy_reference_s_extrapolated"] = per_ref * G
    print(name, json.dumps(out), flush=True)
    return out


def main():
    res = {}
    res["config5_er_125k"] = one("config5_er_125k", gtok.synth.er_batch_device(125_000, DEV, seed=0))
    d = gtok.synth.mix_batch_device(100_000, DEV, seed=1, min_nodes=10, max_nodes=49, families=("er", "ba", "sbm", "path", "star", "complete"))
    res["graph_token_100k_10_49"] = one("graph_token_100k_10_49", d)
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "time_graph_tasks.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
