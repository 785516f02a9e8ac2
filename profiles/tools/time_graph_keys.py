"""Timing of gtok_graph_keys with HIP events, beside the torch route that produces the same identities (the canonical folded entry
lists ops.duplicate_graphs(confirm=True) compares: a gather, one sort of (graph, a, b, t) packed into int64, unique_consecutive in
closure mode) run over the whole batch - the only way to such keys without the kernel.  Inputs: a ZINC-full-shaped batch
(zinc_like(249,456): LISTED + ATTRS, and CLOSURE through the register kernel) and the 125 k-graph config-5 ER share (LISTED and
CLOSURE through the LDS matrix).  `python profiles/tools/time_graph_keys.py OUT_DIR` writes OUT_DIR/time_graph_keys.json (the
figures of profiles/graph_keys/timing.md) and prints one line per input."""
import ctypes
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
gtok = importlib.import_module("glearning-benchmark_amd")
DEV = "cuda:0"
HBM_PEAK = 8.0e12          # bytes / s, MI355X specification


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


def torch_route(b, closure, attrs):
    """the canonical lists of every graph of the batch, as ops._canonical_lists builds them for the graphs it has to compare"""
    gs = torch.arange(b.num_graphs, device=b.device)
    return gtok.ops._canonical_lists([b], [0, b.num_graphs], gs, closure, attrs)


def one(name, b, labels, runs):
    G = b.num_graphs
    out = dict(graphs=G, nodes=b.num_nodes_total, entries=b.num_edges_total, max_nodes=b.max_nodes, flags=b.flags)
    for tag, mode, attrs in runs:
        flags = gtok.ops._keys_flags([b], mode, attrs)
        keys = torch.empty((G, 2), dtype=torch.int64, device=DEV)
        info = torch.zeros(4, dtype=torch.int32, device=DEV)
        cs = b.c_struct()
        lib, st = gtok._lib.lib(), gtok.ops._stream(DEV)
        call = lambda: lib.gtok_graph_keys(ctypes.byref(cs), labels.data_ptr(), flags, keys.data_ptr(), info.data_ptr(), st)
        assert call() == 0
        r = events(call)
        read = 4 * (b.num_nodes_total + G) + 4 * b.num_edges_total + 4 * (G + 1) + 8 * (G + 1) + 4 * G      # rowptr, col, node_ptr, edge_ptr, labels
        if attrs:
            read += b.num_nodes_total + b.num_edges_total
        r["bytes_read"] = int(read)
        r["bytes_per_s"] = read / (r["ms_median"] * 1e-3)
        r["fraction_of_hbm_peak"] = r["bytes_per_s"] / HBM_PEAK
        r["info"] = info.tolist()
        r["ops_graph_keys"] = events(lambda: gtok.ops.graph_keys(b, labels, mode, attrs))
        r["torch_route"] = events(lambda: torch_route(b, mode == "closure", attrs), warmup=1, reps=5)
        out[tag] = r
    print(name, json.dumps(out), flush=True)
    return out


def main():
    res = dict(hbm_peak_bytes_per_s=HBM_PEAK)
    d = gtok.synth.zinc_like(249_456, seed=0)
    b = gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], d["x"], d["edge_attr"]).to(DEV)
    labels = torch.zeros(b.num_graphs, dtype=torch.int32, device=DEV)
    res["zinc_full_249456"] = one("zinc_full_249456", b, labels, (("listed_attrs", "listed", True), ("listed", "listed", False), ("closure_reg", "closure", False)))
    d = gtok.synth.er_batch_device(125_000, DEV, seed=0)
    b = gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"]).to(DEV)
    labels = torch.zeros(b.num_graphs, dtype=torch.int32, device=DEV)
    res["config5_er_125k"] = one("config5_er_125k", b, labels, (("listed", "listed", False), ("closure_lds", "closure", False)))
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "time_graph_keys.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
