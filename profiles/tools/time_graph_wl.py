"""Timing of gtok_graph_wl with HIP events, beside the same refinement written with torch on the device (index_add_ over the entry
list: the only route to such keys without the kernel; its keys are checked against the kernel's before anything is timed) and beside
gtok_graph_keys on the same batch (the cost of one streaming pass).  Inputs: a ZINC-full-shaped batch (zinc_like(249,456): ATTRS
through the csr kernel, structure only through the register kernel) and the 125 k-graph config-5 ER share (structure only through
the LDS matrix), 3 rounds.  `python profiles/tools/time_graph_wl.py OUT_DIR` writes OUT_DIR/time_graph_wl.json (the figures of
profiles/graph_wl/timing.md) and prints one line per input."""
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
ROUNDS = 3


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


# ---- the refinement in torch: int64 arithmetic wraps mod 2^64, a logical right shift is an arithmetic one with the sign bits masked
def _s(c):
    return c - (1 << 64) if c >= 1 << 63 else c


C0, C1, D0, D1 = (_s(c) for c in (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63))


def _shr(z, k):
    return (z >> k) & ((1 << (64 - k)) - 1)


def _mix(z):
    z = (z ^ _shr(z, 30)) * _s(0xBF58476D1CE4E5B9)
    z = (z ^ _shr(z, 27)) * _s(0x94D049BB133111EB)
    return z ^ _shr(z, 31)


def torch_route(b, rounds, attrs, both_directions):
    """keys int64 [G, 2] of a batch of SIMPLE graphs (listed once: both_directions adds the way back; or flagged): every step a torch
    op over the node or the entry list - row ids by repeat_interleave, degrees by bincount, a round by a gather, a mix and index_add_"""
    dev, G = b.device, b.num_graphs
    nptr = b.node_ptr.to(torch.int64)
    nc = nptr[1:] - nptr[:-1]
    N = b.num_nodes_total
    gid = torch.repeat_interleave(torch.arange(G, device=dev), nc)
    rows = torch.arange(N, device=dev) + gid                                 # where node v's row bounds sit in rowptr
    deg_listed = (b.rowptr[rows + 1] - b.rowptr[rows]).to(torch.int64)
    v = torch.repeat_interleave(torch.arange(N, device=dev), deg_listed)     # global node of every entry's row
    u = b.col.to(torch.int64) + nptr[gid[v]]
    t = (1 + b.eattr.to(torch.int64)) * D1 if attrs else None
    if both_directions:
        v, u = torch.cat([v, u]), torch.cat([u, v])
    deg = torch.bincount(v, minlength=N)
    a = (1 + b.nattr.to(torch.int64)) << 16 if attrs else 0
    c = _mix((deg | a) ^ C0)
    for _ in range(rounds):
        term = _mix(c[u] ^ C1 ^ t) if attrs else _mix(c ^ C1)[u]
        c = _mix((c.clone().index_add_(0, v, term)) ^ D0)
    keys = torch.empty((G, 2), dtype=torch.int64, device=dev)
    head = nc | (rounds << 32)
    for j, (C, D) in enumerate(((C0, D0), (C1, D1))):
        S = torch.zeros(G, dtype=torch.int64, device=dev).index_add_(0, gid, _mix(c ^ C))
        keys[:, j] = _mix(S + _mix(head ^ C) + _mix(torch.zeros_like(nc) ^ D))
    return keys


def one(name, b, runs, both_directions):
    G = b.num_graphs
    out = dict(graphs=G, nodes=b.num_nodes_total, entries=b.num_edges_total, max_nodes=b.max_nodes, flags=b.flags, rounds=ROUNDS)
    lib, st = gtok._lib.lib(), gtok.ops._stream(DEV)
    cs = b.c_struct()
    labels = torch.zeros(G, dtype=torch.int32, device=DEV)
    keys = torch.empty((G, 2), dtype=torch.int64, device=DEV)
    colors = torch.empty(b.num_nodes_total, dtype=torch.int64, device=DEV)
    info = torch.zeros(4, dtype=torch.int32, device=DEV)
    for tag, attrs, kernel in runs:
        flags = gtok._lib.WL_ATTRS if attrs else 0
        if kernel:
            os.environ["GTOK_WL_KERNEL"] = kernel
        call = lambda with_colors=True: lib.gtok_graph_wl(ctypes.byref(cs), labels.data_ptr(), ROUNDS, flags, keys.data_ptr(),
                                                          colors.data_ptr() if with_colors else None, info.data_ptr(), None, 0, st)
        assert call() == 0
        r = events(call)
        r["without_colors"] = events(lambda: call(False))
        r["keys_equal_torch_route"] = bool(torch.equal(keys, torch_route(b, ROUNDS, attrs, both_directions)))
        read = 4 * (b.num_nodes_total + G) + 4 * b.num_edges_total + 4 * (G + 1) + 8 * (G + 1) + 4 * G      # rowptr, col, node_ptr, edge_ptr, labels
        if attrs:
            read += b.num_nodes_total + b.num_edges_total
        r["bytes_read_once"] = int(read)
        r["bytes_written"] = int(16 * G + 8 * b.num_nodes_total)
        r["fraction_of_hbm_peak"] = (read + r["bytes_written"]) / (r["ms_median"] * 1e-3) / HBM_PEAK
        r["info"] = info.tolist()
        r["ops_graph_wl_keys"] = events(lambda: gtok.ops.graph_wl_keys(b, ROUNDS, labels, attrs, with_colors=True))
        os.environ.pop("GTOK_WL_KERNEL", None)
        r["torch_route"] = events(lambda: torch_route(b, ROUNDS, attrs, both_directions), warmup=1, reps=5)
        out[tag] = r
    out["graph_keys_listed"] = events(lambda: gtok.ops.graph_keys(b, labels, "listed", b.nattr is not None))
    out["graph_keys_closure"] = events(lambda: gtok.ops.graph_keys(b, labels, "closure"))
    print(name, json.dumps(out), flush=True)
    return out


def main():
    res = dict(hbm_peak_bytes_per_s=HBM_PEAK)
    d = gtok.synth.zinc_like(249_456, seed=0)
    b = gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], d["x"], d["edge_attr"]).to(DEV)
    res["zinc_full_249456"] = one("zinc_full_249456", b, (("attrs_csr", True, None), ("structure_reg", False, None), ("structure_csr", False, "csr")), False)
    d = gtok.synth.er_batch_device(125_000, DEV, seed=0)
    b = gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"]).to(DEV)
    res["config5_er_125k"] = one("config5_er_125k", b, (("structure_lds", False, None),), True)
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "time_graph_wl.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
