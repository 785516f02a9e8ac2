"""SENT rows -> batched CSR, timed two ways on the same rows.  Recorded, not gated.

    python profiles/tools/time_sent_decode_csr.py OUT_DIR      (copy OUT_DIR/timing.md to profiles/sent_decode_csr/)

new  ops.sent_decode_csr: gtok_sent_decode_sizes, two prefix sums, one read-back of the totals, gtok_sent_decode_csr, one
     read-back of info - straight from the rows as they are (16-bit slab / int32 slab).
old  what the library offered before: rows re-padded to int32 where they are 16-bit (ops.unpack_rows), gtok_sent_decode with
     edge_cap = ld and node_cap = max_num_nodes, a torch interleave of the padded edge arrays, GraphBatch.from_coo_device.
Shapes: (zinc) 249,456 ZINC-like molecules, labelled, one epoch of 16-bit rows, max_len 1024; (config5) 125,000 unlabelled ER
graphs of 10-256 nodes cut at 600 tokens, int32 rows.  Every figure is wall time around a device synchronise (both routes read
back from the device).  This driver starts PROCS fresh processes per shape, each under a time limit of its own; a process
warms both routes up, then times them alternately REPEATS times and reports its medians; the table holds the median, min and
max of the processes' medians.  One more process records the peak device memory of both routes on a batch of 1,000 molecules
and one 16,384-node ring.  A process that fails stops the run."""
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PROCS, REPEATS = int(os.environ.get("PROCS", 3)), int(os.environ.get("REPEATS", 5))
LIMIT = int(os.environ.get("CHILD_LIMIT", 240))       # seconds per process


# ------------------------------------------------------------------------------------------------ the two routes (child side)
def old_route(gtok, torch, ids, ln, maxn, labeled, nt, phases=None):
    dev, (G, ld) = ids.device, ids.shape
    t = [time.perf_counter()]

    def mark():
        if phases is not None:
            torch.cuda.synchronize(); t.append(time.perf_counter())
    if ids.dtype == torch.int16:
        ids = gtok.ops.unpack_rows(ids, None, ln, ld, 5)
    mark()
    r = gtok.ops.sent_decode(ids, ln, maxn, labeled, nt, edge_cap=ld, node_cap=maxn)
    mark()
    ok = r["status"] != 1
    m, n = torch.where(ok, r["num_edges"], 0), torch.where(ok, r["num_nodes"], 0)
    inside = torch.arange(ld, device=dev)[None, :] < m[:, None]
    a, b = r["edge_a"][inside], r["edge_b"][inside]
    keep = torch.stack([torch.ones_like(a, dtype=torch.bool), a != b], 1)
    src, dst = torch.stack([a, b], 1)[keep], torch.stack([b, a], 1)[keep]
    gid = torch.repeat_interleave(torch.arange(G, device=dev), m.to(torch.int64))
    ec = 2 * m.to(torch.int64) - torch.bincount(gid[a == b], minlength=G)
    x = ea = None
    if labeled:
        ty = r["edge_type"][inside]
        ea = torch.stack([ty, ty], 1)[keep]
        x = r["node_type"][torch.arange(maxn, device=dev)[None, :] < n[:, None]]
    mark()
    batch = gtok.GraphBatch.from_coo_device(n, ec, src, dst, x, ea, device=dev, check_symmetric=False)
    mark()
    if phases is not None:
        for k, d in zip(("repad", "gtok_sent_decode", "interleave", "from_coo_device"), (t[i + 1] - t[i] for i in range(4))):
            phases.setdefault(k, []).append(d * 1e3)
    return batch


def new_route(gtok, torch, ids, ln, maxn, labeled, nt, phases=None):
    if phases is None:
        return gtok.ops.sent_decode_csr(ids, ln, maxn, labeled, nt)[0]
    sync = torch.cuda.synchronize
    sync(); t0 = time.perf_counter()
    nn, ne, _ = gtok.ops.sent_decode_sizes(ids, ln, maxn, labeled, nt)
    sync(); t1 = time.perf_counter()
    rows = ln.numel()
    np64 = torch.zeros(rows + 1, dtype=torch.int64, device=ids.device); torch.cumsum(nn, 0, dtype=torch.int64, out=np64[1:])
    ep = torch.zeros(rows + 1, dtype=torch.int64, device=ids.device); torch.cumsum(ne, 0, dtype=torch.int64, out=ep[1:])
    N, E = torch.stack([np64[-1], ep[-1]]).tolist()
    t2 = time.perf_counter()
    o = gtok.ops._decode_csr_launch(ids, ln, None, None, maxn, labeled, nt, np64.to(torch.int32), ep, N, E)
    sync(); t3 = time.perf_counter()
    for k, d in (("gtok_sent_decode_sizes", t1 - t0), ("prefix_sums_and_totals", t2 - t1), ("gtok_sent_decode_csr", t3 - t2)):
        phases.setdefault(k, []).append(d * 1e3)
    return o


def same(torch, a, b):
    eq = lambda x, y: (x is None and y is None) or (x is not None and y is not None and torch.equal(x, y))
    return all(eq(getattr(a, k), getattr(b, k)) for k in ("node_ptr", "edge_ptr", "rowptr", "col", "eorder", "nattr", "eattr")) and \
        (a.max_degree, a.max_nodes, a.max_edges, a.chunk_nodes, a.chunk_edges) == (b.max_degree, b.max_nodes, b.max_edges, b.chunk_nodes, b.chunk_edges)


def child(shape: str) -> dict:
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    gtok = importlib.import_module("glearning-benchmark_amd")
    dev = torch.device("cuda:0")
    med = lambda v: sorted(v)[len(v) // 2]
    if shape == "zinc":
        d = gtok.synth.zinc_like(249456, seed=1000)
        b = gtok.GraphBatch.from_coo_device(d["node_counts"], d["edge_counts"], d["src"], d["dst"], d["x"], d["edge_attr"], device=dev)
        maxn, labeled, nt = b.max_nodes, True, 9
        ids, ln = gtok.ops.sent(b, maxn, 1024, 0, 0, labeled=True, num_node_types=9, num_edge_types=4, u16=True)
    elif shape == "config5":
        d = gtok.synth.er_batch_device(125000, dev, seed=1000)
        b = gtok.GraphBatch.from_coo_device(d["node_counts"], d["edge_counts"], d["src"], d["dst"], device=dev)
        maxn, labeled, nt = b.max_nodes, False, 0
        ids, ln = gtok.ops.sent(b, maxn, 600, 0, 0)
    else:                                    # peak memory: 1,000 molecules (unlabelled) and one ring of 16,384 nodes listed one way
        z = gtok.synth.zinc_like(1000, seed=3)
        a = np.arange(16384, dtype=np.int64)
        nc, ec = np.concatenate([z["node_counts"], [16384]]), np.concatenate([z["edge_counts"], [16384]])
        b = gtok.GraphBatch.from_coo(nc, ec, np.concatenate([z["src"], a]), np.concatenate([z["dst"], (a + 1) % 16384])).to(dev)
        maxn, labeled, nt = 16384, False, 0
        ids, ln = gtok.ops.sent_large(b, maxn, 1 << 20, 0, 0)
    del b
    torch.cuda.synchronize()
    res = dict(shape=shape, rows=int(ids.shape[0]), ld=int(ids.shape[1]), id_bytes=ids.element_size(), tokens=int(torch.clamp(ln, max=ids.shape[1]).sum()),
               device=f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]}; "
                      f"library built for {gtok.lib().gtok_target().decode()})")
    routes = dict(new=new_route, old=old_route)
    if shape == "peak":
        for name, f in routes.items():
            torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = f(gtok, torch, ids, ln, maxn, labeled, nt)
            torch.cuda.synchronize()
            res[name + "_peak_mb"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            res[name + "_result_mb"] = (torch.cuda.memory_allocated() - base) / 2 ** 20
            del out
        res["rows_mb"] = ids.numel() * ids.element_size() / 2 ** 20
        return res
    outs = {k: f(gtok, torch, ids, ln, maxn, labeled, nt) for k, f in routes.items()}      # warm-up, and the two results compared
    res["equal"] = same(torch, outs["new"], outs["old"])
    res["nodes"], res["entries"] = outs["new"].num_nodes_total, outs["new"].num_edges_total
    del outs
    times = dict(new=[], old=[])
    for _ in range(REPEATS):
        for name, f in routes.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            out = f(gtok, torch, ids, ln, maxn, labeled, nt)
            torch.cuda.synchronize(); times[name].append((time.perf_counter() - t0) * 1e3)
            del out
    phases = dict(new={}, old={})
    for _ in range(3):
        for name, f in routes.items():
            out = f(gtok, torch, ids, ln, maxn, labeled, nt, phases=phases[name])
            del out
    res.update(new_ms=med(times["new"]), old_ms=med(times["old"]),
               phases={r: {k: med(v) for k, v in p.items()} for r, p in phases.items()})
    return res


# ------------------------------------------------------------------------------------------------ the driver
def main():
    if len(sys.argv) < 2 or (sys.argv[1] == "--child" and len(sys.argv) < 3):
        sys.exit("usage: python profiles/tools/time_sent_decode_csr.py OUT_DIR")
    if sys.argv[1] == "--child":
        print("RESULT " + json.dumps(child(sys.argv[2])))
        return
    out_dir = sys.argv[1]
    os.makedirs(out_dir, exist_ok=True)
    runs = []
    for shape, n in (("zinc", PROCS), ("config5", PROCS), ("peak", 1)):
        for i in range(n):
            p = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child", shape],
                               capture_output=True, text=True)
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(p.stdout[-2000:], p.stderr[-4000:])
                sys.exit(f"process {i} of shape {shape} ended with status {p.returncode}: stopping")
            runs.append(json.loads(line[0][7:]))
            print(runs[-1], flush=True)
            with open(os.path.join(out_dir, "timing.json"), "w") as f:
                json.dump(runs, f, indent=1)
    stat = lambda v: f"{sorted(v)[len(v) // 2]:.2f} ({min(v):.2f} - {max(v):.2f})"
    lines = ["# SENT rows -> batched CSR: timing", "",
             f"`python profiles/tools/time_sent_decode_csr.py OUT_DIR` on {runs[0]['device']}.  Wall time around a device synchronise, ms per call of the whole route.  "
             f"{PROCS} fresh processes per shape; each warms both routes up and times them alternately {REPEATS} times; a cell is the median (min - max) of the "
             "processes' medians.  new = `ops.sent_decode_csr` on the rows as they are; old = re-pad to int32 where needed, `gtok_sent_decode` with "
             "edge_cap = ld, a torch interleave, `GraphBatch.from_coo_device`.", "",
             "| shape | rows | ld | bytes per id | tokens | new, ms | old, ms | results equal |", "|---|---|---|---|---|---|---|---|"]
    for shape in ("zinc", "config5"):
        rs = [r for r in runs if r["shape"] == shape]
        r0 = rs[0]
        lines.append(f"| {shape} | {r0['rows']:,} | {r0['ld']} | {r0['id_bytes']} | {r0['tokens']:,} | {stat([r['new_ms'] for r in rs])} | "
                     f"{stat([r['old_ms'] for r in rs])} | {all(r['equal'] for r in rs)} |")
    lines += ["", "Phases (each closed by a synchronise of its own, so they add up to more than the route; medians of three, first process), ms:", ""]
    for shape in ("zinc", "config5"):
        r0 = [r for r in runs if r["shape"] == shape][0]
        for route in ("new", "old"):
            lines.append(f"* {shape}, {route}: " + ", ".join(f"{k} {v:.2f}" for k, v in r0["phases"][route].items()))
    pk = [r for r in runs if r["shape"] == "peak"][0]
    lines += ["", f"Peak device memory beyond the rows themselves, 1,000 molecules and one 16,384-node ring ({pk['rows']:,} rows x {pk['ld']:,} int32 ids = "
              f"{pk['rows_mb']:.0f} MB): new {pk['new_peak_mb']:.1f} MB (the result: {pk['new_result_mb']:.1f} MB), old {pk['old_peak_mb']:.1f} MB "
              f"(the result: {pk['old_result_mb']:.1f} MB).", ""]
    with open(os.path.join(out_dir, "timing.md"), "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
