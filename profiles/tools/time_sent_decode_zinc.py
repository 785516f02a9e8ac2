"""ZINC-remapped SENT rows -> batched CSR, timed beside the un-remapped decoder on rows of the same walk.  Recorded, not gated.

    python profiles/tools/time_sent_decode_zinc.py PARENT_LIB OUT_DIR      (copy OUT_DIR/timing.md to profiles/sent_decode_zinc/)

Shape: 249,456 ZINC-like molecules (ZINC-full), labelled, 37 nodes, 28 node types, 4 edge types, one epoch, max_len 1024, as a
16-bit slab and as 8-bit packed rows (rows from multiples of 16 ids).
(a) ops.sent_decode_csr on the UN-remapped rows, with the parent's library (PARENT_LIB, loaded through GTOK_LIB) and this tree's, in
    PROCS fresh processes each, the two alternating in who goes first: did the existing kernels change?
(b) ops.sent_decode_zinc_csr on the remapped rows of the same walk, in the same processes of this tree's library, against (a).
(c) gtok_unremap_zinc alone (device events around 20 launches), with the bytes it reads and writes per second.
Routes are wall time around a device synchronise (they read back twice); a process warms everything up, times the routes
alternately REPEATS times and reports medians.  Each process runs under a time limit of its own; one that fails stops the run."""
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PROCS, REPEATS = int(os.environ.get("PROCS", 5)), int(os.environ.get("REPEATS", 7))
LIMIT = int(os.environ.get("CHILD_LIMIT", 240))       # seconds per process
G, M, T, ET, MAX_LEN = int(os.environ.get("GRAPHS", 249456)), 37, 28, 4, 1024
med = lambda v: sorted(v)[len(v) // 2]


def child() -> dict:
    import torch
    sys.path.insert(0, ROOT)
    gtok = importlib.import_module("glearning-benchmark_amd")
    ops, dev = gtok.ops, torch.device("cuda:0")
    d = gtok.synth.zinc_like(G, seed=1000)
    b = gtok.GraphBatch.from_coo_device(d["node_counts"], d["edge_counts"], d["src"], d["dst"], d["x"], d["edge_attr"], device=dev)
    kw = dict(labeled=True, num_node_types=T, num_edge_types=ET, u16=True)
    raw, ln = ops.sent(b, M, MAX_LEN, 0, 0, **kw)
    zinc, zln = ops.sent(b, M, MAX_LEN, 0, 0, remap_zinc=True, **kw)
    del b
    ld = int(raw.shape[1])
    pack = lambda ids: ops.pack_rows_scan(ids, ln, 1, int(torch.clamp(ln, max=ld).sum()) + 16 * G, 16)
    raw8, rptr, s1 = pack(raw)
    zinc8, zptr, s2 = pack(zinc)
    assert torch.equal(ln, zln) and int(s1.item()) == 0 and int(s2.item()) == 0
    rstart, zstart = rptr[:-1].contiguous(), zptr[:-1].contiguous()
    has_zinc = all(hasattr(gtok.lib(), n) for n in gtok._lib.ZINC_DECODE_SYMBOLS)
    routes = {"raw_u16": lambda: ops.sent_decode_csr(raw, ln, M, True, T),
              "raw_u8": lambda: ops.sent_decode_csr(raw8, ln, M, True, T, row_start=rstart, ld=ld)}
    if has_zinc:
        routes["zinc_u16"] = lambda: ops.sent_decode_zinc_csr(zinc, ln, M, T)
        routes["zinc_u8"] = lambda: ops.sent_decode_zinc_csr(zinc8, ln, M, T, row_start=zstart, ld=ld)
    outs = {k: f() for k, f in routes.items()}                                    # warm-up, and the results compared
    same = lambda x, y: all(torch.equal(getattr(x[0], k), getattr(y[0], k)) for k in ("node_ptr", "edge_ptr", "rowptr", "col", "nattr", "eattr")) \
        and torch.equal(x[1], y[1])
    res = dict(rows=G, ld=ld, tokens=int(torch.clamp(ln, max=ld).sum()), zinc=has_zinc, equal=all(same(o, outs["raw_u16"]) for o in outs.values()),
               device=f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]})")
    del outs
    times = {k: [] for k in routes}
    for _ in range(REPEATS):
        for k, f in routes.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            out = f()
            torch.cuda.synchronize(); times[k].append((time.perf_counter() - t0) * 1e3)
            del out
    res["ms"] = {k: med(v) for k, v in times.items()}
    if has_zinc:
        res["unremap"] = {}
        for name, ids, start in (("u16", zinc, None), ("u8", zinc8, zstart)):
            out = ops.unremap_zinc(ids, ln, M, T, row_start=start, ld=ld)
            ok = torch.equal(out, raw.to(torch.int32) & 0xFFFF) or bool(((out != (raw.to(torch.int32) & 0xFFFF)).sum(1) <= 1).all())
            per = []
            for _ in range(REPEATS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    ops.unremap_zinc(ids, ln, M, T, row_start=start, ld=ld)
                e1.record(); torch.cuda.synchronize()
                per.append(e0.elapsed_time(e1) / 20)
            read = res["tokens"] * ids.element_size() + G * (4 + (8 if start is not None else 0))
            res["unremap"][name] = dict(ms=med(per), read_bytes=read, written_bytes=G * ld * 4, ok=ok)
            del out
    return res


def main():
    if len(sys.argv) == 2 and sys.argv[1] == "--child":
        print("RESULT " + json.dumps(child()))
        return 0
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    parent_lib, out_dir = os.path.abspath(sys.argv[1]), sys.argv[2]
    os.makedirs(out_dir, exist_ok=True)
    sides = {"parent": [], "branch": []}
    for i in range(PROCS):
        for side in (("parent", "branch") if i % 2 == 0 else ("branch", "parent")):
            env = {k: v for k, v in os.environ.items() if k != "GTOK_LIB"}
            if side == "parent":
                env["GTOK_LIB"] = parent_lib
            t0 = time.perf_counter()
            p = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, env=env)
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(p.stdout[-2000:], p.stderr[-4000:])
                sys.exit(f"process {i} of the {side}'s library ended with status {p.returncode}: stopping")
            res = json.loads(line[0][7:])
            if not res["equal"] or res["zinc"] != (side == "branch"):
                sys.exit(f"process {i} of the {side}'s library: results differ, or the wrong library was loaded: stopping")
            sides[side].append(res)
            print(i, side, res["ms"], res.get("unremap"), f"({time.perf_counter() - t0:.0f} s)", flush=True)
            with open(os.path.join(out_dir, "timing.json"), "w") as f:
                json.dump(sides, f, indent=1)
    r0 = sides["branch"][0]
    cell = lambda v: ", ".join(f"{x:.3f}" for x in v) + f": {med(v):.3f}"
    lines = ["# ZINC-remapped SENT rows -> batched CSR: timing", "",
             f"`python profiles/tools/time_sent_decode_zinc.py PARENT_LIB OUT_DIR` on {r0['device']}.  {r0['rows']:,} ZINC-like molecules, labelled, one epoch: "
             f"{r0['tokens']:,} tokens in rows of ld {r0['ld']}, as a 16-bit slab and as 8-bit packed rows.  Wall time around a device synchronise, ms per call of "
             f"the whole route (sizes pass, prefix sums, read-back, CSR pass, read-back); {PROCS} fresh processes per library, the two alternating in who goes "
             f"first; a process reports the median of {REPEATS}; a cell lists the processes' medians, then their median.", "",
             "## (a) `ops.sent_decode_csr` on un-remapped rows: the parent's library against this one", "",
             "| rows | parent, ms | this build, ms | this build's median inside the parent's range | the parent's median inside this build's range |", "|---|---|---|---|---|"]
    for k in ("raw_u16", "raw_u8"):
        a, b = [r["ms"][k] for r in sides["parent"]], [r["ms"][k] for r in sides["branch"]]
        lines.append(f"| {k[4:]} | {cell(a)} | {cell(b)} | {min(a) <= med(b) <= max(a)} | {min(b) <= med(a) <= max(b)} |")
    lines += ["", "## (b) `ops.sent_decode_zinc_csr` on the remapped rows of the same walk, against (a) in the same process", "",
              "| rows | un-remapped, ms | remapped, ms | remapped / un-remapped per process |", "|---|---|---|---|"]
    for k in ("u16", "u8"):
        a, b = [r["ms"]["raw_" + k] for r in sides["branch"]], [r["ms"]["zinc_" + k] for r in sides["branch"]]
        lines.append(f"| {k} | {cell(a)} | {cell(b)} | {', '.join(f'{y / x:.3f}' for x, y in zip(a, b))} |")
    lines += ["", "## (c) `gtok_unremap_zinc` alone (device events around 20 launches)", "",
              "| rows | ms per launch | bytes read | bytes written | GB/s (read + written) | equals the raw rows (but for a cut row's last id) |", "|---|---|---|---|---|---|"]
    for k in ("u16", "u8"):
        u = [r["unremap"][k] for r in sides["branch"]]
        ms = med([x["ms"] for x in u])
        lines.append(f"| {k} | {cell([x['ms'] for x in u])} | {u[0]['read_bytes']:,} | {u[0]['written_bytes']:,} | "
                     f"{(u[0]['read_bytes'] + u[0]['written_bytes']) / ms / 1e6:.0f} | {all(x['ok'] for x in u)} |")
    with open(os.path.join(out_dir, "timing.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
