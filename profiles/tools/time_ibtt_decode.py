"""IBTT rows -> batched CSR, timed beside the project's other decoder and the host route.  Recorded, not gated.

    python profiles/tools/time_ibtt_decode.py OUT_DIR      (copy OUT_DIR/timing.md to profiles/ibtt_decode/)

Workloads: (zinc) 249,456 ZINC-like molecules serialised by gtok_ibtt_zinc, int32 rows, ld 240; (config5) 125,000 ER graphs of
10-256 nodes serialised by gtok_ibtt_synth at max_len 600, int32 rows.  Per workload: gtok_ibtt_decode_sizes, gtok_ibtt_decode_csr
(each closed by a synchronise of its own), the whole ops.ibtt_decode_csr call; ops.sent_decode_csr on the SENT rows of the same
graphs (16-bit labelled rows / int32 rows cut at 600, the shapes of profiles/sent_decode_csr/timing.md); and the only route
there was before: a D2H copy of SAMPLE rows and the host reference decoder of tests/_ibtt_decode_ref.py over them.  Wall time
around a device synchronise.  One fresh process per workload, each under a time limit of its own; a process warms every route
up, then times them alternately REPEATS times; a cell is the median (min - max).  A process that fails stops the run."""
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPEATS, SAMPLE = int(os.environ.get("REPEATS", 7)), int(os.environ.get("SAMPLE", 2000))
LIMIT = int(os.environ.get("CHILD_LIMIT", 240))       # seconds per process

ZINC_FIXED = ["<bos>", "<eos>", "<pad>", "<unk>", "<q>", "<p>", "<atom>", "<bond>", "C", "N", "O", "F", "P", "S", "Cl", "Br", "I",
              "single", "double", "triple", "aromatic", "regression", "X", "unknown"]


def child(shape: str) -> dict:
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    gtok = importlib.import_module("glearning-benchmark_amd")
    import _ibtt_decode_ref as ref
    ops, dev = gtok.ops, torch.device("cuda:0")
    sync = torch.cuda.synchronize
    if shape == "zinc":
        d = gtok.synth.zinc_like(249456, seed=1000)
        b = gtok.GraphBatch.from_coo_device(d["node_counts"], d["edge_counts"], d["src"], d["dst"], d["x"], d["edge_attr"], device=dev)
        maxn, grammar = b.max_nodes, "zinc"
        vocab = {t: i for i, t in enumerate(ZINC_FIXED + [str(i) for i in range(maxn)])}
        lut = ops.zinc_lut(vocab, maxn)
        ids, ln = ops.ibtt_zinc(b, lut, 240, vocab["<pad>"], ld=240)
        sent_args = (maxn, True, 28)
        sids, sln = ops.sent(b, maxn, 1024, 0, 0, labeled=True, num_node_types=28, num_edge_types=4, u16=True)
    else:
        d = gtok.synth.er_batch_device(125000, dev, seed=1000)
        b = gtok.GraphBatch.from_coo_device(d["node_counts"], d["edge_counts"], d["src"], d["dst"], device=dev)
        maxn, grammar = b.max_nodes, "synth"
        vocab = {t: i for i, t in enumerate(["<pad>", "<bos>", "<eos>", "<e>", "<n>", "<q>", "<p>", "yes", "no"] + [str(i) for i in range(maxn)])}
        lut = ops.synth_lut(vocab, maxn)
        ids, ln = ops.ibtt_synth(b, lut, None, 600, vocab["<pad>"], ld=600)
        sent_args = (maxn, False, 0)
        sids, sln = ops.sent(b, maxn, 600, 0, 0)
    del b
    inv = ops.ibtt_inverse_lut(lut, len(vocab), vocab["<pad>"]).to(dev)
    rows = int(ln.numel())
    sync()
    res = dict(shape=shape, rows=rows, ld=int(ids.shape[1]), tokens=int(torch.clamp(ln, max=ids.shape[1]).sum()), sent_ld=int(sids.shape[1]),
               sent_id_bytes=sids.element_size(), sent_tokens=int(torch.clamp(sln, max=sids.shape[1]).sum()),
               device=f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]}; "
                      f"library built for {gtok.lib().gtok_target().decode()})")

    def sizes():
        return ops.ibtt_decode_sizes(ids, ln, grammar, inv, maxn)

    nn, ne, st = sizes()
    np64 = torch.zeros(rows + 1, dtype=torch.int64, device=dev); torch.cumsum(nn, 0, dtype=torch.int64, out=np64[1:])
    ep = torch.zeros(rows + 1, dtype=torch.int64, device=dev); torch.cumsum(ne, 0, dtype=torch.int64, out=ep[1:])
    N, E = int(np64[-1]), int(ep[-1])
    np32 = np64.to(torch.int32)
    res.update(nodes=N, entries=E, status={str(k): int((st == k).sum()) for k in (0, 1, 3)})

    def host():
        h_ids, h_ln = ids[:SAMPLE].cpu().numpy(), ln[:SAMPLE].cpu().numpy()
        return ref.expected(ref.rows_of(h_ids, h_ln), ops._ibtt_grammar(grammar), inv_h, maxn)

    inv_h = inv.cpu().numpy()
    routes = dict(sizes=sizes,
                  csr=lambda: ops._ibtt_decode_csr_launch(ids, ln, None, None, grammar, inv, maxn, np32, ep, N, E),
                  whole=lambda: ops.ibtt_decode_csr(ids, ln, grammar, inv, maxn),
                  sent_whole=lambda: ops.sent_decode_csr(sids, sln, *sent_args),
                  host_sample=host)
    # the device result over the sample equals the host reference's (the routes compute the same thing)
    got = ops.ibtt_decode_csr(ids[:SAMPLE].contiguous(), ln[:SAMPLE].contiguous(), grammar, inv, maxn)[0]
    want = host()["batch"]
    res["equal_on_sample"] = all(torch.equal(getattr(got, k).cpu(), getattr(want, k)) for k in ("node_ptr", "edge_ptr", "rowptr", "col"))
    for f in routes.values():
        f()
    times = {k: [] for k in routes}
    for _ in range(REPEATS):
        for name, f in routes.items():
            sync(); t0 = time.perf_counter()
            out = f()
            sync(); times[name].append((time.perf_counter() - t0) * 1e3)
            del out
    res["ms"] = {k: [sorted(v)[len(v) // 2], min(v), max(v)] for k, v in times.items()}
    return res


def main():
    if len(sys.argv) < 2 or (sys.argv[1] == "--child" and len(sys.argv) < 3):
        sys.exit("usage: python profiles/tools/time_ibtt_decode.py OUT_DIR")
    if sys.argv[1] == "--child":
        print("RESULT " + json.dumps(child(sys.argv[2])))
        return
    out_dir = sys.argv[1]
    os.makedirs(out_dir, exist_ok=True)
    runs = []
    for shape in ("zinc", "config5"):
        p = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child", shape], capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(p.stdout[-2000:], p.stderr[-4000:])
            sys.exit(f"the process of shape {shape} ended with status {p.returncode}: stopping")
        runs.append(json.loads(line[0][7:]))
        print(runs[-1], flush=True)
        with open(os.path.join(out_dir, "timing.json"), "w") as f:
            json.dump(runs, f, indent=1)
    cell = lambda v: f"{v[0]:.2f} ({v[1]:.2f} - {v[2]:.2f})"
    lines = ["# IBTT rows -> batched CSR: timing", "",
             f"`python profiles/tools/time_ibtt_decode.py OUT_DIR` on {runs[0]['device']}.  Wall time around a device synchronise, ms per call; one fresh "
             f"process per workload, every route warmed up, then timed alternately {REPEATS} times; a cell is the median (min - max).  sizes / csr = the two "
             "entry points alone; whole = `ops.ibtt_decode_csr` (both passes, two prefix sums, two read-backs); SENT = `ops.sent_decode_csr` on the SENT rows "
             f"of the same graphs; host = a D2H copy of the first {SAMPLE:,} rows and the host reference decoder (tests/_ibtt_decode_ref.py) over them.", "",
             "| workload | rows | ld | tokens | status 0 / 1 / 3 | sizes, ms | csr, ms | whole, ms | SENT rows: ld, bytes per id, tokens | SENT whole, ms | "
             f"host, {SAMPLE:,} rows, ms | host, all rows (scaled), s | equal on the sample |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in runs:
        m, s = r["ms"], r["status"]
        lines.append(f"| {r['shape']} | {r['rows']:,} | {r['ld']} | {r['tokens']:,} | {s['0']:,} / {s['1']:,} / {s['3']:,} | {cell(m['sizes'])} | {cell(m['csr'])} | "
                     f"{cell(m['whole'])} | {r['sent_ld']}, {r['sent_id_bytes']}, {r['sent_tokens']:,} | {cell(m['sent_whole'])} | {cell(m['host_sample'])} | "
                     f"{m['host_sample'][0] * r['rows'] / SAMPLE / 1e3:.1f} | {r['equal_on_sample']} |")
    with open(os.path.join(out_dir, "timing.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
