"""HIP builder (gtok_csr_from_coo behind GraphBatch.from_coo_device) against the torch chain (builder="torch") on inputs
already in HBM, alternated in one process, symmetry check included; one JSON line per corpus.

    python profiles/tools/coo_build_timing.py [--reps 7] [--shares 125000]
"""
import argparse
import importlib
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
gtok = importlib.import_module("glearning-benchmark_amd")


def corpus_on_device(d, labeled, dev):
    t = lambda a: torch.as_tensor(a).to(dev, dtype=torch.int64)
    args = [t(d[k]) for k in ("node_counts", "edge_counts", "src", "dst")]
    return args + ([t(d["x"]), t(d["edge_attr"])] if labeled else [None, None])


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def h2d_split(dev, reps):
    """Storage held on the host (the bench's boundary.csr_ingestion leg): from_collated(device=...) pays the upload of the
    int64 arrays whatever the builder; timed whole, the upload alone (pageable host memory, as the leg does it), and the
    build from the uploaded arrays."""
    d = gtok.synth.zinc_like(249456, seed=1000)
    ds = gtok.synth.InMemoryLike(d)
    st = gtok.csr.collated_storage(ds)
    host = [torch.as_tensor(st[k]) for k in ("node_counts", "edge_index", "edge_slices", "x", "edge_attr")]
    whole = lambda: gtok.GraphBatch.from_dataset(ds, device=dev)
    up = {}
    def upload():
        up["t"] = [t.to(dev, dtype=torch.int64) for t in host]
    def build():
        nc, ei, es, x, ea = up["t"]
        gtok.GraphBatch.from_collated(nc, ei, es, x, ea, device=dev)
    whole(); upload(); build()
    t = {"whole": [], "upload": [], "build": []}
    for _ in range(reps):
        t["whole"] += timed(whole, 1); t["upload"] += timed(upload, 1); t["build"] += timed(build, 1)
    med = lambda v: sorted(v)[len(v) // 2]
    mb = sum(x.numel() * 8 for x in host) / 1e6
    print(json.dumps(dict(corpus="zinc_full_host_storage", collated_storage_ms=round(med(t["whole"]) * 1e3, 3),
                          h2d_ms=round(med(t["upload"]) * 1e3, 3), build_from_device_storage_ms=round(med(t["build"]) * 1e3, 3),
                          h2d_mb=round(mb, 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shares", type=int, default=125000)
    ap.add_argument("--h2d-only", action="store_true", help="only the split of host-held ZINC-full storage: H2D copy vs build")
    a = ap.parse_args()
    dev = "cuda:0"
    h2d_split(dev, a.reps)
    if a.h2d_only:
        return
    corpora = [("zinc_full", gtok.synth.zinc_like(249456, seed=0), True),
               ("synth_er_share", gtok.synth.er_batch_device(a.shares, dev, seed=0), False),
               ("synth_mix_share", gtok.synth.mix_batch_device(a.shares, dev, seed=0), False)]
    for name, d, labeled in corpora:
        args = corpus_on_device(d, labeled, dev)
        run = {b: (lambda b=b: gtok.GraphBatch.from_coo_device(*args, device=dev, builder=b)) for b in ("auto", "torch")}
        for f in run.values():
            f()
        t = {"auto": [], "torch": []}
        for _ in range(a.reps):                       # alternated
            for b in ("auto", "torch"):
                t[b] += timed(run[b], 1)
        in_bytes = sum(x.numel() * 8 for x in args if x is not None)
        g = run["auto"]()
        out_bytes = sum(x.numel() * x.element_size() for x in (g.node_ptr, g.edge_ptr, g.rowptr, g.col, g.nattr, g.eattr) if x is not None)
        med = lambda v: sorted(v)[len(v) // 2]
        hip = med(t["auto"])
        print(json.dumps(dict(corpus=name, graphs=len(d["node_counts"]), entries=int(args[2].numel()), hip_ms=round(hip * 1e3, 3),
                              torch_ms=round(med(t["torch"]) * 1e3, 3), hip_min_ms=round(min(t["auto"]) * 1e3, 3),
                              in_mb=round(in_bytes / 1e6, 1), out_mb=round(out_bytes / 1e6, 1),
                              roofline_fraction_8tbs=round((in_bytes + out_bytes) / 8e12 / hip, 4))), flush=True)


if __name__ == "__main__":
    main()
