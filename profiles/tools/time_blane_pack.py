"""The packed legs of bench.py's `u16_rows` block (which bench.py itself times for the ZINC workloads only) on the config-5 shaped
workloads: 125 k ER / seven-family graphs of 10-256 nodes, max_len 600, ld 608, K epochs per launch of 16-bit rows.

  unpadded            ops.sent(pad=False, u16=True)                                 the plain walk
  packed_scan         ... + gtok_pack_rows_scan behind it                           the two-call route (all there was for this kernel)
  packed_beside_slab  ops.sent(pad=False, u16=True, packed=pk)                      gtok_sent_packed writing the slab as well
  packed              ops.sent(u16=True, packed=pk, slab=False)                     GTOK_SENT_PACK_ONLY

pk is sized as bench.py sizes it (total of the first launch x 1.04 + 4096); launch j walks epochs j K .. j K + K - 1; a leg is N
launches back to back inside one HIP event pair, after two warm-up launches.  Prints one JSON line (ms per epoch).
    python profiles/tools/time_blane_pack.py er|mix K [launches]        GTOK_LIB=<other build> for an A/B
    python profiles/tools/time_blane_pack.py er|mix K --memory          peak device memory of one launch per route instead
"""
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
gtok = importlib.import_module("glearning-benchmark_amd")
dev = torch.device("cuda:0")
G, ld, MAXN, MAX_LEN = 125000, 608, 256, 600


def main():
    wl, K = sys.argv[1], int(sys.argv[2])
    memory = "--memory" in sys.argv
    n = int(sys.argv[3]) if len(sys.argv) > 3 and not memory else max(6, 48 // K)
    d = (gtok.synth.mix_batch_device if wl == "mix" else gtok.synth.er_batch_device)(G, dev, seed=1000)
    b = gtok.GraphBatch.from_coo_device(d["node_counts"], d["edge_counts"], d["src"], d["dst"], device=dev)
    ln = torch.empty(K * G, dtype=torch.int32, device=dev)
    gtok.ops.sent(b, MAXN, MAX_LEN, 0, 0, ld=ld, epochs=K, u16=True, pad=False)        # mirror, lane order
    base = torch.cuda.memory_allocated()
    if memory:
        out = dict(workload=wl, K=K, graphs=G, resident_batch_bytes=base)
        for name in ("slab", "slab_and_packed", "packed_alone"):
            torch.cuda.synchronize(); torch.cuda.empty_cache(); gtok.ops._PACK_SCRATCH.clear()
            torch.cuda.reset_peak_memory_stats()
            if name == "slab":
                ids, l = gtok.ops.sent(b, MAXN, MAX_LEN, 0, 0, ld=ld, epochs=K, u16=True, pad=False)
                need = int(((l.reshape(-1).clamp(0, ld) + 7) // 8 * 8).sum().item())
                del ids, l
            else:
                pk = gtok.ops.PackedRows(K * G, int(need * 1.04) + 4096, True, dev)
                r = gtok.ops.sent(b, MAXN, MAX_LEN, 0, 0, ld=ld, epochs=K, u16=True, pad=False, packed=pk, slab=name == "slab_and_packed")
                out[name + "_fused"] = bool(pk.fused); out[name + "_status"] = int(pk.status().item())
                del pk, r
            torch.cuda.synchronize()
            out[name + "_peak_bytes_above_the_batch"] = torch.cuda.max_memory_allocated() - base
        print(json.dumps(out))
        return
    ids = torch.empty((K * G, ld), dtype=torch.int16, device=dev)
    kw = dict(ld=ld, epochs=K, u16=True)

    def timed(f):
        for j in range(2):
            f(j)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for j in range(n):
            f(j)
        e.record(); torch.cuda.synchronize()
        return round(s.elapsed_time(e) / (n * K), 5)

    walk = lambda j: gtok.ops.sent(b, MAXN, MAX_LEN, 0, j * K, out=(ids, ln), pad=False, **kw)
    walk(0)
    need = int(((ln.clamp(0, ld) + 7) // 8 * 8).sum().item())
    pk = gtok.ops.PackedRows(K * G, int(need * 1.04) + 4096, True, dev)
    out = dict(workload=wl, K=K, graphs=G, launches=n, kernel=gtok.ops.last_sent_kernel(), lib=os.environ.get("GTOK_LIB", "this tree"))
    out["unpadded_ms_per_epoch"] = timed(walk)

    def scan(j):
        walk(j)
        return gtok.ops.pack_rows_u16(ids, ln, None, elem_bytes=2, capacity=K * G * ld, check_status=False)
    out["packed_scan_ms_per_epoch"] = timed(scan)
    beside = lambda j: gtok.ops.sent(b, MAXN, MAX_LEN, 0, j * K, out=(ids, ln), pad=False, packed=pk, **kw)
    out["packed_beside_slab_ms_per_epoch"] = timed(beside)
    out["beside_fused"], out["beside_status"] = bool(pk.fused), int(pk.status().item())
    alone = lambda j: gtok.ops.sent(b, MAXN, MAX_LEN, 0, j * K, out=(None, ln), packed=pk, slab=False, **kw)
    out["packed_ms_per_epoch"] = timed(alone)
    out["alone_fused"], out["alone_status"] = bool(pk.fused), int(pk.status().item())
    out["unpadded_again_ms_per_epoch"] = timed(walk)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
