"""Cycles of the append at a unit's end in sent_blane_kernel's PACK instantiations (gtok_sent_packed beside an int32 slab), next to
the unit's whole life.  Needs a -DGTOK_PHASE_TIMING build loaded through GTOK_LIB (phase_timing_blane.py says how to build one;
never ship it): the last 8 columns of the row of every unit's lane 0 then hold the phase sums, with columns 5 / 6 = cycles until
the fill-mark atomic answered (the unit's row stores draining + the first batch of loads + the atomic) / cycles of the rest of the
copy, and column 7 the unit's life on the 100 MHz clock.
    GTOK_LIB=glearning-benchmark_amd/csrc/libgtok_prof.so python profiles/tools/phase_timing_blane_pack.py [graphs] [epochs per launch]"""
import importlib, os, sys
import numpy as np, torch
sys.path.insert(0, os.getcwd())
gtok = importlib.import_module("glearning-benchmark_amd")
dev = torch.device("cuda", 0)
G = int(sys.argv[1]) if len(sys.argv) > 1 else 125000
K = int(sys.argv[2]) if len(sys.argv) > 2 else 4
for name, d in (("er", gtok.synth.er_batch_device(G, dev, seed=1000)), ("mix", gtok.synth.mix_batch_device(G, dev, seed=1000))):
    b = gtok.GraphBatch.from_coo_device(d["node_counts"], d["edge_counts"], d["src"], d["dst"], device=dev)
    pk = gtok.ops.PackedRows(K * G, K * G * 608, False, dev)
    for k in range(3):
        ids, ln = gtok.ops.sent(b, b.max_nodes, 600, 0, k * K, ld=608, epochs=K, packed=pk, pad=False)
    torch.cuda.synchronize()
    assert pk.fused and int(pk.status()) == 0
    first = b.lane_order[::64].long()
    ph = ids.view(K, G, 608)[:, first][:, :, -8:].reshape(-1, 8).cpu().numpy().astype(np.int64)
    walk, tail, ask, copy = ph[:, :4].sum(1), ph[:, 4], ph[:, 5], ph[:, 6]
    life = (ph[:, 7] & 0xFFFFFFFF) / 100.0
    print(f"== {name}: {ph.shape[0]} (unit, epoch) pairs, {K} epochs per launch, int32 rows beside the slab ({gtok.ops.last_sent_kernel()})")
    for nme, v in (("walk (phases 0-3)", walk), ("row end + append", tail), ("  until the atomic answered", ask), ("  rest of the copy", copy)):
        print(f"{nme:28s} mean {v.mean():10.0f} cycles  p50 {np.percentile(v, 50):10.0f}  max {v.max():10.0f}  share of the phases {v.sum() / (walk + tail).sum():.3f}")
    print("unit life us (min p10 p50 p90 max):", " ".join(f"{np.percentile(life, p):7.1f}" for p in (0, 10, 50, 90, 100)))
