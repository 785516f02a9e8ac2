"""Median and range of the bench.py figures blane_pack_ab.sh collected: python profiles/tools/blane_pack_ab_table.py OUT_DIR"""
import glob
import json
import os
import statistics
import sys

# bench.py's own figures, then the legs of time_blane_pack.py (bench.py times its u16_rows block for the ZINC workloads only)
KEYS = [("", "bench.py ms_per_step", lambda r: r["ms_per_step"]),
        ("", "bench.py epoch_loop.ms_per_epoch", lambda r: r["epoch_loop"]["ms_per_epoch"]),
        ("legs_", "unpadded", lambda r: r["unpadded_ms_per_epoch"]),
        ("legs_", "unpadded, again at the end", lambda r: r["unpadded_again_ms_per_epoch"]),
        ("legs_", "packed_scan (two calls)", lambda r: r["packed_scan_ms_per_epoch"]),
        ("legs_", "packed_beside_slab", lambda r: r["packed_beside_slab_ms_per_epoch"]),
        ("legs_", "packed (no slab)", lambda r: r["packed_ms_per_epoch"])]


def main():
    d = sys.argv[1]
    print("| workload | K | figure (ms per epoch) | parent: median [min .. max] | this commit: median [min .. max] |")
    print("|---|---|---|---|---|")
    for wl in ("synth_er", "synth_mix"):
        for K in (1, 14):
            load = lambda pre, lib: [json.load(open(f)) for f in sorted(glob.glob(os.path.join(d, f"{pre}{wl}_K{K}_{lib}_*.json")))]
            for pre, name, get in KEYS:
                cells = []
                for lib in ("parent", "branch"):
                    v = []
                    for r in load(pre, lib):
                        try:
                            v.append(float(get(r)))
                        except (KeyError, TypeError):
                            pass
                    cells.append(f"{statistics.median(v):.4f} [{min(v):.4f} .. {max(v):.4f}] (n = {len(v)})" if v else "-")
                print(f"| {wl} | {K} | {name} | {cells[0]} | {cells[1]} |")
            flags = [" / ".join(sorted({f"beside: fused {r['beside_fused']}, status {r['beside_status']}; alone: fused {r['alone_fused']}, status {r['alone_status']}"
                                        for r in load("legs_", lib)})) for lib in ("parent", "branch")]
            print(f"| {wl} | {K} | packed legs | {flags[0]} | {flags[1]} |")


if __name__ == "__main__":
    main()
