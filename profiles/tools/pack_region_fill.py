"""How evenly do the regions of gtok_sent_packed's buffer fill when sent_blane_kernel packs config-5 rows?  CPU only.

The launcher cuts the buffer into R regions (R = 64, halved while the launch has fewer than 64 R (unit, epoch) pairs); pair
vu = unit * K + epoch (unit-major) appends to region vu mod R; units are 64 consecutive graphs of the lane order (graphs by
expected walk length, ops._lane_order, restated here with numpy).  A row takes min(len, ld) ids rounded up to 8 (16-bit ids,
16-byte pieces).  The lengths are the CPU oracle's.  Prints fullest region / mean region for K = 1, 2, 8: bench.py sizes its
buffer as total x 1.04 + 4096, so a ratio below 1.04 means no region overflows under that rule.

    python profiles/tools/pack_region_fill.py [graphs] > profiles/blane_pack/region_fill.txt
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
synth = importlib.import_module("glearning-benchmark_amd.synth")
import oracle as orc  # noqa: E402

MAX_LEN, LD = 600, 608


def lane_order(d, typical_len):
    """ops._lane_order on the host: one direction per edge in d, so e is the edge count and closure degrees are plain counts"""
    n = d["node_counts"].astype(np.float64)
    e = d["edge_counts"].astype(np.float64)
    G = n.size
    nptr = np.concatenate([[0], np.cumsum(d["node_counts"])])
    eg = np.repeat(np.arange(G), d["edge_counts"])
    deg = np.bincount(nptr[eg] + d["src"], minlength=nptr[-1]) + np.bincount(nptr[eg] + d["dst"], minlength=nptr[-1])
    leaves = np.add.reduceat((deg == 1).astype(np.int64), nptr[:-1]).astype(np.float64)
    r = np.maximum(leaves - 1, 0)
    members = np.maximum(e - n + 1, 0)
    steps_full = np.maximum(n + r, 1)
    a = (n + 2 * r + 2 * np.minimum(n, members)) / steps_full
    q = members / (steps_full * steps_full)
    L = float(typical_len)
    cut = np.where(q > 1e-9, (np.sqrt(a * a + 4 * q * L) - a) / np.maximum(2 * q, 1e-9), L / np.maximum(a, 1e-9))
    steps = np.clip(np.rint(np.minimum(cut, steps_full)), 0, 1023).astype(np.int64)
    p = np.clip(2 * e / np.maximum(n * n, 1), 0.0, 1.0)
    key = steps * 1024 + np.rint(p * 1023).astype(np.int64)
    return np.argsort(-key, kind="stable")


def main():
    G = int(sys.argv[1]) if len(sys.argv) > 1 else 24000
    print(f"{G} graphs, max_len {MAX_LEN}, ld {LD}, 16-bit ids (rows rounded up to 8 ids); corpora drawn with torch's CPU generator")
    for name, d in (("ER, seed 3", synth.er_batch_device(G, "cpu", seed=3)), ("seven-family mix, seed 4", synth.mix_batch_device(G, "cpu", seed=4))):
        coo = orc.Coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], None, None)
        order = lane_order(d, MAX_LEN)
        units = (G + 63) // 64
        size, top = [], 0
        for ep in range(8):
            ids, ln = orc.sent(coo, 256, MAX_LEN, 0, ep, ld=LD, nthreads=os.cpu_count() or 1)
            size.append((np.minimum(ln, LD) + 7) // 8 * 8)
            top = max(top, int(ids.max()))
        print(f"{name}: largest id {top}")
        for K in (1, 2, 8):
            vunits, R = units * K, 64
            while R > 1 and vunits < 64 * R:
                R >>= 1
            fill = np.zeros(R, np.int64)
            for ep in range(K):
                per_unit = np.add.reduceat(size[ep][order], np.arange(0, G, 64))
                np.add.at(fill, (np.arange(units) * K + ep) % R, per_unit)
            print(f"  K = {K}: {vunits} pairs, {R} regions, total {int(fill.sum())} ids, fullest region / mean = {fill.max() / fill.mean():.4f}")


if __name__ == "__main__":
    main()
