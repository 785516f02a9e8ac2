"""Lock-step statistics of sent_lane_kernel on a ZINC-like corpus, from the CPU oracle's rows alone (host only, no GPU).

A lane of sent_lane_kernel walks one graph; the 64 lanes of a wave advance together, one walk step per loop iteration, so a
unit of 64 graphs costs (its longest walk) x 64 lane-steps, and the bracket list of a step costs the whole wave whenever one
lane has a bracket.  Everything here is read off unremapped rows (remap_zinc = 0):
  walk step      = a position token outside LADJ ... RADJ (a node visit, a RESET or a new component: one loop iteration)
  bracket member = a position token inside LADJ ... RADJ, charged to the step before it
  unit           = 64 consecutive graphs in the order of the lane sort key min(255, nodes + leaves), stable, descending
                   (gtok_csr_lane_sort; its cut by LDS fit is ignored: molecules always fit 64 to a unit)
The choice-set sizes of the pick (row / live / unvisited) are not in the rows and are not reported.

  python3 profiles/tools/lockstep_stats.py [--graphs 249456] [--seed 1000]     (bench.py's ZINC-full corpus: seed 1000)
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
gtok = importlib.import_module("glearning-benchmark_amd")
import oracle as orc  # noqa: E402

LADJ, RADJ, IDX = 2, 3, 6          # include/gtok.h: GTOK_SENT_LADJ, GTOK_SENT_RADJ, GTOK_SENT_IDX_OFFSET
NN, MAX_LEN, SMAX, CHUNK = 37, 512, 128, 16384


def walk_tables(d, nthreads):
    """Per graph: walk steps, and bracket members at each step ([G, SMAX] uint8)."""
    nptr = np.concatenate([[0], np.cumsum(d["node_counts"])])
    eptr = np.concatenate([[0], np.cumsum(d["edge_counts"])])
    G = len(d["node_counts"])
    steps = np.zeros(G, np.int64)
    members = np.zeros((G, SMAX), np.uint8)
    for g0 in range(0, G, CHUNK):
        g1 = min(G, g0 + CHUNK)
        n0, n1, e0, e1 = nptr[g0], nptr[g1], eptr[g0], eptr[g1]
        coo = orc.Coo(d["node_counts"][g0:g1], d["edge_counts"][g0:g1], d["src"][e0:e1], d["dst"][e0:e1],
                      d["x"][n0:n1], d["edge_attr"][e0:e1])
        ids, ln = orc.sent(coo, NN, MAX_LEN, 0, 0, labeled=True, num_node_types=9, num_edge_types=4, graph_base=g0,
                           ld=MAX_LEN, nthreads=nthreads)
        assert int(ln.max()) < MAX_LEN, "a row was cut: raise MAX_LEN"
        valid = np.arange(MAX_LEN)[None, :] < ln[:, None]
        depth = np.cumsum((ids == LADJ) & valid, 1) - np.cumsum((ids == RADJ) & valid, 1)
        pos = valid & (ids >= IDX) & (ids < IDX + NN)
        step = pos & (depth == 0)
        mem = pos & (depth > 0)
        sidx = np.cumsum(step, 1) - 1
        steps[g0:g1] = step.sum(1)
        assert int(steps[g0:g1].max()) < SMAX
        rows = np.broadcast_to(np.arange(g1 - g0)[:, None], ids.shape)
        flat = np.bincount(rows[mem] * SMAX + sidx[mem], minlength=(g1 - g0) * SMAX)
        members[g0:g1] = flat.reshape(g1 - g0, SMAX)
    return steps, members


def leaves_of(d):
    src = d["src"]
    nptr = np.concatenate([[0], np.cumsum(d["node_counts"])])
    gof = np.repeat(np.arange(len(d["node_counts"])), d["edge_counts"])
    deg = np.bincount(nptr[gof] + src, minlength=int(nptr[-1]))            # entries per node (rows list both directions)
    return np.add.reduceat((deg == 1).astype(np.int64), nptr[:-1]) * (d["node_counts"] > 0)


def units(perm):
    U = (perm.size + 63) // 64
    p = np.full(U * 64, -1, np.int64)
    p[:perm.size] = perm
    return p.reshape(U, 64)


def order_stats(steps, perm):
    u = units(perm)
    s = np.where(u >= 0, steps[np.maximum(u, 0)], 0)
    umax = s.max(1)
    return steps.sum() / (64.0 * umax.sum()), int(umax.max()), umax


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=249456)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--threads", type=int, default=min(16, orc.num_threads()))
    a = ap.parse_args()
    d = gtok.synth.zinc_like(a.graphs, seed=a.seed)
    G = a.graphs
    nodes = d["node_counts"].astype(np.int64)
    steps, members = walk_tables(d, a.threads)
    key = np.minimum(255, nodes + leaves_of(d))
    by_key = np.argsort(-key, kind="stable")
    by_steps = np.argsort(-steps, kind="stable")
    print(f"corpus: synth.zinc_like({G}, seed={a.seed}); oracle rows, labelled, unremapped, seed 0, epoch 0")
    print(f"walk steps per graph            {steps.mean():.2f} mean (nodes {nodes.mean():.2f}), max {steps.max()}")
    for name, perm in (("current key (nodes + leaves)", by_key), ("dataset order", np.arange(G)),
                       ("perfect sort by steps", by_steps)):
        e, longest, _ = order_stats(steps, perm)
        print(f"lock-step efficiency, {name:29s} {e:.3f}   (longest unit {longest} steps)")
    # brackets, in the units of the current key
    u = units(by_key)
    m = np.where((u >= 0)[:, :, None], members[np.maximum(u, 0)], 0)    # [U, 64, SMAX]
    _, _, umax = order_stats(steps, by_key)
    wave_steps = int(umax.sum())
    has = m > 0
    any_lane = has.any(1)                                                  # [U, SMAX]
    lanes = has.sum(1)
    big = m.max(1)
    nb = int(any_lane.sum())
    sizes = members[members > 0]
    print(f"wave-steps (sum of unit maxima) {wave_steps}")
    print(f"wave-steps with a bracket       {nb / wave_steps:.3f}   (the wave runs the bracket list)")
    live = np.arange(SMAX)[None, :] < umax[:, None]
    print(f"lanes listing a bracket         {lanes[live].mean() / 64:.3f} of 64 per wave-step; "
          f"{lanes[any_lane].mean() / 64:.3f} of 64 ({lanes[any_lane].mean():.2f} lanes) in the wave-steps with one")
    print(f"bracket members at one step     max {int(sizes.max())}, mean {sizes.mean():.3f};  "
          f"sizes {np.bincount(sizes).tolist()[1:]} (1, 2, 3, ...)")
    print(f"bracket wave-steps whose largest bracket has <= 1 / <= 3 members   "
          f"{(big[any_lane] <= 1).mean():.3f} / {(big[any_lane] <= 3).mean():.3f}")


if __name__ == "__main__":
    main()
