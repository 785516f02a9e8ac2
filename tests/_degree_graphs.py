"""Deterministic graphs at the degree limits of the SENT kernels, and the adjacency bit-matrix mirror of include/gtok.h restated
with Python integers and sets.

Every builder returns ONE graph in the dict shape `_util.both` takes (node_counts / edge_counts of length 1, src, dst, x, edge_attr)
plus two keys of its own: `degree`, the graph's true largest closure degree (a self loop counts once), stated by the builder from the
family's formula - the tests assert it against the lists, so a fixture cannot drift off its boundary - and `both`, the listing:
False = every edge once, as (a, b) with a < b in ascending order; True = both directions, row-sorted (simple-symmetric: what the
lane-per-graph kernel accepts).  `batch_of` concatenates graphs into a batch dict whose `degree` is the largest of its graphs'.
Types: x[v] = (5 v + 3) % 28; an edge's forward entry (a < b) carries (a + b) % 3, its backward entry 3 + (a + b) % 2 - the two
directions differ on purpose -, a self loop 5: num_node_types = 28, num_edge_types = 6."""
import numpy as np

NODE_TYPES, EDGE_TYPES = 28, 6
KEYS = ("node_counts", "edge_counts", "src", "dst", "x", "edge_attr")


def _graph(n, pairs, both, degree):
    """pairs: the undirected edges as (a, b), a < b"""
    p = np.array(sorted(set(pairs)), np.int64).reshape(-1, 2)
    assert p.shape[0] == len(pairs) and (p[:, 0] < p[:, 1]).all() and (p.size == 0 or (p.min() >= 0 and p.max() < n))
    a, b = p[:, 0], p[:, 1]
    if both:
        s, t, ty = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([(a + b) % 3, 3 + (a + b) % 2])
        o = np.lexsort((t, s))
        s, t, ty = s[o], t[o], ty[o]
    else:
        s, t, ty = a, b, (a + b) % 3
    return dict(node_counts=np.array([n], np.int64), edge_counts=np.array([s.size], np.int64), src=s, dst=t,
                x=(5 * np.arange(n, dtype=np.int64) + 3) % NODE_TYPES, edge_attr=ty.astype(np.int64), degree=int(degree), both=bool(both))


def _pair(a, b):
    return (a, b) if a < b else (b, a)


def star(n, hub=0, both=False):
    """n nodes, every other node a leaf of `hub`: the hub has degree n - 1"""
    return _graph(n, [_pair(hub, v) for v in range(n) if v != hub], both, n - 1 if n > 1 else 0)


def wheel(n, both=False):
    """hub 0 joined to every node of a ring on 1 .. n - 1 (n >= 5): the hub has degree n - 1, a rim node 3"""
    rim = [_pair(1 + i, 1 + (i + 1) % (n - 1)) for i in range(n - 1)]
    return _graph(n, [(0, v) for v in range(1, n)] + rim, both, n - 1)


def bipartite(a, b, both=False):
    """complete K(a, b): nodes 0 .. a - 1 on one side (degree b), a .. a + b - 1 on the other (degree a)"""
    return _graph(a + b, [(u, a + v) for u in range(a) for v in range(b)], both, max(a, b))


def complete(n, both=False):
    return _graph(n, [(u, v) for u in range(n) for v in range(u + 1, n)], both, n - 1 if n > 1 else 0)


def path(n, both=False):
    return _graph(n, [(v, v + 1) for v in range(n - 1)], both, min(2, max(n - 1, 0)))


def ring(n, both=False):
    """n >= 3"""
    return _graph(n, [_pair(v, (v + 1) % n) for v in range(n)], both, 2)


def sparse(n, both=False):
    """a ring on n nodes (n >= 16) with a chord from every eighth node to the one opposite: degrees 2 and 3 - the large graph that
    sets a batch's row width without touching its largest degree"""
    chords = {_pair(v, (v + n // 2) % n) for v in range(0, n, 8)}
    ringp = {_pair(v, (v + 1) % n) for v in range(n)}
    return _graph(n, sorted(ringp | chords), both, 3)


def empty(n=0):
    """n isolated nodes"""
    return _graph(n, [], False, 0)


def with_self_loop(graph, v):
    """`graph` (one graph) with the entry (v, v) added - type 5; a both-directions listing stays row-sorted (it is no longer simple).
    The loop counts 1 towards v's degree."""
    n = int(graph["node_counts"][0])
    assert graph["node_counts"].size == 1 and 0 <= v < n
    nb = set(graph["dst"][graph["src"] == v].tolist()) | set(graph["src"][graph["dst"] == v].tolist())
    s, t, ty = np.append(graph["src"], v), np.append(graph["dst"], v), np.append(graph["edge_attr"], 5)
    if graph["both"]:
        o = np.lexsort((t, s))
        s, t, ty = s[o], t[o], ty[o]
    deg_v = len(nb | {v})
    return dict(node_counts=graph["node_counts"].copy(), edge_counts=np.array([s.size], np.int64), src=s, dst=t, x=graph["x"].copy(),
                edge_attr=ty, degree=max(graph["degree"], deg_v), both=graph["both"])


def batch_of(*graphs):
    """the graphs (or batches) side by side, in the order given"""
    d = {k: np.concatenate([np.asarray(g[k], np.int64) for g in graphs]) for k in KEYS}
    d["degree"] = max([g["degree"] for g in graphs], default=0)
    d["both"] = all(g["both"] or int(np.sum(g["edge_counts"])) == 0 for g in graphs)
    return d


# ------------------------------------------------------------------------------------------------ the mirror, restated
def adjbits_reference(node_counts, edge_counts, src, dst, words):
    """include/gtok.h, gtok_csr.adj_rows / gtok_csr_adjbits, with Python integers and sets: -> (rows uint64 [sum N, W], planes uint64
    [G, 8, W], max_degree).  The symmetric closure of the listed entries; an entry with an endpoint outside [0, N_g) is skipped;
    duplicates collapse; a self loop sets the node's own bit and counts 1; planes[g, p, w] bit l = bit p of the degree of node
    64 w + l (so a degree of 256 reads 0 there), nodes at or beyond N_g contribute 0."""
    node_counts, edge_counts = np.asarray(node_counts, np.int64), np.asarray(edge_counts, np.int64)
    G, W = node_counts.size, int(words)
    nptr = np.concatenate([[0], np.cumsum(node_counts)])
    eptr = np.concatenate([[0], np.cumsum(edge_counts)])
    rows = np.zeros((int(nptr[-1]), W), np.uint64)
    planes = np.zeros((G, 8, W), np.uint64)
    mask, maxdeg = (1 << 64) - 1, 0
    src, dst = np.asarray(src).tolist(), np.asarray(dst).tolist()
    for g in range(G):
        n = int(node_counts[g])
        assert n <= 64 * W
        nb = [set() for _ in range(n)]
        for i in range(int(eptr[g]), int(eptr[g + 1])):
            a, b = src[i], dst[i]
            if 0 <= a < n and 0 <= b < n:
                nb[a].add(b); nb[b].add(a)
        pl = [[0] * W for _ in range(8)]
        for u in range(n):
            bits = sum(1 << v for v in nb[u])
            deg = len(nb[u])
            maxdeg = max(maxdeg, deg)
            for w in range(W):
                rows[nptr[g] + u, w] = np.uint64((bits >> (64 * w)) & mask)
            for p in range(8):
                if (deg >> p) & 1:
                    pl[p][u >> 6] |= 1 << (u & 63)
        for p in range(8):
            for w in range(W):
                planes[g, p, w] = np.uint64(pl[p][w])
    return rows, planes, maxdeg


def csr_arrays(node_counts, edge_counts, src, dst):
    """gtok_csr's index arrays of a batch in COO form, entries kept in list order inside every row (a stable sort by row alone, so
    a row's columns stay as unsorted as the list has them) and columns passed through unchecked: (node_ptr int32 [G + 1], edge_ptr
    int64 [G + 1], rowptr int32 [sum N + G], col int32 [sum E]).  src must lie inside its graph; dst need not."""
    node_counts, edge_counts = np.asarray(node_counts, np.int64), np.asarray(edge_counts, np.int64)
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    G = node_counts.size
    nptr = np.concatenate([[0], np.cumsum(node_counts)]).astype(np.int64)
    eptr = np.concatenate([[0], np.cumsum(edge_counts)]).astype(np.int64)
    rowptr, col = np.zeros(int(nptr[-1]) + G, np.int32), np.zeros(int(eptr[-1]), np.int32)
    for g in range(G):
        n, s, t = int(node_counts[g]), src[eptr[g]:eptr[g + 1]], dst[eptr[g]:eptr[g + 1]]
        assert s.size == 0 or (s.min() >= 0 and s.max() < n)
        o = np.argsort(s, kind="stable")
        col[eptr[g]:eptr[g + 1]] = t[o]
        rowptr[nptr[g] + g:nptr[g + 1] + g + 1] = np.concatenate([[0], np.cumsum(np.bincount(s, minlength=n))])
    return nptr.astype(np.int32), eptr, rowptr, col


# ------------------------------------------------------------------------------------------------ the instances the tests walk
def plane_batch(leaves, both, big=0):
    """The plane-switch batch: a star of `leaves` + 1 nodes (hub 3: degree = leaves) beside paths and small rings (degree <= 2) and,
    with big = 128 or 256, one large sparse graph (degree 3) that widens the rows to 2 or 4 words.  The star sits in the middle."""
    gs = [path(1, both), path(2, both), path(9, both), ring(3, both), ring(12, both), star(leaves + 1, 3, both), path(30, both), ring(17, both),
          empty(0), path(5, both)]
    if big:
        gs.insert(2, sparse(big, both))
    return batch_of(*gs)


# name -> (builder(both) -> one graph, uncut unlabelled length at seed 7, epoch 1, graph_base 0 as a batch of its own).  A star's walk
# is 3 n - 4 tokens from a leaf and 3 n - 2 from the hub (every leaf but the first two costs RESET, hub, leaf); at this seed the walks
# start at nodes other than the hubs chosen here (the 17-node star's starts at node 3), so the lengths are the 3 n - 4 ones.
LIMIT_GRAPHS = {
    "star16": (lambda both: star(16, 0, both), 44),
    "star17": (lambda both: star(17, 0, both), 47),
    "star64_hub0": (lambda both: star(64, 0, both), 188),
    "star64_hub63": (lambda both: star(64, 63, both), 188),
    "K64": (lambda both: complete(64, both), 2143),
    "star256_hub0": (lambda both: star(256, 0, both), 764),
    "star256_hub64": (lambda both: star(256, 64, both), 764),
    "star256_hub255": (lambda both: star(256, 255, both), 764),
    "wheel256": (lambda both: wheel(256, both), 1021),
    "K8_248": (lambda both: bipartite(8, 248, both), 2971),
    "K256": (lambda both: complete(256, both), 33151),
    "K256_loop": (lambda both: with_self_loop(complete(256, both), 255), 33152),
}
LENGTH_SEED, LENGTH_EPOCH = 7, 1
