"""The definitions of gtok_graph_tasks (include/gtok.h), restated with numpy - the yardstick of tests/test_host_graph_tasks.py
(which pins it to synth._has_cycle / synth._bfs_dist and to networkx) and tests/test_gpu_graph_tasks.py.

The graph of a listed edge set is its SIMPLE UNDIRECTED CLOSURE: nodes 0..n-1, {u, v} an edge iff (u, v) or (v, u) is listed and
u != v; duplicates collapse; self loops are counted apart.  Two forms of the same thing: a dense closure matrix (the definition
as written, for graphs of up to DENSE_MAX nodes) and a symmetric CSR (for the 16,384-node graphs, whose matrix would take 268 MB);
the host tests hold them against each other."""
import numpy as np

DENSE_MAX = 1024
BAD_QUERY = -2


class Closure:
    def __init__(self, n, src, dst, dense=None):
        src, dst = np.asarray(src, np.int64).reshape(-1), np.asarray(dst, np.int64).reshape(-1)
        assert src.size == dst.size and (src.size == 0 or (min(src.min(), dst.min()) >= 0 and max(src.max(), dst.max()) < n))
        self.n = int(n)
        self.loops = int((src == dst).sum())
        keep = src != dst
        lo, hi = np.minimum(src[keep], dst[keep]), np.maximum(src[keep], dst[keep])
        key = np.unique(lo * max(self.n, 1) + hi)
        lo, hi = key // max(self.n, 1), key % max(self.n, 1)
        self.m = int(key.size)                          # distinct undirected non-loop edges
        self.dense = self.n <= DENSE_MAX if dense is None else dense
        if self.dense:
            self.A = np.zeros((self.n, self.n), bool)
            self.A[lo, hi] = True
            self.A[hi, lo] = True
        else:
            rows, cols = np.concatenate([lo, hi]), np.concatenate([hi, lo])
            order = np.argsort(rows, kind="stable")
            self.cols = cols[order]
            self.indptr = np.zeros(self.n + 1, np.int64)
            np.cumsum(np.bincount(rows, minlength=self.n), out=self.indptr[1:])

    def _next(self, frontier, visited):
        """the nodes outside `visited` with a neighbour in `frontier` (index array) - one level"""
        if self.dense:
            return np.nonzero(self.A[frontier].any(0) & ~visited)[0]
        starts, counts = self.indptr[frontier], self.indptr[frontier + 1] - self.indptr[frontier]
        total = int(counts.sum())
        idx = np.repeat(starts - (np.cumsum(counts) - counts), counts) + np.arange(total)
        nb = np.unique(self.cols[idx])
        return nb[~visited[nb]]

    def levels(self, s, visited=None):
        """hop counts from s (-1: unreachable); `visited` (bool [n]) is updated in place when given"""
        dist = np.full(self.n, -1, np.int64)
        visited = np.zeros(self.n, bool) if visited is None else visited
        frontier = np.array([s], np.int64)
        dist[s] = 0; visited[s] = True
        d = 0
        while frontier.size:
            d += 1
            frontier = self._next(frontier, visited)
            dist[frontier] = d; visited[frontier] = True
        return dist

    def num_components(self):
        visited = np.zeros(self.n, bool)
        comp = 0
        while not visited.all():
            self.levels(int(np.argmin(visited)), visited)       # the lowest unvisited node
            comp += 1
        return comp

    def has_cycle(self, comp=None):
        comp = self.num_components() if comp is None else comp
        return int(self.loops > 0 or self.m > self.n - comp)

    def dist(self, u, v, cache=None):
        if not (0 <= u < self.n and 0 <= v < self.n):
            return BAD_QUERY
        if u == v:
            return 0
        cache = {} if cache is None else cache
        if u not in cache:
            cache[u] = self.levels(u)
        return int(cache[u][v])


def batch_answers(node_counts, edge_counts, src, dst, queries=None, query_ptr=None):
    """-> dict(has_cycle [G], num_components [G], dist [Q] or None, info [4]) of a batched COO, as gtok_graph_tasks defines them
    (info: status bit 0 for a query endpoint outside its graph, the largest dist, the queries answered -1, the graphs with a cycle)."""
    node_counts, edge_counts = np.asarray(node_counts, np.int64), np.asarray(edge_counts, np.int64)
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    G = node_counts.size
    eptr = np.concatenate([[0], np.cumsum(edge_counts)])
    if queries is not None:
        queries = np.asarray(queries, np.int64).reshape(-1, 2)
        qptr = np.arange(G + 1) if query_ptr is None else np.asarray(query_ptr, np.int64)
        dist = np.zeros(queries.shape[0], np.int32)
    cyc, comp = np.zeros(G, np.int32), np.zeros(G, np.int32)
    for g in range(G):
        c = Closure(node_counts[g], src[eptr[g]:eptr[g + 1]], dst[eptr[g]:eptr[g + 1]])
        comp[g] = c.num_components()
        cyc[g] = c.has_cycle(comp[g])
        if queries is not None:
            cache = {}
            for q in range(qptr[g], qptr[g + 1]):
                dist[q] = c.dist(int(queries[q, 0]), int(queries[q, 1]), cache)
    info = np.array([0, 0, 0, int(cyc.sum())], np.int32)
    if queries is not None:
        info[0] = int((dist == BAD_QUERY).any())
        info[1] = max(0, int(dist.max())) if dist.size else 0
        info[2] = int((dist == -1).sum())
    return dict(has_cycle=cyc, num_components=comp, dist=dist if queries is not None else None, info=info)
