"""The key of gtok_graph_wl (include/gtok.h; csrc/gtok_graph_wl_hash.hpp, frozen in DESIGN.md section 5c), restated with numpy and
Python integers - the yardstick of tests/test_host_graph_wl.py and tests/test_gpu_graph_wl.py - beside the DEFINITION it digests: an
exact, hash-free colour refinement (exact_classes() below), in which a colour is the rank of a sorted tuple, ranked jointly over a
corpus.

The graph is the simple undirected closure of the listed entries: A(v) = the distinct neighbours u != v, loop_v = (v, v) is listed.
  a_v      = 0 structure only; 1 + nattr[v] with attributes
  t_vu     = 0 structure only; 1 + the attribute byte of the entry (v, u) as row v lists it, with attributes
  c_0[v]   = mix((deg_v | loop_v << 15 | a_v << 16) ^ C0)
  c_r+1[v] = mix((c_r[v] + sum over u in A(v) of mix(c_r[u] ^ C1 ^ (t_vu * D1))) ^ D0)
  S_j      = sum over v of mix(c_R[v] ^ C_j)
  key_j    = mix(S_j + mix((N | R << 32) ^ C_j) + mix(label ^ D_j))          R = rounds, or N when rounds == 0
With attributes the graph must be listed simple and symmetric (what GTOK_CSR_SIMPLE_SYMMETRIC claims): each direction has its byte."""
import numpy as np

from _graph_keys_ref import C, D, U, mix, per_graph, u8

M = (1 << 64) - 1


def closure(n, src, dst, edge_attr=None):
    """-> (rows: the sorted distinct neighbours of every node, loop flags, t: {(v, u): 1 + byte} or None)"""
    src, dst = np.asarray(src, np.int64).reshape(-1).tolist(), np.asarray(dst, np.int64).reshape(-1).tolist()
    nb = [set() for _ in range(n)]
    loop = np.zeros(n, np.int64)
    for u, v in zip(src, dst):
        if u == v:
            loop[u] = 1
        else:
            nb[u].add(v); nb[v].add(u)
    t = None
    if edge_attr is not None:
        t = {}
        for u, v, b in zip(src, dst, u8(edge_attr).tolist()):
            assert u != v and (u, v) not in t, "attributes go with a simple listing"
            t[(u, v)] = 1 + int(b)
        assert all((v, u) in t for u, v in t), "attributes go with a symmetric listing"
    return [sorted(s) for s in nb], loop, t


def rounds_run(n, rounds):
    return int(rounds) if rounds >= 1 else int(n)


def node_colors(n, src, dst, rounds, x=None, edge_attr=None):
    """-> uint64 [n]: c_R"""
    rows, loop, t = closure(n, src, dst, edge_attr if x is not None else None)
    deg = np.array([len(r) for r in rows], np.int64)
    a = np.zeros(n, np.int64) if x is None else 1 + u8(x).astype(np.int64)
    c = mix((deg | loop << 15 | a << 16).astype(U) ^ U(C[0])) if n else np.zeros(0, U)
    ui = np.array([u for r in rows for u in r], np.int64)
    vi = np.repeat(np.arange(n), deg)
    tw = np.zeros(ui.size, U) if t is None else np.array([t[(v, u)] for v, u in zip(vi.tolist(), ui.tolist())], U) * U(D[1])
    for _ in range(rounds_run(n, rounds)):
        term = mix(c[ui] ^ U(C[1]) ^ tw) if ui.size else np.zeros(0, U)
        s = c.copy()
        np.add.at(s, vi, term)
        c = mix(s ^ U(D[0]))
    return c


def wl_key(n, src, dst, rounds, label=0, x=None, edge_attr=None):
    """-> (uint64 [2], uint64 [n])"""
    c = node_colors(n, src, dst, rounds, x, edge_attr)
    head = np.array([int(n) | rounds_run(n, rounds) << 32], U)
    lab = np.array([int(label) & 0xFFFFFFFF], U)
    out = np.zeros(2, U)
    for j in range(2):
        s = mix(c ^ U(C[j])).sum(dtype=U) if n else U(0)
        out[j] = mix(np.array([s], U) + mix(head ^ U(C[j])) + mix(lab ^ U(D[j])))[0]
    return out, c


def batch_wl(node_counts, edge_counts, src, dst, rounds, labels=None, x=None, edge_attr=None):
    """-> (keys uint64 [G, 2], colours uint64 [sum N]) as gtok_graph_wl defines them"""
    ks, cs = [], [np.zeros(0, U)]
    for n, s, d, lab, xx, ea in per_graph(node_counts, edge_counts, src, dst, labels, x, edge_attr):
        k, c = wl_key(n, s, d, rounds, lab, xx, ea)
        ks.append(k); cs.append(c)
    return np.array(ks, U).reshape(-1, 2), np.concatenate(cs)


# ---- the same with Python integers, term by term (the worked examples of DESIGN.md) ------------------------------------------------
def _mix(z):
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9 & M
    z = (z ^ (z >> 27)) * 0x94D049BB133111EB & M
    return z ^ (z >> 31)


def key_by_hand(n, entries, rounds, label=0, nattr=None, eattr=None):
    """entries: [(v, u)] as listed (row v lists u); with attributes eattr[i] is entry i's byte"""
    A = [set() for _ in range(n)]
    loop = [0] * n
    for v, u in entries:
        if v == u:
            loop[v] = 1
        else:
            A[v].add(u); A[u].add(v)
    t = {(v, u): 0 for v in range(n) for u in A[v]}
    if nattr is not None:
        for (v, u), b in zip(entries, eattr):
            t[(v, u)] = 1 + b
    c = [_mix((len(A[v]) | loop[v] << 15 | (0 if nattr is None else 1 + nattr[v]) << 16) ^ C[0]) for v in range(n)]
    R = rounds if rounds >= 1 else n
    for _ in range(R):
        c = [_mix(((c[v] + sum(_mix(c[u] ^ C[1] ^ (t[(v, u)] * D[1] & M)) for u in A[v])) & M) ^ D[0]) for v in range(n)]
    return [_mix((sum(_mix(cv ^ C[j]) for cv in c) + _mix((n | R << 32) ^ C[j]) + _mix((label & 0xFFFFFFFF) ^ D[j])) & M) for j in range(2)], c


# ---- the definition: exact refinement, colours = ranks of sorted tuples, jointly over the corpus ------------------------------------
def exact_classes(graphs, rounds, attrs=False):
    """graphs: [(n, src, dst, label, x, edge_attr)] -> [signature per graph]: two graphs get equal signatures exactly when R rounds of
    colour refinement cannot tell them apart (same N, same label, same multiset of final colours).  No hashing: the colours of a round
    are the ranks of the sorted distinct tuples (own colour, sorted multiset of (t_vu, neighbour's colour)) over ALL graphs.  With
    rounds == 0 every graph is read off at round N (graphs of different N never compare equal, so ranks of one round suffice)."""
    cl = [closure(n, s, d, ea if attrs else None) for n, s, d, _, _, ea in graphs]
    tup = [[(len(rows[v]), int(loop[v]), 0 if not attrs else 1 + int(u8(x)[v])) for v in range(n)]
           for (n, _, _, _, x, _), (rows, loop, _) in zip(graphs, cl)]

    def ranked(tup):
        rank = {t: i for i, t in enumerate(sorted({t for g in tup for t in g}))}
        return [[rank[t] for t in g] for g in tup]

    col = ranked(tup)
    last = max([rounds_run(g[0], rounds) for g in graphs] + [0])
    at = {0: col}
    for r in range(1, last + 1):
        tup = [[(c[v], tuple(sorted(((t[(v, u)] if t else 0), c[u]) for u in rows[v]))) for v in range(len(c))]
               for c, (rows, _, t) in zip(col, cl)]
        col = ranked(tup)
        at[r] = col
    out = []
    for i, g in enumerate(graphs):
        R = rounds_run(g[0], rounds)
        out.append((int(g[0]), R, int(g[3]), tuple(sorted(at[R][i]))))
    return out


def classes(sigs):
    first = {}
    return np.array([first.setdefault(s, i) for i, s in enumerate(sigs)], np.int64)


def renumbered(rng, n, src, dst, x=None, edge_attr=None):
    """the same graph under a random permutation of its ids, the entries shuffled (and, without attributes, re-oriented at random) ->
    (perm, src, dst, x, edge_attr): node v of the input is node perm[v] of the output"""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    perm = rng.permutation(n)
    order = rng.permutation(src.size)
    s2, d2 = perm[src[order]] if src.size else src, perm[dst[order]] if src.size else dst
    if edge_attr is None and src.size:
        flip = rng.integers(0, 2, src.size).astype(bool)
        s2, d2 = np.where(flip, d2, s2), np.where(flip, s2, d2)
    x2 = None
    if x is not None:
        x2 = np.empty(n, np.int64)
        x2[perm] = np.asarray(x, np.int64)
    return perm, s2, d2, x2, None if edge_attr is None else np.asarray(edge_attr, np.int64)[order]
