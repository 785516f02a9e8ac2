"""The SENT walk of DESIGN.md §5 restated in plain Python: walk(...) -> (tokens, visit_index).

The C oracle (oracle.sent) returns tokens only; the visit order - which node got which position id - is the yardstick of
gtok_sent_large_order, so it is produced here, by a walk that tests/test_host_order.py pins to the oracle token for token.
Every per-node set is a sorted list (bisect): a 16,384-node star or path walks in well under a second.  Philox comes from the
oracle library (oracle.philox4x32_10, checked against the Random123 vectors by the oracle's own tests)."""
from bisect import bisect_left, insort

import numpy as np

SOS, RESET, LADJ, RADJ, EOS, IDX = 0, 1, 2, 3, 4, 6


def walk(orc, n, src, dst, max_len, seed, epoch, gid, labeled=False, x=None, edge_attr=None, max_num_nodes=0, num_node_types=0):
    """One graph (n nodes, entries src[i] -> dst[i] in list order) -> (the first max_len tokens, int32 [n]: visit index per node, -1 =
    not visited when the walk stopped).  gid = graph_base + the graph's index."""
    node_off = IDX + max_num_nodes
    edge_off = node_off + num_node_types
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32)
    state = dict(d=0, buf=None)

    def below(m):
        d = state["d"]
        if d & 3 == 0:
            state["buf"] = orc.philox4x32_10([d >> 2, epoch & 0xFFFFFFFF, gid & 0xFFFFFFFF, (gid >> 32) & 0xFFFFFFFF], key)
        state["d"] = d + 1
        return (int(state["buf"][d & 3]) * m) >> 32

    adj, etype = [set() for _ in range(n)], {}
    for i, (a, b) in enumerate(zip(map(int, src), map(int, dst))):
        if 0 <= a < n and 0 <= b < n:
            adj[a].add(b); adj[b].add(a)
            if labeled:
                etype.setdefault((a, b), int(edge_attr[i]))
    adj = [sorted(s) for s in adj]                        # uncovered edges of a node: the other ends, ascending node id
    type_of = lambda a, b: etype.get((a, b), etype.get((b, a), 0))
    vidx = np.full(n, -1, np.int32)
    order, live, unvis, out = [], [], list(range(n)), [SOS]

    def drop(a, b):                                       # the edge (a, b) is covered, seen from a
        del adj[a][bisect_left(adj[a], b)]
        if not adj[a] and vidx[a] >= 0:
            i = bisect_left(live, a)
            if i < len(live) and live[i] == a:
                del live[i]

    def visit(v):
        vidx[v] = len(order); order.append(v)
        del unvis[bisect_left(unvis, v)]
        out.append(IDX + int(vidx[v]))
        if labeled:
            out.append(node_off + int(x[v]))
        members = sorted((int(vidx[a]), a) for a in adj[v] if vidx[a] >= 0)
        if members:
            out.append(LADJ)
            for k, a in members:
                if labeled:
                    out.append(edge_off + type_of(v, a))
                out.append(IDX + k)
                drop(v, a)
                if a != v:
                    drop(a, v)
            out.append(RADJ)
        if adj[v]:
            insort(live, v)

    if n > 0:
        cur = below(n)
        visit(cur)
        while len(out) < max_len:
            if adj[cur]:
                nxt = adj[cur][below(len(adj[cur]))]
                drop(cur, nxt); drop(nxt, cur)
                if labeled:
                    out.append(edge_off + type_of(cur, nxt))
                visit(nxt)
                cur = nxt
            elif live:
                cur = live[below(len(live))]
                out += [RESET, IDX + int(vidx[cur])]
            elif unvis:
                cur = unvis[below(len(unvis))]
                out.append(RESET)
                visit(cur)
            else:
                break
    out.append(EOS)
    return np.array(out[:max_len], np.int32), vidx


def walk_batch(orc, node_counts, edge_counts, src, dst, max_len, seed, epoch=0, graph_base=0, labeled=False, x=None, edge_attr=None,
               max_num_nodes=0, num_node_types=0):
    """A batch in COO form -> (list of token arrays, visit_index int32 [sum N]) for one epoch."""
    nptr = np.concatenate([[0], np.cumsum(node_counts)]).astype(np.int64)
    eptr = np.concatenate([[0], np.cumsum(edge_counts)]).astype(np.int64)
    toks, vis = [], np.empty(int(nptr[-1]), np.int32)
    for g in range(len(node_counts)):
        n0, n1, e0, e1 = nptr[g], nptr[g + 1], eptr[g], eptr[g + 1]
        t, v = walk(orc, int(n1 - n0), src[e0:e1], dst[e0:e1], max_len, seed, epoch, graph_base + g, labeled,
                    None if x is None else x[n0:n1], None if edge_attr is None else edge_attr[e0:e1], max_num_nodes, num_node_types)
        toks.append(t); vis[n0:n1] = v
    return toks, vis
