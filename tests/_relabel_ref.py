"""gtok_csr_relabel (include/gtok.h) restated with numpy, graph by graph: relabel(...) -> dict of every output array, status and info.

Inputs are host arrays in gtok_csr's layout.  A skipped graph (status 1) leaves its slices at the fill value the caller chose:
the kernel promises nothing about them, so the tests compare built graphs only - and the guard words around every array."""
import numpy as np


def relabel(node_ptr, edge_ptr, rowptr, col, nattr, eattr, max_nodes, max_edges, old_of_new, target_node_ptr=None, target_max_nodes=None,
            fill=-7):
    node_ptr = np.asarray(node_ptr, np.int64); edge_ptr = np.asarray(edge_ptr, np.int64)
    tptr = node_ptr if target_node_ptr is None else np.asarray(target_node_ptr, np.int64)
    G = node_ptr.size - 1
    if target_max_nodes is None:
        target_max_nodes = int(np.diff(tptr).max()) if G else 0
    T, E = int(tptr[-1]), int(edge_ptr[-1])
    out = dict(rowptr=np.full(T + G, fill, np.int32), col=np.full(E, fill, np.int32), eorder=np.full(E, fill, np.int32),
               nattr=None if nattr is None else np.full(T, fill & 0xFF, np.uint8), eattr=None if eattr is None else np.full(E, fill & 0xFF, np.uint8),
               status=np.zeros(G, np.int32))
    info = np.zeros(8, np.int32)
    groups = np.zeros(((G + 63) // 64, 2), np.int64)
    for g in range(G):
        nb, ne, tb, te, e0, e1 = node_ptr[g], node_ptr[g + 1], tptr[g], tptr[g + 1], edge_ptr[g], edge_ptr[g + 1]
        n, nt, e = int(ne - nb), int(te - tb), int(e1 - e0)
        ok = 0 <= nb <= ne <= node_ptr[-1] and 0 <= tb <= te <= T and 0 <= e0 <= e1 <= E and n <= max_nodes and nt <= target_max_nodes \
            and n <= nt and e <= max_edges
        if ok:
            oon = np.asarray(old_of_new[tb:te], np.int64)
            named = oon[(oon >= 0) & (oon < n)]
            ok = named.size == n and np.unique(named).size == n
        if ok:
            rp = np.asarray(rowptr[nb + g:ne + g + 1], np.int64)
            ok = (rp[0] == 0 and rp[-1] == e and (np.diff(rp) >= 0).all()) if n else e == 0
        if ok:
            c = np.asarray(col[e0:e1], np.int64)
            ok = bool(((c >= 0) & (c < n)).all())
        if not ok:
            out["status"][g] = 1
            info[0] += 1
            continue
        new_of_old = np.empty(n, np.int64)
        present = (oon >= 0) & (oon < n)
        new_of_old[oon[present]] = np.nonzero(present)[0]
        deg_old = np.diff(rp)
        row_old = np.repeat(np.arange(n), deg_old)
        new_row, new_col = new_of_old[row_old], new_of_old[c]
        perm = np.lexsort((np.arange(e), new_col, new_row))          # by new row, then new column, then input position: stable
        deg_new = np.zeros(nt, np.int64)
        deg_new[present] = deg_old[oon[present]]
        out["rowptr"][tb + g:te + g + 1] = np.concatenate([[0], np.cumsum(deg_new)])
        out["col"][e0:e1] = new_col[perm]
        out["eorder"][e0:e1] = perm
        if eattr is not None:
            out["eattr"][e0:e1] = np.asarray(eattr[e0:e1])[perm]
        if nattr is not None:
            na = np.full(nt, 255, np.uint8)
            na[present] = np.asarray(nattr[nb:ne])[oon[present]]
            out["nattr"][tb:te] = na
        pairs = new_row * (nt + 1) + new_col
        simple = np.unique(pairs).size == e and not (row_old == c).any()
        out["status"][g] = 0 if simple else 2
        info[6] += 0 if simple else 1
        info[1] = max(info[1], int(deg_new.max()) if nt else 0)
        info[2] = max(info[2], nt); info[3] = max(info[3], e)
        groups[g // 64] += (nt, e)
    if G:
        info[4], info[5] = groups[:, 0].max(), groups[:, 1].max()
    out["info"] = info
    return out
