"""A host reference decoder for IBTT rows: plain Python, one token at a time, written from the grammar rules of include/gtok.h
(gtok_ibtt_decode_sizes) - the yardstick of tests/test_gpu_ibtt_decode.py.  Its entries go through the HOST GraphBatch.from_coo.

    decode_row(tokens, grammar, inv, max_num_nodes) -> dict(status, n, src, dst, etype, ntype, query)
    expected(rows, grammar, inv, max_num_nodes)     -> dict(status, batch, node_counts, edge_counts, src, dst, query, ...)
"""
import numpy as np

from _util import gtok

ZINC, SYNTH = 0, 1
# LUT slots (include/gtok.h: GTOK_ZLUT_* / GTOK_SLUT_*)
Z_BOS, Z_EOS, Z_ATOM, Z_BOND, Z_Q, Z_REGRESSION, Z_P, Z_ATOM0, Z_BOND0, Z_NODE0 = 0, 1, 2, 3, 4, 5, 6, 7, 17, 22
S_BOS, S_E, S_N, S_Q, S_P, S_NODE0 = 0, 1, 2, 3, 4, 5


def inverse_lut(lut, vocab_size, pad_id=None):
    """inv[id] = the one LUT slot that holds id, else -1; pad_id names no token (restated here so that the yardstick does not lean
    on ops.py)"""
    inv = [-1] * vocab_size
    count = [0] * vocab_size
    for slot, tid in enumerate(np.asarray(lut).reshape(-1).tolist()):
        if 0 <= tid < vocab_size:
            count[tid] += 1
            inv[tid] = slot
    return np.array([s if c == 1 and t != pad_id else -1 for t, (s, c) in enumerate(zip(inv, count))], np.int32)


def _classes(tokens, inv):
    return [int(inv[t]) if 0 <= t < len(inv) else -1 for t in tokens]


def _empty(status):
    return dict(status=status, n=0, src=[], dst=[], etype=[], ntype=[], query=[0, 0, 0, 0])


def _zinc(tokens, inv, maxn):
    c = _classes(tokens, inv)
    if len(c) < 1:
        return _empty(1)
    dropped = c[-1] == Z_EOS
    if dropped:
        c.pop()
    if not c:
        return _empty(3)
    if c[0] != Z_BOS:
        return _empty(1)
    i, ntype = 1, []
    while i + 1 < len(c) and c[i] == Z_ATOM and Z_ATOM0 <= c[i + 1] <= Z_ATOM0 + 9:
        t = c[i + 1] - Z_ATOM0
        ntype.append(255 if t == 9 else t)
        i += 2
    n = len(ntype)
    is_node = lambda s: s >= Z_NODE0 and s - Z_NODE0 < n
    is_type = lambda s: Z_BOND0 <= s <= Z_BOND0 + 4
    bonds = []
    while i + 3 < len(c) and c[i] == Z_BOND and is_type(c[i + 1]) and is_node(c[i + 2]) and is_node(c[i + 3]):
        bonds.append((c[i + 2] - Z_NODE0, c[i + 3] - Z_NODE0, c[i + 1] - Z_BOND0))
        i += 4
    rest, tail = c[i:], [Z_Q, Z_REGRESSION, Z_P]
    if rest == tail:
        status = 1 if dropped else 0
    elif len(rest) < 3 and rest == tail[:len(rest)]:
        status = 3
    elif len(rest) < 4 and rest[0] == Z_BOND and all(ok(s) for ok, s in zip((is_type, is_node), rest[1:])):
        status = 3
    elif rest == [Z_ATOM] and not bonds:
        status = 3
    else:
        status = 1
    if n > maxn:
        status = 1
    if status == 1:
        return _empty(1)
    src, dst, et = [], [], []
    for u, v, t in bonds:
        src.append(u); dst.append(v); et.append(t)
        if u != v:
            src.append(v); dst.append(u); et.append(t)
    return dict(status=status, n=n, src=src, dst=dst, etype=et, ntype=ntype, query=[0, 0, 0, 0])


def _synth(tokens, inv, maxn):
    c = _classes(tokens, inv)
    L = len(c)
    if L < 1 or c[0] != S_BOS:
        return _empty(1)
    i, edges = 1, []
    while i + 2 < L and c[i] >= S_NODE0 and c[i + 1] >= S_NODE0 and c[i + 2] == S_E:
        edges.append((c[i] - S_NODE0, c[i + 1] - S_NODE0))
        i += 3
    top = max([max(e) for e in edges], default=-1)
    S, q_seen, status, query = 0, False, 1, [0, 0, 0, 0]
    if i == L:
        status = 3
    elif c[i] != S_N:
        status = 3 if L - i <= 2 and all(s >= S_NODE0 for s in c[i:]) else 1
    else:
        i += 1
        while i < L and c[i] == S_NODE0 + S:
            S += 1
            i += 1
        if i == L:
            status = 3
        elif c[i] != S_Q:
            status = 1
        else:
            q_seen = True
            after = L - i - 1
            if after >= 1 and c[L - 1] == S_P and 0 <= after - 1 <= 3:
                status = 0
                query = ([after - 1] + [int(t) for t in tokens[i + 1:L - 1]] + [0, 0, 0])[:4]
            elif after <= 3:
                status = 3
            else:
                status = 1
    if q_seen:
        n = S
        if top >= S:
            status = 1
    else:
        n = max(S, top + 1)
    if n > maxn:
        status = 1
    if status == 1:
        return _empty(1)
    return dict(status=status, n=n, src=[u for u, _ in edges], dst=[v for _, v in edges], etype=[], ntype=[], query=query)


def decode_row(tokens, grammar, inv, max_num_nodes):
    return (_zinc if grammar == ZINC else _synth)([int(t) for t in tokens], inv, max_num_nodes)


def expected(rows, grammar, inv, max_num_nodes):
    """rows: a list of token lists (an int32 row is a list of ints; a row with a negative start or len < 1 is [])."""
    dec = [decode_row(r, grammar, inv, max_num_nodes) for r in rows]
    cat = lambda k: np.array([v for d in dec for v in d[k]], np.int64)
    nc = np.array([d["n"] for d in dec], np.int64); ec = np.array([len(d["src"]) for d in dec], np.int64)
    typed = grammar == ZINC
    batch = gtok.GraphBatch.from_coo(nc, ec, cat("src"), cat("dst"), cat("ntype") if typed else None, cat("etype") if typed else None,
                                     check_symmetric=False)
    return dict(status=np.array([d["status"] for d in dec], np.int32), batch=batch, node_counts=nc, edge_counts=ec, src=cat("src"),
                dst=cat("dst"), ntype=cat("ntype"), etype=cat("etype"), query=np.array([d["query"] for d in dec], np.int32).reshape(-1, 4),
                rows=dec)


def rows_of(ids, ln, ld=None, row_start=None):
    """the token lists a decoder call reads: ids a [rows, ld] array, or a flat array with row_start"""
    ids = np.asarray(ids)
    out = []
    for r, n in enumerate(np.asarray(ln).tolist()):
        if row_start is None:
            out.append(ids[r, :max(0, min(n, ids.shape[1]))].tolist())
        else:
            s = int(row_start[r]); n = n if ld is None else min(n, ld)
            out.append([] if s < 0 or n < 1 else ids[s:s + n].tolist())
    return out
