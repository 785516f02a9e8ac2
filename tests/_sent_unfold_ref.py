"""The unfold of ZINC-remapped labelled SENT rows, restated in Python from the rule in include/gtok.h (not from the kernel):
pre() - the inverse of the remap - and unfold() - one id of look-ahead, one bit of state."""
import numpy as np

X, NONE = 2, None


def remap(t, M, T):
    """trainer/train_agtt.py:171-244 on one raw id"""
    node_off, edge_off = 6 + M, 6 + M + T
    if t == 0:
        return 0
    if t in (1, 2, 3, 5):
        return X
    if t == 4:
        return 1
    if node_off <= t < edge_off:
        return 8 + (t - node_off) if t - node_off < 9 else 22 + t
    if t >= edge_off:
        return 17 + (t - edge_off) if t - edge_off < 4 else 22 + t
    return 22 + (t - 6) if 6 <= t < node_off else 22 + t


def pre(i, M, T):
    """the raw id t >= 0 outside {1, 2, 3, 5} with remap(t) == i, or NONE"""
    node_off, edge_off = 6 + M, 6 + M + T
    if i == 0 or i == 1:
        return 4 * i
    if 8 <= i <= 16:
        t = node_off + (i - 8)
    elif 17 <= i <= 20:
        t = edge_off + (i - 17)
    elif 22 <= i < 22 + M:
        t = 6 + (i - 22)
    elif i >= 22 + node_off:
        t = i - 22
    else:
        return NONE
    return t if remap(t, M, T) == i else NONE


def unfold(row, M, T):
    """the ids of one row (a sequence of ints: its first min(len, ld) ids) -> the unfolded ids"""
    edge_off, out, opened = 6 + M + T, [], False
    for k, i in enumerate(row):
        if i == X:
            nxt = pre(row[k + 1], M, T) if k + 1 < len(row) else NONE
            if opened:
                out.append(3); opened = False
            elif nxt is not NONE and nxt >= edge_off:
                out.append(2); opened = True
            else:
                out.append(1)
        else:
            p = pre(i, M, T)
            out.append(5 if p is NONE else p)
    return out


def unfold_rows(ids, ln, M, T, pad=5):
    """int [G, ld] rows (any integer dtype; 16-bit ids already widened), len [G] -> int32 [G, ld]: unfolded, `pad` behind them"""
    ids = np.asarray(ids); G, ld = ids.shape
    out = np.full((G, ld), pad, np.int32)
    for g in range(G):
        L = max(0, min(int(ln[g]), ld))
        out[g, :L] = unfold(ids[g, :L].tolist(), M, T)
    return out
