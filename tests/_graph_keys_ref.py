"""The key of gtok_graph_keys (include/gtok.h; csrc/gtok_graph_keys_hash.hpp, frozen in DESIGN.md), restated with numpy - the
yardstick of tests/test_host_graph_keys.py and tests/test_gpu_graph_keys.py - beside the DEFINITION it digests: the reference's tuple
key (test/train_performance_test.py:70-74), tuple_key() below.

  entry word   a | b << 14 | t << 28, a = min(u, v), b = max(u, v), t = the entry's attribute byte (0 without attributes)
  node word    u | x[u] << 14 | 1 << 40                                 (with attributes only)
  S_j          sum of mix(word ^ C_j) over the terms, mod 2^64
  key_j        mix(S_j + mix((N | terms << 32) ^ C_j) + mix(label ^ D_j))   (label: the int32's 32-bit pattern)

LISTED: the terms are all listed entries.  CLOSURE: the LISTED key of simple_once_listing() - every distinct edge once, every looped
node's loop once."""
import numpy as np

C = (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F)
D = (0x165667B19E3779F9, 0x85EBCA77C2B2AE63)
U = np.uint64


def mix(z):
    """the splitmix64 finaliser on a uint64 array (array arithmetic wraps mod 2^64)"""
    z = np.atleast_1d(np.asarray(z, U)).copy()
    z ^= z >> U(30); z *= U(0xBF58476D1CE4E5B9)
    z ^= z >> U(27); z *= U(0x94D049BB133111EB)
    z ^= z >> U(31)
    return z


def u8(a):
    """attribute ids as the batch stores them (csr._to_u8): anything outside 0..254 is 255"""
    a = np.asarray(a, np.int64).reshape(-1)
    return np.where((a >= 0) & (a < 255), a, 255).astype(U)


def words(n, src, dst, x=None, edge_attr=None):
    src, dst = np.asarray(src, np.int64).reshape(-1), np.asarray(dst, np.int64).reshape(-1)
    a, b = np.minimum(src, dst).astype(U), np.maximum(src, dst).astype(U)
    t = np.zeros(src.size, U) if edge_attr is None else u8(edge_attr)
    w = a | b << U(14) | t << U(28)
    if x is not None:
        w = np.concatenate([w, np.arange(n, dtype=U) | u8(x) << U(14) | U(1 << 40)])
    return w


def digest(n, w, label=0):
    """-> uint64 [2]"""
    out = np.zeros(2, U)
    head = np.array([int(n) | int(w.size) << 32], U)
    lab = np.array([int(label) & 0xFFFFFFFF], U)
    for j in range(2):
        s = mix(w ^ U(C[j])).sum(dtype=U) if w.size else U(0)
        out[j] = mix(np.array([s], U) + mix(head ^ U(C[j])) + mix(lab ^ U(D[j])))[0]
    return out


def simple_once_listing(src, dst):
    """the simple undirected closure of a listing, listed once: every distinct {u, v}, u != v, as (min, max); every looped node as (v, v)"""
    src, dst = np.asarray(src, np.int64).reshape(-1), np.asarray(dst, np.int64).reshape(-1)
    pairs = np.unique(np.minimum(src, dst) << 14 | np.maximum(src, dst))
    return pairs >> 14, pairs & 16383


def listed_key(n, src, dst, label=0, x=None, edge_attr=None):
    return digest(n, words(n, src, dst, x, edge_attr), label)


def closure_key(n, src, dst, label=0):
    return listed_key(n, *simple_once_listing(src, dst), label)


def tuple_key(n, src, dst, label=0, x=None, edge_attr=None):
    """compute_graph_hash of the reference: (num_nodes, the sorted tuple of the listed edges with each edge's endpoints sorted, label);
    with attributes every edge carries its byte and the node bytes follow"""
    src, dst = np.asarray(src, np.int64).reshape(-1).tolist(), np.asarray(dst, np.int64).reshape(-1).tolist()
    if x is None:
        return (int(n), tuple(sorted(tuple(sorted(e)) for e in zip(src, dst))), int(label))
    t = u8(edge_attr).tolist()
    return (int(n), tuple(sorted(tuple(sorted(e)) + (tt,) for e, tt in zip(zip(src, dst), t))), tuple(u8(x).tolist()), int(label))


def closure_tuple_key(n, src, dst, label=0):
    return tuple_key(n, *simple_once_listing(src, dst), label)


def fast_key(n, src, dst, label=0, x=None, edge_attr=None):
    """tuple_key with the sorted list held as the bytes of a sorted array of packed (a, b, t): equal exactly when the tuples are, and
    quick enough for corpora of thousands of graphs"""
    src, dst = np.asarray(src, np.int64).reshape(-1), np.asarray(dst, np.int64).reshape(-1)
    t = 0 if edge_attr is None else u8(edge_attr).astype(np.int64) << 28
    lst = np.sort(np.minimum(src, dst) | np.maximum(src, dst) << 14 | t).tobytes()
    return (int(n), lst, None if x is None else u8(x).tobytes(), int(label))


def per_graph(node_counts, edge_counts, src, dst, labels=None, x=None, edge_attr=None):
    """the graphs of a batched COO one by one: (n, src, dst, label, x, edge_attr)"""
    node_counts, edge_counts = np.asarray(node_counts, np.int64), np.asarray(edge_counts, np.int64)
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    nptr, eptr = np.concatenate([[0], np.cumsum(node_counts)]), np.concatenate([[0], np.cumsum(edge_counts)])
    for g in range(node_counts.size):
        e = slice(eptr[g], eptr[g + 1])
        yield (int(node_counts[g]), src[e], dst[e], 0 if labels is None else int(labels[g]),
               None if x is None else np.asarray(x)[nptr[g]:nptr[g + 1]], None if edge_attr is None else np.asarray(edge_attr)[e])


def batch_keys(node_counts, edge_counts, src, dst, labels=None, mode="listed", x=None, edge_attr=None):
    """-> uint64 [G, 2], as gtok_graph_keys defines them"""
    out = [listed_key(n, s, d, lab, xx, ea) if mode == "listed" else closure_key(n, s, d, lab)
           for n, s, d, lab, xx, ea in per_graph(node_counts, edge_counts, src, dst, labels, x, edge_attr)]
    return np.array(out, U).reshape(-1, 2)


def batch_tuples(node_counts, edge_counts, src, dst, labels=None, mode="listed", x=None, edge_attr=None, fast=False):
    key = fast_key if fast else tuple_key
    return [key(n, s, d, lab, xx, ea) if mode == "listed" else key(n, *simple_once_listing(s, d), lab)
            for n, s, d, lab, xx, ea in per_graph(node_counts, edge_counts, src, dst, labels, x, edge_attr)]


def classes(tuples):
    """group[i] = the index of the first graph with graph i's tuple"""
    first = {}
    return np.array([first.setdefault(t, i) for i, t in enumerate(tuples)], np.int64)


def tree_splits(tree):
    """a synth.graph_token_tree directory ({path: records}, cycle_check) -> {split: batched COO + labels (yes = 1) + family names}"""
    out = {}
    for rel, recs in tree.items():
        _, _, alg, split, _ = rel.split("/")
        tok = recs[0]["text"].split()
        e = [(int(tok[i - 2]), int(tok[i - 1])) for i, t in enumerate(tok) if t == "<e>"]
        n = tok.index("<q>") - tok.index("<n>") - 1
        d = out.setdefault(split, dict(node_counts=[], edge_counts=[], src=[], dst=[], labels=[], family=[]))
        d["node_counts"].append(n); d["edge_counts"].append(len(e)); d["labels"].append(int(tok[tok.index("<p>") + 1] == "yes"))
        d["src"] += [u for u, _ in e]; d["dst"] += [v for _, v in e]; d["family"].append(alg)
    return {s: {k: (v if k == "family" else np.asarray(v, np.int64)) for k, v in d.items()} for s, d in out.items()}


def set_report(tuples_per_split):
    """the reference's Test 2 on lists of tuple keys: (unique per split, overlap matrix)"""
    sets = [set(t) for t in tuples_per_split]
    return [len(s) for s in sets], [[len(a & b) for b in sets] for a in sets]
