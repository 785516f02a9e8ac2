"""gtok_ibtt_decode_sizes / gtok_ibtt_decode_csr (include/gtok.h): IBTT rows back to a batched CSR on the device.

Two yardsticks.  (1) IBTT keeps the input's node numbering and edge order, so rows the CPU oracle serialised decode to the
input batch itself (GraphBatch.from_coo of the input).  (2) The host reference decoder of tests/_ibtt_decode_ref.py - one token
at a time, from the grammar rules - judges every row of every test, cut and malformed ones included: status and all arrays are
compared exactly.  No test skips or filters rows."""
import ctypes

import numpy as np
import pytest
import torch

import _ibtt_decode_ref as ref
from _util import gtok, orc, zinc_vocab

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_lib = gtok._lib
MAXN = _lib.SENT_LARGE_MAX_NODES
ZINC, SYNTH = ref.ZINC, ref.SYNTH


# ------------------------------------------------------------------------------------------------ vocabularies, inputs
def synth_vocab(num_node_ids):
    toks = ["<pad>", "<bos>", "<eos>", "<e>", "<n>", "<q>", "<p>", "yes", "no"] + [str(i) for i in range(num_node_ids)]
    return {t: i for i, t in enumerate(toks)}


class Vocab:
    def __init__(self, grammar, num_node_ids, vocab=None):
        self.grammar = grammar
        self.vocab = vocab if vocab is not None else (zinc_vocab(num_node_ids) if grammar == ZINC else synth_vocab(num_node_ids))
        self.lut = (gtok.ops.zinc_lut if grammar == ZINC else gtok.ops.synth_lut)(self.vocab, num_node_ids).numpy()
        self.size = max(self.vocab.values()) + 1
        self.pad = self.vocab["<pad>"]
        self.inv_t = gtok.ops.ibtt_inverse_lut(self.lut, self.size, self.pad)
        self.inv = ref.inverse_lut(self.lut, self.size, self.pad)
        assert np.array_equal(self.inv_t.numpy(), self.inv)


def molecules(specs):
    """specs: [(num_atoms, [(u, v), ...])] -> a PyG-coalesced batch: both directions, row-sorted, node types 0..8, mirrored entries
    with equal bond types (0..4)"""
    nc, ec, srcs, dsts, xs, eas = [], [], [], [], [], []
    for n, pairs in specs:
        p = np.array(sorted({(min(u, v), max(u, v)) for u, v in pairs}), np.int64).reshape(-1, 2)
        s, d = np.concatenate([p[:, 0], p[:, 1]]), np.concatenate([p[:, 1], p[:, 0]])
        o = np.lexsort((d, s))
        nc.append(n); ec.append(s.size); srcs.append(s[o]); dsts.append(d[o]); xs.append((np.arange(n) * 5 + n) % 9); eas.append((s[o] + d[o]) % 5)
    cat = lambda l: np.concatenate(l) if l else np.zeros(0, np.int64)
    return dict(node_counts=np.array(nc, np.int64), edge_counts=np.array(ec, np.int64), src=cat(srcs), dst=cat(dsts), x=cat(xs), edge_attr=cat(eas))


def path(n):
    return (n, [(i, i + 1) for i in range(n - 1)])


def edge_lists(specs):
    """specs: [(num_nodes, [(u, v), ...])] as listed"""
    return dict(node_counts=np.array([n for n, _ in specs], np.int64), edge_counts=np.array([len(e) for _, e in specs], np.int64),
                src=np.array([u for _, e in specs for u, _ in e], np.int64), dst=np.array([v for _, e in specs for _, v in e], np.int64))


def oracle_rows(d, V, max_len=1 << 20, query=None, ld=None):
    if V.grammar == ZINC:
        coo = orc.Coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], d["x"], d["edge_attr"])
        ld = ld or int(4 + 2 * d["node_counts"].max() + 2 * d["edge_counts"].max())
        return orc.ibtt_zinc(coo, V.lut, max_len, V.pad, ld)
    coo = orc.Coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"])
    ld = ld or int(8 + d["node_counts"].max() + 3 * d["edge_counts"].max())
    return orc.ibtt_synth(coo, V.lut, query, max_len, V.pad, ld)


def input_batch(d, typed):
    return gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], d["x"] if typed else None,
                                    d["edge_attr"] if typed else None, check_symmetric=False)


def zinc_tokens(V, types, bonds, tail=("q", "regression", "p")):
    """a molecule row written by hand: bonds (u, v, type) exactly as listed"""
    L = V.lut
    t = [L[0]]
    for a in types:
        t += [L[2], L[7 + a]]
    for u, v, b in bonds:
        t += [L[3], L[17 + b], L[22 + u], L[22 + v]]
    return [int(x) for x in t + [L[{"q": 4, "regression": 5, "p": 6, "eos": 1}[k]] for k in tail]]


def slab(rows, pad):
    ld = max(4, max(len(r) for r in rows))
    ids = np.full((len(rows), ld), pad, np.int32)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = r
    return ids, np.array([len(r) for r in rows], np.int32)


# ------------------------------------------------------------------------------------------------ comparing
def _identity_order(edge_ptr):
    ep = edge_ptr.cpu().numpy()
    return (np.arange(int(ep[-1])) - np.repeat(ep[:-1], np.diff(ep))).astype(np.int32)


def same_batch(got, want, what, eorder=True):
    h = lambda t: None if t is None else t.cpu().numpy()
    assert got.num_graphs == want.num_graphs, what
    for k in ("node_ptr", "edge_ptr", "rowptr", "col", "nattr", "eattr"):
        a, b = h(getattr(got, k)), h(getattr(want, k))
        assert (a is None) == (b is None), (what, k)
        if a is not None:
            assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
            bad = np.nonzero(a != b)[0]
            assert bad.size == 0, f"{what}: {k} differs at {bad[:8]}: {a[bad[:8]]} vs {b[bad[:8]]}"
    if eorder:
        eo = lambda x: _identity_order(x.edge_ptr) if x.eorder is None else h(x.eorder)
        assert np.array_equal(eo(got), eo(want)), (what, "eorder")
    for k in ("max_degree", "max_nodes", "max_edges", "chunk_nodes", "chunk_edges"):       # info[1..5]
        assert getattr(got, k) == getattr(want, k), (what, k, getattr(got, k), getattr(want, k))


def decode_and_check(ids_t, ln_t, V, maxn, rows, what, row_start=None, ld=None):
    """decode on the device; compare status, every array and the query with the reference decoder's over `rows` (token lists)"""
    out = gtok.ops.ibtt_decode_csr(ids_t, ln_t, V.grammar, V.inv_t, maxn, row_start=row_start, ld=ld)
    got, st = out[0], out[1].cpu().numpy()
    exp = ref.expected(rows, V.grammar, V.inv, maxn)
    bad = np.nonzero(st != exp["status"])[0]
    assert bad.size == 0, f"{what}: status differs at rows {bad[:8]}: {st[bad[:8]]} vs {exp['status'][bad[:8]]}"
    same_batch(got, exp["batch"], what)
    if V.grammar == SYNTH:
        assert np.array_equal(out[2].cpu().numpy(), exp["query"]), (what, "query")
    else:
        assert len(out) == 2
    return got, st, exp


def decode_slab(ids, ln, V, maxn, what):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return decode_and_check(t(ids), t(ln), V, maxn, ref.rows_of(ids, ln), what)


# ------------------------------------------------------------------------------------------------ 1. chunk borders
def test_molecules_whose_records_straddle_the_64_token_border():
    V = Vocab(ZINC, 40)
    d = molecules([path(1), path(2), path(31), path(32), path(33), (10, [(i, i + 1) for i in range(9)] + [(0, 9)])])
    ids, ln = oracle_rows(d, V)
    assert ln.tolist()[:5] == [6, 12, 186, 192, 198] and ln[5] == 64            # 4 + 2 N + 4 B
    got, st, exp = decode_slab(ids, ln, V, 40, "paths")
    assert (st == 0).all()
    same_batch(got, input_batch(d, True), "paths vs the input", eorder=False)     # yardstick 1
    # rows of exactly 63 and 65 tokens: the 33-atom path cut by max_len (ends in <eos>) and by len (does not)
    big = molecules([path(33)] * 3)
    for cut in (63, 64, 65):
        ci, cl = oracle_rows(big, V, max_len=cut)
        assert cl.tolist() == [cut] * 3
        _, st, _ = decode_slab(ci, cl, V, 40, f"max_len {cut}")
        assert (st == 3).all()
        _, st, _ = decode_slab(ids[2:5], np.minimum(ln[2:5], cut).astype(np.int32), V, 40, f"len {cut}")
        assert (st == 3).all()


def test_graph_token_rows_of_63_64_and_65_tokens():
    V = Vocab(SYNTH, 40)
    rng = np.random.default_rng(2)
    specs = [(6, [(int(a), int(b)) for a, b in rng.integers(0, 6, (17, 2))]) for _ in range(2)] + [(4, [(int(a), int(b)) for a, b in rng.integers(0, 4, (18, 2))])]
    d = edge_lists(specs)
    query = np.array([[2, 7, 8, 0], [3, 8, 7, 9], [3, 9, 9, 9]], np.int32)       # 4 + 3 M + N + nq tokens
    ids, ln = oracle_rows(d, V, query=query)
    assert ln.tolist() == [63, 64, 65]
    got, st, exp = decode_slab(ids, ln, V, 40, "63 / 64 / 65")
    assert (st == 0).all()
    same_batch(got, input_batch(d, False), "63 / 64 / 65 vs the input")
    # 70 edges: more than one step of 64 records, cut at the borders
    d = edge_lists([(9, [(int(a), int(b)) for a, b in rng.integers(0, 9, (70, 2))])] * 3)
    ids, ln = oracle_rows(d, V)
    got, st, _ = decode_slab(ids, ln, V, 40, "70 edges")
    same_batch(got, input_batch(d, False), "70 edges vs the input")
    for cut in (63, 64, 65, 192, 193, 194):
        _, st, _ = decode_slab(ids, np.minimum(ln, cut).astype(np.int32), V, 40, f"len {cut}")
        assert (st == 3).all()


# ------------------------------------------------------------------------------------------------ 2. every cut position
@pytest.mark.parametrize("grammar", [ZINC, SYNTH])
def test_every_cut_position_of_one_graph(grammar):
    V = Vocab(grammar, 40)
    if grammar == ZINC:
        d = molecules([(6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 5), (1, 4)])])
        query = None
    else:
        d = edge_lists([(6, [(0, 1), (5, 2), (2, 3), (3, 3), (4, 0), (1, 5), (2, 1)])])
        query = np.array([[2, 7, 8, 0]], np.int32)
    full_ids, full_ln = oracle_rows(d, V, query=query)
    full = int(full_ln[0])
    rows = []
    for max_len in range(1, full + 2):
        ci, cl = oracle_rows(d, V, max_len=max_len, query=query, ld=full + 1)
        rows.append(ci[0, :int(cl[0])].tolist())
    ids, ln = slab(rows, V.pad)
    got, st, exp = decode_slab(ids, ln, V, 6, "cut by max_len")
    assert set(st.tolist()) == {0, 3}                                              # both occur, status 1 nowhere
    assert st[-1] == 0 and st[0] == 3
    # the same rows read with ld narrower than len: cut without the <eos>
    for w in (full - 1, full // 2, 5):
        narrow = np.ascontiguousarray(ids[:, :w])
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        _, st2, _ = decode_and_check(t(narrow), t(ln), V, 6, ref.rows_of(narrow, ln), f"ld {w}")
        assert 1 not in st2.tolist() and 3 in st2.tolist()
    # ... and every prefix of the whole row, all rows reading the same buffer
    flat = torch.from_numpy(full_ids[0, :full].copy()).to(DEV)
    pl = np.arange(1, full + 1, dtype=np.int32)
    starts = torch.zeros(full, dtype=torch.int64, device=DEV)
    _, st3, _ = decode_and_check(flat, torch.from_numpy(pl).to(DEV), V, 6, [full_ids[0, :n].tolist() for n in pl], "prefixes", row_start=starts)
    assert st3.tolist() == [3] * (full - 1) + [0]


# ------------------------------------------------------------------------------------------------ 3. malformed rows
def _with_defects(good, defects, pad):
    """good row, defect, good row, defect, ... as a flat int32 buffer with row_start / len"""
    rows = []
    for i, dft in enumerate(defects):
        rows += [list(good[i % len(good)]), list(dft)]
    rows.append(list(good[0]))
    starts, flat, at = [], [], 3
    for r in rows:
        starts.append(at); flat += r; at += len(r)
    buf = np.full(at + 3, pad, np.int32); buf[3:at] = flat
    return rows, buf, np.array(starts, np.int64), np.array([len(r) for r in rows], np.int32)


def test_malformed_molecule_rows_are_empty_graphs_and_leave_their_neighbours_intact():
    V = Vocab(ZINC, 40)
    maxn = 12
    d = molecules([path(5), (6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 5)]), path(12)])
    ids, ln = oracle_rows(d, V)
    good = [ids[g, :int(ln[g])].tolist() for g in range(3)]
    g0 = good[1]
    edit = lambda i, v: g0[:i] + [v] + g0[i + 1:]
    first_bond = 1 + 2 * 6
    too_many = oracle_rows(molecules([path(13)]), V)
    defects = [
        edit(0, V.vocab["<eos>"]),                                  # wrong first token
        edit(2, V.vocab["<unk>"]),                                  # an id no slot owns
        edit(2, V.size + 5),                                        # id >= inv_len
        edit(2, -3),                                                # a negative int32 id
        edit(first_bond + 2, int(V.lut[22 + 6])),                   # bond endpoint >= N
        g0 + [V.vocab["<eos>"]],                                    # <p> followed by <eos>
        too_many[0][0, :int(too_many[1][0])].tolist(),              # N > max_num_nodes
        g0,                                                         # (negative row_start, below)
        g0,                                                         # (len 0, below)
    ]
    rows, buf, starts, lens = _with_defects(good, defects, V.pad)
    starts[2 * 7 + 1] = -1; rows[2 * 7 + 1] = []
    lens[2 * 8 + 1] = 0; rows[2 * 8 + 1] = []
    t = lambda a: torch.from_numpy(a).to(DEV)
    got, st, exp = decode_and_check(t(buf), t(lens), V, maxn, rows, "defects", row_start=t(starts))
    assert st.tolist() == [0, 1] * len(defects) + [0]
    nn = np.diff(got.node_ptr.cpu().numpy())
    assert (nn[1::2] == 0).all() and nn[0::2].tolist() == [(5, 6, 12)[i % 3] for i in range(len(defects))] + [5]
    nn2, ne2, st2 = gtok.ops.ibtt_decode_sizes(t(buf), t(lens), ZINC, V.inv_t, maxn, row_start=t(starts))      # (query = NULL)
    assert np.array_equal(st2.cpu().numpy(), st) and bool((nn2[1::2] == 0).all()) and bool((ne2[1::2] == 0).all())
    o = gtok.ops._ibtt_decode_csr_launch(t(buf), t(lens), t(starts), None, ZINC, V.inv_t, maxn, got.node_ptr, got.edge_ptr, got.num_nodes_total,
                                         got.num_edges_total)
    info = o["info"].cpu().numpy()
    assert info[0] == 0 and info[6] == len(defects)


def test_malformed_graph_token_rows_are_empty_graphs_and_leave_their_neighbours_intact():
    V = Vocab(SYNTH, 40)
    maxn = 12
    d = edge_lists([(5, [(0, 1), (4, 2), (2, 2)]), (6, [(0, 5), (5, 1), (3, 2), (1, 4)]), (12, [(11, 0), (3, 7)])])
    query = np.array([[1, 7, 0, 0], [3, 8, 7, 8], [0, 0, 0, 0]], np.int32)
    ids, ln = oracle_rows(d, V, query=query)
    good = [ids[g, :int(ln[g])].tolist() for g in range(3)]
    g1 = good[1]                                                    # <bos> 4 records <n> 0..5 <q> q0 q1 q2 <p>
    edit = lambda i, v: g1[:i] + [v] + g1[i + 1:]
    node = lambda k: int(V.lut[5 + k])
    n_at = 1 + 3 * 4
    swapped = list(g1); swapped[n_at + 2], swapped[n_at + 3] = swapped[n_at + 3], swapped[n_at + 2]
    too_many = oracle_rows(edge_lists([(13, [(0, 1)])]), V)
    defects = [
        edit(0, V.vocab["<n>"]),                                    # wrong first token
        edit(4, V.vocab["yes"]),                                    # an id no slot owns
        edit(4, V.size),                                            # id >= inv_len
        edit(4, -1),                                                # a negative int32 id
        edit(1, node(6)),                                           # edge endpoint >= N after a full node list
        swapped,                                                    # node list out of order
        g1[:-1] + [7, V.vocab["<p>"]],                              # four tokens after <q>
        too_many[0][0, :int(too_many[1][0])].tolist(),              # N > max_num_nodes
        g1, g1,                                                     # (negative row_start, len 0)
    ]
    rows, buf, starts, lens = _with_defects(good, defects, V.pad)
    starts[2 * 8 + 1] = -5; rows[2 * 8 + 1] = []
    lens[2 * 9 + 1] = 0; rows[2 * 9 + 1] = []
    t = lambda a: torch.from_numpy(a).to(DEV)
    got, st, exp = decode_and_check(t(buf), t(lens), V, maxn, rows, "defects", row_start=t(starts))
    assert st.tolist() == [0, 1] * len(defects) + [0]
    keep = np.array([i % 3 for i in range(len(defects))] + [0])
    assert np.array_equal(exp["query"][0::2], query[keep]) and (exp["query"][1::2] == 0).all()
    nn2, ne2, st2 = gtok.ops.ibtt_decode_sizes(t(buf), t(lens), SYNTH, V.inv_t, maxn, row_start=t(starts))     # query = NULL: skipped
    assert np.array_equal(st2.cpu().numpy(), st) and np.array_equal(nn2.cpu().numpy(), exp["node_counts"]) and np.array_equal(ne2.cpu().numpy(), exp["edge_counts"])


# ------------------------------------------------------------------------------------------------ 4. the scatter
def test_rows_of_more_than_64_entries_self_loops_duplicates_and_unsorted_lists():
    V = Vocab(SYNTH, 80)
    rng = np.random.default_rng(4)
    centre_first = [(0, i) for i in range(1, 71)]
    leaf_first = [(i, 0) for i in range(1, 71)]
    both_ways = [e for i in range(1, 71) for e in ((i, 0), (0, i))]          # row 0 fills up across three steps, between other rows
    dense = [(int(a), int(b)) for a, b in rng.integers(0, 50, (3000, 2))]    # (no entry is staged: any count goes through the same path)
    d = edge_lists([(71, centre_first), (71, leaf_first), (71, both_ways), (50, dense), (3, [(0, 1), (1, 2)])])
    ids, ln = oracle_rows(d, V)
    got, st, exp = decode_slab(ids, ln, V, 80, "stars")
    assert (st == 0).all() and got.max_degree >= 70 and got.eorder is not None
    eo = got.eorder.cpu().numpy()
    assert not np.array_equal(eo, _identity_order(got.edge_ptr))
    want = input_batch(d, False)
    same_batch(got, want, "stars vs the input")
    # sorted lists alone: info[7] stays 0 and no eorder is kept
    d2 = edge_lists([(71, centre_first), (71, leaf_first)])
    i2, l2 = oracle_rows(d2, V)
    got2, _, _ = decode_slab(i2, l2, V, 80, "sorted stars")
    assert got2.eorder is None
    # molecules written by hand: a star listed leaf-first, a self loop, a duplicate bond, a bond listed high end first
    Z = Vocab(ZINC, 80)
    rows = [zinc_tokens(Z, [0] * 71, [(i, 0, 1 + i % 4) for i in range(1, 71)]),
            zinc_tokens(Z, [0] * 71, [(0, i, i % 5) for i in range(1, 71)]),
            zinc_tokens(Z, [1, 2, 3], [(0, 1, 1), (2, 2, 2), (1, 2, 3)]),
            zinc_tokens(Z, [1, 2, 9], [(0, 1, 1), (0, 1, 2), (1, 0, 4), (2, 1, 0)])]
    ids, ln = slab(rows, Z.pad)
    got, st, exp = decode_slab(ids, ln, Z, 80, "hand-made molecules")
    assert (st == 0).all() and exp["edge_counts"].tolist() == [140, 140, 5, 8] and got.max_degree == 70
    assert got.nattr.cpu().numpy()[-1] == 255                                   # 'X'


# ------------------------------------------------------------------------------------------------ 5. widths and forms
@pytest.mark.parametrize("grammar", [ZINC, SYNTH])
def test_slab_packed_rows_at_4_2_and_1_bytes_and_rows_in_another_order(grammar):
    V = Vocab(grammar, 40)
    assert V.size < 256
    G = 150
    if grammar == ZINC:
        d = gtok.synth.zinc_like(G, seed=7)
        d["x"] = d["x"] % 9
        query = None
    else:
        rng = np.random.default_rng(8)
        d = edge_lists([(int(n), [(int(a), int(b)) for a, b in rng.integers(0, n, (int(e), 2))]) for n, e in zip(rng.integers(1, 38, G), rng.integers(0, 60, G))])
        query = np.zeros((G, 4), np.int32); query[:, 0] = np.arange(G) % 4
        query[:, 1:] = np.where(np.arange(3)[None, :] < query[:, :1], rng.integers(7, V.size, (G, 3)), 0)
    ids, ln = oracle_rows(d, V, max_len=150, query=query)
    rows = ref.rows_of(ids, ln)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    ids_t, ln_t = t(ids), t(ln)
    got, st, exp = decode_and_check(ids_t, ln_t, V, 40, rows, "int32 slab")
    assert 0 in st.tolist() and 3 in st.tolist() and 1 not in st.tolist()
    whole = st == 0
    ld = int(ids.shape[1])
    for eb, align in ((4, 1), (2, 8), (1, 16)):
        packed, row_ptr, pst = gtok.ops.pack_rows_scan(ids_t, ln_t, eb, G * ld, align)
        assert int(pst.item()) == 0 and packed.element_size() == eb
        gp, sp, _ = decode_and_check(packed, ln_t, V, 40, rows, f"packed, {eb} bytes", row_start=row_ptr[:-1].contiguous(), ld=ld)
        same_batch(gp, got, f"packed, {eb} bytes vs the slab")
    # rows in another order than they are stored
    perm = np.random.default_rng(9).permutation(G)
    starts = row_ptr[:-1][t(perm)].contiguous()
    decode_and_check(packed, ln_t[t(perm)].contiguous(), V, 40, [rows[i] for i in perm], "permuted rows", row_start=starts, ld=ld)
    # the uncut rows are the input graphs
    if whole.all():
        same_batch(got, input_batch(d, grammar == ZINC), "vs the input", eorder=grammar == SYNTH)
    else:
        sub_n, sub_e = exp["node_counts"][whole], exp["edge_counts"][whole]
        assert np.array_equal(sub_n, d["node_counts"][whole]) and np.array_equal(sub_e, d["edge_counts"][whole])


# ------------------------------------------------------------------------------------------------ 6. large
def test_a_path_of_16384_nodes_and_one_node_too_many():
    V = Vocab(SYNTH, MAXN)
    a = np.arange(MAXN - 1)
    d = edge_lists([(MAXN, list(zip(a.tolist(), (a + 1).tolist()))), (3, [(2, 1), (1, 0)])])
    ids, ln = oracle_rows(d, V)
    assert int(ln[0]) == 4 + 3 * (MAXN - 1) + MAXN
    got, st, exp = decode_slab(ids, ln, V, MAXN, "largest path")
    assert st.tolist() == [0, 0] and exp["node_counts"].tolist() == [MAXN, 3]
    same_batch(got, input_batch(d, False), "largest path vs the input")
    got, st, exp = decode_slab(ids, ln, V, MAXN - 1, "one node too many")
    assert st.tolist() == [1, 0] and np.diff(got.node_ptr.cpu().numpy()).tolist() == [0, 3]


# ------------------------------------------------------------------------------------------------ 7. raw calls
GUARD = 4096
FILL32, FILL8 = -77, 0xAB


class Raw:
    """caller-side arrays of gtok_ibtt_decode_csr with 4,096-element guard regions on both sides of every output"""

    def __init__(self, rows, N, E, typed):
        self.sizes = dict(rowptr=N + rows, col=E, eorder=E, nattr=N if typed else 0, eattr=E if typed else 0, info=8)
        self.buf = {}
        for k, n in self.sizes.items():
            u8 = k in ("nattr", "eattr")
            self.buf[k] = torch.full((GUARD + n + GUARD,), FILL8 if u8 else FILL32, dtype=torch.uint8 if u8 else torch.int32, device=DEV)
        self.typed = typed

    def view(self, k):
        return self.buf[k][GUARD:GUARD + self.sizes[k]]

    def struct(self, node_ptr, edge_ptr):
        p = lambda k: self.buf[k].data_ptr() + GUARD * self.buf[k].element_size()
        typed = lambda k: p(k) if (self.typed or k not in ("nattr", "eattr")) else None
        return _lib.GtokCsrBuilt(node_ptr.data_ptr(), edge_ptr.data_ptr(), p("rowptr"), p("col"), p("eorder"), typed("nattr"), typed("eattr"), p("info"))

    def guards_untouched(self):
        for k, b in self.buf.items():
            fill = FILL8 if b.dtype == torch.uint8 else FILL32
            assert bool((b[:GUARD] == fill).all()) and bool((b[GUARD + self.sizes[k]:] == fill).all()), k

    def untouched(self):
        for k, b in self.buf.items():
            assert bool((b == (FILL8 if b.dtype == torch.uint8 else FILL32)).all()), k


def _zinc_case():
    V = Vocab(ZINC, 40)
    d = gtok.synth.zinc_like(80, seed=12)
    d["x"] = d["x"] % 9
    ids, ln = oracle_rows(d, V)
    return V, d, ids, ln


def test_a_tampered_edge_ptr_is_counted_and_nothing_is_written_outside_a_slice():
    V, d, ids, ln = _zinc_case()
    want = input_batch(d, True)
    rows, ld = ids.shape
    nc, ec = d["node_counts"].copy(), d["edge_counts"].copy()
    ec[11] -= 1                      # one entry too few for row 11
    nc[60] += 1                      # one node too many for row 60
    node_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(nc)]).astype(np.int32)).to(DEV)
    edge_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(ec)]).astype(np.int64)).to(DEV)
    raw = Raw(rows, int(nc.sum()), int(ec.sum()), True)
    ids_t, ln_t, inv = torch.from_numpy(ids).to(DEV), torch.from_numpy(ln).to(DEV), V.inv_t.to(DEV)
    cout = raw.struct(node_ptr, edge_ptr)
    assert _lib.lib().gtok_ibtt_decode_csr(ids_t.data_ptr(), 4, None, ld, ln_t.data_ptr(), rows, ZINC, inv.data_ptr(), inv.numel(), 40,
                                           ctypes.byref(cout), None) == 0
    torch.cuda.synchronize()
    raw.guards_untouched()
    info = raw.view("info").cpu().numpy()
    assert info[0] == 2 and info[6] == 0
    g_np, g_ep = node_ptr.cpu().numpy(), edge_ptr.cpu().numpy()
    w_np, w_ep = want.node_ptr.numpy(), want.edge_ptr.numpy()
    out = {k: raw.view(k).cpu().numpy() for k in ("rowptr", "col", "nattr", "eattr")}
    for g in range(rows):
        if g in (11, 60):
            continue
        n, e = int(nc[g]), int(ec[g])
        assert np.array_equal(out["rowptr"][g_np[g] + g:g_np[g] + g + n + 1], want.rowptr.numpy()[w_np[g] + g:w_np[g] + g + n + 1]), g
        assert np.array_equal(out["col"][g_ep[g]:g_ep[g] + e], want.col.numpy()[w_ep[g]:w_ep[g] + e]), g
        assert np.array_equal(out["nattr"][g_np[g]:g_np[g] + n], want.nattr.numpy()[w_np[g]:w_np[g] + n]), g
        assert np.array_equal(out["eattr"][g_ep[g]:g_ep[g] + e], want.eattr.numpy()[w_ep[g]:w_ep[g] + e]), g
    assert (out["col"][g_ep[11]:g_ep[12]] == FILL32).all() and (out["nattr"][g_np[60]:g_np[61]] == FILL8).all()


def test_error_codes_and_no_rows_leave_the_outputs_untouched():
    V, d, ids, ln = _zinc_case()
    want = input_batch(d, True)
    rows, ld = ids.shape
    node_ptr, edge_ptr = want.node_ptr.to(DEV), want.edge_ptr.to(DEV)
    raw = Raw(rows, want.num_nodes_total, want.num_edges_total, True)
    cout = raw.struct(node_ptr, edge_ptr)
    ids_t, ln_t, inv = torch.from_numpy(ids).to(DEV), torch.from_numpy(ln).to(DEV), V.inv_t.to(DEV)
    L = _lib.lib()

    def csr(eb=4, ld_=ld, ln_=ln_t, n=rows, gr=ZINC, inv_=inv, il=inv.numel(), maxn=40, out=cout):
        return L.gtok_ibtt_decode_csr(ids_t.data_ptr(), eb, None, ld_, None if ln_ is None else ln_.data_ptr(), n, gr,
                                      None if inv_ is None else inv_.data_ptr(), il, maxn, ctypes.byref(out), None)
    assert csr(eb=3) == -1 and csr(ld_=0) == -1 and csr(ln_=None) == -1 and csr(n=-1) == -1 and csr(gr=2) == -1
    assert csr(inv_=None) == -1 and csr(il=0) == -1 and csr(maxn=MAXN + 1) == -2
    no_types = raw.struct(node_ptr, edge_ptr); no_types.nattr = None
    assert csr(out=no_types) == -1                                   # molecules need nattr / eattr
    assert csr(n=0) == 0
    sizes = [torch.full((rows,), FILL32, dtype=torch.int32, device=DEV) for _ in range(3)]
    query = torch.full((rows, 4), FILL32, dtype=torch.int32, device=DEV)

    def call_sizes(eb=4, gr=SYNTH, il=inv.numel(), maxn=40, n=rows):
        return L.gtok_ibtt_decode_sizes(ids_t.data_ptr(), eb, None, ld, ln_t.data_ptr(), n, gr, inv.data_ptr(), il, maxn,
                                        *[s.data_ptr() for s in sizes], query.data_ptr(), None)
    assert call_sizes(eb=8) == -1 and call_sizes(gr=-1) == -1 and call_sizes(il=-4) == -1 and call_sizes(maxn=MAXN + 1) == -2 and call_sizes(n=0) == 0
    torch.cuda.synchronize()
    raw.untouched()
    assert all(bool((s == FILL32).all()) for s in sizes) and bool((query == FILL32).all())
    with pytest.raises(gtok.GtokError, match="GTOK_E_TOO_LARGE"):
        gtok.ops.ibtt_decode_csr(ids_t, ln_t, "zinc", V.inv_t, MAXN + 1)
    empty, st = gtok.ops.ibtt_decode_csr(ids_t[:0], ln_t[:0], "zinc", V.inv_t, 40)
    assert empty.num_graphs == 0 and st.numel() == 0 and empty.col.numel() == 0 and empty.rowptr.numel() == 0


# ------------------------------------------------------------------------------------------------ 8. the vocab is an input
def test_a_vocab_with_shuffled_node_ids_and_one_that_lacks_a_node_index():
    d = molecules([path(7), path(9), (8, [(0, 7), (7, 3), (1, 2)]), path(3)])
    base = zinc_vocab(40)
    rng = np.random.default_rng(10)
    node_toks = [str(i) for i in range(40)]
    shuffled = dict(base)
    for tok, i in zip(node_toks, rng.permutation([base[t] for t in node_toks]).tolist()):
        shuffled[tok] = i
    V = Vocab(ZINC, 40, shuffled)
    assert not np.array_equal(V.lut, Vocab(ZINC, 40).lut)
    ids, ln = oracle_rows(d, V)
    got, st, _ = decode_slab(ids, ln, V, 40, "shuffled node ids")
    assert (st == 0).all()
    same_batch(got, input_batch(d, True), "shuffled node ids vs the input", eorder=False)
    lacking = {t: i for t, i in base.items() if t != "7"}
    W = Vocab(ZINC, 40, lacking)
    assert W.lut[22 + 7] == W.pad and W.inv[W.pad] == -1
    ids, ln = oracle_rows(d, W)
    got, st, exp = decode_slab(ids, ln, W, 40, "no token for node 7")
    assert st.tolist() == [0, 1, 1, 0]                              # a molecule that uses node 7 is malformed, not a wrong graph
    assert np.diff(got.node_ptr.cpu().numpy()).tolist() == [7, 0, 0, 3]


# ------------------------------------------------------------------------------------------------ 9. through the interface
def test_gpu_serialiser_torch_ops_and_the_dataset_method():
    V = Vocab(ZINC, 40)
    d = gtok.synth.zinc_like(200, seed=14)
    d["x"] = d["x"] % 9
    want = input_batch(d, True)
    dev = gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], d["x"], d["edge_attr"]).to(DEV)
    ids, ln = gtok.ops.ibtt_zinc(dev, torch.from_numpy(V.lut), 4096, V.pad)
    got, st = gtok.ops.ibtt_decode_csr(ids, ln, "zinc", V.inv_t, 40, check_symmetric=True)
    assert bool((st == 0).all()) and got.flags & _lib.CSR_SIMPLE_SYMMETRIC
    same_batch(got, want, "ibtt_zinc -> ibtt_decode_csr", eorder=False)
    decode_and_check(ids, ln, V, 40, ref.rows_of(ids.cpu().numpy(), ln.cpu().numpy()), "GPU serialiser's rows")
    inv = V.inv_t.to(DEV)
    nn, ne, s3, q = torch.ops.gtok.ibtt_decode_sizes(ids, ln, ZINC, inv, 40)
    assert torch.equal(s3, st) and torch.equal(torch.cumsum(nn, 0), got.node_ptr[1:].to(torch.int64)) and not bool(q.any())
    rowptr, col, eorder, nattr, eattr, info = torch.ops.gtok.ibtt_decode_csr(ids, ln, ZINC, inv, 40, got.node_ptr, got.edge_ptr,
                                                                             got.num_nodes_total, got.num_edges_total)
    assert torch.equal(rowptr, got.rowptr) and torch.equal(col, got.col) and torch.equal(nattr, got.nattr) and torch.equal(eattr, got.eattr)
    v = info.tolist()
    assert v[0] == 0 and v[1:6] == [want.max_degree, want.max_nodes, want.max_edges, want.chunk_nodes, want.chunk_edges] and v[6] == 0
    m = lambda x: x.to("meta")
    fake = torch.ops.gtok.ibtt_decode_csr(m(ids), m(ln), ZINC, m(inv), 40, m(got.node_ptr), m(got.edge_ptr), got.num_nodes_total, got.num_edges_total)
    real = (rowptr, col, eorder, nattr, eattr, info)
    assert [(tuple(f.shape), f.dtype) for f in fake] == [(tuple(r.shape), r.dtype) for r in real]
    fake = torch.ops.gtok.ibtt_decode_sizes(m(ids), m(ln), ZINC, m(inv), 40)
    assert [(tuple(f.shape), f.dtype) for f in fake] == [(tuple(r.shape), r.dtype) for r in (nn, ne, s3, q)]
    # the dataset decodes its own rows with the vocab it tokenized with
    ds = gtok.graph_data_loader.ZINCTokenizationDataset(split="train", zinc_dataset=gtok.synth.InMemoryLike(d))
    tids, tln = ds.tokenize(V.vocab, device=torch.device(DEV))
    back, bst = ds.decode_batch(tids, tln)
    assert bool((bst == 0).all())
    same_batch(back, want, "decode_batch", eorder=False)
