"""gtok_unremap_zinc / gtok_sent_decode_zinc_sizes / gtok_sent_decode_zinc_csr (include/gtok.h): ZINC-remapped labelled SENT rows
back to raw ids and to a batched CSR on the device.

The expected result of every test is built the same way: the Python unfold of tests/_sent_unfold_ref.py (written from the rule in
include/gtok.h, pinned to the C oracle's rows by tests/test_host_sent_decode_zinc.py), then the C oracle's decoder and the HOST
GraphBatch.from_coo as in tests/test_gpu_sent_decode_csr.py.  Everything is compared exactly."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from _sent_unfold_ref import X, unfold_rows
from _util import both, edge_case_graphs, golden_zinc_coo, gtok, orc, zinc_data_list
from test_gpu_sent_decode_csr import FILL32, GUARD, Raw, _identity_order, check, expected, same_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_lib = gtok._lib
MAXN = _lib.SENT_LARGE_MAX_NODES
RESET, LADJ, RADJ, PAD = 1, 2, 3, 5
ZINC = dict(labeled=True, num_node_types=28, num_edge_types=4)


def _host(ids):
    h = ids.cpu().numpy()
    return h.view(np.uint16).astype(np.int32) if h.dtype == np.int16 else h.astype(np.int32)


def expected_zinc(ids, ln, M, T):
    """remapped rows on the host (int32 [G, ld]), len -> what test_gpu_sent_decode_csr.expected gives for the unfolded rows"""
    return expected(unfold_rows(ids, ln, M, T), ln, M, True, T)


def decode_and_check(ids, ln, M, T, what):
    got, st = gtok.ops.sent_decode_zinc_csr(ids, ln, M, T)
    exp = expected_zinc(_host(ids), ln.cpu().numpy(), M, T)
    check(got, st, exp, what)
    return got, st, exp


# ------------------------------------------------------------------------------------------------ 1. molecules, every row format
@functools.lru_cache(maxsize=None)
def _molecules(max_len):
    d = gtok.synth.zinc_like(300, seed=21)
    batch, coo = both(d)
    dev = batch.to(DEV)
    ids, ln = gtok.ops.sent(dev, 37, max_len, 5, 3, remap_zinc=True, **ZINC)
    raw, rln = gtok.ops.sent(dev, 37, max_len, 5, 3, **ZINC)
    assert torch.equal(ln, rln)
    exp = expected_zinc(ids.cpu().numpy(), ln.cpu().numpy(), 37, 28)
    return batch, coo, ids, ln, raw, exp


@pytest.mark.parametrize("max_len", [4096, 50])
def test_molecules_as_slab_u16_slab_and_packed_rows(max_len):
    batch, _, ids, ln, raw, exp = _molecules(max_len)
    dev = batch.to(DEV)
    ld = int(ids.shape[1])
    assert int(ids.max()) == 97                                        # (one byte per id holds every remapped id)
    got, st = gtok.ops.sent_decode_zinc_csr(ids, ln, 37, 28)
    check(got, st, exp, f"int32 slab max_len={max_len}")
    assert max_len != 50 or (exp["status"] == 3).sum() > 100
    # ... which is what the un-remapped rows of the same walk decode to
    graw, sraw = gtok.ops.sent_decode_csr(raw, ln, 37, True, 28)
    assert torch.equal(sraw, st)
    same_batch(got, graw, "the un-remapped rows of the same walk")
    nn, ne, s2 = gtok.ops.sent_decode_zinc_sizes(ids, ln, 37, 28)
    assert torch.equal(s2, st) and torch.equal(torch.cumsum(nn, 0).to(torch.int32), got.node_ptr[1:]) and torch.equal(torch.cumsum(ne, 0), got.edge_ptr[1:])
    # the same rows as a slab of 16-bit ids (written by the walk)
    i16, l16 = gtok.ops.sent(dev, 37, max_len, 5, 3, remap_zinc=True, u16=True, ld=ld, **ZINC)
    assert i16.dtype == torch.int16 and torch.equal(l16, ln)
    g16, s16 = gtok.ops.sent_decode_zinc_csr(i16, l16, 37, 28)
    assert torch.equal(s16, st)
    same_batch(g16, got, "16-bit slab")
    # packed rows at 1, 2 and 4 bytes per id
    for eb, align in ((1, 16), (2, 8), (4, 1)):
        packed, row_ptr, pst = gtok.ops.pack_rows_scan(ids, ln, eb, 300 * ld, align)
        assert int(pst.item()) == 0 and packed.element_size() == eb
        gp, sp = gtok.ops.sent_decode_zinc_csr(packed, ln, 37, 28, row_start=row_ptr[:-1].contiguous(), ld=ld)
        assert torch.equal(sp, st)
        same_batch(gp, got, f"packed rows, {eb} bytes per id")
    # a row that did not fit its packed buffer (row_start -1) is an empty graph, status 1
    starts = row_ptr[:-1].clone()
    starts[7] = -1
    gm, sm = gtok.ops.sent_decode_zinc_csr(packed, ln, 37, 28, row_start=starts, ld=ld)
    ln0 = ln.cpu().numpy().copy(); ln0[7] = 0
    check(gm, sm, expected_zinc(ids.cpu().numpy(), ln0, 37, 28), "row_start -1")
    assert int(sm[7]) == 1 and int(gm.node_ptr[8] - gm.node_ptr[7]) == 0
    if max_len == 4096:
        # the folded id as the LAST token of a 64-token chunk, its successor in the next one, in all three roles
        h, r, n = ids.cpu().numpy(), raw.cpu().numpy(), ln.cpu().numpy()
        at63 = (n > 64) & (h[:, 63] == X)
        roles = np.bincount(r[at63, 63], minlength=4)
        assert roles[LADJ] > 0 and roles[RADJ] > 0 and roles[RESET] > 0 and roles[0] == 0, roles
        assert (exp["status"] == 0).all()
        gf, _ = gtok.ops.sent_decode_zinc_csr(ids, ln, 37, 28, check_symmetric=True)
        assert gf.flags & _lib.CSR_SIMPLE_SYMMETRIC and gf.checked and not (got.flags & _lib.CSR_SIMPLE_SYMMETRIC)
        same_batch(gf, got, "check_symmetric")


# ------------------------------------------------------------------------------------------------ 2. unremap_zinc == the raw rows
@pytest.mark.parametrize("max_len", [4096, 50])
def test_unremap_zinc_gives_the_raw_rows_of_the_same_walk(max_len):
    batch, coo, ids, ln, raw, _ = _molecules(max_len)
    ld = int(ids.shape[1])
    want, wln = orc.sent(coo, 37, max_len, 5, 3, ld=ld, **ZINC)       # the oracle's un-remapped rows, padding included
    n = ln.cpu().numpy()
    assert np.array_equal(wln, n) and np.array_equal(raw.cpu().numpy(), want)
    out = gtok.ops.unremap_zinc(ids, ln, 37, 28)
    assert out.dtype == torch.int32 and tuple(out.shape) == (300, ld)
    got, h = out.cpu().numpy(), ids.cpu().numpy()
    assert np.array_equal(got, unfold_rows(h, n, 37, 28)), "the kernel is not the Python unfold"
    ends_in_x = h[np.arange(300), np.minimum(n, ld) - 1] == X
    if max_len == 4096:
        assert not ends_in_x.any() and np.array_equal(got, want)
    else:
        # a cut may leave a row ending in the folded id: only that last id may differ (RESET where the walk wrote LADJ)
        assert ends_in_x.sum() > 10
        last = np.zeros_like(got, bool)
        last[np.nonzero(ends_in_x)[0], n[ends_in_x] - 1] = True
        assert np.array_equal(got[~last], want[~last])
        differs = got[last] != want[last]
        assert (got[last][differs] == RESET).all() and (want[last][differs] == LADJ).all()
    # every row format gives the same slab; another pad id
    i16, _ = gtok.ops.sent(batch.to(DEV), 37, max_len, 5, 3, remap_zinc=True, u16=True, ld=ld, **ZINC)
    assert torch.equal(gtok.ops.unremap_zinc(i16, ln, 37, 28), out)
    for eb, align in ((1, 16), (2, 8), (4, 1)):
        packed, row_ptr, _ = gtok.ops.pack_rows_scan(ids, ln, eb, 300 * ld, align)
        assert torch.equal(gtok.ops.unremap_zinc(packed, ln, 37, 28, row_start=row_ptr[:-1].contiguous(), ld=ld), out), eb
    starts = row_ptr[:-1].clone(); starts[7] = -1
    o7 = gtok.ops.unremap_zinc(packed, ln, 37, 28, row_start=starts, ld=ld, pad_id=-3).cpu().numpy()
    assert (o7[7] == -3).all() and np.array_equal(np.where(o7 == -3, PAD, o7)[np.arange(300) != 7], got[np.arange(300) != 7])
    with pytest.raises(ValueError):
        gtok.ops.unremap_zinc(packed, ln, 37, 28, row_start=starts)


# ------------------------------------------------------------------------------------------------ 3. the flag across chunks
def _complete(n):
    iu, iv = np.triu_indices(n, 1)
    return np.concatenate([iu, iv]), np.concatenate([iv, iu])


def test_brackets_longer_than_a_chunk_carry_the_flag_across_chunks():
    parts = [_complete(40), _complete(70), (np.array([0, 1, 1, 2]), np.array([1, 0, 2, 1]))]
    src = np.concatenate([p[0] for p in parts]).astype(np.int64); dst = np.concatenate([p[1] for p in parts]).astype(np.int64)
    d = dict(node_counts=np.array([40, 70, 3]), edge_counts=np.array([p[0].size for p in parts]), src=src, dst=dst,
             x=np.concatenate([np.arange(n) % 9 for n in (40, 70, 3)]), edge_attr=(src + dst) % 4)
    batch, _ = both(d)
    dev = batch.to(DEV)
    kw = dict(labeled=True, num_node_types=9, num_edge_types=4)
    ids, ln = gtok.ops.sent(dev, 70, 1 << 20, 9, 0, remap_zinc=True, **kw)
    raw, _ = gtok.ops.sent(dev, 70, 1 << 20, 9, 0, **kw)
    row = raw[1, :int(ln[1])].cpu().numpy()
    opens, closes = np.nonzero(row == LADJ)[0], np.nonzero(row == RADJ)[0]
    assert opens.size == closes.size and int((closes - opens - 1).max()) > 64      # a bracket of more than one 64-token chunk
    _, _, exp = decode_and_check(ids, ln, 70, 9, "complete graphs, whole")
    assert (exp["status"] == 0).all() and exp["edge_counts"].tolist() == [40 * 39, 70 * 69, 4]
    assert torch.equal(gtok.ops.unremap_zinc(ids, ln, 70, 9), raw)
    h = ids.cpu().numpy()
    for cut in (63, 64, 65, 128, 129):
        cl = torch.clamp(ln, max=cut)
        _, _, exp = decode_and_check(ids, cl, 70, 9, f"complete graphs cut at {cut}")
        assert exp["status"].tolist() == [3, 3, 0]
        assert np.array_equal(gtok.ops.unremap_zinc(ids, cl, 70, 9).cpu().numpy(), unfold_rows(h, cl.cpu().numpy(), 70, 9)), cut


# ------------------------------------------------------------------------------------------------ 4. out-of-range types
@pytest.mark.parametrize("M,T,ET", [(8, 28, 6), (8, 3, 2)])
def test_hand_made_graphs_with_out_of_range_types(M, T, ET):
    """types 200 / 254 / 77: the fallback ids (22 + t), node types that spill into the bond range where T = 3; max_len 9, 5, 2 and 1
    cut inside a bracket, between a position and its type, behind SOS"""
    batch, _ = both(edge_case_graphs())
    dev = batch.to(DEV)
    kw = dict(labeled=True, num_node_types=T, num_edge_types=ET)
    seen = set()
    for max_len in (4096, 9, 5, 2, 1):
        ids, ln = gtok.ops.sent(dev, M, max_len, 3, 2, remap_zinc=True, **kw)
        raw, _ = gtok.ops.sent(dev, M, max_len, 3, 2, **kw)
        what = f"hand-made M={M} T={T} max_len={max_len}"
        got, st, exp = decode_and_check(ids, ln, M, T, what)
        graw, sraw = gtok.ops.sent_decode_csr(raw, ln, M, True, T)
        assert torch.equal(sraw, st)
        same_batch(got, graw, what + ": the un-remapped rows")
        i16, _ = gtok.ops.sent(dev, M, max_len, 3, 2, remap_zinc=True, u16=True, ld=int(ids.shape[1]), **kw)
        g16, s16 = gtok.ops.sent_decode_zinc_csr(i16, ln, M, T)
        assert torch.equal(s16, st)
        same_batch(g16, got, what + ": 16-bit slab")
        un = gtok.ops.unremap_zinc(ids, ln, M, T).cpu().numpy()
        assert np.array_equal(un, unfold_rows(ids.cpu().numpy(), ln.cpu().numpy(), M, T)), what
        assert torch.equal(gtok.ops.unremap_zinc(i16, ln, M, T).cpu(), torch.from_numpy(un))
        seen |= set(exp["status"].tolist())
        if max_len == 4096:
            assert int(ids.max()) > 255 and (exp["status"] == 0).all() and np.array_equal(un, raw.cpu().numpy())
    assert seen == {0, 3}


# ------------------------------------------------------------------------------------------------ 5. damaged rows
def damage(ids, ln, M, copies, rng):
    """`copies` copies of random rows of a valid remapped slab, each with one or two changes: an id in 0..7; a random position; one
    of 21, 17, 8, 22 + M + 3; a deleted id; a shorter len; the first id removed; an X inserted; an X removed"""
    R, ld = ids.shape
    out = np.full((copies, ld), PAD, np.int32); oln = np.empty(copies, np.int32)
    for c in range(copies):
        r = int(rng.integers(0, R))
        row = ids[r, :int(min(ln[r], ld))].tolist()
        for _ in range(int(rng.integers(1, 3))):
            L = len(row)
            if L == 0:
                break
            kind = int(rng.integers(0, 8))
            i = int(rng.integers(1, L)) if L > 1 else 0
            if kind == 0:
                row[i] = int(rng.integers(0, 8))
            elif kind == 1:
                row[i] = 22 + int(rng.integers(0, M))
            elif kind == 2:
                row[i] = (21, 17, 8, 22 + M + 3)[int(rng.integers(0, 4))]
            elif kind == 3:
                del row[i]
            elif kind == 4:
                row = row[:int(rng.integers(1, L + 1))]
            elif kind == 5:
                row = row[1:]
            elif kind == 6:
                if L < ld:
                    row.insert(i, X)
            else:
                xs = [k for k, t in enumerate(row) if t == X]
                if xs:
                    del row[xs[int(rng.integers(0, len(xs)))]]
        out[c, :len(row)] = row; oln[c] = len(row)
    return out, oln


def test_damaged_rows_get_the_status_and_graphs_of_their_unfolded_ids():
    d = gtok.synth.zinc_like(200, seed=62)
    batch, _ = both(d)
    ids, ln = gtok.ops.sent(batch.to(DEV), 37, 1024, 8, 0, remap_zinc=True, **ZINC)
    bad_ids, bad_ln = damage(ids.cpu().numpy(), ln.cpu().numpy(), 37, 1000, np.random.default_rng(6))
    t_ids, t_ln = torch.from_numpy(bad_ids).to(DEV), torch.from_numpy(bad_ln).to(DEV)
    got, st, exp = decode_and_check(t_ids, t_ln, 37, 28, "damaged rows")
    counts = np.bincount(exp["status"], minlength=4)
    assert counts[0] >= 100 and counts[1] >= 100 and counts[3] >= 100 and counts[2] == 0, counts
    nn, ne, s2 = gtok.ops.sent_decode_zinc_sizes(t_ids, t_ln, 37, 28)
    o = gtok.ops._decode_zinc_csr_launch(t_ids, t_ln, None, None, 37, 28, got.node_ptr, got.edge_ptr, got.num_nodes_total, got.num_edges_total)
    info = o["info"].cpu().numpy()
    assert info[0] == 0 and info[6] == int((exp["status"] == 1).sum())
    assert torch.equal(s2, st) and bool((nn[st == 1] == 0).all()) and bool((ne[st == 1] == 0).all())
    assert np.array_equal(gtok.ops.unremap_zinc(t_ids, t_ln, 37, 28).cpu().numpy(), unfold_rows(bad_ids, bad_ln, 37, 28))


# ------------------------------------------------------------------------------------------------ 6. raw calls, guard regions
def _call_csr(ids, eb, ld, ln, rows, maxn, nt, cout):
    return _lib.lib().gtok_sent_decode_zinc_csr(None if ids is None else ids.data_ptr(), eb, None, ld, None if ln is None else ln.data_ptr(), rows,
                                                maxn, nt, ctypes.byref(cout), None)


def test_slices_that_do_not_match_are_skipped_and_nothing_is_written_outside():
    _, _, ids, ln, _, exp = _molecules(4096)
    want = exp["batch"]
    rows, ld = int(ids.shape[0]), int(ids.shape[1])
    nc, ec = exp["node_counts"].copy(), exp["edge_counts"].copy()
    ec[11] -= 1                      # one entry too few for row 11
    nc[200] -= 1                     # one node too few for row 200
    node_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(nc)]).astype(np.int32)).to(DEV)
    edge_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(ec)]).astype(np.int64)).to(DEV)
    raw = Raw(rows, int(nc.sum()), int(ec.sum()), True)
    assert _call_csr(ids, 4, ld, ln, rows, 37, 28, raw.struct(node_ptr, edge_ptr)) == 0
    torch.cuda.synchronize()
    raw.guards_untouched()
    info = raw.view("info").cpu().numpy()
    assert info[0] == 2 and info[6] == 0
    g_np, g_ep = node_ptr.cpu().numpy(), edge_ptr.cpu().numpy()
    w_np, w_ep = want.node_ptr.numpy(), want.edge_ptr.numpy()
    out = {k: raw.view(k).cpu().numpy() for k in ("rowptr", "col", "eorder", "nattr", "eattr")}
    w_eo = _identity_order(want.edge_ptr) if want.eorder is None else want.eorder.numpy()
    for g in range(rows):
        if g in (11, 200):
            continue
        n, e = int(nc[g]), int(ec[g])
        assert np.array_equal(out["rowptr"][g_np[g] + g:g_np[g] + g + n + 1], want.rowptr.numpy()[w_np[g] + g:w_np[g] + g + n + 1]), g
        assert np.array_equal(out["col"][g_ep[g]:g_ep[g] + e], want.col.numpy()[w_ep[g]:w_ep[g] + e]), g
        assert np.array_equal(out["eorder"][g_ep[g]:g_ep[g] + e], w_eo[w_ep[g]:w_ep[g] + e]), g
        assert np.array_equal(out["nattr"][g_np[g]:g_np[g] + n], want.nattr.numpy()[w_np[g]:w_np[g] + n]), g
        assert np.array_equal(out["eattr"][g_ep[g]:g_ep[g] + e], want.eattr.numpy()[w_ep[g]:w_ep[g] + e]), g
    assert (out["col"][g_ep[11]:g_ep[12]] == FILL32).all() and (out["nattr"][g_np[200]:g_np[201]] == 0xAB).all()


def test_error_codes_and_no_rows_leave_the_outputs_untouched_and_unremap_writes_its_slab_only():
    _, _, ids, ln, raw_ids, exp = _molecules(4096)
    rows, ld = int(ids.shape[0]), int(ids.shape[1])
    want = exp["batch"]
    node_ptr, edge_ptr = want.node_ptr.to(DEV), want.edge_ptr.to(DEV)
    raw = Raw(rows, want.num_nodes_total, want.num_edges_total, True)
    cout = raw.struct(node_ptr, edge_ptr)
    assert _call_csr(ids, 3, ld, ln, rows, 37, 28, cout) == -1                        # elem_bytes 3: GTOK_E_INVAL
    assert _call_csr(ids, 4, ld, ln, rows, MAXN + 1, 28, cout) == -2                  # GTOK_E_TOO_LARGE
    assert _call_csr(ids, 4, ld, None, rows, 37, 28, cout) == -1                      # null len
    assert _call_csr(ids, 4, 0, ln, rows, 37, 28, cout) == -1                         # ld <= 0
    assert _call_csr(ids, 4, ld, ln, -1, 37, 28, cout) == -1
    assert _call_csr(ids, 4, ld, ln, rows, 37, -1, cout) == -1
    assert _call_csr(ids, 4, ld, ln, 0, 37, 28, cout) == 0                            # no rows: a no-op
    assert _call_csr(None, 4, ld, None, 0, 37, 28, cout) == 0
    sizes = [torch.full((rows,), FILL32, dtype=torch.int32, device=DEV) for _ in range(3)]
    call_sizes = lambda eb, ln_, n, maxn: _lib.lib().gtok_sent_decode_zinc_sizes(ids.data_ptr(), eb, None, ld, None if ln_ is None else ln_.data_ptr(), n,
                                                                                maxn, 28, *[t.data_ptr() for t in sizes], None)
    assert call_sizes(3, ln, rows, 37) == -1 and call_sizes(4, ln, rows, MAXN + 1) == -2 and call_sizes(4, None, rows, 37) == -1
    assert call_sizes(4, ln, 0, 37) == 0
    # gtok_unremap_zinc: the same codes, a null output; a call that runs writes exactly [rows, ld]
    slab = torch.full((GUARD + rows * ld + GUARD,), FILL32, dtype=torch.int32, device=DEV)
    out_p = slab.data_ptr() + GUARD * 4
    unremap = lambda eb, ld_, ln_, n, maxn, out: _lib.lib().gtok_unremap_zinc(ids.data_ptr(), eb, None, ld_, None if ln_ is None else ln_.data_ptr(), n,
                                                                             maxn, 28, PAD, out, None)
    assert unremap(3, ld, ln, rows, 37, out_p) == -1 and unremap(4, 0, ln, rows, 37, out_p) == -1 and unremap(4, ld, None, rows, 37, out_p) == -1
    assert unremap(4, ld, ln, rows, MAXN + 1, out_p) == -2 and unremap(4, ld, ln, rows, 37, None) == -1
    assert unremap(4, ld, ln, 0, 37, out_p) == 0 and unremap(4, ld, ln, 0, 37, None) == 0
    torch.cuda.synchronize()
    raw.untouched()
    assert all(bool((t == FILL32).all()) for t in sizes) and bool((slab == FILL32).all())
    assert unremap(4, ld, ln, rows, 37, out_p) == 0
    torch.cuda.synchronize()
    assert bool((slab[:GUARD] == FILL32).all()) and bool((slab[GUARD + rows * ld:] == FILL32).all())
    assert torch.equal(slab[GUARD:GUARD + rows * ld].view(rows, ld), raw_ids)
    with pytest.raises(gtok.GtokError, match="GTOK_E_TOO_LARGE"):
        gtok.ops.sent_decode_zinc_csr(ids, ln, MAXN + 1, 28)
    empty, st = gtok.ops.sent_decode_zinc_csr(ids[:0], ln[:0], 37, 28)
    assert empty.num_graphs == 0 and st.numel() == 0 and empty.col.numel() == 0 and empty.rowptr.numel() == 0
    assert tuple(gtok.ops.unremap_zinc(ids[:0], ln[:0], 37, 28).shape) == (0, ld)


# ------------------------------------------------------------------------------------------------ 7. through the interface
def _tokenizer(max_len=4096):
    tok = gtok.Graph2TrailTokenizer(dataset_names=[], max_length=max_len, truncation_length=max_len, labeled_graph=True, seed=5, device=DEV)
    tok.set_num_nodes(37); tok.set_num_node_and_edge_types(28, 4)
    return tok


def test_tokenizer_torch_ops_and_the_round_trip_to_the_input():
    batch, _, ids, ln, raw, exp = _molecules(4096)
    dev = batch.to(DEV)
    tok = _tokenizer()
    tids, tln = tok.tokenize_batch(dev, epoch=3, remap_zinc=True)
    assert torch.equal(tids, ids) and torch.equal(tln, ln)
    want, wst = gtok.ops.sent_decode_zinc_csr(ids, ln, 37, 28)
    got, st = tok.decode_batch_zinc(tids, tln)
    assert torch.equal(st, wst)
    same_batch(got, want, "decode_batch_zinc")
    for r in (0, 17, 299):
        row = ids[r, :int(ln[r])].to(torch.long).cpu()
        one = tok.decode_zinc(row)
        s, d, ty, x = exp["lists"][r]
        assert one["status"] == 0 and one["num_nodes"] == x.size
        assert np.array_equal(one["edge_index"].numpy(), np.stack([s, d])) and np.array_equal(one["edge_attr"].numpy(), np.minimum(ty, 255))
        assert np.array_equal(one["x"].numpy(), x)
        assert tok.decode(row)["status"] == 1                        # (the un-remapped decoder does not read these rows)
    # torch.ops.gtok.* == ops
    assert torch.equal(torch.ops.gtok.unremap_zinc(ids, ln, 37, 28), raw)
    nn, ne, s3 = torch.ops.gtok.sent_decode_zinc_sizes(ids, ln, 37, 28)
    assert torch.equal(s3, wst) and torch.equal(torch.cumsum(nn, 0), want.node_ptr[1:].to(torch.int64))
    rowptr, col, eorder, nattr, eattr, info = torch.ops.gtok.sent_decode_zinc_csr(ids, ln, 37, 28, want.node_ptr, want.edge_ptr,
                                                                                  want.num_nodes_total, want.num_edges_total)
    assert torch.equal(rowptr, want.rowptr) and torch.equal(col, want.col) and torch.equal(nattr, want.nattr) and torch.equal(eattr, want.eattr)
    v = info.tolist()
    assert v[0] == 0 and v[1:6] == [want.max_degree, want.max_nodes, want.max_edges, want.chunk_nodes, want.chunk_edges] and v[6] == 0
    assert np.array_equal(eorder.cpu().numpy(), _identity_order(want.edge_ptr) if want.eorder is None else want.eorder.cpu().numpy())
    # the round trip the decoder exists for: remapped rows -> the input graphs, in the input's numbering
    order = tok.visit_order(dev, epoch=3)
    back, bst = tok.decode_batch_like_zinc(tids, tln, like=dev, order=order, check_symmetric=True)
    assert int((bst != 0).sum()) == 0 and back.flags & _lib.CSR_SIMPLE_SYMMETRIC
    same = gtok.ops.graphs_equal(back, dev)
    assert tuple(same.shape) == (300,) and bool(same.all()), f"{int((~same).sum())} of 300 remapped rows do not decode to their input"


def _tiled(batch, K):
    """K copies of a device batch, one after another (what K epochs of it decode to)"""
    counts = lambda ptr: (ptr[1:] - ptr[:-1]).repeat(K)
    node_ptr = torch.zeros(K * batch.num_graphs + 1, dtype=torch.int32, device=batch.device)
    torch.cumsum(counts(batch.node_ptr), 0, dtype=torch.int32, out=node_ptr[1:])
    edge_ptr = torch.zeros(K * batch.num_graphs + 1, dtype=torch.int64, device=batch.device)
    torch.cumsum(counts(batch.edge_ptr), 0, out=edge_ptr[1:])
    rep = lambda t: None if t is None else t.repeat(K)
    return gtok.GraphBatch(K * batch.num_graphs, batch.max_nodes, batch.max_edges, node_ptr, edge_ptr, rep(batch.rowptr), rep(batch.col), None,
                           rep(batch.nattr), rep(batch.eattr))


def test_round_trip_of_8_bit_rows_packed_by_the_walk():
    """3,500 molecules x 8 epochs = 28,000 walks: the fewest at which the molecule kernel walks and packs (pk.fused); the 8-bit packed
    rows alone - no slab - decode to the input graphs"""
    G, K = 3500, 8
    d = gtok.synth.zinc_like(G, seed=23)
    batch, _ = both(d)
    dev = batch.to(DEV)
    tok = _tokenizer(1024)
    ld = gtok.ops.sent_safe_ld(dev, True, 1024)
    pk = gtok.ops.PackedRows(K * G, K * G * 128, True, DEV, elem_bytes=1)
    none, ln = gtok.ops.sent(dev, 37, 1024, seed=5, epoch=2, ld=ld, epochs=K, u16=True, packed=pk, slab=False, remap_zinc=True, **ZINC)
    assert none is None and pk.fused and pk.buf.dtype == torch.uint8 and int(pk.status()) == 0
    assert gtok.ops.last_sent_kernel() == "sent_lane_kernel"
    order = tok.visit_order(dev, epoch=2, epochs=K)
    back, st = tok.decode_batch_like_zinc(pk.buf, ln.reshape(-1), like=dev, order=order, row_start=pk.row_start)
    assert int((st != 0).sum()) == 0
    want = _tiled(dev, K)
    same = gtok.ops.graphs_equal(back, want)
    assert tuple(same.shape) == (K * G,) and bool(same.all()), f"{int((~same).sum())} of {K * G} packed rows do not decode to their input"


def test_dataset_decode_rows_picks_the_decoder_from_the_remap_switch():
    gdl = gtok.graph_data_loader
    src = gdl.ZINCDatasetForAutoGraph(split="train", zinc_dataset=zinc_data_list(golden_zinc_coo()))
    tok = gtok.Graph2TrailTokenizer(dataset_names=[], max_length=1024, truncation_length=1024, labeled_graph=True, undirected=True, device=DEV)
    max_nodes = max(d.num_nodes for d in src)
    nt, et = gdl.get_zinc_num_types()
    tok.set_num_nodes(max_nodes); tok.set_num_node_and_edge_types(nt, et)
    plain = gtok.agtt.TokenizedGraphDataset(src, tok, task="zinc", remap_to_fixed_vocab=False, device=DEV)
    remap = gtok.agtt.TokenizedGraphDataset(src, tok, task="zinc", remap_to_fixed_vocab=True, device=DEV)
    rids, rln = remap.tokenize_epoch(2)
    pids, pln = plain.tokenize_epoch(2)
    assert torch.equal(rln, pln) and not torch.equal(rids, pids)
    got, st = remap.decode_rows(rids, rln)
    want, wst = plain.decode_rows(pids, pln)
    assert torch.equal(st, wst) and int((st != 0).sum()) == 0 and got.num_graphs == len(src)
    same_batch(got, want, "decode_rows: remapped against un-remapped rows of the same epoch")
    exp = expected_zinc(rids.cpu().numpy(), rln.cpu().numpy(), max_nodes, nt)
    check(got, st, exp, "decode_rows")
    i16, l16 = remap.tokenize_epoch_u16(2)
    g16, s16 = remap.decode_rows(i16, l16)
    assert torch.equal(s16, st)
    same_batch(g16, got, "decode_rows over the 16-bit epoch slab")
