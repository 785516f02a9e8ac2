"""gtok_sent_packed where sent_blane_kernel walks (unlabelled batches of >= 20 k walks of graphs up to 256 nodes: config 5): the
walk appends every finished unit's rows to the packed buffer itself.  Every comparison is against the CPU oracle (orc.sent)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from _util import both, gtok, orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, MAXN, MAX_LEN, LD, PAD = 9, 256, 600, 608, 5
G5 = 20480
E_UNSUPPORTED, E_INVAL = gtok._lib.E_UNSUPPORTED, -1

_CORPUS, _ORACLE = {}, {}


def _corpus(name):
    """(device batch, oracle corpus) of the two config-5 corpora test_gpu_parity.py shows to run sent_blane_kernel<W=4> by default"""
    if name not in _CORPUS:
        d = gtok.synth.er_batch_device(G5, DEV, seed=3) if name == "er" else gtok.synth.mix_batch_device(G5, DEV, seed=4)
        batch, coo = both(d, False)
        _CORPUS[name] = (batch.to(DEV), coo)
    return _CORPUS[name]


def _oracle(name, epoch):
    """the oracle's rows (ld = LD) and lengths of one epoch of a config-5 corpus, computed once"""
    if (name, epoch) not in _ORACLE:
        _ORACLE[(name, epoch)] = orc.sent(_corpus(name)[1], MAXN, MAX_LEN, SEED, epoch, ld=LD, nthreads=8)
    return _ORACLE[(name, epoch)]


def _oracle_epochs(name, epoch0, K):
    refs = [_oracle(name, epoch0 + e) for e in range(K)]
    return np.concatenate([r for r, _ in refs]), np.concatenate([l for _, l in refs])


def _need(rln, ld, ev):
    return int(((np.clip(rln, 0, ld) + ev - 1) // ev * ev).sum())


def _host(t, u16):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _regions(G, K, capacity):
    """the launcher's rule, restated: (regions, ids per region)"""
    vunits, m = (G + 63) // 64 * K, 64
    while m > 1 and vunits < 64 * m:
        m >>= 1
    return m, (capacity // m) & ~7


def _check_rows(pk, ln, ref, rln, ld, u16, G, K):
    """the equalities of a complete fill: starts, alignment, lengths, the ids at row_start, the fill mark, no overlap, one region per row"""
    ev = 8 if u16 else 4
    rows = K * G
    lnh, st, buf = ln.reshape(-1).cpu().numpy(), pk.row_start[:rows].cpu().numpy(), _host(pk.buf, u16)
    assert int(pk.status()) == 0
    assert (st >= 0).all() and (st % ev == 0).all(), "every row placed, from a 16-byte boundary"
    assert np.array_equal(lnh, rln), "lengths are the oracle's"
    n = np.clip(rln, 0, ld)
    size = (n + ev - 1) // ev * ev
    assert int(pk.used()) == int(size.sum())
    order = np.argsort(st, kind="stable")
    ends = st[order] + size[order]
    assert (st[order][1:] >= ends[:-1]).all(), "rows overlap"
    assert ends.max() <= pk.capacity
    m, rc = _regions(G, K, pk.capacity)
    assert (st // rc == (st + size - 1) // rc).all() and (st // rc < m).all(), "a row lies inside one region"
    cols = np.arange(ld)[None, :]
    for r0 in range(0, rows, 8192):                       # (in slices: [rows, ld] index arrays of int64 are large)
        r1 = min(rows, r0 + 8192)
        got = buf[np.minimum(st[r0:r1, None] + cols, buf.size - 1)]
        inside = cols < n[r0:r1, None]
        assert np.array_equal(np.where(inside, got, 0), np.where(inside, ref[r0:r1, :ld], 0)), f"packed ids of rows {r0}..{r1} are not the oracle's"


def _slab_equals_oracle(ids, ref, u16):
    got = _host(ids.reshape(-1, ids.shape[-1]), u16)
    assert np.array_equal(got.astype(np.int32), ref), "slab is not the oracle's"


# ------------------------------------------------------------------------------------------------ 1. the default route
@pytest.mark.parametrize("name", ["er", "mix"])
@pytest.mark.parametrize("u16,slab,K", [(True, False, 8), (False, True, 3), (True, True, 1), (False, False, 1)])
def test_config5_rows_are_packed_by_the_bit_matrix_walk(name, u16, slab, K):
    """Config-5 shaped batches (20,480 graphs of 10-256 nodes, max_len 600) on the default route: sent_blane_kernel<W=4> packs the
    rows itself (fused; on the parent commit the C call answered GTOK_E_UNSUPPORTED and fused was False).  K = 8: 2,560 pairs on
    2,048 resident waves, so pairs come from the ticket counters too.  Capacity by bench.py's rule: total x 1.04 + 4096."""
    b, coo = _corpus(name)
    epoch0 = 2
    ref, rln = _oracle_epochs(name, epoch0, K)
    ev = 8 if u16 else 4
    pk = gtok.ops.PackedRows(K * G5, int(_need(rln, LD, ev) * 1.04) + 4096, u16, DEV)
    pk.buf.fill_(0x2B2B)
    ids, ln = gtok.ops.sent(b, MAXN, MAX_LEN, seed=SEED, epoch=epoch0, ld=LD, epochs=K, u16=u16, packed=pk, slab=slab)
    assert pk.fused is True, "the walk itself packs config-5 rows"
    assert gtok.ops.last_sent_kernel().startswith("sent_blane_kernel<W=4>"), gtok.ops.last_sent_kernel()
    assert (ids is None) == (not slab) and tuple(ln.shape) == ((K, G5) if K > 1 else (G5,))
    _check_rows(pk, ln, ref, rln, LD, u16, G5, K)
    plain, pln = gtok.ops.sent(b, MAXN, MAX_LEN, seed=SEED, epoch=epoch0, ld=LD, epochs=K, u16=u16)
    _slab_equals_oracle(plain, ref, u16)
    assert torch.equal(pln, ln)
    stt = torch.zeros(1, dtype=torch.int32, device=DEV)
    back = gtok.ops.unpack_rows_at(pk.buf, pk.row_start, ln.reshape(-1), LD, PAD, status=stt, u16=u16)
    assert torch.equal(back, plain.reshape(-1, LD)) and int(stt.item()) == 0
    if slab:
        assert torch.equal(ids, plain), "the slab written beside the packed rows"


# ------------------------------------------------------------------------------------------------ 2. the other instantiations
def _one_direction_er(G, seed, lo, hi, p_lo, p_hi):
    d = gtok.synth.er_batch(G, seed=seed, min_nodes=lo, max_nodes=hi, min_sparsity=p_lo, max_sparsity=p_hi)
    nptr = np.concatenate([[0], np.cumsum(d["node_counts"])])
    eg = np.repeat(np.arange(G), d["edge_counts"])
    deg = np.bincount(nptr[eg] + d["src"], minlength=nptr[-1]) + np.bincount(nptr[eg] + d["dst"], minlength=nptr[-1])
    return d, int(deg.max())


@pytest.mark.parametrize("W,lo,hi,p_lo,p_hi,narrow,u16,slab,with_query", [
    (1, 10, 64, 0.02, 0.08, True, True, False, False),
    (1, 10, 64, 0.3, 0.5, False, False, True, False),
    (2, 65, 128, 0.005, 0.03, True, False, False, False),
    (2, 65, 128, 0.1, 0.2, False, True, True, False),
    (2, 65, 128, 0.1, 0.2, False, True, False, True),
    (1, 10, 64, 0.02, 0.08, True, False, True, True),
])
def test_w1_and_w2_instantiations_pack_with_both_counter_widths(W, lo, hi, p_lo, p_hi, narrow, u16, slab, with_query):
    """One-direction ER graphs of <= 64 and of 65-128 nodes (not simple-symmetric lists: the molecule kernel does not take them),
    3,000 graphs x 8 epochs = 24,000 walks; closure degrees <= 15 (4 counter planes) and above (8).  With `query` tails the three
    query ids are part of the packed row."""
    G, K, epoch0, max_len = 3000, 8, 1, 400
    d, maxdeg = _one_direction_er(G, 100 * W + int(narrow), lo, hi, p_lo, p_hi)
    assert (maxdeg <= 15) == narrow, maxdeg
    batch, coo = both(d, False)
    assert not (batch.flags & gtok._lib.CSR_SIMPLE_SYMMETRIC)
    b = batch.to(DEV)
    ld = 416
    q = None
    if with_query:
        rng = np.random.default_rng(5)
        q = np.stack([rng.integers(0, d["node_counts"]), rng.integers(0, d["node_counts"])], 1).astype(np.int32)
    refs = [orc.sent(coo, 128, max_len, SEED, epoch0 + e, ld=ld, query=q, nthreads=8) for e in range(K)]
    ref, rln = np.concatenate([r for r, _ in refs]), np.concatenate([l for _, l in refs])
    if not narrow:
        assert (rln == max_len + (3 if with_query else 0)).any(), "the dense graphs' rows are cut at max_len"
    pk = gtok.ops.PackedRows(K * G, int(_need(rln, ld, 8 if u16 else 4) * 1.04) + 4096, u16, DEV)
    qt = None if q is None else torch.from_numpy(q)
    ids, ln = gtok.ops.sent(b, 128, max_len, seed=SEED, epoch=epoch0, ld=ld, epochs=K, u16=u16, packed=pk, slab=slab, query=qt)
    assert pk.fused is True and gtok.ops.last_sent_kernel() == f"sent_blane_kernel<W={W}>", gtok.ops.last_sent_kernel()
    assert (b.adj_max_degree <= 15) == narrow
    _check_rows(pk, ln, ref, rln, ld, u16, G, K)
    if with_query:      # the tail: [6 + nodes, 6 + u, 6 + v] behind the trail, inside the packed row
        st, buf = pk.row_start[:G].cpu().numpy(), _host(pk.buf, u16)
        tail = np.stack([buf[st + rln[:G] - 3 + j] for j in range(3)], 1).astype(np.int64)
        assert np.array_equal(tail, np.stack([6 + d["node_counts"], 6 + q[:, 0], 6 + q[:, 1]], 1))
    plain, pln = gtok.ops.sent(b, 128, max_len, seed=SEED, epoch=epoch0, ld=ld, epochs=K, u16=u16, query=qt)
    _slab_equals_oracle(plain, ref, u16)
    back = gtok.ops.unpack_rows_at(pk.buf, pk.row_start, ln.reshape(-1), ld, PAD, u16=u16)
    assert torch.equal(back, plain.reshape(-1, ld)) and torch.equal(pln, ln)
    if slab:
        assert torch.equal(ids, plain)


# ------------------------------------------------------------------------------------------------ 3. too small a buffer
@pytest.mark.parametrize("u16,slab", [(True, True), (False, False)])
def test_half_the_capacity_skips_whole_units_and_touches_nothing_else(u16, slab):
    name, K, epoch0 = "er", 3, 2
    b, coo = _corpus(name)
    ref, rln = _oracle_epochs(name, epoch0, K)
    ev = 8 if u16 else 4
    need = _need(rln, LD, ev)
    cap = need // 2 // 8 * 8
    pk = gtok.ops.PackedRows(K * G5, cap, u16, DEV)
    assert pk.capacity == cap
    GUARD = 0x7777
    big = torch.full((cap + 8192,), GUARD, dtype=pk.buf.dtype, device=DEV)
    pk.buf = big[:cap]
    ids, ln = gtok.ops.sent(b, MAXN, MAX_LEN, seed=SEED, epoch=epoch0, ld=LD, epochs=K, u16=u16, packed=pk, slab=slab)
    assert pk.fused is True and int(pk.status()) == 2
    assert int(pk.used()) == need, "the fill marks count what did not fit as well"
    assert np.array_equal(ln.reshape(-1).cpu().numpy(), rln), "len keeps the true lengths"
    st = pk.row_start[:K * G5].cpu().numpy()
    n = np.clip(rln, 0, LD)
    size = (n + ev - 1) // ev * ev
    kept = st >= 0
    assert kept.any() and (~kept).any() and (st[~kept] == -1).all()
    assert (st[kept] % ev == 0).all() and (st[kept] + size[kept] <= cap).all(), "a kept row ends inside the buffer"
    m, rc = _regions(G5, K, cap)
    assert (st[kept] // rc == (st[kept] + size[kept] - 1) // rc).all()
    allbuf = _host(big, u16)
    assert (allbuf[cap:] == GUARD).all(), "written past capacity"
    cover = np.zeros(cap + 1, np.int64)
    np.add.at(cover, st[kept], 1)
    np.add.at(cover, st[kept] + size[kept], -1)
    cover = np.cumsum(cover)[:cap]
    assert cover.max() == 1, "rows overlap"
    assert (allbuf[:cap][cover == 0] == GUARD).all(), "the gaps between the rows are untouched"
    cols = np.arange(LD)[None, :]
    rows = np.nonzero(kept)[0]
    for r0 in range(0, rows.size, 8192):
        rr = rows[r0:r0 + 8192]
        got = allbuf[st[rr, None] + np.minimum(cols, size[rr, None] - 1)]
        inside = cols < n[rr, None]
        assert np.array_equal(np.where(inside, got, 0), np.where(inside, ref[rr], 0)), "a kept row is the oracle's"
    stt = torch.zeros(1, dtype=torch.int32, device=DEV)
    back = gtok.ops.unpack_rows_at(pk.buf, pk.row_start, ln.reshape(-1), LD, PAD, status=stt, u16=u16)
    bh = _host(back, u16).astype(np.int32)
    assert int(stt.item()) == 2 and np.array_equal(bh[kept], ref[kept]) and (bh[~kept] == PAD).all()
    if slab:
        _slab_equals_oracle(ids, ref, u16)


# ------------------------------------------------------------------------------------------------ 4. what is refused, and how
def _c_call(b, p, ids, ld, ln, buf, cap, start, state):
    cs = b.c_struct()
    rc = gtok._lib.lib().gtok_sent_packed(ctypes.byref(cs), ctypes.byref(p), ids, ld, ln.data_ptr(), buf, cap, start.data_ptr(), state.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def _params(flags, max_num_nodes=MAXN, max_len=MAX_LEN, K=1):
    return gtok._lib.GtokSentParams(max_num_nodes, 0, 0, 0, max_len, 0, PAD, flags, SEED, 2, 0, None, K, 0)


def test_c_abi_accepts_config5_and_refuses_small_8_bit_and_wide_rows_before_writing(monkeypatch):
    U16, NO_PAD, U8 = gtok._lib.SENT_U16, gtok._lib.SENT_NO_PAD, gtok._lib.SENT_PACK_U8
    b, coo = _corpus("er")
    gtok.ops.sent(b, MAXN, MAX_LEN, seed=SEED, epoch=2, ld=LD, u16=True)            # builds the bit-matrix mirror and the lane order
    assert b.adj_rows is not None
    ref, rln = _oracle("er", 2)
    cap = int(_need(rln, LD, 8) * 1.04) + 4096
    GUARD = 0x3C3C

    def fresh(rows, ld):
        return (torch.full((cap + 64,), GUARD, dtype=torch.int16, device=DEV), torch.empty((rows, ld), dtype=torch.int16, device=DEV),
                torch.empty(rows, dtype=torch.int32, device=DEV), torch.full((rows,), -7, dtype=torch.int64, device=DEV),
                torch.zeros(gtok.ops.PACK_STATE_WORDS, dtype=torch.int64, device=DEV))

    def untouched(buf, start, state):
        return bool((buf == GUARD).all()) and bool((start == -7).all()) and not bool(state.any())

    # accepted: the batch of case 1 - and what it wrote is the oracle's
    buf, ids, ln, start, state = fresh(G5, LD)
    assert _c_call(b, _params(U16 | NO_PAD), ids.data_ptr(), LD, ln, buf.data_ptr(), cap, start, state) == 0
    assert int(state[0]) == 0 and bool((buf[cap:] == GUARD).all()) and np.array_equal(ln.cpu().numpy(), rln)
    back = gtok.ops.unpack_rows_at(buf[:cap], start, ln, LD, PAD, u16=True)
    assert np.array_equal(_host(back, True).astype(np.int32), ref)
    # (b) 8-bit rows: position ids reach 6 + 255 here
    buf, ids, ln, start, state = fresh(G5, LD)
    assert _c_call(b, _params(U16 | NO_PAD | U8), ids.data_ptr(), LD, ln, buf.data_ptr(), cap, start, state) == E_UNSUPPORTED
    assert untouched(buf, start, state)
    # (c) ld = 2048 at 16 bits: a row's 16-byte pieces are counted in 8 bits - the two-call route takes it, so not TOO_LARGE
    wide = torch.empty((G5, 2048), dtype=torch.int16, device=DEV)
    assert _c_call(b, _params(U16 | NO_PAD), wide.data_ptr(), 2048, ln, buf.data_ptr(), cap, start, state) == E_UNSUPPORTED
    assert untouched(buf, start, state)
    assert _c_call(b, _params(U16 | NO_PAD), wide.data_ptr(), 2040, ln, buf.data_ptr(), cap, start, state) == 0       # the widest row it takes
    del wide
    # bad arguments
    buf, ids, ln, start, state = fresh(G5, LD)
    assert _c_call(b, _params(U16 | NO_PAD), ids.data_ptr(), LD, ln, buf.data_ptr() + 2, cap, start, state) == E_INVAL
    assert _c_call(b, _params(U16 | NO_PAD), ids.data_ptr() + 2, LD, ln, buf.data_ptr(), cap, start, state) == E_INVAL
    assert _c_call(b, _params(U16 | NO_PAD), ids.data_ptr(), 604, ln, buf.data_ptr(), cap, start, state) == E_INVAL      # ld % 8
    assert _c_call(b, _params(U16 | NO_PAD), ids.data_ptr(), LD, ln, None, cap, start, state) == E_INVAL
    assert _c_call(b, _params(U16 | NO_PAD), ids.data_ptr(), LD, ln, buf.data_ptr(), -1, start, state) == E_INVAL
    assert untouched(buf, start, state)
    i32 = torch.empty((G5, 612), dtype=torch.int32, device=DEV)
    b32 = torch.full((cap,), GUARD, dtype=torch.int32, device=DEV)
    assert _c_call(b, _params(NO_PAD), i32.data_ptr(), 612, ln, b32.data_ptr(), cap, start, state) == 0                  # ld % 4 at 32 bits
    assert _c_call(b, _params(NO_PAD), i32.data_ptr(), 610, ln, b32.data_ptr(), cap, start, state) == E_INVAL
    del i32, b32
    # (a) 300 graphs pinned to the kernel: too few pairs for regions to mean anything
    monkeypatch.setenv("GTOK_SENT_KERNEL", "blane")
    d = gtok.synth.er_batch(300, seed=89, min_nodes=10, max_nodes=60)
    small, scoo = both(d, False)
    sb = small.to(DEV)
    for K in (1, 3):
        full, fln = gtok.ops.sent(sb, 60, 512, seed=SEED, epoch=2, ld=LD, epochs=K, u16=True)
        assert gtok.ops.last_sent_kernel().startswith("sent_blane_kernel") and sb.adj_rows is not None
        buf, ids, ln, start, state = fresh(K * 300, LD)
        assert _c_call(sb, _params(U16 | NO_PAD, 60, 512, K), ids.data_ptr(), LD, ln, buf.data_ptr(), cap, start, state) == E_UNSUPPORTED
        assert untouched(buf, start, state)


def test_ops_sent_falls_back_for_small_8_bit_and_wide_rows(monkeypatch):
    b, coo = _corpus("er")
    ref, rln = _oracle("er", 2)
    cols = np.arange(LD)[None, :]
    inside = cols < np.clip(rln, 0, LD)[:, None]
    # (c) ld = 2048: the two-call route, rows in dataset order
    pk = gtok.ops.PackedRows(G5, int(_need(rln, 2048, 8) * 1.04) + 4096, True, DEV)
    ids, ln = gtok.ops.sent(b, MAXN, MAX_LEN, seed=SEED, epoch=2, ld=2048, u16=True, packed=pk, slab=False)
    assert pk.fused is False and gtok.ops.last_sent_kernel().startswith("sent_blane_kernel<W=4>") and int(pk.status()) == 0
    assert np.array_equal(ln.cpu().numpy(), rln) and bool((pk.row_start[1:G5] > pk.row_start[:G5 - 1]).all())
    back = _host(gtok.ops.unpack_rows_at(pk.buf, pk.row_start, ln, 2048, PAD, u16=True), True).astype(np.int32)
    assert np.array_equal(back[:, :LD], ref) and (back[:, LD:] == PAD).all()
    # (b) 8-bit rows: graphs of up to 200 nodes keep every id below 256 - the rows as bytes, from gtok_pack_rows_scan
    d = gtok.synth.er_batch_device(G5, DEV, seed=6, min_nodes=10, max_nodes=200)
    batch, coo2 = both(d, False)
    b2 = batch.to(DEV)
    ref2, rln2 = orc.sent(coo2, 200, MAX_LEN, SEED, 0, ld=LD, nthreads=8)
    assert ref2.max() < 256
    pk8 = gtok.ops.PackedRows(G5, int(_need(rln2, LD, 16) * 1.04) + 4096, True, DEV, elem_bytes=1)
    _, ln2 = gtok.ops.sent(b2, 200, MAX_LEN, seed=SEED, epoch=0, ld=LD, u16=True, packed=pk8, slab=False)
    assert pk8.fused is False and gtok.ops.last_sent_kernel().startswith("sent_blane_kernel") and int(pk8.status()) == 0
    assert np.array_equal(ln2.cpu().numpy(), rln2)
    st, buf = pk8.row_start[:G5].cpu().numpy(), pk8.buf.cpu().numpy()
    assert (st >= 0).all() and (st % 16 == 0).all() and buf.dtype == np.uint8
    got = buf[np.minimum(st[:, None] + cols, buf.size - 1)]
    in2 = cols < np.clip(rln2, 0, LD)[:, None]
    assert np.array_equal(np.where(in2, got, 0), np.where(in2, ref2, 0))
    #     ... and where an id >= 256 exists (sparse graphs of 252-256 nodes, rows long enough to visit every node): an error
    d3 = gtok.synth.er_batch_device(G5, DEV, seed=7, min_nodes=252, max_nodes=256, min_sparsity=0.004, max_sparsity=0.008)
    b3 = both(d3, False)[0].to(DEV)
    pk8b = gtok.ops.PackedRows(G5, G5 * 1600, True, DEV, elem_bytes=1)
    with pytest.raises(gtok.GtokError, match="does not fit 8 bits"):
        gtok.ops.sent(b3, MAXN, 2000, seed=SEED, epoch=0, ld=2000, u16=True, packed=pk8b, slab=False)
    assert pk8b.fused is False
    del pk8b
    # (a) 300 graphs pinned to the kernel
    monkeypatch.setenv("GTOK_SENT_KERNEL", "blane")
    d = gtok.synth.er_batch(300, seed=89, min_nodes=10, max_nodes=60)
    small, scoo = both(d, False)
    sb = small.to(DEV)
    rs, ls = orc.sent(scoo, 60, 512, SEED, 2, ld=LD)
    pks = gtok.ops.PackedRows(300, 300 * LD, True, DEV)
    ids, ln = gtok.ops.sent(sb, 60, 512, seed=SEED, epoch=2, ld=LD, u16=True, packed=pks)
    assert pks.fused is False and gtok.ops.last_sent_kernel().startswith("sent_blane_kernel") and int(pks.status()) == 0
    assert bool((pks.row_start[1:300] > pks.row_start[:299]).all())
    assert np.array_equal(_host(gtok.ops.unpack_rows_at(pks.buf, pks.row_start, ln, LD, PAD, u16=True), True).astype(np.int32), rs)
    assert np.array_equal(ln.cpu().numpy(), ls)


# ------------------------------------------------------------------------------------------------ 5. hipGraph
def test_captured_in_a_hip_graph_and_replayed_twice():
    name, K, epoch0 = "mix", 3, 2
    b, coo = _corpus(name)
    ref, rln = _oracle_epochs(name, epoch0, K)
    pk = gtok.ops.PackedRows(K * G5, int(_need(rln, LD, 8) * 1.04) + 4096, True, DEV)
    kw = dict(seed=SEED, epoch=epoch0, ld=LD, epochs=K, u16=True, packed=pk, slab=False)
    gtok.ops.sent(b, MAXN, MAX_LEN, **kw)                           # warm-up: mirror, lane order, staging scratch
    assert pk.fused is True
    torch.cuda.synchronize()
    holder = {}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        holder["ln"] = gtok.ops.sent(b, MAXN, MAX_LEN, **kw)[1]
    assert pk.fused is True
    for rep in range(2):
        pk.buf.fill_(0x1111); pk.row_start.fill_(-9); holder["ln"].fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        _check_rows(pk, holder["ln"], ref, rln, LD, True, G5, K)


# ------------------------------------------------------------------------------------------------ 6. the exchange, the torch op
def test_gather_tokens_and_the_torch_op_on_rows_packed_by_this_kernel():
    import socket
    import torch.distributed as tdist
    name, epoch0 = "er", 2
    b, coo = _corpus(name)
    ref, rln = _oracle(name, epoch0)
    cap = int(_need(rln, LD, 8) * 1.04) + 4096
    pk = gtok.ops.PackedRows(G5, cap, True, DEV)
    _, ln = gtok.ops.sent(b, MAXN, MAX_LEN, seed=SEED, epoch=epoch0, ld=LD, u16=True, packed=pk, slab=False)
    assert pk.fused is True and int(pk.status()) == 0
    plain, pln = gtok.ops.sent(b, MAXN, MAX_LEN, seed=SEED, epoch=epoch0, ld=LD, u16=True)
    _slab_equals_oracle(plain, ref, True)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    tdist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        st = {}
        g_ids, g_ln = gtok.dist.gather_tokens(None, ln, G5, PAD, force=True, compact=True, packed=pk, ld=LD, stats=st)
        p_ids, p_ln = gtok.dist.gather_tokens(plain, pln, G5, PAD, force=True)
        (a_buf, a_start), a_ln = gtok.dist.gather_tokens(None, ln, G5, PAD, force=True, compact=True, packed=pk, ld=LD, as_packed=True)
    finally:
        tdist.destroy_process_group()
    assert int(st["status"]) == 0
    assert torch.equal(g_ids[:G5], p_ids[:G5]) and torch.equal(g_ln[:G5], p_ln[:G5])
    assert np.array_equal(_host(g_ids[:G5], True).astype(np.int32), ref) and np.array_equal(g_ln[:G5].cpu().numpy(), rln)
    idx = torch.randperm(G5, generator=torch.Generator().manual_seed(2))[:500].to(DEV)
    lmax = int(pln[idx].max())
    X, A = gtok.ops.collate_packed(a_buf, a_start[:G5], a_ln[:G5], LD, idx, PAD, lmax)
    rX, rA = gtok.ops.collate_packed(plain, None, pln, LD, idx, PAD, lmax)
    assert torch.equal(X, rX) and torch.equal(A, rA)
    # torch.ops.gtok.sent_packed on the same tensors
    args = (b.node_ptr, b.edge_ptr, b.rowptr, b.col, None, None, None, b.max_nodes, b.max_edges, MAXN, MAX_LEN, LD, SEED, epoch0, 1, False, 0, 0,
            False, PAD, 0, True, cap)
    tln, tpacked, tstart, tstate = torch.ops.gtok.sent_packed(*args)
    assert gtok.ops.last_sent_kernel().startswith("sent_blane_kernel<W=4>")
    assert tstate.tolist() == [_need(rln, LD, 8), 0] and np.array_equal(tln.cpu().numpy(), rln)
    assert not bool((tstart[1:] > tstart[:-1]).all()), "rows in completion order: the walk packed them (the two-call route packs in dataset order)"
    assert torch.equal(torch.ops.gtok.unpack_rows_at(tpacked, tstart, tln, LD, PAD, 0, 0, True), plain)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode() as mode:
        fk = [mode.from_tensor(a) if isinstance(a, torch.Tensor) else a for a in args]
        f = torch.ops.gtok.sent_packed(*fk)
    real = (tln, tpacked, tstart, tstate)
    assert [tuple(t.shape) for t in f] == [tuple(t.shape) for t in real] and [t.dtype for t in f] == [t.dtype for t in real]
