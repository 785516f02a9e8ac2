"""Packed rows at ONE byte per id (ABI v8) on the GPU: gtok_pack_rows* / gtok_unpack_rows* / gtok_collate_* with elem_bytes 1,
the walk that packs 8-bit rows itself (gtok_sent_packed + GTOK_SENT_PACK_U8), the torch ops and the one-rank exchange.
Expected values come from the CPU oracle (orc.sent, orc.row_offsets) and numpy: the 8-bit packed form is row r's
n_r = min(len[r], ld) ids as the bytes row_ptr[r] .. row_ptr[r] + n_r of the buffer - stated here, the oracle's pack_rows
knows 2 and 4 bytes."""
import ctypes
import os

import numpy as np
import pytest
import torch

from _util import both, gtok, orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ZKW = dict(labeled=True, num_node_types=9, num_edge_types=4, remap_zinc=True)
TOO_WIDE = "an id does not fit 8 bits: use 16-bit packed rows"
GUARD = 0xA5


def _zinc_dev(G, seed):
    d = gtok.synth.zinc_like(G, seed=seed)
    coo = orc.Coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], d["x"], d["edge_attr"])
    b = gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], d["x"], d["edge_attr"]).to(DEV)
    return d, coo, b


def _u(t):
    """int16 storage of a 16-bit slab -> the ids it holds (unsigned); int32 as it is"""
    a = t.cpu().numpy()
    return a.view(np.uint16).astype(np.int32) if a.dtype == np.int16 else a


def _rows_at(buf, start, n, ld):
    """the first n[r] bytes from start[r] of every row, zeros behind them -> int32 [rows, ld]"""
    cols = np.arange(ld)[None, :]
    got = buf[np.minimum(np.maximum(start, 0)[:, None] + cols, buf.size - 1)].astype(np.int32)
    return np.where(cols < n[:, None], got, 0)


def _inside(ref, n):
    return np.where(np.arange(ref.shape[1])[None, :] < n[:, None], ref, 0)


def _slabs(ref):
    """(int32 slab, 16-bit slab) on the device of the oracle's rows"""
    return torch.from_numpy(ref.astype(np.int32)).to(DEV), torch.from_numpy(ref.astype(np.uint16).view(np.int16)).to(DEV)


def _random_rows(rows=3001, ld=176, seed=3, junk=True):
    """ids 0..255 (255 present), lengths 0..ld with 0, 1, 15, 16, 17 and ld present; behind a row's end the slab holds ids that do
    NOT fit a byte - a packer must not look at them"""
    rng = np.random.default_rng(seed)
    ln = rng.integers(0, ld + 1, rows).astype(np.int32)
    ln[:6] = (0, 1, 15, 16, 17, ld)
    ids = rng.integers(0, 256, (rows, ld)).astype(np.int32)
    ids[5, ::7] = 255
    if junk:
        ids[np.arange(ld)[None, :] >= ln[:, None]] = 0x1234
    return ids, ln


def _pack_c(kind, src, ln, ld, align, capacity, tail=4096):
    """the C ABI on a buffer of the test's own: `capacity` bytes to pack into, `tail` guard bytes behind them -> (bytes, row_ptr, status)"""
    L = gtok._lib.lib()
    rows = int(ln.numel())
    buf = torch.full((capacity + tail,), GUARD, dtype=torch.uint8, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    if kind == "scan":
        ptr = torch.empty(rows + 1, dtype=torch.int64, device=DEV)
        rc = L.gtok_pack_rows_scan(src.data_ptr(), src.element_size(), ld, ln.data_ptr(), rows, align, 1, buf.data_ptr(), capacity,
                                   ptr.data_ptr(), status.data_ptr(), st)
    else:
        ptr = gtok.ops.row_offsets(ln, ld, align)
        fn = L.gtok_pack_rows_u16 if src.element_size() == 2 else L.gtok_pack_rows
        rc = fn(src.data_ptr(), ld, ln.data_ptr(), rows, ptr.data_ptr(), 1, buf.data_ptr(), capacity, status.data_ptr(), st)
    assert rc == 0, (kind, rc)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), ptr.cpu().numpy(), int(status.item())


def _corpora():
    d = gtok.synth.zinc_like(30016, seed=77)
    _, coo = both(d)
    ref, rln = orc.sent(coo, 37, 1024, 5, 2, ld=176, **ZKW)
    rnd, rnd_ln = _random_rows()
    return (("zinc", ref, rln), ("random", rnd, rnd_ln))


# ---------------------------------------------------------------------------------------------------- 1. pack
@pytest.mark.parametrize("align", [16, 1])
def test_pack_rows_at_one_byte_per_id(align):
    ld = 176
    for name, ref, rln in _corpora():
        n = np.clip(rln, 0, ld)
        want_ptr = orc.row_offsets(rln, ld, align)
        total = int(want_ptr[-1])
        want = _inside(ref, n)
        assert want.max() <= 255
        ln = torch.from_numpy(rln).to(DEV)
        for src in _slabs(ref):
            what = (name, align, src.dtype)
            two = None
            for kind in ("rows", "scan"):
                buf, ptr, st = _pack_c(kind, src, ln, ld, align, total)
                assert st == 0 and np.array_equal(ptr, want_ptr), what + (kind,)
                assert np.array_equal(_rows_at(buf[:total], ptr[:-1], n, ld), want), what + (kind,)
                assert (buf[total:] == GUARD).all(), what + (kind, "guard")
                if align == 1:                       # packed tightly: the buffer IS the rows' ids back to back
                    assert np.array_equal(buf[:total].astype(np.int32), ref[np.arange(ld)[None, :] < n[:, None]]), what + (kind,)
                # the one-pass route writes what the two calls write, row for row (bytes between rows are nobody's)
                if two is None:
                    two = _rows_at(buf[:total], ptr[:-1], n, ld)
                else:
                    assert np.array_equal(_rows_at(buf[:total], ptr[:-1], n, ld), two), what
            # the ops: uint8 storage, 16-id alignment by default
            fn = gtok.ops.pack_rows_u16 if src.dtype == torch.int16 else gtok.ops.pack_rows
            packed, ptr = fn(src, ln, elem_bytes=1, align=align)
            assert packed.dtype == torch.uint8 and np.array_equal(ptr.cpu().numpy(), want_ptr)
            assert np.array_equal(_rows_at(packed.cpu().numpy(), want_ptr[:-1], n, ld), want), what
            packed, ptr, status = gtok.ops.pack_rows_scan(src, ln, 1, (total + 15) // 16 * 16, align=align)
            assert packed.dtype == torch.uint8 and int(status.item()) == 0 and np.array_equal(ptr.cpu().numpy(), want_ptr)
            assert np.array_equal(_rows_at(packed.cpu().numpy(), want_ptr[:-1], n, ld), want), what
        if align == 16:
            p16, ptr16 = gtok.ops.pack_rows(_slabs(ref)[0], ln, elem_bytes=1)            # the default alignment of 8-bit rows
            assert np.array_equal(ptr16.cpu().numpy(), want_ptr)
            pc, pptr = gtok.ops.pack_rows(_slabs(ref)[0], ln, elem_bytes=1, capacity=total + 160)
            assert np.array_equal(pptr.cpu().numpy(), want_ptr) and pc.numel() == total + 160


# ---------------------------------------------------------------------------------------------------- 2. status bits
def test_pack_rows_status_bits_at_one_byte_per_id():
    ld = 176
    ref, rln = _random_rows(junk=False)
    n = np.clip(rln, 0, ld)
    ln = torch.from_numpy(rln).to(DEV)
    wide = ref.copy()
    r = int(np.nonzero(n >= 17)[0][100])
    wide[r, n[r] - 1] = 256                                            # one id that does not fit, in one row
    for align in (16, 1):
        ptr = orc.row_offsets(rln, ld, align)
        total = int(ptr[-1])
        for src, wsrc in zip(_slabs(ref), _slabs(wide)):
            for kind in ("rows", "scan"):
                assert _pack_c(kind, wsrc, ln, ld, align, total)[2] == 1, (align, src.dtype, kind)
            fn = gtok.ops.pack_rows_u16 if src.dtype == torch.int16 else gtok.ops.pack_rows
            for extra in (dict(), dict(capacity=total + 16)):           # two calls / the one-pass route
                with pytest.raises(gtok.GtokError, match="does not fit 8 bits"):
                    fn(wsrc, ln, elem_bytes=1, align=align, **extra)
                assert int(fn(wsrc, ln, elem_bytes=1, align=align, check_status=False, **extra)[2].item()) == 1
            # half the capacity: bit 1, the rows that fit are intact, the others are written nowhere
            cap = total // 2 // 16 * 16
            fits = ptr[:-1] + n <= cap
            assert 0 < fits.sum() < fits.size
            for kind in ("rows", "scan"):
                buf, got_ptr, st = _pack_c(kind, src, ln, ld, align, cap)
                assert st == 2 and np.array_equal(got_ptr, ptr), (align, src.dtype, kind)
                got = _rows_at(buf[:cap], ptr[:-1], n, ld)
                assert np.array_equal(got[fits], _inside(ref, n)[fits])
                last = int((ptr[:-1] + (n + align - 1) // align * align)[fits].max())
                assert (buf[last:] == GUARD).all(), (align, src.dtype, kind, "a skipped row was written")
            with pytest.raises(gtok.GtokError, match="too small"):
                fn(src, ln, elem_bytes=1, align=align, capacity=cap)


# ---------------------------------------------------------------------------------------------------- 3. readers
def test_readers_of_8_bit_packed_rows():
    ld, pad = 176, 5
    for name, ref, rln in _corpora():
        rows = rln.size
        n = np.clip(rln, 0, ld)
        ln = torch.from_numpy(rln).to(DEV)
        ids32, ids16 = _slabs(ref)
        padded = np.where(np.arange(ld)[None, :] < n[:, None], ref, pad).astype(np.int32)
        for align in (16, 1):
            packed, ptr = gtok.ops.pack_rows_u16(ids16, ln, elem_bytes=1, align=align)
            assert packed.dtype == torch.uint8
            st = torch.zeros(1, dtype=torch.int32, device=DEV)
            out = gtok.ops.unpack_rows(packed, ptr, ln, ld, pad, status=st)
            assert out.dtype == torch.int32 and np.array_equal(out.cpu().numpy(), padded) and int(st.item()) == 0, (name, align)
            assert torch.equal(out, gtok.ops.unpack_rows(ids16, None, ln, ld, pad))       # == the same call over the slab
            out16 = gtok.ops.unpack_rows(packed, ptr, ln, ld, pad, u16=True)
            assert out16.dtype == torch.int16 and np.array_equal(_u(out16), padded), (name, align)
            at = gtok.ops.unpack_rows_at(packed, ptr[:-1].contiguous(), ln, ld, pad, status=st)
            at16 = gtok.ops.unpack_rows_at(packed, ptr[:-1].contiguous(), ln, ld, pad, status=st, u16=True)
            assert np.array_equal(at.cpu().numpy(), padded) and np.array_equal(_u(at16), padded) and int(st.item()) == 0, (name, align)
        # segments: what an all-gather of two ranks' buffers gives (rows [0, per) and [per, 2 per), each buffer `stride` bytes)
        per = (rows + 1) // 2
        lnp = np.concatenate([rln, np.zeros(2 * per - rows, np.int32)])
        refp = np.concatenate([ref, np.zeros((2 * per - rows, ld), ref.dtype)])
        stride = max(int(orc.row_offsets(lnp[:per], ld, 16)[-1]), int(orc.row_offsets(lnp[per:], ld, 16)[-1])) + 64
        segs = []
        for s in range(2):
            p, _, stt = gtok.ops.pack_rows_scan(_slabs(refp[s * per:(s + 1) * per])[1], torch.from_numpy(lnp[s * per:(s + 1) * per]).to(DEV), 1, stride)
            assert int(stt.item()) == 0 and p.numel() == stride
            segs.append(p)
        cat = torch.cat(segs)
        all_ln = torch.from_numpy(lnp).to(DEV)
        all_ptr = gtok.ops.row_offsets(all_ln, ld, 16)
        assert np.array_equal(all_ptr.cpu().numpy(), orc.row_offsets(lnp, ld, 16))
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        for u16 in (False, True):
            seg = gtok.ops.unpack_rows(cat, all_ptr, all_ln, ld, pad, segment_rows=per, segment_stride=stride, status=st, u16=u16)
            assert np.array_equal(_u(seg)[:rows], padded) and int(st.item()) == 0, (name, "segments", u16)
        starts = torch.from_numpy(np.concatenate([orc.row_offsets(lnp[:per], ld, 16)[:-1], orc.row_offsets(lnp[per:], ld, 16)[:-1]])).to(DEV)
        seg = gtok.ops.unpack_rows_at(cat, starts, all_ln, ld, pad, segment_rows=per, segment_stride=stride, status=st, u16=True)
        assert np.array_equal(_u(seg)[:rows], padded) and int(st.item()) == 0
        # the collates over the 8-bit buffer == the same calls over the slab
        packed, ptr = gtok.ops.pack_rows(ids32, ln, elem_bytes=1)
        order = torch.randperm(rows, generator=torch.Generator().manual_seed(1)).to(DEV)
        idx = order[:333]
        lmax = int(ln[idx].max())
        X, A = gtok.ops.collate_packed(packed, ptr, ln, ld, idx, pad, lmax)
        rX, rA = gtok.ops.collate_packed(ids16, None, ln, ld, idx, pad, lmax)
        want = padded[idx.cpu().numpy()][:, :lmax]
        assert torch.equal(X, rX) and torch.equal(A, rA) and np.array_equal(X.cpu().numpy(), want)
        y = torch.arange(rows, dtype=torch.float32, device=DEV) * 0.25
        X, A, Y = gtok.ops.collate_batch(packed, ptr, ln, ld, idx.cpu().numpy(), pad, lmax, y)
        assert torch.equal(X, rX) and torch.equal(A, rA) and torch.equal(Y, y[idx])
        Xa, Aa, lm, off = gtok.ops.collate_epoch(packed, ptr, ln, ld, order, 128, pad)
        Xs, As, lms, offs = gtok.ops.collate_epoch(ids16, None, ln, ld, order, 128, pad)
        assert lm == lms and off == offs and torch.equal(Xa, Xs) and torch.equal(Aa, As)


# ---------------------------------------------------------------------------------------------------- 4. the walk packs
def _check_packed8(pk, ln, ld, status=0):
    """rows start on multiples of 16 ids, do not overlap, the fill marks add up to their sizes, the regions fill evenly"""
    ln = ln.reshape(-1).cpu().numpy()
    st = pk.row_start[:ln.size].cpu().numpy()
    n = np.clip(ln, 0, ld)
    assert pk.buf.dtype == torch.uint8 and (st >= 0).all() and (st % 16 == 0).all()
    size = (n + 15) // 16 * 16
    order = np.argsort(st, kind="stable")
    ends = st[order] + size[order]
    assert (st[order][1:] >= ends[:-1]).all(), "rows overlap"
    assert int(pk.used()) == int(size.sum()) and int(pk.status()) == status and ends.max() <= pk.capacity
    if pk.fused:
        fill = pk.state[gtok.ops.PACK_STATE_FILL::gtok.ops.PACK_STATE_STRIDE].cpu().numpy()
        fill = fill[fill > 0]
        assert fill.size in (1, 2, 4, 8, 16, 32, 64) and (fill % 16 == 0).all() and fill.max() <= 1.06 * fill.mean(), (fill.size, fill.max() / fill.mean())
    return st, n


@pytest.mark.parametrize("slab", [True, False])
@pytest.mark.parametrize("K", [1, 3])
def test_the_walk_packs_8_bit_rows_itself(K, slab):
    G, ld = 30016, 176
    d, coo, b = _zinc_dev(G, seed=77)
    pk = gtok.ops.PackedRows(K * G, K * G * 112, True, DEV, elem_bytes=1)
    guard = torch.full((4096,), GUARD, dtype=torch.uint8, device=DEV)
    ids, ln = gtok.ops.sent(b, 37, 1024, seed=5, epoch=2, ld=ld, pad=False, epochs=K, u16=True, packed=pk, slab=slab, **ZKW)
    assert pk.fused and gtok.ops.last_sent_kernel() == "sent_lane_kernel" and (ids is None) == (not slab)
    st, n = _check_packed8(pk, ln, ld)
    buf = pk.buf.cpu().numpy()
    lnv = ln.reshape(K, G).cpu().numpy()
    for e in sorted({0, K - 1}):                                        # the oracle's rows, first and last epoch
        ref, rln = orc.sent(coo, 37, 1024, 5, 2 + e, ld=ld, **ZKW)
        assert np.array_equal(lnv[e], rln)
        assert np.array_equal(_rows_at(buf, st.reshape(K, G)[e], np.clip(rln, 0, ld), ld), _inside(ref, np.clip(rln, 0, ld))), e
    # the bytes between a row's end and the next 16-byte boundary are zeros
    r = np.arange(0, K * G, 97)
    for i in r:
        assert not buf[st[i] + n[i]:st[i] + (n[i] + 15) // 16 * 16].any()
    full, fln = gtok.ops.sent(b, 37, 1024, seed=5, epoch=2, ld=ld, epochs=K, u16=True, **ZKW)      # the padded 16-bit launch
    stt = torch.zeros(1, dtype=torch.int32, device=DEV)
    back = gtok.ops.unpack_rows_at(pk.buf, pk.row_start, ln.reshape(-1), ld, 5, status=stt, u16=True)
    assert torch.equal(back, full.reshape(-1, ld)) and int(stt.item()) == 0 and torch.equal(fln, ln)
    if slab:
        m = torch.arange(ld, device=DEV)[None, :] < ln.reshape(-1, 1)
        assert torch.equal(torch.where(m, ids.reshape(-1, ld), 0), torch.where(m, full.reshape(-1, ld), 0))
    assert bool((guard == GUARD).all())


def test_the_walk_packs_8_bit_rows_from_reused_staging_rows():
    G, ld, K = 30016, 176, 28                              # 13,132 (unit, epoch) pairs on 4,096 resident waves: every staging row is reused
    d, coo, b = _zinc_dev(G, seed=81)
    pk = gtok.ops.PackedRows(K * G, K * G * 108, True, DEV, elem_bytes=1)
    none, ln = gtok.ops.sent(b, 37, 1024, seed=6, epoch=1, ld=ld, epochs=K, u16=True, packed=pk, slab=False, **ZKW)
    assert none is None and pk.fused and tuple(ln.shape) == (K, G)
    st, n = _check_packed8(pk, ln, ld)
    back = _u(gtok.ops.unpack_rows_at(pk.buf, pk.row_start, ln.reshape(-1), ld, 5, u16=True)).reshape(K, G, ld)
    for e in (0, K - 1):
        ref, rln = orc.sent(coo, 37, 1024, 6, 1 + e, ld=ld, **ZKW)
        assert np.array_equal(back[e], ref) and np.array_equal(ln[e].cpu().numpy(), rln), e


def test_the_walk_packs_8_bit_rows_of_a_slab_too_narrow_for_some_rows():
    """ld below the longest rows: a packed row holds the first ld ids, out_len keeps the true length"""
    G, ld = 30016, 80
    d, coo, b = _zinc_dev(G, seed=86)
    ref, rln = orc.sent(coo, 37, 1024, 4, 1, ld=ld, **ZKW)
    assert int((rln > ld).sum()) == 19970 and int((rln <= ld).sum()) == 10046
    n = np.clip(rln, 0, ld)
    for slab in (True, False):
        pk = gtok.ops.PackedRows(G, G * 80, True, DEV, elem_bytes=1)
        ids, ln = gtok.ops.sent(b, 37, 1024, seed=4, epoch=1, ld=ld, u16=True, packed=pk, slab=slab, **ZKW)
        assert pk.fused and np.array_equal(ln.cpu().numpy(), rln)
        st, _ = _check_packed8(pk, ln, ld)
        assert np.array_equal(_rows_at(pk.buf.cpu().numpy(), st, n, ld), _inside(ref, n))
        assert np.array_equal(_u(gtok.ops.unpack_rows_at(pk.buf, pk.row_start, ln, ld, 5, u16=True)), ref)
        if slab:
            assert np.array_equal(_u(ids), ref)


# ---------------------------------------------------------------------------------------------------- 5. too small a buffer
def test_the_walk_skips_whole_units_when_the_8_bit_buffer_is_too_small():
    G, ld = 30016, 176
    d, coo, b = _zinc_dev(G, seed=78)
    ref, rln = orc.sent(coo, 37, 1024, 1, 0, ld=ld, **ZKW)
    n = np.clip(rln, 0, ld)
    need = int(((n + 15) // 16 * 16).sum())
    cap = need // 2 // 16 * 16
    pk = gtok.ops.PackedRows(G, cap, True, DEV, elem_bytes=1)
    assert pk.capacity == cap and pk.buf.numel() == cap
    guard = torch.full((4096,), GUARD, dtype=torch.uint8, device=DEV)
    pk.buf.fill_(0x77)
    _, ln = gtok.ops.sent(b, 37, 1024, seed=1, ld=ld, pad=False, u16=True, packed=pk, **ZKW)
    assert pk.fused and int(pk.status()) == 2 and int(pk.used()) == need and np.array_equal(ln.cpu().numpy(), rln)
    st = pk.row_start[:G].cpu().numpy()
    assert (st < 0).any() and (st >= 0).any()
    assert ((st < 0) | ((st % 16 == 0) & (st + (n + 15) // 16 * 16 <= cap))).all(), "a row that was written lies inside the buffer"
    kept = st >= 0
    assert np.array_equal(_rows_at(pk.buf.cpu().numpy(), st, n, ld)[kept], _inside(ref, n)[kept])
    # whole units: the rows of a 64-graph unit are kept or skipped together (units are 64 consecutive graphs of the sorted layout)
    sb = b.lane_sorted
    assert sb is not None and sb.graph_ids is not None and sb.unit_ptr is not None
    order, up = sb.graph_ids.cpu().numpy(), sb.unit_ptr.cpu().numpy()
    for u in range(0, up.size - 1, 7):
        k = kept[order[up[u]:up[u + 1]]]
        assert k.all() or not k.any(), u
    stt = torch.zeros(1, dtype=torch.int32, device=DEV)
    back = _u(gtok.ops.unpack_rows_at(pk.buf, pk.row_start, ln, ld, 5, status=stt, u16=True))
    assert np.array_equal(back[kept], ref[kept]) and (back[~kept] == 5).all() and int(stt.item()) == 2
    assert bool((guard == GUARD).all())


# ---------------------------------------------------------------------------------------------------- 6. ids that do not fit
def test_ids_that_do_not_fit_a_byte_raise_the_flag_and_ops_sent_raises():
    G, ld = 30016, 176
    d, coo, b = _zinc_dev(G, seed=77)
    for remap, rows_with in ((False, G), (True, 13560)):
        kw = dict(ZKW, remap_zinc=remap)
        ref, rln = orc.sent(coo, 250, 1024, 5, 2, ld=ld, **kw)
        top = _inside(ref, np.clip(rln, 0, ld)).max(1)
        assert int(top.max()) == (305 if remap else 283) and int((top > 255).sum()) == rows_with
        pk = gtok.ops.PackedRows(G, G * 112, True, DEV, elem_bytes=1)
        with pytest.raises(gtok.GtokError, match=TOO_WIDE):
            gtok.ops.sent(b, 250, 1024, seed=5, epoch=2, ld=ld, pad=False, u16=True, packed=pk, **kw)
        assert pk.fused and int(pk.state[0].item()) & 1 and int(pk.status().item()) & 1
        with pytest.raises(gtok.GtokError, match=TOO_WIDE):
            pk.verify()
        # check_ids=False leaves the verdict to the caller; the 16-bit buffer of the same launch is fine
        _, ln = gtok.ops.sent(b, 250, 1024, seed=5, epoch=2, ld=ld, pad=False, u16=True, packed=pk, slab=False, check_ids=False, **kw)
        assert int(pk.status().item()) == 1 and np.array_equal(ln.cpu().numpy(), rln)
        pk16 = gtok.ops.PackedRows(G, G * 112, True, DEV)
        _, ln = gtok.ops.sent(b, 250, 1024, seed=5, epoch=2, ld=ld, pad=False, u16=True, packed=pk16, slab=False, **kw)
        assert int(pk16.status().item()) == 0
        assert np.array_equal(_u(gtok.ops.unpack_rows_at(pk16.buf, pk16.row_start, ln, ld, 5, u16=True)), ref)
    # un-remapped with max_num_nodes = 200: the largest id is 233 - the id space is a property of the data, and these fit
    kw = dict(ZKW, remap_zinc=False)
    ref, rln = orc.sent(coo, 200, 1024, 5, 2, ld=ld, **kw)
    n = np.clip(rln, 0, ld)
    assert int(_inside(ref, n).max()) == 233
    pk = gtok.ops.PackedRows(G, G * 112, True, DEV, elem_bytes=1)
    _, ln = gtok.ops.sent(b, 200, 1024, seed=5, epoch=2, ld=ld, u16=True, packed=pk, slab=False, **kw)
    st, _ = _check_packed8(pk, ln, ld)
    assert pk.fused and np.array_equal(_rows_at(pk.buf.cpu().numpy(), st, n, ld), _inside(ref, n)) and np.array_equal(ln.cpu().numpy(), rln)
    # an 8-bit buffer goes with the 16-bit walk only
    with pytest.raises(ValueError):
        gtok.ops.sent(b, 37, 1024, seed=5, ld=ld, u16=False, packed=pk, **ZKW)


# ---------------------------------------------------------------------------------------------------- 7. the fallback
def test_8_bit_rows_fall_back_to_the_one_pass_pack_where_another_kernel_walks():
    G, ld = 3000, 176                                          # too few walks for the lane kernel: sent_reg_kernel
    d, coo, b = _zinc_dev(G, seed=79)
    ref, rln = orc.sent(coo, 37, 1024, 3, 0, ld=ld, **ZKW)
    n = np.clip(rln, 0, ld)
    ptr = orc.row_offsets(rln, ld, 16)
    for slab in (True, False):
        pk = gtok.ops.PackedRows(G, G * 120, True, DEV, elem_bytes=1)
        ids, ln = gtok.ops.sent(b, 37, 1024, seed=3, ld=ld, pad=False, u16=True, packed=pk, slab=slab, **ZKW)
        assert pk.fused is False and gtok.ops.last_sent_kernel() == "sent_reg_kernel" and np.array_equal(ln.cpu().numpy(), rln)
        st, _ = _check_packed8(pk, ln, ld)
        assert np.array_equal(st, ptr[:-1])                                             # dataset order, 16-id alignment
        assert np.array_equal(_rows_at(pk.buf.cpu().numpy(), st, n, ld), _inside(ref, n))
    # undersized: the rows the scan skipped are marked -1, as the fused route marks them; nothing of them is in the buffer
    cap = int(ptr[-1]) // 2 // 16 * 16
    pk = gtok.ops.PackedRows(G, cap, True, DEV, elem_bytes=1)
    pk.buf.fill_(GUARD)
    _, ln = gtok.ops.sent(b, 37, 1024, seed=3, ld=ld, u16=True, packed=pk, slab=False, **ZKW)
    skip = ptr[:-1] + n > cap
    st = pk.row_start[:G].cpu().numpy()
    assert pk.fused is False and int(pk.status()) == 2 and skip.any() and (~skip).any()
    assert (st[skip] == -1).all() and np.array_equal(st[~skip], ptr[:-1][~skip])
    buf = pk.buf.cpu().numpy()
    assert np.array_equal(_rows_at(buf, st, n, ld)[~skip], _inside(ref, n)[~skip])
    assert (buf[int((ptr[:-1] + (n + 15) // 16 * 16)[~skip].max()):] == GUARD).all()
    back = _u(gtok.ops.unpack_rows_at(pk.buf, pk.row_start, ln, ld, 5, u16=True))
    assert np.array_equal(back[~skip], ref[~skip]) and (back[skip] == 5).all()
    # an id that does not fit comes out of this route too
    pk = gtok.ops.PackedRows(G, G * 120, True, DEV, elem_bytes=1)
    with pytest.raises(gtok.GtokError, match=TOO_WIDE):
        gtok.ops.sent(b, 250, 1024, seed=3, ld=ld, u16=True, packed=pk, **dict(ZKW, remap_zinc=False))
    assert pk.fused is False and int(pk.status()) & 1


# ---------------------------------------------------------------------------------------------------- 8. the C ABI alone
def test_sent_pack_u8_through_the_c_abi_alone():
    G, ld = 30016, 176
    d, coo, b = _zinc_dev(G, seed=80)
    gtok.ops.sent(b, 37, 1024, seed=0, ld=ld, u16=True, **ZKW)            # builds the reordered copy
    sb = b.lane_sorted
    assert sb is not None
    L, lb = gtok._lib.lib(), gtok._lib
    assert L.gtok_version() == 8
    cs = sb.c_struct()
    pk = gtok.ops.PackedRows(2 * G, 2 * G * 112, True, DEV, elem_bytes=1)
    ids = torch.empty((2, G, ld), dtype=torch.int16, device=DEV)
    ln = torch.empty((2, G), dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    flags = lb.SENT_U16 | lb.SENT_NO_PAD | lb.SENT_PACK_U8
    p = lb.GtokSentParams(37, 1, 9, 4, 1024, 1, 5, flags, 9, 0, 0, None, 2, 0)
    pk.state.zero_()
    rc = L.gtok_sent_packed(ctypes.byref(cs), ctypes.byref(p), ids.data_ptr(), ld, ln.data_ptr(), pk.buf.data_ptr(), pk.capacity,
                            pk.row_start.data_ptr(), pk.state.data_ptr(), st)
    assert rc == 0
    pk.fused = True
    starts, n = _check_packed8(pk, ln, ld)
    buf = pk.buf.cpu().numpy()
    for e in range(2):
        ref, rln = orc.sent(coo, 37, 1024, 9, e, ld=ld, **ZKW)
        assert np.array_equal(ln[e].cpu().numpy(), rln)
        assert np.array_equal(_rows_at(buf, starts.reshape(2, G)[e], np.clip(rln, 0, ld), ld), _inside(ref, np.clip(rln, 0, ld))), e
    # what is refused, before anything is launched: the flag with gtok_sent; without GTOK_SENT_U16; ld not a multiple of 16; a misaligned buffer
    before = (pk.buf.clone(), pk.row_start.clone(), pk.state.clone())
    assert L.gtok_sent(ctypes.byref(cs), ctypes.byref(p), ids.data_ptr(), ld, ln.data_ptr(), st) == -1
    args = lambda pp, **o: [ctypes.byref(cs), ctypes.byref(pp), ids.data_ptr(), o.get("ld", ld), ln.data_ptr(), o.get("buf", pk.buf.data_ptr()),
                            pk.capacity, pk.row_start.data_ptr(), pk.state.data_ptr(), st]
    p32 = lb.GtokSentParams(37, 1, 9, 4, 1024, 1, 5, lb.SENT_NO_PAD | lb.SENT_PACK_U8, 9, 0, 0, None, 2, 0)
    assert L.gtok_sent_packed(*args(p32)) == -1
    assert L.gtok_sent_packed(*args(p, ld=168)) == -1
    assert L.gtok_sent_packed(*args(p, buf=pk.buf.data_ptr() + 8)) == -1
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, (pk.buf, pk.row_start, pk.state)))
    # a batch another kernel walks: GTOK_E_UNSUPPORTED, nothing written
    d2, coo2, b2 = _zinc_dev(3000, seed=79)
    ids2, ln2 = gtok.ops.sent(b2, 37, 1024, seed=3, ld=ld, u16=True, **ZKW)
    assert gtok.ops.last_sent_kernel() == "sent_reg_kernel"
    cs2 = b2.c_struct()
    p1 = lb.GtokSentParams(37, 1, 9, 4, 1024, 1, 5, lb.SENT_U16 | lb.SENT_PACK_U8, 0, 0, 0, None, 1, 0)
    pk2 = gtok.ops.PackedRows(3000, 3000 * 120, True, DEV, elem_bytes=1)
    pk2.row_start.fill_(-7); pk2.buf.fill_(GUARD); pk2.state.zero_()
    rc = L.gtok_sent_packed(ctypes.byref(cs2), ctypes.byref(p1), ids2.data_ptr(), ld, ln2.data_ptr(), pk2.buf.data_ptr(), pk2.capacity,
                            pk2.row_start.data_ptr(), pk2.state.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == lb.E_UNSUPPORTED == -6 and bool((pk2.row_start == -7).all()) and not bool(pk2.state.any()) and bool((pk2.buf == GUARD).all())


# ---------------------------------------------------------------------------------------------------- 9. the torch ops
def test_sent_packed_torch_op_at_one_byte_per_id_real_and_fake():
    for G, K, fused_kernel in ((30016, 2, True), (700, 3, False)):
        d = gtok.synth.zinc_like(G, seed=56)
        batch, coo = both(d)
        b = batch.to(DEV)
        args = (b.node_ptr, b.edge_ptr, b.rowptr, b.col, b.nattr, b.eattr, None, b.max_nodes, b.max_edges, 37, 1024, 176, 9, 2, K, True, 9, 4,
                True, 5, 0, True, K * G * 112 + 5)
        ln, packed, start, state = torch.ops.gtok.sent_packed(*args, elem_bytes=1)
        assert packed.dtype == torch.uint8 and packed.numel() == (K * G * 112 + 5 + 15) // 16 * 16
        assert tuple(ln.shape) == (K * G,) and tuple(start.shape) == (K * G,) and state.tolist()[1] == 0
        assert (gtok.ops.last_sent_kernel() == "sent_lane_kernel") == fused_kernel
        assert state.tolist()[0] == int(((ln.clamp(0, 176) + 15) // 16 * 16).sum())
        slab = _u(torch.ops.gtok.unpack_rows_at(packed, start, ln, 176, 5, 0, 0, True))
        buf, stn = packed.cpu().numpy(), start.cpu().numpy()
        for e in range(K):
            ref, rln = orc.sent(coo, 37, 1024, 9, 2 + e, ld=176, **ZKW)
            n = np.clip(rln, 0, 176)
            assert np.array_equal(ln[e * G:(e + 1) * G].cpu().numpy(), rln) and np.array_equal(slab[e * G:(e + 1) * G], ref), e
            assert np.array_equal(_rows_at(buf, stn[e * G:(e + 1) * G], n, 176), _inside(ref, n)), e
        idx = torch.arange(0, K * G, 11, device=DEV)
        X, A = torch.ops.gtok.collate_packed(packed, start, ln, 176, idx, 5, 176)
        want = np.where(np.arange(176)[None, :] < ln[idx].cpu().numpy()[:, None], slab[idx.cpu().numpy()], 5)
        assert np.array_equal(X.cpu().numpy(), want)
        from torch._subclasses.fake_tensor import FakeTensorMode
        with FakeTensorMode() as mode:
            fk = [mode.from_tensor(a) if isinstance(a, torch.Tensor) else a for a in args]
            f = torch.ops.gtok.sent_packed(*fk, elem_bytes=1)
            f2 = torch.ops.gtok.sent_packed(*fk)                       # what exists: positional calls, the slab's width
        real = (ln, packed, start, state)
        assert [tuple(t.shape) for t in f] == [tuple(t.shape) for t in real] and [t.dtype for t in f] == [t.dtype for t in real]
        assert f2[1].dtype == torch.int16 and f2[1].numel() == (K * G * 112 + 5 + 7) // 8 * 8


# ---------------------------------------------------------------------------------------------------- 10. a captured launch
def test_the_8_bit_pack_only_launch_captured_in_a_hip_graph_and_replayed():
    G, ld, K = 30016, 176, 4
    d, coo, b = _zinc_dev(G, seed=84)
    pk = gtok.ops.PackedRows(K * G, K * G * 108, True, DEV, elem_bytes=1)
    gtok.ops.sent(b, 37, 1024, seed=3, epoch=8, ld=ld, epochs=K, u16=True, packed=pk, slab=False, **ZKW)     # warm-up: layout, scratch
    torch.cuda.synchronize()
    holder = {}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        holder["ln"] = gtok.ops.sent(b, 37, 1024, seed=3, epoch=8, ld=ld, epochs=K, u16=True, packed=pk, slab=False, **ZKW)[1]
    refs = {e: orc.sent(coo, 37, 1024, 3, 8 + e, ld=ld, **ZKW) for e in (0, K - 1)}
    for rep in range(3):
        pk.buf.fill_(0x11); pk.row_start.fill_(-9); holder["ln"].fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert int(pk.status()) == 0
        back = _u(gtok.ops.unpack_rows_at(pk.buf, pk.row_start, holder["ln"].reshape(-1), ld, 5, u16=True)).reshape(K, G, ld)
        for e, (ref, rln) in refs.items():
            assert np.array_equal(back[e], ref) and np.array_equal(holder["ln"][e].cpu().numpy(), rln), (rep, e)


# ---------------------------------------------------------------------------------------------------- 11. the exchange
def test_one_rank_nccl_gather_at_one_byte_per_id():
    import socket
    import torch.distributed as tdist
    G, ld = 30001, 176
    d, coo, b = _zinc_dev(G, seed=92)
    ref, rln = orc.sent(coo, 37, 1024, 21, 3, ld=ld, **ZKW)
    ids32, ln = gtok.ops.sent(b, 37, 1024, 21, 3, ld=ld, **ZKW)
    ids16, _ = gtok.ops.sent(b, 37, 1024, 21, 3, ld=ld, u16=True, **ZKW)
    pk = gtok.ops.PackedRows(G, G * 112, True, DEV, elem_bytes=1)
    _, pln = gtok.ops.sent(b, 37, 1024, 21, 3, ld=ld, u16=True, packed=pk, slab=False, **ZKW)
    assert pk.fused and np.array_equal(pln.cpu().numpy(), rln)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    tdist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        sp, s8, s16 = {}, {}, {}
        p_ids, p_ln = gtok.dist.gather_tokens(ids32, ln, G, 5, force=True, stats=sp)
        p16, _ = gtok.dist.gather_tokens(ids16, ln, G, 5, force=True)
        assert np.array_equal(p_ids.cpu().numpy(), ref) and np.array_equal(p_ln.cpu().numpy(), rln)
        c_ids, c_ln = gtok.dist.gather_tokens(ids32, ln, G, 5, force=True, compact=True, elem_bytes=1, stats=s8)
        assert c_ids.data_ptr() != ids32.data_ptr() and torch.equal(c_ids, p_ids) and torch.equal(c_ln, p_ln) and s8["elem_bytes"] == 1
        u_ids, u_ln = gtok.dist.gather_tokens(ids16, ln, G, 5, force=True, compact=True, elem_bytes=1)
        assert u_ids.dtype == torch.int16 and torch.equal(u_ids, p16) and torch.equal(u_ln, p_ln)
        gtok.dist.gather_tokens(ids16, ln, G, 5, force=True, compact=True, elem_bytes=2, stats=s16)
        need8 = int(orc.row_offsets(rln, ld, 16)[-1])
        assert s8["capacity"] == need8 and s8["bytes_sent_per_rank"] == need8 + (G + 1) * 4
        assert s8["capacity"] * 1 < 0.56 * s16["capacity"] * 2                           # half the payload of the 16-bit rows, plus alignment
        k_ids, _ = gtok.dist.gather_tokens(ids32, ln, G, 5, force=True, compact=True, elem_bytes=1, capacity=need8 + 100, stats=s8)
        assert torch.equal(k_ids, p_ids) and int(s8["status"]) == 0 and s8["elem_bytes"] == 1
        # rows the walk packed itself, re-padded here or left packed
        sq = {}
        f_ids, f_ln = gtok.dist.gather_tokens(None, pln, G, 5, force=True, compact=True, packed=pk, ld=ld, stats=sq)
        assert f_ids.dtype == torch.int16 and torch.equal(f_ids, p16) and torch.equal(f_ln, p_ln) and sq["elem_bytes"] == 1 and int(sq["status"]) == 0
        assert sq["bytes_sent_per_rank"] == pk.capacity + G * 8 + (G + 1) * 4
        (g_buf, g_start), g_ln = gtok.dist.gather_tokens(ids16, pln, G, 5, force=True, compact=True, packed=pk, as_packed=True, stats=sq)
        assert g_buf.dtype == torch.uint8 and g_buf.data_ptr() != pk.buf.data_ptr() and sq["elem_bytes"] == 1 and sq["as_packed"]
        assert torch.equal(g_ln, p_ln) and torch.equal(gtok.ops.unpack_rows_at(g_buf, g_start, g_ln, ld, 5, u16=True), p16)
        n = np.clip(rln, 0, ld)
        assert np.array_equal(_rows_at(g_buf.cpu().numpy(), g_start.cpu().numpy(), n, ld), _inside(ref, n))
        # an id that does not fit: the agreed verdict fails the call
        wide = ids32.clone()
        wide[7, 0] = 300
        with pytest.raises(gtok.GtokError, match=TOO_WIDE):
            gtok.dist.gather_tokens(wide, ln, G, 5, force=True, compact=True, elem_bytes=1, capacity=need8 + 100)
    finally:
        tdist.destroy_process_group()
