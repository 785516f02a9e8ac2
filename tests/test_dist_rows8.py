"""CPU, world_size 2 over gloo: the compact all-gather at ONE byte per id (dist.gather_tokens(..., elem_bytes=1) and the
pre-packed route with an 8-bit ops.PackedRows).  The 8-bit packed form is stated here in numpy (`_Rows8`: the oracle's
pack_rows knows 2 and 4 bytes); what is under test is the collective logic around it - capacities, segment strides and
overflow tests that count ids = bytes, rows that start on multiples of 16, and the verdict every rank agrees on."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from _util import both, gtok, orc

ALIGN = 16          # ids per 16 bytes at one byte per id


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _slab(ids):
    a = ids.numpy()
    return a.view(np.uint16).astype(np.int64) if a.dtype == np.int16 else a.astype(np.int64)


class _Rows8:
    """rows_impl for dist.gather_tokens on CPU tensors: the packed format at one byte per id, in numpy.  Row r's
    n_r = min(len[r], ld) ids are the bytes row_ptr[r] .. row_ptr[r] + n_r of a uint8 buffer; status bit 0: an id above 255,
    bit 1: a row that would end past `capacity` (skipped, nothing written)."""
    reads = []          # (first byte, one past the last byte, segment's first byte, segment's end) of every row a reader fetched

    @staticmethod
    def row_offsets(ln, ld, align=8):
        return torch.from_numpy(orc.row_offsets(ln.numpy(), ld, align))

    @staticmethod
    def pack_rows(ids, ln, row_ptr, elem_bytes=2, capacity=None, check_status=True, align=8):
        assert elem_bytes == 1 and align == ALIGN, (elem_bytes, align)
        src, n = _slab(ids), np.clip(ln.numpy(), 0, ids.shape[1])
        ptr = orc.row_offsets(ln.numpy(), ids.shape[1], align)
        if row_ptr is not None:
            assert np.array_equal(ptr, row_ptr.numpy())
        cap = int(ptr[-1]) if capacity is None else int(capacity)
        buf = np.full(max(cap, 1), 0xAB, np.uint8)
        st = 0
        for r in range(n.size):
            if ptr[r] + n[r] > cap:
                st |= 2
                continue
            if (src[r, :n[r]] > 255).any():
                st |= 1
            buf[ptr[r]:ptr[r] + n[r]] = src[r, :n[r]] & 255
        if check_status and st:
            raise ValueError(f"pack status {st}")
        out = (torch.from_numpy(buf), torch.from_numpy(ptr))
        return out if check_status else out + (torch.tensor([st], dtype=torch.int32),)

    pack_rows_u16 = pack_rows

    @classmethod
    def _read(cls, p, starts, n, ld, pad_id, segment_rows, segment_stride, status, u16):
        out = np.full((n.size, ld), pad_id, dtype=np.int32)
        for r in range(n.size):
            seg = r // segment_rows if segment_rows else 0
            lo, hi = seg * segment_stride, ((seg + 1) * segment_stride if segment_rows else p.size)
            if starts[r] < 0 or starts[r] + n[r] > hi - lo:
                if n[r] and status is not None:
                    status |= 2
                continue
            at = lo + starts[r]
            if n[r]:
                cls.reads.append((at, at + n[r], lo, hi))
            out[r, :n[r]] = p[at:at + n[r]]
        return torch.from_numpy(out.astype(np.uint16).view(np.int16)) if u16 else torch.from_numpy(out)

    @classmethod
    def unpack_rows(cls, packed, row_ptr, ln, ld, pad_id, segment_rows=0, segment_stride=0, status=None, u16=False):
        assert packed.dtype == torch.uint8
        ptr, n = row_ptr.numpy(), np.clip(ln.numpy(), 0, ld)
        rows = np.arange(n.size)
        first = (rows // segment_rows) * segment_rows if segment_rows else np.zeros_like(rows)
        return cls._read(packed.numpy(), ptr[:-1] - ptr[first], n, ld, pad_id, segment_rows, segment_stride, status, u16)

    @classmethod
    def unpack_rows_at(cls, packed, row_start, ln, ld, pad_id, segment_rows=0, segment_stride=0, status=None, u16=False):
        assert packed.dtype == torch.uint8
        return cls._read(packed.numpy(), row_start.numpy(), np.clip(ln.numpy(), 0, ld), ld, pad_id, segment_rows, segment_stride, status, u16)


def _prepacked8(ids, ln, capacity, seed, wide=False):
    """an 8-bit ops.PackedRows as the walk leaves it, filled by hand: rows in a scrambled order, each from a multiple of 16, in
    two regions of the buffer; rows that do not fit their region are marked -1 (status bit 1)"""
    rows, ld = ids.shape
    pk = gtok.ops.PackedRows(rows, capacity, True, "cpu", elem_bytes=1)
    assert pk.buf.dtype == torch.uint8 and pk.capacity % ALIGN == 0 and pk.elem_bytes == 1
    cap = pk.capacity
    half = cap // 2 // ALIGN * ALIGN
    buf = np.full(cap, 0xAB, np.uint8)
    start = np.full(rows, -1, np.int64)
    fill, st = [0, half], 0
    for i, r in enumerate(np.random.default_rng(seed).permutation(rows)):
        n = int(min(max(ln[r], 0), ld))
        reg = i & 1
        if fill[reg] + n > (reg + 1) * half:
            st |= 2
            continue
        buf[fill[reg]:fill[reg] + n] = ids[r, :n] & 255
        start[r] = fill[reg]
        fill[reg] += (n + ALIGN - 1) // ALIGN * ALIGN
    pk.buf.copy_(torch.from_numpy(buf))
    pk.row_start.copy_(torch.from_numpy(start))
    pk.state.zero_()
    pk.state[0] = st | (1 if wide else 0)
    return pk


def _worker(rank, world, port, G, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ld, per = 160, -(-G // world)
        d = gtok.synth.zinc_like(G, seed=77)
        _, coo = both(d)
        lo, hi = gtok.dist.block_bounds(G, world)[rank]          # G is odd: the last block is one row short
        kw = dict(labeled=True, num_node_types=9, num_edge_types=4, remap_zinc=True)
        ids, ln = orc.sent(coo.slice(lo, hi), 37, 1024, 11, 2, graph_base=lo, ld=ld, **kw)
        ref_ids, ref_ln = orc.sent(coo, 37, 1024, 11, 2, ld=ld, **kw)
        assert ref_ids[np.arange(ld)[None, :] < ref_ln[:, None]].max() < 256          # every id of this corpus fits a byte
        t_ids, t_ln = torch.from_numpy(ids), torch.from_numpy(ln)
        i16 = torch.from_numpy(ids.astype(np.uint16).view(np.int16))
        full = torch.from_numpy(ref_ids)
        full16 = torch.from_numpy(ref_ids.astype(np.uint16).view(np.int16))
        ok = True
        # ---- the rows of uneven shards come back in dataset order, from either slab; the payload counts one byte per id
        st = {}
        c_ids, c_ln = gtok.dist.gather_tokens(t_ids, t_ln, G, 5, compact=True, elem_bytes=1, rows_impl=_Rows8, stats=st)
        need = max(int(orc.row_offsets(ref_ln[r * per:(r + 1) * per], ld, ALIGN)[-1]) for r in range(world))
        ok = ok and torch.equal(c_ids, full) and np.array_equal(c_ln.numpy(), ref_ln) and st["elem_bytes"] == 1 and st["capacity"] == need \
            and st["bytes_sent_per_rank"] == need + (per + 1) * 4
        u_ids, u_ln = gtok.dist.gather_tokens(i16, t_ln, G, 5, compact=True, elem_bytes=1, rows_impl=_Rows8, stats=st)
        ok = ok and u_ids.dtype == torch.int16 and torch.equal(u_ids, full16) and np.array_equal(u_ln.numpy(), ref_ln)
        k_ids, _ = gtok.dist.gather_tokens(t_ids, t_ln, G, 5, compact=True, elem_bytes=1, capacity=need + 40, rows_impl=_Rows8, stats=st)
        ok = ok and torch.equal(k_ids, full) and int(st["status"]) == 0 and st["capacity"] == (need + 40 + 15) // 16 * 16
        # ---- rows the walk packed itself (scrambled order, explicit starts), re-padded or left packed
        cap = need + 64 * ALIGN
        pp = _prepacked8(ids.astype(np.int64), ln, cap, seed=rank)
        f_ids, f_ln = gtok.dist.gather_tokens(i16, t_ln, G, 5, compact=True, packed=pp, rows_impl=_Rows8, stats=st)
        ok = ok and f_ids.dtype == torch.int16 and torch.equal(f_ids, full16) and np.array_equal(f_ln.numpy(), ref_ln) and int(st["status"]) == 0 \
            and st["elem_bytes"] == 1 and st["prepacked"] and st["bytes_sent_per_rank"] == pp.capacity + per * 8 + (per + 1) * 4
        (g_buf, g_start), g_ln = gtok.dist.gather_tokens(None, t_ln, G, 5, compact=True, packed=pp, ld=ld, as_packed=True, rows_impl=_Rows8, stats=st)
        back = _Rows8.unpack_rows_at(g_buf, g_start, g_ln, ld, 5, u16=True)
        ok = ok and g_buf.dtype == torch.uint8 and g_buf.numel() == world * pp.capacity and st["as_packed"] and bool((g_start % ALIGN == 0).all()) \
            and torch.equal(back, full16) and np.array_equal(g_ln.numpy(), ref_ln)
        # ---- one rank overflows its capacity: its skipped rows are pad / (start -1, length 0) on BOTH ranks, nobody reads beyond a segment
        small = need // 2 // ALIGN * ALIGN
        _Rows8.reads.clear()
        st = {}
        s_ids, s_ln = gtok.dist.gather_tokens(t_ids, t_ln, G, 5, compact=True, elem_bytes=1, capacity=small, rows_impl=_Rows8, stats=st)
        all_ptr = np.concatenate([orc.row_offsets(ref_ln[r * per:(r + 1) * per], ld, ALIGN)[:-1] for r in range(world)])
        fits = all_ptr + np.clip(ref_ln, 0, ld) <= small
        ok = ok and int(st["status"]) == 2 and np.array_equal(s_ln.numpy(), ref_ln) and 0 < fits.sum() < G
        ok = ok and torch.equal(s_ids[torch.from_numpy(fits)], full[torch.from_numpy(fits)]) and bool((s_ids[torch.from_numpy(~fits)] == 5).all())
        ok = ok and len(_Rows8.reads) == int(fits.sum()) and all(l <= a and b <= h for a, b, l, h in _Rows8.reads)
        pp = _prepacked8(ids.astype(np.int64), ln, cap, seed=rank)          # (every rank passes a buffer of the same capacity)
        if rank == 1:
            dropped = np.arange(hi - lo) % 3 == 1                # rank 1's walk had to skip a third of its rows
            pp.row_start[torch.from_numpy(dropped)] = -1
            pp.state[0] = 2
        _Rows8.reads.clear()
        (g_buf, g_start), g_ln = gtok.dist.gather_tokens(None, t_ln, G, 5, compact=True, packed=pp, ld=ld, as_packed=True, rows_impl=_Rows8, stats=st)
        gone = np.zeros(G, bool)
        blo, bhi = gtok.dist.block_bounds(G, world)[1]
        gone[blo:bhi] = np.arange(bhi - blo) % 3 == 1
        gs, gl = g_start.numpy(), g_ln.numpy()
        ok = ok and int(st["status"]) == 2 and bool((gs[gone] == -1).all()) and bool((gl[gone] == 0).all()) and np.array_equal(gl[~gone], ref_ln[~gone])
        seg_end = (np.arange(G) // per + 1) * pp.capacity
        ok = ok and bool((gs[~gone] >= seg_end[~gone] - pp.capacity).all()) and bool((gs[~gone] + np.clip(gl[~gone], 0, ld) <= seg_end[~gone]).all())
        d_ids, d_ln = gtok.dist.gather_tokens(i16, t_ln, G, 5, compact=True, packed=pp, rows_impl=_Rows8, stats=st)
        keep = torch.from_numpy(~gone)
        ok = ok and int(st["status"]) == 2 and torch.equal(d_ids[keep], full16[keep]) and bool((d_ids[~keep] == 5).all()) \
            and all(l <= a and b <= h for a, b, l, h in _Rows8.reads)
        # ---- one rank holds an id >= 256: BOTH ranks raise, after the collectives, with the same message - whatever the capacity's origin
        wide = t_ids.clone()
        if rank == 1:
            wide[0, 0] = 256
        for extra in (dict(), dict(capacity=need + 40)):
            try:
                gtok.dist.gather_tokens(wide, t_ln, G, 5, compact=True, elem_bytes=1, rows_impl=_Rows8, **extra)
                ok = False
            except gtok.GtokError as e:
                ok = ok and "an id does not fit 8 bits: use 16-bit packed rows" in str(e)
        pw = _prepacked8(ids.astype(np.int64), ln, cap, seed=rank, wide=rank == 1)
        for extra in (dict(), dict(as_packed=True)):
            try:
                gtok.dist.gather_tokens(None, t_ln, G, 5, compact=True, packed=pw, ld=ld, rows_impl=_Rows8, **extra)
                ok = False
            except gtok.GtokError as e:
                ok = ok and "an id does not fit 8 bits: use 16-bit packed rows" in str(e)
        q.put((rank, bool(ok)))
    except Exception:                       # report instead of leaving the parent to time out
        import traceback
        traceback.print_exc()
        q.put((rank, False))
    finally:
        dist.destroy_process_group()


def test_two_rank_gather_at_one_byte_per_id():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    G = 101                                       # odd: the last block is short and gets padded for the gather
    procs = [ctx.Process(target=_worker, args=(r, 2, port, G, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res == [(0, True), (1, True)]


def test_abi_version_8_and_the_8_bit_packed_rows_object():
    assert gtok._lib.ABI_VERSION == 8 and gtok._lib.SENT_PACK_U8 == 8
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gtok.h")) as f:
        header = f.read()
    assert "#define GTOK_ABI_VERSION 8" in header and "#define GTOK_SENT_PACK_U8 8" in header
    pk = gtok.ops.PackedRows(10, 100, True, "cpu", elem_bytes=1)
    assert pk.buf.dtype == torch.uint8 and pk.capacity == 112 and pk.buf.numel() == 112
    old = gtok.ops.PackedRows(10, 100, True, "cpu")                       # (what exists: positional u16, the slab's width)
    assert old.buf.dtype == torch.int16 and old.capacity == 104 and gtok.ops.PackedRows(10, 100, False, "cpu").buf.dtype == torch.int32
    try:
        gtok.ops.PackedRows(10, 100, False, "cpu", elem_bytes=1)          # 8-bit rows come from the 16-bit walk
        assert False
    except ValueError:
        pass
    pk.state[0] = 1
    try:
        pk.verify()
        assert False
    except gtok.GtokError as e:
        assert "an id does not fit 8 bits: use 16-bit packed rows" in str(e)
