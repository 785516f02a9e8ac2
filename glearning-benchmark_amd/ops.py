"""Tensor-level entry points over the C ABI (include/gtok.h).

PyTorch is plumbing here: it owns the device buffers and the HIP stream the
kernels are enqueued on.  Every function raises if libgtok.so is missing or
the tensors are not on a GPU — there is no CPU path in the product.
"""
import ctypes
import os
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import GtokSentParams, GtokVocabTable, check, lib
from .csr import GraphBatch

SENT_SOS, SENT_RESET, SENT_LADJ, SENT_RADJ, SENT_EOS, SENT_PAD, SENT_IDX_OFFSET = 0, 1, 2, 3, 4, 5, 6
SENT_MAX_NODES = 512        # include/gtok.h: GTOK_MAX_NODES - the largest graph gtok_sent walks (sent_large: _lib.SENT_LARGE_MAX_NODES)

ZINC_ATOM_SYMBOLS = ("C", "N", "O", "F", "P", "S", "Cl", "Br", "I", "X")
ZINC_BOND_NAMES = ("unknown", "single", "double", "triple", "aromatic")


def _stream(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _need_gpu(t: torch.Tensor, what: str) -> None:
    if t.device.type != "cuda":
        raise _lib.GtokError(f"{what}: tensors must live on the GPU (got {t.device}); the tokenizer has no CPU path")


def _need(symbols, what: str) -> None:
    """Entry points that came without an ABI version step (_lib.*_SYMBOLS): a library loaded through GTOK_LIB may lack them."""
    if not all(hasattr(lib(), n) for n in symbols):
        raise _lib.GtokError(f"{_lib.LIB_PATH} has no {what}: it was built before they were added")


def _round4(v: int) -> int:
    return max(4, (int(v) + 3) // 4 * 4)


def _alloc_out(G: int, ld: int, device, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Fresh [G, ld] int32 slab + [G] lengths, or the caller's preallocated pair (`out`)."""
    if out is not None:
        ids, ln = out
        if ids.dtype != torch.int32 or ln.dtype != torch.int32 or tuple(ids.shape) != (G, ld) \
                or ln.numel() != G or not ids.is_contiguous() or ids.device != torch.device(device):
            raise ValueError("out must be (int32 [G, ld] contiguous, int32 [G]) on the batch's device")
        return ids, ln
    return (torch.empty((G, ld), dtype=torch.int32, device=device),
            torch.empty((G,), dtype=torch.int32, device=device))


# ------------------------------------------------------------------------------------------------
# LUT builders (vocab is an INPUT: SURVEY.md F5)
# ------------------------------------------------------------------------------------------------
def zinc_lut(vocab: Dict[str, int], num_node_ids: int) -> torch.Tensor:
    """int32 LUT for gtok_ibtt_zinc; a token absent from `vocab` maps to vocab['<pad>'] exactly as
    TokenDataset does (graph_data_loader/data_loader.py:482)."""
    pad = vocab["<pad>"]
    toks = ["<bos>", "<eos>", "<atom>", "<bond>", "<q>", "regression", "<p>"]
    toks += list(ZINC_ATOM_SYMBOLS) + list(ZINC_BOND_NAMES) + [str(i) for i in range(num_node_ids)]
    return torch.tensor([vocab.get(t, pad) for t in toks], dtype=torch.int32)


def synth_lut(vocab: Dict[str, int], num_node_ids: int) -> torch.Tensor:
    pad = vocab["<pad>"]
    toks = ["<bos>", "<e>", "<n>", "<q>", "<p>"] + [str(i) for i in range(num_node_ids)]
    return torch.tensor([vocab.get(t, pad) for t in toks], dtype=torch.int32)


# ------------------------------------------------------------------------------------------------
# tokenizers
# ------------------------------------------------------------------------------------------------
def ibtt_zinc(batch: GraphBatch, lut: torch.Tensor, max_len: int, pad_id: int,
              ld: Optional[int] = None, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """CSR -> IBTT molecular ids.  Returns (ids int32 [G, ld], len int32 [G])."""
    _need_gpu(batch.col, "ibtt_zinc")
    dev = batch.device
    lut = lut.to(dev, dtype=torch.int32).contiguous()
    if ld is None:
        ld = _round4(min(max_len, 4 + 2 * batch.max_nodes + 4 * batch.max_edges))
    ids, ln = _alloc_out(batch.num_graphs, ld, dev, out)
    pack8(batch)
    cs = batch.c_struct()
    check(lib().gtok_ibtt_zinc(ctypes.byref(cs), lut.data_ptr(), lut.numel(), max_len, pad_id,
                               ids.data_ptr(), ld, ln.data_ptr(), _stream(dev)), "gtok_ibtt_zinc")
    return ids, ln


def ibtt_synth(batch: GraphBatch, lut: torch.Tensor, query: Optional[torch.Tensor], max_len: int, pad_id: int,
               ld: Optional[int] = None, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """CSR -> graph-token grammar ids.  query: int32 [G,4] = (count, id0, id1, id2) or None."""
    _need_gpu(batch.col, "ibtt_synth")
    dev = batch.device
    lut = lut.to(dev, dtype=torch.int32).contiguous()
    if query is not None:
        query = query.to(dev, dtype=torch.int32).contiguous()
        if tuple(query.shape) != (batch.num_graphs, 4):
            raise ValueError("query must be [G, 4]")
    if ld is None:
        ld = _round4(min(max_len, 3 * batch.max_edges + batch.max_nodes + 7))
    ids, ln = _alloc_out(batch.num_graphs, ld, dev, out)
    cs = batch.c_struct()
    check(lib().gtok_ibtt_synth(ctypes.byref(cs), lut.data_ptr(), lut.numel(),
                                None if query is None else query.data_ptr(), max_len, pad_id,
                                ids.data_ptr(), ld, ln.data_ptr(), _stream(dev)), "gtok_ibtt_synth")
    return ids, ln


def sent_safe_ld(batch: GraphBatch, labeled: bool, max_len: int, with_query: bool = False) -> int:
    """Width no SENT row of this batch can exceed (length bound)."""
    n, e = batch.max_nodes, batch.max_edges
    bound = (2 + 7 * n + 2 * e) if labeled else (2 + 5 * n + e)
    # a multiple of 16 ids: every row then starts on a 64-byte boundary and the kernels' 64-byte store bursts are whole
    return (min(max_len, bound) + (3 if with_query else 0) + 15) // 16 * 16


def pack8(batch: GraphBatch) -> bool:
    """Give a device batch of small graphs its byte-packed rowptr / col mirror (gtok_csr_pack8; once per batch,
    kept on the batch object).  Returns whether the batch has one now.  A layout step like the CSR build: the
    lane-per-graph SENT kernel reads the mirror instead of the int32 arrays."""
    if batch.rowptr8 is not None:
        return True
    if os.environ.get("GTOK_NO_PACK8") == "1":      # tests: the lane kernel's int32 staging path (C-ABI callers without a mirror)
        return False
    if batch.col.device.type != "cuda" or batch.num_graphs == 0 or batch.max_edges > 255 or batch.max_nodes > 64 \
            or not (batch.flags & _lib.CSR_SIMPLE_SYMMETRIC):
        return False
    dev = batch.device
    r8 = torch.empty(batch.rowptr.numel() + 16, dtype=torch.uint8, device=dev)   # + slack: 16-byte vector loads of the
    c8 = torch.empty(batch.col.numel() + 16, dtype=torch.uint8, device=dev)      # last chunk may run past the end
    cs = batch.c_struct()
    check(lib().gtok_csr_pack8(ctypes.byref(cs), batch.rowptr.numel(), batch.col.numel(), r8.data_ptr(), c8.data_ptr(),
                               _stream(dev)), "gtok_csr_pack8")
    batch.rowptr8, batch.col8 = r8, c8
    return True


LANE_UNIT_LDS = 10224      # LDS bytes a unit of the reordered batch may need: 16 waves per CU stay resident (160 KB / 16, less the 16 bytes of the workgroup's ticket counter)


def csr_check(batch: GraphBatch) -> Dict[str, int]:
    """gtok_csr_check: verify on the device what GTOK_CSR_SIMPLE_SYMMETRIC claims and measure the batch maxima.  Returns
    dict(violations, max_degree, max_nodes, max_edges); one 32-byte read-back.  violations == 0 (and at least one entry)
    is what GraphBatch.flags |= CSR_SIMPLE_SYMMETRIC needs."""
    _need_gpu(batch.rowptr, "csr_check")
    dev = batch.device
    info = torch.empty(8, dtype=torch.int32, device=dev)
    cs = batch.c_struct()
    check(lib().gtok_csr_check(ctypes.byref(cs), info.data_ptr(), _stream(dev)), "gtok_csr_check")
    v = info.tolist()
    return dict(violations=v[0], max_degree=v[1], max_nodes=v[2], max_edges=v[3])


COO_STATUS_TEXT = {_lib.COO_BAD_ENDPOINT: "edge endpoint outside [0, num_nodes)",
                   _lib.COO_BAD_SLICES: "slices decrease or do not start at 0",
                   _lib.COO_BAD_TOTALS: "the slices' totals differ from num_nodes / num_entries",
                   _lib.COO_BAD_INDEX: "index outside [0, number of storage graphs)",
                   _lib.COO_SORT_TOO_LARGE: f"an unsorted graph has more than {_lib.COO_SORT_NODES} nodes (too large for the device sort)"}


class CooInputError(ValueError):
    """gtok_csr_from_coo found its input damaged: `status` holds the GTOK_COO_* bits of info[6]."""

    def __init__(self, status: int):
        self.status = int(status)
        super().__init__("csr_from_coo: " + "; ".join(t for b, t in COO_STATUS_TEXT.items() if self.status & b))


def _type_column(a, dev, what: str):
    """Column 0 of x / edge_attr ([n] or [n, k]); int64 device tensors are then read in place (with their stride), anything
    else is converted and uploaded the way from_coo_device converts it."""
    if a is None:
        return None
    t = torch.as_tensor(a)
    if t.dim() == 0 or t.dim() > 2:
        raise ValueError(f"{what} must be [n] or [n, k]")
    if t.dim() == 2:
        if t.shape[1] == 0:
            raise ValueError(f"{what} has no column")
        t = t[:, 0]
    return t


def _on_device(t, dev):
    """A type column as gtok_coo takes it: (int64 tensor on dev, element stride)."""
    if t is None:
        return None, 0
    if t.dtype != torch.int64 or t.device != dev or (t.numel() > 1 and t.stride(0) < 1):
        t = t.to(dev, dtype=torch.int64).contiguous()
    return t, max(1, int(t.stride(0)))


def _coo_prepare(src, dst, node_slices, edge_slices, x, edge_attr, indices, num_nodes, num_entries, device):
    """Argument checks and conversions of csr_from_coo (nothing is launched here): -> dict of device tensors and totals."""
    if device is None:
        device = src.device if torch.is_tensor(src) and src.device.type == "cuda" else "cuda"
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.GtokError(f"csr_from_coo: the build runs on the GPU (got device {dev}); the tokenizer has no CPU path")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    raw = {k: torch.as_tensor(v) for k, v in (("node_slices", node_slices), ("edge_slices", edge_slices))}
    for k, t in raw.items():
        if t.dim() != 1 or t.numel() < 1:
            raise ValueError(f"{k} must be a 1-D array of S + 1 offsets")
    if raw["node_slices"].numel() != raw["edge_slices"].numel():
        raise ValueError("node_slices and edge_slices differ in length")
    S = raw["node_slices"].numel() - 1
    s_t, d_t = torch.as_tensor(src), torch.as_tensor(dst)
    if s_t.dim() != 1 or d_t.dim() != 1 or s_t.numel() != d_t.numel():
        raise ValueError("src and dst must be 1-D and of one length (the two rows of edge_index)")
    idx = None
    if indices is not None:
        idx = torch.as_tensor(list(indices) if not torch.is_tensor(indices) and not isinstance(indices, np.ndarray) else indices)
        if idx.dim() != 1:
            raise ValueError("indices must be 1-D")
        if idx.numel() and (idx.dtype.is_floating_point or idx.dtype == torch.bool):
            raise ValueError("indices must be integers")
    G = S if idx is None else int(idx.numel())
    xa, ea = _type_column(x, dev, "x"), _type_column(edge_attr, dev, "edge_attr")
    if ea is not None and ea.numel() != s_t.numel():
        raise ValueError("edge_attr length does not match edge_index")
    host = raw["node_slices"].device.type == "cpu" and raw["edge_slices"].device.type == "cpu"
    if x is not None and host and xa.numel() != int(raw["node_slices"][-1]):
        raise ValueError("x length does not match node_slices")
    N, E = num_nodes, num_entries
    if idx is None:
        if E is None:
            E = s_t.numel()
        if N is None and xa is not None:
            N = xa.numel()
    if N is None or E is None:               # totals the inputs do not show: from host slices, else one read of two words
        ns, es = raw["node_slices"].to(torch.int64), raw["edge_slices"].to(torch.int64)
        if idx is not None:
            ii = idx.to(ns.device, torch.int64)
            inside = (ii >= 0) & (ii < S)                 # (an index outside the storage is the kernel's to report, counted as 0)
            ii = torch.where(inside, ii, 0)
            cnt = lambda sl: torch.where(inside, (sl[1:] - sl[:-1])[ii], 0).sum()
            tot = torch.stack([cnt(ns), cnt(es)]) if S else torch.zeros(2, dtype=torch.int64)
        else:
            tot = torch.stack([ns[-1] - ns[0], es[-1] - es[0]])
        tn, te = tot.tolist()
        N = tn if N is None else N
        E = te if E is None else E
    N, E = int(N), int(E)
    if N < 0 or E < 0:
        raise ValueError("num_nodes and num_entries must be >= 0")
    if N + G >= 2 ** 31:
        raise ValueError("batch too large for int32 node offsets; shard it")
    i64 = lambda t: t.reshape(-1).to(dev, dtype=torch.int64).contiguous()
    (xa, xs), (ea, eas) = _on_device(xa, dev), _on_device(ea, dev)
    return dict(dev=dev, G=G, S=S, N=N, E=E, src=i64(s_t), dst=i64(d_t), node_slices=i64(raw["node_slices"]),
                edge_slices=i64(raw["edge_slices"]), indices=None if idx is None else i64(idx), x=xa, x_stride=xs, ea=ea, ea_stride=eas)


def _coo_launch(p: dict, check_symmetric: bool):
    """gtok_csr_from_coo on the current stream of p's device: -> (outputs dict, info int32 [8]) with no host read."""
    dev, G, S, N, E = p["dev"], p["G"], p["S"], p["N"], p["E"]
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    o = dict(node_ptr=i32(G + 1), edge_ptr=torch.empty(G + 1, dtype=torch.int64, device=dev), rowptr=i32(N + G), col=i32(E), eorder=i32(E),
             nattr=None if p["x"] is None else torch.empty(N, dtype=torch.uint8, device=dev),
             eattr=None if p["ea"] is None else torch.empty(E, dtype=torch.uint8, device=dev), info=i32(8))
    L = lib()
    ws = torch.empty(max(16, int(L.gtok_csr_from_coo_workspace(G, S))), dtype=torch.uint8, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    cin = _lib.GtokCoo(G, S, N, E, ptr(p["node_slices"]), ptr(p["edge_slices"]), ptr(p["indices"]), ptr(p["src"]), ptr(p["dst"]),
                       ptr(p["x"]), p["x_stride"], ptr(p["ea"]), p["ea_stride"])
    cout = _lib.GtokCsrBuilt(*[ptr(o[n]) for n, _ in _lib.GtokCsrBuilt._fields_])
    check(L.gtok_csr_from_coo(ctypes.byref(cin), int(bool(check_symmetric)), ctypes.byref(cout), ws.data_ptr(), ws.numel(), _stream(dev)),
          "gtok_csr_from_coo")
    return o, o["info"]


def _coo_batch(o: dict, v, G: int, N: int, E: int, check_symmetric: bool) -> GraphBatch:
    """The GraphBatch of gtok_csr_from_coo's outputs and its read-back info, filled as GraphBatch.from_coo_device fills it."""
    flags = _lib.CSR_SIMPLE_SYMMETRIC if (check_symmetric and E and v[0] == 0) else 0
    b = GraphBatch(G, v[2], v[3], o["node_ptr"], o["edge_ptr"], o["rowptr"], o["col"], o["eorder"] if v[7] else None, o["nattr"], o["eattr"],
                   flags, v[4], v[5], v[1] if N else 0)
    b.checked = bool(check_symmetric and E)
    return b


def _csr_from_coo(src, dst, node_slices, edge_slices, x=None, edge_attr=None, indices=None, check_symmetric=True,
                  num_nodes=None, num_entries=None, device=None) -> Tuple[Optional[GraphBatch], int]:
    """csr_from_coo without the raise: -> (batch, 0) or (None, status bits)."""
    p = _coo_prepare(src, dst, node_slices, edge_slices, x, edge_attr, indices, num_nodes, num_entries, device)
    o, info = _coo_launch(p, check_symmetric)
    v = info.tolist()                                       # the one host read of the build
    if v[6]:
        return None, v[6]
    return _coo_batch(o, v, p["G"], p["N"], p["E"], check_symmetric), 0


def csr_from_coo(src, dst, node_slices, edge_slices, x=None, edge_attr=None, indices=None, check_symmetric: bool = True,
                 num_nodes: Optional[int] = None, num_entries: Optional[int] = None, device=None) -> GraphBatch:
    """The device GraphBatch of PyG collated storage, built by gtok_csr_from_coo (include/gtok.h): src / dst the two rows of
    edge_index (LOCAL node ids), node_slices / edge_slices = slices['x'] / slices['edge_index'] ([S + 1]), x [n(, k)] and
    edge_attr [E(, k)] optional (column 0 is the type), indices the storage graphs to take, in order (dataset._indices;
    None = all).  The same arrays, flags and maxima as GraphBatch.from_coo on the same graphs, bit for bit; eorder is None
    when every graph was already row-sorted.  Inputs of other dtypes or on the host are converted and uploaded.  The totals
    of the batch come from the host side (x.shape[0], the entry count, host slices) or from num_nodes / num_entries; only
    when neither shows them (device slices with indices, or without x) are they read back first.  One 32-byte read-back
    otherwise.  A damaged input (endpoints outside the graph, decreasing slices, wrong totals, an index outside the storage,
    an unsorted graph of more than COO_SORT_NODES nodes) raises CooInputError, a ValueError."""
    b, status = _csr_from_coo(src, dst, node_slices, edge_slices, x, edge_attr, indices, check_symmetric, num_nodes, num_entries, device)
    if status:
        raise CooInputError(status)
    return b


def lane_sorted(batch: GraphBatch, verify: bool = False) -> Optional[GraphBatch]:
    """The copy of a device batch of small symmetric graphs that sent_lane_kernel walks fastest (made once per batch,
    kept on the batch object): graphs stored by descending expected walk length - nodes + leaves, a walk restarts once
    per dead end - and dealt to waves in units of <= 64 neighbours whose staged bytes fit LANE_UNIT_LDS, so that the 64
    walks of a wave end together (in dataset order a unit of ZINC runs 41 steps for walks of 28 on average).
    `graph_ids` carries every slot's dataset index: output rows, lengths, query entries and RNG identity follow it, the
    tokens are those of the batch in dataset order.  A layout step like the CSR build, never part of an epoch.
    Built on the device by gtok_csr_lane_sort (counting sort, single-pass scans, the byte mirror in the same pass): a dozen
    small launches and ONE 32-byte read-back (the unit count and the LDS sizes of the launch).  verify=True: the batch's
    flags are not trusted - the same call checks GTOK_CSR_SIMPLE_SYMMETRIC on the device and sets it on `batch`
    (None is returned when the batch turns out not to be simple and symmetric, or to hold a graph of more nodes or
    entries than batch.max_nodes / batch.max_edges claim)."""
    if batch.lane_sorted is not None:
        return batch.lane_sorted
    if batch.col.device.type != "cuda" or batch.num_graphs == 0 or batch.max_nodes > 64 or batch.max_edges > 255 \
            or batch.graph_ids is not None or batch.num_edges_total == 0:
        return None
    if not verify and not (batch.flags & _lib.CSR_SIMPLE_SYMMETRIC):
        return None
    dev, G = batch.device, batch.num_graphs
    N, E = batch.num_nodes_total, batch.num_edges_total
    L = lib()
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)
    o = dict(graph_ids=i32(G), node_ptr=i32(G + 1), edge_ptr=torch.empty(G + 1, dtype=torch.int64, device=dev), rowptr=i32(N + G), col=i32(E),
             nattr=None if batch.nattr is None else u8(N), eattr=None if batch.eattr is None else u8(E),
             rowptr8=u8(N + G + 16), col8=u8(E + 16),          # + slack: 16-byte vector loads of the last chunk may run past the end
             unit_ptr=i32(G + 1), unit_info=i32(8 * G), info=i32(8))
    if os.environ.get("GTOK_NO_PACK8") == "1":              # tests: the lane kernel's int32 staging path
        o["rowptr8"] = o["col8"] = None
    ws = torch.empty(int(L.gtok_csr_lane_sort_workspace(G)), dtype=torch.uint8, device=dev)
    outs = _lib.GtokCsrSorted(*[None if o[n] is None else o[n].data_ptr() for n, _ in _lib.GtokCsrSorted._fields_])
    cs = batch.c_struct()
    check(L.gtok_csr_lane_sort(ctypes.byref(cs), LANE_UNIT_LDS, int(verify), ctypes.byref(outs), ws.data_ptr(), ws.numel(), _stream(dev)),
          "gtok_csr_lane_sort")
    viol, maxdeg, maxn, maxe, units, chunk_n, chunk_e, _ = o["info"].tolist()          # the one host read of the preparation
    if verify:
        # (a claim below the measured maxima would give the lane kernel a graph its 64-bit visited sets cannot hold; the
        # claims are <= 64 / 255 here, so the measured maxima are too)
        if viol or maxn > batch.max_nodes or maxe > batch.max_edges:
            return None
        batch.flags |= _lib.CSR_SIMPLE_SYMMETRIC
        batch.max_degree = maxdeg
    out = GraphBatch(G, batch.max_nodes, batch.max_edges, o["node_ptr"], o["edge_ptr"], o["rowptr"], o["col"], None, o["nattr"], o["eattr"],
                     batch.flags, chunk_n, chunk_e, batch.max_degree or maxdeg)
    out.graph_ids, out.num_units = o["graph_ids"], units
    out.unit_ptr = o["unit_ptr"][:units + 1].clone()        # (the arrays are sized for one unit per graph: keep what is used)
    out.unit_info = o["unit_info"][:8 * units].clone().view(units, 8)
    out.rowptr8, out.col8 = o["rowptr8"], o["col8"]
    batch.lane_sorted = out
    return out


_POPCOUNT8 = None


def _lane_order(batch: GraphBatch, typical_len: int) -> torch.Tensor:
    """The order sent_blane_kernel's lanes take the graphs in (64 consecutive entries share a wave, and a wave lasts as
    long as its slowest walk and, at every step, as its largest bracket).  A heuristic that only moves time, never tokens:
    graphs are grouped by the number of trail steps they are expected to take and, within a group, by density, so that
    the brackets of a wave's walks grow at the same pace.  The model: a walk takes n + r steps (r restarts ~ leaves - 1:
    the walk comes back once per dead end) and writes n position tokens, 2 per restart, the e - n + 1 bracket members and
    2 per non-empty bracket; members pile up with the square of the steps taken, the rest linearly - a t + q t^2 tokens
    after t steps - and a row cut at `typical_len` tokens stops where that reaches it (a 256-node star: 1.5 tokens per
    step, 400 steps of its 510; a dense random graph: 3 t + p t^2 / 2)."""
    global _POPCOUNT8
    dev = batch.device
    n = (batch.node_ptr[1:] - batch.node_ptr[:-1]).to(torch.float64)
    e = (batch.edge_ptr[1:] - batch.edge_ptr[:-1]).to(torch.float64)
    if batch.flags & _lib.CSR_SIMPLE_SYMMETRIC:
        e = e / 2
    # leaves = nodes of closure degree 1: bit 0 of the degree set, every higher bit clear (the mirror's degree planes)
    pl = batch.adj_planes
    higher = pl[:, 1]
    for k in range(2, 8):
        higher = higher | pl[:, k]
    deg1 = (pl[:, 0] & ~higher).contiguous().view(torch.uint8)
    if _POPCOUNT8 is None or _POPCOUNT8.device != dev:
        _POPCOUNT8 = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.int64, device=dev)
    leaves = _POPCOUNT8[deg1.long()].reshape(batch.num_graphs, -1).sum(1).to(torch.float64)
    r = (leaves - 1).clamp(min=0)
    members = (e - n + 1).clamp(min=0)
    steps_full = (n + r).clamp(min=1)
    a = (n + 2 * r + 2 * torch.minimum(n, members)) / steps_full
    q = members / (steps_full * steps_full)
    L = float(typical_len)
    cut = torch.where(q > 1e-9, (torch.sqrt(a * a + 4 * q * L) - a) / (2 * q).clamp(min=1e-9), L / a.clamp(min=1e-9))
    steps = torch.minimum(cut, steps_full).round().clamp(0, 1023).to(torch.int64)
    p = (2 * e / (n * n).clamp(min=1)).clamp(min=0.0, max=1.0)
    key = steps * 1024 + (p * 1023).round().to(torch.int64)
    return torch.argsort(key, descending=True, stable=True).to(torch.int32)


def adjbits(batch: GraphBatch) -> bool:
    """Give a device batch of graphs with <= 256 nodes its adjacency bit-matrix mirror (gtok_csr_adjbits; once per
    batch, kept on the batch object) and the order its graphs are dealt to lanes (longest walks first, so that the 64
    walks of a wave have similar lengths).  Returns whether the batch has one now.  A layout step like the CSR build:
    the lane-per-graph SENT kernel for unlabelled graphs reads one row of it per trail step."""
    if batch.adj_rows is not None:
        return True
    if os.environ.get("GTOK_NO_ADJBITS") == "1":
        return False
    if batch.col.device.type != "cuda" or batch.num_graphs == 0 or batch.max_nodes > 256:
        return False
    dev, G = batch.device, batch.num_graphs
    W = _adj_words(batch.max_nodes)
    total_nodes = batch.rowptr.numel() - G
    rows = torch.empty((max(total_nodes, 1), W), dtype=torch.int64, device=dev)
    planes = torch.empty((G, 8, W), dtype=torch.int64, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    cs = batch.c_struct()
    check(lib().gtok_csr_adjbits(ctypes.byref(cs), W, rows.data_ptr(), planes.data_ptr(), info.data_ptr(), _stream(dev)),
          "gtok_csr_adjbits")
    maxdeg = int(info.item())
    if maxdeg > 255:          # a 256-node graph with a full row and a self loop: 8 counter planes cannot hold it
        return False
    batch.adj_rows, batch.adj_planes, batch.adj_words, batch.adj_max_degree = rows, planes, W, maxdeg
    return True


PACK_STATE_FILL, PACK_STATE_STRIDE, PACK_REGIONS = 16, 16, 64       # include/gtok.h: GTOK_PACK_STATE_*
PACK_STATE_WORDS = PACK_STATE_FILL + PACK_STATE_STRIDE * PACK_REGIONS
ID_TOO_WIDE_8 = "an id does not fit 8 bits: use 16-bit packed rows"


class PackedRows:
    """The packed twin of a SENT launch's rows (ops.sent(..., packed=PackedRows(...)): gtok_sent_packed - the walk of either
    lane-per-graph kernel, sent_lane_kernel or sent_blane_kernel, packs; other batches go through gtok_pack_rows_scan).  buf: `capacity` ids of
    the slab's width, every row from a 16-byte boundary; row_start int64 [rows]: where row (epoch, graph) starts in buf, -1 for a row
    that did not fit (rows lie in the order their 64-graph units finished, inside up to 64 regions of the buffer that fill side by
    side, not in dataset order - readers go through row_start: ops.unpack_rows_at, ops.collate_packed(buf, row_start, ...)); state
    int64 [PACK_STATE_WORDS]: the status word and the regions' fill marks (include/gtok.h).  Size the buffer as the expected total
    + a few per cent.  fused: whether the walk kernel itself wrote it (else gtok_sent + gtok_pack_rows_scan did: dataset order).
    elem_bytes=1 (GTOK_SENT_PACK_U8; with ops.sent(..., u16=True) only): buf is torch.uint8 - one byte per id, rows from multiples
    of 16 ids, capacity rounded up to 16; status bit 0 then says that an id did not fit 8 bits and the buffer is not to be used
    (verify() raises).  elem_bytes=None: the slab's width, as `u16` says."""
    __slots__ = ("buf", "row_start", "_ring", "_slot", "capacity", "fused", "elem_bytes")
    RING = 32          # state blocks (8 KB each) zeroed together: a launch takes the next one instead of paying a memset of its own

    def __init__(self, rows: int, capacity: int, u16: bool, device, elem_bytes: Optional[int] = None):
        if elem_bytes is None:
            elem_bytes = 2 if u16 else 4
        if elem_bytes != (2 if u16 else 4) and not (elem_bytes == 1 and u16):
            raise ValueError("PackedRows: elem_bytes is the slab's id width (2 with u16, else 4), or 1 with u16=True")
        self.elem_bytes = int(elem_bytes)
        al = 16 if elem_bytes == 1 else 8
        self.capacity = max(al, -(-int(capacity) // al) * al)
        self.buf = torch.empty(self.capacity, dtype={1: torch.uint8, 2: torch.int16, 4: torch.int32}[self.elem_bytes], device=device)
        self.row_start = torch.empty(max(1, int(rows)), dtype=torch.int64, device=device)
        self._ring = torch.zeros((self.RING, PACK_STATE_WORDS), dtype=torch.int64, device=device)
        self._slot = 0
        self.fused = None

    @property
    def state(self) -> torch.Tensor:
        """int64 [PACK_STATE_WORDS]: the status word and the fill marks of the LAST fill (include/gtok.h)"""
        return self._ring[self._slot]

    def _fresh_state(self) -> torch.Tensor:
        """a zeroed state block for the next launch: the next one of the ring (all of them are zeroed again, in one launch, when the
        ring wraps); under stream capture the block is zeroed inside the capture - replays reuse it"""
        if torch.cuda.is_current_stream_capturing():
            self.state.zero_()
            return self.state
        self._slot = (self._slot + 1) % self.RING
        if self._slot == 0:
            self._ring.zero_()
        return self.state

    def status(self) -> torch.Tensor:
        """int32 [1] on the device: the pack_rows status bits of this fill (bit 1: the buffer was too small for some rows; bit 0, 8-bit
        rows only: an id did not fit 8 bits - the buffer is not to be used)."""
        return self.state[0:1].to(torch.int32)

    def verify(self) -> None:
        """Raise when the last fill met an id that does not fit the buffer's width (status bit 0; one host read)."""
        if int(self.state[0].item()) & 1:
            raise _lib.GtokError(ID_TOO_WIDE_8)

    def used(self) -> torch.Tensor:
        """int64 scalar on the device: ids the fill took (the regions' fill marks added up; skipped rows included)."""
        return self.state[PACK_STATE_FILL::PACK_STATE_STRIDE].sum()


def sent(batch: GraphBatch, max_num_nodes: int, max_len: int, seed: int, epoch: int = 0, labeled: bool = False,
         num_node_types: int = 0, num_edge_types: int = 0, remap_zinc: bool = False, pad_id: int = SENT_PAD,
         graph_base: int = 0, query: Optional[torch.Tensor] = None,
         ld: Optional[int] = None, out=None, pad: bool = True, epochs: int = 1, u16: bool = False,
         packed: Optional[PackedRows] = None, slab: bool = True, check_ids: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """SENT trail walk.  Returns (ids int32 [G, ld], len int32 [G]); len > ld flags a too-narrow slab.
    pad=False (GTOK_SENT_NO_PAD): rows are only written up to their length - for consumers that go through `len`
    (ops.collate does); the rest of the slab keeps whatever it held.
    epochs=K > 1 (gtok_sent_params.epoch_count): the trails of epochs epoch .. epoch + K - 1 in ONE launch - returns
    (ids [K, G, ld], len [K, G]); slice e is what a call with epoch + e returns.  The trainer re-tokenizes its splits every
    epoch (trainer/train_agtt.py:246-250): K epochs of a small split fill the chip where one cannot.
    u16=True (GTOK_SENT_U16): the slab holds 16-bit ids (torch.int16 storage, to be read as unsigned: every SENT id fits) -
    half the bytes; readers: ops.collate_packed / ops.unpack_rows with row_ptr=None, ops.pack_rows_u16.
    packed=PackedRows(K * G, capacity, u16, device): the rows are ALSO appended to packed.buf (a fresh fill: its state is
    zeroed first) - by the walk kernel itself where the batch runs sent_lane_kernel, or sent_blane_kernel with >= 20,000 walks
    (graphs x epochs), 16- / 32-bit packed ids and ld <= 2040 / 1020 (gtok_sent_packed: no second pass over the rows), else by
    gtok_pack_rows_scan behind the walk; either way packed.row_start / packed.state describe the result and packed.fused says which.
    slab=False (with packed=; GTOK_SENT_PACK_ONLY): the caller reads the packed rows alone - no [K, G, ld] slab is written or
    allocated (the walk stages its rows in a per-device scratch of 64 rows per resident wave: 262,144 rows x ld ids on an MI355X whatever K
    is - 92 MB at ZINC's ld 176, 319 MB at config 5's ld 608) and
    the first return value is None; out=(staging, len) then names the caller's own staging space (or None) and length tensor.
    packed=PackedRows(..., elem_bytes=1) (with u16=True; GTOK_SENT_PACK_U8): one byte per id in packed.buf.  Whether every id fits
    is a property of the data, so the status word is read back behind the launch (one host read) and GtokError raised when one
    did not; check_ids=False - and any launch under stream capture - leaves that to the caller (packed.verify(), packed.status())."""
    _need_gpu(batch.col, "sent")
    dev = batch.device
    K = max(1, int(epochs))
    if query is not None:
        query = query.to(dev, dtype=torch.int32).contiguous()
        if tuple(query.shape) != (batch.num_graphs, 2):
            raise ValueError("query must be [G, 2] (query_u, query_v)")
    if ld is None:
        ld = sent_safe_ld(batch, labeled, max_len, query is not None)
    G = batch.num_graphs
    if not slab and packed is None:
        raise ValueError("slab=False goes with packed=")
    ids, staging, ln = _sent_out(out, slab, K, G, ld, u16, dev)
    if _lib.library_version() < 4 and (K > 1 or u16 or not pad):
        # (GTOK_LIB pointing at an ABI v3 build: it would ignore epoch_count and the row flags and write an int32 [G, ld] slab)
        raise _lib.GtokError(f"the loaded library has ABI version {_lib.library_version()}: epochs > 1, u16 and pad=False need version 4")
    params = lambda flags: _sent_params(max_num_nodes, max_len, labeled, num_node_types, num_edge_types, remap_zinc, pad_id, flags,
                                        seed, epoch, graph_base, query, K)
    p = params((0 if pad else _lib.SENT_NO_PAD) | (_lib.SENT_U16 if u16 else 0))
    cs, lb = _sent_layouts(batch, p, max_len)
    global _LAST_SENT, _LAST_CONSTS
    _LAST_SENT, _LAST_CONSTS = (cs, p), False
    rc = _lib.E_UNSUPPORTED if packed is None else _sent_packed(cs, p, params, packed, ids, staging, ln, K * G, ld, u16, dev)
    if rc == _lib.E_UNSUPPORTED:
        if ids is None:             # another kernel walks: it needs the slab after all (a temporary one)
            ids = torch.empty((K * G, ld), dtype=torch.int16 if u16 else torch.int32, device=dev)
        kc = _sent_consts(lb, p) if lb is not None and labeled and remap_zinc else None
        if kc is not None:          # the reordered batch's constants mirror: the walk emits staged bytes as tokens
            check(lib().gtok_sent_prepared(ctypes.byref(cs), ctypes.byref(p), ctypes.byref(kc), ids.data_ptr(), ld, ln.data_ptr(), _stream(dev)),
                  "gtok_sent_prepared")
            _LAST_CONSTS = True
        else:
            check(lib().gtok_sent(ctypes.byref(cs), ctypes.byref(p), ids.data_ptr(), ld, ln.data_ptr(), _stream(dev)),
                  "gtok_sent")
        if packed is not None and G:           # another kernel walked: the one-pass pack behind it (dataset order)
            _pack_behind_walk(packed, ids, ln, K * G, ld, dev)
    if packed is not None and packed.buf.dtype == torch.uint8 and check_ids and G and not torch.cuda.is_current_stream_capturing():
        packed.verify()
    shape = (K, G) if K > 1 else (G,)
    return (ids.view(*shape, ld) if slab else None), ln.view(shape)


_LARGE_WS = {}


def _large_workspace(dev, need: int) -> torch.Tensor:
    """gtok_sent_large's workspace: one uint8 buffer per device, grown on demand, shared by every launch on that device (launches on
    one stream follow each other; its contents mean nothing between launches)."""
    key = torch.device(dev).index or 0
    t = _LARGE_WS.get(key)
    if t is None or t.numel() < need:
        t = torch.empty(max(16, need), dtype=torch.uint8, device=dev)
        _LARGE_WS[key] = t
    return t


def sent_large(batch: GraphBatch, max_num_nodes: int, max_len: int, seed: int, epoch: int = 0, labeled: bool = False,
               num_node_types: int = 0, num_edge_types: int = 0, remap_zinc: bool = False, pad_id: int = SENT_PAD,
               graph_base: int = 0, query: Optional[torch.Tensor] = None, ld: Optional[int] = None, out=None, pad: bool = True,
               epochs: int = 1, u16: bool = False, workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """gtok_sent_large: the SENT trail walk for batches ops.sent refuses - graphs of up to _lib.SENT_LARGE_MAX_NODES nodes, any edge
    list (one direction or both, duplicates, self loops), in dataset order.  Same tokens, same keywords and same returns as
    ops.sent (minus packed= / slab=: packed rows of such batches come from ops.pack_rows_scan over the slab).  workspace: a
    uint8 tensor of the caller's own (launches on several streams must not share the module's); None = a cached one per device."""
    _need_gpu(batch.col, "sent_large")
    if not hasattr(lib(), "gtok_sent_large"):
        raise _lib.GtokError("the loaded library has no gtok_sent_large: rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`)")
    dev = batch.device
    K = max(1, int(epochs))
    if query is not None:
        query = query.to(dev, dtype=torch.int32).contiguous()
        if tuple(query.shape) != (batch.num_graphs, 2):
            raise ValueError("query must be [G, 2] (query_u, query_v)")
    if ld is None:
        ld = sent_safe_ld(batch, labeled, max_len, query is not None)
    G = batch.num_graphs
    ids, _, ln = _sent_out(out, True, K, G, ld, u16, dev)
    p = _sent_params(max_num_nodes, max_len, labeled, num_node_types, num_edge_types, remap_zinc, pad_id,
                     (0 if pad else _lib.SENT_NO_PAD) | (_lib.SENT_U16 if u16 else 0), seed, epoch, graph_base, query, K)
    cs = batch.c_struct()
    need = int(lib().gtok_sent_large_workspace(batch.max_nodes, batch.max_edges, G * K))
    if need < 0:
        check(need, "gtok_sent_large_workspace")
    ws = workspace if workspace is not None else _large_workspace(dev, need)
    if ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.device != torch.device(dev):
        raise ValueError("workspace: a contiguous uint8 tensor on the batch's device")
    check(lib().gtok_sent_large(ctypes.byref(cs), ctypes.byref(p), ids.data_ptr(), ld, ln.data_ptr(), ws.data_ptr(), ws.numel(),
                                _stream(dev)), "gtok_sent_large")
    global _LAST_SENT
    _LAST_SENT = "sent_large_kernel"
    shape = (K, G) if K > 1 else (G,)
    return ids.view(*shape, ld), ln.view(shape)


def sent_order(batch: GraphBatch, max_len: int, seed: int, epoch: int = 0, epochs: int = 1, graph_base: int = 0, with_rows: bool = False,
               max_num_nodes: Optional[int] = None, labeled: bool = False, num_node_types: int = 0, num_edge_types: int = 0,
               remap_zinc: bool = False, pad_id: int = SENT_PAD, query: Optional[torch.Tensor] = None, ld: Optional[int] = None,
               pad: bool = True, u16: bool = False, workspace: Optional[torch.Tensor] = None):
    """gtok_sent_large_order: the visit order of the SENT walks of (seed, epoch .. epoch + K - 1, graph_base + g) - visit_index int32
    [K, N_total]: visit_index[e, node_ptr[g] + u] = k when node u of graph g was the k-th node first visited (position token 6 + k),
    -1 when the walk stopped (max_len) before it got there.  It is the order of the rows of ops.sent as well (every SENT kernel emits
    the same tokens), for any batch in dataset order with graphs of up to _lib.SENT_LARGE_MAX_NODES nodes.  Pass the max_len and
    labeled the rows were written with (they decide where a cut walk stops); nothing else of the row format matters.
    with_rows=True: -> (visit_index, ids, len), the rows ops.sent_large returns (its keywords), from the same launch.
    workspace: as ops.sent_large."""
    _need_gpu(batch.col, "sent_order")
    _need(_lib.ORDER_SYMBOLS, "gtok_sent_large_order / gtok_csr_relabel")
    dev = batch.device
    K = max(1, int(epochs))
    G, N = batch.num_graphs, batch.num_nodes_total
    if max_num_nodes is None:
        max_num_nodes = batch.max_nodes
    vis = torch.empty((K, N), dtype=torch.int32, device=dev)
    ids = ln = None
    flags = 0
    if with_rows:
        if query is not None:
            query = query.to(dev, dtype=torch.int32).contiguous()
            if tuple(query.shape) != (G, 2):
                raise ValueError("query must be [G, 2] (query_u, query_v)")
        if ld is None:
            ld = sent_safe_ld(batch, labeled, max_len, query is not None)
        ids, _, ln = _sent_out(None, True, K, G, ld, u16, dev)
        flags = (0 if pad else _lib.SENT_NO_PAD) | (_lib.SENT_U16 if u16 else 0)
    p = _sent_params(max_num_nodes, max_len, labeled, num_node_types, num_edge_types, remap_zinc, pad_id, flags, seed, epoch, graph_base,
                     query if with_rows else None, K)
    cs = batch.c_struct()
    need = int(lib().gtok_sent_large_workspace(batch.max_nodes, batch.max_edges, G * K))
    if need < 0:
        check(need, "gtok_sent_large_workspace")
    ws = workspace if workspace is not None else _large_workspace(dev, need)
    if ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.device != torch.device(dev):
        raise ValueError("workspace: a contiguous uint8 tensor on the batch's device")
    spare = vis if N else torch.empty(1, dtype=torch.int32, device=dev)      # (the library wants an address: an empty tensor has none)
    check(lib().gtok_sent_large_order(ctypes.byref(cs), ctypes.byref(p), None if ids is None else ids.data_ptr(), int(ld or 0),
                                      None if ln is None else ln.data_ptr(), spare.data_ptr(), N, ws.data_ptr(), ws.numel(), _stream(dev)),
          "gtok_sent_large_order")
    if not with_rows:
        return vis
    shape = (K, G) if K > 1 else (G,)
    return vis, ids.view(*shape, ld), ln.view(shape)


def _sent_params(max_num_nodes: int, max_len: int, labeled: bool, num_node_types: int, num_edge_types: int, remap_zinc: bool,
                 pad_id: int = SENT_PAD, flags: int = 0, seed: int = 0, epoch: int = 0, graph_base: int = 0,
                 query: Optional[torch.Tensor] = None, epochs: int = 1) -> GtokSentParams:
    """include/gtok.h: gtok_sent_params of a call's arguments and a flags word (GTOK_SENT_*)."""
    return GtokSentParams(max_num_nodes, int(labeled), num_node_types, num_edge_types, max_len, int(remap_zinc), pad_id, flags,
                          seed & (2 ** 64 - 1), epoch & (2 ** 64 - 1), graph_base, None if query is None else query.data_ptr(),
                          max(1, int(epochs)), 0)


def _sent_out(out, slab: bool, K: int, G: int, ld: int, u16: bool, dev):
    """(slab or None, the caller's own staging rows or None, lengths) of a sent() call: allocated, or the caller's `out` validated."""
    want = torch.int16 if u16 else torch.int32
    if out is None:
        return (torch.empty((K * G, ld), dtype=want, device=dev) if slab else None), None, torch.empty((K * G,), dtype=torch.int32, device=dev)
    if slab:
        ids, ln = out
        if ids.dtype != want or ln.dtype != torch.int32 or ids.numel() != K * G * ld or ln.numel() != K * G \
                or not ids.is_contiguous() or not ln.is_contiguous() or ids.device != torch.device(dev) or (G and ids.shape[-1] != ld):
            raise ValueError(f"out must be ({want} [K * G, ld] contiguous, int32 [K * G]) on the batch's device")
        return ids, None, ln
    staging, ln = out         # (staging rows of the caller's own - launches on several streams must not share the module's - , lengths)
    if staging is not None and (staging.dtype != want or not staging.is_contiguous() or staging.device != torch.device(dev)):
        raise ValueError("out[0] with slab=False: contiguous staging space of the rows' id width on the batch's device (or None)")
    if ln.dtype != torch.int32 or ln.numel() != K * G or not ln.is_contiguous():
        raise ValueError("out[1]: contiguous int32 [K * G]")
    return None, staging, ln


def _adj_words(max_nodes: int) -> int:        # 64-bit words of a row of the adjacency bit-matrix mirror (<= 256 nodes)
    return 1 if max_nodes <= 64 else 2 if max_nodes <= 128 else 4


def _mirror_wanted(cs: _lib.GtokCsr, p: GtokSentParams) -> bool:
    """Whether gtok_sent would launch sent_blane_kernel if the batch had its bit-matrix mirror: the launcher's own choice (GTOK_SENT_KERNEL
    included) for a copy of the C struct that claims one as adjbits() builds it.  (Scalars alone are read: the claim is never dereferenced.)"""
    claim = _lib.GtokCsr.from_buffer_copy(cs)
    claim.adj_rows = claim.adj_planes = 1
    claim.adj_words, claim.adj_max_degree = _adj_words(cs.max_nodes), 0
    return lib().gtok_sent_kernel_name(ctypes.byref(claim), ctypes.byref(p)).startswith(b"sent_blane_kernel")


def lane_consts(sb: GraphBatch, max_num_nodes: int, num_node_types: int, num_edge_types: int) -> Optional[dict]:
    """The constants mirror of a reordered batch (ops.lane_sorted's copy, or a caller-prepared one) for one set of tokenizer
    settings, built by gtok_sent_lane_consts on first use and kept on the batch, one per settings key: ntok8 / etok8 - the
    remapped token of every node / entry type byte, which the labelled + remapped walk stages in place of the bytes - and
    `status` (the ONE host read of the build; non-zero: a token does not fit a byte and `consts`, the C struct gtok_sent_prepared
    takes, is None).  A layout step like lane_sorted, never part of an epoch.  None: not such a batch, or a library without it."""
    if sb.graph_ids is None or sb.unit_ptr is None or sb.rowptr8 is None or sb.col8 is None or sb.nattr is None or sb.eattr is None \
            or sb.col.device.type != "cuda" or not hasattr(lib(), "gtok_sent_prepared"):
        return None
    key = (int(max_num_nodes), int(num_node_types), int(num_edge_types))
    hit = sb.lane_consts.get(key)
    if hit is None:
        if torch.cuda.is_current_stream_capturing():      # (the status read-back cannot be captured: this launch goes without)
            return None
        dev, N, E = sb.device, sb.num_nodes_total, sb.num_edges_total
        ntok8 = torch.empty(N + 16, dtype=torch.uint8, device=dev)      # (+ 16: the slack the byte mirrors carry)
        etok8 = torch.empty(E + 16, dtype=torch.uint8, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        p = _sent_params(key[0], 0, True, key[1], key[2], True)
        cs = sb.c_struct()
        check(lib().gtok_sent_lane_consts(ctypes.byref(cs), ctypes.byref(p), N, E, ntok8.data_ptr(), etok8.data_ptr(), status.data_ptr(),
                                          _stream(dev)), "gtok_sent_lane_consts")
        st = int(status.item())
        c = None if st else _lib.GtokSentConsts(ntok8.data_ptr(), etok8.data_ptr(), key[0], key[1], key[2], 0)
        hit = sb.lane_consts[key] = dict(ntok8=ntok8[:N], etok8=etok8[:E], status=st, consts=c)   # (item assignment: the cached C struct stays)
    return hit


def _sent_consts(lb: GraphBatch, p: GtokSentParams):
    """gtok_sent_consts for this launch of the reordered batch `lb`, or None (switched off, not applicable, a token beyond a byte)."""
    if os.environ.get("GTOK_NO_LANE_CONSTS") == "1":       # tests, A/B
        return None
    hit = lb.lane_consts.get((p.max_num_nodes, p.num_node_types, p.num_edge_types))
    if hit is None:
        hit = lane_consts(lb, p.max_num_nodes, p.num_node_types, p.num_edge_types)
    return None if hit is None else hit["consts"]


def _sent_layouts(batch: GraphBatch, p: GtokSentParams, max_len: int):
    """(the C struct sent() launches: the batch with the layouts its kernel reads, each built on first use and kept on the batch;
    the reordered batch behind it - ops.lane_sorted's copy or the caller's own - or None)"""
    if not batch.prepared:          # (a batch prepared by the caller - torch.ops.gtok.csr_prepare - is launched as it stands)
        pack8(batch)
        # the bit-matrix mirror is only built where gtok_sent would pick the kernel that reads it - and never again for a batch
        # that turned out unusable (a closure degree above 255)
        if not batch.adj_unusable and _mirror_wanted(batch.c_struct(), p):
            if adjbits(batch):
                if os.environ.get("GTOK_BLANE_ORDER", "1") != "0" and batch.lane_order_len != max(1, max_len):
                    batch.lane_order, batch.lane_order_len = _lane_order(batch, max(1, max_len)), max(1, max_len)   # once per (batch, max_len)
            elif batch.col.device.type == "cuda" and batch.max_nodes <= 256 and os.environ.get("GTOK_NO_ADJBITS") != "1":
                batch.adj_unusable = True
    cs = batch.c_struct()
    if os.environ.get("GTOK_NO_LANE_SORT") != "1" and batch.graph_ids is None and not batch.prepared \
            and lib().gtok_sent_kernel_name(ctypes.byref(cs), ctypes.byref(p)) == b"sent_lane_kernel":
        sb = lane_sorted(batch)                                       # once per resident batch
        if sb is not None:
            return sb.c_struct(), sb
    return cs, (batch if batch.graph_ids is not None else None)


def _sent_packed(cs, p: GtokSentParams, params, packed: PackedRows, ids, staging, ln, rows: int, ld: int, u16: bool, dev) -> int:
    """sent(packed=): gtok_sent_packed - the walk packs its rows.  Returns 0, or GTOK_E_UNSUPPORTED where it cannot (another kernel, no rows,
    an ld that is not whole 16-byte pieces).  ids None (slab=False): the rows are staged in `staging` or the module's scratch (GTOK_SENT_PACK_ONLY)."""
    if _lib.library_version() < 6:
        raise _lib.GtokError(f"the loaded library has ABI version {_lib.library_version()}: packed= needs version 6")
    pk8 = packed.buf.dtype == torch.uint8
    if pk8 and not u16:
        raise ValueError("packed: 8-bit packed rows go with u16=True (the slab / staging rows stay 16-bit)")
    if pk8 and _lib.library_version() < 8:
        raise _lib.GtokError(f"the loaded library has ABI version {_lib.library_version()}: 8-bit packed rows need version 8")
    if (not pk8 and packed.buf.dtype != (torch.int16 if u16 else torch.int32)) or packed.row_start.numel() < rows or packed.buf.device != ln.device:
        raise ValueError("packed: a PackedRows of this launch's rows, id width and device")
    packed._fresh_state()
    rc, flags = _lib.E_UNSUPPORTED, p.flags
    if rows and ld % (16 if pk8 else 8 if u16 else 4) == 0:
        if pk8:
            flags |= _lib.SENT_PACK_U8
        dst = ids
        if ids is None:
            need = int(lib().gtok_sent_pack_scratch_rows(_stream(dev))) * ld
            if staging is not None and staging.numel() < need:
                raise ValueError(f"out[0] with slab=False: {need} ids of staging space (gtok_sent_pack_scratch_rows() x ld)")
            dst = staging if staging is not None else _pack_scratch(dev, ld, u16)
            flags |= _lib.SENT_PACK_ONLY
        pp = p if flags == p.flags else params(flags)
        rc = lib().gtok_sent_packed(ctypes.byref(cs), ctypes.byref(pp), dst.data_ptr(), ld, ln.data_ptr(), packed.buf.data_ptr(),
                                    packed.capacity, packed.row_start.data_ptr(), packed.state.data_ptr(), _stream(dev))
        if rc != _lib.E_UNSUPPORTED:
            check(rc, "gtok_sent_packed")
    packed.fused = rc == 0
    return rc


def _pack_behind_walk(packed: PackedRows, ids: torch.Tensor, ln: torch.Tensor, rows: int, ld: int, dev) -> None:
    """sent(packed=) behind a kernel that does not pack: gtok_pack_rows_scan over the slab, described in `packed` as the fused route does."""
    ptr = torch.empty(rows + 1, dtype=torch.int64, device=dev)
    st = torch.empty(1, dtype=torch.int32, device=dev)
    pb = packed.buf.element_size()          # (1: 8-bit packed rows from the 16-bit slab, 16-id alignment)
    check(lib().gtok_pack_rows_scan(ids.data_ptr(), ids.element_size(), ld, ln.data_ptr(), rows, 16 if pb == 1 else 8, pb, packed.buf.data_ptr(),
                                    packed.capacity, ptr.data_ptr(), st.data_ptr(), _stream(dev)), "gtok_pack_rows_scan")
    # a row the scan skipped keeps its offset in ptr: it is marked -1 here, as the fused route marks it
    skipped = ptr[:-1] + ln.clamp(0, ld) > packed.capacity
    packed.row_start[:rows].copy_(torch.where(skipped, -1, ptr[:-1]))
    packed.state[PACK_STATE_FILL:PACK_STATE_FILL + 1].copy_(ptr[-1:])
    packed.state[0:1].copy_(st.to(torch.int64) & (3 if pb == 1 else 2))


_PACK_SCRATCH = {}


def _pack_scratch(dev, ld: int, u16: bool) -> torch.Tensor:
    """the staging rows of GTOK_SENT_PACK_ONLY launches: one buffer per (device, width, id size), grown on demand, shared by every
    launch on that device (launches on one stream follow each other; callers with several streams pass their own slab)"""
    key = (torch.device(dev).index or 0, bool(u16))
    rows = int(lib().gtok_sent_pack_scratch_rows(_stream(dev)))
    if rows < 0:
        check(rows, "gtok_sent_pack_scratch_rows")
    t = _PACK_SCRATCH.get(key)
    if t is None or t.numel() < rows * ld:
        t = torch.empty(rows * ld, dtype=torch.int16 if u16 else torch.int32, device=dev)
        _PACK_SCRATCH[key] = t
    return t


_LAST_SENT = None
_LAST_CONSTS = False


def last_sent_consts() -> bool:
    """Whether the most recent ops.sent call launched the instantiation that reads the constants mirror (gtok_sent_prepared:
    sent_lane_kernel<..., TOK8>).  last_sent_kernel() names the kernel template either way."""
    return bool(_LAST_CONSTS) and not isinstance(_LAST_SENT, str)


def last_sent_kernel() -> str:
    """Name of the kernel the most recent ops.sent call of this process launched (tests, bench labels): what the C ABI's
    gtok_sent_kernel_name answers for the very structs that call passed to gtok_sent ("sent_large_kernel" after ops.sent_large)."""
    if _LAST_SENT is None:
        return ""
    if isinstance(_LAST_SENT, str):
        return _LAST_SENT
    cs, p = _LAST_SENT
    return lib().gtok_sent_kernel_name(ctypes.byref(cs), ctypes.byref(p)).decode()


def sent_kernel_name(batch: GraphBatch, max_num_nodes: int, max_len: int, labeled: bool = False, num_node_types: int = 0,
                     num_edge_types: int = 0, remap_zinc: bool = False, epochs: int = 1) -> str:
    """Name of the kernel gtok_sent() picks for this batch (for profiles and bench labels)."""
    p = _sent_params(max_num_nodes, max_len, labeled, num_node_types, num_edge_types, remap_zinc, epochs=epochs)
    cs = batch.c_struct()
    return lib().gtok_sent_kernel_name(ctypes.byref(cs), ctypes.byref(p)).decode()


def sent_decode(ids: torch.Tensor, ln: torch.Tensor, max_num_nodes: int, labeled: bool = False, num_node_types: int = 0,
                edge_cap: Optional[int] = None, node_cap: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """Un-remapped SENT rows -> graphs in visit-index space (node k = the k-th node the trail visited): num_nodes,
    num_edges, status int32 [G]; edge_a, edge_b, edge_type int32 [G, edge_cap]; node_type int32 [G, node_cap].
    status: 0 complete, 1 malformed, 2 capacity exceeded, 3 cut before EOS."""
    _need_gpu(ids, "sent_decode")
    if ids.dtype != torch.int32 or ids.dim() != 2 or not ids.is_contiguous():
        raise ValueError("sent_decode expects a contiguous int32 [G, ld] slab")
    dev, (G, ld) = ids.device, ids.shape
    ecap = int(edge_cap) if edge_cap is not None else ld
    ncap = int(node_cap) if node_cap is not None else max(1, max_num_nodes)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    out = dict(num_nodes=i32(G), num_edges=i32(G), status=i32(G), edge_a=i32(G, ecap), edge_b=i32(G, ecap),
               edge_type=i32(G, ecap), node_type=i32(G, ncap))
    _lib.check(_lib.lib().gtok_sent_decode(ids.data_ptr(), ld, ln.data_ptr(), G, max_num_nodes, int(labeled), num_node_types,
                                           out["num_nodes"].data_ptr(), out["num_edges"].data_ptr(), out["edge_a"].data_ptr(),
                                           out["edge_b"].data_ptr(), out["edge_type"].data_ptr(), ecap,
                                           out["node_type"].data_ptr(), ncap, out["status"].data_ptr(), _stream(dev)),
               "gtok_sent_decode")
    return out


def _decode_rows(ids: torch.Tensor, ln: torch.Tensor, row_start: Optional[torch.Tensor], ld: Optional[int], what: str):
    """The row arguments of gtok_sent_decode_sizes / gtok_sent_decode_csr, checked: -> (elem_bytes, ld, rows)."""
    _need_gpu(ids, what)
    if ln.dtype != torch.int32 or ln.dim() != 1 or not ln.is_contiguous() or ln.device != ids.device:
        raise ValueError(f"{what}: lengths must be a contiguous int32 vector on the rows' device")
    rows = int(ln.numel())
    if not ids.is_contiguous():
        raise ValueError(f"{what}: ids must be contiguous")
    if row_start is None:
        if ids.dtype not in (torch.int32, torch.int16) or ids.dim() != 2 or int(ids.shape[0]) != rows:
            raise ValueError(f"{what}: without row_start, ids is an int32 or int16 [rows, ld] slab with one length per row")
        if ld is not None and int(ld) != int(ids.shape[1]):
            raise ValueError(f"{what}: ld is the slab's width")
        ld = int(ids.shape[1])
    else:
        if ids.dtype not in (torch.uint8, torch.int16, torch.int32) or ids.dim() != 1:
            raise ValueError(f"{what}: with row_start, ids is a flat uint8 / int16 / int32 buffer of packed rows")
        if row_start.dtype != torch.int64 or row_start.dim() != 1 or not row_start.is_contiguous() or int(row_start.numel()) < rows \
                or row_start.device != ids.device:
            raise ValueError(f"{what}: row_start must be a contiguous int64 vector of (at least) one start per row on the rows' device")
        ld = 0x7FFFFFFF if ld is None else int(ld)           # (a packed row holds min(len, ld) ids: by default all of its len)
    return ids.element_size(), ld, rows


def _built_arrays(what: str, dev, G: int, N: int, E: int, nattr: bool, eattr: bool, node_ptr=None, edge_ptr=None, status: bool = False):
    """Fresh arrays of a gtok_csr_built for G graphs of N nodes and E entries in all: -> (dict of the arrays, the C struct).  node_ptr /
    edge_ptr: the caller's own where the call reads them (pass 2 of the decoders), checked here and part of the dict; nattr / eattr
    None when not asked for; status: an int32 [G] beside them.  info is zero when G == 0 (the caller then launches nothing)."""
    if node_ptr is not None and (
            node_ptr.dtype != torch.int32 or edge_ptr.dtype != torch.int64 or node_ptr.numel() != G + 1 or edge_ptr.numel() != G + 1
            or not node_ptr.is_contiguous() or not edge_ptr.is_contiguous() or node_ptr.device != dev or edge_ptr.device != dev):
        raise ValueError(f"{what}: node_ptr int32 [rows + 1] and edge_ptr int64 [rows + 1] on the rows' device")
    N, E = int(N), int(E)
    if N < 0 or E < 0 or N + G >= 2 ** 31:
        raise ValueError(f"{what}: totals out of range (a batch holds fewer than 2^31 nodes + graphs; shard it)")
    # (the library wants an address for every array, and an empty tensor has none: one spare element, sliced off)
    new = lambda n, dt: torch.empty(n + 1, dtype=dt, device=dev)
    full = dict(rowptr=new(N + G, torch.int32), col=new(E, torch.int32), eorder=new(E, torch.int32),
                nattr=new(N, torch.uint8) if nattr else None, eattr=new(E, torch.uint8) if eattr else None, info=new(8, torch.int32))
    if status:
        full["status"] = new(G, torch.int32)
    ptr = lambda t: None if t is None else t.data_ptr()
    cout = _lib.GtokCsrBuilt(ptr(node_ptr), ptr(edge_ptr), *[ptr(full[n]) for n in ("rowptr", "col", "eorder", "nattr", "eattr", "info")])
    o = {k: None if t is None else t[:-1] for k, t in full.items()}
    if node_ptr is not None:
        o = dict(node_ptr=node_ptr, edge_ptr=edge_ptr, **o)
    if G == 0:
        o["info"].zero_()
    return o, cout


def _decoded_batch(what: str, nn: torch.Tensor, ne: torch.Tensor, launch, check_symmetric: bool) -> GraphBatch:
    """The second half of sent_decode_csr / ibtt_decode_csr: the sizes of pass 1 prefix-summed, their totals read back, pass 2 -
    launch(node_ptr, edge_ptr, N, E) -> the dict of its arrays - and `info` read back into the GraphBatch's maxima."""
    dev, rows = nn.device, int(nn.numel())
    node_ptr64 = torch.zeros(rows + 1, dtype=torch.int64, device=dev); torch.cumsum(nn, 0, dtype=torch.int64, out=node_ptr64[1:])
    edge_ptr = torch.zeros(rows + 1, dtype=torch.int64, device=dev); torch.cumsum(ne, 0, dtype=torch.int64, out=edge_ptr[1:])
    N, E = torch.stack([node_ptr64[-1], edge_ptr[-1]]).tolist()            # the read-back of the two totals
    if N + rows >= 2 ** 31:
        raise ValueError("batch too large for int32 node offsets; shard it")
    o = launch(node_ptr64.to(torch.int32), edge_ptr, N, E)
    v = o["info"].tolist()                                                  # ... and of info
    if v[0]:
        raise _lib.GtokError(f"{what}: {v[0]} rows changed between the two passes")
    b = GraphBatch(rows, v[2], v[3], o["node_ptr"], o["edge_ptr"], o["rowptr"], o["col"], o["eorder"] if v[7] else None, o["nattr"], o["eattr"],
                   0, v[4], v[5], v[1] if N else 0)
    if check_symmetric and E:
        if csr_check(b)["violations"] == 0:
            b.flags |= _lib.CSR_SIMPLE_SYMMETRIC
        b.checked = True
    return b


def sent_decode_sizes(ids: torch.Tensor, ln: torch.Tensor, max_num_nodes: int, labeled: bool = False, num_node_types: int = 0,
                      row_start: Optional[torch.Tensor] = None, ld: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """gtok_sent_decode_sizes: (num_nodes, num_entries, status) int32 [rows] of un-remapped SENT rows - the sizes of the graphs
    sent_decode_csr builds (a status-1 row: 0, 0).  ids / row_start / ld as there.  Nothing is read back."""
    eb, ld, rows = _decode_rows(ids, ln, row_start, ld, "sent_decode_sizes")
    _need(_lib.DECODE_CSR_SYMBOLS, "gtok_sent_decode_sizes / gtok_sent_decode_csr")
    dev = ids.device
    nn, ne, st = (torch.empty(rows, dtype=torch.int32, device=dev) for _ in range(3))
    if rows:
        check(lib().gtok_sent_decode_sizes(ids.data_ptr(), eb, None if row_start is None else row_start.data_ptr(), ld, ln.data_ptr(), rows,
                                           int(max_num_nodes), int(bool(labeled)), int(num_node_types), nn.data_ptr(), ne.data_ptr(),
                                           st.data_ptr(), _stream(dev)), "gtok_sent_decode_sizes")
    return nn, ne, st


def _decode_csr_launch(ids, ln, row_start, ld, max_num_nodes, labeled, num_node_types, node_ptr, edge_ptr, N: int, E: int) -> dict:
    """gtok_sent_decode_csr on the current stream into fresh arrays of the given totals: -> dict of gtok_csr_built's arrays
    (nattr / eattr None when unlabelled); no host read."""
    eb, ld, rows = _decode_rows(ids, ln, row_start, ld, "sent_decode_csr")
    _need(_lib.DECODE_CSR_SYMBOLS, "gtok_sent_decode_sizes / gtok_sent_decode_csr")
    dev = ids.device
    o, cout = _built_arrays("sent_decode_csr", dev, rows, N, E, labeled, labeled, node_ptr, edge_ptr)
    if rows == 0:
        return o
    ptr = lambda t: None if t is None else t.data_ptr()
    check(lib().gtok_sent_decode_csr(ids.data_ptr(), eb, ptr(row_start), ld, ln.data_ptr(), rows, int(max_num_nodes), int(bool(labeled)),
                                     int(num_node_types), ctypes.byref(cout), _stream(dev)), "gtok_sent_decode_csr")
    return o


def sent_decode_csr(ids: torch.Tensor, ln: torch.Tensor, max_num_nodes: int, labeled: bool = False, num_node_types: int = 0,
                    row_start: Optional[torch.Tensor] = None, check_symmetric: bool = False,
                    ld: Optional[int] = None) -> Tuple[GraphBatch, torch.Tensor]:
    """Un-remapped SENT rows -> (GraphBatch on the rows' device, status int32 [rows]): row r becomes graph r in visit-index
    space (node k = the k-th node the trail visited), every decoded edge listed in both directions, the arrays those of
    GraphBatch.from_coo over that list (include/gtok.h: gtok_sent_decode_sizes / gtok_sent_decode_csr).  status: 0 complete,
    1 malformed (an empty graph), 3 cut before EOS (the part that was read).
    ids: an int32 or int16 (16-bit ids) [rows, ld] slab, or - with row_start int64 [rows] - a flat uint8 / int16 / int32 buffer
    of packed rows (PackedRows.buf / .row_start, pack_rows_scan's packed / row_ptr; a negative start = an empty row; ld = the
    slab width the rows were cut at, when some len exceeds it).  Every row must lie inside `ids`: that is not checked.
    Two read-backs: the two totals after the sizing pass, `info` after the build.  check_symmetric: gtok_csr_check over the
    result sets CSR_SIMPLE_SYMMETRIC when every graph is simple (a third read-back); a batch without a single entry is left
    unflagged and unchecked, as GraphBatch.from_coo leaves it."""
    nn, ne, status = sent_decode_sizes(ids, ln, max_num_nodes, labeled, num_node_types, row_start, ld)
    launch = lambda node_ptr, edge_ptr, N, E: _decode_csr_launch(ids, ln, row_start, ld, max_num_nodes, labeled, num_node_types, node_ptr, edge_ptr, N, E)
    return _decoded_batch("sent_decode_csr", nn, ne, launch, check_symmetric), status


# ------------------------------------------------------------------------------------------------
# ZINC-remapped SENT rows -> ids / CSR (include/gtok.h: gtok_unremap_zinc, gtok_sent_decode_zinc_sizes / gtok_sent_decode_zinc_csr)
# ------------------------------------------------------------------------------------------------
_ZINC_WHAT = "gtok_unremap_zinc / gtok_sent_decode_zinc_sizes / gtok_sent_decode_zinc_csr"


def unremap_zinc(ids: torch.Tensor, ln: torch.Tensor, max_num_nodes: int, num_node_types: int, row_start: Optional[torch.Tensor] = None,
                 ld: Optional[int] = None, pad_id: int = SENT_PAD) -> torch.Tensor:
    """gtok_unremap_zinc: ZINC-remapped labelled SENT rows (sent(..., remap_zinc=True)) -> int32 [rows, ld], row r its first
    min(len, ld) ids UNFOLDED to the raw ids of the same walk (include/gtok.h: the rule), pad_id behind them.  max_num_nodes /
    num_node_types: the walk's own.  ids / row_start as sent_decode_csr; with row_start (packed rows) ld - the width of the
    result - must be given.  Only the last id of a row that a cut leaves ending in the folded id can differ from the walk's raw
    row (RESET where it wrote LADJ).  Nothing is read back."""
    if row_start is not None and ld is None:
        raise ValueError("unremap_zinc: with row_start, ld (the width of the result) must be given")
    eb, ld, rows = _decode_rows(ids, ln, row_start, ld, "unremap_zinc")
    _need(_lib.ZINC_DECODE_SYMBOLS, _ZINC_WHAT)
    out = torch.empty((rows, ld), dtype=torch.int32, device=ids.device)
    if rows:
        check(lib().gtok_unremap_zinc(ids.data_ptr(), eb, None if row_start is None else row_start.data_ptr(), ld, ln.data_ptr(), rows,
                                      int(max_num_nodes), int(num_node_types), int(pad_id), out.data_ptr(), _stream(ids.device)),
              "gtok_unremap_zinc")
    return out


def sent_decode_zinc_sizes(ids: torch.Tensor, ln: torch.Tensor, max_num_nodes: int, num_node_types: int,
                           row_start: Optional[torch.Tensor] = None, ld: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """gtok_sent_decode_zinc_sizes: sent_decode_sizes for ZINC-remapped labelled rows."""
    eb, ld, rows = _decode_rows(ids, ln, row_start, ld, "sent_decode_zinc_sizes")
    _need(_lib.ZINC_DECODE_SYMBOLS, _ZINC_WHAT)
    dev = ids.device
    nn, ne, st = (torch.empty(rows, dtype=torch.int32, device=dev) for _ in range(3))
    if rows:
        check(lib().gtok_sent_decode_zinc_sizes(ids.data_ptr(), eb, None if row_start is None else row_start.data_ptr(), ld, ln.data_ptr(), rows,
                                                int(max_num_nodes), int(num_node_types), nn.data_ptr(), ne.data_ptr(), st.data_ptr(),
                                                _stream(dev)), "gtok_sent_decode_zinc_sizes")
    return nn, ne, st


def _decode_zinc_csr_launch(ids, ln, row_start, ld, max_num_nodes, num_node_types, node_ptr, edge_ptr, N: int, E: int) -> dict:
    """gtok_sent_decode_zinc_csr on the current stream into fresh arrays of the given totals: -> dict of gtok_csr_built's arrays;
    no host read."""
    eb, ld, rows = _decode_rows(ids, ln, row_start, ld, "sent_decode_zinc_csr")
    _need(_lib.ZINC_DECODE_SYMBOLS, _ZINC_WHAT)
    dev = ids.device
    o, cout = _built_arrays("sent_decode_zinc_csr", dev, rows, N, E, True, True, node_ptr, edge_ptr)
    if rows == 0:
        return o
    check(lib().gtok_sent_decode_zinc_csr(ids.data_ptr(), eb, None if row_start is None else row_start.data_ptr(), ld, ln.data_ptr(), rows,
                                          int(max_num_nodes), int(num_node_types), ctypes.byref(cout), _stream(dev)),
          "gtok_sent_decode_zinc_csr")
    return o


def sent_decode_zinc_csr(ids: torch.Tensor, ln: torch.Tensor, max_num_nodes: int, num_node_types: int,
                         row_start: Optional[torch.Tensor] = None, check_symmetric: bool = False,
                         ld: Optional[int] = None) -> Tuple[GraphBatch, torch.Tensor]:
    """ZINC-remapped labelled SENT rows (sent(..., remap_zinc=True): what every ZINC run trains on) -> (GraphBatch, status int32
    [rows]): sent_decode_csr over the unfolded rows (unremap_zinc), the unfold done in registers while the row is parsed.  The
    result is that of sent_decode_csr over the raw rows of the same walk; a damaged row decodes as its unfolded ids do.  Ids behind
    EOS (a query tail) are not parsed.  ids / row_start / ld / check_symmetric and the read-backs as sent_decode_csr."""
    nn, ne, status = sent_decode_zinc_sizes(ids, ln, max_num_nodes, num_node_types, row_start, ld)
    launch = lambda node_ptr, edge_ptr, N, E: _decode_zinc_csr_launch(ids, ln, row_start, ld, max_num_nodes, num_node_types, node_ptr, edge_ptr, N, E)
    return _decoded_batch("sent_decode_zinc_csr", nn, ne, launch, check_symmetric), status


# ------------------------------------------------------------------------------------------------
# IBTT rows -> CSR (include/gtok.h: gtok_ibtt_decode_sizes / gtok_ibtt_decode_csr)
# ------------------------------------------------------------------------------------------------
IBTT_GRAMMARS = {"zinc": _lib.IBTT_GRAMMAR_ZINC, "synth": _lib.IBTT_GRAMMAR_SYNTH}


def _ibtt_grammar(grammar) -> int:
    g = IBTT_GRAMMARS.get(grammar, grammar)
    if g not in (_lib.IBTT_GRAMMAR_ZINC, _lib.IBTT_GRAMMAR_SYNTH):
        raise ValueError("grammar is 'zinc' / 'synth' (or GTOK_IBTT_GRAMMAR_ZINC / _SYNTH)")
    return int(g)


def ibtt_inverse_lut(lut, vocab_size: int, pad_id: Optional[int] = None) -> torch.Tensor:
    """The vocab of the IBTT decoder, built on the host from the LUT the rows were tokenized with (zinc_lut / synth_lut):
    int32 [vocab_size], inv[id] = the LUT slot that holds id, -1 for an id no slot holds AND for an id that two slots share
    (vocab['<pad>'] when tokens are absent from the vocab: such an id names no token).  pad_id: that id, -1 whatever holds it (one
    absent token alone would otherwise own it).  LUT ids outside [0, vocab_size) have no entry.  A host tensor; ibtt_decode_*
    move it to the rows' device."""
    lut = np.asarray(lut.cpu() if isinstance(lut, torch.Tensor) else lut, dtype=np.int64).reshape(-1)
    vocab_size = int(vocab_size)
    if vocab_size < 1:
        raise ValueError("vocab_size must be positive")
    inv = np.full(vocab_size, -1, np.int32)
    ok = (lut >= 0) & (lut < vocab_size)
    owners = np.bincount(lut[ok], minlength=vocab_size)
    slots = np.nonzero(ok)[0]
    inv[lut[slots]] = slots
    inv[owners != 1] = -1
    if pad_id is not None and 0 <= int(pad_id) < vocab_size:
        inv[int(pad_id)] = -1
    return torch.from_numpy(inv)


def _ibtt_inv(inv: torch.Tensor, dev) -> torch.Tensor:
    if inv.dim() != 1 or inv.numel() < 1:
        raise ValueError("inv is a non-empty int32 vector (ibtt_inverse_lut)")
    return inv.to(dev, dtype=torch.int32).contiguous()


def ibtt_decode_sizes(ids: torch.Tensor, ln: torch.Tensor, grammar, inv: torch.Tensor, max_num_nodes: int,
                      row_start: Optional[torch.Tensor] = None, ld: Optional[int] = None, with_query: bool = False):
    """gtok_ibtt_decode_sizes: (num_nodes, num_entries, status) int32 [rows] of IBTT rows - the sizes of the graphs
    ibtt_decode_csr builds (a status-1 row: 0, 0) - and, with_query (graph-token rows), query int32 [rows, 4].  ids / row_start /
    ld as sent_decode_csr.  Nothing is read back."""
    eb, ld, rows = _decode_rows(ids, ln, row_start, ld, "ibtt_decode_sizes")
    _need(_lib.IBTT_DECODE_SYMBOLS, "gtok_ibtt_decode_sizes / gtok_ibtt_decode_csr")
    g = _ibtt_grammar(grammar)
    dev = ids.device
    inv = _ibtt_inv(inv, dev)
    nn, ne, st = (torch.empty(rows, dtype=torch.int32, device=dev) for _ in range(3))
    query = torch.zeros((rows, 4), dtype=torch.int32, device=dev) if with_query else None
    if rows:
        check(lib().gtok_ibtt_decode_sizes(ids.data_ptr(), eb, None if row_start is None else row_start.data_ptr(), ld, ln.data_ptr(), rows,
                                           g, inv.data_ptr(), inv.numel(), int(max_num_nodes), nn.data_ptr(), ne.data_ptr(), st.data_ptr(),
                                           query.data_ptr() if with_query and g == _lib.IBTT_GRAMMAR_SYNTH else None, _stream(dev)),
              "gtok_ibtt_decode_sizes")
    return (nn, ne, st, query) if with_query else (nn, ne, st)


def _ibtt_decode_csr_launch(ids, ln, row_start, ld, grammar, inv, max_num_nodes, node_ptr, edge_ptr, N: int, E: int) -> dict:
    """gtok_ibtt_decode_csr on the current stream into fresh arrays of the given totals: -> dict of gtok_csr_built's arrays
    (nattr / eattr None for graph-token rows); no host read."""
    eb, ld, rows = _decode_rows(ids, ln, row_start, ld, "ibtt_decode_csr")
    _need(_lib.IBTT_DECODE_SYMBOLS, "gtok_ibtt_decode_sizes / gtok_ibtt_decode_csr")
    g = _ibtt_grammar(grammar)
    dev = ids.device
    inv = _ibtt_inv(inv, dev)
    typed = g == _lib.IBTT_GRAMMAR_ZINC
    o, cout = _built_arrays("ibtt_decode_csr", dev, rows, N, E, typed, typed, node_ptr, edge_ptr)
    if rows == 0:
        return o
    ptr = lambda t: None if t is None else t.data_ptr()
    check(lib().gtok_ibtt_decode_csr(ids.data_ptr(), eb, ptr(row_start), ld, ln.data_ptr(), rows, g, inv.data_ptr(), inv.numel(),
                                     int(max_num_nodes), ctypes.byref(cout), _stream(dev)), "gtok_ibtt_decode_csr")
    return o


def ibtt_decode_csr(ids: torch.Tensor, ln: torch.Tensor, grammar, inv: torch.Tensor, max_num_nodes: int,
                    row_start: Optional[torch.Tensor] = None, ld: Optional[int] = None, check_symmetric: bool = False):
    """IBTT rows -> (GraphBatch on the rows' device, status int32 [rows]) for grammar 'zinc', plus query int32 [rows, 4] for
    grammar 'synth': row r becomes graph r in the input's own node numbering and edge order (include/gtok.h:
    gtok_ibtt_decode_sizes / gtok_ibtt_decode_csr).  status: 0 complete, 1 malformed (an empty graph), 3 a well-formed prefix
    (the part that was read).  inv: ibtt_inverse_lut of the LUT the rows were tokenized with.  ids / row_start / ld as
    sent_decode_csr; every row must lie inside `ids`: that is not checked.  Two read-backs: the two totals after the sizing
    pass, `info` after the build; check_symmetric as sent_decode_csr (a third)."""
    g = _ibtt_grammar(grammar)
    synth = g == _lib.IBTT_GRAMMAR_SYNTH
    sizes = ibtt_decode_sizes(ids, ln, g, inv, max_num_nodes, row_start, ld, with_query=synth)
    nn, ne, status = sizes[:3]
    launch = lambda node_ptr, edge_ptr, N, E: _ibtt_decode_csr_launch(ids, ln, row_start, ld, g, inv, max_num_nodes, node_ptr, edge_ptr, N, E)
    b = _decoded_batch("ibtt_decode_csr", nn, ne, launch, check_symmetric)
    return (b, status, sizes[3]) if synth else (b, status)


# ------------------------------------------------------------------------------------------------
# a batched CSR in another numbering (include/gtok.h: gtok_csr_relabel), graph equality
# ------------------------------------------------------------------------------------------------
_RELABEL_WS = {}


def _relabel_launch(batch: GraphBatch, old_of_new: torch.Tensor, target_node_ptr: torch.Tensor, target_max_nodes: int, total: int) -> dict:
    """gtok_csr_relabel on the current stream into fresh arrays: -> dict(rowptr, col, eorder, nattr, eattr, info, status); no host read."""
    _need_gpu(batch.col, "csr_relabel")
    _need(_lib.ORDER_SYMBOLS, "gtok_sent_large_order / gtok_csr_relabel")
    dev, G, E = batch.device, batch.num_graphs, batch.num_edges_total
    total = int(total)
    if old_of_new.dtype != torch.int32 or old_of_new.dim() != 1 or not old_of_new.is_contiguous() or old_of_new.device != dev \
            or int(old_of_new.numel()) != total:
        raise ValueError("csr_relabel: old_of_new must be a contiguous int32 vector of one entry per target node on the batch's device")
    if target_node_ptr.dtype != torch.int32 or target_node_ptr.numel() != G + 1 or not target_node_ptr.is_contiguous() or target_node_ptr.device != dev:
        raise ValueError("csr_relabel: target_node_ptr must be a contiguous int32 [G + 1] on the batch's device")
    o, cout = _built_arrays("csr_relabel", dev, G, total, E, batch.nattr is not None, batch.eattr is not None, status=True)
    if G == 0:
        return o
    need = int(lib().gtok_csr_relabel_workspace(G, E))
    if need < 0:
        check(need, "gtok_csr_relabel_workspace")
    key = torch.device(dev).index or 0
    ws = _RELABEL_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _RELABEL_WS[key] = torch.empty(max(16, need), dtype=torch.uint8, device=dev)
    cs = batch.c_struct()
    oon = old_of_new if total else torch.empty(1, dtype=torch.int32, device=dev)
    check(lib().gtok_csr_relabel(ctypes.byref(cs), target_node_ptr.data_ptr(), int(target_max_nodes), oon.data_ptr(), ctypes.byref(cout),
                                 o["status"].data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)), "gtok_csr_relabel")
    return o


def csr_relabel(batch: GraphBatch, old_of_new: torch.Tensor, target_node_ptr: Optional[torch.Tensor] = None,
                target_max_nodes: Optional[int] = None) -> Tuple[GraphBatch, torch.Tensor]:
    """gtok_csr_relabel: `batch` renumbered through a per-graph node map -> (GraphBatch, status int32 [G]).  old_of_new int32
    [target total]: the old id of target node t of graph g at target_node_ptr[g] + t, anything outside [0, N_old) = absent (such a
    node comes out isolated, type 255) - a visit_index slice of ops.sent_order when `batch` was decoded from SENT rows.
    target_node_ptr int32 [G + 1] (None: the batch's own node_ptr), target_max_nodes: a bound on the target node counts (None: read
    from target_node_ptr, one host read).  Rows come out in ascending new column, duplicates in input order; eorder = every entry's
    local index in the old graph's entry list.  status: 0 built, 2 built but not simple (a duplicate or a self loop), 1 skipped (the
    map names an old node twice or not at all, damaged arrays: the graph's arrays are undefined).  One read-back (`info`): the
    returned batch carries its maxima, as ops.sent_decode_csr sets them."""
    dev = batch.device
    old_of_new = old_of_new.to(dev, dtype=torch.int32).contiguous().reshape(-1)
    if target_node_ptr is None:
        target_node_ptr = batch.node_ptr
        if target_max_nodes is None:
            target_max_nodes = batch.max_nodes
    else:
        target_node_ptr = target_node_ptr.to(dev, dtype=torch.int32).contiguous()
        if target_max_nodes is None:
            target_max_nodes = int((target_node_ptr[1:] - target_node_ptr[:-1]).max()) if batch.num_graphs else 0
    total = int(old_of_new.numel())
    o = _relabel_launch(batch, old_of_new, target_node_ptr, target_max_nodes, total)
    v = o["info"].tolist()
    b = GraphBatch(batch.num_graphs, v[2], v[3], target_node_ptr, batch.edge_ptr, o["rowptr"], o["col"], o["eorder"], o["nattr"], o["eattr"],
                   0, v[4], v[5], v[1])
    if batch.num_graphs and batch.num_edges_total and v[0] == 0 and v[6] == 0 and (batch.flags & _lib.CSR_SIMPLE_SYMMETRIC):
        b.flags |= _lib.CSR_SIMPLE_SYMMETRIC          # (a renumbering keeps a verified simple symmetric batch simple and symmetric)
        b.checked = batch.checked
    return b, o["status"]


def graphs_equal(a: GraphBatch, b: GraphBatch) -> torch.Tensor:
    """bool [G]: graph g of `a` and of `b` have the same node and entry counts and equal rowptr / col / nattr / eattr slices (an
    attribute array only one of the two has: unequal wherever a node / an entry exists).  Two graphs in one numbering and in
    ops.csr_relabel's canonical entry order are the same graph iff this says so.  Torch segment reductions on the device; the result stays there."""
    if a.num_graphs != b.num_graphs:
        raise ValueError("graphs_equal: batches of different graph counts")
    dev, G = a.device, a.num_graphs
    if b.device != dev:
        raise ValueError("graphs_equal: batches on different devices")
    na, nb_ = a.node_ptr[1:] - a.node_ptr[:-1], b.node_ptr[1:] - b.node_ptr[:-1]
    ea, eb = a.edge_ptr[1:] - a.edge_ptr[:-1], b.edge_ptr[1:] - b.edge_ptr[:-1]
    same = (na == nb_) & (ea == eb)
    if G == 0:
        return same
    gid = torch.arange(G, device=dev)
    n64, e64 = na.to(torch.int64), ea.to(torch.int64)

    def segments(x, y, counts_a, ptr_a, ptr_b, extra):
        """per graph: no element of x's slice differs from y's (compared where the counts agree: indices built from a's pointers)"""
        cnt = torch.where(same, counts_a + extra, torch.zeros_like(counts_a))
        seg = torch.repeat_interleave(gid, cnt)
        start = torch.cumsum(cnt, 0) - cnt
        local = torch.arange(seg.numel(), device=dev) - start[seg]
        ia = ptr_a.to(torch.int64)[seg] + (seg if extra else 0) + local
        ib = ptr_b.to(torch.int64)[seg] + (seg if extra else 0) + local
        diff = (x[ia] != y[ib]).to(torch.int32)
        bad = torch.zeros(G, dtype=torch.int32, device=dev)
        bad.index_add_(0, seg, diff)
        return bad == 0

    same = same & segments(a.rowptr, b.rowptr, n64, a.node_ptr, b.node_ptr, 1)
    same = same & segments(a.col, b.col, e64, a.edge_ptr, b.edge_ptr, 0)
    for xa, xb, cnt, pa, pb in ((a.nattr, b.nattr, n64, a.node_ptr, b.node_ptr), (a.eattr, b.eattr, e64, a.edge_ptr, b.edge_ptr)):
        if xa is None and xb is None:
            continue
        if xa is None or xb is None:
            same = same & (cnt == 0)
        else:
            same = same & segments(xa, xb, cnt, pa, pb, 0)
    return same


# ------------------------------------------------------------------------------------------------
# the task answers of a batch (include/gtok.h: gtok_graph_tasks): cycle check, components, shortest-path distances
# ------------------------------------------------------------------------------------------------
TASKS_MAX_NODES_ANY = 512      # beyond it gtok_graph_tasks searches the CSR itself and needs GTOK_CSR_SIMPLE_SYMMETRIC
TASKS_BAD_QUERY, TASKS_DAMAGED = 1, 2       # info[0] bits


class GraphTasks:
    """What ops.graph_tasks returns, all device tensors: has_cycle int32 [G] (1 / 0), num_components int32 [G], dist int32 [Q] (None
    without queries; -1 unreachable, -2 an endpoint outside its graph), info int32 [4].  Nothing is read back unless status() is
    called."""
    __slots__ = ("has_cycle", "num_components", "dist", "info")

    def __init__(self, has_cycle, num_components, dist, info):
        self.has_cycle, self.num_components, self.dist, self.info = has_cycle, num_components, dist, info

    def status(self) -> Dict[str, int]:
        """One 16-byte read-back of info: status bits (TASKS_BAD_QUERY, TASKS_DAMAGED), the largest distance, the queries answered
        -1, the graphs with a cycle."""
        v = self.info.tolist()
        return dict(status=v[0], max_dist=v[1], unreachable=v[2], cycles=v[3])


def _graph_tasks_launch(batch: GraphBatch, queries: Optional[torch.Tensor], query_ptr: Optional[torch.Tensor], has_cycle: bool = True,
                        num_components: bool = True):
    """gtok_graph_tasks on the current stream into fresh arrays -> (has_cycle, num_components, dist, info), None for what was not
    asked for; no host read."""
    _need_gpu(batch.col, "graph_tasks")
    _need(_lib.GRAPH_TASKS_SYMBOLS, "gtok_graph_tasks")
    dev, G = batch.device, batch.num_graphs
    if batch.max_nodes > _lib.SENT_LARGE_MAX_NODES:
        raise _lib.GtokError(f"graph_tasks: a graph of {batch.max_nodes} nodes is beyond the {_lib.SENT_LARGE_MAX_NODES} the search holds in LDS "
                             "(GTOK_E_TOO_LARGE)")
    if batch.max_nodes > TASKS_MAX_NODES_ANY and not (batch.flags & _lib.CSR_SIMPLE_SYMMETRIC):
        raise _lib.GtokError(f"graph_tasks: graphs of more than {TASKS_MAX_NODES_ANY} nodes (this batch: {batch.max_nodes}) are searched over the CSR "
                             "itself, which must list every edge once in each direction, without loops: the batch does not carry "
                             "GTOK_CSR_SIMPLE_SYMMETRIC (build it with check_symmetric=True from a both-directions edge list) (GTOK_E_UNSUPPORTED)")
    if batch.graph_ids is not None:
        raise ValueError("graph_tasks: a batch in dataset order only (not ops.lane_sorted's copy)")
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    cyc, comp = (i32(G) if has_cycle else None), (i32(G) if num_components else None)
    info = torch.zeros(4, dtype=torch.int32, device=dev)
    dist = None
    if queries is None:
        if query_ptr is not None:
            raise ValueError("graph_tasks: query_ptr without queries")
        Q = 0
    else:
        queries = queries.to(dev, dtype=torch.int32).contiguous()
        if queries.dim() != 2 or queries.shape[1] != 2:
            raise ValueError("graph_tasks: queries must be [Q, 2] (local node ids)")
        Q = int(queries.shape[0])
        if query_ptr is None:
            if Q != G:
                raise ValueError(f"graph_tasks: without query_ptr there is exactly one query per graph ({G}), got {Q}")
        else:
            query_ptr = query_ptr.to(dev, dtype=torch.int64).contiguous().reshape(-1)
            if int(query_ptr.numel()) != G + 1:
                raise ValueError("graph_tasks: query_ptr must be [G + 1]")
        if G == 0 and Q:
            raise ValueError("graph_tasks: queries but no graphs")
        dist = i32(Q)
    if G == 0 or not (has_cycle or num_components or queries is not None):
        return cyc, comp, dist, info
    p = lambda t: None if t is None else t.data_ptr()
    qn = queries if (queries is None or Q) else torch.empty((1, 2), dtype=torch.int32, device=dev)    # (an empty tensor's pointer may be null)
    dd = dist if (dist is None or Q) else i32(1)
    cs = batch.c_struct()
    check(lib().gtok_graph_tasks(ctypes.byref(cs), p(qn), p(query_ptr), Q, p(cyc), p(comp), p(dd), info.data_ptr(), _stream(dev)),
          "gtok_graph_tasks")
    return cyc, comp, dist, info


def graph_tasks(batch: GraphBatch, queries: Optional[torch.Tensor] = None, query_ptr: Optional[torch.Tensor] = None,
                has_cycle: bool = True, num_components: bool = True) -> GraphTasks:
    """gtok_graph_tasks: the answers of the two graph-token tasks for every graph of the batch, on the device -> GraphTasks.  The
    graph of a CSR slice is the simple undirected closure of its entries (one direction or both, duplicates and self loops allowed up
    to 512 nodes; larger graphs need a GTOK_CSR_SIMPLE_SYMMETRIC batch).  queries int32 [Q, 2] local node ids, graph g's at
    query_ptr[g] .. query_ptr[g + 1] (int64 [G + 1]; None: one per graph, the tensor ops.sent(query=) takes).  Labels of the
    reference are host arithmetic on top: `lenK` <-> dist - 1, dist <= 0 = the item is dropped."""
    return GraphTasks(*_graph_tasks_launch(batch, queries, query_ptr, has_cycle, num_components))


def check_task_labels(batch: GraphBatch, task: str, labels: torch.Tensor, query_nodes: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bool [G]: records whose stored label disagrees with their graph - the device version of the reference's consistency script
    (test/data_distribution_test.py:136-140) behind ops.parse_graph_texts -> GraphBatch.from_coo_device.  labels int32 [G] in
    gtok_parse_graph_text's conventions: cycle_check 1 / 0, shortest_path K - 1 for `lenK`; NO_LABEL = none, never a disagreement.
    query_nodes int32 [G, 2] (shortest_path), (-1, -1) = none, never a disagreement; a labelled pair that is unreachable, equal or
    outside its graph disagrees with any label."""
    if task not in ("cycle_check", "shortest_path"):
        raise ValueError('task must be "cycle_check" or "shortest_path"')
    dev = batch.device
    labels = labels.to(dev, dtype=torch.int32).reshape(-1)
    if int(labels.numel()) != batch.num_graphs:
        raise ValueError("check_task_labels: one label per graph")
    has = labels != NO_LABEL
    if task == "cycle_check":
        r = graph_tasks(batch, num_components=False)
        return has & (r.has_cycle != labels)
    if query_nodes is None:
        raise ValueError("check_task_labels: shortest_path needs query_nodes [G, 2]")
    query_nodes = query_nodes.to(dev, dtype=torch.int32).reshape(-1, 2)
    r = graph_tasks(batch, query_nodes, has_cycle=False, num_components=False)
    asked = ~((query_nodes[:, 0] == -1) & (query_nodes[:, 1] == -1))
    return has & asked & ((r.dist - 1) != labels)


# ------------------------------------------------------------------------------------------------
# a key per graph, duplicate graphs, split leakage (include/gtok.h: gtok_graph_keys)
# ------------------------------------------------------------------------------------------------
KEYS_MAX_NODES_ANY = 512       # beyond it closure keys stream the CSR itself and need GTOK_CSR_SIMPLE_SYMMETRIC
KEYS_DAMAGED = 2               # info[0] bit
_KEY_MODES = {"listed": _lib.KEYS_LISTED, "closure": _lib.KEYS_CLOSURE}


def _keys_flags(batches, mode: str, attrs: bool) -> int:
    """GTOK_KEYS_* of (mode, attrs); the argument errors that need no device"""
    if mode not in _KEY_MODES:
        raise ValueError('graph_keys: mode must be "listed" or "closure"')
    if attrs and mode == "closure":
        raise ValueError("graph_keys: closure keys are structure only - attrs=True goes with mode=\"listed\" (GTOK_E_INVAL)")
    for b in batches:
        if attrs and (b.nattr is None or b.eattr is None):
            raise ValueError("graph_keys: attrs=True needs a batch with node and edge attributes (GTOK_E_INVAL)")
        if b.graph_ids is not None:
            raise ValueError("graph_keys: a batch in dataset order only (not ops.lane_sorted's copy)")
    return _KEY_MODES[mode] | (_lib.KEYS_ATTRS if attrs else 0)


def _labels_of(batch: GraphBatch, labels, dev) -> Optional[torch.Tensor]:
    if labels is None:
        return None
    labels = torch.as_tensor(labels).to(dev, dtype=torch.int32).contiguous().reshape(-1)
    if int(labels.numel()) != batch.num_graphs:
        raise ValueError("graph_keys: one label per graph")
    return labels


def _graph_keys_launch(batch: GraphBatch, labels: Optional[torch.Tensor], flags: int, info: Optional[torch.Tensor] = None):
    """gtok_graph_keys on the current stream -> (keys int64 [G, 2], info int32 [4]); no host read."""
    _need_gpu(batch.col, "graph_keys")
    _need(_lib.GRAPH_KEYS_SYMBOLS, "gtok_graph_keys")
    dev, G = batch.device, batch.num_graphs
    if batch.max_nodes > _lib.SENT_LARGE_MAX_NODES:
        raise _lib.GtokError(f"graph_keys: a graph of {batch.max_nodes} nodes is beyond the {_lib.SENT_LARGE_MAX_NODES} whose ids fit a key's "
                             "14-bit fields (GTOK_E_TOO_LARGE)")
    if (flags & _lib.KEYS_CLOSURE) and batch.max_nodes > KEYS_MAX_NODES_ANY and not (batch.flags & _lib.CSR_SIMPLE_SYMMETRIC):
        raise _lib.GtokError(f"graph_keys: closure keys of graphs of more than {KEYS_MAX_NODES_ANY} nodes (this batch: {batch.max_nodes}) are read "
                             "off the CSR itself, which must list every edge once in each direction, without loops: the batch does not "
                             "carry GTOK_CSR_SIMPLE_SYMMETRIC (GTOK_E_UNSUPPORTED)")
    labels = _labels_of(batch, labels, dev)
    if info is None:
        info = torch.zeros(4, dtype=torch.int32, device=dev)
    elif info.dtype != torch.int32 or info.numel() != 4 or info.device != dev or not info.is_contiguous():
        raise ValueError("graph_keys: info must be int32 [4] on the batch's device")
    keys = torch.empty((G, 2), dtype=torch.int64, device=dev)
    if G == 0:
        return keys, info
    cs = batch.c_struct()
    check(lib().gtok_graph_keys(ctypes.byref(cs), None if labels is None else labels.data_ptr(), flags, keys.data_ptr(), info.data_ptr(),
                                _stream(dev)), "gtok_graph_keys")
    return keys, info


def graph_keys(batch: GraphBatch, labels: Optional[torch.Tensor] = None, mode: str = "listed", attrs: bool = False,
               info: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gtok_graph_keys: a 128-bit key per graph -> int64 [G, 2] on the device (the two uint64 words, bit for bit).  mode "listed": the
    reference's key (test/train_performance_test.py:70-74) - all listed entries with their endpoints sorted, duplicates and loops
    counting, N and the label; attrs=True adds the edge and node attribute bytes (ZINC).  mode "closure": the key of the simple
    undirected closure - a once-listed, a both-directions and a messy listing of one graph share it (beyond 512 nodes: a
    GTOK_CSR_SIMPLE_SYMMETRIC batch).  A key identifies a NUMBERED graph, not an isomorphism class, and equal keys only make equal
    graphs overwhelmingly likely: ops.duplicate_graphs(confirm=True) compares.  labels int32 [G] or None; info: an int32 [4] tensor of
    the caller's to accumulate the status into (bit KEYS_DAMAGED, the damaged graphs), else it is dropped."""
    flags = _keys_flags([batch], mode, attrs)
    return _graph_keys_launch(batch, labels, flags, info)[0]


class Duplicates:
    """What ops.duplicate_graphs returns - device tensors over the concatenation of the splits: group int64 [T] (the index of the first
    graph of graph i's class), split int64 [T], is_first bool [T]; split_ptr: the splits' offsets (host ints)."""
    __slots__ = ("group", "split", "is_first", "split_ptr")

    def __init__(self, group, split, is_first, split_ptr):
        self.group, self.split, self.is_first, self.split_ptr = group, split, is_first, list(split_ptr)

    @property
    def num_splits(self) -> int:
        return len(self.split_ptr) - 1

    def _presence(self):
        """(bool [classes, S]: the class has a member in the split; int64 [T]: the class of every graph)"""
        heads, cls = torch.unique(self.group, return_inverse=True)
        P = torch.zeros((int(heads.numel()), self.num_splits), dtype=torch.bool, device=self.group.device)
        P[cls, self.split] = True
        return P, cls

    def unique_per_split(self) -> torch.Tensor:
        """int64 [S]: the distinct graphs of every split (the reference's len(hashes[split]))"""
        return self._presence()[0].sum(0)

    def overlap(self) -> torch.Tensor:
        """int64 [S, S]: the classes present in both splits (the reference's len(hashes[a] & hashes[b])); the diagonal = unique_per_split"""
        P, _ = self._presence()
        if self.num_splits == 0:
            return torch.zeros((0, 0), dtype=torch.int64, device=P.device)
        return torch.stack([(P & P[:, a:a + 1]).sum(0) for a in range(self.num_splits)])

    def leaked(self, a: int, b: int) -> torch.Tensor:
        """int64: the graphs of split b (indices inside split b) whose class occurs in split a"""
        P, cls = self._presence()
        hit = (self.split == b) & P[cls, a]
        return hit.nonzero().reshape(-1) - self.split_ptr[b]


def _group_by_keys(keys: torch.Tensor) -> torch.Tensor:
    """group[i] = the lowest index with graph i's key: two stable sorts of the key columns, then head flags"""
    T = int(keys.shape[0])
    ar = torch.arange(T, device=keys.device)
    if T == 0:
        return ar
    o1 = torch.sort(keys[:, 1], stable=True).indices
    order = o1[torch.sort(keys[o1, 0], stable=True).indices]
    ks = keys[order]
    head = torch.ones(T, dtype=torch.bool, device=keys.device)
    head[1:] = (ks[1:] != ks[:-1]).any(1)
    head_pos = torch.cummax(torch.where(head, ar, torch.zeros_like(ar)), 0).values
    group = torch.empty_like(ar)
    group[order] = order[head_pos]
    return group


def _canonical_lists(bl, ptr, gs: torch.Tensor, closure: bool, attrs: bool, rank=None):
    """The canonical folded entry lists of the graphs `gs` (sorted indices into the concatenation): (graph slot, a, b, t) packed into
    int64, sorted (closure: distinct) -> (vals = the packed (a, b, t), starts, counts per slot); with attrs also the node bytes the same
    way.  Torch gathers over the chosen graphs only.  rank (ops.isomorphic_duplicates): one int64 [N] per batch, a numbering of every
    graph's nodes that replaces the stored one - the entries are renumbered through it and, with attrs, kept DIRECTED (row, column:
    each direction of a symmetric listing carries its own byte) and the node bytes are laid out in the new numbering."""
    dev = gs.device
    K = int(gs.numel())
    packed, nvals = [], []
    for s, b in enumerate(bl):
        sel = ((gs >= ptr[s]) & (gs < ptr[s + 1])).nonzero().reshape(-1)
        if sel.numel() == 0:
            continue
        l = gs[sel] - ptr[s]
        nptr, eptr = b.node_ptr.to(torch.int64), b.edge_ptr
        nc = nptr[l + 1] - nptr[l]
        jn = torch.repeat_interleave(torch.arange(int(l.numel()), device=dev), nc)
        node_loc = torch.arange(int(jn.numel()), device=dev) - (torch.cumsum(nc, 0) - nc)[jn]
        rowidx = nptr[l][jn] + l[jn] + node_loc
        x = b.rowptr[rowidx].to(torch.int64)
        deg = (b.rowptr[rowidx + 1].to(torch.int64) - x).clamp(min=0)
        je = torch.repeat_interleave(torch.arange(int(jn.numel()), device=dev), deg)
        k = torch.arange(int(je.numel()), device=dev) - (torch.cumsum(deg, 0) - deg)[je]
        ent = eptr[l][jn][je] + x[je] + k
        u, c = node_loc[je], b.col[ent].to(torch.int64)
        t = b.eattr[ent].to(torch.int64) if attrs else torch.zeros_like(u)
        slot = sel[jn][je]
        if rank is not None:
            base = nptr[l][jn]
            u, c = rank[s][base + node_loc][je], rank[s][base[je] + c]
        lo, hi = (u, c) if rank is not None and attrs else (torch.minimum(u, c), torch.maximum(u, c))
        packed.append((((slot << 14 | lo) << 14 | hi) << 8) | t)
        if attrs:
            nv = b.nattr[nptr[l][jn] + node_loc].to(torch.int64)
            if rank is not None:              # node k of the new numbering: the node whose rank is k
                nv = torch.empty_like(nv).scatter_(0, (torch.cumsum(nc, 0) - nc)[jn] + rank[s][nptr[l][jn] + node_loc], nv)
            nvals.append(nv)
    vals = torch.sort(torch.cat(packed)).values if packed else torch.zeros(0, dtype=torch.int64, device=dev)
    if closure:
        vals = torch.unique_consecutive(vals)
    cnt = torch.bincount(vals >> 36, minlength=K)
    out = [(vals & ((1 << 36) - 1), torch.cumsum(cnt, 0) - cnt, cnt)]
    if attrs:
        nv = torch.cat(nvals) if nvals else torch.zeros(0, dtype=torch.int64, device=dev)
        n_all = torch.cat([b.node_counts().to(torch.int64) for b in bl])[gs]
        out.append((nv, torch.cumsum(n_all, 0) - n_all, n_all))
    return out


def _segments_equal(vals, starts, cnts, sa, sb) -> torch.Tensor:
    """bool [P]: the lists of slots sa[p] and sb[p] are equal"""
    same = cnts[sa] == cnts[sb]
    c = torch.where(same, cnts[sa], torch.zeros_like(cnts[sa]))
    P = int(sa.numel())
    pid = torch.repeat_interleave(torch.arange(P, device=sa.device), c)
    off = torch.arange(int(pid.numel()), device=sa.device) - (torch.cumsum(c, 0) - c)[pid]
    diff = (vals[starts[sa][pid] + off] != vals[starts[sb][pid] + off]).to(torch.int64)
    bad = torch.zeros(P, dtype=torch.int64, device=sa.device).index_add_(0, pid, diff)
    return same & (bad == 0)


def _confirm_groups(bl, ll, ptr, group: torch.Tensor, closure: bool, attrs: bool, budget_bytes: int) -> torch.Tensor:
    """Classes by key -> classes by the graphs themselves: every member of a class of two or more is compared with the class's first
    member - N, the label, the canonical entry list (and the node bytes) - in chunks of at most ~budget_bytes of gathered lists; the
    members that differ (a digest collision, or keys= that say nothing) leave the class, the first of them heads a new one and the
    others are compared with it in the next round."""
    dev, T = group.device, int(group.numel())
    ar = torch.arange(T, device=dev)
    n_all = torch.cat([b.node_counts().to(torch.int64) for b in bl])
    e_all = torch.cat([b.edge_ptr[1:] - b.edge_ptr[:-1] for b in bl])
    lab = torch.cat([torch.zeros(b.num_graphs, dtype=torch.int32, device=dev) if l is None else l for b, l in zip(bl, ll)])
    per_chunk = max(1, int(budget_bytes) // 64)              # ~8 int64 temporaries per gathered entry
    group = group.clone()
    pending = group != ar
    while True:
        mem = pending.nonzero().reshape(-1)
        if mem.numel() == 0:
            break
        heads = group[mem]
        ok = (n_all[mem] == n_all[heads]) & (lab[mem] == lab[heads])
        if not closure:
            ok &= e_all[mem] == e_all[heads]
        cost = e_all[mem] + e_all[heads] + (n_all[mem] + n_all[heads] if attrs else 0) + 1
        chunk = (torch.cumsum(cost, 0) - cost) // per_chunk
        sizes = torch.unique_consecutive(chunk, return_counts=True)[1].tolist()
        i0 = 0
        for sz in sizes:
            m, h = mem[i0:i0 + sz], heads[i0:i0 + sz]
            gs, inv = torch.unique(torch.cat([m, h]), return_inverse=True)
            eq = torch.ones(sz, dtype=torch.bool, device=dev)
            for vals, starts, cnts in _canonical_lists(bl, ptr, gs, closure, attrs):
                eq &= _segments_equal(vals, starts, cnts, inv[:sz], inv[sz:])
            ok[i0:i0 + sz] &= eq
            i0 += sz
        pending[mem[ok]] = False
        bad = mem[~ok]
        if bad.numel() == 0:
            break
        first_bad = torch.full((T,), T, dtype=torch.int64, device=dev).scatter_reduce_(0, group[bad], bad, "amin")
        group[bad] = first_bad[group[bad]]
        pending[bad] = group[bad] != bad
    return group


def duplicate_graphs(batches, labels=None, mode: str = "listed", attrs: bool = False, confirm: bool = True, keys=None,
                     budget_bytes: int = 256 << 20) -> Duplicates:
    """The classes of equal graphs of one batch or of a sequence of batches (the splits of a corpus), on the device -> Duplicates over
    their concatenation.  Two graphs are equal when the reference's key says so (ops.graph_keys: mode, attrs; labels: one tensor per
    batch, or None).  Keys come from gtok_graph_keys unless `keys` supplies them (int64 [T, 2], or one [G, 2] per batch); grouping is
    two stable sorts of the key columns.  confirm=True makes the answer exact, as the reference's set of tuples is: the members of
    every class of two or more are compared with the class's first member, and one that differs is re-grouped by the graphs
    themselves, never merged.  confirm=False trusts the 128 bits."""
    single = isinstance(batches, GraphBatch)
    bl = [batches] if single else list(batches)
    if not bl:
        raise ValueError("duplicate_graphs: no batch")
    if labels is None:
        ll = [None] * len(bl)
    else:
        ll = [labels] if single else list(labels)
        if len(ll) != len(bl):
            raise ValueError("duplicate_graphs: one label tensor (or None) per batch")
    flags = _keys_flags(bl, mode, attrs)
    dev = bl[0].device
    if any(b.device != dev for b in bl):
        raise ValueError("duplicate_graphs: batches on different devices")
    ll = [_labels_of(b, l, dev) for b, l in zip(bl, ll)]
    ptr = [0]
    for b in bl:
        ptr.append(ptr[-1] + b.num_graphs)
    T = ptr[-1]
    if keys is None:
        keys = torch.cat([_graph_keys_launch(b, l, flags)[0] for b, l in zip(bl, ll)])
    else:
        keys = torch.cat([torch.as_tensor(k).reshape(-1, 2) for k in keys]) if isinstance(keys, (list, tuple)) else torch.as_tensor(keys)
        keys = keys.to(dev, dtype=torch.int64)
        if tuple(keys.shape) != (T, 2):
            raise ValueError(f"duplicate_graphs: keys must be int64 [{T}, 2]")
    split = torch.repeat_interleave(torch.arange(len(bl), device=dev), torch.tensor([b.num_graphs for b in bl], device=dev))
    group = _group_by_keys(keys)
    if confirm and T:
        group = _confirm_groups(bl, ll, ptr, group, mode == "closure", attrs, budget_bytes)
    return Duplicates(group, split, group == torch.arange(T, device=dev), ptr)


def split_leakage(splits: Dict[str, object], mode: str = "listed", attrs: bool = False, confirm: bool = True) -> Dict[str, object]:
    """The reference's data-leakage report (test/train_performance_test.py:146-207, Test 2) for {"train": (batch, labels), ...} (a
    value may also be a batch alone), computed on the device with one small read-back:
      total / unique   {split: graphs, distinct graphs}           (`{split}: {unique} unique graphs (from {total} total)`)
      overlap          {(a, b): classes present in both}          for every pair a before b (train-val, train-test, val-test)
      example          {(a, b): (index in a, index in b) of one shared graph, or None}
      leakage          any overlap at all
      duplicates       the Duplicates object (device tensors)"""
    names = list(splits)
    vals = [v if isinstance(v, (tuple, list)) else (v, None) for v in splits.values()]
    dup = duplicate_graphs([v[0] for v in vals], [v[1] for v in vals], mode, attrs, confirm)
    S, T, dev = len(names), dup.split_ptr[-1], dup.group.device
    P, cls = dup._presence()
    ov = dup.overlap()
    ar = torch.arange(T, device=dev)
    pairs = [(a, b) for a in range(S) for b in range(a + 1, S)]
    ex = []
    for a, b in pairs:
        if T == 0:
            ex += [ar.new_tensor(0), ar.new_tensor(0)]
            continue
        in_b = (dup.split == b) & P[cls, a]
        ib = torch.where(in_b, ar, torch.full_like(ar, T)).min()
        g = dup.group[ib.clamp(max=T - 1)]
        ia = torch.where((dup.split == a) & (dup.group == g) & (ib < T), ar, torch.full_like(ar, T)).min()
        ex += [ia, ib]
    flat = torch.cat([ov.reshape(-1)] + [torch.stack(ex)] * bool(ex)).tolist()          # the one read-back
    ovh = [flat[a * S:(a + 1) * S] for a in range(S)]
    exh = flat[S * S:]
    out = dict(splits=names, total={n: dup.split_ptr[i + 1] - dup.split_ptr[i] for i, n in enumerate(names)},
               unique={n: ovh[i][i] for i, n in enumerate(names)}, overlap={}, example={}, duplicates=dup)
    for p, (a, b) in enumerate(pairs):
        key = (names[a], names[b])
        out["overlap"][key] = ovh[a][b]
        ia, ib = exh[2 * p], exh[2 * p + 1]
        out["example"][key] = (ia - dup.split_ptr[a], ib - dup.split_ptr[b]) if ovh[a][b] else None
    out["leakage"] = any(out["overlap"].values())
    return out


# ------------------------------------------------------------------------------------------------
# numbering-independent keys: Weisfeiler-Lehman colour refinement (include/gtok.h: gtok_graph_wl)
# ------------------------------------------------------------------------------------------------
WL_MAX_NODES_ANY = 512         # beyond it the kernel pulls over the CSR rows and needs GTOK_CSR_SIMPLE_SYMMETRIC; rounds=0 ends here
_WL_WS = {}


def _wl_workspace(dev, need: int) -> torch.Tensor:
    """gtok_graph_wl's workspace (graphs of more than 4,096 nodes only): one uint8 buffer per device, grown on demand, as
    _large_workspace keeps gtok_sent_large's"""
    key = torch.device(dev).index or 0
    t = _WL_WS.get(key)
    if t is None or t.numel() < need:
        t = torch.empty(max(16, need), dtype=torch.uint8, device=dev)
        _WL_WS[key] = t
    return t


def _wl_flags(batches, rounds: int, attrs: bool) -> int:
    """GTOK_WL_* of attrs; the argument errors that need no device"""
    if not 0 <= int(rounds) <= _lib.WL_MAX_ROUNDS:
        raise ValueError(f"graph_wl_keys: rounds must be in [0, {_lib.WL_MAX_ROUNDS}] (0 = as many rounds as the graph has nodes) (GTOK_E_INVAL)")
    for b in batches:
        if attrs and (b.nattr is None or b.eattr is None):
            raise ValueError("graph_wl_keys: attrs=True needs a batch with node and edge attributes (GTOK_E_INVAL)")
        if b.graph_ids is not None:
            raise ValueError("graph_wl_keys: a batch in dataset order only (not ops.lane_sorted's copy)")
    return _lib.WL_ATTRS if attrs else 0


def _graph_wl_launch(batch: GraphBatch, labels: Optional[torch.Tensor], rounds: int, flags: int, with_colors: bool,
                     info: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """gtok_graph_wl on the current stream -> (keys int64 [G, 2], colours int64 [N] or None, info int32 [4]); no host read."""
    _need_gpu(batch.col, "graph_wl_keys")
    _need(_lib.GRAPH_WL_SYMBOLS, "gtok_graph_wl")
    dev, G = batch.device, batch.num_graphs
    sym = bool(batch.flags & _lib.CSR_SIMPLE_SYMMETRIC)
    if batch.max_nodes > _lib.SENT_LARGE_MAX_NODES:
        raise _lib.GtokError(f"graph_wl_keys: a graph of {batch.max_nodes} nodes is beyond the {_lib.SENT_LARGE_MAX_NODES} the kernels hold "
                             "(GTOK_E_TOO_LARGE)")
    if batch.max_nodes > WL_MAX_NODES_ANY and not sym:
        raise _lib.GtokError(f"graph_wl_keys: graphs of more than {WL_MAX_NODES_ANY} nodes (this batch: {batch.max_nodes}) are refined over the "
                             "CSR rows themselves, which must list every edge once in each direction, without loops: the batch does not "
                             "carry GTOK_CSR_SIMPLE_SYMMETRIC (GTOK_E_UNSUPPORTED)")
    if (flags & _lib.WL_ATTRS) and not sym and G:
        raise _lib.GtokError("graph_wl_keys: attrs=True reads each direction's own attribute byte off the CSR rows: the batch does not carry "
                             "GTOK_CSR_SIMPLE_SYMMETRIC (GTOK_E_UNSUPPORTED)")
    if rounds == 0 and batch.max_nodes > WL_MAX_NODES_ANY:
        raise _lib.GtokError(f"graph_wl_keys: rounds=0 runs as many rounds as a graph has nodes and ends at {WL_MAX_NODES_ANY} nodes (this "
                             f"batch: {batch.max_nodes}): give a round count (GTOK_E_UNSUPPORTED)")
    labels = _labels_of(batch, labels, dev)
    if info is None:
        info = torch.zeros(4, dtype=torch.int32, device=dev)
    elif info.dtype != torch.int32 or info.numel() != 4 or info.device != dev or not info.is_contiguous():
        raise ValueError("graph_wl_keys: info must be int32 [4] on the batch's device")
    keys = torch.empty((G, 2), dtype=torch.int64, device=dev)
    colors = torch.zeros(batch.num_nodes_total, dtype=torch.int64, device=dev) if with_colors else None
    if G == 0:
        return keys, colors, info
    need = int(lib().gtok_graph_wl_workspace(batch.max_nodes, G))
    if need < 0:
        check(need, "gtok_graph_wl_workspace")
    ws = None
    if need > 0:
        ws = workspace if workspace is not None else _wl_workspace(dev, need)
        if ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.device != torch.device(dev):
            raise ValueError("workspace: a contiguous uint8 tensor on the batch's device")
    cs = batch.c_struct()
    check(lib().gtok_graph_wl(ctypes.byref(cs), None if labels is None else labels.data_ptr(), int(rounds), flags, keys.data_ptr(),
                              None if colors is None else colors.data_ptr(), info.data_ptr(), None if ws is None else ws.data_ptr(),
                              0 if ws is None else ws.numel(), _stream(dev)), "gtok_graph_wl")
    return keys, colors, info


def graph_wl_keys(batch: GraphBatch, rounds: int = 3, labels: Optional[torch.Tensor] = None, attrs: bool = False,
                  with_colors: bool = False, info: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """gtok_graph_wl: a 128-bit key per graph that does NOT depend on its numbering -> int64 [G, 2] on the device (the two uint64 words,
    bit for bit); with_colors=True: (keys, colours int64 [N]), the final colour of every node (a damaged graph's stay 0).  The key is
    that of `rounds` rounds of Weisfeiler-Lehman colour refinement over the simple undirected closure of the listed entries (rounds=0: as
    many rounds as the graph has nodes, up to 512 nodes): isomorphic graphs always share it - the same molecule decoded from two epochs'
    token rows, a renumbered, re-oriented or re-listed copy.  It is an invariant, not an isomorphism class: graphs colour refinement
    cannot tell apart (regular graphs of equal degree) share it too, and 128 bits can collide; ops.isomorphic_duplicates confirms what
    can be confirmed.  attrs=True: node and edge attribute bytes enter the colours (GTOK_CSR_SIMPLE_SYMMETRIC batches only, as are
    graphs of more than 512 nodes).  labels int32 [G] or None; info: an int32 [4] tensor of the caller's to accumulate the status into
    (bit KEYS_DAMAGED, the damaged graphs); workspace: a uint8 tensor of the caller's own (graphs of more than 4,096 nodes; launches on
    several streams must not share the module's), None = a cached one per device."""
    flags = _wl_flags([batch], rounds, attrs)
    keys, colors, _ = _graph_wl_launch(batch, labels, int(rounds), flags, with_colors, info, workspace)
    return (keys, colors) if with_colors else keys


class IsoDuplicates(Duplicates):
    """What ops.isomorphic_duplicates returns: Duplicates (group, split, is_first, split_ptr; overlap / leaked / unique_per_split) plus
    proven bool [T]: graph i IS isomorphic to the first graph of its class (the first itself: True).  proven = False means
    "WL-equivalent" - no round of colour refinement tells the two apart - not "isomorphic"."""
    __slots__ = ("proven",)

    def __init__(self, group, split, is_first, split_ptr, proven):
        super().__init__(group, split, is_first, split_ptr)
        self.proven = proven


def _wl_ranks(bl, colors: torch.Tensor):
    """The nodes of the concatenation sorted by (graph, colour) -> (sorted colours, rank of every node inside its graph, one int64 [N]
    per batch; discrete bool [T]: the graph's N colours are distinct, so the ranks number it canonically; node starts, node counts)"""
    dev = colors.device
    n_all = torch.cat([b.node_counts().to(torch.int64) for b in bl])
    T, N = int(n_all.numel()), int(colors.numel())
    gid = torch.repeat_interleave(torch.arange(T, device=dev), n_all)
    starts = torch.cumsum(n_all, 0) - n_all
    o1 = torch.sort(colors, stable=True).indices
    order = o1[torch.sort(gid[o1], stable=True).indices]
    cs = colors[order]
    rank = torch.empty(N, dtype=torch.int64, device=dev)
    rank[order] = torch.arange(N, device=dev) - starts[gid]              # (gid is sorted: gid[order] == gid)
    rep = torch.zeros(T, dtype=torch.int64, device=dev)
    if N > 1:
        same = (cs[1:] == cs[:-1]) & (gid[1:] == gid[:-1])
        rep.index_add_(0, gid[1:], same.to(torch.int64))
    sizes = [b.num_nodes_total for b in bl]
    return cs, list(torch.split(rank, sizes)), rep == 0, starts, n_all


def _confirm_wl(bl, ll, ptr, group: torch.Tensor, colors: torch.Tensor, attrs: bool, budget_bytes: int):
    """Classes by key -> (classes, proven).  Every member of a class of two or more is compared with the class's first member: N, the
    label and the sorted colours (what the key digests: a member that differs there is a digest collision and leaves the class); where
    both colourings are discrete, the entry lists (and, with attrs, the node bytes) in the numbering the colour ranks give - equal
    lists prove the isomorphism, different ones split the member off.  The first member split off heads a new class and the others are
    compared with it in the next round, as in _confirm_groups."""
    dev, T = group.device, int(group.numel())
    ar = torch.arange(T, device=dev)
    cs, rank, discrete, nstart, n_all = _wl_ranks(bl, colors)
    e_all = torch.cat([b.edge_ptr[1:] - b.edge_ptr[:-1] for b in bl])
    lab = torch.cat([torch.zeros(b.num_graphs, dtype=torch.int32, device=dev) if l is None else l for b, l in zip(bl, ll)])
    per_chunk = max(1, int(budget_bytes) // 64)
    group = group.clone()
    proven = group == ar
    pending = ~proven
    while True:
        mem = pending.nonzero().reshape(-1)
        if mem.numel() == 0:
            break
        heads = group[mem]
        ok = (n_all[mem] == n_all[heads]) & (lab[mem] == lab[heads]) & (discrete[mem] == discrete[heads])
        ok &= _segments_equal(cs, nstart, n_all, mem, heads)
        sure = torch.zeros_like(ok)
        cand = (ok & discrete[mem]).nonzero().reshape(-1)                   # the pairs whose lists can be compared
        if cand.numel():
            cm, ch = mem[cand], heads[cand]
            cost = e_all[cm] + e_all[ch] + (n_all[cm] + n_all[ch] if attrs else 0) + 1
            chunk = (torch.cumsum(cost, 0) - cost) // per_chunk
            sizes = torch.unique_consecutive(chunk, return_counts=True)[1].tolist()
            eq_all = torch.ones(int(cand.numel()), dtype=torch.bool, device=dev)
            i0 = 0
            for sz in sizes:
                gs, inv = torch.unique(torch.cat([cm[i0:i0 + sz], ch[i0:i0 + sz]]), return_inverse=True)
                eq = torch.ones(sz, dtype=torch.bool, device=dev)
                for vals, starts, cnts in _canonical_lists(bl, ptr, gs, not attrs, attrs, rank):
                    eq &= _segments_equal(vals, starts, cnts, inv[:sz], inv[sz:])
                eq_all[i0:i0 + sz] = eq
                i0 += sz
            sure[cand] = eq_all
            ok[cand] = eq_all
        proven[mem[sure]] = True
        pending[mem[ok]] = False
        bad = mem[~ok]
        if bad.numel() == 0:
            break
        first_bad = torch.full((T,), T, dtype=torch.int64, device=dev).scatter_reduce_(0, group[bad], bad, "amin")
        group[bad] = first_bad[group[bad]]
        pending[bad] = group[bad] != bad
        proven[bad] = group[bad] == bad
    return group, proven


def isomorphic_duplicates(batches, labels=None, rounds: int = 0, attrs: bool = False, confirm: bool = True, keys=None, colors=None,
                          budget_bytes: int = 256 << 20) -> IsoDuplicates:
    """The classes of graphs that colour refinement cannot tell apart, whatever their numbering, of one batch or of a sequence of batches
    (a sample and the training split; the epochs of a decoded corpus), on the device -> IsoDuplicates over their concatenation.  Keys
    and node colours come from gtok_graph_wl (ops.graph_wl_keys: rounds, attrs; labels: one tensor per batch, or None) unless `keys`
    (int64 [T, 2], or one [G, 2] per batch) and - with confirm - `colors` (int64 [total nodes], or one per batch) supply them; grouping
    is ops.duplicate_graphs'.  confirm=True compares every member of a class with the class's first member: a member whose colours
    differ under an equal key leaves the class; where both graphs have as many distinct colours as nodes (a DISCRETE colouring, found
    with a sort over (graph, colour)) the colour ranks number both canonically and their entry lists in that numbering (with attrs the
    directed entries with their bytes, and the node bytes) are compared - equal lists prove the isomorphism (proven = True), different
    ones split the member off into a class of its own.  A member with a colouring that is not discrete (rings, most molecules: symmetric
    atoms share a colour) stays in the class with proven = False: "WL-equivalent", which is not "isomorphic" (a 6-cycle and two
    triangles are WL-equivalent).  confirm=False trusts the 128 bits and proves nothing beyond the class heads."""
    single = isinstance(batches, GraphBatch)
    bl = [batches] if single else list(batches)
    if not bl:
        raise ValueError("isomorphic_duplicates: no batch")
    if labels is None:
        ll = [None] * len(bl)
    else:
        ll = [labels] if single else list(labels)
        if len(ll) != len(bl):
            raise ValueError("isomorphic_duplicates: one label tensor (or None) per batch")
    flags = _wl_flags(bl, rounds, attrs)
    dev = bl[0].device
    if any(b.device != dev for b in bl):
        raise ValueError("isomorphic_duplicates: batches on different devices")
    ll = [_labels_of(b, l, dev) for b, l in zip(bl, ll)]
    ptr = [0]
    for b in bl:
        ptr.append(ptr[-1] + b.num_graphs)
    T = ptr[-1]
    N = sum(b.num_nodes_total for b in bl)
    if keys is None:
        got = [_graph_wl_launch(b, l, int(rounds), flags, confirm) for b, l in zip(bl, ll)]
        keys = torch.cat([g[0] for g in got])
        colors = torch.cat([g[1] for g in got]) if confirm else None
    else:
        keys = torch.cat([torch.as_tensor(k).reshape(-1, 2) for k in keys]) if isinstance(keys, (list, tuple)) else torch.as_tensor(keys)
        keys = keys.to(dev, dtype=torch.int64)
        if tuple(keys.shape) != (T, 2):
            raise ValueError(f"isomorphic_duplicates: keys must be int64 [{T}, 2]")
        if confirm:
            if colors is None:
                raise ValueError("isomorphic_duplicates: confirm=True with keys= needs the node colours too (colors=)")
            colors = torch.cat([torch.as_tensor(c).reshape(-1) for c in colors]) if isinstance(colors, (list, tuple)) else torch.as_tensor(colors)
            colors = colors.to(dev, dtype=torch.int64).reshape(-1)
            if int(colors.numel()) != N:
                raise ValueError(f"isomorphic_duplicates: colors must be int64 [{N}]")
    split = torch.repeat_interleave(torch.arange(len(bl), device=dev), torch.tensor([b.num_graphs for b in bl], device=dev))
    group = _group_by_keys(keys)
    ar = torch.arange(T, device=dev)
    proven = group == ar
    if confirm and T:
        group, proven = _confirm_wl(bl, ll, ptr, group, colors, attrs, budget_bytes)
    return IsoDuplicates(group, split, group == ar, ptr, proven)


def unique_novel(generated: GraphBatch, references, rounds: int = 0, attrs: bool = False, keys=None, colors=None) -> Dict[str, torch.Tensor]:
    """Uniqueness and novelty of a batch of generated (decoded) graphs against one reference batch or a sequence of them (the training
    split), whatever numbering each graph has - ops.isomorphic_duplicates over [generated] + references, confirmed; device tensors,
    nothing read back:
      unique      bool [G]  the graph is the first of its class inside `generated`
      novel       bool [G]  its class occurs in no reference batch
      num_unique, num_novel   int64 scalars: their counts (the two rates are these over G)
    Classes are those of colour refinement: a generated graph that no round tells apart from a reference graph counts as known.
    keys= / colors=: as ops.isomorphic_duplicates takes them, for the concatenation."""
    refs = [references] if isinstance(references, GraphBatch) else list(references)
    dup = isomorphic_duplicates([generated] + refs, None, rounds, attrs, True, keys, colors)
    G = generated.num_graphs
    P, cls = dup._presence()
    unique = dup.is_first[:G]
    novel = ~P[cls[:G], 1:].any(1)
    return dict(unique=unique, novel=novel, num_unique=unique.sum(), num_novel=novel.sum())


def remap_zinc(ids: torch.Tensor, ln: torch.Tensor, idx_offset: int, node_idx_offset: int,
               edge_idx_offset: int) -> torch.Tensor:
    _need_gpu(ids, "remap_zinc")
    ids = ids.contiguous()
    out = torch.empty_like(ids)
    check(lib().gtok_remap_zinc(ids.data_ptr(), out.data_ptr(), ids.shape[1], ln.data_ptr(), ids.shape[0],
                                idx_offset, node_idx_offset, edge_idx_offset, _stream(ids.device)),
          "gtok_remap_zinc")
    return out


def collate(ids: torch.Tensor, ln: torch.Tensor, index: torch.Tensor, pad_id: int,
            out_ld: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Rows `index` of the slab -> (X int64 [B, out_ld], attn bool [B, out_ld])."""
    _need_gpu(ids, "collate")
    dev = ids.device
    index = index.to(dev, dtype=torch.int64).contiguous()
    B = int(index.numel())
    X = torch.empty((B, out_ld), dtype=torch.int64, device=dev)
    A = torch.empty((B, out_ld), dtype=torch.bool, device=dev)
    check(lib().gtok_collate(ids.data_ptr(), ids.shape[1], ln.data_ptr(), index.data_ptr(), B, pad_id,
                             X.data_ptr(), A.data_ptr(), out_ld, None, _stream(dev)), "gtok_collate")
    return X, A


# ------------------------------------------------------------------------------------------------
# packed (ragged) rows: the form token rows take when they leave the GPU (all-gather, D2H)
# ------------------------------------------------------------------------------------------------
ROW_ALIGN = 8      # ids: 16-byte aligned row starts at 2 bytes per id (the vector path of pack / unpack)
ROW_ALIGN_8BIT = 16      # ... at 1 byte per id (elem_bytes=1: the default there)
_PACKED_DTYPE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _row_align(align: Optional[int], elem_bytes: int) -> int:
    return int(align) if align is not None else (ROW_ALIGN_8BIT if elem_bytes == 1 else ROW_ALIGN)


def row_offsets(ln: torch.Tensor, ld: int, align: int = ROW_ALIGN) -> torch.Tensor:
    """int64 [rows + 1]: row r of the packed form starts at element row_ptr[r] and holds min(len[r], ld) ids;
    starts are multiples of `align` (gtok_row_offsets)."""
    _need_gpu(ln, "row_offsets")
    if ln.dtype != torch.int32 or not ln.is_contiguous():
        raise ValueError("row_offsets expects a contiguous int32 length vector")
    ptr = torch.empty(ln.numel() + 1, dtype=torch.int64, device=ln.device)
    check(lib().gtok_row_offsets(ln.data_ptr(), ln.numel(), int(ld), int(align), ptr.data_ptr(), _stream(ln.device)),
          "gtok_row_offsets")
    return ptr


def _pack_verdict(packed, row_ptr, status, cap, what):
    st = int(status.item())
    if st & 1:
        raise _lib.GtokError(f"{what}: " + (ID_TOO_WIDE_8 if packed.element_size() == 1 else "an id does not fit 16 bits; pack with elem_bytes=4"))
    if st & 2:
        raise _lib.GtokError(f"{what}: capacity {cap} is too small for these rows")
    return packed, row_ptr


def pack_rows_scan(ids: torch.Tensor, ln: torch.Tensor, elem_bytes: int, capacity: int, align: Optional[int] = None):
    """row_offsets + pack_rows / pack_rows_u16 in ONE pass (gtok_pack_rows_scan): for callers that know a capacity before
    they know the sizes.  ids: the int32 slab or the 16-bit slab (int16 storage).  Returns (packed, row_ptr, status) - nothing
    waits for the host (status bit 0: an id needs more bits than elem_bytes has, bit 1: rows that did not fit `capacity` were
    skipped).  elem_bytes=1: uint8 storage; align defaults to 16 ids there, else to ROW_ALIGN."""
    _need_gpu(ids, "pack_rows_scan")
    if ids.dtype not in (torch.int32, torch.int16) or ids.dim() != 2 or not ids.is_contiguous() or ln.dtype != torch.int32 or not ln.is_contiguous():
        raise ValueError("pack_rows_scan expects a contiguous int32 / int16 [rows, ld] slab and contiguous int32 lengths")
    src_bytes = ids.element_size()
    if elem_bytes not in ((1, 2, 4, 8) if src_bytes == 2 else (1, 2, 4)):
        raise ValueError("elem_bytes must be 1, 2 or 4 (8 also from a 16-bit slab)")
    align = _row_align(align, elem_bytes)
    dev, (rows, ld) = ids.device, ids.shape
    if int(ln.numel()) != rows:
        raise ValueError("pack_rows_scan: one length per row")
    cap = int(capacity)
    packed = torch.empty(max(cap, 1), dtype=_PACKED_DTYPE[elem_bytes], device=dev)
    row_ptr = torch.empty(rows + 1, dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)          # (set by the call)
    check(lib().gtok_pack_rows_scan(ids.data_ptr(), src_bytes, ld, ln.data_ptr(), rows, int(align), elem_bytes, packed.data_ptr(), cap,
                                    row_ptr.data_ptr(), status.data_ptr(), _stream(dev)), "gtok_pack_rows_scan")
    return packed, row_ptr, status


def pack_rows(ids: torch.Tensor, ln: torch.Tensor, row_ptr: Optional[torch.Tensor] = None, elem_bytes: int = 2,
              capacity: Optional[int] = None, align: Optional[int] = None, check_status: bool = True):
    """[rows, ld] int32 slab + lengths -> (packed, row_ptr): row r's ids back to back from packed[row_ptr[r]], int16
    storage (ids 0..65535 kept as their 16 bits), int32, or uint8 (elem_bytes=1: ids 0..255, align defaults to 16).  capacity: elements to allocate (an all-gather needs the
    same size on every rank); default = exactly row_ptr[-1] (one host read).  Raises when elem_bytes is 1 or 2 and an id
    needs more bits, or when `capacity` is too small; check_status=False hands the status tensor back instead
    (packed, row_ptr, status) and leaves the host out of it."""
    _need_gpu(ids, "pack_rows")
    if ids.dtype != torch.int32 or ids.dim() != 2 or not ids.is_contiguous() or ln.dtype != torch.int32:
        raise ValueError("pack_rows expects a contiguous int32 [rows, ld] slab and int32 lengths")
    dev, (rows, ld) = ids.device, ids.shape
    if int(ln.numel()) != rows:
        raise ValueError("pack_rows: one length per row")
    if elem_bytes not in (1, 2, 4):
        raise ValueError("elem_bytes must be 1, 2 or 4")
    align = _row_align(align, elem_bytes)
    if row_ptr is None and capacity is not None and _lib.library_version() >= 5:       # sizes not needed first: one pass
        packed, row_ptr, status = pack_rows_scan(ids, ln.contiguous(), elem_bytes, capacity, align)
        return (packed, row_ptr, status) if not check_status else _pack_verdict(packed, row_ptr, status, int(capacity), "pack_rows")
    if row_ptr is None:
        row_ptr = row_offsets(ln, ld, align)
    cap = int(row_ptr[-1]) if capacity is None else int(capacity)
    packed = torch.empty(max(cap, 1), dtype=_PACKED_DTYPE[elem_bytes], device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib().gtok_pack_rows(ids.data_ptr(), ld, ln.data_ptr(), rows, row_ptr.data_ptr(), elem_bytes, packed.data_ptr(),
                               cap, status.data_ptr(), _stream(dev)), "gtok_pack_rows")
    if not check_status:
        return packed, row_ptr, status
    return _pack_verdict(packed, row_ptr, status, cap, "pack_rows")


def pack_rows_u16(ids16: torch.Tensor, ln: torch.Tensor, row_ptr: Optional[torch.Tensor] = None, elem_bytes: int = 2,
                  capacity: Optional[int] = None, align: Optional[int] = None, check_status: bool = True):
    """pack_rows reading a 16-bit slab (ops.sent(..., u16=True)): -> (packed, row_ptr) with uint8, int16, int32 or int64 storage
    (elem_bytes 1 / 2 / 4 / 8; 1 = ids 0..255, align defaults to 16, raises when an id needs more bits; 8 = the dtype the reference's token tensors have: the packed buffer can leave for the host as
    it is).  check_status=False: (packed, row_ptr, status) and no host read."""
    _need_gpu(ids16, "pack_rows_u16")
    if ids16.dtype != torch.int16 or ids16.dim() != 2 or not ids16.is_contiguous() or ln.dtype != torch.int32:
        raise ValueError("pack_rows_u16 expects a contiguous int16 [rows, ld] slab and int32 lengths")
    if elem_bytes not in (1, 2, 4, 8):
        raise ValueError("elem_bytes must be 1, 2, 4 or 8")
    align = _row_align(align, elem_bytes)
    dev, (rows, ld) = ids16.device, ids16.shape
    if int(ln.numel()) != rows:
        raise ValueError("pack_rows_u16: one length per row")
    if row_ptr is None and capacity is not None and _lib.library_version() >= 5:       # sizes not needed first: one pass
        packed, row_ptr, status = pack_rows_scan(ids16, ln.contiguous(), elem_bytes, capacity, align)
        return (packed, row_ptr, status) if not check_status else _pack_verdict(packed, row_ptr, status, int(capacity), "pack_rows_u16")
    if row_ptr is None:
        row_ptr = row_offsets(ln, ld, align)
    cap = int(row_ptr[-1]) if capacity is None else int(capacity)
    packed = torch.empty(max(cap, 1), dtype=_PACKED_DTYPE[elem_bytes], device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib().gtok_pack_rows_u16(ids16.data_ptr(), ld, ln.data_ptr(), rows, row_ptr.data_ptr(), elem_bytes, packed.data_ptr(),
                                   cap, status.data_ptr(), _stream(dev)), "gtok_pack_rows_u16")
    if not check_status:
        return packed, row_ptr, status
    return _pack_verdict(packed, row_ptr, status, cap, "pack_rows_u16")


def unpack_rows(packed: torch.Tensor, row_ptr: Optional[torch.Tensor], ln: torch.Tensor, ld: int, pad_id: int,
                segment_rows: int = 0, segment_stride: int = 0, out: Optional[torch.Tensor] = None,
                status: Optional[torch.Tensor] = None, u16: bool = False) -> torch.Tensor:
    """packed rows -> [rows, ld] int32 slab with pad_id behind every row (gtok_unpack_rows_checked).  segment_rows /
    segment_stride: the packed buffer is the concatenation of per-rank buffers (see include/gtok.h).  row_ptr=None: the
    strided form - `packed` is itself a [rows, ld] slab of 16- or 32-bit ids (ops.sent(..., u16=True)), widened in place.
    Rows that would end beyond their segment or the buffer come out as all pad; `status` (int32 [1], zeroed by the
    caller) gets bit 1 then.  u16=True (gtok_unpack_rows_u16): the slab holds 16-bit ids (int16 storage, as ops.sent(...,
    u16=True) writes it) - half the bytes of the pass."""
    _need_gpu(packed, "unpack_rows")
    dev, rows = packed.device, int(ln.numel())
    eb = packed.element_size()
    if eb not in (1, 2, 4):
        raise ValueError("unpack_rows expects uint8, int16 or int32 storage")
    want = torch.int16 if u16 else torch.int32
    ids = torch.empty((rows, ld), dtype=want, device=dev) if out is None else out
    if ids.dtype != want:
        raise ValueError(f"out must be {want}")
    fn = lib().gtok_unpack_rows_u16 if u16 else lib().gtok_unpack_rows_checked
    check(fn(packed.data_ptr(), eb, None if row_ptr is None else row_ptr.data_ptr(), ln.data_ptr(), rows,
             int(segment_rows), int(segment_stride), int(packed.numel()), int(pad_id), ids.data_ptr(), int(ld),
             None if status is None else status.data_ptr(), _stream(dev)), "gtok_unpack_rows")
    return ids


def unpack_rows_at(packed: torch.Tensor, row_start: torch.Tensor, ln: torch.Tensor, ld: int, pad_id: int, segment_rows: int = 0,
                   segment_stride: int = 0, out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None,
                   u16: bool = False) -> torch.Tensor:
    """unpack_rows for rows with explicit starts (gtok_unpack_rows_at; what ops.sent(..., packed=) writes): row r's ids start at
    element (r // segment_rows) * segment_stride + row_start[r] (segment_rows == 0: at row_start[r]); a negative start or a row
    beyond its segment comes out as all pad, status bit 1."""
    _need_gpu(packed, "unpack_rows_at")
    dev, rows = packed.device, int(ln.numel())
    eb = packed.element_size()
    if eb not in (1, 2, 4) or row_start.dtype != torch.int64 or int(row_start.numel()) < rows or not row_start.is_contiguous():
        raise ValueError("unpack_rows_at expects uint8 / int16 / int32 storage and one contiguous int64 start per row")
    want = torch.int16 if u16 else torch.int32
    ids = torch.empty((rows, ld), dtype=want, device=dev) if out is None else out
    if ids.dtype != want:
        raise ValueError(f"out must be {want}")
    check(lib().gtok_unpack_rows_at(packed.data_ptr(), eb, row_start.data_ptr(), ln.data_ptr(), rows, int(segment_rows), int(segment_stride),
                                    int(packed.numel()), int(pad_id), ids.data_ptr(), 2 if u16 else 4, int(ld),
                                    None if status is None else status.data_ptr(), _stream(dev)), "gtok_unpack_rows_at")
    return ids


def collate_packed(packed: torch.Tensor, row_ptr: Optional[torch.Tensor], ln: torch.Tensor, ld: int, index: torch.Tensor,
                   pad_id: int, out_ld: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """ops.collate over the packed form: rows `index` -> (X int64 [B, out_ld], attn bool [B, out_ld]).  row_ptr=None: the
    strided form - `packed` is a [rows, ld] slab of 16- or 32-bit ids read in place (ops.sent(..., u16=True))."""
    _need_gpu(packed, "collate_packed")
    dev = packed.device
    index = index.to(dev, dtype=torch.int64).contiguous()
    B = int(index.numel())
    X = torch.empty((B, out_ld), dtype=torch.int64, device=dev)
    A = torch.empty((B, out_ld), dtype=torch.bool, device=dev)
    check(lib().gtok_collate_packed(packed.data_ptr(), packed.element_size(), None if row_ptr is None else row_ptr.data_ptr(),
                                    ln.data_ptr(), int(ld), index.data_ptr(), B, int(pad_id), X.data_ptr(), A.data_ptr(), int(out_ld),
                                    _stream(dev)), "gtok_collate_packed")
    return X, A


def collate_batch(packed: torch.Tensor, row_ptr: Optional[torch.Tensor], ln: torch.Tensor, ld: int, index_host: np.ndarray, pad_id: int,
                  out_ld: int, y: Optional[torch.Tensor] = None):
    """collate_packed for a row list that is a HOST array (int64 numpy, what a DataLoader's sampler produced): the indices travel
    in the kernel's arguments (gtok_collate_batch: no upload) and the labels y[index] come out of the same launch.
    -> (X int64 [B, out_ld], attn bool [B, out_ld], Y or None)."""
    _need_gpu(packed, "collate_batch")
    dev = packed.device
    idx = np.ascontiguousarray(index_host, dtype=np.int64)
    B = int(idx.size)
    X = torch.empty((B, out_ld), dtype=torch.int64, device=dev)
    A = torch.empty((B, out_ld), dtype=torch.bool, device=dev)
    Y = None
    if y is not None:
        if y.dim() != 1 or not y.is_contiguous() or y.element_size() not in (4, 8):
            raise ValueError("y must be a contiguous 1-D tensor of 4- or 8-byte elements")
        Y = torch.empty(B, dtype=y.dtype, device=dev)
    check(lib().gtok_collate_batch(packed.data_ptr(), packed.element_size(), None if row_ptr is None else row_ptr.data_ptr(), ln.data_ptr(), int(ld),
                                   idx.ctypes.data, B, int(ln.numel()), int(pad_id), X.data_ptr(), A.data_ptr(), int(out_ld),
                                   None if y is None else y.data_ptr(), 0 if y is None else y.element_size(), None if Y is None else Y.data_ptr(),
                                   _stream(dev)), "gtok_collate_batch")
    return X, A, Y


def collate_epoch(packed: torch.Tensor, row_ptr: Optional[torch.Tensor], ln: torch.Tensor, ld: int, order: torch.Tensor, batch_size: int,
                  pad_id: int):
    """Every batch of an epoch collated by ONE call (gtok_collate_epoch): rows `order` (int64, on the device) cut into batches of
    batch_size -> (X int64 arena, attn bool arena, lmax list[int], off list[int]): batch b is
    X.as_strided((B_b, lmax[b]), (lmax[b], 1), off[b]) - what collate_packed(index=order[b * batch_size:...], out_ld=lmax[b]) gives.
    row_ptr=None: `packed` is a [rows, ld] slab of 16- / 32-bit ids (ops.sent(..., u16=True)).  One small read-back per EPOCH
    (the batch widths), none per batch."""
    _need_gpu(packed, "collate_epoch")
    dev = packed.device
    order = order.to(dev, dtype=torch.int64).contiguous()
    n, bs = int(order.numel()), int(batch_size)
    nb = -(-n // bs) if n else 0
    lmax = torch.empty(max(nb, 1), dtype=torch.int32, device=dev)
    off = torch.empty(nb + 1, dtype=torch.int64, device=dev)
    L = lib()
    check(L.gtok_collate_epoch_plan(ln.data_ptr(), int(ld), order.data_ptr(), n, bs, lmax.data_ptr(), off.data_ptr(), _stream(dev)),
          "gtok_collate_epoch_plan")
    off_h = off.tolist()                       # the one synchronisation of the epoch: the arena is sized exactly
    total = off_h[-1]
    X = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
    A = torch.empty(max(total, 1), dtype=torch.bool, device=dev)
    check(L.gtok_collate_epoch(packed.data_ptr(), packed.element_size(), None if row_ptr is None else row_ptr.data_ptr(), ln.data_ptr(), int(ld),
                               order.data_ptr(), n, bs, int(pad_id), lmax.data_ptr(), off.data_ptr(), X.data_ptr(), A.data_ptr(), total,
                               _stream(dev)), "gtok_collate_epoch")
    return X, A, lmax[:nb].tolist(), off_h


def zinc_text_tails(y: torch.Tensor, ln: torch.Tensor, max_len: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """What follows `<p>` in every ZINC text, rendered on the device (gtok_zinc_text_tails; reference
    zinc_dataset_indexbase.py:186-195, :217-221): y float32 [G] labels, ln int32 [G] ids per row (gtok_ibtt_zinc's lengths).
    Returns (take int32 [G], suf_bytes uint8 [total], suf_ptr int64 [G + 1]) on the device: ids_to_text(ids, take, strings,
    (suf_bytes, suf_ptr)) gives exactly the strings ZINCTokenizationDataset.__getitem__ returns."""
    _need_gpu(ln, "zinc_text_tails")
    if y.dtype != torch.float32 or ln.dtype != torch.int32 or y.numel() != ln.numel():
        raise ValueError("zinc_text_tails expects float32 labels and int32 lengths of one size")
    dev, G = ln.device, int(ln.numel())
    y, ln = y.to(dev).contiguous(), ln.contiguous()
    take = torch.empty(G, dtype=torch.int32, device=dev)
    slen = torch.empty(G, dtype=torch.int64, device=dev)
    L = lib()
    max_len = int(min(max_len, 2 ** 31 - 1))
    check(L.gtok_zinc_text_tails(y.data_ptr(), ln.data_ptr(), G, int(max_len), take.data_ptr(), None, None, slen.data_ptr(),
                                 _stream(dev)), "gtok_zinc_text_tails")
    sp = torch.zeros(G + 1, dtype=torch.int64, device=dev)
    torch.cumsum(slen, 0, out=sp[1:])
    sb = torch.empty(max(56 * G, 1), dtype=torch.uint8, device=dev)      # a tail is at most 56 bytes: no size round trip
    check(L.gtok_zinc_text_tails(y.data_ptr(), ln.data_ptr(), G, int(max_len), take.data_ptr(), sp.data_ptr(), sb.data_ptr(), None,
                                 _stream(dev)), "gtok_zinc_text_tails")
    return take, sb, sp


def ids_to_text(ids: torch.Tensor, take: torch.Tensor, strings: Sequence[str], suffixes=None):
    """Rows of ids -> texts on the device (gtok_ids_to_text): row r = the strings of its first take[r] ids joined by single
    spaces + suffixes[r] verbatim.  Returns (blob uint8 [total], text_ptr int64 [rows + 1]) on the device; text r is
    blob[text_ptr[r] : text_ptr[r + 1]].  `strings[t]` is the text of id t (ASCII).  `suffixes`: one bytes object per row,
    or (suf_bytes uint8, suf_ptr int64 [rows + 1]) already on the device (zinc_text_tails)."""
    _need_gpu(ids, "ids_to_text")
    if ids.dtype != torch.int32 or ids.dim() != 2 or not ids.is_contiguous() or take.dtype != torch.int32:
        raise ValueError("ids_to_text expects a contiguous int32 [rows, ld] slab and int32 counts")
    dev, (rows, ld) = ids.device, ids.shape
    enc = [t.encode("ascii") for t in strings]
    tptr = np.zeros(len(enc) + 1, np.int32); np.cumsum([len(b) for b in enc], out=tptr[1:])
    tab = torch.frombuffer(bytearray(b"".join(enc) or b"\0"), dtype=torch.uint8).to(dev)
    tab_ptr = torch.from_numpy(tptr).to(dev)
    sb = sp = None
    if isinstance(suffixes, tuple) and len(suffixes) == 2 and torch.is_tensor(suffixes[0]):
        sb, sp = suffixes
        if sb.dtype != torch.uint8 or sp.dtype != torch.int64 or sp.numel() != rows + 1 or sb.device != dev or sp.device != dev:
            raise ValueError("device suffixes are (uint8 bytes, int64 [rows + 1] offsets) on the ids' device")
        sb, sp = sb.contiguous(), sp.contiguous()
    elif suffixes is not None:
        if len(suffixes) != rows:
            raise ValueError("one suffix per row")
        sptr = np.zeros(rows + 1, np.int64); np.cumsum(np.fromiter(map(len, suffixes), np.int64, rows), out=sptr[1:])
        sb = torch.frombuffer(bytearray(b"".join(suffixes) or b"\0"), dtype=torch.uint8).to(dev)
        sp = torch.from_numpy(sptr).to(dev)
    tlen = torch.empty(rows, dtype=torch.int64, device=dev)
    L = lib()
    args = (ids.data_ptr(), ld, take.data_ptr(), rows, tab.data_ptr(), tab_ptr.data_ptr(), len(enc),
            None if sb is None else sb.data_ptr(), None if sp is None else sp.data_ptr())
    check(L.gtok_ids_to_text(*args, None, None, tlen.data_ptr(), _stream(dev)), "gtok_ids_to_text")
    text_ptr = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
    torch.cumsum(tlen, 0, out=text_ptr[1:])
    total = int(text_ptr[-1])
    blob = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    check(L.gtok_ids_to_text(*args, text_ptr.data_ptr(), blob.data_ptr(), None, _stream(dev)), "gtok_ids_to_text")
    return blob[:total], text_ptr


# ------------------------------------------------------------------------------------------------
# text -> ids (TokenDataset)
# ------------------------------------------------------------------------------------------------
NO_LABEL = -2 ** 31


def parse_graph_texts(text_bytes: torch.Tensor, text_ptr: torch.Tensor) -> Dict[str, torch.Tensor]:
    """graph-token texts -> edges / node counts / query nodes / labels on the device (the reference's
    parse_graph_from_text + parse_query_nodes_from_text + parse_label_from_text + the num_nodes rule).  Returns
    device tensors: num_edges, num_nodes, label (NO_LABEL = none), status int32 [G]; query int32 [G, 2] (-1 = none);
    edge_ptr int64 [G+1]; src, dst int32 [sum E] in text order.  status != 0 marks a text outside the canonical
    grammar: ignore its other fields and parse it on the host."""
    _need_gpu(text_bytes, "parse_graph_texts")
    dev = text_bytes.device
    text_ptr = text_ptr.to(dev, dtype=torch.int64).contiguous()
    G = int(text_ptr.numel()) - 1
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    ne, nn, q, lab, st = i32(G), i32(G), i32(G, 2), i32(G), i32(G)
    L = _lib.lib()
    edge_ptr = torch.zeros(G + 1, dtype=torch.int64, device=dev)
    if not G:
        return dict(num_edges=ne, num_nodes=nn, query=q, label=lab, status=st, edge_ptr=edge_ptr, src=i32(0), dst=i32(0))
    # sizing: one streaming pass that counts the `<e>` tokens (exact for canonical texts), then ONE parse that fills
    cnt = i32(G)
    _lib.check(L.gtok_count_edge_tokens(text_bytes.data_ptr(), text_ptr.data_ptr(), G, cnt.data_ptr(), _stream(dev)),
               "gtok_count_edge_tokens")
    torch.cumsum(cnt, 0, dtype=torch.int64, out=edge_ptr[1:])
    # No host round trip for the size: an edge of a text the parser accepts is at least 8 bytes (`0 1 <e> `), so the edge
    # arrays are sized by the bytes; a corpus with enough junk to count more `<e>` than that has its ranges clamped for this
    # pass and is parsed again with exact arrays (seen in the one read-back below).
    bound = int(text_bytes.numel()) // 8 + G + 1
    clamped = edge_ptr.clamp(max=bound)

    def parse(ptr, n_edges):
        s_, d_ = i32(max(n_edges, 1)), i32(max(n_edges, 1))
        _lib.check(L.gtok_parse_graph_text(text_bytes.data_ptr(), text_ptr.data_ptr(), G, ptr.data_ptr(), s_.data_ptr(),
                                           d_.data_ptr(), ne.data_ptr(), nn.data_ptr(), q.data_ptr(), lab.data_ptr(),
                                           st.data_ptr(), _stream(dev)), "gtok_parse_graph_text")
        return s_, d_
    src, dst = parse(clamped, bound)
    # every canonical text owns exactly its first num_edges slots; normally that is its whole range (one `<e>` token per
    # edge).  Texts outside the grammar (status != 0) own nothing, and a canonical text may carry a stray `<e>` where the
    # grammar allows any word (right after <q> / <p>): then the ranges are squeezed.
    keep = torch.where(st == 0, ne, torch.zeros_like(ne))
    cap, differ = torch.stack([edge_ptr[-1], (keep != cnt).any().to(torch.int64)]).tolist()
    if cap > bound:
        src, dst = parse(edge_ptr, cap)
        keep = torch.where(st == 0, ne, torch.zeros_like(ne))
        differ = int(not torch.equal(keep, cnt))
    if not differ:
        return dict(num_edges=ne, num_nodes=nn, query=q, label=lab, status=st, edge_ptr=edge_ptr, src=src[:cap], dst=dst[:cap])
    keep = keep.to(torch.int64)
    new_ptr = torch.zeros(G + 1, dtype=torch.int64, device=dev)
    torch.cumsum(keep, 0, out=new_ptr[1:])
    total = int(new_ptr[-1])
    idx = torch.repeat_interleave(edge_ptr[:-1] - new_ptr[:-1], keep, output_size=total) + torch.arange(total, device=dev)
    return dict(num_edges=ne, num_nodes=nn, query=q, label=lab, status=st, edge_ptr=new_ptr, src=src[idx], dst=dst[idx])


def find_token(x: torch.Tensor, token: int) -> torch.Tensor:
    """First column of `token` in every row of an int64 [B, L] batch (-1: absent): the `<q>` search of
    trainer/train_ibtt.py:88-103 / train_agtt.py:78-114 as one launch (query nodes sit at pos + 2, pos + 3)."""
    _need_gpu(x, "find_token")
    if x.dtype != torch.int64 or x.dim() != 2 or not x.is_contiguous():
        raise ValueError("find_token expects a contiguous int64 [B, L] tensor")
    pos = torch.empty(x.shape[0], dtype=torch.int32, device=x.device)
    _lib.check(_lib.lib().gtok_find_token(x.data_ptr(), int(x.shape[0]), int(x.shape[1]), int(token), pos.data_ptr(),
                                          _stream(x.device)), "gtok_find_token")
    return pos


def vocab_stats_synth(batch: GraphBatch, num_ids: int, query_nodes: Optional[torch.Tensor] = None, graph_base: int = 0,
                      out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Occurrence count and first position ((graph_base + g) << 32 | position in the text) of every node-id token
    `str(i)`, i < num_ids, in the graph-token texts this batch stands for: the corpus pass of
    build_vocab_from_texts (data_loader.py:451-463) on the device.  query_nodes: int32 [G, 2] (u, v), negative = none.
    `out` = (count, first) int64 [num_ids] to ACCUMULATE into (shards / ranks); fresh tables otherwise."""
    dev = batch.device
    _need_gpu(batch.col, "vocab_stats_synth")
    if out is None:
        count = torch.zeros(num_ids, dtype=torch.int64, device=dev)
        first = torch.full((num_ids,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev)
    else:
        count, first = out
        if count.dtype != torch.int64 or first.dtype != torch.int64 or count.numel() != num_ids or first.numel() != num_ids:
            raise ValueError("out must be two int64 [num_ids] tensors")
    if query_nodes is not None:
        if query_nodes.dtype != torch.int32 or tuple(query_nodes.shape) != (batch.num_graphs, 2):
            raise ValueError("query_nodes must be int32 [G, 2]")
        query_nodes = query_nodes.to(dev).contiguous()
    cs = batch.c_struct()
    _lib.check(_lib.lib().gtok_vocab_stats_synth(ctypes.byref(cs), None if query_nodes is None else query_nodes.data_ptr(),
                                                 int(graph_base), int(num_ids), count.data_ptr(), first.data_ptr(),
                                                 _stream(dev)), "gtok_vocab_stats_synth")
    return count, first


def vocab_stats_text(text_bytes: torch.Tensor, text_ptr: torch.Tensor, capacity: int = 1 << 16, base_offset: int = 0,
                     out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """Count and first position of every distinct whitespace-separated token of the texts (gtok_vocab_stats_text): the
    corpus pass of build_vocab_from_texts (data_loader.py:451-463) and of the ZINC dynamic-token scan
    (trainer/train_ibtt.py:361-372) on the device.  Returns the open-addressing table as device tensors
    {key uint64-as-int64, count, first int64, len int32, status int32 [1]} of `capacity` slots; pass it back as `out`
    to accumulate further shards (base_offset = the shard's byte offset in the whole corpus).  text_stats_entries()
    turns a finished table into (token, count, first) triples.  Tokens are told apart by a 64-bit hash AND verified byte
    for byte against the slot's first occurrence (status bit 2 = a collision; text_stats_entries raises) - within one
    call; with shards accumulated over several calls a cross-shard collision is not seen, and text_stats_entries needs
    the WHOLE corpus blob, since a slot's `first` may lie in any shard."""
    _need_gpu(text_bytes, "vocab_stats_text")
    dev = text_bytes.device
    text_ptr = text_ptr.to(dev, dtype=torch.int64).contiguous()
    G = int(text_ptr.numel()) - 1
    if capacity < 16 or capacity & (capacity - 1):
        raise ValueError("capacity must be a power of two >= 16")
    if out is None:
        out = dict(key=torch.zeros(capacity, dtype=torch.int64, device=dev), count=torch.zeros(capacity, dtype=torch.int64, device=dev),
                   first=torch.full((capacity,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev),
                   len=torch.zeros(capacity, dtype=torch.int32, device=dev), status=torch.zeros(1, dtype=torch.int32, device=dev))
    elif out["key"].numel() != capacity:
        raise ValueError("out was built for another capacity")
    _lib.check(_lib.lib().gtok_vocab_stats_text(text_bytes.data_ptr(), text_ptr.data_ptr(), G, int(base_offset), capacity,
                                                out["key"].data_ptr(), out["count"].data_ptr(), out["first"].data_ptr(),
                                                out["len"].data_ptr(), out["status"].data_ptr(), _stream(dev)),
               "gtok_vocab_stats_text")
    return out


def text_stats_entries(table: Dict[str, torch.Tensor], text_bytes: torch.Tensor, base_offset: int = 0):
    """[(token, count, first)] of a finished gtok_vocab_stats_text table, in Counter.most_common order (count
    descending, first appearance ascending).  The token strings are read back from the corpus blob at `first`
    (only the table and one byte range per DISTINCT token cross to the host).  Raises when the table overflowed."""
    st = int(table["status"].item())
    if st & 4:
        raise _lib.GtokError("vocab_stats_text: two different tokens share a 64-bit identity (hash collision): "
                             "build this vocab with the host function (build_vocab_from_texts)")
    if st:
        raise _lib.GtokError(f"vocab_stats_text: table {'overflowed' if st & 1 else 'was not consistent'} (status {st}): use a larger capacity")
    used = (table["key"] != 0).nonzero(as_tuple=True)[0]
    cnt, fst, ln = table["count"][used], table["first"][used], table["len"][used].to(torch.int64)
    order = torch.argsort(fst)                      # stable secondary key first ...
    order = order[torch.argsort(cnt[order], descending=True, stable=True)]
    cnt, fst, ln = cnt[order].cpu().tolist(), fst[order].cpu().tolist(), ln[order].cpu().tolist()
    # gather the token bytes on the device: one [sum len] buffer instead of a host copy of the corpus
    lens = torch.tensor(ln, dtype=torch.int64, device=text_bytes.device)
    starts = torch.tensor(fst, dtype=torch.int64, device=text_bytes.device) - base_offset
    ptr = torch.zeros(len(ln) + 1, dtype=torch.int64, device=text_bytes.device)
    torch.cumsum(lens, 0, out=ptr[1:])
    idx = torch.arange(int(ptr[-1]), device=text_bytes.device)
    tok = torch.repeat_interleave(torch.arange(len(ln), device=text_bytes.device), lens, output_size=int(ptr[-1]))
    blob = bytes(text_bytes[starts[tok] + (idx - ptr[tok])].cpu().numpy())
    p = ptr.cpu().tolist()
    return [(blob[p[i]:p[i + 1]].decode("utf-8"), cnt[i], fst[i]) for i in range(len(ln))]


def _fnv1a(b: bytes) -> int:
    h = 2166136261
    for c in b:
        h = ((h ^ c) * 16777619) & 0xFFFFFFFF
    return h


class VocabTable:
    """Open-addressing table (FNV-1a, linear probing) for gtok_text_to_ids, built on the host."""

    def __init__(self, vocab: Dict[str, int], device):
        self.pad_id = int(vocab["<pad>"])
        cap = 16
        while cap < 2 * max(1, len(vocab)):
            cap *= 2
        key_off = np.full(cap, -1, np.int32); key_len = np.zeros(cap, np.int32); ids = np.zeros(cap, np.int32)
        blob = bytearray()
        for tok, i in vocab.items():
            b = tok.encode("utf-8")
            if not b or any(c in b" \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f" for c in b):
                continue  # can never come out of str.split()
            s = _fnv1a(b) & (cap - 1)
            while key_off[s] >= 0:
                s = (s + 1) & (cap - 1)
            key_off[s], key_len[s], ids[s] = len(blob), len(b), i
            blob += b
        self.capacity = cap
        t = lambda a: torch.from_numpy(a).to(device)
        self.key_off, self.key_len, self.ids = t(key_off), t(key_len), t(ids)
        self.key_bytes = torch.frombuffer(bytearray(blob or b"\0"), dtype=torch.uint8).clone().to(device)

    def c_struct(self) -> GtokVocabTable:
        return GtokVocabTable(self.capacity, self.pad_id, self.key_off.data_ptr(), self.key_len.data_ptr(),
                              self.ids.data_ptr(), self.key_bytes.data_ptr())


def pack_texts(texts: Sequence[str]) -> Tuple[torch.Tensor, torch.Tensor]:
    """Concatenate texts into (bytes uint8 [total], text_ptr int64 [G+1]); ASCII only (str.split() on
    non-ASCII whitespace is not reproduced on the device)."""
    try:
        blob = "".join(texts).encode("ascii")        # one join + one encode: ASCII, so a text's length in bytes is len(text)
    except UnicodeEncodeError:
        raise ValueError("gtok text path handles ASCII text only") from None
    ptr = np.zeros(len(texts) + 1, np.int64)
    np.cumsum(np.fromiter(map(len, texts), np.int64, len(texts)), out=ptr[1:])
    return torch.frombuffer(bytearray(blob or b"\0"), dtype=torch.uint8), torch.from_numpy(ptr)


def text_to_ids(text_bytes: torch.Tensor, text_ptr: torch.Tensor, table: VocabTable, max_len: int,
                strip_label: bool = True, ld: Optional[int] = None, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    _need_gpu(text_bytes, "text_to_ids")
    dev = text_bytes.device
    text_ptr = text_ptr.to(dev, dtype=torch.int64).contiguous()
    G = int(text_ptr.numel()) - 1
    if ld is None:
        ld = _round4(max_len)
    ids, ln = _alloc_out(G, ld, dev, out)
    vs = table.c_struct()
    check(lib().gtok_text_to_ids(text_bytes.data_ptr(), text_ptr.data_ptr(), G, ctypes.byref(vs), int(strip_label),
                                 max_len, ids.data_ptr(), ld, ln.data_ptr(), _stream(dev)), "gtok_text_to_ids")
    return ids, ln
