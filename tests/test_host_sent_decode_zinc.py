"""gtok_unremap_zinc / gtok_sent_decode_zinc_sizes / gtok_sent_decode_zinc_csr, the parts that need no GPU: the binding of the three
entry points by symbol, their argument checks, the torch ops' registration and meta kernels, the tokenizer's and the dataset's
methods - and the Python unfold the GPU tests expect (tests/_sent_unfold_ref.py) against the C oracle's rows."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from _sent_unfold_ref import NONE, X, pre, remap, unfold_rows
from _util import both, edge_case_graphs, gtok, orc

_lib = gtok._lib
NAMES = ("gtok_unremap_zinc", "gtok_sent_decode_zinc_sizes", "gtok_sent_decode_zinc_csr")


def test_the_entry_points_are_bound_by_symbol_with_their_arity():
    L = _lib.lib()
    for n in NAMES:
        assert n in _lib.SYMBOLS and hasattr(L, n), n
    assert len(L.gtok_unremap_zinc.argtypes) == 11
    assert len(L.gtok_sent_decode_zinc_sizes.argtypes) == 12 and len(L.gtok_sent_decode_zinc_csr.argtypes) == 10      # the siblings' without `labeled`
    assert L.gtok_sent_decode_zinc_csr.argtypes[8] == ctypes.POINTER(_lib.GtokCsrBuilt)
    assert all(getattr(L, n).restype is ctypes.c_int32 for n in NAMES)
    # a tuple of their own: a library of the same ABI version that lacks them still loads (GTOK_LIB, A/B timing)
    assert set(_lib.ZINC_DECODE_SYMBOLS) == set(NAMES) and set(NAMES) <= _lib._MAY_BE_MISSING
    assert not set(NAMES) & (set(_lib.OPTIONAL_SYMBOLS) | set(_lib.DECODE_CSR_SYMBOLS) | set(_lib.IBTT_DECODE_SYMBOLS) | set(_lib.ORDER_SYMBOLS))
    assert _lib.ABI_VERSION == 8 and L.gtok_version() == 8


def test_host_side_argument_errors_come_before_any_device_is_asked_for():
    """null pointers / sizes / widths are refused by host code alone: these calls run without a GPU"""
    L = _lib.lib()
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.addressof(buf)
    out = _lib.GtokCsrBuilt(p, p, p, p, p, p, p, p)
    sizes = lambda eb, ld, ln, rows, maxn, nt=28: L.gtok_sent_decode_zinc_sizes(p, eb, None, ld, ln, rows, maxn, nt, p, p, p, None)
    csr = lambda eb, ld, ln, rows, maxn, nt=28, o=out: L.gtok_sent_decode_zinc_csr(p, eb, None, ld, ln, rows, maxn, nt, ctypes.byref(o), None)
    unremap = lambda eb, ld, ln, rows, maxn, nt=28, o=p: L.gtok_unremap_zinc(p, eb, None, ld, ln, rows, maxn, nt, 5, o, None)
    for call in (sizes, csr, unremap):
        assert call(3, 8, p, 4, 37) == -1 and call(0, 8, p, 4, 37) == -1 and call(8, 8, p, 4, 37) == -1      # elem_bytes
        assert call(4, 0, p, 4, 37) == -1 and call(4, -1, p, 4, 37) == -1                                     # ld <= 0
        assert call(4, 8, p, -1, 37) == -1 and call(4, 8, p, 4, -1) == -1 and call(4, 8, p, 4, 37, -1) == -1  # negative sizes
        assert call(4, 8, None, 4, 37) == -1                                                                  # null len
        assert call(4, 8, p, 4, _lib.SENT_LARGE_MAX_NODES + 1) == -2                                          # GTOK_E_TOO_LARGE
        assert call(4, 8, p, 0, 37) == 0 and call(4, 8, None, 0, 37) == 0                                     # no rows: a no-op
    assert unremap(4, 8, p, 4, 37, o=None) == -1                                                              # null out_ids
    assert unremap(4, 8, p, 4, _lib.SENT_LARGE_MAX_NODES + 1, o=None) == -2
    assert L.gtok_sent_decode_zinc_sizes(p, 4, None, 8, p, 4, 37, 28, None, p, p, None) == -1
    assert csr(4, 8, p, 4, 37, o=_lib.GtokCsrBuilt(p, p, p, None, p, p, p, p)) == -1
    assert csr(4, 8, p, 4, 37, o=_lib.GtokCsrBuilt(p, p, p, p, p, None, None, p)) == -1                      # always labelled: the type arrays
    assert L.gtok_sent_decode_zinc_csr(p, 4, None, 8, p, 4, 37, 28, None, None) == -1
    assert list(buf) == [0] * 64


def test_torch_ops_are_cuda_only_and_their_meta_kernels_give_the_documented_shapes():
    for n in ("unremap_zinc", "sent_decode_zinc_sizes", "sent_decode_zinc_csr"):
        assert hasattr(torch.ops.gtok, n), n
    ids = torch.zeros((5, 16), dtype=torch.int32); ln = torch.full((5,), 16, dtype=torch.int32)
    node_ptr, edge_ptr = torch.zeros(6, dtype=torch.int32), torch.zeros(6, dtype=torch.int64)
    with pytest.raises((NotImplementedError, RuntimeError)):        # no CPU kernel exists
        torch.ops.gtok.unremap_zinc(ids, ln, 37, 28)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.gtok.sent_decode_zinc_sizes(ids, ln, 37, 28)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.gtok.sent_decode_zinc_csr(ids, ln, 37, 28, node_ptr, edge_ptr, 40, 90)
    m = lambda t: t.to("meta")
    un = torch.ops.gtok.unremap_zinc(m(ids).to(torch.int16), m(ln), 37, 28)
    assert tuple(un.shape) == (5, 16) and un.dtype == torch.int32
    nn, ne, st = torch.ops.gtok.sent_decode_zinc_sizes(m(ids), m(ln), 37, 28)
    assert [tuple(t.shape) for t in (nn, ne, st)] == [(5,)] * 3 and {t.dtype for t in (nn, ne, st)} == {torch.int32}
    out = torch.ops.gtok.sent_decode_zinc_csr(m(ids).to(torch.int16), m(ln), 37, 28, m(node_ptr), m(edge_ptr), 40, 90)
    assert [tuple(t.shape) for t in out] == [(45,), (90,), (90,), (40,), (90,), (8,)]
    assert [t.dtype for t in out] == [torch.int32] * 3 + [torch.uint8] * 2 + [torch.int32]
    # packed rows: a flat 8-bit buffer with row_start and the width of the result
    flat, starts = torch.zeros(80, dtype=torch.uint8, device="meta"), torch.zeros(5, dtype=torch.int64, device="meta")
    assert tuple(torch.ops.gtok.unremap_zinc(flat, m(ln), 37, 28, starts, 16).shape) == (5, 16)
    out = torch.ops.gtok.sent_decode_zinc_csr(flat, m(ln), 37, 28, m(node_ptr), m(edge_ptr), 7, 12, starts, 16)
    assert tuple(out[0].shape) == (12,) and tuple(out[1].shape) == (12,) and tuple(out[3].shape) == (7,)


def test_method_signatures_and_what_they_refuse():
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(gtok.ops.unremap_zinc) == ["ids", "ln", "max_num_nodes", "num_node_types", "row_start", "ld", "pad_id"]
    assert inspect.signature(gtok.ops.unremap_zinc).parameters["pad_id"].default == gtok.ops.SENT_PAD
    assert sig(gtok.ops.sent_decode_zinc_sizes) == ["ids", "ln", "max_num_nodes", "num_node_types", "row_start", "ld"]
    assert sig(gtok.ops.sent_decode_zinc_csr) == ["ids", "ln", "max_num_nodes", "num_node_types", "row_start", "check_symmetric", "ld"]
    tok = gtok.Graph2TrailTokenizer(dataset_names=[], max_length=64, labeled_graph=True, device="cpu")
    assert sig(tok.decode_batch_zinc) == ["ids", "ln", "row_start", "check_symmetric"]
    assert sig(tok.decode_batch_like_zinc) == ["ids", "ln", "like", "order", "row_start", "check_symmetric"]
    assert sig(tok.decode_zinc) == ["tokens"]
    assert sig(tok.decode_batch_like) == ["ids", "ln", "like", "order", "row_start", "check_symmetric"]      # (unchanged)
    assert sig(gtok.agtt.TokenizedGraphDataset.decode_rows) == ["self", "ids", "ln", "row_start"]
    ids, ln = torch.zeros((1, 4), dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError):                # set_num_nodes() first, as for tokenize_batch
        tok.decode_batch_zinc(ids, ln)
    tok.set_num_nodes(37); tok.set_num_node_and_edge_types(28, 4)
    with pytest.raises(gtok.GtokError):              # host tensors: refused, never decoded on the CPU
        tok.decode_batch_zinc(ids, ln)
    with pytest.raises(gtok.GtokError):
        gtok.ops.unremap_zinc(ids, ln, 37, 28)
    with pytest.raises(gtok.GtokError):
        gtok.ops.sent_decode_zinc_sizes(ids, ln, 37, 28)


def test_unlabelled_tokenizers_are_refused():
    """unlabelled remapped rows are ambiguous (position X position): no entry point, and the tokenizer says so"""
    tok = gtok.Graph2TrailTokenizer(dataset_names=[], max_length=64, labeled_graph=False, device="cpu")
    tok.set_num_nodes(37)
    ids, ln = torch.zeros((1, 4), dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="labelled"):
        tok.decode_batch_zinc(ids, ln)
    with pytest.raises(ValueError, match="labelled"):
        tok.decode_batch_like_zinc(ids, ln, None, None)
    with pytest.raises(ValueError, match="labelled"):
        tok.decode_zinc([0, 1])


# ------------------------------------------------------------------------------------------------ the reference against the oracle
def test_pre_inverts_the_oracles_remap():
    for M, T in ((37, 28), (37, 9), (8, 28), (8, 3), (1, 0)):
        node_off, edge_off = 6 + M, 6 + M + T
        raw = np.array([t for t in range(edge_off + 300) if t not in (1, 2, 3, 5)], np.int32)[None, :]
        ids = orc.remap_zinc(raw, np.array([raw.shape[1]]), 6, node_off, edge_off)[0]
        assert [remap(int(t), M, T) for t in raw[0]] == ids.tolist(), (M, T)
        assert [pre(int(i), M, T) for i in ids] == raw[0].tolist(), (M, T)
        folded = orc.remap_zinc(np.array([[1, 2, 3, 5]], np.int32), np.array([4]), 6, node_off, edge_off)[0]
        assert folded.tolist() == [X] * 4 and pre(X, M, T) is NONE and pre(-1, M, T) is NONE and pre(21, M, T) is NONE


@pytest.mark.parametrize("max_len", [4096, 50])
def test_unfold_of_the_oracles_remapped_molecules_is_its_raw_rows(max_len):
    _, coo = both(gtok.synth.zinc_like(300, seed=21))
    kw = dict(labeled=True, num_node_types=28, num_edge_types=4)
    ids, ln = orc.sent(coo, 37, max_len, 5, 3, remap_zinc=True, **kw)
    raw, rln = orc.sent(coo, 37, max_len, 5, 3, **kw)
    assert np.array_equal(ln, rln) and int(ids.max()) == 97
    got = unfold_rows(ids, ln, 37, 28)
    ends_in_x = ids[np.arange(300), ln - 1] == X
    last = np.zeros_like(got, bool)
    last[np.nonzero(ends_in_x)[0], ln[ends_in_x] - 1] = True
    assert np.array_equal(got[~last], raw[~last])                         # padding included
    assert ((got[last] == raw[last]) | ((got[last] == 1) & (raw[last] == 2))).all()
    if max_len == 4096:
        assert not ends_in_x.any()
        at63 = (ln > 64) & (ids[:, 63] == X)                              # the folded id at a chunk's last token, in all three roles
        assert np.bincount(raw[at63, 63], minlength=4).tolist() == [0, 19, 8, 10]
    else:
        assert ends_in_x.sum() > 10 and (got[last] != raw[last]).any()
    a = orc.sent_decode_rows(got, ln, 37, True, 28); b = orc.sent_decode_rows(raw, ln, 37, True, 28)
    assert all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("M,T,ET", [(8, 28, 6), (8, 3, 2)])
def test_unfold_of_the_hand_made_graphs_with_out_of_range_types(M, T, ET):
    _, coo = both(edge_case_graphs())
    kw = dict(labeled=True, num_node_types=T, num_edge_types=ET)
    for max_len in (4096, 9, 5, 2, 1):
        ids, ln = orc.sent(coo, M, max_len, 3, 2, remap_zinc=True, **kw)
        raw, _ = orc.sent(coo, M, max_len, 3, 2, **kw)
        got = unfold_rows(ids, ln, M, T)
        for g, k in np.argwhere(got != raw):
            assert k == ln[g] - 1 and ids[g, k] == X and got[g, k] == 1 and raw[g, k] == 2, (max_len, g, k)
        a = orc.sent_decode_rows(got, ln, M, True, T); b = orc.sent_decode_rows(raw, ln, M, True, T)
        assert all(np.array_equal(a[k], b[k]) for k in a), max_len
