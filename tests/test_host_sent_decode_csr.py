"""gtok_sent_decode_sizes / gtok_sent_decode_csr, the parts that need no GPU: the binding of the two entry points by symbol, the
torch ops' registration and meta kernels, the tokenizer's methods, the argument checks of the Python layer."""
import ctypes
import inspect

import pytest
import torch

from _util import gtok

_lib = gtok._lib
NAMES = ("gtok_sent_decode_sizes", "gtok_sent_decode_csr")


def test_the_entry_points_are_bound_by_symbol_with_their_arity():
    L = _lib.lib()
    for n in NAMES:
        assert n in _lib.SYMBOLS and hasattr(L, n), n
    assert len(L.gtok_sent_decode_sizes.argtypes) == 13 and len(L.gtok_sent_decode_csr.argtypes) == 11
    assert L.gtok_sent_decode_csr.argtypes[9] == ctypes.POINTER(_lib.GtokCsrBuilt)
    assert L.gtok_sent_decode_sizes.restype is ctypes.c_int32 and L.gtok_sent_decode_csr.restype is ctypes.c_int32
    # a tuple of their own: a library of the same ABI version that lacks them still loads (GTOK_LIB, A/B timing)
    assert set(_lib.DECODE_CSR_SYMBOLS) == set(NAMES) and not set(NAMES) & set(_lib.OPTIONAL_SYMBOLS)
    assert _lib.ABI_VERSION == 8 and L.gtok_version() == 8


def test_host_side_argument_errors_come_before_any_device_is_asked_for():
    """null pointers / sizes / widths are refused by host code alone: these calls run without a GPU"""
    L = _lib.lib()
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.addressof(buf)
    out = _lib.GtokCsrBuilt(p, p, p, p, p, p, p, p)
    sizes = lambda eb, ld, ln, rows, maxn: L.gtok_sent_decode_sizes(p, eb, None, ld, ln, rows, maxn, 0, 0, p, p, p, None)
    csr = lambda eb, ld, ln, rows, maxn, o=out: L.gtok_sent_decode_csr(p, eb, None, ld, ln, rows, maxn, 0, 0, ctypes.byref(o), None)
    for call in (sizes, csr):
        assert call(3, 8, p, 4, 37) == -1 and call(0, 8, p, 4, 37) == -1 and call(8, 8, p, 4, 37) == -1      # elem_bytes
        assert call(4, 0, p, 4, 37) == -1 and call(4, -1, p, 4, 37) == -1                                     # ld <= 0
        assert call(4, 8, p, -1, 37) == -1 and call(4, 8, p, 4, -1) == -1                                     # negative sizes
        assert call(4, 8, None, 4, 37) == -1                                                                  # null len
        assert call(4, 8, p, 4, _lib.SENT_LARGE_MAX_NODES + 1) == -2                                          # GTOK_E_TOO_LARGE
        assert call(4, 8, p, 0, 37) == 0 and call(4, 8, None, 0, 37) == 0                                     # no rows: a no-op
    assert L.gtok_sent_decode_sizes(p, 4, None, 8, p, 4, 37, 0, 0, None, p, p, None) == -1
    assert csr(4, 8, p, 4, 37, _lib.GtokCsrBuilt(p, p, p, None, p, p, p, p)) == -1
    assert L.gtok_sent_decode_csr(p, 4, None, 8, p, 4, 37, 1, 0, ctypes.byref(_lib.GtokCsrBuilt(p, p, p, p, p, None, None, p)), None) == -1
    assert list(buf) == [0] * 64


def test_torch_ops_are_cuda_only_and_their_meta_kernels_give_the_documented_shapes():
    assert hasattr(torch.ops.gtok, "sent_decode_sizes") and hasattr(torch.ops.gtok, "sent_decode_csr")
    ids = torch.zeros((5, 16), dtype=torch.int32); ln = torch.full((5,), 16, dtype=torch.int32)
    with pytest.raises((NotImplementedError, RuntimeError)):        # no CPU kernel exists
        torch.ops.gtok.sent_decode_sizes(ids, ln, 37, True, 9)
    node_ptr, edge_ptr = torch.zeros(6, dtype=torch.int32), torch.zeros(6, dtype=torch.int64)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.gtok.sent_decode_csr(ids, ln, 37, True, 9, node_ptr, edge_ptr, 40, 90)
    m = lambda t: t.to("meta")
    nn, ne, st = torch.ops.gtok.sent_decode_sizes(m(ids), m(ln), 37, True, 9)
    assert [tuple(t.shape) for t in (nn, ne, st)] == [(5,)] * 3 and {t.dtype for t in (nn, ne, st)} == {torch.int32}
    for labeled in (True, False):
        out = torch.ops.gtok.sent_decode_csr(m(ids).to(torch.int16), m(ln), 37, labeled, 9, m(node_ptr), m(edge_ptr), 40, 90)
        want = [(45,), (90,), (90,), (40,) if labeled else (0,), (90,) if labeled else (0,), (8,)]
        assert [tuple(t.shape) for t in out] == want
        assert [t.dtype for t in out] == [torch.int32] * 3 + [torch.uint8] * 2 + [torch.int32]
    # packed rows: a flat buffer with row_start
    out = torch.ops.gtok.sent_decode_csr(torch.zeros(80, dtype=torch.uint8, device="meta"), m(ln), 37, False, 0, m(node_ptr), m(edge_ptr), 7, 12,
                                         torch.zeros(5, dtype=torch.int64, device="meta"), 16)
    assert tuple(out[0].shape) == (12,) and tuple(out[1].shape) == (12,)


def test_tokenizer_has_decode_and_decode_batch():
    tok = gtok.Graph2TrailTokenizer(dataset_names=[], max_length=64, labeled_graph=True, device="cpu")
    assert list(inspect.signature(tok.decode_batch).parameters) == ["ids", "ln", "row_start", "check_symmetric"]
    assert list(inspect.signature(tok.decode).parameters) == ["tokens"]
    with pytest.raises(RuntimeError):                # set_num_nodes() first, as for tokenize_batch
        tok.decode_batch(torch.zeros((1, 4), dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    tok.set_num_nodes(37); tok.set_num_node_and_edge_types(9, 4)
    with pytest.raises(gtok.GtokError):              # host tensors: refused, never decoded on the CPU
        tok.decode_batch(torch.zeros((1, 4), dtype=torch.int32), torch.zeros(1, dtype=torch.int32))


def test_python_layer_refuses_rows_it_cannot_describe():
    params = list(inspect.signature(gtok.ops.sent_decode_csr).parameters)
    assert params[:7] == ["ids", "ln", "max_num_nodes", "labeled", "num_node_types", "row_start", "check_symmetric"]
    with pytest.raises(gtok.GtokError):
        gtok.ops.sent_decode_sizes(torch.zeros((2, 4), dtype=torch.int32), torch.zeros(2, dtype=torch.int32), 37)
