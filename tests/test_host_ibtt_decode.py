"""gtok_ibtt_decode_sizes / gtok_ibtt_decode_csr, the parts that need no GPU: ops.ibtt_inverse_lut, the binding, the host-side
argument errors, the torch ops' meta kernels - and the yardstick of the GPU tests itself: the host reference decoder
(tests/_ibtt_decode_ref.py) gives back the input graphs on rows of the CPU oracle's serialisers."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import _ibtt_decode_ref as ref
from _util import gtok, orc, zinc_vocab

_lib = gtok._lib
NAMES = ("gtok_ibtt_decode_sizes", "gtok_ibtt_decode_csr")


def synth_vocab(num_node_ids):
    toks = ["<pad>", "<bos>", "<eos>", "<e>", "<n>", "<q>", "<p>", "yes", "no"] + [str(i) for i in range(num_node_ids)]
    return {t: i for i, t in enumerate(toks)}


def test_inverse_lut_gives_minus_one_for_shared_pad_and_unowned_ids():
    v = zinc_vocab(12, with_fallbacks=False)                 # no 'X', no 'unknown': both slots hold <pad>'s id
    lut = gtok.ops.zinc_lut(v, 12)
    inv = gtok.ops.ibtt_inverse_lut(lut, len(v))
    assert inv.dtype == torch.int32 and tuple(inv.shape) == (len(v),) and inv.device.type == "cpu"
    assert int(inv[v["<pad>"]]) == -1 and int(inv[v["<unk>"]]) == -1
    assert int(inv[v["<bos>"]]) == 0 and int(inv[v["C"]]) == 7 and int(inv[v["aromatic"]]) == 21 and int(inv[v["11"]]) == 22 + 11
    assert np.array_equal(inv.numpy(), ref.inverse_lut(lut.numpy(), len(v)))
    # node ids the vocab lacks map to pad: pad is shared, every other id keeps its slot
    lut20 = gtok.ops.zinc_lut(v, 20)
    inv20 = gtok.ops.ibtt_inverse_lut(lut20, len(v))
    assert int(inv20[v["<pad>"]]) == -1 and int(inv20[v["11"]]) == 33
    # a LUT id outside [0, vocab_size) has no entry; a smaller table simply ends sooner
    small = gtok.ops.ibtt_inverse_lut(lut, 10)
    assert tuple(small.shape) == (10,) and np.array_equal(small.numpy(), inv.numpy()[:10])
    weird = gtok.ops.ibtt_inverse_lut(torch.tensor([3, -1, 99, 3, 4], dtype=torch.int32), 6)
    assert weird.tolist() == [-1, -1, -1, -1, 4, -1]
    with pytest.raises(ValueError):
        gtok.ops.ibtt_inverse_lut(lut, 0)
    # one absent token alone would own <pad>'s id: pad_id names no token
    full = zinc_vocab(12)
    lacking = {t: i for t, i in full.items() if t != "7"}
    lut7 = gtok.ops.zinc_lut(lacking, 12)
    assert int(lut7[22 + 7]) == lacking["<pad>"] and int(gtok.ops.ibtt_inverse_lut(lut7, len(full))[lacking["<pad>"]]) == 22 + 7
    inv7 = gtok.ops.ibtt_inverse_lut(lut7, len(full), lacking["<pad>"])
    assert int(inv7[lacking["<pad>"]]) == -1 and int(inv7[lacking["8"]]) == 22 + 8
    assert np.array_equal(inv7.numpy(), ref.inverse_lut(lut7.numpy(), len(full), lacking["<pad>"]))


def _molecules(n_graphs, seed):
    d = gtok.synth.zinc_like(n_graphs, seed=seed)
    d["x"] = d["x"] % 9                                      # the nine symbols: 'X' (a type outside 0..8) comes back as 255
    return d, orc.Coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], d["x"], d["edge_attr"])


def _same(got, want, keys):
    for k in keys:
        a, b = getattr(got, k), getattr(want, k)
        assert (a is None) == (b is None), k
        assert a is None or torch.equal(a, b), k


def test_reference_decoder_gives_back_the_molecules_the_oracle_serialised():
    d, coo = _molecules(60, 3)
    v = zinc_vocab(40)
    lut = gtok.ops.zinc_lut(v, 40)
    ids, ln = orc.ibtt_zinc(coo, lut.numpy(), 4096, v["<pad>"], 256)
    inv = ref.inverse_lut(lut.numpy(), len(v))
    exp = ref.expected(ref.rows_of(ids, ln), ref.ZINC, inv, 40)
    assert (exp["status"] == 0).all()
    want = gtok.GraphBatch.from_coo(d["node_counts"], d["edge_counts"], d["src"], d["dst"], d["x"], d["edge_attr"], check_symmetric=False)
    _same(exp["batch"], want, ("node_ptr", "edge_ptr", "rowptr", "col", "nattr", "eattr"))
    for k in ("max_degree", "max_nodes", "max_edges", "chunk_nodes", "chunk_edges"):
        assert getattr(exp["batch"], k) == getattr(want, k), k
    # cut rows: a prefix of the molecule, never a malformed row
    ids, ln = orc.ibtt_zinc(coo, lut.numpy(), 30, v["<pad>"], 32)
    exp = ref.expected(ref.rows_of(ids, ln), ref.ZINC, inv, 40)
    assert set(exp["status"].tolist()) == {3} and (exp["node_counts"] <= d["node_counts"]).all() and exp["node_counts"].max() > 0


def test_reference_decoder_gives_back_the_edge_lists_the_oracle_serialised():
    rng = np.random.default_rng(5)
    nc = rng.integers(1, 30, 40)
    ec = rng.integers(0, 50, 40)
    src = np.concatenate([rng.integers(0, n, e) for n, e in zip(nc, ec)]); dst = np.concatenate([rng.integers(0, n, e) for n, e in zip(nc, ec)])
    v = synth_vocab(30)
    lut = gtok.ops.synth_lut(v, 30)
    query = np.zeros((40, 4), np.int32)
    query[:, 0] = np.arange(40) % 4
    for g in range(40):
        query[g, 1:1 + query[g, 0]] = rng.integers(7, len(v), query[g, 0])
    ids, ln = orc.ibtt_synth(orc.Coo(nc, ec, src, dst), lut.numpy(), query, 4096, v["<pad>"], 256)
    inv = ref.inverse_lut(lut.numpy(), len(v))
    exp = ref.expected(ref.rows_of(ids, ln), ref.SYNTH, inv, 30)
    assert (exp["status"] == 0).all() and np.array_equal(exp["query"], query)
    want = gtok.GraphBatch.from_coo(nc, ec, src, dst, check_symmetric=False)
    _same(exp["batch"], want, ("node_ptr", "edge_ptr", "rowptr", "col", "eorder"))
    ids, ln = orc.ibtt_synth(orc.Coo(nc, ec, src, dst), lut.numpy(), query, 20, v["<pad>"], 20)
    exp = ref.expected(ref.rows_of(ids, ln), ref.SYNTH, inv, 30)
    assert 1 not in exp["status"].tolist() and 3 in exp["status"].tolist()


def test_the_entry_points_are_bound_by_symbol_with_their_arity():
    L = _lib.lib()
    for n in NAMES:
        assert n in _lib.SYMBOLS and hasattr(L, n), n
    assert len(L.gtok_ibtt_decode_sizes.argtypes) == 15 and len(L.gtok_ibtt_decode_csr.argtypes) == 12
    assert L.gtok_ibtt_decode_csr.argtypes[10] == ctypes.POINTER(_lib.GtokCsrBuilt)
    assert set(_lib.IBTT_DECODE_SYMBOLS) == set(NAMES) and not set(NAMES) & set(_lib.OPTIONAL_SYMBOLS)
    assert _lib.ABI_VERSION == 8 and L.gtok_version() == 8


def test_host_side_argument_errors_come_before_any_device_is_asked_for():
    L = _lib.lib()
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.addressof(buf)
    out = _lib.GtokCsrBuilt(p, p, p, p, p, p, p, p)
    sizes = lambda eb, ld, ln, rows, gr, inv, il, maxn: L.gtok_ibtt_decode_sizes(p, eb, None, ld, ln, rows, gr, inv, il, maxn, p, p, p, None, None)
    csr = lambda eb, ld, ln, rows, gr, inv, il, maxn, o=out: L.gtok_ibtt_decode_csr(p, eb, None, ld, ln, rows, gr, inv, il, maxn, ctypes.byref(o), None)
    for call in (sizes, csr):
        assert call(3, 8, p, 4, 0, p, 8, 37) == -1 and call(0, 8, p, 4, 0, p, 8, 37) == -1                    # elem_bytes
        assert call(4, 0, p, 4, 0, p, 8, 37) == -1 and call(4, -1, p, 4, 1, p, 8, 37) == -1                   # ld <= 0
        assert call(4, 8, p, -1, 0, p, 8, 37) == -1 and call(4, 8, p, 4, 0, p, 8, -1) == -1                   # negative sizes
        assert call(4, 8, p, 4, 2, p, 8, 37) == -1 and call(4, 8, p, 4, -1, p, 8, 37) == -1                   # grammar
        assert call(4, 8, p, 4, 0, p, 0, 37) == -1 and call(4, 8, p, 4, 0, None, 8, 37) == -1                 # inv_len <= 0, null inv
        assert call(4, 8, None, 4, 0, p, 8, 37) == -1                                                         # null len
        assert call(4, 8, p, 4, 1, p, 8, _lib.SENT_LARGE_MAX_NODES + 1) == -2                                 # GTOK_E_TOO_LARGE
        assert call(4, 8, p, 0, 0, p, 8, 37) == 0 and call(4, 8, None, 0, 1, None, 8, 37) == 0                # no rows: a no-op
    assert L.gtok_ibtt_decode_sizes(p, 4, None, 8, p, 4, 0, p, 8, 37, None, p, p, None, None) == -1
    assert csr(4, 8, p, 4, 1, p, 8, 37, _lib.GtokCsrBuilt(p, p, p, None, p, p, p, p)) == -1
    assert csr(4, 8, p, 4, 0, p, 8, 37, _lib.GtokCsrBuilt(p, p, p, p, p, None, None, p)) == -1              # molecules need the type arrays
    assert list(buf) == [0] * 64


def test_torch_ops_are_cuda_only_and_their_meta_kernels_give_the_documented_shapes():
    assert hasattr(torch.ops.gtok, "ibtt_decode_sizes") and hasattr(torch.ops.gtok, "ibtt_decode_csr")
    ids = torch.zeros((5, 16), dtype=torch.int32); ln = torch.full((5,), 16, dtype=torch.int32); inv = torch.zeros(9, dtype=torch.int32)
    with pytest.raises((NotImplementedError, RuntimeError)):        # no CPU kernel exists
        torch.ops.gtok.ibtt_decode_sizes(ids, ln, 0, inv, 37)
    node_ptr, edge_ptr = torch.zeros(6, dtype=torch.int32), torch.zeros(6, dtype=torch.int64)
    m = lambda t: t.to("meta")
    out = torch.ops.gtok.ibtt_decode_sizes(m(ids), m(ln), 1, m(inv), 37)
    assert [tuple(t.shape) for t in out] == [(5,), (5,), (5,), (5, 4)] and {t.dtype for t in out} == {torch.int32}
    for grammar in (0, 1):
        out = torch.ops.gtok.ibtt_decode_csr(m(ids), m(ln), grammar, m(inv), 37, m(node_ptr), m(edge_ptr), 40, 90)
        want = [(45,), (90,), (90,), (40,) if grammar == 0 else (0,), (90,) if grammar == 0 else (0,), (8,)]
        assert [tuple(t.shape) for t in out] == want
        assert [t.dtype for t in out] == [torch.int32] * 3 + [torch.uint8] * 2 + [torch.int32]


def test_python_layer_and_the_dataset_method():
    params = list(inspect.signature(gtok.ops.ibtt_decode_csr).parameters)
    assert params == ["ids", "ln", "grammar", "inv", "max_num_nodes", "row_start", "ld", "check_symmetric"]
    with pytest.raises(gtok.GtokError):               # host tensors: refused, never decoded on the CPU
        gtok.ops.ibtt_decode_sizes(torch.zeros((2, 4), dtype=torch.int32), torch.zeros(2, dtype=torch.int32), "zinc", torch.zeros(4, dtype=torch.int32), 37)
    ds_mod = gtok.graph_data_loader.zinc_dataset_indexbase
    assert list(inspect.signature(ds_mod.ZINCTokenizationDataset.decode_batch).parameters)[:3] == ["self", "ids", "ln"]
