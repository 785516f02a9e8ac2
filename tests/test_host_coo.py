"""torch.ops.gtok.csr_from_coo's fake kernel and ops.csr_from_coo's argument checks: both answer before any launch, no GPU needed."""
import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from _util import gtok


def test_csr_from_coo_fake_kernel_shapes_and_dtypes():
    with FakeTensorMode():
        i64 = lambda n: torch.empty(n, dtype=torch.int64, device="cuda")
        src, dst, ns, es = i64(120), i64(120), i64(11), i64(11)
        x, ea = torch.empty(47, 3, dtype=torch.int64, device="cuda"), i64(120)
        out = torch.ops.gtok.csr_from_coo(src, dst, ns, es, x, ea, None, 47, 120, True)
        assert [tuple(t.shape) for t in out] == [(11,), (11,), (57,), (120,), (120,), (47,), (120,), (8,)]
        assert [t.dtype for t in out] == [torch.int32, torch.int64, torch.int32, torch.int32, torch.int32, torch.uint8, torch.uint8, torch.int32]
        sub = torch.ops.gtok.csr_from_coo(src, dst, ns, es, None, None, i64(4), 20, 33, False)
        assert [tuple(t.shape) for t in sub] == [(5,), (5,), (24,), (33,), (33,), (0,), (0,), (8,)]


@pytest.mark.parametrize("case, match", [
    (dict(dst=np.zeros(5, np.int64)), "one length"),
    (dict(src=np.zeros((2, 6), np.int64)), "1-D"),
    (dict(edge_slices=np.array([0, 6], np.int64)), "differ in length"),
    (dict(node_slices=np.zeros((2, 2), np.int64)), "S \\+ 1 offsets"),
    (dict(edge_attr=np.zeros(5, np.int64)), "edge_attr length"),
    (dict(x=np.zeros(4, np.int64)), "x length"),
    (dict(x=np.zeros((7, 0), np.int64)), "no column"),
    (dict(indices=np.zeros((2, 2), np.int64)), "indices must be 1-D"),
    (dict(indices=np.array([0.5])), "integers"),
    (dict(num_nodes=2 ** 31), "int32 node offsets"),
    (dict(num_entries=-1), ">= 0"),
])
def test_csr_from_coo_rejects_bad_arguments_before_any_launch(case, match):
    args = dict(src=np.array([0, 1, 1, 2, 0, 0], np.int64), dst=np.array([1, 0, 2, 1, 0, 0], np.int64),
                node_slices=np.array([0, 3, 7], np.int64), edge_slices=np.array([0, 4, 5, 6], np.int64)[[0, 1, 3]])
    args.update(case)
    with pytest.raises(ValueError, match=match):
        gtok.ops._coo_prepare(args.pop("src"), args.pop("dst"), args.pop("node_slices"), args.pop("edge_slices"), args.get("x"),
                              args.get("edge_attr"), args.get("indices"), args.get("num_nodes"), args.get("num_entries"), "cuda:0")


def test_csr_from_coo_refuses_a_cpu_build():
    with pytest.raises(gtok.GtokError, match="GPU"):
        gtok.ops.csr_from_coo(np.zeros(1, np.int64), np.zeros(1, np.int64), np.array([0, 1]), np.array([0, 1]), device="cpu")
    with pytest.raises(ValueError, match="builder"):
        gtok.GraphBatch.from_coo_device([1], [0], [], [], device="cpu", builder="hip")


def test_from_coo_device_off_the_gpu_sets_the_flags_from_coo_sets():
    """check_symmetric=True on a non-CUDA device: the same GTOK_CSR_SIMPLE_SYMMETRIC verdict, and the same `checked`, as
    from_coo - on a clean corpus, one with a self loop and one with an entry whose reverse is missing."""
    d = gtok.synth.zinc_like(300, seed=7)
    ep = np.concatenate([[0], np.cumsum(d["edge_counts"])])
    k = int(ep[17]) + 3                                    # an entry of graph 17
    loop = dict(d, dst=d["dst"].copy())
    loop["dst"][k] = loop["src"][k]
    ec = d["edge_counts"].copy(); ec[17] -= 1
    missing = dict(d, src=np.delete(d["src"], k), dst=np.delete(d["dst"], k), edge_attr=np.delete(d["edge_attr"], k), edge_counts=ec)
    verdicts = []
    for c in (d, loop, missing):
        args = (c["node_counts"], c["edge_counts"], c["src"], c["dst"], c["x"], c["edge_attr"])
        h = gtok.GraphBatch.from_coo(*args, check_symmetric=True)
        b = gtok.GraphBatch.from_coo_device(*args, device="cpu", builder="torch", check_symmetric=True)
        assert (b.flags, b.checked) == (h.flags, h.checked)
        assert torch.equal(b.rowptr, h.rowptr) and torch.equal(b.col, h.col)
        verdicts.append(bool(h.flags & gtok._lib.CSR_SIMPLE_SYMMETRIC))
    assert verdicts == [True, False, False]
    # check_symmetric=False: no verdict either way
    assert gtok.GraphBatch.from_coo_device(*args[:4], device="cpu", builder="torch", check_symmetric=False).flags == 0
