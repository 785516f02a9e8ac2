"""gtok_ibtt_zinc's kernel choice, pinned on the host: gtok_ibtt_zinc_kernel_name reads scalars of the struct it is given, so it runs
without a GPU and without any device array behind the pointers."""
import ctypes
import itertools

import pytest

from _util import gtok

_lib = gtok._lib

GRAPHS = (1, 1023, 1024, 250000)
SHAPES = ((38, 80), (48, 96), (49, 96), (255, 255), (256, 255), (255, 256), (300, 6000), (300, 6001), (65535, 6000), (65536, 100))   # (max_nodes, max_edges)
SYMMETRIC = (True, False)           # GTOK_CSR_SIMPLE_SYMMETRIC
EORDER = (False, True)              # the batch claims an eorder array (its entries are not in list order)
PINS = (None, "", "lane", "quad", "wave")           # GTOK_IBTT_KERNEL
INNER = list(itertools.product(SYMMETRIC, EORDER, PINS))        # 20 cells per (graphs, shape), in this order

NAMES = {"w": "ibtt_zinc_kernel", "l": "ibtt_zinc_lane_kernel", "q": "ibtt_zinc_quad_kernel"}

# What gtok_ibtt_zinc_kernel_name of the commit BEFORE gtok_ibtt_zinc was split into one launcher per kernel answered over the grid:
# one row per (graphs, shape) in GRAPHS x SHAPES order, one letter of NAMES per cell of INNER.  Recorded from that commit's library,
# never recomputed from the code under test (GTOK_LIB=<that library> runs this very table against it).
EXPECTED = """
wwlqwwwwwwwwwwwwwwww
wwlqwwwwwwwwwwwwwwww
wwlqwwwwwwwwwwwwwwww
wwlqwwwwwwwwwwwwwwww
wwwqwwwwwwwwwwwwwwww
wwwqwwwwwwwwwwwwwwww
wwwqwwwwwwwwwwwwwwww
wwwwwwwwwwwwwwwwwwww
wwwqwwwwwwwwwwwwwwww
wwwwwwwwwwwwwwwwwwww
wwlqwwwwwwwwwwwwwwww
wwlqwwwwwwwwwwwwwwww
wwlqwwwwwwwwwwwwwwww
wwlqwwwwwwwwwwwwwwww
wwwqwwwwwwwwwwwwwwww
wwwqwwwwwwwwwwwwwwww
wwwqwwwwwwwwwwwwwwww
wwwwwwwwwwwwwwwwwwww
wwwqwwwwwwwwwwwwwwww
wwwwwwwwwwwwwwwwwwww
qqlqwwwwwwwwwwwwwwww
qqlqwwwwwwwwwwwwwwww
qqlqwwwwwwwwwwwwwwww
qqlqwwwwwwwwwwwwwwww
qqqqwwwwwwwwwwwwwwww
qqqqwwwwwwwwwwwwwwww
qqqqwwwwwwwwwwwwwwww
wwwwwwwwwwwwwwwwwwww
qqqqwwwwwwwwwwwwwwww
wwwwwwwwwwwwwwwwwwww
qqlqwwwwwwwwwwwwwwww
qqlqwwwwwwwwwwwwwwww
qqlqwwwwwwwwwwwwwwww
qqlqwwwwwwwwwwwwwwww
qqqqwwwwwwwwwwwwwwww
qqqqwwwwwwwwwwwwwwww
qqqqwwwwwwwwwwwwwwww
wwwwwwwwwwwwwwwwwwww
qqqqwwwwwwwwwwwwwwww
wwwwwwwwwwwwwwwwwwww
""".split()


def make_csr(graphs, max_nodes, max_edges, symmetric=False, eorder=False):
    """A gtok_csr of scalars alone; the array it names is a claim (address 1), which gtok_ibtt_zinc_kernel_name never follows."""
    cs = _lib.GtokCsr()
    cs.num_graphs, cs.max_nodes, cs.max_edges = graphs, max_nodes, max_edges
    cs.flags = _lib.CSR_SIMPLE_SYMMETRIC if symmetric else 0
    if eorder:
        cs.eorder = 1
    return cs


def kernel_name(cs):
    return gtok.lib().gtok_ibtt_zinc_kernel_name(ctypes.byref(cs)).decode()


def set_pin(monkeypatch, pin):
    if pin is None:
        monkeypatch.delenv("GTOK_IBTT_KERNEL", raising=False)
    else:
        monkeypatch.setenv("GTOK_IBTT_KERNEL", pin)


def test_kernel_choice_table(monkeypatch):
    assert len(EXPECTED) == len(GRAPHS) * len(SHAPES) and all(len(row) == len(INNER) for row in EXPECTED)
    wrong = []
    for r, (graphs, shape) in enumerate(itertools.product(GRAPHS, SHAPES)):
        for c, (sym, eorder, pin) in enumerate(INNER):
            set_pin(monkeypatch, pin)
            got = kernel_name(make_csr(graphs, *shape, symmetric=sym, eorder=eorder))
            if got != NAMES[EXPECTED[r][c]]:
                wrong.append((graphs, shape, sym, eorder, pin, got, NAMES[EXPECTED[r][c]]))
    assert not wrong, f"{len(wrong)} cells differ, the first (graphs, shape, symmetric, eorder, pin, got, expected): {wrong[:5]}"
    # every kernel is in the table, and only batches in list order with the flag ever leave the wave kernel
    assert set("".join(EXPECTED)) == set(NAMES)
    assert all(set(row[len(PINS):]) == {"w"} for row in EXPECTED)


@pytest.mark.parametrize("graphs,max_nodes,max_edges,kw,pin,name", [
    (250000, 38, 80, dict(symmetric=True), None, "ibtt_zinc_quad_kernel"),
    (1023, 38, 80, dict(symmetric=True), None, "ibtt_zinc_kernel"),
    (1, 38, 80, dict(symmetric=True), "quad", "ibtt_zinc_quad_kernel"),
    (250000, 255, 255, dict(symmetric=True), "lane", "ibtt_zinc_lane_kernel"),
    (250000, 256, 255, dict(symmetric=True), "lane", "ibtt_zinc_quad_kernel"),         # a pin that does not apply leaves the default
    (250000, 300, 6001, dict(symmetric=True), "quad", "ibtt_zinc_kernel"),
    (250000, 38, 80, dict(symmetric=True), "wave", "ibtt_zinc_kernel"),
    (250000, 38, 80, dict(symmetric=True, eorder=True), "quad", "ibtt_zinc_kernel"),
    (250000, 38, 80, dict(), "lane", "ibtt_zinc_kernel"),
])
def test_kernel_choice_examples(monkeypatch, graphs, max_nodes, max_edges, kw, pin, name):
    set_pin(monkeypatch, pin)
    assert kernel_name(make_csr(graphs, max_nodes, max_edges, **kw)) == name


def test_no_batch_has_no_name():
    assert gtok.lib().gtok_ibtt_zinc_kernel_name(None).decode() == ""
