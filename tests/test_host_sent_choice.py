"""gtok_sent's kernel choice and ops.sent's mirror decision, pinned on the host: gtok_sent_kernel_name reads scalars of the
structs it is given, so it runs without a GPU and without any device array behind the pointers."""
import ctypes
import itertools
import os
import re

import pytest

from _util import ROOT, gtok

_lib, ops = gtok._lib, gtok.ops

GRAPHS = (1000, 2000, 19999, 20000, 27999, 28000, 125000)
SHAPES = ((38, 80), (64, 255), (64, 256), (65, 200), (128, 4000), (256, 4000), (300, 4000))      # (max_nodes, max_edges)
SYMMETRIC = (True, False)           # GTOK_CSR_SIMPLE_SYMMETRIC
EPOCHS = (1, 16)
MODES = ("plain", "labelled", "labelled+remap")
MIRROR = (False, True)              # the batch claims an adjacency bit-matrix mirror
PINS = (None, "lane", "reg", "lds", "blane")        # GTOK_SENT_KERNEL
INNER = list(itertools.product(SYMMETRIC, EPOCHS, MODES, MIRROR, PINS))      # 120 cells per (graphs, shape), in this order

NAMES = {"l": "sent_lane_kernel", "r": "sent_reg_kernel", "-": "",
         "1": "sent_lds_kernel<W=1>", "2": "sent_lds_kernel<W=2>", "4": "sent_lds_kernel<W=4>", "8": "sent_lds_kernel<W=8>",
         "a": "sent_blane_kernel<W=1>", "b": "sent_blane_kernel<W=2>", "c": "sent_blane_kernel<W=4>"}

# What gtok_sent_kernel_name of the commit BEFORE the launcher was split into one function per kernel answered over the grid:
# one row per (graphs, shape) in GRAPHS x SHAPES order, one letter of NAMES per cell of INNER.  Recorded from that commit's
# library, never recomputed from the code under test (GTOK_LIB=<that library> runs this very table against it).
EXPECTED = """
rlr1rrlr1arlr1rrlr1rrlr1rrlr1rrlr1rrlr1arlr1rrlr1rrlr1rrlr1rrrr1rrrr1arrr1rrrr1rrrr1rrrr1rrrr1rrrr1arrr1rrrr1rrrr1rrrr1r
rlr1rrlr1arlr1rrlr1rrlr1rrlr1rrlr1rrlr1arlr1rrlr1rrlr1rrlr1rrrr1rrrr1arrr1rrrr1rrrr1rrrr1rrrr1rrrr1arrr1rrrr1rrrr1rrrr1r
rrr1rrrr1arrr1rrrr1rrrr1rrrr1rrrr1rrrr1arrr1rrrr1rrrr1rrrr1rrrr1rrrr1arrr1rrrr1rrrr1rrrr1rrrr1rrrr1arrr1rrrr1rrrr1rrrr1r
222222222b22222222222222222222222222222b22222222222222222222222222222b22222222222222222222222222222b22222222222222222222
222222222b22222222222222222222222222222b22222222222222222222222222222b22222222222222222222222222222b22222222222222222222
444444444c44444444444444444444444444444c44444444444444444444444444444c44444444444444444444444444444c44444444444444444444
888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888
rlr1rrlr1arlr1rrlr1rrlr1rrlr1rllr1lllr1allr1lllr1lllr1lllr1lrrr1rrrr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1r
rlr1rrlr1arlr1rrlr1rrlr1rrlr1rllr1lllr1allr1lllr1lllr1lllr1lrrr1rrrr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1r
rrr1rrrr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1rrrr1rrrr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1r
222222222b2222222222222222222222222b222b22222222222222222222222222222b2222222222222222222222222b222b22222222222222222222
222222222b2222222222222222222222222b222b22222222222222222222222222222b2222222222222222222222222b222b22222222222222222222
444444444c4444444444444444444444444c444c44444444444444444444444444444c4444444444444444444444444c444c44444444444444444444
888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888
rlr1rrlr1arlr1rrlr1rrlr1rrlr1rllr1lllr1allr1lllr1lllr1lllr1lrrr1rrrr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1r
rlr1rrlr1arlr1rrlr1rrlr1rrlr1rllr1lllr1allr1lllr1lllr1lllr1lrrr1rrrr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1r
rrr1rrrr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1rrrr1rrrr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1r
222222222b2222222222222222222222222b222b22222222222222222222222222222b2222222222222222222222222b222b22222222222222222222
222222222b2222222222222222222222222b222b22222222222222222222222222222b2222222222222222222222222b222b22222222222222222222
444444444c4444444444444444444444444c444c44444444444444444444444444444c4444444444444444444444444c444c44444444444444444444
888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888
rlr1ralr1arlr1rrlr1rrlr1rrlr1rllr1lllr1allr1lllr1lllr1lllr1lrrr1rarr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1r
rlr1ralr1arlr1rrlr1rrlr1rrlr1rllr1lllr1allr1lllr1lllr1lllr1lrrr1rarr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1r
rrr1rarr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1r
22222b222b2222222222222222222222222b222b2222222222222222222222222b222b2222222222222222222222222b222b22222222222222222222
22222b222b2222222222222222222222222b222b2222222222222222222222222b222b2222222222222222222222222b222b22222222222222222222
44444c444c4444444444444444444444444c444c4444444444444444444444444c444c4444444444444444444444444c444c44444444444444444444
888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888
rlr1ralr1arlr1rrlr1rrlr1rrlr1rllr1lllr1allr1lllr1lllr1lllr1lrrr1rarr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1r
rlr1ralr1arlr1rrlr1rrlr1rrlr1rllr1lllr1allr1lllr1lllr1lllr1lrrr1rarr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1r
rrr1rarr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1r
22222b222b2222222222222222222222222b222b2222222222222222222222222b222b2222222222222222222222222b222b22222222222222222222
22222b222b2222222222222222222222222b222b2222222222222222222222222b222b2222222222222222222222222b222b22222222222222222222
44444c444c4444444444444444444444444c444c4444444444444444444444444c444c4444444444444444444444444c444c44444444444444444444
888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888
llr1lllr1allr1lllr1lllr1lllr1lllr1lllr1allr1lllr1lllr1lllr1lrrr1rarr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1r
llr1lllr1allr1lllr1lllr1lllr1lllr1lllr1allr1lllr1lllr1lllr1lrrr1rarr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1r
rrr1rarr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1r
22222b222b2222222222222222222222222b222b2222222222222222222222222b222b2222222222222222222222222b222b22222222222222222222
22222b222b2222222222222222222222222b222b2222222222222222222222222b222b2222222222222222222222222b222b22222222222222222222
44444c444c4444444444444444444444444c444c4444444444444444444444444c444c4444444444444444444444444c444c44444444444444444444
888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888
llr1lllr1allr1lllr1lllr1lllr1lllr1lllr1allr1lllr1lllr1lllr1lrrr1rarr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1r
llr1lllr1allr1lllr1lllr1lllr1lllr1lllr1allr1lllr1lllr1lllr1lrrr1rarr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1r
rrr1rarr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1rrrr1rarr1arrr1rrrr1rrrr1rrrr1r
22222b222b2222222222222222222222222b222b2222222222222222222222222b222b2222222222222222222222222b222b22222222222222222222
22222b222b2222222222222222222222222b222b2222222222222222222222222b222b2222222222222222222222222b222b22222222222222222222
44444c444c4444444444444444444444444c444c4444444444444444444444444c444c4444444444444444444444444c444c44444444444444444444
888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888888
""".split()

# the same for two reordered batches (graph_ids / unit_ptr set, as ops.lane_sorted builds them): 30,000 molecules of (38, 80)
# that are simple and symmetric - they qualify for sent_lane_kernel - and the same without the flag, which nothing can launch
EXPECTED_REORDERED = """
llllllllllllllllllllllllllllll
------------------------------
""".split()
REORDERED_INNER = list(itertools.product(EPOCHS, MODES, PINS))     # 30 cells per row; the rows: with the flag, without


def make_csr(graphs, max_nodes, max_edges, symmetric=False, mirror=False, reordered=False):
    """A gtok_csr of scalars alone; the arrays it names are claims (address 1), which gtok_sent_kernel_name never follows."""
    cs = _lib.GtokCsr()
    cs.num_graphs, cs.max_nodes, cs.max_edges = graphs, max_nodes, max_edges
    cs.flags = _lib.CSR_SIMPLE_SYMMETRIC if symmetric else 0
    if mirror:
        cs.adj_rows = cs.adj_planes = 1
        cs.adj_words, cs.adj_max_degree = (1 if max_nodes <= 64 else 2 if max_nodes <= 128 else 4), 0
    if reordered:
        cs.graph_ids = cs.unit_ptr = 1
        cs.num_units, cs.chunk_nodes, cs.chunk_edges = (graphs + 63) // 64, 64 * max_nodes, 64 * max_edges
    return cs


def make_params(mode="plain", epochs=1):
    """max_num_nodes 300 covers every shape of the grid, so the ZINC remap always folds into constants."""
    lab = mode != "plain"
    return _lib.GtokSentParams(300, int(lab), 9 if lab else 0, 4 if lab else 0, 1024, int(mode == "labelled+remap"), ops.SENT_PAD,
                               0, 0, 0, 0, None, epochs, 0)


def kernel_name(cs, p):
    return gtok.lib().gtok_sent_kernel_name(ctypes.byref(cs), ctypes.byref(p)).decode()


def set_pin(monkeypatch, pin):
    if pin is None:
        monkeypatch.delenv("GTOK_SENT_KERNEL", raising=False)
    else:
        monkeypatch.setenv("GTOK_SENT_KERNEL", pin)


def grid():
    """(row, column, graphs, (max_nodes, max_edges), symmetric, epochs, mode, mirror, pin) for every cell of the table"""
    for r, (graphs, shape) in enumerate(itertools.product(GRAPHS, SHAPES)):
        for c, (sym, K, mode, mirror, pin) in enumerate(INNER):
            yield r, c, graphs, shape, sym, K, mode, mirror, pin


def test_kernel_choice_table(monkeypatch):
    assert len(EXPECTED) == len(GRAPHS) * len(SHAPES) and all(len(row) == len(INNER) for row in EXPECTED)
    wrong = []
    for r, c, graphs, shape, sym, K, mode, mirror, pin in grid():
        set_pin(monkeypatch, pin)
        got = kernel_name(make_csr(graphs, *shape, symmetric=sym, mirror=mirror), make_params(mode, K))
        if got != NAMES[EXPECTED[r][c]]:
            wrong.append((graphs, shape, sym, K, mode, mirror, pin, got, NAMES[EXPECTED[r][c]]))
    assert not wrong, f"{len(wrong)} cells differ, the first (graphs, shape, symmetric, K, mode, mirror, pin, got, expected): {wrong[:5]}"


def test_kernel_choice_reordered(monkeypatch):
    assert len(EXPECTED_REORDERED) == 2 and all(len(row) == len(REORDERED_INNER) for row in EXPECTED_REORDERED)
    for row, sym in zip(EXPECTED_REORDERED, (True, False)):
        for c, (K, mode, pin) in enumerate(REORDERED_INNER):
            set_pin(monkeypatch, pin)
            got = kernel_name(make_csr(30000, 38, 80, symmetric=sym, reordered=True), make_params(mode, K))
            assert got == NAMES[row[c]], (sym, K, mode, pin, got)
    # a qualifying one takes the molecule kernel whatever is pinned; one without the flag has no kernel
    assert set(EXPECTED_REORDERED[0]) == {"l"} and set(EXPECTED_REORDERED[1]) == {"-"}


@pytest.mark.parametrize("graphs,max_nodes,max_edges,kw,pin,name", [
    (30000, 38, 80, dict(symmetric=True), None, "sent_lane_kernel"),
    (2000, 38, 80, dict(symmetric=True), None, "sent_reg_kernel"),
    (2000, 38, 80, dict(symmetric=True, epochs=16), None, "sent_lane_kernel"),
    (125000, 256, 4000, dict(mirror=True), None, "sent_blane_kernel<W=4>"),
    (1000, 256, 4000, dict(mirror=True), None, "sent_lds_kernel<W=4>"),
    (1000, 300, 4000, dict(), None, "sent_lds_kernel<W=8>"),
    (30000, 38, 80, dict(symmetric=True), "reg", "sent_reg_kernel"),
    (1000, 200, 4000, dict(mirror=True), "blane", "sent_blane_kernel<W=4>"),
])
def test_kernel_choice_examples(monkeypatch, graphs, max_nodes, max_edges, kw, pin, name):
    set_pin(monkeypatch, pin)
    epochs = kw.pop("epochs", 1)
    assert kernel_name(make_csr(graphs, max_nodes, max_edges, **kw), make_params(epochs=epochs)) == name


def mirror_before(graphs, max_nodes, max_edges, symmetric, epochs, mode, pin):
    """The specification: whether ops.sent built a mirror before it asked the launcher - the rule it carried in Python, with its
    copies of the launcher's two thresholds, and behind it ops.adjbits' own guard (no mirror for graphs of more than 256 nodes)."""
    walks = graphs * epochs
    lane_takes = max_nodes <= 64 and max_edges <= 255 and symmetric and walks >= 28000
    wants_blane = pin == "blane" or (not pin and mode == "plain" and walks >= 20000 and not lane_takes)
    return wants_blane and max_nodes <= 256


def test_mirror_decision_equals_the_python_rule_it_replaces(monkeypatch):
    """ops._mirror_wanted is asked about batches WITHOUT a mirror (it makes the claim itself); a batch that has one already gets
    the same answer."""
    exceptions = 0
    for r, c, graphs, shape, sym, K, mode, mirror, pin in grid():
        set_pin(monkeypatch, pin)
        got = ops._mirror_wanted(make_csr(graphs, *shape, symmetric=sym, mirror=mirror), make_params(mode, K))
        want = mirror_before(graphs, *shape, sym, K, mode, pin)
        if pin == "blane" and mode != "plain" and shape[0] <= 256:
            # the one intended difference: sent_blane_kernel walks unlabelled rows only, so a pin cannot make it take a labelled
            # or remapped batch - no kernel would read the mirror the old rule built there
            assert want and not got, (graphs, shape, sym, K, mode, mirror, pin)
            exceptions += 1
        else:
            assert got == want, (graphs, shape, sym, K, mode, mirror, pin, got, want)
    assert exceptions == len(GRAPHS) * 6 * len(SYMMETRIC) * len(EPOCHS) * 2 * len(MIRROR)
    # a reordered batch (not what ops.sent is given: it reorders a copy itself): the rule it replaces, except that the one without
    # the flag - which no kernel can walk: gtok_sent refuses it - is no longer offered to gtok_csr_adjbits first, which refused it too
    for sym, (K, mode, pin) in itertools.product(SYMMETRIC, REORDERED_INNER):
        set_pin(monkeypatch, pin)
        got = ops._mirror_wanted(make_csr(30000, 38, 80, symmetric=sym, reordered=True), make_params(mode, K))
        assert got == (pin == "blane" and mode == "plain"), (sym, K, mode, pin)
        if sym or pin:
            assert got == (mirror_before(30000, 38, 80, sym, K, mode, pin) and not (pin == "blane" and mode != "plain"))
    assert not hasattr(ops, "LANE_MIN_GRAPHS") and not hasattr(ops, "ADJBITS_MIN_GRAPHS")       # the launcher alone knows its thresholds


def header_defines():
    """#define NAME <integer expression over earlier names> of include/gtok.h"""
    out = {}
    with open(os.path.join(ROOT, "include", "gtok.h")) as f:
        for m in re.finditer(r"^#define (GTOK_\w+) (\(?-?[\w +*]+\)?)\s*(?:/\*.*)?$", f.read(), flags=re.M):
            try:
                out[m.group(1)] = int(eval(m.group(2), {"__builtins__": {}}, dict(out)))
            except Exception:
                pass
    return out


def test_python_constants_equal_the_header():
    d = header_defines()
    assert d["GTOK_PACK_REGIONS"] == 64 and d["GTOK_E_UNSUPPORTED"] == -6       # (the parser reads both forms)
    assert (ops.PACK_STATE_FILL, ops.PACK_STATE_STRIDE, ops.PACK_REGIONS, ops.PACK_STATE_WORDS) == \
        (d["GTOK_PACK_STATE_FILL"], d["GTOK_PACK_STATE_STRIDE"], d["GTOK_PACK_REGIONS"], d["GTOK_PACK_STATE_WORDS"])
    assert (_lib.SENT_NO_PAD, _lib.SENT_U16, _lib.SENT_PACK_ONLY, _lib.SENT_PACK_U8) == \
        (d["GTOK_SENT_NO_PAD"], d["GTOK_SENT_U16"], d["GTOK_SENT_PACK_ONLY"], d["GTOK_SENT_PACK_U8"])
    assert _lib.E_UNSUPPORTED == d["GTOK_E_UNSUPPORTED"] and _lib.ERRORS[d["GTOK_E_UNSUPPORTED"]] == "GTOK_E_UNSUPPORTED"
    assert _lib.CSR_SIMPLE_SYMMETRIC == d["GTOK_CSR_SIMPLE_SYMMETRIC"] and _lib.ABI_VERSION == d["GTOK_ABI_VERSION"]
    assert ops.SENT_PAD == d["GTOK_SENT_PAD"] and ops.SENT_IDX_OFFSET == d["GTOK_SENT_IDX_OFFSET"]
