"""The constants mirror of the labelled + remapped lane-per-graph walk (include/gtok.h: gtok_sent_lane_consts), restated with
numpy: ntok8 / etok8 - the token the walk emits for every node / entry type byte - and the fits-a-byte verdict.  The token
formula is held against the oracle's remap of un-remapped type tokens (oracle.remap_zinc, pinned to the reference's own
output by tests/test_oracle_golden.py) for every attribute value and three tokenizer settings; tests/test_gpu_lane_consts.py
holds the device builder against this restatement."""
import numpy as np
import pytest

from _util import gtok, orc

IDX = 6      # include/gtok.h: GTOK_SENT_IDX_OFFSET
SETTINGS = [(37, 9, 4), (64, 28, 5), (200, 9, 4)]      # (max_num_nodes, num_node_types, num_edge_types)


def tok8_reference(nattr, eattr, max_num_nodes, num_node_types, num_edge_types):
    """(node tokens, entry tokens, status) as int64 arrays / int: the tokens BEFORE they are narrowed to a byte (the mirror holds
    their low bytes) and bit 0 of the status word - some token does not fit a byte."""
    node_off = IDX + max_num_nodes
    edge_off = node_off + num_node_types
    x, a = np.asarray(nattr, np.int64), np.asarray(eattr, np.int64)
    b = x - num_node_types
    ntok = 22 + node_off + x                                      # everything else: 22 + the un-remapped token
    ntok = np.where((b >= 0) & (b < 4), 17 + b, ntok)             # the four ids behind the node types read as bonds
    ntok = np.where(x < min(num_node_types, 9), 8 + x, ntok)      # atoms
    etok = np.where(a < 4, 17 + a, 22 + edge_off + a)
    wide = bool((ntok > 255).any() or (etok > 255).any())
    return ntok, etok, int(wide)


@pytest.mark.parametrize("mnn,nnt,net", SETTINGS)
def test_token_formula_equals_the_oracle_remap_for_every_attribute_byte(mnn, nnt, net):
    node_off, edge_off = IDX + mnn, IDX + mnn + nnt
    v = np.arange(256, dtype=np.int64)
    ntok, etok, _ = tok8_reference(v, v, mnn, nnt, net)
    ln = np.array([256], np.int32)
    ref_n = orc.remap_zinc((node_off + v).astype(np.int32)[None, :], ln, IDX, node_off, edge_off)[0]
    ref_e = orc.remap_zinc((edge_off + v).astype(np.int32)[None, :], ln, IDX, node_off, edge_off)[0]
    assert np.array_equal(ntok, ref_n), np.nonzero(ntok != ref_n)[0][:8]
    assert np.array_equal(etok, ref_e), np.nonzero(etok != ref_e)[0][:8]


def test_all_three_ranges_of_both_formulas_are_taken():
    v = np.arange(256)
    ntok, etok, _ = tok8_reference(v, v, 37, 9, 4)
    assert ntok[:9].tolist() == list(range(8, 17)) and ntok[9:13].tolist() == [17, 18, 19, 20] and ntok[13] == 22 + 43 + 13
    assert etok[:4].tolist() == [17, 18, 19, 20] and etok[4] == 22 + 52 + 4
    ntok28, _, _ = tok8_reference(v, v, 64, 28, 5)
    assert ntok28[8] == 16 and ntok28[9] == 22 + 70 + 9 and ntok28[28:32].tolist() == [17, 18, 19, 20]      # atoms stop at 9 types


def test_fits_a_byte_verdict_at_the_edge():
    # (37, 9, 4): a node type x >= 13 becomes 65 + x, an entry type a >= 4 becomes 74 + a
    for x, want in ((190, 0), (191, 1)):
        ntok, _, st = tok8_reference([0, 5, x], [0, 1], 37, 9, 4)
        assert int(ntok.max()) == 65 + x == 255 + want and st == want
    for a, want in ((181, 0), (182, 1)):
        _, etok, st = tok8_reference([0], [1, a], 37, 9, 4)
        assert int(etok.max()) == 74 + a == 255 + want and st == want
    # the attribute byte 255 never fits; neither does any fall-through token under max_num_nodes = 200 with node types beyond 12
    assert tok8_reference([255], [0], 37, 9, 4)[2] == 1 and tok8_reference([0], [255], 37, 9, 4)[2] == 1
    assert tok8_reference([13], [0], 200, 9, 4)[2] == 0 and tok8_reference([28], [0], 200, 9, 4)[2] == 1      # 228 + 13 = 241, 228 + 28 = 256
    assert tok8_reference([0, 8, 12], [0, 3], 200, 9, 4)[2] == 0 and tok8_reference([0], [4], 200, 9, 4)[2] == 0   # 22 + 215 + 4 = 241


def test_binding_declares_the_two_entry_points_as_optional():
    _lib = gtok._lib
    names = ("gtok_sent_lane_consts", "gtok_sent_prepared")
    assert _lib.LANE_CONSTS_SYMBOLS == names and set(names) <= set(_lib.SYMBOLS) and set(names) <= _lib._MAY_BE_MISSING
    L = gtok.lib()
    assert all(hasattr(L, n) for n in names) and _lib.ABI_VERSION == 8 and L.gtok_version() == 8
    import ctypes
    assert ctypes.sizeof(_lib.GtokSentConsts) == 32
