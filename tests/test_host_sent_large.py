"""gtok_sent_large, the parts that need no GPU: the workspace arithmetic (pure host code of the C ABI), the binding of the two
entry points by symbol, and the Python constants against include/gtok.h."""
import ctypes
import os
import re

from _util import ROOT, gtok

_lib = gtok._lib
MAXN, WAVES = _lib.SENT_LARGE_MAX_NODES, _lib.SENT_LARGE_WAVES


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


def _ws(n, e, walks):
    return int(_lib.lib().gtok_sent_large_workspace(n, e, walks))


def test_the_entry_points_are_bound_by_symbol_and_the_abi_version_stays():
    L = _lib.lib()
    assert hasattr(L, "gtok_sent_large") and hasattr(L, "gtok_sent_large_workspace")
    assert L.gtok_sent_large_workspace.restype is ctypes.c_int64 and len(L.gtok_sent_large.argtypes) == 8
    assert _lib.ABI_VERSION == 8 and L.gtok_version() == 8
    assert set(_lib.OPTIONAL_SYMBOLS) == {"gtok_sent_large", "gtok_sent_large_workspace"} <= set(_lib.SYMBOLS)   # (a build without them still loads)


def test_python_constants_equal_the_header():
    d = header_defines()
    assert (MAXN, WAVES) == (d["GTOK_SENT_LARGE_MAX_NODES"], d["GTOK_SENT_LARGE_WAVES"])
    assert MAXN == 16384 and gtok.ops.SENT_MAX_NODES == d["GTOK_MAX_NODES"] == 512 and _lib.ABI_VERSION == d["GTOK_ABI_VERSION"] == 8
    assert WAVES >= 1


def test_workspace_is_a_multiple_of_16_and_monotonic():
    shapes = [(0, 0), (1, 0), (1, 1), (3, 7), (513, 1026), (514, 1027), (5000, 14000), (MAXN, 1), (MAXN, 2 ** 31 - 1)]
    for n, e in shapes:
        for walks in (0, 1, 2, WAVES - 1, WAVES):
            b = _ws(n, e, walks)
            assert b >= 0 and b % 16 == 0, (n, e, walks, b)
            assert (b == 0) == (walks == 0)
            assert _ws(n + 1 if n < MAXN else n, e, walks) >= b and _ws(n, min(e + 1, 2 ** 31 - 1), walks) >= b and _ws(n, e, walks + 1) >= b
    # strictly more room for a strictly larger graph, once the 16-byte rounding is out of the way
    assert _ws(1024, 4096, 8) > _ws(512, 4096, 8) and _ws(1024, 8192, 8) > _ws(1024, 4096, 8) and _ws(1024, 4096, 9) > _ws(1024, 4096, 8)
    # a slice per wave: linear in the walks up to the wave count ...
    assert _ws(700, 3000, 10) == 10 * _ws(700, 3000, 1)


def test_workspace_is_flat_beyond_the_wave_count():
    for n, e in [(1, 1), (600, 2400), (MAXN, 50000)]:
        top = _ws(n, e, WAVES)
        assert top > _ws(n, e, WAVES - 1)
        for walks in (WAVES + 1, 10 * WAVES, 2 ** 40):
            assert _ws(n, e, walks) == top


def test_workspace_error_codes():
    assert _ws(-1, 0, 1) == -1 and _ws(0, -1, 1) == -1 and _ws(0, 0, -1) == -1                  # GTOK_E_INVAL
    assert _ws(MAXN + 1, 0, 1) == -2 and _ws(2 ** 31 - 1, 0, 0) == -2                             # GTOK_E_TOO_LARGE
    assert _ws(MAXN, 0, 1) > 0
