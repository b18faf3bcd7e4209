"""The helper modules of tests/: the structure that keeps them the only shared code -- no test module imports another, no helper
module loads torch or lyra_amd on import, no function or class exists twice -- and the span checkers on buffers with a known
fault: each fault must raise, the clean buffer must pass."""
import ast
import glob
import os

import numpy as np
import pytest

from span_cases import FILL16, _check_ext, _check_packets, _check_rows, _check_state

HERE = os.path.dirname(os.path.abspath(__file__))
FILL = 85
SPANS = [(5, 1, 3), (9, 6, 2)]            # (stream id, first row, rows) in a buffer of 12 rows


def _trees():
    return {os.path.basename(p): ast.parse(open(p).read(), p) for p in sorted(glob.glob(os.path.join(HERE, "*.py")))}


def _imported(node):
    return [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""]


def test_no_test_module_imports_another():
    bad = [(name, n.lineno, m) for name, tree in _trees().items() if name.startswith("test_") for n in ast.walk(tree)
           if isinstance(n, (ast.Import, ast.ImportFrom)) for m in _imported(n) if m.split(".")[0].startswith("test_")]
    assert not bad, f"test modules imported by test modules (file, line, module): {bad}"


def _module_level(node):
    """the statements that run on import: everything but the bodies of functions"""
    for child in ast.iter_child_nodes(node):
        if not isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)):
            yield child
            yield from _module_level(child)


def test_helper_modules_load_neither_torch_nor_the_package():
    bad = [(name, n.lineno, m) for name, tree in _trees().items() if not name.startswith("test_") and name != "conftest.py"
           for n in _module_level(tree) if isinstance(n, (ast.Import, ast.ImportFrom)) for m in _imported(n)
           if m.split(".")[0] in ("torch", "lyra_amd")]
    assert not bad, f"helper modules importing torch or lyra_amd at module level (file, line, module): {bad}"


def test_no_function_or_class_exists_twice():
    """Helpers, fixtures and classes of more than two lines (the `def` line and one more).  Test functions are left out: a test
    is its module's own, and three ABI modules hold the same three lines over their own table of names."""
    seen, twice = {}, []
    for name, tree in _trees().items():
        for n in tree.body:
            if (isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)) and not n.name.startswith("test_")
                    and n.end_lineno - n.lineno + 1 > 2):
                first = seen.setdefault(ast.dump(n), (name, n.name))
                if first[0] != name:
                    twice.append((n.name, first[0], name))
    assert not twice, f"the same definition in two files (name, file, file): {twice}"


# ---- the span checkers ----------------------------------------------------------------------------------------------------
def _buffer():
    """12 rows of 8 bytes, the spans' rows numbered, every other row the filler; and the rows by stream id"""
    want = {5: np.arange(24, dtype=np.uint8).reshape(3, 8), 9: np.arange(100, 116, dtype=np.uint8).reshape(2, 8)}
    buf = np.full((12, 8), FILL, np.uint8)
    for (i, first, n) in SPANS:
        buf[first:first + n] = want[i]
    return buf, want


def _faulty(buf, row, col, value):
    out = buf.copy()
    out[row, col] = value
    return out


def test_check_rows_sees_each_fault():
    buf, want = _buffer()
    _check_rows("clean", buf, SPANS, want)
    with pytest.raises(AssertionError, match="stream 9 differs at written hops \\[1\\]"):
        _check_rows("a wrong byte in a span", _faulty(buf, 7, 3, 0), SPANS, want)
    with pytest.raises(AssertionError, match="rows outside every span were written"):
        _check_rows("a written row between the spans", _faulty(buf, 4, 0, 1), SPANS, want)
    # written=: stream 5 wrote its rows 0 and 2 only, row 1 still holds the filler
    written = {5: np.array([True, False, True]), 9: np.ones(2, bool)}
    part = buf.copy()
    part[2] = FILL
    _check_rows("clean, written=", part, SPANS, want, written=written)
    with pytest.raises(AssertionError, match="stream 5: rows of noise hops do not hold 85"):
        _check_rows("a row that should still hold the filler", buf, SPANS, want, written=written)
    with pytest.raises(AssertionError, match="stream 5 differs at written hops \\[2\\]"):
        _check_rows("a wrong byte in a written row", _faulty(part, 3, 7, 0), SPANS, want, written=written)


def test_check_packets_sees_each_fault():
    sizes = {5: np.array([8, 0, 3], np.int32), 9: np.array([5, 8], np.int32)}
    buf, want = _buffer()
    for (i, first, n) in SPANS:                       # the twin's rows: the filler behind every packet
        for h in range(n):
            want[i][h, sizes[i][h]:] = FILL
        buf[first:first + n] = want[i]
    nb = np.full(12, FILL * 0x01010101, np.int32)
    for (i, first, n) in SPANS:
        nb[first:first + n] = sizes[i]
    _check_packets("clean", buf, nb, SPANS, want, sizes)
    with pytest.raises(AssertionError, match="packet rows: stream 5 differs"):
        _check_packets("a wrong byte in a packet", _faulty(buf, 1, 2, 99), nb, SPANS, want, sizes)
    with pytest.raises(AssertionError, match="packet rows: stream 5 differs"):
        _check_packets("a byte behind a packet", _faulty(buf, 3, 4, 0), nb, SPANS, want, sizes)
    with pytest.raises(AssertionError, match="packet rows: rows outside every span were written"):
        _check_packets("a written row between the spans", _faulty(buf, 4, 0, 1), nb, SPANS, want, sizes)
    wrong = nb.copy()
    wrong[6] = 8
    with pytest.raises(AssertionError, match="packet_bytes: stream 9 differs"):
        _check_packets("a wrong size", buf, wrong, SPANS, want, sizes)


def test_check_ext_sees_each_fault():
    rate_of = {5: 150, 9: 100}                        # rows of 3 and of 2 samples in a buffer 4 samples (8 bytes) wide
    want = {5: np.arange(9, dtype=np.int16).reshape(3, 3), 9: np.arange(50, 54, dtype=np.int16).reshape(2, 2)}
    buf = np.full((12, 4), FILL16, np.int16)
    for (i, first, n) in SPANS:
        buf[first:first + n, :rate_of[i] // 50] = want[i]
    assert buf.nbytes == 12 * 8
    _check_ext("clean", buf, SPANS, want, rate_of)
    with pytest.raises(AssertionError, match="stream 5 \\(150 Hz\\) differs at hops \\[2\\]"):
        _check_ext("a wrong sample in a span", _faulty(buf, 3, 1, -1), SPANS, want, rate_of)
    with pytest.raises(AssertionError, match="samples behind a row's rate / 50"):
        _check_ext("a sample behind a row", _faulty(buf, 6, 2, 0), SPANS, want, rate_of)
    with pytest.raises(AssertionError, match="rows outside every span, were written"):
        _check_ext("a written row between the spans", _faulty(buf, 4, 0, 0), SPANS, want, rate_of)


class _Blobs:
    """stands in for a context: export_streams gives row `id` of a table"""

    def __init__(self, table):
        self.table = table

    def export_streams(self, ids):
        return self.table[np.asarray(ids, np.int64)] if len(ids) else np.zeros((0, self.table.shape[1]), np.uint8)


def test_check_state_sees_each_fault():
    table = np.random.default_rng(1).integers(0, 256, size=(16, 32), dtype=np.uint8)
    twin, lanes = _Blobs(table), np.array([10, 11, 12], np.int32)
    _check_state("clean", _Blobs(table.copy()), twin, [5, 9], lanes)
    with pytest.raises(AssertionError, match="span streams \\[9\\] differ"):
        _check_state("a differing span stream", _Blobs(_faulty(table, 9, 31, table[9, 31] ^ 1)), twin, [5, 9], lanes)
    dirty = _Blobs(_faulty(table, 11, 0, table[11, 0] ^ 1))
    with pytest.raises(AssertionError, match="lanes \\[11\\] differ"):
        _check_state("a dirtied lane", dirty, twin, [5, 9], lanes)
    _check_state("a dirtied lane that is not in the (empty) lane list", dirty, twin, [5, 9], [])
    with pytest.raises(AssertionError, match="span streams \\[5\\] differ"):
        _check_state("an empty lane list still checks the span streams", _Blobs(_faulty(table, 5, 0, table[5, 0] ^ 1)), twin, [5, 9], [])
