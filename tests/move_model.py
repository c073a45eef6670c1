"""An independent model of row movement and of the operators made of nothing else ("The row-movement contract"):
plain Python lists over value bit patterns, numpy only to read Arrow buffers.  It shares no code with sqlrs_amd beyond the dtype
constants and the expression classes, and calls neither the library nor the oracle.

Representation
  cell     None (NULL) | int (Int32 / Int64 value) | int in [0, 2^64) (the bit pattern of a Float64: -0.0 != +0.0, every NaN payload
           is itself) | bool | bytes (Utf8)
  Col      a dtype and a list of cells
  batch    a list of Col of one length

Row movement: `take` (a None index gives a NULL row), `keep`, `concat`, `slice`, `broadcast`.
Operators: `limit_stream` (limit.rs:35-79), `cross_join_stream` (cross_join.rs:30-56), `project` (bare InputRef and Constant),
`simple_agg` (tests/agg_model.py over one constant key), `text_form` (util/mod.rs:53-80).

`compare(got, expected, what)` is exact, bit for bit, and reads the Arrow buffers of `got` itself: type, length, null_count,
validity per row, the value image under every valid row, the bytes of every valid Utf8 row, and the shape of the offsets
(offsets[0] == 0 for an unsliced array, non-decreasing, NULL rows of zero length).  What lies under a NULL of a fixed-width column
is not looked at.  Nothing here needs a tolerance."""
from dataclasses import dataclass
from decimal import Decimal
from typing import List, Optional

import numpy as np
import pyarrow as pa

import agg_model
from sqlrs_amd import abi
from sqlrs_amd.expr import Constant, InputRef

I32, I64, F64, BOOL, UTF8 = abi.INT32, abi.INT64, abi.FLOAT64, abi.BOOLEAN, abi.UTF8
PA_TYPE = {I32: pa.int32(), I64: pa.int64(), F64: pa.float64(), BOOL: pa.bool_(), UTF8: pa.string()}
DTYPE_OF = {v: k for k, v in PA_TYPE.items()}
DTYPE_NAME = {I32: "i32", I64: "i64", F64: "f64", BOOL: "bool", UTF8: "utf8"}
_EXP, _FRAC = 0x7ff << 52, (1 << 52) - 1


@dataclass
class Col:
    dtype: int
    cells: list

    def __len__(self):
        return len(self.cells)

    @property
    def nulls(self) -> int:
        return sum(1 for c in self.cells if c is None)


# ---- row movement -------------------------------------------------------------------------------------------------------------------
def take(col: Col, idx) -> Col:
    return Col(col.dtype, [None if i is None else col.cells[i] for i in idx])


def keep(col: Col, mask) -> Col:
    """the rows whose mask is True; False and None drop a row"""
    assert len(mask) == len(col)
    return Col(col.dtype, [c for c, m in zip(col.cells, mask) if m is not None and bool(m)])


def concat(cols: List[Col]) -> Col:
    assert cols and all(c.dtype == cols[0].dtype for c in cols)
    return Col(cols[0].dtype, [cell for c in cols for cell in c.cells])


def slice(col: Col, lo: int, n: int) -> Col:  # noqa: A001  (the operation's name)
    assert 0 <= lo and n >= 0 and lo + n <= len(col)
    return Col(col.dtype, col.cells[lo:lo + n])


def broadcast(dtype: int, cell, n: int) -> Col:
    return Col(dtype, [cell] * n)


def rows(batch) -> int:
    return len(batch[0]) if batch else 0


def take_batch(batch, idx):
    return [take(c, idx) for c in batch]


def concat_batches(batches):
    return [concat([b[c] for b in batches]) for c in range(len(batches[0]))]


def slice_batch(batch, lo, n):
    return [slice(c, lo, n) for c in batch]


def keep_batch(batch, mask):
    return [keep(c, mask) for c in batch]


# ---- operators ----------------------------------------------------------------------------------------------------------------------
def limit_stream(batches, limit: Optional[int], offset: Optional[int]):
    """limit.rs:35-79 -> (output batches, input batches pulled before `done`).  `limit_val` is the limit, or — without a LIMIT clause
    — the cardinality of the CURRENT batch, exactly as the reference computes it (so OFFSET without LIMIT ends the stream at the
    batch that crosses offset + its own cardinality)."""
    if limit is not None and limit == 0:
        return [], 0                       # returns before the child is polled
    off = offset or 0
    returned, outs, pulled = 0, [], 0
    for b in batches:
        pulled += 1
        card = rows(b)
        limit_val = card if limit is None else limit
        start = max(returned, off) - returned
        end = min(off + limit_val, returned + card) - returned
        returned += card
        if start >= end:
            continue
        outs.append(b if (start, end) == (0, card) else slice_batch(b, start, end - start))
        if returned >= off + limit_val:
            break
    return outs, pulled


def cross_join_stream(left_batches, right_batches):
    """cross_join.rs:30-56: the left side concatenated; per right batch, per left row, that row broadcast beside the right batch.
    An empty right batch still yields one empty batch per left row; no left batch yields nothing."""
    if not left_batches:
        return []
    left = concat_batches(left_batches)
    outs = []
    for rb in right_batches:
        r = rows(rb)
        for i in range(rows(left)):
            outs.append([broadcast(c.dtype, c.cells[i], r) for c in left] + [Col(c.dtype, list(c.cells)) for c in rb])
    return outs


def constant_cell(e: Constant):
    if e.value is None:
        return None
    if e.dtype == F64:
        return int(np.array([float(e.value)], dtype=np.float64).view(np.uint64)[0])
    if e.dtype == BOOL:
        return bool(e.value)
    if e.dtype == UTF8:
        return str(e.value).encode()
    return int(e.value)


def project(batch, exprs):
    """bare InputRef and Constant only (computed columns: tests/expr_model.py)"""
    n = rows(batch)
    out = []
    for e in exprs:
        if isinstance(e, InputRef):
            out.append(Col(batch[e.index].dtype, list(batch[e.index].cells)))
        elif isinstance(e, Constant):
            out.append(broadcast(e.dtype, constant_cell(e), n))
        else:
            raise TypeError(f"move_model.project: {e!r} is a computed column")
    return out


class NoInput(Exception):
    """simple_agg over no batch at all (simple_agg.rs:63 unwraps a None)"""


def simple_agg(batches, aggs):
    """aggs [(func, column, distinct)] with func in count / sum / min / max -> a one-row batch.  The accumulators are those of
    tests/agg_model.py, run over ONE constant key; only what that model does not carry is stated here: MIN / MAX of Utf8 (byte
    order), COUNT DISTINCT (distinct value images, a NULL among them: count.rs:31-58), and the shape of the answer for zero rows (COUNT = 0, the rest NULL)."""
    if not batches:
        raise NoInput()
    whole = concat_batches(batches)
    n = rows(whole)
    out = []
    for func, ci, distinct in aggs:
        col = whole[ci]
        vals = [c for c in col.cells if c is not None]
        if distinct:
            assert func == "count"
            out.append(Col(I64, [len(set(col.cells))]))   # count.rs:31-58: a NULL is one more distinct value of the HashSet
        elif col.dtype == UTF8:
            assert func in ("min", "max", "count")
            out.append(Col(I64, [len(vals)]) if func == "count" else Col(UTF8, [(min(vals) if func == "min" else max(vals)) if vals else None]))
        else:
            npdt = {I64: np.int64, I32: np.int32, F64: np.uint64}[col.dtype]
            arr = np.array([0 if c is None else c for c in col.cells], dtype=npdt)
            if col.dtype == F64:
                arr = arr.view(np.float64)
            valid = np.array([c is not None for c in col.cells], dtype=bool)
            g = agg_model.aggregate(np.zeros(n, np.int64), None, [(arr, valid)], [(func, 0)])
            rdt = I64 if func == "count" or (func == "sum" and col.dtype != F64) else col.dtype
            if len(g) == 0:
                out.append(Col(rdt, [0 if func == "count" else None]))
                continue
            c = g.cols[0]
            assert len(g) == 1
            if c.how[0] == agg_model.FINITE:  # a Float64 sum: exact in ANY order when every value is an integer and sum |x| < 2^53
                assert c.S[0] < 2.0 ** 53 and all(float(v).is_integer() for v in arr[valid].tolist()), "sums handed to simple_agg must be exact"
            else:
                assert c.how[0] in (agg_model.EXACT, agg_model.ONE, agg_model.NULL), "sums handed to simple_agg must be exact"
            bits = int(c.bits[0])
            out.append(Col(rdt, [None if not c.valid[0] else bits if rdt == F64 else agg_model.wrap_i64(bits)]))
    return out


def f64_text(bits: int) -> str:
    """Rust's Display of an f64: the shortest digits that round-trip (Python's repr), written positionally"""
    if bits & _EXP == _EXP:
        return "NaN" if bits & _FRAC else ("-inf" if bits >> 63 else "inf")
    x = float(np.array([bits], dtype=np.uint64).view(np.float64)[0])
    s = format(Decimal(repr(x)), "f")
    if "." in s:
        s = s.rstrip("0").rstrip(".")
    return s


def text_form(batch) -> str:
    """util/mod.rs:53-80: cells joined by a space, every row ends with a newline"""
    def cell(dt, v):
        if v is None:
            return "NULL"
        if dt == UTF8:
            return v.decode() if v else "(empty)"
        if dt == BOOL:
            return "true" if v else "false"
        if dt == F64:
            return f64_text(v)
        return str(v)
    return "".join(" ".join(cell(c.dtype, c.cells[r]) for c in batch) + "\n" for r in range(rows(batch)))


# ---- pyarrow <-> model ----------------------------------------------------------------------------------------------------------
def _bitmap(buf, offset, n) -> np.ndarray:
    if n == 0:
        return np.zeros(0, dtype=bool)
    raw = np.frombuffer(buf, dtype=np.uint8, count=(offset + n + 7) // 8)
    return np.unpackbits(raw, bitorder="little")[offset:offset + n].astype(bool)


def read_column(arr: pa.Array):
    """(valid bool[n], images list, int32 offsets or None) straight from the buffers: no float conversion, no to_pylist"""
    if isinstance(arr, pa.ChunkedArray):
        arr = arr.combine_chunks()
    n, off, bufs = len(arr), arr.offset, arr.buffers()
    valid = _bitmap(bufs[0], off, n) if bufs[0] is not None else np.ones(n, dtype=bool)
    t = arr.type
    if t == pa.string():
        offs = np.frombuffer(bufs[1], dtype=np.int32, count=off + n + 1)[off:] if bufs[1] is not None else np.zeros(1, np.int32)
        data = bytes(bufs[2]) if bufs[2] is not None else b""
        return valid, [data[offs[i]:offs[i + 1]] for i in range(n)], offs
    if t == pa.bool_():
        return valid, (_bitmap(bufs[1], off, n).tolist() if n else []), None
    npdt = {pa.int32(): np.int32, pa.int64(): np.int64, pa.float64(): np.uint64}[t]
    vals = np.frombuffer(bufs[1], dtype=npdt, count=off + n)[off:] if n else np.zeros(0, npdt)
    return valid, [int(v) for v in vals.tolist()], None


def from_arrow(arr) -> Col:
    valid, images, _ = read_column(arr)
    return Col(DTYPE_OF[arr.type], [v if ok else None for v, ok in zip(images, valid.tolist())])


def batch_from_arrow(rb: pa.RecordBatch):
    return [from_arrow(rb.column(i)) for i in range(rb.num_columns)]


def to_arrow(col: Col, validity="auto") -> pa.Array:
    """validity: "auto" (a bitmap exactly when a cell is None) | "all_set" (a bitmap although no cell is None)"""
    n = len(col)
    mask = np.array([c is None for c in col.cells], dtype=bool)
    if col.dtype == F64:
        raw = np.array([0 if c is None else c for c in col.cells], dtype=np.uint64).view(np.float64)
        arr = pa.array(raw, mask=mask if mask.any() else None, from_pandas=False)
    elif col.dtype == UTF8:
        arr = pa.array([None if c is None else c.decode() for c in col.cells], type=pa.string())
    else:
        arr = pa.array(col.cells, type=PA_TYPE[col.dtype])
    if validity == "all_set" and not mask.any():
        bufs = arr.buffers()
        bufs[0] = pa.py_buffer(bytes([0xff]) * ((n + 7) // 8 + 8))
        arr = pa.Array.from_buffers(arr.type, n, bufs, null_count=0)
    return arr


def batch_to_arrow(batch, names=None, validity="auto") -> pa.RecordBatch:
    names = names or [f"c{i}" for i in range(len(batch))]
    return pa.RecordBatch.from_arrays([to_arrow(c, validity) for c in batch], names=list(names))


# ---- comparison ---------------------------------------------------------------------------------------------------------------------
def compare_column(got: pa.Array, exp: Col, what=""):
    assert got.type == PA_TYPE[exp.dtype], f"{what}: type {got.type}, expected {PA_TYPE[exp.dtype]}"
    assert len(got) == len(exp), f"{what}: {len(got)} rows, expected {len(exp)}"
    valid, images, offs = read_column(got)
    want_valid = np.array([c is not None for c in exp.cells], dtype=bool)
    bad = np.nonzero(valid != want_valid)[0]
    assert len(bad) == 0, f"{what}: row {bad[0]} of {len(exp)} is {'valid' if valid[bad[0]] else 'NULL'}, expected {exp.cells[bad[0]]!r} ({len(bad)} rows differ)"
    assert got.null_count == exp.nulls, f"{what}: null_count {got.null_count}, expected {exp.nulls} (the bits are right)"
    for i, (g, e) in enumerate(zip(images, exp.cells)):
        if e is not None and g != e:
            raise AssertionError(f"{what}: row {i} of {len(exp)} holds {g!r}, expected {e!r}")
    if offs is not None:
        if got.offset == 0:
            assert offs[0] == 0, f"{what}: offsets[0] = {offs[0]}"
        assert (np.diff(offs) >= 0).all(), f"{what}: the offsets decrease at row {int(np.nonzero(np.diff(offs) < 0)[0][0])}"
        length = np.diff(offs)
        bad = np.nonzero(~want_valid & (length != 0))[0]
        assert len(bad) == 0, f"{what}: NULL row {bad[0]} has {length[bad[0]]} bytes"


def compare(got, expected, what=""):
    """got: a pyarrow RecordBatch (or a list of arrays); expected: a model batch"""
    cols = got.columns if isinstance(got, pa.RecordBatch) else list(got)
    assert len(cols) == len(expected), f"{what}: {len(cols)} columns, expected {len(expected)}"
    for i, (g, e) in enumerate(zip(cols, expected)):
        compare_column(g, e, f"{what}: column {i} ({DTYPE_NAME[e.dtype]})")


def compare_stream(got_batches, expected_batches, what=""):
    assert len(got_batches) == len(expected_batches), f"{what}: {len(got_batches)} batches, expected {len(expected_batches)}"
    for k, (g, e) in enumerate(zip(got_batches, expected_batches)):
        compare(g, e, f"{what}: batch {k}")


def compare_limit(got_batches, got_pulled, expected, what=""):
    """expected = limit_stream(...): the output batches and how many input batches were pulled before `done`"""
    outs, pulled = expected
    assert got_pulled == pulled, f"{what}: {got_pulled} input batches pulled, expected {pulled}"
    compare_stream(got_batches, outs, what)


def compare_text(got: str, expected: str, what=""):
    g, e = got.split("\n"), expected.split("\n")
    for k, (a, b) in enumerate(zip(g, e)):
        assert a == b, f"{what}: line {k}: {a!r}, expected {b!r}"
    assert len(g) == len(e), f"{what}: {len(g) - 1} lines, expected {len(e) - 1}"

