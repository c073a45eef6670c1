"""An independent model of ORDER BY: plain Python / numpy / pyarrow containers, no call into the library or the oracle.  What it
pins (order.rs:27-66: concat -> lexsort, nulls first, stable -> take):

* NULL keys come first WHATEVER the direction of the key; two NULLs tie;
* valid keys follow in the key's total order, or in its reverse for DESC: integers by value, Booleans false < true, Utf8 keys
  as `bytes` (unsigned bytes, a string before every extension of it — "a" < "a\\x00"), doubles in the IEEE total order
  (-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN, NaNs among themselves by payload);
* several keys: the first decides, the next breaks its ties;
* rows that tie on every key keep their input order (across the input batches).

The model returns a PERMUTATION; the expected columns are the inputs taken by it, so a payload travels untouched — a NaN keeps
its sign and payload, a NULL stays a NULL.  Two forms:

  perm_fast   numpy.lexsort over explicit (validity, key image) columns — any size
  perm_slow   the definition restated row by row: functools.cmp_to_key over (is_valid, value) with a comparator that uses no
              image — small n; tests/test_order_model_cpu.py holds the two against each other

`compare` is exact: validity bit for bit, fixed-width values as unsigned integers of their width wherever valid (a double as
its uint64), Utf8 as bytes; what sits under a NULL is not looked at.  There is no tolerance in a sort."""
import functools
from typing import List

import numpy as np
import pyarrow as pa

import expr_model as X
from sqlrs_amd.expr import InputRef

_SIGN = np.uint64(1 << 63)
_ALL = np.uint64((1 << 64) - 1)
_M63 = (1 << 63) - 1


# ---- key columns -----------------------------------------------------------------------------------------------------------------
def as_table(batches) -> pa.Table:
    if isinstance(batches, pa.Table):
        return batches.combine_chunks()
    return pa.Table.from_batches(list(batches)).combine_chunks()


def _one(col):
    if isinstance(col, pa.ChunkedArray):
        return col.combine_chunks() if col.num_chunks != 1 else col.chunk(0)
    return col


def _raw(arr, dtype):
    n = len(arr)
    if n == 0:
        return np.zeros(0, dtype)
    return np.frombuffer(arr.buffers()[1], dtype=dtype, count=arr.offset + n)[arr.offset:]


def _valid(arr):
    n = len(arr)
    return np.asarray(arr.is_valid()).astype(bool) if n else np.zeros(0, bool)


def key_kind(t) -> str:
    return {pa.int64(): "i64", pa.int32(): "i32", pa.float64(): "f64", pa.bool_(): "bool", pa.string(): "utf8"}[t]


def key_arrays(table: pa.Table, order_by) -> List[pa.Array]:
    """the key columns as pyarrow arrays: an InputRef is the column itself, anything else is evaluated by tests/expr_model.py
    (row by row in Python: small inputs only)"""
    out = []
    for ob in order_by:
        if isinstance(ob.expr, InputRef):
            out.append(_one(table.column(ob.expr.index)))
        else:
            (batch,) = table.to_batches() if table.num_rows else [pa.RecordBatch.from_pylist([], schema=table.schema)]
            res = X.evaluate(ob.expr, batch)
            assert all(s == X.EXACT for s in res.state), "an ORDER BY key must be exact in the expression model"
            out.append(X.to_arrow(res))
    return out


# ---- fast form: images -----------------------------------------------------------------------------------------------------------
def image(arr) -> np.ndarray:
    """order-preserving uint64 image of the VALID values of a key column (whatever under a NULL)"""
    kind = key_kind(arr.type)
    if kind == "i64":
        return _raw(arr, np.uint64) ^ _SIGN
    if kind == "i32":
        return _raw(arr, np.int32).astype(np.int64).view(np.uint64) ^ _SIGN
    if kind == "f64":
        b = _raw(arr, np.uint64)
        return np.where(b >> np.uint64(63) != 0, b ^ _ALL, b | _SIGN)
    if kind == "bool":
        return np.asarray(arr.fill_null(False)).astype(np.uint64)
    vals = [b"" if v is None else v for v in arr.cast(pa.binary()).to_pylist()]
    rank = {v: r for r, v in enumerate(sorted(set(vals)))}  # (Python orders bytes as unsigned bytes, a prefix first)
    return np.array([rank[v] for v in vals], dtype=np.uint64)


def perm_fast(batches, order_by) -> np.ndarray:
    table = as_table(batches)
    n = table.num_rows
    cols = []  # numpy.lexsort: the LAST column is the most significant
    for ob, arr in reversed(list(zip(order_by, key_arrays(table, order_by)))):
        valid = _valid(arr)
        img = image(arr)
        if not ob.asc:
            img = img ^ _ALL
        cols.append(np.where(valid, img, np.uint64(0)))  # NULLs tie
        cols.append(valid.astype(np.uint8))              # ... and come first
    if not cols or n == 0:
        return np.arange(n, dtype=np.int64)
    return np.lexsort(tuple(cols)).astype(np.int64)      # (stable: ties in input order)


# ---- row-by-row restatement ------------------------------------------------------------------------------------------------------
def _cmp_f64_bits(a: int, b: int) -> int:
    """IEEE totalOrder on bit patterns, as sign-magnitude integers: a negative sorts before a positive (-0.0 before +0.0), two
    positives by magnitude, two negatives by magnitude reversed"""
    sa, sb = a >> 63, b >> 63
    if sa != sb:
        return -1 if sa else 1
    ma, mb = a & _M63, b & _M63
    if ma == mb:
        return 0
    return (1 if ma < mb else -1) if sa else (-1 if ma < mb else 1)


def _cmp_plain(a, b) -> int:
    return -1 if a < b else (1 if a > b else 0)  # Python ints (integers, Booleans 0 / 1) and bytes


def perm_slow(batches, order_by) -> list:
    table = as_table(batches)
    keys = []
    for ob, arr in zip(order_by, key_arrays(table, order_by)):
        keys.append((X.column_values(arr), _cmp_f64_bits if arr.type == pa.float64() else _cmp_plain, ob.asc))

    def cmp(i, j):
        for vals, c, asc in keys:
            a, b = vals[i], vals[j]
            if a is None or b is None:
                if a is None and b is None:
                    continue
                return -1 if a is None else 1   # NULLs first, whatever the direction
            r = c(a, b)
            if r:
                return r if asc else -r
        return i - j

    return sorted(range(table.num_rows), key=functools.cmp_to_key(cmp))


# ---- expected output -------------------------------------------------------------------------------------------------------------
def take(table: pa.Table, perm) -> pa.Table:
    return table.take(pa.array(np.asarray(perm, dtype=np.int64))).combine_chunks()


def expected(batches, order_by, limit=None, offset=0, perm=None) -> pa.Table:
    """ORDER BY [LIMIT limit OFFSET offset] of the batches"""
    table = as_table(batches)
    p = perm_fast(table, order_by) if perm is None else np.asarray(perm, dtype=np.int64)
    if limit is not None:
        p = p[offset:offset + limit]
    return take(table, p)


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def compare(got, exp: pa.Table, label=""):
    """`got`: a RecordBatch / Table / list of batches an operator emitted; `exp`: the model's table"""
    if isinstance(got, pa.RecordBatch):
        got = pa.Table.from_batches([got])
    elif not isinstance(got, pa.Table):
        got = [g for g in got if g is not None]
        assert got or exp.num_rows == 0, f"{label}: no batch where {exp.num_rows} rows were expected"
        got = pa.Table.from_batches(got) if got else exp.slice(0, 0)
    assert got.num_columns == exp.num_columns, f"{label}: {got.num_columns} columns, expected {exp.num_columns}"
    assert got.num_rows == exp.num_rows, f"{label}: {got.num_rows} rows, expected {exp.num_rows}"
    for c in range(exp.num_columns):
        g, e = _one(got.column(c)), _one(exp.column(c))
        assert g.type == e.type, f"{label}: column {c} is {g.type}, expected {e.type}"
        gv, ev = _valid(g), _valid(e)
        bad = np.nonzero(gv != ev)[0]
        assert len(bad) == 0, f"{label}: column {c}: validity differs at rows {bad[:8].tolist()} ({len(bad)} rows)"
        if e.type == pa.string():
            gb, eb = g.cast(pa.binary()).fill_null(b""), e.cast(pa.binary()).fill_null(b"")
            if gb.equals(eb):
                continue
            gx, ex = gb.to_pylist(), eb.to_pylist()
            bad = [i for i in range(len(ex)) if gx[i] != ex[i]]
            assert not bad, f"{label}: column {c}: {len(bad)} strings differ, first rows {bad[:8]}: got {[gx[i] for i in bad[:4]]}, expected {[ex[i] for i in bad[:4]]}"
            continue
        if e.type == pa.bool_():
            gx, ex = np.asarray(g.fill_null(False)).astype(np.uint8), np.asarray(e.fill_null(False)).astype(np.uint8)
        else:
            width = np.uint32 if e.type in (pa.int32(), pa.uint32()) else np.uint64
            gx, ex = _raw(g, width), _raw(e, width)
        bad = np.nonzero(ev & (gx != ex))[0]
        assert len(bad) == 0, (f"{label}: column {c}: {len(bad)} values differ, first rows {bad[:8].tolist()}: got "
                               f"{[hex(int(gx[i])) for i in bad[:4]]}, expected {[hex(int(ex[i])) for i in bad[:4]]}")

