"""A plain model of ``BoundExpr::eval_column`` for the edge-value tests: pure Python / numpy, written from the
rules and not from the formulas of the evaluators under test.

* integers are Python ``int``s, wrapped to two's complement explicitly after ``+ - *`` and ``/``;
* doubles travel as their 64-bit patterns (Python ints); an arithmetic node is ONE numpy float64 operation;
* comparisons of doubles use the IEEE total order computed from the bit pattern with Python integers;
* casts decide their range with exact integers (``math.trunc`` of a finite double against ``-(2**(w-1))`` and
  ``2**(w-1) - 1``): no floating-point limit constant anywhere in this file;
* AND / OR are Kleene over ``None``; any other binary node is NULL when an operand is NULL.

Rows carry a state next to their value:

``EXACT``    the value (or ``None`` = NULL) is what every evaluator must return, bit for bit;
``ANY_NAN``  the row is valid and holds *a* NaN whose sign and payload the hardware chooses (an arithmetic node with a
             NaN operand, or ``inf - inf``, ``0 * inf``, ``inf / inf`` ...): compared as "is NaN";
``LEFT_OUT`` a comparison or a cast (or anything above one) consumed an ``ANY_NAN`` row: not compared at all.

``left_out_fraction`` is what the tests cap at ``MAX_LEFT_OUT``.
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import pyarrow as pa

from sqlrs_amd import abi
from sqlrs_amd.expr import Alias, BinaryOp, BoundExpr, Constant, InputRef, TypeCast

EXACT, ANY_NAN, LEFT_OUT = 0, 1, 2
MAX_LEFT_OUT = 0.02

_BITS = {abi.INT32: 32, abi.INT64: 64}
_ARITH = ("+", "-", "*", "/")
_CMP = (">", "<", ">=", "<=", "=", "!=", "<>")
_SIGN = 1 << 63
_ALL = (1 << 64) - 1
_EXP = 0x7FF << 52
_FRAC = (1 << 52) - 1


class DivideByZero(Exception):
    """what every evaluator reports as the Arrow error "Divide by zero error" """


class ModelTypeError(Exception):
    pass


@dataclass
class Result:
    dtype: int
    vals: list   # per row: None (NULL) | int (integers, booleans 0 / 1, doubles as their bit pattern) | bytes (Utf8)
    state: list  # per row: EXACT | ANY_NAN | LEFT_OUT

    def __len__(self):
        return len(self.vals)

    @property
    def left_out_fraction(self) -> float:
        return sum(1 for s in self.state if s == LEFT_OUT) / max(len(self.vals), 1)


# ---- bit patterns ----------------------------------------------------------------------------------------------------------
def f64_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def bits_f64(b: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def is_nan_bits(b: int) -> bool:
    return (b & _EXP) == _EXP and (b & _FRAC) != 0


def total_order_key(b: int) -> int:
    """IEEE 754 totalOrder as an unsigned key: negative -> all bits flipped, otherwise the sign bit set"""
    return (b ^ _ALL) if (b >> 63) else (b | _SIGN)


def wrap(v: int, bits: int) -> int:
    """two's complement reduction of any integer to `bits` bits"""
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


# ---- pyarrow <-> model -----------------------------------------------------------------------------------------------------
def column_values(arr) -> list:
    """a pyarrow array as the model's values: doubles by bit pattern, strings as bytes, booleans as 0 / 1"""
    if isinstance(arr, pa.ChunkedArray):
        arr = arr.combine_chunks()
    n = len(arr)
    t = arr.type
    if t == pa.float64():
        if n == 0:
            return []
        raw = np.frombuffer(arr.buffers()[1], dtype=np.uint64, count=arr.offset + n)[arr.offset:]
        valid = np.asarray(arr.is_valid())
        return [int(b) if ok else None for b, ok in zip(raw.tolist(), valid.tolist())]
    if t == pa.string():
        return [None if v is None else v.encode() for v in arr.to_pylist()]
    if t == pa.bool_():
        return [None if v is None else int(v) for v in arr.to_pylist()]
    return arr.to_pylist()


def f64_array(bits: list) -> pa.Array:
    """pyarrow float64 array from bit patterns (None = NULL): sign of zero, NaN sign and payload survive"""
    raw = np.array([0 if b is None else b for b in bits], dtype=np.uint64)
    mask = np.array([b is None for b in bits], dtype=bool)
    return pa.array(raw.view(np.float64), mask=mask if mask.any() else None, from_pandas=False)


def to_arrow(res: Result) -> pa.Array:
    if res.dtype == abi.FLOAT64:
        return f64_array(res.vals)
    if res.dtype == abi.UTF8:
        return pa.array([None if v is None else v.decode() for v in res.vals], type=pa.string())
    if res.dtype == abi.BOOLEAN:
        return pa.array([None if v is None else bool(v) for v in res.vals], type=pa.bool_())
    return pa.array(res.vals, type=abi.pa_type(res.dtype))


# ---- the evaluator ---------------------------------------------------------------------------------------------------------
def _constant(e: Constant, rows: int) -> Result:
    if e.dtype not in (abi.INT32, abi.INT64, abi.FLOAT64, abi.BOOLEAN, abi.UTF8):
        raise ModelTypeError("constant of unsupported type")
    if e.value is None:
        v = None
    elif e.dtype == abi.FLOAT64:
        v = f64_bits(float(e.value))
    elif e.dtype == abi.UTF8:
        v = str(e.value).encode()
    elif e.dtype == abi.BOOLEAN:
        v = int(bool(e.value))
    else:
        v = int(e.value)
        if wrap(v, _BITS[e.dtype]) != v:
            raise ModelTypeError("integer constant outside its type")
    return Result(e.dtype, [v] * rows, [EXACT] * rows)


def _f64_op(op: str, a: list, b: list) -> list:
    """ONE numpy float64 operation over the rows (NULL rows computed on zeros and ignored by the caller)"""
    x = np.array([0 if v is None else v for v in a], dtype=np.uint64).view(np.float64)
    y = np.array([0 if v is None else v for v in b], dtype=np.uint64).view(np.float64)
    with np.errstate(all="ignore"):
        r = x + y if op == "+" else x - y if op == "-" else x * y if op == "*" else x / y
    return r.view(np.uint64).tolist()


def _arith(op: str, l: Result, r: Result) -> Result:
    if l.dtype != r.dtype or l.dtype not in (abi.INT32, abi.INT64, abi.FLOAT64):
        raise ModelTypeError("arithmetic over unequal or non-numeric types")
    n = len(l)
    vals, state = [None] * n, [EXACT] * n
    if l.dtype == abi.FLOAT64:
        raw = None
        for i in range(n):
            a, b, sa, sb = l.vals[i], r.vals[i], l.state[i], r.state[i]
            if (a is None and sa == EXACT) or (b is None and sb == EXACT):
                continue  # NULL, whatever the other side is
            if sa == LEFT_OUT or sb == LEFT_OUT:
                state[i] = LEFT_OUT
                continue
            if op == "/" and sb == EXACT and (b & ~_SIGN) == 0:
                raise DivideByZero()  # a valid row divides by +0.0 or -0.0
            if raw is None:
                raw = _f64_op(op, [None if s != EXACT else v for v, s in zip(l.vals, l.state)],
                              [None if s != EXACT else v for v, s in zip(r.vals, r.state)])
            if sa == ANY_NAN or sb == ANY_NAN or is_nan_bits(a) or is_nan_bits(b) or is_nan_bits(raw[i]):
                vals[i], state[i] = f64_bits(math.nan), ANY_NAN
            else:
                vals[i] = raw[i]
        return Result(l.dtype, vals, state)
    bits = _BITS[l.dtype]
    for i in range(n):
        a, b, sa, sb = l.vals[i], r.vals[i], l.state[i], r.state[i]
        if (a is None and sa == EXACT) or (b is None and sb == EXACT):
            continue
        if sa != EXACT or sb != EXACT:
            state[i] = LEFT_OUT
            continue
        if op == "+":
            v = a + b
        elif op == "-":
            v = a - b
        elif op == "*":
            v = a * b
        else:
            if b == 0:
                raise DivideByZero()
            v = abs(a) // abs(b)  # truncation toward zero
            if (a < 0) != (b < 0):
                v = -v
        vals[i] = wrap(v, bits)  # (MIN / -1 = 2**(w-1) wraps back to MIN)
    return Result(l.dtype, vals, state)


def _compare(op: str, l: Result, r: Result) -> Result:
    if l.dtype != r.dtype or l.dtype not in (abi.INT32, abi.INT64, abi.FLOAT64, abi.BOOLEAN, abi.UTF8):
        raise ModelTypeError("comparison of unequal or unsupported types")
    n = len(l)
    vals, state = [None] * n, [EXACT] * n
    for i in range(n):
        a, b, sa, sb = l.vals[i], r.vals[i], l.state[i], r.state[i]
        if (a is None and sa == EXACT) or (b is None and sb == EXACT):
            continue
        if sa != EXACT or sb != EXACT:
            state[i] = LEFT_OUT
            continue
        if l.dtype == abi.FLOAT64:
            a, b = total_order_key(a), total_order_key(b)
        # (integers exactly, booleans false < true, Utf8 bytewise: Python compares ints and bytes that way)
        v = a > b if op == ">" else a < b if op == "<" else a >= b if op == ">=" else a <= b if op == "<=" \
            else a == b if op == "=" else a != b
        vals[i] = int(v)
    return Result(abi.BOOLEAN, vals, state)


def _kleene(op: str, l: Result, r: Result) -> Result:
    if l.dtype != abi.BOOLEAN or r.dtype != abi.BOOLEAN:
        raise ModelTypeError("AND / OR over non-Boolean operands")
    n = len(l)
    vals, state = [None] * n, [EXACT] * n
    decides = 0 if op == "and" else 1  # FALSE decides an AND, TRUE an OR
    for i in range(n):
        a, b, sa, sb = l.vals[i], r.vals[i], l.state[i], r.state[i]
        if (sa == EXACT and a == decides) or (sb == EXACT and b == decides):
            vals[i] = decides
        elif sa != EXACT or sb != EXACT:
            state[i] = LEFT_OUT
        elif a is None or b is None:
            vals[i] = None
        else:
            vals[i] = 1 - decides
    return Result(abi.BOOLEAN, vals, state)


def _cast(x: Result, to: int) -> Result:
    if x.dtype == to:
        return x
    if to not in (abi.INT32, abi.INT64, abi.FLOAT64) or x.dtype not in (abi.BOOLEAN, abi.INT32, abi.INT64, abi.FLOAT64):
        raise ModelTypeError("unsupported cast")
    n = len(x)
    vals, state = [None] * n, [EXACT] * n
    for i in range(n):
        v, s = x.vals[i], x.state[i]
        if s != EXACT:
            state[i] = LEFT_OUT
            continue
        if v is None:
            continue
        if x.dtype == abi.FLOAT64:  # -> integer: truncation, out of range / NaN / inf -> NULL
            f = bits_f64(v)
            if math.isnan(f) or math.isinf(f):
                continue
            t = math.trunc(f)
            w = _BITS[to]
            if -(2 ** (w - 1)) <= t <= 2 ** (w - 1) - 1:
                vals[i] = t
        elif to == abi.FLOAT64:  # round to nearest even, as numpy's astype does
            vals[i] = int(np.array([v], dtype=np.int64).astype(np.float64).view(np.uint64)[0])
        else:  # integer / Boolean -> integer
            w = _BITS[to]
            if -(2 ** (w - 1)) <= v <= 2 ** (w - 1) - 1:
                vals[i] = v
    return Result(to, vals, state)


def evaluate(expr: BoundExpr, batch: pa.RecordBatch) -> Result:
    rows = batch.num_rows
    if isinstance(expr, Alias):
        return evaluate(expr.expr, batch)
    if isinstance(expr, InputRef):
        col = batch.column(expr.index)
        return Result(abi.dtype_of(col.type), column_values(col), [EXACT] * rows)
    if isinstance(expr, Constant):
        return _constant(expr, rows)
    if isinstance(expr, TypeCast):
        return _cast(evaluate(expr.expr, batch), expr.cast_type)
    if isinstance(expr, BinaryOp):
        l, r = evaluate(expr.left, batch), evaluate(expr.right, batch)
        op = expr.op.lower()
        if op in _ARITH:
            return _arith(op, l, r)
        if op in _CMP:
            return _compare("!=" if op == "<>" else op, l, r)
        if op in ("and", "or"):
            return _kleene(op, l, r)
    raise ModelTypeError(f"unsupported node {expr!r}")


# ---- comparing an evaluator's output with the model ------------------------------------------------------------------------
def assert_column_matches(got, res: Result, what="") -> float:
    """`got` (a pyarrow array) is the model's result bit for bit: validity, values by bit pattern (-0.0, NaN sign and
    payload count), row order; ANY_NAN rows hold some NaN; LEFT_OUT rows are not looked at.  Returns the left-out fraction
    after asserting it is within MAX_LEFT_OUT."""
    if isinstance(got, pa.ChunkedArray):
        got = got.combine_chunks()
    assert got.type == abi.pa_type(res.dtype), (what, got.type, res.dtype)
    assert len(got) == len(res), (what, len(got), len(res))
    assert res.left_out_fraction <= MAX_LEFT_OUT, (what, "rows left out", res.left_out_fraction)
    g = column_values(got)
    bad = []
    for i, (gv, mv, s) in enumerate(zip(g, res.vals, res.state)):
        if s == LEFT_OUT:
            continue
        if s == ANY_NAN:
            ok = gv is not None and is_nan_bits(gv)
        else:
            ok = gv == mv and (gv is None) == (mv is None)
        if not ok:
            bad.append((i, gv, mv, s))
    assert not bad, (what, f"{len(bad)} of {len(g)} rows differ (row, got, model, state)", bad[:8])
    return res.left_out_fraction


def assert_filter_matches(got: pa.RecordBatch, batch: pa.RecordBatch, res: Result, what="", rid=-1) -> float:
    """`got` = the rows of `batch` whose predicate `res` is TRUE, in input order, every column bit for bit.  Column `rid`
    of the batch numbers its rows 0 .. n-1; a LEFT_OUT row may be kept or dropped."""
    assert res.dtype == abi.BOOLEAN
    assert res.left_out_fraction <= MAX_LEFT_OUT, (what, "rows left out", res.left_out_fraction)
    assert got.num_columns == batch.num_columns, what
    ids = got.column(rid).to_pylist()
    assert all(a < b for a, b in zip(ids, ids[1:])), (what, "row order")
    unknown = {i for i, s in enumerate(res.state) if s == LEFT_OUT}
    sure = [i for i, (v, s) in enumerate(zip(res.vals, res.state)) if s != LEFT_OUT and v == 1]
    assert [i for i in ids if i not in unknown] == sure, (what, "kept rows", len(ids), len(sure),
                                                          sorted(set(ids) ^ set(sure) - unknown)[:8])
    src = batch.take(pa.array(ids, type=pa.int64()))
    for c in range(batch.num_columns):
        assert got.column(c).type == batch.column(c).type, (what, c)
        assert column_values(got.column(c)) == column_values(src.column(c)), (what, "column", c)
    return res.left_out_fraction


def kept_rows(res: Result) -> Optional[List[int]]:
    """rows a Filter keeps, or None when a LEFT_OUT row makes the answer open"""
    if any(s == LEFT_OUT for s in res.state):
        return None
    return [i for i, v in enumerate(res.vals) if v == 1]


# ---- edge pools: the values at which integer wrap, cast range, total order and rounding change (Parity) ---------
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
POOL_I64 = [I64_MIN, I64_MIN + 1, -(2 ** 53) - 1, -(2 ** 31) - 1, -(2 ** 31), -1, 0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 53 + 1,
            I64_MAX - 1, I64_MAX]
POOL_I32 = [I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX - 1, I32_MAX]
NAN_POS, NAN_NEG = 0x7FF8000000000000, 0xFFF8000000000000
NAN_POS_PAYLOAD, NAN_NEG_PAYLOAD = 0x7FF8000000000123, 0xFFF800000000BEEF
_two63 = f64_bits(2.0 ** 63)
POOL_F64_BITS = [f64_bits(x) for x in (
    0.0, -0.0, math.inf, -math.inf, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308,
    1.7976931348623157e308, -1.7976931348623157e308, 2.0 ** 31, -(2.0 ** 31), 2.0 ** 31 - 0.5, -(2.0 ** 31) - 0.5,
    -(2.0 ** 31) - 1, 2.0 ** 53, -(2.0 ** 53), 2.0 ** 53 + 2, -(2.0 ** 63), 2.0 ** 63)] + [
    NAN_POS, NAN_NEG, NAN_POS_PAYLOAD, NAN_NEG_PAYLOAD,
    (_two63 | _SIGN) + 1,  # the double below -2^63
    _two63 - 1]            # the double below 2^63
POOL_UTF8 = ["", "a", "ab", "abc", "b", "é", "éa", "\U0001f600", "z"]  # prefixes of each other, bytes >= 0x80
POOLS = {abi.INT64: POOL_I64, abi.INT32: POOL_I32, abi.FLOAT64: POOL_F64_BITS}
NP_TYPE = {abi.INT64: np.int64, abi.INT32: np.int32}


def pool_constant(dtype: int, v) -> Constant:
    """a pool member (doubles: a bit pattern) or None as a Constant of `dtype`"""
    if v is not None and dtype == abi.FLOAT64:
        v = bits_f64(v)
    return Constant(v, dtype)


def array_of(dtype: int, vals: list) -> pa.Array:
    """values (doubles as bit patterns, None = NULL) -> pyarrow array of `dtype`"""
    if dtype == abi.FLOAT64:
        return f64_array(vals)
    if dtype == abi.BOOLEAN:
        return pa.array([None if v is None else bool(v) for v in vals], type=pa.bool_())
    return pa.array(vals, type=abi.pa_type(dtype))


def cross_batch(dtype: int, pool: Optional[list] = None, with_null: bool = True) -> pa.RecordBatch:
    """columns (x, y, rid): the full cross product of the pool (plus NULL) with itself"""
    p = list(POOLS[dtype] if pool is None else pool) + ([None] if with_null else [])
    xs = [a for a in p for _ in p]
    ys = [b for _ in p for b in p]
    return pa.RecordBatch.from_arrays([array_of(dtype, xs), array_of(dtype, ys), pa.array(np.arange(len(xs), dtype=np.int64))],
                                      names=["x", "y", "rid"])


def ordinary(rng, dtype: int, n: int) -> list:
    if dtype == abi.INT64:
        return rng.integers(-10 ** 6, 10 ** 6, n).tolist()
    if dtype == abi.INT32:
        return rng.integers(-30000, 30000, n).tolist()
    return np.round(rng.normal(0, 300, n), 2).view(np.uint64).tolist()  # (never 0.0: see edge_column)


def edge_column(rng, dtype: int, n: int, nulls: float, pool_share: float = 0.3, pool: Optional[list] = None) -> pa.Array:
    """n rows: every pool member at least once when n allows it (at random rows), `pool_share` of the remaining rows drawn
    from the pool, ordinary values elsewhere, `nulls` of all rows NULL"""
    pool = list(POOLS[dtype] if pool is None else pool)
    vals = ordinary(rng, dtype, n)
    if dtype == abi.FLOAT64:
        vals = [v if (v & ~_SIGN) else f64_bits(1.0) for v in vals]
    take = rng.random(n) < pool_share
    picks = rng.integers(0, len(pool), n)
    for i in range(n):
        if take[i]:
            vals[i] = pool[int(picks[i])]
    once = rng.permutation(n)[:len(pool)]
    order = rng.permutation(len(pool))
    for k, i in enumerate(once.tolist()):
        vals[i] = pool[int(order[k])]
    if nulls:
        m = rng.random(n) < nulls
        vals = [None if m[i] else v for i, v in enumerate(vals)]
    return array_of(dtype, vals)


TREE_DTYPES = [abi.INT64, abi.INT64, abi.INT32, abi.INT32, abi.FLOAT64, abi.FLOAT64]  # columns of tree_batch, then rid


def tree_batch(seed: int, n: int, nulls: float = 0.1, pool_share: float = 0.0) -> pa.RecordBatch:
    """the batch the random trees run over: two columns of each numeric type + rid.  The pool members occur once each per
    column (pool_share 0): hardware NaNs stay rare enough for the left-out cap"""
    rng = np.random.default_rng(seed)
    cols = [edge_column(rng, d, n, nulls, pool_share) for d in TREE_DTYPES]
    cols.append(pa.array(np.arange(n, dtype=np.int64)))
    return pa.RecordBatch.from_arrays(cols, names=["a", "b", "c", "d", "e", "f", "rid"])


def random_tree(rng, want: int, depth: int, arith: bool = False, root: bool = False) -> BoundExpr:
    """a random expression of type `want` (a numeric dtype or BOOLEAN), at most `depth` operator levels, over the columns
    of tree_batch and constants of the pools (a tenth of them NULL).  `arith`: the parent is an arithmetic node — a double
    constant there is finite and not the largest (a NaN or inf constant would turn every row into a hardware NaN).  `root`: the
    outermost call — it returns an operator node, never a bare column or constant"""
    numeric = (abi.INT64, abi.INT32, abi.FLOAT64)
    if want != abi.BOOLEAN:
        r = rng.random()
        if depth == 0 or (r < 0.25 and not root):
            if rng.random() < 0.65:
                return InputRef(int(rng.choice([i for i, d in enumerate(TREE_DTYPES) if d == want])))
            if rng.random() < 0.1:
                return Constant(None, want)
            pool = POOLS[want]
            if arith and want == abi.FLOAT64:
                pool = [v for v in pool if (v & ~_SIGN) < f64_bits(1e308)]
            return pool_constant(want, pool[int(rng.integers(0, len(pool)))])
        if r < 0.45:
            src = [d for d in numeric + (abi.BOOLEAN,) if d != want]
            return TypeCast(random_tree(rng, src[int(rng.integers(0, len(src)))], depth - 1), want)
        op = str(rng.choice(["+", "-", "*", "/"], p=[0.3, 0.3, 0.3, 0.1]))
        right = random_tree(rng, want, depth - 1, True)
        if op == "/" and rng.random() < 0.8:  # (mostly a divisor that cannot be zero: the error case has tests of its own)
            pool = [v for v in POOLS[want] if (v if want != abi.FLOAT64 else v & ~_SIGN) != 0]
            if want == abi.FLOAT64:
                pool = [v for v in pool if (v & ~_SIGN) < f64_bits(1e308)]
            right = pool_constant(want, pool[int(rng.integers(0, len(pool)))])
        return BinaryOp(op, random_tree(rng, want, depth - 1, True), right)
    r = rng.random()
    if depth == 0 or r < 0.5:
        d = numeric[int(rng.integers(0, 3))]
        op = str(rng.choice([">", "<", ">=", "<=", "=", "!="]))
        return BinaryOp(op, random_tree(rng, d, max(depth - 1, 0)), random_tree(rng, d, max(depth - 1, 0)))
    if r < 0.6:
        op = str(rng.choice([">", "<", ">=", "<=", "=", "!="]))
        return BinaryOp(op, random_tree(rng, abi.BOOLEAN, depth - 1), random_tree(rng, abi.BOOLEAN, depth - 1))
    if r < 0.65 and not root:
        return Constant(None if rng.random() < 0.3 else bool(rng.integers(0, 2)), abi.BOOLEAN)
    return BinaryOp(str(rng.choice(["and", "or"])), random_tree(rng, abi.BOOLEAN, depth - 1), random_tree(rng, abi.BOOLEAN, depth - 1))


N_TREES, TREE_ROWS, TREE_SEED = 200, 4096, 11
_trees = {}


def trees_batch() -> pa.RecordBatch:
    """the one batch all random trees run over"""
    if "batch" not in _trees:
        _trees["batch"] = tree_batch(TREE_SEED, TREE_ROWS)
    return _trees["batch"]


def tree_case(k: int):
    """tree k of the 200: (expression, result dtype, the model's outcome over trees_batch()).  The seed of a tree is the
    first of 7000 + k, 8000 + k, ... for which the model alone leaves out at most MAX_LEFT_OUT of the rows."""
    if k not in _trees:
        want = [abi.BOOLEAN, abi.BOOLEAN, abi.INT64, abi.INT32, abi.FLOAT64][k % 5]
        for attempt in range(50):
            rng = np.random.default_rng(7000 + k + 1000 * attempt)
            e = random_tree(rng, want, int(rng.integers(1, 5)), root=True)
            out = model_outcome(e, trees_batch())
            if out is DIV0 or out.left_out_fraction <= MAX_LEFT_OUT:
                break
        else:
            raise AssertionError(f"tree {k}: no seed within the left-out cap")
        _trees[k] = (e, want, out)
    return _trees[k]


def program_shape(expr: BoundExpr):
    """(postfix nodes, deepest operand stack) of an expression: what the small-batch program compiler bounds"""
    nodes = expr.nodes()
    sp = deepest = 0
    for nd in nodes:
        if nd.op in (abi.EXPR_INPUT_REF, abi.EXPR_CONSTANT):
            sp += 1
        elif nd.op != abi.EXPR_TYPE_CAST:
            sp -= 1
        deepest = max(deepest, sp)
    return len(nodes), deepest


# ---- the case matrix shared by the CPU and the GPU tests: operator x type x pool, casts, Kleene, division by zero ----------
NUMERIC = {"i64": abi.INT64, "i32": abi.INT32, "f64": abi.FLOAT64}
ARITH_OPS, CMP_OPS = ["+", "-", "*", "/"], [">", "<", ">=", "<=", "=", "!="]
DIV0 = "Divide by zero error"


def _is_zero(dtype: int, v) -> bool:
    return v is not None and (v & ~_SIGN if dtype == abi.FLOAT64 else v) == 0


_batches = {}


def matrix_batch(dtype: int, nonzero_y: bool = False) -> pa.RecordBatch:
    """(x, y, rid): pool + NULL crossed with pool + NULL; `nonzero_y`: without the zeros in y (a divisor column)"""
    key = (dtype, nonzero_y)
    if key not in _batches:
        p = list(POOLS[dtype]) + [None]
        q = [v for v in p if not (nonzero_y and _is_zero(dtype, v))]
        xs = [a for a in p for _ in q]
        ys = [b for _ in p for b in q]
        _batches[key] = pa.RecordBatch.from_arrays(
            [array_of(dtype, xs), array_of(dtype, ys), pa.array(np.arange(len(xs), dtype=np.int64))], names=["x", "y", "rid"])
    return _batches[key]


def binary_cases(dtype: int, op: str, form: str):
    """[(label, expression, batch)]: `x op y` over the cross product (form "colcol"), or `x op k` and `k op y` for every
    pool member and NULL as the constant k (form "colconst").  A division never meets a zero divisor here."""
    div = op == "/"
    b = matrix_batch(dtype, nonzero_y=div)
    if form == "colcol":
        return [(f"x {op} y", BinaryOp(op, InputRef(0), InputRef(1)), b)]
    out = []
    for k in list(POOLS[dtype]) + [None]:
        name = "NULL" if k is None else (hex(k) if dtype == abi.FLOAT64 else str(k))
        if not (div and _is_zero(dtype, k)):
            out.append((f"x {op} {name}", BinaryOp(op, InputRef(0), pool_constant(dtype, k)), b))
        out.append((f"{name} {op} y", BinaryOp(op, pool_constant(dtype, k), InputRef(1)), b))
    return out


CAST_SOURCES = {"bool": abi.BOOLEAN, "i32": abi.INT32, "i64": abi.INT64, "f64": abi.FLOAT64}


def cast_batch(src: int) -> pa.RecordBatch:
    """(x, rid): the pool of `src` and NULL (Boolean: false, true, NULL)"""
    key = ("cast", src)
    if key not in _batches:
        p = ([0, 1] if src == abi.BOOLEAN else list(POOLS[src])) + [None]
        p = p * 3  # (more than one validity byte)
        _batches[key] = pa.RecordBatch.from_arrays([array_of(src, p), pa.array(np.arange(len(p), dtype=np.int64))], names=["x", "rid"])
    return _batches[key]


def bool_batch() -> pa.RecordBatch:
    """(p, q, rid): all nine (value, NULL) pairs, repeated past one 64-row word"""
    if "bool" not in _batches:
        t = [0, 1, None]
        ps = [a for a in t for _ in t] * 8
        qs = [b for _ in t for b in t] * 8
        _batches["bool"] = pa.RecordBatch.from_arrays(
            [array_of(abi.BOOLEAN, ps), array_of(abi.BOOLEAN, qs), pa.array(np.arange(len(ps), dtype=np.int64))], names=["p", "q", "rid"])
    return _batches["bool"]


def utf8_batch() -> pa.RecordBatch:
    if "utf8" not in _batches:
        p = POOL_UTF8 + [None]
        xs = [a for a in p for _ in p]
        ys = [b for _ in p for b in p]
        _batches["utf8"] = pa.RecordBatch.from_arrays(
            [pa.array(xs, type=pa.string()), pa.array(ys, type=pa.string()), pa.array(np.arange(len(xs), dtype=np.int64))],
            names=["x", "y", "rid"])
    return _batches["utf8"]


def model_outcome(expr: BoundExpr, batch: pa.RecordBatch):
    """the model's Result, or DIV0 when a valid row divides by zero"""
    try:
        return evaluate(expr, batch)
    except DivideByZero:
        return DIV0


def backend_column(be, expr: BoundExpr, batch):
    """eval_column through a backend: the result column, or DIV0 for the evaluators' Arrow error"""
    from sqlrs_amd.executor import eval_column
    try:
        return eval_column(be, expr, batch).column(0)
    except abi.ExecutorError as err:
        assert err.status == abi.ERR_ARROW and DIV0 in err.message, err
        return DIV0


def backend_filter(be, expr: BoundExpr, batch, **kw):
    """FilterExecutor over one batch: the kept rows, or DIV0"""
    from sqlrs_amd.executor import FilterExecutor
    try:
        (out,) = list(FilterExecutor(be, expr, [batch], **kw).execute())
        return out
    except abi.ExecutorError as err:
        assert err.status == abi.ERR_ARROW and DIV0 in err.message, err
        return DIV0


def check_eval(be, expr: BoundExpr, batch: pa.RecordBatch, what="", exp=None) -> float:
    """eval_column of `be` against the model (and, for a Boolean result, FilterExecutor too); returns the left-out fraction"""
    exp = model_outcome(expr, batch) if exp is None else exp
    got = backend_column(be, expr, batch)
    if exp is DIV0 or got is DIV0:
        assert exp is DIV0 and got is DIV0, (what, "divide by zero: model", exp is DIV0, "evaluator", got is DIV0)
        return 0.0
    frac = assert_column_matches(got, exp, what)
    if exp.dtype == abi.BOOLEAN:
        assert_filter_matches(backend_filter(be, expr, batch), batch, exp, what + " (filter)")
    return frac


def div0_cases():
    """[(label, expression, batch, raises)]: a valid row with a zero divisor raises; a NULL row with a zero divisor, a NULL
    dividend over zero and a NULL constant divisor do not"""
    out = []
    for kind, dt in NUMERIC.items():
        zeros = [f64_bits(0.0), f64_bits(-0.0)] if dt == abi.FLOAT64 else [0]
        one = f64_bits(1.5) if dt == abi.FLOAT64 else 7
        for z in zeros:
            # one valid zero anywhere in the batch: the first row, the first and the last row of another wave, the last row
            # of a full workgroup and of a full small batch (whichever wave sees it, the error must reach the caller)
            for n, row in ((70, 0), (70, 64), (70, 69), (1024, 1023), (4096, 4095)):
                y = array_of(dt, [one] * row + [z] + [one] * (n - row - 1))
                b = pa.RecordBatch.from_arrays([array_of(dt, [one] * n), y], names=["x", "y"])
                out.append((f"{kind}: zero divisor in valid row {row} of {n}", InputRef(0) / InputRef(1), b, True))
            n = 70
            x = array_of(dt, [one] * n)
            ynull = pa.RecordBatch.from_arrays([x, array_of(dt, [one, None] * (n // 2))], names=["x", "y"])
            # (the value under a NULL is whatever the producer left there: pyarrow leaves zero)
            out.append((f"{kind}: NULL divisor rows", InputRef(0) / InputRef(1), ynull, False))
            xnull = pa.RecordBatch.from_arrays([array_of(dt, [None] * n), array_of(dt, [z] * n)], names=["x", "y"])
            out.append((f"{kind}: NULL dividend over zero", InputRef(0) / InputRef(1), xnull, False))
            out.append((f"{kind}: NULL dividend over a zero constant", InputRef(0) / pool_constant(dt, z), xnull, False))
            full = pa.RecordBatch.from_arrays([x, x], names=["x", "y"])
            out.append((f"{kind}: zero constant divisor", InputRef(0) / pool_constant(dt, z), full, True))
            out.append((f"{kind}: NULL constant divisor", InputRef(0) / Constant(None, dt), full, False))
            out.append((f"{kind}: NULL constant dividend over zero", Constant(None, dt) / pool_constant(dt, z), full, False))
    return out
