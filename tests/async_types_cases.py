"""sqlrs_filter_set_async_all_types / sqlrs_project_set_async_all_types: the cases of tests/test_async_all_types_cpu.py and
tests/test_gpu_async_all_types.py, and the eligibility rule of include/sqlrs_hip.h restated from the batch, the expression's
nodes and the header's constants (no library call: numpy and pyarrow only).

The rule, switch on: a HOST batch takes the one-launch kernel when it has at most 4096 rows and 12 columns, the expression at
most 24 nodes and 8 operands in flight, both operands of every comparison the same type (Utf8 only there, Boolean also under
AND / OR and as the source of a cast), its Utf8 constants at most 1024 bytes, and the staged bytes fit 512 KiB.  Every case
here is far from the byte limit except the batch that crosses it on purpose, so `fits` compares the raw buffer bytes with the
limit and refuses to answer in between."""
import numpy as np
import pyarrow as pa

import expr_model as M
from async_utf8_cases import str_array
from sqlrs_amd import abi
from sqlrs_amd.expr import BinaryOp, Constant, InputRef, TypeCast

SA_MAX_ROWS, SA_MAX_COLS, SA_PROG_MAX, SA_STACK_MAX, SA_POOL_MAX, SA_AREA, SP_PROGS = 4096, 12, 24, 8, 1024, 512 * 1024, 6
NUMERIC = (abi.INT32, abi.INT64, abi.FLOAT64)
CMP_OPS = (">", "<", ">=", "<=", "=", "!=")


# ---- the rule ---------------------------------------------------------------------------------------------------------
def compiles(expr, dtypes, wide=True):
    """(result dtype, bytes of Utf8 constants, reads something only the all-types program knows) or None: not a program"""
    nodes = expr.nodes()
    if not nodes or len(nodes) > SA_PROG_MAX:
        return None
    st, pool, is_wide = [], 0, False
    for n in nodes:
        if n.op == abi.EXPR_INPUT_REF:
            if not 0 <= n.index < len(dtypes) or len(st) >= SA_STACK_MAX:
                return None
            d = dtypes[n.index]
            if d not in NUMERIC:
                if not wide or d not in (abi.UTF8, abi.BOOLEAN):
                    return None
                is_wide = True
            st.append(d)
        elif n.op == abi.EXPR_CONSTANT:
            if len(st) >= SA_STACK_MAX:
                return None
            if n.dtype == abi.UTF8:
                if not wide:
                    return None
                pool += 0 if n.is_null or n.s is None else len(n.s)
                if pool > SA_POOL_MAX:
                    return None
                is_wide = True
            elif n.dtype not in NUMERIC + (abi.BOOLEAN,):
                return None
            st.append(n.dtype)
        elif n.op == abi.EXPR_TYPE_CAST:
            if not st or st[-1] == abi.UTF8:
                return None
            if st[-1] != n.dtype:
                if n.dtype not in NUMERIC:
                    return None
                st[-1] = n.dtype
        else:
            if len(st) < 2:
                return None
            r, l = st.pop(), st.pop()
            if abi.EXPR_PLUS <= n.op <= abi.EXPR_DIVIDE:
                if l != r or l not in NUMERIC:
                    return None
                st.append(l)
            elif abi.EXPR_GT <= n.op <= abi.EXPR_NOTEQ:
                if l != r:
                    return None
                st.append(abi.BOOLEAN)
            elif n.op in (abi.EXPR_AND, abi.EXPR_OR):
                if l != abi.BOOLEAN or r != abi.BOOLEAN:
                    return None
                st.append(abi.BOOLEAN)
            else:
                return None
    return (st[0], pool, is_wide) if len(st) == 1 else None


def raw_bytes(batch):
    return sum(b.size for c in batch.columns for b in c.buffers() if b is not None)


def fits(batch, pool=0):
    """the staged bytes against the slot: no layout arithmetic, so no answer within a tenth of the limit"""
    raw = raw_bytes(batch) + pool
    assert not 0.9 * SA_AREA <= raw <= 1.1 * SA_AREA, ("a case too close to the slot's size for this rule", raw)
    return raw < SA_AREA


def dtypes_of(batch):
    return [abi.dtype_of(f.type) for f in batch.schema]


def filter_eligible(expr, batch, on=True):
    dt = dtypes_of(batch)
    if batch.num_rows > SA_MAX_ROWS or not 0 < len(dt) <= SA_MAX_COLS:
        return False
    if not on and abi.BOOLEAN in dt:  # (switch off: a Boolean column is not laid out)
        return False
    c = compiles(expr, dt, wide=on)
    return c is not None and c[0] == abi.BOOLEAN and fits(batch, c[1])


def project_eligible(exprs, batch, on=True):
    dt = dtypes_of(batch)
    if batch.num_rows > SA_MAX_ROWS or not 0 < len(dt) <= SA_MAX_COLS or not 0 < len(exprs) <= SA_MAX_COLS:
        return False
    pool = computed = 0
    for e in exprs:
        if isinstance(e, InputRef):  # a bare reference: copied by the host, any of the five types
            continue
        c = compiles(e, dt, wide=on)
        computed += 1
        if c is None or c[0] == abi.UTF8 or computed > SP_PROGS:
            return False
        pool += c[1]
    return fits(batch, pool)


def count_eligible(expr, batches, on=True):
    if isinstance(expr, (list, tuple)):
        return sum(1 for b in batches if project_eligible(expr, b, on))
    return sum(1 for b in batches if filter_eligible(expr, b, on))


def binary_nodes(e):
    return sum(1 for n in e.nodes() if n.op >= abi.EXPR_PLUS)


# ---- the stream -------------------------------------------------------------------------------------------------------
# a int64 0, b float64 1, c int32 2, s utf8 3, t utf8 4, p bool 5, q bool 6, rid int64 7
A, B, C_, S, T, P, Q, RID = range(8)
LONG = "x" * 150 + "é" * 75  # 300 bytes; LONG + "a" and LONG + "b" differ only in their last byte
VOCAB = M.POOL_UTF8 + ["ab", "ab", "abd", ""] + [LONG + "a", LONG + "b"]
SIZES = [1024] * 8 + [0, 1, 63, 64, 65, 1023, 1025, 4096, 4097]

_cache = {}


def _cached(fn):
    def wrapped(*a):
        key = (fn.__name__,) + a
        if key not in _cache:
            _cache[key] = fn(*a)
        return _cache[key]
    return wrapped


def _strings(rng, rows, vocab, nulls, long_share=0.01, shift=0):
    w = np.full(len(vocab), (1 - 2 * long_share) / (len(vocab) - 2))
    w[-2:] = long_share
    vals = [vocab[i] for i in rng.choice(len(vocab), rows, p=w)]
    return str_array(vals, (rng.random(rows) < nulls) if rows else None, shift=shift)


def stream_batch(rng, rows, nulls=0.15, wide_strings=False, shift=0):
    def mask():
        return rng.random(rows) < nulls
    if wide_strings:  # ~200-byte strings: two Utf8 columns of 4096 x 200 bytes are over the slot
        s = str_array(["s%05d" % i + "y" * int(rng.integers(180, 220)) for i in range(rows)], mask())
        t = str_array(["s%05d" % i + "y" * int(rng.integers(180, 220)) for i in range(rows)], mask())
    else:
        s, t = _strings(rng, rows, VOCAB, nulls, shift=shift), _strings(rng, rows, VOCAB, nulls)
        if rows > 3:  # LONG + "a" against LONG + "b" in one row, both ways, and against itself
            sl, tl = s.to_pylist(), t.to_pylist()
            sl[0], tl[0], sl[1], tl[1], sl[2], tl[2] = LONG + "a", LONG + "b", LONG + "b", LONG + "a", LONG + "a", LONG + "a"
            s, t = str_array(sl, np.array([v is None for v in sl]), shift=shift), str_array(tl, np.array([v is None for v in tl]))
    return pa.RecordBatch.from_arrays(
        [pa.array(rng.integers(-10, 10, rows), mask=mask()), pa.array(np.round(rng.random(rows), 3), mask=mask()),
         pa.array(rng.integers(-5, 5, rows).astype(np.int32), mask=mask()), s, t,
         pa.array(rng.random(rows) < 0.5, mask=mask()), pa.array(rng.random(rows) < 0.3, mask=mask()),
         pa.array(np.arange(rows, dtype=np.int64))], names=["a", "b", "c", "s", "t", "p", "q", "rid"])


@_cached
def stream():
    rng = np.random.default_rng(101)
    bs = [stream_batch(rng, rows) for rows in SIZES]
    bs.insert(5, stream_batch(rng, 4096, wide_strings=True))
    return bs


@_cached
def adjacent_utf8_stream():
    """(s utf8, t utf8, rid int64) at 65 and 1025 rows, NO NULL in either Utf8 column: the one shape in which the Filter goes from
    one Utf8 column's byte copy to the next column's lengths through the bare `else __syncthreads()` and not through the barriers
    of a bitmap pass.  It pins that route's RESULT; it cannot tell whether that barrier is there (a thread's first stores into the
    lengths go to the entries it read itself, and the scan's stores come behind the next column's own first barrier)"""
    rng = np.random.default_rng(211)
    return [pa.RecordBatch.from_arrays([_strings(rng, rows, VOCAB, 0.0), _strings(rng, rows, VOCAB, 0.0, shift=5), pa.array(np.arange(rows, dtype=np.int64))],
                                       names=["s", "t", "rid"]) for rows in (65, 1025)]


def stream_predicates():
    s, t, a, p, q = InputRef(S), InputRef(T), InputRef(A), InputRef(P), InputRef(Q)
    u = lambda v: Constant(v, abi.UTF8)  # noqa: E731
    return {
        "s_eq_const": s.eq(u("ab")),
        "s_ne_empty": s.ne(u("")),
        "s_ge_t": s >= t,
        "s_lt_e_acute": s < u("é"),
        "s_eq_null": s.eq(u(None)),
        "s_eq_and_num": s.eq(u("ab")) & (a > Constant(3, abi.INT64)),
        "s_gt_t_or_p": (s > t) | p,
        "p": p,
        "p_and_q": p & q,
        "p_eq_q": p.eq(q),
        "cast_p_plus_a": (TypeCast(p, abi.INT64) + a) > Constant(0, abi.INT64),
        "numeric_only": (a + Constant(1, abi.INT64)) > TypeCast(InputRef(C_), abi.INT64),  # Boolean PAYLOAD columns alone
        "numeric_conj": a > Constant(3, abi.INT64),  # ... and through the `column OP constant` path
    }


def stream_projection():
    """computed Boolean / numeric columns over the new operand kinds next to bare references of every type"""
    s, t, a, p, q = InputRef(S), InputRef(T), InputRef(A), InputRef(P), InputRef(Q)
    return [s >= t, InputRef(S), InputRef(P), TypeCast(p, abi.INT64) + a, (s.eq(Constant("ab", abi.UTF8))) | q, InputRef(B), InputRef(RID)]


# ---- cross products ---------------------------------------------------------------------------------------------------
def utf8_cross_cases():
    """[(label, expression)] over expr_model.utf8_batch(): six comparisons x {column-column, column-constant, constant-column}"""
    out = []
    for op in CMP_OPS:
        out.append((f"x {op} y", BinaryOp(op, InputRef(0), InputRef(1))))
        for v in M.POOL_UTF8 + [None]:
            out.append((f"x {op} {v!r}", BinaryOp(op, InputRef(0), Constant(v, abi.UTF8))))
            out.append((f"{v!r} {op} y", BinaryOp(op, Constant(v, abi.UTF8), InputRef(1))))
    return out


def bool_cross_cases():
    out = []
    for op in CMP_OPS + ("and", "or"):
        out.append((f"p {op} q", BinaryOp(op, InputRef(0), InputRef(1))))
        for v in (False, True, None):
            out.append((f"p {op} {v!r}", BinaryOp(op, InputRef(0), Constant(v, abi.BOOLEAN))))
            out.append((f"{v!r} {op} q", BinaryOp(op, Constant(v, abi.BOOLEAN), InputRef(1))))
    return out


# ---- fuzz -------------------------------------------------------------------------------------------------------------
ALL_TYPES = (abi.INT64, abi.INT32, abi.FLOAT64, abi.UTF8, abi.BOOLEAN)
FUZZ_STRINGS = M.POOL_UTF8 + ["ab", "abc", "zz", LONG[:40], LONG[:40] + "a"]


def fuzz_schema(rng):
    """every type once and up to five more columns in random order; with rid at most 11 of the 12 columns a slot lays out"""
    n = int(rng.integers(0, 6))
    dts = list(ALL_TYPES) + [ALL_TYPES[int(i)] for i in rng.integers(0, 5, n)]
    rng.shuffle(dts)
    return dts


def fuzz_batch(rng, dts, rows):
    cols = []
    for d in dts:
        mask = (rng.random(rows) < float(rng.choice([0.0, 0.1, 0.5]))) if rows else None
        if d == abi.UTF8:
            vals = [FUZZ_STRINGS[i] for i in rng.integers(0, len(FUZZ_STRINGS), rows)]
            cols.append(str_array(vals, mask, shift=int(rng.integers(0, 2)) * 3))
        elif d == abi.BOOLEAN:
            cols.append(pa.array(rng.random(rows) < 0.5, mask=mask))
        elif d == abi.FLOAT64:
            cols.append(pa.array(rng.integers(-40, 40, rows) * 0.25, mask=mask))  # (exact in every +, -, * of a small tree)
        else:
            cols.append(pa.array(rng.integers(-20, 20, rows).astype(np.int32 if d == abi.INT32 else np.int64), mask=mask))
    cols.append(pa.array(np.arange(rows, dtype=np.int64)))
    return pa.RecordBatch.from_arrays(cols, names=[f"c{i}" for i in range(len(dts))] + ["rid"])


def fuzz_tree(rng, dts, want, depth):
    """a random tree of type `want` over the columns `dts`: Utf8 operands only under comparisons, Boolean columns under
    comparisons, AND / OR and casts, numeric arithmetic without division (no NaN, no error: nothing is left out)"""
    cols = [i for i, d in enumerate(dts) if d == want]

    def leaf():
        if cols and rng.random() < 0.75:
            return InputRef(int(rng.choice(cols)))
        if rng.random() < 0.1:
            return Constant(None, want)
        if want == abi.UTF8:
            return Constant(FUZZ_STRINGS[int(rng.integers(0, len(FUZZ_STRINGS)))], abi.UTF8)
        if want == abi.BOOLEAN:
            return Constant(bool(rng.random() < 0.5), abi.BOOLEAN)
        if want == abi.FLOAT64:
            return Constant(float(rng.integers(-8, 8)) * 0.5, abi.FLOAT64)
        return Constant(int(rng.integers(-6, 6)), want)
    if want == abi.UTF8 or depth <= 0:
        return leaf()
    r = rng.random()
    if want == abi.BOOLEAN:
        if r < 0.2:
            return leaf()
        if r < 0.6:
            t = ALL_TYPES[int(rng.integers(0, 5))]
            op = CMP_OPS[int(rng.integers(0, 6))]
            l, r = fuzz_tree(rng, dts, t, depth - 1), fuzz_tree(rng, dts, t, depth - 1)
            if t == abi.UTF8 and isinstance(l, Constant) and isinstance(r, Constant):  # (one side of a Utf8 comparison is a column)
                l = InputRef(dts.index(abi.UTF8))
            return BinaryOp(op, l, r)
        return BinaryOp("and" if r < 0.8 else "or", fuzz_tree(rng, dts, abi.BOOLEAN, depth - 1), fuzz_tree(rng, dts, abi.BOOLEAN, depth - 1))
    if r < 0.3:
        return leaf()
    if r < 0.5:  # a cast from another numeric type or from Boolean (small values: always in range)
        src = [abi.INT64, abi.INT32, abi.FLOAT64, abi.BOOLEAN][int(rng.integers(0, 4))]
        return TypeCast(fuzz_tree(rng, dts, src, depth - 1), want)
    return BinaryOp("+-*"[int(rng.integers(0, 3))], fuzz_tree(rng, dts, want, depth - 1), fuzz_tree(rng, dts, want, depth - 1))


@_cached
def fuzz_case(seed):
    """(batches, [filter predicates], [projection])"""
    rng = np.random.default_rng(900 + seed)
    dts = fuzz_schema(rng)
    batches = [fuzz_batch(rng, dts, rows) for rows in (1024, 65, 0, 700, 5000)]
    preds = [fuzz_tree(rng, dts, abi.BOOLEAN, 3) for _ in range(4)]
    proj = [fuzz_tree(rng, dts, [abi.BOOLEAN, abi.INT64, abi.FLOAT64, abi.INT32][k % 4], 2) for k in range(3)]
    proj = [e for e in proj if not isinstance(e, (InputRef, Constant))]
    proj += [InputRef(i) for i in range(len(dts) + 1)][-4:]
    return batches, preds, proj


# ---- expected values, computed once and shared ------------------------------------------------------------------------
@_cached
def stream_model(name):
    """the model's Result of stream predicate `name` for every batch of stream()"""
    e = stream_predicates()[name]
    return [M.evaluate(e, b) for b in stream()]


@_cached
def stream_projection_model():
    return [[M.evaluate(e, b) for e in stream_projection()] for b in stream()]


def assert_filter_stream(got, batches, results, what, rid):
    """`got` = one output batch per input batch, each the model's kept rows; nothing left out for these types"""
    assert len(got) == len(batches), (what, len(got), len(batches))
    for k, (g, b, res) in enumerate(zip(got, batches, results)):
        assert M.assert_filter_matches(g, b, res, f"{what} batch {k}", rid=rid) == 0


def assert_project_stream(got, batches, exprs, results, what):
    assert len(got) == len(batches), (what, len(got), len(batches))
    for k, (g, b, row) in enumerate(zip(got, batches, results)):
        assert g.num_rows == b.num_rows and g.num_columns == len(exprs), (what, k)
        for c, (e, res) in enumerate(zip(exprs, row)):
            assert M.assert_column_matches(g.column(c), res, f"{what} batch {k} column {c}") == 0


def same_batches(got, exp, what=""):
    assert [g.num_rows for g in got] == [e.num_rows for e in exp], what
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g.num_columns == e.num_columns, (what, k)
        for c in range(g.num_columns):
            assert g.column(c).type == e.column(c).type, (what, k, c)
            assert M.column_values(g.column(c)) == M.column_values(e.column(c)), (what, "batch", k, "column", c)
