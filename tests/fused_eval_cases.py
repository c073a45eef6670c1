"""The cases of the fused-evaluation route of the synchronous Filter / Project (SQLRS_EXPR_FUSED_EVAL; witnesses
`fused_eval_filter_batches` / `fused_eval_project_columns`), shared by test_fused_eval_cpu.py (the conditions the GPU file
relies on) and test_gpu_fused_eval.py (the device against expr_model and against the switch-off route).

Case builders only: the expressions and batches come from expr_model (tree_case, binary_cases, cast_batch, bool_batch,
div0_cases, program_shape); this file adds the forecast "this expression compiles", the row counts at which the kernels change
shape, and the expressions of the two-sweep cases, whose result numpy states directly."""
import functools

import numpy as np
import pyarrow as pa

import expr_model as M
from sqlrs_amd import abi
from sqlrs_amd.expr import BinaryOp, Constant, InputRef, TypeCast

# the limits of the route (small_async.hpp: SA_PROG_MAX, SA_STACK_MAX; expr_fused_kernels.hpp: FE_MAX_COLS, FE_MAX_PROGS and the
# grid: min(ceil(rows / 1024), 2048) workgroups, so one sweep of the grid is 2^21 rows).  test_gpu_fused_eval.py takes none of
# them on trust: the counters say whether an expression of exactly / one past each limit ran fused.
PROG_MAX, STACK_MAX, MAX_COLS, MAX_PROGS = 24, 8, 16, 4
SWEEP_ROWS = 2048 * 1024
ROW_COUNTS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]
SWEEP_N = 2 * SWEEP_ROWS + 77  # two full sweeps, then one full 64-row group and a ragged one
FORMS = ["host", "device", "window"]


# ---- the forecast ----------------------------------------------------------------------------------------------------------
def compiles(expr, dtypes) -> bool:
    """a WELL-TYPED expression over columns of `dtypes` runs as a program: at most PROG_MAX nodes, STACK_MAX operands in
    flight, MAX_COLS distinct columns, and neither a Utf8 column nor a Utf8 constant"""
    nodes = expr.nodes()
    n, deepest = M.program_shape(expr)
    if n > PROG_MAX or deepest > STACK_MAX:
        return False
    cols = set()
    for nd in nodes:
        if nd.op == abi.EXPR_INPUT_REF:
            if dtypes[nd.index] == abi.UTF8:
                return False
            cols.add(nd.index)
        elif nd.op == abi.EXPR_CONSTANT and nd.dtype == abi.UTF8:
            return False
    return len(cols) <= MAX_COLS


def takes_cmp_const(expr, dtypes) -> bool:
    """`column OP constant` (a non-NULL constant of the column's numeric type): the Filter's first one-pass route, which is
    tried before the program"""
    nd = expr.nodes()
    if len(nd) != 3:
        return False
    a, b, o = nd
    return (a.op == abi.EXPR_INPUT_REF and b.op == abi.EXPR_CONSTANT and not b.is_null and abi.EXPR_GT <= o.op <= abi.EXPR_NOTEQ
            and dtypes[a.index] == b.dtype and b.dtype in (abi.INT32, abi.INT64, abi.FLOAT64))


def is_computed(expr) -> bool:
    """not a bare InputRef / constant: a column the program kernel writes"""
    return len(expr.nodes()) > 1


def binary_nodes(expr) -> int:
    return sum(1 for n in expr.nodes() if n.op >= abi.EXPR_PLUS)


def dtypes_of(batch) -> list:
    return [abi.dtype_of(batch.column(k).type) for k in range(batch.num_columns)]


# ---- expressions of known shape ---------------------------------------------------------------------------------------------
def left_deep(m, col=0):
    """2 m - 1 nodes, stack 2, over int64 column `col`"""
    a = InputRef(col)
    e = a
    for i in range(m - 1):
        e = e + (a if i % 2 else Constant(M.POOL_I64[i % len(M.POOL_I64)], abi.INT64))
    return e


def right_deep(m):
    """stack m, over the int64 columns 0 and 1"""
    e = InputRef(0)
    for i in range(m - 1):
        e = BinaryOp("-" if i % 2 else "+", InputRef(1) if i % 2 else InputRef(0), e)
    return e


def limit_exprs():
    """{label: (expression over trees_batch, runs fused)}: exactly at and one past the node and the stack limit, as values and
    as predicates"""
    n24 = BinaryOp("+", left_deep(11), TypeCast(InputRef(2), abi.INT64))  # 21 + 2 + 1 nodes
    n25 = left_deep(13)
    s8, s9 = right_deep(8), right_deep(9)
    zero = Constant(0, abi.INT64)
    return {"24 nodes": (n24, True), "25 nodes": (n25, False), "stack 8": (s8, True), "stack 9": (s9, False),
            "stack 8, predicate": (s8 > zero, True), "stack 9, predicate": (s9 > zero, False)}


def wide_batch(ncols, n=300, seed=5) -> pa.RecordBatch:
    """`ncols` int64 columns (every third with NULLs) + rid"""
    rng = np.random.default_rng(seed)
    cols = [M.edge_column(rng, abi.INT64, n, 0.2 if k % 3 == 0 else 0.0) for k in range(ncols)]
    cols.append(pa.array(np.arange(n, dtype=np.int64)))
    return pa.RecordBatch.from_arrays(cols, names=[f"c{k}" for k in range(ncols)] + ["rid"])


def sum_of_columns(ncols):
    """c0 + c1 + ... : 2 ncols - 1 nodes, stack 2, ncols distinct columns"""
    e = InputRef(0)
    for k in range(1, ncols):
        e = e + InputRef(k)
    return e


def shape_exprs():
    """over tree_batch (a, b int64; c, d int32; e, f float64; rid): every operator class, numeric and Boolean results"""
    a, b, c, d, e, f = (InputRef(i) for i in range(6))
    return [("a + b", a + b), ("c * d", c * d), ("e - f", e - f), ("a < b", a < b), ("e >= f", e >= f), ("c = d", c.eq(d)),
            ("cast(e, i64)", TypeCast(e, abi.INT64)), ("cast(a, i32)", TypeCast(a, abi.INT32)), ("cast(c, f64)", TypeCast(c, abi.FLOAT64)),
            ("(a > 0) and (e < f)", (a > Constant(0, abi.INT64)) & (e < f)), ("(c < d) or (a = b)", (c < d) | a.eq(b)),
            ("e / 3.0", e / Constant(3.0, abi.FLOAT64)), ("a / -1", a / Constant(-1, abi.INT64)),
            ("e != -0.0 or a > b", e.ne(Constant(-0.0, abi.FLOAT64)) | (a > b))]


@functools.lru_cache(maxsize=None)
def row_count_case(n, nulls):
    """(batch, [(label, expression, model result)]) of shape_exprs over n rows"""
    batch = M.tree_batch(3000 + n, n, nulls, pool_share=0.3)
    return batch, [(f"n = {n}, nulls {nulls}: {l}", e, M.evaluate(e, batch)) for l, e in shape_exprs()]


# ---- Boolean columns as operands ---------------------------------------------------------------------------------------------
def bool_operand_cases():
    """[(label, expression)] over bool_batch (p, q, rid): Boolean columns under comparisons, AND / OR, casts, and as a result"""
    p, q = InputRef(0), InputRef(1)
    out = [(f"p {op} q", BinaryOp(op, p, q)) for op in M.CMP_OPS + ["and", "or"]]
    for k in (False, True, None):
        out.append((f"p = {k}", p.eq(Constant(k, abi.BOOLEAN))))
        out.append((f"{k} or q", BinaryOp("or", Constant(k, abi.BOOLEAN), q)))
        out.append((f"p and {k}", BinaryOp("and", p, Constant(k, abi.BOOLEAN))))
    for name, dt in M.NUMERIC.items():
        out.append((f"cast(p, {name})", TypeCast(p, dt)))
        out.append((f"cast(p, {name}) > cast(q, {name})", TypeCast(p, dt) > TypeCast(q, dt)))
    out.append(("(p and q) or (p != q)", (p & q) | p.ne(q)))
    return out


# ---- the two-sweep cases: numpy is the model -----------------------------------------------------------------------------------
K_WRAP, C_LT = (1 << 62), -(1 << 61)


@functools.lru_cache(maxsize=1)
def sweep_case():
    """SWEEP_N rows of (i, j64, i2 int64; rid): i and j64 near +-2^62 so that i + j64 wraps, NULLs in i (random) and j64 (every
    64-row group alternately all valid / half NULL).  Returns the columns as numpy (values, valid) pairs and the batch."""
    n = SWEEP_N
    rng = np.random.default_rng(77)
    i = rng.integers(-(1 << 62) - 1000, (1 << 62) + 1000, n, dtype=np.int64)
    i[::5] = (1 << 62) + rng.integers(0, 1 << 61, len(i[::5]), dtype=np.int64)
    j = rng.integers(-(1 << 62), (1 << 62), n, dtype=np.int64)
    j[::7] = (1 << 62) + rng.integers(0, 1 << 61, len(j[::7]), dtype=np.int64)
    i2 = rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64)
    vi = rng.random(n) >= 0.1
    vj = np.ones(n, bool)
    grp = np.arange(n) >> 6
    vj[(grp % 2 == 1) & (np.arange(n) % 2 == 0)] = False
    cols = {"i": (i, vi), "j64": (j, vj), "i2": (i2, None)}
    arrays = [pa.array(v, mask=None if ok is None else ~ok) for v, ok in cols.values()] + [pa.array(np.arange(n, dtype=np.int64))]
    return cols, pa.RecordBatch.from_arrays(arrays, names=list(cols) + ["rid"])


def sweep_predicate():
    """i + j64 > K OR i2 < C"""
    return ((InputRef(0) + InputRef(1)) > Constant(K_WRAP, abi.INT64)) | (InputRef(2) < Constant(C_LT, abi.INT64))


def sweep_value():
    """i * 3 - j64"""
    return InputRef(0) * Constant(3, abi.INT64) - InputRef(1)


def sweep_predicate_numpy(cols):
    """(value where valid, valid) of sweep_predicate by Kleene over masks: TRUE when either side is TRUE, NULL when neither is
    and one is NULL"""
    (i, vi), (j, vj), (i2, _) = cols["i"], cols["j64"], cols["i2"]
    with np.errstate(over="ignore"):
        s = (i.view(np.uint64) + j.view(np.uint64)).view(np.int64)
    left_valid = vi & vj
    left = left_valid & (s > K_WRAP)
    right = i2 < C_LT
    true = left | right
    valid = true | left_valid  # (right is never NULL: FALSE OR NULL = NULL)
    return true, valid


def sweep_value_numpy(cols):
    (i, vi), (j, vj) = cols["i"], cols["j64"]
    with np.errstate(over="ignore"):
        v = (i.view(np.uint64) * np.uint64(3) - j.view(np.uint64)).view(np.int64)
    return v, vi & vj


# ---- every case whose model result the GPU file compares against: the left-out cap is checked on the model alone ------------------
def model_results():
    """yields (label, Result) of every modelled case of the GPU file (divisions by zero excluded: they have no Result)"""
    for n in ROW_COUNTS:
        for nulls in (0.0, 0.1):
            for label, _, res in row_count_case(n, nulls)[1]:
                yield label, res
    for k in range(M.N_TREES):
        e, _, out = M.tree_case(k)
        if out is not M.DIV0:
            yield f"tree {k}", out
    for kind, dt in M.NUMERIC.items():
        for op in M.ARITH_OPS + M.CMP_OPS:
            for form in ("colcol", "colconst"):
                for label, e, b in M.binary_cases(dt, op, form):
                    yield f"{kind}: {label}", M.evaluate(e, b)
    for label, e in bool_operand_cases():
        yield label, M.evaluate(e, M.bool_batch())
    for label, (e, _) in limit_exprs().items():
        yield label, M.evaluate(e, M.trees_batch())
