"""Every device route of the expression evaluator against the independent edge-value model (tests/expr_model.py), and
against each other on the same input.

routes                                   what tells that the route ran (hip.profile_read)
* per-node kernels (expr.hip)            `expr_binary` / `expr_cast` rise by the nodes evaluated
* in-kernel postfix program              `async_fast_batches` rises by the batches pushed, `expr_binary` and
                                         `async_conj_batches` do not move
* conjunction fast path (ops.hip)        `async_fast_batches` AND `async_conj_batches` rise by the batches pushed
* fused `col OP const` filter            `filter_cmp_const` rises
* RowFilter of the partition pass        `hash_partition_filter` rises

All comparisons are bit exact — values by bit pattern (so -0.0 and the sign and payload of a NaN count), validity, row
order — apart from the rows on which the model says the hardware chooses the NaN (expr_model: ANY_NAN is compared as "is a
NaN", LEFT_OUT not at all); every comparison asserts that at most 2 % of its rows are left out."""
import ctypes as C
from contextlib import contextmanager

import numpy as np
import pyarrow as pa
import pytest

import expr_model as M
from sqlrs_amd import abi
from sqlrs_amd.executor import FilterExecutor, ProjectExecutor, eval_column
from sqlrs_amd.expr import BinaryOp, Constant, InputRef, TypeCast

pytestmark = pytest.mark.gpu

# The limits of the small-batch kernels (small_async.hpp / plumbing.hip).  None of them is taken on trust: the counters say
# whether a batch of SA_ROWS / SA_ROWS + 1 rows (test_row_counts, test_conjunction_fast_path), a tree of SA_PROG_MAX /
# SA_PROG_MAX + 1 nodes and SA_STACK_MAX / SA_STACK_MAX + 1 operands (test_program_limits) and a projection of SP_PROGS
# computed columns (check_program) ran in the one-launch kernel, so a limit that moves in the library turns those tests red.
SA_ROWS, SA_PROG_MAX, SA_STACK_MAX, SP_PROGS = 4096, 24, 8, 6
# The fused filter's tile has no such witness in the counters: the library reports it (sqlrs_filter_tile_rows).
TILE_SIZES = {"tile - 1": (1, -1), "tile": (1, 0), "tile + 1": (1, 1), "2 tile + 1": (2, 1)}


def filter_rows(be, n) -> int:
    """a row count of test_fused_filter: a number, or a TILE_SIZES name resolved with the library's tile"""
    if isinstance(n, int):
        return n
    tile = be.fn("filter_tile_rows")()
    assert tile > 4097 and tile % 64 == 0, tile
    times, plus = TILE_SIZES[n]
    return times * tile + plus


# ---- which route ran ---------------------------------------------------------------------------------------------------------
def counters(be) -> dict:
    cap = 512  # (profile_read's 64 entries may not reach the counters at the end of a long session)
    names, ms, n_l = (C.c_char_p * cap)(), (C.c_double * cap)(), (C.c_int64 * cap)()
    n = be.fn("ctx_profile_read")(be.ctx, cap, names, ms, n_l)
    assert n <= cap
    return {names[k].decode(): n_l[k] for k in range(n)}


@contextmanager
def route(be, exactly=None, at_least=None, still=()):
    """asserts how far the profile counters move across the block: `exactly` / `at_least` {name: by}, `still` names at rest"""
    before = counters(be)
    yield
    after = counters(be)
    moved = {k: after.get(k, 0) - before.get(k, 0) for k in set(after) | set(before)}
    for k, by in (exactly or {}).items():
        assert moved.get(k, 0) == by, (k, "moved by", moved.get(k, 0), "expected", by)
    for k, by in (at_least or {}).items():
        assert moved.get(k, 0) >= by, (k, "moved by", moved.get(k, 0), "expected at least", by)
    for k in still:
        assert moved.get(k, 0) == 0, (k, "moved by", moved.get(k, 0), "expected to rest")


@pytest.fixture(autouse=True)
def profiled(hip):
    hip.profile(True)
    yield
    hip.profile(False)


def binary_nodes(e) -> int:
    return sum(1 for n in e.nodes() if n.op >= abi.EXPR_PLUS)


def program_accepts(e) -> bool:
    nodes, deepest = M.program_shape(e)
    return nodes <= SA_PROG_MAX and deepest <= SA_STACK_MAX


def is_conjunction_shape(e) -> bool:
    """`col OP const [AND col OP const]...` with non-NULL constants of the column's type: the shape the async Filter is
    meant to take without the program.  Only a forecast — `async_conj_batches` says whether the library did."""
    nd = e.nodes()
    if len(nd) < 3 or (len(nd) - 3) % 4 or len(nd) > 15:
        return False
    for k in range(1 + (len(nd) - 3) // 4):
        at = 0 if k == 0 else 3 + (k - 1) * 4
        a, b, o = nd[at:at + 3]
        if a.op != abi.EXPR_INPUT_REF or b.op != abi.EXPR_CONSTANT or b.is_null or not (abi.EXPR_GT <= o.op <= abi.EXPR_NOTEQ):
            return False
        if k and nd[at + 3].op != abi.EXPR_AND:
            return False
    return True


def guarded(fn):
    """fn() or M.DIV0 for the evaluators' Arrow error"""
    try:
        return fn()
    except abi.ExecutorError as err:
        assert err.status == abi.ERR_ARROW and M.DIV0 in err.message, err
        return M.DIV0


# ---- the per-node route ------------------------------------------------------------------------------------------------------
def check_per_node(hip, cases, casts=None):
    """cases [(label, expr, batch, model outcome)] of ONE batch, none dividing by zero: eval_column, then ProjectExecutor
    (synchronous push) with HOST and with DEVICE output, each against the model; `expr_binary` counts every binary node"""
    batch = cases[0][2]
    nb = sum(binary_nodes(e) for _, e, _, _ in cases)
    exact = {"expr_binary": 3 * nb}
    if casts is not None:
        exact["expr_cast"] = 3 * casts
    with route(hip, exactly=exact, still=("async_fast_batches", "filter_cmp_const")):
        for label, e, b, exp in cases:
            assert b is batch
            M.assert_column_matches(eval_column(hip, e, b).column(0), exp, label)
        exprs = [e for _, e, _, _ in cases]
        (host,) = list(ProjectExecutor(hip, exprs, [batch]).execute())
        (dev,) = list(ProjectExecutor(hip, exprs, [batch], out_mem=abi.MEM_DEVICE).execute())
        dev = hip.to_host(dev).to_arrow()
        for c, (label, _, _, exp) in enumerate(cases):
            M.assert_column_matches(host.column(c), exp, label + " (project, HOST)")
            M.assert_column_matches(dev.column(c), exp, label + " (project, DEVICE)")


def check_program(hip, cases, fast=True):
    """the same cases through ProjectExecutor(depth=1) — sqlrs_project_push_async, at most SP_PROGS computed columns a
    projection — and, for Boolean results, FilterExecutor(depth=1); `fast` False: shapes the program compiler refuses, which
    must come back from the synchronous operator all the same"""
    batch = cases[0][2]
    assert batch.num_rows <= SA_ROWS or not fast
    for at in range(0, len(cases), SP_PROGS):
        group = cases[at:at + SP_PROGS]
        exprs = [e for _, e, _, _ in group]
        with route(hip, exactly={"async_fast_batches": 1 if fast else 0, "async_conj_batches": 0},
                   still=("expr_binary", "expr_cast") if fast else ()):
            (out,) = list(ProjectExecutor(hip, exprs + [InputRef(batch.num_columns - 1)], [batch], depth=1).execute())
        assert out.column(len(group)).to_pylist() == list(range(batch.num_rows))
        for c, (label, _, _, exp) in enumerate(group):
            M.assert_column_matches(out.column(c), exp, label + " (project_push_async)")
    for label, e, b, exp in cases:
        if exp.dtype != abi.BOOLEAN:
            continue
        conj = int(fast and is_conjunction_shape(e))  # (`(x > 0) and (y < 0)` is a program as a projection, a conjunction as a filter)
        with route(hip, exactly={"async_fast_batches": 1 if fast else 0, "async_conj_batches": conj},
                   still=("expr_binary", "expr_cast", "filter_cmp_const") if fast else ()):
            (out,) = list(FilterExecutor(hip, e, [b], depth=1).execute())
        M.assert_filter_matches(out, b, exp, label + " (filter_push_async)")


def with_model(cases):
    out = []
    for label, e, b in cases:
        exp = M.model_outcome(e, b)
        assert exp is not M.DIV0, label
        out.append((label, e, b, exp))
    return out


@pytest.mark.parametrize("form", ["colcol", "colconst"])
@pytest.mark.parametrize("op", M.ARITH_OPS + M.CMP_OPS)
@pytest.mark.parametrize("kind", list(M.NUMERIC))
def test_binary_operators_over_the_pool_cross_product(hip, kind, op, form):
    """operator x type x pool: per-node kernels (arith_kernel / cmp_kernel) and the postfix program; one assertion per
    arithmetic operator that inf - inf, 0 * inf, inf / inf come back as NaNs is part of the ANY_NAN comparison"""
    cases = with_model([(f"{kind}: {l}", e, b) for l, e, b in M.binary_cases(M.NUMERIC[kind], op, form)])
    check_per_node(hip, cases)
    program = [c for c in cases if not is_conjunction_shape(c[1])]
    check_program(hip, program)
    conj = [c for c in cases if is_conjunction_shape(c[1])]
    for label, e, b, exp in conj:  # (`x OP k`: the conjunction path of the async filter; as a projection it is a program)
        with route(hip, exactly={"async_fast_batches": 1, "async_conj_batches": 1}, still=("expr_binary", "filter_cmp_const")):
            (out,) = list(FilterExecutor(hip, e, [b], depth=1).execute())
        M.assert_filter_matches(out, b, exp, label + " (conjunction)")
    if conj:
        check_program(hip, [(l, TypeCast(e, abi.INT32), b, M.evaluate(TypeCast(e, abi.INT32), b)) for l, e, b, _ in conj])


INF = float("inf")


@pytest.mark.parametrize("op,a,b", [("-", INF, INF), ("+", INF, -INF), ("*", 0.0, INF), ("*", -0.0, -INF), ("/", INF, INF), ("/", -INF, INF)])
def test_invalid_operations_make_a_nan_on_the_device(hip, op, a, b):
    """inf - inf, inf + -inf, 0 * inf, inf / inf: whatever its sign and payload, the result is a NaN — per node, with a
    constant operand, and in the program"""
    n = 130
    batch = pa.RecordBatch.from_arrays([pa.array([a] * n), pa.array([b] * n), pa.array(np.arange(n))], names=["x", "y", "rid"])
    for e in (BinaryOp(op, InputRef(0), InputRef(1)), BinaryOp(op, InputRef(0), Constant(b, abi.FLOAT64)),
              BinaryOp(op, Constant(a, abi.FLOAT64), InputRef(1))):
        exp = M.evaluate(e, batch)
        assert exp.state == [M.ANY_NAN] * n
        with route(hip, exactly={"expr_binary": 1}, still=("async_fast_batches",)):
            got = eval_column(hip, e, batch).column(0)
        assert got.null_count == 0 and np.isnan(got.to_numpy()).all()
        with route(hip, exactly={"async_fast_batches": 1, "async_conj_batches": 0}, still=("expr_binary",)):
            (out,) = list(ProjectExecutor(hip, [e], [batch], depth=1).execute())
        assert out.column(0).null_count == 0 and np.isnan(out.column(0).to_numpy()).all()


@pytest.mark.parametrize("dst", ["i32", "i64", "f64"])
@pytest.mark.parametrize("src", list(M.CAST_SOURCES))
def test_cast_lattice(hip, src, dst):
    """cast_kernel / cast_bool_kernel and the program's SAO_CAST: truncation, both range bounds inclusive (-2^63 -> INT64_MIN),
    NaN / inf -> NULL, int64 -> double to nearest even"""
    s, d = M.CAST_SOURCES[src], M.NUMERIC[dst]
    b = M.cast_batch(s)
    col = with_model([(f"cast {src} -> {dst}", TypeCast(InputRef(0), d), b)])
    pool = [False, True] if s == abi.BOOLEAN else M.POOLS[s]
    consts = with_model([(f"cast {src} constant {k} -> {dst}",
                          TypeCast(Constant(k, s) if s == abi.BOOLEAN else M.pool_constant(s, k), d), b) for k in list(pool) + [None]])
    check_per_node(hip, col + consts, casts=0 if s == d else 1 + len(consts))
    check_program(hip, consts)
    check_program(hip, col, fast=s != abi.BOOLEAN)  # (a Boolean COLUMN is bit-packed: the synchronous operator takes the batch)


def test_the_double_that_is_int64_min_casts_to_int64_min(hip):
    vals = [-(2.0 ** 63), float(np.nextafter(-(2.0 ** 63), -np.inf)), float(np.nextafter(-(2.0 ** 63), 0.0)),
            float(np.nextafter(2.0 ** 63, 0.0)), 2.0 ** 63] * 20
    b = pa.RecordBatch.from_arrays([pa.array(vals, type=pa.float64()), pa.array(np.arange(len(vals)))], names=["x", "rid"])
    e = TypeCast(InputRef(0), abi.INT64)
    exp = M.evaluate(e, b)
    assert exp.vals[:5] == [-(2 ** 63), None, -(2 ** 63) + 1024, 2 ** 63 - 1024, None]
    check_per_node(hip, [("f64 -> i64 around -2^63", e, b, exp)], casts=1)
    check_program(hip, [("f64 -> i64 around -2^63", e, b, exp)])
    keep = e.eq(Constant(M.I64_MIN, abi.INT64))  # ... and as a predicate
    check_program(hip, [("cast = INT64_MIN", keep, b, M.evaluate(keep, b))])


@pytest.mark.parametrize("op", M.CMP_OPS)
def test_utf8_and_boolean_comparisons(hip, op):
    """cmp_utf8_kernel with a constant on either side; bool_words_kernel over Boolean columns, constants and the results of
    comparisons (the latter in the program as well)"""
    u = M.utf8_batch()
    cases = [(f"utf8 x {op} y", BinaryOp(op, InputRef(0), InputRef(1)), u)]
    for k in M.POOL_UTF8 + [None]:
        cases.append((f"utf8 x {op} {k!r}", BinaryOp(op, InputRef(0), Constant(k, abi.UTF8)), u))
        cases.append((f"utf8 {k!r} {op} y", BinaryOp(op, Constant(k, abi.UTF8), InputRef(1)), u))
    check_per_node(hip, with_model(cases))
    b = M.bool_batch()
    cases = [(f"bool p {op} q", BinaryOp(op, InputRef(0), InputRef(1)), b)]
    for k in (False, True, None):
        cases.append((f"bool p {op} {k}", BinaryOp(op, InputRef(0), Constant(k, abi.BOOLEAN)), b))
        cases.append((f"bool {k} {op} q", BinaryOp(op, Constant(k, abi.BOOLEAN), InputRef(1)), b))
    check_per_node(hip, with_model(cases))
    cases = []
    for kind, dt in M.NUMERIC.items():
        pool, m = M.POOLS[dt], M.matrix_batch(dt)
        for i in (0, len(pool) // 2, len(pool) - 1):
            e = BinaryOp(op, InputRef(0) > M.pool_constant(dt, pool[i]), InputRef(1) <= M.pool_constant(dt, pool[-1 - i]))
            cases.append((f"{kind}: (x > {pool[i]}) {op} (y <= {pool[-1 - i]})", e, m))
        e = BinaryOp(op, InputRef(0) < InputRef(1), Constant(None, abi.BOOLEAN))
        cases.append((f"{kind}: (x < y) {op} NULL", e, m))
    for dt in M.NUMERIC.values():
        sub = with_model([c for c in cases if c[2] is M.matrix_batch(dt)])
        check_per_node(hip, sub)
        check_program(hip, sub)


@pytest.mark.parametrize("op", ["and", "or"])
def test_kleene_and_or(hip, op):
    b = M.bool_batch()
    cases = [(f"p {op} q", BinaryOp(op, InputRef(0), InputRef(1)), b)]
    for k in (False, True, None):
        cases.append((f"p {op} {k}", BinaryOp(op, InputRef(0), Constant(k, abi.BOOLEAN)), b))
        cases.append((f"{k} {op} q", BinaryOp(op, Constant(k, abi.BOOLEAN), InputRef(1)), b))
        for k2 in (False, True, None):
            cases.append((f"{k} {op} {k2}", BinaryOp(op, Constant(k, abi.BOOLEAN), Constant(k2, abi.BOOLEAN)), b))
    check_per_node(hip, with_model(cases))
    m = M.matrix_batch(abi.INT64)  # comparison results (valid, NULL) in the program
    cases = with_model([(f"(x > 0) {op} (y < 0)", BinaryOp(op, InputRef(0) > Constant(0, abi.INT64), InputRef(1) < Constant(0, abi.INT64)), m),
                        (f"(x > 0) {op} NULL", BinaryOp(op, InputRef(0) > Constant(0, abi.INT64), Constant(None, abi.BOOLEAN)), m),
                        (f"TRUE {op} (y < x)", BinaryOp(op, Constant(True, abi.BOOLEAN), InputRef(1) < InputRef(0)), m)])
    check_per_node(hip, cases)
    check_program(hip, cases)


@pytest.mark.parametrize("kind", list(M.NUMERIC))
def test_scalar_scalar_expressions(hip, kind):
    dt = M.NUMERIC[kind]
    b, pool, cases = M.cast_batch(abi.INT64), M.POOLS[dt], []
    for op in M.ARITH_OPS + M.CMP_OPS:
        for i, k in enumerate(list(pool) + [None]):
            k2 = pool[(i * 5 + 3) % len(pool)]
            if op == "/" and M._is_zero(dt, k2):
                k2 = pool[-1]
            cases.append((f"{kind}: {k} {op} {k2}", BinaryOp(op, M.pool_constant(dt, k), M.pool_constant(dt, k2)), b))
    cases = with_model(cases)
    check_per_node(hip, cases)
    check_program(hip, cases)


def test_integer_min_over_minus_one_wraps_on_every_route(hip):
    """the project's choice (Parity, Unpinned): MIN / -1 = MIN, per node and in the program, column and constant"""
    for dt, lo in ((abi.INT64, M.I64_MIN), (abi.INT32, M.I32_MIN)):
        b = pa.RecordBatch.from_arrays([M.array_of(dt, [lo, lo + 1, -1] * 30), M.array_of(dt, [-1, -1, lo] * 30), pa.array(np.arange(90))],
                                       names=["x", "y", "rid"])
        cases = with_model([("x / y", InputRef(0) / InputRef(1), b), ("x / -1", InputRef(0) / Constant(-1, dt), b),
                            ("MIN / y", Constant(lo, dt) / InputRef(1), b)])
        assert cases[0][3].vals[:3] == [lo, -(lo + 1), 0]
        check_per_node(hip, cases)
        check_program(hip, cases)


# ---- divide by zero ----------------------------------------------------------------------------------------------------------
def test_divide_by_zero(hip):
    """a valid row with a zero divisor raises on the per-node route and in the program; a NULL row over zero, a NULL dividend
    and a NULL constant divisor do not"""
    for label, e, b, raises in M.div0_cases():
        exp = M.model_outcome(e, b)
        assert (exp is M.DIV0) == raises, label
        with route(hip, exactly={"expr_binary": 1}, still=("async_fast_batches",)):
            got = guarded(lambda: eval_column(hip, e, b).column(0))
        with route(hip, exactly={"async_fast_batches": 1, "async_conj_batches": 0}, still=("expr_binary",)):
            prog = guarded(lambda: list(ProjectExecutor(hip, [e], [b], depth=1).execute())[0].column(0))
        keep = e.eq(e)
        with route(hip, exactly={"async_fast_batches": 1, "async_conj_batches": 0}, still=("expr_binary",)):
            filt = guarded(lambda: list(FilterExecutor(hip, keep, [b], depth=1).execute())[0])
        if raises:
            assert got is M.DIV0 and prog is M.DIV0 and filt is M.DIV0, label
        else:
            M.assert_column_matches(got, exp, label)
            M.assert_column_matches(prog, exp, label + " (program)")
            assert filt is not M.DIV0, label


@pytest.mark.parametrize("op_kind", ["filter", "project"])
def test_divide_by_zero_surfaces_at_the_wait_of_its_ticket_only(hip, op_kind):
    """three batches pushed before the first wait (one launch group): the second divides by zero — its sqlrs_batch_wait
    returns the Arrow error, the first and the third hand out their batches"""
    good = pa.RecordBatch.from_arrays([pa.array([6, 8, -9] * 40), pa.array([3, -2, 1] * 40)], names=["x", "y"])
    bad = pa.RecordBatch.from_arrays([pa.array([6, 8, -9] * 40), pa.array([3, -2, 1] * 39 + [3, 0, 1])], names=["x", "y"])
    e = InputRef(0) / InputRef(1)
    h, keep = C.c_void_p(), []
    if op_kind == "filter":
        p = (e > Constant(-100, abi.INT64)).pack()
        keep.append(p)
        hip.check(hip.fn("filter_create")(hip.ctx, C.byref(p.abi), C.byref(h)))
    else:
        arr, k = abi.pack_exprs([e])
        keep += [arr, k]
        hip.check(hip.fn("project_create")(hip.ctx, 1, arr, C.byref(h)))
    try:
        tickets = []
        with route(hip, exactly={"async_fast_batches": 3}, still=("expr_binary",)):
            for b in (good, bad, good):
                hb = abi.as_batch(b)
                keep.append(hb)
                t = C.c_void_p()
                hip.check(hip.fn(op_kind + "_push_async")(h, hb.ptr, C.byref(t)))
                tickets.append(t)
            status, outs = [], []
            for t in tickets:
                out = C.POINTER(abi.Batch)()
                status.append(hip.fn("batch_wait")(t, C.byref(out)))
                if status[-1] == abi.ERR_ARROW:
                    assert M.DIV0 in hip.fn("last_error")(hip.ctx).decode()
                outs.append(hip.wrap(out))
        assert status == [abi.OK, abi.ERR_ARROW, abi.OK]
        assert outs[1] is None
        exp = M.evaluate(e, good)
        for o in (outs[0], outs[2]):
            got = o.to_arrow()
            o.release()
            assert got.num_rows == good.num_rows
            if op_kind == "project":
                M.assert_column_matches(got.column(0), exp)
    finally:
        hip.fn(op_kind + "_destroy")(h)


# ---- row counts at which the kernels change shape ---------------------------------------------------------------------------
def shape_exprs():
    a, b, c, d, e, f = (InputRef(i) for i in range(6))
    return [("a + b", a + b), ("c * d", c * d), ("e - f", e - f), ("a < b", a < b), ("e >= f", e >= f), ("c = d", c.eq(d)),
            ("cast(e, i64)", TypeCast(e, abi.INT64)), ("cast(a, i32)", TypeCast(a, abi.INT32)), ("cast(a, f64)", TypeCast(a, abi.FLOAT64)),
            ("(a > 0) and (e < f)", (a > Constant(0, abi.INT64)) & (e < f)), ("(c < d) or (a = b)", (c < d) | a.eq(b)),
            ("e / 3.0", e / Constant(3.0, abi.FLOAT64)), ("a / -1", a / Constant(-1, abi.INT64)), ("e != -0.0", e.ne(Constant(-0.0, abi.FLOAT64)))]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097])
def test_row_counts(hip, n):
    """per-node kernels: 256-thread blocks, a ballot word per 64 rows; small-batch kernels: 1024 threads x 4 rows; 4097 rows
    take the synchronous operator inside push_async and still agree"""
    for nulls in (0.0, 0.1, 0.5):
        batch = M.tree_batch(1000 + n, n, nulls, pool_share=0.3)
        cases = with_model([(f"n = {n}, nulls {nulls}: {l}", e, batch) for l, e in shape_exprs()])
        assert all(c[3].left_out_fraction == 0 for c in cases)
        check_per_node(hip, cases, casts=3)
        check_program(hip, cases, fast=n <= SA_ROWS)


# ---- random trees ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(M.N_TREES))
def test_random_trees(hip, k):
    """the 200 trees of the CPU test: per node, and through the program when it is within SA_PROG_MAX nodes and SA_STACK_MAX
    operands (the synchronous operator otherwise) — the model's result either way, a division by zero included"""
    e, want, exp = M.tree_case(k)
    b = M.trees_batch()
    label = f"tree {k}: {e}"
    fast = program_accepts(e)
    with route(hip, exactly={"expr_binary": binary_nodes(e)}, still=("async_fast_batches",)):
        got = guarded(lambda: eval_column(hip, e, b).column(0))
    with route(hip, exactly={"async_fast_batches": 1 if fast else 0, "async_conj_batches": 0}, still=("expr_binary",) if fast else ()):
        prog = guarded(lambda: list(ProjectExecutor(hip, [e], [b], depth=1).execute())[0].column(0))
    if exp is M.DIV0:
        assert got is M.DIV0 and prog is M.DIV0, label
        return
    assert got is not M.DIV0 and prog is not M.DIV0, label
    M.assert_column_matches(got, exp, label)
    M.assert_column_matches(prog, exp, label + " (program)")
    if want == abi.BOOLEAN:
        with route(hip, exactly={"async_fast_batches": 1 if fast else 0, "async_conj_batches": int(fast and is_conjunction_shape(e))}):
            (out,) = list(FilterExecutor(hip, e, [b], depth=1).execute())
        M.assert_filter_matches(out, b, exp, label + " (filter_push_async)")


def test_program_limits(hip):
    """exactly SA_PROG_MAX nodes and exactly SA_STACK_MAX operands run in the kernel; one more of either falls back to the
    synchronous operator — and agrees"""
    b = M.trees_batch()
    a, c = InputRef(0), InputRef(2)

    def left_deep(m):  # 2 m - 1 nodes, stack 2
        e = a
        for i in range(m - 1):
            e = e + (a if i % 2 else Constant(M.POOL_I64[i % len(M.POOL_I64)], abi.INT64))
        return e

    def right_deep(m):  # stack m
        e = a
        for i in range(m - 1):
            e = BinaryOp("-" if i % 2 else "+", InputRef(1) if i % 2 else a, e)
        return e
    n24 = BinaryOp("+", left_deep(11), TypeCast(c, abi.INT64))  # 21 + 2 + 1 = 24 nodes
    n25 = left_deep(13)
    s8, s9 = right_deep(8), right_deep(9)
    assert M.program_shape(n24)[0] == SA_PROG_MAX and M.program_shape(n25)[0] == SA_PROG_MAX + 1
    assert M.program_shape(s8)[1] == SA_STACK_MAX and M.program_shape(s9)[1] == SA_STACK_MAX + 1
    p8, p9 = s8 > Constant(0, abi.INT64), s9 > Constant(0, abi.INT64)  # ... and as predicates (Filter)
    for label, e, fast in (("24 nodes", n24, True), ("25 nodes", n25, False), ("stack 8", s8, True), ("stack 9", s9, False),
                           ("stack 8, predicate", p8, True), ("stack 9, predicate", p9, False)):
        case = with_model([(label, e, b)])
        check_program(hip, case, fast=fast)
        check_per_node(hip, case)


# ---- the conjunction fast path ---------------------------------------------------------------------------------------------
CONJ_CONSTS = {
    abi.INT64: [M.I64_MIN, M.I64_MAX, M.I32_MIN, M.I32_MAX, 0],
    abi.INT32: [M.I32_MIN, M.I32_MAX, -1, -30000, 5],  # (negative constants: the sign extension of the constant's image)
    abi.FLOAT64: [M.f64_bits(0.0), M.f64_bits(-0.0), M.f64_bits(float("inf")), M.f64_bits(float("-inf")), M.NAN_POS, M.NAN_NEG,
                  M.NAN_NEG_PAYLOAD],
}
CONJ_COLS = {abi.INT64: 0, abi.INT32: 2, abi.FLOAT64: 4}


def conj_batch(n, nulls, seed=0):
    """tree_batch plus a Utf8 payload column with NULLs and empty strings (rid stays last)"""
    t = M.tree_batch(2000 + n + seed, n, nulls, pool_share=0.3)
    s = pa.array([None if (i % 7 == 3 and nulls) else ("" if i % 5 == 0 else "s" * (i % 11) + str(i)) for i in range(n)], type=pa.string())
    cols = [t.column(i) for i in range(6)] + [s, t.column(6)]
    return pa.RecordBatch.from_arrays(cols, names=["a", "b", "c", "d", "e", "f", "s", "rid"])


def term(dt, op, k, second=False):
    return BinaryOp(op, InputRef(CONJ_COLS[dt] + int(second)), M.pool_constant(dt, k))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097])
def test_conjunction_fast_path(hip, n):
    """1 to 4 terms of `col OP const`, all six operators, the extreme constants of every type, NULLs in the predicate and
    in the payload columns (Utf8 among them); `<` / `>=` against MIN and `>` / `<=` against MAX keep nothing or every valid
    row; 4097 rows take the synchronous operator"""
    fast = n <= SA_ROWS
    rng = np.random.default_rng(n)
    for nulls in (0.0, 0.5) if n > 65 else (0.0, 0.1, 0.5):
        b = conj_batch(n, nulls)
        preds = [(dt, op, k) for dt in M.NUMERIC.values() for op in M.CMP_OPS for k in CONJ_CONSTS[dt]]
        if n not in (1, 65, 1025, 4096):  # (the full single-term matrix at four sizes, a third of it elsewhere)
            preds = preds[n % 3::3]
        cases = [(f"{dt}: col {op} {k}", term(dt, op, k)) for dt, op, k in preds]
        for terms in (2, 3, 4, 2, 3, 4, 4, 4):
            picks = [preds[int(i)] for i in rng.integers(0, len(preds), terms)]
            e = None
            for j, (dt, op, k) in enumerate(picks):
                t = term(dt, op, k, second=bool(j % 2))
                e = t if e is None else (e & t)
            cases.append((" and ".join(f"{dt}: col {op} {k}" for dt, op, k in picks), e))
        for label, e in cases:
            assert is_conjunction_shape(e)
            exp = M.evaluate(e, b)
            with route(hip, exactly={"async_fast_batches": int(fast), "async_conj_batches": int(fast)}, still=("expr_binary",) if fast else ()):
                (out,) = list(FilterExecutor(hip, e, [b], depth=1).execute())
            M.assert_filter_matches(out, b, exp, f"n = {n}, nulls {nulls}: {label}")
        for dt, lo, hi in ((abi.INT64, M.I64_MIN, M.I64_MAX), (abi.INT32, M.I32_MIN, M.I32_MAX)):
            valid = b.num_rows - b.column(CONJ_COLS[dt]).null_count
            for op, k, expect in (("<", lo, 0), (">=", lo, valid), (">", hi, 0), ("<=", hi, valid)):
                with route(hip, exactly={"async_fast_batches": int(fast), "async_conj_batches": int(fast)}, still=("expr_binary",) if fast else ()):
                    (out,) = list(FilterExecutor(hip, term(dt, op, k), [b], depth=1).execute())
                assert out.num_rows == expect, (dt, op, k)


# ---- the fused `col OP const` filter ------------------------------------------------------------------------------------------
def unique_mask(make_expr, arr: pa.Array) -> np.ndarray:
    """kept rows of `make_expr(column)` as a boolean array: the model runs over the column's DISTINCT values (by bit pattern,
    NULL apart) and its verdicts are spread back — the predicate looks at one row at a time"""
    dt = abi.dtype_of(arr.type)
    n = len(arr)
    raw = np.frombuffer(arr.buffers()[1], dtype=np.uint64 if dt != abi.INT32 else np.uint32, count=n).astype(np.uint64)
    valid = np.asarray(arr.is_valid()) if arr.null_count else np.ones(n, dtype=bool)
    uniq, inv = np.unique(raw, return_inverse=True)
    vals = uniq.tolist() if dt == abi.FLOAT64 else [M.wrap(int(v), 32 if dt == abi.INT32 else 64) for v in uniq.tolist()]
    small = pa.RecordBatch.from_arrays([M.array_of(dt, vals)], names=["x"])
    res = M.evaluate(make_expr(InputRef(0)), small)
    assert all(s == M.EXACT for s in res.state)
    keep = np.array([v == 1 for v in res.vals], dtype=bool)[inv]
    return keep & valid


def raw_bits(arr: pa.Array):
    """(validity, value bit patterns) of a fixed-width column as numpy arrays"""
    n = len(arr)
    raw = np.frombuffer(arr.buffers()[1], dtype=np.uint32 if arr.type == pa.int32() else np.uint64, count=n, offset=arr.offset * (arr.type.bit_width // 8))
    valid = np.asarray(arr.is_valid()) if arr.null_count else np.ones(n, dtype=bool)
    return valid, raw


def assert_rows_taken(got: pa.Array, src: pa.Array, ids: np.ndarray, what):
    """`got` = rows `ids` of `src`, bit for bit: validity, and the value under every valid row"""
    assert got.type == src.type and len(got) == len(ids), what
    gv, gr = raw_bits(got)
    sv, sr = raw_bits(src)
    assert (gv == sv[ids]).all(), (what, "validity")
    assert (gr[gv] == sr[ids][gv]).all(), (what, "values")


def palette_column(rng, dt: int, n: int, nulls: float) -> pa.Array:
    """n rows drawn from 600 distinct values — the whole pool and ordinary values — so that the model, which runs over the
    DISTINCT values (unique_mask), costs the same at every size; every pool member occurs once n is a few thousand rows"""
    palette = M.column_values(M.edge_column(rng, dt, 600, 0.0, pool_share=0.1))
    vals = [palette[i] for i in rng.integers(0, len(palette), n).tolist()]
    if nulls:
        m = rng.random(n) < nulls
        vals = [None if m[i] else v for i, v in enumerate(vals)]
    return M.array_of(dt, vals)


@pytest.mark.parametrize("kind", list(M.NUMERIC))
@pytest.mark.parametrize("n", [1, 65, 4095, 4097] + list(TILE_SIZES))
def test_fused_filter(hip, n, kind):
    """sqlrs_filter_push of one `col OP const`: every constant of the conjunction cases (INT64 / INT32 MIN and MAX, +-0.0,
    +-inf, NaNs of both signs) under all six operators at the tile-straddling sizes, with and without NULLs in the predicate
    column; kept fractions 0 (`< MIN`), 1 (`>= MIN`) and about a half (`> 0`, `> +0.0`, `> -0.0`)"""
    dt = M.NUMERIC[kind]
    n = filter_rows(hip, n)
    rng = np.random.default_rng(n * 7 + dt)
    for nulls in (0.0, 0.3):
        x = palette_column(rng, dt, n, nulls)
        p = palette_column(rng, abi.FLOAT64, n, 0.2)
        b = pa.RecordBatch.from_arrays([x, p, pa.array(np.arange(n, dtype=np.int64))], names=["x", "p", "rid"])
        if n > 1000:
            assert (x.null_count > 0) == bool(nulls)
        fractions = []
        for k in CONJ_CONSTS[dt]:
            for op in M.CMP_OPS:
                keep = unique_mask(lambda c: BinaryOp(op, c, M.pool_constant(dt, k)), x)
                with route(hip, at_least={"filter_cmp_const": 1}, still=("expr_binary", "async_fast_batches")):
                    (out,) = list(FilterExecutor(hip, BinaryOp(op, InputRef(0), M.pool_constant(dt, k)), [b]).execute())
                what = f"{kind} n = {n} nulls {nulls}: x {op} {k}"
                ids = np.flatnonzero(keep)
                assert out.num_rows == len(ids) and (out.column(2).to_numpy() == ids).all(), what
                assert_rows_taken(out.column(0), x, ids, what)
                assert_rows_taken(out.column(1), p, ids, what)
                fractions.append(len(ids) / max(n - x.null_count, 1))
        if n > 1000:
            assert 0.0 in fractions and 1.0 in fractions and any(0.3 < f < 0.7 for f in fractions), fractions


# ---- RowFilter in the partition pass ---------------------------------------------------------------------------------------
PART_ROWS = 300_017


@pytest.mark.parametrize("kind", ["i64", "f64"])
@pytest.mark.parametrize("parts", [1, 8])
def test_hash_partition_filter_edge_constants(hip, parts, kind):
    """sqlrs_hash_partition_filter on its one-pass route: the kept rows of every partition as multisets, for the extreme
    constants over an int64 and a float64 predicate column — and the same rows as the fused filter keeps"""
    from sqlrs_amd import distributed as D
    dt = M.NUMERIC[kind]
    rng = np.random.default_rng(parts * 10 + dt)
    keys = rng.permutation(PART_ROWS).astype(np.int64) * 7919 - 10 ** 9  # distinct
    x = palette_column(rng, dt, PART_ROWS, 0.0)
    xbits = np.frombuffer(x.buffers()[1], dtype=np.uint64, count=PART_ROWS)
    b = pa.RecordBatch.from_arrays([pa.array(keys), x], names=["k", "x"])
    pid = D.partition_of(keys, parts)
    for k in CONJ_CONSTS[dt]:
        for op in M.CMP_OPS:
            what = f"{kind} parts = {parts}: x {op} {k}"
            keep = unique_mask(lambda c: BinaryOp(op, c, M.pool_constant(dt, k)), x)
            pred = BinaryOp(op, InputRef(1), M.pool_constant(dt, k))
            with route(hip, exactly={"hash_partition_filter": 1}, still=("expr_binary", "filter_cmp_const")):
                out, starts, rows = hip.hash_partition_filter(b, InputRef(0), pred, parts, abi.MEM_DEVICE)
            got = hip.to_host(out).to_arrow(["k", "x"])
            out.release()
            gk = got.column(0).to_numpy()
            gx = np.frombuffer(got.column(1).buffers()[1], dtype=np.uint64, count=got.num_rows)
            assert sum(rows) == int(keep.sum()), what
            for p in range(parts):
                lo, hi = starts[p], starts[p] + rows[p]
                sel = keep & (pid == p)
                assert rows[p] == int(sel.sum()), what
                o1, o2 = np.argsort(gk[lo:hi], kind="stable"), np.argsort(keys[sel], kind="stable")
                assert (gk[lo:hi][o1] == keys[sel][o2]).all(), what
                assert (gx[lo:hi][o1] == xbits[sel][o2]).all(), what
            if op in (">", "=") and parts == 8:  # cross-route: the fused filter keeps the same rows
                with route(hip, at_least={"filter_cmp_const": 1}):
                    (f,) = list(FilterExecutor(hip, pred, [b]).execute())
                assert (f.column(0).to_numpy() == keys[keep]).all(), what


# ---- all routes on the same input --------------------------------------------------------------------------------------------
REVERSED = {">": "<", "<": ">", ">=": "<=", "<=": ">=", "=": "=", "!=": "!="}


@pytest.mark.parametrize("kind", list(M.NUMERIC))
def test_routes_agree_on_col_op_const(hip, kind):
    """`col OP const` over one 4096-row batch: the per-node mask, the fused filter (synchronous push), the conjunction path
    (push_async) and the program (`const OP' col` and the mask as a projected column) keep the same rows — the model's"""
    dt = M.NUMERIC[kind]
    b = conj_batch(4096, 0.1, seed=5)
    ci = CONJ_COLS[dt]
    for k in CONJ_CONSTS[dt]:
        for op in M.CMP_OPS:
            what = f"{kind}: col {op} {k}"
            e = BinaryOp(op, InputRef(ci), M.pool_constant(dt, k))
            rev = BinaryOp(REVERSED[op], M.pool_constant(dt, k), InputRef(ci))
            exp = M.evaluate(e, b)
            model_ids = M.kept_rows(exp)
            with route(hip, exactly={"expr_binary": 1}, still=("filter_cmp_const", "async_fast_batches")):
                mask = eval_column(hip, e, b).column(0)
            node_ids = [i for i, v in enumerate(mask.to_pylist()) if v]
            with route(hip, at_least={"filter_cmp_const": 1}, still=("expr_binary", "async_fast_batches")):
                (fused,) = list(FilterExecutor(hip, e, [b]).execute())
            with route(hip, exactly={"async_fast_batches": 1, "async_conj_batches": 1}, still=("expr_binary", "filter_cmp_const")):
                (conj,) = list(FilterExecutor(hip, e, [b], depth=1).execute())
            with route(hip, exactly={"async_fast_batches": 1, "async_conj_batches": 0}, still=("expr_binary", "filter_cmp_const")):
                (prog,) = list(FilterExecutor(hip, rev, [b], depth=1).execute())
            with route(hip, exactly={"async_fast_batches": 1, "async_conj_batches": 0}, still=("expr_binary",)):
                (proj,) = list(ProjectExecutor(hip, [e], [b], depth=1).execute())
            proj_ids = [i for i, v in enumerate(proj.column(0).to_pylist()) if v]
            assert node_ids == model_ids, what
            assert fused.column(-1).to_pylist() == model_ids, what + " (fused filter)"
            assert conj.column(-1).to_pylist() == model_ids, what + " (conjunction)"
            assert prog.column(-1).to_pylist() == model_ids, what + " (program)"
            assert proj_ids == model_ids, what + " (projected mask)"
            M.assert_filter_matches(fused, b, exp, what + " (fused filter)")
            M.assert_filter_matches(conj, b, exp, what + " (conjunction)")
