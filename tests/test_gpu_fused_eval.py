"""The fused-evaluation route of the synchronous Filter / Project (SQLRS_EXPR_FUSED_EVAL of sqlrs_filter_create /
sqlrs_project_create; `fused_eval=True` on FilterExecutor / ProjectExecutor) against the independent edge-value model
(tests/expr_model.py) on the cases of tests/fused_eval_cases.py, and against the switch-off route on the same input.

Every comparison with the model is bit exact — values by bit pattern (-0.0, a NaN's sign and payload), validity, row order —
apart from the rows on which the model says the hardware chooses the NaN (ANY_NAN: "is a NaN"; LEFT_OUT: not compared; at most
2 % of a case, asserted on the model alone in test_fused_eval_cpu.py).  The switch-off output of the same input is compared
under the same rule.

Which route ran is asserted on every push: `fused_eval_filter_batches` rises by the pushes whose mask the program kernel wrote,
`fused_eval_project_columns` by the computed columns it wrote, with the per-node scopes `expr_binary` / `expr_cast` at rest — or
the counts rest and `expr_binary` moves by the binary nodes of the expressions.

The grid of the two kernels covers 2^21 rows per sweep (2048 workgroups x 1024 rows): the 4 194 381-row cases run three sweeps,
the last over 77 rows — one full 64-row group and a ragged one."""
import ctypes as C
import os
import subprocess
from contextlib import contextmanager

import numpy as np
import pyarrow as pa
import pytest

import expr_model as M
import fused_eval_cases as F
from sqlrs_amd import abi
from sqlrs_amd.executor import FilterExecutor, ProjectExecutor
from sqlrs_amd.expr import BinaryOp, Constant, InputRef, TypeCast

pytestmark = pytest.mark.gpu

FB, PC = "fused_eval_filter_batches", "fused_eval_project_columns"
PER_NODE = ("expr_binary", "expr_cast")
WIDTH = {abi.INT32: 4, abi.INT64: 8, abi.FLOAT64: 8}


# ---- which route ran ---------------------------------------------------------------------------------------------------------
def counters(be) -> dict:
    cap = 512
    names, ms, n_l = (C.c_char_p * cap)(), (C.c_double * cap)(), (C.c_int64 * cap)()
    n = be.fn("ctx_profile_read")(be.ctx, cap, names, ms, n_l)
    assert n <= cap
    return {names[k].decode(): n_l[k] for k in range(n)}


@contextmanager
def route(be, what="", exactly=None, at_least=None, still=()):
    """asserts how far the profile counters move across the block: `exactly` / `at_least` {name: by}, `still` names at rest"""
    before = counters(be)
    yield
    after = counters(be)
    moved = {k: after.get(k, 0) - before.get(k, 0) for k in set(after) | set(before)}
    for k, by in (exactly or {}).items():
        assert moved.get(k, 0) == by, (what, k, "moved by", moved.get(k, 0), "expected", by)
    for k, by in (at_least or {}).items():
        assert moved.get(k, 0) >= by, (what, k, "moved by", moved.get(k, 0), "expected at least", by)
    for k in still:
        assert moved.get(k, 0) == 0, (what, k, "moved by", moved.get(k, 0), "expected to rest")


@pytest.fixture(scope="module")
def hip():
    """a ctx of this module's own: its profile entries stay out of the session's shared ctx"""
    import sqlrs_amd
    be = sqlrs_amd.new_ctx(0)
    yield be
    be.close()


@pytest.fixture(autouse=True)
def profiled(hip):
    hip.profile(True)
    yield
    hip.profile(False)


# ---- input forms -------------------------------------------------------------------------------------------------------------
def lend(lb, first=0, rows=None, nulls=None):
    """a caller-built DEVICE batch over the buffers of the library batch `lb` (owner NULL): all of it, or its rows [first, first +
    rows) with `first` a multiple of 64 — values at that row, bitmaps (validity, Boolean values) advanced by whole words.
    `nulls`: the null_count to state per column that has a bitmap (-1: unknown)"""
    assert first % 64 == 0
    n = lb.num_rows if rows is None else rows
    cols = []
    for k in range(lb.num_columns):
        c = lb.column(k)
        assert c.mem == abi.MEM_DEVICE
        if c.dtype == abi.UTF8:
            assert first == 0 and n == lb.num_rows
            values = c.values
        elif c.dtype == abi.BOOLEAN:
            values = (c.values + first // 8) if c.values else c.values
        else:
            values = (c.values + WIDTH[c.dtype] * first) if c.values else c.values
        validity = (c.validity + first // 8) if c.validity else None
        cols.append(abi.Column(c.dtype, abi.MEM_DEVICE, n, (c.null_count if nulls is None else nulls[k]) if validity else 0, values, validity,
                               c.offsets if c.dtype == abi.UTF8 else None))
    return abi.RawBatch(cols, n, keepalive=lb)


def give(hip, b: pa.RecordBatch, form):
    """`b` as the operator's input: "host"; "device" (a caller-built DEVICE batch); "unknown" (the same with null_count -1 on
    every column that has a bitmap); "window" (128 other rows in front of the batch's, pointers advanced)"""
    if form == "host":
        return b
    if form == "device":
        return lend(hip.to_device(b))
    if form == "unknown":
        return lend(hip.to_device(b), nulls=[-1] * b.num_columns)
    front = b.take(pa.array(np.arange(128) % b.num_rows))
    whole = pa.Table.from_batches([front, b]).combine_chunks().to_batches()[0]
    return lend(hip.to_device(whole), 128, b.num_rows, [b.column(k).null_count for k in range(b.num_columns)])


# ---- running the operators -----------------------------------------------------------------------------------------------------
def guarded(fn):
    """fn() or M.DIV0 for the evaluators' Arrow error"""
    try:
        return fn()
    except abi.ExecutorError as err:
        assert err.status == abi.ERR_ARROW and M.DIV0 in err.message, err
        return M.DIV0


def project(hip, exprs, given, fused, out_mem=abi.MEM_HOST) -> pa.RecordBatch:
    (out,) = list(ProjectExecutor(hip, exprs, [given], out_mem=out_mem, fused_eval=fused).execute())
    if out_mem == abi.MEM_DEVICE:
        host = hip.to_host(out)
        out.release()
        out = host.to_arrow()
        host.release()
    return out


def filtered(hip, expr, given, fused, out_mem=abi.MEM_HOST, names=None) -> pa.RecordBatch:
    (out,) = list(FilterExecutor(hip, expr, [given], out_mem=out_mem, fused_eval=fused).execute())
    if out_mem == abi.MEM_DEVICE:
        host = hip.to_host(out)
        out.release()
        out = host.to_arrow(names)
        host.release()
    return out


def assert_same_column(on, off, res, what):
    """the switch-on and the switch-off column under the model's rule: bit for bit where the row is EXACT, "is a NaN" where it
    is ANY_NAN, not looked at where it is LEFT_OUT"""
    assert on.type == off.type and len(on) == len(off) == len(res), what
    a, b = M.column_values(on), M.column_values(off)
    bad = []
    for i, (x, y, s) in enumerate(zip(a, b, res.state)):
        if s == M.LEFT_OUT:
            continue
        ok = (x is not None and y is not None and M.is_nan_bits(x) and M.is_nan_bits(y)) if s == M.ANY_NAN else (x == y and (x is None) == (y is None))
        if not ok:
            bad.append((i, x, y, s))
    assert not bad, (what, "switch on / off differ (row, on, off, state)", bad[:8])


def check_project(hip, cases, batch, given, fused_expected=None, out_mem=abi.MEM_HOST):
    """cases [(label, expression, model Result or DIV0)] over `batch` (handed in as `given`) as ONE projection + rid, switch on and
    off; returns nothing.  `fused_expected`: whether the program kernel is to run (default: every expression compiles)"""
    dt = F.dtypes_of(batch)
    exprs = [e for _, e, _ in cases] + [InputRef(batch.num_columns - 1)]
    computed = sum(1 for e in exprs if F.is_computed(e))
    fused = all(F.compiles(e, dt) for e in exprs) if fused_expected is None else fused_expected
    nb = sum(F.binary_nodes(e) for e in exprs)
    what = cases[0][0]
    with route(hip, what, exactly={PC: computed if fused else 0, FB: 0}, still=PER_NODE if fused else ()):
        on = guarded(lambda: project(hip, exprs, given, True, out_mem))
    with route(hip, what + " (switch off)", exactly={PC: 0, FB: 0, "expr_binary": nb}):
        off = guarded(lambda: project(hip, exprs, given, False, out_mem))
    if any(res is M.DIV0 for _, _, res in cases):
        assert on is M.DIV0 and off is M.DIV0, what
        return
    assert on is not M.DIV0 and off is not M.DIV0, what
    for out in (on, off):
        assert out.num_rows == batch.num_rows and out.column(len(cases)).to_pylist() == list(range(batch.num_rows)), what
    for c, (label, _, res) in enumerate(cases):
        M.assert_column_matches(on.column(c), res, label + " (fused)")
        M.assert_column_matches(off.column(c), res, label + " (per node)")
        assert_same_column(on.column(c), off.column(c), res, label)


def check_filter(hip, label, e, res, batch, given, out_mem=abi.MEM_HOST):
    """the predicate `e` over `batch` (handed in as `given`, rid last), switch on and off"""
    dt = F.dtypes_of(batch)
    cmp_const = F.takes_cmp_const(e, dt)
    fused = F.compiles(e, dt) and not cmp_const
    names = list(batch.schema.names)
    with route(hip, label, exactly={FB: int(fused), PC: 0}, at_least={"filter_cmp_const": int(cmp_const)},
               still=PER_NODE if (fused or cmp_const) else ()):
        on = guarded(lambda: filtered(hip, e, given, True, out_mem, names))
    with route(hip, label + " (switch off)", exactly={FB: 0, PC: 0}, at_least={"filter_cmp_const": int(cmp_const)}):
        off = guarded(lambda: filtered(hip, e, given, False, out_mem, names))
    if res is M.DIV0:
        assert on is M.DIV0 and off is M.DIV0, label
        return
    assert on is not M.DIV0 and off is not M.DIV0, label
    M.assert_filter_matches(on, batch, res, label + " (fused)")
    M.assert_filter_matches(off, batch, res, label + " (per node)")
    unknown = {i for i, s in enumerate(res.state) if s == M.LEFT_OUT}
    assert [i for i in on.column(-1).to_pylist() if i not in unknown] == [i for i in off.column(-1).to_pylist() if i not in unknown], label


def check_both(hip, cases, batch, given=None, out_mem=abi.MEM_HOST):
    """cases [(label, expression, model outcome)]: as one projection (four computed columns a launch), and every Boolean one
    as a Filter"""
    given = batch if given is None else given
    good = [c for c in cases if c[2] is not M.DIV0]
    if good:
        check_project(hip, good, batch, given, out_mem=out_mem)
    for c in cases:
        if c[2] is M.DIV0:
            check_project(hip, [c], batch, given, out_mem=out_mem)
    for label, e, res in cases:
        boolean = res.dtype == abi.BOOLEAN if res is not M.DIV0 else e.nodes()[-1].op >= abi.EXPR_GT  # (a comparison, AND or OR on top)
        if boolean:
            check_filter(hip, label, e, res, batch, given, out_mem)


def with_model(cases):
    """[(label, expression, batch)] of ONE batch -> (batch, [(label, expression, model outcome)])"""
    batch = cases[0][2]
    assert all(b is batch for _, _, b in cases)
    return batch, [(label, e, M.model_outcome(e, b)) for label, e, b in cases]


# ---- 1. row counts, validity, input forms -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", F.FORMS + ["unknown"])
@pytest.mark.parametrize("n", F.ROW_COUNTS)
def test_row_counts_and_input_forms(hip, n, form):
    """1 .. 4097 rows: below, at and past a 64-row group, a 256-thread workgroup's first trip and its 1024 rows, four workgroups;
    columns without NULLs and with them; null_count -1 with a bitmap ("unknown")"""
    for nulls in (0.0, 0.1):
        if form == "unknown" and not nulls:
            continue
        batch, cases = F.row_count_case(n, nulls)
        assert all(res.left_out_fraction == 0 for _, _, res in cases)
        check_both(hip, cases, batch, give(hip, batch, form))


@pytest.mark.parametrize("out_mem", [abi.MEM_HOST, abi.MEM_DEVICE], ids=["out_host", "out_device"])
def test_out_mem(hip, out_mem):
    batch, cases = F.row_count_case(1025, 0.1)
    for form in ("host", "device"):
        check_both(hip, cases, batch, give(hip, batch, form), out_mem=out_mem)


# ---- 2. three sweeps of the grid: numpy is the model --------------------------------------------------------------------------------
def raw(col, np_type):
    if isinstance(col, pa.ChunkedArray):
        col = col.combine_chunks()
    valid = np.asarray(col.is_valid()) if col.null_count else np.ones(len(col), bool)
    if np_type is bool:
        return np.asarray(col.fill_null(False)), valid
    return np.frombuffer(col.buffers()[1], dtype=np_type, count=len(col), offset=col.offset * 8), valid


def test_two_full_sweeps_and_a_ragged_tail(hip):
    """2 * 2^21 + 77 rows, DEVICE input: the wrapping `i + j64 > k OR i2 < c` over nullable operands as a Filter and as a
    projected column next to `i * 3 - j64`, against numpy and against the switch-off output"""
    cols, batch = F.sweep_case()
    n = batch.num_rows
    assert n == 4_194_381
    given = lend(hip.to_device(batch))
    true, valid = F.sweep_predicate_numpy(cols)
    value, value_valid = F.sweep_value_numpy(cols)
    pred, val = F.sweep_predicate(), F.sweep_value()
    with route(hip, "sweep filter", exactly={FB: 1}, still=PER_NODE):
        on = filtered(hip, pred, given, True)
    with route(hip, "sweep filter (switch off)", exactly={FB: 0}, at_least={"expr_binary": 4}):
        off = filtered(hip, pred, given, False)
    kept = np.flatnonzero(true)
    for out in (on, off):
        assert out.num_rows == len(kept) and (raw(out.column(3), np.int64)[0] == kept).all()
    for c, name in enumerate(["i", "j64", "i2"]):
        v, ok = cols[name]
        ok = np.ones(n, bool) if ok is None else ok
        for out in (on, off):
            gv, gok = raw(out.column(c), np.int64)
            assert (gok == ok[kept]).all() and (gv[gok] == v[kept][gok]).all(), name
    exprs = [val, pred, InputRef(3)]
    with route(hip, "sweep project", exactly={PC: 2, "fused_eval_project": 1}, still=PER_NODE):
        on = project(hip, exprs, given, True)
    with route(hip, "sweep project (switch off)", exactly={PC: 0, "expr_binary": 6}):
        off = project(hip, exprs, given, False)
    for out in (on, off):
        gv, gok = raw(out.column(0), np.int64)
        assert (gok == value_valid).all() and (gv[gok] == value[gok]).all()
        gb, gok = raw(out.column(1), bool)
        assert (gok == valid).all() and (gb[gok] == true[gok]).all()
        assert (raw(out.column(2), np.int64)[0] == np.arange(n)).all()


# ---- 3. operator coverage ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(M.N_TREES))
def test_random_trees(hip, k):
    """the 200 trees of expr_model as a projected column and, the Boolean ones, as a Filter: fused when the forecast says the tree
    compiles (asserted by the counters), per node otherwise — the model's result either way, a division by zero included"""
    e, want, exp = M.tree_case(k)
    b = M.trees_batch()
    check_both(hip, [(f"tree {k}: {e}", e, exp)], b)


@pytest.mark.parametrize("form", ["colcol", "colconst"])
@pytest.mark.parametrize("op", M.ARITH_OPS + M.CMP_OPS)
@pytest.mark.parametrize("kind", list(M.NUMERIC))
def test_binary_operators_over_the_pool_cross_product(hip, kind, op, form):
    batch, cases = with_model([(f"{kind}: {l}", e, b) for l, e, b in M.binary_cases(M.NUMERIC[kind], op, form)])
    assert all(res is not M.DIV0 for _, _, res in cases)
    check_both(hip, cases, batch, give(hip, batch, "device"))


@pytest.mark.parametrize("dst", ["i32", "i64", "f64"])
@pytest.mark.parametrize("src", list(M.CAST_SOURCES))
def test_cast_lattice(hip, src, dst):
    """SAO_CAST from every source (a Boolean COLUMN among them: the loader reads its bit), column and constant operands"""
    s, d = M.CAST_SOURCES[src], M.NUMERIC[dst]
    b = M.cast_batch(s)
    pool = [False, True] if s == abi.BOOLEAN else M.POOLS[s]
    cases = [(f"cast {src} -> {dst}", TypeCast(InputRef(0), d), b), (f"cast {src} -> {dst} = cast", TypeCast(InputRef(0), d).eq(TypeCast(InputRef(0), d)), b)]
    cases += [(f"cast {src} constant {k} -> {dst}", TypeCast(Constant(k, s) if s == abi.BOOLEAN else M.pool_constant(s, k), d), b)
              for k in list(pool) + [None]]
    batch, cases = with_model(cases)
    for form in ("host", "window"):
        check_both(hip, cases, batch, give(hip, batch, form))


def test_the_double_that_is_int64_min_casts_to_int64_min(hip):
    vals = [-(2.0 ** 63), float(np.nextafter(-(2.0 ** 63), -np.inf)), float(np.nextafter(-(2.0 ** 63), 0.0)),
            float(np.nextafter(2.0 ** 63, 0.0)), 2.0 ** 63] * 20
    b = pa.RecordBatch.from_arrays([pa.array(vals, type=pa.float64()), pa.array(np.arange(len(vals)))], names=["x", "rid"])
    e = TypeCast(InputRef(0), abi.INT64)
    keep = e.eq(Constant(M.I64_MIN, abi.INT64))
    batch, cases = with_model([("f64 -> i64 around -2^63", e, b), ("cast = INT64_MIN", keep, b)])
    assert cases[0][2].vals[:5] == [-(2 ** 63), None, -(2 ** 63) + 1024, 2 ** 63 - 1024, None]
    check_both(hip, cases, batch)


def test_boolean_columns_as_operands_and_results(hip):
    b = M.bool_batch()
    batch, cases = with_model([(l, e, b) for l, e in F.bool_operand_cases()])
    for form in ("host", "device", "window"):
        check_both(hip, cases, batch, give(hip, batch, form))
    # the whole predicate is a Boolean column: `WHERE p` (a bare InputRef is no computed column, but it is a program for the Filter)
    res = M.evaluate(InputRef(0), b)
    check_filter(hip, "WHERE p", InputRef(0), res, b, b)


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
    batch, cases = with_model(cases)
    check_both(hip, cases, batch)


# ---- 4. division by zero ----------------------------------------------------------------------------------------------------------------
def test_divide_by_zero(hip):
    """a valid row with a zero divisor makes the push fail with the evaluator's text — whichever wave sees it; a NULL row over
    zero, a NULL dividend and a NULL constant divisor do not"""
    for label, e, b, raises in M.div0_cases():
        exp = M.model_outcome(e, b)
        assert (exp is M.DIV0) == raises, label
        with route(hip, label, exactly={PC: 1}, still=PER_NODE):
            prog = guarded(lambda: project(hip, [e], b, True).column(0))
        keep = e.eq(e)
        with route(hip, label, exactly={FB: 1}, still=PER_NODE):
            filt = guarded(lambda: filtered(hip, keep, b, True))
        if raises:
            assert prog is M.DIV0 and filt is M.DIV0, label
        else:
            M.assert_column_matches(prog, exp, label)
            assert filt is not M.DIV0 and filt.num_rows == sum(1 for v in exp.vals if v is not None), label


def test_rows_past_the_end_do_not_divide(hip):
    """a window of 70 rows whose array goes on with zero divisors: the 58 rows past `rows` in the last group are not evaluated"""
    n, tail = 70, 58 + 64
    x = pa.array([7] * (128 + n + tail), type=pa.int64())
    y = pa.array([1] * 128 + [3] * n + [0] * tail, type=pa.int64())
    whole = pa.RecordBatch.from_arrays([x, y, pa.array(np.arange(128 + n + tail) - 128)], names=["x", "y", "rid"])
    given = lend(hip.to_device(whole), 128, n)
    e = InputRef(0) / InputRef(1)
    with route(hip, "window", exactly={PC: 1}, still=PER_NODE):
        out = project(hip, [e, InputRef(2)], given, True)
    assert out.column(0).to_pylist() == [2] * n and out.column(1).to_pylist() == list(range(n))
    with route(hip, "window", exactly={FB: 1}, still=PER_NODE):
        out = filtered(hip, e.eq(Constant(2, abi.INT64)), given, True)
    assert out.num_rows == n


@pytest.mark.parametrize("op_kind", ["filter", "project"])
def test_the_operator_works_after_a_division_by_zero(hip, op_kind):
    good = pa.RecordBatch.from_arrays([pa.array([6, 8, -9] * 40), pa.array([3, -2, 1] * 40)], names=["x", "y"])
    bad = pa.RecordBatch.from_arrays([pa.array([6, 8, -9] * 40), pa.array([3, -2, 1] * 39 + [3, 0, 1])], names=["x", "y"])
    e = InputRef(0) / InputRef(1)
    h, keep = C.c_void_p(), []
    if op_kind == "filter":
        p = (e > Constant(-100, abi.INT64)).pack()
        p.abi.reserved = abi.EXPR_FUSED_EVAL
        keep.append(p)
        hip.check(hip.fn("filter_create")(hip.ctx, C.byref(p.abi), C.byref(h)))
    else:
        arr, k = abi.pack_exprs([e])
        arr[0].reserved = abi.EXPR_FUSED_EVAL
        keep += [arr, k]
        hip.check(hip.fn("project_create")(hip.ctx, 1, arr, C.byref(h)))
    try:
        status, outs = [], []
        with route(hip, op_kind, exactly={FB if op_kind == "filter" else PC: 3}, still=PER_NODE):
            for b in (good, bad, good):
                hb = abi.as_batch(b)
                keep.append(hb)
                out = C.POINTER(abi.Batch)()
                status.append(hip.fn(op_kind + "_push")(h, hb.ptr, abi.MEM_HOST, C.byref(out)))
                if status[-1] == abi.ERR_ARROW:
                    assert M.DIV0 in hip.fn("last_error")(hip.ctx).decode()
                outs.append(hip.wrap(out))
        assert status == [abi.OK, abi.ERR_ARROW, abi.OK] and outs[1] is None
        exp = M.evaluate(e, good)
        for o in (outs[0], outs[2]):
            got = o.to_arrow()
            o.release()
            assert got.num_rows == good.num_rows
            if op_kind == "project":
                M.assert_column_matches(got.column(0), exp)
    finally:
        hip.fn(op_kind + "_destroy")(h)


# ---- 5. program limits ----------------------------------------------------------------------------------------------------------------
def test_program_limits(hip):
    """exactly 24 nodes and exactly 8 operands in flight run fused; one more of either takes the per-node route — counts at rest,
    `expr_binary` moving (check_project / check_filter assert both from the forecast) — and agrees"""
    b = M.trees_batch()
    dt = F.dtypes_of(b)
    for label, (e, fused) in F.limit_exprs().items():
        assert F.compiles(e, dt) == fused, label
        check_both(hip, [(label, e, M.model_outcome(e, b))], b)


def test_five_computed_columns_take_two_launches(hip):
    batch, cases = F.row_count_case(257, 0.1)
    five = cases[:5]
    exprs = [e for _, e, _ in five] + [InputRef(batch.num_columns - 1)]
    with route(hip, "five columns", exactly={PC: 5, "fused_eval_project": 2}, still=PER_NODE):
        on = project(hip, exprs, batch, True)
    for c, (label, _, res) in enumerate(five):
        M.assert_column_matches(on.column(c), res, label)


def test_sixteen_columns_a_launch(hip):
    """four expressions over five fresh columns each: the fourth does not fit the 16 columns of the first launch and opens a second;
    over four fresh columns each they share one"""
    b = F.wide_batch(20)

    def sums(width, count):
        out = []
        for k in range(count):
            e = InputRef(width * k)
            for c in range(width * k + 1, width * (k + 1)):
                e = e + InputRef(c)
            out.append(e)
        return out
    for width, launches in ((4, 1), (5, 2)):
        exprs = sums(width, 4)
        with route(hip, f"{width} columns each", exactly={PC: 4, "fused_eval_project": launches}, still=PER_NODE):
            on = project(hip, exprs, b, True)
        for c, e in enumerate(exprs):
            M.assert_column_matches(on.column(c), M.evaluate(e, b), f"{width} columns each: {c}")


def test_a_utf8_operand_sends_the_whole_projection_per_node(hip):
    n = 300
    t = M.tree_batch(41, n, 0.1)
    s = pa.array([None if i % 7 == 3 else "s" * (i % 3) for i in range(n)], type=pa.string())
    b = pa.RecordBatch.from_arrays([t.column(i) for i in range(6)] + [s, t.column(6)], names=["a", "b", "c", "d", "e", "f", "s", "rid"])
    cases = [("a + b", InputRef(0) + InputRef(1)), ("s = 's'", InputRef(6).eq(Constant("s", abi.UTF8))), ("e < f", InputRef(4) < InputRef(5))]
    cases = [(l, e, M.evaluate(e, b)) for l, e in cases]
    assert not F.compiles(cases[1][1], F.dtypes_of(b))
    check_project(hip, cases, b, b, fused_expected=False)
    check_filter(hip, "s = 's' or e < f", cases[1][1] | cases[2][1], M.evaluate(cases[1][1] | cases[2][1], b), b, b)
    # ... while a Utf8 payload column next to compiled expressions does not matter
    check_project(hip, [cases[0], cases[2]], b, b, fused_expected=True)


# ---- 6. precedence: what was one pass before stays what it was -------------------------------------------------------------------------
def test_the_existing_one_pass_routes_come_first(hip):
    n = 70_000  # (the conjunction route starts at 2^16 rows)
    rng = np.random.default_rng(3)
    i = pa.array(rng.integers(0, 1000, n))
    g = pa.array(np.round(rng.normal(0, 100, n), 1))
    gn = pa.array(np.round(rng.normal(0, 100, n), 1), mask=rng.random(n) < 0.1)
    b = pa.RecordBatch.from_arrays([i, g, gn, pa.array(np.arange(n))], names=["i", "g", "gn", "rid"])
    given = lend(hip.to_device(b))

    def conj(gcol):
        return ((InputRef(0) >= Constant(100, abi.INT64)) & (InputRef(0) < Constant(600, abi.INT64))) & (InputRef(gcol) < Constant(10.0, abi.FLOAT64))
    iv, gv, gnv = i.to_numpy(), g.to_numpy(), gn.fill_null(1e9).to_numpy()
    with route(hip, "col > const", exactly={FB: 0}, at_least={"filter_cmp_const": 1}, still=PER_NODE):
        out = filtered(hip, InputRef(0) > Constant(500, abi.INT64), given, True)
    assert (raw(out.column(3), np.int64)[0] == np.flatnonzero(iv > 500)).all()
    with route(hip, "conjunction", exactly={FB: 0}, at_least={"filter_conj_mask": 1}, still=PER_NODE):
        out = filtered(hip, conj(1), given, True)
    assert (raw(out.column(3), np.int64)[0] == np.flatnonzero((iv >= 100) & (iv < 600) & (gv < 10.0))).all()
    with route(hip, "conjunction over a nullable column", exactly={FB: 1}, still=PER_NODE + ("filter_conj_mask",)):
        out = filtered(hip, conj(2), given, True)
    assert (raw(out.column(3), np.int64)[0] == np.flatnonzero((iv >= 100) & (iv < 600) & (gnv < 10.0))).all()
    with route(hip, "conjunction over a nullable column (switch off)", exactly={FB: 0}, at_least={"expr_binary": 5}):
        off = filtered(hip, conj(2), given, False)
    assert out.equals(off)


def test_a_bare_input_ref_still_shares_the_inputs_buffers(hip):
    batch, _ = F.row_count_case(1025, 0.1)
    lb = hip.to_device(batch)
    shared = {}
    for fused in (False, True):
        with route(hip, "bare refs", exactly={PC: 0, FB: 0}, still=PER_NODE):
            (out,) = list(ProjectExecutor(hip, [InputRef(0), InputRef(4)], [lb], out_mem=abi.MEM_DEVICE, fused_eval=fused).execute())
        shared[fused] = [out.column(k).values == lb.column(c).values for k, c in ((0, 0), (1, 4))]
        out.release()
    assert shared[True] == shared[False] == [True, True]
    # ... and next to a computed column too
    with route(hip, "bare ref + computed", exactly={PC: 1}, still=PER_NODE):
        (out,) = list(ProjectExecutor(hip, [InputRef(0), InputRef(0) + InputRef(1)], [lb], out_mem=abi.MEM_DEVICE, fused_eval=True).execute())
    assert out.column(0).values == lb.column(0).values
    out.release()
    lb.release()


# ---- 7. error parity ------------------------------------------------------------------------------------------------------------------
def failure(fn):
    try:
        fn()
    except abi.ExecutorError as err:
        return err.status, err.message
    return None


@pytest.mark.parametrize("name,expr", [
    ("int64 + int32", lambda: InputRef(0) + InputRef(2)),
    ("int64 < float64", lambda: InputRef(0) < InputRef(4)),
    ("int64 and int64", lambda: BinaryOp("and", InputRef(0), InputRef(1))),
    ("cast to boolean", lambda: TypeCast(InputRef(0), abi.BOOLEAN)),
    ("cast to utf8, compared", lambda: TypeCast(InputRef(0), abi.UTF8).eq(Constant("1", abi.UTF8))),
])
def test_errors_are_those_of_the_per_node_route(hip, name, expr):
    """mixed operand types and unsupported casts do not compile: the per-node evaluator raises, the same status and message with
    the switch on and off — also when a compiled expression stands in front"""
    b = M.tree_batch(43, 200, 0.1)
    e = expr()
    for exprs in ([e], [InputRef(0) + InputRef(1), e]):
        off = failure(lambda: project(hip, exprs, b, False))
        with route(hip, name, exactly={PC: 0}):
            on = failure(lambda: project(hip, exprs, b, True))
        assert off is not None and on == off, (name, on, off)
    off = failure(lambda: filtered(hip, e, b, False))
    with route(hip, name, exactly={FB: 0}):
        on = failure(lambda: filtered(hip, e, b, True))
    assert off is not None and on == off, (name, on, off)


# ---- 8. payload columns: compaction is unchanged -------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_mem", [abi.MEM_HOST, abi.MEM_DEVICE], ids=["out_host", "out_device"])
@pytest.mark.parametrize("form", ["host", "device"])
def test_utf8_and_boolean_payload_columns(hip, form, out_mem):
    n = 4097
    t = M.tree_batch(47, n, 0.1, pool_share=0.3)
    s = pa.array([None if i % 7 == 3 else ("" if i % 5 == 0 else "s" * (i % 11) + str(i)) for i in range(n)], type=pa.string())
    p = pa.array([None if i % 11 == 5 else bool((i * 7) % 3 == 0) for i in range(n)], type=pa.bool_())
    b = pa.RecordBatch.from_arrays([t.column(i) for i in range(6)] + [s, p, t.column(6)], names=["a", "b", "c", "d", "e", "f", "s", "p", "rid"])
    for label, e in (("(a > b) or (e < f)", (InputRef(0) > InputRef(1)) | (InputRef(4) < InputRef(5))),
                     ("p and c < d", InputRef(7) & (InputRef(2) < InputRef(3)))):
        check_filter(hip, label, e, M.evaluate(e, b), b, give(hip, b, form), out_mem)


# ---- 9. the C++ mirror ----------------------------------------------------------------------------------------------------------------
def test_cpp_builder_with_and_without_fused_eval():
    """host/fused_eval_check.cpp: Project(Filter(scan)) through ExecutorBuilder over 200 003 rows in 1024-row batches, with and
    without `fused_eval`: equal text, and the counts say which route ran"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "host", "fused_eval_check")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(root, "host"), "-s", "fused_eval_check"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
