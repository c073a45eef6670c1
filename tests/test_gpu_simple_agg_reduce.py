"""SimpleAgg's reduce route (SQLRS_SIMPLE_AGG_REDUCE / SQLRS_SIMPLE_AGG_FILTER of sqlrs_simple_agg_create, witness
`simple_reduce_batches`) against the independent model
(tests/agg_model.py over the rows expr_model keeps) on the cases of tests/simple_reduce_cases.py.

Keys, validity, COUNT, integer SUM and MIN / MAX (f64 included) are compared bit for bit, SUM(f64) inside the model's any-order
bound — never by class: test_simple_agg_reduce_cpu.py asserts that no case has a classed group.  Which route ran is asserted:
`reduced_batches` equals the pushes and the scopes `agg_update` / `lds_agg` and every agg_* counter stay at rest, or — switch
off, or a shape the route does not admit — `reduced_batches` is 0 and the table is the one the switch-off operator returns.

The grid of sr_reduce_kernel covers at most 2^21 rows per sweep (2048 workgroups x 1024 rows): the 4 194 381-row cases run three
sweeps, the last over 77 rows — one full 64-row group and a ragged one."""
import ctypes as C
from contextlib import contextmanager

import numpy as np
import pyarrow as pa
import pytest

import agg_edge_cases as E
import simple_reduce_cases as S
from sqlrs_amd import abi
from sqlrs_amd.executor import SimpleAggExecutor
from sqlrs_amd.expr import AggFunc, Constant, InputRef

pytestmark = pytest.mark.gpu

SUM_F = [("sum", "f")]
WIDTH = {abi.INT32: 4, abi.INT64: 8, abi.FLOAT64: 8}


# ---- which route ran ---------------------------------------------------------------------------------------------------------
def counters(be) -> dict:
    cap = 512
    names, ms, n_l = (C.c_char_p * cap)(), (C.c_double * cap)(), (C.c_int64 * cap)()
    n = be.fn("ctx_profile_read")(be.ctx, cap, names, ms, n_l)
    assert n <= cap
    return {names[k].decode(): n_l[k] for k in range(n)}


@contextmanager
def route(be, label, reduced):
    """`reduced` pushes through the reduce route and the aggregate routes at rest — or, reduced = 0, the row route moving"""
    before = counters(be)
    yield
    after = counters(be)
    moved = {k: after.get(k, 0) - before.get(k, 0) for k in set(after) | set(before)}
    seen = {k: v for k, v in moved.items() if v}
    assert moved.get("simple_reduce_batches", 0) == reduced, (label, seen)
    if reduced:
        at_rest = [k for k in moved if k.startswith("agg_") or k == "lds_agg"]
        assert all(moved[k] == 0 for k in at_rest), (label, seen)
    else:
        assert moved.get("agg_update", 0) > 0 and moved.get("simple_reduce", 0) == 0, (label, seen)


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
    rows) with `first` a multiple of 64 — values and validity pointers advanced"""
    assert first % 64 == 0
    n = lb.num_rows if rows is None else rows
    cols = []
    for k in range(lb.num_columns):
        c = lb.column(k)
        assert c.mem == abi.MEM_DEVICE
        values = (c.values + WIDTH[c.dtype] * first) if c.values else c.values
        validity = (c.validity + first // 8) if c.validity else None
        cols.append(abi.Column(c.dtype, abi.MEM_DEVICE, n, (c.null_count if nulls is None else nulls[k]) if validity else 0, values, validity, None))
    return abi.RawBatch(cols, n, keepalive=lb)


def give(hip, batches, form):
    out = []
    for b in batches:
        if form == "host":
            out.append(b)
        elif form == "device" or b.num_rows == 0:
            out.append(lend(hip.to_device(b)))
        else:  # a window: 128 other rows in front of the batch's
            front = b.take(pa.array(np.arange(128) % b.num_rows))
            whole = pa.Table.from_batches([front, b]).combine_chunks().to_batches()[0]
            out.append(lend(hip.to_device(whole), 128, b.num_rows, [b.column(k).null_count for k in range(b.num_columns)]))
    return out


def run(hip, batches, aggs, label, reduce=True, child_filter=None, reduced=None):
    """the operator's one row; `reduced`: pushes expected on the reduce route (default: all when `reduce`)"""
    reduced = (len(batches) if reduce else 0) if reduced is None else reduced
    ex = SimpleAggExecutor(hip, aggs, batches, reduce=reduce, child_filter=child_filter)
    with route(hip, label, reduced):
        (out,) = list(ex.execute())
    assert ex.reduced_batches == reduced, (label, ex.reduced_batches)
    return out


# ---- 1. sizes, batching, validity, input forms ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("funcs", [E.ALL_FUNCS, SUM_F], ids=["all_funcs", "sum_f"])
@pytest.mark.parametrize("form", ["host", "device", "window"])
@pytest.mark.parametrize("name", S.SMALL)
def test_reduce_route(hip, name, form, funcs):
    c = S.case(name)
    out = run(hip, give(hip, S.with_empty(c.batches()), form), E.agg_funcs(funcs), f"{name} {form}")
    assert S.compare_one_row(out, c.model(funcs), funcs, f"{name} {form}") == 0


@pytest.mark.parametrize("name", S.LARGE)
def test_reduce_route_three_sweeps(hip, name):
    c = S.case(name)
    given = give(hip, S.with_empty(c.batches()), "device")
    for funcs in (E.ALL_FUNCS, SUM_F):
        out = run(hip, given, E.agg_funcs(funcs), name)
        assert S.compare_one_row(out, c.model(funcs), funcs, name) == 0


# ---- 2. the switch off ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.SMALL)
def test_switch_off(hip, name):
    c = S.case(name)
    out = run(hip, S.with_empty(c.batches()), E.agg_funcs(E.ALL_FUNCS), name, reduce=False)
    S.compare_one_row(out, c.model(E.ALL_FUNCS), E.ALL_FUNCS, name)


# ---- 3. filters and computed arguments --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("fname,cname,nans", S.FILTER_CASES)
def test_filter_fused(hip, fname, cname, nans, form):
    c, expr, mask = S.filter_case(fname, cname, nans)
    kept = S.kept_of(mask)
    label = f"{fname} {cname} {form}"
    given = give(hip, S.with_empty(c.batches()), form)
    out = run(hip, given, E.agg_funcs(E.ALL_FUNCS), label, child_filter=expr)
    assert S.compare_one_row(out, S.kept_model(c, kept, E.ALL_FUNCS), E.ALL_FUNCS, label) == 0
    if fname == "range_and_g":  # sum(f * g), sum(i + j) (wrapping), count(f) under i >= c1 AND i < c2 AND g < c3
        out = run(hip, given, S.computed_aggs(), label + " computed", child_filter=expr)
        assert S.compare_one_row(out, S.kept_model(c, kept, S.COMPUTED_FUNCS, S.computed_args(c)), S.COMPUTED_FUNCS, label) == 0


@pytest.mark.parametrize("fname,cname,nans", [k for k in S.FILTER_CASES if k[1].startswith("n4097")])
def test_filter_with_the_switch_off(hip, fname, cname, nans):
    """the filter entry without the reduce route: handed to the inner operator"""
    c, expr, mask = S.filter_case(fname, cname, nans)
    ex = SimpleAggExecutor(hip, E.agg_funcs(E.ALL_FUNCS), S.with_empty(c.batches()), child_filter=expr)
    (out,) = list(ex.execute())
    assert ex.reduced_batches == 0
    S.compare_one_row(out, S.kept_model(c, S.kept_of(mask), E.ALL_FUNCS), E.ALL_FUNCS, f"{fname} {cname} off")


# ---- 4. divide by zero --------------------------------------------------------------------------------------------------------------
G_BELOW = 0.5


def _div0_case(where):
    """n4097_random with j = 0 in a kept valid row ("kept"), or only in rows the filter g < 0.5 drops and in rows whose j is NULL"""
    c = S.case("n4097_random")
    g, gv = c.cols["g"]
    jv = c.cols["j"][1]
    kept = (g < G_BELOW) & gv
    if where == "kept":
        rows = np.nonzero(kept & jv & c.cols["i"][1])[0][7:8]
    else:
        rows = np.concatenate([np.nonzero(~kept)[0][::5], np.nonzero(~jv)[0][::3]])
    assert len(rows)
    return S.with_zero_divisors(c, rows), kept


@pytest.mark.parametrize("reduce", [True, False], ids=["on", "off"])
def test_divide_by_zero_on_a_kept_row(hip, reduce):
    c, _ = _div0_case("kept")
    ex = SimpleAggExecutor(hip, S.quotient_aggs(), c.batches(), reduce=reduce, child_filter=InputRef(S.G) < Constant(G_BELOW, abi.FLOAT64))
    with pytest.raises(abi.ExecutorError) as e:
        list(ex.execute())
    assert (e.value.status, e.value.message) == (abi.ERR_ARROW, "Divide by zero error")


@pytest.mark.parametrize("reduce", [True, False], ids=["on", "off"])
def test_zero_divisors_in_dropped_and_null_rows(hip, reduce):
    c, kept = _div0_case("dropped")
    ex = SimpleAggExecutor(hip, S.quotient_aggs(), c.batches(), reduce=reduce, child_filter=InputRef(S.G) < Constant(G_BELOW, abi.FLOAT64))
    (out,) = list(ex.execute())
    assert ex.reduced_batches == (len(c.batches()) if reduce else 0)
    S.compare_one_row(out, S.kept_model(c, kept, S.QUOTIENT_FUNCS, S.quotient_arg(c, kept)), S.QUOTIENT_FUNCS, f"reduce {reduce}")


# ---- 5. shapes the route does not admit ----------------------------------------------------------------------------------------------
def _with_more_columns(c):
    """[k, f, g, i, j, s (utf8), b (boolean)]"""
    out = []
    for b in c.batches():
        n = b.num_rows
        s = pa.array([None if r % 11 == 0 else f"s{(r * 7919) % 1000:04d}" for r in range(n)], type=pa.string())
        flag = pa.array([None if r % 13 == 0 else r % 3 != 0 for r in range(n)], type=pa.bool_())
        out.append(pa.RecordBatch.from_arrays(list(b.columns) + [s, flag], names=list(b.schema.names) + ["s", "b"]))
    return out


# (aggregates whose value does not depend on the order of the additions: the switch-off operator sums doubles with atomics, and two
#  runs of IT differ in the last bits)
EXACT_FUNCS = [("sum", "i"), ("min", "f"), ("max", "g"), ("count", "j")]
FALLBACKS = {
    "distinct": (lambda: [AggFunc("count", InputRef(S.I), abi.INT64, distinct=True)] + E.agg_funcs(EXACT_FUNCS), None),
    "min_utf8": (lambda: [AggFunc("min", InputRef(5), abi.UTF8)] + E.agg_funcs(EXACT_FUNCS), None),
    "boolean_in_filter": (lambda: E.agg_funcs(EXACT_FUNCS), lambda: InputRef(6) & (InputRef(S.G) < Constant(0.5, abi.FLOAT64))),
    "five_arguments": (lambda: E.agg_funcs(EXACT_FUNCS) + [AggFunc("count", InputRef(S.F) + InputRef(S.G), abi.INT64)], None),
}


@pytest.mark.parametrize("shape", list(FALLBACKS))
def test_fallback_is_the_switch_off(hip, shape):
    aggs, flt = FALLBACKS[shape]
    batches = _with_more_columns(S.case("n4097_random"))
    tables = []
    for reduce in (True, False):
        ex = SimpleAggExecutor(hip, aggs(), batches, reduce=reduce, child_filter=flt() if flt else None)
        (out,) = list(ex.execute())
        assert ex.reduced_batches == 0, shape
        tables.append(out)
    assert tables[0].schema.types == tables[1].schema.types
    for a, b in zip(tables[0].columns, tables[1].columns):
        assert a.is_valid().to_pylist() == b.is_valid().to_pylist(), shape
        if a.type == pa.float64():  # (bit for bit)
            assert a.buffers()[1].to_pybytes() == b.buffers()[1].to_pybytes(), shape
        else:
            assert a.to_pylist() == b.to_pylist(), shape


# ---- 6. the same bits twice -----------------------------------------------------------------------------------------------------------
def test_sum_f64_is_reproducible(hip):
    c = S.case("n100003_random")
    given = give(hip, c.batches(), "device")
    aggs = E.agg_funcs(E.ALL_FUNCS)
    first, second = (run(hip, given, aggs, "twice") for _ in range(2))
    for a, b in zip(first.columns, second.columns):
        assert a.buffers()[1].to_pybytes() == b.buffers()[1].to_pybytes()


# ---- 7. what the operator holds ---------------------------------------------------------------------------------------------------------
def _entries(aggs, keep, reduce=False, child_filter=None):
    """the entries of sqlrs_simple_agg_create: the aggregates, SQLRS_SIMPLE_AGG_REDUCE on the first, the WHERE as a last one"""
    funcs = [a.abi_struct(keep) for a in aggs]
    if child_filter is not None:
        pf = child_filter.pack()
        keep.append(pf)
        funcs.append(abi.AggFunc(0, 0, 0, abi.SIMPLE_AGG_FILTER, pf.abi))
    if reduce and funcs:
        funcs[0].reserved |= abi.SIMPLE_AGG_REDUCE
    return (abi.AggFunc * max(len(funcs), 1))(*funcs), len(funcs)


def _create(hip, aggs, keep, reduce=False, child_filter=None):
    arr, n = _entries(aggs, keep, reduce, child_filter)
    h = C.c_void_p()
    hip.check(hip.fn("simple_agg_create")(hip.ctx, n, arr, C.byref(h)))
    return h


def test_a_stream_costs_a_few_cells(hip):
    rng = np.random.default_rng(7)
    rows, pushes = 1 << 20, 16
    data = [rng.standard_normal(rows) for _ in range(pushes)]
    lent = [lend(hip.to_device(pa.RecordBatch.from_arrays([pa.array(d)], names=["x"]))) for d in data]
    keep = []
    h = _create(hip, [AggFunc("sum", InputRef(0), abi.FLOAT64), AggFunc("count", InputRef(0), abi.INT64)], keep, reduce=True)
    try:
        hip.synchronize()
        hip.fn("ctx_pool_trim")(hip.ctx)
        before, reduced = hip.fn("ctx_pool_bytes")(hip.ctx), counters(hip).get("simple_reduce_batches", 0)
        for b in lent:
            hip.check(hip.fn("simple_agg_push")(h, b.ptr))
        hip.synchronize()
        hip.fn("ctx_pool_trim")(hip.ctx)
        held = hip.fn("ctx_pool_bytes")(hip.ctx) - before
        assert counters(hip).get("simple_reduce_batches", 0) - reduced == pushes
        assert held <= 1 << 20, held  # (state cells, one partial record per workgroup, the plan — of 128 MiB pushed)
        out = C.POINTER(abi.Batch)()
        hip.check(hip.fn("simple_agg_finish")(h, abi.MEM_HOST, C.byref(out)))
        got = hip.wrap(out).to_arrow()
    finally:
        hip.fn("simple_agg_destroy")(h)
    assert got.column(1).to_pylist() == [rows * pushes] and got.column(0).null_count == 0


# ---- 8. the flags of the create call, through the C ABI ------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduce", [True, False], ids=["on", "off"])
def test_flags_of_the_create_call(hip, reduce):
    """both flags as a native caller sets them; the filter entry adds no output column"""
    c, expr, mask = S.filter_case("i_gt_c", "n4097_random", False)
    batches = c.batches()
    keep = []
    h = _create(hip, E.agg_funcs(E.ALL_FUNCS), keep, reduce=reduce, child_filter=expr)
    before = counters(hip).get("simple_reduce_batches", 0)
    try:
        held = [abi.as_batch(b) for b in batches]  # (alive until finish, as a caller's batches are)
        for hb in held:
            hip.check(hip.fn("simple_agg_push")(h, hb.ptr))
        out = C.POINTER(abi.Batch)()
        hip.check(hip.fn("simple_agg_finish")(h, abi.MEM_HOST, C.byref(out)))
        got = hip.wrap(out).to_arrow()
    finally:
        hip.fn("simple_agg_destroy")(h)
    assert counters(hip).get("simple_reduce_batches", 0) - before == (len(batches) if reduce else 0)
    S.compare_one_row(got, S.kept_model(c, S.kept_of(mask), E.ALL_FUNCS), E.ALL_FUNCS, f"reduce {reduce}")


def test_a_filter_entry_alone_is_refused(hip):
    keep = []
    arr, n = _entries([], keep, child_filter=InputRef(S.I) > Constant(0, abi.INT64))
    h = C.c_void_p()
    assert n == 1 and hip.fn("simple_agg_create")(hip.ctx, n, arr, C.byref(h)) == abi.ERR_INTERNAL


@pytest.mark.parametrize("reduce", [True, False], ids=["on", "off"])
def test_a_referenced_column_changes_its_type(hip, reduce):
    """the second batch holds int64 where the first held float64: the inner operator's status (by finish at the latest), the reduce
    route's at the push"""
    first = pa.RecordBatch.from_arrays([pa.array(np.arange(100, dtype=np.float64))], names=["x"])
    second = pa.RecordBatch.from_arrays([pa.array(np.arange(100, dtype=np.int64))], names=["x"])
    ex = SimpleAggExecutor(hip, [AggFunc("sum", InputRef(0), abi.FLOAT64), AggFunc("min", InputRef(0), abi.FLOAT64)], [first, second], reduce=reduce)
    with pytest.raises(abi.ExecutorError) as e:
        list(ex.execute())
    assert (e.value.status, e.value.message) == (abi.ERR_ARROW, "concat_batches: schema mismatch")


def test_finish_without_a_batch(hip):
    keep = []
    h = _create(hip, E.agg_funcs(SUM_F), keep, reduce=True)
    try:
        out = C.POINTER(abi.Batch)()
        assert hip.fn("simple_agg_finish")(h, abi.MEM_HOST, C.byref(out)) == abi.ERR_INTERNAL
    finally:
        hip.fn("simple_agg_destroy")(h)


def test_cpp_builder_with_and_without_simple_agg_reduce():
    """host/simple_agg_reduce_check.cpp: SimpleAgg(Filter(scan)) through ExecutorBuilder, with and without `simple_agg_reduce`, equal
    one-row results on an integer-exact table"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "host", "simple_agg_reduce_check")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(root, "host"), "-s", "simple_agg_reduce_check"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout


def test_device_output(hip):
    c = S.case("n4097_random")
    ex = SimpleAggExecutor(hip, E.agg_funcs(E.ALL_FUNCS), c.batches(), out_mem=abi.MEM_DEVICE, reduce=True)
    (dev,) = list(ex.execute())
    host = hip.to_host(dev)
    S.compare_one_row(host.to_arrow(), c.model(E.ALL_FUNCS), E.ALL_FUNCS, "device output")
