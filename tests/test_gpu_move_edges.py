"""Row movement and the operators made of nothing else on the device, against the independent model (tests/move_model.py) on the
cases of tests/move_edge_cases.py: take, bit-gather, Utf8 take, concat, copy, scalar broadcast, the all-NULL column and the
compaction of every payload type; upload, materialize, emit, sqlrs_batch_copy and the Arrow C Data Interface; Limit, CrossJoin,
Project's pass-through and constant columns, SimpleAgg and sqlrs_batch_to_string.  HOST, library-owned, lent and windowed DEVICE
input, HOST and DEVICE output.  Every comparison is exact (move_model.compare: the Arrow buffers bit for bit, never to_pylist).

Which route ran is asserted over the scopes of sqlrs_ctx_profile_read ("The row-movement contract"):

  concat through the cross join   `concat` + the column count (several parts); `gather` + both sides' column counts per probe
  concat through ORDER BY         `concat` + at least the column count
  Limit                           `gather` + the column count per batch that is cut; a batch returned whole leaves it at rest
  CrossJoin                       `concat` + the left column count once (several left batches; one batch: at rest); `gather` + both
                                  sides' column counts per call that has left rows
  Project                         pass-through and constant columns: `gather`, `concat`, `compact` at rest
  Filter (synchronous route)      some rows kept: `compact` + the fixed-width columns, `compact_iota` and `gather` + the Utf8 columns;
                                  none kept: `gather` + the Utf8 columns (a take of no rows), the other two at rest; all kept: all
                                  three at rest (the input is handed on); `filter_cmp_const`, `async_fast_batches` always at rest
  Arrow C import / export         no scope moves; the Limit behind it as above"""
import ctypes as C
from contextlib import contextmanager

import pyarrow as pa
import pytest

import move_edge_cases as E
import move_model as M
from order_plan import read_counters as counters
from sqlrs_amd import abi
from sqlrs_amd.executor import CrossJoinExecutor, FilterExecutor, OrderExecutor, ProjectExecutor, SimpleAggExecutor
from sqlrs_amd.expr import InputRef, OrderBy

pytestmark = pytest.mark.gpu
NCOLS = len(E.COLS)
WIDTH = {M.I32: 4, M.I64: 8, M.F64: 8}


@contextmanager
def route(be, label, exactly=None, at_least=None, still=()):
    """asserts how far the profile counters move across the block: `exactly` / `at_least` {name: by}, `still` names at rest"""
    before = counters(be)
    yield
    after = counters(be)
    moved = {k: after.get(k, 0) - before.get(k, 0) for k in set(after) | set(before)}
    for k, by in (exactly or {}).items():
        assert moved.get(k, 0) == by, (label, k, "moved by", moved.get(k, 0), "expected", by)
    for k, by in (at_least or {}).items():
        assert moved.get(k, 0) >= by, (label, k, "moved by", moved.get(k, 0), "expected at least", by)
    for k in still:
        assert moved.get(k, 0) == 0, (label, k, "moved by", moved.get(k, 0), "expected to rest")


@pytest.fixture(autouse=True)
def profiled(hip):
    hip.profile(True)
    yield
    hip.profile(False)


# ---- input forms --------------------------------------------------------------------------------------------------------------------
def lend(lb, first=0, rows=None, nulls=None):
    """a caller-built DEVICE batch over the descriptors of the library batch `lb` (owner NULL, `lb` kept alive): the whole batch, or
    its rows [first, first + rows) with `first` a multiple of 64 — fixed-width and bitmap pointers advanced, Utf8 `offsets` advanced
    with `values` unchanged (offsets[0] > 0); `nulls`: the window's NULL count per column"""
    assert first % 64 == 0
    n = lb.num_rows if rows is None else rows
    cols = []
    for i in range(lb.num_columns):
        c = lb.column(i)
        assert c.mem == abi.MEM_DEVICE
        values, validity, offsets = c.values, c.validity, c.offsets
        if first:
            if validity:
                validity += first // 8
            if c.dtype == M.UTF8:
                offsets += 4 * first
            elif c.dtype == M.BOOL:
                values += first // 8
            else:
                values += WIDTH[c.dtype] * first
        nc = c.null_count if nulls is None else (nulls[i] if validity else 0)
        cols.append(abi.Column(c.dtype, abi.MEM_DEVICE, n, nc, values, validity, offsets))
    return abi.RawBatch(cols, n, keepalive=lb)


def give(hip, batch, mode, form, seed=0, names=E.COLS):
    """the model batch in its input form -> what an operator takes (release() it unless it is a pyarrow batch)"""
    if form == "host":
        return E.arrow_of(batch, mode, names)
    if form == "window":
        assert len(batch) == NCOLS
        lb = hip.to_device(E.arrow_of(E.with_margins(seed, batch), mode, names))
        return lend(lb, E.WINDOW_LEAD, M.rows(batch), [c.nulls for c in batch])
    lb = hip.to_device(E.arrow_of(batch, mode, names))
    return lb if form == "owned" else lend(lb)


def release(x):
    if not isinstance(x, pa.RecordBatch):
        x.release()


def pointers(x):
    cols = x.cols if isinstance(x, abi.RawBatch) else [x.column(i) for i in range(x.num_columns)]
    return {p for c in cols for p in (c.values, c.validity, c.offsets) if p}


# ---- outputs ------------------------------------------------------------------------------------------------------------------------
def host_arrow(lb) -> pa.RecordBatch:
    """a HOST library batch as pyarrow arrays over copies of its buffers, with the null_count the library STATES"""
    arrays = []
    for i in range(lb.num_columns):
        c = lb.column(i)
        assert c.mem == abi.MEM_HOST and c.length == lb.num_rows
        n, nb = c.length, (c.length + 7) // 8
        assert c.validity or c.null_count == 0, (i, "null_count", c.null_count, "without a validity buffer")
        validity = pa.py_buffer(C.string_at(c.validity, nb)) if c.validity else None
        t = abi.pa_type(c.dtype)
        if c.dtype == M.UTF8:
            offs = C.string_at(c.offsets, 4 * (n + 1))
            end = int.from_bytes(offs[-4:], "little", signed=True)
            bufs = [validity, pa.py_buffer(offs), pa.py_buffer(C.string_at(c.values, end) if end > 0 else b"")]
        elif c.dtype == M.BOOL:
            bufs = [validity, pa.py_buffer(C.string_at(c.values, nb))]
        else:
            bufs = [validity, pa.py_buffer(C.string_at(c.values, WIDTH[c.dtype] * n))]
        arrays.append(pa.Array.from_buffers(t, n, bufs, null_count=c.null_count))
    return pa.RecordBatch.from_arrays(arrays, names=[f"c{i}" for i in range(len(arrays))])


def fetch(hip, out, out_mem=None) -> pa.RecordBatch:
    """an operator's output as pyarrow: a pyarrow batch as it is; a library batch through host_arrow (a DEVICE one copied first)"""
    if isinstance(out, pa.RecordBatch):
        return out
    if out_mem is not None:
        assert all(out.column(i).mem == out_mem for i in range(out.num_columns))
    if out.num_columns and out.column(0).mem == abi.MEM_DEVICE:
        h = hip.to_host(out)
        out.release()
        out = h
    got = host_arrow(out)
    out.release()
    return got


# ---- a. concat ------------------------------------------------------------------------------------------------------------------------
def cross_join_concat(hip, parts, right, out_mem):
    h = C.c_void_p()
    hip.check(hip.fn("cross_join_create")(hip.ctx, C.byref(h)))
    try:
        for p in parts:
            b = abi.as_batch(p)
            hip.check(hip.fn("cross_join_build_push")(h, b.ptr))
        rb = abi.as_batch(right)
        out = C.POINTER(abi.Batch)()
        hip.check(hip.fn("cross_join_probe_push")(h, rb.ptr, out_mem, C.byref(out)))
        return hip.wrap(out)
    finally:
        hip.fn("cross_join_destroy")(h)


@pytest.mark.parametrize("name", E.names(family="a", via="cross"))
def test_concat_through_the_cross_join(hip, name):
    """the parts pushed into the cross join's build side and probed with ONE right row: the left columns are the concatenation"""
    c = E.case(name)
    parts = [give(hip, p, c.part_mode(k), c.form, c.seed * 40 + k) for k, p in enumerate(c.parts)]
    one = E.palette(77, 1, "none")
    for out_mem in (abi.MEM_HOST, abi.MEM_DEVICE):
        with route(hip, name, exactly={"concat": NCOLS, "gather": 2 * NCOLS}):
            out = cross_join_concat(hip, parts, E.arrow_of(one, "none"), out_mem)
        got = fetch(hip, out, out_mem)
        M.compare(got.columns[:NCOLS], c.expected, name)
        M.compare(got.columns[NCOLS:], [M.broadcast(col.dtype, col.cells[0], M.rows(c.expected)) for col in one], name + ": right side")
    for p in parts:
        release(p)


@pytest.mark.parametrize("name", E.names(family="a", via="order"))
def test_concat_through_an_identity_order(hip, name):
    """ORDER BY the row id over the parts: the input is already in order, so the output is the concatenation"""
    c = E.case(name)
    parts = [give(hip, p, c.part_mode(k), c.form, c.seed * 40 + k) for k, p in enumerate(c.parts)]
    for out_mem in (abi.MEM_HOST, abi.MEM_DEVICE):
        with route(hip, name, at_least={"concat": NCOLS}):
            (out,) = list(OrderExecutor(hip, [OrderBy(InputRef(NCOLS - 1))], parts, out_mem=out_mem).execute())
        M.compare(fetch(hip, out), c.expected, name)
    for p in parts:
        release(p)


# ---- b. slice -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.names(family="b"))
def test_limit_slices(hip, name):
    c = E.case(name)
    outs, pulled = c.expected
    cuts = sum(1 for o in outs if not any(o is b for b in c.batches))
    for out_mem in (abi.MEM_HOST, abi.MEM_DEVICE):
        child = [give(hip, b, c.batch_mode(k), c.form, k) for k, b in enumerate(c.batches)]
        with route(hip, name, exactly={"gather": NCOLS * cuts}, still=("concat", "compact")):
            got, got_pulled = E.limit_run(hip, child, c.limit, c.offset, out_mem)
        M.compare_limit([fetch(hip, g) for g in got], got_pulled, c.expected, name)
        for b in child:
            release(b)


# ---- c. product -----------------------------------------------------------------------------------------------------------------------
def product_calls(c):
    """probe calls that reach the gathers: restated from CrossJoinExecutor.execute (ranges of left rows per right batch)"""
    L = sum(E.LEFT_SPLIT[c.L])
    calls = 0
    for rb in c.right:
        r = M.rows(rb)
        per_call = max(1, c.max_rows_per_call // max(r, 1))
        calls += 0 if L == 0 else 1 if r == 0 else len(range(0, L, per_call))
    return calls


@pytest.mark.parametrize("name", E.names(family="c"))
def test_cross_join_product(hip, name):
    c = E.case(name)
    left = [E.arrow_of(b) for b in c.left]
    right = [E.arrow_of(b) for b in c.right]
    with route(hip, name, exactly={"concat": NCOLS, "gather": 2 * NCOLS * product_calls(c)}):
        got = list(CrossJoinExecutor(hip, left, right, E.product_schema(), max_rows_per_call=c.max_rows_per_call).execute())
    M.compare_stream(got, c.expected, name)


def test_cross_join_single_left_batch_leaves_concat_at_rest(hip):
    left, right = E.palette(5, 65, "n10"), E.palette(6, 3, "n10")
    lb = hip.to_device(E.arrow_of(left))
    with route(hip, "one left batch", exactly={"gather": 2 * NCOLS}, still=("concat",)):
        got = list(CrossJoinExecutor(hip, [lb], [E.arrow_of(right)], E.product_schema()).execute())
    lb.release()
    M.compare_stream(got, M.cross_join_stream([left], [right]), "one left batch")


# ---- d. pass-through and constants ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.names(family="d"))
def test_project_pass_through_and_constants(hip, name):
    c = E.case(name)
    for out_mem in (abi.MEM_HOST, abi.MEM_DEVICE):
        src = give(hip, c.batch, c.mode, c.form, c.rows)
        lent = pointers(src) if c.form in ("lent", "window") else set()
        with route(hip, name, still=("gather", "concat", "compact", "compact_iota")):
            (out,) = list(ProjectExecutor(hip, c.exprs, [src], out_mem=out_mem).execute())
        if out_mem == abi.MEM_DEVICE:
            if c.form == "owned":        # the header promises shared, reference-counted buffers: the input goes first
                src.release()
            assert not (pointers(out) & lent), (name, "the DEVICE result aliases the caller's buffers")
        M.compare(fetch(hip, out), c.expected, name)
        release(src)


# ---- e. compaction ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.names(family="e"))
def test_filter_compacts_every_payload_type(hip, name):
    c = E.case(name)
    kept = M.rows(c.expected)
    some = 0 < kept < c.rows
    fixed = sum(1 for col in c.batch if col.dtype in WIDTH)
    utf8 = sum(1 for col in c.batch if col.dtype == M.UTF8)
    plan = dict(exactly={"compact": fixed if some else 0, "compact_iota": utf8 if some else 0, "gather": utf8 if kept < c.rows else 0},
                still=("filter_cmp_const", "async_fast_batches", "concat"))
    names = ("mask",) + E.COLS
    for out_mem in (abi.MEM_HOST, abi.MEM_DEVICE):
        src = give(hip, c.batch, "n10", c.form, names=names)
        with route(hip, name, **plan):
            (out,) = list(FilterExecutor(hip, InputRef(0), [src], out_mem=out_mem).execute())
        release(src)
        M.compare(fetch(hip, out), c.expected, name)


# ---- f. one group -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.names(family="f"))
def test_simple_agg_one_group(hip, name):
    c = E.case(name)
    if c.shape == "nobatch":
        with pytest.raises(abi.ExecutorError) as e:
            list(SimpleAggExecutor(hip, E.agg_funcs(), []).execute())
        assert e.value.status == abi.ERR_INTERNAL
        return
    for out_mem in (abi.MEM_HOST, abi.MEM_DEVICE):
        child = [give(hip, b, c.mode, c.form, names=E.AGG_COLS) for b in c.batches]
        with route(hip, name, still=("filter_cmp_const",) + (("concat",) if len(child) == 1 else ())):   # (several batches: HashAgg's input is concatenated)
            (out,) = list(SimpleAggExecutor(hip, E.agg_funcs(), child, out_mem=out_mem).execute())
        M.compare(fetch(hip, out), c.expected, name)
        for b in child:
            release(b)


# ---- g. text form -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.names(family="g"))
def test_text_form(hip, name):
    c = E.case(name)
    rb = E.arrow_of(c.batch)
    M.compare_text(hip.batch_to_string(rb), c.expected, name + ": HOST")
    lb = hip.to_device(rb)
    M.compare_text(hip.batch_to_string(lb), c.expected, name + ": DEVICE")
    lent = lend(lb)
    M.compare_text(hip.batch_to_string(lent), c.expected, name + ": lent")
    lent.release()


# ---- h. Arrow C Data Interface --------------------------------------------------------------------------------------------------------
class Imported:
    """a pyarrow array (a RecordBatch or a StructArray) exported, optionally edited, and imported by the library"""

    def __init__(self, hip, obj, edit=None):
        self.hip = hip
        arr, sch = abi.ArrowArrayC(), abi.ArrowSchemaC()
        obj._export_to_c(C.addressof(arr), C.addressof(sch))
        if edit:
            edit(arr)
        out = C.POINTER(abi.Batch)()
        st = hip.fn("batch_import_arrow")(hip.ctx, C.byref(arr), C.byref(sch), C.byref(out))
        if st != abi.OK:
            pa.Array._import_from_c(C.addressof(arr), C.addressof(sch))      # (nothing was consumed: give pyarrow's exports back)
            hip.check(st)
        assert not arr.release and not sch.release
        self.p = out

    ptr = property(lambda self: self.p)
    num_rows = property(lambda self: self.p.contents.num_rows)

    def export(self) -> pa.RecordBatch:
        """the batch MOVED into exported structures and imported by pyarrow (zero copy for a HOST batch of the library's)"""
        return export(self.hip, self)


def export(hip, lb) -> pa.RecordBatch:
    arr, sch = abi.ArrowArrayC(), abi.ArrowSchemaC()
    p, lb.p = lb.p, None
    hip.check(hip.fn("batch_export_arrow")(hip.ctx, p, None, C.byref(arr), C.byref(sch)))
    return pa.RecordBatch._import_from_c(C.addressof(arr), C.addressof(sch))


def unknown_null_counts(arr):
    for i in range(arr.n_children):
        arr.children[i].contents.null_count = -1


@pytest.mark.parametrize("name", E.names(family="h"))
def test_arrow_c_import_and_export(hip, name):
    c = E.case(name)
    base = E.arrow_of(c.base, c.base_mode)
    first, rows = c.window

    def imported():
        if c.kind == "struct_slice":
            return Imported(hip, pa.StructArray.from_arrays(base.columns, names=base.schema.names).slice(first, rows))
        return Imported(hip, base.slice(first, rows), unknown_null_counts if c.kind == "null_count_unknown" else None)
    with route(hip, name, still=("gather", "concat", "compact")):
        M.compare(imported().export(), c.expected, name + ": straight back")                  # HOST, zero copy
        src = imported()
        dev = hip.to_device(src)
        hip.fn("batch_release")(src.p)
        M.compare(export(hip, dev), c.expected, name + ": through the device")
    # one Limit that cuts it: rows [1, 1 + m) of the imported batch
    m = max(rows - 2, 0)
    exp = M.limit_stream([c.expected], m, 1)
    src = imported()
    with route(hip, name, exactly={"gather": NCOLS if exp[0] else 0}):
        got, pulled = E.limit_run(hip, [src], m, 1, abi.MEM_DEVICE)
    hip.fn("batch_release")(src.p)
    M.compare_limit([export(hip, g) for g in got], pulled, exp, name + ": behind a Limit")
