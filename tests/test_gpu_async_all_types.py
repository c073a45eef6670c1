"""sqlrs_filter_set_async_all_types / sqlrs_project_set_async_all_types on the GPU: Utf8 and Boolean operands inside the
one-launch kernels of push_async.  Which route ran is asserted from the counters of sqlrs_ctx_profile_read
(`async_fast_batches` against the rule restated in tests/async_types_cases.py, `expr_binary` / `expr_cast` at rest for the
batches the kernel took); what came out is compared with the model of tests/expr_model.py (nothing left out for these
types), with the synchronous hip stream and with the oracle."""
import ctypes as C
from contextlib import contextmanager

import numpy as np
import pyarrow as pa
import pytest

import async_types_cases as K
import expr_model as M
from async_utf8_cases import str_array
from sqlrs_amd import abi
from sqlrs_amd.executor import FilterExecutor, ProjectExecutor
from sqlrs_amd.expr import BinaryOp, Constant, InputRef, TypeCast

pytestmark = pytest.mark.gpu


def counters(be) -> dict:
    cap = 512
    names, ms, n_l = (C.c_char_p * cap)(), (C.c_double * cap)(), (C.c_int64 * cap)()
    n = be.fn("ctx_profile_read")(be.ctx, cap, names, ms, n_l)
    assert n <= cap
    return {names[k].decode(): n_l[k] for k in range(n)}


@contextmanager
def route(be, fast, per_node_at_most=0):
    """`async_fast_batches` moves by exactly `fast`; the per-node evaluator (expr_binary + expr_cast) by at most
    `per_node_at_most` launches (0: at rest — what the batches the kernel took must leave it at)"""
    before = counters(be)
    yield
    after = counters(be)
    moved = {k: after.get(k, 0) - before.get(k, 0) for k in set(after) | set(before)}
    assert moved.get("async_fast_batches", 0) == fast, ("async_fast_batches moved by", moved.get("async_fast_batches", 0), "predicted", fast)
    per_node = moved.get("expr_binary", 0) + moved.get("expr_cast", 0)
    assert per_node <= per_node_at_most, ("expr_binary + expr_cast moved by", per_node, "at most", per_node_at_most)


@pytest.fixture(autouse=True)
def profiled(hip):
    hip.profile(True)
    yield
    hip.profile(False)


def nodes_above_leaves(e) -> int:
    return sum(1 for n in e.nodes() if n.op not in (abi.EXPR_INPUT_REF, abi.EXPR_CONSTANT))


_sync = {}


def sync_and_oracle(hip, oracle, key, make):
    """the synchronous hip stream and the oracle's, computed once per case"""
    if key not in _sync:
        _sync[key] = (list(make(hip).execute()), list(make(oracle).execute()))
    return _sync[key]


# ---- stream parity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.stream_predicates()))
@pytest.mark.parametrize("depth", [1, 8])
def test_filter_stream(hip, oracle, name, depth):
    bs, e = K.stream(), K.stream_predicates()[name]
    predicted = K.count_eligible(e, bs)
    assert predicted == len(bs) - 2
    with route(hip, predicted, per_node_at_most=nodes_above_leaves(e) * (len(bs) - predicted)):
        got = list(FilterExecutor(hip, e, bs, depth=depth, async_all_types=True).execute())
    K.assert_filter_stream(got, bs, K.stream_model(name), name, K.RID)
    sync, orc = sync_and_oracle(hip, oracle, ("filter", name), lambda be: FilterExecutor(be, e, bs))
    K.same_batches(got, sync, name + " against push")
    K.same_batches(got, orc, name + " against the oracle")
    with route(hip, K.count_eligible(e, bs, on=False), per_node_at_most=10 ** 9):  # switch off: every batch carries Boolean columns
        off = list(FilterExecutor(hip, e, bs, depth=depth).execute())
    K.same_batches(off, got, name + " switch off")


@pytest.mark.parametrize("depth", [1, 8])
def test_project_stream(hip, oracle, depth):
    bs, ex = K.stream(), K.stream_projection()
    predicted = K.count_eligible(ex, bs)
    assert predicted == len(bs) - 2
    per_node = sum(nodes_above_leaves(e) for e in ex)
    with route(hip, predicted, per_node_at_most=per_node * (len(bs) - predicted)):
        got = list(ProjectExecutor(hip, ex, bs, depth=depth, async_all_types=True).execute())
    K.assert_project_stream(got, bs, ex, K.stream_projection_model(), "projection")
    sync, orc = sync_and_oracle(hip, oracle, ("project",), lambda be: ProjectExecutor(be, ex, bs))
    K.same_batches(got, sync, "against push")
    K.same_batches(got, orc, "against the oracle")
    with route(hip, 0, per_node_at_most=10 ** 9):
        off = list(ProjectExecutor(hip, ex, bs, depth=depth).execute())
    K.same_batches(off, got, "switch off")


# ---- cross products ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["utf8", "bool"])
def test_cross_products_through_filter_and_project(hip, kind):
    """72 / 100 rows (more than one 64-bit word), every pair of pool values and NULL, six comparisons (and AND / OR), the
    forms column-column, column-constant, constant-column; each expression is ONE fast batch through either operator"""
    batch, cases = (M.utf8_batch(), K.utf8_cross_cases()) if kind == "utf8" else (M.bool_batch(), K.bool_cross_cases())
    assert batch.num_rows > 64
    for label, e in cases:
        res = M.evaluate(e, batch)
        with route(hip, 1):
            (got,) = list(FilterExecutor(hip, e, [batch], depth=1, async_all_types=True).execute())
        assert M.assert_filter_matches(got, batch, res, label + " (filter)") == 0
        ex = [e, InputRef(0), InputRef(1), InputRef(2)]
        with route(hip, 1):
            (got,) = list(ProjectExecutor(hip, ex, [batch], depth=1, async_all_types=True).execute())
        assert M.assert_column_matches(got.column(0), res, label + " (project)") == 0
        for c in range(3):
            assert M.column_values(got.column(c + 1)) == M.column_values(batch.column(c)), (label, c)


# ---- layout edges -----------------------------------------------------------------------------------------------------
def test_sliced_utf8_input(hip, oracle):
    """offsets[0] != 0 on either operand (the bytes of a slice start inside the parent's buffer): data_base matters"""
    rng = np.random.default_rng(7)
    rows = 300
    vals = [K.VOCAB[i] for i in rng.integers(0, len(K.VOCAB), rows)]
    other = [K.VOCAB[i] for i in rng.integers(0, len(K.VOCAB), rows)]
    b = pa.RecordBatch.from_arrays([str_array(vals, rng.random(rows) < 0.2, shift=11), str_array(other, None, shift=5),
                                    pa.array(rng.random(rows) < 0.5, mask=rng.random(rows) < 0.2), pa.array(np.arange(rows, dtype=np.int64))],
                                   names=["s", "t", "p", "rid"])
    for label, e in (("s < t", InputRef(0) < InputRef(1)), ("s = 'ab'", InputRef(0).eq(Constant("ab", abi.UTF8))), ("t >= s or p", (InputRef(1) >= InputRef(0)) | InputRef(2))):
        res = M.evaluate(e, b)
        with route(hip, 1):
            (got,) = list(FilterExecutor(hip, e, [b], depth=1, async_all_types=True).execute())
        assert M.assert_filter_matches(got, b, res, label) == 0
        K.same_batches([got], list(FilterExecutor(oracle, e, [b]).execute()), label)
        with route(hip, 1):
            (got,) = list(ProjectExecutor(hip, [e, InputRef(0), InputRef(1)], [b], depth=1, async_all_types=True).execute())
        assert M.assert_column_matches(got.column(0), res, label) == 0
        assert M.column_values(got.column(1)) == M.column_values(b.column(0)) and M.column_values(got.column(2)) == M.column_values(b.column(1))


def test_adjacent_utf8_columns_without_nulls(hip, oracle):
    """sa_filter_kernel, 65 and 1025 rows: two Utf8 payload columns side by side, neither with a NULL (tests/async_types_cases.py,
    adjacent_utf8_stream: the route from one Utf8 column to the next without a bitmap pass between them), narrow and wide kernel"""
    bs = K.adjacent_utf8_stream()
    assert all(c.null_count == 0 for b in bs for c in b.columns) and [b.num_rows for b in bs] == [65, 1025]
    for label, e in (("rid % 3", (InputRef(2) - (InputRef(2) / Constant(3, abi.INT64)) * Constant(3, abi.INT64)) > Constant(0, abi.INT64)), ("s >= t", InputRef(0) >= InputRef(1))):
        with route(hip, len(bs)):
            got = list(FilterExecutor(hip, e, bs, depth=1, async_all_types=True).execute())
        assert all(0 < g.num_rows < b.num_rows for g, b in zip(got, bs)), label
        sync, orc = sync_and_oracle(hip, oracle, ("adjacent", label), lambda be: FilterExecutor(be, e, bs))
        K.same_batches(got, sync, label + " against push")
        K.same_batches(got, orc, label + " against the oracle")


def test_all_rows_kept(hip):
    """4096 rows kept whole with Boolean and Utf8 payload: the last word of the compacted bitmaps and the end offset"""
    rng = np.random.default_rng(9)
    b = K.stream_batch(rng, 4096, nulls=0.1)
    p_true = pa.array(np.ones(4096, dtype=bool))
    b = b.set_column(K.P, "p", p_true)
    for label, e in (("p", InputRef(K.P)), ("p = p", InputRef(K.P).eq(InputRef(K.P))), ("rid >= 0", InputRef(K.RID) >= Constant(0, abi.INT64))):
        with route(hip, 1):
            (got,) = list(FilterExecutor(hip, e, [b], depth=1, async_all_types=True).execute())
        assert got.num_rows == 4096
        K.same_batches([got], [b], label)
    # ... and all but the rows of the last word's upper half
    e = InputRef(K.RID) < Constant(4096 - 37, abi.INT64)
    with route(hip, 1):
        (got,) = list(FilterExecutor(hip, e, [b], depth=1, async_all_types=True).execute())
    K.same_batches([got], [b.slice(0, 4096 - 37)], "all but 37")


def test_constant_pool(hip, oracle):
    """1024 bytes of Utf8 constants are a fast batch, 1025 the synchronous operator; two equal constants work"""
    b = K.stream()[0]
    s, t = InputRef(K.S), InputRef(K.T)
    u = lambda v: Constant(v, abi.UTF8)  # noqa: E731
    big = K.LONG + "a"  # (a value of the columns: the comparison has something to equal)
    pad = "x" * (1024 - 2 * len(big.encode()))
    cases = [("1024 bytes", (s.eq(u(big)) | t.eq(u(big))) | s.eq(u(pad)), 1),
             ("1025 bytes", (s.eq(u(big)) | t.eq(u(big))) | s.eq(u(pad + "x")), 0),
             ("one constant of 1024", s.ne(u("x" * 1024)), 1), ("one constant of 1025", s.ne(u("x" * 1025)), 0),
             ("two equal constants", s.eq(u("ab")) | t.eq(u("ab")), 1),
             ("empty and NULL constants", s.eq(u("")) | t.eq(u(None)), 1)]
    for label, e, fast in cases:
        assert K.filter_eligible(e, b) == bool(fast), label
        with route(hip, fast, per_node_at_most=0 if fast else 10 ** 9):
            (got,) = list(FilterExecutor(hip, e, [b], depth=1, async_all_types=True).execute())
        assert M.assert_filter_matches(got, b, M.evaluate(e, b), label, rid=K.RID) == 0
        K.same_batches([got], list(FilterExecutor(oracle, e, [b]).execute()), label)
        with route(hip, fast, per_node_at_most=0 if fast else 10 ** 9):
            (got,) = list(ProjectExecutor(hip, [e, s], [b], depth=1, async_all_types=True).execute())
        assert M.assert_column_matches(got.column(0), M.evaluate(e, b), label) == 0


def outcome(fn):
    try:
        return ("ok", fn())
    except abi.ExecutorError as err:
        return ("error", err.status, err.message)


def test_expressions_that_do_not_compile_stay_synchronous(hip):
    """a Utf8-versus-Int64 comparison, a Utf8 cast, a lone Utf8 constant as a projection: the synchronous operator's error
    or result, and no fast batch"""
    b = K.stream()[0]
    s, a = InputRef(K.S), InputRef(K.A)
    for label, e in (("s = a", s.eq(a)), ("cast(s as bigint) > a", TypeCast(s, abi.INT64) > a), ("s", s)):
        assert not K.filter_eligible(e, b)
        exp = outcome(lambda: list(FilterExecutor(hip, e, [b]).execute()))
        with route(hip, 0, per_node_at_most=10 ** 9):
            got = outcome(lambda: list(FilterExecutor(hip, e, [b], depth=1, async_all_types=True).execute()))
        assert got[0] == exp[0], (label, got, exp)
        if got[0] == "ok":
            K.same_batches(got[1], exp[1], label)
        else:
            assert got[1:] == exp[1:], label
    for label, ex in (("'k'", [Constant("k", abi.UTF8), s]), ("s = a", [s.eq(a)])):
        assert not K.project_eligible(ex, b)
        exp = outcome(lambda: list(ProjectExecutor(hip, ex, [b]).execute()))
        with route(hip, 0, per_node_at_most=10 ** 9):
            got = outcome(lambda: list(ProjectExecutor(hip, ex, [b], depth=1, async_all_types=True).execute()))
        assert got[0] == exp[0], (label, got, exp)
        if got[0] == "ok":
            K.same_batches(got[1], exp[1], label)
        else:
            assert got[1:] == exp[1:], label


def test_divide_by_zero_arrives_at_the_wait_of_its_ticket(hip):
    """a wide program that divides by zero in one valid row of the second batch: the first batch comes out, the error is the
    evaluator's, and both batches were fast ones"""
    rng = np.random.default_rng(13)
    good, bad = K.stream_batch(rng, 200, nulls=0.0), K.stream_batch(rng, 200, nulls=0.0)
    good = good.set_column(K.A, "a", pa.array(np.full(200, 2, dtype=np.int64)))
    d = np.full(200, 2, dtype=np.int64)
    d[131] = 0
    bad = bad.set_column(K.A, "a", pa.array(d))
    e = ((Constant(8, abi.INT64) / InputRef(K.A)) > Constant(3, abi.INT64)) & (InputRef(K.S).ne(Constant("zz", abi.UTF8)) | InputRef(K.P))
    assert K.filter_eligible(e, bad)
    seen = []
    with route(hip, 2):
        with pytest.raises(abi.ExecutorError) as err:
            for out in FilterExecutor(hip, e, [good, bad], depth=1, async_all_types=True).execute():
                seen.append(out)
    assert err.value.status == abi.ERR_ARROW and M.DIV0 in err.value.message
    assert len(seen) == 1
    assert M.assert_filter_matches(seen[0], good, M.evaluate(e, good), "the batch in front of the error", rid=K.RID) == 0


# ---- the setters ------------------------------------------------------------------------------------------------------
def test_setters_refuse_a_null_handle(hip):
    assert hip.fn("filter_set_async_all_types")(None, 1) == abi.ERR_INTERNAL
    assert hip.fn("project_set_async_all_types")(None, 1) == abi.ERR_INTERNAL


def _push_wait(hip, push, h, batch, names=None):
    b = abi.as_batch(batch)
    t = C.c_void_p()
    hip.check(hip.fn(push)(h, b.ptr, C.byref(t)))
    out = C.POINTER(abi.Batch)()
    hip.check(hip.fn("batch_wait")(t, C.byref(out)))
    lb = hip.wrap(out)
    try:
        return lb.to_arrow(names or list(batch.schema.names))
    finally:
        lb.release()


def test_toggling_mid_stream_changes_the_route_and_never_the_batch(hip):
    b = K.stream()[1]
    e = K.stream_predicates()["s_gt_t_or_p"]
    exp = M.evaluate(e, b)
    packed = e.pack()
    h = C.c_void_p()
    hip.check(hip.fn("filter_create")(hip.ctx, C.byref(packed.abi), C.byref(h)))
    try:
        for on, fast in ((None, 0), (1, 1), (1, 1), (0, 0), (7, 1), (0, 0)):  # (any non-zero value is "on")
            if on is not None:
                assert hip.fn("filter_set_async_all_types")(h, on) == abi.OK
            with route(hip, fast, per_node_at_most=0 if fast else 10 ** 9):
                got = _push_wait(hip, "filter_push_async", h, b)
            assert M.assert_filter_matches(got, b, exp, f"on = {on}", rid=K.RID) == 0
    finally:
        hip.fn("filter_destroy")(h)
    ex = [e, InputRef(K.S)]
    arr, keep = abi.pack_exprs(ex)
    hip.check(hip.fn("project_create")(hip.ctx, len(ex), arr, C.byref(h)))
    try:
        for on, fast in ((None, 0), (1, 1), (0, 0), (1, 1)):
            if on is not None:
                assert hip.fn("project_set_async_all_types")(h, on) == abi.OK
            with route(hip, fast, per_node_at_most=0 if fast else 10 ** 9):
                got = _push_wait(hip, "project_push_async", h, b, ["mask", "s"])
            assert M.assert_column_matches(got.column(0), exp, f"on = {on}") == 0
            assert M.column_values(got.column(1)) == M.column_values(b.column(K.S))
    finally:
        hip.fn("project_destroy")(h)


# ---- fuzz -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_fuzz(hip, seed):
    """random schemas over all five types, random trees that mix the new operand kinds with the numeric ones"""
    fb, preds, proj = K.fuzz_case(seed)
    for k, e in enumerate(preds):
        predicted = K.count_eligible(e, fb)
        with route(hip, predicted, per_node_at_most=nodes_above_leaves(e) * (len(fb) - predicted)):
            got = list(FilterExecutor(hip, e, fb, depth=2, async_all_types=True).execute())
        K.assert_filter_stream(got, fb, [M.evaluate(e, b) for b in fb], f"seed {seed} predicate {k}", -1)
        K.same_batches(got, list(FilterExecutor(hip, e, fb).execute()), f"seed {seed} predicate {k} against push")
    predicted = K.count_eligible(proj, fb)
    with route(hip, predicted, per_node_at_most=sum(nodes_above_leaves(e) for e in proj) * (len(fb) - predicted)):
        got = list(ProjectExecutor(hip, proj, fb, depth=2, async_all_types=True).execute())
    K.assert_project_stream(got, fb, proj, [[M.evaluate(e, b) for e in proj] for b in fb], f"seed {seed} projection")
    K.same_batches(got, list(ProjectExecutor(hip, proj, fb).execute()), f"seed {seed} projection against push")
