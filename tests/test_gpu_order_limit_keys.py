"""ORDER BY ... LIMIT with SQLRS_ORDER_LIMIT_ALL_KEYS on the first key (order_topk.hip): a Utf8 first key, a fixed-width
first key with NULLs, a key expression.  The rows are those of Limit(Order(..)) on the CPU oracle over the whole batch, column by column;
which route ran is read from the `order_topk_keys*` witnesses of sqlrs_ctx_profile_read and from topk_candidates.  The shapes
(order_limit_keys_cases.py) are the ones the numpy model of test_order_limit_keys_cpu.py places on the candidates route or on
an ignored one.  n = 2^17 + 67 rows (not a multiple of 64, sample step 2) pushed as two slices, so the concatenated Utf8
offsets of the second slice do not start at 0; SQLRS_ORDER_TOPK=1 lifts the size rule to the test size."""
import numpy as np
import pyarrow as pa
import pytest

import order_limit_keys_cases as K
from order_plan import read_counters
from sqlrs_amd import abi
from sqlrs_amd.executor import LimitExecutor, OrderExecutor
from sqlrs_amd.expr import InputRef, OrderBy

pytestmark = pytest.mark.gpu

N, OFF = K.N, 37
NEW = ("order_topk_keys", "order_topk_keys_ignored")
_batches, _expected = {}, {}


def batch_of(name, payload_f64=False):
    """{key, int64 row id[, nullable float64]} of a shared case, built once"""
    key = (name, payload_f64)
    if key not in _batches:
        cols, names = [K.arrow_key(K.BY_NAME[name]), pa.array(np.arange(N, dtype=np.int64))], ["k", "row"]
        if payload_f64:
            rng = np.random.default_rng(11)
            cols.append(pa.array(rng.random(N), mask=rng.random(N) < 0.1))
            names.append("x")
        _batches[key] = pa.RecordBatch.from_arrays(cols, names=names)
    return _batches[key]


def expected(oracle, tag, b, ob, k):
    """Limit(Order(..)) on the oracle over the whole batch, computed once per (case, keys, k)"""
    if tag not in _expected:
        _expected[tag] = pa.Table.from_batches(list(LimitExecutor(oracle, k, OFF, OrderExecutor(oracle, ob, [b]).execute()).execute()))
    return _expected[tag]


def delta(hip, before):
    after = read_counters(hip)
    return {name: after.get(name, 0) - before.get(name, 0) for name in NEW + ("order_topk", "order_topk_ignored")}


def run(hip, b, ob, k, on=True, out_mem=abi.MEM_HOST):
    before = read_counters(hip)
    ex = OrderExecutor(hip, ob, [b.slice(0, N // 3), b.slice(N // 3)], limit_hint=OFF + k, limit_all_keys=on, out_mem=out_mem)
    got = pa.Table.from_batches(list(LimitExecutor(hip, k, OFF, ex.execute()).execute()))
    return got, ex.topk_candidates, delta(hip, before)


def same_rows(got, exp, k):
    assert got.num_rows == exp.num_rows == k
    for i in range(exp.num_columns):
        assert got.column(i).combine_chunks().equals(exp.column(i).combine_chunks()), exp.column_names[i]


def on_route(case, cand, d):
    if case.expect == "topk":
        assert 0 < cand < N // 4, cand
        assert d["order_topk_keys"] == 1 and d["order_topk_keys_ignored"] == 0, d
    else:
        assert cand == 0
        assert d["order_topk_keys_ignored"] == 1 and d["order_topk_keys"] == 0, d
    assert d["order_topk"] == 0 and d["order_topk_ignored"] == 0, d     # (the plain route's witnesses count its own path only)


@pytest.fixture(autouse=True)
def forced_size_rule(monkeypatch):
    monkeypatch.setenv("SQLRS_ORDER_TOPK", "1")


@pytest.mark.parametrize("case", K.UTF8_CASES, ids=lambda c: c.name)
def test_utf8_first_key(hip, oracle, case):
    b, k = batch_of(case.name), case.hint - OFF
    ob = [OrderBy(InputRef(0), asc=case.asc)]
    got, cand, d = run(hip, b, ob, k)
    same_rows(got, expected(oracle, case.name, b, ob, k), k)
    on_route(case, cand, d)


@pytest.mark.parametrize("case", K.FIXED_CASES, ids=lambda c: c.name)
def test_nullable_fixed_width_first_key(hip, oracle, case):
    """f64_5pct_nulls_desc: NaN, +-inf and +-0.0 among the values; the NULLs cover the limit and the second key decides"""
    b, k = batch_of(case.name), case.hint - OFF
    ob = [OrderBy(InputRef(0), asc=case.asc)]
    if case.kind == "f64":
        ob.append(OrderBy(InputRef(1), asc=False))
    got, cand, d = run(hip, b, ob, k)
    same_rows(got, expected(oracle, case.name, b, ob, k), k)
    on_route(case, cand, d)


def test_several_keys_threshold_on_the_first(hip, oracle):
    """ORDER BY name, row DESC: 50 distinct names; the threshold is on the first key, the candidates are sorted on both"""
    case = K.BY_NAME["fifty_values"]
    b, k = batch_of(case.name), 1000
    ob = [OrderBy(InputRef(0), asc=True), OrderBy(InputRef(1), asc=False)]
    got, cand, d = run(hip, b, ob, k)
    same_rows(got, expected(oracle, "fifty_values/row_desc", b, ob, k), k)
    on_route(case, cand, d)


def expr_batch():
    rng = np.random.default_rng(7)
    a = rng.integers(-(1 << 40), 1 << 40, N, dtype=np.int64)
    bb = rng.integers(-(1 << 40), 1 << 40, N, dtype=np.int64)
    return pa.RecordBatch.from_arrays([pa.array(a), pa.array(bb, mask=rng.random(N) < 0.01), pa.array(np.arange(N, dtype=np.int64))],
                                      names=["a", "b", "row"])


def test_key_expression(hip, oracle):
    """ORDER BY a + b, b with NULLs: the expression is evaluated once over the input, NULL sums first"""
    b, k = expr_batch(), 1000
    ob = [OrderBy(InputRef(0) + InputRef(1), asc=True)]
    got, cand, d = run(hip, b, ob, k)
    same_rows(got, expected(oracle, "a+b", b, ob, k), k)
    assert 0 < cand < N // 4 and d["order_topk_keys"] == 1, (cand, d)


def test_key_expression_error_is_the_full_sorts(hip):
    """ORDER BY a / b with one b = 0: the same status and text with the switch on as with it off"""
    rng = np.random.default_rng(7)
    a = rng.integers(1, 1 << 40, N, dtype=np.int64)
    bb = rng.integers(1, 1 << 20, N, dtype=np.int64)
    bb[N // 2] = 0
    b = pa.RecordBatch.from_arrays([pa.array(a), pa.array(bb), pa.array(np.arange(N, dtype=np.int64))], names=["a", "b", "row"])
    ob = [OrderBy(InputRef(0) / InputRef(1), asc=True)]
    seen = []
    for on in (False, True):
        with pytest.raises(abi.ExecutorError) as e:
            run(hip, b, ob, 1000, on=on)
        seen.append((e.value.status, str(e.value)))   # (the text carries sqlrs_last_error)
    assert seen[0] == seen[1], seen
    assert "Divide by zero" in seen[0][1], seen


@pytest.mark.parametrize("name", ["letters_asc", "i64_1pct_nulls"])
def test_switch_off_changes_nothing(hip, oracle, name):
    case = K.BY_NAME[name]
    b, k = batch_of(name), case.hint - OFF
    ob = [OrderBy(InputRef(0), asc=case.asc)]
    got, cand, d = run(hip, b, ob, k, on=False)
    same_rows(got, expected(oracle, name, b, ob, k), k)
    assert cand == 0 and d["order_topk_keys"] == 0 and d["order_topk_keys_ignored"] == 0, (cand, d)


def test_plain_first_key_keeps_its_route(hip, oracle):
    """switch on, a plain Int64 first key without NULLs: order_topk serves it, as without the switch"""
    rng = np.random.default_rng(7)
    b = pa.RecordBatch.from_arrays([pa.array(rng.integers(-(1 << 40), 1 << 40, N, dtype=np.int64)), pa.array(np.arange(N, dtype=np.int64))],
                                   names=["k", "row"])
    ob = [OrderBy(InputRef(0), asc=True)]
    got, cand, d = run(hip, b, ob, 1000)
    same_rows(got, expected(oracle, "plain_i64", b, ob, 1000), 1000)
    assert 0 < cand < N // 4 and d["order_topk"] == 1 and d["order_topk_keys"] == 0 and d["order_topk_keys_ignored"] == 0, (cand, d)


@pytest.mark.parametrize("name,out_mem", [("letters_1pct_nulls_desc", abi.MEM_DEVICE), ("f64_5pct_nulls_desc", abi.MEM_HOST)],
                         ids=["utf8_device", "f64_host"])
def test_out_mem_and_a_nullable_payload(hip, oracle, name, out_mem):
    case = K.BY_NAME[name]
    b, k = batch_of(name, payload_f64=True), case.hint - OFF
    ob = [OrderBy(InputRef(0), asc=case.asc), OrderBy(InputRef(1), asc=True)]
    got, cand, d = run(hip, b, ob, k, out_mem=out_mem)
    same_rows(got, expected(oracle, name + "/payload", b, ob, k), k)
    on_route(case, cand, d)
