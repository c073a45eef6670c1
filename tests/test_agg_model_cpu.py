"""The aggregate model (agg_model.py) and its cases (agg_edge_cases.py) checked without a GPU:

* the model's numpy against the same definitions written row by row with Python integers;
* the model against the CPU oracle on every case family at small sizes, single and multi batch, and on the join cases
  (HashAgg over HashJoin);
* the two conditions of agg_edge_cases.py on every case test_gpu_agg_edges.py runs (same seeds, same builders);
* planted faults: each is applied to the EXPECTED table of the model, never to a library, and `compare` must reject it on
  every case family it concerns."""
import functools
import math

import numpy as np
import pyarrow as pa
import pytest

import agg_edge_cases as E
import agg_model as M
from sqlrs_amd.executor import HashAggExecutor, HashJoinExecutor
from sqlrs_amd.expr import InputRef, JoinCondition

FUNCS = E.ALL_FUNCS


def table_of(batches):
    batches = list(batches)
    return pa.Table.from_batches(batches) if batches else None


@pytest.mark.parametrize("name", list(E.SMALL_CASES))
def test_model_equals_its_row_by_row_restatement(name):
    case = E.small_case(name)
    g = case.model(FUNCS)
    args = [case.cols[c] for c in E.COLS]
    slow = M.aggregate_slow(case.keys, case.key_valid, args, [(f, E.COLS.index(c)) for f, c in FUNCS],
                            None if case.arrival is None else case.ranges())
    assert len(slow) == len(g)
    for gi, (k, cells) in enumerate(slow):
        assert (k is None) == (not g.key_valid[gi]) and (k is None or k == g.keys[gi])
        for col, cell in zip(g.cols, cells):
            if cell is None:
                assert not col.valid[gi]
            elif isinstance(cell, tuple):
                assert col.valid[gi] and col.how[gi] == cell[0] and col.S[gi] == cell[2] and col.m[gi] == cell[3]
                assert cell[0] in (M.NAN, M.ZERO) or int(col.bits[gi]) == cell[1]
            else:
                assert col.valid[gi] and int(col.bits[gi]) == cell % (1 << 64), (col.func, col.kind, gi)


@pytest.mark.parametrize("name", list(E.SMALL_CASES))
def test_model_agrees_with_the_oracle(oracle, name):
    """HashAggExecutor(oracle) over the case's batches in their arrival order: groups, order, validity, every bit pattern,
    SUM(f64) inside the model's bound"""
    case = E.small_case(name)
    got = table_of(HashAggExecutor(oracle, E.agg_funcs(FUNCS), [InputRef(0)], case.batches()).execute())
    M.compare(got, case.model(FUNCS), name)


@pytest.mark.parametrize("kind", ["unique", "duplicates", "attribute"])
def test_model_of_the_join_cases_agrees_with_the_oracle(oracle, kind):
    """the join written out row by row by the cases module = HashAgg(HashJoin) of the oracle"""
    jc = E.join_case(kind)
    probe = jc.probe.batches()
    schema = pa.schema([(f"b.{f.name}", f.type) for f in jc.build_batch.schema] + [(f"p.{f.name}", f.type) for f in probe[0].schema])
    join = HashJoinExecutor(oracle, [jc.build_batch], probe, "inner", JoinCondition([(InputRef(0), InputRef(0))]), schema, 2)
    gb = [InputRef(1)] if kind == "attribute" else [InputRef(0)]
    got = table_of(HashAggExecutor(oracle, E.agg_funcs(FUNCS, first_col=3), gb, join.execute()).execute())
    M.compare(got, jc.joined.model(FUNCS), kind)


def test_model_of_distinct_agrees_with_the_oracle(oracle):
    case = E.build("distinct_small", n=3000, seed=62, groups=60, keyspace="sparse", nullable="random", batches=2)
    aggs = E.agg_funcs([("count", "i")], distinct=True) + E.agg_funcs([("sum", "i")], distinct=True)
    got = table_of(HashAggExecutor(oracle, aggs, [InputRef(0)], case.batches()).execute())
    M.compare(got, E.distinct_case(case).model([("count", "j"), ("sum", "i")]), "distinct")


# ---- the two conditions, on every case of the GPU file ---------------------------------------------------------------------------
COVER_FUNCS = [("sum", "f"), ("sum", "g"), ("min", "f"), ("max", "f"), ("min", "i"), ("max", "i"), ("min", "j"), ("max", "j")]


@functools.lru_cache(maxsize=None)
def facts(name):
    """(class shares of SUM(f) and SUM(g), the (what, value) pairs the case covers)"""
    if name.startswith("join_"):
        case = E.join_case(name[5:]).joined
    else:
        case = E.gpu_case(name)
    # (the classes of the sums, not their values; what a case covers is only collected below 2^18 rows: the pools are covered by
    #  the small cases, and MIN / MAX over the 2^21-row cases would be most of this file's time)
    funcs = COVER_FUNCS if case.n < (1 << 18) else COVER_FUNCS[:2]
    g = case.model(funcs, classes_only=True)
    cover = set()
    if case.n >= (1 << 18):
        return M.class_share(g), cover
    for col, (fn, c) in zip(g.cols, funcs):
        pool = {"f": E.F64_POOL, "i": [v % (1 << 64) for v in E.I64_POOL], "j": [v % (1 << 64) for v in E.I32_POOL]}.get(c, [])
        if fn in ("min", "max"):
            have = set(col.bits[col.valid].tolist())
            cover |= {(fn, c, v) for v in pool if v in have}
    for c, pool in (("f", E.F64_POOL), ("i", E.I64_POOL), ("j", E.I32_POOL)):
        v, valid = case.cols[c]
        bits = (M.f64_bits(v) if c == "f" else v.astype(np.int64).view(np.uint64))[slice(None) if valid is None else valid]
        have = set(np.unique(bits).tolist())
        cover |= {("sum", c, x % (1 << 64)) for x in pool if x % (1 << 64) in have}
    return M.class_share(g), cover


GPU_CASE_NAMES = list(E.GPU_CASES) + ["join_unique", "join_duplicates", "join_attribute"]


@pytest.mark.parametrize("name", GPU_CASE_NAMES)
def test_at_most_a_tenth_of_the_sums_is_compared_by_class(name):
    shares, _ = facts(name)
    for by_class, groups in shares:
        assert 10 * by_class <= groups, (name, by_class, groups)


def test_every_edge_value_is_a_min_a_max_and_a_sum_operand_somewhere():
    cover = set()
    for name in GPU_CASE_NAMES:
        cover |= facts(name)[1]
    missing = [(fn, c, hex(v % (1 << 64))) for c, pool in (("f", E.F64_POOL), ("i", E.I64_POOL), ("j", E.I32_POOL))
               for v in pool for fn in ("min", "max", "sum") if (fn, c, v % (1 << 64)) not in cover]
    assert not missing, missing


# ---- planted faults ---------------------------------------------------------------------------------------------------------
def cells_of(table):
    """[(valid bool[], bits uint64[], kind)] per column of an expected table, to be edited"""
    out = []
    for c in range(table.num_columns):
        t = table.column(c).type
        kind = "f64" if t == pa.float64() else ("i32" if t == pa.int32() else "i64")
        valid, bits = M.column_bits(table.column(c), kind)
        out.append([valid.copy(), bits.copy(), kind])
    return out


def table_from(cells):
    cols = []
    for valid, bits, kind in cells:
        if kind == "f64":
            v, t = M.bits_f64(bits), pa.float64()
        elif kind == "i32":
            v, t = bits.view(np.int64).astype(np.int32), pa.int32()
        else:
            v, t = bits.view(np.int64), pa.int64()
        cols.append(pa.array(v, type=t, mask=~valid))
    return pa.table(cols, names=[f"c{i}" for i in range(len(cols))])


def rejected(cells, groups) -> bool:
    try:
        M.compare(table_from(cells), groups)
    except AssertionError:
        return True
    return False


def col_at(fn, c):
    return 1 + FUNCS.index((fn, c))


def group_rows(case, gi, groups):
    """rows of group gi"""
    if groups.key_valid[gi]:
        at = case.keys == groups.keys[gi]
        return np.nonzero(at if case.key_valid is None else at & case.key_valid)[0]
    return np.nonzero(~case.key_valid)[0]


@functools.lru_cache(maxsize=None)
def expected(name):
    case = E.small_case(name)
    groups = case.model(FUNCS)
    table = M.to_table(groups)
    assert M.compare(table, groups) >= 0  # (the expectation passes its own comparison)
    return case, groups, table


FAMILIES = list(E.SMALL_CASES)


def test_fault_dropped_smallest_row():
    """SUM(f) of a group without its smallest-|x| valid row.  Tried on every FINITE group of every family; the inputs are
    made so (agg_edge_cases._ordinary: zeros and subnormals are rare) that the dropped value exceeds gamma * S — is visible
    — in at least 90 % of them, which is asserted, and every visible one must be rejected."""
    tried = visible = caught = 0
    for name in FAMILIES:
        case, groups, table = expected(name)
        col = groups.cols[col_at("sum", "f") - 1]
        v, valid = case.cols["f"]
        for gi in np.nonzero(col.how == M.FINITE)[0]:
            rows = group_rows(case, gi, groups)
            rows = rows if valid is None else rows[valid[rows]]
            xs = v[rows]
            drop = int(np.argmin(np.abs(xs)))
            rest = np.delete(xs, drop)
            cells = cells_of(table)
            cells[col_at("sum", "f")][1][gi] = M.f64_bits([math.fsum(rest)])[0]
            tried += 1
            seen = abs(xs[drop]) > 2 * float(M.gamma(col.m[gi] + 1)) * col.S[gi]  # (beyond the bound around either sum)
            visible += seen
            r = rejected(cells, groups)
            caught += r
            assert r or not seen, (name, gi, xs[drop], col.S[gi])
    assert tried > 1000 and visible >= 0.9 * tried, (tried, visible)
    assert caught >= visible


def test_fault_null_slot_added_to_a_sum():
    """one NULL row's slot value added into SUM(f) and SUM(i)"""
    concerned = 0
    for name in FAMILIES:
        case, groups, table = expected(name)
        for c in ("f", "i"):
            v, valid = case.cols[c]
            if valid is None:
                continue
            col = groups.cols[col_at("sum", c) - 1]
            for gi in np.nonzero((col.how == M.FINITE) | (col.how == M.EXACT))[0]:
                rows = group_rows(case, gi, groups)
                nulls, vals = rows[~valid[rows]], rows[valid[rows]]
                if c == "f":
                    nulls = nulls[np.isfinite(v[nulls]) & (np.abs(v[nulls]) > 1e-3)]
                else:
                    nulls = nulls[v[nulls] != 0]
                if len(nulls) == 0 or col.m[gi] > 100:
                    continue
                cells = cells_of(table)
                if c == "f":
                    cells[col_at("sum", c)][1][gi] = M.f64_bits([math.fsum(list(v[vals]) + [v[nulls[0]]])])[0]
                else:
                    cells[col_at("sum", c)][1][gi] = np.uint64(M.wrap_i64(sum(int(x) for x in v[vals]) + int(v[nulls[0]])) % (1 << 64))
                assert rejected(cells, groups), (name, c, gi)
                concerned += 1
                break
    assert concerned >= 6


def test_fault_count_includes_nulls():
    concerned = 0
    for name in FAMILIES:
        case, groups, table = expected(name)
        for c in E.COLS:
            valid = case.cols[c][1]
            if valid is None:
                continue
            col = groups.cols[col_at("count", c) - 1]
            for gi in range(len(groups)):
                rows = group_rows(case, gi, groups)
                if len(rows) != col.m[gi]:
                    cells = cells_of(table)
                    cells[col_at("count", c)][1][gi] = np.uint64(len(rows))
                    assert rejected(cells, groups), (name, c, gi)
                    concerned += 1
                    break
    assert concerned >= 12


def test_fault_sum_saturates_instead_of_wrapping():
    concerned = 0
    for name in FAMILIES:
        case, groups, table = expected(name)
        v, valid = case.cols["i"]
        for gi in range(len(groups)):
            rows = group_rows(case, gi, groups)
            rows = rows if valid is None else rows[valid[rows]]
            true = sum(int(x) for x in v[rows]) if len(rows) <= 200 else 0
            if not (E.INT64_MIN <= true <= E.INT64_MAX):
                cells = cells_of(table)
                cells[col_at("sum", "i")][1][gi] = np.uint64(max(E.INT64_MIN, min(E.INT64_MAX, true)) % (1 << 64))
                assert rejected(cells, groups), (name, gi)
                concerned += 1
                break
    assert concerned >= len(FAMILIES) - 3  # (one row, five large groups, 21 groups of three half-NULL rows: nothing to try)


NEG_ZERO, POS_ZERO = 0x8000000000000000, 0


def test_fault_min_takes_the_zeros_for_equal():
    """MIN(f) of a group whose smallest value is -0.0 reported as +0.0"""
    concerned = 0
    for name in FAMILIES:
        _, groups, table = expected(name)
        col = groups.cols[col_at("min", "f") - 1]
        for gi in np.nonzero(col.valid & (col.bits == NEG_ZERO))[0][:3]:
            cells = cells_of(table)
            cells[col_at("min", "f")][1][gi] = POS_ZERO
            assert rejected(cells, groups), (name, gi)
            concerned += 1
    assert concerned >= 1


def test_fault_min_max_skip_nan():
    """MIN / MAX(f) over the group's values that are no NaN (NULL when nothing is left)"""
    concerned = 0
    for name in FAMILIES:
        case, groups, table = expected(name)
        v, valid = case.cols["f"]
        for fn in ("min", "max"):
            col = groups.cols[col_at(fn, "f") - 1]
            for gi in np.nonzero(col.valid & np.isnan(M.bits_f64(col.bits)))[0]:
                rows = group_rows(case, gi, groups)
                xs = v[rows if valid is None else rows[valid[rows]]]
                xs = xs[~np.isnan(xs)]
                cells = cells_of(table)
                if len(xs):
                    img = M.total_order(M.f64_bits(xs))
                    cells[col_at(fn, "f")][1][gi] = M.total_order_back(np.array([img.min() if fn == "min" else img.max()]))[0]
                else:
                    cells[col_at(fn, "f")][0][gi] = False
                assert rejected(cells, groups), (name, fn, gi)
                concerned += 1
    assert concerned >= 2 * (len(FAMILIES) - 3)


def test_fault_neutral_valued_group_reported_null():
    """MAX(i) of an all-INT64_MIN group and MIN(i) of an all-INT64_MAX group (their ordered images are the accumulators' starts)
    reported NULL; the same for the f64 patterns 0xFFFF..F / 0x7FFF..F"""
    concerned = 0
    for name in FAMILIES:
        _, groups, table = expected(name)
        for fn, c, neutral in (("max", "i", E.INT64_MIN % (1 << 64)), ("min", "i", E.INT64_MAX), ("max", "f", 0xFFFFFFFFFFFFFFFF), ("min", "f", 0x7FFFFFFFFFFFFFFF)):
            col = groups.cols[col_at(fn, c) - 1]
            for gi in np.nonzero(col.valid & (col.bits == neutral))[0][:2]:
                cells = cells_of(table)
                cells[col_at(fn, c)][0][gi] = False
                assert rejected(cells, groups), (name, fn, c, gi)
                concerned += 1
    assert concerned >= 4 * (len(FAMILIES) - 3)


def test_fault_all_null_group_reported_as_zero():
    concerned = 0
    for name in FAMILIES:
        _, groups, table = expected(name)
        for fn, c in FUNCS:
            col = groups.cols[col_at(fn, c) - 1]
            for gi in np.nonzero(~col.valid)[0][:1]:
                cells = cells_of(table)
                cells[col_at(fn, c)][0][gi], cells[col_at(fn, c)][1][gi] = True, 0
                assert rejected(cells, groups), (name, fn, c, gi)
                concerned += 1
    assert concerned >= 12 * 4  # (SUM / MIN / MAX of four columns in the nullable families)


def test_fault_two_groups_swapped():
    for name in FAMILIES:
        _, groups, table = expected(name)
        if len(groups) < 2:
            continue
        cells = cells_of(table)
        for valid, bits, _ in cells:
            for arr in (valid, bits):
                arr[[0, 1]] = arr[[1, 0]]
        assert rejected(cells, groups), name
