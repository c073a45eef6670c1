"""The CPU oracle against the independent edge-value model (tests/expr_model.py).

Every GPU parity test compares the library with the oracle, and the oracle was written from the same formulas as the
device evaluators: a mistake they share is invisible there.  Here the oracle's ``eval_column`` and ``FilterExecutor`` meet
a model that shares none of those formulas, over the edge values of every type: integer extremes and their 2^31 / 2^53
neighbours, +-0.0, +-inf, NaNs of both signs and two payloads, subnormals, the doubles around +-2^31, +-2^53 and +-2^63.
All comparisons are bit exact (expr_model.assert_column_matches); the rows a hardware-made NaN leaves out are capped at 2 %
inside every comparison."""
import numpy as np
import pyarrow as pa
import pytest

import expr_model as M
from sqlrs_amd import abi
from sqlrs_amd.expr import BinaryOp, Constant, InputRef, TypeCast


@pytest.mark.parametrize("form", ["colcol", "colconst"])
@pytest.mark.parametrize("op", M.ARITH_OPS + M.CMP_OPS)
@pytest.mark.parametrize("kind", list(M.NUMERIC))
def test_binary_operators_over_the_pool_cross_product(oracle, kind, op, form):
    """every operator x every numeric type, column-column and column-constant (either side, NULL constants too), over the
    full cross product of the type's pool (and NULL) with itself"""
    for label, e, b in M.binary_cases(M.NUMERIC[kind], op, form):
        M.check_eval(oracle, e, b, f"{kind}: {label}")


@pytest.mark.parametrize("op", M.CMP_OPS)
def test_utf8_and_boolean_comparisons(oracle, op):
    """Utf8 bytewise (empty string, proper prefixes, bytes >= 0x80), Booleans false < true; constants on either side"""
    u = M.utf8_batch()
    M.check_eval(oracle, BinaryOp(op, InputRef(0), InputRef(1)), u, f"utf8 x {op} y")
    for k in M.POOL_UTF8 + [None]:
        M.check_eval(oracle, BinaryOp(op, InputRef(0), Constant(k, abi.UTF8)), u, f"utf8 x {op} {k!r}")
        M.check_eval(oracle, BinaryOp(op, Constant(k, abi.UTF8), InputRef(1)), u, f"utf8 {k!r} {op} y")
    b = M.bool_batch()
    M.check_eval(oracle, BinaryOp(op, InputRef(0), InputRef(1)), b, f"bool p {op} q")
    for k in (False, True, None):
        M.check_eval(oracle, BinaryOp(op, InputRef(0), Constant(k, abi.BOOLEAN)), b, f"bool p {op} {k}")
        M.check_eval(oracle, BinaryOp(op, Constant(k, abi.BOOLEAN), InputRef(1)), b, f"bool {k} {op} q")


@pytest.mark.parametrize("dst", ["i32", "i64", "f64"])
@pytest.mark.parametrize("src", list(M.CAST_SOURCES))
def test_cast_lattice(oracle, src, dst):
    """bool / int32 / int64 / float64 -> int32 / int64 / float64 over the source's pool: truncation, NULL outside the
    target's range (both bounds inclusive), NaN and +-inf -> NULL, int -> double to nearest even"""
    s, d = M.CAST_SOURCES[src], M.NUMERIC[dst]
    M.check_eval(oracle, TypeCast(InputRef(0), d), M.cast_batch(s), f"cast {src} -> {dst}")
    pool = [False, True] if s == abi.BOOLEAN else M.POOLS[s]
    for k in list(pool) + [None]:  # a constant under the cast (and a second column so that the batch has rows)
        c = Constant(k, s) if s == abi.BOOLEAN else M.pool_constant(s, k)
        M.check_eval(oracle, TypeCast(c, d), M.cast_batch(s), f"cast {src} constant {k} -> {dst}")


def test_the_double_that_is_int64_min_casts_to_int64_min(oracle):
    """-2^63 is exactly INT64_MIN: in range (num-traits' inclusive lower bound for a float as wide as the integer); the
    doubles next to it on either side, and 2^63, decide the other way"""
    vals = [-(2.0 ** 63), float(np.nextafter(-(2.0 ** 63), -np.inf)), float(np.nextafter(-(2.0 ** 63), 0.0)),
            float(np.nextafter(2.0 ** 63, 0.0)), 2.0 ** 63]
    b = pa.RecordBatch.from_arrays([pa.array(vals, type=pa.float64())], names=["x"])
    exp = M.evaluate(TypeCast(InputRef(0), abi.INT64), b)
    assert exp.vals == [-(2 ** 63), None, -(2 ** 63) + 1024, 2 ** 63 - 1024, None]
    M.check_eval(oracle, TypeCast(InputRef(0), abi.INT64), b, "f64 -> i64 around -2^63", exp)


@pytest.mark.parametrize("op", ["and", "or"])
def test_kleene_and_or_over_all_nine_pairs(oracle, op):
    b = M.bool_batch()
    M.check_eval(oracle, BinaryOp(op, InputRef(0), InputRef(1)), b, f"p {op} q")
    for k in (False, True, None):
        M.check_eval(oracle, BinaryOp(op, InputRef(0), Constant(k, abi.BOOLEAN)), b, f"p {op} {k}")
        M.check_eval(oracle, BinaryOp(op, Constant(k, abi.BOOLEAN), InputRef(1)), b, f"{k} {op} q")
        for k2 in (False, True, None):
            M.check_eval(oracle, BinaryOp(op, Constant(k, abi.BOOLEAN), Constant(k2, abi.BOOLEAN)), b, f"{k} {op} {k2}")


def test_divide_by_zero(oracle):
    for label, e, b, raises in M.div0_cases():
        exp = M.model_outcome(e, b)
        assert (exp is M.DIV0) == raises, label
        M.check_eval(oracle, e, b, label, exp)


def test_integer_min_over_minus_one_wraps(oracle):
    """the project's choice (Parity, Unpinned): MIN / -1 wraps to MIN in both widths"""
    for dt, lo in ((abi.INT64, M.I64_MIN), (abi.INT32, M.I32_MIN)):
        b = pa.RecordBatch.from_arrays([M.array_of(dt, [lo, lo + 1, -1]), M.array_of(dt, [-1, -1, lo])], names=["x", "y"])
        exp = M.evaluate(InputRef(0) / InputRef(1), b)
        assert exp.vals == [lo, -(lo + 1), 0]
        M.check_eval(oracle, InputRef(0) / InputRef(1), b, f"MIN / -1 ({dt})", exp)


def test_scalar_scalar_expressions(oracle):
    """both operands constants: the result is a column of the batch's length all the same"""
    b = M.cast_batch(abi.INT64)
    for dt in M.NUMERIC.values():
        pool = M.POOLS[dt]
        for op in M.ARITH_OPS + M.CMP_OPS:
            for i, k in enumerate(list(pool) + [None]):
                k2 = pool[(i * 5 + 3) % len(pool)]
                if op == "/" and M._is_zero(dt, k2):
                    k2 = pool[-1]
                M.check_eval(oracle, BinaryOp(op, M.pool_constant(dt, k), M.pool_constant(dt, k2)), b, f"{dt}: {k} {op} {k2}")


@pytest.mark.parametrize("k", range(M.N_TREES))
def test_random_trees(oracle, k):
    """200 seeded trees of depth up to 4 over the pools: arithmetic, casts, comparisons (also of comparison results),
    Kleene AND / OR, NULL constants; value-typed and Boolean results"""
    e, _, exp = M.tree_case(k)
    M.check_eval(oracle, e, M.trees_batch(), f"tree {k}: {e}", exp)


def test_the_trees_cover_the_operators_and_stay_within_the_left_out_cap():
    """(the model alone) most trees evaluate without a division by zero, every operator and cast occurs, and no tree leaves
    out more than 2 % of its rows"""
    ops, ok = set(), 0
    for k in range(M.N_TREES):
        e, want, r = M.tree_case(k)
        ops |= {(n.op, n.dtype) for n in e.nodes() if n.op >= abi.EXPR_TYPE_CAST}
        if r is not M.DIV0:
            ok += 1
            assert r.dtype == want
            assert r.left_out_fraction <= M.MAX_LEFT_OUT, (k, r.left_out_fraction)
    assert ok >= 150, ok
    assert {o for o, _ in ops} >= set(range(abi.EXPR_PLUS, abi.EXPR_OR + 1))
    assert {d for o, d in ops if o == abi.EXPR_TYPE_CAST} == {abi.INT32, abi.INT64, abi.FLOAT64}
