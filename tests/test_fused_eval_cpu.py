"""What test_gpu_fused_eval.py relies on, checked without a GPU: the left-out cap on the model alone, the forecast "this
expression compiles" at its edges, and the switch declared alike in the header, abi.py, the executors and the mirrors."""
import inspect
import os
import re

import expr_model as M
import fused_eval_cases as F
from sqlrs_amd import abi
from sqlrs_amd.expr import Constant, InputRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_modelled_case_leaves_out_at_most_the_cap():
    """the cap is a condition of the cases, not of the device: no GPU comparison can hide behind it"""
    seen = 0
    for label, res in F.model_results():
        assert res.left_out_fraction <= M.MAX_LEFT_OUT, (label, res.left_out_fraction)
        seen += 1
    assert seen > 500


def test_two_sweep_case_is_two_sweeps_and_a_ragged_tail():
    assert F.SWEEP_N == 4_194_381 and F.SWEEP_N - 2 * F.SWEEP_ROWS == 64 + 13
    cols, batch = F.sweep_case()
    assert batch.num_rows == F.SWEEP_N and batch.column(0).null_count > 0 and batch.column(1).null_count > 0
    true, valid = F.sweep_predicate_numpy(cols)
    assert 0.1 < true.mean() < 0.9 and 0 < (~valid).sum() < F.SWEEP_N // 4
    s = cols["i"][0].astype(object)[:2000] + cols["j64"][0].astype(object)[:2000]  # exact integers: some sums leave int64
    assert any(v > M.I64_MAX or v < M.I64_MIN for v in s)
    # the numpy statement agrees with the model on a prefix
    head = batch.slice(0, 3000)
    res = M.evaluate(F.sweep_predicate(), head)
    assert [None if not ok else int(t) for t, ok in zip(true[:3000], valid[:3000])] == res.vals
    res = M.evaluate(F.sweep_value(), head)
    v, ok = F.sweep_value_numpy(cols)
    assert [None if not o else int(x) for x, o in zip(v[:3000], ok[:3000])] == res.vals


def test_forecast_edges():
    dt = F.dtypes_of(M.trees_batch())
    lim = F.limit_exprs()
    for label, (e, fused) in lim.items():
        assert F.compiles(e, dt) == fused, label
    assert M.program_shape(lim["24 nodes"][0])[0] == F.PROG_MAX and M.program_shape(lim["25 nodes"][0])[0] == F.PROG_MAX + 1
    assert M.program_shape(lim["stack 8"][0])[1] == F.STACK_MAX and M.program_shape(lim["stack 9"][0])[1] == F.STACK_MAX + 1
    # 16 / 17 distinct columns (a column named twice counts once); the node limit bounds one expression at 12 columns, so the
    # column limit is reached by the computed columns of ONE launch together: the forecast per expression stays true
    wide = [abi.INT64] * 17
    assert F.compiles(F.sum_of_columns(12), wide) and not F.compiles(F.sum_of_columns(13), wide)
    assert F.compiles(InputRef(16) + InputRef(16), wide)
    # Utf8: a column or a constant anywhere
    assert not F.compiles(InputRef(0).eq(Constant("a", abi.UTF8)), [abi.UTF8])
    assert not F.compiles(InputRef(1).eq(InputRef(1)), [abi.INT64, abi.UTF8])
    assert F.compiles(InputRef(0).eq(InputRef(0)), [abi.INT64, abi.UTF8])  # (a Utf8 payload column does not matter)
    assert F.compiles(InputRef(0) & InputRef(1), [abi.BOOLEAN, abi.BOOLEAN])
    # precedence forecast of the Filter
    assert F.takes_cmp_const(InputRef(0) > Constant(1, abi.INT64), [abi.INT64])
    assert not F.takes_cmp_const(InputRef(0) > Constant(None, abi.INT64), [abi.INT64])
    assert not F.takes_cmp_const(InputRef(0) > Constant(1, abi.INT64), [abi.INT32])
    assert not F.takes_cmp_const(Constant(1, abi.INT64) < InputRef(0), [abi.INT64])
    assert not F.is_computed(InputRef(0)) and not F.is_computed(Constant(1, abi.INT64)) and F.is_computed(InputRef(0) + InputRef(0))


def test_columns_of_one_launch():
    """the 16-column limit binds the computed columns that share a launch: 4 expressions over 4 fresh columns each fit one
    launch, a fifth column set opens the next"""
    assert F.MAX_PROGS * 4 == F.MAX_COLS


def test_the_switch_is_declared_alike_everywhere():
    """a flag of the create calls (the set of entry points is pinned by the bindings' tests), 2 everywhere"""
    header = open(os.path.join(ROOT, "include", "sqlrs_hip.h")).read()
    h = re.search(r"^#define\s+SQLRS_EXPR_FUSED_EVAL\s+(\d+)\s*$", header, flags=re.M)
    assert h, "sqlrs_hip.h does not define SQLRS_EXPR_FUSED_EVAL"
    assert int(h.group(1)) == abi.EXPR_FUSED_EVAL == 2 and abi.EXPR_FUSED_EVAL != abi.EXPR_STAGE_ALL_TYPES
    for scope in ("push_many", "push_async", "sqlrs_eval_expr", "HashAgg", "join_agg", "join filter"):
        assert scope in header[header.index("Opt-in, SQLRS_EXPR_FUSED_EVAL"):h.start()], scope
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert re.search(r"^pub const SQLRS_EXPR_FUSED_EVAL: i32 = 2;$", ffi, flags=re.M)
    from sqlrs_amd.executor import FilterExecutor, ProjectExecutor
    for cls in (FilterExecutor, ProjectExecutor):
        assert inspect.signature(cls.__init__).parameters["fused_eval"].default is False, cls
    for path in ("host/sqlrs_executor.hpp", "bindings/rust/src/executors.rs"):
        text = open(os.path.join(ROOT, path)).read()
        assert len(re.findall(r"^\s*bool fused_eval\b|pub fused_eval: bool", text, flags=re.M)) >= 2, path
        assert "SQLRS_EXPR_FUSED_EVAL" in text, path


def test_packed_expressions_carry_the_flag_only_when_asked():
    e = InputRef(0) + InputRef(0)
    assert e.pack().abi.reserved == 0
    arr, keep = abi.pack_exprs([e, e])
    assert arr[0].reserved == 0 and arr[1].reserved == 0
