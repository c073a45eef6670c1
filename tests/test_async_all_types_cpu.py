"""sqlrs_filter_set_async_all_types / sqlrs_project_set_async_all_types without a GPU: the three declarations agree, the
executors take the flag, the oracle (which has no such entry point) runs unchanged with it, the cases of
tests/async_types_cases.py are what they claim, and the model and the oracle agree on every one of them."""
import inspect
import os
import re

import pytest

import async_types_cases as K
import expr_model as M
from sqlrs_amd import abi
from sqlrs_amd.executor import FilterExecutor, ProjectExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTERS = ("filter_set_async_all_types", "project_set_async_all_types")


def test_header_abi_and_rust_declare_both_setters_with_the_same_arity():
    header = open(os.path.join(ROOT, "include", "sqlrs_hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    abi_src = open(os.path.join(ROOT, "sqlrs_amd", "abi.py")).read()
    for name in SETTERS:
        h = re.search(r"\bint sqlrs_" + name + r"\s*\(([^;{}]*?)\)\s*;", header)
        assert h, f"include/sqlrs_hip.h does not declare sqlrs_{name}"
        r = re.search(r"pub fn sqlrs_" + name + r"\((.*?)\) -> c_int;", rust)
        assert r, f"ffi.rs does not declare sqlrs_{name}"
        a = re.search(r'"' + name + r'": \(i, \[(.*?)\]\)', abi_src)
        assert a, f"abi.py does not declare {name}"
        arity = [len([x for x in m.group(1).split(",") if x.strip()]) for m in (h, r, a)]
        assert arity == [2, 2, 2], (name, arity)
        op = name.split("_")[0]
        assert f"sqlrs_{op}_t *" in h.group(1) and "int on" in h.group(1), h.group(1)
        assert f"*mut sqlrs_{op}_t" in r.group(1) and "c_int" in r.group(1), r.group(1)


def test_the_mirrors_carry_the_flag():
    for cls in (FilterExecutor, ProjectExecutor):
        p = inspect.signature(cls.__init__).parameters
        assert "async_all_types" in p and p["async_all_types"].default is False, cls
    hpp = open(os.path.join(ROOT, "host", "sqlrs_executor.hpp")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "executors.rs")).read()
    for name in SETTERS:
        assert f"sqlrs_{name}(" in hpp and f"sqlrs_{name}(" in rs, name
    assert hpp.count("bool async_all_types = false;") == 2 and rs.count("pub async_all_types: bool") == 2


def test_the_oracle_runs_unchanged_with_the_flag(oracle):
    bs = K.stream()[:3]
    for name in ("s_eq_and_num", "p_and_q"):
        e = K.stream_predicates()[name]
        K.same_batches(list(FilterExecutor(oracle, e, bs, depth=2, async_all_types=True).execute()), list(FilterExecutor(oracle, e, bs).execute()), name)
    ex = K.stream_projection()
    K.same_batches(list(ProjectExecutor(oracle, ex, bs, depth=2, async_all_types=True).execute()), list(ProjectExecutor(oracle, ex, bs).execute()))


def test_the_streams_are_mostly_eligible_and_never_wholly():
    bs = K.stream()
    assert [b.num_rows for b in bs] == K.SIZES[:5] + [4096] + K.SIZES[5:]
    assert K.raw_bytes(bs[5]) > 2 * K.SA_AREA  # the batch of ~200-byte strings: over the slot
    for name, e in K.stream_predicates().items():
        n = K.count_eligible(e, bs)
        assert 0.75 * len(bs) <= n < len(bs), (name, n)
        assert n == len(bs) - 2, (name, n)  # 4097 rows and the batch over the slot
        assert K.count_eligible(e, bs, on=False) == 0, name  # (every batch carries Boolean columns)
    ex = K.stream_projection()
    n = K.count_eligible(ex, bs)
    assert 0.75 * len(bs) <= n < len(bs) and K.count_eligible(ex, bs, on=False) == 0
    for seed in range(8):
        fb, preds, proj = K.fuzz_case(seed)
        for e in preds + [proj]:
            n = K.count_eligible(e, fb)
            assert 0.75 * len(fb) <= n < len(fb), (seed, n)


def test_the_rule_on_its_own_edges():
    b = K.stream()[0]
    u = lambda v: K.Constant(v, abi.UTF8)  # noqa: E731
    s, a = K.InputRef(K.S), K.InputRef(K.A)
    assert K.filter_eligible(s.eq(u("x" * 1024)), b) and not K.filter_eligible(s.eq(u("x" * 1025)), b)
    assert K.filter_eligible(s.eq(u("x" * 512)) | s.eq(u("x" * 512)), b) and not K.filter_eligible(s.eq(u("x" * 512)) | s.eq(u("x" * 513)), b)
    assert not K.filter_eligible(s.eq(a), b)                       # Utf8 against Int64
    assert not K.filter_eligible(s, b)                              # a Utf8 result
    assert not K.filter_eligible(K.TypeCast(s, abi.INT64) > a, b)   # a Utf8 cast
    assert not K.project_eligible([u("k")], b) and K.project_eligible([s >= u("k"), s], b)
    assert not K.filter_eligible(s.eq(u("ab")), b, on=False)


@pytest.mark.parametrize("name", sorted(K.stream_predicates()))
def test_model_and_oracle_agree_on_the_stream(oracle, name):
    bs = K.stream()
    got = list(FilterExecutor(oracle, K.stream_predicates()[name], bs).execute())
    K.assert_filter_stream(got, bs, K.stream_model(name), name, K.RID)


def test_model_and_oracle_agree_on_the_projection(oracle):
    bs, ex = K.stream(), K.stream_projection()
    K.assert_project_stream(list(ProjectExecutor(oracle, ex, bs).execute()), bs, ex, K.stream_projection_model(), "projection")


def test_model_and_oracle_agree_on_the_cross_products(oracle):
    for batch, cases in ((M.utf8_batch(), K.utf8_cross_cases()), (M.bool_batch(), K.bool_cross_cases())):
        for label, e in cases:
            assert M.check_eval(oracle, e, batch, label) == 0


@pytest.mark.parametrize("seed", range(8))
def test_model_and_oracle_agree_on_the_fuzz_cases(oracle, seed):
    fb, preds, proj = K.fuzz_case(seed)
    for k, e in enumerate(preds):
        got = list(FilterExecutor(oracle, e, fb).execute())
        K.assert_filter_stream(got, fb, [M.evaluate(e, b) for b in fb], f"seed {seed} predicate {k}", -1)
    got = list(ProjectExecutor(oracle, proj, fb).execute())
    K.assert_project_stream(got, fb, proj, [[M.evaluate(e, b) for e in proj] for b in fb], f"seed {seed} projection")
