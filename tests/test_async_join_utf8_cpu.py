"""sqlrs_hash_join_set_async_utf8 off the GPU: the header and abi.py declare the setter alike, a backend without the entry
point (the oracle) runs a HashJoinExecutor with ``async_utf8=True`` unchanged, and every case of tests/async_utf8_cases.py is
mixed by the restated rule: some batches eligible, some not — what keeps the GPU tests' count assertions from being vacuous."""
import inspect
import os
import re

import pytest

import async_utf8_cases as cases
from sqlrs_amd import abi
from sqlrs_amd.executor import HashJoinExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_the_setter_with_the_headers_arity():
    header = open(os.path.join(ROOT, "include", "sqlrs_hip.h")).read()
    m = re.search(r"\bint\s+sqlrs_hash_join_set_async_utf8\s*\(([^)]*)\)\s*;", header)
    assert m, "the header declares sqlrs_hash_join_set_async_utf8"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 2 and params[0].startswith("sqlrs_hash_join_t *") and params[1].startswith("int ")
    d = re.search(r'"hash_join_set_async_utf8":\s*\((\w+),\s*\[([^\]]*)\]\)', inspect.getsource(abi.Backend._declare))
    assert d, "abi.py declares hash_join_set_async_utf8"
    assert d.group(1) == "i" and [a.strip() for a in d.group(2).split(",")] == ["vp", "C.c_int"]


def test_oracle_runs_unchanged_with_the_flag(oracle):
    assert getattr(oracle.lib, oracle.prefix + "hash_join_set_async_utf8", None) is None
    from test_gpu_parity import join_schema
    c = cases.empty_strings_case()
    sch = join_schema(c.lb, c.rbs[0])
    for jt in cases.JOIN_TYPES:
        exp = list(HashJoinExecutor(oracle, [c.lb], c.rbs, jt, c.cond, sch, c.lb.num_columns).execute())
        for depth in (0, 3):
            got = list(HashJoinExecutor(oracle, [c.lb], c.rbs, jt, c.cond, sch, c.lb.num_columns, depth=depth, async_general=True,
                                        async_utf8=True).execute())
            assert len(got) == len(exp) and all(g.equals(e) for g, e in zip(got, exp))


@pytest.mark.parametrize("case", cases.all_cases(), ids=repr)
def test_every_case_is_mixed(case):
    """0 < eligible < len(batches) under every (join type, async_general) the case is run with; with the Utf8 switch off the
    same rule admits nothing (every case carries a Utf8 column)"""
    assert case.runs
    for jt, general in case.runs:
        n = cases.count_eligible(case, jt, general)
        print(f"{case.name} {jt} general={general}: eligible {n} of {len(case.rbs)}")
        assert 0 < n < len(case.rbs), (case.name, jt, general, n)
        assert cases.count_eligible(case, jt, general, utf8=False) == 0


def test_the_cases_hold_what_they_are_for():
    """the shapes the GPU tests rely on, checked where they are built"""
    for form in cases.FORMS:
        c = cases.form_case(form)
        m = cases.max_run(c.lb, c.lkey)
        assert m == (1 if form.startswith("unique") else 4)
        s1 = c.lb.column(1)
        lens = [len(x.encode()) if x is not None else 0 for x in s1.to_pylist()]
        assert cases.lmax_of(s1) == 22 and (s1[-1].as_py() is None or lens[-1] == 22)
        assert any(cases.offsets_of(s1)[i + 1] > cases.offsets_of(s1)[i] for i in range(len(s1)) if not s1[i].is_valid)  # bytes under a NULL slot
        assert all(int(cases.offsets_of(b.column(3))[0]) == 5 for b in c.rbs)  # offsets[0] != 0
        full = [b for b in c.rbs if b.num_rows == 4096]
        assert len(full) == 1
        if form.startswith("unique"):  # the full batch is kept whole by the Inner join, and the rule admits it
            keys = set(c.lb.column(0).to_pylist())
            assert all(k in keys for k in full[0].column(1).to_pylist())
            assert cases.eligible(c.lb, full[0], 0, 1, "inner", 1, False)
        assert sorted(b.num_rows for b in c.rbs) == sorted(cases.SIZES + [1024])
    ch = cases.chunk_case()
    assert cases.max_run(ch.lb, 0) == 4 and cases.lmax_of(ch.lb.column(2)) == 0
    b = cases.bound_case()
    want = [cases.eligible(b.lb, rb, 0, 0, "inner", 1, False) for rb in b.rbs]
    assert want == [False, True, False, True] and b.rbs[2].num_rows == b.rbs[1].num_rows + 1
    assert cases.out_bytes(b.lb, b.rbs[0], 4096) > cases.SA_AREA and cases.lmax_of(b.lb.column(1)) == 200
    mixed = 0
    for seed in cases.FUZZ_SEEDS:
        c, jt, general, _ = cases.fuzz_case(seed)
        n = cases.count_eligible(c, jt, general)
        mixed += 0 < n < len(c.rbs)
    assert mixed >= 5  # (the fuzz is not a row of all-synchronous streams)
