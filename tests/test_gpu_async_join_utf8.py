"""sqlrs_hash_join_set_async_utf8: Utf8 payload columns, build side and probe side, through both one-launch kernels of
sqlrs_hash_join_probe_push_async (sa_probe_kernel<true>, sa_probe_general_kernel<true>, csrc/join_async.hip).  The async stream must be
the synchronous stream and the oracle's, batch for batch (exact Arrow equality), the tail batch of Left / Full included; which
batches take a kernel is the rule of include/sqlrs_hip.h as tests/async_utf8_cases.py restates it."""
import ctypes as C
import os

import pyarrow as pa
import pytest

import async_utf8_cases as cases
from sqlrs_amd import abi
from sqlrs_amd.executor import HashJoinExecutor
from sqlrs_amd.expr import InputRef, JoinCondition
from test_gpu_async import fast_batches, same_batches
from test_gpu_parity import join_schema

pytestmark = pytest.mark.gpu


def run(be, case, jt, depth=0, general=False, utf8=False, rbs=None):
    rbs = case.rbs if rbs is None else rbs
    sch = join_schema(case.lb, case.rbs[0])
    return list(HashJoinExecutor(be, [case.lb], rbs, jt, case.cond, sch, case.lb.num_columns, depth=depth, async_general=general,
                                 async_utf8=utf8).execute())


_ref_cache = {}


def reference_streams(hip, oracle, case, jt):
    """the oracle's stream and the synchronous probe_push stream of one case and join type: computed once, shared, not changed"""
    key = (case.name, jt)
    if key not in _ref_cache:
        _ref_cache[key] = (run(oracle, case, jt), run(hip, case, jt))
        same_batches(_ref_cache[key][1], _ref_cache[key][0])
    return _ref_cache[key]


def check_case(hip, oracle, case, jt, depth, general):
    """switch on: exactly the batches the rule admits take a kernel and the stream is the reference's; switch off: none does"""
    exp, sync = reference_streams(hip, oracle, case, jt)
    want = cases.count_eligible(case, jt, general)
    before = fast_batches(hip)
    got = run(hip, case, jt, depth=depth, general=general, utf8=True)
    took = fast_batches(hip) - before
    print(f"{case.name} {jt} depth {depth} general {general}: fast batches {took}, eligible {want} of {len(case.rbs)}")
    assert took == want
    if (jt, general) in case.runs:
        assert 0 < want < len(case.rbs)
    same_batches(got, exp)
    same_batches(got, sync)
    before = fast_batches(hip)
    off = run(hip, case, jt, depth=depth, general=general, utf8=False)
    assert fast_batches(hip) - before == cases.count_eligible(case, jt, general, utf8=False) == 0  # (today: a Utf8 column, no kernel)
    same_batches(off, exp)


@pytest.mark.parametrize("depth", [1, 8])
@pytest.mark.parametrize("form", cases.FORMS)
@pytest.mark.parametrize("jt", cases.JOIN_TYPES)
def test_join_types_and_table_forms(hip, oracle, jt, form, depth):
    """every join type over the direct-address table, the 16-byte-slot table, dd_table and the slot table with runs, with
    async_general on and off: two Utf8 columns per side next to NULL-bearing fixed-width ones, empty / NULL (bytes underneath) /
    multi-byte strings, Lmax in the last build row, probe offsets that start at 5, probe rows without partner (Right / Full: NULL
    and no bytes in the build columns), sizes 0 .. 4096 (kept whole) and 5000 / NULL probe keys (synchronous)"""
    case = cases.form_case(form)
    for general in (True, False):
        check_case(hip, oracle, case, jt, depth, general)


@pytest.mark.parametrize("jt", cases.JOIN_TYPES)
def test_chunks_running_base_and_end_offset(hip, oracle, jt):
    """M = 4 and every probe row hits: 1024, 2048 (exact multiples of the 1024-row chunk) and 2800 (three chunks) output rows;
    one build column of only empty strings (Lmax = 0)"""
    case = cases.chunk_case()
    exp, _ = reference_streams(hip, oracle, case, jt)
    assert [b.num_rows for b in exp[:3]] == [1024, 2048, 2800]
    check_case(hip, oracle, case, jt, 2, True)


@pytest.mark.parametrize("jt", cases.JOIN_TYPES)
def test_empty_and_all_null_string_columns(hip, oracle, jt):
    case = cases.empty_strings_case()
    for general in (True, False):
        check_case(hip, oracle, case, jt, 3, general)


def test_adjacent_utf8_columns_without_nulls(hip, oracle):
    """sa_probe_kernel<true>, 65 and 1025 rows: two Utf8 build columns and two Utf8 probe columns side by side, none with a NULL
    (tests/async_utf8_cases.py, adjacent_case: the route from one Utf8 column to the next without a bitmap pass between them)"""
    case = cases.adjacent_case()
    assert all(c.null_count == 0 for b in [case.lb] + case.rbs for c in b.columns) and [b.num_rows for b in case.rbs[:2]] == [65, 1025]
    check_case(hip, oracle, case, "inner", 1, False)


@pytest.mark.parametrize("jt", ["inner", "right"])
def test_byte_bound(hip, oracle, jt):
    """a 200-byte build string: 4096 probe rows exceed SA_AREA by construction (synchronous); the largest batch under the bound
    takes the kernel — also when every row gathers the 200-byte string, the reservation used to the last byte — one row more
    does not"""
    case = cases.bound_case()
    general = jt != "inner"
    exp, _ = reference_streams(hip, oracle, case, jt)
    for k, b in enumerate(case.rbs):  # batch by batch: WHICH batch took the kernel, not only how many
        before = fast_batches(hip)
        got = run(hip, case, jt, depth=1, general=general, utf8=True, rbs=[b])
        assert fast_batches(hip) - before == (1 if k in (1, 3) else 0), (jt, k)
        same_batches(got[:1], exp[k:k + 1])
    check_case(hip, oracle, case, jt, 2, general)


def test_employee_join_department_from_the_reference_csv(hip, oracle):
    """`employee JOIN department ON department_id = id` over tests/golden/csv (Utf8 and Int64 columns, cast as
    test_async_filter_over_the_reference_csv_table does): the oracle's batch, through the one-launch kernel"""
    import pyarrow.csv as pacsv
    root = os.path.dirname(os.path.abspath(__file__))

    def table(name):
        t = pacsv.read_csv(os.path.join(root, "golden", "csv", name))
        t = t.cast(pa.schema([pa.field(f.name, pa.int64() if pa.types.is_integer(f.type) else pa.string()) for f in t.schema]))
        return t.combine_chunks().to_batches()[0]
    emp, dep = table("employee.csv"), table("department.csv")
    cond = JoinCondition([(InputRef(emp.schema.names.index("department_id")), InputRef(dep.schema.names.index("id")))])
    sch = join_schema(emp, dep)
    for jt, general in (("inner", False), ("left", True)):
        exp = list(HashJoinExecutor(oracle, [emp], [dep], jt, cond, sch, emp.num_columns).execute())
        before = fast_batches(hip)
        got = list(HashJoinExecutor(hip, [emp], [dep], jt, cond, sch, emp.num_columns, depth=2, async_general=general, async_utf8=True).execute())
        assert fast_batches(hip) - before == 1
        same_batches(got, exp)
        assert got[0].num_rows == 3 and "Engineering" in got[0].column(emp.num_columns + 1).to_pylist()
        before = fast_batches(hip)
        off = list(HashJoinExecutor(hip, [emp], [dep], jt, cond, sch, emp.num_columns, depth=2, async_general=general).execute())
        assert fast_batches(hip) == before
        same_batches(off, exp)


@pytest.mark.parametrize("seed", cases.FUZZ_SEEDS)
def test_fuzz_async_join_utf8(hip, oracle, seed):
    case, jt, general, depth = cases.fuzz_case(seed)
    exp = run(oracle, case, jt)
    want = cases.count_eligible(case, jt, general)
    before = fast_batches(hip)
    got = run(hip, case, jt, depth=depth, general=general, utf8=True)
    took = fast_batches(hip) - before
    print(f"fuzz {seed} {jt} general {general} depth {depth}: fast batches {took}, eligible {want} of {len(case.rbs)}")
    assert took == want
    same_batches(got, exp)
    same_batches(got, run(hip, case, jt))
    before = fast_batches(hip)
    off = run(hip, case, jt, depth=depth, general=general, utf8=False)
    assert fast_batches(hip) - before == cases.count_eligible(case, jt, general, utf8=False)
    same_batches(off, exp)


def test_switch_semantics_and_the_fast_path_hook(hip, oracle, monkeypatch):
    """the setter's calling rules are those of sqlrs_hash_join_set_async_general; SQLRS_ASYNC_FAST=0 (a hook: the suite runs
    under SQLRS_HOOKS=1) sends every batch through the synchronous operator and the stream stays the same"""
    case = cases.form_case("dup_dense")
    exp, _ = reference_streams(hip, oracle, case, "left")
    ex = HashJoinExecutor(hip, [case.lb], [], "left", case.cond, join_schema(case.lb, case.rbs[0]), case.lb.num_columns)
    h, keep = ex._create()
    try:
        setter = hip.fn("hash_join_set_async_utf8")
        assert setter(h, 1) == abi.OK and setter(h, 0) == abi.OK and setter(h, 1) == abi.OK
        b = abi.as_batch(case.lb)
        hip.check(hip.fn("hash_join_build_push")(h, b.ptr))
        hip.check(hip.fn("hash_join_build_finish")(h))
        assert setter(h, 1) == abi.OK  # (still before the first probe call)
        rb = abi.as_batch(case.rbs[0])
        t = C.c_void_p()
        hip.check(hip.fn("hash_join_probe_push_async")(h, rb.ptr, C.byref(t)))
        assert setter(h, 0) == abi.ERR_INTERNAL and setter(h, 1) == abi.ERR_INTERNAL
        out = C.POINTER(abi.Batch)()
        hip.check(hip.fn("batch_wait")(t, C.byref(out)))
        hip.fn("batch_release")(out)
    finally:
        hip.fn("hash_join_destroy")(h)
    monkeypatch.setenv("SQLRS_ASYNC_FAST", "0")
    before = fast_batches(hip)
    got = run(hip, case, "left", depth=2, general=True, utf8=True)
    assert fast_batches(hip) == before
    same_batches(got, exp)
