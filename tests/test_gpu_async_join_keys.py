"""sqlrs_hash_join_set_async_keys: NULL probe keys, Utf8 keys and keys of 2 to 4 columns through both one-launch kernels of
sqlrs_hash_join_probe_push_async (the KEYS instantiations of sa_probe_kernel / sa_probe_general_kernel, sa_probe_key, csrc/join_async.hip).
The async stream must be the synchronous stream and the oracle's, batch for batch (exact Arrow equality), the tail batch of Left /
Full included; which batches take a kernel is the rule of include/sqlrs_hip.h as tests/async_keys_cases.py restates it, and the
counts it gives are the ones worked out by hand there.  With the switch off the count is what it was."""
import ctypes as C
import os

import pyarrow as pa
import pytest

import async_keys_cases as cases
from sqlrs_amd import abi
from sqlrs_amd.executor import HashJoinExecutor, _emit
from sqlrs_amd.expr import InputRef, JoinCondition
from test_gpu_async import fast_batches, same_batches
from test_gpu_parity import join_schema

pytestmark = pytest.mark.gpu


def run(be, case, jt, depth=0, general=False, keys=False, utf8=True, filt=True, rbs=None):
    rbs = case.rbs if rbs is None else rbs
    sch = join_schema(case.lb, case.rbs[0])
    return list(HashJoinExecutor(be, [case.lb], rbs, jt, case.cond, sch, case.lb.num_columns, depth=depth, async_general=general, async_utf8=utf8,
                                 async_filter=filt, async_keys=keys).execute())


_ref_cache = {}


def reference_streams(hip, oracle, case, jt):
    """the oracle's stream and the synchronous probe_push stream of one case and join type: computed once, shared, not changed"""
    key = (case.name, jt)
    if key not in _ref_cache:
        _ref_cache[key] = (run(oracle, case, jt), run(hip, case, jt))
        same_batches(_ref_cache[key][1], _ref_cache[key][0])
    return _ref_cache[key]


def check_case(hip, oracle, case, jt, depth, general, **sw):
    """switch on: exactly the batches the rule admits take a kernel — the hand count — and the stream is the reference's; switch
    off: the batches the rule as it was admits, and the same stream"""
    exp, sync = reference_streams(hip, oracle, case, jt)
    want = cases.count_eligible(case, jt, general, **sw)
    before = fast_batches(hip)
    got = run(hip, case, jt, depth=depth, general=general, keys=True, **sw)
    took = fast_batches(hip) - before
    print(f"{case.name} {jt} depth {depth} general {general} {sw}: fast batches {took}, eligible {want} of {len(case.rbs)}")
    assert took == want
    if case.want is not None and not sw:
        assert want == case.want[(jt, general)]
    same_batches(got, exp)
    same_batches(got, sync)
    before = fast_batches(hip)
    off = run(hip, case, jt, depth=depth, general=general, keys=False, **sw)
    assert fast_batches(hip) - before == cases.count_eligible(case, jt, general, keys=False, **sw)
    same_batches(off, exp)


@pytest.mark.parametrize("depth", [1, 8])
@pytest.mark.parametrize("jt", cases.JOIN_TYPES)
@pytest.mark.parametrize("e", cases.EXACT, ids=lambda e: "_".join(map(str, e)))
def test_null_probe_keys_exact_mode(hip, oracle, e, jt, depth):
    """int64 / int32 / float64 keys over the direct-address table, the slot table, dd_table and the slot table with runs; 0, 1 and 3
    build rows with a NULL key (3: M = 3); NULL probe keys in the first row, the last row, rows 63 / 64, every row, none under a
    bitmap; the value of an existing build key under NULL slots; Right / Full: a NULL key without partner emits (NULL, r)"""
    case = cases.exact_case(*e)
    for general in (True, False):
        check_case(hip, oracle, case, jt, depth, general)


@pytest.mark.parametrize("depth", [1, 8])
@pytest.mark.parametrize("jt", cases.JOIN_TYPES)
@pytest.mark.parametrize("dup", [False, True], ids=["unique", "dup"])
def test_utf8_key(hip, oracle, dup, jt, depth):
    """a Utf8 key, matched by hash: the empty string versus NULL, a string and its proper prefix, a last-byte difference, 1- / 8- / 9-
    / 200-byte strings, multi-byte UTF-8, bytes under NULL slots, probe offsets from 5; unique build keys and every key four times"""
    case = cases.utf8_case(dup)
    for general in (True, False):
        check_case(hip, oracle, case, jt, depth, general)


@pytest.mark.parametrize("depth", [1, 8])
@pytest.mark.parametrize("jt", cases.JOIN_TYPES)
@pytest.mark.parametrize("name", list(cases.MULTI) + ["unique_pair", "mismatch"])
def test_two_to_four_key_columns(hip, oracle, name, jt, depth):
    """(int64, int64), (int32, Utf8), (float64, int64, Utf8, int32): a NULL in every position, swapped values (one hash); the
    Inner / unique route in hash mode (unique_pair); an int32 probe column against an int64 build column finds nothing (mismatch)"""
    case = cases.multi_case(name) if name in cases.MULTI else cases.unique_pair_case() if name == "unique_pair" else cases.mismatch_case()
    for general in (True, False):
        check_case(hip, oracle, case, jt, depth, general)
    if name == "mismatch":
        assert all(b.num_rows == 0 for b in reference_streams(hip, oracle, case, "inner")[0])


@pytest.mark.parametrize("depth", [1, 8])
@pytest.mark.parametrize("jt", cases.JOIN_TYPES)
def test_with_the_join_filter_inside_the_kernel(hip, oracle, jt, depth):
    """async_filter: `l.x > r.v` over payload columns; the NULL-key probe rows meet the NULL build row and only the filter keeps
    them out.  With the filter switch off the filtered join takes no kernel"""
    case = cases.filter_case()
    for general in (True, False):
        check_case(hip, oracle, case, jt, depth, general)
    check_case(hip, oracle, case, jt, depth, True, filt=False)


def test_divide_by_zero_on_a_null_key_candidate(hip, oracle):
    """`l.x / r.v > 0`: the second batch's NULL-key row meets the NULL build row with v = 0 — the evaluator's error at that ticket,
    in the synchronous stream and in the async one; the batch before it is delivered"""
    case = cases.div0_case()
    for jt in ("inner", "left"):
        exp = run(oracle, case, jt, rbs=case.rbs[:1])[:1]
        for kw in ({}, {"depth": 1, "general": True, "keys": True}):
            got = []
            with pytest.raises(abi.ExecutorError) as ei:
                for b in HashJoinExecutor(hip, [case.lb], case.rbs, jt, case.cond, join_schema(case.lb, case.rbs[0]), case.lb.num_columns, depth=kw.get("depth", 0),
                                          async_general=kw.get("general", False), async_filter=True, async_keys=kw.get("keys", False)).execute():
                    got.append(b)
            assert ei.value.status == abi.ERR_ARROW and "ivide by zero" in str(ei.value), (jt, kw)
            same_batches(got, exp)


@pytest.mark.parametrize("jt", cases.JOIN_TYPES)
def test_utf8_key_needs_the_utf8_switch(hip, oracle, jt):
    """async_utf8 off: a Utf8 key (or a Utf8 column anywhere) is synchronous — predicted count 0"""
    for case in (cases.utf8_case(False), cases.multi_case("i32_str")):
        assert cases.count_eligible(case, jt, True, utf8=False) == 0
        check_case(hip, oracle, case, jt, 2, True, utf8=False)


@pytest.mark.parametrize("jt", ["left", "inner"])
def test_byte_bound(hip, oracle, jt):
    """M = 2 and a 100-byte build string: the largest batch the rule admits uses the output area to within two rows' worth, the
    batch one row larger is synchronous — batch by batch: WHICH batch took the kernel"""
    case = cases.bound_case()
    exp, _ = reference_streams(hip, oracle, case, jt)
    for k, b in enumerate(case.rbs):
        before = fast_batches(hip)
        got = run(hip, case, jt, depth=1, general=True, keys=True, rbs=[b])
        assert fast_batches(hip) - before == (0 if k == 1 else 1), (jt, k)
        same_batches(got[:1], exp[k:k + 1])
    check_case(hip, oracle, case, jt, 2, True)


@pytest.mark.parametrize("what", ["five", "bool", "expr"])
def test_keys_that_stay_synchronous(hip, oracle, what):
    """five key columns, a Boolean key, a key expression that is not a bare column reference: no kernel, the same stream"""
    case = cases.refused_case(what)
    for jt in ("inner", "full"):
        check_case(hip, oracle, case, jt, 2, True)


@pytest.mark.parametrize("seed", cases.FUZZ_SEEDS)
def test_fuzz_async_join_keys(hip, oracle, seed):
    case, jt, general, depth = cases.fuzz_case(seed)
    check_case(hip, oracle, case, jt, depth, general)


class RawJoin:
    """one join through the raw ABI (build side pushed and finished), for call orders the executor does not produce"""

    def __init__(self, be, case, jt, **flags):
        sch = join_schema(case.lb, case.rbs[0])
        self.be, self.names = be, list(sch.names)
        self.h, self.keep = HashJoinExecutor(be, [case.lb], [], jt, case.cond, sch, case.lb.num_columns, **flags)._create()
        b = abi.as_batch(case.lb)
        be.check(be.fn("hash_join_build_push")(self.h, b.ptr))
        be.check(be.fn("hash_join_build_finish")(self.h))

    def push_async(self, rb):
        b = abi.as_batch(rb)
        t = C.c_void_p()
        self.be.check(self.be.fn("hash_join_probe_push_async")(self.h, b.ptr, C.byref(t)))
        return t

    def wait(self, t):
        out = C.POINTER(abi.Batch)()
        self.be.check(self.be.fn("batch_wait")(t, C.byref(out)))
        return _emit(self.be, out, abi.MEM_HOST, self.names)

    def finish(self):
        out = C.POINTER(abi.Batch)()
        self.be.check(self.be.fn("hash_join_finish")(self.h, abi.MEM_HOST, C.byref(out)))
        return _emit(self.be, out, abi.MEM_HOST, self.names)

    def close(self):
        self.be.fn("hash_join_destroy")(self.h)


@pytest.mark.parametrize("e", [("i64", "unique_sparse", 3), ("i64", "unique_dense", 1)], ids=lambda e: "_".join(map(str, e)))
def test_finish_before_wait_with_null_probe_keys(hip, oracle, e):
    """Left join, NULL probe keys that mark the NULL build rows visited: every batch pushed, none waited for, sqlrs_hash_join_finish
    first — it waits for the probe kernels' marks — then the tickets: the tail and the batches are the oracle's"""
    case = cases.exact_case(*e)
    rbs = case.rbs[:9]
    exp_tail = run(oracle, case, "left", rbs=rbs)
    before = fast_batches(hip)
    j = RawJoin(hip, case, "left", async_general=True, async_keys=True)
    try:
        tickets = [j.push_async(b) for b in rbs]
        assert fast_batches(hip) - before == len(rbs)
        tail = j.finish()
        got = [j.wait(t) for t in tickets]
    finally:
        j.close()
    same_batches(got + [tail], exp_tail)
    nulls_in_tail = [k for k in tail.column(0).to_pylist() if k is None]
    assert not nulls_in_tail  # (the NULL build rows were visited by NULL probe keys)


def test_switch_semantics(hip):
    """the setter's calling rules are those of sqlrs_hash_join_set_async_general"""
    case = cases.unique_pair_case()
    setter = hip.fn("hash_join_set_async_keys")
    assert setter(None, 1) == abi.ERR_INTERNAL
    j = RawJoin(hip, case, "left")
    try:
        assert setter(j.h, 1) == abi.OK and setter(j.h, 0) == abi.OK and setter(j.h, 1) == abi.OK  # (after build_finish, before the first probe call)
        j.wait(j.push_async(case.rbs[2]))
        assert setter(j.h, 0) == abi.ERR_INTERNAL and setter(j.h, 1) == abi.ERR_INTERNAL
    finally:
        j.close()


def _csv_table(name):
    import pyarrow.csv as pacsv
    t = pacsv.read_csv(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "csv", name))
    t = t.cast(pa.schema([pa.field(f.name, pa.int64() if pa.types.is_integer(f.type) else pa.string()) for f in t.schema]))
    return t.combine_chunks().to_batches()[0]


@pytest.mark.parametrize("jt", cases.JOIN_TYPES)
def test_the_reference_tables_join_on_a_utf8_key_and_on_a_key_with_a_null(hip, oracle, jt):
    """tests/golden/csv: `employee JOIN state ON state_code = state` (a Utf8 key; CO twice on the build side) and `department JOIN
    employee ON id = department_id` with employee as the probe side, whose department_id holds a NULL: one fast batch each, equal
    to the oracle"""
    emp, state, dep = _csv_table("employee.csv"), _csv_table("state.csv"), _csv_table("department.csv")
    assert emp.column(emp.schema.names.index("department_id")).null_count == 1
    for lb, rb, lk, rk in ((emp, state, "state", "state_code"), (dep, emp, "id", "department_id")):
        cond = JoinCondition([(InputRef(lb.schema.names.index(lk)), InputRef(rb.schema.names.index(rk)))])
        sch = join_schema(lb, rb)
        exp = list(HashJoinExecutor(oracle, [lb], [rb], jt, cond, sch, lb.num_columns).execute())
        before = fast_batches(hip)
        got = list(HashJoinExecutor(hip, [lb], [rb], jt, cond, sch, lb.num_columns, depth=2, async_general=True, async_utf8=True, async_keys=True).execute())
        assert fast_batches(hip) - before == 1, (lk, jt)
        same_batches(got, exp)
        assert got[0].num_rows >= 3
        before = fast_batches(hip)
        off = list(HashJoinExecutor(hip, [lb], [rb], jt, cond, sch, lb.num_columns, depth=2, async_general=True, async_utf8=True).execute())
        assert fast_batches(hip) == before
        same_batches(off, exp)
