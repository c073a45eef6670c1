"""sqlrs_hash_join_set_async_filter: a join WITH a join filter through ONE launch per probe batch of
sqlrs_hash_join_probe_push_async — the filter evaluated on the joined row inside sa_probe_kernel<., true> /
sa_probe_general_kernel<., true> (csrc/join_async.hip) with apply_join_filter's semantics.  The async stream must be the synchronous
stream and the oracle's, batch for batch, the tail batch of Left / Full included; which batches take a kernel is the rule of
include/sqlrs_hip.h, restated in tests/async_filter_cases.py."""
import ctypes as C

import pytest

import async_filter_cases as fc
from sqlrs_amd import abi
from sqlrs_amd.executor import FilterExecutor, HashJoinExecutor, _emit
from sqlrs_amd.expr import Constant, InputRef
from test_gpu_async import fast_batches, same_batches
from test_gpu_parity import join_schema

pytestmark = pytest.mark.gpu


def run(be, case, rbs, jt, filt, **kw):
    return list(HashJoinExecutor(be, [case.lb], rbs, jt, case.cond(filt), join_schema(case.lb, case.rbs[0]), case.lb.num_columns, **kw).execute())


_streams = {}


def reference_streams(oracle, hip, case, jt, filt):
    """the oracle's stream and the synchronous hip stream of a case: computed once, shared by the depths"""
    key = (case.name, jt, filt)
    if key not in _streams:
        exp = run(oracle, case, case.rbs, jt, filt)
        same_batches(run(hip, case, case.rbs, jt, filt), exp)
        _streams[key] = exp
    return _streams[key]


@pytest.mark.parametrize("depth", [1, 8])
@pytest.mark.parametrize("filt", ["both", "right_only", "left_only", "none"])
@pytest.mark.parametrize("form", fc.FORMS)
@pytest.mark.parametrize("jt", fc.JOIN_TYPES)
def test_parity_with_the_oracle_and_the_synchronous_stream(hip, oracle, jt, form, filt, depth):
    case = fc.form_case(form)
    exp = reference_streams(oracle, hip, case, jt, filt)
    want = fc.count_eligible(case, case.rbs, jt, case.filters[filt])
    before = fast_batches(hip)
    got = run(hip, case, case.rbs, jt, filt, depth=depth, async_general=True, async_filter=True)
    took = fast_batches(hip) - before
    print(f"{jt} {form} {filt} depth {depth}: fast batches {took}, eligible {want} of {len(case.rbs)}")
    assert took == want and 0 < want < len(case.rbs)
    same_batches(got, exp)
    before = fast_batches(hip)
    off = run(hip, case, case.rbs, jt, filt, depth=depth, async_general=True, async_filter=False)
    assert fast_batches(hip) == before
    same_batches(off, exp)


@pytest.mark.parametrize("filt", ["both", "none", "arith"])
@pytest.mark.parametrize("form", ["unique_dense", "unique_sparse"])
def test_inner_unique_route_with_only_the_filter_switch(hip, oracle, form, filt):
    """general off: sa_probe_kernel<., true> takes the eligible batches of an Inner join over unique keys, and nothing of a Left join"""
    case = fc.form_case(form)
    want = fc.count_eligible(case, case.rbs, "inner", case.filters[filt], general=False)
    before = fast_batches(hip)
    got = run(hip, case, case.rbs, "inner", filt, depth=3, async_filter=True)
    assert fast_batches(hip) - before == want and 0 < want < len(case.rbs)
    same_batches(got, reference_streams(oracle, hip, case, "inner", filt))
    before = fast_batches(hip)
    got = run(hip, case, case.rbs[:4], "left", filt, depth=3, async_filter=True)
    assert fast_batches(hip) == before
    same_batches(got, run(oracle, case, case.rbs[:4], "left", filt))


@pytest.mark.parametrize("filt", ["both", "none"])
@pytest.mark.parametrize("jt", ["inner", "full"])
def test_skew_compacts_sixteen_chunks_in_pair_order(hip, oracle, jt, filt):
    """1024 probe rows x 16 build rows: 16384 candidates, the kept ones compacted across 16 chunks of phase A with a running base;
    probe-row major, build insertion order minor"""
    case = fc.skew_case()
    exp = run(oracle, case, case.rbs, jt, filt)
    before = fast_batches(hip)
    got = run(hip, case, case.rbs, jt, filt, depth=2, async_general=True, async_filter=True)
    assert fast_batches(hip) - before == 2 == fc.count_eligible(case, case.rbs, jt, case.filters[filt])
    same_batches(got, exp)
    if filt == "both" and jt == "inner":
        assert 1024 < exp[0].num_rows < fc.SA_MAX_OUT_ROWS


@pytest.mark.parametrize("filt", ["arith", "all"])
@pytest.mark.parametrize("jt", ["inner", "full"])
def test_arith_and_all_over_duplicate_sparse_keys(hip, oracle, jt, filt):
    case = fc.form_case("dup_sparse")
    want = fc.count_eligible(case, case.rbs, jt, case.filters[filt])
    before = fast_batches(hip)
    got = run(hip, case, case.rbs, jt, filt, depth=4, async_general=True, async_filter=True)
    assert fast_batches(hip) - before == want and 0 < want < len(case.rbs)
    same_batches(got, reference_streams(oracle, hip, case, jt, filt))


class RawJoin:
    """one join through the raw ABI (build side pushed and finished), for call orders the executor does not produce"""

    def __init__(self, be, case, jt, filt, **flags):
        self.be, self.names = be, list(join_schema(case.lb, case.rbs[0]).names)
        ex = HashJoinExecutor(be, [case.lb], [], jt, case.cond(filt), join_schema(case.lb, case.rbs[0]), case.lb.num_columns, **flags)
        self.h, self.keep = ex._create()
        b = abi.as_batch(case.lb)
        be.check(be.fn("hash_join_build_push")(self.h, b.ptr))
        be.check(be.fn("hash_join_build_finish")(self.h))

    def push(self, rb):
        b = abi.as_batch(rb)
        out = C.POINTER(abi.Batch)()
        self.be.check(self.be.fn("hash_join_probe_push")(self.h, b.ptr, abi.MEM_HOST, C.byref(out)))
        return _emit(self.be, out, abi.MEM_HOST, self.names)

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

    def set_filter(self, on):
        return self.be.fn("hash_join_set_async_filter")(self.h, on)

    def close(self):
        self.be.fn("hash_join_destroy")(self.h)


@pytest.mark.parametrize("form", ["unique_dense", "dup_sparse"])
def test_divide_by_zero_is_that_tickets_error_and_marks_nothing(hip, oracle, form):
    """`r.w / l.d = 1`, one matched valid pair with d = 0 in the third batch: the stream raises the evaluator's error there, the
    batches before it are delivered; batch by batch on a Left join the failed batch leaves no visited mark and later tickets
    are unaffected — the tail equals the oracle's for the same sequence"""
    case = fc.form_case(form)
    rbs, k = fc.div0_batches(case)
    for jt in ("inner", "left", "full"):
        exp_before = run(oracle, case, rbs[:k], jt, "div0")[:k]
        for kw in ({}, {"depth": 1, "async_general": True, "async_filter": True}):
            got = []
            with pytest.raises(abi.ExecutorError) as ei:
                for b in HashJoinExecutor(hip, [case.lb], rbs, jt, case.cond("div0"), join_schema(case.lb, rbs[0]), case.lb.num_columns, **kw).execute():
                    got.append(b)
            assert ei.value.status == abi.ERR_ARROW and "ivide by zero" in str(ei.value), (jt, kw)
            same_batches(got, exp_before)

    def sequence(j, push):
        out = []
        for i, b in enumerate(rbs):
            if i == k:
                with pytest.raises(abi.ExecutorError) as ei:
                    push(j, b)
                assert ei.value.status == abi.ERR_ARROW and "ivide by zero" in str(ei.value)
            else:
                out.append(push(j, b))
        out.append(j.finish())
        return out
    jo = RawJoin(oracle, case, "left", "div0")
    try:
        exp = sequence(jo, lambda j, b: j.push(b))
    finally:
        jo.close()
    before = fast_batches(hip)
    jh = RawJoin(hip, case, "left", "div0", async_general=True, async_filter=True)
    try:
        got = sequence(jh, lambda j, b: j.wait(j.push_async(b)))
    finally:
        jh.close()
    assert fast_batches(hip) - before == len(rbs)  # (the failing batch took the kernel too)
    same_batches(got, exp)
    assert got[-1].num_rows > 0


def test_utf8_payload_columns_next_to_the_filter(hip, oracle):
    """Utf8 payload columns on both sides with the three switches on; a filter that READS a Utf8 column does not compile: the
    synchronous operator takes every batch"""
    case = fc.utf8_case()
    flags = dict(async_general=True, async_utf8=True, async_filter=True)
    for jt in fc.JOIN_TYPES:
        exp = run(oracle, case, case.rbs, jt, "both")
        want = fc.count_eligible(case, case.rbs, jt, case.filters["both"], utf8=True)
        before = fast_batches(hip)
        got = run(hip, case, case.rbs, jt, "both", depth=3, **flags)
        assert fast_batches(hip) - before == want and 0 < want < len(case.rbs), jt
        same_batches(got, exp)
        assert fc.count_eligible(case, case.rbs, jt, case.filters["utf8_ref"], utf8=True) == 0
        before = fast_batches(hip)
        got = run(hip, case, case.rbs, jt, "utf8_ref", depth=3, **flags)
        assert fast_batches(hip) == before
        same_batches(got, run(oracle, case, case.rbs, jt, "utf8_ref"))
    before = fast_batches(hip)  # the Utf8 switch off: a batch with Utf8 columns is not eligible, filter switch or not
    got = run(hip, case, case.rbs[:2], "inner", "both", depth=3, async_general=True, async_filter=True)
    assert fast_batches(hip) == before
    same_batches(got, run(oracle, case, case.rbs[:2], "inner", "both"))


def test_finish_with_tickets_outstanding(hip, oracle):
    """a Left join with a filter at depth 8: eight batches pushed, none waited for, sqlrs_hash_join_finish first — the tail holds
    exactly the build rows no KEPT pair marked"""
    case = fc.form_case("dup_dense")
    rbs = [b for b in case.rbs if 63 <= b.num_rows <= 1025 and b.column(1).null_count == 0]
    assert len(rbs) == 9 and all(fc.eligible(case, b, "left", case.filters["both"]) for b in rbs)
    rbs = rbs[:8]
    exp = run(oracle, case, rbs, "left", "both")
    before = fast_batches(hip)
    j = RawJoin(hip, case, "left", "both", async_general=True, async_filter=True)
    try:
        tickets = [j.push_async(b) for b in rbs]
        assert fast_batches(hip) - before == len(rbs) == 8
        tail = j.finish()
        got = [j.wait(t) for t in tickets]
    finally:
        j.close()
    same_batches(got + [tail], exp)


def test_switch_semantics(hip, oracle):
    case = fc.form_case("unique_dense")
    rbs = case.rbs[:3]
    exp = run(oracle, case, rbs, "inner", "both")
    assert hip.fn("hash_join_set_async_filter")(None, 1) == abi.ERR_INTERNAL
    for first in ("push", "push_async"):  # after the first probe call of either kind: an error, the setting stays
        j = RawJoin(hip, case, "inner", "both")
        try:
            assert j.set_filter(1) == abi.OK and j.set_filter(0) == abi.OK and j.set_filter(1) == abi.OK
            before = fast_batches(hip)
            got = [j.push(rbs[0])] if first == "push" else [j.wait(j.push_async(rbs[0]))]
            assert j.set_filter(0) == abi.ERR_INTERNAL and j.set_filter(1) == abi.ERR_INTERNAL
            got += [j.wait(j.push_async(b)) for b in rbs[1:]]
            assert fast_batches(hip) - before == (2 if first == "push" else 3)
        finally:
            j.close()
        same_batches(got, exp)


def test_filter_operator_then_filtered_join_on_one_ctx(hip, oracle):
    """Filter -> filtered-join probe, both through push_async on ONE ctx at depth 3: the group flush between two operators keeps
    the tickets in order"""
    case = fc.form_case("dup_dense")
    pred = InputRef(2) > Constant(0, abi.INT64)  # r.w > 0 on the probe batches
    bs = [b for b in case.rbs if b.num_rows <= 1025 and b.column(1).null_count == 0]

    def plan(be, d, **flags):
        f = FilterExecutor(be, pred, bs, depth=d).execute()
        return list(HashJoinExecutor(be, [case.lb], f, "full", case.cond("both"), join_schema(case.lb, bs[0]), case.lb.num_columns, depth=d, **flags).execute())
    before = fast_batches(hip)
    got = plan(hip, 3, async_general=True, async_filter=True)
    assert fast_batches(hip) - before == 2 * len(bs)
    same_batches(got, plan(oracle, 0))
