"""sqlrs_hash_join_set_async_general: Left / Right / Full joins and build sides with duplicate keys through ONE launch per probe
batch of sqlrs_hash_join_probe_push_async (sa_probe_general_kernel, csrc/join_async.hip).  The async stream must be the synchronous
stream and the oracle's, batch for batch, the tail batch of Left / Full included; which batches take the kernel is the rule of
include/sqlrs_hip.h, restated here from the batch, the build side's true M and the header's constants."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest

from sqlrs_amd import abi
from sqlrs_amd.executor import HashJoinExecutor, _emit
from sqlrs_amd.expr import InputRef, JoinCondition
from test_gpu_async import fast_batches, same_batches
from test_gpu_parity import join_schema

pytestmark = pytest.mark.gpu

SA_MAX_ROWS, SA_MAX_OUT_ROWS, SA_AREA, SA_MAX_COLS = 4096, 16384, 512 * 1024, 12  # (sqlrs_hip.h / csrc/small_async.hpp)


def up64(x):
    return (x + 63) & ~63


def max_run(lb, key_col):
    """M: the most build rows that share one key"""
    k = lb.column(key_col).to_numpy(zero_copy_only=False)
    return int(np.unique(k, return_counts=True)[1].max()) if len(k) else 1


def out_bytes(lb, rb, out_rows):
    widths = [4 if pa.types.is_int32(f.type) else 8 for f in list(lb.schema) + list(rb.schema)]
    return 64 + sum(up64(w * out_rows) + up64((out_rows + 7) // 8) for w in widths)


def eligible(lb, rb, rkey, m):
    """the header's rule for one probe batch with the switch on (fixed-width columns, one INPUT_REF key, no filter: by construction)"""
    rows = rb.num_rows
    if rows > SA_MAX_ROWS or rb.column(rkey).null_count or lb.num_columns + rb.num_columns > SA_MAX_COLS:
        return False
    return rows * m <= SA_MAX_OUT_ROWS and out_bytes(lb, rb, rows * m) <= SA_AREA


def todays_fast(lb, rbs, rkey, jt, m):
    """batches the switch-off path takes: Inner over unique build keys only"""
    if jt != "inner" or m != 1:
        return 0
    return sum(1 for b in rbs if b.num_rows <= SA_MAX_ROWS and b.column(rkey).null_count == 0)


def run(be, lb, rbs, jt, cond, depth=0, general=False):
    sch = join_schema(lb, rbs[0])
    return list(HashJoinExecutor(be, [lb], rbs, jt, cond, sch, lb.num_columns, depth=depth, async_general=general).execute())


FORMS = ["unique_dense", "unique_sparse", "dup_dense", "dup_sparse"]
_case_cache = {}


def form_case(form):
    """build side, probe batches (shared by the join types and depths: built once)"""
    if form in _case_cache:
        return _case_cache[form]
    rng = np.random.default_rng(17 + FORMS.index(form))
    conv = (lambda x: x.astype(np.int64) * 7919 - 5) if form.endswith("sparse") else (lambda x: x.astype(np.int64))
    if form.startswith("unique"):
        nb = 2000
        raw = rng.permutation(3000)[:nb]  # (keys >= 2500 are never probed: unvisited build rows)
    else:
        nb = 3000
        raw = rng.integers(0, 2000, nb)
    lb = pa.RecordBatch.from_arrays([pa.array(conv(raw)), pa.array(rng.random(nb), mask=rng.random(nb) < 0.1),
                                     pa.array(np.arange(nb, dtype=np.int32))], names=["k", "x", "i"])
    rbs = []
    for rows in [1024] * 6 + [0, 1, 63, 64, 65, 1023, 2048, 5000]:
        rbs.append(pa.RecordBatch.from_arrays([pa.array(rng.random(rows), mask=rng.random(rows) < 0.2),
                                               pa.array(conv(rng.integers(0, 2500, rows)))], names=["v", "k"]))
    rbs.insert(3, pa.RecordBatch.from_arrays([pa.array(rng.random(1024)), pa.array(conv(rng.integers(0, 2500, 1024)), mask=rng.random(1024) < 0.1)],
                                             names=["v", "k"]))  # NULL probe keys: the synchronous operator inside the stream
    _case_cache[form] = (lb, rbs)
    return _case_cache[form]


_oracle_cache = {}


def oracle_stream(oracle, tag, lb, rbs, jt, cond):
    if tag not in _oracle_cache:
        _oracle_cache[tag] = run(oracle, lb, rbs, jt, cond)
    return _oracle_cache[tag]


@pytest.mark.parametrize("depth", [1, 8])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("jt", ["inner", "left", "right", "full"])
def test_join_types_and_table_forms(hip, oracle, jt, form, depth):
    """every join type over the direct-address table, the 16-byte-slot table, dd_table and the slot table with runs; NULLs in a
    build and a probe payload column, probe keys without partner, unvisited build rows; a batch with NULL probe keys and one of
    5000 rows take the synchronous operator inside the same stream"""
    lb, rbs = form_case(form)
    cond = JoinCondition([(InputRef(0), InputRef(1))])
    m = max_run(lb, 0)
    assert (m == 1) == form.startswith("unique")
    exp = oracle_stream(oracle, (jt, form), lb, rbs, jt, cond)
    before = fast_batches(hip)
    got = run(hip, lb, rbs, jt, cond, depth=depth, general=True)
    took = fast_batches(hip) - before
    want = sum(1 for b in rbs if eligible(lb, b, 1, m))
    print(f"{jt} {form} depth {depth}: M = {m}, fast batches {took}, eligible {want} of {len(rbs)}")
    assert took == want and 0 < want < len(rbs)
    same_batches(got, exp)
    same_batches(got, run(hip, lb, rbs, jt, cond))
    before = fast_batches(hip)
    off = run(hip, lb, rbs, jt, cond, depth=depth, general=False)
    assert fast_batches(hip) - before == todays_fast(lb, rbs, 1, jt, m)
    same_batches(off, exp)


def test_pair_order_under_skew(hip, oracle):
    """one key carried by 16 build rows: 1024 probe rows that all hit it emit 16384 rows — probe-row major, build insertion
    order minor (hash_join.rs:225-234)"""
    rng = np.random.default_rng(5)
    nb, hot = 1000, 77
    keys = np.arange(nb, dtype=np.int64)
    keys[rng.choice(np.setdiff1d(np.arange(nb), [hot]), 15, replace=False)] = hot  # 16 rows carry `hot`, scattered over the build side
    lb = pa.RecordBatch.from_arrays([pa.array(keys), pa.array(np.arange(nb, dtype=np.int32))], names=["k", "i"])
    rbs = [pa.RecordBatch.from_arrays([pa.array(np.full(rows, hot, dtype=np.int64)), pa.array(np.arange(rows, dtype=np.int32) + 100 * rows)],
                                      names=["k", "v"]) for rows in (1024, 64)]
    m = max_run(lb, 0)
    assert m == 16
    cond = JoinCondition([(InputRef(0), InputRef(0))])
    for jt in ("inner", "full"):
        exp = run(oracle, lb, rbs, jt, cond)
        assert [b.num_rows for b in exp[:2]] == [16384, 1024]
        for k, b in enumerate(rbs):
            before = fast_batches(hip)
            got = run(hip, lb, [b], jt, cond, depth=2, general=True)
            assert fast_batches(hip) - before == int(eligible(lb, b, 0, m)) == 1
            same_batches(got[:1], exp[k:k + 1])
        same_batches(run(hip, lb, rbs, jt, cond, depth=2, general=True), exp)


def test_capacity_boundary(hip, oracle):
    """rows x M == SA_MAX_OUT_ROWS is taken, one row more is not; the same at the byte bound of the slot's output area; a key
    carried by 5000 rows: no 1024-row batch is taken"""
    rng = np.random.default_rng(9)
    nk, m = 300, 8
    keys = np.repeat(np.arange(nk, dtype=np.int64), m)
    rng.shuffle(keys)
    cond = JoinCondition([(InputRef(0), InputRef(0))])
    # (a) the row bound: narrow columns, so that the bytes do not decide
    lb = pa.RecordBatch.from_arrays([pa.array(keys), pa.array(np.arange(nk * m, dtype=np.int32))], names=["k", "i"])
    assert max_run(lb, 0) == m
    rows_ok = SA_MAX_OUT_ROWS // m
    rbs = [pa.RecordBatch.from_arrays([pa.array(rng.integers(0, nk, rows)), pa.array(rng.integers(0, 9, rows).astype(np.int32))], names=["k", "v"])
           for rows in (rows_ok, rows_ok + 1)]
    assert out_bytes(lb, rbs[1], (rows_ok + 1) * m) <= SA_AREA and rows_ok + 1 <= SA_MAX_ROWS  # (only rows x M decides)
    assert [eligible(lb, b, 0, m) for b in rbs] == [True, False]
    # (b) the byte bound alone: ten 8-byte columns
    lb8 = pa.RecordBatch.from_arrays([pa.array(keys)] + [pa.array(rng.random(nk * m), mask=rng.random(nk * m) < 0.1) for _ in range(4)],
                                     names=["k", "a", "b", "c", "d"])

    def probe8(rows):
        return pa.RecordBatch.from_arrays([pa.array(rng.integers(0, nk, rows))] + [pa.array(rng.random(rows)) for _ in range(4)],
                                          names=["k", "p", "q", "r", "s"])
    one = probe8(1)
    rows8 = max(r for r in range(1, SA_MAX_ROWS) if out_bytes(lb8, one, r * m) <= SA_AREA)
    rbs8 = [probe8(rows8), probe8(rows8 + 1)]
    assert (rows8 + 1) * m < SA_MAX_OUT_ROWS  # (only the bytes decide)
    assert [eligible(lb8, b, 0, m) for b in rbs8] == [True, False]
    for jt in ("inner", "left"):
        for l, pair in ((lb, rbs), (lb8, rbs8)):
            exp = run(oracle, l, pair, jt, cond)
            for k, b in enumerate(pair):
                before = fast_batches(hip)
                got = run(hip, l, [b], jt, cond, depth=1, general=True)
                assert fast_batches(hip) - before == (1 if k == 0 else 0), (jt, l.num_columns, k)
                same_batches(got[:1], exp[k:k + 1])
            same_batches(run(hip, l, pair, jt, cond, depth=2, general=True), exp)
    # (c) one key 5000 times
    keys = np.concatenate([np.full(5000, 7, dtype=np.int64), np.arange(100, 600, dtype=np.int64)])
    lbh = pa.RecordBatch.from_arrays([pa.array(keys), pa.array(np.arange(len(keys), dtype=np.int32))], names=["k", "i"])
    pk = rng.integers(100, 700, (2, 1024))
    pk[:, 5] = 7  # (one probe row per batch meets the hot key)
    rbh = [pa.RecordBatch.from_arrays([pa.array(pk[i]), pa.array(rng.integers(0, 9, 1024).astype(np.int32))], names=["k", "v"]) for i in range(2)]
    assert not any(eligible(lbh, b, 0, max_run(lbh, 0)) for b in rbh)
    before = fast_batches(hip)
    got = run(hip, lbh, rbh, "left", cond, depth=2, general=True)
    assert fast_batches(hip) == before
    same_batches(got, run(oracle, lbh, rbh, "left", cond))


class RawJoin:
    """one join through the raw ABI (build side pushed and finished), for call orders the executor does not produce"""

    def __init__(self, be, lb, rb0, jt, cond, general):
        self.be, self.names = be, list(join_schema(lb, rb0).names)
        ex = HashJoinExecutor(be, [lb], [], jt, cond, join_schema(lb, rb0), lb.num_columns, async_general=general)
        self.h, self.keep = ex._create()
        b = abi.as_batch(lb)
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

    def set_general(self, on):
        return self.be.fn("hash_join_set_async_general")(self.h, on)

    def close(self):
        self.be.fn("hash_join_destroy")(self.h)


def dup_case(seed, nbatches=6):
    rng = np.random.default_rng(seed)
    nb = 3000
    lb = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 2000, nb)), pa.array(rng.random(nb), mask=rng.random(nb) < 0.1)], names=["k", "x"])
    rbs = [pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 2500, 1024)), pa.array(rng.random(1024), mask=rng.random(1024) < 0.2)], names=["k", "v"])
           for _ in range(nbatches)]
    return lb, rbs, JoinCondition([(InputRef(0), InputRef(0))])


@pytest.mark.parametrize("jt", ["left", "full"])
def test_finish_before_wait(hip, oracle, jt):
    """six batches pushed, none waited for; sqlrs_hash_join_finish first — it launches what is pending and waits for the probe
    kernels' marks — then the tickets: the tail and all six batches are the oracle's"""
    lb, rbs, cond = dup_case(21)
    exp = run(oracle, lb, rbs, jt, cond)
    before = fast_batches(hip)
    j = RawJoin(hip, lb, rbs[0], jt, cond, True)
    try:
        tickets = [j.push_async(b) for b in rbs]
        assert fast_batches(hip) - before == len(rbs)
        tail = j.finish()
        got = [j.wait(t) for t in tickets]
    finally:
        j.close()
    same_batches(got + [tail], exp)


def test_mixed_synchronous_and_async_calls(hip, oracle):
    """Left join over duplicate keys, probe_push and probe_push_async alternating on one operator: both only ever set marks"""
    lb, rbs, cond = dup_case(22, nbatches=8)
    exp = run(oracle, lb, rbs, "left", cond)
    j = RawJoin(hip, lb, rbs[0], "left", cond, True)
    try:
        got, pending = [], None
        for k, b in enumerate(rbs):
            if k % 2 == 0:
                pending = j.push_async(b)
            else:
                later = j.push(b)
                got += [j.wait(pending), later]
        tail = j.finish()
    finally:
        j.close()
    same_batches(got + [tail], exp)


def test_switch_semantics(hip, oracle, monkeypatch):
    lb, rbs, cond = dup_case(23, nbatches=3)
    exp = run(oracle, lb, rbs, "left", cond)
    for first in ("push", "push_async"):  # after the first probe call of either kind: an error, the setting stays
        j = RawJoin(hip, lb, rbs[0], "left", cond, False)
        try:
            assert j.set_general(1) == abi.OK and j.set_general(0) == abi.OK and j.set_general(1) == abi.OK
            before = fast_batches(hip)
            got = [j.push(rbs[0])] if first == "push" else [j.wait(j.push_async(rbs[0]))]
            assert j.set_general(0) == abi.ERR_INTERNAL and j.set_general(1) == abi.ERR_INTERNAL
            got += [j.wait(j.push_async(b)) for b in rbs[1:]]
            assert fast_batches(hip) - before == (2 if first == "push" else 3)
            got.append(j.finish())
        finally:
            j.close()
        same_batches(got, exp)
    j = RawJoin(hip, lb, rbs[0], "left", cond, True)  # on, then off again: today's counts
    try:
        assert j.set_general(0) == abi.OK
        before = fast_batches(hip)
        got = [j.wait(j.push_async(b)) for b in rbs] + [j.finish()]
        assert fast_batches(hip) == before
    finally:
        j.close()
    same_batches(got, exp)
    monkeypatch.setenv("SQLRS_ASYNC_FAST", "0")  # every batch through the synchronous operator, switch or not
    before = fast_batches(hip)
    got = run(hip, lb, rbs, "left", cond, depth=2, general=True)
    assert fast_batches(hip) == before
    same_batches(got, exp)


@pytest.mark.parametrize("seed", range(8))
def test_fuzz_async_join_general(hip, oracle, seed):
    """random join type, key kind, dense / sparse keys, duplicate rate (none, x2, one hot key), 1-4 payload columns per side with
    NULL rates 0 / 5 / 50 / 100 %, batch sizes 0-4096, depth 1-6: the stream, tail included, is the oracle's"""
    rng = np.random.default_rng(7000 + seed)
    jt = ["inner", "left", "right", "full"][seed % 4]  # (every join type twice, every duplicate rate at least twice)
    kk = str(rng.choice(["i32", "i64", "f64"]))
    mul = int(rng.choice([1, 7919]))
    nb = int(rng.choice([50, 3000, 20000]))
    dupl = ["x2", "hot", "none"][seed % 3]
    if dupl == "none":
        raw = rng.permutation(3 * nb)[:nb]
    elif dupl == "x2":
        raw = rng.integers(0, max(nb // 2, 1), nb)
    else:
        raw = rng.permutation(3 * nb)[:nb]
        raw[rng.choice(nb, min(nb // 4, 40), replace=False)] = raw[0]
    kconv = {"i32": lambda x: (x * mul).astype(np.int32), "i64": lambda x: (x * mul).astype(np.int64), "f64": lambda x: (x * mul).astype(np.float64) * 0.25}[kk]

    def col(kind, rows, p):
        vals = {"i64": lambda: rng.integers(-20, 20, rows), "f64": lambda: np.round(rng.random(rows), 2),
                "i32": lambda: rng.integers(-20, 20, rows).astype(np.int32)}[kind]()
        return pa.array(vals, mask=(rng.random(rows) < p) if p else None)

    def payload(rows, spec):
        return [col(k, rows, p) for k, p in spec]
    lspec = [(str(rng.choice(["i64", "f64", "i32"])), float(rng.choice([0.0, 0.05, 0.5, 1.0]))) for _ in range(int(rng.integers(1, 5)))]
    rspec = [(str(rng.choice(["i64", "f64", "i32"])), float(rng.choice([0.0, 0.05, 0.5, 1.0]))) for _ in range(int(rng.integers(1, 5)))]
    lb = pa.RecordBatch.from_arrays(payload(nb, lspec) + [pa.array(kconv(raw))], names=[f"l{i}" for i in range(len(lspec))] + ["k"])
    sizes = [int(x) for x in rng.choice([0, 1, 7, 64, 100, 1000, 1024, 2047, 4096], size=10)]
    rbs = [pa.RecordBatch.from_arrays([pa.array(kconv(rng.integers(0, 3 * nb, n)))] + payload(n, rspec), names=["k"] + [f"r{i}" for i in range(len(rspec))])
           for n in sizes]
    cond = JoinCondition([(InputRef(len(lspec)), InputRef(0))])
    m = max_run(lb, len(lspec))
    before = fast_batches(hip)
    got = run(hip, lb, rbs, jt, cond, depth=int(rng.integers(1, 7)), general=True)
    assert fast_batches(hip) - before == sum(1 for b in rbs if eligible(lb, b, 0, m)), (jt, kk, dupl, m)
    same_batches(got, run(oracle, lb, rbs, jt, cond))
