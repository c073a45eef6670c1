"""ORDER BY ... LIMIT over ranks on the device: sqlrs_range_select against its numpy restatement bit for bit (every key
type, NULL keys, DESC, several keys, an expression key, payloads of every type), and the acceptance check: W ranks
simulated in one process (one thread per rank, the collectives as barriers) run distributed_topk with the library's
calls, and the root's first min(k, N) rows must equal sqlrs_order over the whole table followed by the same OFFSET /
LIMIT, ties included."""
import ctypes as C
import threading

import numpy as np
import pyarrow as pa
import pytest

from sqlrs_amd import abi
from sqlrs_amd import distributed as D
from sqlrs_amd.executor import OrderExecutor
from sqlrs_amd.expr import BinaryOp, Constant, InputRef, OrderBy

pytestmark = pytest.mark.gpu

ALL_ONES = np.uint64((1 << 64) - 1)


def bits(a):
    a = np.asarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def values(arr):
    """numpy values of an arrow column with NULL slots zeroed (False for booleans)"""
    fill = False if pa.types.is_boolean(arr.type) else 0
    return np.asarray(arr.fill_null(fill).to_numpy(zero_copy_only=False))


def key_array(rng, kind, n):
    if kind == "i64":
        return rng.integers(-1000, 1000, n, dtype=np.int64)
    if kind == "i64_wide":
        return rng.integers(-(1 << 62), 1 << 62, n, dtype=np.int64)
    if kind == "f64":  # the values whose encoding a select and an Order could disagree on
        return rng.choice(np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1.5, -2.5, 1e-300, 3.0]), n)
    if kind == "i32":
        return rng.integers(-(1 << 31), (1 << 31) - 1, n).astype(np.int32)
    if kind == "bool":
        return rng.random(n) < 0.5
    raise ValueError(kind)


def make_case(n, kinds, nulls, seed):
    """-> (batch: key columns, Utf8 / Boolean / nullable f64 payloads, the row id last; numpy keys [(values, valid, asc)])"""
    rng = np.random.default_rng(seed)
    arrays, names, keys = [], [], []
    for k, (kind, asc) in enumerate(kinds):
        v = key_array(rng, kind, n)
        ok = (rng.random(n) > 0.2) if nulls else None
        arrays.append(pa.array(v, mask=None if ok is None else ~ok))
        names.append(f"k{k}")
        keys.append((v, ok, asc))
    arrays += [pa.array([f"s{i % 97}" if i % 11 else None for i in range(n)], type=pa.string()),
               pa.array(rng.random(n) < 0.3, mask=rng.random(n) < 0.1),
               pa.array(rng.random(n), mask=rng.random(n) < 0.25),
               pa.array(np.arange(n, dtype=np.int64))]
    names += ["s", "b", "x", "rid"]
    return pa.RecordBatch.from_arrays(arrays, names=names), keys


def order_by_of(keys):
    return [OrderBy(InputRef(k), asc=asc) for k, (_, _, asc) in enumerate(keys)]


def check_select(hip, batch, order_by, keys, row_base, bound, out_mem=abi.MEM_DEVICE):
    n = batch.num_rows
    t = D.range_tuples_numpy(keys, row_base) if n else np.zeros((0, 2 * len(keys) + 1), np.uint64)
    (exp_rid,) = D.range_select_numpy([np.arange(n, dtype=np.int64)], t, bound)
    got = hip.range_select(batch, order_by, row_base, bound, out_mem)
    g = (hip.to_host(got) if out_mem == abi.MEM_DEVICE else got).to_arrow(batch.schema.names)
    got.release()
    assert g.num_rows == len(exp_rid)
    assert np.array_equal(np.asarray(g.column(batch.num_columns - 1).to_numpy(zero_copy_only=False)), exp_rid)
    for c in range(batch.num_columns - 1):  # every column moved with its row (values by bit pattern, validity)
        src, out = batch.column(c).take(pa.array(exp_rid, type=pa.int64())), g.column(c)
        assert src.is_null().equals(out.is_null()), batch.schema.names[c]
        if pa.types.is_string(src.type):
            assert src.equals(out)
        else:
            assert np.array_equal(bits(values(src)), bits(values(out))), batch.schema.names[c]
    return len(exp_rid)


def bounds_of(keys, n, row_base, seed):
    """the all-zero and all-ones tuples, and row tuples at several ranks (near the start, the middle, the end)"""
    tw = 2 * len(keys) + 1
    out = [np.zeros(tw, np.uint64), np.full(tw, ALL_ONES, np.uint64)]
    if n:
        t = D.range_tuples_numpy(keys, row_base)
        srt = t[np.lexsort(t.T[::-1])]
        rng = np.random.default_rng(seed)
        out += [srt[j] for j in sorted({0, 1, n // 100, int(rng.integers(0, n)), n // 2, n - 1}) if j < n]
        mid = srt[n // 2].copy()
        mid[-1] += np.uint64(1)  # between two row tuples
        out.append(mid)
    return out


@pytest.mark.parametrize("kind", ["i64", "i64_wide", "f64", "i32", "bool"])
@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("asc", [True, False])
def test_select_one_key(hip, kind, nulls, asc):
    n = 100_003
    batch, keys = make_case(n, [(kind, asc)], nulls, ["i64", "i64_wide", "f64", "i32", "bool"].index(kind) * 4 + 2 * nulls + asc)
    for b in bounds_of(keys, n, 1 << 33, 1):
        check_select(hip, batch, order_by_of(keys), keys, 1 << 33, b)


@pytest.mark.parametrize("kinds", [[("i64", False), ("f64", True)], [("i32", True), ("bool", False), ("i64_wide", False)]])
def test_select_several_keys(hip, kinds):
    n = 70_001
    batch, keys = make_case(n, kinds, True, len(kinds))
    for b in bounds_of(keys, n, 12345, 2):
        check_select(hip, batch, order_by_of(keys), keys, 12345, b)


def test_select_bound_inside_a_run_of_equal_keys(hip):
    """a bound whose key is that of 40 % of the rows: the run is cut at the bound's position"""
    n = 50_000
    rng = np.random.default_rng(8)
    k = np.where(rng.random(n) < 0.4, 7, rng.integers(0, 15, n)).astype(np.int64)
    batch = pa.RecordBatch.from_arrays([pa.array(k), pa.array(np.arange(n, dtype=np.int64))], names=["k", "rid"])
    keys = [(k, None, True)]
    t = D.range_tuples_numpy(keys, 900)
    srt = t[np.lexsort(t.T[::-1])]
    run = np.nonzero(srt[:, 1] == D.ordered_key_np(np.array([7], np.int64))[0])[0]
    for j in (run[0], run[len(run) // 3], run[-1]):
        assert check_select(hip, batch, order_by_of(keys), keys, 900, srt[j]) == j


def test_select_expression_key_host_output(hip):
    n = 30_000
    batch, keys = make_case(n, [("i64", False)], True, 5)
    v, ok, _ = keys[0]
    ekeys = [(v * 3 - 11, ok, False)]
    ob = [OrderBy(BinaryOp("-", BinaryOp("*", InputRef(0), Constant.of(3)), Constant.of(11)), asc=False)]
    for b in bounds_of(ekeys, n, 0, 3):
        check_select(hip, batch, ob, ekeys, 0, b, out_mem=abi.MEM_HOST)


def test_select_many_keys_writes_tuples(hip):
    """more keys than the kernel arguments hold (17): the tuples are written and compared"""
    n = 20_000
    batch, keys = make_case(n, [("i32", bool(q % 2)) for q in range(17)], True, 17)
    for b in bounds_of(keys, n, 77, 4)[::2]:
        check_select(hip, batch, order_by_of(keys), keys, 77, b)


def test_select_empty_and_tiny(hip):
    for n in (0, 1, 63, 64, 65):
        batch, keys = make_case(n, [("f64", True), ("i64", False)], True, n)
        for b in bounds_of(keys, n, 5, n):
            check_select(hip, batch, order_by_of(keys), keys, 5, b)


def _raw_select(hip, batch, order_by, row_base, bound_ptr, use_out=True):
    arr, _keep = hip._order_by_array(order_by)
    b = abi.as_batch(batch)
    out = C.POINTER(abi.Batch)()
    st = hip.fn("range_select")(hip.ctx, b.ptr, len(order_by), arr, row_base, bound_ptr, abi.MEM_DEVICE,
                                C.byref(out) if use_out else None)
    return st, (hip.fn("last_error")(hip.ctx) or b"").decode()


def test_select_errors(hip):
    b = pa.RecordBatch.from_arrays([pa.array(["x", "y", "z"]), pa.array([3, 1, 2], type=pa.int64())], names=["s", "k"])
    bound = np.full(3, ALL_ONES, dtype=np.uint64)
    bp = bound.ctypes.data_as(C.POINTER(C.c_uint64))
    st, msg = _raw_select(hip, b, [OrderBy(InputRef(0))], 0, bp)
    assert st == abi.ERR_INTERNAL and "Utf8" in msg
    st, msg = _raw_select(hip, b, [OrderBy(InputRef(1))], -1, bp)
    assert st == abi.ERR_INTERNAL and "row_base" in msg
    st, msg = _raw_select(hip, b, [OrderBy(InputRef(1))], 0, None)
    assert st == abi.ERR_INTERNAL and "null" in msg
    st, msg = _raw_select(hip, b, [OrderBy(InputRef(1))], 0, bp, use_out=False)
    assert st == abi.ERR_INTERNAL and "null" in msg
    st, msg = _raw_select(hip, b, [], 0, bp)
    assert st == abi.ERR_INTERNAL and "key" in msg
    got = hip.range_select(b, [OrderBy(InputRef(1))], 0, bound)  # still usable afterwards
    assert hip.to_host(got).to_arrow(["s", "k"]).column(1).to_pylist() == [3, 1, 2]
    got.release()


# ---- W ranks in one process: the acceptance check ---------------------------------------------------------------------
class SimRanks:
    """W threads, one per rank; allgather = a barrier over per-rank slots; device calls serialised by a lock"""

    def __init__(self, world):
        self.world = world
        self.barrier = threading.Barrier(world)
        self.slots = [None] * world
        self.lock = threading.Lock()

    def allgather(self, rank, obj):
        self.barrier.wait()
        self.slots[rank] = obj
        self.barrier.wait()
        out = list(self.slots)
        self.barrier.wait()
        return out

    def run(self, fn):
        res, errs = [None] * self.world, []

        def body(r):
            try:
                res[r] = fn(r)
            except BaseException as e:  # noqa: BLE001
                errs.append(e)
                self.barrier.abort()

        th = [threading.Thread(target=body, args=(r,)) for r in range(self.world)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        if errs:
            raise errs[0]
        return res


def topk_ranks(hip, batch, order_by, world, cuts, k, samples_per_rank=256):
    """distributed_topk on W simulated ranks with sqlrs_range_sample / _bound / _select and sqlrs_order_* + set_limit on the
    root -> (root result as an arrow table of its first min(k, N) rows, info)"""
    nk = len(order_by)
    sim = SimRanks(world)
    slices = [batch.slice(cuts[r], cuts[r + 1] - cuts[r]) for r in range(world)]

    def rank_fn(r):
        def locked(f):
            with sim.lock:
                return f()

        def select(row_base, bound):
            def call():
                got = hip.range_select(slices[r], order_by, row_base, bound, abi.MEM_HOST)
                t = got.to_arrow(batch.schema.names)
                got.release()
                return t
            t = locked(call)
            return t, t.num_rows

        def gather_to_root(cand, count):
            return [c for c in sim.allgather(r, cand) if c.num_rows]  # rank order

        def order(received, limit):
            if not received:
                return None
            (o,) = locked(lambda: list(OrderExecutor(hip, order_by, received, limit_hint=limit).execute()))
            return o

        return D.distributed_topk(
            cuts[r + 1] - cuts[r], world, r, k=k, allgather=lambda obj: sim.allgather(r, obj),
            sample=lambda rb, m: locked(lambda: hip.range_sample(slices[r], order_by, rb, m)),
            bound=lambda t, n, kk, a: hip.range_bound(nk, t, n, kk, a), select=select,
            gather_to_root=gather_to_root, order=order, samples_per_rank=samples_per_rank)

    out = sim.run(rank_fn)
    assert all(res is None for res, _ in out[1:])
    res, info = out[0]
    assert all(i == info for _, i in out)  # every rank saw the same attempts and counts
    need = min(k, batch.num_rows)
    tab = pa.Table.from_batches([res]).slice(0, need) if res is not None else None
    return tab, info


def sim_table(shape, n, seed=0):
    rng = np.random.default_rng(seed)
    rid = pa.array(np.arange(n, dtype=np.int64))
    if shape == "random":
        b = pa.RecordBatch.from_arrays([pa.array(rng.integers(-(1 << 62), 1 << 62, n, dtype=np.int64)),
                                        pa.array(rng.random(n)), rid], names=["k", "v", "rid"])
        return b, [OrderBy(InputRef(0), asc=True)]
    if shape == "ties_desc":
        s = pa.array([f"r{i % 1013}" if i % 17 else None for i in range(n)])
        b = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 30, n, dtype=np.int64)), s, rid], names=["k", "s", "rid"])
        return b, [OrderBy(InputRef(0), asc=False)]
    if shape == "two_keys_nulls":
        a = pa.array(rng.integers(0, 30, n, dtype=np.int64), mask=rng.random(n) < 0.1)
        f = pa.array(rng.random(n).round(2), mask=rng.random(n) < 0.2)
        b = pa.RecordBatch.from_arrays([a, f, rid], names=["a", "f", "rid"])
        return b, [OrderBy(InputRef(0), asc=False), OrderBy(InputRef(1), asc=True)]
    raise ValueError(shape)


def uneven_cuts(n, world):
    w = np.array([3, 1, 0, 5, 2, 4, 1, 2][:world], dtype=np.float64)
    if world == 2:
        w = np.array([0.0, 1.0])
    c = np.concatenate([[0], np.cumsum(w)]) / w.sum() * n
    return [int(x) for x in c]


def assert_same_rows(got, exp, names):
    assert got.num_rows == exp.num_rows
    for name in names:
        g, e = got.column(name).combine_chunks(), exp.column(name).combine_chunks()
        assert g.is_null().equals(e.is_null()), name
        if pa.types.is_floating(g.type) or pa.types.is_integer(g.type):
            assert np.array_equal(bits(values(g)), bits(values(e))), name
        else:
            assert g.equals(e), name


@pytest.mark.parametrize("shape", ["ties_desc", "two_keys_nulls", "random"])
@pytest.mark.parametrize("world", [2, 3, 8])
def test_simulated_ranks_equal_order_limit(hip, shape, world):
    n = 60_000
    batch, order_by = sim_table(shape, n, world)
    cuts = uneven_cuts(n, world)
    assert any(cuts[r + 1] == cuts[r] for r in range(world))  # one slice is empty
    (full,) = list(OrderExecutor(hip, order_by, [batch]).execute())
    full = pa.Table.from_batches([full])
    for k in (0, 1, 10, 1000, n - 1, n, n + 5):
        got, info = topk_ranks(hip, batch, order_by, world, cuts, k)
        need = min(k, n)
        assert info["candidates"] >= need and info["total_rows"] == n
        if need == 0:
            assert got is None or got.num_rows == 0
            continue
        assert_same_rows(got, full.slice(0, need), batch.schema.names)
        off = min(7, need)  # OFFSET 7 LIMIT k - 7 on both
        assert_same_rows(got.slice(off), full.slice(off, need - off), batch.schema.names)
        if k <= 1000:
            assert info["candidates"] < n // 4, (k, info)  # only candidates travel


def test_selectivity_eight_ranks(hip):
    """1e7 random int64 rows over 8 ranks, 1024 samples per rank, k = 1000: the first bound is enough and few rows travel"""
    import torch
    n, world, k = 10_000_000, 8, 1000
    g = torch.Generator(device="cuda:0").manual_seed(11)
    key = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device="cuda:0", generator=g)
    rid = torch.arange(n, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    batch = abi.RawBatch([abi.device_column(abi.INT64, n, key.data_ptr()), abi.device_column(abi.INT64, n, rid.data_ptr())],
                         n, keepalive=(key, rid))
    order_by = [OrderBy(InputRef(0), asc=True)]
    cuts = [n * r // world for r in range(world + 1)]
    sim = SimRanks(world)

    def rank_fn(r):
        sl = abi.RawBatch([abi.device_column(abi.INT64, cuts[r + 1] - cuts[r], key.data_ptr() + 8 * cuts[r]),
                           abi.device_column(abi.INT64, cuts[r + 1] - cuts[r], rid.data_ptr() + 8 * cuts[r])],
                          cuts[r + 1] - cuts[r], keepalive=(key, rid))

        def select(row_base, bound):
            with sim.lock:
                got = hip.range_select(sl, order_by, row_base, bound, abi.MEM_HOST)
                t = got.to_arrow(["k", "rid"])
                got.release()
            return t, t.num_rows

        def order(received, limit):
            with sim.lock:
                (o,) = list(OrderExecutor(hip, order_by, received, limit_hint=limit).execute())
            return o

        def sample(rb, m):
            with sim.lock:
                return hip.range_sample(sl, order_by, rb, m)

        return D.distributed_topk(cuts[r + 1] - cuts[r], world, r, k=k, allgather=lambda obj: sim.allgather(r, obj),
                                  sample=sample, bound=lambda t, nn, kk, a: hip.range_bound(1, t, nn, kk, a),
                                  select=select, gather_to_root=lambda c, cnt: [b for b in sim.allgather(r, c) if b.num_rows],
                                  order=order,
                                  samples_per_rank=1024)

    out = sim.run(rank_fn)
    res, info = out[0]
    T = 1024 * world
    assert info["attempts"] == 0, info
    assert k <= info["candidates"] <= max(4 * k, 8 * n // T), info
    got = pa.Table.from_batches([res]).slice(0, k)
    kh = key.cpu().numpy()
    exp = np.argsort(kh, kind="stable")[:k]
    assert np.array_equal(got.column("rid").to_numpy(), exp)
    assert np.array_equal(got.column("k").to_numpy(), kh[exp])


def test_distributed_topk_world_1_rccl(hip):
    """distributed_topk with the library's calls and the RCCL all-to-all of a one-rank communicator"""
    n, k = 200_000, 777
    batch, order_by = sim_table("two_keys_nulls", n, 5)
    xchg = hip.exchange_create(hip.exchange_unique_id(), 0, 1)
    dev = hip.to_device(batch)
    held = []
    try:
        def select(row_base, bound):
            got = hip.range_select(dev, order_by, row_base, bound)
            held.append(got)
            return got, got.num_rows

        def gather_to_root(cand, count):
            got, recv = hip.exchange_all_to_all(xchg, cand, [0], [count])
            assert recv == [count]
            held.append(got)
            return got

        def order(received, limit):
            (o,) = list(OrderExecutor(hip, order_by, [received], limit_hint=limit).execute())
            return o

        res, info = D.distributed_topk(
            n, 1, 0, k=k, allgather=lambda obj: [obj], sample=lambda rb, m: hip.range_sample(dev, order_by, rb, m),
            bound=lambda t, nn, kk, a: hip.range_bound(2, t, nn, kk, a), select=select, gather_to_root=gather_to_root,
            order=order)
        (exp,) = list(OrderExecutor(hip, order_by, [batch]).execute())
        assert k <= info["candidates"] < n // 10
        got = pa.Table.from_batches([res]).rename_columns(batch.schema.names)  # (a device batch carries no names)
        assert_same_rows(got.slice(0, k), pa.Table.from_batches([exp]).slice(0, k),
                         batch.schema.names)
    finally:
        for h in held:
            h.release()
        dev.release()
        hip.fn("exchange_destroy")(xchg)
