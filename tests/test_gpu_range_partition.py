"""sqlrs_range_sample / _splitters / _partition (range_partition.hip) on the device against their numpy restatement
(sqlrs_amd/distributed.py), the fast multi-split against the general path, and the acceptance check of the multi-GPU
ORDER BY: W ranks simulated in one process (slice -> sample -> splitters -> partition -> route -> Order per destination),
whose outputs concatenated in rank order must equal sqlrs_order over the whole table bit for bit, ties included."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest

from sqlrs_amd import abi
from sqlrs_amd import distributed as D
from sqlrs_amd.executor import OrderExecutor
from sqlrs_amd.expr import InputRef, OrderBy

pytestmark = pytest.mark.gpu


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
    if kind == "f64":  # the values whose encoding a partition and an Order could disagree on
        return rng.choice(np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1.5, -2.5, 1e-300, 3.0]), n)
    if kind == "i32":
        return rng.integers(-(1 << 31), (1 << 31) - 1, n).astype(np.int32)
    if kind == "bool":
        return rng.random(n) < 0.5
    raise ValueError(kind)


def make_case(n, kinds, nulls, seed, payload=True):
    """-> (pyarrow batch: key columns, a float payload, the row id last; numpy keys [(values, valid, asc)])"""
    rng = np.random.default_rng(seed)
    arrays, names, keys = [], [], []
    for k, (kind, asc) in enumerate(kinds):
        v = key_array(rng, kind, n)
        ok = (rng.random(n) > 0.2) if nulls else None
        arrays.append(pa.array(v, mask=None if ok is None else ~ok))
        names.append(f"k{k}")
        keys.append((v, ok, asc))
    if payload:
        arrays.append(pa.array(rng.random(n)))
        names.append("pay")
    arrays.append(pa.array(np.arange(n, dtype=np.int64)))
    names.append("rid")
    return pa.RecordBatch.from_arrays(arrays, names=names), keys


def order_by_of(keys):
    return [OrderBy(InputRef(k), asc=asc) for k, (_, _, asc) in enumerate(keys)]


def check_partition(hip, batch, keys, row_base, parts, seed, out_mem=abi.MEM_DEVICE):
    n = batch.num_rows
    t = D.range_tuples_numpy(keys, row_base) if n else np.zeros((0, 2 * len(keys) + 1), np.uint64)
    rng = np.random.default_rng(seed)
    smp = t[rng.integers(0, n, 64)] if n else t
    spl = D.range_splitters_numpy(smp, parts)
    got, offs = hip.range_partition(batch, order_by_of(keys), row_base, parts, spl if parts > 1 else None, out_mem)
    g = (hip.to_host(got) if out_mem == abi.MEM_DEVICE else got).to_arrow(batch.schema.names)
    got.release()
    rid = np.arange(n, dtype=np.int64)
    (prid,), eoffs = D.range_partition_numpy([rid], t, spl)
    assert offs == eoffs
    assert np.array_equal(np.asarray(g.column(batch.num_columns - 1).to_numpy(zero_copy_only=False)), prid)
    for c in range(batch.num_columns - 1):  # every column moved with its row (values by bit pattern, validity)
        src, out = batch.column(c).take(pa.array(prid)), g.column(c)
        assert src.is_null().equals(out.is_null())
        assert np.array_equal(bits(values(src)), bits(values(out)))
    return offs


@pytest.mark.parametrize("rows", [0, 1, 63, (1 << 16) - 1, 1 << 16, 1 << 20])
@pytest.mark.parametrize("kind", ["i64", "f64"])
@pytest.mark.parametrize("asc", [True, False])
def test_partition_rows_one_key(hip, rows, kind, asc):
    """one key without NULLs, (key, payload, row id): the fast multi-split from 2^16 rows on, the general path below"""
    batch, keys = make_case(rows, [(kind, asc)], False, rows + 7 * asc)
    for parts in ((2, 8, 256) if rows >= (1 << 16) else (1, 2, 7)):
        check_partition(hip, batch, keys, 1 << 33, parts, parts)


@pytest.mark.parametrize("kinds", [[("i32", True)], [("bool", False)], [("i64_wide", False), ("f64", True)],
                                   [("i32", False), ("bool", True), ("f64", False)]])
@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("rows", [63, 100_000])
def test_partition_general_keys(hip, kinds, nulls, rows):
    """int32 / boolean keys, 1-3 keys, NULL keys, asc and desc: the general path"""
    batch, keys = make_case(rows, kinds, nulls, len(kinds) * 10 + nulls + rows)
    for parts in (1, 7, 8, 256):
        check_partition(hip, batch, keys, 12345, parts, parts + rows)


def test_partition_host_output_and_host_input(hip):
    batch, keys = make_case(5000, [("i64", False)], True, 3)
    check_partition(hip, batch, keys, 0, 5, 1, out_mem=abi.MEM_HOST)


@pytest.mark.parametrize("rows", [0, 1, 63, 1 << 16, 1 << 20])
@pytest.mark.parametrize("samples", [0, 1, 1024])
def test_sample_tuples(hip, rows, samples):
    batch, keys = make_case(rows, [("f64", False), ("i32", True)], True, rows + samples)
    got = hip.range_sample(batch, order_by_of(keys), 77, samples)
    exp = D.range_tuples_numpy(keys, 77, D.range_sample_rows(rows, samples)) if rows else np.zeros((0, 5), np.uint64)
    assert got.shape == exp.shape and np.array_equal(got, exp)


def test_splitters_device_library_equals_numpy(hip):
    rng = np.random.default_rng(1)
    t = rng.integers(0, 4, (3000, 5)).astype(np.uint64)
    for parts in (1, 2, 7, 256):
        assert np.array_equal(hip.range_splitters(2, t, parts), D.range_splitters_numpy(t, parts))


def _fast_vs_general(hip, monkeypatch, batch, keys, parts, spl):
    outs = []
    for hook in ("0", "1"):
        monkeypatch.setenv("SQLRS_RANGE_PART_GENERAL", hook)
        got, offs = hip.range_partition(batch, order_by_of(keys), 5_000_000, parts, spl)
        outs.append((hip.to_host(got).to_arrow(batch.schema.names), offs))
        got.release()
    monkeypatch.delenv("SQLRS_RANGE_PART_GENERAL")
    assert outs[0][1] == outs[1][1]
    for c in range(batch.num_columns):
        a, b = outs[0][0].column(c), outs[1][0].column(c)
        assert np.array_equal(bits(a.to_numpy()), bits(b.to_numpy()))
    return outs[0]


@pytest.mark.parametrize("kind", ["i64_wide", "f64"])
@pytest.mark.parametrize("ids", ["0", "1"])
def test_fast_path_equals_general_path(hip, monkeypatch, kind, ids):
    """2^20 rows of (key, f64 value, int64 row id) through the multi-split and through the general path (hook); both
    forms of the multi-split's scatter (part searched again / read back as a byte, SQLRS_RANGE_PART_IDS)"""
    monkeypatch.setenv("SQLRS_RANGE_PART_IDS", ids)
    n = 1 << 20
    batch, keys = make_case(n, [(kind, kind == "f64")], False, 99)
    t = D.range_tuples_numpy(keys, 5_000_000)
    spl = D.range_splitters_numpy(t[::997], 8)
    out, offs = _fast_vs_general(hip, monkeypatch, batch, keys, 8, spl)
    (prid,), eoffs = D.range_partition_numpy([np.arange(n)], t, spl)
    assert offs == eoffs and np.array_equal(out.column(2).to_numpy(), prid)


def test_fast_path_with_null_key_splitters(hip):
    """a splitter whose key is NULL (from a rank that has NULL keys) lies below every row of a rank without NULLs"""
    n = 1 << 17
    batch, keys = make_case(n, [("i64", True)], False, 4, payload=False)
    t = D.range_tuples_numpy(keys, 0)
    null_spl = np.array([[0, 0, 3]], dtype=np.uint64)
    spl = np.concatenate([null_spl, D.range_splitters_numpy(t[::101], 4)])
    got, offs = hip.range_partition(batch, order_by_of(keys), 0, 5, spl)
    got.release()
    assert offs == D.range_partition_numpy([np.arange(n)], t, spl)[1] and offs[1] == 0


# ---- W ranks in one process: the acceptance check ---------------------------------------------------------------------
def sim_table(shape, n, seed=0):
    rng = np.random.default_rng(seed)
    rid = np.arange(n, dtype=np.int64)
    if shape == "random":
        k = rng.integers(-(1 << 62), 1 << 62, n, dtype=np.int64)
    elif shape == "ties":
        k = rng.integers(0, 50, n, dtype=np.int64)
    elif shape == "all_equal":
        k = np.full(n, 9, dtype=np.int64)
    elif shape == "presorted":
        k = np.sort(rng.integers(0, 1 << 40, n, dtype=np.int64))
    elif shape == "reverse":
        k = np.sort(rng.integers(0, 1 << 40, n, dtype=np.int64))[::-1].copy()
    if shape in ("random", "ties", "all_equal", "presorted", "reverse"):
        b = pa.RecordBatch.from_arrays([pa.array(k), pa.array(rng.random(n)), pa.array(rid)], names=["k", "v", "rid"])
        return b, [OrderBy(InputRef(0), asc=shape != "reverse")]
    if shape == "two_keys_nulls":
        a = pa.array(rng.integers(0, 30, n, dtype=np.int64), mask=rng.random(n) < 0.1)
        f = pa.array(rng.random(n).round(2), mask=rng.random(n) < 0.2)
        b = pa.RecordBatch.from_arrays([a, f, pa.array(rid)], names=["a", "f", "rid"])
        return b, [OrderBy(InputRef(0), asc=False), OrderBy(InputRef(1), asc=True)]
    if shape == "utf8_payload":
        k = rng.integers(0, 1000, n, dtype=np.int64)
        s = pa.array([f"r{i % 1013}" if i % 17 else None for i in range(n)])
        b = pa.RecordBatch.from_arrays([s, pa.array(k), pa.array(rid)], names=["s", "k", "rid"])
        return b, [OrderBy(InputRef(1), asc=True)]
    raise ValueError(shape)


def uneven_cuts(n, world):
    w = np.array([3, 1, 0, 5, 2, 4, 1, 2][:world], dtype=np.float64)
    if world == 2:
        w = np.array([0.0, 1.0])
    c = np.concatenate([[0], np.cumsum(w)]) / w.sum() * n
    return [int(x) for x in c]


def simulate(hip, batch, order_by, world, cuts, samples=256):
    """every 'rank' samples, partitions its slice (device) with its row_base; parts routed on the host in source-rank
    order; sqlrs_order per destination -> the destination outputs and the rows each destination received"""
    nk = len(order_by)
    slices = [batch.slice(cuts[r], cuts[r + 1] - cuts[r]) for r in range(world)]
    tuples = np.concatenate([hip.range_sample(slices[r], order_by, cuts[r], samples) for r in range(world)]).reshape(-1, 2 * nk + 1)
    spl = hip.range_splitters(nk, tuples, world)
    recv = [[] for _ in range(world)]
    for r in range(world):
        got, offs = hip.range_partition(slices[r], order_by, cuts[r], world, spl if world > 1 else None, abi.MEM_HOST)
        t = got.to_arrow(batch.schema.names)
        got.release()
        for p in range(world):
            if offs[p + 1] > offs[p]:
                recv[p].append(t.slice(offs[p], offs[p + 1] - offs[p]))
    outs = []
    for p in range(world):
        if recv[p]:
            (o,) = list(OrderExecutor(hip, order_by, recv[p]).execute())
            outs.append(o)
    return outs, [sum(x.num_rows for x in r) for r in recv]


@pytest.mark.parametrize("shape", ["random", "ties", "all_equal", "presorted", "reverse", "two_keys_nulls", "utf8_payload"])
@pytest.mark.parametrize("world", [2, 3, 8])
def test_simulated_ranks_equal_single_order(hip, shape, world):
    n = 300_000
    batch, order_by = sim_table(shape, n, world)
    cuts = uneven_cuts(n, world)
    assert any(cuts[r + 1] == cuts[r] for r in range(world))  # one slice is empty
    outs, sizes = simulate(hip, batch, order_by, world, cuts)
    (exp,) = list(OrderExecutor(hip, order_by, [batch]).execute())
    got = pa.Table.from_batches(outs).combine_chunks()
    exp = pa.Table.from_batches([exp])
    assert got.num_rows == n
    assert got.column("rid").equals(exp.column("rid"))  # the order, ties included
    for name in batch.schema.names:
        g, e = got.column(name), exp.column(name)
        assert g.is_null().equals(e.is_null())
        if pa.types.is_floating(g.type) or pa.types.is_integer(g.type):
            assert np.array_equal(bits(values(g)), bits(values(e)))
        else:
            assert g.equals(e)
    assert sum(sizes) == n


@pytest.mark.parametrize("shape", ["random", "all_equal", "presorted"])
def test_balance_eight_ranks(hip, shape):
    n = 800_000
    batch, order_by = sim_table(shape, n, 1)
    world = 8
    cuts = [n * r // world for r in range(world + 1)]
    slices = [batch.slice(cuts[r], cuts[r + 1] - cuts[r]) for r in range(world)]
    tuples = np.concatenate([hip.range_sample(slices[r], order_by, cuts[r], 1024) for r in range(world)])
    spl = hip.range_splitters(1, tuples, world)
    sizes = np.zeros(world, dtype=np.int64)
    for r in range(world):
        got, offs = hip.range_partition(slices[r], order_by, cuts[r], world, spl)
        got.release()
        sizes += np.diff(offs)
    assert sizes.sum() == n and sizes.max() <= 1.15 * n / world, sizes.tolist()


def test_distributed_order_world_1_rccl(hip):
    """distributed_order with the library's calls and the RCCL all-to-all of a one-rank communicator"""
    n = 200_000
    batch, order_by = sim_table("ties", n, 5)
    xchg = hip.exchange_create(hip.exchange_unique_id(), 0, 1)
    dev = hip.to_device(batch)
    try:
        def exchange(parts, offsets):
            got, recv = hip.exchange_all_to_all(xchg, parts, offsets[:1], [offsets[1] - offsets[0]])
            assert recv == [n]
            return got

        def order(received):
            (o,) = list(OrderExecutor(hip, order_by, [received]).execute())
            return o

        piece = D.distributed_order(
            n, 1, 0, allgather=lambda obj: [obj], sample=lambda rb, m: hip.range_sample(dev, order_by, rb, m),
            splitters=lambda t, w: hip.range_splitters(1, t, w),
            partition=lambda rb, spl: hip.range_partition(dev, order_by, rb, 1, spl if len(spl) else None),
            exchange=exchange, order=order)
        (exp,) = list(OrderExecutor(hip, order_by, [batch]).execute())
        assert piece.num_rows == n
        for c in range(exp.num_columns):
            assert np.array_equal(bits(values(piece.column(c))), bits(values(exp.column(c))))
    finally:
        dev.release()
        hip.fn("exchange_destroy")(xchg)


# ---- errors -----------------------------------------------------------------------------------------------------------
def _raw_partition(hip, batch, order_by, parts, spl_ptr, row_base=0):
    arr, _keep = hip._order_by_array(order_by)
    b = abi.as_batch(batch)
    out = C.POINTER(abi.Batch)()
    offs = (C.c_int64 * (max(parts, 1) + 1))()
    st = hip.fn("range_partition")(hip.ctx, b.ptr, len(order_by), arr, row_base, parts, spl_ptr, abi.MEM_DEVICE,
                                   C.byref(out), offs)
    return st, (hip.fn("last_error")(hip.ctx) or b"").decode()


def test_errors(hip):
    b = pa.RecordBatch.from_arrays([pa.array(["x", "y", "z"]), pa.array([3, 1, 2], type=pa.int64())], names=["s", "k"])
    spl = np.zeros((8, 3), dtype=np.uint64)
    sp = spl.ctypes.data_as(C.POINTER(C.c_uint64))
    st, msg = _raw_partition(hip, b, [OrderBy(InputRef(0))], 2, sp)
    assert st == abi.ERR_INTERNAL and "Utf8" in msg
    with pytest.raises(abi.ExecutorError, match="Utf8"):
        hip.range_sample(b, [OrderBy(InputRef(0))], 0, 4)
    for parts in (0, 257):
        st, msg = _raw_partition(hip, b, [OrderBy(InputRef(1))], parts, sp)
        assert st == abi.ERR_INTERNAL and "num_parts" in msg
    st, msg = _raw_partition(hip, b, [OrderBy(InputRef(1))], 3, None)
    assert st == abi.ERR_INTERNAL and "NULL" in msg
    bad = np.array([[1, 5, 0], [1, 4, 0]], dtype=np.uint64)
    st, msg = _raw_partition(hip, b, [OrderBy(InputRef(1))], 3, bad.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert st == abi.ERR_INTERNAL and "nondecreasing" in msg
    # still usable afterwards; one part needs no splitters
    got, offs = hip.range_partition(b, [OrderBy(InputRef(1))], 0, 1, None)
    assert offs == [0, 3]
    got.release()


def test_row_limit_guard(hip):
    """a batch that claims 2^31 rows is refused at the ABI entrance (SQLRS_ERR_ARROW), before any column is read"""
    import torch
    keep = torch.zeros(8, dtype=torch.int64, device="cuda:0")
    cols = (abi.Column * 1)()
    cols[0].dtype, cols[0].mem, cols[0].length, cols[0].null_count = abi.INT64, abi.MEM_DEVICE, 1 << 31, 0
    cols[0].values = keep.data_ptr()
    raw = abi.Batch()
    raw.num_rows, raw.num_columns, raw.columns = 1 << 31, 1, cols
    arr, _k = hip._order_by_array([OrderBy(InputRef(0))])
    spl = np.zeros((1, 3), dtype=np.uint64)
    out = C.POINTER(abi.Batch)()
    offs = (C.c_int64 * 3)()
    st = hip.fn("range_partition")(hip.ctx, C.byref(raw), 1, arr, 0, 2, spl.ctypes.data_as(C.POINTER(C.c_uint64)),
                                   abi.MEM_DEVICE, C.byref(out), offs)
    assert st == abi.ERR_ARROW and b"2^31" in hip.fn("last_error")(hip.ctx)
    tup = np.zeros((4, 3), dtype=np.uint64)
    w = C.c_int()
    st = hip.fn("range_sample")(hip.ctx, C.byref(raw), 1, arr, 0, 4, tup.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(w))
    assert st == abi.ERR_ARROW and b"2^31" in hip.fn("last_error")(hip.ctx)
    del keep
