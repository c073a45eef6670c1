"""SQLRS_EXPR_STAGE_ALL_TYPES on the GPU: the four blocking operators fed the pieces of tests/host_stage_cases.py as caller-built
HOST batches (windows into one offsets array, a stated null_count of -1, garbage in the unused bits of a bitmap's last byte).
With the flag on the result equals the flag-off result bit for bit AND the oracle's over the same rows as ordinary pyarrow
batches; `stage_all_types_batches` counts every pushed host batch and `stage_stitch_flushes` the flushes."""
import numpy as np
import pyarrow as pa
import pytest

import host_stage_cases as H
from sqlrs_amd import abi
from sqlrs_amd.executor import HashAggExecutor, HashJoinAggExecutor, HashJoinExecutor, OrderExecutor
from sqlrs_amd.expr import AggFunc, Constant, InputRef, JoinCondition, OrderBy

pytestmark = pytest.mark.gpu

GPU_CASES = [("A", "minus_one", "empty_null"), ("A", "none", "window37"), ("B", "tail_ones", "window37"),
             ("B", "first_at_3", "long5000"), ("B", "present_zero", "values_null"), ("C", "minus_one", "multibyte"),
             ("C", "all_null", "empty_null"), ("D", "present_zero", "empty_null"), ("E", "minus_one", "window37"),
             ("F64", "minus_one", "multibyte"), ("F65", "tail_ones", "long5000")]
PA_TYPES = {H.INT64: pa.int64(), H.FLOAT64: pa.float64(), H.UTF8: pa.string(), H.BOOLEAN: pa.bool_()}
COUNTERS = ("stage_all_types_batches", "stage_stitch_flushes")
_cache = {}


def the_case(key):
    if key not in _cache:
        _cache[key] = H.build_case(*key)
    return _cache[key]


def raw_batch(piece: H.Piece) -> abi.RawBatch:
    """the piece as the caller-built sqlrs_batch_t it describes: the buffers as they are, null_count as stated"""
    def ptr(a):
        return None if a is None else a.ctypes.data
    cols = [abi.Column(cb.dtype, abi.MEM_HOST, piece.n, cb.null_count if cb.validity is not None else 0, ptr(cb.values),
                       ptr(cb.validity), ptr(cb.offsets)) for cb in piece.cols]
    return abi.RawBatch(cols, piece.n, keepalive=piece)


def arrow_batch(piece: H.Piece, names=H.Case.names) -> pa.RecordBatch:
    """the same rows as an ordinary pyarrow batch (what the oracle is fed)"""
    return pa.RecordBatch.from_arrays([pa.array(cb.logical, type=PA_TYPES[cb.dtype]) for cb in piece.cols], names=list(names))


def counters(be):
    p = be.profile_read()
    return {k: p.get(k, (0, 0))[1] for k in COUNTERS}


def moved(be, before):
    now = counters(be)
    return {k: now[k] - before[k] for k in COUNTERS}


def assert_bit_for_bit(got, exp):
    """values, strings, validity, null_count and row order of two lists of host batches"""
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g.num_rows == e.num_rows and g.num_columns == e.num_columns
        for i in range(g.num_columns):
            a, b = g.column(i), e.column(i)
            assert a.type == b.type and a.null_count == b.null_count, i
            assert (a.buffers()[0] is None) == (b.buffers()[0] is None), i  # no validity at all without NULLs
            assert a.equals(b), i
            if pa.types.is_floating(a.type):
                x, y = a.fill_null(0).to_numpy(zero_copy_only=False), b.fill_null(0).to_numpy(zero_copy_only=False)
                assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), i


def run_three_ways(hip, oracle, case, make, n_host_batches=None):
    """make(backend, batches, flag) -> list of output batches.  Flag off, flag on (with the witnesses) and the oracle."""
    raws = [raw_batch(p) for p in case.pieces]
    off = make(hip, raws, False)
    before = counters(hip)
    on = make(hip, raws, True)
    m = moved(hip, before)
    assert m["stage_all_types_batches"] == (len(raws) if n_host_batches is None else n_host_batches), m
    assert m["stage_stitch_flushes"] >= 1, m
    assert_bit_for_bit(on, off)
    exp = make(oracle, [arrow_batch(p) for p in case.pieces], False)
    assert [b.num_rows for b in on] == [b.num_rows for b in exp]
    for g, e in zip(on, exp):
        for i in range(g.num_columns):
            assert g.column(i).equals(e.column(i)), (case.name, i)  # (every SUM here is over eighths: exact in any order)
    return on


K, V, S, P = (InputRef(i) for i in range(4))
K_MOD_3 = K - (K / Constant(3, abi.INT64)) * Constant(3, abi.INT64)  # k % 3 (k >= 0)
AGGS = [AggFunc("sum", V, abi.FLOAT64), AggFunc("min", V, abi.FLOAT64), AggFunc("max", K, abi.INT64), AggFunc("count", P, abi.INT64),
        AggFunc("min", S, abi.UTF8), AggFunc("count", S, abi.INT64)]


@pytest.mark.parametrize("key", GPU_CASES, ids="/".join)
@pytest.mark.parametrize("group_by", ["s", "p_kmod3"])
def test_hash_agg(hip, oracle, key, group_by):
    gb = [S] if group_by == "s" else [P, K_MOD_3]

    def make(be, batches, flag):
        return list(HashAggExecutor(be, AGGS, gb, batches, stage_all_types=flag).execute())
    run_three_ways(hip, oracle, the_case(key), make)


def model_order(case):
    """ORDER BY s DESC, k — NULLs first, stable — over the logical rows, in plain Python"""
    rows = [tuple(cb.logical[r] for cb in p.cols) for p in case.pieces for r in range(p.n)]
    rows.sort(key=lambda r: r[0])  # k ascending, stable
    nulls = [r for r in rows if r[2] is None]
    rest = sorted((r for r in rows if r[2] is not None), key=lambda r: r[2].encode("utf-8"), reverse=True)  # (reverse keeps ties in order)
    return nulls + rest


@pytest.mark.parametrize("key", GPU_CASES, ids="/".join)
def test_order(hip, oracle, key):
    case = the_case(key)

    def make(be, batches, flag):
        return list(OrderExecutor(be, [OrderBy(S, False), OrderBy(K, True)], batches, stage_all_types=flag).execute())
    (out,) = run_three_ways(hip, oracle, case, make)
    got = list(zip(*[out.column(i).to_pylist() for i in range(4)]))
    assert got == model_order(case)  # stable ties: rows of one (s, k) in order of arrival


def probe_batch(case):
    """a few probe rows over the strings the build side may hold, one that it cannot, one NULL"""
    rng = np.random.default_rng(len(case.name))
    pool = H.POOL + H.MULTI + ["L" * 4999 + "!", "no such string"]
    s = [pool[i] for i in rng.integers(0, len(pool), 24)] + [None]
    return pa.RecordBatch.from_arrays([pa.array(s, type=pa.string()), pa.array(np.arange(len(s), dtype=np.int64))], names=["s", "id"])


@pytest.mark.parametrize("key", GPU_CASES, ids="/".join)
@pytest.mark.parametrize("jt", ["inner", "left"])
def test_hash_join_build_side_in_pieces(hip, oracle, key, jt):
    case = the_case(key)
    probe = probe_batch(case)
    schema = pa.schema([pa.field(f"l.{n}", PA_TYPES[d]) for n, d in zip(case.names, case.dtypes)] + [pa.field(f"r.{f.name}", f.type) for f in probe.schema])

    def make(be, batches, flag):
        return list(HashJoinExecutor(be, batches, [probe], jt, JoinCondition([(S, InputRef(0))]), schema, 4, stage_all_types=flag).execute())
    run_three_ways(hip, oracle, case, make)


@pytest.mark.parametrize("key", GPU_CASES, ids="/".join)
def test_join_agg_probe_side_in_pieces(hip, oracle, key):
    case = the_case(key)
    names = sorted(set(H.POOL + H.MULTI))
    dim = pa.RecordBatch.from_arrays([pa.array(names, type=pa.string()), pa.array(np.arange(len(names), dtype=np.int64) * 10)], names=["name", "w"])
    schema = pa.schema([pa.field("d.name", pa.string()), pa.field("d.w", pa.int64())] + [pa.field(f"f.{n}", PA_TYPES[d]) for n, d in zip(case.names, case.dtypes)])
    cond = JoinCondition([(InputRef(0), InputRef(2))])  # dim.name = fact.s
    aggs = [AggFunc("count", InputRef(2), abi.INT64), AggFunc("sum", InputRef(3), abi.FLOAT64), AggFunc("max", InputRef(1), abi.INT64)]
    gb = [InputRef(0)]

    def make(be, batches, flag):
        if be is oracle:  # (the oracle composes the two operators)
            join = HashJoinExecutor(be, [dim], batches, "inner", cond, schema, 2)
            return list(HashAggExecutor(be, aggs, gb, join.execute()).execute())
        return list(HashJoinAggExecutor(be, [dim], batches, cond, schema, 2, aggs, gb, stage_all_types=flag).execute())
    # the flag on the first build key covers the build side the operator owns too: its one host batch is staged and counted
    run_three_ways(hip, oracle, the_case(key), make, n_host_batches=1 + len(case.pieces))


def small_batch(lo, n, s=None, key=None):
    s = [None if (lo + r) % 5 == 0 else f"g{(lo + r) % 4}" for r in range(n)] if s is None else s
    key = np.full(n, 7, np.int64) if key is None else key
    return pa.RecordBatch.from_arrays([pa.array(key), pa.array(np.arange(lo, lo + n) / 8.0), pa.array(s, type=pa.string()),
                                       pa.array([(lo + r) % 3 == 0 for r in range(n)])], names=list(H.Case.names))


def test_order_of_arrival_across_a_device_batch(hip):
    """two staged host batches, one DEVICE batch, one staged host batch: rows (Order over equal keys) and groups (HashAgg, first
    seen) come out in order of arrival — the device batch flushes the stage first"""
    parts = [small_batch(0, 70), small_batch(70, 3), small_batch(73, 130), small_batch(203, 9)]
    whole = pa.Table.from_batches(parts).combine_chunks().to_batches()[0]
    dev = hip.to_device(parts[2])
    try:
        feed = [parts[0], parts[1], dev, parts[3]]
        before = counters(hip)
        (out,) = OrderExecutor(hip, [OrderBy(K, True)], feed, stage_all_types=True).execute()
        assert moved(hip, before) == {"stage_all_types_batches": 3, "stage_stitch_flushes": 2}
        for i in range(4):
            assert out.column(i).equals(whole.column(i)), i
        before = counters(hip)
        # g2 and g3 are first seen in the device batch, g4 in the host batch behind it
        late = [small_batch(0, 8, ["g0", "g1"] * 4), small_batch(8, 4, ["g1", "g0", None, "g1"]), dev,
                small_batch(203, 9, ["g3", "g4", "g0"] * 3)]
        (agg,) = HashAggExecutor(hip, [AggFunc("count", K, abi.INT64)], [S], late, stage_all_types=True).execute()
        assert moved(hip, before)["stage_all_types_batches"] == 3
        seen = []
        for b in (late[0], late[1], parts[2], late[3]):
            for x in b.column(2).to_pylist():
                if x not in seen:
                    seen.append(x)
        assert agg.column(0).to_pylist() == seen
        assert sum(agg.column(1).to_pylist()) == 8 + 4 + 130 + 9
    finally:
        dev.release()


@pytest.mark.parametrize("op", ["order", "hash_agg"])
def test_schema_change_reports_what_it_reports_without_the_flag(hip, op):
    """a batch whose column type differs from the staged schema's is not staged: same status and last_error as with the flag off"""
    first = small_batch(0, 40)
    other = small_batch(40, 40, key=np.full(40, 7.0))  # Float64 where the staged schema has Int64

    def run(flag):
        ex = (OrderExecutor(hip, [OrderBy(K, True)], [first, other], stage_all_types=flag) if op == "order" else
              HashAggExecutor(hip, [AggFunc("sum", K, abi.INT64)], [S], [first, other], stage_all_types=flag))
        try:
            out = list(ex.execute())
        except abi.ExecutorError as e:
            return e.status, e.message
        return abi.OK, [b.to_pydict() for b in out]
    assert run(True) == run(False)


def decimal_text(keys):
    """the decimal text of non-negative int64 keys below 10^7 as one Utf8 column (offsets, chars), vectorised"""
    digits = (keys.astype(np.int32)[:, None] // 10 ** np.arange(6, -1, -1, dtype=np.int32)) % 10
    keep = np.cumsum(digits != 0, axis=1) > 0
    keep[:, -1] = True  # "0"
    off = np.zeros(len(keys) + 1, np.int32)
    np.cumsum(keep.sum(axis=1), out=off[1:])
    return off, (digits + 48).astype(np.uint8)[keep]


def test_crossing_a_flush(hip):
    """2^22 + 1500 rows in 1024-row batches into Order BY an Int64 permutation key: the stage flushes once on the way and once at
    finish; s = the key's decimal text (NULL at every 97th row), p = key & 1"""
    n, step = (1 << 22) + 1500, 1024
    key = np.random.default_rng(22).permutation(n).astype(np.int64)
    valid = np.arange(n) % 97 != 0
    off, chars = decimal_text(key)
    lens = np.diff(off)
    lens[~valid] = 0  # a NULL row holds no bytes
    keep = np.repeat(valid, np.diff(off))
    chars = chars[keep]
    off = np.zeros(n + 1, np.int32)
    np.cumsum(lens, out=off[1:])
    vbits = np.packbits(valid, bitorder="little")
    pbits = np.packbits((key & 1).astype(bool), bitorder="little")  # 1024 rows = 128 bytes: every batch starts on a byte
    ka, oa, ca, va, pa_ = key.ctypes.data, off.ctypes.data, chars.ctypes.data, vbits.ctypes.data, pbits.ctypes.data
    feed = []
    for lo in range(0, n, step):
        m = min(step, n - lo)
        feed.append(abi.RawBatch([abi.Column(abi.INT64, abi.MEM_HOST, m, 0, ka + 8 * lo, None, None),
                                  abi.Column(abi.UTF8, abi.MEM_HOST, m, -1, ca, va + lo // 8, oa + 4 * lo),  # a window: offsets[0] != 0
                                  abi.Column(abi.BOOLEAN, abi.MEM_HOST, m, 0, pa_ + lo // 8, None, None)], m))
    before = counters(hip)
    (out,) = OrderExecutor(hip, [OrderBy(InputRef(0), True)], feed, stage_all_types=True).execute()
    assert moved(hip, before) == {"stage_all_types_batches": len(feed), "stage_stitch_flushes": 2}
    order = np.argsort(key, kind="stable")
    assert np.array_equal(out.column(0).to_numpy(), key[order])
    exp_valid = valid[order]
    exp_off, exp_chars = decimal_text(np.arange(n, dtype=np.int64))  # the sorted keys are 0 .. n - 1
    exp_keep = np.repeat(exp_valid, np.diff(exp_off))
    exp_lens = np.diff(exp_off)
    exp_lens[~exp_valid] = 0
    s = out.column(1)
    assert s.null_count == int((~valid).sum())
    got_valid = np.unpackbits(np.frombuffer(s.buffers()[0], np.uint8), bitorder="little")[:n].astype(bool)
    got_off = np.frombuffer(s.buffers()[1], np.int32)[:n + 1]
    got_chars = np.frombuffer(s.buffers()[2], np.uint8)[:got_off[-1]]
    got_p = np.unpackbits(np.frombuffer(out.column(2).buffers()[1], np.uint8), bitorder="little")[:n]
    # the 4096 input rows around the flush boundary first: where they went (their key), and what arrived there
    for r in range(n - 4096, n):  # (2596 rows before the boundary, the 1500 behind it)
        at = int(key[r])
        assert bool(got_valid[at]) == bool(valid[r]), r
        text = bytes(got_chars[got_off[at]:got_off[at + 1]])
        assert text == (str(at).encode() if valid[r] else b""), (r, at, text)
        assert int(got_p[at]) == at & 1, r
    assert np.array_equal(got_valid, exp_valid)
    assert np.array_equal(np.diff(got_off), exp_lens) and got_off[0] == 0
    assert np.array_equal(got_chars, exp_chars[exp_keep])
    assert np.array_equal(got_p, (np.arange(n) & 1).astype(np.uint8)) and out.column(2).null_count == 0


def test_flag_off_leaves_the_counters_absent():
    """the same kind of pushes without the flag, on a ctx of their own: neither counter is ever reported"""
    import sqlrs_amd
    be = sqlrs_amd.new_ctx(0)
    try:
        case = the_case(GPU_CASES[2])
        raws = [raw_batch(p) for p in case.pieces]
        list(HashAggExecutor(be, AGGS, [S], raws).execute())
        list(OrderExecutor(be, [OrderBy(S, False), OrderBy(K, True)], raws).execute())
        list(OrderExecutor(be, [OrderBy(K, True)], [small_batch(0, 70), small_batch(70, 3)]).execute())
        prof = be.profile_read()
        assert not set(COUNTERS) & set(prof), prof
        list(OrderExecutor(be, [OrderBy(K, True)], [small_batch(0, 70), small_batch(70, 3)], stage_all_types=True).execute())
        assert be.profile_read()["stage_all_types_batches"][1] == 2  # (and the names are there once the flag is used)
    finally:
        be.close()
