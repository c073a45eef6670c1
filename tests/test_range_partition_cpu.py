"""The multi-GPU ORDER BY (range partition + exchange + local Order) on CPU: sqlrs_range_splitters through ctypes (host
arithmetic, no device), the invariants of the numpy restatement of the range partition, and a gloo world-2 run of
distributed_order with the numpy partition and the oracle's Order whose concatenated rank outputs must equal the oracle's
Order over the whole table (a row-id payload column makes the order of ties visible)."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from sqlrs_amd import distributed as D  # noqa: E402

ALL_ONES = (1 << 64) - 1


def lib():
    from sqlrs_amd import build as B
    lb = C.CDLL(B.OUT)
    lb.sqlrs_range_splitters.argtypes = [C.c_int, C.c_int64, C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_uint64)]
    lb.sqlrs_range_splitters.restype = C.c_int
    lb.sqlrs_range_tuple_words.argtypes = [C.c_int]
    lb.sqlrs_range_tuple_words.restype = C.c_int
    return lb


def splitters_c(num_keys, tuples, parts):
    tw = 2 * num_keys + 1
    t = np.ascontiguousarray(np.asarray(tuples, dtype=np.uint64).reshape(-1, tw))
    out = np.zeros((max(parts - 1, 1), tw), dtype=np.uint64)
    st = lib().sqlrs_range_splitters(num_keys, len(t), t.ctypes.data_as(C.POINTER(C.c_uint64)), parts,
                                     out.ctypes.data_as(C.POINTER(C.c_uint64)))
    return st, out[:parts - 1]


def test_tuple_words():
    lb = lib()
    assert [lb.sqlrs_range_tuple_words(k) for k in (1, 2, 3)] == [3, 5, 7]
    assert lb.sqlrs_range_tuple_words(0) < 0


@pytest.mark.parametrize("parts", [1, 2, 7, 8, 256])
def test_splitters_are_sorted_quantiles(parts):
    rng = np.random.default_rng(parts)
    t = np.stack([np.ones(5000, np.uint64), rng.integers(0, 1 << 63, 5000).astype(np.uint64) * np.uint64(2),
                  np.arange(5000, dtype=np.uint64)], axis=1)
    st, sp = splitters_c(1, t, parts)
    assert st == 0 and sp.shape == (parts - 1, 3)
    srt = t[np.lexsort(t.T[::-1])]
    for j in range(1, parts):  # the (j * T // W)-th smallest tuple
        assert (sp[j - 1] == srt[j * len(t) // parts]).all()
    assert (sp == D.range_splitters_numpy(t, parts)).all()
    for j in range(1, parts - 1):  # nondecreasing (lexicographic)
        assert tuple(sp[j - 1]) <= tuple(sp[j])


def test_splitters_lexicographic_on_later_words():
    """ties on the first words are broken by the later ones (validity, key, ..., position)"""
    t = np.array([[1, 5, 9], [1, 5, 2], [0, 0, 7], [1, 4, 100], [1, 5, 3]], dtype=np.uint64)
    st, sp = splitters_c(1, t, 5)
    assert st == 0
    assert sp.tolist() == [[1, 4, 100], [1, 5, 2], [1, 5, 3], [1, 5, 9]]


def test_splitters_repeat_when_fewer_tuples_than_parts():
    t = np.array([[1, 10, 0], [1, 20, 1], [1, 30, 2]], dtype=np.uint64)
    st, sp = splitters_c(1, t, 8)
    assert st == 0
    picks = [t[j * 3 // 8] for j in range(1, 8)]
    assert sp.tolist() == [p.tolist() for p in picks]
    assert len({tuple(r) for r in sp.tolist()}) < 7  # repeated splitters: some parts stay empty


def test_splitters_without_tuples_send_everything_to_part_0():
    st, sp = splitters_c(2, np.zeros((0, 5), np.uint64), 4)
    assert st == 0 and (sp == np.uint64(ALL_ONES)).all() and sp.shape == (3, 5)
    cols, offs = D.range_partition_numpy([np.arange(10)], D.range_tuples_numpy([(np.arange(10), None, False),
                                                                                (np.arange(10) % 3 == 0, None, True)], 0), sp)
    assert offs == [0, 10, 10, 10, 10]


def test_splitters_reject_bad_arguments():
    lb = lib()
    t = np.zeros((4, 3), np.uint64)
    out = np.zeros((300, 3), np.uint64)
    tp, op = t.ctypes.data_as(C.POINTER(C.c_uint64)), out.ctypes.data_as(C.POINTER(C.c_uint64))
    assert lb.sqlrs_range_splitters(1, 4, tp, 0, op) != 0      # num_parts < 1
    assert lb.sqlrs_range_splitters(1, 4, tp, 257, op) != 0    # num_parts > 256
    assert lb.sqlrs_range_splitters(1, 4, tp, 2, None) != 0    # no splitter array
    assert lb.sqlrs_range_splitters(1, 4, None, 2, op) != 0    # no tuples
    assert lb.sqlrs_range_splitters(1, -1, tp, 2, op) != 0     # negative count
    assert lb.sqlrs_range_splitters(0, 4, tp, 2, op) != 0      # no key
    assert lb.sqlrs_range_splitters(1, 4, tp, 1, None) == 0    # one part: nothing to write


def test_numpy_partition_invariants():
    """parts are contiguous in tuple order (every tuple of part p is below every tuple of part p + 1, on the right side of
    the splitters) and input order is kept inside a part"""
    rng = np.random.default_rng(5)
    n = 20_000
    k1 = rng.integers(-50, 50, n).astype(np.int32)
    k2 = rng.random(n)
    v2 = rng.random(n) > 0.1
    keys = [(k1, None, False), (k2, v2, True)]
    t = D.range_tuples_numpy(keys, 1234)
    sample = t[D.range_sample_rows(n, 300)]
    for parts in (1, 2, 7, 8):
        sp = D.range_splitters_numpy(sample, parts)
        rows = np.arange(n)
        (prow, pt), offs = D.range_partition_numpy([rows, np.arange(n)], t, sp)
        assert offs[0] == 0 and offs[-1] == n and all(offs[p] <= offs[p + 1] for p in range(parts))
        tl = [tuple(r) for r in t.tolist()]
        for p in range(parts):
            seg = prow[offs[p]:offs[p + 1]]
            assert (np.diff(seg) > 0).all()  # input order inside a part
            for r in seg[:50].tolist() + seg[-50:].tolist():
                if p > 0:
                    assert tuple(sp[p - 1].tolist()) <= tl[r]
                if p < parts - 1:
                    assert tl[r] < tuple(sp[p].tolist())
        # contiguous in tuple order: the largest tuple of a part is below the smallest of the next non-empty one
        nonempty = [p for p in range(parts) if offs[p + 1] > offs[p]]
        for a, b in zip(nonempty, nonempty[1:]):
            assert max(tl[r] for r in prow[offs[a]:offs[a + 1]]) < min(tl[r] for r in prow[offs[b]:offs[b + 1]])


def test_key_encoding_orders_like_the_local_order():
    """-0.0 < +0.0, NaN beyond +inf (IEEE total order, what the Order sorts by), int32 widened, DESC complemented"""
    f = np.array([np.nan, np.inf, 1.0, 0.0, -0.0, -1.0, -np.inf], dtype=np.float64)
    u = D.ordered_key_np(f)
    assert (np.diff(u.astype(object)) < 0).all()  # strictly decreasing as listed
    i = np.array([-(1 << 31), -1, 0, 1, (1 << 31) - 1], dtype=np.int32)
    assert (D.ordered_key_np(i) == D.ordered_key_np(i.astype(np.int64))).all()
    t = D.range_tuples_numpy([(i, None, False)], 0)
    assert (np.diff(t[:, 1].astype(object)) < 0).all()


# ---- gloo world 2: distributed_order with the numpy partition and the oracle's Order ---------------------------------
N = 6000
CASES = ["i64_asc", "i64_desc", "f64_specials_desc", "i32_asc", "two_keys_nulls", "all_equal"]


def make_table(case):
    """-> (columns [(name, values, valid or None)], order_by [(column index, asc)]); the last column is the row id"""
    rng = np.random.default_rng(CASES.index(case) + 11)
    rid = np.arange(N, dtype=np.int64)
    if case in ("i64_asc", "i64_desc"):
        k = rng.integers(-300, 300, N, dtype=np.int64)  # many ties
        return [("k", k, None), ("v", rng.random(N), None), ("rid", rid, None)], [(0, case == "i64_asc")]
    if case == "f64_specials_desc":
        k = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.5, -2.5, 1e300]), N)
        return [("k", k, None), ("rid", rid, None)], [(0, False)]
    if case == "i32_asc":
        k = rng.integers(-(1 << 31), (1 << 31) - 1, N).astype(np.int32)
        k[::7] = -1
        return [("k", k, None), ("rid", rid, None)], [(0, True)]
    if case == "two_keys_nulls":
        a = rng.integers(0, 20, N, dtype=np.int64)
        b = rng.random(N).round(1)
        return [("a", a, rng.random(N) > 0.15), ("b", b, rng.random(N) > 0.25), ("rid", rid, None)], [(0, False), (1, True)]
    if case == "all_equal":
        return [("k", np.full(N, 42, dtype=np.int64), None), ("rid", rid, None)], [(0, True)]
    raise ValueError(case)


def to_batch(cols, lo, hi):
    import pyarrow as pa
    arrs = [pa.array(v[lo:hi], mask=None if ok is None else ~ok[lo:hi]) for _, v, ok in cols]
    return pa.RecordBatch.from_arrays(arrs, names=[nm for nm, _, _ in cols])


def oracle_order(oracle, batch, order_by):
    from sqlrs_amd.executor import OrderExecutor
    from sqlrs_amd.expr import InputRef, OrderBy
    if batch.num_rows == 0:
        return batch
    (out,) = list(OrderExecutor(oracle, [OrderBy(InputRef(c), asc=a) for c, a in order_by], [batch]).execute())
    return out


def worker(rank, world, port, result_path, case, cuts):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import pyarrow as pa
    from oracle_backend import load_oracle
    oracle = load_oracle()
    cols, order_by = make_table(case)
    lo, hi = cuts[rank], cuts[rank + 1]
    mine = [(nm, v[lo:hi], None if ok is None else ok[lo:hi]) for nm, v, ok in cols]
    keys = [(mine[c][1], mine[c][2], asc) for c, asc in order_by]

    def allgather(obj):
        out = [None] * world
        dist.all_gather_object(out, obj)
        return out

    def sample(row_base, m):
        return D.range_tuples_numpy(keys, row_base, D.range_sample_rows(hi - lo, m))

    def partition(row_base, splitters):
        t = D.range_tuples_numpy(keys, row_base)
        data = [v for _, v, _ in mine] + [np.ones(hi - lo, bool) if ok is None else ok for _, _, ok in mine]
        return D.range_partition_numpy(data, t, splitters)

    def exchange(parts, offsets):
        tens = [torch.from_numpy(np.ascontiguousarray(p.view(np.uint8) if p.dtype == np.bool_ else p)) for p in parts]
        got = [t.numpy() for t in D.all_to_all_columns(dist, tens, offsets, world, torch)]
        nc = len(mine)
        return [(mine[c][0], got[c], got[nc + c].astype(bool)) for c in range(nc)]

    def order(received):
        b = pa.RecordBatch.from_arrays([pa.array(v, mask=~ok) for _, v, ok in received], names=[nm for nm, _, _ in received])
        return oracle_order(oracle, b, order_by)

    piece = D.distributed_order(hi - lo, world, rank, allgather=allgather, sample=sample, partition=partition,
                                exchange=exchange, order=order, samples_per_rank=64)
    pieces = allgather(piece.to_pylist() if hasattr(piece, "to_pylist") else pa.Table.from_batches([piece]).to_pylist())
    if rank == 0:
        got = [row for p in pieces for row in p]
        exp = oracle_order(oracle, to_batch(cols, 0, N), order_by)
        exp_rows = pa.Table.from_batches([exp]).to_pylist()
        assert len(got) == N
        # row ids make the order of ties visible; float keys compared by bit pattern (NaN, -0.0)
        assert [r["rid"] for r in got] == [r["rid"] for r in exp_rows]
        with open(result_path, "w") as f:
            f.write(f"ok {[len(p) for p in pieces]}")
    dist.barrier()
    dist.destroy_process_group()


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("case", CASES)
def test_distributed_order_world2_gloo(tmp_path, case):
    result = tmp_path / "result.txt"
    cuts = [0, N // 3, N]  # uneven slices
    mp.spawn(worker, args=(2, free_port(), str(result), case, cuts), nprocs=2, join=True)
    text = result.read_text()
    assert text.startswith("ok")
    sizes = eval(text[3:])
    assert min(sizes) > 0  # both ranks received rows (the all-equal keys too: the position breaks the ties)


def test_distributed_order_world2_gloo_one_empty_slice(tmp_path):
    result = tmp_path / "result.txt"
    mp.spawn(worker, args=(2, free_port(), str(result), "two_keys_nulls", [0, 0, N]), nprocs=2, join=True)
    assert result.read_text().startswith("ok")
