"""ORDER BY ... LIMIT over ranks (the distributed selection by tuple bound) on CPU: sqlrs_range_bound through ctypes (host
arithmetic, no device) against its numpy restatement, the statistics behind its slack, and a gloo world-2 run of
distributed_topk with the numpy select and the oracle's Order, whose root result must equal the oracle's Order over the
whole table sliced the same way (a row-id payload column makes the order of ties visible)."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
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
    lb.sqlrs_range_bound.argtypes = [C.c_int, C.c_int64, C.POINTER(C.c_uint64), C.c_int64, C.c_int64, C.c_int,
                                     C.POINTER(C.c_uint64)]
    lb.sqlrs_range_bound.restype = C.c_int
    return lb


def bound_c(lb, num_keys, tuples, total_rows, k, attempt):
    tw = 2 * num_keys + 1
    t = np.ascontiguousarray(np.asarray(tuples, dtype=np.uint64).reshape(-1, tw))
    out = np.full(tw, 7, dtype=np.uint64)
    st = lb.sqlrs_range_bound(num_keys, len(t), t.ctypes.data_as(C.POINTER(C.c_uint64)), total_rows, k, attempt,
                              out.ctypes.data_as(C.POINTER(C.c_uint64)))
    return st, out


def random_tuples(rng, T, num_keys):
    t = np.zeros((T, 2 * num_keys + 1), dtype=np.uint64)
    for q in range(num_keys):
        t[:, 2 * q] = (rng.random(T) > 0.1).astype(np.uint64)
        t[:, 2 * q + 1] = np.where(t[:, 2 * q] == 1, rng.integers(0, 40, T).astype(np.uint64) << np.uint64(58), 0)
    t[:, -1] = rng.permutation(T * 3)[:T].astype(np.uint64)  # distinct positions
    return t


def test_bound_equals_numpy():
    lb = lib()
    rng = np.random.default_rng(3)
    checked = 0
    for T in (0, 1, 5, 64, 1000, 8192):
        for num_keys in (1, 2):
            t = random_tuples(rng, T, num_keys)
            for N in (1, 10, 999, 10_000, 10 ** 7, 10 ** 12):
                for k in (-3, 0, 1, 2, 7, 100, N // 3, N - 1, N, N + 5):
                    for attempt in (0, 1, 2, 5, 40):
                        st, got = bound_c(lb, num_keys, t, N, k, attempt)
                        assert st == 0
                        exp = D.range_bound_numpy(t, N, k, attempt)
                        assert np.array_equal(got, exp), (T, N, k, attempt)
                        checked += 1
    assert checked == 3600


def test_bound_edges():
    lb = lib()
    t = random_tuples(np.random.default_rng(1), 500, 1)
    st, b = bound_c(lb, 1, t, 1000, 0, 0)
    assert st == 0 and (b == 0).all()              # k = 0: keeps nothing
    st, b = bound_c(lb, 1, t, 1000, 1000, 0)
    assert st == 0 and (b == ALL_ONES).all()       # k >= N: keeps every row
    st, b = bound_c(lb, 1, t, 1000, 5000, 0)
    assert st == 0 and (b == ALL_ONES).all()
    st, b = bound_c(lb, 1, np.zeros((0, 3), np.uint64), 1000, 10, 0)
    assert st == 0 and (b == ALL_ONES).all()       # no tuples
    # j = (c + ceil(2 sqrt c) + 2) 4^a - 1 with c = ceil(k T / N): k = 10, T = 500, N = 1000 -> c = 5, j = 11
    srt = t[np.lexsort(t.T[::-1])]
    st, b = bound_c(lb, 1, t, 1000, 10, 0)
    assert st == 0 and np.array_equal(b, srt[11])
    st, b = bound_c(lb, 1, t, 1000, 10, 1)
    assert st == 0 and np.array_equal(b, srt[47])


def test_bound_monotone_and_reaches_all_ones():
    lb = lib()
    rng = np.random.default_rng(2)
    for T, N, k in [(8192, 10 ** 7, 1000), (300, 5000, 1), (1, 10, 3), (4096, 10 ** 9, 10 ** 6), (64, 100, 99)]:
        t = random_tuples(rng, T, 2)
        prev, a = None, 0
        while True:
            st, b = bound_c(lb, 2, t, N, k, a)
            assert st == 0
            if prev is not None:
                assert tuple(prev.tolist()) <= tuple(b.tolist())  # nondecreasing in the attempt
            if (b == ALL_ONES).all():
                break
            prev, a = b, a + 1
            assert a < 40
        assert a <= 1 + int(np.log(T) / np.log(4)) + 1
        st, b = bound_c(lb, 2, t, N, k, a + 3)
        assert (b == ALL_ONES).all()                    # stays there


def test_bound_rejects_bad_arguments():
    lb = lib()
    t = np.zeros((4, 3), np.uint64)
    out = np.zeros(3, np.uint64)
    tp, op = t.ctypes.data_as(C.POINTER(C.c_uint64)), out.ctypes.data_as(C.POINTER(C.c_uint64))
    assert lb.sqlrs_range_bound(0, 4, tp, 10, 1, 0, op) != 0     # no key
    assert lb.sqlrs_range_bound(1, -1, tp, 10, 1, 0, op) != 0    # negative count
    assert lb.sqlrs_range_bound(1, 4, None, 10, 1, 0, op) != 0   # no tuples
    assert lb.sqlrs_range_bound(1, 4, tp, -1, 1, 0, op) != 0     # negative total
    assert lb.sqlrs_range_bound(1, 4, tp, 10, 1, -1, op) != 0    # negative attempt
    assert lb.sqlrs_range_bound(1, 4, tp, 10, 1, 0, None) != 0   # no output
    assert lb.sqlrs_range_bound(1, 0, None, 10, 1, 0, op) == 0   # no tuples is fine: all ones


def test_bound_slack_keeps_second_attempts_rare():
    """the slack grows with sqrt(c): on random keys (1e7 rows, 8192 samples) the first bound keeps fewer than k rows in
    <= 2.5 % of the draws for k = 1e3 .. 1e5; a constant slack of 2 (j = c + 1) would miss in 6 - 45 %"""
    rng = np.random.default_rng(0)
    N, T, trials = 10_000_000, 8192, 400
    for k in (1000, 10_000, 100_000):
        c = -(-k * T // N)
        j = D.range_bound_index(T, N, k, 0)
        short = const2 = 0
        for _ in range(trials):
            srt = np.sort(rng.choice(N, T, replace=False))  # ranks of the sampled rows among all rows
            short += srt[j] < k                             # rows strictly below the bound = its rank
            const2 += srt[c + 1] < k
        assert short / trials <= 0.025, (k, short)
        assert const2 > 4 * short, (k, short, const2)


def test_numpy_select_keeps_rows_below_the_bound_in_input_order():
    rng = np.random.default_rng(4)
    n = 3000
    keys = [(rng.integers(0, 7, n, dtype=np.int64), rng.random(n) > 0.2, False)]
    t = D.range_tuples_numpy(keys, 500)
    srt = t[np.lexsort(t.T[::-1])]
    for j in (0, 1, 100, 2999):
        (rid,) = D.range_select_numpy([np.arange(n)], t, srt[j])
        assert len(rid) == j and (np.diff(rid) > 0).all()
        assert {tuple(r) for r in t[rid].tolist()} == {tuple(r) for r in srt[:j].tolist()}
    assert len(D.range_select_numpy([np.arange(n)], t, np.zeros(3, np.uint64))[0]) == 0
    assert len(D.range_select_numpy([np.arange(n)], t, np.full(3, ALL_ONES, np.uint64))[0]) == n


# ---- gloo world 2: distributed_topk with the numpy select and the oracle's Order -------------------------------------
N = 6000
SPR = 64  # samples per rank
CUTS = [0, N // 3, N]
# name: (table shape, k = offset + limit, offset, rank cuts)
CASES = {
    "ties": ("ties", 137, 37, CUTS),
    "null_keys": ("nulls", 300, 0, CUTS),
    "desc_f64": ("f64_desc", 50, 5, CUTS),
    "two_keys": ("two_keys", 500, 100, CUTS),
    "empty_slice": ("ties", 123, 0, [0, 0, N]),
    "k0": ("ties", 0, 0, CUTS),
    "k1": ("nulls", 1, 0, CUTS),
    "k_past_n": ("two_keys", N + 5, 10, CUTS),
    "narrow_first_bound": ("narrow", 200, 0, CUTS),
}


def make_table(shape, cuts):
    """-> (columns [(name, values, valid or None)], order_by [(column index, asc)]); the last column is the row id"""
    rng = np.random.default_rng(len(shape))
    rid = np.arange(N, dtype=np.int64)
    if shape == "ties":
        return [("k", rng.integers(0, 20, N, dtype=np.int64), None), ("rid", rid, None)], [(0, True)]
    if shape == "nulls":
        k = rng.integers(-50, 50, N, dtype=np.int64)
        return [("k", k, rng.random(N) > 0.3), ("v", rng.random(N), None), ("rid", rid, None)], [(0, True)]
    if shape == "f64_desc":
        k = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.5, -2.5, 1e300]), N)
        return [("k", k, None), ("rid", rid, None)], [(0, False)]
    if shape == "two_keys":
        a = rng.integers(0, 10, N, dtype=np.int64)
        b = rng.random(N).round(1)
        return [("a", a, rng.random(N) > 0.15), ("b", b, rng.random(N) > 0.25), ("rid", rid, None)], [(0, False), (1, True)]
    if shape == "narrow":
        # every row distributed_topk samples holds a tiny key, no other row does: the first bounds keep almost nothing
        k = rng.integers(1 << 20, 1 << 30, N, dtype=np.int64)
        total, world = cuts[-1], len(cuts) - 1
        for r in range(world):
            n_r = cuts[r + 1] - cuts[r]
            want = -(-SPR * world * n_r // total)
            k[cuts[r] + D.range_sample_rows(n_r, want)] = -5
        return [("k", k, None), ("rid", rid, None)], [(0, True)]
    raise ValueError(shape)


def oracle_order(oracle, batch, order_by):
    from sqlrs_amd.executor import OrderExecutor
    from sqlrs_amd.expr import InputRef, OrderBy
    if batch.num_rows == 0:
        return batch
    (out,) = list(OrderExecutor(oracle, [OrderBy(InputRef(c), asc=a) for c, a in order_by], [batch]).execute())
    return out


def run_case(rank, world, oracle, name):
    import pyarrow as pa
    shape, k, offset, cuts = CASES[name]
    cols, order_by = make_table(shape, cuts)
    lo, hi = cuts[rank], cuts[rank + 1]
    mine = [(nm, v[lo:hi], None if ok is None else ok[lo:hi]) for nm, v, ok in cols]
    keys = [(mine[c][1], mine[c][2], asc) for c, asc in order_by]

    def allgather(obj):
        out = [None] * world
        dist.all_gather_object(out, obj)
        return out

    def sample(row_base, m):
        return D.range_tuples_numpy(keys, row_base, D.range_sample_rows(hi - lo, m))

    def select(row_base, bound):
        t = D.range_tuples_numpy(keys, row_base)
        data = [v for _, v, _ in mine] + [np.ones(hi - lo, bool) if ok is None else ok for _, _, ok in mine]
        got = D.range_select_numpy(data, t, bound)
        return got, len(got[0])

    def gather_to_root(cand, count):
        pieces = allgather(cand)  # the candidates of rank 0, 1, ... (only the root keeps them)
        nc = len(mine)
        return [(mine[c][0], np.concatenate([p[c] for p in pieces]), np.concatenate([p[nc + c] for p in pieces]))
                for c in range(nc)]

    def order(received, limit):
        b = pa.RecordBatch.from_arrays([pa.array(v, mask=~ok) for _, v, ok in received], names=[nm for nm, _, _ in received])
        return oracle_order(oracle, b, order_by)

    res, info = D.distributed_topk(hi - lo, world, rank, k=k, allgather=allgather, sample=sample, select=select,
                                   gather_to_root=gather_to_root, order=order, samples_per_rank=SPR)
    if rank != 0:
        assert res is None
        return None
    need = min(k, N)
    got = pa.Table.from_batches([res]).to_pylist()[:need] if res.num_rows else []
    assert len(got) == need and info["candidates"] >= need and info["total_rows"] == N
    arrs = [pa.array(v, mask=None if ok is None else ~ok) for _, v, ok in cols]
    exp = pa.Table.from_batches([oracle_order(oracle, pa.RecordBatch.from_arrays(arrs, names=[nm for nm, _, _ in cols]),
                                              order_by)]).to_pylist()
    # the first min(k, N) rows, ties in the global order (row ids); then OFFSET / LIMIT on both
    assert [r["rid"] for r in got] == [r["rid"] for r in exp[:need]], name
    assert [r["rid"] for r in got[offset:k]] == [r["rid"] for r in exp[offset:k]], name
    return info


def worker(rank, world, port, result_path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle_backend import load_oracle
    oracle = load_oracle()
    lines = []
    for name in CASES:
        info = run_case(rank, world, oracle, name)
        if rank == 0:
            lines.append(f"{name} {info['attempts']} {info['candidates']}")
    if rank == 0:
        with open(result_path, "w") as f:
            f.write("\n".join(lines))
    dist.barrier()
    dist.destroy_process_group()


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_distributed_topk_world2_gloo(tmp_path):
    result = tmp_path / "result.txt"
    mp.spawn(worker, args=(2, free_port(), str(result)), nprocs=2, join=True)
    stats = {ln.split()[0]: (int(ln.split()[1]), int(ln.split()[2])) for ln in result.read_text().splitlines()}
    assert set(stats) == set(CASES)
    assert stats["narrow_first_bound"][0] > 0       # attempt 0 kept too few rows: the bound widened
    assert stats["k0"] == (0, 0)                     # nothing travels
    assert stats["k_past_n"][1] == N                 # every row travels
    for name in ("ties", "null_keys", "desc_f64", "empty_slice"):
        assert stats[name][1] < N // 2, (name, stats[name])  # only candidates travel
