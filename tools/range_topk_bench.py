#!/usr/bin/env python
"""sqlrs_range_select (the per-rank step of ORDER BY ... LIMIT over ranks) against sqlrs_range_partition (2 and 8 parts,
the full ORDER BY's step) and against a local Order with sqlrs_order_set_limit, on the same DEVICE batch in one process
(HIP events of the library's timer around each call, median of --reps).  Shape of tools/range_partition_bench.py: 1e8
rows of (int64 key, f64 value); the select's bound is sqlrs_range_bound's first bound for k = --k from 65536 samples
(about 1e4 rows kept).  A second shape runs the select over two keys with NULLs (int64 with 10 % NULLs DESC, f64 with
NULLs) and a third column.  Prints one JSON line per leg.

    python tools/range_topk_bench.py [--rows 1e8] [--k 2000] [--reps 10] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (first: torch's HIP runtime is the one the process loads)

import sqlrs_amd  # noqa: E402
from sqlrs_amd import abi  # noqa: E402
from sqlrs_amd.expr import InputRef, OrderBy  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--k", type=int, default=2000)
    ap.add_argument("--samples", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, k = int(a.rows), a.k
    hip = sqlrs_amd.hip(0)
    g = torch.Generator(device="cuda:0").manual_seed(7)
    key = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device="cuda:0", generator=g)
    val = torch.rand(n, dtype=torch.float64, device="cuda:0", generator=g)
    torch.cuda.synchronize()
    batch = abi.RawBatch([abi.device_column(abi.INT64, n, key.data_ptr()), abi.device_column(abi.FLOAT64, n, val.data_ptr())],
                         n, keepalive=(key, val))
    ob = [OrderBy(InputRef(0), asc=True)]
    bound = hip.range_bound(1, hip.range_sample(batch, ob, 0, a.samples), n, k, 0)

    timer = C.c_void_p()
    hip.check(hip.fn("timer_create")(hip.ctx, C.byref(timer)))

    def timed(call):
        ms, wall, rows = [], [], None
        for r in range(a.reps + 1):  # the first call warms the pool and the code objects
            hip.check(hip.fn("timer_start")(timer))
            t0 = time.perf_counter()
            out = call()
            hip.check(hip.fn("timer_stop")(timer))
            t1 = time.perf_counter()
            e = C.c_double()
            hip.check(hip.fn("timer_elapsed_ms")(timer, C.byref(e)))
            rows = out.num_rows
            out.release()
            if r:
                ms.append(e.value)
                wall.append((t1 - t0) * 1e3)
        return statistics.median(ms), statistics.median(wall), rows

    def order_limit(b, order_by):
        arr, _keep = hip._order_by_array(order_by)
        h = C.c_void_p()
        hip.check(hip.fn("order_create")(hip.ctx, len(order_by), arr, C.byref(h)))
        try:
            hip.check(hip.fn("order_set_limit")(h, k))
            hip.check(hip.fn("order_push")(h, abi.as_batch(b).ptr))
            out = C.POINTER(abi.Batch)()
            hip.check(hip.fn("order_finish")(h, abi.MEM_DEVICE, C.byref(out)))
            return hip.wrap(out)
        finally:
            hip.fn("order_destroy")(h)

    def part(W):
        spl = hip.range_splitters(1, hip.range_sample(batch, ob, 0, 1024 * W), W)
        return lambda: hip.range_partition(batch, ob, 0, W, spl)[0]

    legs = []

    def leg(name, call, nbytes, **extra):
        ms, wall, rows = timed(call)
        rec = {"leg": name, "rows": n, "ms": round(ms, 4), "wall_ms": round(wall, 4), "out_rows": rows, **extra}
        if nbytes:
            rec["bytes"] = nbytes
            rec["TB_s"] = round(nbytes / (ms * 1e-3) / 1e12, 3)
        legs.append(rec)
        print(json.dumps(rec), flush=True)

    # select: the key once (8 B / row) + the mask (1 bit / row, written, read by the tile offsets) + the kept rows
    leg("select", lambda: hip.range_select(batch, ob, 0, bound), 8 * n + 2 * n // 8, k=k, samples=a.samples)
    leg("range_partition_2", part(2), None)
    leg("range_partition_8", part(8), None)
    leg("order_set_limit", lambda: order_limit(batch, ob), None, k=k)

    # general shape: two keys with NULLs and a third column
    ka = torch.randint(0, 1 << 40, (n,), dtype=torch.int64, device="cuda:0", generator=g)
    kb = torch.rand(n, dtype=torch.float64, device="cuda:0", generator=g)
    nb = (n + 63) // 64
    va = torch.randint(-(1 << 62), 1 << 62, (nb,), dtype=torch.int64, device="cuda:0", generator=g)
    va = va | (va >> 1) | (va >> 2)  # ~ 7 / 8 of the bits set
    vb = torch.full((nb,), -1, dtype=torch.int64, device="cuda:0")
    vb[::3] = va[::3]
    torch.cuda.synchronize()
    b2 = abi.RawBatch([abi.device_column(abi.INT64, n, ka.data_ptr(), va.data_ptr(), -1),
                       abi.device_column(abi.FLOAT64, n, kb.data_ptr(), vb.data_ptr(), -1),
                       abi.device_column(abi.FLOAT64, n, val.data_ptr())], n, keepalive=(ka, kb, va, vb, val))
    ob2 = [OrderBy(InputRef(0), asc=False), OrderBy(InputRef(1), asc=True)]
    bound2 = hip.range_bound(2, hip.range_sample(b2, ob2, 0, a.samples), n, k, 0)
    leg("select_two_keys_nulls", lambda: hip.range_select(b2, ob2, 0, bound2), None, k=k, samples=a.samples)
    leg("order_set_limit_two_keys_nulls", lambda: order_limit(b2, ob2), None, k=k)
    hip.fn("timer_destroy")(timer)
    if a.out:
        with open(a.out, "w") as f:
            for r in legs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
