#!/usr/bin/env python
"""sqlrs_range_partition against sqlrs_hash_partition on the same DEVICE batch in one process (HIP events of the library's
timer around each call, median of --reps): (int64 key, f64 value) rows, W parts, the splitters from 1024 samples per
part.  Legs: hash fast path; range fast path with the part read back as a byte (default) and searched again in the
scatter (SQLRS_RANGE_PART_IDS=0); range general path (SQLRS_RANGE_PART_GENERAL=1).  Prints one JSON line per leg and a
summary line with the range / hash ratio of the fast paths.

    python tools/range_partition_bench.py [--rows 1e8] [--parts 8] [--reps 10] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

os.environ.setdefault("SQLRS_HOOKS", "1")  # the A/B legs switch routes through the library's hooks
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (first: torch's HIP runtime is the one the process loads)

import sqlrs_amd  # noqa: E402
from sqlrs_amd import abi  # noqa: E402
from sqlrs_amd.expr import InputRef, OrderBy  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--parts", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, W = int(a.rows), a.parts
    hip = sqlrs_amd.hip(0)
    g = torch.Generator(device="cuda:0").manual_seed(7)
    key = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device="cuda:0", generator=g)
    val = torch.rand(n, dtype=torch.float64, device="cuda:0", generator=g)
    torch.cuda.synchronize()
    batch = abi.RawBatch([abi.device_column(abi.INT64, n, key.data_ptr()), abi.device_column(abi.FLOAT64, n, val.data_ptr())],
                         n, keepalive=(key, val))
    ob = [OrderBy(InputRef(0), asc=True)]
    spl = hip.range_splitters(1, hip.range_sample(batch, ob, 0, 1024 * W), W)

    timer = C.c_void_p()
    hip.check(hip.fn("timer_create")(hip.ctx, C.byref(timer)))

    def timed(call):
        ms, wall = [], []
        for r in range(a.reps + 1):  # the first call warms the pool and the code objects
            hip.check(hip.fn("timer_start")(timer))
            t0 = time.perf_counter()
            out, offs = call()
            hip.check(hip.fn("timer_stop")(timer))
            t1 = time.perf_counter()
            e = C.c_double()
            hip.check(hip.fn("timer_elapsed_ms")(timer, C.byref(e)))
            out.release()
            if r:
                ms.append(e.value)
                wall.append((t1 - t0) * 1e3)
        return statistics.median(ms), statistics.median(wall), offs

    def env(**kv):
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    legs = []
    fast_bytes = n * (8 + 2 * 16)  # histogram pass reads the key; scatter reads and writes both columns
    for name, kv, call, nbytes in [
        ("hash_fast", {}, lambda: hip.hash_partition(batch, InputRef(0), W, abi.MEM_DEVICE), fast_bytes),
        ("range_fast", {}, lambda: hip.range_partition(batch, ob, 0, W, spl), fast_bytes + 2 * n),
        ("range_fast_search", {"SQLRS_RANGE_PART_IDS": "0"}, lambda: hip.range_partition(batch, ob, 0, W, spl), fast_bytes),
        ("range_general", {"SQLRS_RANGE_PART_GENERAL": "1"}, lambda: hip.range_partition(batch, ob, 0, W, spl), None),
    ]:
        env(**kv)
        ms, wall, offs = timed(call)
        env(**{k: None for k in kv})
        rec = {"leg": name, "rows": n, "parts": W, "ms": round(ms, 4), "wall_ms": round(wall, 4),
               "max_part_over_mean": round(max(offs[p + 1] - offs[p] for p in range(W)) * W / n, 4)}
        if nbytes:
            rec["bytes"] = nbytes
            rec["TB_s"] = round(nbytes / (ms * 1e-3) / 1e12, 3)
        legs.append(rec)
        print(json.dumps(rec), flush=True)
    hip.fn("timer_destroy")(timer)
    by = {r["leg"]: r for r in legs}
    summary = {"summary": "range_partition vs hash_partition (fast paths, same batch)",
               "ratio_range_fast_over_hash_fast": round(by["range_fast"]["ms"] / by["hash_fast"]["ms"], 3),
               "ratio_range_fast_search_over_hash_fast": round(by["range_fast_search"]["ms"] / by["hash_fast"]["ms"], 3),
               "target": 1.25}
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in legs + [summary]:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
