#!/usr/bin/env python
"""Aggregates without GROUP BY with SQLRS_SIMPLE_AGG_REDUCE (the flag on the first entry of sqlrs_simple_agg_create) off and on,
alternating in one process (HIP events of the library's timer around push ... finish).  The off leg is the code without the
switch: a HashAgg over one constant key, a WHERE below it handed to that operator (the SQLRS_SIMPLE_AGG_FILTER entry) — or, with
--lib (an older build of the library, which knows neither flag: off positions only), run as a Filter operator in front of
every push, which is what that library's callers do.

Legs over --rows DEVICE rows of {i int64 uniform in [0, 1000), f float64, g float64 uniform in [0, 1)}, pushed as one batch:
    sum_f             sum(f)
    four_cells_f      count(f), sum(f), min(f), max(f)
    q6_shape          sum(f * g) WHERE i >= 100 AND i < 140 AND g < 0.5        (2 % of the rows)
and one over --host-rows rows of the same columns as 1024-row HOST batches (the reference's batch shape, csv.rs:105):
    host_1024         count(f), sum(f), min(f), max(f)

5 warm-ups, then --reps runs per leg and switch position.  Prints one JSON line per leg: median ms and max - min spread of
either position, on_over_off, and for the on position the bytes of the referenced columns over the median as a fraction of
8 TB/s (q6_shape: i and g of every row, f of the kept rows).

    python tools/simple_agg_bench.py [--rows 1e8] [--host-rows 2e6] [--reps 20] [--lib PATH] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import pyarrow as pa  # noqa: E402
import torch  # noqa: E402,F401  (first: torch's HIP runtime is the one the process loads)

import sqlrs_amd  # noqa: E402
from sqlrs_amd import abi  # noqa: E402
from sqlrs_amd.expr import AggFunc, Constant, InputRef  # noqa: E402

WARMUPS = 5
I, F, G = 0, 1, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--host-rows", type=float, default=2e6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lib", default=None, help="another build of libsqlrs_hip.so (an older one: off positions only)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hip = abi.Backend(a.lib, "sqlrs_", 0) if a.lib else sqlrs_amd.hip(0)
    can_reduce = can_filter = a.lib is None
    timer = C.c_void_p()
    hip.check(hip.fn("timer_create")(hip.ctx, C.byref(timer)))

    def table(n, seed):
        rng = np.random.default_rng(seed)
        return pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 1000, n, dtype=np.int64)), pa.array(rng.standard_normal(n)),
                                           pa.array(rng.random(n))], names=["i", "f", "g"])

    def one_run(batches, aggs, flt, on):
        """ms from in front of the first push to behind finish, and the one output row"""
        keep = []
        funcs = [x.abi_struct(keep) for x in aggs]
        pf = flt.pack() if flt is not None else None
        if pf is not None and can_filter:
            funcs.append(abi.AggFunc(0, 0, 0, abi.SIMPLE_AGG_FILTER, pf.abi))
        if on:
            funcs[0].reserved |= abi.SIMPLE_AGG_REDUCE
        arr = (abi.AggFunc * len(funcs))(*funcs)
        h, f = C.c_void_p(), C.c_void_p()
        hip.check(hip.fn("simple_agg_create")(hip.ctx, len(funcs), arr, C.byref(h)))
        try:
            if pf is not None and not can_filter:
                hip.check(hip.fn("filter_create")(hip.ctx, C.byref(pf.abi), C.byref(f)))
            hip.check(hip.fn("timer_start")(timer))
            for b in batches:
                if f:
                    kept = C.POINTER(abi.Batch)()
                    hip.check(hip.fn("filter_push")(f, b.ptr, abi.MEM_DEVICE, C.byref(kept)))
                    hip.check(hip.fn("simple_agg_push")(h, kept))
                    hip.fn("batch_release")(kept)
                else:
                    hip.check(hip.fn("simple_agg_push")(h, b.ptr))
            out = C.POINTER(abi.Batch)()
            hip.check(hip.fn("simple_agg_finish")(h, abi.MEM_HOST, C.byref(out)))
            hip.check(hip.fn("timer_stop")(timer))
            e = C.c_double()
            hip.check(hip.fn("timer_elapsed_ms")(timer, C.byref(e)))
            lb = hip.wrap(out)
            row = [c.to_pylist()[0] for c in lb.to_arrow().columns]
            lb.release()
            return e.value, row
        finally:
            hip.fn("simple_agg_destroy")(h)
            if f:
                hip.fn("filter_destroy")(f)

    legs = []

    def leg(name, batches, rows, aggs, flt, bytes_per_row):
        rec = {"leg": name, "rows": rows, "batches": len(batches)}
        positions = [False, True] if can_reduce else [False]
        for on in positions:
            for _ in range(WARMUPS):
                one_run(batches, aggs, flt, on)
        ms = {False: [], True: []}
        for _ in range(a.reps):  # off, on, off, on, ...
            for on in positions:
                t, row = one_run(batches, aggs, flt, on)
                ms[on].append(t)
                rec["on_row" if on else "off_row"] = row
        for on in positions:
            tag = "on" if on else "off"
            rec[f"{tag}_ms"] = round(statistics.median(ms[on]), 4)
            rec[f"{tag}_spread_ms"] = round(max(ms[on]) - min(ms[on]), 4)
        if can_reduce:
            rec["on_over_off"] = round(rec["on_ms"] / rec["off_ms"], 4)
            rec["on_fraction_of_8TBps"] = round(bytes_per_row * rows / (rec["on_ms"] * 1e-3) / 8e12, 4)
        legs.append(rec)
        print(json.dumps(rec), flush=True)

    n = int(a.rows)
    dev = hip.to_device(table(n, 7))
    four = [AggFunc(fn, InputRef(F), abi.INT64 if fn == "count" else abi.FLOAT64) for fn in ("count", "sum", "min", "max")]
    where = ((InputRef(I) >= Constant(100, abi.INT64)) & (InputRef(I) < Constant(140, abi.INT64))) & (InputRef(G) < Constant(0.5, abi.FLOAT64))
    leg("sum_f", [dev], n, [AggFunc("sum", InputRef(F), abi.FLOAT64)], None, 8)
    leg("four_cells_f", [dev], n, four, None, 8)
    leg("q6_shape", [dev], n, [AggFunc("sum", InputRef(F) * InputRef(G), abi.FLOAT64)], where, 16 + 8 * 0.02)
    dev.release()
    m = int(a.host_rows)
    whole = table(m, 8)
    host = [abi.HostBatch(whole.slice(lo, min(1024, m - lo))) for lo in range(0, m, 1024)]
    leg("host_1024", host, m, four, None, 8)
    hip.fn("timer_destroy")(timer)
    if a.out:
        with open(a.out, "w") as fh:
            for r in legs:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
