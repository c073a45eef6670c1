#!/usr/bin/env python
"""The synchronous Filter / Project with SQLRS_EXPR_FUSED_EVAL (the flag on the expression handed to sqlrs_filter_create /
on exprs[0] of sqlrs_project_create) off and on, alternating in one process (HIP events of the library's timer around ONE
sqlrs_filter_push / sqlrs_project_push, DEVICE in, DEVICE out).  The off position is this build without the flag, or — with
--lib, an older build of the library, which does not know the flag and runs every expression node by node — that library on
a ctx of its own over its own copy of the table, in the same process.

--rows DEVICE rows of {i int64 uniform in [0, 1000), j int32 uniform in [1, 1000), f float64 standard normal, g float64 uniform
in [0.5, 1.5), gn = g with 10 % NULLs}, pushed as one batch.  Filter legs (all five columns are carried and compacted), each at
about 2 % and about 50 % kept:
    or_2 / or_50          f + g > c OR i < k
    range_gn_2 / _50      i >= a AND i < b AND gn < c        (gn nullable: off the conjunction route)
Project legs:
    f_g_f                 f * g + f
    cast_j_over_gn        cast(j as double) / gn
    four_columns          f * g + f, cast(j as double) / gn, i + cast(j as bigint), f < g

5 warm-ups, then --reps runs per leg and switch position.  Prints one JSON line per leg: median ms and max - min spread of
either position, on_over_off, the kept fraction, and for the on position the bytes of the leg's floor over the median as a
fraction of 8 TB/s.  The floor of a kernel: the referenced columns read once, the outputs written once (a mask or validity word
per 64 rows).  The floor of a Filter push: that plus the compaction as it is — the mask and every carried column read once, the
kept rows written.

    python tools/fused_eval_bench.py [--rows 1e8] [--reps 20] [--lib PATH] [--out FILE]"""
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
from sqlrs_amd.expr import Constant, InputRef, TypeCast  # noqa: E402

WARMUPS = 5
I, J, F, G, GN = range(5)
WIDTH = {I: 8, J: 4, F: 8, G: 8, GN: 8 + 1 / 8}  # bytes a row of the column costs to read (gn: its validity bit too)
ROW_BYTES = sum(WIDTH.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lib", default=None, help="an older build of libsqlrs_hip.so: the off position")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    on_be = sqlrs_amd.hip(0)
    off_be = abi.Backend(a.lib, "sqlrs_", 0) if a.lib else on_be
    n = int(a.rows)
    rng = np.random.default_rng(7)
    g = rng.random(n) + 0.5
    table = pa.RecordBatch.from_arrays(
        [pa.array(rng.integers(0, 1000, n, dtype=np.int64)), pa.array(rng.integers(1, 1000, n, dtype=np.int32)), pa.array(rng.standard_normal(n)),
         pa.array(g), pa.array(g, mask=rng.random(n) < 0.1)], names=["i", "j", "f", "g", "gn"])
    dev = {True: on_be.to_device(table)}
    dev[False] = off_be.to_device(table) if off_be is not on_be else dev[True]
    del table, g
    timers = {}
    for be in {id(on_be): on_be, id(off_be): off_be}.values():
        t = C.c_void_p()
        be.check(be.fn("timer_create")(be.ctx, C.byref(t)))
        timers[id(be)] = t

    def one_run(kind, exprs, on):
        """ms of one push, and the rows it returned"""
        be = on_be if on else off_be
        timer = timers[id(be)]
        flag = abi.EXPR_FUSED_EVAL if on else 0
        h, out = C.c_void_p(), C.POINTER(abi.Batch)()
        if kind == "filter":
            packed = exprs[0].pack()
            packed.abi.reserved = flag
            be.check(be.fn("filter_create")(be.ctx, C.byref(packed.abi), C.byref(h)))
        else:
            arr, keep = abi.pack_exprs(exprs)
            arr[0].reserved = flag
            be.check(be.fn("project_create")(be.ctx, len(exprs), arr, C.byref(h)))
        try:
            be.check(be.fn("timer_start")(timer))
            be.check(be.fn(kind + "_push")(h, dev[on].ptr, abi.MEM_DEVICE, C.byref(out)))
            be.check(be.fn("timer_stop")(timer))
            e = C.c_double()
            be.check(be.fn("timer_elapsed_ms")(timer, C.byref(e)))
            rows = out.contents.num_rows
            be.fn("batch_release")(out)
            return e.value, rows
        finally:
            be.fn(kind + "_destroy")(h)

    def witness():
        return {k: v[1] for k, v in on_be.profile_read().items() if k.startswith("fused_eval_") and k.endswith(("batches", "columns"))}

    legs = []

    def leg(name, kind, exprs, read_cols, out_bytes):
        """`read_cols`: the columns the expressions reference; `out_bytes`: bytes per row the kernel writes (Project: the computed
        columns and their validity; Filter: the mask)"""
        rec = {"leg": name, "rows": n, "off": "lib" if a.lib else "flag off"}
        for on in (False, True):
            for _ in range(WARMUPS):
                one_run(kind, exprs, on)
        before = witness()
        ms, rows = {False: [], True: []}, {}
        for _ in range(a.reps):  # off, on, off, on, ...
            for on in (False, True):
                t, rows[on] = one_run(kind, exprs, on)
                ms[on].append(t)
        after = witness()
        rec["fused_witness"] = {k: after.get(k, 0) - before.get(k, 0) for k in after}
        assert rows[True] == rows[False], (name, rows)
        for on in (False, True):
            tag = "on" if on else "off"
            rec[f"{tag}_ms"] = round(statistics.median(ms[on]), 4)
            rec[f"{tag}_spread_ms"] = round(max(ms[on]) - min(ms[on]), 4)
        rec["on_over_off"] = round(rec["on_ms"] / rec["off_ms"], 4)
        floor = sum(WIDTH[c] for c in read_cols) + out_bytes
        if kind == "filter":
            kept = rows[True] / n
            rec["kept"] = round(kept, 4)
            floor += 1 / 8 + ROW_BYTES + kept * ROW_BYTES  # compaction: the mask and every column read, the kept rows written
        rec["floor_bytes_per_row"] = round(floor, 3)
        rec["on_fraction_of_8TBps"] = round(floor * n / (rec["on_ms"] * 1e-3) / 8e12, 4)
        legs.append(rec)
        print(json.dumps(rec), flush=True)

    def either(c, k):
        return ((InputRef(F) + InputRef(G)) > Constant(c, abi.FLOAT64)) | (InputRef(I) < Constant(k, abi.INT64))

    def ranged(lo, hi, c):
        return ((InputRef(I) >= Constant(lo, abi.INT64)) & (InputRef(I) < Constant(hi, abi.INT64))) & (InputRef(GN) < Constant(c, abi.FLOAT64))
    leg("or_2", "filter", [either(3.4, 10)], [F, G, I], 1 / 8)
    leg("or_50", "filter", [either(1.5, 260)], [F, G, I], 1 / 8)
    leg("range_gn_2", "filter", [ranged(100, 140, 1.0)], [I, GN], 1 / 8)
    leg("range_gn_50", "filter", [ranged(0, 1000, 1.06)], [I, GN], 1 / 8)
    fgf = InputRef(F) * InputRef(G) + InputRef(F)
    quot = TypeCast(InputRef(J), abi.FLOAT64) / InputRef(GN)
    leg("f_g_f", "project", [fgf], [F, G], 8 + 1 / 8)
    leg("cast_j_over_gn", "project", [quot], [J, GN], 8 + 1 / 8)
    leg("four_columns", "project", [fgf, quot, InputRef(I) + TypeCast(InputRef(J), abi.INT64), InputRef(F) < InputRef(G)], [F, G, J, GN, I],
        3 * (8 + 1 / 8) + 2 / 8)
    for be in {id(on_be): on_be, id(off_be): off_be}.values():
        be.fn("timer_destroy")(timers[id(be)])
    if a.out:
        with open(a.out, "w") as fh:
            for r in legs:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
