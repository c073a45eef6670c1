#!/usr/bin/env python
"""The CSV scan's host parser against its device parser (sqlrs_csv_set_device_parse), file -> HBM, in one process.

Writes a seeded quote-free file (int64, %.6f float, boolean, short Utf8: sqlrs_amd/csvparse.generate, one block of
--block-rows records repeated to --mib MiB of text) under a temporary directory, reads it once so that it sits in the page
cache, then drains a reader with out_mem = DEVICE to the end — host parser and device parser alternating, batch_size 1024
and 2^22, --reps times each; the host clock runs from sqlrs_csv_open to a sqlrs_ctx_synchronize behind the last batch.
Prints per leg MB/s of file text and rows/s (median, min - max), the three counters of sqlrs_csv_device_stats and, from one
extra profiled device run per batch size, sqlrs_ctx_profile_read's per-kernel totals with the kernels' own rate over the
file's bytes (a KERNEL figure: file read and host-to-device copy are not in it).

    python tools/csv_device_bench.py [--mib 1024] [--reps 5] [--piece -1] [--legs host,device] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/csv_device_bench.py --legs device --reps 2"""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sqlrs_amd  # noqa: E402
from sqlrs_amd import abi, csvparse  # noqa: E402


def drain(be, path, batch_size, device_parse):
    """-> (seconds, rows, batches, stats)"""
    h = C.c_void_p()
    t0 = time.perf_counter()
    be.check(be.fn("csv_open")(be.ctx, path.encode(), 1, b",", batch_size, 10, C.byref(h)))
    rows = batches = 0
    try:
        if device_parse is not None:
            be.check(be.fn("csv_set_device_parse")(h, device_parse))
        nxt, rel = be.fn("csv_next_batch"), be.fn("batch_release")
        while True:
            out = C.POINTER(abi.Batch)()
            be.check(nxt(h, abi.MEM_DEVICE, C.byref(out)))
            if not out:
                break
            rows += out.contents.num_rows
            batches += 1
            rel(out)
        be.synchronize()
        dt = time.perf_counter() - t0
        d, hr, pf = C.c_int64(), C.c_int64(), C.c_int64()
        be.fn("csv_device_stats")(h, C.byref(d), C.byref(hr), C.byref(pf))
        return dt, rows, batches, (d.value, hr.value, pf.value)
    finally:
        be.fn("csv_close")(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--block-rows", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--piece", type=int, default=-1, help="argument of sqlrs_csv_set_device_parse (< 0: the library's piece size)")
    ap.add_argument("--legs", default="host,device", help="device: the device parser alone (a run under a tracer)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    hip = sqlrs_amd.hip(0)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench.csv")
        data, _ = csvparse.generate(a.block_rows, seed=1)
        header, body = data.split(b"\n", 1)
        reps = max(1, -(-a.mib * (1 << 20) // len(body)))
        with open(path, "wb") as f:
            f.write(header + b"\n")
            for _ in range(reps):
                f.write(body)
        size = os.path.getsize(path)
        with open(path, "rb") as f:  # into the page cache
            while f.read(1 << 24):
                pass
        say(f"# csv_device_bench: {size / 2**20:.1f} MiB of text, {reps * a.block_rows} records of (int64, %.6f float, boolean, "
            f"Utf8), {hip.version()}")
        say(f"# out_mem = DEVICE, piece = {a.piece}, {a.reps} repeats per leg, host and device alternating; host clock open -> synchronize")
        drain(hip, path, 1 << 22, a.piece)  # warm-up: pinned buffers, the pool's blocks, code objects
        summary = {}
        for bs in (1024, 1 << 22):
            times = {"host": [], "device": []}
            info = {}
            legs = [(leg, dp) for leg, dp in (("host", None), ("device", a.piece)) if leg in a.legs.split(",")]
            for _ in range(a.reps):
                for leg, dp in legs:
                    dt, rows, batches, st = drain(hip, path, bs, dp)
                    times[leg].append(dt)
                    info[leg] = (rows, batches, st)
            for leg, _ in legs:
                t = sorted(times[leg])
                rows, batches, st = info[leg]
                med = statistics.median(t)
                say(f"batch_size {bs:>8}  {leg:6}  {size / med / 1e6:9.1f} MB/s median ({size / t[-1] / 1e6:.1f} - {size / t[0] / 1e6:.1f})  "
                    f"{rows / med / 1e6:8.2f} Mrows/s  {med * 1e3:9.1f} ms median ({t[0] * 1e3:.1f} - {t[-1] * 1e3:.1f})  "
                    f"rows {rows} batches {batches}  device_rows {st[0]} host_rows {st[1]} patched_fields {st[2]}")
            if len(legs) < 2:
                continue
            summary[bs] = (statistics.median(times["device"]), min(times["host"]))
            say(f"batch_size {bs:>8}  device median {summary[bs][0] * 1e3:.1f} ms {'<' if summary[bs][0] < summary[bs][1] else '>='} "
                f"host minimum {summary[bs][1] * 1e3:.1f} ms  ({summary[bs][1] / summary[bs][0]:.1f}x)")
        for bs in (1024, 1 << 22):  # per-kernel totals of one device run (event pairs around every launch group: not a timed run)
            hip.profile(True)
            dt, rows, batches, st = drain(hip, path, bs, a.piece)
            prof = hip.profile_read()
            hip.profile(False)
            total = sum(ms for ms, _ in prof.values())
            say(f"# profiled device run, batch_size {bs}: {dt * 1e3:.1f} ms on the host clock, kernels {total:.1f} ms = "
                f"{size / (total / 1e3) / 1e9:.2f} GB/s of file text (kernel figure)")
            for name, (ms, n) in sorted(prof.items(), key=lambda kv: -kv[1][0]):
                say(f"    {name:16} {ms:10.3f} ms  {n:8d} launches")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
