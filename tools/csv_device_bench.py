#!/usr/bin/env python
"""The CSV scan's host parser against its device parser (sqlrs_csv_set_device_parse), file -> HBM, in one process.

Writes a seeded quote-free file (int64, %.6f float, boolean, short Utf8: sqlrs_amd/csvparse.generate, one block of
--block-rows records repeated to --mib MiB of text) under a temporary directory, reads it once so that it sits in the page
cache, then drains a reader with out_mem = DEVICE to the end — host parser and device parser alternating, batch_size 1024
and 2^22, --reps times each; the host clock runs from sqlrs_csv_open to a sqlrs_ctx_synchronize behind the last batch.
Prints per leg MB/s of file text and rows/s (median, min - max), the three counters of sqlrs_csv_device_stats and, from one
extra profiled device run per batch size, sqlrs_ctx_profile_read's per-kernel totals with the kernels' own rate over the
file's bytes (a KERNEL figure: file read and host-to-device copy are not in it).

--quoted (sqlrs_csv_set_device_quotes): the block is csvparse.generate_quoted's — about half of the Utf8 fields and a tenth
of the typed ones quoted — and a third leg, device_q, reads with the switch on (the device leg, switch off, hands every piece
back: host_rows = all rows); then the quote-free file is read by device and device_q, for what the parity pass and the
masked kernels cost where there is nothing to mask.

    python tools/csv_device_bench.py [--mib 1024] [--reps 5] [--piece -1] [--legs host,device] [--quoted] [--out FILE]
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


def drain(be, path, batch_size, device_parse, device_quotes=None):
    """-> (seconds, rows, batches, stats)"""
    h = C.c_void_p()
    t0 = time.perf_counter()
    be.check(be.fn("csv_open")(be.ctx, path.encode(), 1, b",", batch_size, 10, C.byref(h)))
    rows = batches = 0
    try:
        if device_parse is not None:
            be.check(be.fn("csv_set_device_parse")(h, device_parse))
        if device_quotes is not None:
            be.check(be.fn("csv_set_device_quotes")(h, device_quotes))
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


def write_file(path, block, mib):
    """header + the block's records repeated to `mib` MiB, read once into the page cache -> (bytes, repeats)"""
    header, body = block.split(b"\n", 1)
    reps = max(1, -(-mib * (1 << 20) // len(body)))
    with open(path, "wb") as f:
        f.write(header + b"\n")
        for _ in range(reps):
            f.write(body)
    with open(path, "rb") as f:
        while f.read(1 << 24):
            pass
    return os.path.getsize(path), reps


def bench_file(hip, say, path, size, legs, piece, reps):
    """the legs alternating, `reps` times per batch size; then one profiled run per device leg"""
    args = {"host": (None, None), "device": (piece, None), "device_q": (piece, 1)}
    for leg in legs:
        if leg != "host":
            drain(hip, path, 1 << 22, *args[leg])  # warm-up: pinned buffers, the pool's blocks, code objects
    for bs in (1024, 1 << 22):
        times = {leg: [] for leg in legs}
        info = {}
        for _ in range(reps):
            for leg in legs:
                dt, rows, batches, st = drain(hip, path, bs, *args[leg])
                times[leg].append(dt)
                info[leg] = (rows, batches, st)
        for leg in legs:
            t = sorted(times[leg])
            rows, batches, st = info[leg]
            med = statistics.median(t)
            say(f"batch_size {bs:>8}  {leg:8}  {size / med / 1e6:9.1f} MB/s median ({size / t[-1] / 1e6:.1f} - {size / t[0] / 1e6:.1f})  "
                f"{rows / med / 1e6:8.2f} Mrows/s  {med * 1e3:9.1f} ms median ({t[0] * 1e3:.1f} - {t[-1] * 1e3:.1f})  "
                f"rows {rows} batches {batches}  device_rows {st[0]} host_rows {st[1]} patched_fields {st[2]}")
        if "host" in legs:
            for leg in legs[1:]:
                med, hmin = statistics.median(times[leg]), min(times["host"])
                say(f"batch_size {bs:>8}  {leg} median {med * 1e3:.1f} ms {'<' if med < hmin else '>='} "
                    f"host minimum {hmin * 1e3:.1f} ms  ({hmin / med:.1f}x)")
        elif len(legs) == 2:
            a, b = (statistics.median(times[leg]) for leg in legs)
            say(f"batch_size {bs:>8}  {legs[1]} median / {legs[0]} median = {b / a:.3f}")
    for leg in legs:  # per-kernel totals of one run (event pairs around every launch group: not a timed run)
        if leg == "host":
            continue
        for bs in (1024, 1 << 22):
            hip.profile(True)
            dt, rows, batches, st = drain(hip, path, bs, *args[leg])
            prof = hip.profile_read()
            hip.profile(False)
            total = sum(ms for ms, _ in prof.values())
            if total <= 0:
                continue
            say(f"# profiled {leg} run, batch_size {bs}: {dt * 1e3:.1f} ms on the host clock, kernels {total:.1f} ms = "
                f"{size / (total / 1e3) / 1e9:.2f} GB/s of file text (kernel figure)")
            for name, (ms, n) in sorted(prof.items(), key=lambda kv: -kv[1][0]):
                say(f"    {name:16} {ms:10.3f} ms  {n:8d} launches")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--block-rows", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--piece", type=int, default=-1, help="argument of sqlrs_csv_set_device_parse (< 0: the library's piece size)")
    ap.add_argument("--legs", default=None, help="of host,device,device_q (default host,device; --quoted: all three); "
                    "device alone: the device parser under a tracer")
    ap.add_argument("--quoted", action="store_true", help="the quoted file, then the quote-free file with the switch off and on")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    hip = sqlrs_amd.hip(0)
    want = (a.legs or ("host,device,device_q" if a.quoted else "host,device")).split(",")
    legs = [leg for leg in ("host", "device", "device_q") if leg in want]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench.csv")
        block, _ = (csvparse.generate_quoted if a.quoted else csvparse.generate)(a.block_rows, seed=1)
        size, reps = write_file(path, block, a.mib)
        say(f"# csv_device_bench: {size / 2**20:.1f} MiB of text, {reps * a.block_rows} records of (int64, %.6f float, boolean, "
            f"Utf8){', quoted fields (csvparse.generate_quoted)' if a.quoted else ''}, {hip.version()}")
        say(f"# out_mem = DEVICE, piece = {a.piece}, {a.reps} repeats per leg, the legs alternating ({', '.join(legs)}; device_q = "
            f"sqlrs_csv_set_device_quotes on); host clock open -> synchronize")
        bench_file(hip, say, path, size, legs, a.piece, a.reps)
        if a.quoted:
            block, _ = csvparse.generate(a.block_rows, seed=1)
            size, reps = write_file(path, block, a.mib)
            say()
            say(f"# the quote-free file: {size / 2**20:.1f} MiB of text, {reps * a.block_rows} records; the switch off (device) and on (device_q)")
            bench_file(hip, say, path, size, ["device", "device_q"], a.piece, a.reps)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
