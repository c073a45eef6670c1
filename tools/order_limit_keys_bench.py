#!/usr/bin/env python
"""ORDER BY ... LIMIT k with SQLRS_ORDER_LIMIT_ALL_KEYS (the flag on the first key of sqlrs_order_create) off and on, on
the same DEVICE batch in one process (HIP events of the library's timer around each sqlrs_order_finish, retained push: no
input copy in either leg).  The off leg is the code
without the switch: a first key the plain hint does not serve runs the full sort.  k = 100 of --rows rows of
{key, int64 row id}; the keys: Utf8 random 0-12 letters; Utf8 "Customer#%09d"; Utf8 with 1 % NULLs DESC; Int64 with 1 % NULLs;
Float64 with 5 % NULLs DESC; the expression a + b over two int64 columns; a Utf8 key whose rows agree on their first 80 bytes
(the n / 2 guard fires: the on leg pays the sample sort and one mask pass on top of the full sort).  5 warm-ups and --reps
timed finishes per leg.  Prints one JSON line per shape: the median ms of either leg, the off leg's spread (max - min of its
timings), on_over_off, the candidates and the order_* route witnesses the on leg moved per finish.

    python tools/order_limit_keys_bench.py [--rows 1e7] [--k 100] [--reps 20] [--out FILE]"""
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
from sqlrs_amd.expr import InputRef, OrderBy  # noqa: E402

WARMUPS = 5


def utf8_array(lens, data, null=None):
    """a pyarrow Utf8 array from per-row lengths and the concatenated bytes (no Python loop over the rows)"""
    off = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=off[1:])
    validity = None if null is None else pa.py_buffer(np.packbits(~null, bitorder="little").tobytes())
    return pa.Array.from_buffers(pa.utf8(), len(lens), [validity, pa.py_buffer(off), pa.py_buffer(data)],
                                 null_count=0 if null is None else int(null.sum()))


def letters(rng, n, null=None):
    lens = rng.integers(0, 13, n)
    return utf8_array(lens, rng.integers(97, 123, int(lens.sum()), dtype=np.uint8), null)


def numbered(rng, n, prefix, digits, top):
    """prefix + a zero-padded random number below `top`, all rows of one length"""
    ids = rng.permutation(n).astype(np.int64) if top is None else rng.integers(0, top, n, dtype=np.int64)
    m = np.empty((n, len(prefix) + digits), dtype=np.uint8)
    m[:, :len(prefix)] = np.frombuffer(prefix, dtype=np.uint8)
    for d in range(digits):
        m[:, len(prefix) + digits - 1 - d] = 48 + (ids // 10 ** d) % 10
    return utf8_array(np.full(n, m.shape[1], dtype=np.int64), m.reshape(-1))


def read_counters(be):
    cap = 512
    names, ms, n_l = (C.c_char_p * cap)(), (C.c_double * cap)(), (C.c_int64 * cap)()
    n = be.fn("ctx_profile_read")(be.ctx, cap, names, ms, n_l)
    return {names[i].decode(): n_l[i] for i in range(min(n, cap))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, k = int(a.rows), a.k
    hip = sqlrs_amd.hip(0)
    rng = np.random.default_rng(7)
    row = pa.array(np.arange(n, dtype=np.int64))
    timer = C.c_void_p()
    hip.check(hip.fn("timer_create")(hip.ctx, C.byref(timer)))

    def finish_ms(dev, order_by, on):
        """one Order over the device batch: (ms of sqlrs_order_finish, candidates, output rows)"""
        arr, _keep = hip._order_by_array(order_by)
        arr[0].reserved = abi.ORDER_LIMIT_ALL_KEYS if on else 0
        h = C.c_void_p()
        hip.check(hip.fn("order_create")(hip.ctx, len(order_by), arr, C.byref(h)))
        try:
            hip.check(hip.fn("order_set_limit")(h, k))
            hip.check(hip.fn("order_push_retained")(h, abi.as_batch(dev).ptr))
            out = C.POINTER(abi.Batch)()
            hip.check(hip.fn("timer_start")(timer))
            hip.check(hip.fn("order_finish")(h, abi.MEM_DEVICE, C.byref(out)))
            hip.check(hip.fn("timer_stop")(timer))
            e = C.c_double()
            hip.check(hip.fn("timer_elapsed_ms")(timer, C.byref(e)))
            lb = hip.wrap(out)
            rows = lb.num_rows
            lb.release()
            return e.value, hip.fn("order_topk_candidates")(h), rows
        finally:
            hip.fn("order_destroy")(h)

    legs = []

    def shape(name, cols, order_by):
        dev = hip.to_device(pa.RecordBatch.from_arrays(cols, names=[f"c{i}" for i in range(len(cols))]))
        rec = {"shape": name, "rows": n, "k": k}
        try:
            for on in (False, True):
                for _ in range(WARMUPS):
                    finish_ms(dev, order_by, on)
                before = read_counters(hip)
                runs = [finish_ms(dev, order_by, on) for _ in range(a.reps)]
                after = read_counters(hip)
                ms = [r[0] for r in runs]
                tag = "on" if on else "off"
                rec[f"{tag}_ms"] = round(statistics.median(ms), 4)
                rec[f"{tag}_spread_ms"] = round(max(ms) - min(ms), 4)
                rec[f"{tag}_out_rows"] = runs[-1][2]
                if on:
                    rec["candidates"] = runs[-1][1]
                    rec["on_routes_per_finish"] = {
                        key[len("order_"):]: (after[key] - before.get(key, 0)) / a.reps
                        for key in sorted(after) if key.startswith("order_") and after[key] != before.get(key, 0)}
            rec["on_over_off"] = round(rec["on_ms"] / rec["off_ms"], 4)
            rec["off_minus_on_ms"] = round(rec["off_ms"] - rec["on_ms"], 4)
        finally:
            dev.release()
        legs.append(rec)
        print(json.dumps(rec), flush=True)

    key0 = [OrderBy(InputRef(0), asc=True)]
    key0_desc = [OrderBy(InputRef(0), asc=False)]
    shape("utf8_letters_0_12", [letters(rng, n), row], key0)
    shape("utf8_customer_numbers", [numbered(rng, n, b"Customer#", 9, None), row], key0)
    shape("utf8_letters_1pct_nulls_desc", [letters(rng, n, rng.random(n) < 0.01), row], key0_desc)
    shape("i64_1pct_nulls", [pa.array(rng.integers(-(1 << 62), 1 << 62, n, dtype=np.int64), mask=rng.random(n) < 0.01), row], key0)
    shape("f64_5pct_nulls_desc", [pa.array(rng.standard_normal(n), mask=rng.random(n) < 0.05), row], key0_desc)
    shape("expr_a_plus_b", [pa.array(rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64)),
                            pa.array(rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64)), row],
          [OrderBy(InputRef(0) + InputRef(1), asc=True)])
    shape("utf8_80_shared_bytes_guard", [numbered(rng, n, b"q" * 80, 7, 10_000_000), row], key0)
    hip.fn("timer_destroy")(timer)
    if a.out:
        with open(a.out, "w") as f:
            for r in legs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
