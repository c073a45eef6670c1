"""The candidate rule of SQLRS_ORDER_LIMIT_ALL_KEYS (order_topk.hip) restated in numpy, without a GPU: the sampled rows,
the NULLs-first sample sort, the quantile, the 64-byte zero-padded image compare and both guards.  For every shape of
order_limit_keys_cases.py the candidates' stable sort must reproduce the first `hint` rows of the full stable sort, and the
shape must land where test_gpu_order_limit_keys.py expects it (0 < kept < n / 4, or an ignored route) — which keeps that
test's conditions honest.  Rows at or below the threshold in this model at n = 2^17 + 67, hint 1037, default_rng(7) (printed by
`pytest -s`): letters asc 10 004 (the empty strings), desc 2 191; 1 % NULLs DESC 2 240; 5 % NULLs 6 503 (the threshold row is
NULL: exactly the NULL rows); customers 2 180; with outliers asc 2 182, desc 2 162; fifty values 2 600; 60 shared bytes 2 163;
"ab" + NUL bytes and 80 shared bytes: all 131 139 rows tie (n / 2 guard); sampled rows empty, hint 100 000: 70 564, below the
hint; Int64 1 % NULLs 2 154; Float64 5 % NULLs DESC 6 454; Int32 DESC with one NULL 2 170."""
import math
import os
import re

import numpy as np
import pytest

import order_limit_keys_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rule ------------------------------------------------------------------------------------------------------------------
def fixed_image(values: np.ndarray) -> np.ndarray:
    """i64_to_ordered / f64_to_ordered (device_utils.hpp), int32 widened: [n, 1] uint64 words"""
    if values.dtype == np.float64:
        b = values.view(np.uint64)
        u = np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))
    else:
        u = values.astype(np.int64).view(np.uint64) ^ np.uint64(1 << 63)
    return u.reshape(-1, 1)


def utf8_image(values) -> np.ndarray:
    """the first 64 bytes as eight big-endian 64-bit words, zero padded: [n, 8] uint64"""
    m = np.zeros((len(values), 64), dtype=np.uint8)
    for i, s in enumerate(values):
        s = s[:64]
        m[i, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    return m.view(">u8").astype(np.uint64)


def full_order(values, null, asc, kind) -> np.ndarray:
    """row ids in the ORDER BY's own order of the first key: NULLs first in either direction, stable"""
    n = len(values)
    null = np.zeros(n, dtype=bool) if null is None else null
    if kind == "utf8":
        rows = sorted(range(n), key=lambda i: b"" if null[i] else values[i], reverse=not asc)  # (reverse keeps ties in input order)
        rows = np.array(rows, dtype=np.int64)
    else:
        u = fixed_image(values)[:, 0]
        u = np.where(null, np.uint64(0), u if asc else ~u)
        rows = np.argsort(u, kind="stable")
    return rows[np.argsort(~null[rows], kind="stable")]


def candidates(values, null, asc, kind, hint):
    """(row ids kept in input order or None when a guard ignores the hint, number of rows at or below the threshold)"""
    n = len(values)
    null = np.zeros(n, dtype=bool) if null is None else null
    S = K.SAMPLES
    rows = np.minimum(np.arange(S, dtype=np.int64) * (n // S), n - 1)
    if kind == "utf8":
        sv = [values[i] for i in rows.tolist()]
    else:
        sv = values[rows]
    order = full_order(sv, null[rows], asc, kind)                 # the sample sorted as the operator sorts: the strings themselves
    q = min(S - 1, math.ceil(hint * S / n * 2.0) + 64)
    t = int(rows[order[q]])
    img = utf8_image(values) if kind == "utf8" else fixed_image(values)
    if null[t]:
        keep = null.copy()                                          # the threshold row is NULL: exactly the NULL rows
    else:
        x, tw = (img, img[t]) if asc else (~img, ~img[t])
        below = np.zeros(n, dtype=bool)
        open_ = np.ones(n, dtype=bool)                              # equal to the threshold on every word so far
        for w in range(img.shape[1]):
            below |= open_ & (x[:, w] < tw[w])
            open_ &= x[:, w] == tw[w]
        keep = null | below | open_                                 # a tie on all words is kept
    kept = int(keep.sum())
    if kept < hint or kept > n // 2:
        return None, kept
    return np.flatnonzero(keep), kept


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.name)
def test_candidates_hold_the_first_rows(case):
    values, null = K.make(case)
    n = len(values)
    assert n == K.N
    cand, kept = candidates(values, null, case.asc, case.kind, case.hint)
    print(f"{case.name}: {kept} at or below the threshold, {'ignored' if cand is None else 'kept'}")
    if case.expect == "ignored_many":
        assert cand is None and kept > n // 2
        return
    if case.expect == "ignored_few":
        assert cand is None and kept < case.hint
        return
    assert cand is not None and 0 < kept < n // 4, kept
    full = full_order(values, null, case.asc, case.kind)
    sub_null = None if null is None else null[cand]
    sub_vals = [values[i] for i in cand.tolist()] if case.kind == "utf8" else values[cand]
    sub = cand[full_order(sub_vals, sub_null, case.asc, case.kind)]
    assert np.array_equal(sub[:case.hint], full[:case.hint])


def test_image_order_is_weaker_than_the_string_order():
    """truncation and zero padding are monotone: a <= b implies image(a) <= image(b)"""
    v = sorted([b"", b"a", b"a\x00", b"ab", b"b" * 64, b"b" * 64 + b"a", b"b" * 64 + b"z", b"b" * 65, b"c"])
    img = [tuple(r) for r in utf8_image(v).tolist()]
    assert img == sorted(img)
    assert img[1] == img[2] and img[4] == img[5] == img[6] == img[7]


# ---- ABI plumbing --------------------------------------------------------------------------------------------------------------
def test_abi_carries_the_flag_as_the_header_defines_it():
    """the switch is SQLRS_ORDER_LIMIT_ALL_KEYS in `reserved` of the first sqlrs_order_by_t: the same value in the header, in
    abi.py and in the generated Rust constants; no entry point was added for it"""
    from sqlrs_amd import abi
    header = open(os.path.join(ROOT, "include", "sqlrs_hip.h")).read()
    h = re.search(r"^#define\s+SQLRS_ORDER_LIMIT_ALL_KEYS\s+(\d+)\s*$", header, flags=re.M)
    assert h, "sqlrs_hip.h does not define SQLRS_ORDER_LIMIT_ALL_KEYS"
    assert int(h.group(1)) == abi.ORDER_LIMIT_ALL_KEYS == 1
    assert ("reserved", __import__("ctypes").c_int32) in abi.OrderBy._fields_
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert re.search(r"pub const SQLRS_ORDER_LIMIT_ALL_KEYS: i32 = 1;", ffi)
    assert "sqlrs_order_set_limit_all_keys" not in header and "sqlrs_order_set_limit_all_keys" not in ffi


def test_executor_takes_the_switch_and_defaults_to_off():
    import inspect

    from sqlrs_amd.executor import OrderExecutor
    p = inspect.signature(OrderExecutor.__init__).parameters
    assert p["limit_all_keys"].default is False
