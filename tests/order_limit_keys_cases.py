"""The first-key shapes of ORDER BY ... LIMIT with SQLRS_ORDER_LIMIT_ALL_KEYS, shared by the numpy model of the candidate
rule (test_order_limit_keys_cpu.py) and the GPU test (test_gpu_order_limit_keys.py).  A case's key is a list of `bytes` (Utf8)
or a numpy array (fixed width) plus a boolean `null` mask; `expect` says where the case must land: "topk" (0 < kept < n / 4),
or an ignored route — "ignored_many" (more than n / 2 candidates) / "ignored_few" (fewer than the hint).  Every case is drawn
from default_rng(7), so both tests see the same rows."""
from collections import namedtuple

import numpy as np

N = (1 << 17) + 67      # not a multiple of 64; the sample step n // 65536 is 2
HINT = 1037             # k = 1000, offset = 37
SAMPLES = 65536

Case = namedtuple("Case", "name kind asc hint expect make")   # make(rng, n) -> (values, null mask or None)

_LETTERS = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)


def _random_letters(rng, n, lo=0, hi=12):
    lens = rng.integers(lo, hi + 1, n)
    flat = _LETTERS[rng.integers(0, 26, int(lens.sum()))].tobytes()
    ends = np.cumsum(lens)
    return [flat[e - l:e] for e, l in zip(ends.tolist(), lens.tolist())]


def _letters(rng, n):
    return _random_letters(rng, n), None


def _letters_nulls(frac):
    def make(rng, n):
        return _random_letters(rng, n), rng.random(n) < frac
    return make


def _customers(rng, n):
    return [b"Customer#%09d" % i for i in rng.permutation(n).tolist()], None


def _customers_outliers(rng, n):
    v = [b"Customer#%09d" % i for i in rng.permutation(n).tolist()]
    for i in range(500, n, 1000):                 # (odd spacing against the sample step: about half of them are sampled)
        j = i + int(rng.integers(0, 7))
        v[j] = (b"Apple" if (i // 1000) % 2 else b"Zebra") + b"%05d" % i
    return v, None


def _fifty_values(rng, n):
    names = [b"name-%02d-" % i + bytes(rng.integers(97, 123, int(rng.integers(0, 9))).astype(np.uint8)) for i in range(50)]
    return [names[i] for i in rng.integers(0, 50, n).tolist()], None


def _shared_60(rng, n):
    prefix = b"p" * 60                            # the images differ in their last word only; the 6th digit lies beyond it
    return [prefix + b"%06d" % i for i in rng.integers(0, 1_000_000, n).tolist()], None


def _ab_nul(rng, n):
    return [b"ab" + b"\x00" * k for k in rng.integers(0, 4, n).tolist()], None   # zero padding: every image is equal


def _shared_80(rng, n):
    prefix = b"q" * 80
    return [prefix + b"%07d" % i for i in rng.integers(0, 10_000_000, n).tolist()], None


def _sampled_rows_empty(rng, n):
    v = _random_letters(rng, n)
    for i in range(0, n, n // SAMPLES):
        v[i] = b""
    v[n - 1] = b""
    return v, None


def _i64_nulls(rng, n):
    return rng.integers(-(1 << 62), 1 << 62, n, dtype=np.int64), rng.random(n) < 0.01


def _f64_nulls(rng, n):
    v = rng.standard_normal(n)
    v[rng.integers(0, n, 64)] = np.nan
    v[rng.integers(0, n, 64)] = np.inf
    v[rng.integers(0, n, 64)] = -np.inf
    v[rng.integers(0, n, 64)] = 0.0
    v[rng.integers(0, n, 64)] = -0.0
    return v, rng.random(n) < 0.05


def _i32_one_null(rng, n):
    null = np.zeros(n, dtype=bool)
    null[n // 2 + 1] = True
    return rng.integers(-(1 << 30), 1 << 30, n).astype(np.int32), null


UTF8_CASES = [
    Case("letters_asc", "utf8", True, HINT, "topk", _letters),
    Case("letters_desc", "utf8", False, HINT, "topk", _letters),
    Case("letters_1pct_nulls_desc", "utf8", False, HINT, "topk", _letters_nulls(0.01)),
    Case("letters_5pct_nulls", "utf8", True, HINT, "topk", _letters_nulls(0.05)),       # the threshold row is NULL
    Case("customers", "utf8", True, HINT, "topk", _customers),
    Case("customers_outliers_asc", "utf8", True, HINT, "topk", _customers_outliers),
    Case("customers_outliers_desc", "utf8", False, HINT, "topk", _customers_outliers),
    Case("fifty_values", "utf8", True, HINT, "topk", _fifty_values),
    Case("shared_60_bytes", "utf8", True, HINT, "topk", _shared_60),
    Case("ab_plus_nul_bytes", "utf8", True, HINT, "ignored_many", _ab_nul),
    Case("shared_80_bytes", "utf8", True, HINT, "ignored_many", _shared_80),
    Case("sampled_rows_empty", "utf8", True, 100_000, "ignored_few", _sampled_rows_empty),
]
FIXED_CASES = [
    Case("i64_1pct_nulls", "i64", True, HINT, "topk", _i64_nulls),
    Case("f64_5pct_nulls_desc", "f64", False, HINT, "topk", _f64_nulls),                # the NULLs cover the limit
    Case("i32_one_null_desc", "i32", False, HINT, "topk", _i32_one_null),
]
CASES = UTF8_CASES + FIXED_CASES
BY_NAME = {c.name: c for c in CASES}


def make(case, n=N):
    """(values, null mask or None) of the case"""
    return case.make(np.random.default_rng(7), n)


def arrow_key(case, n=N):
    import pyarrow as pa
    values, null = make(case, n)
    if case.kind == "utf8":
        return pa.array([None if (null is not None and null[i]) else values[i] for i in range(n)], type=pa.binary()).cast(pa.utf8())
    return pa.array(values, mask=null)
