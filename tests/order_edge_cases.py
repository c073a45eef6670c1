"""Seeded cases of ORDER BY for tests/test_order_model_cpu.py (model against its row-by-row restatement and against the oracle,
the conditions every case is named for) and tests/test_gpu_order_edges.py (every device route, asserted by witness).  numpy and
pyarrow only; `run` at the bottom drives a backend (the oracle or the HIP library) over a case.

A case holds its input batches, its order-by list, the hooks it needs, an optional LIMIT / OFFSET and the route it is made for:

  general     the LSD path of sqlrs_order_finish: Utf8 / Boolean / expression keys, a double among several keys, few rows
  narrow      one plain key of <= 32 varying bits without NULLs, >= 2^20 rows (order_fast_impl)
  wide        ... of more than 32 varying bits: the splitter route (order_wide)
  in_order    rows that arrive in the requested order
  composite   <= 4 integer keys whose fields fit 64 bits, a valid bit per nullable key (order_composite)
  null_split  one key with NULLs the composite cannot take, >= 2^21 rows with >= 2^20 valid (order_null_split)
  topk        ORDER BY .. LIMIT with the hint of sqlrs_order_set_limit (order_topk), forced at 2^17 rows by SQLRS_ORDER_TOPK=1

Key pools are the values at which those routes go wrong: NaNs of both signs and several payloads (the ends of the total order:
0xFFFF..F has the image 0), +-inf, +-0.0 (neighbours in the image, equal as numbers), +-subnormal, +-DBL_MIN, +-DBL_MAX, 1.0
and its neighbours; the ends of int64 and int32; ranges of exactly 2^32 - 2 .. 2^32 + 1 (narrow | wide); ranges on a step of
the key-bit count; composite fields of 64 and 65 bits; garbage under NULL slots."""
import functools
import zlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import pyarrow as pa

from join_edge_cases import mix64
from sqlrs_amd import abi
from sqlrs_amd.expr import BinaryOp, InputRef, OrderBy, TypeCast

I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
POOL_I64 = [I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX]
POOL_I32 = [I32_MIN, I32_MAX]
NANS = [0x7FF8000000000000, 0xFFF8000000000001, 0x7FF8000000000123, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF]
ONE = 0x3FF0000000000000
POOL_F64 = NANS + [0x7FF0000000000000, 0xFFF0000000000000, 0x0, 0x8000000000000000, 0x1, 0x8000000000000001,
                   0x0010000000000000, 0x8010000000000000, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF, ONE - 1, ONE, ONE + 1]
NEG_ZERO, POS_INF, POS_NAN, NEG_NAN = 0x8000000000000000, 0x7FF0000000000000, 0x7FF8000000000000, 0xFFFFFFFFFFFFFFFF
PREFIX = "abcdefghijklmnopq"  # 17 characters: every length 0..17 on a common prefix
POOL_UTF8 = (["", "a", "a\x00", "a\x00\x00", "é", "漢", "\U0001f642", "z", "Z", "~", "\x7f"] + [PREFIX[:k] for k in range(18)] +
             [("x" * (L - 1)) + c for L in (8, 9, 16, 24) for c in ("a", "b")] +
             [("x" * (L - 2)) + c for L in (8, 9, 16, 24) for c in ("é", "ê")])  # (é / ê: C3 A9 / C3 AA — the last BYTE differs)

N20, NODD, N21 = 1 << 20, 1_300_000, 1 << 21
N21P = N21 + 4097          # just past 2^21, no multiple of 64
NSPLIT = 2_200_000
NTOPK = 1 << 17
GENERAL_SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537]  # (4096: one sort tile, sort.hip RS_TILE)
ROUTES = ("general", "narrow", "wide", "in_order", "composite", "null_split", "topk")


def seed_of(name: str) -> int:
    return zlib.crc32(name.encode())


# ---- columns ---------------------------------------------------------------------------------------------------------------------
def f64_of(bits) -> np.ndarray:
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


def with_validity(values: np.ndarray, valid: np.ndarray, pad_ones: bool = False) -> pa.Array:
    """an array over exactly these buffers: what sits under a NULL slot stays where it is; pad_ones: the bits behind the last
    row of the validity buffer (whole 8-byte words) are set — they are unspecified"""
    n = len(values)
    bits = np.zeros(((n + 63) // 64) * 64, dtype=bool)
    bits[:n] = valid
    if pad_ones:
        bits[n:] = True
    vbuf = pa.py_buffer(np.packbits(bits, bitorder="little").tobytes())
    t = {np.dtype(np.int64): pa.int64(), np.dtype(np.int32): pa.int32(), np.dtype(np.float64): pa.float64()}[values.dtype]
    return pa.Array.from_buffers(t, n, [vbuf, pa.py_buffer(np.ascontiguousarray(values).tobytes())], null_count=int(n - valid.sum()))


def plant(rng, col: np.ndarray, values, times: int = 1, avoid=()):
    """writes every value `times` times at random rows (not in `avoid`); returns the rows used"""
    n = len(col)
    rows = [r for r in rng.permutation(n)[: len(values) * times + len(avoid)].tolist() if r not in avoid][: len(values) * times]
    for i, r in enumerate(rows):
        col[r] = values[i % len(values)]
    return rows


def nan_payload_column(rng, n):
    bits = rng.integers(0, 1 << 62, n, dtype=np.uint64) | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))
    edge = rng.random(n) < 0.2
    bits[edge] = rng.choice(np.array(POOL_F64, dtype=np.uint64), int(edge.sum()))
    return pa.array(f64_of(bits), from_pandas=False)


def utf8_by_take(rng, n, nulls=0.1):
    pool = pa.array(POOL_UTF8 + [None], type=pa.string())
    idx = rng.integers(0, len(POOL_UTF8), n)
    if n and nulls:
        idx[rng.random(n) < nulls] = len(POOL_UTF8)
    return pool.take(pa.array(idx))


def mix_columns(rng, n, mix: str):
    """the columns beside the keys -> (arrays, names)"""
    row = pa.array(np.arange(n, dtype=np.int64))
    if mix == "key":
        return [], []
    if mix == "row":
        return [row], ["row"]
    if mix == "nanpay":             # the carried 8-byte column is a double with NaN payloads
        return [nan_payload_column(rng, n)], ["x"]
    if mix in ("more2", "more4", "more5"):   # carry + k plain 8-byte columns: the packed gather runs as 2, 4, 3 + 2
        k = int(mix[4:])
        cols = [row] + [pa.array(rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64)) if q % 2 else nan_payload_column(rng, n) for q in range(k)]
        return cols, ["row"] + [f"p{q}" for q in range(k)]
    if mix == "mixed":              # a nullable double, an int32, a Boolean and a Utf8 column gathered by the permutation
        f = f64_of(rng.choice(np.array(POOL_F64, dtype=np.uint64), n))
        cols = [row, with_validity(f, rng.random(n) >= 0.1), pa.array(rng.integers(I32_MIN, I32_MAX, n).astype(np.int32)),
                pa.array(rng.random(n) < 0.5, mask=rng.random(n) < 0.2), utf8_by_take(rng, n)]
        return cols, ["row", "f", "i", "b", "s"]
    raise ValueError(mix)


# ---- the case --------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    route: str
    batches: List[pa.RecordBatch]
    order_by: List[OrderBy]
    env: Dict[str, str] = field(default_factory=dict)
    limit: Optional[int] = None
    offset: int = 0
    props: dict = field(default_factory=dict)   # what the case is named for, checked by test_order_model_cpu.py

    @property
    def rows(self) -> int:
        return sum(b.num_rows for b in self.batches)

    def table(self) -> pa.Table:
        return pa.Table.from_batches(self.batches).combine_chunks()

    def reduced(self, n: int) -> "Case":
        """the first rows of the case (for the row-by-row restatement), as one batch"""
        t = self.table().slice(0, n)
        b = t.to_batches()[0] if t.num_rows else pa.RecordBatch.from_pylist([], schema=t.schema)
        return Case(self.name, self.route, [b], self.order_by, self.env, self.limit, self.offset, self.props)


_BUILDERS = {}


def _case(name, route):
    assert route in ROUTES and name not in _BUILDERS, name

    def deco(fn):
        _BUILDERS[name] = (route, fn)
        return fn
    return deco


def _make(name, route, keys, asc, mix="row", form="one", env=None, limit=None, offset=0, props=None, exprs=None, rng=None):
    """keys: arrays (numpy or pyarrow) most significant first; exprs: the order-by expressions when they are not the key columns"""
    rng = rng or np.random.default_rng(seed_of(name) + 1)
    arrays = [k if isinstance(k, pa.Array) else pa.array(k, from_pandas=False) for k in keys]
    n = len(arrays[0])
    extra, names = mix_columns(rng, n, mix)
    b = pa.RecordBatch.from_arrays(arrays + extra, names=[f"k{i}" for i in range(len(arrays))] + names)
    if form == "one":
        batches = [b]
    elif form == "three":           # several batches with an empty one among them
        batches = [b.slice(0, n // 3), b.slice(0, 0), b.slice(n // 3)]
    else:
        raise ValueError(form)
    ob = [OrderBy(e, asc=a) for e, a in zip(exprs or [InputRef(i) for i in range(len(asc))], asc)]
    return Case(name, route, batches, ob, dict(env or {}), limit, offset, dict(props or {}))


@functools.lru_cache(maxsize=48)   # (the 2^21-row cases hold ~100 MB each)
def case(name: str) -> Case:
    route, fn = _BUILDERS[name]
    c = fn(name, route, np.random.default_rng(seed_of(name)))
    assert c.name == name and c.route == route
    return c


def all_cases() -> List[str]:
    return list(_BUILDERS)


def cases_of(*routes) -> List[str]:
    return [n for n, (r, _) in _BUILDERS.items() if r in routes]


# ---- f64 keys on the fast routes -------------------------------------------------------------------------------------------------
def _f64_random_bits(rng, n):
    return rng.standard_normal(n).view(np.uint64).copy()


def _reg_f64():
    for asc in (True, False):
        d = "asc" if asc else "desc"

        @_case(f"f64_pool_{d}", "wide")
        def _(name, route, rng, asc=asc):
            bits = _f64_random_bits(rng, NODD)
            plant(rng, bits, POOL_F64, times=40)
            return _make(name, route, [f64_of(bits)], [asc], mix="nanpay" if asc else "mixed", form="three", props={"pool": "f64"})

        @_case(f"f64_cluster12_{d}", "wide")
        def _(name, route, rng, asc=asc):
            bits = _f64_random_bits(rng, N20 + 1)
            rows = rng.permutation(len(bits))[:6000]
            bits[rows] = np.uint64(ONE) + rng.integers(0, 1 << 12, 6000, dtype=np.uint64)   # differ only in the lowest 12 mantissa bits
            bits[rows[:3]] = [ONE - 1, ONE, ONE + 1]
            return _make(name, route, [f64_of(bits)], [asc], mix="row", props={"cluster12": 6000})

        @_case(f"f64_narrow_around_zero_{d}", "narrow")
        def _(name, route, rng, asc=asc):    # |bits| < 2^20 with both signs: +-0.0 and +-subnormals, neighbours in the image
            bits = rng.integers(0, 1 << 20, N20, dtype=np.uint64) | (rng.integers(0, 2, N20, dtype=np.uint64) << np.uint64(63))
            plant(rng, bits, [0x0, NEG_ZERO, 0x1, 0x8000000000000001], times=500)
            return _make(name, route, [f64_of(bits)], [asc], mix="nanpay", props={"pool": "f64_zero"})

        @_case(f"f64_narrow_at_one_{d}", "narrow")
        def _(name, route, rng, asc=asc):    # 1.0 and 2^24 of its upper neighbours, the lower one too
            bits = np.uint64(ONE) + rng.integers(0, 1 << 24, NODD, dtype=np.uint64)
            plant(rng, bits, [ONE - 1, ONE, ONE + 1], times=3)
            return _make(name, route, [f64_of(bits)], [asc], mix="more2", form="three")

    # 2^20 neighbouring bit patterns around an edge value: every value of the pool on the narrow route
    for label, lo in (("pos_nans", POS_NAN), ("top_end", 0x7FFFFFFFFFFFFFFF - (1 << 20) + 1), ("neg_top_end", 0xFFFFFFFFFFFFFFFF - (1 << 20) + 1),
                      ("neg_nans", 0xFFF8000000000001), ("pos_inf", POS_INF - (1 << 19)), ("neg_inf", 0xFFF0000000000000 - (1 << 19)),
                      ("dbl_min", 0x0010000000000000 - (1 << 19)), ("neg_dbl_min", 0x8010000000000000 - (1 << 19))):
        @_case(f"f64_narrow_near_{label}", "narrow")
        def _(name, route, rng, lo=lo, label=label):
            bits = np.uint64(lo) + rng.integers(0, 1 << 20, N20 + 1, dtype=np.uint64)
            plant(rng, bits, [v for v in POOL_F64 + [lo, lo + (1 << 20) - 1] if lo <= v < lo + (1 << 20)], times=3)
            return _make(name, route, [f64_of(bits)], [len(label) % 2 == 0], mix="row" if len(label) % 3 else "nanpay", props={"pool": "f64_part"})

    for label, value in (("neg_zero", NEG_ZERO), ("pos_nan", POS_NAN), ("pos_inf", POS_INF), ("neg_nan", NEG_NAN)):
        for asc in (True, False):
            @_case(f"f64_heavy_{label}_{'asc' if asc else 'desc'}", "wide")
            def _(name, route, rng, asc=asc, value=value):   # 30 % of the rows carry one edge value
                bits = _f64_random_bits(rng, NODD)
                plant(rng, bits, POOL_F64, times=5)
                bits[rng.random(NODD) < 0.3] = value
                return _make(name, route, [f64_of(bits)], [asc], mix="row" if asc else "more4", props={"heavy": value})


def _reg_i64():
    @_case("i64_pool_full_range", "wide")
    def _(name, route, rng):
        k = rng.integers(I64_MIN, I64_MAX, NODD, dtype=np.int64, endpoint=True)
        plant(rng, k, POOL_I64, times=20)
        return _make(name, route, [k], [True], mix="mixed", form="three", props={"pool": "i64"})

    @_case("i64_pool_full_range_desc", "wide")
    def _(name, route, rng):
        k = rng.integers(I64_MIN, I64_MAX, N20, dtype=np.int64, endpoint=True)
        plant(rng, k, POOL_I64, times=20)
        return _make(name, route, [k], [False], mix="key", props={"pool": "i64"})

    # the narrow | wide boundary: max - min of exactly 2^32 - 2 .. 2^32 + 1, from 0 and straddling 0
    for d, dn in ((2 ** 32 - 2, "2p32m2"), (2 ** 32 - 1, "2p32m1"), (2 ** 32, "2p32"), (2 ** 32 + 1, "2p32p1")):
        for lo, ln in ((0, "from0"), (-(2 ** 31) - 12345, "straddle")):
            @_case(f"i64_range_{dn}_{ln}", "narrow" if d <= 0xffffffff else "wide")
            def _(name, route, rng, d=d, lo=lo):
                n = N20 if lo == 0 else N20 + 1        # the smallest row counts the fast routes take
                k = lo + rng.integers(0, d, n, dtype=np.int64, endpoint=True)
                plant(rng, k, [lo, lo + d])
                return _make(name, route, [k], [lo == 0], mix="row", props={"range": d})

    # a range exactly on a step of the key-bit count
    for kb in (16, 24, 31):
        for d, dn in ((2 ** kb - 1, f"2p{kb}m1"), (2 ** kb, f"2p{kb}")):
            @_case(f"i64_kbits_{dn}", "narrow")
            def _(name, route, rng, d=d):
                lo = -777
                k = lo + rng.integers(0, d, NODD, dtype=np.int64, endpoint=True)
                plant(rng, k, [lo, lo + d])
                return _make(name, route, [k], [True], mix="row" if d % 2 else "nanpay", form="three", props={"range": d})

    @_case("i64_narrow_at_min", "narrow")
    def _(name, route, rng):        # the narrow route at the low end of int64: the image starts at 0
        k = I64_MIN + rng.integers(0, 1 << 28, N20, dtype=np.int64)
        plant(rng, k, [I64_MIN, I64_MIN + 1])
        return _make(name, route, [k], [False], mix="more5", props={"pool": "i64_min"})

    @_case("i64_narrow_at_max", "narrow")
    def _(name, route, rng):
        k = I64_MAX - rng.integers(0, 1 << 28, N20, dtype=np.int64)
        plant(rng, k, [I64_MAX, I64_MAX - 1])
        return _make(name, route, [k], [True], mix="mixed", props={"pool": "i64_max"})

    @_case("i64_narrow_around_zero", "narrow")
    def _(name, route, rng):
        k = rng.integers(-(1 << 27), 1 << 27, NODD, dtype=np.int64)
        plant(rng, k, [-1, 0, 1], times=3)
        return _make(name, route, [k], [True], mix="key", form="three", props={"pool": "i64_zero"})

    @_case("i64_wide_past_2p21", "wide")
    def _(name, route, rng):        # one count just past 2^21: G doubles, groups of ~1 K rows
        k = rng.integers(I64_MIN, I64_MAX, N21P, dtype=np.int64, endpoint=True)
        plant(rng, k, POOL_I64)
        return _make(name, route, [k], [True], mix="row", props={"pool": "i64"})

    @_case("i32_min_max_full", "narrow")
    def _(name, route, rng):        # INT32_MIN and INT32_MAX together: a range of 2^32 - 1 stays narrow
        k = rng.integers(I32_MIN, I32_MAX, NODD, dtype=np.int64, endpoint=True).astype(np.int32)
        plant(rng, k, POOL_I32, times=3)
        return _make(name, route, [k], [True], mix="row", form="three", props={"range": 2 ** 32 - 1, "pool": "i32"})

    @_case("i32_min_max_clustered_desc", "narrow")
    def _(name, route, rng):        # ... with a filler on 21 bits: two groups of equal top bits hold every row -> all bits through HBM
        k = rng.integers(-(1 << 20), 1 << 20, NODD).astype(np.int32)
        plant(rng, k, POOL_I32, times=3)
        return _make(name, route, [k], [False], mix="row", props={"range": 2 ** 32 - 1, "pool": "i32", "hbm_only": True})

    # the optimistic key range, forced with SQLRS_ORDER_SAMPLE=1; one outlier per end in a chunk the sample does not read
    for label, outliers in (("holds", ()), ("missed_low", (-5,)), ("missed_high", ((1 << 31) + 12345,)), ("missed_both", (-5, (1 << 31) + 12345))):
        @_case(f"i64_sampled_{label}", "narrow")
        def _(name, route, rng, outliers=outliers):
            k = rng.integers(1 << 20, 1 << 30, NODD, dtype=np.int64)
            rows = [2048 * 3 + 7, 2048 * 21 + 100]
            for r, v in zip(rows, outliers):
                k[r] = v
            return _make(name, route, [k], [True], mix="row", env={"SQLRS_ORDER_SAMPLE": "1"},
                         props={"sampled": True, "outlier_rows": rows[: len(outliers)], "missed": bool(outliers)})

    @_case("f64_sampled_pool", "wide")
    def _(name, route, rng):        # a sampled range of more than 32 bits: offsets from 0 over the whole 64-bit image
        bits = _f64_random_bits(rng, NODD)
        plant(rng, bits, POOL_F64, times=10)
        return _make(name, route, [f64_of(bits)], [True], mix="row", env={"SQLRS_ORDER_SAMPLE": "1"}, props={"sampled": True, "pool": "f64"})

    @_case("i64_sampled_33bit_ends_unsampled", "wide")
    def _(name, route, rng):        # the sample fits 32 bits, the keys do not: the exact retry, then the splitter route
        k = rng.integers(0, 1 << 31, NODD, dtype=np.int64)
        k[2048 * 3 + 1], k[2048 * 21 + 9] = -17, (1 << 32) + 4
        return _make(name, route, [k], [False], mix="row", env={"SQLRS_ORDER_SAMPLE": "1"},
                     props={"sampled": True, "outlier_rows": [2048 * 3 + 1, 2048 * 21 + 9], "missed": True})

    # rows already in order
    for label, asc in (("asc_ties", True), ("desc_f64_pool", False)):
        @_case(f"in_order_{label}", "in_order")
        def _(name, route, rng, asc=asc):
            if asc:
                k = np.sort(rng.integers(0, 1 << 20, N20, dtype=np.int64))
                return _make(name, route, [k], [True], mix="mixed", form="three")
            bits = _f64_random_bits(rng, N20 + 1)
            plant(rng, bits, POOL_F64, times=3)
            img = np.where(bits >> np.uint64(63) != 0, ~bits, bits | np.uint64(1 << 63))
            return _make(name, route, [f64_of(bits[np.argsort(img, kind="stable")[::-1]])], [False], mix="nanpay", props={"pool": "f64"})

    @_case("in_order_but_one_pair", "narrow")
    def _(name, route, rng):        # one inversion between two sampled pairs: the rows go through the sort
        k = np.sort(rng.integers(0, 1 << 20, N20, dtype=np.int64))
        k[700_003], k[700_004] = k[700_004] + 5, k[700_003]
        return _make(name, route, [k], [True], mix="row")

    # few distinct values over many bits: the heavy-value probe sends a narrow range to the splitter route
    @_case("i64_50_values_over_26_bits", "wide")
    def _(name, route, rng):
        k = rng.choice(rng.integers(0, 1 << 26, 50, dtype=np.int64), NODD)
        return _make(name, route, [k], [True], mix="more2", props={"heavy_to_wide": True})

    @_case("i64_50_values_over_26_bits_no_probe", "narrow")
    def _(name, route, rng):
        k = rng.choice(rng.integers(0, 1 << 26, 50, dtype=np.int64), NODD)
        return _make(name, route, [k], [False], mix="row", env={"SQLRS_ORDER_HEAVY_PROBE": "0"}, props={"hbm_only": True})

    @_case("i64_wide_declined_sample_blind", "general")
    def _(name, route, rng):
        """a mixed group beyond FIN_CAP: the rows the splitter route samples (a jittered grid, restated here to CONSTRUCT the
        column — never an expectation) hold values 2^40 apart, every other row a distinct value between the first two of them:
        one group holds nearly every row, the route declines and the general path sorts"""
        n = N20
        G, per_group = 512, 16                         # (order_wide: 2^9 groups of 16 samples at 2^20 rows)
        S = G * per_group
        stride = n // S
        k = rng.permutation(n).astype(np.int64) + 1              # distinct, all in (0, 2^40)
        for i in range(S):
            k[min(n - 1, i * stride + mix64(i) % stride)] = i << 40
        return _make(name, route, [k], [True], mix="row", props={"declined": True})


def _reg_composite():
    def nullable(values, null):
        return with_validity(values, ~null)

    @_case("comp_fields_64_bits", "composite")
    def _(name, route, rng):        # 32 + 32 bits: the composite fills the word
        a = rng.integers(0, 1 << 32, NODD, dtype=np.int64)
        b = rng.integers(I32_MIN, I32_MAX, NODD, dtype=np.int64, endpoint=True)
        a[0], a[1], b[2], b[3] = 0, (1 << 32) - 1, I32_MIN, I32_MAX
        a[5:5000] = a[5]
        return _make(name, route, [a, b], [True, False], mix="row", form="three", props={"field_bits": 64})

    @_case("comp_fields_65_bits", "general")
    def _(name, route, rng):        # 33 + 32 bits: one too many
        a = rng.integers(0, 1 << 33, N20, dtype=np.int64)
        b = rng.integers(I32_MIN, I32_MAX, N20, dtype=np.int64, endpoint=True)
        a[0], a[1], b[2], b[3] = 0, (1 << 33) - 1, I32_MIN, I32_MAX
        a[5:5000] = a[5]
        return _make(name, route, [a, b], [True, False], mix="row", props={"field_bits": 65})

    @_case("comp_nullable_63_value_bits_desc", "composite")
    def _(name, route, rng):        # 63 value bits + the valid bit = 64
        k = rng.integers(0, I64_MAX, NODD, dtype=np.int64, endpoint=True)
        k[7], k[8] = 0, I64_MAX
        null = rng.random(NODD) < 0.3
        null[7] = null[8] = False
        k[null] = 12345                                # (what sits under a NULL widens nothing here)
        return _make(name, route, [nullable(k, null)], [False], mix="row", props={"field_bits": 64, "nullable": True})

    @_case("comp_nullable_64_value_bits", "null_split")
    def _(name, route, rng):        # 64 value bits + the valid bit = 65: the NULL split takes it
        k = rng.integers(I64_MIN, I64_MAX, NSPLIT, dtype=np.int64, endpoint=True)
        rows = plant(rng, k, POOL_I64, times=3)
        null = rng.random(NSPLIT) < 0.15
        null[rows] = False
        return _make(name, route, [nullable(k, null)], [True], mix="row", form="three", props={"field_bits": 65, "pool": "i64"})

    @_case("comp_full_range_key_and_a_constant", "composite")
    def _(name, route, rng):        # 64 + 0 bits: both ends of int64 in one field
        k = rng.integers(I64_MIN, I64_MAX, N20, dtype=np.int64, endpoint=True)
        plant(rng, k, POOL_I64, times=5)
        return _make(name, route, [np.full(N20, 3, dtype=np.int32), k], [False, False], mix="row", props={"field_bits": 64, "pool": "i64"})

    @_case("comp_constant_key_among_others", "composite")
    def _(name, route, rng):        # a 0-bit field
        return _make(name, route, [rng.integers(0, 3, N20, dtype=np.int64), np.full(N20, -7, dtype=np.int64),
                                   rng.integers(0, 200, N20).astype(np.int32), rng.integers(0, 5, N20, dtype=np.int64)],
                     [True, True, False, True], mix="more2", props={"constant_key": 1})

    @_case("comp_i32_i64_mixed_directions", "composite")
    def _(name, route, rng):
        a = rng.integers(-50, 50, N20 + 1).astype(np.int32)
        b = rng.integers(1990, 2025, N20 + 1, dtype=np.int64)
        c = rng.integers(-(1 << 40), 1 << 40, N20 + 1, dtype=np.int64)
        return _make(name, route, [a, b, c], [False, True, False], mix="mixed")

    @_case("comp_i32_ends_desc_then_i64", "composite")
    def _(name, route, rng):
        a = rng.integers(I32_MIN, I32_MAX, N20, dtype=np.int64, endpoint=True).astype(np.int32)
        plant(rng, a, POOL_I32, times=3)
        return _make(name, route, [a, rng.integers(-1000, 1000, N20, dtype=np.int64)], [False, True], mix="row", props={"pool": "i32"})

    @_case("comp_two_nullable_keys_garbage_under_nulls", "composite")
    def _(name, route, rng):        # small ranges; under the NULL slots of the first key a value no row holds
        a = rng.integers(0, 50, NODD).astype(np.int32)
        b = rng.integers(-(1 << 33), 1 << 33, NODD, dtype=np.int64)
        na, nb = rng.random(NODD) < 0.1, rng.random(NODD) < 0.2
        a[na], b[nb] = 63, (1 << 33) - 1
        return _make(name, route, [nullable(a, na), nullable(b, nb)], [False, True], mix="nanpay", form="three", props={"nullable": True})

    @_case("comp_garbage_under_nulls_widens_the_range", "general")
    def _(name, route, rng):
        """INT64_MIN / INT64_MAX under the NULL slots of a 10-bit key: the measured range takes 64 bits, the composite declines
        (65 with the valid bit) — and the garbage must not show in the result"""
        a = rng.integers(0, 1000, N20, dtype=np.int64)
        na = rng.random(N20) < 0.1
        a[na] = rng.choice(np.array([I64_MIN, I64_MAX], dtype=np.int64), int(na.sum()))
        return _make(name, route, [nullable(a, na), rng.integers(0, 100, N20, dtype=np.int64)], [True, False], mix="row",
                     props={"garbage": True})


def _reg_null_split():
    @_case("nsplit_f64_nulls_and_nans", "null_split")
    def _(name, route, rng):        # NULLs and NaNs together, NaN and extreme patterns under the NULL slots
        bits = _f64_random_bits(rng, NSPLIT)
        plant(rng, bits, POOL_F64, times=50)
        null = rng.random(NSPLIT) < 0.15
        bits[null] = rng.choice(np.array(NANS + [0x7FEFFFFFFFFFFFFF, 0xFFF0000000000000], dtype=np.uint64), int(null.sum()))
        return _make(name, route, [with_validity(f64_of(bits), ~null)], [True], mix="mixed", form="three", props={"pool": "f64", "garbage": True})

    @_case("nsplit_f64_desc_validity_flips_every_64_rows", "null_split")
    def _(name, route, rng):        # NULLs still first under DESC; unspecified padding bits behind the last row
        n = N21P + 100_000
        bits = _f64_random_bits(rng, n)
        plant(rng, bits, POOL_F64, times=5)
        valid = (np.arange(n) // 64) % 2 == 0
        return _make(name, route, [with_validity(f64_of(bits), valid, pad_ones=True)], [False], mix="row", props={"padding": True, "pool": "f64"})

    @_case("nsplit_exactly_2p21_rows_2p20_valid", "null_split")
    def _(name, route, rng):
        k = rng.integers(0, 1 << 30, N21, dtype=np.int64)
        valid = np.zeros(N21, dtype=bool)
        valid[rng.permutation(N21)[:N20]] = True
        k[~valid] = I64_MIN                            # a single key with NULLs and a 64-bit measured range: not the composite's
        k[valid.argmax()] = I64_MAX
        return _make(name, route, [with_validity(k, valid)], [True], mix="row", props={"valid_rows": N20})

    @_case("nsplit_one_valid_row_short", "general")
    def _(name, route, rng):
        k = rng.integers(0, 1 << 30, N21, dtype=np.int64)
        valid = np.zeros(N21, dtype=bool)
        valid[rng.permutation(N21)[:N20 - 1]] = True
        k[~valid] = I64_MIN
        k[valid.argmax()] = I64_MAX
        return _make(name, route, [with_validity(k, valid)], [True], mix="row", props={"valid_rows": N20 - 1})


def _reg_topk():
    env = {"SQLRS_ORDER_TOPK": "1"}

    def topk(name, route, keys, asc, threshold, limit=1000, offset=37, mix="row", exprs=None, **props):
        return _make(name, route, keys, asc, mix=mix, form="three", env=env, limit=limit, offset=offset, exprs=exprs,
                     props=dict(props, threshold=threshold))

    @_case("topk_ties_at_the_threshold", "topk")
    def _(name, route, rng):        # 50 values: the threshold lands inside a run of ~2600 equal keys
        return topk(name, route, [rng.integers(0, 50, NTOPK, dtype=np.int64)], [True], threshold=("i64", 0))

    @_case("topk_desc_threshold_on_a_nan", "topk")
    def _(name, route, rng):        # DESC: more positive NaNs than k
        bits = _f64_random_bits(rng, NTOPK)
        bits[rng.permutation(NTOPK)[:6000]] = rng.choice(np.array([POS_NAN, 0x7FF8000000000123, 0x7FFFFFFFFFFFFFFF], dtype=np.uint64), 6000)
        return topk(name, route, [f64_of(bits)], [False], threshold=("f64", POS_NAN), mix="nanpay")

    @_case("topk_asc_threshold_on_a_negative_nan", "topk")
    def _(name, route, rng):
        bits = _f64_random_bits(rng, NTOPK)
        bits[rng.permutation(NTOPK)[:6000]] = rng.choice(np.array([NEG_NAN, 0xFFF8000000000001], dtype=np.uint64), 6000)
        return topk(name, route, [f64_of(bits)], [True], threshold=("f64", 0xFFF8000000000001))

    @_case("topk_desc_three_nans_above_the_threshold", "topk")
    def _(name, route, rng):        # the threshold is an ordinary double; three NaNs sort in front of everything
        bits = _f64_random_bits(rng, NTOPK)
        bits[[5, 70_000, NTOPK - 1]] = [POS_NAN, 0x7FFFFFFFFFFFFFFF, 0x7FF8000000000123]
        bits[[6, 7]] = [POS_INF, POS_INF]
        return topk(name, route, [f64_of(bits)], [False], threshold=("f64", f64_bits_of(0.5)))

    @_case("topk_asc_three_negative_nans_below_the_threshold", "topk")
    def _(name, route, rng):
        bits = _f64_random_bits(rng, NTOPK)
        bits[[5, 70_000, NTOPK - 1]] = [NEG_NAN, 0xFFF8000000000001, NEG_NAN]
        bits[[6, 7]] = [0xFFF0000000000000, 0xFFF0000000000000]
        return topk(name, route, [f64_of(bits)], [True], threshold=("f64", f64_bits_of(-0.5)))

    @_case("topk_threshold_on_negative_zero", "topk")
    def _(name, route, rng):        # 900 negatives, 3000 x -0.0, 3000 x +0.0, the rest positive
        bits = np.abs(rng.standard_normal(NTOPK)).view(np.uint64).copy() + np.uint64(1)
        rows = rng.permutation(NTOPK)
        bits[rows[:900]] |= np.uint64(1 << 63)
        bits[rows[900:3900]] = NEG_ZERO
        bits[rows[3900:6900]] = 0
        return topk(name, route, [f64_of(bits)], [True], threshold=("f64", NEG_ZERO))

    @_case("topk_threshold_on_int64_min", "topk")
    def _(name, route, rng):
        k = rng.integers(I64_MIN, I64_MAX, NTOPK, dtype=np.int64, endpoint=True)
        k[rng.permutation(NTOPK)[:6000]] = I64_MIN
        return topk(name, route, [k], [True], threshold=("i64", I64_MIN), mix="mixed")

    @_case("topk_desc_threshold_on_int64_max", "topk")
    def _(name, route, rng):
        k = rng.integers(I64_MIN, I64_MAX, NTOPK, dtype=np.int64, endpoint=True)
        k[rng.permutation(NTOPK)[:6000]] = I64_MAX
        return topk(name, route, [k], [False], threshold=("i64", I64_MAX), offset=0)

    @_case("topk_second_key_f64", "topk")
    def _(name, route, rng):
        bits = rng.choice(np.array(POOL_F64, dtype=np.uint64), NTOPK)
        return topk(name, route, [rng.integers(0, 2000, NTOPK, dtype=np.int64), f64_of(bits)], [True, False], threshold=("i64", 40))

    @_case("topk_second_key_utf8", "topk")
    def _(name, route, rng):
        return topk(name, route, [rng.integers(0, 2000, NTOPK).astype(np.int32), utf8_by_take(rng, NTOPK)], [False, True], threshold=("i32", 1960))

    @_case("topk_by_the_size_rule", "topk")
    def _(name, route, rng):        # no hook: >= 2^20 rows and a limit of at most a sixteenth of them
        k = rng.integers(I64_MIN, I64_MAX, N20, dtype=np.int64, endpoint=True)
        return _make(name, route, [k], [True], mix="row", limit=1000, offset=37, props={"threshold": ("i64", -(2 ** 63) + (2 ** 64 // 256))})

    @_case("topk_hint_ignored_sample_not_representative", "general")
    def _(name, route, rng):        # every sampled row is tiny, almost no other row is: fewer candidates than the limit
        k = rng.integers(1 << 20, 1 << 30, NTOPK, dtype=np.int64)
        k[::NTOPK // 65536] = -5
        return _make(name, route, [k], [True], mix="row", env=env, limit=100_000, offset=0, props={"ignored": True})

    @_case("topk_one_row_short_of_2p17", "general")
    def _(name, route, rng):        # below the forced size rule: the hint is not looked at
        return _make(name, route, [rng.integers(0, 50, NTOPK - 1, dtype=np.int64)], [True], mix="row", env=env, limit=1000, offset=37)


def f64_bits_of(x: float) -> int:
    return int(np.array([x], dtype=np.float64).view(np.uint64)[0])


# ---- the general path --------------------------------------------------------------------------------------------------------------
def _utf8_keys(rng, n, nulls=0.1):
    return utf8_by_take(rng, n, nulls)


def _reg_general():
    def forms():
        yield "utf8_asc", lambda rng, n: dict(keys=[_utf8_keys(rng, n), rng.integers(0, 3, n, dtype=np.int64)], asc=[True, True])
        yield "utf8_desc", lambda rng, n: dict(keys=[_utf8_keys(rng, n), rng.integers(0, 3, n, dtype=np.int64)], asc=[False, False])
        yield "int5_then_utf8", lambda rng, n: dict(keys=[rng.integers(0, 5, n, dtype=np.int64), _utf8_keys(rng, n)], asc=[True, False])
        yield "utf8_all_null", lambda rng, n: dict(keys=[pa.nulls(n, pa.string()), rng.integers(0, 3, n, dtype=np.int64)], asc=[True, False])
        yield "utf8_all_equal", lambda rng, n: dict(keys=[pa.array(["a\x00é"] * n, type=pa.string())], asc=[False])
        yield "bool_with_nulls_desc", lambda rng, n: dict(keys=[pa.array(rng.random(n) < 0.5, mask=(rng.random(n) < 0.3) if n else None)], asc=[False])
        yield "f64_pool_nullable_desc", lambda rng, n: dict(
            keys=[with_validity(f64_of(rng.choice(np.array(POOL_F64, dtype=np.uint64), n)), rng.random(n) >= 0.2, pad_ones=True)], asc=[False])
        yield "i64_pool_then_f64_pool", lambda rng, n: dict(
            keys=[rng.choice(np.array(POOL_I64, dtype=np.int64), n), f64_of(rng.choice(np.array(POOL_F64, dtype=np.uint64), n))], asc=[False, True])
        yield "i32_nullable_desc", lambda rng, n: dict(
            keys=[with_validity(rng.choice(np.array(POOL_I32 + [-1, 0, 1], dtype=np.int32), n), rng.random(n) >= 0.3)], asc=[False])
        yield "expr_add_wraps", lambda rng, n: dict(     # a + b over the ends of int64: the sum wraps
            keys=[rng.choice(np.array(POOL_I64, dtype=np.int64), n), rng.choice(np.array(POOL_I64, dtype=np.int64), n)], asc=[True],
            exprs=[BinaryOp("+", InputRef(0), InputRef(1))])
        yield "expr_cast_makes_nulls", lambda rng, n: dict(  # CAST(double AS INT32): NaN, inf and what does not fit become NULL
            keys=[f64_of(np.where(rng.random(n) < 0.5, rng.choice(np.array(POOL_F64, dtype=np.uint64), n),
                                  (rng.standard_normal(n) * 1000).view(np.uint64)))], asc=[False],
            exprs=[TypeCast(InputRef(0), abi.INT32)])

    big = {"utf8_asc": GENERAL_SIZES, "utf8_desc": GENERAL_SIZES[:12] + [70_001], "int5_then_utf8": GENERAL_SIZES[:12] + [65537],
           "f64_pool_nullable_desc": GENERAL_SIZES, "i64_pool_then_f64_pool": GENERAL_SIZES[:12] + [65535], "bool_with_nulls_desc": GENERAL_SIZES[:12] + [65536]}
    mixes = ["row", "mixed", "nanpay", "key", "more2"]
    for fname, make in forms():
        for q, n in enumerate(big.get(fname, GENERAL_SIZES[:12])):
            @_case(f"gen_{fname}_{n}", "general")
            def _(name, route, rng, make=make, n=n, q=q, fname=fname):
                spec = make(rng, n)
                return _make(name, route, spec["keys"], spec["asc"], mix=mixes[q % len(mixes)] if n else "row", form="three" if q % 3 == 1 else "one",
                             exprs=spec.get("exprs"), props={"pool": fname})

    @_case("gen_utf8_every_pool_string_once", "general")
    def _(name, route, rng):        # every string of the pool and a NULL, each once: no ties to hide behind
        vals = POOL_UTF8 + [None]
        order = rng.permutation(len(vals))
        return _make(name, route, [pa.array([vals[i] for i in order], type=pa.string())], [True], mix="row", props={"pool": "utf8"})

    @_case("gen_utf8_every_pool_string_once_desc", "general")
    def _(name, route, rng):
        vals = POOL_UTF8 + [None]
        order = rng.permutation(len(vals))
        return _make(name, route, [pa.array([vals[i] for i in order], type=pa.string())], [False], mix="row", props={"pool": "utf8"})

    @_case("gen_f64_pool_below_the_fast_size", "general")
    def _(name, route, rng):        # one row short of 2^20: the fast routes leave it alone
        bits = _f64_random_bits(rng, N20 - 1)
        plant(rng, bits, POOL_F64, times=20)
        return _make(name, route, [f64_of(bits)], [True], mix="nanpay", props={"pool": "f64"})

    @_case("gen_f64_then_i64_at_fast_size", "general")
    def _(name, route, rng):        # a double among several keys: not the composite's
        bits = rng.choice(np.array(POOL_F64, dtype=np.uint64), N20)
        return _make(name, route, [f64_of(bits), rng.integers(0, 1000, N20, dtype=np.int64)], [True, False], mix="row", props={"pool": "f64"})


_reg_f64()
_reg_i64()
_reg_composite()
_reg_null_split()
_reg_topk()
_reg_general()


# ---- driving a backend -------------------------------------------------------------------------------------------------------------
def run(be, c: Case, batches=None, hinted=True, retain=False) -> pa.Table:
    """ORDER BY [LIMIT] of the case on a backend -> the emitted rows as one table"""
    from sqlrs_amd.executor import LimitExecutor, OrderExecutor
    batches = c.batches if batches is None else batches
    ex = OrderExecutor(be, c.order_by, batches, retain_inputs=retain, limit_hint=(c.offset + c.limit) if (c.limit is not None and hinted) else None)
    out = ex.execute()
    if c.limit is not None:
        out = LimitExecutor(be, c.limit, c.offset, out).execute()
    got = [b for b in out if b is not None]
    t = pa.Table.from_batches(got) if got else c.table().slice(0, 0)
    return t.rename_columns(c.table().schema.names) if t.num_columns == c.table().num_columns else t
