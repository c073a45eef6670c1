"""Seeded cases of the hash join on one fixed-width key, for tests/test_join_model_cpu.py (model against oracle, conditions,
planted faults) and tests/test_gpu_join_edges.py (every device route).  The cases are numpy and pyarrow only; `run` at the
bottom drives a backend (the oracle or the HIP library) over one of them.

A case holds its build batches, its probe batches and the route family (`route`) it is made for:

  dense        unique keys over a range the direct-address table takes (<= 4 x rows + 1024)
  dd           duplicate keys over such a range, no NULL key: runs by key (dd_table)
  slots        unique keys the direct-address table refuses: the 16-byte-slot table (or, forced, LDS tables of the keys)
  slots_dup    duplicate keys (or several NULL keys) there: the slot table with CSR runs (or LDS tables of the distinct keys)

Key pools are the values at which those tables go wrong: the ends of int64 (whose range `hi - lo + 1` wraps to 0), -1 (the
slot table's "empty" word, as a double the NaN 0xFFFF..F), the neighbours of 2^31 and 2^32 (32-bit offsets and packed entries),
doubles that differ only in sign or payload.  Probe keys hold `min - 1`, `max + 1` and `min + 2^63` of the build side, so that
`key - min` wraps; NULL probe keys sit on slots whose VALUE is a build key.  Hits are drawn from four fifths of the build rows,
so that Left / Full joins have a tail."""
import functools

import numpy as np
import pyarrow as pa

import expr_model as X

I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
POOL_I64 = [I64_MIN, I64_MAX, -1, 0, 1, -2, 2 ** 31 - 1, 2 ** 31, -(2 ** 31) - 1, 2 ** 32, 2 ** 63 - 2]
POOL_I32 = [I32_MIN, I32_MAX, -1, 0]
SUBNORMAL = 0x0000000000000001
POOL_F64 = [0x0, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, SUBNORMAL, 0x7FF8000000000000,
            0xFFF8000000000001, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF]  # the last one = EMPTY_KEY
NAN_PAYLOADS = [0x7FF8000000000000, 0xFFF8000000000001, 0x7FF8000000000123, 0x7FFFFFFFFFFFFFFF]
STRINGS = ["", "a", "bc", "", "Zoë", "漢", "\U0001f642", "xyz" * 5]
PROBE_SIZES = [0, 1, 63, 64, 65, 511, 512, 513, 2 ** 15 - 1, 2 ** 15, 2 ** 15 + 1, 3 * 2 ** 15 + 7, 2 ** 16 - 1, 2 ** 16, 70_001]
JOIN_TYPES = ["inner", "left", "right", "full"]


def mix64(x: int) -> int:
    """the slot table's hash (a 64-bit finaliser), restated to CONSTRUCT keys that land on chosen slots — never an expectation"""
    m = (1 << 64) - 1
    x &= m
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & m
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & m
    x ^= x >> 33
    return x


def slot_capacity(n: int) -> int:
    cap = 64
    while 2 * cap < 3 * n:
        cap <<= 1
    return cap


# ---- columns ---------------------------------------------------------------------------------------------------------------------
def key_array(kind, keys, null):
    """keys: Python ints (values; bit patterns for f64; 0 / 1 for bool); null: bool per row or None"""
    mask = None if null is None or not np.any(null) else np.asarray(null, dtype=bool)
    if kind == "f64":
        raw = np.array([k & ((1 << 64) - 1) for k in keys], dtype=np.uint64).view(np.float64)
        return pa.array(raw, mask=mask, from_pandas=False)
    if kind == "bool":
        return pa.array(np.array(keys, dtype=bool), mask=mask)
    return pa.array(np.array(keys, dtype=np.int64 if kind == "i64" else np.int32), mask=mask)


def f64_payload(rng, n):
    bits = rng.integers(0, 1 << 62, n, dtype=np.uint64) | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))
    nan = rng.random(n) < 0.15
    bits[nan] = rng.choice(np.array(NAN_PAYLOADS, dtype=np.uint64), int(nan.sum()))
    neg0 = rng.random(n) < 0.05
    bits[neg0] = 0x8000000000000000
    return pa.array(bits.view(np.float64), mask=(rng.random(n) < 0.15) if n else None, from_pandas=False)


def i32_payload(rng, n):
    v = rng.integers(-3, 4, n).astype(np.int32)
    edge = rng.random(n) < 0.1
    v[edge] = rng.choice(np.array([I32_MIN, I32_MAX], dtype=np.int32), int(edge.sum()))
    return pa.array(v, mask=(rng.random(n) < 0.1) if n else None)


def bool_payload(rng, n):
    return pa.array(rng.random(n) < 0.5, mask=(rng.random(n) < 0.2) if n else None)


def utf8_payload(rng, n):
    vals = [STRINGS[i] for i in rng.integers(0, len(STRINGS), n)]
    null = rng.random(n) < 0.2
    return pa.array([None if z else v for v, z in zip(vals, null)], type=pa.string())


PAYLOADS = {"full": ("x", "i", "b", "s"), "numeric": ("x", "i"), "utf8": ("x", "i", "s"), "key_only": ()}
_MAKE = {"x": f64_payload, "i": i32_payload, "b": bool_payload, "s": utf8_payload}


def build_batch(rng, kind, keys, null, payload):
    cols, names = [key_array(kind, keys, null)], ["k"]
    for c in PAYLOADS[payload]:
        cols.append(_MAKE[c](rng, len(keys)))
        names.append(c)
    return pa.RecordBatch.from_arrays(cols, names=names)


def probe_batch(rng, kind, keys, null, payload):
    """(v f64, k key, w int32[, t Utf8, c Boolean]): the key is column 1.  A key-only build side keeps a numeric probe side."""
    n = len(keys)
    p = PAYLOADS["numeric" if payload == "key_only" else payload]
    cols, names = [f64_payload(rng, n), key_array(kind, keys, null), i32_payload(rng, n)], ["v", "k", "w"]
    if "s" in p:
        cols.append(utf8_payload(rng, n))
        names.append("t")
    if "b" in p:
        cols.append(bool_payload(rng, n))
        names.append("c")
    return pa.RecordBatch.from_arrays(cols, names=names)


LKEY, RKEY = 0, 1


class Case:
    def __init__(self, name, kind, route, build, probes, payload, all_hit=False, dup=False, facts=None):
        self.name, self.kind, self.route, self.build, self.probes, self.payload = name, kind, route, build, probes, payload
        self.all_hit, self.dup = all_hit, dup
        self.facts = facts  # what the GPU file's dispatch restatement reads: rows, NULL keys, the valid keys' ends, uniqueness

    @property
    def nleft(self):
        return self.build[0].num_columns

    def schema(self):
        return pa.schema([(f"l.{f.name}", f.type) for f in self.build[0].schema] + [(f"r.{f.name}", f.type) for f in self.probes[0].schema])

    def right_types(self):
        return [f.type for f in self.probes[0].schema]

    def filter_cols(self):
        """(l.i, r.w) in the joined schema, or None for a key-only build side"""
        return None if self.payload == "key_only" else (2, self.nleft + 2)

    def __repr__(self):
        return self.name


# ---- probe keys ------------------------------------------------------------------------------------------------------------------
def _wrap(v, kind):
    bits = 32 if kind == "i32" else 64
    return X.wrap(v, bits)


def miss_keys(kind, bkeys, bnull):
    """keys that have no build row, at the places where a table could think otherwise"""
    have = {k for k, z in zip(bkeys, bnull) if not z}
    if kind == "bool":
        return [k for k in (0, 1) if k not in have]
    if kind == "f64":
        valid = sorted(have)
        cand = POOL_F64 + [k ^ (1 << 63) for k in valid[:50]] + [k ^ 1 for k in valid[:50]] + [k + 1 for k in valid[-20:]]
        return [c & ((1 << 64) - 1) for c in cand if (c & ((1 << 64) - 1)) not in have]
    lo, hi = (min(have), max(have)) if have else (0, 0)
    pool = POOL_I64 if kind == "i64" else POOL_I32
    cand = pool + [lo - 1, hi + 1, lo + 2 ** 63, hi + 2 ** 63, lo - 2, hi + 2, lo + 2 ** 32, lo - 2 ** 32, lo + 2 ** 31, hi - 2 ** 31,
                   (lo + hi) // 2, (lo + hi) // 2 + 1] + [k + 1 for k in sorted(have)[:40]] + [k - 1 for k in sorted(have)[-40:]]
    out = [_wrap(c, kind) for c in cand]
    return [c for c in dict.fromkeys(out) if c not in have]


def probe_keys(rng, kind, bkeys, bnull, n, mode, hit_rows, miss_share=0.34):
    """mode: hit (every key has a build row) | mix (`miss_share` are misses) | nulls (mix, and a tenth NULL over slots that hold a build key)"""
    hits = [bkeys[r] for r in hit_rows if not bnull[r]]
    keys = [hits[i] for i in rng.integers(0, len(hits), n)] if n else []
    null = np.zeros(n, dtype=bool)
    if mode != "hit" and n:
        misses = miss_keys(kind, bkeys, bnull)
        if misses:
            for i in np.nonzero(rng.random(n) < miss_share)[0]:
                keys[i] = misses[int(rng.integers(0, len(misses)))]
    if mode == "nulls" and n:
        null = rng.random(n) < 0.1
        null[n // 2] = True
        for i in np.nonzero(null)[0]:
            keys[i] = hits[int(rng.integers(0, len(hits)))]  # (the slot under a NULL holds a key that HAS a build row)
    return keys, null


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def make(name, kind, route, bkeys, bnull=None, probes=(), payload="numeric", build_cuts=(), all_hit=False, hit_rows=None, seed=0,
         hit_share=0.8, miss_share=0.34):
    """probes: (rows, mode) per probe batch; build_cuts: row numbers at which the build side is cut into batches; hit_rows: the build
    rows probe hits are drawn from (default: a seeded four fifths of them)"""
    rng = np.random.default_rng(1000 + seed)
    n = len(bkeys)
    bnull = np.zeros(n, dtype=bool) if bnull is None else np.asarray(bnull, dtype=bool)
    if hit_rows is None:
        hit_rows = [r for r in range(n) if rng.random() < hit_share]
    whole = build_batch(rng, kind, bkeys, bnull, payload)
    cuts = [0] + list(build_cuts) + [n]
    build = [whole.slice(a, b - a) for a, b in zip(cuts, cuts[1:])]
    pbs = []
    for rows, mode in probes:
        keys, null = probe_keys(rng, kind, bkeys, bnull, rows, mode, hit_rows, miss_share)
        pbs.append(probe_batch(rng, kind, keys, null, payload))
    valid = [k for k, z in zip(bkeys, bnull) if not z]
    facts = dict(rows=n, nulls=int(bnull.sum()), lo=min(valid) if valid else None, hi=max(valid) if valid else None,
                 unique=len(set(valid)) == len(valid), distinct=len(set(valid)), kind=kind, key_only=payload == "key_only",
                 max_run=max([valid.count(k) for k in set(valid)] + [int(bnull.sum())]) if len(set(valid)) != len(valid) else max(1, int(bnull.sum())))
    dup = (len(set(valid)) != len(valid)) or int(bnull.sum()) > 1
    return Case(name, kind, route, build, pbs, payload, all_hit=all_hit, dup=dup, facts=facts)


def _shuffled(rng, xs):
    xs = list(xs)
    rng.shuffle(xs)
    return xs


def _sparse_i64(rng, n, avoid=()):
    out, have = [], set(avoid)
    while len(out) < n:
        v = int(rng.integers(I64_MIN, I64_MAX, dtype=np.int64))
        if v not in have:
            have.add(v)
            out.append(v)
    return out


SMALL = [(65, "nulls"), (1, "mix"), (0, "mix"), (64, "mix"), (63, "hit")]
TILES = [(513, "nulls"), (511, "mix"), (512, "mix"), (0, "mix"), (1, "hit")]
ALLHIT = [(2 ** 16, "hit"), (2 ** 16 - 1, "hit"), (70_001, "mix"), (2 ** 16, "hit"), (513, "nulls")]
RANGES = [(2 ** 15 - 1, "mix"), (2 ** 15, "hit"), (2 ** 15 + 1, "mix"), (3 * 2 ** 15 + 7, "mix"), (513, "nulls")]


def _cases():
    out = []

    def add(*a, **kw):
        kw.setdefault("seed", len(out))
        out.append(make(*a, **kw))
    rng = np.random.default_rng(77)
    # -- the ends of int64: `hi - lo + 1` wraps to 0 (the range test of dense_range.hpp)
    add("i64_extremes_2_hit_max", "i64", "slots", [I64_MIN, I64_MAX], probes=SMALL, payload="full", hit_rows=[1])
    add("i64_extremes_2_hit_min", "i64", "slots", [I64_MAX, I64_MIN], probes=SMALL, payload="numeric", hit_rows=[1])
    keys = _shuffled(rng, POOL_I64 + _sparse_i64(rng, 60_000 - len(POOL_I64), POOL_I64))
    pool_rows = [r for r, k in enumerate(keys) if k in POOL_I64]
    add("i64_extremes_60000", "i64", "slots", keys, probes=RANGES + [(70_001, "mix")], payload="numeric",
        hit_rows=pool_rows + list(range(0, 60_000, 2)))
    # -- dense ranges at the ends and the middle of int64; probe keys one below, one above, 2^63 away
    add("i64_dense_at_min_257", "i64", "dense", _shuffled(rng, range(I64_MIN, I64_MIN + 257)), probes=TILES, payload="full")
    add("i64_dense_at_max_256", "i64", "dense", _shuffled(rng, range(I64_MAX - 255, I64_MAX + 1)), probes=TILES, payload="utf8")
    add("i64_dense_around_zero", "i64", "dense", _shuffled(rng, range(-600, 600)), probes=SMALL + TILES, payload="full")
    add("i64_dense_around_2p31", "i64", "dense", _shuffled(rng, range(2 ** 31 - 1000, 2 ** 31 + 1000)), probes=TILES + [(4096, "mix")], payload="numeric")
    add("i64_dense_255", "i64", "dense", _shuffled(rng, range(-(2 ** 31) - 101, -(2 ** 31) - 101 + 255)), probes=TILES, payload="numeric")
    add("i64_dense_65535", "i64", "dense", _shuffled(rng, range(2 ** 32 - 30_000, 2 ** 32 - 30_000 + 65_535)), probes=ALLHIT, payload="numeric")
    add("i64_dense_65536", "i64", "dense", _shuffled(rng, range(-(2 ** 31) - 40_000, -(2 ** 31) - 40_000 + 65_536)), probes=ALLHIT, payload="key_only")
    add("i64_dense_65536_all_hit", "i64", "dense", _shuffled(rng, range(-70_000, -70_000 + 65_536)),
        probes=[(2 ** 16, "hit"), (70_001, "hit"), (2 ** 16 - 1, "hit")], payload="numeric", all_hit=True)
    # -- a range of exactly 4 x rows + 1024, and one more
    for name, span, route in (("i64_range_exact", 4 * 1000 + 1024, "dense"), ("i64_range_exact_plus_1", 4 * 1000 + 1025, "slots")):
        base = 2 ** 32 - 2000
        inner = rng.permutation(span - 2)[:998] + 1
        add(name, "i64", route, _shuffled(rng, [base, base + span - 1] + [base + int(v) for v in inner]), probes=TILES, payload="numeric")
    # -- NULL build keys: none above, one (it has a head of its own beside the table), several (duplicates: NULL = NULL)
    add("i64_one_key_and_a_null", "i64", "dense", [I64_MIN, 5], bnull=[False, True], probes=[(64, "mix"), (1, "hit"), (65, "mix")], payload="full", hit_rows=[0])
    keys = _shuffled(rng, range(-150, 150))
    add("i64_dense_one_null", "i64", "dense", keys, bnull=[r == 17 for r in range(300)], probes=SMALL + TILES, payload="full")
    add("i64_dense_three_nulls", "i64", "slots_dup", keys, bnull=[r in (3, 170, 299) for r in range(300)], probes=SMALL + TILES, payload="full")
    # -- build rows next to the packed table's "empty" pattern: 2^8 - 1 and 2^16 - 1 are the all-ones of 8 and 16 bits
    for n in (256, 257):
        add(f"i64_dense_{n}", "i64", "dense", _shuffled(rng, range(-1 - n // 2, -1 - n // 2 + n)), probes=TILES, payload="numeric")
    # -- the slot table: keys that hash to its last three slots (linear probing wraps past cap - 1, next to the reserved slots
    #    cap and cap + 1), the key -1 that lives in cap + 1, a NULL key that lives in cap
    n = 80
    cap = slot_capacity(n)
    tail_keys = []
    while len(tail_keys) < 14:
        v = int(rng.integers(I64_MIN, I64_MAX, dtype=np.int64))
        if mix64(v) & (cap - 1) >= cap - 3:
            tail_keys.append(v)
    keys = tail_keys + [-1] + _sparse_i64(rng, n - 16, tail_keys + [-1]) + [0]
    add("i64_slot_wrap", "i64", "slots", keys, bnull=[r == n - 1 for r in range(n)], probes=SMALL + TILES, payload="full",
        hit_rows=list(range(0, 15)) + list(range(20, 60)) + [n - 1])
    keys2 = (tail_keys + [-1] + _sparse_i64(rng, 24, tail_keys + [-1])) * 2
    assert slot_capacity(len(keys2)) == cap
    add("i64_slot_wrap_twice", "i64", "slots_dup", keys2, probes=SMALL + TILES, payload="full", hit_rows=list(range(0, 15)) + list(range(20, 35)))
    # -- one key 5 000 times: over a range of two keys (runs by key), and among sparse keys (CSR runs)
    add("i64_one_key_5000_dense", "i64", "dd", [2 ** 32] * 2500 + [2 ** 32 + 1] + [2 ** 32] * 2500, probes=[(512, "mix"), (511, "mix"), (513, "nulls")],
        payload="numeric", hit_rows=[0, 1, 2], miss_share=0.97)
    keys = _shuffled(rng, [I64_MAX] * 5000 + _sparse_i64(rng, 200, [I64_MAX]))
    add("i64_one_key_5000_sparse", "i64", "slots_dup", keys, probes=[(64, "mix"), (63, "mix"), (65, "nulls")], payload="numeric", miss_share=0.9)
    # -- every key exactly twice
    keys = _shuffled(rng, list(range(-1500, 1500)) * 2)
    add("i64_twice_dense", "i64", "dd", keys, probes=TILES + [(4096, "mix"), (2 ** 15 + 1, "mix")], payload="full")
    keys = _shuffled(rng, (POOL_I64 + _sparse_i64(rng, 1500, POOL_I64)) * 2)
    add("i64_twice_sparse", "i64", "slots_dup", keys, probes=TILES + [(4096, "mix"), (2 ** 15 + 1, "mix")], payload="full")
    # -- three build batches, a NULL in the second
    keys = _shuffled(rng, range(2 ** 31 - 450, 2 ** 31 + 450))
    add("i64_three_build_batches_dense", "i64", "dense", keys, bnull=[r == 400 for r in range(900)], probes=SMALL + TILES, payload="full", build_cuts=(300, 600))
    keys = _shuffled(rng, POOL_I64 + _sparse_i64(rng, 889, POOL_I64))
    add("i64_three_build_batches_sparse", "i64", "slots", keys, bnull=[r == 400 for r in range(900)], probes=SMALL + TILES, payload="utf8", build_cuts=(300, 600))
    # -- float64 keys, by pattern
    rnd = [int(v) for v in rng.integers(1, 1 << 62, 800, dtype=np.uint64)]
    keys = _shuffled(rng, POOL_F64 + [v for v in dict.fromkeys(rnd) if v not in POOL_F64][:760])
    pool_rows = [r for r, k in enumerate(keys) if k in POOL_F64]
    add("f64_pool_unique", "f64", "slots", keys, probes=SMALL + TILES + [(4096, "mix"), (2 ** 15 + 1, "mix")], payload="full",
        hit_rows=pool_rows + list(range(0, len(keys), 2)))
    add("f64_pool_twice", "f64", "slots_dup", _shuffled(rng, keys * 2), probes=SMALL + TILES + [(4096, "mix")], payload="numeric")
    # -- int32 keys: both ends (a sign-extended range of 2^32: never the direct-address table), and a dense set
    rnd = [int(v) for v in rng.integers(I32_MIN, I32_MAX, 700)]
    keys = _shuffled(rng, POOL_I32 + [v for v in dict.fromkeys(rnd) if v not in POOL_I32])
    add("i32_extremes", "i32", "slots", keys, probes=SMALL + TILES + [(4096, "mix")], payload="full",
        hit_rows=[r for r, k in enumerate(keys) if k in POOL_I32] + list(range(0, len(keys), 2)))
    add("i32_dense_at_min", "i32", "dense", _shuffled(rng, range(I32_MIN, I32_MIN + 700)), probes=SMALL + TILES, payload="numeric")
    add("i32_dense_twice_at_max", "i32", "dd", _shuffled(rng, list(range(I32_MAX - 699, I32_MAX + 1)) * 2), probes=SMALL + TILES, payload="numeric")
    # -- Boolean keys
    add("bool_true_and_null", "bool", "dense", [1, 0], bnull=[False, True], probes=[(64, "mix"), (1, "hit"), (65, "mix")], payload="full", hit_rows=[0])
    add("bool_duplicates", "bool", "slots_dup", [1, 1, 0, 0, 1], bnull=[False, False, False, True, True], probes=[(65, "nulls"), (1, "hit"), (64, "nulls")],
        payload="numeric", hit_rows=[0, 1, 3, 4], all_hit=True)
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    return {c.name: c for c in _cases()}


def case(name):
    return all_cases()[name]


def names(route=None, kind=None):
    return [c.name for c in all_cases().values() if (route is None or c.route in (route if isinstance(route, tuple) else (route,)))
            and (kind is None or c.kind == kind)]


# ---- driving a backend -----------------------------------------------------------------------------------------------------------
def run(be, case, jt, probes=None, filt=None, indices_only=False, build=None, **kw):
    """the batches HashJoinExecutor(be) emits for the case: one per probe batch, then the tail (Left / Full)"""
    from sqlrs_amd.executor import HashJoinExecutor
    from sqlrs_amd.expr import InputRef, JoinCondition
    cond = JoinCondition([(InputRef(LKEY), InputRef(RKEY))], filt)
    ex = HashJoinExecutor(be, case.build if build is None else build, case.probes if probes is None else probes, jt, cond,
                          case.schema(), case.nleft, **kw)
    return list(ex.execute(indices_only=indices_only))


def filter_of(case):
    """l.i > r.w over the joined row: NULL where either side is (every (NULL, row) candidate of a Right / Full join)"""
    from sqlrs_amd.expr import InputRef
    li, rw = case.filter_cols()
    return InputRef(li) > InputRef(rw)
