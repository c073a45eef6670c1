"""sqlrs_hash_join_set_async_keys: the cases of tests/test_async_join_keys_cpu.py and tests/test_gpu_async_join_keys.py, the
eligibility rule of include/sqlrs_hip.h restated from the batch, the build side and the header's constants, and the arithmetic of a
hashed key (csrc/key_hash.hpp) restated in Python integers (no library call: numpy and pyarrow only).  The byte formulas are those
of tests/async_utf8_cases.py."""
import struct

import numpy as np
import pyarrow as pa

from async_utf8_cases import SA_AREA, SA_MAX_COLS, SA_MAX_OUT_ROWS, SA_MAX_ROWS, in_bytes, is_str, out_bytes, rand_strings, str_array, width_of
from sqlrs_amd import abi
from sqlrs_amd.expr import Constant, InputRef, JoinCondition

JOIN_TYPES = ["inner", "left", "right", "full"]
FORMS = ["unique_dense", "unique_sparse", "dup_dense", "dup_sparse"]
SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4096, 4097]  # (a wave ballot, a 1024-row chunk, the row limit; 4097: synchronous)

# ---- the key of a row, as normalize_keys' hash mode computes it (csrc/key_hash.hpp) ------------------------------------------
M64 = (1 << 64) - 1
TAG_32, TAG_64, TAG_UTF8 = 0x3232323200000000, 0x9E3779B97F4A7C15, 0x7575757575757575


def mix64(x):
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & M64
    return x ^ (x >> 33)


def combine_hashes(l, r):
    return ((17 * 37 + l) * 37 + r) & M64


def fnv1a(data):
    x = 0xCBF29CE484222325
    for b in data:
        x = ((x ^ b) * 0x100000001B3) & M64
    return x


def value_hash(kind, v):
    """kind: "i32" (zero-extended) / "i64" / "f64" (bit pattern) / "str" """
    if kind == "i32":
        return mix64(((int(v) & 0xFFFFFFFF) + TAG_32) & M64)
    if kind == "i64":
        return mix64(((int(v) & M64) + TAG_64) & M64)
    if kind == "f64":
        return mix64((struct.unpack("<Q", struct.pack("<d", float(v)))[0] + TAG_64) & M64)
    return mix64(fnv1a(v.encode() if isinstance(v, str) else bytes(v)) ^ TAG_UTF8)


def row_key(kinds, values):
    """acc = 0; a NULL leaves it unchanged; one column: acc = v, several: acc = combine_hashes(v, acc)"""
    acc = 0
    for kind, v in zip(kinds, values):
        if v is None:
            continue
        h = value_hash(kind, v)
        acc = combine_hashes(h, acc) if len(kinds) > 1 else h
    return acc


# the three fixed tables of host/key_hash_check.cpp (the same rows, in the same order)
KEY_TABLES = [
    (["str"], [[""], [None], ["a"], ["ab"], ["abc"], ["abd"], ["12345678"], ["123456789"], ["x" * 200], ["é漢\U0001f642"]]),
    (["i64", "i64"], [[1, 2], [2, 1], [None, 5], [5, None], [None, None], [-1, -(1 << 63)], [0, 0]]),
    (["f64", "i64", "str", "i32"], [[0.5, 7, "k", -1], [None, 7, "k", -1], [0.5, None, "k", -1], [0.5, 7, None, -1], [0.5, 7, "k", None],
                                    [-0.0, 0, "", 0], [None, None, None, None], [1e300, (1 << 63) - 1, "Zoë", 2147483647]]),
]


# ---- what the rule reads ----------------------------------------------------------------------------------------------
def kind_of(t):
    return "i32" if pa.types.is_int32(t) else "i64" if pa.types.is_int64(t) else "f64" if pa.types.is_float64(t) else "str" if is_str(t) else "other"


def exact_mode(lb, on):
    """one fixed-width build key: compared exactly; otherwise (a Utf8 key, several columns) matched by hash"""
    return len(on) == 1 and kind_of(lb.schema.field(on[0][0]).type) in ("i32", "i64", "f64")


def max_run(lb, on):
    """M: the most build rows that share one key — exact mode: one value (NULL keys share one); hash mode: one hash"""
    if lb.num_rows == 0:
        return 1
    cols = [lb.column(l).to_pylist() for l, _ in on]
    if exact_mode(lb, on):
        keys = cols[0]
    else:
        kinds = [kind_of(lb.schema.field(l).type) for l, _ in on]
        keys = [row_key(kinds, vals) for vals in zip(*cols)]
    counts = {}
    for k in keys:
        counts[k] = counts.get(k, 0) + 1
    return max(counts.values())


def eligible(case, rb, jt, m, general, keys=True, utf8=True, filt=True):
    """the header's rule for one probe batch.  keys / utf8 / filt / general: the four switches; keys = False is the rule as it
    was: ONE exactly compared fixed-width key without a NULL in the batch"""
    lb, on, rows = case.lb, case.on, rb.num_rows
    if rows > SA_MAX_ROWS or lb.num_columns + rb.num_columns > SA_MAX_COLS or not case.bare_refs:
        return False
    if case.filter is not None and not filt:
        return False
    if not 1 <= len(on) <= (4 if keys else 1):
        return False
    exact = exact_mode(lb, on)
    if not exact and not keys:
        return False
    for l, r in on:
        kind = kind_of(rb.schema.field(r).type)
        if kind == "other" or (kind == "str" and not utf8):
            return False  # (a Boolean key; a Utf8 key without the Utf8 switch)
        if exact and rb.schema.field(r).type != lb.schema.field(l).type:
            return False
        if not exact and len(on) == 1 and kind != "str":
            return False
        if rb.column(r).null_count and not keys:
            return False
    for f in list(lb.schema) + list(rb.schema):
        if not (width_of(f.type) or (utf8 and is_str(f.type))):
            return False  # (Boolean; Utf8 with the switch off)
    inner_unique = jt == "inner" and m == 1
    if not inner_unique and not general:
        return False
    out_rows = rows if inner_unique else rows * m
    return out_rows <= SA_MAX_OUT_ROWS and out_bytes(lb, rb, out_rows) <= SA_AREA and in_bytes(rb) <= SA_AREA


def count_eligible(case, jt, general, keys=True, utf8=True, filt=True):
    m = max_run(case.lb, case.on)
    return sum(1 for b in case.rbs if eligible(case, b, jt, m, general, keys, utf8, filt))


# ---- arrays -----------------------------------------------------------------------------------------------------------
def fixed_array(values, null_mask=None, bitmap=False):
    """a fixed-width array whose NULL slots KEEP the values underneath; bitmap: a validity bitmap even without a NULL"""
    values = np.ascontiguousarray(values)
    n = len(values)
    t = pa.from_numpy_dtype(values.dtype)
    nulls = int(null_mask.sum()) if null_mask is not None else 0
    if not nulls and not bitmap:
        return pa.array(values)
    mask = null_mask if null_mask is not None else np.zeros(n, dtype=bool)
    validity = pa.py_buffer(np.packbits(~mask, bitorder="little").tobytes())
    return pa.Array.from_buffers(t, n, [validity, pa.py_buffer(values.tobytes())], nulls if nulls else -1)  # (-1: counted from the bitmap, which is then kept)


def null_pattern(rng, rows, what):
    m = np.zeros(rows, dtype=bool)
    if not rows or what == "none":
        return m
    if what == "all":
        m[:] = True
    if "first" in what:
        m[0] = True
    if "last" in what:
        m[-1] = True
    if "6364" in what:
        m[[i for i in (63, 64) if i < rows]] = True
    if "random" in what:
        m |= rng.random(rows) < 0.1
    return m


# (size -> where the NULL keys sit)
PATTERNS = {0: "none", 1: "all", 63: "last", 64: "first 6364", 65: "6364", 1023: "random", 1024: "all", 1025: "bitmap", 4096: "first last random",
            4097: "random"}


class Case:
    def __init__(self, name, lb, rbs, on, want, filt=None, bare_refs=True, cond=None):
        """on: (build column, probe column) pairs; want: {(join type, async_general): batches the rule admits with every other
        switch on} — counted by hand where the case is built"""
        self.name, self.lb, self.rbs, self.on, self.want, self.filter, self.bare_refs = name, lb, rbs, on, want, filt, bare_refs
        self.cond = cond if cond is not None else JoinCondition([(InputRef(l), InputRef(r)) for l, r in on], filt)

    def __repr__(self):
        return self.name


_cache = {}


def _cached(fn):
    def wrapped(*a):
        key = (fn.__name__,) + a
        if key not in _cache:
            _cache[key] = fn(*a)
        return _cache[key]
    return wrapped


def _want(inner_false, inner_true, outer_true):
    """{(jt, general): count}: Inner with async_general off / on, the outer joins with it on (off: they take no kernel)"""
    w = {("inner", False): inner_false, ("inner", True): inner_true}
    for jt in JOIN_TYPES[1:]:
        w[(jt, False)] = 0
        w[(jt, True)] = outer_true
    return w


# ---- NULL probe keys, exact mode ----------------------------------------------------------------------------------------
DTYPES = {"i64": np.int64, "i32": np.int32, "f64": np.float64}
EXACT = [("i64", f, n) for f in FORMS for n in (0, 1, 3)] + [("i32", "unique_dense", 1), ("i32", "unique_sparse", 0), ("i32", "dup_sparse", 3),
                                                             ("i32", "dup_dense", 0), ("f64", "unique_sparse", 1), ("f64", "dup_sparse", 3), ("f64", "unique_sparse", 3)]


@_cached
def exact_case(dtype, form, nnull):
    """build (k, x, y): 600 rows over the table form's keys, `nnull` of them with a NULL key (M = 3 on a unique form with 3 of
    them); probe (k, v): every size of SIZES with the NULL keys where PATTERNS says, the value of an existing build key or anything
    else underneath, keys in and out of the build side's range"""
    rng = np.random.default_rng(100 * list(DTYPES).index(dtype) + 10 * FORMS.index(form) + nnull)
    if dtype == "f64":
        conv = lambda x: x.astype(np.float64) * 0.5 + 0.25
    elif form.endswith("sparse"):
        conv = lambda x: (x.astype(np.int64) * 7919 - 5).astype(DTYPES[dtype])
    else:
        conv = lambda x: (x.astype(np.int64) - 17).astype(DTYPES[dtype])
    if form.startswith("unique"):
        raw = rng.permutation(900)[:600]
    else:
        raw = np.repeat(np.arange(150), 4)  # M = 4
        rng.shuffle(raw)
    nb = len(raw)
    knull = np.zeros(nb, dtype=bool)
    knull[[0, nb // 2, nb - 1][:nnull]] = True
    kvals = conv(raw)
    kvals[knull] = kvals[1]  # (an existing key under the NULL slots)
    lb = pa.RecordBatch.from_arrays([fixed_array(kvals, knull), pa.array(rng.integers(-50, 50, nb), mask=rng.random(nb) < 0.1), pa.array(rng.random(nb))],
                                    names=["k", "x", "y"])
    rbs = []
    for rows in SIZES:
        pat = PATTERNS[rows]
        keys = conv(rng.integers(0, 1100, rows))
        mask = null_pattern(rng, rows, pat)
        under = rng.random(rows) < 0.5
        keys[mask & under] = kvals[1]
        rbs.append(pa.RecordBatch.from_arrays([fixed_array(keys, mask, bitmap=pat == "bitmap"),
                                               pa.array(rng.integers(-9, 9, rows).astype(np.int32), mask=(rng.random(rows) < 0.2) if rows else None)], names=["k", "v"]))
    m = 4 if form.startswith("dup") else max(nnull, 1)
    # by hand: 9 batches have <= 4096 rows.  M = 1: all 9 on every route.  M = 3: the 4096-row batch is laid out for 12288 rows,
    # five columns (8 + 8 + 8 + 8 + 4 bytes, int32 key: 4 + 8 + 8 + 4 + 4) -> at most 4 x 98304 + 49152 + 5 x 1536 + 64 < 524288: 9.
    # M = 4: 16384 rows, int64 / float64 key: 4 x 131072 + 65536 > 524288 -> 8; int32 key: 3 x 65536 + 2 x 131072 + 5 x 2048 + 64
    # = 469056 -> 9.  Without async_general only Inner over M = 1 takes a kernel.
    gen = 9 if (m < 4 or dtype == "i32") else 8
    return Case(f"null_{dtype}_{form}_{nnull}", lb, rbs, [(0, 0)], _want(9 if m == 1 else 0, gen, gen))


# ---- a Utf8 key -----------------------------------------------------------------------------------------------------------
SPECIAL = ["", "a", "ab", "abc", "abd", "12345678", "123456789", "é", "漢字", "Zoë\U0001f642", "prefix", "prefixx"]


@_cached
def utf8_case(dup):
    """build (s, x): the special strings (empty, a string and its proper prefix, a last-byte difference, 1 / 8 / 9 bytes, multi-byte)
    and 300 others, one NULL key with bytes underneath; unique — then with a 200-byte key — or every key four times.  probe (v, t):
    t drawn from the build keys, near misses and NULLs (bytes underneath), its offsets starting at 5"""
    rng = np.random.default_rng(211 + dup)
    keys = SPECIAL + [f"key{i:04d}" for i in range(300)] + ([] if dup else ["L" * 200])
    vals = keys + ["abc"]  # (the NULL key's bytes: an existing key)
    knull = np.zeros(len(vals), dtype=bool)
    knull[-1] = True
    idx = np.arange(len(vals))
    if dup:
        idx = np.repeat(idx, 4)
        rng.shuffle(idx)
    lb = pa.RecordBatch.from_arrays([str_array([vals[i] for i in idx], knull[idx]), pa.array(rng.integers(-50, 50, len(idx)), mask=rng.random(len(idx)) < 0.1)],
                                    names=["s", "x"])
    pool = keys + ["abe", "ab ", "A", "prefi", "key", "key03000", "L" * 199 + "M", "é漢"]
    rbs = []
    for rows in SIZES:
        t = [pool[i] for i in rng.integers(0, len(pool), rows)]
        mask = null_pattern(rng, rows, PATTERNS[rows].replace("bitmap", "none"))
        rbs.append(pa.RecordBatch.from_arrays([pa.array(rng.integers(-9, 9, rows).astype(np.int32), mask=(rng.random(rows) < 0.2) if rows else None),
                                               str_array(t, mask, shift=5)], names=["v", "t"]))
    # by hand.  unique (Lmax = 200): the build key column alone needs out_rows x 200 bytes -> 4096 rows (819200) do not fit, 1025 do:
    # 8 batches.  dup (M = 4 — the NULL key's four rows share table[cap] — Lmax = 14, "Zoë" + U+1F642 = 4 + 4 ... the longest is
    # "123456789" / "key0000" .. : <= 14): 1025 rows -> 4100 output rows, <= 4100 x 14 + 4 x B_t + fixed columns, far below; 4096
    # rows -> 16384 output rows: s 65600 + 229376, x 131072, v 65536, t 65600 + 4 x B_t (B_t >= 4096 x 5) -> over 524288: 8 batches.
    return Case(f"utf8_{'dup' if dup else 'unique'}", lb, rbs, [(0, 1)], _want(0 if dup else 8, 8, 8))


# ---- two to four key columns ----------------------------------------------------------------------------------------------
def _key_col(rng, kind, n, null_rate, domain):
    mask = rng.random(n) < null_rate if null_rate else None
    if kind == "str":
        return str_array([domain[i] for i in rng.integers(0, len(domain), n)], mask)
    vals = np.asarray(domain)[rng.integers(0, len(domain), n)].astype(DTYPES[kind])
    return fixed_array(vals, mask)


MULTI = {"i64_i64": ["i64", "i64"], "i32_str": ["i32", "str"], "f64_i64_str_i32": ["f64", "i64", "str", "i32"]}
_DOMAIN = {"i64": list(range(-3, 40)), "i32": list(range(-2, 9)), "f64": [0.25 * i for i in range(8)], "str": ["", "a", "ab", "b", "é", "漢字", "abc"]}


@_cached
def multi_case(name):
    """build (key columns.., x), probe (v, key columns..): values from small domains so that tuples repeat, a NULL in every key
    position (5 % per column, so also in several at once), swapped values (a, b) / (b, a) — one hash under combine_hashes"""
    kinds = MULTI[name]
    rng = np.random.default_rng(307 + len(kinds) * 7 + list(MULTI).index(name))
    nb = 400 if len(kinds) == 2 else 700
    lb = pa.RecordBatch.from_arrays([_key_col(rng, k, nb, 0.05, _DOMAIN[k]) for k in kinds] + [pa.array(rng.integers(-50, 50, nb), mask=rng.random(nb) < 0.1)],
                                    names=[f"k{i}" for i in range(len(kinds))] + ["x"])
    rbs = []
    for rows in SIZES:
        rbs.append(pa.RecordBatch.from_arrays([pa.array(rng.integers(-9, 9, rows).astype(np.int32))] + [_key_col(rng, k, rows, 0.05, _DOMAIN[k]) for k in kinds],
                                              names=["v"] + [f"k{i}" for i in range(len(kinds))]))
    on = [(i, i + 1) for i in range(len(kinds))]
    # by hand, from M (MULTI_M, counted by hash): tuples repeat, M >= 2, so nothing without async_general.  With it the eight batches
    # of <= 1025 rows: 1025 x 11 = 11275 <= 16384 rows, and at most ten columns of <= 8 bytes (80 + 10 / 8 bytes a row) plus <= 6-byte
    # strings give < 11275 x 100 + 10 x 128 + 64 bytes < 524288.  The 4096-row batch: M = 11 -> 45056 rows > 16384; M = 3 -> 12288 rows
    # x (3 x 8 + 4 + 2 x 8) bytes = 540672 > 524288; M = 2 -> 8192 rows x (4 x 8 + 2 x 4 + 4 x 8 - the Utf8 columns' offsets count 4)
    # = 8192 x 68 = 557056 > 524288: not taken.
    return Case(f"multi_{name}", lb, rbs, on, _want(0, 8, 8))


MULTI_M = {"i64_i64": 3, "i32_str": 11, "f64_i64_str_i32": 2}


@_cached
def unique_pair_case():
    """(int64, int64) keys (a, a + 1000): no tuple twice, no swapped partner, one all-NULL key -> M = 1 by hash: the Inner / unique
    route in hash mode.  Probe rows: hits, misses, swapped tuples (a + 1000, a) — one hash with (a, a + 1000): match-by-hash finds them — NULLs"""
    rng = np.random.default_rng(331)
    a = rng.permutation(800)[:500].astype(np.int64)
    n0, n1 = np.zeros(500, dtype=bool), np.zeros(500, dtype=bool)
    n0[7] = n1[7] = True
    lb = pa.RecordBatch.from_arrays([fixed_array(a, n0), fixed_array(a + 1000, n1), pa.array(rng.random(500))], names=["a", "b", "y"])
    rbs = []
    for rows in SIZES:
        pa_ = rng.integers(0, 900, rows).astype(np.int64)
        pb = pa_ + 1000
        swap = rng.random(rows) < 0.1
        pa_[swap], pb[swap] = pb[swap], pa_[swap].copy()
        both = null_pattern(rng, rows, PATTERNS[rows])
        rbs.append(pa.RecordBatch.from_arrays([fixed_array(pa_, both), fixed_array(pb, both | (rng.random(rows) < 0.02) if rows else both)], names=["a", "b"]))
    # by hand: M = 1, five 8-byte columns: all 9 batches of <= 4096 rows, on every route
    return Case("unique_pair", lb, rbs, [(0, 0), (1, 1)], _want(9, 9, 9))


@_cached
def mismatch_case():
    """an int32 probe column against an int64 build column: the values agree, the tags do not — no row finds a partner, in push_async
    and in push alike; the batches are taken all the same"""
    c = unique_pair_case()
    hit = c.lb.column(0).to_numpy(zero_copy_only=False)[20:30].astype(np.int64)  # (valid build keys: row 7 holds the NULL one)
    rbs = []
    for n in (65, 1024, 4097):
        v = np.resize(hit, n)
        rbs.append(pa.RecordBatch.from_arrays([pa.array(v.astype(np.int32)), pa.array(v + 1000)], names=["a", "b"]))
    # by hand: M = 1, the two batches of <= 4096 rows, on every route
    return Case("mismatch_i32_i64", c.lb, rbs, [(0, 0), (1, 1)], _want(2, 2, 2))


# ---- composition ------------------------------------------------------------------------------------------------------------
@_cached
def filter_case():
    """exact int64 key with one NULL build key, filter `l.x > r.v` over payload columns: the NULL-key probe rows find the NULL
    build row (x = -100) and only the filter keeps them out (v >= -9)"""
    c = exact_case("i64", "unique_sparse", 1)
    x = c.lb.column(1).to_numpy(zero_copy_only=False).copy()
    xm = np.isnan(x)
    x = np.where(xm, 0, x).astype(np.int64)
    x[0] = -100  # (row 0 holds the NULL key)
    xm[0] = False
    lb = pa.RecordBatch.from_arrays([c.lb.column(0), fixed_array(x, xm), c.lb.column(2)], names=c.lb.schema.names)
    rbs = [pa.RecordBatch.from_arrays([b.column(0), b.column(1).cast(pa.int64())], names=b.schema.names) for b in c.rbs]
    filt = InputRef(1) > InputRef(4)
    # by hand: M = 1, five 8-byte columns: the 9 batches of <= 4096 rows
    return Case("filter_payload", lb, rbs, [(0, 0)], _want(9, 9, 9), filt=filt)


@_cached
def div0_case():
    """`l.x / r.v > 0` on the same tables: a NULL-key probe row whose partner (the NULL build row) is valid and whose v = 0"""
    c = filter_case()
    k = fixed_array(np.array([5, 6, 7], dtype=np.int64), np.array([False, True, False]))
    rb = pa.RecordBatch.from_arrays([k, pa.array(np.array([1, 0, 2], dtype=np.int64))], names=["k", "v"])
    nz = lambda b: pa.RecordBatch.from_arrays([b.column(0), pa.array([1 if v == 0 else v for v in b.column(1).to_pylist()], type=pa.int64())], names=b.schema.names)
    return Case("div0", c.lb, [nz(c.rbs[3]), rb, nz(c.rbs[4])], [(0, 0)], None, filt=(InputRef(1) / InputRef(4)) > Constant(0, abi.INT64))


@_cached
def bound_case():
    """the byte bound on the general route: an (int64, int64) key, every build tuple twice (M = 2), a 100-byte build string beside
    it — every probe row reserves 2 x 100 bytes for that column alone, so the bytes decide long before the row limit does: the
    largest batch the rule admits, the batch one row larger, and a small one"""
    rng = np.random.default_rng(347)
    a = np.repeat(np.arange(200, dtype=np.int64), 2)
    lb = pa.RecordBatch.from_arrays([pa.array(a), pa.array(a * 3), str_array(["s" * 100] + rand_strings(rng, len(a) - 1))], names=["a", "b", "s"])
    probe = lambda rows: pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 220, rows)), pa.array(rng.integers(0, 220, rows) * 3)], names=["a", "b"])
    case = Case("bound", lb, [], [(0, 0), (1, 1)], None)
    fits = [r for r in range(1, SA_MAX_ROWS + 1) if eligible(case, probe(r), "left", 2, True)]
    assert fits == list(range(1, fits[-1] + 1))
    r_ok = fits[-1]
    case.rbs = [probe(r_ok), probe(r_ok + 1), probe(64)]
    case.r_ok = r_ok
    case.want = _want(0, 2, 2)
    return case


@_cached
def refused_case(what):
    """five key columns / a Boolean key / a key expression that is not a bare reference: nothing takes a kernel"""
    rng = np.random.default_rng(353)
    n = 200
    if what == "five":
        cols = [pa.array(rng.integers(0, 5, n)) for _ in range(5)]
        lb = pa.RecordBatch.from_arrays(cols, names=list("abcde"))
        rbs = [pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 5, r)) for _ in range(5)], names=list("abcde")) for r in (64, 1024)]
        return Case("five_keys", lb, rbs, [(i, i) for i in range(5)], _want(0, 0, 0))
    if what == "bool":
        lb = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 50, n)), pa.array(rng.random(n) < 0.5)], names=["a", "f"])
        rbs = [pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 60, r)), pa.array(rng.random(r) < 0.5)], names=["a", "f"]) for r in (64, 1024)]
        return Case("bool_key", lb, rbs, [(0, 0), (1, 1)], _want(0, 0, 0))
    lb = pa.RecordBatch.from_arrays([pa.array(rng.permutation(n).astype(np.int64)), pa.array(rng.integers(0, 9, n))], names=["a", "b"])
    rbs = [pa.RecordBatch.from_arrays([pa.array(rng.integers(0, n, r)), pa.array(rng.integers(0, 9, r))], names=["a", "b"]) for r in (64, 1024)]
    cond = JoinCondition([(InputRef(0), InputRef(0)), (InputRef(1), InputRef(1) + Constant(0, abi.INT64))])
    return Case("expr_key", lb, rbs, [(0, 0), (1, 1)], _want(0, 0, 0), bare_refs=False, cond=cond)


def mixed_cases():
    """the cases with 0 < eligible < batches on some route"""
    return [exact_case(*e) for e in EXACT] + [utf8_case(False), utf8_case(True)] + [multi_case(n) for n in MULTI] + [unique_pair_case(), mismatch_case(),
                                                                                                                 filter_case(), bound_case()]


# ---- the fuzz ---------------------------------------------------------------------------------------------------------
FUZZ_SEEDS = list(range(8))


@_cached
def fuzz_case(seed):
    """random join type, 1-3 key columns from {i64, i32, f64, str} with NULL rates 0 / 5 / 50 %, payload columns on both sides,
    sizes from SIZES; -> (case, join type, async_general, depth)"""
    rng = np.random.default_rng(9300 + seed)
    jt = JOIN_TYPES[seed % 4]
    general = seed != 4
    nk = int(rng.integers(1, 4))
    kinds = [str(rng.choice(["i64", "i32", "f64", "str"])) for _ in range(nk)]
    nb = int(rng.choice([5, 300, 3000]))
    dom = {"i64": list(range(0, 3 * nb, 2)) if nk == 1 else list(range(12)), "i32": list(range(0, 3 * nb, 3)) if nk == 1 else list(range(7)),
           "f64": [0.5 * i for i in range(2 * nb if nk == 1 else 6)], "str": [f"s{i}" for i in range(2 * nb)] if nk == 1 else ["", "a", "ab", "é", "zz"]}
    rates = [float(rng.choice([0.0, 0.05, 0.5])) for _ in range(nk)]
    lb = pa.RecordBatch.from_arrays([_key_col(rng, k, nb, p, dom[k]) for k, p in zip(kinds, rates)] + [pa.array(rng.random(nb), mask=rng.random(nb) < 0.1)],
                                    names=[f"k{i}" for i in range(nk)] + ["y"])
    sizes = [int(x) for x in rng.choice(SIZES, size=8)]
    rbs = [pa.RecordBatch.from_arrays([_key_col(rng, k, n, p, dom[k]) for k, p in zip(kinds, rates)] + [str_array(rand_strings(rng, n), (rng.random(n) < 0.2) if n else None)],
                                      names=[f"k{i}" for i in range(nk)] + ["t"]) for n in sizes]
    return Case(f"fuzz{seed}", lb, rbs, [(i, i) for i in range(nk)], None), jt, general, int(rng.integers(1, 9))
