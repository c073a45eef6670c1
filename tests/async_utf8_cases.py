"""sqlrs_hash_join_set_async_utf8: the cases of tests/test_async_join_utf8_cpu.py and tests/test_gpu_async_join_utf8.py, and the
eligibility rule of include/sqlrs_hip.h restated from the batch, the build side's true M, the true Lmax of every Utf8 build
column and the header's constants (no library call: numpy and pyarrow only)."""
import numpy as np
import pyarrow as pa

from sqlrs_amd.expr import InputRef, JoinCondition

SA_MAX_ROWS, SA_MAX_OUT_ROWS, SA_AREA, SA_MAX_COLS = 4096, 16384, 512 * 1024, 12  # (sqlrs_hip.h / csrc/small_async.hpp)
JOIN_TYPES = ["inner", "left", "right", "full"]
FORMS = ["unique_dense", "unique_sparse", "dup_dense", "dup_sparse"]


def up64(x):
    return (x + 63) & ~63


# ---- what the rule reads ----------------------------------------------------------------------------------------------
def offsets_of(arr):
    """the int32 offsets the ABI hands over for a Utf8 column: rows + 1 of them (a slice: its own window)"""
    buf = arr.buffers()[1]
    if buf is None:
        return np.zeros(1, dtype=np.int32)
    return np.frombuffer(buf, dtype=np.int32)[arr.offset:arr.offset + len(arr) + 1]


def lmax_of(arr):
    """the longest string of a build column in bytes, NULL slots included"""
    d = np.diff(offsets_of(arr))
    return int(d.max()) if len(d) else 0


def bytes_of(arr):
    """B_c = offsets[rows] - offsets[0]"""
    o = offsets_of(arr)
    return int(o[-1]) - int(o[0])


def max_run(lb, key_col):
    """M: the most build rows that share one key"""
    k = lb.column(key_col).to_numpy(zero_copy_only=False)
    return int(np.unique(k, return_counts=True)[1].max()) if len(k) else 1


def is_str(t):
    return pa.types.is_string(t)


def width_of(t):
    return 4 if pa.types.is_int32(t) else 8 if (pa.types.is_int64(t) or pa.types.is_float64(t)) else 0


def has_utf8(lb, rb):
    return any(is_str(f.type) for f in list(lb.schema) + list(rb.schema))


def out_bytes(lb, rb, out_rows):
    """64 + the pieces of every output column laid out for out_rows rows"""
    rows = rb.num_rows
    total = 64
    for side, b in (("build", lb), ("probe", rb)):
        for c in range(b.num_columns):
            t, arr = b.schema.field(c).type, b.column(c)
            if is_str(t):
                nbytes = out_rows * lmax_of(arr) if side == "build" else (bytes_of(arr) * (out_rows // rows) if rows else 0)
                total += up64(4 * (out_rows + 1)) + up64((out_rows + 7) // 8) + up64(nbytes)
            else:
                total += up64(width_of(t) * out_rows) + up64((out_rows + 7) // 8)
    return total


def in_bytes(rb):
    """the staged probe batch"""
    rows = rb.num_rows
    total = 0
    for c in range(rb.num_columns):
        t, arr = rb.schema.field(c).type, rb.column(c)
        total += up64(4 * (rows + 1)) + up64(bytes_of(arr)) if is_str(t) else up64(width_of(t) * rows)
        if arr.null_count:
            total += up64((rows + 7) // 8 + 8)
    return total


def eligible(lb, rb, lkey, rkey, jt, m, general, utf8=True):
    """the header's rule for one probe batch (one INPUT_REF key, no join filter: by construction).  `general`, `utf8`: the two
    switches; utf8 = False is today's rule, which refuses every batch with a Utf8 column on either side"""
    rows = rb.num_rows
    if rows > SA_MAX_ROWS or rb.column(rkey).null_count or lb.num_columns + rb.num_columns > SA_MAX_COLS:
        return False
    if not width_of(rb.schema.field(rkey).type) or rb.schema.field(rkey).type != lb.schema.field(lkey).type:
        return False  # (a Utf8 key)
    for f in list(lb.schema) + list(rb.schema):
        if not (width_of(f.type) or (utf8 and is_str(f.type))):
            return False  # (Boolean; Utf8 with the switch off)
    inner_unique = jt == "inner" and m == 1
    if not inner_unique and not general:
        return False
    out_rows = rows if inner_unique else rows * m
    return out_rows <= SA_MAX_OUT_ROWS and out_bytes(lb, rb, out_rows) <= SA_AREA and in_bytes(rb) <= SA_AREA


def count_eligible(case, jt, general, utf8=True):
    m = max_run(case.lb, case.lkey)
    return sum(1 for b in case.rbs if eligible(case.lb, b, case.lkey, case.rkey, jt, m, general, utf8))


# ---- strings ----------------------------------------------------------------------------------------------------------
PIECES = ["", "a", "bc", "xyz", "é", "漢", "\U0001f642", "Zoë"]  # (1- to 4-byte code points)


def rand_strings(rng, n, max_pieces=4):
    """n strings of 0-16 bytes: empty ones, ASCII, multi-byte UTF-8"""
    counts = rng.integers(0, max_pieces + 1, n)
    picks = rng.integers(0, len(PIECES), (n, max_pieces))
    return ["".join(PIECES[picks[i, q]] for q in range(counts[i])) for i in range(n)]


def str_array(values, null_mask=None, shift=0):
    """a Utf8 array over `values`; rows of `null_mask` are NULL WITH their bytes left underneath (non-zero length in a NULL
    slot); shift > 0: the offsets start at `shift`, not 0, as those of a slice do (arr.offset stays 0: the ABI sees them as they are)"""
    arr = pa.array(values, type=pa.string())
    n = len(arr)
    if (null_mask is None or not null_mask.any()) and not shift:
        return arr
    offs = np.frombuffer(arr.buffers()[1], dtype=np.int32)[:n + 1] if n else np.zeros(1, dtype=np.int32)
    data = arr.buffers()[2].to_pybytes() if arr.buffers()[2] is not None else b""
    offs = (offs + shift).astype(np.int32)
    data = b"#" * shift + data
    validity, nulls = None, 0
    if null_mask is not None and null_mask.any():
        validity = pa.py_buffer(np.packbits(~null_mask, bitorder="little").tobytes())
        nulls = int(null_mask.sum())
    return pa.StringArray.from_buffers(n, pa.py_buffer(offs.tobytes()), pa.py_buffer(data), validity, nulls)


# ---- cases ------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, lb, rbs, lkey, rkey, runs):
        """runs: the (join type, async_general) pairs under which 0 < eligible batches < len(rbs)"""
        self.name, self.lb, self.rbs, self.lkey, self.rkey, self.runs = name, lb, rbs, lkey, rkey, runs
        self.cond = JoinCondition([(InputRef(lkey), InputRef(rkey))])

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


SIZES = [1024, 1024, 1024, 0, 1, 63, 64, 65, 1023, 1025, 2048, 4096, 5000]


@_cached
def form_case(form):
    """build (k, s1, x, s2) — two Utf8 columns next to a NULL-bearing float64 one, the longest string in the LAST row, NULL
    slots with bytes underneath; probe (t1, k, v, t2) — t2 with offsets that do not start at 0; every size of the issue's list,
    the 4096-row batch hitting with every row (kept whole), a 5000-row batch and one with NULL probe keys (synchronous)"""
    rng = np.random.default_rng(31 + FORMS.index(form))
    conv = (lambda x: x.astype(np.int64) * 7919 - 5) if form.endswith("sparse") else (lambda x: x.astype(np.int64))
    if form.startswith("unique"):
        nb = 2000
        raw = rng.permutation(3000)[:nb]  # (keys >= 2500 are never probed: unvisited build rows)
    else:
        raw = np.repeat(np.arange(700), 4)  # M = 4 exactly
        rng.shuffle(raw)
        nb = len(raw)
    s1 = rand_strings(rng, nb)
    s1[-1] = "L" * 18 + "éé"  # 22 bytes: Lmax sits in the last row
    s2 = rand_strings(rng, nb, 2)
    lb = pa.RecordBatch.from_arrays(
        [pa.array(conv(raw)), str_array(s1, rng.random(nb) < 0.1), pa.array(rng.random(nb), mask=rng.random(nb) < 0.1), str_array(s2, rng.random(nb) < 0.5)],
        names=["k", "s1", "x", "s2"])

    def probe(rows, keys, key_nulls=None):
        return pa.RecordBatch.from_arrays(
            [str_array(rand_strings(rng, rows), rng.random(rows) < 0.2), pa.array(conv(keys), mask=key_nulls),
             pa.array(rng.integers(-9, 9, rows).astype(np.int32), mask=rng.random(rows) < 0.2), str_array(rand_strings(rng, rows, 2), None, shift=5)],
            names=["t1", "k", "v", "t2"])
    rbs = []
    for rows in SIZES:
        keys = rng.choice(raw[raw < 2500], rows) if rows == 4096 else rng.integers(0, 2500, rows)
        rbs.append(probe(rows, keys))
    rbs.insert(3, probe(1024, rng.integers(0, 2500, 1024), rng.random(1024) < 0.1))
    unique = form.startswith("unique")
    runs = [(jt, g) for jt in JOIN_TYPES for g in (False, True) if g or (unique and jt == "inner")]
    return Case(form, lb, rbs, 0, 1, runs)


@_cached
def chunk_case():
    """every build key four times, every probe row hits: 256 / 512 rows emit exactly 1024 / 2048 rows (whole chunks: the end
    offset), 700 rows 2800 (the running base across three chunks); a 5000-row batch keeps the case mixed"""
    rng = np.random.default_rng(41)
    raw = np.repeat(np.arange(500, dtype=np.int64), 4)
    rng.shuffle(raw)
    nb = len(raw)
    lb = pa.RecordBatch.from_arrays([pa.array(raw), str_array(rand_strings(rng, nb), rng.random(nb) < 0.1), str_array([""] * nb)],
                                    names=["k", "s", "e"])  # (e: only empty strings, Lmax = 0)
    rbs = [pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 500, rows)), str_array(rand_strings(rng, rows), rng.random(rows) < 0.2, shift=3)],
                                      names=["k", "t"]) for rows in (256, 512, 700, 5000)]
    return Case("chunks", lb, rbs, 0, 0, [(jt, True) for jt in JOIN_TYPES])


@_cached
def empty_strings_case():
    """Inner / unique route: a build column of only empty strings (Lmax = 0), one of only NULLs, probe columns likewise"""
    rng = np.random.default_rng(43)
    nb = 300
    lb = pa.RecordBatch.from_arrays([pa.array(rng.permutation(400)[:nb].astype(np.int32)), str_array([""] * nb), pa.array([None] * nb, type=pa.string())],
                                    names=["k", "e", "n"])
    rbs = [pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 400, rows).astype(np.int32)), str_array([""] * rows), pa.array([None] * rows, type=pa.string())],
                                      names=["k", "e", "n"]) for rows in (0, 1, 65, 1024, 4097)]
    return Case("empty_strings", lb, rbs, 0, 0, [(jt, g) for jt in JOIN_TYPES for g in (False, True) if g or jt == "inner"])


@_cached
def bound_case():
    """a build column with a 200-byte string: 4096 probe rows would need 4096 x 200 bytes for it alone (synchronous); the
    largest batch the rule admits, and the batch one row larger"""
    rng = np.random.default_rng(47)
    nb = 1000
    s = rand_strings(rng, nb)
    s[17] = "漢" * 66 + "ab"  # 200 bytes
    lb = pa.RecordBatch.from_arrays([pa.array(np.arange(nb, dtype=np.int64)), str_array(s)], names=["k", "s"])

    def probe(rows):
        return pa.RecordBatch.from_arrays([pa.array(rng.integers(0, nb + 100, rows))], names=["k"])
    one = probe(1)
    fits = [r for r in range(1, SA_MAX_ROWS + 1) if eligible(lb, pa.RecordBatch.from_arrays([pa.array(np.zeros(r, dtype=np.int64))], names=["k"]), 0, 0, "inner", 1, False)]
    assert one.num_rows == 1 and fits and fits == list(range(1, fits[-1] + 1))  # (the bound is monotonic in the rows)
    r_ok = fits[-1]
    keys_hit17 = np.full(r_ok, 17, dtype=np.int64)  # every row gathers the 200-byte string: the reservation is used to the last byte
    rbs = [probe(4096), pa.RecordBatch.from_arrays([pa.array(keys_hit17)], names=["k"]), probe(r_ok + 1), probe(r_ok)]
    return Case("bound", lb, rbs, 0, 0, [(jt, g) for jt in JOIN_TYPES for g in (False, True) if g or jt == "inner"])


@_cached
def adjacent_case():
    """Inner / unique route: two ADJACENT Utf8 columns without a NULL on the build side, and two on the probe side, at 65 and
    1025 rows — the one shape in which sa_probe_kernel<true> goes from one Utf8 column's byte copy to the next column's lengths
    through the bare `else __syncthreads()` and not through the barriers of a bitmap pass.  It pins that route's RESULT, for build
    rows and for probe rows; it cannot tell whether that barrier is there (a thread's first stores into the lengths go to the
    entries it read itself, the scan's come behind the next column's first barrier); a 5000-row batch is synchronous"""
    rng = np.random.default_rng(53)
    nb = 1500
    lb = pa.RecordBatch.from_arrays([pa.array(rng.permutation(2000)[:nb].astype(np.int64)), str_array(rand_strings(rng, nb)), str_array(rand_strings(rng, nb, 2))],
                                    names=["k", "s1", "s2"])
    rbs = [pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 2000, rows)), str_array(rand_strings(rng, rows)), str_array(rand_strings(rng, rows, 2), None, shift=3)],
                                      names=["k", "t1", "t2"]) for rows in (65, 1025, 5000)]
    return Case("adjacent_utf8", lb, rbs, 0, 0, [("inner", False)])


def all_cases():
    return [form_case(f) for f in FORMS] + [chunk_case(), empty_strings_case(), bound_case(), adjacent_case()]


# ---- the fuzz ---------------------------------------------------------------------------------------------------------
FUZZ_SEEDS = list(range(10))


@_cached
def fuzz_case(seed):
    """random join type, 1-4 columns per side from {i64, f64, i32, str} with NULL rates 0 / 5 / 50 / 100 %, duplicate rate (none,
    x2, one hot key), sizes from the list above; -> (case, join type, async_general, depth)"""
    rng = np.random.default_rng(9100 + seed)
    jt = JOIN_TYPES[seed % 4]
    general = seed != 0  # (seed 0: Inner over unique keys with only this switch on — sa_probe_kernel's own route)
    nb = int(rng.choice([50, 1000, 3000]))
    dupl = ["none", "x2", "hot"][seed % 3]
    if dupl == "none":
        raw = rng.permutation(3 * nb)[:nb]
    elif dupl == "x2":
        raw = rng.integers(0, max(nb // 2, 1), nb)
    else:
        raw = rng.permutation(3 * nb)[:nb]
        raw[rng.choice(nb, 5, replace=False)] = raw[0]
    mul = int(rng.choice([1, 7919]))

    def col(kind, rows, p):
        mask = rng.random(rows) < p if p else None
        if kind == "str":
            return str_array(rand_strings(rng, rows), mask, shift=int(rng.integers(0, 2)) * 7)
        vals = {"i64": lambda: rng.integers(-20, 20, rows), "f64": lambda: np.round(rng.random(rows), 2),
                "i32": lambda: rng.integers(-20, 20, rows).astype(np.int32)}[kind]()
        return pa.array(vals, mask=mask)

    def spec():
        return [(str(rng.choice(["i64", "f64", "i32", "str"])), float(rng.choice([0.0, 0.05, 0.5, 1.0]))) for _ in range(int(rng.integers(1, 5)))]
    lspec, rspec = spec(), spec()
    lb = pa.RecordBatch.from_arrays([col(k, nb, p) for k, p in lspec] + [pa.array((raw * mul).astype(np.int64))],
                                    names=[f"l{i}" for i in range(len(lspec))] + ["k"])
    sizes = [int(x) for x in rng.choice([0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 4096, 5000], size=10)]
    rbs = [pa.RecordBatch.from_arrays([pa.array((rng.integers(0, 3 * nb, n) * mul).astype(np.int64))] + [col(k, n, p) for k, p in rspec],
                                      names=["k"] + [f"r{i}" for i in range(len(rspec))]) for n in sizes]
    return Case(f"fuzz{seed}", lb, rbs, len(lspec), 0, []), jt, general, int(rng.integers(1, 7))
