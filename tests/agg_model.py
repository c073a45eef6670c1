"""An independent model of GROUP BY aggregation over edge values: numpy and Python integers, no oracle, no library.

`aggregate(keys, key_valid, args, funcs, batches=None)` restates what HashAgg computes (hash_agg.rs:32-150 with
count.rs / sum.rs / min_max.rs per accumulator) for ONE int64 key column:

* groups come out in first-seen order; NULL keys form one group;
* COUNT          the number of valid argument values;
* SUM int64      the exact integer sum reduced mod 2^64 and read as signed — the wrapping of the library's cells and of
                 sum.rs's `+`; an int32 argument is widened first (SUM -> INT64 does not wrap at 32 bits);
* MIN/MAX int    exact;
* MIN/MAX f64    IEEE total order ON THE BIT PATTERN: -0.0 < +0.0, negative NaNs below -Inf, positive NaNs above +Inf,
                 payloads order (device_utils.hpp f64_to_ordered, the oracle's cmp_f64).  The result is a bit pattern and
                 is compared as one;
* SUM f64        a CLASSED expectation.  m = valid values of the group, exact = math.fsum of them, S = fsum of |x|:
    NAN     a NaN among the values, or +Inf and -Inf together: compared as "is a NaN" (sign and payload are the adder's);
    INF     compared exactly (bit pattern);
    ZERO    every value is +-0: compared as "is a zero" — THE SIGN IS NOT COMPARED.  For a group that mixes -0.0 and
            +0.0 the order of the additions decides it, and for an all -0.0 group the oracle starts from the first value
            (-0.0) while an accumulator cell that starts at +0.0 ends at +0.0; the arrow kernel the reference calls
            (arrow::compute::sum) is not available to settle which of the two the reference returns;
    ONE     m == 1, finite and not a zero: compared exactly (0.0 + x == x bit for bit);
    FINITE  |got - exact| <= gamma * S with gamma = k u / (1 - k u), u = 2^-53, k = m + 1: the standard bound for a sum
            of m terms in ANY order or tree (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), so no
            tolerance is measured; the + 1 is the one extra rounding of the multiplicity product `cell * m` of the fused
            join over duplicate build keys;
* validity       SUM / MIN / MAX are NULL exactly when COUNT of that argument is 0.

`batches` [(lo, hi), ...] gives the order in which row ranges arrive (first-seen order follows it); the values of a group
do not depend on it.

`compare(got_table, groups)` compares by bit pattern apart from the classes above and returns how many SUM(f64) groups
were compared by class (NAN / INF / ZERO) instead of by value."""
import math
from dataclasses import dataclass, field

import numpy as np

U = 2.0 ** -53
SIGN = np.uint64(1 << 63)
EXACT, NAN, INF, ZERO, ONE, FINITE, NULL = range(7)   # how a cell is compared
CLASS_NAMES = ["EXACT", "NAN", "INF", "ZERO", "ONE", "FINITE", "NULL"]
BY_CLASS = (NAN, INF, ZERO)


def f64_bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def bits_f64(b) -> np.ndarray:
    return np.ascontiguousarray(b, dtype=np.uint64).view(np.float64)


def total_order(bits: np.ndarray) -> np.ndarray:
    """the unsigned image under which IEEE total order is integer order: negative values reversed below the positives"""
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    return np.where(bits & SIGN != 0, ~bits, bits | SIGN)


def total_order_back(img: np.ndarray) -> np.ndarray:
    img = np.ascontiguousarray(img, dtype=np.uint64)
    return np.where(img & SIGN != 0, img & ~SIGN, ~img)


@dataclass
class Column:
    """the expectation of one aggregate, one entry per group"""
    func: str
    kind: str                 # "i64" / "i32" / "f64": the type of the RESULT column
    valid: np.ndarray         # bool
    bits: np.ndarray          # uint64: expected bit pattern (SUM f64 FINITE: fsum's; int32 results sign-extended)
    how: np.ndarray           # EXACT / NAN / INF / ZERO / ONE / FINITE / NULL
    S: np.ndarray = None      # SUM f64: sum of |x|
    m: np.ndarray = None      # valid values


@dataclass
class Groups:
    keys: np.ndarray          # int64, first-seen order
    key_valid: np.ndarray     # bool
    cols: list = field(default_factory=list)

    def __len__(self):
        return len(self.keys)


def _group_ids(keys, key_valid, order):
    """(gid per row, group keys, group key validity) with groups numbered in first-seen order along `order`"""
    n = len(keys)
    kv = np.ones(n, bool) if key_valid is None else np.asarray(key_valid, bool)
    ko, vo = np.asarray(keys, np.int64)[order], kv[order]
    pos = np.nonzero(vo)[0]
    uniq, first, inv = np.unique(ko[pos], return_index=True, return_inverse=True)
    first_pos = pos[first]
    nulls = np.nonzero(~vo)[0]
    if len(nulls):  # NULL keys are ONE group whatever their slot holds
        uniq, first_pos = np.append(uniq, 0), np.append(first_pos, nulls[0])
    by_first = np.argsort(first_pos, kind="stable")
    rank = np.empty(len(first_pos), np.int64)
    rank[by_first] = np.arange(len(first_pos))
    go = np.empty(n, np.int64)
    go[pos] = rank[np.asarray(inv).reshape(-1)]
    if len(nulls):
        go[nulls] = rank[-1]
    gid = np.empty(n, np.int64)
    gid[order] = go
    gvalid = np.ones(len(uniq), bool)
    if len(nulls):
        gvalid[-1] = False
    return gid, uniq[by_first].astype(np.int64), gvalid[by_first]


def _segments(gid, valid, G):
    """rows of every group's VALID values, contiguous: (row permutation, start per group, count per group)"""
    rows = np.nonzero(valid)[0]
    rows = rows[np.argsort(gid[rows], kind="stable")]
    m = np.bincount(gid[rows], minlength=G).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(m)[:-1]]).astype(np.int64) if G else np.zeros(0, np.int64)
    return rows, start, m


def _reduce(ufunc, vals, start, m, empty):
    """ufunc.reduceat over the non-empty segments; `empty` where a group has no valid value"""
    out = np.full(len(m), empty, dtype=vals.dtype)
    ne = m > 0
    if ne.any():
        out[ne] = ufunc.reduceat(vals, start[ne])
    return out


def _sum_f64(x, start, m, classes_only=False):
    G = len(m)
    how = np.full(G, NULL, np.int64)
    bits = np.zeros(G, np.uint64)
    S = np.zeros(G, np.float64)
    xb = f64_bits(x)
    isnan, ispinf, isninf, iszero = np.isnan(x), x == np.inf, x == -np.inf, x == 0.0
    any_ = lambda f: _reduce(np.logical_or, f, start, m, False)  # noqa: E731
    all_ = lambda f: _reduce(np.logical_and, f, start, m, False)  # noqa: E731
    g_nan, g_pinf, g_ninf, g_zero = any_(isnan), any_(ispinf), any_(isninf), all_(iszero)
    has = m > 0
    nan = has & (g_nan | (g_pinf & g_ninf))
    inf = has & ~nan & (g_pinf | g_ninf)
    zero = has & ~nan & ~inf & g_zero
    one = has & ~nan & ~inf & ~zero & (m == 1)
    fin = has & ~nan & ~inf & ~zero & ~one
    how[nan], how[inf], how[zero], how[one], how[fin] = NAN, INF, ZERO, ONE, FINITE
    bits[inf] = np.where(g_pinf[inf], f64_bits([np.inf])[0], f64_bits([-np.inf])[0])
    bits[one] = xb[start[one]]
    if classes_only:
        return how, bits, S
    xl, axl = x.tolist(), np.abs(x).tolist()  # (Python floats once: fsum over array slices boxes every element)
    fs = np.zeros(G, np.float64)
    for g, lo, hi in zip(np.nonzero(fin)[0].tolist(), start[fin].tolist(), (start[fin] + m[fin]).tolist()):
        fs[g], S[g] = math.fsum(xl[lo:hi]), math.fsum(axl[lo:hi])
    bits[fin] = f64_bits(fs)[fin]
    return how, bits, S


def aggregate(keys, key_valid, args, funcs, batches=None, cache=None, classes_only=False) -> Groups:
    """keys int64[n]; key_valid bool[n] or None; args [(values, valid or None)] with int64 / int32 / float64 values;
    funcs [(name, argument index)] with name in count / sum / min / max; batches [(lo, hi)] in arrival order.
    `classes_only`: SUM(f64) columns carry their classes but no fsum / S (for counting classes: not to be compared with).
    `cache`: a dict of the caller's that keeps the groups and the columns of ONE input between calls with other `funcs`"""
    n = len(keys)
    cache = {} if cache is None else cache
    if "groups" not in cache:
        order = np.arange(n) if batches is None else np.concatenate([np.arange(lo, hi) for lo, hi in batches] + [np.zeros(0, np.int64)]).astype(np.int64)
        assert len(order) == n and (n == 0 or len(np.unique(order)) == n), "batches must cover every row once"
        cache["groups"] = _group_ids(keys, key_valid, order) if n else (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, bool))
    gid, gk, gv = cache["groups"]
    G = len(gk)
    out = Groups(gk, gv)
    for name, ai in funcs:
        key = (name, ai, classes_only) if name == "sum" else (name, ai)
        if key not in cache:
            cache[key] = _column(name, args[ai], gid, G, n, cache, classes_only)
        out.cols.append(cache[key])
    return out


def _column(name, arg, gid, G, n, cache, classes_only=False) -> Column:
    vals, valid = arg
    vals = np.asarray(vals)
    kind = {"int64": "i64", "int32": "i32", "float64": "f64"}[vals.dtype.name]
    seg = ("segments", None if valid is None else id(valid))  # (columns with one validity array share their segments)
    if seg not in cache:
        cache[seg] = _segments(gid, np.ones(n, bool) if valid is None else np.asarray(valid, bool), G)
    rows, start, m = cache[seg]
    v = vals[rows]
    has = m > 0
    if name == "count":
        col = Column(name, "i64", np.ones(G, bool), m.astype(np.int64).view(np.uint64), np.full(G, EXACT))
    elif name == "sum" and kind != "f64":
        s = _reduce(np.add, v.astype(np.int64).view(np.uint64), start, m, np.uint64(0))  # (uint64 addition wraps mod 2^64)
        col = Column(name, "i64", has, s, np.where(has, EXACT, NULL))
    elif name == "sum":
        how, bits, S = _sum_f64(v, start, m, classes_only)
        col = Column(name, "f64", has, bits, how, S, m)
    elif name in ("min", "max") and kind != "f64":
        r = _reduce(np.minimum if name == "min" else np.maximum, v.astype(np.int64), start, m, np.int64(0))
        col = Column(name, kind, has, r.view(np.uint64), np.where(has, EXACT, NULL))
    elif name in ("min", "max"):
        img = _reduce(np.minimum if name == "min" else np.maximum, total_order(f64_bits(v)), start, m, np.uint64(0))
        col = Column(name, "f64", has, total_order_back(img), np.where(has, EXACT, NULL))
    else:
        raise ValueError(name)
    col.m = m
    return col


def wrap_i64(x: int) -> int:
    """a Python integer reduced mod 2^64 and read as signed"""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def aggregate_slow(keys, key_valid, args, funcs, batches=None):
    """the same definitions once more, row by row with Python integers and dicts (small inputs): what `aggregate`'s numpy
    is checked against.  Returns [(key or None, [cell or None, ...])] with SUM f64 cells as (how, bits, S, m)."""
    n = len(keys)
    order = range(n) if batches is None else [r for lo, hi in batches for r in range(lo, hi)]
    groups = {}
    for r in order:
        k = None if (key_valid is not None and not key_valid[r]) else int(keys[r])
        st = groups.setdefault(k, [[] for _ in args])
        for ai, (vals, valid) in enumerate(args):
            if valid is None or valid[r]:
                st[ai].append(vals[r])
    out = []
    for k, st in groups.items():
        cells = []
        for name, ai in funcs:
            xs = st[ai]
            isf = np.asarray(args[ai][0]).dtype == np.float64
            if name == "count":
                cells.append(len(xs))
            elif not xs:
                cells.append(None)
            elif name == "sum" and not isf:
                cells.append(wrap_i64(sum(int(x) for x in xs)))
            elif name == "sum":
                fx = [float(x) for x in xs]
                if any(math.isnan(x) for x in fx) or (math.inf in fx and -math.inf in fx):
                    cells.append((NAN, 0, 0.0, len(fx)))
                elif math.inf in fx or -math.inf in fx:
                    cells.append((INF, int(f64_bits([math.inf if math.inf in fx else -math.inf])[0]), 0.0, len(fx)))
                elif all(x == 0.0 for x in fx):
                    cells.append((ZERO, 0, 0.0, len(fx)))
                elif len(fx) == 1:
                    cells.append((ONE, int(f64_bits(fx)[0]), 0.0, 1))
                else:
                    cells.append((FINITE, int(f64_bits([math.fsum(fx)])[0]), math.fsum(abs(x) for x in fx), len(fx)))
            elif not isf:
                cells.append(int(min(xs) if name == "min" else max(xs)))
            else:
                def key_of(x):
                    b = int(f64_bits([x])[0])
                    return (~b) & ((1 << 64) - 1) if b >> 63 else b | (1 << 63)
                w = min(xs, key=key_of) if name == "min" else max(xs, key=key_of)
                cells.append(int(f64_bits([w])[0]))
        out.append((k, cells))
    return out


def gamma(k):
    """k u / (1 - k u)"""
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


def column_bits(arr, kind):
    """(valid bool[G], bits uint64[G]) of a pyarrow array / chunked array; int32 sign-extended"""
    import pyarrow as pa
    if isinstance(arr, pa.ChunkedArray):
        arr = arr.combine_chunks()
    valid = np.asarray(arr.is_valid())
    exp_type = {"i64": pa.int64(), "i32": pa.int32(), "f64": pa.float64()}[kind]
    assert arr.type == exp_type, (arr.type, exp_type)
    # the values buffer as it is: a NaN's payload and sign must not pass through a float conversion
    buf = arr.buffers()[1]
    npdt = {"i64": np.int64, "i32": np.int32, "f64": np.uint64}[kind]
    if len(arr) == 0:
        return valid, np.zeros(0, np.uint64)
    raw = np.frombuffer(buf, dtype=npdt, count=arr.offset + len(arr))[arr.offset:]
    bits = raw if kind == "f64" else raw.astype(np.int64).view(np.uint64)
    return valid, np.array(bits, dtype=np.uint64)


def compare(got_table, groups: Groups, label="") -> int:
    """got_table: pyarrow Table / RecordBatch [key, one column per aggregate] (None = no rows).  Asserts the number and order
    of the groups, every key, every validity and every value (by bit pattern apart from the SUM f64 classes); returns the
    number of SUM(f64) groups compared by class (NAN / INF / ZERO) instead of by value."""
    G = len(groups)
    if got_table is None:
        assert G == 0, f"{label}: no output, {G} groups expected"
        return 0
    assert got_table.num_rows == G, f"{label}: {got_table.num_rows} groups, expected {G}"
    assert got_table.num_columns == 1 + len(groups.cols), f"{label}: {got_table.num_columns} columns"
    kvalid, kbits = column_bits(got_table.column(0), "i64")
    bad = np.nonzero((kvalid != groups.key_valid) | (kvalid & (kbits.view(np.int64) != groups.keys)))[0]
    assert len(bad) == 0, (f"{label}: group {bad[0]} of {G}: key {kbits.view(np.int64)[bad[0]] if kvalid[bad[0]] else None}, expected "
                           f"{groups.keys[bad[0]] if groups.key_valid[bad[0]] else None} ({len(bad)} groups differ: order or key)")
    by_class = 0
    for c, col in enumerate(groups.cols):
        what = f"{label}: column {c + 1} {col.func}({col.kind})"
        valid, bits = column_bits(got_table.column(c + 1), col.kind)
        bad = np.nonzero(valid != col.valid)[0]
        assert len(bad) == 0, f"{what}: group {bad[0]} key {groups.keys[bad[0]]}: valid {valid[bad[0]]}, expected {col.valid[bad[0]]} (m = {col.m[bad[0]]})"
        how = col.how
        exact = (how == EXACT) | (how == INF) | (how == ONE)
        bad = np.nonzero(exact & (bits != col.bits))[0]
        assert len(bad) == 0, (f"{what}: group {bad[0]} key {groups.keys[bad[0]]} ({CLASS_NAMES[how[bad[0]]]}, m = {col.m[bad[0]]}): "
                               f"{bits[bad[0]]:#018x}, expected {col.bits[bad[0]]:#018x} ({len(bad)} groups differ)")
        if col.func == "sum" and col.kind == "f64":
            got = bits_f64(bits)
            bad = np.nonzero((how == NAN) & ~np.isnan(got))[0]
            assert len(bad) == 0, f"{what}: group {bad[0]} key {groups.keys[bad[0]]}: {got[bad[0]]!r}, expected a NaN"
            bad = np.nonzero((how == ZERO) & (got != 0.0))[0]
            assert len(bad) == 0, f"{what}: group {bad[0]} key {groups.keys[bad[0]]}: {got[bad[0]]!r}, expected a zero"
            fin = how == FINITE
            with np.errstate(invalid="ignore", over="ignore"):
                # (long double: the difference of two doubles and the product gamma * S carry no rounding of their own that matters)
                err = np.abs(got.astype(np.longdouble) - bits_f64(col.bits).astype(np.longdouble))
                bound = gamma(col.m + 1).astype(np.longdouble) * col.S.astype(np.longdouble)
                bad = np.nonzero(fin & ~(err <= bound))[0]
            assert len(bad) == 0, (f"{what}: group {bad[0]} key {groups.keys[bad[0]]} (m = {col.m[bad[0]]}): {got[bad[0]]!r}, fsum "
                                   f"{bits_f64(col.bits)[bad[0]]!r}, |diff| {float(err[bad[0]])!r} > gamma S = {float(bound[bad[0]])!r} ({len(bad)} groups differ)")
            by_class += int(np.isin(how, BY_CLASS).sum())
    return by_class


def class_share(groups: Groups):
    """per SUM(f64) column: (groups compared by class, groups with a value)"""
    out = []
    for col in groups.cols:
        if col.func == "sum" and col.kind == "f64":
            out.append((int(np.isin(col.how, BY_CLASS).sum()), int((col.how != NULL).sum())))
    return out


def to_table(groups: Groups):
    """the expectation as a pyarrow Table (FINITE cells: fsum; NAN cells: the default NaN; ZERO cells: +0.0) — what the planted
    faults of the CPU tests are applied to"""
    import pyarrow as pa
    cols = [pa.array(groups.keys, type=pa.int64(), mask=~groups.key_valid)]
    for col in groups.cols:
        bits = col.bits.copy()
        if col.kind == "f64":
            bits[col.how == NAN] = f64_bits([np.nan])[0]
            v, t = bits_f64(bits), pa.float64()
        elif col.kind == "i32":
            v, t = bits.view(np.int64).astype(np.int32), pa.int32()
        else:
            v, t = bits.view(np.int64), pa.int64()
        cols.append(pa.array(v, type=t, mask=~col.valid))
    return pa.table(cols, names=[f"c{i}" for i in range(len(cols))])
