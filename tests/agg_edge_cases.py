"""Seeded edge-value inputs of the aggregate tests, shared by test_agg_model_cpu.py (model against oracle, the conditions,
the planted faults) and test_gpu_agg_edges.py (every device route against the model).

A case is ONE int64 key column and four argument columns:

  f  float64  the column SUM(f64) is asserted on: ordinary values of magnitude 1e-3 .. 1e4, -0.0 / +0.0 / +-subnormal /
              +-DBL_MIN sprinkled in, 1e16, 1.0, -1e16 triples (cancellation) in three groups, and — as far as a tenth of
              the case's groups allows — groups made of ONE repeated value of F64_POOL (all-NaN, all -0.0, all +Inf ...)
              and groups of ordinary values with one NaN / Inf in them.  Finite magnitudes stay below 1e17, so no partial
              sum overflows in any order (S <= 1e300 in every group by a wide margin)
  g  float64  a second float column without NaN / Inf (two-argument forms)
  i  int64    values near +-2^62 (three rows wrap), INT64_MIN / INT64_MAX / -1 / 0 sprinkled in and as whole groups
  j  int32    the full int32 range, INT32_MIN / INT32_MAX sprinkled in and as whole groups

Group shapes: groups of one row, groups whose arguments are all NULL, groups of one repeated edge value, a hot group of
>= half the rows (optionally made of the value whose ordered image is the MIN or the MAX accumulator's neutral start), keys
arriving sorted, NULL keys, validity that flips every 64 rows, and batches in which the NULLs arrive late.

Two CONDITIONS hold for the cases and are asserted on the CPU (test_agg_model_cpu.py), never measured on the device:
  1. at most a tenth of a case's SUM(f64) groups are compared by class (NAN / INF / ZERO) instead of by value;
  2. every value of the pools is the MIN, the MAX and a SUM operand of some group of some GPU case."""
import functools

import numpy as np
import pyarrow as pa

import agg_model as M
from sqlrs_amd import abi
from sqlrs_amd.expr import AggFunc, InputRef

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
# NaNs of both signs with payload 1 (signalling), 2^51 (the quiet bit) and all ones: 0x7FFF...F and 0xFFFF...F are the
# values whose ordered images are ~0 and 0, the neutral starts of the MIN and the MAX accumulator
F64_NAN = [0x7FF0000000000001, 0x7FF8000000000000, 0x7FFFFFFFFFFFFFFF, 0xFFF0000000000001, 0xFFF8000000000000, 0xFFFFFFFFFFFFFFFF]
F64_INF = [0x7FF0000000000000, 0xFFF0000000000000]
F64_ZERO = [0x0000000000000000, 0x8000000000000000]
F64_TINY = [0x0000000000000001, 0x8000000000000001, 0x0010000000000000, 0x8010000000000000]  # +-smallest subnormal, +-DBL_MIN
F64_POOL = F64_NAN + F64_INF + F64_ZERO + F64_TINY
F64_CLASSED = F64_NAN + F64_INF + F64_ZERO  # a group made of one of these is compared by class
I64_POOL = [INT64_MIN, INT64_MAX, -1, 0]    # ordered images 0 (MAX neutral) and ~0 (MIN neutral); -1 = ~0 as a raw cell
I32_POOL = [INT32_MIN, INT32_MAX]
COLS = ("f", "g", "i", "j")
DTYPE = {"f": abi.FLOAT64, "g": abi.FLOAT64, "i": abi.INT64, "j": abi.INT32}
ALL_NULL_GROUPS, CANCEL_GROUPS = 3, 3
N_PART = (1 << 21) + 77  # the partition route's size in the GPU tests: above its 2^21 threshold, no multiple of any tile


class Case:
    """keys / columns in ARRIVAL order; `bounds` cuts them into batches"""

    def __init__(self, name, keys, key_valid, cols, bounds, arrival=None):
        self.name, self.keys, self.key_valid, self.cols, self.bounds = name, keys, key_valid, cols, bounds
        self.arrival = arrival  # order of the batches (indices into bounds); None = as stored
        self._cache, self._batches = {}, None

    @property
    def n(self):
        return len(self.keys)

    def ranges(self):
        r = [(self.bounds[k], self.bounds[k + 1]) for k in range(len(self.bounds) - 1)]
        return r if self.arrival is None else [r[k] for k in self.arrival]

    def batches(self):
        """[pyarrow.RecordBatch] with columns k, f, g, i, j in arrival order"""
        if self._batches is None:
            arrays = [pa.array(self.keys, type=pa.int64(), mask=None if self.key_valid is None else ~self.key_valid)]
            for c in COLS:
                v, valid = self.cols[c]
                arrays.append(pa.array(v, mask=None if valid is None else ~valid))
            whole = pa.RecordBatch.from_arrays(arrays, names=["k"] + list(COLS))
            self._batches = [whole.slice(lo, hi - lo) for lo, hi in self.ranges()]
        return self._batches

    def model(self, funcs, classes_only=False) -> M.Groups:
        """funcs [(name, column letter)]; classes_only: agg_model.aggregate"""
        args = [self.cols[c] for c in COLS]
        return M.aggregate(self.keys, self.key_valid, args, [(f, COLS.index(c)) for f, c in funcs],
                           None if self.arrival is None else self.ranges(), cache=self._cache, classes_only=classes_only)


def agg_funcs(funcs, first_col=1, distinct=False):
    """[(name, column letter)] -> [AggFunc] over a batch whose argument columns f, g, i, j start at `first_col`"""
    out = []
    for name, c in funcs:
        rt = abi.INT64 if name == "count" or (name == "sum" and c in "ij") else DTYPE[c]
        out.append(AggFunc(name, InputRef(first_col + COLS.index(c)), rt, distinct=distinct))
    return out


def _f64(bits):
    return np.array(bits, dtype=np.uint64).view(np.float64)


def _ordinary(rng, n):
    f = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 5, n)
    g = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 5, n)
    for col in (f, g):
        at = np.nonzero(rng.random(n) < 0.004)[0]  # (rare: a group's smallest |x| is mostly an ordinary value, see the dropped-row fault)
        col[at] = _f64(F64_ZERO + F64_TINY)[rng.integers(0, 6, len(at))]
    with np.errstate(over="ignore"):
        i = np.where(rng.random(n) < 0.5, np.int64(1 << 62), np.int64(-(1 << 62))) + rng.integers(-1000, 1000, n)
    at = np.nonzero(rng.random(n) < 0.01)[0]
    i[at] = np.array(I64_POOL, np.int64)[rng.integers(0, 4, len(at))]
    j = rng.integers(INT32_MIN, INT32_MAX + 1, n).astype(np.int32)
    at = np.nonzero(rng.random(n) < 0.01)[0]
    j[at] = np.array(I32_POOL, np.int32)[rng.integers(0, 2, len(at))]
    return f, g, i, j


def build(name, n, seed, groups, keyspace="dense", hot=0.0, hot_pure=None, sorted_keys=False, null_keys=0.0, nullable=None,
          batches=1, late_nulls=False, reverse=False, sampled_groups=0, special_rows=2) -> Case:
    """keyspace  dense: `groups` consecutive keys from -777 (dense_gaps: every second one); sparse: spread over 2^40 values; full64: over all of int64,
                 with -1, INT64_MIN and INT64_MAX among the keys
    hot         share of the rows in ONE group; hot_pure "min_neutral" / "max_neutral": that group holds only the value whose
                 ordered image is the MIN / MAX accumulator's start (f: 0x7FFF..F / 0xFFFF..F, i: INT64_MAX / INT64_MIN)
    nullable    None, "random" (15 % per column) or "flip64" (validity flips every 64 rows, out of phase between the columns);
                 either way three groups have only NULL arguments
    special_rows  further rows of every special group (edge-valued, cancelling): with sorted keys, the length of their runs
    sampled_groups  K > 0: the 64-row groups 0 and 4 of every 8 — the rows the key statistics hash at >= 2^22 rows
                 (agg_partition.hip key_stats_kernel, sample_shift 3) — hold only the first K groups, so the estimate is K
    batches     a number (cut at odd places) or a list of batch sizes; late_nulls: the first batch has no NULL at all and the
                 all-NULL groups only arrive after it; reverse: the batches arrive last first"""
    rng = np.random.default_rng(seed)
    G = max(1, min(groups, n))
    # ---- roles of the planned groups (a role is dropped when the case has too few groups for it)
    room = list(range(G))
    take = lambda k: [room.pop(0) for _ in range(min(k, len(room)))]  # noqa: E731
    hot_g = take(1)[0] if hot and G > 1 else None
    allnull = take(ALL_NULL_GROUPS) if nullable and G >= 8 else []
    budget = (G - len(allnull)) // 12 - (1 if hot_pure else 0)  # groups SUM(f) may compare by class: under a tenth, with margin
    classed = [F64_CLASSED[(seed + k) % len(F64_CLASSED)] for k in range(len(F64_CLASSED))][:max(budget, 0)]
    pure_f = dict(zip(take(len(classed)), classed))
    mixed = (F64_NAN + F64_INF)[:max(budget - len(classed), 0)]
    mixed_f = dict(zip(take(len(mixed)), mixed))
    if G >= 8:
        pure_f.update(zip(take(len(F64_TINY)), F64_TINY))
    cancel = take(CANCEL_GROUPS) if G >= 16 else []
    special = list(pure_f) + list(mixed_f) + cancel
    pure_i = dict(zip((special + room)[:4], I64_POOL)) if G >= 8 else {}
    pure_j = dict(zip((special + room)[4:6], I32_POOL)) if G >= 8 else {}
    single = take(min(G // 8, 50))
    # ---- rows: one per planned group, two more for the special ones, the hot rows, the rest at random
    parts = [np.arange(G)]
    if n >= G + special_rows * len(special):
        parts.append(np.repeat(np.array(special, np.int64), special_rows))
    left = n - sum(len(p) for p in parts)
    if hot_g is not None:
        parts.append(np.full(min(left, int(hot * n)), hot_g))
        left = n - sum(len(p) for p in parts)
    fill = np.array(sorted(set(range(G)) - set(single)) or [0])
    parts.append(fill[rng.integers(0, len(fill), left)])
    grp = rng.permutation(np.concatenate(parts).astype(np.int64))
    if sampled_groups:
        seen = np.isin((np.arange(n) >> 6) & 7, (0, 4))
        grp[seen] = rng.integers(0, sampled_groups, int(seen.sum()))
    # ---- batches
    if isinstance(batches, int):
        cuts = sorted(set(int(x) for x in (np.arange(1, batches) * n // batches + 13) if 0 < x < n)) if batches > 1 else []
        bounds = [0] + cuts + [n]
    else:
        assert sum(batches) == n
        bounds = [0] + list(np.cumsum(batches))
    if late_nulls and allnull and len(bounds) > 2:  # the all-NULL groups arrive after the first batch
        head = np.isin(grp[:bounds[1]], allnull)
        grp[:bounds[1]][head] = fill[rng.integers(0, len(fill), int(head.sum()))]
        grp[n - len(allnull):] = allnull
    # ---- keys
    perm = rng.permutation(G).astype(np.int64)
    if keyspace == "dense":
        gkeys = perm - 777
    elif keyspace == "dense_gaps":  # every second value of the range
        gkeys = 2 * perm - 777
    elif keyspace == "sparse":
        gkeys = ((perm + 1) * 0x9E3779B1) % (1 << 40) - (1 << 39)
    else:
        with np.errstate(over="ignore"):
            gkeys = (perm.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)
        if G >= 8:
            gkeys[room[-3:] if len(room) >= 3 else [G - 3, G - 2, G - 1]] = [-1, INT64_MIN, INT64_MAX]
    assert len(np.unique(gkeys)) == G
    if sorted_keys:
        assert len(bounds) == 2
        grp = grp[np.argsort(gkeys[grp], kind="stable")]
    keys = gkeys[grp]
    key_valid = None
    if null_keys:
        key_valid = rng.random(n) >= null_keys
        keys = np.where(key_valid, keys, rng.integers(-5, 5, n))  # (a NULL key's slot holds anything)
        if late_nulls and len(bounds) > 2:
            key_valid[:bounds[1]] = True
            keys[:bounds[1]] = gkeys[grp[:bounds[1]]]
    # ---- values
    f, g, i, j = _ordinary(rng, n)
    for gi, bits in pure_f.items():
        f[grp == gi] = _f64([bits])[0]
    for gi, bits in mixed_f.items():
        f[np.nonzero(grp == gi)[0][0]] = _f64([bits])[0]
    for gi in cancel:
        at = np.nonzero(grp == gi)[0]
        f[at] = np.array([1e16, 1.0, -1e16])[np.arange(len(at)) % 3]
    for gi, v in pure_i.items():
        i[grp == gi] = v
    for gi, v in pure_j.items():
        j[grp == gi] = v
    if hot_pure and hot_g is not None:
        at = grp == hot_g
        mn = hot_pure == "min_neutral"
        f[at], i[at], j[at] = _f64([0x7FFFFFFFFFFFFFFF if mn else 0xFFFFFFFFFFFFFFFF])[0], (INT64_MAX if mn else INT64_MIN), (INT32_MAX if mn else INT32_MIN)
    # ---- validity
    valid = {c: None for c in COLS}
    if nullable:
        row = np.arange(n)
        if nullable == "random":
            valid = {c: rng.random(n) >= 0.15 for c in COLS}
        else:
            valid = {"f": (row >> 6) & 1 == 0, "g": (row >> 7) & 1 == 0, "i": (row >> 6) & 1 == 1, "j": (row >> 6) % 3 != 0}
        dead = np.isin(grp, allnull)
        for c in COLS:
            valid[c] = valid[c] & ~dead
            if late_nulls and len(bounds) > 2:
                valid[c][:bounds[1]] = True
    cols = {"f": (f, valid["f"]), "g": (g, valid["g"]), "i": (i, valid["i"]), "j": (j, valid["j"])}
    arrival = list(range(len(bounds) - 1))[::-1] if reverse else None
    return Case(name, keys, key_valid, cols, [int(b) for b in bounds], arrival)


# ---- the cases of the GPU file (test_gpu_agg_edges.py); the CPU file checks the two conditions on every one of them -------------
ROW_SIZES = [1, 63, 64, 65, 4097, 100_003]
GPU_CASES = {}
for _n in ROW_SIZES:
    _g = max(1, min(_n // 3, 400))
    GPU_CASES[f"row_{_n}"] = dict(n=_n, seed=_n, groups=_g, keyspace="sparse", hot=0.5 if _n >= 4097 else 0.0, null_keys=0.02 if _n > 1 else 0.0,
                                  nullable="flip64" if _n >= 63 else None)
    GPU_CASES[f"row_{_n}_3_batches"] = dict(n=_n, seed=_n + 1, groups=_g, keyspace="full64", nullable="random" if _n > 1 else None, batches=3,
                                            late_nulls=True, hot=0.5 if _n >= 4097 else 0.0, hot_pure="max_neutral" if _n == 4097 else None)
GPU_CASES.update({
    "row_plain_4097": dict(n=4097, seed=5, groups=300, keyspace="dense", hot=0.5, hot_pure="min_neutral"),  # no NULL anywhere: no has-value counts
    "threshold_below": dict(n=(1 << 21) - 1, seed=21, groups=3000, keyspace="dense"),
    "threshold_at": dict(n=1 << 21, seed=22, groups=3000, keyspace="dense"),
    "part_dense": dict(n=N_PART, seed=31, groups=40_000, keyspace="dense"),
    "part_dense_hot": dict(n=N_PART, seed=32, groups=40_000, keyspace="dense", hot=0.55, hot_pure="max_neutral"),
    "part_sparse": dict(n=N_PART, seed=33, groups=50_000, keyspace="sparse"),
    "part_sparse_hot": dict(n=N_PART, seed=34, groups=50_000, keyspace="sparse", hot=0.55, hot_pure="min_neutral"),
    "part_full64": dict(n=N_PART, seed=35, groups=60_000, keyspace="full64"),
    "part_sorted": dict(n=N_PART, seed=36, groups=40_000, keyspace="dense", sorted_keys=True),
    # (sorted keys over a range of more than 512 x 4096 values: two partition levels; 2 rows a key, 8 000 a bucket — and runs of 300
    #  rows of every edge value, Inf and the NaNs among them, and of 21 000 rows of the NaN 0xFFFF..F)
    "part_sorted_wide": dict(n=1 << 22, seed=43, groups=2_100_000, keyspace="dense", sorted_keys=True, hot=0.005, hot_pure="max_neutral",
                             special_rows=300),
    "part_nullable": dict(n=N_PART, seed=37, groups=30_000, keyspace="sparse", nullable="flip64", null_keys=0.01, hot=0.5),
    "part_few_groups": dict(n=N_PART, seed=38, groups=24, keyspace="sparse"),
    "part_wide_range": dict(n=N_PART, seed=39, groups=1_200_000, keyspace="dense_gaps"),
    # (900 sampled groups: 2 bucket tables of 2048 slots for <= 2 cells, 4 of 1024 for 3 — 4 800 groups overflow them by a sixth)
    "part_underestimated": dict(n=1 << 22, seed=40, groups=4800, keyspace="sparse", sampled_groups=900),
    "part_far_underestimated": dict(n=1 << 22, seed=42, groups=200_000, keyspace="dense", sampled_groups=1000),
    "merge_small_last": dict(n=(1 << 21) + 1000, seed=41, groups=60_000, keyspace="sparse", batches=[1 << 21, 1000]),
    "merge_small_first": dict(n=(1 << 21) + 1000, seed=41, groups=60_000, keyspace="sparse", batches=[1 << 21, 1000], reverse=True),
    "simple_3_batches": dict(n=5000, seed=51, groups=1, batches=3, nullable="random"),
    "simple_1_batch": dict(n=5000, seed=52, groups=1),
    "distinct": dict(n=20_011, seed=61, groups=150, keyspace="sparse", nullable="random", batches=2),
})
# every family at a size the oracle handles quickly: the model is checked against it (test_agg_model_cpu.py)
SMALL_CASES = {
    "one_row": dict(n=1, seed=1, groups=1),
    "plain": dict(n=5000, seed=2, groups=400, keyspace="dense"),
    "hot_min_neutral": dict(n=5000, seed=3, groups=300, keyspace="sparse", hot=0.55, hot_pure="min_neutral"),
    "hot_max_neutral": dict(n=5000, seed=4, groups=300, keyspace="full64", hot=0.55, hot_pure="max_neutral", nullable="random"),
    "sorted": dict(n=4097, seed=5, groups=300, keyspace="dense", sorted_keys=True),
    "flip64_null_keys": dict(n=5000, seed=6, groups=250, keyspace="sparse", nullable="flip64", null_keys=0.03),
    "late_nulls_3_batches": dict(n=5000, seed=7, groups=250, keyspace="full64", nullable="random", null_keys=0.03, batches=3, late_nulls=True),
    "reversed_batches": dict(n=3000, seed=8, groups=200, keyspace="dense", nullable="flip64", batches=[2000, 1000], reverse=True),
    "few_groups": dict(n=2000, seed=9, groups=5, keyspace="sparse"),
    "tiny_65": dict(n=65, seed=10, groups=21, keyspace="sparse", nullable="flip64"),
}


@functools.lru_cache(maxsize=3)
def gpu_case(name) -> Case:
    return build(name, **GPU_CASES[name])


def small_case(name) -> Case:
    return build(name, **SMALL_CASES[name])


ALL_FUNCS = [(fn, c) for c in COLS for fn in ("count", "sum", "min", "max")]


# ---- join + aggregate ---------------------------------------------------------------------------------------------------------
class JoinCase:
    """build batch [k, attr], probe batches [k, f, g, i, j]; `joined` is the join written out row by row (a probe row once per
    build row with its key, in probe order: hash_join.rs:207-253) with the GROUP BY column as its key — what the model sees"""

    def __init__(self, build_batch, probe: Case, joined: Case):
        self.build_batch, self.probe, self.joined = build_batch, probe, joined


def join_case(kind, n=70_001, nkeys=300, seed=71) -> JoinCase:
    """unique        300 unique build keys over a dense range, probe keys inside and outside it
    duplicates    multiplicities 1 - 4 over the same range
    attribute     900 unique build keys, GROUP BY a build attribute (300 values, three join keys each — the poisoned join keys
                  stay under a tenth of the attribute values): some join keys
                  have only NULL arguments, one attribute value's only valid argument is INT64_MIN / 0xFFFF..F (MAX neutral) and
                  another's INT64_MAX / 0x7FFF..F (MIN neutral)"""
    rng = np.random.default_rng(seed + len(kind))
    nkeys = 3 * nkeys if kind == "attribute" else nkeys
    probe = build(f"join_{kind}", n, seed, groups=nkeys + 40, keyspace="dense", hot=0.5 if kind != "attribute" else 0.0,
                  nullable="flip64" if kind == "attribute" else None)
    bkeys = np.arange(nkeys, dtype=np.int64) - 777  # the probe's keys -777 .. nkeys + 40 - 778: the last 40 have no partner
    mult = rng.integers(1, 5, nkeys) if kind == "duplicates" else np.ones(nkeys, np.int64)
    attr = (np.arange(nkeys) % (nkeys // 3)).astype(np.int64) * 10 + 3
    cols = {c: (v.copy(), None if valid is None else valid.copy()) for c, (v, valid) in probe.cols.items()}
    if kind == "attribute":
        # attribute values 3 and 13 own ONE join key each (two keys with several probe rows; the others of their class move on)
        k0, k1 = np.nonzero(np.bincount(probe.keys + 777, minlength=nkeys)[:nkeys] >= 2)[0][:2]
        attr[(attr == 3) | (attr == 13)] = 23
        attr[k0], attr[k1] = 3, 13
        for key_at, fbits, iv in ((k0, 0xFFFFFFFFFFFFFFFF, INT64_MIN), (k1, 0x7FFFFFFFFFFFFFFF, INT64_MAX)):
            at = np.nonzero(probe.keys == bkeys[key_at])[0]
            assert len(at) >= 2
            for c, v in (("f", _f64([fbits])[0]), ("i", iv)):
                cols[c][0][at] = v
                cols[c][1][at] = False
                cols[c][1][at[0]] = True  # one valid value, the rest of the attribute's rows NULL
        probe = Case(probe.name, probe.keys, probe.key_valid, cols, probe.bounds)
    order = rng.permutation(np.repeat(np.arange(nkeys), mult))
    build_batch = pa.RecordBatch.from_arrays([pa.array(bkeys[order]), pa.array(attr[order])], names=["bk", "attr"])
    at = probe.keys + 777
    has = (at >= 0) & (at < nkeys) & (True if probe.key_valid is None else probe.key_valid)
    reps = np.where(has, mult[np.clip(at, 0, nkeys - 1)], 0)
    rows = np.repeat(np.arange(n), reps)
    jkeys = probe.keys[rows] if kind != "attribute" else attr[at[rows]]
    jcols = {c: (v[rows], None if valid is None else valid[rows]) for c, (v, valid) in probe.cols.items()}
    return JoinCase(build_batch, probe, Case(f"joined_{kind}", jkeys, None, jcols, [0, len(rows)]))


def distinct_case(case: Case, col="i") -> Case:
    """the rows of `case` with every (key, value of `col`) pair kept once, in first-seen order: what COUNT(DISTINCT) /
    SUM(DISTINCT) aggregate (count.rs:31-58 keeps NULL as ONE of the distinct values, sum.rs:99-132 skips it).  In the
    result column `i` holds the distinct values with their validity and column `j` is all valid, so that
    ("count", "j") is COUNT(DISTINCT col) and ("sum", "i") is SUM(DISTINCT col)."""
    order = np.concatenate([np.arange(lo, hi) for lo, hi in case.ranges()])
    v, valid = case.cols[col]
    valid = np.ones(case.n, bool) if valid is None else valid
    kv = np.ones(case.n, bool) if case.key_valid is None else case.key_valid
    rows = np.stack([kv, np.where(kv, case.keys, 0), valid, np.where(valid, v, 0)], axis=1).astype(np.int64)[order]
    _, first = np.unique(rows, axis=0, return_index=True)
    keep = order[np.sort(first)]
    cols = {c: (case.cols[c][0][keep], None) for c in COLS}
    cols["i"] = (v[keep].astype(np.int64), valid[keep])
    return Case(case.name + "_distinct", case.keys[keep], None if case.key_valid is None else case.key_valid[keep], cols, [0, len(keep)])
