"""Seeded cases of the hash exchange primitives, for tests/test_partition_model_cpu.py (model against the package's restatement,
planted faults, what the library claims about itself) and tests/test_gpu_partition_edges.py (every device route).  numpy and
pyarrow only; the pools and payload makers are those of tests/join_edge_cases.py.

A case names
  form      stable (sqlrs_hash_partition) | filter (sqlrs_hash_partition_filter)
  kind      the key: i64 | f64 | i32 | bool | utf8 as a column reference, i64_plus1 (`col + 1` over an int64 column, wraps at the
            end of int64), cast_i32 (`CAST(col AS INT64)` over an int32 column)
  dist      pool (the edge pools mixed with random keys) | equal (one key: one partition receives whole tiles) | ends (two keys
            that the model places in partition 0 and in partition parts - 1) | runs64 / runs64_off (runs of 64 equal keys aligned /
            misaligned to the waves) | few (keys of fewer than `parts` partitions: the first, a middle and the last one are empty)
  nulls     the share of NULL keys: 0, 0.1 or 1
  payload   key_only | numeric | full | utf8 (join_edge_cases.PAYLOADS: nullable f64, int32, Boolean, Utf8 columns behind the key)
            | plain (`ncols` 8-byte columns without NULLs, the key in column `kcol`, beside it a NaN-rich double `v` and, with three
            columns, the row number `rid`)
  rows, parts, mem_in (device | host | slice: rows [3, 3 + rows) of a longer HOST batch, handed over with its offset), mem_out
  pred      filter form: none | key | carried | other (`col OP const` over the key, over the double, over the row number) | and
            (a composed predicate) | nullable (over a column with NULLs) | none_pass | all_pass
  route     what it is made for: fast | general (stable form), fused | composed (filter form)

Row counts: 65536 is the threshold of the fast routes, 4096 one tile (SP_TILE), 65537 leaves one row in the last tile."""
import functools

import numpy as np
import pyarrow as pa

import partition_model as M
from join_edge_cases import (I32_MAX, I32_MIN, I64_MAX, I64_MIN, NAN_PAYLOADS, POOL_F64, POOL_I32, POOL_I64, STRINGS, bool_payload,
                             f64_payload, i32_payload, key_array, utf8_payload)

ROWS = [0, 1, 63, 64, 65, 4095, 4096, 4097, 65535, 65536, 65537, 65536 + 4096, 3 * 4096 * 8 + 1]
PARTS = [1, 2, 3, 8, 255, 256]
FAST_ROWS = 1 << 16
TILE = 4096
PAYLOADS = {"full": ("x", "i", "b", "s"), "numeric": ("x", "i"), "utf8": ("x", "i", "s"), "key_only": ()}
_MAKE = {"x": f64_payload, "i": i32_payload, "b": bool_payload, "s": utf8_payload}
COLUMN_KIND = {"i64": "i64", "f64": "f64", "i32": "i32", "bool": "bool", "utf8": "utf8", "i64_plus1": "i64", "cast_i32": "i32"}
UTF8_POOL = STRINGS + ["a" * 8, "a" * 9, "a\x00", "a\x00b", "é", "ée", " ", "NULL"]


# ---- keys --------------------------------------------------------------------------------------------------------------------------
def _pool(ck):
    return {"i64": POOL_I64, "i32": POOL_I32, "f64": POOL_F64 + NAN_PAYLOADS, "bool": [0, 1]}[ck]


def random_keys(rng, ck, m):
    if ck == "i64":
        wide = rng.integers(I64_MIN, I64_MAX, m, dtype=np.int64)
        near = rng.integers(-10 ** 12, 10 ** 12, m, dtype=np.int64)
        return [int(v) for v in np.where(rng.random(m) < 0.5, wide, near)]
    if ck == "i32":
        return [int(v) for v in rng.integers(I32_MIN, I32_MAX, m, dtype=np.int64)]
    if ck == "f64":
        return [int(v) for v in rng.integers(0, 1 << 63, m, dtype=np.uint64) | (rng.integers(0, 2, m, dtype=np.uint64) << np.uint64(63))]
    if ck == "bool":
        return [int(v) for v in rng.integers(0, 2, m)]
    return [f"key{int(v)}" for v in rng.integers(0, 400, m)]


def _image(ck, v):
    """the model's image of a key VALUE of the case library (ints; bit patterns for f64)"""
    return v & M.MASK


def _search(ck, parts, want, avoid=()):
    """the first candidate key (pool first, then 0, 1, 2, ... / small doubles) that the model places in a partition of `want`"""
    cands = list(_pool(ck)) + ([0, 1] if ck == "bool" else list(range(2, 200_000)))
    for v in cands:
        if ck == "i32" and not I32_MIN <= v <= I32_MAX:
            continue
        if v not in avoid and M.part_of(_image(ck, v), parts) in want:
            return v
    raise AssertionError(f"no {ck} key for partitions {sorted(want)[:4]} of {parts}")


def key_values(rng, ck, dist, n, parts, plus=0):
    """n key values (Python ints / strings).  `plus`: the key expression adds this to the column, so the column holds value - plus"""
    if n == 0:
        return []
    if ck == "utf8":
        if dist == "equal":
            return [""] * n
        vals = UTF8_POOL + random_keys(rng, ck, 60)
        if dist in ("runs64", "runs64_off"):
            shift = 23 if dist == "runs64_off" else 0
            return [vals[((i + shift) // 64) % len(vals)] for i in range(n)]
        pick = rng.integers(0, len(vals), n)
        return [vals[j] for j in pick]
    if dist == "pool":
        pool, rnd = _pool(ck), random_keys(rng, ck, n)
        pick = rng.integers(0, len(pool), n)
        use = rng.random(n) < 0.5
        out = [pool[pick[i]] if use[i] else rnd[i] for i in range(n)]
    elif dist == "equal":
        out = [{"i64": I64_MIN, "i32": I32_MIN, "f64": 0x8000000000000000, "bool": 1}[ck]] * n
    elif dist == "ends":
        lo, hi = _search(ck, parts, {0}), _search(ck, parts, {parts - 1})
        out = [lo if s else hi for s in rng.random(n) < 0.5]
        out[0], out[-1] = lo, hi
    elif dist in ("runs64", "runs64_off"):
        vals = list(_pool(ck)) + random_keys(rng, ck, n // 64 + 2)
        rng.shuffle(vals)
        shift = 23 if dist == "runs64_off" else 0
        out = [vals[((i + shift) // 64) % len(vals)] for i in range(n)]
    elif dist == "few":
        assert parts >= 8 and ck != "bool"
        empty = {0, parts // 2, parts - 1}
        allowed = [p for p in range(parts) if p not in empty][:5]
        vals = []
        for p in allowed:
            vals.append(_search(ck, parts, {p}, avoid=vals))
            vals.append(_search(ck, parts, {p}, avoid=vals))
        pick = rng.integers(0, len(vals), n)
        out = [vals[j] for j in pick]
    else:
        raise ValueError(dist)
    if plus:  # (the column holds what the expression maps onto the chosen key: value - plus, wrapped to int64)
        out = [M.X.wrap(v - plus, 64) for v in out]
    return out


def key_column(ck, vals, null):
    if ck == "utf8":
        return pa.array([None if z else v for v, z in zip(vals, null)], type=pa.string())
    return key_array(ck, vals, null)


# ---- cases -------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, form, kind, dist, rows, parts, payload, route, nulls=0.0, ncols=None, kcol=0, mem_in="device", mem_out="device",
                 pred="none", seed=0):
        self.form, self.kind, self.dist, self.rows, self.parts, self.payload, self.route = form, kind, dist, rows, parts, payload, route
        self.nulls, self.kcol, self.mem_in, self.mem_out, self.pred_name, self.seed = nulls, kcol, mem_in, mem_out, pred, seed
        self.ncols = ncols if payload == "plain" else 1 + len(PAYLOADS[payload])
        assert payload == "plain" or kcol == 0
        assert form == "filter" or pred == "none"
        shape = f"{payload}{self.ncols}k{kcol}" if payload == "plain" else payload
        self.name = f"{form}-{kind}-{dist}-n{rows}-p{parts}-{shape}-null{nulls:g}-{mem_in}-{mem_out}" + ("" if form == "stable" else f"-{pred}")

    def __repr__(self):
        return self.name

    @functools.cached_property
    def batch(self) -> pa.RecordBatch:
        """the input: `rows` rows (for mem_in == "slice": rows [3, 3 + rows) of a longer batch, buffers at a non-zero offset)"""
        rng = np.random.default_rng(5000 + self.seed)
        ck = COLUMN_KIND[self.kind]
        lead = 3 if self.mem_in == "slice" else 0
        n = self.rows + lead
        vals = key_values(rng, ck, self.dist, n, self.parts, plus=1 if self.kind == "i64_plus1" else 0)
        null = np.ones(n, dtype=bool) if self.nulls >= 1 else (rng.random(n) < self.nulls)
        if 0 < self.nulls < 1 and n > lead + 8:
            null[lead + 1] = True
        key = key_column(ck, vals, null)
        if self.payload == "plain":
            rid = pa.array(np.arange(n, dtype=np.int64))
            bits = rng.integers(0, 1 << 62, n, dtype=np.uint64) | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))
            nan = rng.random(n) < 0.1
            bits[nan] = rng.choice(np.array(NAN_PAYLOADS + [0x8000000000000000, 0], dtype=np.uint64), int(nan.sum()))
            val = pa.array(bits.view(np.float64), from_pandas=False)
            others = [("v", val), ("rid", rid)][:self.ncols - 1]
            cols = others[:self.kcol] + [("k", key)] + others[self.kcol:]
        else:
            cols = [("k", key)] + [(c, _MAKE[c](rng, n)) for c in PAYLOADS[self.payload]]
        b = pa.RecordBatch.from_arrays([a for _, a in cols], names=[nm for nm, _ in cols])
        return b.slice(lead, self.rows) if lead else b

    def column(self, name) -> int:
        return self.batch.schema.names.index(name)

    @property
    def key(self):
        from sqlrs_amd import abi
        from sqlrs_amd.expr import Constant, InputRef, TypeCast
        if self.kind == "i64_plus1":
            return InputRef(self.kcol) + Constant(1, abi.INT64)
        if self.kind == "cast_i32":
            return TypeCast(InputRef(self.kcol), abi.INT64)
        return InputRef(self.kcol)

    @property
    def pred(self):
        """the predicate; the constants are those of test_hash_partition_filter_edge_constants (INT64_MIN, 0, +0.0): the constants
        themselves are tested there"""
        from sqlrs_amd import abi
        from sqlrs_amd.expr import Constant, InputRef
        p = self.pred_name
        if p == "none":
            return None
        zero = Constant(0, abi.INT64)
        if p == "key":
            return InputRef(self.kcol) > (zero if COLUMN_KIND[self.kind] == "i64" else Constant(0.0, abi.FLOAT64))
        if p == "carried":
            return InputRef(self.column("v")) > Constant(0.0, abi.FLOAT64)
        if p == "other":
            return InputRef(self.column("rid")) <= Constant(self.rows // 2 + (3 if self.mem_in == "slice" else 0), abi.INT64)
        if p == "and":
            return (InputRef(self.column("v")) > Constant(0.0, abi.FLOAT64)) & (InputRef(self.column("rid")) >= Constant(7, abi.INT64))
        if p == "nullable":
            return InputRef(self.column("x")) > Constant(0.0, abi.FLOAT64)
        lowest = Constant(I64_MIN, abi.INT64)
        ref = InputRef(self.column("rid"))
        return ref < lowest if p == "none_pass" else ref >= lowest

    # ---- the model's view (computed once per case) ----
    @functools.cached_property
    def ids(self):
        return M.key_ids(self.batch, self.key)

    @functools.cached_property
    def keep(self):
        return M.keep_mask(self.batch, self.pred)

    @functools.cached_property
    def expected(self):
        """Stable / Kept of a fixed-width key; None for a Utf8 key (the model states properties: M.utf8_partitions)"""
        if COLUMN_KIND[self.kind] == "utf8":
            return None
        if self.form == "stable":
            return M.expected_stable(self.batch, self.ids, self.parts)
        return M.expected_filter(self.batch, self.ids, self.keep, self.parts)


def _cases():
    out = []

    def add(form, *a, **kw):
        kw.setdefault("seed", len(out))
        out.append(Case(form, *a, **kw))

    def route_s(rows, parts=8):
        return "fast" if rows >= FAST_ROWS and parts > 1 else "general"
    # ---- sqlrs_hash_partition -------------------------------------------------------------------------------------------------
    for n in ROWS:  # every row count: the fast shape (fast from 65536 rows on) and a general shape
        add("stable", "i64", "pool", n, 8, "plain", route_s(n), ncols=2)
        add("stable", "i64", "pool", n, 3, "numeric", "general", nulls=0.1)
    # every part count on the fast route, the key in column 0, 1 and 2 of 1 to 3 columns, int64 and float64 keys
    add("stable", "f64", "pool", 65537, 2, "plain", "fast", ncols=1, kcol=0)
    add("stable", "f64", "pool", 65537, 3, "plain", "fast", ncols=3, kcol=1)
    add("stable", "i64", "pool", 65537, 255, "plain", "fast", ncols=3, kcol=2)
    add("stable", "f64", "pool", 65537, 256, "plain", "fast", ncols=2, kcol=1)
    add("stable", "i64", "pool", 65536, 256, "plain", "fast", ncols=3, kcol=0)
    add("stable", "i64", "pool", 65536, 1, "plain", "general", ncols=2)           # one part: not the fast route
    # every part count on the general route, every key type
    for parts, kind, payload in ((1, "i32", "full"), (2, "bool", "full"), (3, "utf8", "full"), (8, "f64", "full"), (255, "i32", "utf8"),
                                 (256, "i64", "full"), (256, "utf8", "numeric"), (255, "f64", "key_only")):
        add("stable", kind, "pool", 4097, parts, payload, "general", nulls=0.1)
    # key distributions, on both routes
    for dist, parts in (("equal", 8), ("ends", 256), ("ends", 3), ("runs64", 8), ("runs64_off", 255), ("few", 8), ("few", 256)):
        add("stable", "i64" if parts != 3 else "f64", dist, 65536 + 4096, parts, "plain", "fast", ncols=2 if parts != 255 else 3, kcol=parts % 2)
        add("stable", "f64" if parts != 3 else "i32", dist, 4097, parts, "full", "general")
    add("stable", "i32", "few", 4097, 255, "numeric", "general", nulls=0.1)
    add("stable", "utf8", "equal", 4097, 8, "utf8", "general")
    add("stable", "utf8", "runs64_off", 4097, 8, "numeric", "general", nulls=0.1)
    add("stable", "bool", "equal", 4096, 2, "numeric", "general")
    # NULL keys: none, a tenth, all of them; every key type
    for kind in ("i64", "f64", "i32", "bool", "utf8"):
        for nulls in (0.0, 0.1, 1.0):
            add("stable", kind, "pool", 4097, 8, "utf8" if kind in ("i64", "utf8") else "numeric", "general", nulls=nulls)
    add("stable", "utf8", "pool", 4097, 200, "key_only", "general", nulls=0.1)
    # shapes one condition away from the fast route
    add("stable", "i64", "pool", 65536, 8, "plain", "general", nulls=0.1, ncols=2)      # NULL keys
    add("stable", "i64", "pool", 65536, 8, "plain", "general", nulls=1.0, ncols=1)
    add("stable", "i32", "pool", 65536, 8, "key_only", "general")                       # a 4-byte key
    add("stable", "i64", "pool", 65537, 8, "numeric", "general")                        # nullable, 4-byte payload
    add("stable", "i64_plus1", "pool", 65536, 8, "plain", "general", ncols=2)           # an expression key
    add("stable", "i64_plus1", "ends", 4097, 8, "numeric", "general", nulls=0.1)
    add("stable", "cast_i32", "pool", 4097, 8, "numeric", "general", nulls=0.1)
    add("stable", "cast_i32", "pool", 65536, 3, "key_only", "general")
    add("stable", "utf8", "pool", 3 * 4096 * 8 + 1, 256, "utf8", "general", nulls=0.1)
    add("stable", "bool", "pool", 65537, 2, "full", "general", nulls=0.1)
    # input and output forms
    for mem_in, mem_out in (("host", "device"), ("slice", "device"), ("device", "host"), ("slice", "host")):
        add("stable", "i64", "pool", 65536, 8, "plain", "fast", ncols=3, kcol=1, mem_in=mem_in, mem_out=mem_out)
        add("stable", "f64", "pool", 4097, 8, "full", "general", nulls=0.1, mem_in=mem_in, mem_out=mem_out)
    add("stable", "utf8", "pool", 4095, 3, "full", "general", nulls=0.1, mem_in="slice", mem_out="host")
    add("stable", "bool", "pool", 65, 2, "full", "general", nulls=0.1, mem_in="slice", mem_out="host")
    add("stable", "i64", "pool", 0, 8, "full", "general", mem_in="host", mem_out="host")
    add("stable", "i64", "pool", 1, 256, "full", "general", mem_in="slice", mem_out="host")
    # ---- sqlrs_hash_partition_filter ------------------------------------------------------------------------------------------
    for n in ROWS:  # every row count: fused from 65536 rows on
        add("filter", "i64", "pool", n, 8, "plain", "fused" if n >= FAST_ROWS else "composed", ncols=2, pred="carried")
    for parts, ncols, kcol, pred in ((1, 2, 0, "carried"), (2, 3, 2, "other"), (3, 1, 0, "key"), (255, 2, 1, "key"), (256, 1, 0, "none"),
                                     (256, 2, 0, "carried"), (8, 3, 1, "none_pass"), (8, 3, 0, "all_pass"), (3, 2, 1, "none")):
        add("filter", "i64", "pool", 65537 if parts % 2 else 65536, parts, "plain", "fused", ncols=ncols, kcol=kcol, pred=pred)
    for dist, parts, pred in (("equal", 8, "carried"), ("equal", 256, "none"), ("ends", 256, "carried"), ("ends", 2, "carried"), ("runs64", 8, "other"),
                              ("runs64_off", 255, "carried"), ("few", 8, "carried"), ("few", 256, "none")):
        add("filter", "i64", dist, 65536 + 4096, parts, "plain", "fused", ncols=3 if pred == "other" else 2, kcol=0 if parts != 255 else 1, pred=pred)
    add("filter", "i64", "pool", 65536, 8, "plain", "fused", ncols=2, mem_in="host", pred="carried")
    add("filter", "i64", "pool", 65537, 8, "plain", "fused", ncols=3, kcol=2, mem_in="slice", pred="other")
    # composed: one condition of the fused route broken
    add("filter", "i64", "pool", 65536, 8, "plain", "composed", ncols=2, mem_out="host", pred="carried")            # HOST output
    add("filter", "i64", "pool", 65536, 8, "plain", "composed", ncols=3, pred="and")                                # a composed predicate
    add("filter", "f64", "pool", 65536, 8, "plain", "composed", ncols=2, kcol=1, pred="carried")                    # a non-Int64 key
    add("filter", "f64", "pool", 65537, 256, "plain", "composed", ncols=2, pred="key")
    add("filter", "i64", "pool", 65536, 8, "numeric", "composed", pred="nullable")                                  # nullable, 4-byte columns
    add("filter", "i64", "pool", 65536, 8, "plain", "composed", nulls=0.1, ncols=2, pred="carried")                 # NULL keys
    add("filter", "i64_plus1", "pool", 65536, 8, "plain", "composed", ncols=2, pred="carried")                      # an expression key
    add("filter", "i64", "pool", 65536, 8, "plain", "composed", ncols=3, pred="none_pass", mem_out="host")
    for kind, payload, parts, pred in (("i32", "numeric", 3, "nullable"), ("bool", "full", 2, "nullable"), ("utf8", "utf8", 8, "nullable"),
                                       ("f64", "full", 255, "key"), ("utf8", "full", 256, "none"), ("cast_i32", "numeric", 8, "none"),
                                       ("i64", "full", 1, "nullable")):
        add("filter", kind, "pool", 4097, parts, payload, "composed", nulls=0.1, pred=pred)
    add("filter", "i64", "few", 4097, 8, "numeric", "composed", pred="nullable", mem_in="slice", mem_out="host")
    add("filter", "f64", "ends", 4096, 256, "full", "composed", pred="nullable", mem_in="host")
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = {}
    for c in _cases():
        assert c.name not in cases, c.name
        cases[c.name] = c
    return cases


def case(name) -> Case:
    return all_cases()[name]


def names(form=None, route=None, **attrs):
    return [c.name for c in all_cases().values() if (form is None or c.form == form) and (route is None or c.route == route)
            and all(getattr(c, k) == v for k, v in attrs.items())]
