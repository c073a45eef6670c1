"""An independent model of the hash exchange primitives sqlrs_hash_partition and sqlrs_hash_partition_filter: plain Python
integers and numpy / pyarrow containers, no call into the library, the oracle or sqlrs_amd.distributed.  What it pins (DESIGN.md,
"The hash-partition contract"):

* key image of a row: None for a NULL key, otherwise a 64-bit unsigned integer — an int64 value mod 2^64, an int32 value sign-
  extended and then mod 2^64, the bit pattern of a double (-0.0 != +0.0, every NaN payload is a key of its own), 0 / 1 for a
  Boolean; an expression key is evaluated with tests/expr_model.py first;
* partition of an image: p = ((mix64(image ^ 0x5851f42d4c957f2d) >> 32) * parts) >> 32 with mix64 the 64-bit finaliser
  x ^= x >> 33; x *= 0xff51afd7ed558ccd; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33 (all mod 2^64); a NULL key: 0;
* Utf8 keys: the partition is a function of a library-internal hash of the bytes, which the model does not predict.  It states
  the properties instead (`utf8_partitions` reads the assignment off an output and asserts them): equal strings share a
  partition, every NULL is in partition 0, every partition is < parts.  With that assignment the stable output is determined;
* sqlrs_hash_partition: the rows partition-major, input order kept inside a partition, and the parts + 1 offsets;
* sqlrs_hash_partition_filter: per partition the MULTISET of the whole rows whose predicate is TRUE (FALSE and NULL drop a row,
  tests/expr_model.py); the order inside a partition is unspecified, the regions lie inside the batch and do not overlap.

`compare` is exact everywhere: a partitioner only moves rows.  Doubles compare by bit pattern, NULLs as NULLs (what lies under
a NULL is not looked at)."""
from collections import Counter
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import pyarrow as pa

import expr_model as X
from join_model import compare_batch

MASK = (1 << 64) - 1
PART_SALT = 0x5851f42d4c957f2d
MAX_PARTS = 256


def mix64(x: int) -> int:
    x &= MASK
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & MASK
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & MASK
    x ^= x >> 33
    return x


def part_of(image: Optional[int], parts: int) -> int:
    """partition of one key image; None (a NULL key) -> 0"""
    if image is None:
        return 0
    return ((mix64(image ^ PART_SALT) >> 32) * parts) >> 32


# ---- key images --------------------------------------------------------------------------------------------------------------------
def images_of(arr) -> list:
    """key image of every row of a key COLUMN: None | int in [0, 2^64) | bytes (Utf8: an identity, not an image)"""
    t = arr.type
    assert t in (pa.int32(), pa.int64(), pa.float64(), pa.bool_(), pa.string()), t
    vals = X.column_values(arr)
    if t == pa.string():
        return vals
    return [None if v is None else v & MASK for v in vals]  # (a negative Python int & MASK = its sign extension mod 2^64)


def key_ids(batch: pa.RecordBatch, key) -> list:
    """key image of every row for a key EXPRESSION over the batch (InputRef, arithmetic, Cast: tests/expr_model.py)"""
    res = X.evaluate(key, batch)
    assert all(s == X.EXACT for s in res.state), "a key expression must be exact in the model"
    assert res.dtype in (X.abi.INT32, X.abi.INT64, X.abi.FLOAT64, X.abi.BOOLEAN, X.abi.UTF8), res.dtype
    if res.dtype == X.abi.UTF8:
        return list(res.vals)
    return [None if v is None else v & MASK for v in res.vals]


def is_utf8(ids) -> bool:
    return any(isinstance(k, bytes) for k in ids)


def partitions(ids, parts: int) -> list:
    """partition of every row of fixed-width key images"""
    assert 1 <= parts <= MAX_PARTS and not is_utf8(ids)
    memo = {}
    out = []
    for k in ids:
        p = memo.get(k)
        if p is None:
            p = memo[k] = part_of(k, parts)
        out.append(p)
    return out


# ---- expectations ------------------------------------------------------------------------------------------------------------------
@dataclass
class Stable:
    """sqlrs_hash_partition: output row j = input row perm[j]; partition p = rows [offsets[p], offsets[p + 1])"""
    batch: pa.RecordBatch
    offsets: List[int]
    perm: np.ndarray


@dataclass
class Kept:
    """sqlrs_hash_partition_filter: rows[p] = the input rows of partition p that pass, ascending"""
    batch: pa.RecordBatch
    rows: List[np.ndarray]


def stable_from(batch, pids, parts) -> Stable:
    p = np.asarray(pids, dtype=np.int64).reshape(-1)
    assert len(p) == batch.num_rows and (len(p) == 0 or (0 <= p.min() and p.max() < parts))
    counts = np.bincount(p, minlength=parts) if len(p) else np.zeros(parts, np.int64)
    return Stable(batch, [0] + [int(v) for v in np.cumsum(counts)], np.argsort(p, kind="stable"))


def expected_stable(batch, ids, parts) -> Stable:
    return stable_from(batch, partitions(ids, parts), parts)


def keep_mask(batch, pred) -> np.ndarray:
    """rows a predicate keeps: mask TRUE; FALSE and NULL drop the row.  None: every row"""
    if pred is None:
        return np.ones(batch.num_rows, dtype=bool)
    res = X.evaluate(pred, batch)
    assert res.dtype == X.abi.BOOLEAN and all(s == X.EXACT for s in res.state)
    return np.array([v == 1 for v in res.vals], dtype=bool).reshape(-1)


def kept_from(batch, pids, keep, parts) -> Kept:
    p = np.asarray(pids, dtype=np.int64).reshape(-1)
    keep = np.asarray(keep, dtype=bool).reshape(-1)
    assert len(p) == len(keep) == batch.num_rows
    return Kept(batch, [np.nonzero(keep & (p == q))[0] for q in range(parts)])


def expected_filter(batch, ids, keep, parts) -> Kept:
    return kept_from(batch, partitions(ids, parts), keep, parts)


def utf8_partitions(got_keys, offsets, ids, parts) -> list:
    """the partition of every INPUT row of a Utf8-keyed run, read off the output's key column and offsets; asserts the properties
    the contract gives a Utf8 key: equal strings share a partition, every NULL is in partition 0, partitions are < parts"""
    assert len(offsets) == parts + 1 and offsets[0] == 0 and offsets[-1] == len(ids) == len(got_keys), (offsets[:4], offsets[-1], len(ids))
    assert all(a <= b for a, b in zip(offsets, offsets[1:])), "offsets must not decrease"
    where = {}
    out_ids = images_of(got_keys)
    for p in range(parts):
        for k in set(out_ids[offsets[p]:offsets[p + 1]]):
            assert k not in where, f"key {k!r} is in partitions {where[k]} and {p}"
            where[k] = p
    assert where.get(None, 0) == 0, f"NULL keys are in partition {where[None]}, not 0"
    missing = set(ids) - set(where)
    assert not missing, f"{len(missing)} keys of the input are not in the output, e.g. {sorted(missing, key=repr)[:3]}"
    return [where[k] for k in ids]


# ---- comparison --------------------------------------------------------------------------------------------------------------------
def rows_of(batch, start=0, length=None) -> list:
    """whole rows as tuples of None | int | bytes (doubles by bit pattern)"""
    b = batch.slice(start, length)
    cols = [X.column_values(b.column(c)) for c in range(b.num_columns)]
    return list(zip(*cols)) if cols else [()] * b.num_rows


def _same_types(got, batch, label):
    assert got.num_columns == batch.num_columns, f"{label}: {got.num_columns} columns, expected {batch.num_columns}"
    for c in range(batch.num_columns):
        assert got.column(c).type == batch.column(c).type, f"{label}: column {c} is {got.column(c).type}, expected {batch.column(c).type}"


def compare(got: pa.RecordBatch, layout, expected, label=""):
    """Stable: layout = the parts + 1 offsets; the offsets and every column of every row, bit for bit.
    Kept: layout = (part_start, part_rows); the regions lie inside the batch, do not overlap, hold the model's number of rows and,
    as multisets of whole rows, the model's rows."""
    if isinstance(expected, Stable):
        offsets = [int(v) for v in layout]
        assert offsets == expected.offsets, (f"{label}: offsets differ, first at partition "
                                             f"{next(i for i, (a, b) in enumerate(zip(offsets + [None] * len(expected.offsets), expected.offsets + [None] * len(offsets))) if a != b)}: "
                                             f"got {offsets[:6]}..{offsets[-3:]}, expected {expected.offsets[:6]}..{expected.offsets[-3:]}")
        want = expected.batch.take(pa.array(expected.perm, type=pa.int64()))
        compare_batch(got, want, label)
        return
    assert isinstance(expected, Kept)
    starts, rows = [int(v) for v in layout[0]], [int(v) for v in layout[1]]
    parts = len(expected.rows)
    assert len(starts) == len(rows) == parts, f"{label}: {len(starts)} starts and {len(rows)} row counts for {parts} partitions"
    _same_types(got, expected.batch, label)
    for p in range(parts):
        assert rows[p] >= 0 and 0 <= starts[p] and starts[p] + rows[p] <= got.num_rows, \
            f"{label}: partition {p} = [{starts[p]}, {starts[p] + rows[p]}) leaves the batch of {got.num_rows} rows"
    used = sorted((starts[p], starts[p] + rows[p], p) for p in range(parts) if rows[p])
    for (a0, a1, pa_), (b0, b1, pb) in zip(used, used[1:]):
        assert a1 <= b0, f"{label}: the regions of partitions {pa_} [{a0}, {a1}) and {pb} [{b0}, {b1}) overlap"
    for p in range(parts):
        assert rows[p] == len(expected.rows[p]), f"{label}: partition {p} holds {rows[p]} rows, expected {len(expected.rows[p])}"
    for p in range(parts):
        if not rows[p]:
            continue
        g = Counter(rows_of(got, starts[p], rows[p]))
        e = Counter(rows_of(expected.batch.take(pa.array(expected.rows[p], type=pa.int64()))))
        if g != e:
            extra, lack = list((g - e).items())[:3], list((e - g).items())[:3]
            raise AssertionError(f"{label}: partition {p}: rows differ as multisets; not expected: {extra}; missing: {lack}")


def compare_kept_in_order(got: pa.RecordBatch, layout, expected: Kept, label=""):
    """the composed route (Filter, then the stable partition): contiguous partitions in order, input order kept inside each"""
    starts, rows = [int(v) for v in layout[0]], [int(v) for v in layout[1]]
    perm = np.concatenate([np.asarray(r, dtype=np.int64) for r in expected.rows] + [np.zeros(0, np.int64)])
    offs = [0] + [int(v) for v in np.cumsum([len(r) for r in expected.rows])]
    assert starts == offs[:-1] and rows == [b - a for a, b in zip(offs, offs[1:])], f"{label}: the partitions are not contiguous and in order"
    compare(got, offs, Stable(expected.batch, offs, perm), label)
