"""An independent model of the hash join on ONE fixed-width key column: plain Python / numpy / pyarrow containers, no call into
the library or the oracle.  What it pins ("The single-key contract of the join"):

* key identity: NULL is one class (NULL = NULL matches, two NULL build keys are duplicates); int32, int64 and Boolean keys
  compare by value; float64 keys by their 64-bit pattern (-0.0 != 0.0, two NaNs are equal only with equal sign and payload);
* pairs of one probe batch: probe rows ascending; per probe row the build rows of the same identity in build insertion order
  across the build batches; Right / Full: a probe row without partner gives (NULL, row) IN PLACE;
* join filter: evaluated with tests/expr_model.py on the intermediate rows ((NULL, row) rows included), a pair is kept when the
  predicate is valid and TRUE; Right / Full: probe rows left without any pair are appended as (NULL, row), ascending, BEHIND
  the survivors;
* tail (Left / Full): the build rows that are in no final pair of any probe batch, ascending, every right column NULL;
* one joined batch per probe batch — an empty one when there is no pair — and, for Left / Full, the tail even when it is
  empty; Inner / Right have no tail (test_join_model_cpu.py pins both against the oracle).

`compare` is exact everywhere: there is no tolerance in a join."""
from typing import List, Optional

import numpy as np
import pyarrow as pa

import expr_model as X

OUTER_RIGHT = ("right", "full")
OUTER_LEFT = ("left", "full")


def key_ids(arr) -> list:
    """identity of every key of a column: None (NULL) or an int — the value of an integer / Boolean key, the bit pattern of a double"""
    t = arr.type
    assert t in (pa.int32(), pa.int64(), pa.float64(), pa.bool_()), t
    return X.column_values(arr)


class JoinModel:
    def __init__(self, build_batches: List[pa.RecordBatch], lkey: int, join_type: str, filt=None):
        self.jt, self.filt, self.lkey = join_type.lower(), filt, lkey
        self.build = pa.Table.from_batches(build_batches).combine_chunks() if build_batches else None
        self.rows_of = {}  # identity -> build rows, in insertion order
        if self.build is not None:
            for row, k in enumerate(key_ids(self.build.column(lkey))):
                self.rows_of.setdefault(k, []).append(row)
        self.visited = set()

    # ---- one probe batch -----------------------------------------------------------------------------------------------------
    def raw_pairs(self, probe: pa.RecordBatch, rkey: int):
        """(left, right) before the join filter; left[i] None = NULL"""
        left, right = [], []
        for r, k in enumerate(key_ids(probe.column(rkey))):
            partners = self.rows_of.get(k, [])
            if partners:
                left += partners
                right += [r] * len(partners)
            elif self.jt in OUTER_RIGHT:
                left.append(None)
                right.append(r)
        return left, right

    def pairs(self, probe: pa.RecordBatch, rkey: int, mark: bool = True):
        """the final pairs of one probe batch (after the join filter); marks the build rows they visit"""
        left, right = self.raw_pairs(probe, rkey)
        if self.filt is not None:
            res = X.evaluate(self.filt, self.joined(probe, left, right))
            assert res.dtype == X.abi.BOOLEAN and all(s == X.EXACT for s in res.state)
            keep = [i for i, v in enumerate(res.vals) if v == 1]
            left, right = [left[i] for i in keep], [right[i] for i in keep]
            if self.jt in OUTER_RIGHT:
                have = set(right)
                orphans = [r for r in range(probe.num_rows) if r not in have]
                left += [None] * len(orphans)
                right += orphans
        if mark:
            self.visited.update(l for l in left if l is not None)
        return left, right

    def joined(self, probe: pa.RecordBatch, left, right) -> pa.RecordBatch:
        li = pa.array(left, type=pa.int64())
        ri = pa.array(right, type=pa.int64())
        cols = [self.build.column(c).take(li) for c in range(self.build.num_columns)]
        cols += [probe.column(c).take(ri) for c in range(probe.num_columns)]
        cols = [c.combine_chunks() if isinstance(c, pa.ChunkedArray) else c for c in cols]
        return pa.RecordBatch.from_arrays(cols, names=[f"c{i}" for i in range(len(cols))])

    def index_batch(self, left, right) -> pa.RecordBatch:
        """the pairs as sqlrs_hash_join_probe_indices returns them"""
        return pa.RecordBatch.from_arrays([pa.array(left, type=pa.uint64()), pa.array(right, type=pa.uint32())],
                                          names=["left_indices", "right_indices"])

    def tail_rows(self) -> Optional[list]:
        if self.jt not in OUTER_LEFT or self.build is None:
            return None
        return [r for r in range(self.build.num_rows) if r not in self.visited]

    def tail(self, right_types) -> Optional[pa.RecordBatch]:
        rows = self.tail_rows()
        if rows is None:
            return None
        li = pa.array(rows, type=pa.int64())
        cols = [self.build.column(c).take(li) for c in range(self.build.num_columns)]
        cols = [c.combine_chunks() if isinstance(c, pa.ChunkedArray) else c for c in cols]
        cols += [pa.nulls(len(rows), type=t) for t in right_types]
        return pa.RecordBatch.from_arrays(cols, names=[f"c{i}" for i in range(len(cols))])


def index_pairs(build_batches, probe_batches, lkey, rkey, join_type):
    """expected output of sqlrs_hash_join_probe_indices, one batch per probe batch (the entry point applies no filter)"""
    if not build_batches:
        return []
    m = JoinModel(build_batches, lkey, join_type)
    return [m.index_batch(*m.raw_pairs(p, rkey)) for p in probe_batches]


def join(build_batches, probe_batches, lkey, rkey, join_type, filt=None, right_types=None):
    """expected output of the operator: one joined batch per probe batch, then the tail (Left / Full).  An empty build CHILD
    (no batch at all) emits nothing."""
    if not build_batches:
        return []
    m = JoinModel(build_batches, lkey, join_type, filt)
    out = [m.joined(p, *m.pairs(p, rkey)) for p in probe_batches]
    if right_types is None:
        right_types = [f.type for f in probe_batches[0].schema] if probe_batches else []
    t = m.tail(right_types)
    return out + ([t] if t is not None else [])


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def _views(arr):
    """(validity bool[], values) of a column: fixed-width values as unsigned integers of their width, Utf8 as a list of bytes"""
    if isinstance(arr, pa.ChunkedArray):
        arr = arr.combine_chunks() if arr.num_chunks != 1 else arr.chunk(0)
    n = len(arr)
    valid = np.asarray(arr.is_valid()).astype(bool) if n else np.zeros(0, bool)
    t = arr.type
    if t == pa.string():
        return valid, [None if v is None else v.encode() for v in arr.to_pylist()]
    if t == pa.bool_():
        return valid, np.array([bool(v) for v in arr.fill_null(False).to_pylist()], dtype=np.uint8)
    width = {pa.int32(): np.uint32, pa.uint32(): np.uint32, pa.int64(): np.uint64, pa.uint64(): np.uint64, pa.float64(): np.uint64}[t]
    if n == 0:
        return valid, np.zeros(0, width)
    raw = np.frombuffer(arr.buffers()[1], dtype=width, count=arr.offset + n)[arr.offset:]
    return valid, raw


def compare_batch(got, exp, label=""):
    assert got is not None, f"{label}: no batch where {exp.num_rows} rows were expected"
    assert got.num_columns == exp.num_columns, f"{label}: {got.num_columns} columns, expected {exp.num_columns}"
    assert got.num_rows == exp.num_rows, f"{label}: {got.num_rows} rows, expected {exp.num_rows}"
    for c in range(exp.num_columns):
        g, e = got.column(c), exp.column(c)
        assert g.type == e.type, f"{label}: column {c} is {g.type}, expected {e.type}"
        gv, gx = _views(g)
        ev, ex = _views(e)
        bad = np.nonzero(gv != ev)[0]
        assert len(bad) == 0, f"{label}: column {c}: validity differs at rows {bad[:8].tolist()} ({len(bad)} rows)"
        if isinstance(ex, list):
            bad = [i for i in range(len(ex)) if ev[i] and gx[i] != ex[i]]
        else:
            bad = np.nonzero(ev & (gx != ex))[0].tolist()
        assert not bad, (f"{label}: column {c}: {len(bad)} values differ, first rows {bad[:8]}: got "
                         f"{[gx[i] if isinstance(gx, list) else hex(int(gx[i])) for i in bad[:4]]}, expected "
                         f"{[ex[i] if isinstance(ex, list) else hex(int(ex[i])) for i in bad[:4]]}")


def compare(got, exp, label=""):
    """`got`: the batches an operator emitted (pyarrow RecordBatches), `exp`: the model's; same number of batches, every batch
    row for row: validity bit for bit, fixed-width values through integer views (a double as its uint64: NaN payloads and the
    sign of zero count) wherever valid, Utf8 by value"""
    got, exp = list(got), list(exp)
    assert len(got) == len(exp), f"{label}: {len(got)} batches, expected {len(exp)}"
    for i, (g, e) in enumerate(zip(got, exp)):
        compare_batch(g, e, f"{label} batch {i}")
