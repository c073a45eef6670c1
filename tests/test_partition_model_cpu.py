"""The model of the hash exchange primitives (tests/partition_model.py) and its case library (tests/partition_edge_cases.py), without a
GPU: the model against the package's own CPU restatement (sqlrs_amd.distributed.partition_of / partition_numpy, which the
product's CPU path uses) on every fixed-width case, exactly; twelve planted faults, each rejected by `compare` on a named case; and
the case library against what it claims (empty partitions, first and last partition, the routes the cases are made for)."""
import numpy as np
import pyarrow as pa
import pytest

import partition_edge_cases as E
import partition_model as M
from sqlrs_amd import abi
from sqlrs_amd import distributed as D
from sqlrs_amd.expr import BinaryOp, Constant, InputRef

FIXED = [n for n, c in E.all_cases().items() if E.COLUMN_KIND[c.kind] != "utf8"]


# ---- the model itself ------------------------------------------------------------------------------------------------------------
def test_mix64_and_part_of_by_hand():
    """the finaliser on values worked out by hand from its definition, and the ends of the multiply-shift"""
    assert M.mix64(0) == 0
    x = 1
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) % 2 ** 64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) % 2 ** 64
    x ^= x >> 33
    assert M.mix64(1) == x == 0xb456bcfc34c2cb2c
    assert M.part_of(None, 256) == 0
    for parts in E.PARTS:
        seen = {M.part_of(k, parts) for k in range(5000)}
        assert seen == set(range(parts)), (parts, sorted(set(range(parts)) - seen))
    # by the formula a NULL key hashed as the value 0 would NOT sit in partition 0 (the discrepancy the header text hides)
    assert [M.part_of(0, p) for p in (8, 200, 256)] == [1, 29, 38]


def test_key_images():
    assert M.images_of(pa.array([-1, None, 2 ** 31 - 1, -(2 ** 31)], type=pa.int32())) == [2 ** 64 - 1, None, 2 ** 31 - 1, 2 ** 64 - 2 ** 31]
    assert M.images_of(pa.array([-1, 2 ** 63 - 1, -(2 ** 63)], type=pa.int64())) == [2 ** 64 - 1, 2 ** 63 - 1, 2 ** 63]
    assert M.images_of(pa.array([0.0, -0.0, None])) == [0, 1 << 63, None]
    assert M.images_of(pa.array([True, None, False])) == [1, None, 0]
    b = pa.RecordBatch.from_arrays([pa.array([2 ** 63 - 1, -1, None], type=pa.int64())], names=["k"])
    assert M.key_ids(b, InputRef(0) + Constant(1, abi.INT64)) == [2 ** 63, 0, None]      # wraps at the end of int64


@pytest.mark.parametrize("name", FIXED)
def test_model_equals_the_package_restatement(name):
    """exact, on every fixed-width case: partition ids, and for the stable form the offsets and the order of partition_numpy"""
    c = E.case(name)
    ids = c.ids
    img = np.array([0 if k is None else k for k in ids], dtype=np.uint64)
    valid = np.array([k is not None for k in ids], dtype=bool)
    pid = D.partition_of(img, c.parts, valid) if len(img) else np.zeros(0, np.uint32)
    assert pid.tolist() == M.partitions(ids, c.parts), name
    if c.form == "stable":
        (got,), offs = D.partition_numpy([img], c.parts, valid) if len(img) else ((img,), [0] * (c.parts + 1))
        assert offs == c.expected.offsets, name
        assert (got == img[c.expected.perm]).all(), name
    else:
        keep = c.keep
        outs, starts, rows = D.partition_filter_numpy([img], c.parts, keep) if valid.all() else (None, None, [int((keep & (pid == p)).sum()) for p in range(c.parts)])
        assert rows == [len(r) for r in c.expected.rows], name


# ---- planted faults --------------------------------------------------------------------------------------------------------------
def one(**attrs):
    (n,) = E.names(**attrs)
    return E.case(n)


def fake_stable(c, part=M.part_of, image=lambda k: k, tweak=None):
    """a partitioner built from the model with a fault planted: `image` re-maps a key image, `part` places it, `tweak` edits the
    (pids, perm, offsets) it would return"""
    pids = np.array([part(None if k is None else image(k), c.parts) for k in c.ids], dtype=np.int64)
    perm = np.argsort(pids, kind="stable")
    offsets = [0] + np.cumsum(np.bincount(pids, minlength=c.parts)).tolist()
    if tweak:
        perm, offsets = tweak(perm, offsets)
    return c.batch.take(pa.array(perm, type=pa.int64())), offsets


def fake_filter(c, keep=None, starts_edit=None):
    pids = np.array(M.partitions(c.ids, c.parts), dtype=np.int64)
    keep = c.keep if keep is None else keep
    rows = [np.nonzero(keep & (pids == p))[0] for p in range(c.parts)]
    perm = np.concatenate(rows)
    starts = [0] + np.cumsum([len(r) for r in rows]).tolist()[:-1]
    if starts_edit:
        starts = starts_edit(starts, [len(r) for r in rows])
    return c.batch.take(pa.array(perm, type=pa.int64())), (starts, [len(r) for r in rows])


def low_half(k, parts):
    return 0 if k is None else ((M.mix64(k ^ M.PART_SALT) & 0xffffffff) * parts) >> 32


def modulo(k, parts):
    return 0 if k is None else (M.mix64(k ^ M.PART_SALT) >> 32) % parts


def null_as_zero(k, parts):
    return M.part_of(0 if k is None else k, parts)


def merged_255(k, parts):
    return min(M.part_of(k, parts), 254)


def is_nan(b):
    return (b >> 52) & 0x7ff == 0x7ff and b & ((1 << 52) - 1) != 0


def reverse_in_one_tile(perm, offsets):
    p = next(q for q in range(len(offsets) - 1) if offsets[q + 1] - offsets[q] >= 2)
    lo, hi = offsets[p], min(offsets[p + 1], offsets[p] + E.TILE)
    perm = perm.copy()
    perm[lo:hi] = perm[lo:hi][::-1].copy()
    return perm, offsets


def duplicate_a_row(perm, offsets):
    perm = perm.copy()
    perm[E.TILE // 2] = perm[E.TILE // 2 + 1]
    return perm, offsets


def last_offset_off_by_one(perm, offsets):
    offsets = list(offsets)
    offsets[-2] += 1 if offsets[-2] < offsets[-1] else -1
    return perm, offsets


I64_8 = dict(form="stable", kind="i64", dist="pool", rows=4097, parts=8, payload="utf8")
STABLE_FAULTS = {
    # fault: (the named case that rejects it, fake_stable arguments)
    "part_of from the low 32 bits of the hash": (dict(I64_8, nulls=0.0), dict(part=low_half)),
    "% parts in place of the multiply-shift": (dict(I64_8, nulls=0.0), dict(part=modulo)),
    "NULL keys sent to part_of(0)": (dict(I64_8, nulls=0.1), dict(part=null_as_zero)),
    "Int32 zero-extended": (dict(form="stable", kind="i32", dist="pool", rows=4097, parts=255, payload="utf8"), dict(image=lambda k: k & 0xffffffff)),
    "-0.0 folded onto +0.0": (dict(form="stable", kind="f64", dist="pool", rows=4097, parts=255, payload="key_only"), dict(image=lambda k: 0 if k == 1 << 63 else k)),
    "a NaN payload dropped": (dict(form="stable", kind="f64", dist="pool", rows=4097, parts=255, payload="key_only"),
                              dict(image=lambda k: 0x7ff8000000000000 if is_nan(k) else k)),
    "order inside a partition reversed within one tile": (dict(form="stable", kind="i64", dist="equal", rows=65536 + 4096, parts=8), dict(tweak=reverse_in_one_tile)),
    "one row duplicated over another in a full tile": (dict(form="stable", kind="i64", dist="pool", rows=4096, parts=8, payload="plain"), dict(tweak=duplicate_a_row)),
    "an offset off by one at the last partition": (dict(form="stable", kind="i64", dist="pool", rows=4097, parts=256, payload="full"), dict(tweak=last_offset_off_by_one)),
    "part id 255 merged into 254": (dict(form="stable", kind="i64", dist="pool", rows=65536, parts=256, payload="plain"), dict(part=merged_255)),
}


@pytest.mark.parametrize("fault", STABLE_FAULTS)
def test_planted_fault_in_the_stable_form_is_rejected(fault):
    attrs, plant = STABLE_FAULTS[fault]
    c = one(**attrs)
    M.compare(*fake_stable(c), c.expected, "no fault")           # the fake without a fault passes
    with pytest.raises(AssertionError):
        M.compare(*fake_stable(c, **plant), c.expected, fault)


def test_planted_fault_a_null_mask_row_kept_is_rejected():
    c = one(form="filter", kind="i32", pred_name="nullable")
    M.compare(*fake_filter(c), c.expected, "no fault")
    res = M.X.evaluate(c.pred, c.batch)
    assert None in res.vals
    kept_nulls = np.array([v != 0 for v in res.vals], dtype=bool)     # NULL treated as TRUE
    with pytest.raises(AssertionError):
        M.compare(*fake_filter(c, keep=kept_nulls), c.expected, "a NULL-mask row kept")


def test_planted_fault_overlapping_regions_is_rejected():
    c = one(form="filter", kind="i32", pred_name="nullable")

    def overlap(starts, rows):
        p = next(q for q in range(1, len(rows)) if rows[q] and rows[q - 1])
        return starts[:p] + [starts[p] - 1] + starts[p + 1:]
    M.compare(*fake_filter(c), c.expected, "no fault")
    with pytest.raises(AssertionError, match="overlap"):
        M.compare(*fake_filter(c, starts_edit=overlap), c.expected, "overlapping regions")
    with pytest.raises(AssertionError, match="leaves the batch"):
        M.compare(*fake_filter(c, starts_edit=lambda s, r: s[:-1] + [s[-1] + 1]), c.expected, "a region past the end")


def test_utf8_properties_are_asserted():
    """utf8_partitions reads the assignment off an output and rejects: a string in two partitions, a NULL outside partition 0"""
    c = one(form="stable", kind="utf8", dist="pool", rows=4097, parts=8, payload="utf8", nulls=0.1)
    ids = c.ids
    place = {k: (0 if k is None else (len(k) * 5 + 3) % 8) for k in set(ids)}

    def run(pid_of):
        st = M.stable_from(c.batch, [pid_of(i, k) for i, k in enumerate(ids)], 8)
        got = c.batch.take(pa.array(st.perm, type=pa.int64()))
        pids = M.utf8_partitions(got.column(c.kcol), st.offsets, ids, 8)
        M.compare(got, st.offsets, M.stable_from(c.batch, pids, 8), "utf8")
    run(lambda i, k: place[k])
    with pytest.raises(AssertionError, match="NULL keys"):
        run(lambda i, k: 1 if k is None else place[k])
    with pytest.raises(AssertionError, match="is in partitions"):
        run(lambda i, k: (place[k] + (i % 2)) % 8 if k == b"a" else place[k])


# ---- the case library is what it claims ------------------------------------------------------------------------------------------
def test_every_row_count_and_part_count_occurs():
    for form in ("stable", "filter"):
        cs = [c for c in E.all_cases().values() if c.form == form]
        assert {c.rows for c in cs} >= set(E.ROWS), form
        assert {c.parts for c in cs} >= set(E.PARTS), form
        assert max(c.rows for c in cs) <= 2 ** 17 + 67
    kinds = {c.kind for c in E.all_cases().values()}
    assert kinds == set(E.COLUMN_KIND)
    assert {c.nulls for c in E.all_cases().values()} == {0.0, 0.1, 1.0}
    assert {c.mem_in for c in E.all_cases().values()} == {"device", "host", "slice"}
    for c in E.all_cases().values():
        if c.mem_in == "slice" and c.rows:
            assert all(col.offset == 3 for col in c.batch.columns), c.name


@pytest.mark.parametrize("name", [n for n, c in E.all_cases().items() if c.dist in ("few", "ends") and E.COLUMN_KIND[c.kind] != "utf8"])
def test_few_and_ends_cases_place_their_keys_as_claimed(name):
    c = E.case(name)
    pids = M.partitions([k for k in c.ids if k is not None], c.parts)
    hit = set(pids)
    if c.dist == "ends":
        assert hit == {0, c.parts - 1}, (name, sorted(hit))
    else:
        assert not hit & {0, c.parts // 2, c.parts - 1} and 0 < len(hit) < c.parts, (name, sorted(hit))
        assert len(set(k for k in c.ids if k is not None)) > len(hit)       # (several keys per occupied partition)


def col_op_const_over_plain_column(c) -> bool:
    e = c.pred
    if e is None:
        return True
    if not (isinstance(e, BinaryOp) and isinstance(e.left, InputRef) and isinstance(e.right, Constant) and e.op in (">", "<", ">=", "<=", "=", "!=")):
        return False
    col = c.batch.column(e.left.index)
    return col.type in (pa.int64(), pa.float64()) and col.null_count == 0 and abi.dtype_of(col.type) == e.right.dtype and e.right.value is not None


def fast_conditions(c) -> dict:
    """the conditions of the fast routes, restated from the header and partition.hip's comments"""
    b = c.batch
    conds = {
        "rows >= 65536": c.rows >= 65536,
        "1 to 3 columns, all 8 bytes wide and NULL-free": 1 <= b.num_columns <= 3 and all(
            col.type in (pa.int64(), pa.float64()) and col.null_count == 0 for col in b.columns),
    }
    if c.form == "stable":
        conds["the key is a bare reference to an Int64 / Float64 column"] = c.kind in ("i64", "f64")
        conds["parts > 1"] = c.parts > 1
    else:
        conds["the key is a bare reference to an Int64 column"] = c.kind == "i64"
        conds["DEVICE output"] = c.mem_out == "device"
        conds["no predicate, or col OP const over a NULL-free Int64 / Float64 column"] = col_op_const_over_plain_column(c)
    return conds


@pytest.mark.parametrize("name", E.all_cases())
def test_cases_fulfil_or_break_the_fast_route_conditions(name):
    c = E.case(name)
    conds = fast_conditions(c)
    if c.route in ("fast", "fused"):
        assert all(conds.values()), (name, [k for k, v in conds.items() if not v])
    else:
        assert c.route in ("general", "composed") and not all(conds.values()), name


def test_routes_and_kinds_are_all_covered():
    cs = list(E.all_cases().values())
    assert {(c.form, c.route) for c in cs} == {("stable", "fast"), ("stable", "general"), ("filter", "fused"), ("filter", "composed")}
    fused = [c for c in cs if c.route == "fused"]
    assert {c.pred_name for c in fused} == {"none", "key", "carried", "other", "none_pass", "all_pass"}
    assert {c.pred_name for c in cs if c.route == "composed"} >= {"and", "nullable", "carried", "none", "key", "none_pass"}
    assert {(c.ncols, c.kcol) for c in cs if c.route == "fast"} >= {(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)}
    assert {c.kind for c in cs if c.route == "fast"} == {"i64", "f64"}
    for c in fused:
        if c.parts == 256:
            assert c.ncols <= 2, c.name      # (the regions take parts x rows x 8 x columns bytes)
        if c.pred_name == "none_pass":
            assert not c.keep.any()
        if c.pred_name == "all_pass":
            assert c.keep.all()
        if c.pred_name in ("key", "carried", "other"):
            assert 0.1 < c.keep.mean() < 0.9, (c.name, c.keep.mean())
    # every boundary case that divides fast from general sits on both sides of 65536 rows
    assert {c.rows for c in cs if c.route == "fast"} >= {65536, 65537} and 65535 in {c.rows for c in cs if c.route == "general"}
