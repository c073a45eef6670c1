"""The model of row movement (tests/move_model.py) and its case library (tests/move_edge_cases.py), without a GPU:

* the model against pyarrow, an implementation nobody here wrote — take / filter / concat_arrays / slice on every case, by bit
  pattern;
* the model against the CPU oracle backend for Limit, CrossJoin, SimpleAgg, Project, Filter and the text form on every case of
  those families: a three-way agreement before any GPU is involved;
* `text_form` pinned to the tables of tests/golden/reference_goldens.json and to the literals of
  test_hip_text_form_matches_oracle;
* thirteen planted faults, each built from the model with one defect and each rejected by `compare` on a named case;
* the case library against what it claims."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest

import move_edge_cases as E
import move_model as M
from sqlrs_amd import abi
from sqlrs_amd.executor import CrossJoinExecutor, FilterExecutor, ProjectExecutor, SimpleAggExecutor
from sqlrs_amd.expr import InputRef

ALL = list(E.all_cases())


def model_batches(c):
    """the model batches a case is made of"""
    if c.family == "a":
        return c.parts
    if c.family == "b":
        return c.batches
    if c.family == "c":
        return c.left + c.right
    if c.family == "f":
        return c.batches
    if c.family == "h":
        return [c.base]
    return [c.batch]


# ---- the model against pyarrow ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_model_equals_pyarrow(name):
    """take <-> Array.take, keep <-> filter, concat <-> concat_arrays, slice <-> Array.slice; compared by bit pattern"""
    c = E.case(name)
    batches = [b for b in model_batches(c) if b]
    if not batches:
        return
    rng = np.random.default_rng(len(name))
    whole = M.concat_batches(batches)
    arrays = [[M.to_arrow(col) for col in b] for b in batches]
    M.compare([pa.concat_arrays([a[k] for a in arrays]) for k in range(len(whole))], whole, f"{name}: concat")
    n = M.rows(whole)
    src = [pa.concat_arrays([a[k] for a in arrays]) for k in range(len(whole))]
    if n == 0:
        M.compare([a.slice(0, 0) for a in src], M.slice_batch(whole, 0, 0), f"{name}: empty slice")
        return
    m = min(n, 700)
    idx = [None if z else int(i) for i, z in zip(rng.integers(0, n, m), rng.random(m) < 0.1)]
    idx[-1] = n - 1
    M.compare([a.take(pa.array(idx, type=pa.int64())) for a in src], M.take_batch(whole, idx), f"{name}: take")
    mask = [None if z else bool(v) for v, z in zip(rng.integers(0, 2, n), rng.random(n) < 0.1)]
    M.compare([a.filter(pa.array(mask, type=pa.bool_()), null_selection_behavior="drop") for a in src], M.keep_batch(whole, mask), f"{name}: keep")
    lo = int(rng.integers(0, n))
    ln = int(rng.integers(0, n - lo + 1))
    M.compare([a.slice(lo, ln) for a in src], M.slice_batch(whole, lo, ln), f"{name}: slice")


# ---- the model against the oracle ---------------------------------------------------------------------------------------------------
def host(batch, mode="n10", names=None):
    return E.arrow_of(batch, mode, names or [f"c{i}" for i in range(len(batch))])


@pytest.mark.parametrize("name", E.names(family="b", form="host"))
def test_limit_model_equals_oracle(oracle, name):
    c = E.case(name)
    outs, pulled = E.limit_run(oracle, [host(b, c.batch_mode(k)) for k, b in enumerate(c.batches)], c.limit, c.offset)
    M.compare_limit(outs, pulled, c.expected, name)


@pytest.mark.parametrize("name", E.names(family="c", per_call="whole"))
def test_cross_join_model_equals_oracle(oracle, name):
    c = E.case(name)
    got = list(CrossJoinExecutor(oracle, [host(b) for b in c.left], [host(b) for b in c.right], E.product_schema()).execute())
    M.compare_stream(got, c.expected, name)


@pytest.mark.parametrize("name", E.names(family="a", via="cross", form="host"))
def test_concat_model_equals_oracle(oracle, name):
    """the oracle's cross join over the parts and a one-row right batch: its left columns are the concatenation"""
    c = E.case(name)
    one = E.palette(77, 1, "none")
    got = list(CrossJoinExecutor(oracle, [host(b, c.part_mode(k)) for k, b in enumerate(c.parts)], [host(one, "none")], E.product_schema()).execute())
    whole = pa.Table.from_batches(got).combine_chunks().to_batches()[0] if got else None
    if M.rows(c.expected) == 0:
        assert whole is None
        return
    M.compare(whole.columns[:6], c.expected, name)


@pytest.mark.parametrize("name", E.names(family="f"))
def test_simple_agg_model_equals_oracle(oracle, name):
    c = E.case(name)
    child = [host(b, c.mode, E.AGG_COLS) for b in c.batches]
    if c.shape == "nobatch":
        with pytest.raises(abi.ExecutorError):
            list(SimpleAggExecutor(oracle, E.agg_funcs(), child).execute())
        with pytest.raises(M.NoInput):
            M.simple_agg([], E.agg_list())
        return
    (got,) = list(SimpleAggExecutor(oracle, E.agg_funcs(), child).execute())
    M.compare(got, c.expected, name)


@pytest.mark.parametrize("name", E.names(family="d", form="host"))
def test_project_model_equals_oracle(oracle, name):
    c = E.case(name)
    (got,) = list(ProjectExecutor(oracle, c.exprs, [host(c.batch, c.mode)]).execute())
    M.compare(got, c.expected, name)


@pytest.mark.parametrize("name", E.names(family="e"))
def test_filter_model_equals_oracle(oracle, name):
    c = E.case(name)
    (got,) = list(FilterExecutor(oracle, InputRef(0), [host(c.batch)]).execute())
    M.compare(got, c.expected, name)


@pytest.mark.parametrize("name", E.names(family="g"))
def test_text_form_model_equals_oracle(oracle, name):
    c = E.case(name)
    M.compare_text(oracle.batch_to_string(host(c.batch)), c.expected, name)


def test_text_form_of_every_other_family_equals_oracle(oracle):
    for name in ("b-nowhere-host", "d-n65-host", "h-slice-o0-lend", "a-cross-off33-host"):
        b = model_batches(E.case(name))[0]
        M.compare_text(oracle.batch_to_string(host(b)), M.text_form(b), name)


# ---- text_form pins -----------------------------------------------------------------------------------------------------------------
def test_text_form_pins():
    """the tables of the reference goldens in the reference's text form, and the literals of test_hip_text_form_matches_oracle"""
    import golden_runner as G
    fx = G.load()
    seen = 0
    for tname, tdef in fx["tables"].items():
        for rb, rows in zip(G.table_batches(tdef), tdef["batches"]):
            typed = [[(float(v) if t == "float64" and v is not None else v) for v, (_, t) in zip(r, tdef["schema"])] for r in rows]
            assert M.text_form(M.batch_from_arrow(rb)) == G.render_rows(typed), tname
            seen += len(rows)
    assert seen > 40
    b = pa.RecordBatch.from_arrays([
        pa.array([12000.0, 0.1, 1e21, 1e-7, -0.0, 1100.2, None, float("inf"), float("nan"), 2.5e-320]),
        pa.array([1, -2, None, 4, 5, 6, 7, 8, 9, 1 << 62], type=pa.int64()),
        pa.array(["x", "", None, "a b", "é", "f", "g", "h", "i", "j"]),
        pa.array([True, False, None, True, True, False, False, True, None, True]),
        pa.array([1, 2, 3, None, 5, 6, 7, 8, 9, -10], type=pa.int32())], names=list("abcde"))
    lines = M.text_form(M.batch_from_arrow(b)).splitlines()
    assert lines[0] == "12000 1 x true 1" and lines[1] == "0.1 -2 (empty) false 2"
    assert lines[2] == "1000000000000000000000 NULL NULL NULL 3"
    assert lines[3] == "0.0000001 4 a b true NULL" and lines[4] == "-0 5 é true 5" and lines[5].startswith("1100.2 6 f")
    assert lines[6].startswith("NULL ") and lines[7].startswith("inf ") and lines[8].startswith("NaN ")
    assert lines[9] == "0." + "0" * 319 + "25 4611686018427387904 j true -10"
    assert M.f64_text(E.F64_BITS["-inf"]) == "-inf" and M.f64_text(E.F64_BITS["-nan_payload"]) == "NaN"
    assert M.f64_text(E.F64_BITS["max"]) == "17976931348623157" + "0" * 292 and M.f64_text(1) == "0." + "0" * 323 + "5"


# ---- planted faults -----------------------------------------------------------------------------------------------------------------
def arrow(batch):
    return [M.to_arrow(c) for c in batch]


def utf8_array(offsets, data: bytes, valid):
    n = len(valid)
    bits = np.packbits(np.array(valid, dtype=np.uint8), bitorder="little").tobytes() + b"\0" * 8
    nulls = n - int(sum(valid))
    return pa.Array.from_buffers(pa.string(), n, [pa.py_buffer(bits) if nulls else None, pa.py_buffer(np.array(offsets, dtype=np.int32).tobytes()),
                                                  pa.py_buffer(data)], null_count=nulls)


def rejected(got, expected, fault):
    with pytest.raises(AssertionError):
        M.compare(got, expected, fault)


def test_fault_concat_carry_bit_dropped():
    """append_bits without the carry into the next word: of a part appended at bit offset 33, the rows that cross a word boundary lose
    their validity bit"""
    c = E.case("a-cross-off33-host")
    M.compare(arrow(c.expected), c.expected, "no fault")
    cells = list(c.expected[0].cells)
    hit = 0
    at = 0
    for ln in c.plan:
        sh = at & 63
        for i in range(ln):
            if sh and (i & 63) >= 64 - sh and cells[at + i] is not None:  # (the bits of source word i / 64 that belong to the next word)
                cells[at + i] = None
                hit += 1
        at += ln
    assert hit > 10
    rejected(arrow([M.Col(M.I64, cells)] + c.expected[1:]), c.expected, "carry dropped")


def test_fault_non_nullable_part_as_all_zeros():
    c = E.case("a-cross-off1-host")
    cols, at = [list(col.cells) for col in c.expected], 0
    assert any(c.part_mode(k) == "none" and ln for k, ln in enumerate(c.plan)) and any(col.nulls for col in c.expected)
    for k, ln in enumerate(c.plan):
        if c.part_mode(k) == "none":
            for cells in cols[:5]:
                cells[at:at + ln] = [None] * ln
        at += ln
    rejected(arrow([M.Col(e.dtype, cells) for e, cells in zip(c.expected, cols)]), c.expected, "all zeros")


def test_fault_boolean_gathered_from_validity():
    c = E.case("b-bit1-host")
    exp = c.expected[0][0]
    fake = [M.Col(col.dtype, [None if v is None else True for v in col.cells]) if col.dtype == M.BOOL else col for col in exp]
    M.compare(arrow(exp), exp, "no fault")
    rejected(arrow(fake), exp, "values from validity")


def test_fault_last_ballot_word_missing():
    """n a multiple of 64 and the guard `(i & ~63) <= n - 64` off by one word: the last validity word is never written (zeros)"""
    c = E.case("d-n64-host")
    assert M.rows(c.expected) % 64 == 0
    fake = [M.Col(col.dtype, col.cells[:-64] + [None] * 64) for col in c.expected]
    rejected(arrow(fake), c.expected, "last word missing")


def test_fault_take_clamps_the_last_index():
    c = E.case("b-bit63-host")
    exp = c.expected[0][0]
    fake = [M.Col(col.dtype, col.cells[:-1] + [col.cells[-2]]) for col in exp]
    rejected(arrow(fake), exp, "last index clamped")


def test_fault_utf8_null_row_with_bytes():
    c = E.case("d-n64-host")
    col = c.expected[0]
    assert col.dtype == M.UTF8 and col.nulls
    valid = [v is not None for v in col.cells]
    strings = [b"?" if v is None else v for v in col.cells]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in strings])])
    M.compare([utf8_array(np.concatenate([[0], np.cumsum([len(v or b"") for v in col.cells])]), b"".join(v or b"" for v in col.cells), valid)], [col], "no fault")
    rejected([utf8_array(offs, b"".join(strings), valid)], [col], "NULL row with a byte")


def windowed_utf8_concat(parts, leads, buggy):
    """the Utf8 column of `parts` concatenated the way concat_columns lays it out when part k arrives as a window whose offsets start
    at leads[k] > 0 and whose data_bytes include the bytes below: with `buggy`, dst[roff] = offsets[0] + boff is written over the
    terminal offset of the part in front"""
    data, offs, valid = b"", [0], []
    for col, lead in zip(parts, leads):
        boff = len(data)
        data += b"L" * lead
        if buggy:
            offs[-1] = boff + lead          # the part's offsets[0], re-based, overwrites the previous terminal offset
        at = boff + lead
        for v in col.cells:
            at += len(v or b"")
            offs.append(at)
            data += v or b""
            valid.append(v is not None)
    return utf8_array(offs, data, valid)


def test_fault_utf8_predecessor_extended_by_offsets0():
    """the suspect of the issue: the last string of the part in front grows by offsets[0] bytes (and offsets[0] of the result is not 0)"""
    c = E.case("a-cross-off33-window")
    parts = [p[4] for p in c.parts]
    exp = [c.expected[4]]
    M.compare([windowed_utf8_concat(parts, [0] * len(parts), False)], exp, "no fault")
    rejected([windowed_utf8_concat(parts, [17] * len(parts), True)], exp, "predecessor extended")
    rejected([windowed_utf8_concat(parts, [0] + [17] * (len(parts) - 1), True)], exp, "predecessor extended, first part at 0")


def test_fault_slice_starts_one_row_late():
    c = E.case("b-bit1-host")
    exp = c.expected[0][0]
    src = c.batches[4]
    M.compare(arrow(M.slice_batch(src, 1, 100)), exp, "no fault")
    rejected(arrow(M.slice_batch(src, 2, 100)), exp, "one row late")


def test_fault_limit_stops_one_batch_late():
    c = E.case("b-inside_first-host")
    outs, pulled = c.expected
    M.compare_limit([arrow(b) for b in outs], pulled, c.expected, "no fault")
    with pytest.raises(AssertionError, match="pulled"):
        M.compare_limit([arrow(b) for b in outs], pulled + 1, c.expected, "one batch late")


def test_fault_cross_join_right_major():
    c = E.case("c-L3-R65-whole")
    exp = c.expected[:3]                                   # the outputs of the first right batch: one per left row
    whole = M.concat_batches(exp)
    L, R = 3, 65
    perm = [(k % L) * R + k // L for k in range(L * R)]    # row k = (left k % L, right k / L)
    fake = M.take_batch(whole, perm)
    got = [arrow(M.slice_batch(fake, i * R, R)) for i in range(L)]
    M.compare_stream([arrow(b) for b in exp], exp, "no fault")
    with pytest.raises(AssertionError):
        M.compare_stream(got, exp, "right-major")


def test_fault_nan_payload_canonicalised():
    c = E.case("d-n4097-host")
    col = c.expected[1]
    assert col.dtype == M.F64
    canon = [0x7ff8 << 48 if (v is not None and v & (0x7ff << 52) == 0x7ff << 52 and v & ((1 << 52) - 1)) else v for v in col.cells]
    assert canon != col.cells
    rejected([M.to_arrow(M.Col(M.F64, canon))], [col], "NaN canonicalised")


def test_fault_negative_zero_rendered_as_zero():
    c = E.case("g-edge")
    M.compare_text(c.expected, c.expected, "no fault")
    assert "\n-0 " in c.expected
    with pytest.raises(AssertionError, match="line 5"):
        M.compare_text(c.expected.replace("\n-0 ", "\n0 "), c.expected, "-0.0 as 0")


def test_fault_null_count_off_by_one():
    c = E.case("d-n64-host")
    col = c.expected[2]
    a = M.to_arrow(col)
    assert col.nulls > 0
    M.compare([a], [col], "no fault")
    rejected([pa.Array.from_buffers(a.type, len(a), a.buffers(), null_count=col.nulls + 1)], [col], "null_count + 1")
    rejected([pa.Array.from_buffers(a.type, len(a), a.buffers(), null_count=col.nulls - 1)], [col], "null_count - 1")


def test_compare_reads_bits_not_values():
    """-0.0 against +0.0, a sign-flipped NaN, offsets[0] != 0 and a wrong type are all differences"""
    z = M.Col(M.F64, [0, 1 << 63, E.F64_BITS["nan"]])
    M.compare([M.to_arrow(z)], [z])
    rejected([M.to_arrow(M.Col(M.F64, [1 << 63, 1 << 63, E.F64_BITS["nan"]]))], [z], "sign of zero")
    rejected([M.to_arrow(M.Col(M.F64, [0, 1 << 63, E.F64_BITS["-nan"]]))], [z], "sign of NaN")
    s = M.Col(M.UTF8, [b"ab", b""])
    rejected([utf8_array([1, 3, 3], b"xab", [True, True])], [s], "offsets[0] = 1")
    rejected([M.to_arrow(M.Col(M.I64, [1]))], [M.Col(M.I32, [1])], "type")


# ---- the library against its claims ---------------------------------------------------------------------------------------------------
def test_every_concat_position_occurs():
    seen = set()
    for n in E.names(family="a"):
        seen |= set(E.concat_positions(E.case(n).plan))
    want = {(o, ln) for o in E.CONCAT_OFFS for ln in E.CONCAT_LENS}
    assert want <= seen, sorted(want - seen)
    for form in ("host", "owned", "lent", "window"):
        got = set()
        for n in E.names(family="a", via="cross", form=form):
            got |= set(E.concat_positions(E.case(n).plan))
        assert want <= got, form
    firsts = [E.case(n).plan for n in E.names(family="a")]
    assert any(p[0] == 0 for p in firsts) and any(p[-1] == 0 for p in firsts) and any(0 in p[1:-1] for p in firsts)
    # nullable and non-nullable parts alternate: a part without NULLs sits beside one with NULLs in every cross case
    for n in E.names(family="a", via="cross"):
        c = E.case(n)
        kinds = [c.parts[k][0].nulls > 0 for k, ln in enumerate(c.plan) if ln > 1]
        assert True in kinds and False in kinds, n


def test_every_dtype_occurs_in_every_family():
    for fam in "abcdefgh":
        dts = set()
        for n in E.names(family=fam):
            c = E.case(n)
            if fam == "f" and c.shape == "nobatch":
                continue
            for b in model_batches(c):
                dts |= {col.dtype for col in b}
        assert dts >= {M.I32, M.I64, M.F64, M.BOOL, M.UTF8} or (fam == "f" and dts >= {M.I32, M.I64, M.F64, M.UTF8}), (fam, dts)


def test_every_row_count_and_null_mode_occurs():
    sizes, nulls = set(), set()
    for c in E.all_cases().values():
        if c.family == "f" and c.shape == "nobatch":
            continue
        for b in model_batches(c):
            sizes.add(M.rows(b))
            assert M.rows(b) <= E.MAX_ROWS, c.name
            for col in b[:5]:
                if len(col):
                    nulls.add("all" if col.nulls == len(col) else "some" if col.nulls else "none")
        if c.family == "b":
            for out in c.expected[0]:
                sizes.add(M.rows(out))
    assert nulls == {"all", "some", "none"}
    assert set(E.ROW_COUNTS) <= sizes, sorted(set(E.ROW_COUNTS) - sizes)    # (255 .. 2049: the lengths of a Limit's gather)
    assert E.POOL_F64 and all(v in {x for c in E.all_cases().values() if c.family == "d" for x in c.batch[2].cells} for v in E.POOL_F64)
    long_rows = [v for c in E.all_cases().values() if c.family == "d" for v in c.batch[4].cells if v is not None and len(v) == 300]
    assert long_rows


def test_arrow_slices_cover_the_grid():
    got = {(E.case(n).offset, E.case(n).length) for n in E.names(family="h", kind="slice")}
    assert got == {(o, ln) for o in E.ARROW_OFFSETS for ln in E.ARROW_LENGTHS}
    assert {E.case(n).kind for n in E.names(family="h")} == {"slice", "null_count_unknown", "validity_no_nulls", "all_empty", "struct_slice"}
    c = E.case("h-all_empty_utf8")
    assert all(v in (None, b"") for v in c.base[4].cells)
    assert all(col.nulls == 0 for col in E.case("h-validity_no_nulls").base)


def test_what_pyarrow_exports_for_a_struct_slice():
    """recorded: a sliced StructArray exports its offset at the struct level (children unsliced) or in the children; either way the
    rows it describes are rows [offset, offset + length) of the base batch"""
    c = E.case("h-struct_slice")
    rb = E.arrow_of(c.base)
    st = pa.StructArray.from_arrays(rb.columns, names=rb.schema.names).slice(c.offset, c.length)
    arr, sch = abi.ArrowArrayC(), abi.ArrowSchemaC()
    st._export_to_c(C.addressof(arr), C.addressof(sch))
    try:
        child_offsets = {arr.children[i].contents.offset for i in range(arr.n_children)}
        print(f"pyarrow {pa.__version__}: struct offset {arr.offset}, child offsets {sorted(child_offsets)}, length {arr.length}")
        assert arr.length == c.length and arr.n_children == 6
        assert {arr.offset + o for o in child_offsets} == {c.offset}
    finally:
        back = pa.Array._import_from_c(C.addressof(arr), C.addressof(sch))
    M.compare([back.field(i) for i in range(6)], c.expected, "struct slice, round trip through pyarrow")


def test_window_margins_make_offsets0_positive():
    b = E.palette(3, 65, "n10")
    big = E.with_margins(3, b)
    assert M.rows(big) == E.WINDOW_LEAD + 65 + E.WINDOW_TAIL and E.WINDOW_LEAD % 64 == 0
    assert sum(len(v or b"") for v in big[4].cells[:E.WINDOW_LEAD]) > 0
    M.compare(arrow(M.slice_batch(big, E.WINDOW_LEAD, 65)), b, "window")
