"""Every device route of the aggregates against the independent edge-value model (tests/agg_model.py) on the cases of
tests/agg_edge_cases.py: NaNs of both signs and several payloads, infinities, -0.0, subnormals, INT64_MIN / INT64_MAX / -1,
int64 sums that wrap, all-NULL groups, groups of one repeated edge value, hot groups made of the value whose ordered image
is an accumulator's neutral start.  Keys, group order, validity, COUNT, integer SUM / MIN / MAX and MIN / MAX(f64) are compared
bit for bit, SUM(f64) by class or inside the any-order bound gamma_{m+1} * sum|x| (agg_model); the CPU file asserts that at
most a tenth of every case's SUM(f64) groups is compared by class.

Which route ran is asserted, not assumed: every run sits in a `route(...)` block over the counters of sqlrs_ctx_profile_read
("Route witnesses of the aggregates"; every `agg_*` counter a run does not name must stay at rest):

  lds_agg / agg_update                       profile scopes: bucket passes of the partition route / updates of the row route
  agg_part_dense / _slim_runs / _slim_blk / _probe_spec / _probe_generic       the kernel family of a bucket pass
  agg_part_interpreted                       a dense / slim pass that interprets its accumulator list per row
  agg_part_packed / _unpacked, _flags, _rec, _in_place, _join, _join_mult, _split, _overflow_rows
  agg_merge_groups, agg_pending_deferred, agg_wide_parts                        operator state (hashagg_op.hip)

Forms are steered with the hooks the library reads per call (monkeypatch.setenv): SQLRS_DENSE_AGG, SQLRS_RP_CLAIM,
SQLRS_RP_SLIM, SQLRS_RP_REC, SQLRS_AGG_SEG, SQLRS_RP_SLIM_DELTA, SQLRS_RP_CHUNK_WGS (and SQLRS_AGG_SPLIT, read per operator).

The segmented mode of the slim bucket pass is decided inside the kernel: test_segmented_mode_over_sorted_keys states the
condition and asserts the one part of it a counter shows (the run-list form).

What no input of <= 2^22 rows reaches inside this process, and the condition in the source that keeps it out:

* accumulator signatures (SUM_F64, COUNT) and (SUM_I64, COUNT) of the dispatch (agg_partition.hip, SQ_SIG2): agg_consume puts
  the COUNT cells of every column in front of the other cells (hashagg_op.hip, "a COUNT cell per column ..."), so `SUM(x),
  COUNT(x)` runs the (COUNT, SUM) kernel with the output columns swapped — both orders are run here and show the same counter;
* the one-cell forms of lds_agg_dense_slim_kernel (SUM_F64 alone, COUNT alone): slim rows need a bucket table of <= 2^12 slots
  (radix_part.hip: `kp.rbits + SLIM_LOCAL_BITS + 7 <= 32`), and a list of one cell is given 2^13 slots of 12 bytes
  (agg_partition.hip: `while (rbits < 14 && (2 << rbits) * dslot <= dense_budget)`) unless its key range is below 2^12, which is a
  single bucket that neither the claimed level (P >= 2) nor two levels (P > 512) take.  Such lists are run through both steered
  forms here and show `agg_part_dense`;
* `merge_groups` of a second pre-aggregated batch and the `track_nn` back-fill for groups created before the first NULL:
  pushed batches are staged and aggregated as ONE batch at finish (hashagg_op.hip: STAGE_DIRECT_ROWS 2^26, STAGE_FLUSH_ROWS
  2^28, read once per process), so a 2^21-row batch followed by a 1 000-row batch is one partition pass whose groups stay
  `pending` (asserted: agg_pending_deferred 1, agg_merge_groups 0).  They stay with the `without_staging` / `early_flushes`
  child re-runs of test_gpu_parity.py / test_gpu_fuzz.py;
* keys outside an optimistically sampled range (KeyPack::oob, the retry with exact statistics): `sampled` needs n >= 2^24
  (agg_partition.hip estimate_distinct).  A key set too large for the estimate IS built without SQLRS_EST_SCALE: at 2^22 rows the
  statistics hash two of every eight 64-row groups, and test_key_set_too_large_for_the_estimate hides 199 000 of 200 000 groups
  from them — overflow rows through the row route and `merge_groups` with pre-aggregated weights.  Every other run asserts
  agg_part_overflow_rows 0 and agg_merge_groups 0;
* the fused join and the eager route below 2^16 probe rows (hashagg_op.hip: `right->num_rows >= (1ll << 16)`): 300 build keys x
  5 000 probe rows take the composed route (asserted), so the fused cases run 70 001 probe rows as well.

DISTINCT runs over the int64 pool only (wrapping SUM included); whether +-0.0 and NaN payloads count as distinct values is
left to the oracle comparison of test_gpu_parity.py."""
import ctypes as C
from contextlib import contextmanager

import numpy as np
import pyarrow as pa
import pytest

import agg_edge_cases as E
import agg_model as M
from sqlrs_amd.executor import HashAggExecutor, HashJoinAggExecutor, SimpleAggExecutor
from sqlrs_amd.expr import InputRef, JoinCondition

pytestmark = pytest.mark.gpu

HOOKS = ("SQLRS_DENSE_AGG", "SQLRS_RP_CLAIM", "SQLRS_RP_SLIM", "SQLRS_RP_REC", "SQLRS_AGG_SEG", "SQLRS_RP_SLIM_DELTA",
         "SQLRS_RP_CHUNK_WGS", "SQLRS_AGG_SPLIT")
AGG_COUNTERS = ("agg_part_dense", "agg_part_slim_runs", "agg_part_slim_blk", "agg_part_probe_spec", "agg_part_probe_generic",
                "agg_part_interpreted", "agg_part_packed", "agg_part_unpacked", "agg_part_flags", "agg_part_rec",
                "agg_part_in_place", "agg_part_join", "agg_part_join_mult", "agg_part_split", "agg_part_overflow_rows",
                "agg_merge_groups", "agg_pending_deferred", "agg_wide_parts")


# ---- which route ran ---------------------------------------------------------------------------------------------------------
def counters(be) -> dict:
    cap = 512
    names, ms, n_l = (C.c_char_p * cap)(), (C.c_double * cap)(), (C.c_int64 * cap)()
    n = be.fn("ctx_profile_read")(be.ctx, cap, names, ms, n_l)
    assert n <= cap
    return {names[k].decode(): n_l[k] for k in range(n)}


@contextmanager
def route(be, label, lds_agg=0, row_route=False, free=(), moves=(), **exactly):
    """asserts how the witnesses move across the block: `lds_agg` bucket passes exactly, the row route's `agg_update` at rest
    unless `row_route` (None: not looked at), every agg_* counter exactly as named (without its agg_ prefix) and at rest otherwise; the names in
    `free` are not looked at, those in `moves` must move"""
    before = counters(be)
    yield
    after = counters(be)
    moved = {k: after.get(k, 0) - before.get(k, 0) for k in set(after) | set(before)}
    seen = {k: v for k, v in moved.items() if v and (k.startswith("agg_") or k == "lds_agg")}
    want = {k: exactly.get(k[4:], 0) for k in AGG_COUNTERS}
    assert not set(exactly) - {k[4:] for k in AGG_COUNTERS}, exactly
    want["lds_agg"] = lds_agg
    for k, by in want.items():
        if k[4:] in moves:
            assert moved.get(k, 0) > 0, f"{label}: {k} at rest; moved: {seen}"
        elif k[4:] not in free:
            assert moved.get(k, 0) == by, f"{label}: {k} moved by {moved.get(k, 0)}, expected {by}; moved: {seen}"
    assert row_route is None or (moved.get("agg_update", 0) > 0) == row_route, f"{label}: agg_update moved by {moved.get('agg_update', 0)}; moved: {seen}"


@pytest.fixture(scope="module")
def hip():
    """a ctx of this module's own (stream, pool, profile): the profile entries and route counts these ~700 runs leave behind
    stay out of the session's shared ctx, whose profile other modules read by entry name"""
    import sqlrs_amd
    be = sqlrs_amd.new_ctx(0)
    yield be
    be.close()


@pytest.fixture(autouse=True)
def profiled(hip, monkeypatch):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    hip.profile(True)
    yield
    hip.profile(False)


def table_of(batches):
    batches = [b for b in batches if b is not None]
    return pa.Table.from_batches(batches) if batches else None


def run_hash_agg(hip, monkeypatch, case, funcs, env=None, label="", **routes):
    """HashAggExecutor(hip) over the case's batches inside a route block, compared with the model; returns the output table"""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    label = f"{case.name} {' '.join(f'{f}({c})' for f, c in funcs)} {env or ''} {label}"
    exp = case.model(funcs)
    with route(hip, label, **routes):
        got = table_of(HashAggExecutor(hip, E.agg_funcs(funcs), [InputRef(0)], case.batches()).execute())
    M.compare(got, exp, label)
    for k in (env or {}):
        monkeypatch.delenv(k)
    return got


# ---- the accumulator cells of a list, as agg_consume lays them out -----------------------------------------------------------------
def cells_of(funcs, nullable=False):
    """kinds in cell order: a COUNT cell per column that is counted or nullable first, then one per SUM / MIN / MAX"""
    cols = []
    for _, c in funcs:
        if c not in cols:
            cols.append(c)
    cells = [("count", c) for c in cols if nullable or ("count", c) in funcs]
    return cells + [(f, c) for f, c in funcs if f != "count"]


def kind_of(cell):
    f, c = cell
    return f if f == "count" else f + ("_f64" if c in "fg" else "_i64")


NAMED = [("count",), ("sum_i64",), ("sum_f64",), ("min_i64",), ("min_f64",), ("max_i64",), ("max_f64",),
         ("count", "sum_f64"), ("sum_f64", "count"), ("count", "sum_i64"), ("sum_i64", "count"), ("min_f64", "max_f64"), ("min_i64", "max_i64")]
NAMED_SLIM = [("count", "sum_f64"), ("sum_f64", "count"), ("sum_f64",), ("count",)]


def specialised(funcs, slim=False, nullable=False):
    return tuple(kind_of(c) for c in cells_of(funcs, nullable)) in (NAMED_SLIM if slim else NAMED)


# the accumulator lists the dispatch names, the orders it cannot see, and lists it interprets
SINGLES = [[("count", "f")], [("sum", "i")], [("sum", "f")], [("min", "i")], [("min", "f")], [("max", "i")], [("max", "f")]]
PAIRS = [[("count", "f"), ("sum", "f")], [("sum", "f"), ("count", "f")], [("count", "i"), ("sum", "i")], [("sum", "i"), ("count", "i")],
         [("min", "f"), ("max", "f")], [("min", "i"), ("max", "i")]]
GENERIC = [[("sum", "f"), ("min", "f"), ("max", "f")], [("max", "i"), ("min", "i")], [("count", "i"), ("sum", "i"), ("min", "i"), ("max", "i")]]
SIGNATURES = SINGLES + PAIRS + GENERIC
SEVEN = [("count", "f"), ("sum", "f"), ("min", "f"), ("max", "f"), ("sum", "i"), ("min", "i"), ("max", "i")]
ROW_FUNCS = SEVEN + [("count", "j"), ("sum", "j"), ("min", "j"), ("max", "j")]


def sig_id(funcs):
    return "+".join(f"{f}_{c}" for f, c in funcs)


# ---- row route ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batches", ["1_batch", "3_batches"])
@pytest.mark.parametrize("n", E.ROW_SIZES)
def test_row_route(hip, monkeypatch, n, batches):
    """global atomics on dense per-group arrays (agg_update_*, agg_minmax_kernel KIND 0 - 3): the seven accumulators and int32
    SUM / MIN / MAX.  As ONE operator (SQLRS_AGG_SPLIT=0), as the three operators the wide list is planned as (one per argument
    column), and pair by pair; 3 batches: no NULL anywhere in the first, then an all-NULL group and NULLs in old groups (staged:
    the batches are aggregated as one, see the module docstring)"""
    case = E.gpu_case(f"row_{n}" + ("_3_batches" if batches == "3_batches" else ""))
    run_hash_agg(hip, monkeypatch, case, ROW_FUNCS, {"SQLRS_AGG_SPLIT": "0"}, row_route=True)
    run_hash_agg(hip, monkeypatch, case, ROW_FUNCS, row_route=True, wide_parts=3)
    for funcs in ([("min", "f"), ("max", "f")], [("max", "i"), ("min", "i")], [("sum", "f"), ("sum", "i")], [("min", "j"), ("max", "j")]):
        run_hash_agg(hip, monkeypatch, case, funcs, row_route=True)


def test_row_route_without_any_null(hip, monkeypatch):
    """no NULL anywhere: no has-value count is kept (track_nn off), so a group is valid whatever its cell holds — the hot group's
    MIN cell ends on ~0, the accumulator's own start (INT64_MAX / NaN 0x7FFF..F)"""
    case = E.gpu_case("row_plain_4097")
    for funcs in ([("min", "i"), ("max", "i")], [("min", "f"), ("max", "f")], [("sum", "f"), ("sum", "i")]):
        run_hash_agg(hip, monkeypatch, case, funcs, row_route=True)
    run_hash_agg(hip, monkeypatch, case, ROW_FUNCS, {"SQLRS_AGG_SPLIT": "0"}, row_route=True)


# ---- the threshold between the routes ------------------------------------------------------------------------------------------
DENSE_SPLIT = dict(lds_agg=1, part_dense=1, part_packed=1, part_rec=1, part_split=1, pending_deferred=1)


def test_threshold_below_takes_the_row_route(hip, monkeypatch):
    run_hash_agg(hip, monkeypatch, E.gpu_case("threshold_below"), [("count", "f"), ("sum", "f")], row_route=True)


def test_threshold_at_takes_the_partition_route(hip, monkeypatch):
    """2^21 rows: exactly one bucket pass and no row of it on the row route"""
    run_hash_agg(hip, monkeypatch, E.gpu_case("threshold_at"), [("count", "f"), ("sum", "f")], **DENSE_SPLIT)


def test_wide_list_runs_as_three_partition_route_operators(hip, monkeypatch):
    """three argument columns at 2^21 rows: one partition-route operator per column, their columns side by side in the groups'
    first-seen order"""
    funcs = [("sum", "f"), ("sum", "g"), ("count", "f"), ("sum", "i"), ("min", "g"), ("max", "i")]
    routes = {k: 3 * v for k, v in DENSE_SPLIT.items()}
    run_hash_agg(hip, monkeypatch, E.gpu_case("threshold_at"), funcs, wide_parts=3, part_interpreted=2, **routes)  # (SUM + MIN, SUM + MAX: interpreted)
    run_hash_agg(hip, monkeypatch, E.gpu_case("threshold_at"), funcs, {"SQLRS_AGG_SPLIT": "0"}, row_route=True)


# ---- partition route: form x accumulator signature ------------------------------------------------------------------------------
def dense_routes(funcs, **more):
    return dict(DENSE_SPLIT, part_interpreted=0 if specialised(funcs) else 1, **more)


def slim_routes(funcs, form):
    """slim rows need a table of <= 2^12 slots (12 + SLIM_LOCAL_BITS + 7 <= 32 bits of the row word): a list of ONE cell gets 2^13
    slots of 12 bytes and keeps the 16-byte rows of lds_agg_dense_kernel (module docstring)"""
    if len(cells_of(funcs)) < 2:
        return dense_routes(funcs) if form == "blk" else dict(dense_routes(funcs), part_split=0)
    return dict(lds_agg=1, part_packed=1, part_split=int(form == "blk"), pending_deferred=1, part_interpreted=0 if specialised(funcs, slim=True) else 1,
                **{"part_slim_" + form: 1})


def probing_routes(funcs, packed=True, split=False, nullable=False, two_columns=False, **more):
    """(the specialised kernels take one value column without flags)"""
    r = dict(lds_agg=1, pending_deferred=1, part_split=int(split))
    r["part_probe_spec" if specialised(funcs) and not nullable and not two_columns else "part_probe_generic"] = 1
    r["part_packed" if packed else "part_unpacked"] = 1
    if packed:
        r["part_rec"] = 1
    r.update(more)
    return r


@pytest.mark.parametrize("funcs", SIGNATURES, ids=sig_id)
@pytest.mark.parametrize("case_name", ["part_dense", "part_dense_hot"])
def test_partition_route_dense(hip, monkeypatch, case_name, funcs):
    """lds_agg_dense_kernel over packed 16-byte records, every bucket cut into chunks whose tables split_emit_dense_kernel
    merges; `hot`: one key holds 55 % of the rows and only the MAX accumulator's neutral value (wave reductions, the carry),
    and the same rows in column form (SQLRS_RP_REC=0)"""
    case = E.gpu_case(case_name)
    run_hash_agg(hip, monkeypatch, case, funcs, **dense_routes(funcs))
    if case_name == "part_dense_hot":
        run_hash_agg(hip, monkeypatch, case, funcs, {"SQLRS_RP_REC": "0"}, **dense_routes(funcs, part_rec=0))


@pytest.mark.parametrize("funcs", SIGNATURES, ids=sig_id)
def test_partition_route_dense_slim_blk(hip, monkeypatch, funcs):
    """SQLRS_RP_CLAIM=1: the claimed single level hands 12-byte slim rows to lds_agg_dense_slim_kernel (`blk` form); with
    SQLRS_RP_SLIM=0 the claimed level keeps 16-byte records for lds_agg_dense_kernel"""
    case = E.gpu_case("part_dense_hot")
    slim = slim_routes(funcs, "blk")
    run_hash_agg(hip, monkeypatch, case, funcs, {"SQLRS_RP_CLAIM": "1"}, **slim)
    if funcs in (SINGLES[2], PAIRS[0], GENERIC[0]):
        run_hash_agg(hip, monkeypatch, case, funcs, {"SQLRS_RP_CLAIM": "1", "SQLRS_RP_SLIM": "0"}, **dense_routes(funcs))
        run_hash_agg(hip, monkeypatch, case, funcs, {"SQLRS_RP_CLAIM": "1", "SQLRS_RP_SLIM_DELTA": "1", "SQLRS_RP_CHUNK_WGS": "40"}, **slim)


@pytest.mark.parametrize("funcs", SIGNATURES, ids=sig_id)
@pytest.mark.parametrize("case_name,env", [("part_sparse", None), ("part_sparse_hot", None), ("part_dense_hot", {"SQLRS_DENSE_AGG": "0"})])
def test_partition_route_probing_packed(hip, monkeypatch, case_name, env, funcs):
    """lds_agg_kernel, specialised by accumulator signature or generic, over packed records; `hot`: the hot key's bucket is
    cut into chunks that meet in a split table (split_emit_kernel), its value is the MIN (sparse) / MAX (dense keys with
    SQLRS_DENSE_AGG=0) accumulator's neutral start"""
    run_hash_agg(hip, monkeypatch, E.gpu_case(case_name), funcs, env, **probing_routes(funcs, split=case_name.endswith("hot")))


@pytest.mark.parametrize("funcs", SIGNATURES, ids=sig_id)
def test_partition_route_probing_unpacked(hip, monkeypatch, funcs):
    """keys over all of int64 (-1 = the LDS EMPTY pattern, INT64_MIN, INT64_MAX among them): key and row id columns"""
    run_hash_agg(hip, monkeypatch, E.gpu_case("part_full64"), funcs, **probing_routes(funcs, packed=False))


@pytest.mark.parametrize("funcs", [SINGLES[2], SINGLES[5], PAIRS[0], PAIRS[4], GENERIC[2], SEVEN[:4]], ids=sig_id)
def test_partition_route_nullable_flags_form(hip, monkeypatch, funcs):
    """validity that flips every 64 rows, NULL keys, three all-NULL groups, a hot key: rows carry flags, the generic kernel"""
    run_hash_agg(hip, monkeypatch, E.gpu_case("part_nullable"), funcs,
                 **probing_routes(funcs, packed=False, split=True, nullable=True, part_flags=1))


@pytest.mark.parametrize("funcs", [[("sum", "f"), ("sum", "g")], [("min", "f"), ("max", "i")], [("count", "f"), ("sum", "f"), ("sum", "i"), ("max", "i")]], ids=sig_id)
@pytest.mark.parametrize("case_name", ["part_sparse_hot", "part_nullable"])
def test_partition_route_two_argument_columns(hip, monkeypatch, case_name, funcs):
    nullable = case_name == "part_nullable"
    run_hash_agg(hip, monkeypatch, E.gpu_case(case_name), funcs,
                 **probing_routes(funcs, packed=False, split=True, nullable=nullable, two_columns=True, part_flags=int(nullable)))


@pytest.mark.parametrize("funcs", [SINGLES[2], PAIRS[0], PAIRS[5], GENERIC[0]], ids=sig_id)
def test_partition_route_few_groups_in_place(hip, monkeypatch, funcs):
    """24 groups: one bucket, the caller's columns read in place in chunks that merge through a split table"""
    run_hash_agg(hip, monkeypatch, E.gpu_case("part_few_groups"), funcs, **probing_routes(funcs, packed=False, split=True, part_in_place=1))


@pytest.mark.parametrize("funcs", [PAIRS[0], SINGLES[2], PAIRS[4]], ids=sig_id)
def test_sorted_keys_through_the_claimed_slim_level(hip, monkeypatch, funcs):
    """keys arriving sorted through the `blk` form of the slim bucket pass.  That form never enters the segmented mode (`seg_mode`
    has `!BLK`); what SQLRS_AGG_SEG switches here is the per-run add of a hot slot on consecutive lanes (`seg_rows` from the
    hot-key loop, COUNT + SUM_F64 only).  The segmented mode itself: test_segmented_mode_over_sorted_keys."""
    case = E.gpu_case("part_sorted")
    slim = slim_routes(funcs, "blk")
    run_hash_agg(hip, monkeypatch, case, funcs, {"SQLRS_RP_CLAIM": "1"}, **slim)
    run_hash_agg(hip, monkeypatch, case, funcs, {"SQLRS_RP_CLAIM": "1", "SQLRS_AGG_SEG": "0"}, **slim)
    run_hash_agg(hip, monkeypatch, case, funcs, **dense_routes(funcs))


@pytest.mark.parametrize("funcs", [PAIRS[0], PAIRS[1]], ids=sig_id)
def test_segmented_mode_over_sorted_keys(hip, monkeypatch, funcs):
    """The segmented mode of lds_agg_dense_slim_kernel (COUNT + SUM_F64: a wave's rows added per run of equal slots, a whole wave
    on one slot through the carry).  The kernel decides it per work item and no counter sees it; what turns it on is stated
    here: the RUN-LIST form (asserted: agg_part_slim_runs), a work item of >= 4096 rows, and rows that reach the bucket as runs
    of >= 2048 rows on average (`hi - lo >= 4096 && k_count * 2048 <= hi - lo && !seg_off && !BLK`).  2^22 rows SORTED by key over
    2.1 M keys are more than 512 direct-addressed buckets of ~8 000 rows, two partition levels, and with one workgroup
    (SQLRS_RP_CHUNK_WGS=1) the chunked first level hands every bucket its rows as the two or three 6144-row chunks they were
    contiguous in.  Among the sorted rows: runs of 300 rows of every edge value (each NaN, +-Inf, -0.0 ...), a run of 21 000 rows
    of the NaN 0xFFFF..F, and two rows a key elsewhere.  SQLRS_AGG_SEG unset and =0 (per-row adds) both inside the model's bound,
    and the counting levels + lds_agg_dense_kernel on the same rows."""
    case = E.gpu_case("part_sorted_wide")
    slim = dict(slim_routes(funcs, "runs"))
    assert slim.get("part_slim_runs") == 1
    run_hash_agg(hip, monkeypatch, case, funcs, {"SQLRS_RP_CHUNK_WGS": "1"}, **slim)
    run_hash_agg(hip, monkeypatch, case, funcs, {"SQLRS_RP_CHUNK_WGS": "1", "SQLRS_AGG_SEG": "0"}, **slim)
    run_hash_agg(hip, monkeypatch, case, funcs, **dict(dense_routes(funcs), part_split=0))


@pytest.mark.parametrize("funcs", [SINGLES[2], PAIRS[0]], ids=sig_id)
def test_partition_route_dense_slim_runs(hip, monkeypatch, funcs):
    """1.2 M keys over a range of 2.4 M: more than 512 direct-addressed buckets, two partition levels; with one workgroup
    (SQLRS_RP_CHUNK_WGS=1) the arena slack of the chunked first level is a fraction of the input and slim rows with run lists
    reach lds_agg_dense_slim_kernel; without the hook the counting levels feed lds_agg_dense_kernel"""
    case = E.gpu_case("part_wide_range")
    run_hash_agg(hip, monkeypatch, case, funcs, {"SQLRS_RP_CHUNK_WGS": "1"}, **slim_routes(funcs, "runs"))
    run_hash_agg(hip, monkeypatch, case, funcs, **dict(dense_routes(funcs), part_split=0))


@pytest.mark.parametrize("case_name", ["merge_small_last", "merge_small_first"])
def test_large_and_small_batch_are_one_pass(hip, monkeypatch, case_name):
    """2^21 rows and 1 000 rows that touch old and new groups, in both orders: staged, so ONE bucket pass whose groups stay
    pending (module docstring); group order follows the arrival order"""
    for funcs in (PAIRS[0], PAIRS[5], GENERIC[0]):
        run_hash_agg(hip, monkeypatch, E.gpu_case(case_name), funcs, **probing_routes(funcs))


@pytest.mark.parametrize("funcs", [PAIRS[0], PAIRS[5], GENERIC[0], [("sum", "i")]], ids=sig_id)
def test_key_set_too_large_for_the_estimate(hip, monkeypatch, funcs):
    """2^22 rows whose hashed sample shows 900 of 4 800 groups: the bucket tables fill up, the rows of the keys that found no
    slot come back as overflow rows and take the row route, and the pre-aggregated groups (some emitted more than once by
    the chunks of a full split table) are merged into the table state with their weights.  With 1 000 of 200 000 groups
    shown, the pass emits more groups than it has room for and the whole batch takes the row route."""
    family = {"part_probe_spec" if specialised(funcs) else "part_probe_generic": 1}
    run_hash_agg(hip, monkeypatch, E.gpu_case("part_underestimated"), funcs, lds_agg=1, row_route=True, part_packed=1, part_rec=1, part_split=1,
                 merge_groups=1, moves=("part_overflow_rows",), **family)
    if funcs in (PAIRS[0], GENERIC[0]):
        run_hash_agg(hip, monkeypatch, E.gpu_case("part_far_underestimated"), funcs, lds_agg=1, row_route=True, part_packed=1, part_rec=1,
                     part_split=1, moves=("part_overflow_rows",), **family)


# ---- join + aggregate ----------------------------------------------------------------------------------------------------------
JOIN_LISTS = [[("count", "f"), ("sum", "f"), ("min", "f"), ("max", "f")], [("sum", "i"), ("count", "i"), ("min", "i"), ("max", "i")],
              [("count", "f"), ("sum", "f")], [("sum", "i")]]


def run_join_agg(hip, jc, funcs, group_by, label, expect_fused, **routes):
    probe = jc.probe.batches()
    schema = pa.schema([(f"b.{f.name}", f.type) for f in jc.build_batch.schema] + [(f"p.{f.name}", f.type) for f in probe[0].schema])
    exp = jc.joined.model(funcs)
    ex = HashJoinAggExecutor(hip, [jc.build_batch], probe, JoinCondition([(InputRef(0), InputRef(0))]), schema, 2,
                             E.agg_funcs(funcs, first_col=3), group_by)
    with route(hip, label, **routes):
        got = table_of(ex.execute())
    assert (ex.fused_batches >= 1) == expect_fused, (label, ex.fused_batches)
    M.compare(got, exp, label)
    return ex


@pytest.mark.parametrize("funcs", JOIN_LISTS, ids=sig_id)
@pytest.mark.parametrize("kind", ["unique", "duplicates"])
def test_fused_join_agg(hip, kind, funcs):
    """300 build keys over a dense range, 70 001 probe rows (half of them on one key, some without partner): the bucket pass
    aggregates probe rows and, for duplicate build keys (multiplicities 1 - 4), multiplies COUNT / SUM cells by the key's build
    rows — Inf and NaN cells, wrapping int64 cells — and leaves MIN / MAX alone.  The model sees the join written out."""
    jc = E.join_case(kind)
    run_join_agg(hip, jc, funcs, [InputRef(0)], f"{kind} {sig_id(funcs)}", True, lds_agg=1, part_dense=1, part_packed=1, part_rec=1,
                 part_join=1, part_join_mult=int(kind == "duplicates"), part_split=1, pending_deferred=1,
                 part_interpreted=0 if specialised(funcs) else 1)


@pytest.mark.parametrize("kind", ["unique", "duplicates"])
def test_join_agg_below_the_fused_size_is_composed(hip, kind):
    """300 build keys x 5 000 probe rows: under the fused route's 2^16 rows, join and aggregate are composed (row route)"""
    jc = E.join_case(kind, n=5000)
    run_join_agg(hip, jc, JOIN_LISTS[0] + JOIN_LISTS[1][:1], [InputRef(0)], kind, False, row_route=True)


@pytest.mark.parametrize("funcs", [JOIN_LISTS[0], JOIN_LISTS[1], [("count", "i"), ("sum", "f"), ("min", "i"), ("max", "f")]], ids=sig_id)
def test_eager_join_agg(hip, funcs):
    """GROUP BY a build attribute with three join keys per value: partial groups by join key (fused bucket pass), then the
    second level — it must ADD the partial counts, carry MIN / MAX through the ordered images (KIND 3) including an attribute
    whose only value is the accumulator's neutral start, and keep an attribute NULL whose partial groups are all NULL"""
    jc = E.join_case("attribute")
    # first level: the probe rows carry NULLs, so flags, unpacked rows and the generic probing kernel over the build keys' buckets,
    # its groups pending; second level: one row-route operator per partial column (no agg_part_* counter moves there)
    ex = run_join_agg(hip, jc, funcs, [InputRef(1)], sig_id(funcs), True, lds_agg=1, row_route=True, part_probe_generic=1, part_unpacked=1,
                      part_flags=1, pending_deferred=1, part_join=1, wide_parts=len(funcs))
    assert ex.eager_groups > 0


# ---- DISTINCT, SimpleAgg --------------------------------------------------------------------------------------------------------
def test_distinct_over_the_int64_pool(hip):
    case = E.gpu_case("distinct")
    aggs = E.agg_funcs([("count", "i")], distinct=True) + E.agg_funcs([("sum", "i")], distinct=True) + E.agg_funcs([("count", "f")])
    exp = E.distinct_case(case).model([("count", "j"), ("sum", "i")])
    exp.cols.append(case.model([("count", "f")]).cols[0])
    with route(hip, "distinct", row_route=True):
        got = table_of(HashAggExecutor(hip, aggs, [InputRef(0)], case.batches()).execute())
    M.compare(got, exp, "distinct")


@pytest.mark.parametrize("case_name", ["simple_1_batch", "simple_3_batches"])
def test_simple_agg_one_group(hip, case_name):
    """SimpleAgg: one group over the f64, i64 and i32 pools; the model's single group is the expectation"""
    case = E.gpu_case(case_name)
    funcs = ROW_FUNCS + [("sum", "g"), ("count", "i")]
    exp = case.model(funcs)
    assert len(exp) == 1
    with route(hip, case_name, row_route=True, wide_parts=4):  # (the wide list: one row-route operator per argument column f, g, i, j)
        (out,) = list(SimpleAggExecutor(hip, E.agg_funcs(funcs), case.batches()).execute())
    got = pa.Table.from_batches([out])
    got = got.add_column(0, "k", pa.array(exp.keys, type=pa.int64()))
    M.compare(got, exp, case_name)


def test_simple_agg_no_rows(hip):
    funcs = ROW_FUNCS
    empty = E.gpu_case("simple_1_batch").batches()[0].slice(0, 0)
    with route(hip, "no rows", wide_parts=3):  # (f, i, j; nothing to update)
        (out,) = list(SimpleAggExecutor(hip, E.agg_funcs(funcs), [empty]).execute())
    assert [c.to_pylist() for c in out.columns] == [[0] if f == "count" else [None] for f, _ in funcs]
