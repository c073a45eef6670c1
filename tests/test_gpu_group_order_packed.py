"""First-seen order of pre-aggregated groups without the pack pass and the separate gather (hashagg_op.hip
emit_pending_group_rows): the dense bucket passes store every group as one 32-byte row and the last pass of the sort over the
first rows gathers the rows straight into the output columns.

Every case runs twice in this process — SQLRS_AGG_ORDER_PACKED unset (the default: on) and =0 (groups as columns, ordered by
pack + sort + gather) — and both outputs are compared with the first-seen order and the values of tests/agg_model.py: keys, order
and COUNT / integer SUM bit for bit, SUM(f64) inside the model's bound (its cells are added by LDS atomics in any order).  Keys
and COUNTs of the two runs are also compared with each other.  Which route ran is asserted with the witnesses of
test_gpu_agg_edges.py (`route`) plus the new count `agg_order_packed`: 1 where the rows route must run, absent where it must
decline and in every run with the hook off.

What an operator cannot reach, and why the cases for it assert a decline instead:
* batches of 200, 40 000 and 2^20 + 5 rows through HashAgg: the partition route starts at 2^21 rows (hashagg_op.hip PART_MIN_ROWS);
  200 and 40 000 probe rows through the fused join+aggregate: it starts at 2^16 probe rows.  So a batch whose first rows need one
  or two digits never has pre-aggregated groups to order.  The sort entry takes two passes at least on this route (sort.hip
  sort_index_u32) and the last pass is the same kernel for 2, 3 and 4 passes; 3 passes run here from 70 001 and 2^20 + 5 probe
  rows, 4 passes from 2^24 + 5 rows; 1 and 2 digits are run by the numpy restatement (test_group_order_packed_cpu.py).
* 1 to 65 groups through HashAgg: so few groups are one bucket that the probing kernel reads in place (agg_partition.hip
  `in_place`), and it keeps columns — asserted; every group count of the list runs through the fused join+aggregate, whose single
  bucket is direct-addressed.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import agg_edge_cases as E
import agg_model as M
import group_order_packed_cases as P
import test_gpu_agg_edges as T
from sqlrs_amd import abi
from sqlrs_amd.executor import HashAggExecutor
from sqlrs_amd.expr import AggFunc, InputRef

pytestmark = pytest.mark.gpu

HOOK = "SQLRS_AGG_ORDER_PACKED"
COUNT_SUM_F, SUM_COUNT_F, COUNT_SUM_I = T.PAIRS[0], T.PAIRS[1], T.PAIRS[2]


@pytest.fixture(scope="module")
def hip():
    import sqlrs_amd
    be = sqlrs_amd.new_ctx(0)
    yield be
    be.close()


@pytest.fixture(autouse=True)
def profiled(hip, monkeypatch):
    for k in T.HOOKS + (HOOK,):
        monkeypatch.delenv(k, raising=False)
    hip.profile(True)
    yield
    hip.profile(False)


# ---- both ways -----------------------------------------------------------------------------------------------------------------
def both_ways(hip, monkeypatch, label, run, exp, packed, env=None, compare=M.compare, **routes):
    """run() with the hook unset and =0 inside a route block each; `packed`: the rows route must run (hook unset)"""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    got = {}
    for way in ("on", "off"):
        if way == "off":
            monkeypatch.setenv(HOOK, "0")
        before = T.counters(hip).get("agg_order_packed", 0)
        with T.route(hip, f"{label} [{way}]", **routes):
            got[way] = run()
        moved = T.counters(hip).get("agg_order_packed", 0) - before
        assert moved == int(packed and way == "on"), f"{label} [{way}]: agg_order_packed moved by {moved}"
        compare(got[way], exp, f"{label} [{way}]")
    monkeypatch.delenv(HOOK)
    for k in (env or {}):
        monkeypatch.delenv(k)
    if got["on"] is not None:
        for c, col in enumerate([None] + list(exp.cols)):
            if col is None or col.func == "count":
                assert got["on"].column(c).equals(got["off"].column(c)), f"{label}: column {c} differs between the two ways"
    return got["on"]


def hash_agg(hip, case, funcs):
    return lambda: T.table_of(HashAggExecutor(hip, E.agg_funcs(funcs), [InputRef(0)], case.batches()).execute())


# ---- light cases: [k, f, i] only, dense keys, every group count exactly ------------------------------------------------------------
class Light:
    """n rows over G dense keys from -777 in random order; row 0 opens a group (first row 0) and the LAST row is the only row of
    its group (first row n - 1)"""

    def __init__(self, n, G, seed):
        rng = np.random.default_rng(seed)
        assert 1 <= G <= n
        if G == 1:
            grp = np.zeros(n, np.int64)
        else:
            body = np.concatenate([np.arange(G - 1), rng.integers(0, G - 1, n - G)])
            grp = np.concatenate([rng.permutation(body), [G - 1]]).astype(np.int64)
        self.keys = rng.permutation(G).astype(np.int64)[grp] - 777
        self.f = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 5, n)
        self.i = rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)
        self.n, self.G = n, G
        self._cache = {}

    def batches(self):
        return [pa.RecordBatch.from_arrays([pa.array(self.keys), pa.array(self.f), pa.array(self.i)], names=["k", "f", "i"])]

    def model(self, funcs):
        return M.aggregate(self.keys, None, [(self.f, None), (self.i, None)], [(f, "fi".index(c)) for f, c in funcs], cache=self._cache)

    def run(self, hip, funcs):
        aggs = [AggFunc(f, InputRef(1 + "fi".index(c)), abi.INT64 if f == "count" or c == "i" else abi.FLOAT64) for f, c in funcs]
        return lambda: T.table_of(HashAggExecutor(hip, aggs, [InputRef(0)], self.batches()).execute())


# (which dense form a light case takes is not what these tests are about: the family counters are left alone, and only a dense
#  form stores rows — agg_order_packed says that one ran)
FAMILY = ("part_split", "part_rec", "part_dense", "part_slim_blk", "part_slim_runs", "part_interpreted")
DENSE_LIGHT = dict(lds_agg=1, part_packed=1, pending_deferred=1, free=FAMILY)


@pytest.mark.parametrize("G", [4095, 4096, 4097, 8193, 70_001])
def test_hash_agg_group_counts(hip, monkeypatch, G):
    """2^21 + 77 rows, direct-addressed tables of 4096 slots (one bucket, two and more), COUNT + SUM(f64) and SUM(i64) alone (one
    cell, cell 1 of the row stays 0); a first row of 0 and one of rows - 1"""
    case = Light(E.N_PART, G, seed=G)
    exp = case.model(COUNT_SUM_F)
    assert len(exp) == G and exp.keys[-1] == case.keys[-1] and exp.keys[0] == case.keys[0]
    both_ways(hip, monkeypatch, f"light G={G}", case.run(hip, COUNT_SUM_F), exp, True, **DENSE_LIGHT)
    both_ways(hip, monkeypatch, f"light G={G} sum(i)", case.run(hip, [("sum", "i")]), case.model([("sum", "i")]), True,
              **DENSE_LIGHT)


@pytest.mark.parametrize("G", [1, 2, 63, 64, 65])
def test_hash_agg_few_groups_decline(hip, monkeypatch, G):
    """few groups in one bucket: read in place by the probing kernel, groups as columns whatever the hook says"""
    case = Light(E.N_PART, G, seed=G)
    both_ways(hip, monkeypatch, f"light G={G}", case.run(hip, COUNT_SUM_F), case.model(COUNT_SUM_F), False, lds_agg=1, part_in_place=1,
              part_unpacked=1, part_probe_spec=1, pending_deferred=1, free=("part_split",))


@pytest.mark.parametrize("n", [200, 40_000, (1 << 20) + 5])
def test_hash_agg_below_the_partition_route(hip, monkeypatch, n):
    """first rows of one, two and three digits — through HashAgg such a batch takes the row route: no pre-aggregated groups"""
    assert P.digits_of(n) == P.PASS_ROWS[n]
    case = Light(n, min(n // 3, 4097), seed=n)
    both_ways(hip, monkeypatch, f"light n={n}", case.run(hip, COUNT_SUM_F), case.model(COUNT_SUM_F), False, row_route=True)


def test_hash_agg_four_digits(hip, monkeypatch):
    """2^24 + 5 rows: first rows of four digits, the last group opens at row 2^24 + 4; integer cells, compared bit for bit"""
    n = (1 << 24) + 5
    assert P.digits_of(n) == 4
    case = Light(n, 70_001, seed=24)
    exp = case.model(COUNT_SUM_I)
    assert exp.keys[-1] == case.keys[-1]
    both_ways(hip, monkeypatch, "light 2^24+5", case.run(hip, COUNT_SUM_I), exp, True, **DENSE_LIGHT)


# ---- the shapes of test_gpu_agg_edges.py: every dense form of the bucket pass -------------------------------------------------------
FORMS = [("part_dense", None, "dense"), ("part_dense_hot", {"SQLRS_RP_CLAIM": "1"}, "blk"), ("part_wide_range", {"SQLRS_RP_CHUNK_WGS": "1"}, "runs")]


@pytest.mark.parametrize("funcs", [COUNT_SUM_F, SUM_COUNT_F, COUNT_SUM_I, [("sum", "f")], [("count", "f")]], ids=T.sig_id)
@pytest.mark.parametrize("case_name,env,form", FORMS, ids=[f[2] for f in FORMS])
def test_dense_forms(hip, monkeypatch, case_name, env, form, funcs):
    """lds_agg_dense_kernel with every bucket cut into chunks (split_emit_dense_kernel emits the rows), the claimed single level's
    slim rows (`blk`, split as well) and the two-level slim form (`runs`, emitted by lds_agg_dense_slim_kernel itself); `SUM, COUNT`
    takes the cells in the other order"""
    case = E.gpu_case(case_name)
    routes = T.dense_routes(funcs) if form == "dense" else T.slim_routes(funcs, form)
    both_ways(hip, monkeypatch, f"{case_name} {T.sig_id(funcs)}", hash_agg(hip, case, funcs), case.model(funcs), True, env, **routes)


def test_row_route_shape(hip, monkeypatch):
    case = E.gpu_case("row_4097")
    both_ways(hip, monkeypatch, "row_4097", hash_agg(hip, case, COUNT_SUM_F), case.model(COUNT_SUM_F), False, row_route=True)


# ---- shapes that must decline -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("funcs", [[("count", "f"), ("sum", "f"), ("max", "f")], T.PAIRS[4], T.PAIRS[5], [("min", "i")]], ids=T.sig_id)
def test_three_aggregates_and_min_max_decline(hip, monkeypatch, funcs):
    case = E.gpu_case("part_dense")
    both_ways(hip, monkeypatch, f"part_dense {T.sig_id(funcs)}", hash_agg(hip, case, funcs), case.model(funcs), False, **T.dense_routes(funcs))


def run_any_order(hip, case, funcs):
    """HashAggExecutor.execute with sqlrs_hash_agg_set_group_order(ANY) before the first push"""
    def run():
        be, keep = hip, []
        gb, k = abi.pack_exprs([InputRef(0)])
        aggs_l = E.agg_funcs(funcs)
        aggs = (abi.AggFunc * len(aggs_l))(*[a.abi_struct(keep) for a in aggs_l])
        h = C.c_void_p()
        be.check(be.fn("hash_agg_create")(be.ctx, 1, gb, len(aggs_l), aggs, C.byref(h)))
        try:
            be.check(be.fn("hash_agg_set_group_order")(h, abi.GROUP_ORDER_ANY))
            for batch in case.batches():
                b = abi.as_batch(batch)
                be.check(be.fn("hash_agg_push")(h, b.ptr))
            out = C.POINTER(abi.Batch)()
            be.check(be.fn("hash_agg_finish")(h, abi.MEM_HOST, C.byref(out)))
            from sqlrs_amd.executor import _emit
            return pa.Table.from_batches([_emit(be, out, abi.MEM_HOST, None)])
        finally:
            be.fn("hash_agg_destroy")(h)
    return run


def test_any_order_declines(hip, monkeypatch):
    """GROUP_ORDER_ANY: nothing is ordered, the groups leave in bucket order — compared with the model group by group (by key)"""
    case, funcs = E.gpu_case("part_dense"), COUNT_SUM_F
    exp = case.model(funcs)

    def by_key(got, exp, label):
        order = np.argsort(exp.keys, kind="stable")
        srt = M.Groups(exp.keys[order], exp.key_valid[order], [M.Column(c.func, c.kind, c.valid[order], c.bits[order], c.how[order],
                                                                      None if c.S is None else c.S[order], c.m[order]) for c in exp.cols])
        M.compare(got.take(pc.sort_indices(got.column(0))), srt, label)

    for way in ("on", "off"):
        if way == "off":
            monkeypatch.setenv(HOOK, "0")
        before = T.counters(hip).get("agg_order_packed", 0)
        with T.route(hip, f"any order [{way}]", **T.dense_routes(funcs)):
            got = run_any_order(hip, case, funcs)()
        assert T.counters(hip).get("agg_order_packed", 0) == before
        by_key(got, exp, f"any order [{way}]")


def test_utf8_key_declines(hip, monkeypatch):
    """a Utf8 key is matched by hash: no direct-addressed tables, groups as columns and the key values gathered by first row"""
    n, G = E.N_PART, 5000
    rng = np.random.default_rng(9)
    ids = np.concatenate([np.arange(G), rng.integers(0, G, n - G)])
    ids = rng.permutation(ids).astype(np.int64)
    i = rng.integers(-1000, 1000, n).astype(np.int64)
    names = np.array([f"key-{v:05d}" for v in range(G)])
    batch = pa.RecordBatch.from_arrays([pa.array(names.tolist()).take(pa.array(ids)), pa.array(i)], names=["k", "i"])
    aggs = [AggFunc("count", InputRef(1), abi.INT64), AggFunc("sum", InputRef(1), abi.INT64)]
    exp = M.aggregate(ids, None, [(i, None)], [("count", 0), ("sum", 0)])
    got = {}
    for way in ("on", "off"):
        if way == "off":
            monkeypatch.setenv(HOOK, "0")
        before = T.counters(hip).get("agg_order_packed", 0)
        got[way] = T.table_of(HashAggExecutor(hip, aggs, [InputRef(0)], [batch]).execute())
        assert T.counters(hip).get("agg_order_packed", 0) == before
        assert got[way].column(0).to_pylist() == names[exp.keys].tolist()
        assert np.array_equal(np.asarray(got[way].column(1).to_numpy()).view(np.uint64), exp.cols[0].bits)
        assert np.array_equal(np.asarray(got[way].column(2).to_numpy()).view(np.uint64), exp.cols[1].bits)
    assert got["on"].equals(got["off"])


# ---- the fused join+aggregate ------------------------------------------------------------------------------------------------------
def join_agg(hip, jc, funcs, expect_fused):
    from sqlrs_amd.executor import HashJoinAggExecutor
    from sqlrs_amd.expr import JoinCondition
    probe = jc.probe.batches()
    schema = pa.schema([(f"b.{f.name}", f.type) for f in jc.build_batch.schema] + [(f"p.{f.name}", f.type) for f in probe[0].schema])

    def run():
        ex = HashJoinAggExecutor(hip, [jc.build_batch], probe, JoinCondition([(InputRef(0), InputRef(0))]), schema, 2,
                                 E.agg_funcs(funcs, first_col=3), [InputRef(0)])
        got = T.table_of(ex.execute())
        assert (ex.fused_batches >= 1) == expect_fused, ex.fused_batches
        return got
    return run


FUSED = dict(lds_agg=1, part_packed=1, part_join=1, pending_deferred=1, free=FAMILY)


@pytest.mark.parametrize("G", P.GROUP_COUNTS)
def test_fused_join_group_counts(hip, monkeypatch, G):
    """G unique build keys over a dense range, probe rows on them and on 40 keys without partner: every group count of the list,
    one direct-addressed bucket up to 4096 keys; 70 001 probe rows (2^20 + 5 for 70 001 keys): first rows of three digits"""
    n = 70_001 if G < 70_001 else (1 << 20) + 5
    assert P.digits_of(n) == 3
    with np.errstate(all="ignore"):  # (join_case spreads an attribute over nkeys // 3 values: unused here, 0 below three keys)
        jc = E.join_case("unique", n=n, nkeys=G, seed=G)
    exp = jc.joined.model(COUNT_SUM_F)
    assert len(exp) == G
    both_ways(hip, monkeypatch, f"join G={G}", join_agg(hip, jc, COUNT_SUM_F, True), exp, True, **FUSED)


@pytest.mark.parametrize("n", [200, 40_000])
def test_fused_join_below_its_size_is_composed(hip, monkeypatch, n):
    """first rows of one and two digits: under 2^16 probe rows join and aggregate are composed (row route)"""
    jc = E.join_case("unique", n=n, nkeys=100, seed=n)
    both_ways(hip, monkeypatch, f"join n={n}", join_agg(hip, jc, COUNT_SUM_F, False), jc.joined.model(COUNT_SUM_F), False, row_route=True)


def gap_join_case(n=70_001, nkeys=3000, seed=73):
    """build keys with gaps: every third key of the dense range has no build row (its slot is removed after the table is built:
    LdsAggParams::partner_bits), the probe rows still carry it"""
    probe = E.build("join_gaps", n, seed, groups=nkeys + 40, keyspace="dense", hot=0.5)
    kept = np.arange(nkeys) % 3 != 1
    bkeys = (np.arange(nkeys, dtype=np.int64) - 777)[kept]
    order = np.random.default_rng(seed).permutation(len(bkeys))
    build_batch = pa.RecordBatch.from_arrays([pa.array(bkeys[order]), pa.array(np.zeros(len(bkeys), np.int64))], names=["bk", "attr"])
    at = probe.keys + 777
    has = (at >= 0) & (at < nkeys) & kept[np.clip(at, 0, nkeys - 1)]
    rows = np.nonzero(has)[0]
    jcols = {c: (v[rows], None) for c, (v, _) in probe.cols.items()}
    return E.JoinCase(build_batch, probe, E.Case("joined_gaps", probe.keys[rows], None, jcols, [0, len(rows)]))


def test_fused_join_over_a_dim_with_gaps(hip, monkeypatch):
    jc = gap_join_case()
    exp = jc.joined.model(COUNT_SUM_F)
    assert 1500 < len(exp) <= 2000
    both_ways(hip, monkeypatch, "join gaps", join_agg(hip, jc, COUNT_SUM_F, True), exp, True, **FUSED)


@pytest.mark.parametrize("funcs", [COUNT_SUM_F, [("sum", "i")]], ids=T.sig_id)
def test_fused_join_over_duplicate_build_keys_multiplies_before_the_row_is_stored(hip, monkeypatch, funcs):
    """multiplicities 1 - 4 (partner_mult): the rows route APPLIES — COUNT / SUM cells are multiplied by the key's build rows before
    the row is stored, as the column form does"""
    jc = E.join_case("duplicates")
    both_ways(hip, monkeypatch, f"join duplicates {T.sig_id(funcs)}", join_agg(hip, jc, funcs, True), jc.joined.model(funcs), True,
              part_join_mult=1, **FUSED)


# ---- a later batch arrives after all: the rows go back to columns and are merged ------------------------------------------------------
def two_batches_without_staging():
    """(child process: SQLRS_STAGE_DIRECT_ROWS is read once) two batches of 2^21 rows and more, each aggregated as it arrives: the
    first one's groups are pending as rows, the second one turns them into columns and merges both"""
    import sqlrs_amd
    be = sqlrs_amd.new_ctx(0)
    be.profile(True)
    case = E.build("two_batches", 2 * E.N_PART, 77, groups=40_000, keyspace="dense", batches=2)
    got = T.table_of(HashAggExecutor(be, E.agg_funcs(COUNT_SUM_F), [InputRef(0)], case.batches()).execute())
    M.compare(got, case.model(COUNT_SUM_F), "two batches")
    c = T.counters(be)
    dense = sum(c.get(k, 0) for k in ("agg_part_dense", "agg_part_slim_blk", "agg_part_slim_runs"))
    assert c.get("agg_merge_groups", 0) == 2 and dense == 2 and c.get("agg_order_packed", 0) == 0, c
    be.close()
    print("two_batches_without_staging ok")


def test_second_batch_turns_the_rows_into_columns():
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", "import conftest, test_gpu_group_order_packed as t; t.two_batches_without_staging()"], cwd=here,
                       env=dict(os.environ, SQLRS_HOOKS="1", SQLRS_STAGE_DIRECT_ROWS="0", SQLRS_TEST_CHILD="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "two_batches_without_staging ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
