"""Every device route of the hash exchange primitives against the independent model (tests/partition_model.py) on the cases of
tests/partition_edge_cases.py: the ends of int64 and int32, -0.0 against +0.0, NaN payloads, all-equal keys, runs of 64 equal keys,
empty first / middle / last partitions, 0 % / 10 % / 100 % NULL keys, Int32 / Boolean / Utf8 / expression keys, 1 to 256 parts, row
counts around one tile (4096) and around the threshold of the fast routes (65536), Int32 / Boolean / Utf8 / nullable payload
columns, HOST, DEVICE and sliced input, HOST and DEVICE output.  Every comparison is exact (partition_model.compare).

Which route ran is asserted over the scopes of sqlrs_ctx_profile_read ("The hash-partition contract"):

  sqlrs_hash_partition         fast      `hash_partition` + 1; `gather` and `radix_sort` at rest
                               general   `gather` + the number of columns; `radix_sort` moves when parts > 1 and rows > 1 (and
                                         rests otherwise: one part or one row is not sorted); `hash_partition` + 1 when rows > 0
  sqlrs_hash_partition_filter  fused     `hash_partition_filter` + 1; `hash_partition`, `gather`, `filter_cmp_const` at rest
                               composed  `hash_partition_filter` at rest; `hash_partition` + 1 when a row is kept

The last two tests check the contract the exchange stands on — rows with equal keys land in the same partition — end to end on
one GPU: the join and the group-by run per partition over W = 2, 3, 8 simulated ranks equal the models' results on the whole
tables."""
from collections import Counter
from contextlib import contextmanager

import numpy as np
import pyarrow as pa
import pytest

import agg_model
import join_edge_cases as J
import join_model
import partition_edge_cases as E
import partition_model as M
from order_plan import read_counters as counters
from sqlrs_amd import abi
from sqlrs_amd.executor import HashAggExecutor, HashJoinExecutor
from sqlrs_amd.expr import AggFunc, InputRef, JoinCondition

pytestmark = pytest.mark.gpu
MEM = {"device": abi.MEM_DEVICE, "host": abi.MEM_HOST}


@contextmanager
def route(be, label, exactly=None, at_least=None, still=()):
    """asserts how far the profile counters move across the block: `exactly` / `at_least` {name: by}, `still` names at rest"""
    before = counters(be)
    yield
    after = counters(be)
    moved = {k: after.get(k, 0) - before.get(k, 0) for k in set(after) | set(before)}
    for k, by in (exactly or {}).items():
        assert moved.get(k, 0) == by, (label, k, "moved by", moved.get(k, 0), "expected", by)
    for k, by in (at_least or {}).items():
        assert moved.get(k, 0) >= by, (label, k, "moved by", moved.get(k, 0), "expected at least", by)
    for k in still:
        assert moved.get(k, 0) == 0, (label, k, "moved by", moved.get(k, 0), "expected to rest")


@pytest.fixture(autouse=True)
def profiled(hip):
    hip.profile(True)
    yield
    hip.profile(False)


def give(hip, c):
    """the case's input in its memory form: a DEVICE batch, a HOST pyarrow batch, or a slice handed over with its offset (the Arrow C
    Data Interface: the values start 24 bytes into their buffer, the validity bits at bit 3)"""
    if c.mem_in == "device":
        return hip.to_device(c.batch)
    if c.mem_in == "slice":
        return abi.ArrowCBatch(hip, c.batch)
    return c.batch


def fetch(hip, out, c) -> pa.RecordBatch:
    names = c.batch.schema.names
    if c.mem_out == "host":
        assert all(out.column(i).mem == abi.MEM_HOST for i in range(out.num_columns))
        return out.to_arrow(names)
    assert all(out.column(i).mem == abi.MEM_DEVICE for i in range(out.num_columns))
    return hip.to_host(out).to_arrow(names)


# ---- a. sqlrs_hash_partition --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.names(form="stable"))
def test_hash_partition(hip, name):
    c = E.case(name)
    src = give(hip, c)
    if c.route == "fast":
        plan = dict(exactly={"hash_partition": 1}, still=("gather", "radix_sort", "hash_partition_filter"))
    elif c.parts > 1 and c.rows > 1:   # (radix_sort_pairs returns before its scope for a single row: nothing to sort)
        plan = dict(exactly={"hash_partition": 1, "gather": c.ncols}, at_least={"radix_sort": 1}, still=("hash_partition_filter",))
    else:
        plan = dict(exactly={"hash_partition": 1 if c.rows else 0, "gather": c.ncols}, still=("radix_sort", "hash_partition_filter"))
    with route(hip, name, **plan):
        out, offs = hip.hash_partition(src, c.key, c.parts, MEM[c.mem_out])
    got = fetch(hip, out, c)
    out.release()
    if c.mem_in != "host":
        src.release()
    exp = c.expected
    if exp is None:  # a Utf8 key: the assignment is read off the output under the contract's properties; the rest is determined
        exp = M.stable_from(c.batch, M.utf8_partitions(got.column(c.kcol), offs, c.ids, c.parts), c.parts)
    M.compare(got, offs, exp, name)


# ---- b. sqlrs_hash_partition_filter -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.names(form="filter"))
def test_hash_partition_filter(hip, name):
    c = E.case(name)
    src = give(hip, c)
    kept = int(c.keep.sum())
    if c.route == "fused":
        plan = dict(exactly={"hash_partition_filter": 1}, still=("hash_partition", "gather", "filter_cmp_const", "radix_sort"))
    else:
        plan = dict(exactly={"hash_partition": 1 if kept else 0}, still=("hash_partition_filter",))
    with route(hip, name, **plan):
        out, starts, rows = hip.hash_partition_filter(src, c.key, c.pred, c.parts, MEM[c.mem_out])
    got = fetch(hip, out, c)
    out.release()
    if c.mem_in != "host":
        src.release()
    exp = c.expected
    if exp is None:  # a Utf8 key (composed route): contiguous partitions of the kept rows
        sub = c.batch.filter(pa.array(c.keep))
        offs = list(starts) + [kept]
        assert got.num_rows == kept and rows == [b - a for a, b in zip(offs, offs[1:])], (name, starts[:4], rows[:4], kept)
        ids = [k for k, z in zip(c.ids, c.keep) if z]
        exp = M.kept_from(sub, M.utf8_partitions(got.column(c.kcol), offs, ids, c.parts), np.ones(kept, dtype=bool), c.parts)
    M.compare(got, (starts, rows), exp, name)
    if c.route == "composed":   # Filter, then the stable partition: the stable order holds here too
        M.compare_kept_in_order(got, (starts, rows), exp, name)
    else:
        cap = (max(c.rows, 1) + 63) // 64 * 64
        assert got.num_rows == c.parts * cap and starts == [p * cap for p in range(c.parts)], (name, got.num_rows, starts[:3])


# ---- d. co-location, end to end -----------------------------------------------------------------------------------------------------
def _arrow_parts(hip, batch, key, W, filter_form=False):
    """the W slices of `batch` hash-partitioned on column `key` (HOST), through either entry point"""
    names = batch.schema.names
    if filter_form:
        out, starts, rows = hip.hash_partition_filter(batch, InputRef(key), None, W, abi.MEM_HOST)
    else:
        out, offs = hip.hash_partition(batch, InputRef(key), W, abi.MEM_HOST)
        starts, rows = offs[:-1], [b - a for a, b in zip(offs, offs[1:])]
    t = out.to_arrow(names)
    out.release()
    assert sum(rows) == batch.num_rows
    return [t.slice(starts[p], rows[p]) for p in range(W)]


def _join_tables(kind, seed):
    """a build and a probe batch over the edge pools: duplicates, NULL keys on both sides (NULL = NULL matches), misses"""
    rng = np.random.default_rng(seed)
    if kind == "bool":
        bkeys, bnull = [1, 0, 1, 0, 1], [False, False, False, True, True]
        nprobe = 2000
    else:
        pool = {"i64": J.POOL_I64, "i32": J.POOL_I32, "f64": J.POOL_F64 + J.NAN_PAYLOADS}[kind]
        rnd = E.random_keys(rng, kind, 2500)
        bkeys = list(pool) * 2 + list(dict.fromkeys(rnd))
        rng.shuffle(bkeys)
        bnull = rng.random(len(bkeys)) < 0.002
        bnull[7] = True
        nprobe = 20_000
    bnull = np.asarray(bnull, dtype=bool)
    build = J.build_batch(rng, kind, bkeys, bnull, "numeric")
    pkeys, pnull = J.probe_keys(rng, kind, bkeys, bnull, nprobe, "nulls", list(range(len(bkeys))))
    probe = J.probe_batch(rng, kind, pkeys, pnull, "numeric")
    return build, probe


@pytest.mark.parametrize("W", [2, 3, 8])
@pytest.mark.parametrize("kind", ["i64", "i32", "f64", "bool"])
def test_join_per_partition_equals_the_join_of_the_whole(hip, kind, W):
    """both sides partitioned on their key, HashJoinExecutor (inner, then full) per pair of slices: the union of the joined rows equals
    tests/join_model.py's join of the whole tables as a multiset of whole rows — a NULL-key row of the full join exactly once"""
    build, probe = _join_tables(kind, 40 + W)
    bparts, pparts = _arrow_parts(hip, build, J.LKEY, W), _arrow_parts(hip, probe, J.RKEY, W)
    schema = pa.schema([(f"l.{f.name}", f.type) for f in build.schema] + [(f"r.{f.name}", f.type) for f in probe.schema])
    cond = JoinCondition([(InputRef(J.LKEY), InputRef(J.RKEY))])
    nleft = build.num_columns
    for jt in ("inner", "full"):
        got = Counter()
        for p in range(W):
            for b in HashJoinExecutor(hip, [bparts[p]], [pparts[p]], jt, cond, schema, nleft).execute():
                got.update(M.rows_of(b))
        exp = Counter()
        for b in join_model.join([build], [probe], J.LKEY, J.RKEY, jt):
            exp.update(M.rows_of(b))
        assert sum(exp.values()) > probe.num_rows // 2
        if got != exp:
            extra, lack = list((got - exp).items())[:3], list((exp - got).items())[:3]
            raise AssertionError(f"{kind} W = {W} {jt}: joined rows differ; not expected: {extra}; missing: {lack}")
        if jt == "full":   # (implied by the multisets; said once more in the issue's words)
            nulls = lambda rows: sum(n for r, n in rows.items() if r[nleft + J.RKEY] is None)
            assert nulls(got) == nulls(exp) > 0


def _group_table(kind, seed, n=20_000):
    rng = np.random.default_rng(seed)
    ck = kind
    vals = E.key_values(rng, ck, "pool", n, 8)
    null = rng.random(n) < 0.1
    arg = rng.integers(-(2 ** 62), 2 ** 62, n, dtype=np.int64)
    arg_null = rng.random(n) < 0.1
    return pa.RecordBatch.from_arrays([E.key_column(ck, vals, null), pa.array(arg, mask=arg_null)], names=["k", "a"])


def _expected_groups(batch) -> set:
    """{(key identity, COUNT(a), SUM(a) or None)}: tests/agg_model.py over the key images; a Python dict for a Utf8 key"""
    ids = M.images_of(batch.column(0))
    a = batch.column(1)
    valid = np.asarray(a.is_valid())
    vals = a.fill_null(0).to_numpy()
    if batch.column(0).type == pa.string():
        groups = {}
        for k, v, ok in zip(ids, vals.tolist(), valid.tolist()):
            g = groups.setdefault(k, [0, 0])
            if ok:
                g[0] += 1
                g[1] += v
        return {(k, c, agg_model.wrap_i64(s) & M.MASK if c else None) for k, (c, s) in groups.items()}
    img = np.array([0 if k is None else k for k in ids], dtype=np.uint64).view(np.int64)
    kv = np.array([k is not None for k in ids], dtype=bool)
    g = agg_model.aggregate(img, kv, [(vals, valid)], [("count", 0), ("sum", 0)])
    out = set()
    for i in range(len(g)):
        key = int(g.keys[i]) & M.MASK if g.key_valid[i] else None
        out.add((key, int(g.cols[0].bits[i]), int(g.cols[1].bits[i]) if g.cols[1].valid[i] else None))
    return out


@pytest.mark.parametrize("W", [2, 3, 8])
@pytest.mark.parametrize("kind", ["i64", "i32", "f64", "bool", "utf8"])
def test_group_by_per_partition_equals_the_group_by_of_the_whole(hip, kind, W):
    """the batch partitioned with sqlrs_hash_partition and with sqlrs_hash_partition_filter (no predicate), HashAggExecutor COUNT and
    SUM(int64) per partition: the concatenated groups equal the model's as a set, and no key identity occurs in two partitions"""
    batch = _group_table(kind, 70 + W)
    exp = _expected_groups(batch)
    assert len(exp) > 20 or kind == "bool"
    aggs = [AggFunc("count", InputRef(1), abi.INT64), AggFunc("sum", InputRef(1), abi.INT64)]
    for filter_form in (False, True):
        what = f"{kind} W = {W} {'filter form' if filter_form else 'stable form'}"
        seen, got = {}, set()
        for p, part in enumerate(_arrow_parts(hip, batch, 0, W, filter_form)):
            for out in HashAggExecutor(hip, aggs, [InputRef(0)], [part]).execute():
                keys = M.images_of(out.column(0))
                cnt, sm = out.column(1).to_pylist(), out.column(2).to_pylist()
                for k, c, s in zip(keys, cnt, sm):
                    assert k not in seen, f"{what}: key {k!r} has groups in partitions {seen[k]} and {p}"
                    seen[k] = p
                    got.add((k, c, None if s is None else s & M.MASK))
        assert seen.get(None, 0) == 0, f"{what}: the NULL group is in partition {seen[None]}"
        assert got == exp, (what, len(got), len(exp), sorted(got ^ exp, key=repr)[:4])
