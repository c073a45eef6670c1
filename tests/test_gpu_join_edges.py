"""Every device route of the hash join on ONE fixed-width key against the independent edge-key model (tests/join_model.py) on the
cases of tests/join_edge_cases.py: INT64_MIN and INT64_MAX together (the key set whose range `hi - lo + 1` wraps to 0), -1 (the
slot table's "empty" word), the neighbours of 2^31 and 2^32, doubles that differ only in sign or NaN payload, NULL = NULL,
Boolean keys, one key 5 000 times, every key twice, build rows next to the packed table's "empty" pattern, keys that hash to the
last slots of the slot table, probe keys one below / one above / 2^63 away from the build range, probe batches at the kernels'
own boundaries (64, JAP_ROWS 512, LJ_RANGE 2^15, the all-hit threshold 2^16).  Index pairs, joined batches and tail are compared
exactly (join_model.compare: validity bit for bit, values through integer views, Utf8 by value).

Which route ran is asserted, not assumed: every run sits in a `route(...)` block over the counters of sqlrs_ctx_profile_read.
`Plan` below restates the host-side dispatch of join.hip / join_async.hip / join_lds.hip from the case's facts (rows, NULL keys, key range,
uniqueness), the join type, the hooks and the probe batches, and the block asserts that every `join_*` counter moved by exactly
the planned number, that `async_fast_batches` did, and that every listed profile scope moved or stayed at rest as planned
("Route witnesses of the join"):

  join_dense_adopted / _refused               the direct-address table became the join's table, or was attempted and refused
  join_dense_one_fetch / _two_fetch           the build sized for the largest admissible range, or from the range it fetched
  join_dense_packed / _plain                  a bit-packed copy beside the 4-byte table, or the 4-byte table alone
  join_probe_pending                          a first probe on the device-side verdict (dense_pending)
  join_allhit_kept / _redone                  an optimistic all-hit probe that stood, or saw a miss
  join_compact_dense / _slots                 the compacting probe of the direct-address table / of the slot table
  join_unique_outer                           join_probe_unique_outer_kernel
  join_dd_stream / _dd_rows                   dd_count_stream_kernel / dd_count_kernel
  join_counts_grouped / _per_row              pair counts per 64-row group / per row
  join_lds_unique / _lds_distinct             a batch matched on LDS tables of the build keys / of its distinct keys
  join_table_late                             the slot table built by hash_join_ensure_table
  scopes: join_build_dense, join_build_dense_dup, join_build, join_build_csr, join_build_lds_unique, join_build_lds_distinct,
  join_partition_lds, join_probe_lds, join_match_compact, join_match_unpermute, join_probe_dense, join_probe_unique,
  join_probe_count_dense_dup, join_probe_count, join_probe_fill, join_semi_mask

Routes are steered only with hooks the library reads per call (monkeypatch.setenv): SQLRS_DENSE_BUILD_ONE_FETCH,
SQLRS_DENSE_PACKED, SQLRS_DENSE_BUILD_DEFER, SQLRS_PROBE_ALLHIT, SQLRS_JOIN_GROUPED, SQLRS_LDS_JOIN, SQLRS_LDS_FIRST,
SQLRS_LJ_RPI, SQLRS_ASYNC_FAST, SQLRS_DENSE_JOIN_SLOTS_PLAIN (and SQLRS_JOIN_COMPOSITE, read per build).  SQLRS_LDS_JOIN=1 forces
the LDS routes at these sizes.

What no input of <= 2^18 rows reaches, and the condition in the source that keeps it out:

* the `range < 2^31` bound of the direct-address table (dense_range.hpp: `span < 2^31 - 1`): a range is admitted up to 4 x rows +
  1024 (16 x rows for a join+aggregate's join), so the bound decides only from 2^29 build rows on.  host/dense_range_check.cpp
  puts the decision itself through both sides of it (test_join_model_cpu.py);
* per-row pair counts CHOSEN by size (join.hip probe_counted: `j->nB < (1ll << 26)`): reached here only through
  SQLRS_JOIN_GROUPED=0, which selects the same kernels' per-row form on every count route;
* a pair total beyond 2^32 (the 64-bit offsets of the fill pass; the `n > 0xffffffff` guards): 5 000 x 70 001 pairs would already
  be 3.5e8, the cases stay under 2^18 pairs per batch;
* the one-fetch build's size bound (`4 * (4 n + 1024) <= 2^30`, n <= 2^24) and its 25-bit packing bound: from 2^24 build rows;
  the two-fetch sequence is reached through SQLRS_DENSE_BUILD_ONE_FETCH=0 instead;
* the LDS routes' own size rule (join_lds.hip: nB >= 2^18, n >= 2^22, n >= 8 nB): forced with SQLRS_LDS_JOIN=1; the rule itself
  stays with test_gpu_parity.py's 4.4 M-row case;
* a look-back rerun with tickets (lookback_timed_out): decided by timing on the device;
* hashed keys — several key columns by default, Utf8 keys: the reference's 64-bit hash IS the contract there (two keys with one
  hash match), so they stay with the oracle comparisons of test_gpu_parity.py / test_gpu_join_composite.py.  The one
  composite case here checks the fall-back to hashes when a key column holds both ends of int64."""
import ctypes as C
import functools
from collections import Counter
from contextlib import contextmanager

import numpy as np
import pyarrow as pa
import pytest

import agg_edge_cases as AE
import agg_model as AM
import async_filter_cases as AF
import async_utf8_cases as AU
import join_edge_cases as E
import join_model as M
from sqlrs_amd import abi
from sqlrs_amd.executor import HashJoinAggExecutor, HashJoinExecutor
from sqlrs_amd.expr import InputRef, JoinCondition

pytestmark = pytest.mark.gpu

HOOKS = ("SQLRS_DENSE_BUILD_ONE_FETCH", "SQLRS_DENSE_PACKED", "SQLRS_DENSE_BUILD_DEFER", "SQLRS_PROBE_ALLHIT", "SQLRS_JOIN_GROUPED",
         "SQLRS_LDS_JOIN", "SQLRS_LDS_FIRST", "SQLRS_LJ_RPI", "SQLRS_ASYNC_FAST", "SQLRS_DENSE_JOIN_SLOTS_PLAIN", "SQLRS_JOIN_COMPOSITE")
JOIN_COUNTERS = ("join_dense_adopted", "join_dense_refused", "join_dense_one_fetch", "join_dense_two_fetch", "join_dense_packed",
                 "join_dense_plain", "join_probe_pending", "join_allhit_kept", "join_allhit_redone", "join_compact_dense",
                 "join_compact_slots", "join_unique_outer", "join_dd_stream", "join_dd_rows", "join_counts_grouped",
                 "join_counts_per_row", "join_lds_unique", "join_lds_distinct", "join_table_late")
SCOPES = ("join_build_dense", "join_build_dense_dup", "join_build", "join_build_csr", "join_build_lds_unique", "join_build_lds_distinct",
          "join_partition_lds", "join_probe_lds", "join_match_compact", "join_match_unpermute", "join_probe_dense", "join_probe_unique",
          "join_probe_count_dense_dup", "join_probe_count", "join_probe_fill", "join_semi_mask")


# ---- which route ran -------------------------------------------------------------------------------------------------------------
def counters(be) -> dict:
    cap = 512
    names, ms, n_l = (C.c_char_p * cap)(), (C.c_double * cap)(), (C.c_int64 * cap)()
    n = be.fn("ctx_profile_read")(be.ctx, cap, names, ms, n_l)
    assert n <= cap
    return {names[k].decode(): n_l[k] for k in range(n)}


@contextmanager
def route(be, label, plan):
    """asserts how the witnesses move across the block: every join_* counter and async_fast_batches by exactly plan.c[name] (0: at
    rest), every scope of SCOPES moved iff it is in plan.scopes"""
    before = counters(be)
    yield
    after = counters(be)
    moved = {k: after.get(k, 0) - before.get(k, 0) for k in set(after) | set(before)}
    seen = {k: v for k, v in moved.items() if v and (k.startswith("join_") or k.startswith("async_"))}
    unknown = set(plan.c) - {k[5:] for k in JOIN_COUNTERS} - {"async_fast_batches"}
    assert not unknown, unknown
    for k in JOIN_COUNTERS:
        assert moved.get(k, 0) == plan.c.get(k[5:], 0), f"{label}: {k} moved by {moved.get(k, 0)}, planned {plan.c.get(k[5:], 0)}; moved: {seen}; plan: {dict(plan.c)} {sorted(plan.scopes)}"
    assert moved.get("async_fast_batches", 0) == plan.c.get("async_fast_batches", 0), f"{label}: async_fast_batches moved by {moved.get('async_fast_batches', 0)}, planned {plan.c.get('async_fast_batches', 0)}; moved: {seen}"
    for k in SCOPES:
        assert (moved.get(k, 0) > 0) == (k in plan.scopes), f"{label}: scope {k} moved by {moved.get(k, 0)}, planned {'moving' if k in plan.scopes else 'at rest'}; moved: {seen}; plan: {dict(plan.c)} {sorted(plan.scopes)}"


class Plan:
    """the host-side dispatch of join.hip and lds_build_first / lds_join_match (join_lds.hip), restated over the facts of a case:
    which counters and scopes a run must move.  build = build_table (dense_try_one_fetch / dense_try_two_fetch), verdict =
    dense_verdict_decide + dense_apply_verdict, resolve = dense_resolve, after_refusal = build_after_refusal, ensure_table =
    hash_join_ensure_table, probe = probe_pairs and the route functions it chooses (probe_allhit_pending, probe_unique_inner,
    probe_unique_outer, probe_counted)"""

    def __init__(self, facts, jt, env=None, lazy=False, key_only_semi=False, slots_per_key=None):
        self.f, self.jt, self.env = facts, jt, env or {}
        self.outer_right = jt in ("right", "full")
        self.c, self.scopes = Counter(), set()
        self.dense = self.dd = self.table = self.lds_first = self.pending = self.miss_seen = False
        self.unique = None
        self.unique_known_dup = False
        self.dup_range = False
        self.lds_prepared_distinct = False
        self.lazy, self.semi = lazy, key_only_semi
        self.spk = slots_per_key
        self.build()

    def hook(self, name, default=None):
        return self.env.get(name, default)

    # ---- build ----
    def build(self):
        f, n = self.f, self.f["rows"]
        if f["kind"] == "f64":
            return self.after_refusal()
        spk = self.spk or (16 if self.lazy else int(self.hook("SQLRS_DENSE_JOIN_SLOTS_PLAIN", 4)))
        max_range = spk * n + 1024
        span = None if f["lo"] is None else f["hi"] - f["lo"]
        self.range_ok = span is not None and span < max_range and span < 2 ** 31 - 1
        self.unique_dense = self.range_ok and f["nulls"] <= 1 and f["unique"]
        if self.hook("SQLRS_DENSE_BUILD_ONE_FETCH") != "0":
            self.c["dense_one_fetch"] += 1
            self.scopes.add("join_build_dense")
            bits = 1
            while (1 << bits) - 1 < n:
                bits += 1
            bits = max(bits, 8)
            if bits > 25 or (max_range + 2) * bits >= 2 ** 32 or self.lazy or self.hook("SQLRS_DENSE_PACKED") == "0":
                bits = 0
            self.c["dense_packed" if bits else "dense_plain"] += 1
            self.bits = bits
            self.pending = bool(bits) and not self.lazy and self.hook("SQLRS_DENSE_BUILD_DEFER") != "0"
            if not self.pending:
                self.resolve(force=True)
            return
        self.c["dense_two_fetch"] += 1
        if self.range_ok:
            self.scopes.add("join_build_dense")
            self.c["dense_plain"] += 1
        self.verdict()

    def verdict(self):
        if self.unique_dense:
            self.c["dense_adopted"] += 1
            self.dense, self.unique = True, True
            return
        self.c["dense_refused"] += 1
        if self.range_ok:
            self.unique, self.unique_known_dup = False, True
            self.dup_range = self.f["nulls"] == 0
        self.after_refusal()

    def resolve(self, force=False):
        if self.pending or force:
            self.pending = False
            self.verdict()

    def after_refusal(self):
        f = self.f
        if self.lazy:
            return
        if self.dup_range:
            self.scopes.add("join_build_dense_dup")
            self.dd, self.unique = True, False
            return
        # (lds_partition_keys: the fullest of the 512 buckets at load 1/2 in <= 8192 slots — a run of > 4096 rows does not fit)
        if (self.hook("SQLRS_LDS_JOIN") == "1" and self.hook("SQLRS_LDS_FIRST") != "0" and not self.outer_right and f["nulls"] == 0 and
                f["rows"] >= 2 and not self.unique_known_dup and f["max_run"] <= 4096):
            self.scopes.add("join_build_lds_unique")
            if f["unique"]:
                self.unique, self.lds_first = True, True
                return
        self.build_hash_table()

    def build_hash_table(self):
        self.table = True
        self.scopes.add("join_build")
        self.unique = self.f["unique"] and self.f["nulls"] <= 1
        if not self.unique:
            self.scopes.add("join_build_csr")

    def ensure_table(self):
        self.resolve()
        if not (self.dense or self.dd or self.table):
            if self.dup_range:  # (a lazy table's duplicate keys over a dense range)
                self.scopes.add("join_build_dense_dup")
                self.dd, self.unique = True, False
                return
            self.c["table_late"] += 1
            self.build_hash_table()

    # ---- probe ----
    def lds_match(self, nulls, distinct):
        f = self.f
        if self.hook("SQLRS_LDS_JOIN") != "1" or nulls or f["nulls"] or f["rows"] < 2 or (not distinct and f["max_run"] > 4096):
            return False
        if distinct:
            if not self.table or f["distinct"] < 2:
                return False
            self.scopes.add("join_build_lds_distinct")
        self.c["lds_distinct" if distinct else "lds_unique"] += 1
        self.scopes |= {"join_partition_lds", "join_probe_lds"}
        return True

    def probe(self, rows, nulls, all_hit, pairs, aligned=True, semi_ok=False):
        """one synchronous probe batch: `nulls`: its key column has NULLs; `all_hit`: every row has a partner; `pairs`: pairs it emits"""
        ah = self.hook("SQLRS_PROBE_ALLHIT") != "0"
        if semi_ok and self.semi and self.jt == "inner":
            self.resolve()
            if self.dense and not nulls and rows >= (1 << 16):
                self.scopes.add("join_semi_mask")
                return
        if self.pending and not self.outer_right and not nulls and rows >= (1 << 16) and self.bits and ah:
            self.scopes.add("join_probe_dense")
            self.c["probe_pending"] += 1
            self.resolve()
            if self.dense and all_hit:
                self.c["allhit_kept"] += 1
                return
            self.c["allhit_redone"] += 1
            if self.dense:
                self.miss_seen = True
        self.resolve()
        lm = False
        if self.lds_first and not self.table and self.unique and not self.outer_right and not self.dense and rows > 0:
            lm = self.lds_match(nulls, False)
        if not lm:
            self.ensure_table()
        if rows == 0:
            return
        if not lm and self.unique and not self.outer_right and not self.dense:
            lm = self.lds_match(nulls, False)
        if self.unique and not self.outer_right:
            if self.dense and not lm and not nulls and rows >= (1 << 16) and not self.miss_seen and ah:
                self.scopes.add("join_probe_dense")
                if all_hit:
                    self.c["allhit_kept"] += 1
                    return
                self.c["allhit_redone"] += 1
                self.miss_seen = True
            if lm:
                self.scopes.add("join_match_compact")
            elif self.dense:
                self.c["compact_dense"] += 1
                self.scopes.add("join_probe_dense")
            else:
                self.c["compact_slots"] += 1
                self.scopes.add("join_probe_unique")
            return
        lmg = False
        if not self.dense and not self.dd and (not self.unique or self.outer_right):
            lmg = self.lds_match(nulls, not self.unique)
        if self.unique and self.outer_right and not lmg:
            self.c["unique_outer"] += 1
            self.scopes.add("join_probe_unique")
            return
        self.c["counts_grouped" if self.hook("SQLRS_JOIN_GROUPED") != "0" else "counts_per_row"] += 1
        if lmg:
            self.scopes.add("join_match_unpermute")
        elif self.dd:
            self.scopes.add("join_probe_count_dense_dup")
            self.c["dd_stream" if (not nulls and rows >= 512 and aligned) else "dd_rows"] += 1
        else:
            self.scopes.add("join_probe_count")
        if pairs:
            self.scopes.add("join_probe_fill")

    def async_probe(self):
        """a batch the one-launch kernels take: the table it reads is there (sa_probe_try / sa_probe_general_try, csrc/join_async.hip)"""
        self.resolve()
        if not self.dense:
            self.ensure_table()
        self.c["async_fast_batches"] += 1


@pytest.fixture(scope="module")
def hip():
    """a ctx of this module's own (stream, pool, profile): the profile entries and route counts these runs leave behind stay out
    of the session's shared ctx, whose profile other modules read by entry name"""
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


# ---- one run ---------------------------------------------------------------------------------------------------------------------
def batch_facts(case, probes, jt):
    """per probe batch (rows, key NULLs, every row has a partner, pairs emitted before the filter) — from the model alone"""
    m = M.JoinModel(case.build, E.LKEY, jt)
    out = []
    for p in probes:
        left, right = m.raw_pairs(p, E.RKEY)
        have = len({r for l, r in zip(left, right) if l is not None})
        out.append((p.num_rows, p.column(E.RKEY).null_count > 0, have == p.num_rows, len(left)))
    return out


@functools.lru_cache(maxsize=None)
def expectation(name, jt, sel, what):
    """the model's output, computed once per (case, join type, selection of probe batches): `what` = pairs | batches | filtered | facts"""
    case = E.case(name)
    probes = [case.probes[i] for i in sel]
    if what == "facts":
        return batch_facts(case, probes, jt)
    if what == "pairs":
        return M.index_pairs(case.build, probes, E.LKEY, E.RKEY, jt)
    return M.join(case.build, probes, E.LKEY, E.RKEY, jt, E.filter_of(case) if what == "filtered" else None, case.right_types())


def run_sync(hip, monkeypatch, case, jt, sel=None, env=None, indices=False, filtered=False, label=""):
    """the synchronous operator over the probe batches `sel` (indices; default: all) of the case inside a route block, compared
    with the model"""
    sel = tuple(range(len(case.probes))) if sel is None else tuple(sel)
    probes = [case.probes[i] for i in sel]
    env = env or {}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    label = f"{case.name} {jt} {env or ''} {'pairs' if indices else 'batches'} {'filtered' if filtered else ''} {label}"
    plan = Plan(case.facts, jt, env, key_only_semi=case.payload == "key_only")
    for rows, nulls, all_hit, pairs in expectation(case.name, jt, sel, "facts"):
        plan.probe(rows, nulls, all_hit, pairs, semi_ok=not indices and not filtered)
    exp = expectation(case.name, jt, sel, "pairs" if indices else ("filtered" if filtered else "batches"))
    with route(hip, label, plan):
        got = E.run(hip, case, jt, probes=probes, filt=E.filter_of(case) if filtered else None, indices_only=indices)
    M.compare(got, exp, label)
    for k in env:
        monkeypatch.delenv(k)
    return plan


def both_outputs(hip, monkeypatch, case, jt, env=None):
    """index pairs and joined batches with the tail, over all probe batches of the case and over its first batch alone"""
    run_sync(hip, monkeypatch, case, jt, None, env, indices=True)
    run_sync(hip, monkeypatch, case, jt, None, env)
    run_sync(hip, monkeypatch, case, jt, (0,), env, label="one batch")


# ---- the direct-address table ----------------------------------------------------------------------------------------------------
DENSE_FORMS = {"deferred": {}, "decided_at_build": {"SQLRS_DENSE_BUILD_DEFER": "0"}, "plain_table": {"SQLRS_DENSE_PACKED": "0"},
               "two_fetch": {"SQLRS_DENSE_BUILD_ONE_FETCH": "0"}, "no_all_hit": {"SQLRS_PROBE_ALLHIT": "0"}}


@pytest.mark.parametrize("jt", E.JOIN_TYPES)
@pytest.mark.parametrize("form", list(DENSE_FORMS))
@pytest.mark.parametrize("name", E.names("dense"))
def test_direct_address_table(hip, monkeypatch, name, form, jt):
    """unique keys over an admissible range: one-fetch or two-fetch build, packed or 4-byte table, the verdict at the build or
    left on the device for the first probe, all-hit attempts kept and redone, the compacting kernel, the unique outer kernel"""
    both_outputs(hip, monkeypatch, E.case(name), jt, DENSE_FORMS[form])


@pytest.mark.parametrize("jt", E.JOIN_TYPES)
@pytest.mark.parametrize("name", ["i64_dense_65536_all_hit", "i64_dense_65535"])
def test_all_hit_probe_first_and_later(hip, monkeypatch, name, jt):
    """the first batch on the device-side verdict (kept when every row hits), later batches on the host's; a batch with a miss
    switches the attempts off for the rest of the join (probe_miss_seen)"""
    case = E.case(name)
    plan = run_sync(hip, monkeypatch, case, jt)
    if jt in ("inner", "left"):
        assert plan.c["probe_pending"] == 1 and plan.c["allhit_kept"] >= 1
        assert (plan.c["allhit_redone"] == 1) == (name == "i64_dense_65535"), plan.c
    plan = run_sync(hip, monkeypatch, case, jt, env={"SQLRS_DENSE_BUILD_DEFER": "0"}, indices=True)
    assert plan.c["probe_pending"] == 0 and (jt in ("right", "full") or plan.c["allhit_kept"] >= 1)
    run_sync(hip, monkeypatch, case, jt, range(len(case.probes) - 1, -1, -1), env={"SQLRS_DENSE_PACKED": "0"})


def test_a_range_one_beyond_the_table_is_refused(hip, monkeypatch):
    """4 x rows + 1024 keys of range are adopted, one more is refused — on both builds; SQLRS_DENSE_JOIN_SLOTS_PLAIN moves the bound"""
    for jt in ("inner", "full"):
        for env in ({}, {"SQLRS_DENSE_BUILD_ONE_FETCH": "0"}, {"SQLRS_DENSE_BUILD_DEFER": "0"}):
            p = run_sync(hip, monkeypatch, E.case("i64_range_exact"), jt, env=env)
            assert p.c["dense_adopted"] == 1 and p.c["dense_refused"] == 0
            p = run_sync(hip, monkeypatch, E.case("i64_range_exact_plus_1"), jt, env=env)
            assert p.c["dense_adopted"] == 0 and p.c["dense_refused"] == 1
        p = run_sync(hip, monkeypatch, E.case("i64_range_exact_plus_1"), jt, env={"SQLRS_DENSE_JOIN_SLOTS_PLAIN": "5"})
        assert p.c["dense_adopted"] == 1
        p = run_sync(hip, monkeypatch, E.case("i64_range_exact"), jt, env={"SQLRS_DENSE_JOIN_SLOTS_PLAIN": "3"})
        assert p.c["dense_refused"] == 1


@pytest.mark.parametrize("jt", E.JOIN_TYPES)
@pytest.mark.parametrize("name", ["i64_dense_around_zero", "i64_twice_dense", "i64_twice_sparse", "f64_pool_unique"])
def test_empty_batches_and_an_empty_tail(hip, name, jt):
    """a probe batch of no row and one that visits every build row: an empty joined batch, and for Left / Full an empty tail —
    batches, not nothing (pinned against the oracle in test_join_model_cpu.py); a build child without a batch emits nothing"""
    case = E.case(name)
    keys = pa.Table.from_batches(case.build).column(E.LKEY).combine_chunks()
    every = pa.RecordBatch.from_arrays([keys if c == E.RKEY else pa.nulls(len(keys), f.type) for c, f in enumerate(case.probes[0].schema)],
                                       names=case.probes[0].schema.names)
    probes = [case.probes[0].slice(0, 0), every]
    plan = Plan(case.facts, jt)
    for rows, nulls, all_hit, pairs in batch_facts(case, probes, jt):
        plan.probe(rows, nulls, all_hit, pairs)
    exp = M.join(case.build, probes, E.LKEY, E.RKEY, jt, None, case.right_types())
    assert exp[0].num_rows == 0 and (jt in ("inner", "right") or exp[-1].num_rows == 0)
    with route(hip, f"{name} {jt} empty outputs", plan):
        got = E.run(hip, case, jt, probes=probes)
    M.compare(got, exp, f"{name} {jt} empty outputs")
    nothing = Plan(case.facts, jt)
    nothing.c.clear()
    nothing.scopes.clear()
    with route(hip, f"{name} {jt} no build batch", nothing):
        assert E.run(hip, case, jt, build=[]) == [] and E.run(hip, case, jt, build=[], indices_only=True) == []


# ---- duplicate keys over a dense range -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jt", E.JOIN_TYPES)
@pytest.mark.parametrize("form", ["grouped", "per_row", "two_fetch"])
@pytest.mark.parametrize("name", E.names("dd"))
def test_runs_by_key_over_a_dense_range(hip, monkeypatch, name, form, jt):
    """dd_table: dd_count_stream_kernel for aligned batches of >= 512 rows without NULL keys, dd_count_kernel otherwise; pair
    counts per 64-row group or per row"""
    env = {"grouped": {}, "per_row": {"SQLRS_JOIN_GROUPED": "0"}, "two_fetch": {"SQLRS_DENSE_BUILD_ONE_FETCH": "0"}}[form]
    case = E.case(name)
    plan = run_sync(hip, monkeypatch, case, jt, env=env)
    assert plan.c["dd_rows"] >= 1 and (plan.c["dd_stream"] >= 1 or max(p.num_rows for p in case.probes) < 512), plan.c
    run_sync(hip, monkeypatch, case, jt, env=env, indices=True)
    run_sync(hip, monkeypatch, case, jt, (0,), env=env, label="one batch")


# ---- the 16-byte-slot table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jt", E.JOIN_TYPES)
@pytest.mark.parametrize("form", ["one_fetch", "two_fetch", "per_row"])
@pytest.mark.parametrize("name", E.names(("slots", "slots_dup")))
def test_slot_table(hip, monkeypatch, name, form, jt):
    """keys the direct-address table refuses — both ends of int64 among them, on the fixed range decision —, doubles, several NULL
    keys: the slot table, unique (compacting probe, unique outer kernel) or with CSR runs (count + fill)"""
    env = {"one_fetch": {}, "two_fetch": {"SQLRS_DENSE_BUILD_ONE_FETCH": "0"}, "per_row": {"SQLRS_JOIN_GROUPED": "0"}}[form]
    case = E.case(name)
    if form == "per_row" and not case.dup:
        env = {"SQLRS_DENSE_BUILD_DEFER": "0"}  # (no count pass over unique keys: the verdict at the build instead)
    nb = len(case.probes)
    sel = tuple(range(nb)) if case.facts["rows"] < 60_000 or form == "one_fetch" else (nb - 2, nb - 1)
    plan = run_sync(hip, monkeypatch, case, jt, sel, env=env)
    assert plan.c["dense_adopted"] == 0 and (case.kind == "f64" or plan.c["dense_refused"] == 1), plan.c
    run_sync(hip, monkeypatch, case, jt, sel, env=env, indices=True)
    run_sync(hip, monkeypatch, case, jt, sel[:1], env=env, label="one batch")


# ---- LDS bucket tables -----------------------------------------------------------------------------------------------------------
LDS_CASES = [n for n in E.names(("slots", "slots_dup")) if E.case(n).facts["rows"] >= 700 and E.case(n).facts["nulls"] == 0]


@pytest.mark.parametrize("jt", E.JOIN_TYPES)
@pytest.mark.parametrize("form", ["lds_first", "table_first", "rpi_1", "per_row"])
@pytest.mark.parametrize("name", LDS_CASES)
def test_lds_tables(hip, monkeypatch, name, form, jt):
    """SQLRS_LDS_JOIN=1: unique build keys matched on LDS tables of the keys (compacted, or un-permuted for Right / Full), duplicate
    keys on tables of the distinct keys; uniqueness from the LDS tables and the slot table built late by a batch with NULL keys
    (SQLRS_LDS_FIRST), one range per work item (SQLRS_LJ_RPI=1: several table builds per bucket)"""
    env = {"SQLRS_LDS_JOIN": "1"}
    env.update({"lds_first": {}, "table_first": {"SQLRS_LDS_FIRST": "0"}, "rpi_1": {"SQLRS_LJ_RPI": "1"}, "per_row": {"SQLRS_JOIN_GROUPED": "0"}}[form])
    case = E.case(name)
    plan = run_sync(hip, monkeypatch, case, jt, env=env)
    assert plan.c["lds_distinct" if case.dup else "lds_unique"] >= 1, plan.c
    if form == "lds_first" and not case.dup and jt in ("inner", "left"):
        assert plan.c["table_late"] == 1, plan.c  # (every such case has a batch with NULL probe keys)
    run_sync(hip, monkeypatch, case, jt, (0, 1), env=env, indices=True)


# ---- join filter on the synchronous path -----------------------------------------------------------------------------------------
FILTER_CASES = ["i64_extremes_2_hit_max", "i64_dense_around_zero", "i64_dense_one_null", "i64_dense_three_nulls", "i64_slot_wrap_twice",
                "i64_twice_dense", "i64_twice_sparse", "f64_pool_unique", "i32_extremes", "bool_true_and_null", "i64_three_build_batches_sparse"]


@pytest.mark.parametrize("jt", E.JOIN_TYPES)
@pytest.mark.parametrize("name", FILTER_CASES)
def test_join_filter(hip, monkeypatch, name, jt):
    """l.i > r.w over the candidate pairs: NULL on every (NULL, row) candidate; Right / Full re-append the probe rows that lost all
    their pairs behind the survivors; only surviving pairs mark build rows as visited (the tail)"""
    case = E.case(name)
    run_sync(hip, monkeypatch, case, jt, filtered=True)
    run_sync(hip, monkeypatch, case, jt, (0,), filtered=True, env={"SQLRS_DENSE_BUILD_DEFER": "0"}, label="one batch")


# ---- probe key buffers that are not 16-byte aligned -------------------------------------------------------------------------------
def device_slice(hip, batch, skip):
    """`batch` (no NULL anywhere) on the device, seen from row `skip` on: column pointers moved by skip x width bytes"""
    dev = hip.to_device(batch)
    cols = []
    for c in range(batch.num_columns):
        col = dev.column(c)
        width = {abi.INT32: 4, abi.INT64: 8, abi.FLOAT64: 8}[col.dtype]
        cols.append(abi.device_column(col.dtype, batch.num_rows - skip, col.values + skip * width))
    return abi.RawBatch(cols, batch.num_rows - skip, keepalive=dev)


@pytest.mark.parametrize("jt", E.JOIN_TYPES)
@pytest.mark.parametrize("name,rows", [("i64_dense_65536_all_hit", 2 ** 16 + 1), ("i64_dense_65535", 70_001), ("i64_twice_dense", 4096), ("i32_dense_twice_at_max", 512),
                                       ("i64_extremes_60000", 513)])
def test_probe_keys_at_an_odd_offset(hip, monkeypatch, name, rows, jt):
    """the probe batch on the device from row 0 (16-byte aligned key column) and from row 1 (8 bytes off: the all-hit kernel's
    8-byte loads, dd_count_kernel in place of the streaming kernel; an int32 key is widened into a buffer of the library's own)"""
    case = E.case(name)
    src = next(p for p in case.probes if p.num_rows >= rows and p.column(E.RKEY).null_count == 0)
    names = src.schema.names[:3]
    whole = pa.RecordBatch.from_arrays([pa.array(np.arange(rows, dtype=np.float64)), src.column(1).slice(0, rows),
                                        pa.array((np.arange(rows) % 7 - 3).astype(np.int32))], names=names)
    sub = pa.RecordBatch.from_arrays([whole.column(c) for c in range(3)], names=names)
    small = E.Case(case.name, case.kind, case.route, case.build, [sub], "numeric" if case.payload != "key_only" else "key_only", facts=case.facts)
    for skip in (0, 1):
        host = whole.slice(skip)
        plan = Plan(case.facts, jt, {}, key_only_semi=case.payload == "key_only")
        for r, nulls, all_hit, pairs in batch_facts(case, [host], jt):
            plan.probe(r, nulls, all_hit, pairs, aligned=(skip == 0) or case.kind == "i32", semi_ok=True)
        exp = M.join(case.build, [host], E.LKEY, E.RKEY, jt, None, small.right_types())
        label = f"{name} {jt} from row {skip}"
        with route(hip, label, plan):
            got = E.run(hip, small, jt, probes=[device_slice(hip, whole, skip)])
        M.compare(got, exp, label)


# ---- the one-launch async kernels ------------------------------------------------------------------------------------------------
ASYNC_CASES = ["i64_extremes_2_hit_min", "i64_dense_around_2p31", "i64_dense_at_max_256", "i64_dense_255", "i64_range_exact_plus_1",
               "f64_pool_twice", "i32_dense_at_min", "i32_dense_twice_at_max"]


def whole_build(case):
    return pa.Table.from_batches(case.build).combine_chunks().to_batches()[0]


@pytest.mark.parametrize("depth", [1, 8])
@pytest.mark.parametrize("jt", E.JOIN_TYPES)
@pytest.mark.parametrize("name", ASYNC_CASES)
def test_async_probe(hip, monkeypatch, name, jt, depth):
    """sqlrs_hash_join_probe_push_async with async_general and async_utf8 on: batches of <= 4096 rows without NULL probe keys take
    one launch (async_fast_batches, by the header's rule restated in async_utf8_cases.eligible), the others the synchronous
    operator inside the stream; with a join filter and async_filter on; and with SQLRS_ASYNC_FAST=0 (every batch synchronous)"""
    case = E.case(name)
    lb = whole_build(case)
    m_run = case.facts["max_run"]  # (by key identity: numpy's unique would merge the NaN payloads of a float64 key)
    probes = [p for p in case.probes if p.num_rows <= 5000]
    filt = E.filter_of(case)
    for filtered, fast in ((False, True), (True, True), (False, False)):
        env = {} if fast else {"SQLRS_ASYNC_FAST": "0"}
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        plan = Plan(case.facts, jt, env)
        for p, (rows, nulls, all_hit, pairs) in zip(probes, batch_facts(case, probes, jt)):
            if filtered:
                ok = fast and AF.filter_compiles(filt, AF.joined_dtypes(lb, p)) and AU.eligible(lb, p, E.LKEY, E.RKEY, jt, m_run, True, True)
            else:
                ok = fast and AU.eligible(lb, p, E.LKEY, E.RKEY, jt, m_run, True, True)
            if ok:
                plan.async_probe()
            else:
                plan.probe(rows, nulls, all_hit, pairs)
        assert not fast or plan.c["async_fast_batches"] >= 2, (name, jt, plan.c)
        exp = M.join(case.build, probes, E.LKEY, E.RKEY, jt, filt if filtered else None, case.right_types())
        label = f"{name} {jt} depth {depth} {'filtered' if filtered else ''} {env}"
        with route(hip, label, plan):
            got = E.run(hip, case, jt, probes=probes, filt=filt if filtered else None, depth=depth, async_general=True, async_utf8=True,
                        async_filter=True)
        M.compare(got, exp, label)
        for k in env:
            monkeypatch.delenv(k)


# ---- the lazy table of a join + aggregate ------------------------------------------------------------------------------------------
def test_join_agg_over_the_extreme_keys(hip):
    """HashJoinAggExecutor over 270 unique build keys that hold INT64_MIN, INT64_MAX and -1 (agg_edge_cases' full64 key space):
    the join's table is lazy — the direct-address attempt (16 slots per key, 4-byte table, decided at the build) is refused on
    the fixed range decision, and the composed route's first probe builds the slot table.  Expected values from agg_model over
    the join written out row by row."""
    n = 5000
    probe = AE.build("join_extremes", n, 91, groups=300, keyspace="full64")
    uniq = np.unique(probe.keys)
    assert AE.INT64_MIN in uniq and AE.INT64_MAX in uniq and -1 in uniq
    rng = np.random.default_rng(92)
    keep = (rng.random(len(uniq)) >= 0.1) | np.isin(uniq, [AE.INT64_MIN, AE.INT64_MAX, -1])
    bkeys = rng.permutation(uniq[keep])
    build_batch = pa.RecordBatch.from_arrays([pa.array(bkeys), pa.array(np.arange(len(bkeys), dtype=np.int64))], names=["bk", "attr"])
    rows = np.nonzero(np.isin(probe.keys, bkeys))[0]
    assert 0 < len(rows) < n
    joined = AE.Case("joined_extremes", probe.keys[rows], None, {c: (v[rows], None if valid is None else valid[rows]) for c, (v, valid) in probe.cols.items()},
                     [0, len(rows)])
    funcs = [("count", "f"), ("sum", "f"), ("min", "f"), ("max", "f"), ("sum", "i"), ("min", "i"), ("max", "i")]
    pb = probe.batches()
    schema = pa.schema([(f"b.{f.name}", f.type) for f in build_batch.schema] + [(f"p.{f.name}", f.type) for f in pb[0].schema])
    facts = dict(rows=len(bkeys), nulls=0, lo=int(bkeys.min()), hi=int(bkeys.max()), unique=True, distinct=len(bkeys), kind="i64", key_only=False, max_run=1)
    plan = Plan(facts, "inner", {}, lazy=True)
    assert plan.c["dense_refused"] == 1 and plan.c["dense_plain"] == 1 and not plan.table
    for b in pb:
        plan.probe(b.num_rows, False, False, 1)
    assert plan.c["table_late"] == 1
    ex = HashJoinAggExecutor(hip, [build_batch], pb, JoinCondition([(InputRef(0), InputRef(0))]), schema, 2, AE.agg_funcs(funcs, first_col=3), [InputRef(0)])
    with route(hip, "join+aggregate over the extreme keys", plan):
        got = pa.Table.from_batches([b for b in ex.execute() if b is not None])
    assert ex.fused_batches == 0
    AM.compare(got, joined.model(funcs), "join+aggregate over the extreme keys")


# ---- SQLRS_JOIN_COMPOSITE over a column that holds both ends of int64 --------------------------------------------------------------
def test_composite_key_falls_back_to_hashes_over_the_extremes(hip, oracle, monkeypatch):
    """two int64 key columns, the first holds INT64_MIN and INT64_MAX: its range is all 2^64 values (0 after the wrap), the
    composite key does not exist and the join runs on hashes — no direct-address attempt (an exact composite key makes one) —
    with the rows it emits without the switch, which are the oracle's.  Without the extremes the same shape IS composed: an exact
    key (the model's pairs over the (a, b) tuples; the hashes' false matches are gone), duplicate keys over a dense range."""
    rng = np.random.default_rng(7)
    nb, npr = 900, 3000
    for extremes in (True, False):
        k1 = rng.integers(-50, 50, nb)
        if extremes:
            k1[[5, 700]] = [E.I64_MIN, E.I64_MAX]
        k2 = np.arange(nb, dtype=np.int64) % 30
        lb = pa.RecordBatch.from_arrays([pa.array(k1), pa.array(k2), pa.array(np.arange(nb, dtype=np.int64))], names=["a", "b", "x"])
        at = rng.integers(0, nb, npr)
        p1, p2 = k1[at].copy(), k2[at].copy()
        p2[rng.random(npr) < 0.3] = 31
        rb = pa.RecordBatch.from_arrays([pa.array(p1), pa.array(p2), pa.array(rng.random(npr))], names=["a", "b", "v"])
        cond = JoinCondition([(InputRef(0), InputRef(0)), (InputRef(1), InputRef(1))])
        sch = pa.schema([(f"l.{f.name}", f.type) for f in lb.schema] + [(f"r.{f.name}", f.type) for f in rb.schema])
        tuples = list(zip(k1.tolist(), k2.tolist()))
        runs = Counter(tuples)
        span2 = int(k2.max() - k2.min()) + 1
        comp = [(a - int(k1.min())) * span2 + (b - int(k2.min())) for a, b in tuples]  # (the composite key of join.hip, when it exists)
        common = dict(rows=nb, nulls=0, unique=len(runs) == nb, distinct=len(runs), key_only=False, max_run=max(runs.values()))
        hashed = dict(common, kind="f64", lo=None, hi=None)  # (hashes: no direct-address attempt, like a double)
        composed = dict(common, kind="i64", lo=min(comp), hi=max(comp))
        build_tuples = set(tuples)
        probes = [rb, rb.slice(0, 65)]
        for jt in ("inner", "full"):
            outs = {}
            for switch in ("0", "1"):
                monkeypatch.setenv("SQLRS_JOIN_COMPOSITE", switch)
                plan = Plan(composed if switch == "1" and not extremes else hashed, jt)
                assert plan.c["dense_one_fetch"] == (1 if switch == "1" and not extremes else 0)
                for p in probes:
                    hits = [t in build_tuples for t in zip(p.column(0).to_pylist(), p.column(1).to_pylist())]
                    plan.probe(p.num_rows, False, all(hits), sum(hits) + (jt == "full"))
                with route(hip, f"composite: extremes {extremes} {jt} switch {switch}", plan):
                    outs[switch] = list(HashJoinExecutor(hip, [lb], probes, jt, cond, sch, 3).execute())
            monkeypatch.delenv("SQLRS_JOIN_COMPOSITE")
            exp = list(HashJoinExecutor(oracle, [lb], probes, jt, cond, sch, 3).execute())
            M.compare(outs["0"], exp, f"composite {extremes} {jt}: hashes against the oracle")
            if extremes:
                M.compare(outs["1"], outs["0"], f"composite {extremes} {jt}: with the switch against without")
            else:  # (the tuples numbered: one exact key for the model, taken out of its output again)
                ids = {t: i for i, t in enumerate(dict.fromkeys(tuples))}
                with_id = lambda b: b.append_column("id", pa.array([ids.get(t, -1) for t in zip(b.column(0).to_pylist(), b.column(1).to_pylist())], type=pa.int64()))  # noqa: E731
                exact = M.join([with_id(lb)], [with_id(p) for p in probes], 3, 3, jt)
                M.compare(outs["1"], [b.select([0, 1, 2, 4, 5, 6]) for b in exact], f"composite {extremes} {jt}: exact tuples")
