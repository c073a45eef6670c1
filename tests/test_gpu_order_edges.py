"""Every device route of ORDER BY against the independent model (tests/order_model.py) on the cases of
tests/order_edge_cases.py: NaNs of both signs and several payloads, +-inf, +-0.0, subnormals, the ends of int64 and int32, key
ranges of exactly 2^32 - 2 .. 2^32 + 1 and on the steps of the key-bit count, composite fields of 64 and 65 bits, garbage under
NULL slots, validity that flips every 64 rows with its padding bits set, top-k thresholds on a NaN / on -0.0 / on the ends of
int64, Utf8 keys with embedded NULs, bytes >= 0x80 and every length around the 8-byte chunks.  Every column of the result is
compared bit for bit (order_model.compare: validity exactly, doubles as uint64, Utf8 as bytes; no tolerance, nothing left out).

Which route ran is asserted, not assumed: every run sits in a `route(...)` block over the `order_*` counters of
sqlrs_ctx_profile_read.  tests/order_plan.py restates the host-side dispatch of ops.hip / order_fast.hip over the case's data
(key range, key bits, sampled rows, splitters, largest group, heavy values, candidates of a threshold) and the hooks, and the
block asserts that EVERY counter moved by exactly the planned number — the others are at rest ("Route witnesses of
ORDER BY"):

  order_general / order_utf8_key            the LSD path sorted the rows / sorted a Utf8 key with sort_perm_by_utf8 (per key)
  order_narrow / order_narrow_hbm_only      order_fast_impl produced the result / its all-bits-through-HBM second try ran
  order_form_lookback / order_form_counting an attempt's (first) split pass chained over its tiles / counted and scanned
  order_rec12 / order_rec16                 an attempt moved 12-byte {key offset, value} / 16-byte {word, value} records
  order_wide / order_wide_declined          order_wide produced the result / was entered and declined
  order_wide_pure_copy / _finish2 / _finish3  it copied groups of one value / launched the finish beyond 8 / 16 x FIN_WG rows
  order_heavy_to_wide                       the heavy-value probe sent a column of <= 32 varying bits to order_wide
  order_range_sampled / order_range_missed  the key range came from a sample / a key lay outside: the exact retry ran
  order_in_order                            the input was returned as it came
  order_composite / _nullable / _too_wide   order_composite produced the result / with a valid bit / declined beyond 64 bits
  order_null_split, order_topk / order_topk_ignored, order_alloc_declined

Every case of a fast route runs a second time under SQLRS_ORDER_FAST=0: the same input on the general path (`order_general`).
The forms are steered only with hooks the library reads per call (monkeypatch.setenv): SQLRS_ORDER_LB, SQLRS_ORDER_LB_TEST_FAIL,
SQLRS_ORDER_SLIM, SQLRS_ORDER_REC, SQLRS_ORDER_REC1, SQLRS_ORDER_WIDE_REC1, SQLRS_ORDER_TILED, SQLRS_ORDER_FINISH_COUNT,
SQLRS_ORDER_HEAVY_PROBE, SQLRS_ORDER_WIDE, SQLRS_ORDER_COMPOSITE, SQLRS_ORDER_SAMPLE, SQLRS_ORDER_TOPK, SQLRS_ORDER_FAST; each
cross of HOOK_CROSSES names the witness that shows the form.

What no witness can show, and what no input of <= 2^22 rows reaches in this process:

* which form of the in-LDS finish a GROUP takes — bucket + count, LSD passes, the neighbour walk, a run longer than OWK_WALK = 192
  rows — is decided inside ow_finish_kernel / owk_finish_kernel per group: no host decision, no counter.  The forms are reached
  through the conditions in the source instead: ~20 rows per value on 16 key bits and 50 values over 26 bits (more than 24 rows in
  a bucket), 6000 doubles that differ only in their lowest 12 mantissa bits (more than 192 equal top bits of a group: LSD over
  all bits), and every such case again under SQLRS_ORDER_FINISH_COUNT=0 (LSD passes and the neighbour walk only);
* order_wide declining because `n < G * samples` (order_fast.hip: `if (n < S)`): G <= 2^16 groups grow with n so that S = 16 G
  <= n / 128 from 2^20 rows on — and below 2^20 rows no fast route is entered; even SQLRS_ORDER_SAMPLES=256 gives S <= n / 8;
* an optimistic key range chosen by SIZE (order_fast: `n >= 2^24`) and top-k without a carried hook below 2^20 rows: forced with
  SQLRS_ORDER_SAMPLE=1 / SQLRS_ORDER_TOPK=1 as the issue states; `topk_by_the_size_rule` takes the size rule of top-k itself;
* a look-back spin that really runs out (g_order_lb_off, `order_lookback_fallbacks`): decided by timing on the device;
  SQLRS_ORDER_LB_TEST_FAIL=1 / 2 treat an attempt as failed and take the same second try;
* `order_alloc_declined` (ops.hip: a hipMalloc failure of a fast attempt is "route not taken"): needs an exhausted pool; every
  run here asserts it at rest;
* the guards `n > 0xffffffff` and the look-back's `n < 2^30`: beyond 2^22 rows (tests/test_gpu_bench_sizes.py runs 2^28)."""
from contextlib import contextmanager

import pytest

import order_edge_cases as E
import order_model as M
import order_plan as P
from sqlrs_amd import abi
from sqlrs_amd.executor import LimitExecutor

pytestmark = pytest.mark.gpu

HOOKS = ("SQLRS_ORDER_LB", "SQLRS_ORDER_LB_TEST_FAIL", "SQLRS_ORDER_SLIM", "SQLRS_ORDER_REC", "SQLRS_ORDER_REC1", "SQLRS_ORDER_WIDE_REC1",
         "SQLRS_ORDER_TILED", "SQLRS_ORDER_FINISH_COUNT", "SQLRS_ORDER_HEAVY_PROBE", "SQLRS_ORDER_WIDE", "SQLRS_ORDER_COMPOSITE",
         "SQLRS_ORDER_SAMPLE", "SQLRS_ORDER_SAMPLES", "SQLRS_ORDER_TOPK", "SQLRS_ORDER_FAST")
ORDER_COUNTERS = tuple("order_" + k for k in P.COUNTERS)


# ---- which route ran -------------------------------------------------------------------------------------------------------------
counters = P.read_counters


@contextmanager
def route(be, label, plan):
    """asserts how the witnesses move across the block: every order_* route counter by exactly plan[name without order_] (0: at rest)"""
    assert not set(plan) - set(P.COUNTERS), set(plan) - set(P.COUNTERS)
    before = counters(be)
    yield
    after = counters(be)
    moved = {k: after.get(k, 0) - before.get(k, 0) for k in ORDER_COUNTERS}
    seen = {k: v for k, v in moved.items() if v}
    for k in ORDER_COUNTERS:
        assert moved[k] == plan.get(k[6:], 0), f"{label}: {k} moved by {moved[k]}, planned {plan.get(k[6:], 0)}; moved: {seen}; plan: {dict(plan)}"


@pytest.fixture(scope="module")
def hip():
    """a ctx of this module's own (stream, pool, profile): the route counts these runs leave behind stay out of the session's
    shared ctx, whose profile other modules read by entry name"""
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


def run_case(hip, monkeypatch, c, exp, extra=None, label="", batches=None, retain=False):
    """the case on the HIP library under its own hooks and `extra`, inside a route block over the restated dispatch, compared
    with the model; -> the plan that was asserted"""
    env = {**c.env, **(extra or {})}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    label = f"{c.name} {extra or ''} {label}"
    want = P.plan(c, extra)
    with route(hip, label, want):
        got = E.run(hip, c, batches=batches, retain=retain)
    M.compare(got, exp, label)
    for k in env:
        monkeypatch.delenv(k)
    return want


# ---- every case on its route, then on the general path --------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.all_cases())
def test_case_runs_on_its_route_and_matches_the_model(hip, monkeypatch, name):
    c = E.case(name)
    exp = M.expected(c.batches, c.order_by, c.limit, c.offset)
    want = run_case(hip, monkeypatch, c, exp)
    assert not P.intended(c, want), (name, P.intended(c, want), dict(want))
    if c.rows >= 1 << 17 and set(want) - {"general", "utf8_key"}:   # a fast route (or an attempt at one) was involved: the general path alone
        off = run_case(hip, monkeypatch, c, exp, {"SQLRS_ORDER_FAST": "0"})
        assert off["general"] == 1 and not set(off) - {"general", "utf8_key", "topk", "topk_ignored"}, dict(off)


# ---- the forms behind the per-call hooks ----------------------------------------------------------------------------------------
# (hooks, case, the witnesses that must show the form: name -> planned count)
HOOK_CROSSES = [
    ({"SQLRS_ORDER_LB": "0"}, "i64_kbits_2p24", {"form_counting": 1, "form_lookback": 0, "rec16": 1, "rec12": 0, "narrow": 1}),
    ({"SQLRS_ORDER_LB": "0"}, "f64_pool_asc", {"form_counting": 1, "form_lookback": 0, "wide": 1}),
    ({"SQLRS_ORDER_LB": "0"}, "i64_narrow_around_zero", {"form_counting": 1, "rec16": 0, "narrow": 1}),
    ({"SQLRS_ORDER_LB_TEST_FAIL": "1"}, "i64_kbits_2p24", {"form_lookback": 1, "form_counting": 1, "narrow": 1}),
    ({"SQLRS_ORDER_LB_TEST_FAIL": "2"}, "i64_kbits_2p24m1", {"form_lookback": 1, "form_counting": 1, "narrow": 1}),
    ({"SQLRS_ORDER_LB_TEST_FAIL": "1"}, "f64_cluster12_asc", {"form_lookback": 1, "form_counting": 1, "wide": 1}),
    ({"SQLRS_ORDER_LB_TEST_FAIL": "1"}, "comp_fields_64_bits", {"form_lookback": 1, "form_counting": 1, "composite": 1}),
    ({"SQLRS_ORDER_SLIM": "0"}, "i64_kbits_2p16", {"rec12": 0, "rec16": 1, "form_lookback": 1}),
    ({"SQLRS_ORDER_SLIM": "0"}, "f64_narrow_around_zero_asc", {"rec12": 0, "rec16": 1}),
    ({"SQLRS_ORDER_REC": "0"}, "i64_kbits_2p31m1", {"rec16": 0, "rec12": 0, "form_counting": 1}),
    ({"SQLRS_ORDER_REC1": "0"}, "i64_kbits_2p31m1", {"rec16": 1, "rec12": 0, "form_counting": 1}),
    ({"SQLRS_ORDER_TILED": "0"}, "i64_kbits_2p31m1", {"rec16": 0, "form_counting": 1}),
    ({"SQLRS_ORDER_TILED": "0"}, "f64_narrow_at_one_desc", {"rec16": 0, "form_counting": 1}),
    ({"SQLRS_ORDER_WIDE_REC1": "0"}, "f64_heavy_neg_zero_asc", {"form_counting": 1, "wide": 1, "wide_pure_copy": 1}),
    ({"SQLRS_ORDER_WIDE_REC1": "0"}, "i64_range_2p32_from0", {"form_counting": 1, "wide": 1}),
    ({"SQLRS_ORDER_FINISH_COUNT": "0"}, "f64_cluster12_desc", {"wide": 1}),          # (no witness: the form is the kernel's own)
    ({"SQLRS_ORDER_FINISH_COUNT": "0"}, "f64_heavy_pos_nan_asc", {"wide": 1}),
    ({"SQLRS_ORDER_FINISH_COUNT": "0"}, "i64_kbits_2p16m1", {"narrow": 1}),
    ({"SQLRS_ORDER_FINISH_COUNT": "0"}, "f64_narrow_around_zero_desc", {"narrow": 1}),
    ({"SQLRS_ORDER_FINISH_COUNT": "0"}, "comp_nullable_63_value_bits_desc", {"composite_nullable": 1}),
    ({"SQLRS_ORDER_HEAVY_PROBE": "0"}, "i64_50_values_over_26_bits", {"heavy_to_wide": 0, "narrow_hbm_only": 1, "narrow": 1}),
    ({"SQLRS_ORDER_HEAVY_PROBE": "0"}, "f64_heavy_neg_nan_desc", {"heavy_to_wide": 0, "wide": 1}),
    ({"SQLRS_ORDER_WIDE": "0"}, "f64_pool_asc", {"general": 1, "wide": 0, "wide_declined": 0}),
    ({"SQLRS_ORDER_WIDE": "0"}, "i64_range_2p32_straddle", {"general": 1, "wide": 0}),
    ({"SQLRS_ORDER_WIDE": "0"}, "comp_fields_64_bits", {"general": 1, "composite": 0}),
    ({"SQLRS_ORDER_WIDE": "0"}, "i64_50_values_over_26_bits", {"heavy_to_wide": 1, "narrow_hbm_only": 1, "narrow": 1}),
    ({"SQLRS_ORDER_COMPOSITE": "0"}, "comp_constant_key_among_others", {"general": 1, "composite": 0}),
    ({"SQLRS_ORDER_COMPOSITE": "0"}, "comp_nullable_63_value_bits_desc", {"general": 1, "composite": 0}),
    ({"SQLRS_ORDER_COMPOSITE": "0"}, "comp_nullable_64_value_bits", {"null_split": 1, "composite_too_wide": 0}),
    ({"SQLRS_ORDER_SAMPLE": "1"}, "i32_min_max_full", {"range_sampled": 1, "range_missed": 1, "narrow": 1}),   # no key bit left: the exact pass
    ({"SQLRS_ORDER_SAMPLE": "1"}, "f64_heavy_neg_nan_asc", {"range_sampled": 1, "range_missed": 0, "wide": 1}),
    ({"SQLRS_ORDER_SAMPLE": "1"}, "f64_narrow_near_neg_top_end", {"range_sampled": 1, "narrow": 1}),
    ({"SQLRS_ORDER_SAMPLE": "1"}, "i64_narrow_at_min", {"range_sampled": 1, "narrow": 1}),
    ({"SQLRS_ORDER_SAMPLE": "1"}, "i64_narrow_at_max", {"range_sampled": 1, "narrow": 1}),
    ({"SQLRS_ORDER_SAMPLE": "1"}, "comp_fields_64_bits", {"range_sampled": 1, "composite": 1}),
    ({"SQLRS_ORDER_SAMPLE": "1"}, "in_order_asc_ties", {"range_sampled": 1, "in_order": 1}),
    ({"SQLRS_ORDER_SAMPLE": "1"}, "nsplit_f64_nulls_and_nans", {"range_sampled": 1, "null_split": 1}),
    ({"SQLRS_ORDER_SAMPLE": "0"}, "i64_sampled_missed_both", {"range_sampled": 0, "range_missed": 0, "narrow": 1}),
    ({"SQLRS_ORDER_TOPK": "0"}, "topk_ties_at_the_threshold", {"topk": 0, "general": 1}),
    ({"SQLRS_ORDER_TOPK": "0"}, "topk_by_the_size_rule", {"topk": 0, "wide": 1}),
]


@pytest.mark.parametrize("hooks,name,shows", HOOK_CROSSES, ids=[f"{'+'.join(f'{k[12:]}={v}' for k, v in h.items())}-{n}" for h, n, _ in HOOK_CROSSES])
def test_forms_behind_the_hooks(hip, monkeypatch, hooks, name, shows):
    c = E.case(name)
    exp = M.expected(c.batches, c.order_by, c.limit, c.offset)
    want = run_case(hip, monkeypatch, c, exp, hooks)
    for k, v in shows.items():
        assert want.get(k, 0) == v, f"{name} {hooks}: the restated dispatch plans {k} = {want.get(k, 0)}, the cross is made for {v}; plan: {dict(want)}"


# ---- input forms -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["i64_kbits_2p24", "in_order_asc_ties", "f64_pool_desc", "comp_fields_64_bits", "gen_utf8_asc_4097"])
def test_retained_device_batches(hip, monkeypatch, name):
    """sqlrs_order_push_retained over DEVICE batches the caller keeps alive (order.rs:19-26 keeps Arcs): borrowed columns, which
    the in-order return must copy before it hands them out"""
    c = E.case(name)
    exp = M.expected(c.batches, c.order_by, c.limit, c.offset)
    # (a Limit without limit or offset hands its FIRST batch through as it is: one per batch)
    dev = [next(iter(LimitExecutor(hip, None, None, [b], out_mem=abi.MEM_DEVICE).execute())) for b in c.batches if b.num_rows]
    try:
        run_case(hip, monkeypatch, c, exp, label="retained", batches=dev, retain=True)
    finally:
        for b in dev:
            b.release()
