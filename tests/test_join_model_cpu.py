"""The join model (join_model.py) and its cases (join_edge_cases.py) checked without a GPU:

* the model against the CPU oracle on every case and join type: index pairs, joined batches and tail, with and without a join
  filter.  The oracle matches by hash alone; on ONE fixed-width key its hash rule and the model's exact identity must coincide
  (a case where they do not is a finding for DESIGN.md, not something to mask);
* whether an empty tail / an empty joined batch is a batch or nothing;
* the conditions every case must meet, computed from the model alone;
* planted faults: each is applied to the EXPECTED output of the model, never to a library, and `compare` must reject it;
* the stand-alone program over dense_range_decide (host/dense_range_check.cpp), built with -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pyarrow as pa
import pytest

import join_edge_cases as E
import join_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(E.all_cases())
WITH_PAYLOAD = [n for n in CASES if E.case(n).payload != "key_only"]


def expected(case, jt, filt=None, probes=None):
    return M.join(case.build, case.probes if probes is None else probes, E.LKEY, E.RKEY, jt, filt, case.right_types())


# ---- model = oracle --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jt", E.JOIN_TYPES)
@pytest.mark.parametrize("name", CASES)
def test_model_agrees_with_the_oracle(oracle, name, jt):
    case = E.case(name)
    M.compare(E.run(oracle, case, jt, indices_only=True), M.index_pairs(case.build, case.probes, E.LKEY, E.RKEY, jt), f"{name} {jt} pairs")
    M.compare(E.run(oracle, case, jt), expected(case, jt), f"{name} {jt} batches")


@pytest.mark.parametrize("jt", E.JOIN_TYPES)
@pytest.mark.parametrize("name", WITH_PAYLOAD)
def test_model_agrees_with_the_oracle_under_a_join_filter(oracle, name, jt):
    case = E.case(name)
    if case.facts["rows"] >= 60_000:
        probes = case.probes[-2:]  # (the filter is evaluated row by row in Python)
    else:
        probes = case.probes
    filt = E.filter_of(case)
    M.compare(E.run(oracle, case, jt, probes=probes, filt=filt), expected(case, jt, filt, probes), f"{name} {jt} filtered")


def test_empty_outputs_are_batches_and_an_empty_build_child_emits_nothing(oracle):
    """one joined batch per probe batch even without a pair; Left / Full: the tail even when every build row was visited;
    Inner / Right: no tail; a build child without any batch: nothing at all"""
    case = E.case("i64_dense_around_zero")
    all_rows = case.build[0]
    probe_all = pa.RecordBatch.from_arrays([all_rows.column(0) if c == E.RKEY else pa.nulls(all_rows.num_rows, f.type)
                                            for c, f in enumerate(case.probes[0].schema)], names=case.probes[0].schema.names)
    no_hit = case.probes[0].slice(0, 0)
    for jt in E.JOIN_TYPES:
        got = E.run(oracle, case, jt, probes=[no_hit, probe_all])
        exp = expected(case, jt, probes=[no_hit, probe_all])
        assert len(exp) == (3 if jt in ("left", "full") else 2)
        assert exp[0].num_rows == 0 and exp[1].num_rows == all_rows.num_rows and (len(exp) == 2 or exp[2].num_rows == 0)
        M.compare(got, exp, f"empty outputs {jt}")
        assert E.run(oracle, case, jt, build=[]) == [] and M.join([], case.probes, E.LKEY, E.RKEY, jt) == []
        assert E.run(oracle, case, jt, build=[], indices_only=True) == [] and M.index_pairs([], case.probes, E.LKEY, E.RKEY, jt) == []


# ---- the conditions of every case ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_every_case_meets_its_conditions(name):
    case = E.case(name)
    m = M.JoinModel(case.build, E.LKEY, "full")
    matched = unmatched = longest = 0
    for p in case.probes:
        left, right = m.pairs(p, E.RKEY)
        matched += sum(1 for l in left if l is not None)
        unmatched += sum(1 for l in left if l is None)
        run = 0
        for i, r in enumerate(right):
            run = run + 1 if i and right[i - 1] == r else 1
            longest = max(longest, run)
    assert matched >= 1, name
    assert (unmatched == 0) == case.all_hit, (name, unmatched)
    assert len(m.tail_rows()) >= 1, name
    assert (longest >= 2) == case.dup, (name, longest)
    # the route family the case is made for, from its facts (the admissible range of the direct-address table: 4 x rows + 1024)
    f = case.facts
    span_ok = f["kind"] != "f64" and f["lo"] is not None and f["hi"] - f["lo"] + 1 <= 4 * f["rows"] + 1024
    unique = f["unique"] and f["nulls"] <= 1
    want = ("dense" if unique else ("dd" if f["nulls"] == 0 else "slots_dup")) if span_ok else ("slots" if unique else "slots_dup")
    assert case.route == want, (name, case.route, want)
    assert all(p.num_rows <= (1 << 18) for p in case.probes)


def test_the_pools_and_probe_sizes_of_the_issue_are_covered():
    keys = {"i64": set(), "i32": set(), "f64": set(), "bool": set()}
    probed = {"i64": set(), "i32": set(), "f64": set(), "bool": set()}
    sizes = set()
    for c in E.all_cases().values():
        for b in c.build:
            keys[c.kind] |= set(M.key_ids(b.column(E.LKEY)))
        for p in c.probes:
            probed[c.kind] |= set(M.key_ids(p.column(E.RKEY)))
            sizes.add(p.num_rows)
    for kind, pool in (("i64", E.POOL_I64), ("i32", E.POOL_I32), ("f64", E.POOL_F64), ("bool", [0, 1, None])):
        assert set(pool) <= keys[kind], (kind, set(pool) - keys[kind])
        assert set(pool) <= probed[kind], (kind, set(pool) - probed[kind])
    assert set(E.PROBE_SIZES) <= sizes, set(E.PROBE_SIZES) - sizes
    assert {c.facts["rows"] for c in E.all_cases().values()} >= {255, 256, 257, 65535, 65536, 60_000}


# ---- planted faults --------------------------------------------------------------------------------------------------------------
def rejected(got, exp) -> bool:
    try:
        M.compare(got, exp)
    except AssertionError:
        return True
    return False


def pairs_of(name, jt, filt=None):
    """(case, model, [(probe, left, right)] of the final pairs)"""
    case = E.case(name)
    m = M.JoinModel(case.build, E.LKEY, jt, filt)
    return case, m, [(p,) + m.pairs(p, E.RKEY) for p in case.probes]


def index_batches(m, per_batch):
    return [m.index_batch(l, r) for _, l, r in per_batch]


def joined_batches(m, per_batch):
    return [m.joined(p, l, r) for p, l, r in per_batch]


def edit_first(per_batch, fn):
    """applies fn(probe, left, right) -> (left, right) | None to the first batch where it returns something"""
    out, done = [], False
    for p, l, r in per_batch:
        e = None if done else fn(p, list(l), list(r))
        if e is not None:
            done = True
            l, r = e
        out.append((p, l, r))
    assert done, "nothing to plant the fault on"
    return out


def drop_probe_key(key):
    def fn(p, l, r):
        ids = M.key_ids(p.column(E.RKEY))
        keep = [i for i in range(len(r)) if not (ids[r[i]] == key and l[i] is not None)]
        return None if len(keep) == len(r) else ([l[i] for i in keep], [r[i] for i in keep])
    return fn


def rematch(m, probe_key, build_key):
    """the pairs of probe rows with `probe_key` given the build row of `build_key` instead"""
    def fn(p, l, r):
        ids = M.key_ids(p.column(E.RKEY))
        hit = [i for i in range(len(r)) if ids[r[i]] == probe_key and l[i] is not None]
        if not hit:
            return None
        for i in hit:
            l[i] = m.rows_of[build_key][0]
        return l, r
    return fn


def test_the_expectation_passes_its_own_comparison():
    for name in ("i64_twice_sparse", "f64_pool_unique", "i64_slot_wrap"):
        for jt in E.JOIN_TYPES:
            _, m, pb = pairs_of(name, jt)
            M.compare(index_batches(m, pb), index_batches(m, pb))
            M.compare(joined_batches(m, pb), joined_batches(m, pb))


def test_fault_two_pairs_of_one_run_swapped():
    for name in ("i64_twice_sparse", "i64_twice_dense", "f64_pool_twice"):
        _, m, pb = pairs_of(name, "inner")

        def fn(p, l, r):
            for i in range(1, len(r)):
                if r[i] == r[i - 1]:
                    l[i], l[i - 1] = l[i - 1], l[i]
                    return l, r
        bad = edit_first(pb, fn)
        assert rejected(index_batches(m, bad), index_batches(m, pb)), name
        assert rejected(joined_batches(m, bad), joined_batches(m, pb)), name


def test_fault_the_null_pair_dropped():
    for name in ("i64_dense_one_null", "i64_slot_wrap", "i64_dense_three_nulls"):
        _, m, pb = pairs_of(name, "inner")
        bad = edit_first(pb, drop_probe_key(None))
        assert rejected(index_batches(m, bad), index_batches(m, pb)), name
        assert rejected(joined_batches(m, bad), joined_batches(m, pb)), name


def test_fault_negative_zero_matched_to_zero():
    """the joined rows differ only in the sign bit of l.k (and in the payload of the other build row)"""
    _, m, pb = pairs_of("f64_pool_unique", "inner")
    bad = edit_first(pb, rematch(m, 0x8000000000000000, 0x0))
    assert rejected(index_batches(m, bad), index_batches(m, pb))
    key_only = lambda bs: [b.select([0]) for b in bs]  # noqa: E731  (l.k alone: -0.0 == 0.0 as doubles, not as bit patterns)
    assert rejected(key_only(joined_batches(m, bad)), key_only(joined_batches(m, pb)))


def test_fault_two_nan_payloads_merged():
    _, m, pb = pairs_of("f64_pool_unique", "inner")
    for probe_key, build_key in ((0x7FF8000000000000, 0x7FFFFFFFFFFFFFFF), (0xFFF8000000000001, 0xFFFFFFFFFFFFFFFF)):
        bad = edit_first(pb, rematch(m, probe_key, build_key))
        assert rejected(index_batches(m, bad), index_batches(m, pb))
        key_only = lambda bs: [b.select([0]) for b in bs]  # noqa: E731
        assert rejected(key_only(joined_batches(m, bad)), key_only(joined_batches(m, pb)))


def test_fault_key_minus_one_lost():
    for name in ("i64_slot_wrap", "i64_dense_around_zero", "i64_twice_sparse"):
        _, m, pb = pairs_of(name, "inner")
        assert rejected(index_batches(m, edit_first(pb, drop_probe_key(-1))), index_batches(m, pb)), name
    _, m, pb = pairs_of("f64_pool_unique", "inner")
    assert rejected(index_batches(m, edit_first(pb, drop_probe_key(0xFFFFFFFFFFFFFFFF))), index_batches(m, pb))


def test_fault_the_int64_max_row_lost():
    for name in ("i64_extremes_2_hit_max", "i64_extremes_60000", "i64_dense_at_max_256"):
        _, m, pb = pairs_of(name, "inner")
        bad = edit_first(pb, drop_probe_key(E.I64_MAX))
        assert rejected(index_batches(m, bad), index_batches(m, pb)), name
        assert rejected(joined_batches(m, bad), joined_batches(m, pb)), name
    _, m, pb = pairs_of("i64_extremes_2_hit_min", "inner")
    assert rejected(index_batches(m, edit_first(pb, drop_probe_key(E.I64_MIN))), index_batches(m, pb))


def test_fault_an_unmatched_right_row_moved_to_the_end():
    for name in ("i64_dense_around_zero", "i64_twice_sparse", "i64_extremes_2_hit_max"):
        for jt in ("right", "full"):
            _, m, pb = pairs_of(name, jt)

            def fn(p, l, r):
                for i in range(len(r) - 1):
                    if l[i] is None:
                        return l[:i] + l[i + 1:] + [None], r[:i] + r[i + 1:] + [r[i]]
            bad = edit_first(pb, fn)
            assert rejected(index_batches(m, bad), index_batches(m, pb)), (name, jt)
            assert rejected(joined_batches(m, bad), joined_batches(m, pb)), (name, jt)


def test_fault_filter_orphans_left_in_place():
    """Right / Full with a join filter: a probe row whose pairs all failed the filter is reported where its first pair stood"""
    for name in ("i64_dense_around_zero", "i64_twice_sparse", "f64_pool_unique"):
        for jt in ("right", "full"):
            case = E.case(name)
            filt = E.filter_of(case)
            m = M.JoinModel(case.build, E.LKEY, jt, filt)
            exp, bad, differs = [], [], 0
            for p in case.probes:
                l, r = m.pairs(p, E.RKEY, mark=False)
                exp.append(m.joined(p, l, r))
                survivors = {(a, b) for a, b in zip(l, r) if a is not None}
                have = {b for _, b in survivors}
                rl, rr = m.raw_pairs(p, E.RKEY)
                bl, br, seen = [], [], set()
                for a, b in zip(rl, rr):
                    if (a, b) in survivors:
                        bl.append(a)
                        br.append(b)
                    elif b not in have and b not in seen:
                        seen.add(b)
                        bl.append(None)
                        br.append(b)
                differs += (bl, br) != (l, r)
                bad.append(m.joined(p, bl, br))
            assert differs, (name, jt)
            assert rejected(bad, exp), (name, jt)


def test_fault_the_tail_in_reverse_order():
    for name in ("i64_dense_around_zero", "i64_extremes_60000", "i64_twice_sparse"):
        case = E.case(name)
        exp = expected(case, "left")
        tail = exp[-1]
        assert tail.num_rows >= 2
        rev = tail.take(pa.array(list(range(tail.num_rows - 1, -1, -1))))
        assert rejected(exp[:-1] + [rev], exp), name


def _replace(batch, c, arr):
    cols = [batch.column(i) for i in range(batch.num_columns)]
    cols[c] = arr
    return pa.RecordBatch.from_arrays(cols, names=batch.schema.names)


def test_fault_one_payload_validity_bit_flipped():
    for name in ("i64_dense_around_zero", "f64_pool_unique"):
        case = E.case(name)
        exp = expected(case, "full")
        b = next(i for i, x in enumerate(exp) if x.num_rows)
        for c in range(1, exp[b].num_columns):
            col = exp[b].column(c).to_pylist()
            row = next(i for i, v in enumerate(col) if v is not None)
            col[row] = None
            assert rejected(exp[:b] + [_replace(exp[b], c, pa.array(col, type=exp[b].column(c).type))] + exp[b + 1:], exp), (name, c)


def test_fault_one_utf8_payload_emptied():
    for name in ("i64_dense_around_zero", "i64_three_build_batches_sparse"):
        case = E.case(name)
        exp = expected(case, "inner")
        planted = 0
        for c in range(exp[0].num_columns):
            if exp[0].column(c).type != pa.string():
                continue
            b = next(i for i, x in enumerate(exp) if any(v for v in x.column(c).to_pylist()))
            col = exp[b].column(c).to_pylist()
            col[next(i for i, v in enumerate(col) if v)] = ""
            assert rejected(exp[:b] + [_replace(exp[b], c, pa.array(col, type=pa.string()))] + exp[b + 1:], exp), (name, c)
            planted += 1
        assert planted == 2, name  # (one Utf8 column on each side)


# ---- the range decision of the direct-address table ------------------------------------------------------------------------------
def test_dense_range_decision_under_sanitizers(tmp_path):
    """host/dense_range_check.cpp over sqlrs_amd/csrc/dense_range.hpp: (0, ~0) and (0, ~0 - 1) refused, exactly max_range accepted
    and one more refused, span 2^31 - 2 accepted and 2^31 - 1 refused, lo > hi refused, one key accepted with range 1"""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed (the oracle is built with it too)"
    exe = str(tmp_path / "dense_range_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "sqlrs_amd", "csrc"), os.path.join(ROOT, "host", "dense_range_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 of " in r.stdout
