"""sqlrs_hash_join_set_async_keys off the GPU: the library exports the setter and the header, abi.py and ffi.rs declare it alike;
the rule tests/async_keys_cases.py restates gives the counts worked out by hand for every case, and every mixed case is mixed;
the cases hold what they are for, checked on the oracle's output; and host/key_hash_check.cpp — csrc/key_hash.hpp under
AddressSanitizer and UBSan — computes the keys the Python restatement of the arithmetic computes."""
import inspect
import os
import re
import shutil
import subprocess

import pyarrow as pa
import pytest

import async_keys_cases as cases
from async_utf8_cases import offsets_of
from sqlrs_amd import abi
from sqlrs_amd.executor import HashJoinExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def join_schema(lb, rb):
    return pa.schema([pa.field(f"l.{f.name}", f.type) for f in lb.schema] + [pa.field(f"r.{f.name}", f.type) for f in rb.schema])


def oracle_run(oracle, case, jt, **kw):
    return list(HashJoinExecutor(oracle, [case.lb], case.rbs, jt, case.cond, join_schema(case.lb, case.rbs[0]), case.lb.num_columns, **kw).execute())


def test_the_library_exports_the_setter_and_the_declarations_agree():
    import ctypes
    from sqlrs_amd import build as b
    assert os.path.exists(b.OUT), "build() has produced the library"
    lib = ctypes.CDLL(b.OUT)  # (loads without a GPU)
    assert getattr(lib, "sqlrs_hash_join_set_async_keys", None) is not None
    header = open(os.path.join(ROOT, "include", "sqlrs_hip.h")).read()
    m = re.search(r"\bint\s+sqlrs_hash_join_set_async_keys\s*\(([^)]*)\)\s*;", header)
    assert m, "the header declares sqlrs_hash_join_set_async_keys"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 2 and params[0].startswith("sqlrs_hash_join_t *") and params[1].startswith("int ")
    d = re.search(r'"hash_join_set_async_keys":\s*\((\w+),\s*\[([^\]]*)\]\)', inspect.getsource(abi.Backend._declare))
    assert d and d.group(1) == "i" and [a.strip() for a in d.group(2).split(",")] == ["vp", "C.c_int"]
    assert "async_keys" in inspect.signature(HashJoinExecutor.__init__).parameters


def test_ffi_rs_is_in_sync_and_declares_the_setter():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi as gen
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    with open(gen.HEADER) as f:
        assert gen.emit(*gen.parse_header(f.read())) == ffi, "include/sqlrs_hip.h changed: run python tools/gen_rust_ffi.py"
    assert re.search(r"pub fn sqlrs_hash_join_set_async_keys\(j: \*mut sqlrs_hash_join_t, on: c_int\) -> c_int;", ffi)
    assert len(re.findall(r"^\s*pub fn sqlrs_", ffi, flags=re.M)) == 118
    for doc in ("bindings/rust/README.md", "INTEGRATION.md"):
        assert "118" in open(os.path.join(ROOT, doc)).read(), doc


def test_oracle_runs_unchanged_with_the_flag(oracle):
    assert getattr(oracle.lib, oracle.prefix + "hash_join_set_async_keys", None) is None
    c = cases.unique_pair_case()
    for jt in cases.JOIN_TYPES:
        exp = oracle_run(oracle, c, jt)
        got = oracle_run(oracle, c, jt, depth=3, async_general=True, async_utf8=True, async_keys=True)
        assert len(got) == len(exp) and all(g.equals(e) for g, e in zip(got, exp))


@pytest.mark.parametrize("case", cases.mixed_cases(), ids=repr)
def test_the_rule_gives_the_hand_counts_and_every_case_is_mixed(case):
    want = case.want
    mixed = 0
    for (jt, general), n in sorted(want.items()):
        got = cases.count_eligible(case, jt, general)
        print(f"{case.name} {jt} general={general}: eligible {got} of {len(case.rbs)}, by hand {n}")
        assert got == n, (case.name, jt, general)
        mixed += 0 < n < len(case.rbs)
    assert mixed >= 1, case.name
    assert want[("inner", True)] > 0 and want[("left", True)] > 0
    # the switches compose: without the Utf8 switch a case with a Utf8 column admits nothing; without the filter switch a filtered join
    # admits nothing; the rule as it was (keys = False) admits only batches of an exact key without a NULL in it
    has_str = any(cases.is_str(f.type) for f in list(case.lb.schema) + list(case.rbs[0].schema))
    if has_str:
        assert all(cases.count_eligible(case, jt, True, utf8=False) == 0 for jt in cases.JOIN_TYPES)
    if case.filter is not None:
        assert all(cases.count_eligible(case, jt, True, filt=False) == 0 for jt in cases.JOIN_TYPES)
    m = cases.max_run(case.lb, case.on)
    for jt in cases.JOIN_TYPES:
        old = cases.count_eligible(case, jt, True, keys=False)
        if not cases.exact_mode(case.lb, case.on):
            assert old == 0
        else:
            assert old == sum(1 for b in case.rbs if not b.column(case.on[0][1]).null_count and cases.eligible(case, b, jt, m, True))
            assert old < want[(jt, True)]  # (every exact case has NULL probe keys in batches the switch adds)


@pytest.mark.parametrize("what", ["five", "bool", "expr"])
def test_refused_keys_admit_nothing(what):
    case = cases.refused_case(what)
    for jt in cases.JOIN_TYPES:
        for general in (False, True):
            assert cases.count_eligible(case, jt, general) == 0 == case.want[(jt, general)]


@pytest.mark.parametrize("e", cases.EXACT, ids=lambda e: "_".join(map(str, e)))
def test_exact_cases_hold_what_they_are_for(oracle, e):
    dtype, form, nnull = e
    c = cases.exact_case(*e)
    assert c.lb.column(0).null_count == nnull
    m = cases.max_run(c.lb, c.on)
    assert m == (4 if form.startswith("dup") else max(nnull, 1))
    assert [b.num_rows for b in c.rbs] == cases.SIZES
    for b in c.rbs:
        pat, k = cases.PATTERNS[b.num_rows], b.column(0)
        valid = [k[i].is_valid for i in range(len(k))]
        if pat == "all":
            assert k.null_count == len(k) > 0
        if "first" in pat:
            assert not valid[0]
        if "last" in pat:
            assert not valid[-1]
        if "6364" in pat:
            assert not valid[63] and (len(k) < 65 or not valid[64])
        if pat == "bitmap":
            assert k.null_count == 0 and k.buffers()[0] is not None
    # the value of an existing build key sits under NULL slots of the probe key column
    import numpy as np
    kv = np.frombuffer(c.lb.column(0).buffers()[1], dtype=cases.DTYPES[dtype])[:c.lb.num_rows]
    live = set(kv[[i for i in range(c.lb.num_rows) if c.lb.column(0)[i].is_valid]].tolist())
    assert kv[1].item() in live
    b = c.rbs[8]
    raw = np.frombuffer(b.column(0).buffers()[1], dtype=cases.DTYPES[dtype])[:b.num_rows]
    assert any(raw[i].item() == kv[1].item() for i in range(b.num_rows) if not b.column(0)[i].is_valid)
    # on the oracle's output: NULL probe keys find the NULL build rows (nnull each), other rows find partners, some find none
    right = oracle_run(oracle, c, "right")
    nleft = c.lb.num_columns
    for b, out in zip(c.rbs, right):
        rows = list(zip(*[out.column(i).to_pylist() for i in range(out.num_columns)]))
        null_probe = [r for r in rows if r[nleft] is None]
        assert len(null_probe) == b.column(0).null_count * max(nnull, 1)
        assert all((r[0] is None) for r in null_probe)  # (their partner's key is NULL too — or there is no partner)
        if b.num_rows >= 63:
            hits = [r for r in rows if r[nleft] is not None and r[0] is not None]
            miss = [r for r in rows if r[nleft] is not None and r[0] is None]
            assert (hits or cases.PATTERNS[b.num_rows] == "all") and (miss or cases.PATTERNS[b.num_rows] == "all")


def test_hashed_cases_hold_what_they_are_for(oracle):
    for dup in (False, True):
        c = cases.utf8_case(dup)
        assert cases.max_run(c.lb, c.on) == (4 if dup else 1)
        keys = set(c.lb.column(0).to_pylist())
        assert {"", "ab", "abc", "abd", "prefix", "prefixx", None} <= keys and ("L" * 200 in keys) == (not dup)
        assert all(int(offsets_of(b.column(1))[0]) == 5 for b in c.rbs)  # (probe offsets start at 5)
        nulls = [i for b in c.rbs[5:6] for i in range(b.num_rows) if not b.column(1)[i].is_valid]
        assert nulls and any(offsets_of(c.rbs[5].column(1))[i + 1] > offsets_of(c.rbs[5].column(1))[i] for i in nulls)  # bytes under NULL slots
        inner = oracle_run(oracle, c, "inner")
        nleft = c.lb.num_columns
        seen = set()
        for out in inner:
            seen |= set(out.column(0).to_pylist())
            assert out.column(0).to_pylist() == out.column(nleft + 1).to_pylist()  # (no false match among these strings; NULL = NULL)
        assert {"", "a", "ab", "abc", "abd", None, "é"} <= seen
        right = oracle_run(oracle, c, "right")
        assert any(l is None and r is not None for out in right for l, r in zip(out.column(0).to_pylist(), out.column(nleft + 1).to_pylist()))
    up = cases.unique_pair_case()
    assert cases.max_run(up.lb, up.on) == 1
    inner = oracle_run(oracle, up, "inner")
    swapped = sum(1 for out in inner for a, ra in zip(out.column(0).to_pylist(), out.column(3).to_pylist()) if a is not None and ra is not None and a != ra)
    assert swapped > 0  # (a + 1000, a) found (a, a + 1000): match-by-hash
    mm = cases.mismatch_case()
    assert all(out.num_rows == 0 for out in oracle_run(oracle, mm, "inner"))
    same = cases.Case("same_types", mm.lb, [pa.RecordBatch.from_arrays([b.column(0).cast(pa.int64()), b.column(1)], names=["a", "b"]) for b in mm.rbs], mm.on, None)
    assert all(out.num_rows == b.num_rows for out, b in zip(oracle_run(oracle, same, "inner"), same.rbs))  # (with int64 every row hits)
    for name in cases.MULTI:
        c = cases.multi_case(name)
        m = cases.max_run(c.lb, c.on)
        assert m == cases.MULTI_M[name], (name, m)
        for i, (l, r) in enumerate(c.on):  # a NULL in every key position, on both sides
            assert c.lb.column(l).null_count > 0 and all(b.column(r).null_count > 0 for b in c.rbs if b.num_rows >= 1023), (name, i)
        inner = oracle_run(oracle, c, "inner")
        assert sum(o.num_rows for o in inner) > 0
        right = oracle_run(oracle, c, "right")
        assert any(v is None for out in right for v in out.column(c.lb.num_columns - 1).to_pylist())
    f = cases.filter_case()
    assert f.lb.column(0)[0].is_valid is False and f.lb.column(1)[0].as_py() == -100
    left = oracle_run(oracle, f, "inner")
    assert all(k is not None for out in left for k in out.column(0).to_pylist())  # (the filter kept every NULL = NULL pair out)
    nofilt = cases.Case("nofilt", f.lb, f.rbs, f.on, None)
    assert any(k is None for out in oracle_run(oracle, nofilt, "inner") for k in out.column(0).to_pylist())
    b = cases.bound_case()
    m = cases.max_run(b.lb, b.on)
    assert m == 2 and b.rbs[1].num_rows == b.rbs[0].num_rows + 1 == b.r_ok + 1
    assert cases.out_bytes(b.lb, b.rbs[0], 2 * b.r_ok) <= cases.SA_AREA < cases.out_bytes(b.lb, b.rbs[1], 2 * (b.r_ok + 1))
    assert cases.SA_AREA - cases.out_bytes(b.lb, b.rbs[0], 2 * b.r_ok) < 400  # (just under: less than two rows' worth)
    mixed = sum(0 < cases.count_eligible(c, jt, g) < len(c.rbs) for c, jt, g, _ in map(cases.fuzz_case, cases.FUZZ_SEEDS))
    assert mixed >= 4


def test_key_hash_header_under_sanitizers(tmp_path):
    """host/key_hash_check.cpp over sqlrs_amd/csrc/key_hash.hpp, with -fsanitize=address,undefined: the key of every row of the
    three fixed tables equals the Python restatement's (async_keys_cases.row_key) — empty string versus NULL, prefixes, a 200-byte
    string, multi-byte UTF-8, swapped values (one key), a NULL in every position, INT64_MIN, -0.0"""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed (the oracle is built with it too)"
    exe = str(tmp_path / "key_hash_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "sqlrs_amd", "csrc"), os.path.join(ROOT, "host", "key_hash_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {(int(t), int(row)): int(key, 16) for t, row, key in (line.split() for line in r.stdout.splitlines())}
    want = {(t, row): cases.row_key(kinds, vals) for t, (kinds, rows) in enumerate(cases.KEY_TABLES) for row, vals in enumerate(rows)}
    assert got == want
    assert want[(1, 0)] == want[(1, 1)] and want[(1, 2)] == want[(1, 3)] and want[(1, 4)] == 0 == want[(2, 6)]  # swapped; NULL either side; all NULL
    assert want[(0, 0)] != want[(0, 1)] == 0  # the empty string is not NULL
    assert len({want[(0, r)] for r in range(10)}) == 10
