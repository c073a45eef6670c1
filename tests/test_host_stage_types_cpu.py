"""SQLRS_EXPR_STAGE_ALL_TYPES without a GPU: the switch is declared alike in the header, the ctypes mirror and the generated
Rust bindings, and the staging bookkeeping + the two stitch functions of sqlrs_amd/csrc/stage_stitch.hpp — host code, built
into a stand-alone program under AddressSanitizer / UBSan — reproduce the concatenation that tests/host_stage_cases.py
restates in numpy, for every row list crossed with every validity shape and every Utf8 shape."""
import inspect
import os
import re
import shutil
import subprocess
import sys

import host_stage_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_switch_is_declared_alike_everywhere():
    from sqlrs_amd import abi
    header = open(os.path.join(ROOT, "include", "sqlrs_hip.h")).read()
    h = re.search(r"^#define\s+SQLRS_EXPR_STAGE_ALL_TYPES\s+(\d+)\s*$", header, flags=re.M)
    assert h, "sqlrs_hip.h does not define SQLRS_EXPR_STAGE_ALL_TYPES"
    assert int(h.group(1)) == abi.EXPR_STAGE_ALL_TYPES == 1
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi as gen
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert gen.emit(*gen.parse_header(header)) == ffi, "include/sqlrs_hip.h changed: run python tools/gen_rust_ffi.py"
    assert re.search(r"^pub const SQLRS_EXPR_STAGE_ALL_TYPES: i32 = 1;$", ffi, flags=re.M)
    assert len(re.findall(r"^\s*pub fn sqlrs_", ffi, flags=re.M)) == 118  # a flag of the create calls, not an entry point


def test_executors_take_the_switch_and_default_to_off():
    from sqlrs_amd.executor import HashAggExecutor, HashJoinAggExecutor, HashJoinExecutor, OrderExecutor
    for cls in (HashAggExecutor, HashJoinExecutor, HashJoinAggExecutor, OrderExecutor):
        assert inspect.signature(cls.__init__).parameters["stage_all_types"].default is False, cls
    for path, n in (("host/sqlrs_executor.hpp", 4), ("bindings/rust/src/executors.rs", 4)):
        text = open(os.path.join(ROOT, path)).read()
        assert len(re.findall(r"^\s*(?:pub |bool )stage_all_types\b|pub stage_all_types: bool", text, flags=re.M)) >= n, path


def test_profile_read_returns_every_entry():
    """the two counts are reported behind every existing entry: a ctx whose profile holds more than 64 entries (scopes of a long
    session plus every route count) must not lose them — Backend.profile_read reads again with room for what the call reports"""
    from sqlrs_amd import abi
    total, calls = 100, []

    class Stub:
        ctx = None

        def fn(self, name):
            assert name == "ctx_profile_read"

            def read(ctx, cap, names, ms, launches):
                calls.append(cap)
                for k in range(min(cap, total)):
                    names[k], ms[k], launches[k] = f"entry_{k}".encode(), 0.0, k + 1
                return total
            return read
    prof = abi.Backend.profile_read(Stub())
    assert len(prof) == total and prof["entry_99"] == (0.0, 100) and calls[0] < total <= calls[-1]


def test_case_lists_cover_the_shapes():
    cases = H.cpu_cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for ln in H.ROW_LISTS:
        assert {n.split("/")[1] for n in names if n.startswith(ln + "/")} == set(H.VALIDITY_SHAPES), ln
        assert {n.split("/")[2] for n in names if n.startswith(ln + "/")} == set(H.UTF8_SHAPES), ln
    assert sum(H.ROW_LISTS["F64"]) == 64 and sum(H.ROW_LISTS["F65"]) == 65 and len(H.ROW_LISTS["A"]) == 130
    by = {c.name: c for c in cases}
    c = by["C/minus_one/window37"]
    assert all(p.cols[2].offsets[0] >= 37 for p in c.pieces) and all(p.cols[2].null_count == -1 for p in c.pieces)
    assert any(len(x or "") == 5000 for p in by["C/minus_one/long5000"].pieces for x in p.cols[2].logical)
    assert all(p.cols[2].values is None for p in by["B/minus_one/values_null"].pieces)
    tail = [p for p in by["B/tail_ones/" + H.UTF8_SHAPES[(1 + 5) % 5]].pieces if p.n & 7]
    assert tail and all(p.cols[1].validity[-1] >> (p.n & 7) == 0xFF >> (p.n & 7) and p.cols[3].values[-1] >> (p.n & 7) == 0xFF >> (p.n & 7) for p in tail)
    # the model drops the validity of a column without NULLs and counts the NULLs itself
    assert all(v is None and n == 0 for n, v, _ in H.model_concat(by["B/present_zero/" + H.UTF8_SHAPES[(1 + 2) % 5]]))
    m = H.model_concat(by["C/minus_one/window37"])
    assert m[0][0] == 0 and all(n > 0 and v is not None for n, v, _ in m[1:])
    assert H.digest_bytes(b"") == 0xCBF29CE484222325 and H.digest_bytes(b"\x00") == (0xCBF29CE484222325 * 0x100000001B3 + 1) % (1 << 64)


def test_stage_stitch_header_under_sanitizers(tmp_path):
    """host/stage_stitch_check.cpp over sqlrs_amd/csrc/stage_stitch.hpp, with -fsanitize=address,undefined: the pieces of every
    case go through the header's bookkeeping, stitch_bits_word / stitch_offset run for every word and row, the program itself
    compares with a naive concatenation, and its digest per case equals the numpy restatement's (host_stage_cases.case_digest);
    then the cap decision at 100 bytes"""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed (the oracle is built with it too)"
    exe = str(tmp_path / "stage_stitch_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "sqlrs_amd", "csrc"), os.path.join(ROOT, "host", "stage_stitch_check.cpp"), "-o", exe], check=True)
    cases = H.cpu_cases()
    path = str(tmp_path / "cases.bin")
    H.write_cases(path, cases)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "cap ok"
    got = {int(i): int(d, 16) for i, d in (line.split() for line in lines[:-1])}
    want = {i: H.case_digest(c) for i, c in enumerate(cases)}
    assert got == want, [cases[i].name for i in want if got.get(i) != want[i]]
