"""The device CSV parser's rules, restated on the host (sqlrs_amd/csvparse.py), against pyarrow.csv: separator ranks ->
(row, column), blank lines, the first ragged record; and the exact-float rule against float().  No GPU."""
import glob
import os
import struct

import numpy as np
import pyarrow as pa
import pyarrow.csv as pacsv
import pytest

from sqlrs_amd import csvparse

CSV_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "csv")


def pyarrow_text(data: bytes, tmp_path, header=True):
    """every field of every record as pyarrow reads it, all columns as strings"""
    p = tmp_path / "f.csv"
    p.write_bytes(data)
    first = data.split(b"\n", 1)[0].rstrip(b"\r").split(b",")
    names = [f.decode() for f in first] if header else [f"f{i}" for i in range(len(first))]
    t = pacsv.read_csv(str(p), read_options=pacsv.ReadOptions(column_names=names, skip_rows=1 if header else 0),
                       convert_options=pacsv.ConvertOptions(strings_can_be_null=False, column_types={n: pa.string() for n in names}))
    return [[v.encode() for v in col.to_pylist()] for col in t.columns]


def quote_free_goldens():
    return sorted(p for p in glob.glob(os.path.join(CSV_DIR, "*.csv")) if b'"' not in open(p, "rb").read())


def test_some_golden_file_is_quote_free():
    assert len(quote_free_goldens()) >= 3


@pytest.mark.parametrize("path", quote_free_goldens(), ids=os.path.basename)
def test_index_fields_on_golden_files(path, tmp_path):
    data = open(path, "rb").read()
    ncols = data.split(b"\n", 1)[0].count(b",") + 1
    recs, bad = csvparse.fields(data, ncols)
    assert bad is None
    exp = pyarrow_text(data, tmp_path)
    assert len(recs) - 1 == len(exp[0])
    for c in range(ncols):
        assert [r[c] for r in recs[1:]] == exp[c]


@pytest.mark.parametrize("variant", sorted(csvparse.VARIANTS))
def test_index_fields_on_the_generated_file(variant, tmp_path):
    data, cols = csvparse.generate(20_000, seed=7, **csvparse.VARIANTS[variant])
    recs, bad = csvparse.fields(data, 4)
    assert bad is None and len(recs) == 20_001 and recs[0] == [b"a", b"b", b"c", b"d"]
    exp = pyarrow_text(data, tmp_path)
    for c in range(4):
        assert [r[c] for r in recs[1:]] == exp[c]
    # ... and typed, pyarrow reads what the generator meant (int64 / double / bool / string, the same NULLs)
    p = tmp_path / "typed.csv"
    p.write_bytes(data)
    t = pacsv.read_csv(str(p), convert_options=pacsv.ConvertOptions(strings_can_be_null=False))
    assert [str(x) for x in t.schema.types] == ["int64", "double", "bool", "string"]
    for c in range(4):
        assert t.column(c).to_pylist() == cols[c]


def test_blank_lines_and_carriage_returns():
    data = b"\n\r\na,b\r\n\r\n\n1,2\n\r\r\n3,\r\n\n"
    recs, bad = csvparse.fields(data, 2)
    # "\r\r\n" is a record of one field "\r" (only ONE trailing '\r' is stripped): ragged for two columns
    assert recs == [[b"a", b"b"], [b"1", b"2"]] and bad == 2
    recs, bad = csvparse.fields(b"x\n\r\r\ny", 1)
    assert recs == [[b"x"], [b"\r"], [b"y"]] and bad is None
    assert csvparse.fields(b"", 3) == ([], None)
    assert csvparse.fields(b"\n\r\n", 3) == ([], None)


@pytest.mark.parametrize("bad_line, row", [(b"4,5\n", 2), (b"4,5,6,7\n", 2), (b"4\n5,6\n", 2)])
def test_first_ragged_record(bad_line, row):
    data = b"a,b,c\n1,2,3\n" + bad_line + b"7,8,9\n1,2\n"
    recs, bad = csvparse.fields(data, 3)
    assert bad == row and recs == [[b"a", b"b", b"c"], [b"1", b"2", b"3"]]


def bits(x: float) -> bytes:
    return struct.pack("<d", x)


def test_generated_easy_floats_are_exact():
    """entitles the GPU test to demand patched_fields == 0"""
    data, cols = csvparse.generate(20_000, seed=3)
    recs, _ = csvparse.fields(data, 4)
    n = 0
    for r in recs[1:]:
        if r[1]:
            v = csvparse.exact_float(r[1])
            assert v is not None and bits(v) == bits(float(r[1])), r[1]
            n += 1
    assert n > 18_000


def test_exact_float_rule_against_float():
    rng = np.random.default_rng(11)
    for _ in range(20_000):
        s = f"{rng.uniform(-1e6, 1e6):.6f}".encode()
        v = csvparse.exact_float(s)
        assert v is not None and bits(v) == bits(float(s)), s
        s = f"{int(rng.integers(0, 10 ** 15))}e{int(rng.integers(-22, 23))}".encode()
        v = csvparse.exact_float(s)
        assert v is not None and bits(v) == bits(float(s)), s
    assert bits(csvparse.exact_float(b"-0.0")) == bits(-0.0)
    assert csvparse.exact_float(b"0007.50") == 7.5 and csvparse.exact_float(b"1E3") == 1000.0
    # outside the rule: left to the host
    for s in [b"9007199254740992", b"1e23", b"1e-23", b"0.00000000000000000000001", b"inf", b"nan", b"1.", b".5", b"1e+5",
              b"", b"-", b"1e", b"12x", repr(0.1 + 0.2).encode()]:
        assert csvparse.exact_float(s) is None, s
