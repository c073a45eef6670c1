"""Quoted fields on the device (sqlrs_csv_set_device_quotes, csrc/csv_device.hip): with the switch on, a piece whose quotes
are all regular is parsed by the gfx950 kernels, any other piece by the host parser — and the stream of batches stays the
host parser's, batch for batch and bit for bit.  Reference = the host parser of the same library, second opinion =
pyarrow.csv.  A lane owns 16 bytes of a piece, a wave 1 KiB, a tile 4 KiB: the files are the smallest that put a quote on
each of those boundaries."""
import ctypes as C
import os

import numpy as np
import pyarrow as pa
import pyarrow.csv as pacsv
import pytest

from sqlrs_amd import abi, csvparse
from sqlrs_amd.executor import CsvScan, HashAggExecutor, ProjectExecutor
from sqlrs_amd.expr import AggFunc, InputRef

pytestmark = pytest.mark.gpu
CSV_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "csv")
KIB = 1024
ROWS = 20_000


def run(hip, path, device_parse=None, device_quotes=None, **kw):
    """-> (scan, HOST arrow batches, the error the scan ended with or None); DEVICE batches are brought down column by
    column through a Project of bare column references (the rows do not move)"""
    scan = CsvScan(hip, str(path), device_parse=device_parse, device_quotes=device_quotes, **kw)
    out, err = [], None
    try:
        for b in scan.execute():
            if kw.get("out_mem", abi.MEM_HOST) == abi.MEM_DEVICE:
                ncols = len(scan.names)
                (b,) = list(ProjectExecutor(hip, [InputRef(i) for i in range(ncols)], [b]).execute())
            out.append(b)
    except abi.ExecutorError as e:
        err = e
    return scan, out, err


def same_column(g, e):
    assert g.type == e.type and len(g) == len(e) and g.null_count == e.null_count
    if pa.types.is_floating(g.type):  # bit for bit (NaN, -0.0)
        assert g.is_null().equals(e.is_null())
        gb = np.asarray(g.fill_null(0.0)).view(np.uint64)
        eb = np.asarray(e.fill_null(0.0)).view(np.uint64)
        assert np.array_equal(gb, eb)
    else:
        assert g.equals(e)


def same_stream(got, exp):
    assert [b.num_rows for b in got] == [b.num_rows for b in exp]
    for g, e in zip(got, exp):
        assert g.num_columns == e.num_columns
        for c in range(g.num_columns):
            same_column(g.column(c), e.column(c))


def check_against_host(hip, path, device_parse, device_quotes=1, **kw):
    hs, exp, herr = run(hip, path, **kw)
    ds, got, derr = run(hip, path, device_parse=device_parse, device_quotes=device_quotes, **kw)
    assert ds.names == hs.names and ds.dtypes == hs.dtypes
    same_stream(got, exp)
    assert (derr is None) == (herr is None)
    if herr is not None:
        assert derr.status == herr.status and str(derr) == str(herr)
    rows = sum(b.num_rows for b in got)
    assert ds.stats["device_rows"] + ds.stats["host_rows"] == rows
    return ds, got, rows


TYPES = {"a": pa.int64(), "b": pa.float64(), "c": pa.bool_(), "d": pa.string()}


def pyarrow_table(path):
    return pacsv.read_csv(str(path), parse_options=pacsv.ParseOptions(newlines_in_values=True),
                          convert_options=pacsv.ConvertOptions(strings_can_be_null=False, column_types=TYPES))


# ---- 1. / 2. / 8. the seeded quoted file -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    d = tmp_path_factory.mktemp("csvquoted")
    out = {}
    for name, eol in (("lf", "\n"), ("crlf", "\r\n")):
        data, cols = csvparse.generate_quoted(ROWS, seed=5, eol=eol)
        p = d / (name + ".csv")
        p.write_bytes(data)
        out[name] = (str(p), cols)
    return out


@pytest.fixture(scope="module")
def host_streams(hip, generated):
    cache = {}

    def get(variant, batch_size):
        if (variant, batch_size) not in cache:
            cache[(variant, batch_size)] = run(hip, generated[variant][0], batch_size=batch_size)[1]
        return cache[(variant, batch_size)]
    return get


@pytest.mark.parametrize("chunk", [4 * KIB, 64 * KIB + 1, -1], ids=["4KiB", "64KiB+1", "default"])
@pytest.mark.parametrize("batch_size", [1000, 65_536])
@pytest.mark.parametrize("variant", ["lf", "crlf"])
def test_generated_quoted_file_is_parsed_on_the_device(hip, generated, host_streams, variant, batch_size, chunk):
    path, cols = generated[variant]
    exp = host_streams(variant, batch_size)
    ds, got, err = run(hip, path, device_parse=chunk, device_quotes=1, batch_size=batch_size)
    assert err is None
    assert ds.dtypes == [abi.INT64, abi.FLOAT64, abi.BOOLEAN, abi.UTF8]
    same_stream(got, exp)
    # the caps: test_csv_quotes_cpu.py shows that the file alone stays within them
    assert ds.stats == {"device_rows": ROWS, "host_rows": 0, "patched_fields": 0}
    if batch_size == 65_536 and chunk == 64 * KIB + 1:  # the second opinion, once per variant
        t = pyarrow_table(path)
        tab = pa.Table.from_batches(got)
        for c in range(4):
            same_column(tab.column(c).combine_chunks(), t.column(c).combine_chunks())
            assert tab.column(c).to_pylist() == cols[c]


def test_generated_quoted_file_into_device_memory(hip, generated):
    path, _ = generated["crlf"]
    ds, got, rows = check_against_host(hip, path, 64 * KIB + 1, batch_size=65_536, out_mem=abi.MEM_DEVICE)
    assert ds.stats == {"device_rows": ROWS, "host_rows": 0, "patched_fields": 0}


@pytest.mark.parametrize("device_quotes", [None, 0], ids=["unset", "0"])
def test_switch_off_is_todays_behaviour(hip, generated, host_streams, device_quotes):
    path, _ = generated["lf"]
    ds, got, err = run(hip, path, device_parse=-1, device_quotes=device_quotes, batch_size=1000)
    assert err is None
    same_stream(got, host_streams("lf", 1000))
    assert ds.stats == {"device_rows": 0, "host_rows": ROWS, "patched_fields": 0}


def test_bounds_and_projection_with_quotes(hip, generated):
    path, cols = generated["lf"]
    for chunk in (-1, 4 * KIB):
        ds, got, rows = check_against_host(hip, path, chunk, bounds=(1000, 30), projection=[3, 0])
        assert rows == 30 and ds.stats["device_rows"] == 30
        tab = pa.Table.from_batches(got)
        assert tab.column(0).to_pylist() == cols[3][1000:1030] and tab.column(1).to_pylist() == cols[0][1000:1030]


# ---- 3. employee.csv: "Manager, Software" ------------------------------------------------------------------------------------
def test_employee_file_is_parsed_on_the_device(hip):
    path = os.path.join(CSV_DIR, "employee.csv")
    assert b'"' in open(path, "rb").read()
    for chunk in (-1, 64):
        ds, got, rows = check_against_host(hip, path, chunk)
        exp = pacsv.read_csv(path, convert_options=pacsv.ConvertOptions(strings_can_be_null=False))
        assert rows == exp.num_rows
        tab = pa.Table.from_batches(got)
        for i, col in enumerate(exp.columns):
            assert tab.column(i).to_pylist() == col.to_pylist()
        assert ds.stats["host_rows"] == 0 and ds.stats["device_rows"] == rows
    scan = CsvScan(hip, path, out_mem=abi.MEM_DEVICE, device_parse=-1, device_quotes=1)
    agg = HashAggExecutor(hip, [AggFunc("count", InputRef(3), abi.INT64), AggFunc("sum", InputRef(5), abi.INT64)],
                          [InputRef(3)], scan.execute(), out_mem=abi.MEM_DEVICE)
    (out,) = list(agg.execute())
    assert hip.batch_to_string(out) == "CA 1 12000\nCO 2 21500\n(empty) 1 NULL\n"
    assert scan.stats["host_rows"] == 0


# ---- 4. quotes on lane, tile and piece boundaries ------------------------------------------------------------------------------
PIECE = 16 * KIB
TILE = 4 * KIB


def boundary_file():
    """-> (file bytes, header length): offsets below are relative to the first piece, which starts behind the header"""
    eol = "\r\n"
    head = "k,v" + eol
    body = "".join(f"r{i},v{i}{eol}" for i in range(10))
    # a "" pair across a 16-byte lane boundary
    start = len(body) + 3
    first = (start // 16 + 2) * 16 + 15
    body += 'b,"' + "p" * (first - start) + '""' + 'q"' + eol
    assert body[first:first + 2] == '""' and first % 16 == 15
    # a closing quote as the last byte of a tile, its "\r\n" in the next
    start = len(body) + 3
    body += 'd,"' + "t" * (TILE - 1 - start) + '"' + eol
    assert body[TILE - 1] == '"' and body[TILE:TILE + 2] == eol
    # a quoted field of 9000 bytes over three tiles, delimiters and line breaks inside, and a "" pair whose quotes are the
    # last byte of one tile and the first of the next
    start = len(body) + 3
    left = ("ab,c\n,d\r\n" * 1000)[:2 * TILE - 1 - start]
    right = ("e,\n\nf," * 1000)[:9000 - len(left) - 2]
    body += 'c,"' + left + '""' + right + '"' + eol
    assert body[2 * TILE - 1:2 * TILE + 1] == '""' and len(left) + 2 + len(right) == 9000
    assert start // TILE == 1 and (start + 9000) // TILE == 3
    # a quoted '\n' that is the last '\n' of the first piece: the cut moves back to the record end in front of the field
    i = 0
    while len(body) < PIECE - 180:
        body += f"f{i},w{i}{eol}"
        i += 1
    cut = len(body)
    body += 'e,"' + "\n" * 300 + 'z"' + eol
    assert cut + 3 < PIECE - 100 and body[PIECE - 1] == "\n" and cut + 303 > PIECE
    body += "".join(f"g{i},x{i}{eol}" for i in range(2000))
    # a quoted last field without a final newline
    body += 'last,"no newline, at the ""end"""'
    return (head + body).encode(), len(head), cut


def test_quotes_on_lane_tile_and_piece_boundaries(hip, tmp_path):
    data, head, cut = boundary_file()
    recs, ragged, bad = csvparse.quoted_fields(data, 2)
    assert bad is None and ragged is None
    pos, is_end, _ = csvparse.quoted_separators(data)
    ends = pos[is_end]
    assert int(ends[ends < head + PIECE].max()) + 1 == head + cut  # where the first piece has to be cut
    assert data.rfind(b"\n", 0, head + PIECE) > head + cut          # ... and it is not the piece's last '\n'
    p = tmp_path / "b.csv"
    p.write_bytes(data)
    for batch_size in (100, 4096):
        ds, got, rows = check_against_host(hip, p, PIECE, batch_size=batch_size)
        assert rows == len(recs) - 1 and ds.stats["host_rows"] == 0 and ds.stats["device_rows"] == rows
    v = pa.Table.from_batches(got).column(1).to_pylist()
    assert [s.encode() for s in v] == [r[1] for r in recs[1:]]
    assert v[-1] == 'no newline, at the "end"' and v[10].endswith('p"q') and len(v[12].encode()) == 8999


# ---- 5. hand-backs -------------------------------------------------------------------------------------------------------------
def regular_lines(n):
    return [f'{i},"s,{i}"' for i in range(n)]


@pytest.mark.parametrize("case", ['12,a"b', '13,"x"y', '"x"y', "unterminated"])
def test_irregular_records_go_to_the_host_parser(hip, tmp_path, case):
    lines = regular_lines(3000)
    if case == "unterminated":
        lines[-1] = '2999,"never closed, to the end'
    else:
        lines[1500] = case
    p = tmp_path / "irregular.csv"
    p.write_text("a,s\n" + "\n".join(lines) + "\n")
    ds, got, rows = check_against_host(hip, p, 4 * KIB, batch_size=100)
    assert ds.stats["device_rows"] > 0 and ds.stats["host_rows"] > 0
    if case == '"x"y':  # one field: the host parser's error, the reader stays with it
        assert rows == 1500 and ds.stats["device_rows"] >= 1000
    else:
        assert rows == 3000
        if case != "unterminated":  # the pieces behind the irregular one are on the device again
            assert ds.stats["device_rows"] >= 2400 and ds.stats["host_rows"] <= 600


def test_record_made_longer_than_a_piece_by_quoted_newlines(hip, tmp_path):
    lines = regular_lines(500)
    lines[200] = '200,"' + "\n" * 2000 + '"'
    p = tmp_path / "long.csv"
    p.write_text("a,s\n" + "\n".join(lines) + "\n")
    ds, got, rows = check_against_host(hip, p, 1 * KIB, batch_size=50)
    assert rows == 500 and ds.stats["device_rows"] > 0 and ds.stats["host_rows"] > 0
    assert pa.Table.from_batches(got).column(1)[200].as_py() == "\n" * 2000


# ---- 6. typed quoted fields, and errors in the third batch ---------------------------------------------------------------------
def typed_lines(n):
    return [f"{i},{i * 0.25},{'true' if i % 2 else 'FALSE'},\"s,{i}\"" for i in range(n)]


def test_typed_quoted_fields(hip, tmp_path):
    lines = typed_lines(300)
    lines[20] = '"12","1.5","TRUE","x"'
    lines[21] = '"","","",""'
    lines[22] = '"-9223372036854775808","1e308","false",""""'
    p = tmp_path / "typed.csv"
    p.write_text("a,b,c,d\n" + "\n".join(lines) + "\n")
    for chunk in (-1, 1 * KIB):
        ds, got, rows = check_against_host(hip, p, chunk, batch_size=100)
        assert ds.dtypes == [abi.INT64, abi.FLOAT64, abi.BOOLEAN, abi.UTF8]
        assert rows == 300 and ds.stats["host_rows"] == 0
        t = pa.Table.from_batches(got).to_pylist()
        assert t[20] == {"a": 12, "b": 1.5, "c": True, "d": "x"}
        assert t[21] == {"a": None, "b": None, "c": None, "d": ""}
        assert t[22] == {"a": -2 ** 63, "b": 1e308, "c": False, "d": '"'}
    assert ds.stats["patched_fields"] == 1  # 1e308


@pytest.mark.parametrize("chunk", [-1, 1 * KIB], ids=["default", "1KiB"])
@pytest.mark.parametrize("field", ['"12x"', '"1""2"'])
def test_errors_in_quoted_typed_fields_are_the_host_parsers(hip, tmp_path, field, chunk):
    lines = typed_lines(400)
    lines[250] = f'{field},2.5,true,"x"'
    p = tmp_path / "bad.csv"
    p.write_text("a,b,c,d\n" + "\n".join(lines) + "\n")
    hs, exp, herr = run(hip, p, batch_size=100)
    ds, got, derr = run(hip, p, device_parse=chunk, device_quotes=1, batch_size=100)
    assert herr is not None and herr.status == abi.ERR_ARROW and "line 251" in str(herr)
    assert len(exp) == 2 and len(got) == 2
    same_stream(got, exp)
    assert derr is not None and derr.status == herr.status and str(derr) == str(herr)
    assert ds.stats["device_rows"] == 200


# ---- 7. a '\r' in front of the closing quote of a record's last field ------------------------------------------------------------
def test_carriage_return_in_front_of_a_closing_quote(hip, tmp_path):
    recs = [f'k{i},"s{i}"\n' for i in range(50)]
    recs[20] = 'k20,"ab\r"\n'      # the host parser pops the '\r' at '\n': "ab"
    recs[21] = 'k21,"ab\r"\r\n'    # ... here the one behind the quote: "ab\r"
    recs[22] = 'k22,"\r"\n'
    recs[23] = '"23\r","cd\r\r"\n'
    recs[49] = 'k49,"at the end\r"'
    p = tmp_path / "cr.csv"
    p.write_bytes(("a,s\n" + "".join(recs)).encode())
    for chunk in (-1, 64):
        ds, got, rows = check_against_host(hip, p, chunk, batch_size=16)
        assert rows == 50
    t = pa.Table.from_batches(got)
    assert t.column(1).to_pylist()[20:24] == ["ab", "ab\r", "", "cd\r"] and t.column(1)[49].as_py() == "at the end"
    assert t.column(0).to_pylist()[20:24] == ["k20", "k21", "k22", "23\r"]


# ---- 9. the switch itself -------------------------------------------------------------------------------------------------------
def test_switch_after_the_first_batch_is_an_error(hip, generated):
    path, _ = generated["lf"]
    h = C.c_void_p()
    hip.check(hip.fn("csv_open")(hip.ctx, path.encode(), 1, b",", 1000, 10, C.byref(h)))
    try:
        hip.check(hip.fn("csv_set_device_quotes")(h, 1))   # either order
        hip.check(hip.fn("csv_set_device_parse")(h, -1))   # ... and the flag survives this call
        out = C.POINTER(abi.Batch)()
        hip.check(hip.fn("csv_next_batch")(h, abi.MEM_HOST, C.byref(out)))
        assert out and out.contents.num_rows == 1000
        hip.fn("batch_release")(out)
        with pytest.raises(abi.ExecutorError) as e:
            hip.check(hip.fn("csv_set_device_quotes")(h, 0))
        assert e.value.status == abi.ERR_INTERNAL
        d, hr, pf = C.c_int64(), C.c_int64(), C.c_int64()
        hip.fn("csv_device_stats")(h, C.byref(d), C.byref(hr), C.byref(pf))
        assert (d.value, hr.value) == (1000, 0)
    finally:
        hip.fn("csv_close")(h)


def test_switch_without_device_parse_leaves_the_host_parser(hip, generated, host_streams):
    path, _ = generated["lf"]
    ds, got, err = run(hip, path, device_quotes=1, batch_size=1000)
    assert err is None
    same_stream(got, host_streams("lf", 1000))
    assert ds.stats == {"device_rows": 0, "host_rows": 0, "patched_fields": 0}
