"""The quoted-field rule of the device CSV parser (sqlrs_csv_set_device_quotes), restated on the host
(sqlrs_amd/csvparse.py: quoted_separators / quoted_fields), against a line-by-line restatement of the host parser's
read_record (csrc/plumbing.hip) and against pyarrow.csv.  No GPU."""
import io
import struct

import numpy as np
import pyarrow as pa
import pyarrow.csv as pacsv
import pytest

from sqlrs_amd import csvparse


def read_record(f: io.BytesIO, delim: int):
    """plumbing.hip read_record, branch by branch -> list of field bytes, or None at the end of the input"""
    fields, cur = [], bytearray()                                   # :139-140
    in_quotes = any_ = was_quoted = False                           # :141
    while True:
        ch = f.read(1)                                              # :143  in.get()
        if not ch:
            break
        any_ = True                                                 # :144
        c = ch[0]
        if in_quotes:                                               # :146
            if c == 34:                                             # :147
                if f.getbuffer()[f.tell():f.tell() + 1] == b'"':    # :148  in.peek() == '"'
                    cur.append(34)                                  # :149
                    f.read(1)                                       # :150
                else:
                    in_quotes = False                               # :152
            else:
                cur.append(c)                                       # :154
            continue                                                # :155
        if c == 34 and not cur and not was_quoted:                  # :157
            in_quotes = was_quoted = True                           # :158-159
        elif c == delim:                                            # :160
            fields.append(bytes(cur))                               # :161
            cur = bytearray()                                       # :162
            was_quoted = False                                      # :163
        elif c == 10:                                               # :164
            if cur and cur[-1] == 13:                               # :165
                cur.pop()
            if not fields and not cur and not was_quoted:           # :166  blank line
                any_ = False                                        # :167
                continue                                            # :168
            fields.append(bytes(cur))                               # :170
            return fields                                           # :171
        else:
            cur.append(c)                                           # :173
    if not any_:                                                    # :175
        return None
    if cur and cur[-1] == 13:                                       # :176
        cur.pop()
    if not fields and not cur and not was_quoted:                   # :177
        return None
    fields.append(bytes(cur))                                       # :178
    return fields                                                   # :179


def host_records(data: bytes, delim: bytes = b","):
    f, out = io.BytesIO(data), []
    while True:
        rec = read_record(f, delim[0])
        if rec is None:
            return out
        out.append(rec)


def test_the_restatement_reads_what_the_header_says():
    assert host_records(b'a,"b,c"\r\n\r\n"x""y",\n') == [[b"a", b"b,c"], [b'x"y', b""]]
    assert host_records(b'a"b,"c"d\n') == [[b'a"b', b'cd']]  # the quirks the regularity rule keeps away from the device
    assert host_records(b'"x"\r,y') == [[b"x\r", b"y"]]


ALPHABET = np.frombuffer(b'ab,"\n\r', dtype=np.uint8)
WEIGHTS = np.array([2, 1, 3, 4, 3, 1], dtype=float) / 14


def test_model_equals_host_parser_on_every_string_it_accepts():
    rng = np.random.default_rng(20240)
    n, with_quotes, accepted = 60_000, 0, 0
    lens = rng.integers(0, 25, n)
    for k in range(n):
        s = rng.choice(ALPHABET, int(lens[k]), p=WEIGHTS).tobytes()
        recs, ragged, bad = csvparse.quoted_fields(s)
        assert ragged is None
        if b'"' not in s:
            assert bad is None
        else:
            with_quotes += 1
        if bad is None:
            accepted += b'"' in s
            assert recs == host_records(s), s
    # the check is worth something only if many strings with quotes pass the rule
    assert with_quotes > 40_000 and accepted > 4_000, (with_quotes, accepted)


def test_model_equals_host_parser_on_random_well_formed_files():
    rng = np.random.default_rng(77)
    pieces = [b"a", b"b", b",", b"\n", b"\r", b"\r\n", b'""', b""]
    for _ in range(5_000):
        recs = []
        for _r in range(int(rng.integers(1, 5))):
            rec = []
            for _c in range(int(rng.integers(1, 4))):
                body = b"".join(pieces[i] for i in rng.integers(0, len(pieces), int(rng.integers(0, 6))))
                if rng.random() < 0.7:
                    rec.append(b'"' + body + b'"')
                else:
                    rec.append(body.replace(b'"', b"").replace(b",", b"").replace(b"\n", b"").replace(b"\r", b"") or b"z")
            recs.append(b",".join(rec))
        eol = b"\r\n" if rng.random() < 0.5 else b"\n"
        s = eol.join(recs) + (eol if rng.random() < 0.8 else b"")
        got, ragged, bad = csvparse.quoted_fields(s)
        assert bad is None and ragged is None, s
        assert got == host_records(s), s


WELL_FORMED = [
    (b'x,"ab\r"\n', [[b"x", b"ab"]]),           # the host pops a '\r' at '\n' even when it came from inside the quotes
    (b'x,"ab\r"\r\n', [[b"x", b"ab\r"]]),
    (b'"ab\r",x\n', [[b"ab\r", b"x"]]),
    (b'x,"ab\r"', [[b"x", b"ab"]]),
    (b'""\n', [[b""]]),
    (b'""""\n', [[b'"']]),
    (b'"a"",b"\n', [[b'a",b']]),
    (b'1,2\n\n\r\n"q,1",2\n', [[b"1", b"2"], [b"q,1", b"2"]]),
    (b'1,"last\nfield"', [[b"1", b"last\nfield"]]),
    (b'"",""\r\n"","x"\r\n', [[b"", b""], [b"", b"x"]]),
    (b'"\n\n"\n\n"\r\n"\n', [[b"\n\n"], [b"\r\n"]]),
]


@pytest.mark.parametrize("data, exp", WELL_FORMED, ids=[repr(d) for d, _ in WELL_FORMED])
def test_model_accepts_well_formed_input(data, exp):
    recs, ragged, bad = csvparse.quoted_fields(data)
    assert bad is None and ragged is None
    assert recs == exp and host_records(data) == exp
    ncols = len(exp[0])
    assert csvparse.quoted_fields(data, ncols) == (exp, None, None)
    rows, first_bad, start, end, bad = csvparse.quoted_index_fields(data, ncols)
    assert (rows, first_bad, bad) == (len(exp), None, None)
    pad = data if data.endswith(b"\n") else data + b"\n"
    sep_of_last = [int(end[r, ncols - 1]) + (pad[end[r, ncols - 1]] == 13) for r in range(rows)]
    assert [[csvparse.unquote(pad, int(start[r, c]), int(end[r, c]), sep_of_last[r] if c == ncols - 1 else int(end[r, c]))
             for c in range(ncols)] for r in range(rows)] == exp


IRREGULAR = [(b'1,a"b\n2,c\n', 3), (b'1,"a"b\n2,c\n', 4), (b'"a"\r,b\n', 2), (b'1,2\n3,"abc\n4,5\n', 6),
             (b'1,2\n3,"a""\n', 9), (b'a,\r"b"\n', 3), (b'x "y"\n', 2)]


@pytest.mark.parametrize("data, pos", IRREGULAR, ids=[repr(d) for d, _ in IRREGULAR])
def test_irregular_quotes_are_rejected_at_their_position(data, pos):
    assert csvparse.quoted_fields(data)[2] == pos
    assert csvparse.quoted_separators(data)[2] == pos
    assert csvparse.quoted_index_fields(data, 2)[4] == pos


def test_ragged_rows_with_quotes():
    data = b'a,b\n"1,1",2\n"3\n",4,5\n6,7\n'
    recs, ragged, bad = csvparse.quoted_fields(data, 2)
    assert bad is None and ragged == 2 and recs == [[b"a", b"b"], [b"1,1", b"2"]]
    assert csvparse.quoted_index_fields(data, 2)[:2] == (2, 2)


def test_quote_free_data_reads_as_before():
    data, _ = csvparse.generate(2_000, seed=9, eol="\r\n", blank_every=13)
    assert csvparse.quoted_fields(data, 4) == csvparse.fields(data, 4) + (None,)


def bits(x: float) -> bytes:
    return struct.pack("<d", x)


@pytest.mark.parametrize("eol", ["\n", "\r\n"], ids=["lf", "crlf"])
def test_generated_quoted_file(eol, tmp_path):
    """entitles the GPU test to demand host_rows == 0 and patched_fields == 0"""
    rows = 20_000
    data, cols = csvparse.generate_quoted(rows, seed=7, eol=eol)
    recs, ragged, bad = csvparse.quoted_fields(data, 4)
    assert bad is None and ragged is None and len(recs) == rows + 1 and recs[0] == [b"a", b"b", b"c", b"d"]
    pos, is_end, _ = csvparse.quoted_separators(data)
    ends = pos[is_end]
    assert int(np.diff(np.concatenate(([-1], ends))).max()) < 512  # the longest record, its line end included
    for r in recs[1:]:
        if r[1]:
            v = csvparse.exact_float(r[1])
            assert v is not None and bits(v) == bits(float(r[1])), r[1]
    # the file has what it promises
    raw = data.decode()
    nq = sum(1 for r, s in zip(recs[1:], cols[3]) if r[3].decode() == s)
    assert nq == rows
    assert 0.4 * rows < raw.count(',"') and any("\n" in s for s in cols[3]) and any('"' in s for s in cols[3])
    assert any("," in s for s in cols[3]) and '\r"' not in raw
    for c, conv in enumerate([int, float, lambda s: s.lower() == b"true"]):
        assert [None if not r[c] else conv(r[c]) for r in recs[1:]] == cols[c]
    # pyarrow reads the same fields
    p = tmp_path / "q.csv"
    p.write_bytes(data)
    types = {"a": pa.int64(), "b": pa.float64(), "c": pa.bool_(), "d": pa.string()}
    t = pacsv.read_csv(str(p), parse_options=pacsv.ParseOptions(newlines_in_values=True),
                       convert_options=pacsv.ConvertOptions(strings_can_be_null=False, column_types=types))
    assert t.num_rows == rows
    for c in range(4):
        assert t.column(c).to_pylist() == cols[c]
    assert sum(v is None for v in cols[0]) > 0.03 * rows
