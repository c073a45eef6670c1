"""Host restatement of the device CSV parser's rules (csrc/csv_kernels.hpp), as ``distributed.py`` restates the partition
kernels: the CPU suite runs these, the kernels implement them.

* ``index_fields``: separator ranks -> (row, column).  A separator is a delimiter byte or a ``\\n`` that ends a record; a
  ``\\n`` that ends a blank line — its predecessor, one ``\\r`` skipped, is a ``\\n`` or the start of the data — is none.
  Separator number f ends field f: row = f // C, column = f % C for C file columns, valid exactly while every ``\\n`` has
  f % C == C - 1 and no delimiter has; the first violation's row is the ragged record, every row before it is good.
* ``exact_float``: the Float64 fields the device writes itself (everything else is left to ``std::from_chars``).
* ``generate``: the seeded quote-free file the tests and ``tools/csv_device_bench.py`` read.
* ``quoted_separators`` / ``quoted_index_fields`` / ``quoted_fields``: the same with RFC-4180 quotes
  (``sqlrs_csv_set_device_quotes``): every quote toggles "inside quotes", separators inside do not count, and the position
  of the first *irregular* quote says whether that reading is the host parser's.  ``generate_quoted``: the seeded file.
"""
from __future__ import annotations

import re
from typing import List, Optional, Tuple

import numpy as np

NL, CR = 10, 13


def separators(data: bytes, delimiter: bytes = b",") -> Tuple[np.ndarray, np.ndarray]:
    """(byte position, is-a-record-end) of every separator of quote-free ``data``.  A last record without ``\\n`` counts:
    the data is read as if it ended in one."""
    if data and not data.endswith(b"\n"):
        data = data + b"\n"
    b = np.frombuffer(data, dtype=np.uint8)
    prev1 = np.concatenate(([NL], b[:-1])) if len(b) else b
    prev2 = np.concatenate(([NL, NL], b[:-2]))[:len(b)] if len(b) else b
    is_delim = b == delimiter[0]
    blank = (prev1 == NL) | ((prev1 == CR) & (prev2 == NL))
    is_end = (b == NL) & ~is_delim & ~blank
    pos = np.flatnonzero(is_delim | is_end)
    return pos, is_end[pos]


def index_fields(data: bytes, ncols: int, delimiter: bytes = b","):
    """-> (rows, first_bad_row, start, end): ``rows`` good records, ``first_bad_row`` the ragged record's row or None,
    ``start`` / ``end`` int64 arrays [rows, ncols] of the fields' byte ranges (blank lines in front of a record and one
    trailing ``\\r`` of it cut off)."""
    if data and not data.endswith(b"\n"):
        data = data + b"\n"
    pos, is_end = separators(data, delimiter)
    f = np.arange(len(pos))
    bad = (f % ncols == ncols - 1) != is_end
    first_bad = int(f[bad][0] // ncols) if bad.any() else None
    rows = first_bad if first_bad is not None else len(pos) // ncols
    end = pos[:rows * ncols].astype(np.int64).reshape(rows, ncols)
    start = np.concatenate(([0], pos[:rows * ncols - 1] + 1)).astype(np.int64)[:rows * ncols].reshape(rows, ncols) \
        if rows else end.copy()
    start, end = start.copy(), end.copy()
    for r in range(rows):  # blank lines in front of the record: "\n" or "\r\n" straight after a record's end
        s, e = start[r, 0], end[r, 0]
        while s < e:
            if data[s] == NL:
                s += 1
            elif data[s] == CR and data[s + 1] == NL:
                s += 2
            else:
                break
        start[r, 0] = s
        s, e = start[r, ncols - 1], end[r, ncols - 1]
        if e > s and data[e - 1] == CR:
            end[r, ncols - 1] = e - 1
    return rows, first_bad, start, end


def fields(data: bytes, ncols: int, delimiter: bytes = b",") -> Tuple[List[List[bytes]], Optional[int]]:
    """the good records as lists of field bytes, and the ragged record's row (None: none)"""
    rows, first_bad, start, end = index_fields(data, ncols, delimiter)
    return [[data[start[r, c]:end[r, c]] for c in range(ncols)] for r in range(rows)], first_bad


_SIMPLE = re.compile(rb"(-?)([0-9]+)(?:\.([0-9]+))?(?:[eE](-?[0-9]+))?")
_POW10 = [float(10 ** k) for k in range(23)]  # exact doubles


def exact_float(s: bytes) -> Optional[float]:
    """``-?digits[.digits][(e|E)[-]digits]`` whose digits form an integer m < 2**53 and whose decimal exponent k, the point
    moved behind the last digit, has |k| <= 22: m and 10**|k| are exact doubles, so ONE IEEE multiply or divide is the
    correctly rounded value.  None: the field is left to the host (``patched_fields``)."""
    m = _SIMPLE.fullmatch(s)
    if not m:
        return None
    sign, ip, fp, ex = m.groups()
    fp = fp or b""
    mant = int(ip + fp)
    if mant >= 2 ** 53:
        return None
    e = int(ex) if ex else 0
    if abs(e) > 9999:
        return None
    k = e - len(fp)
    if abs(k) > 22:
        return None
    v = float(mant) * _POW10[k] if k >= 0 else float(mant) / _POW10[-k]
    return -v if sign else v


I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
_BOOLS = ["true", "True", "TRUE", "false", "False", "FALSE"]
_WORDS = ["alpha", "bravo", "charlie", "delta", "échelon", "foxtrot", "größe", "hotel", "印度", "juliett", "kilo", "lima", "x"]


def generate(rows: int, seed: int = 0, eol: str = "\n", blank_every: int = 0, final_newline: bool = True,
             empty_fraction: float = 0.05):
    """A seeded quote-free file ``a,b,c,d`` of ``rows`` records: int64 (negatives, INT64_MIN / MAX), "easy" float (signed
    ``%.6f`` below 1e6), boolean in the six spellings pyarrow also reads, Utf8 (empty strings, multi-byte UTF-8); about
    ``empty_fraction`` of the typed fields empty, none in the first ten records (where the types are inferred).
    -> (file bytes, columns as Python lists: int / float / bool / str, None = NULL)"""
    rng = np.random.default_rng(seed)
    ints = rng.integers(-10 ** 12, 10 ** 12, rows).tolist()
    mags = rng.integers(0, 10 ** 12, rows)  # micro-units: the value is +-mags / 1e6 < 1e6
    negs = rng.random(rows) < 0.5
    bools = rng.integers(0, 6, rows).tolist()
    words = rng.integers(0, len(_WORDS) + 2, rows).tolist()
    nums = rng.integers(0, 1000, rows).tolist()
    empties = rng.random((rows, 3)) < empty_fraction
    empties[:10] = False
    lines, ci, cf, cb, cs = [], [], [], [], []
    for r in range(rows):
        if r % 1000 == 500:
            ints[r] = I64_MIN if (r // 1000) % 2 else I64_MAX
        e = empties[r]
        a = "" if e[0] else str(ints[r])
        m = int(mags[r])
        b = "" if e[1] else ("-" if negs[r] else "") + f"{m // 10 ** 6}.{m % 10 ** 6:06d}"
        c = "" if e[2] else _BOOLS[bools[r]]
        w = words[r]
        d = "" if (w >= len(_WORDS) and r >= 10) else f"{_WORDS[w % len(_WORDS)]}-{nums[r]}"
        ci.append(None if e[0] else ints[r])
        cf.append(None if e[1] else float(b))
        cb.append(None if e[2] else bools[r] < 3)
        cs.append(d)
        lines.append(f"{a},{b},{c},{d}")
        if blank_every and r % blank_every == blank_every - 1:
            lines.append("")
            if r % (2 * blank_every) == blank_every - 1:
                lines.append("")
    text = "a,b,c,d" + eol + eol.join(lines) + (eol if final_newline else "")
    return text.encode("utf-8"), [ci, cf, cb, cs]


VARIANTS = {"lf": dict(eol="\n"), "crlf": dict(eol="\r\n"), "blank_lines": dict(eol="\n", blank_every=97),
            "no_final_newline": dict(eol="\r\n", final_newline=False)}


# ---- quoted fields (sqlrs_csv_set_device_quotes) -----------------------------------------------------------------------------
QUOTE = 34


def quoted_separators(data: bytes, delimiter: bytes = b","):
    """``separators`` for data with RFC-4180 quotes, every ``"`` toggling "inside quotes": -> (byte position, is-a-record-end,
    position of the first irregular quote or None).  par(i) = number of quotes in [0, i), mod 2.  A quote with par = 0 opens
    and is regular iff it is the first byte or follows the delimiter, a ``\\n`` or a quote (which then closed: an escaped
    pair); a quote with par = 1 closes and is regular iff the delimiter, ``\\n``, ``\\r\\n`` or a quote follows.  A quote left
    open at the end of the data is irregular.  Separators are the delimiters and record-ending ``\\n`` with par = 0."""
    if data and not data.endswith(b"\n"):
        data = data + b"\n"
    b = np.frombuffer(data, dtype=np.uint8)
    n = len(b)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, bool), None
    dl = delimiter[0]
    isq = b == QUOTE
    inq = ((np.cumsum(isq) - isq) & 1).astype(bool)
    prev1 = np.concatenate(([NL], b[:-1]))
    prev2 = np.concatenate(([NL, NL], b[:-2]))[:n]
    next1 = np.concatenate((b[1:], [0]))
    next2 = np.concatenate((b[2:], [0, 0]))[:n]
    is_delim = (b == dl) & ~isq
    blank = (prev1 == NL) | ((prev1 == CR) & (prev2 == NL))
    is_end = (b == NL) & ~is_delim & ~blank & ~inq
    is_delim = is_delim & ~inq
    open_ok = (prev1 == dl) | (prev1 == NL) | (prev1 == QUOTE)
    close_ok = (next1 == dl) | (next1 == NL) | (next1 == QUOTE) | ((next1 == CR) & (next2 == NL))
    bad = isq & np.where(inq, ~close_ok, ~open_ok)
    if isq.sum() & 1:  # left open: the last quote is the one that opened
        bad[np.flatnonzero(isq)[-1]] = True
    bad_quote = int(np.flatnonzero(bad)[0]) if bad.any() else None
    pos = np.flatnonzero(is_delim | is_end)
    return pos, is_end[pos], bad_quote


def quoted_index_fields(data: bytes, ncols: int, delimiter: bytes = b","):
    """``index_fields`` over ``quoted_separators``: -> (rows, first_bad_row, start, end, bad_quote); ``start`` / ``end`` are
    the fields' byte ranges with their outer quotes (blank lines in front of a record and one trailing ``\\r`` cut off).
    The rows mean what the host parser reads only when ``bad_quote`` is None."""
    if data and not data.endswith(b"\n"):
        data = data + b"\n"
    pos, is_end, bad_quote = quoted_separators(data, delimiter)
    f = np.arange(len(pos))
    bad = (f % ncols == ncols - 1) != is_end
    first_bad = int(f[bad][0] // ncols) if bad.any() else None
    rows = first_bad if first_bad is not None else len(pos) // ncols
    end = pos[:rows * ncols].astype(np.int64).reshape(rows, ncols)
    start = np.concatenate(([0], pos[:rows * ncols - 1] + 1)).astype(np.int64)[:rows * ncols].reshape(rows, ncols) \
        if rows else end.copy()
    start, end = start.copy(), end.copy()
    for r in range(rows):
        start[r, 0], _ = _trim(data, start[r, 0], end[r, 0], True, False)
        _, end[r, ncols - 1] = _trim(data, start[r, ncols - 1], end[r, ncols - 1], False, True)
    return rows, first_bad, start, end, bad_quote


def _trim(data, s, e, first, last):
    if first:  # blank lines in front of the record
        while s < e:
            if data[s] == NL:
                s += 1
            elif data[s] == CR and data[s + 1] == NL:
                s += 2
            else:
                break
    if last and e > s and data[e - 1] == CR:
        e -= 1
    return s, e


def unquote(data: bytes, s: int, e: int, sep: int) -> bytes:
    """the value of the field data[s:e] (trimmed) whose separator is at ``sep``: a field that starts with a quote loses the
    outer pair and reads ``""`` as ``"``.  The host parser pops one ``\\r`` from the end of a record's text at ``\\n`` even when
    it came from inside the quotes: a closing quote directly in front of the record's ``\\n`` drops a ``\\r`` before it."""
    if e <= s or data[s] != QUOTE:
        return data[s:e]
    inner = data[s + 1:e - 1]
    if e == sep and data[sep] == NL and inner.endswith(b"\r"):
        inner = inner[:-1]
    return inner.replace(b'""', b'"')


def quoted_fields(data: bytes, ncols: Optional[int] = None, delimiter: bytes = b","):
    """-> (records as lists of field values, the ragged record's row or None, the first irregular quote's position or None).
    ``ncols`` None: records of any length, as the host parser's ``read_record`` returns them (no ragged row)."""
    if data and not data.endswith(b"\n"):
        data = data + b"\n"
    pos, is_end, bad_quote = quoted_separators(data, delimiter)
    recs, cur, s = [], [], 0
    for p, last in zip(pos.tolist(), is_end.tolist()):
        fs, fe = _trim(data, s, p, not cur, last)
        cur.append(unquote(data, fs, fe, p))
        s = p + 1
        if last:
            recs.append(cur)
            cur = []
    first_bad = None
    if ncols is not None:
        first_bad = next((r for r, rec in enumerate(recs) if len(rec) != ncols), None)
        if first_bad is None and cur:
            first_bad = len(recs)
        if first_bad is not None:
            recs = recs[:first_bad]
    return recs, first_bad, bad_quote


_QBODY = ["alpha", "bravo", "échelon", "größe", "印度", "x", " ", ",", ",", "\n", "\r\n", '""', '""', "-7", "a b"]


def generate_quoted(rows: int, seed: int = 0, eol: str = "\n"):
    """The ``a,b,c,d`` schema of ``generate`` with quoted fields: about half of the Utf8 fields quoted, their bodies drawn from
    words, the delimiter, ``\\n``, ``\\r\\n``, ``""`` escapes, multi-byte UTF-8 and the empty ``""``; about a tenth of the typed
    fields quoted (``"123"``, ``"1.500000"``, ``"true"``, ``""``).  No ``\\r`` directly in front of a closing quote, the first
    ten records fully populated and unquoted in the typed columns, every record shorter than 512 bytes.
    -> (file bytes, columns as Python lists: int / float / bool / str, None = NULL)"""
    rng = np.random.default_rng(seed)
    ints = rng.integers(-10 ** 12, 10 ** 12, rows).tolist()
    mags = rng.integers(0, 10 ** 12, rows)
    negs = rng.random(rows) < 0.5
    bools = rng.integers(0, 6, rows).tolist()
    empties = rng.random((rows, 3)) < 0.05
    tq = rng.random((rows, 3)) < 0.10
    empties[:10] = False
    tq[:10] = False
    sq = rng.random(rows) < 0.5
    ntok = rng.integers(0, 9, rows).tolist()
    toks = rng.integers(0, len(_QBODY), (rows, 8)).tolist()
    words = rng.integers(0, len(_WORDS) + 2, rows).tolist()
    nums = rng.integers(0, 1000, rows).tolist()
    lines, ci, cf, cb, cs = [], [], [], [], []
    for r in range(rows):
        if r % 1000 == 500:
            ints[r] = I64_MIN if (r // 1000) % 2 else I64_MAX
        e, q = empties[r], tq[r]
        m = int(mags[r])
        typed = [str(ints[r]), ("-" if negs[r] else "") + f"{m // 10 ** 6}.{m % 10 ** 6:06d}", _BOOLS[bools[r]]]
        vals = [ints[r], float(typed[1]), bools[r] < 3]
        text = []
        for c in range(3):
            t = "" if e[c] else typed[c]
            text.append('"' + t + '"' if q[c] else t)
            vals[c] = None if e[c] else vals[c]
        if sq[r] and r >= 10:
            d = "".join(_QBODY[t] for t in toks[r][:ntok[r]])
            text.append('"' + d + '"')
            d = d.replace('""', '"')
        else:
            w = words[r]
            d = "" if (w >= len(_WORDS) and r >= 10) else f"{_WORDS[w % len(_WORDS)]}-{nums[r]}"
            text.append(d)
        ci.append(vals[0])
        cf.append(vals[1])
        cb.append(vals[2])
        cs.append(d)
        lines.append(",".join(text))
    text = "a,b,c,d" + eol + eol.join(lines) + eol
    return text.encode("utf-8"), [ci, cf, cb, cs]
