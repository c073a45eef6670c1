"""The pieces SQLRS_EXPR_STAGE_ALL_TYPES stages (sqlrs_amd/csrc/stage_stitch.hpp), shared by the CPU check
(tests/test_host_stage_types_cpu.py, host/stage_stitch_check.cpp) and the GPU tests (tests/test_gpu_host_stage_types.py).

A case = (row list, validity shape, Utf8 shape), seeded by its name.  Every piece (pushed HOST batch) has the columns
{k Int64, v Float64, s Utf8, p Boolean}; k never has NULLs, the validity shape applies to v, s and p.  A column of a piece
is kept as the BUFFERS a caller would hand over (`ColBuf`: values / validity / offsets, null_count as the caller states it)
and as the logical Python values (`logical`), from which `model_concat` restates the concatenation the stitch must produce.
"""
from __future__ import annotations

import struct
import zlib
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

INT64, FLOAT64, BOOLEAN, UTF8 = 2, 3, 4, 5  # sqlrs_amd.abi dtypes
KIND_FIXED, KIND_BOOL, KIND_UTF8 = 0, 1, 2  # stage_stitch.hpp: StitchKind

ROW_LISTS = {
    "A": [1] * 130,  # more than 64 pieces in one output word; a partial third word
    "B": [63, 1, 64, 65, 0, 7, 128, 1, 1023, 1024, 1025, 0, 3],  # boundaries around 64 and 1024; empty batches in the middle
    "C": [1024] * 5 + [1000],  # the common shape
    "D": [5],  # a single piece under one word
    "E": [0, 0, 4, 0],  # leading and trailing empty batches
    "F64": [31, 33],  # a total of exactly 64 rows
    "F65": [64, 1],  # ... and of 65
}
VALIDITY_SHAPES = ("none", "first_at_3", "present_zero", "minus_one", "all_null", "tail_ones")
UTF8_SHAPES = ("empty_null", "window37", "long5000", "multibyte", "values_null")

POOL = ["", "a", "ab", "abc", "b", "ba", "zeta", "Zeta", "alpha", "alphabet", "omega", "mu"]
MULTI = ["é", "日本", "😀", "ñandú", "a日", "", "日本語", "zß"]


def pack_bits(bits) -> np.ndarray:
    return np.packbits(np.asarray(bits, dtype=np.uint8), bitorder="little")


@dataclass
class ColBuf:
    dtype: int
    values: Optional[np.ndarray]  # uint8 view of the values buffer (Utf8: the chars the offsets index); None = NULL pointer
    validity: Optional[np.ndarray]  # uint8, ceil(n / 8) bytes; None = NULL pointer
    null_count: int  # as the caller states it (may be -1, may be 0 beside a bitmap)
    offsets: Optional[np.ndarray]  # int32, n + 1 (Utf8)
    logical: list = field(default_factory=list)  # Python values, None = NULL

    def nullable(self) -> bool:
        """does the library look at the bitmap at all?  (upload_column and the stage agree: a pointer and a null_count != 0)"""
        return self.validity is not None and self.null_count != 0


@dataclass
class Piece:
    n: int
    cols: List[ColBuf]


@dataclass
class Case:
    name: str
    pieces: List[Piece]
    names = ("k", "v", "s", "p")
    dtypes = (INT64, FLOAT64, UTF8, BOOLEAN)

    @property
    def rows(self) -> int:
        return sum(p.n for p in self.pieces)


def _validity(vshape: str, j: int, n: int, rng):
    """-> (valid bool[n], validity bytes or None, stated null_count) of one column of piece j"""
    nb = (n + 7) // 8
    if vshape == "none" or (vshape == "first_at_3" and j != 3):
        return np.ones(n, bool), None, 0
    if vshape == "present_zero":
        return np.ones(n, bool), np.full(nb, 0xFF, np.uint8), 0
    if vshape == "all_null":
        return np.zeros(n, bool), np.zeros(nb, np.uint8), n
    valid = rng.random(n) >= 0.3
    if n:
        valid[rng.integers(0, n)] = False  # a NULL-bearing piece bears a NULL
    bits = pack_bits(valid)
    if vshape == "tail_ones" and n & 7:
        bits[-1] |= np.uint8((0xFF << (n & 7)) & 0xFF)  # the unused high bits of the last byte: caller garbage
    return valid, bits, (-1 if vshape == "minus_one" else int(n - valid.sum()))


def build_case(list_name: str, vshape: str, ushape: str) -> Case:
    name = f"{list_name}/{vshape}/{ushape}"
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    row_list = ROW_LISTS[list_name]
    total = sum(row_list)
    # the strings of every row first (window37 lays ALL pieces out in one chars array)
    pool = MULTI if ushape == "multibyte" else POOL
    strings = [pool[i] for i in rng.integers(0, len(pool), total)]
    if ushape == "empty_null":
        strings = ["" if g % 3 == 0 else s for g, s in enumerate(strings)]  # empty strings next to the NULLs below
    if ushape == "values_null":
        strings = [""] * total
    long_todo = ushape == "long5000"
    pieces, g0 = [], 0
    per_piece = []
    for j, n in enumerate(row_list):
        k = rng.integers(0, 7, n).astype(np.int64)
        v = rng.integers(0, 8000, n) / 8.0  # eighths: a SUM is exact whatever order the rows are added in
        p = rng.random(n) < 0.5
        vv, vbits, vnc = _validity(vshape, j, n, rng)
        sv, sbits, snc = _validity(vshape, j, n, rng)
        pv, pbits, pnc = _validity(vshape, j, n, rng)
        s = [strings[g0 + r] if sv[r] else "" for r in range(n)]  # a NULL row holds no bytes
        if long_todo and sv.any() and (j >= len(row_list) // 2 or not any(row_list[j + 1:])):
            s[int(np.argmax(sv))] = "L" * 4999 + "!"  # one 5000-byte string, on a valid row of a middle piece
            long_todo = False
        strings[g0:g0 + n] = s
        per_piece.append((n, k, v, p, (vv, vbits, vnc), (sv, sbits, snc), (pv, pbits, pnc), s))
        g0 += n
    enc = [x.encode("utf-8") for x in strings]
    if ushape == "window37":
        base = 37
        all_off = np.zeros(total + 1, np.int32)
        all_off[0] = base
        if total:
            all_off[1:] = base + np.cumsum([len(b) for b in enc])
        all_chars = np.frombuffer(b"#" * base + b"".join(enc), np.uint8).copy()
    g0 = 0
    for (n, k, v, p, (vv, vbits, vnc), (sv, sbits, snc), (pv, pbits, pnc), s) in per_piece:
        if ushape == "window37":
            off = all_off[g0:g0 + n + 1]  # a window into the one offsets array: offsets[0] != 0
            chars = all_chars
        else:
            e = enc[g0:g0 + n]
            off = np.zeros(n + 1, np.int32)
            if n:
                off[1:] = np.cumsum([len(b) for b in e])
            chars = np.frombuffer(b"".join(e), np.uint8).copy() if off[-1] else (None if ushape == "values_null" else np.zeros(0, np.uint8))
        pbytes = pack_bits(p)
        if vshape == "tail_ones" and n & 7:
            pbytes[-1] |= np.uint8((0xFF << (n & 7)) & 0xFF)
        cols = [
            ColBuf(INT64, k.view(np.uint8), None, 0, None, [int(x) for x in k]),
            ColBuf(FLOAT64, v.view(np.uint8), vbits, vnc, None, [float(x) if ok else None for x, ok in zip(v, vv)]),
            ColBuf(UTF8, chars, sbits, snc, off, [x if ok else None for x, ok in zip(s, sv)]),
            ColBuf(BOOLEAN, pbytes, pbits, pnc, None, [bool(x) if ok else None for x, ok in zip(p, pv)]),
        ]
        pieces.append(Piece(n, cols))
        g0 += n
    return Case(name, pieces)


def cpu_cases() -> List[Case]:
    """every row list crossed with every validity shape (the Utf8 shapes taking turns) and with every Utf8 shape"""
    out, seen = [], set()
    for li, ln in enumerate(ROW_LISTS):
        for vi, vs in enumerate(VALIDITY_SHAPES):
            key = (ln, vs, UTF8_SHAPES[(li + vi) % len(UTF8_SHAPES)])
            seen.add(key)
            out.append(build_case(*key))
        for us in UTF8_SHAPES:
            key = (ln, "minus_one", us)
            if key not in seen:
                seen.add(key)
                out.append(build_case(*key))
    return out


# ---- the concatenation, restated -------------------------------------------------------------------------------------
def model_concat(case: Case):
    """per column: (null_count, validity words or None, payload bytes) of the one Arrow column the pieces add up to: the
    bitmap of a piece the library does not look at (no pointer, or a stated null_count of 0) is all ones; no validity at all
    when no row is NULL; bits at and beyond the row count are 0"""
    rows = case.rows
    words = (rows + 63) // 64
    out = []
    for c, dtype in enumerate(case.dtypes):
        valid = np.ones(rows, bool)
        g = 0
        for p in case.pieces:
            cb = p.cols[c]
            if cb.nullable() and p.n:
                valid[g:g + p.n] = np.unpackbits(cb.validity, bitorder="little")[:p.n].astype(bool)
            g += p.n
        nulls = int(rows - valid.sum())

        def to_words(bits):
            padded = np.zeros(words * 64, np.uint8)
            padded[:rows] = bits
            return np.packbits(padded, bitorder="little").view(np.uint64) if words else np.zeros(0, np.uint64)
        vwords = to_words(valid) if nulls else None
        if dtype == UTF8:
            chunks, off = [], [0]
            for p in case.pieces:
                cb = p.cols[c]
                for r in range(p.n):  # string by string
                    b = bytes(cb.values[cb.offsets[r]:cb.offsets[r + 1]]) if cb.offsets[r + 1] > cb.offsets[r] else b""
                    chunks.append(b)
                    off.append(off[-1] + len(b))
            payload = np.asarray(off, np.int32).tobytes() + b"".join(chunks)
        elif dtype == BOOLEAN:
            bits = np.zeros(rows, np.uint8)
            g = 0
            for p in case.pieces:
                if p.n:
                    bits[g:g + p.n] = np.unpackbits(p.cols[c].values, bitorder="little")[:p.n]
                g += p.n
            payload = to_words(bits).tobytes()
        else:
            payload = b"".join(bytes(p.cols[c].values) for p in case.pieces if p.n)
        out.append((nulls, vwords, payload))
    return out


_K, _H0 = 0x100000001B3, 0xCBF29CE484222325


def digest_bytes(data: bytes) -> int:
    """h = h * K + (byte + 1) over the bytes, mod 2^64, from h = H0 (what host/stage_stitch_check.cpp prints) — in closed form,
    so that numpy can do it"""
    L = len(data)
    h = (_H0 * pow(_K, L, 1 << 64)) & ((1 << 64) - 1)
    if L:
        with np.errstate(over="ignore"):
            pw = np.cumprod(np.full(L, _K, np.uint64))  # K^1 .. K^L, wrapping
            weights = np.concatenate([np.ones(1, np.uint64), pw[:-1]])[::-1]  # K^(L - 1 - i)
            s = np.sum((np.frombuffer(data, np.uint8).astype(np.uint64) + np.uint64(1)) * weights, dtype=np.uint64)
        h = (h + int(s)) & ((1 << 64) - 1)
    return h


def case_digest(case: Case) -> int:
    parts = []
    for nulls, vwords, payload in model_concat(case):
        parts.append(struct.pack("<q", nulls))
        if vwords is not None:
            parts.append(vwords.tobytes())
        parts.append(payload)
    return digest_bytes(b"".join(parts))


def write_cases(path: str, cases: List[Case]) -> None:
    """the buffers of every piece, for host/stage_stitch_check.cpp (little-endian int64 fields; a blob = length, bytes;
    length -1 = a NULL pointer)"""
    def blob(a) -> bytes:
        if a is None:
            return struct.pack("<q", -1)
        b = np.ascontiguousarray(a).tobytes()
        return struct.pack("<q", len(b)) + b
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(cases)))
        for case in cases:
            f.write(struct.pack("<qq", len(case.pieces), len(case.dtypes)))
            for d in case.dtypes:
                f.write(struct.pack("<qq", KIND_UTF8 if d == UTF8 else KIND_BOOL if d == BOOLEAN else KIND_FIXED, 0 if d in (UTF8, BOOLEAN) else 8))
            for p in case.pieces:
                f.write(struct.pack("<q", p.n))
                for cb in p.cols:
                    f.write(blob(cb.values) + blob(cb.validity if cb.nullable() else None) + blob(cb.offsets))
