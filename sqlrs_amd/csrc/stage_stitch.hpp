// stage_stitch.hpp — host staging of small HOST batches of EVERY column type (SQLRS_EXPR_STAGE_ALL_TYPES, host_stage.hpp): the
// bookkeeping of the staged pieces and the two per-element functions that turn the staged raw arrays into one Arrow column.
//
// A pushed batch is a PIECE.  Appending a piece is a handful of memcpys, never a loop over its rows:
//   per stage    row_start[P + 1]   prefix of the pieces' row counts (0-row batches are pieces too)
//   fixed width  the values, appended: they already are the column
//   Utf8         the bytes [offsets[0], offsets[n]) appended to one char array; the n + 1 raw offsets appended verbatim (piece k's
//                entries start at row_start[k] + k); delta[k] = chars before piece k - offsets_k[0]
//   a bitmap     (the validity of any column, a Boolean column's values) ceil(n / 8) bytes appended at BYTE granularity,
//                byte_start[k] = where; a piece without NULLs stages no validity bytes and gets byte_start[k] = -1 (all ones)
// At a flush every raw array is uploaded once and ONE launch per array builds the Arrow form: stitch_bits_word gives a 64-bit
// word of a bitmap (every output word is written by exactly one thread: no atomics, no zero fill), stitch_offset one offset.
// No HIP include: host/stage_stitch_check.cpp compiles this file with a host compiler and runs both functions for every word
// and row under the sanitizers.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#ifndef SQLRS_HD
#ifdef __HIPCC__
#define SQLRS_HD __host__ __device__
#else
#define SQLRS_HD
#endif
#endif

namespace sq {

// the piece of row r: the LAST k in [0, P) with row_start[k] <= r (of several pieces that start at the same row, all but the
// last are empty); needs 0 <= r < row_start[P]
SQLRS_HD inline int64_t stitch_piece_of(const int64_t *row_start, int64_t P, int64_t r) {
  int64_t lo = 0, hi = P; // row_start[lo] <= r < row_start[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (row_start[mid] <= r) lo = mid;
    else hi = mid;
  }
  return lo;
}

// word w (rows [64 w, 64 w + 64)) of the bitmap whose piece k is the bits [0, rows of piece k) at raw + byte_start[k], or all
// ones where byte_start[k] < 0.  Bits at and beyond `rows` are 0 (w may lie beyond the last row: the padding word); a piece's
// bits beyond its row count — caller garbage in its last byte — never reach the result.  Reads only bytes of the pieces.
SQLRS_HD inline uint64_t stitch_bits_word(const uint8_t *raw, const int64_t *row_start, const int64_t *byte_start, int64_t P,
                                          int64_t rows, int64_t w) {
  const int64_t lo = 64 * w, hi = lo + 64 < rows ? lo + 64 : rows;
  if (lo >= rows) return 0;
  uint64_t out = 0;
  for (int64_t k = stitch_piece_of(row_start, P, lo); k < P && row_start[k] < hi; k++) {
    const int64_t s = row_start[k], e = row_start[k + 1];
    if (e <= s) continue;
    const int64_t a = s > lo ? s : lo, b = e < hi ? e : hi; // output rows [a, b) = bits [a - s, b - s) of the piece
    const int nb = (int)(b - a);                           // 1 .. 64
    uint64_t bits = ~0ull;
    if (byte_start[k] >= 0) {
      const int64_t o = a - s;
      const uint8_t *p = raw + byte_start[k] + (o >> 3);
      const int sh = (int)(o & 7), nbytes = (sh + nb + 7) >> 3; // 1 .. 9 bytes, all inside the piece
      bits = 0;
      for (int i = 0; i < nbytes && i < 8; i++) bits |= (uint64_t)p[i] << (8 * i);
      bits >>= sh;
      if (nbytes == 9) bits |= (uint64_t)p[8] << (64 - sh); // (sh > 0 here)
    }
    if (nb < 64) bits &= (1ull << nb) - 1;
    out |= bits << (a - lo);
  }
  return out;
}

// offset r of the stitched Utf8 column, r in [0, rows]: raw_off holds every piece's n + 1 offsets one after the other
SQLRS_HD inline int32_t stitch_offset(const int32_t *raw_off, const int64_t *row_start, const int64_t *delta, int64_t P, int64_t rows,
                                      int64_t total_chars, int64_t r) {
  if (r >= rows) return (int32_t)total_chars;
  const int64_t k = stitch_piece_of(row_start, P, r);
  return (int32_t)((int64_t)raw_off[r + k] + delta[k]);
}

// cleared bits of such a bitmap, counted on the staged bytes (the caller's null_count is not trusted: it may be -1); the tail
// bits of a piece's last byte are masked.  Host only.
inline int64_t stitch_count_clear(const uint8_t *raw, const int64_t *row_start, const int64_t *byte_start, int64_t P) {
  int64_t clear = 0;
  for (int64_t k = 0; k < P; k++) {
    if (byte_start[k] < 0) continue;
    const int64_t n = row_start[k + 1] - row_start[k];
    const uint8_t *p = raw + byte_start[k];
    int64_t set = 0, i = 0;
    for (; i + 8 <= (n >> 3); i += 8) {
      uint64_t x;
      std::memcpy(&x, p + i, 8);
      set += __builtin_popcountll(x);
    }
    for (; i < (n >> 3); i++) set += __builtin_popcount(p[i]);
    if (n & 7) set += __builtin_popcount(p[n >> 3] & ((1u << (n & 7)) - 1));
    clear += n - set;
  }
  return clear;
}

// ---- the staging memory ------------------------------------------------------------------------------------------------------
// where the pinned form of a staged array comes from (hipHostMalloc / hipHostFree in the library, malloc / free in the check)
struct StitchMem {
  void *(*alloc)(size_t bytes) = nullptr; // throws when it cannot
  void (*release)(void *p) = nullptr;
};

// One staged array: a std::vector while there is little of it, a pinned block — kept across flushes — from the moment the stage
// says so (host_stage.hpp: HOST_STAGE_PIN_ROWS).  room() may throw and changes no content; put() after room() cannot fail.
struct StitchBuf {
  std::vector<uint8_t> vec;
  uint8_t *pin = nullptr;
  size_t pin_cap = 0, pin_size = 0;
  size_t size() const { return pin ? pin_size : vec.size(); }
  const uint8_t *data() const { return pin ? pin : vec.data(); }
  void room(size_t add, bool use_pin, const StitchMem &m, size_t min_cap) {
    if (!pin && !use_pin) {
      vec.reserve(vec.size() + add);
      return;
    }
    const size_t have = size();
    if (pin && have + add <= pin_cap) return;
    size_t cap = pin_cap * 2 > min_cap ? pin_cap * 2 : min_cap;
    while (cap < have + add) cap *= 2;
    uint8_t *np = (uint8_t *)m.alloc(cap);
    if (have) std::memcpy(np, data(), have);
    if (pin) m.release(pin);
    pin = np;
    pin_cap = cap;
    pin_size = have;
    vec.clear();
    vec.shrink_to_fit();
  }
  void put(const void *src, size_t add) {
    if (!add) return; // (src may be NULL then)
    if (pin) {
      std::memcpy(pin + pin_size, src, add);
      pin_size += add;
    } else
      vec.insert(vec.end(), (const uint8_t *)src, (const uint8_t *)src + add);
  }
  void clear() {
    vec.clear();
    pin_size = 0;
  }
  void drop(const StitchMem &m) {
    if (pin) m.release(pin);
    pin = nullptr;
    pin_cap = pin_size = 0;
    vec.clear();
  }
};

enum StitchKind { STITCH_FIXED = 0, STITCH_BOOL = 1, STITCH_UTF8 = 2 };

// one column of a piece as the stage reads it.  `validity` is NULL for a piece that has no NULLs (no pointer, or null_count 0).
struct StitchPiece {
  const void *values = nullptr;      // fixed width: n x width bytes; Boolean: ceil(n / 8) bytes; Utf8: the chars offsets index
  const uint8_t *validity = nullptr; // ceil(n / 8) bytes
  const int32_t *offsets = nullptr;  // Utf8: n + 1, 0 <= offsets[0] <= offsets[n]
};

struct StitchBits {
  StitchBuf raw;
  std::vector<int64_t> byte_start; // per piece; -1 = all ones
  bool any = false;                // a piece staged bytes
};

struct StitchCol {
  int kind = STITCH_FIXED;
  size_t width = 0;           // STITCH_FIXED
  StitchBuf vals;             // fixed-width values, or a Utf8 column's chars
  StitchBuf offs;             // Utf8: raw offsets
  std::vector<int64_t> delta; // Utf8, per piece
  StitchBits valid, bits;     // validity; a Boolean column's values
  int64_t chars() const { return (int64_t)vals.size(); }
};

struct StitchStage {
  StitchMem mem;
  int64_t pin_rows = 1ll << 16; // staged rows from which the arrays are pinned memory
  std::vector<int64_t> row_start{0};
  std::vector<StitchCol> cols;
  int64_t rows = 0;
  int64_t pieces() const { return (int64_t)row_start.size() - 1; }

  // the schema of the pieces to come; a stage that held the same number of columns keeps their pinned blocks
  void begin(int ncols, const int *kinds, const size_t *widths) {
    if (cols.size() != (size_t)ncols) {
      drop();
      cols.resize((size_t)ncols);
    }
    for (int i = 0; i < ncols; i++) {
      cols[(size_t)i].kind = kinds[i];
      cols[(size_t)i].width = widths[i];
    }
  }

  // would appending this piece take a Utf8 column's staged chars past `cap`?  (The stage is flushed first then; a single piece
  // beyond the cap is never staged: piece_over_cap.)
  bool would_pass_cap(int64_t n, const StitchPiece *p, int64_t cap) const {
    for (size_t i = 0; i < cols.size(); i++)
      if (cols[i].kind == STITCH_UTF8 && cols[i].chars() + ((int64_t)p[i].offsets[n] - p[i].offsets[0]) > cap) return true;
    return false;
  }
  static bool piece_over_cap(int64_t n, const int32_t *offsets, int64_t cap) { return (int64_t)offsets[n] - offsets[0] > cap; }

  void append(int64_t n, const StitchPiece *p) {
    const bool use_pin = rows + n >= pin_rows;
    const size_t nbytes = (size_t)((n + 7) >> 3);
    // every array's room first, then the copies: a failed allocation leaves the stage as it was
    row_start.reserve(row_start.size() + 1);
    for (size_t i = 0; i < cols.size(); i++) {
      StitchCol &c = cols[i];
      c.valid.byte_start.reserve(c.valid.byte_start.size() + 1);
      if (p[i].validity) c.valid.raw.room(nbytes, use_pin, mem, (size_t)1 << 17);
      if (c.kind == STITCH_FIXED) c.vals.room(c.width * (size_t)n, use_pin, mem, c.width << 20);
      else if (c.kind == STITCH_BOOL) {
        c.bits.byte_start.reserve(c.bits.byte_start.size() + 1);
        c.bits.raw.room(nbytes, use_pin, mem, (size_t)1 << 17);
      } else {
        c.delta.reserve(c.delta.size() + 1);
        c.vals.room((size_t)(p[i].offsets[n] - p[i].offsets[0]), use_pin, mem, (size_t)16 << 20);
        c.offs.room(4 * ((size_t)n + 1), use_pin, mem, (size_t)4 << 20);
      }
    }
    for (size_t i = 0; i < cols.size(); i++) {
      StitchCol &c = cols[i];
      if (p[i].validity && n > 0) {
        c.valid.byte_start.push_back((int64_t)c.valid.raw.size());
        c.valid.raw.put(p[i].validity, nbytes);
        c.valid.any = true;
      } else
        c.valid.byte_start.push_back(-1);
      if (c.kind == STITCH_FIXED) c.vals.put(p[i].values, c.width * (size_t)n);
      else if (c.kind == STITCH_BOOL) {
        c.bits.byte_start.push_back((int64_t)c.bits.raw.size());
        c.bits.raw.put(p[i].values, nbytes);
        c.bits.any = true;
      } else {
        const int32_t first = p[i].offsets[0], last = p[i].offsets[n];
        c.delta.push_back(c.chars() - (int64_t)first);
        c.vals.put(last > first ? (const uint8_t *)p[i].values + first : nullptr, (size_t)(last - first)); // (values may be NULL for an empty range)
        c.offs.put(p[i].offsets, 4 * ((size_t)n + 1));
      }
    }
    rows += n;
    row_start.push_back(rows);
  }

  // empties the stage; the pinned blocks stay with their column for the next flush
  void clear() {
    for (StitchCol &c : cols) {
      c.vals.clear();
      c.offs.clear();
      c.delta.clear();
      for (StitchBits *b : {&c.valid, &c.bits}) {
        b->raw.clear();
        b->byte_start.clear();
        b->any = false;
      }
    }
    row_start.assign(1, 0);
    rows = 0;
  }
  void drop() {
    for (StitchCol &c : cols) {
      c.vals.drop(mem);
      c.offs.drop(mem);
      c.valid.raw.drop(mem);
      c.bits.raw.drop(mem);
    }
    cols.clear();
    row_start.assign(1, 0);
    rows = 0;
  }
};

} // namespace sq
