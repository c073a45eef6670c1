// Stand-alone run of the hashed-key arithmetic (sqlrs_amd/csrc/key_hash.hpp): the key of every row of three fixed tables, computed
// the way the probe kernels' loader does — row by row over columns of values, offsets, bytes and validity bits.  No HIP: built by
// tests/test_async_join_keys_cpu.py with
//   g++ -std=c++17 -fsanitize=address,undefined -I sqlrs_amd/csrc host/key_hash_check.cpp
// and run; it prints `<table> <row> <key in hex>` per row, which the test compares with tests/async_keys_cases.py's restatement of
// the same arithmetic over the same tables (KEY_TABLES).  Every column lives in a heap block of exactly its size, so a read past a
// string's last byte or a column's last value is the sanitizer's to report.
#include "key_hash.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace {
enum Kind { I32, I64, F64, STR };
struct Column {
  Kind kind;
  size_t rows = 0;
  std::unique_ptr<uint8_t[]> values;  // fixed width: rows x width bytes; STR: the bytes
  std::unique_ptr<int32_t[]> offsets; // STR: rows + 1
  std::unique_ptr<uint8_t[]> valid;   // one bit per row, LSB first
};
struct Cell {
  bool null;
  int64_t i;
  double f;
  std::string s;
};
Cell N() { return {true, 0, 0.0, ""}; }
Cell I(int64_t v) { return {false, v, 0.0, ""}; }
Cell F(double v) { return {false, 0, v, ""}; }
Cell S(const std::string &v) { return {false, 0, 0.0, v}; }

Column make(Kind kind, const std::vector<Cell> &cells) {
  Column c;
  c.kind = kind;
  c.rows = cells.size();
  c.valid.reset(new uint8_t[(c.rows + 7) / 8]());
  for (size_t r = 0; r < c.rows; r++)
    if (!cells[r].null) c.valid[r >> 3] |= (uint8_t)(1u << (r & 7));
  if (kind == STR) {
    size_t total = 0;
    for (const Cell &x : cells) total += x.s.size();
    c.values.reset(new uint8_t[total ? total : 1]);
    c.offsets.reset(new int32_t[c.rows + 1]);
    size_t at = 0;
    for (size_t r = 0; r < c.rows; r++) {
      c.offsets[r] = (int32_t)at;
      if (!cells[r].s.empty()) std::memcpy(c.values.get() + at, cells[r].s.data(), cells[r].s.size());
      at += cells[r].s.size();
    }
    c.offsets[c.rows] = (int32_t)at;
  } else {
    const size_t w = kind == I32 ? 4 : 8;
    c.values.reset(new uint8_t[c.rows * w ? c.rows * w : 1]);
    for (size_t r = 0; r < c.rows; r++) {
      if (kind == I32) {
        const int32_t v = (int32_t)cells[r].i;
        std::memcpy(c.values.get() + r * 4, &v, 4);
      } else if (kind == I64) {
        std::memcpy(c.values.get() + r * 8, &cells[r].i, 8);
      } else {
        std::memcpy(c.values.get() + r * 8, &cells[r].f, 8);
      }
    }
  }
  return c;
}
// sa_probe_key's hash mode (join.hip) over host columns
uint64_t row_key(const std::vector<Column> &cols, size_t r) {
  uint64_t acc = 0;
  for (const Column &c : cols) {
    if (!((c.valid[r >> 3] >> (r & 7)) & 1)) continue;
    uint64_t v;
    if (c.kind == STR) {
      v = sq::key_hash_utf8(c.values.get(), c.offsets[r], c.offsets[r + 1]);
    } else if (c.kind == I32) {
      uint32_t x;
      std::memcpy(&x, c.values.get() + r * 4, 4);
      v = sq::key_hash_fixed((uint64_t)x, sq::KEY_TAG_32);
    } else {
      uint64_t x;
      std::memcpy(&x, c.values.get() + r * 8, 8);
      v = sq::key_hash_fixed(x, sq::KEY_TAG_64);
    }
    acc = sq::key_fold(v, acc, cols.size() > 1);
  }
  return acc;
}
void run(int table, const std::vector<Column> &cols) {
  for (size_t r = 0; r < cols[0].rows; r++) std::printf("%d %zu %016" PRIx64 "\n", table, r, row_key(cols, r));
}
} // namespace

int main() {
  {
    std::vector<Column> t;
    t.push_back(make(STR, {S(""), N(), S("a"), S("ab"), S("abc"), S("abd"), S("12345678"), S("123456789"), S(std::string(200, 'x')),
                           S("\xc3\xa9\xe6\xbc\xa2\xf0\x9f\x99\x82")}));
    run(0, t);
  }
  {
    std::vector<Column> t;
    t.push_back(make(I64, {I(1), I(2), N(), I(5), N(), I(-1), I(0)}));
    t.push_back(make(I64, {I(2), I(1), I(5), N(), N(), I(INT64_MIN), I(0)}));
    run(1, t);
  }
  {
    std::vector<Column> t;
    t.push_back(make(F64, {F(0.5), N(), F(0.5), F(0.5), F(0.5), F(-0.0), N(), F(1e300)}));
    t.push_back(make(I64, {I(7), I(7), N(), I(7), I(7), I(0), N(), I(INT64_MAX)}));
    t.push_back(make(STR, {S("k"), S("k"), S("k"), N(), S("k"), S(""), N(), S("Zo\xc3\xab")}));
    t.push_back(make(I32, {I(-1), I(-1), I(-1), I(-1), N(), I(0), N(), I(2147483647)}));
    run(2, t);
  }
  return 0;
}
