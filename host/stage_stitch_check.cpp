// stage_stitch_check.cpp — sqlrs_amd/csrc/stage_stitch.hpp on the host, meant for -fsanitize=address,undefined
// (tests/test_host_stage_types_cpu.py builds and runs it): the pieces of every case of tests/host_stage_cases.py — read from
// the file named by argv[1], every buffer in a heap block of exactly its size — are appended through the header's
// bookkeeping, stitch_bits_word / stitch_offset are called for every word and row, and the result is compared with a naive
// bit-by-bit / string-by-string concatenation.  One line per case: "<case> <digest>", the digest of
// host_stage_cases.case_digest.  Every case runs three times — staged in vectors, staged in "pinned" blocks (malloc here),
// and again on the emptied stage that kept those blocks — and must give the same bytes.  Then the cap decision with a
// cap of 100 bytes.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I sqlrs_amd/csrc host/stage_stitch_check.cpp
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "stage_stitch.hpp"

using namespace sq;

namespace {

[[noreturn]] void die(const std::string &m) {
  std::fprintf(stderr, "stage_stitch_check: %s\n", m.c_str());
  std::exit(1);
}

struct Blob { // a heap block of exactly the buffer's size (or no block: a NULL pointer)
  std::unique_ptr<uint8_t[]> p;
  int64_t len = -1;
  const uint8_t *ptr() const { return len < 0 ? nullptr : p.get(); }
};
int64_t read_i64(FILE *f) {
  int64_t v;
  if (std::fread(&v, 8, 1, f) != 1) die("short case file");
  return v;
}
Blob read_blob(FILE *f) {
  Blob b;
  b.len = read_i64(f);
  if (b.len >= 0) {
    b.p.reset(new uint8_t[(size_t)b.len]); // (length 0: still a block of its own)
    if (b.len && std::fread(b.p.get(), 1, (size_t)b.len, f) != (size_t)b.len) die("short case file");
  }
  return b;
}

struct PieceCol { Blob values, validity, offsets; };
struct PieceIn { int64_t n; std::vector<PieceCol> cols; };

void put_i64(std::vector<uint8_t> &o, int64_t v) { o.insert(o.end(), (const uint8_t *)&v, (const uint8_t *)&v + 8); }
void put_bytes(std::vector<uint8_t> &o, const void *p, size_t n) { if (n) o.insert(o.end(), (const uint8_t *)p, (const uint8_t *)p + n); }

// the stitched columns of a filled stage, in the byte form the digest is taken over
std::vector<uint8_t> stitched_bytes(const StitchStage &st) {
  std::vector<uint8_t> o;
  const int64_t P = st.pieces(), rows = st.rows, words = (rows + 63) / 64;
  const int64_t *rs = st.row_start.data();
  auto bits_of = [&](const StitchBits &b) {
    std::vector<uint64_t> w((size_t)words + 1);
    for (int64_t i = 0; i <= words; i++) w[(size_t)i] = stitch_bits_word(b.raw.data(), rs, b.byte_start.data(), P, rows, i);
    if (w[(size_t)words] != 0) die("the padding word is not 0");
    w.pop_back();
    return w;
  };
  for (const StitchCol &c : st.cols) {
    const int64_t nulls = c.valid.any ? stitch_count_clear(c.valid.raw.data(), rs, c.valid.byte_start.data(), P) : 0;
    put_i64(o, nulls);
    if (nulls) {
      std::vector<uint64_t> w = bits_of(c.valid);
      put_bytes(o, w.data(), 8 * w.size());
    }
    if (c.kind == STITCH_FIXED) put_bytes(o, c.vals.data(), c.vals.size());
    else if (c.kind == STITCH_BOOL) {
      std::vector<uint64_t> w = bits_of(c.bits);
      put_bytes(o, w.data(), 8 * w.size());
    } else {
      if ((int64_t)c.offs.size() != 4 * (rows + P)) die("raw offsets: not rows + pieces entries");
      std::vector<int32_t> off((size_t)rows + 1);
      for (int64_t r = 0; r <= rows; r++)
        off[(size_t)r] = stitch_offset((const int32_t *)c.offs.data(), rs, c.delta.data(), P, rows, c.chars(), r);
      put_bytes(o, off.data(), 4 * off.size());
      put_bytes(o, c.vals.data(), c.vals.size());
    }
  }
  return o;
}

// the same bytes, bit by bit and string by string, straight from the pieces
std::vector<uint8_t> naive_bytes(const std::vector<PieceIn> &pieces, const std::vector<int> &kinds, const std::vector<size_t> &widths) {
  std::vector<uint8_t> o;
  int64_t rows = 0;
  for (const PieceIn &p : pieces) rows += p.n;
  const size_t words = (size_t)((rows + 63) / 64);
  for (size_t c = 0; c < kinds.size(); c++) {
    std::vector<uint64_t> valid(words, 0), bits(words, 0);
    std::vector<int32_t> off{0};
    std::vector<uint8_t> vals;
    int64_t g = 0, nulls = 0;
    for (const PieceIn &p : pieces) {
      const PieceCol &pc = p.cols[c];
      for (int64_t r = 0; r < p.n; r++, g++) {
        const bool v = !pc.validity.ptr() || ((pc.validity.ptr()[r >> 3] >> (r & 7)) & 1);
        if (v) valid[(size_t)(g >> 6)] |= 1ull << (g & 63);
        else nulls++;
        if (kinds[c] == STITCH_BOOL && ((pc.values.ptr()[r >> 3] >> (r & 7)) & 1)) bits[(size_t)(g >> 6)] |= 1ull << (g & 63);
        if (kinds[c] == STITCH_UTF8) {
          const int32_t *po = (const int32_t *)pc.offsets.ptr();
          for (int32_t k = po[r]; k < po[r + 1]; k++) vals.push_back(pc.values.ptr()[k]);
          off.push_back((int32_t)vals.size());
        }
      }
      if (kinds[c] == STITCH_FIXED) put_bytes(vals, pc.values.ptr(), widths[c] * (size_t)p.n);
    }
    put_i64(o, nulls);
    if (nulls) put_bytes(o, valid.data(), 8 * words);
    if (kinds[c] == STITCH_BOOL) put_bytes(o, bits.data(), 8 * words);
    if (kinds[c] == STITCH_UTF8) put_bytes(o, off.data(), 4 * off.size());
    if (kinds[c] != STITCH_BOOL) put_bytes(o, vals.data(), vals.size());
  }
  return o;
}

uint64_t digest(const std::vector<uint8_t> &b) {
  uint64_t h = 0xcbf29ce484222325ULL;
  for (uint8_t x : b) h = h * 0x100000001b3ULL + ((uint64_t)x + 1);
  return h;
}

void *pin_alloc(size_t n) {
  void *p = std::malloc(n);
  if (!p) die("out of memory");
  return p;
}
void pin_release(void *p) { std::free(p); }

void fill(StitchStage &st, const std::vector<PieceIn> &pieces, const std::vector<int> &kinds, const std::vector<size_t> &widths) {
  st.begin((int)kinds.size(), kinds.data(), widths.data());
  std::vector<StitchPiece> sp(kinds.size());
  for (const PieceIn &p : pieces) {
    for (size_t c = 0; c < kinds.size(); c++) {
      sp[c].values = p.cols[c].values.ptr();
      sp[c].validity = p.cols[c].validity.ptr();
      sp[c].offsets = (const int32_t *)p.cols[c].offsets.ptr();
    }
    st.append(p.n, sp.data());
  }
}

void check_cap() {
  const int kind = STITCH_UTF8;
  const size_t width = 0;
  StitchStage st;
  st.mem = StitchMem{pin_alloc, pin_release};
  st.begin(1, &kind, &width);
  std::vector<uint8_t> chars(140, 'x');
  const int32_t off40[3] = {7, 30, 47}, off0[2] = {5, 5}, off100[2] = {20, 120}, off101[2] = {20, 121};
  StitchPiece p;
  p.values = chars.data();
  p.offsets = off40;
  const int64_t cap = 100;
  if (st.would_pass_cap(2, &p, cap)) die("cap: an empty stage refuses 40 bytes");
  st.append(2, &p);
  if (st.would_pass_cap(2, &p, cap)) die("cap: 80 bytes refused");
  st.append(2, &p);
  if (st.cols[0].chars() != 80) die("cap: 80 staged bytes expected");
  if (!st.would_pass_cap(2, &p, cap)) die("cap: 120 bytes accepted");
  p.offsets = off0;
  if (st.would_pass_cap(1, &p, cap)) die("cap: an empty string refused at 80 bytes");
  const int32_t off20[2] = {100, 120}, off21[2] = {100, 121};
  p.offsets = off20;
  if (st.would_pass_cap(1, &p, cap)) die("cap: exactly 100 bytes refused");
  p.offsets = off21;
  if (!st.would_pass_cap(1, &p, cap)) die("cap: 101 bytes accepted");
  if (StitchStage::piece_over_cap(1, off100, cap)) die("cap: a piece of exactly 100 bytes refused");
  if (!StitchStage::piece_over_cap(1, off101, cap)) die("cap: a piece of 101 bytes accepted");
  st.clear();
  p.offsets = off100;
  if (st.would_pass_cap(1, &p, cap)) die("cap: the emptied stage refuses 100 bytes");
  st.drop();
  std::printf("cap ok\n");
}

} // namespace

int main(int argc, char **argv) {
  if (argc < 2) die("usage: stage_stitch_check CASEFILE");
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) die("cannot open the case file");
  const int64_t ncases = read_i64(f);
  for (int64_t ci = 0; ci < ncases; ci++) {
    const int64_t P = read_i64(f), nc = read_i64(f);
    std::vector<int> kinds((size_t)nc);
    std::vector<size_t> widths((size_t)nc);
    for (int64_t c = 0; c < nc; c++) {
      kinds[(size_t)c] = (int)read_i64(f);
      widths[(size_t)c] = (size_t)read_i64(f);
    }
    std::vector<PieceIn> pieces((size_t)P);
    for (PieceIn &p : pieces) {
      p.n = read_i64(f);
      p.cols.resize((size_t)nc);
      for (PieceCol &pc : p.cols) {
        pc.values = read_blob(f);
        pc.validity = read_blob(f);
        pc.offsets = read_blob(f);
      }
    }
    const std::vector<uint8_t> want = naive_bytes(pieces, kinds, widths);
    StitchStage vec_stage, pin_stage;
    vec_stage.mem = pin_stage.mem = StitchMem{pin_alloc, pin_release};
    vec_stage.pin_rows = 1ll << 40; // never pinned
    pin_stage.pin_rows = 100;       // pinned from 100 staged rows on (the vectors' content moves over)
    fill(vec_stage, pieces, kinds, widths);
    if (stitched_bytes(vec_stage) != want) die("case " + std::to_string(ci) + ": staged in vectors, the stitch differs from the naive concatenation");
    for (int round = 0; round < 2; round++) { // the second round reuses the blocks the first one left
      fill(pin_stage, pieces, kinds, widths);
      if (stitched_bytes(pin_stage) != want) die("case " + std::to_string(ci) + ": staged in pinned blocks (round " + std::to_string(round) + "), the stitch differs");
      pin_stage.clear();
    }
    vec_stage.drop();
    pin_stage.drop();
    std::printf("%lld %016llx\n", (long long)ci, (unsigned long long)digest(want));
  }
  std::fclose(f);
  check_cap();
  return 0;
}
