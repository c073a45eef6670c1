// key_hash.hpp — the arithmetic of a hashed join / group key (normalize_keys' hash mode, keys.hip), in ONE place: the fold_*
// kernels of keys.hip fold a column at a time over device columns, the key loader of the one-launch probe kernels (join_async.hip,
// sa_probe_key) folds a row at a time over the columns staged in a pinned slot.  Both must produce the same 64 bits for the same
// row — the build side's table is keyed by the former, a probe row is looked up by the latter.
//   acc = 0; per key column, in order: a NULL leaves acc unchanged (hash_utils.rs:91-104), otherwise
//   v = mix64(value + tag)  (int32 zero-extended, tag KEY_TAG_32; int64 / float64 by bit pattern, tag KEY_TAG_64)
//   v = mix64(fnv1a(bytes) ^ KEY_TAG_UTF8)  (Utf8),  v = mix64(bit ^ KEY_TAG_BOOL)  (Boolean)
//   acc = combine_hashes(v, acc) for several columns, acc = v for one.
// No HIP include: host/key_hash_check.cpp compiles it with a host compiler.
#pragma once
#include <cstdint>

#ifndef SQLRS_HD
#ifdef __HIPCC__
#define SQLRS_HD __host__ __device__
#else
#define SQLRS_HD
#endif
#endif

namespace sq {

SQLRS_HD inline __attribute__((always_inline)) uint64_t mix64(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}

constexpr uint64_t KEY_TAG_32 = 0x3232323200000000ULL, KEY_TAG_64 = 0x9e3779b97f4a7c15ULL, KEY_TAG_UTF8 = 0x7575757575757575ULL,
                   KEY_TAG_BOOL = 0x0808080808080808ULL;

SQLRS_HD inline __attribute__((always_inline)) uint64_t combine_hashes(uint64_t l, uint64_t r) { // hash_utils.rs:13-16
  uint64_t h = (uint64_t)(17 * 37) + l;
  return h * 37 + r;
}
// one valid value of a fixed-width column; `x`: the value's bits (int32: zero-extended)
SQLRS_HD inline __attribute__((always_inline)) uint64_t key_hash_fixed(uint64_t x, uint64_t tag) { return mix64(x + tag); }
SQLRS_HD inline __attribute__((always_inline)) uint64_t key_hash_bool(uint64_t bit) { return mix64(bit ^ KEY_TAG_BOOL); }
// FNV-1a over bytes [beg, end) of `data`
SQLRS_HD inline __attribute__((always_inline)) uint64_t key_fnv1a(const uint8_t *data, int64_t beg, int64_t end) {
  uint64_t x = 0xcbf29ce484222325ULL;
  for (int64_t k = beg; k < end; k++) {
    x ^= data[k];
    x *= 0x100000001b3ULL;
  }
  return x;
}
SQLRS_HD inline __attribute__((always_inline)) uint64_t key_hash_utf8(const uint8_t *data, int64_t beg, int64_t end) {
  return mix64(key_fnv1a(data, beg, end) ^ KEY_TAG_UTF8);
}
// a valid value's hash `v` into the running hash of its row
SQLRS_HD inline __attribute__((always_inline)) uint64_t key_fold(uint64_t v, uint64_t acc, bool multi) { return multi ? combine_hashes(v, acc) : v; }

} // namespace sq
