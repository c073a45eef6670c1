// join_table.hpp — how a probe kernel reads the two tables of the HashJoinExecutor: the open-addressing table of 16-byte slots
// (join_kernels.hpp) and the direct-address table.  No kernel in here: join.hip (through join_probe_kernels.hpp) and join_async.hip
// both include it.
#pragma once
#include "common.hpp"
#include "device_utils.hpp"
#include "prims.hpp"
#include "join_kernels.hpp"

namespace sq {

// returns the slot of `key` (count may be 0 for the two reserved slots) or count==0 on a miss
__device__ __forceinline__ Slot probe_slot(const Slot *__restrict__ table, uint64_t mask, uint64_t key,
                                           bool is_null) {
  const uint64_t cap = mask + 1;
  if (is_null) return load_slot(&table[cap]);
  if (key == EMPTY_KEY) return load_slot(&table[cap + 1]);
  uint64_t s = mix64(key) & mask;
  while (true) {
    Slot sl = load_slot(&table[s]);
    if (sl.key == key) return sl;
    if (sl.key == EMPTY_KEY) {
      sl.count = 0;
      return sl;
    }
    s = (s + 1) & mask;
  }
}

// Direct-address table for build keys that are unique and cover a small integer range (the
// dense surrogate keys of a dimension table): heads[key - kmin] = build row.  4 bytes per
// possible key instead of a 16-byte hash slot at load factor <= 2/3: a 1e6-key dimension needs
// 4 MiB, which one XCD's L2 holds (265 G lookups/s instead of 66 G/s, profiles/r01_ubench).
// Round 5: the probe kernels read a BIT-PACKED copy of the table when there is one — `bits` = ceil(log2(rows + 1)) bits per
// possible key (all ones = empty), entry e at bit e * bits, fetched with ONE unaligned 4-byte load (bits <= 25).  20 bits
// instead of 32 for 1e6 build rows: 2.4 MiB instead of 3.8, which is what lets the table stay in its XCD's 4 MiB L2 NEXT TO
// the key stream and the pair stores (the probe's time is the sum of its L1 miss latencies over 64 miss slots per CU,
// profiles/r02_probe_pmc_ta.txt, and a lookup that has left L2 holds its slot 3-5x longer).  tools/ubench2.hip, same memory
// work and nothing else, 1e8 keys against 1e6: 0.654 ms with 4-byte entries, 0.516 with 3-byte, 0.520 with 20-bit ones
// (profiles/r05a_ubench2.txt, r05b_ubench2.txt); 2e6 build rows: 1.08 -> 0.78 ms.
typedef uint32_t __attribute__((aligned(1))) u32_unaligned;
struct DenseTable {
  const uint32_t *heads;
  uint64_t kmin, range;
  uint32_t null_head; // build row whose key is NULL (NULL = NULL matches) or DENSE_EMPTY
  const uint8_t *packed = nullptr; // bit-packed copy of heads[0 .. range + 2) or null
  uint32_t bits = 0, pmask = 0;    // bits per entry, (1 << bits) - 1 = the packed form of DENSE_EMPTY
  // the build's verdict is still on the device (sqlrs_hash_join::dense_pending): kmin / range are read from `st` by the
  // kernel (dense_table_from_device), which raises bit 1 of its miss flag when the build keys are not a unique dense set
  const unsigned long long *st = nullptr;
  uint64_t st_max_range = 0, st_rows = 0;
};
__device__ __forceinline__ uint32_t dense_packed_raw(const uint8_t *__restrict__ packed, uint32_t bits, uint32_t pmask, uint32_t e) {
  const uint32_t bit = e * bits; // (the host packs only tables of less than 2^32 bits)
  return (*(const u32_unaligned *)(packed + (bit >> 3)) >> (bit & 7)) & pmask;
}
// entry d (d <= range + 1) of the table: the build row or DENSE_EMPTY
__device__ __forceinline__ uint32_t dense_get(const DenseTable &dt, uint64_t d) {
  if (dt.packed) {
    const uint32_t v = dense_packed_raw(dt.packed, dt.bits, dt.pmask, (uint32_t)d);
    return v == dt.pmask ? DENSE_EMPTY : v;
  }
  return dt.heads[d];
}

} // namespace sq
