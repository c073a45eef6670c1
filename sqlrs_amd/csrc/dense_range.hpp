// Whether a build side's key range takes the direct-address table of the join: ONE decision, shared by the device-side
// verdict (dense_dev, join_probe_kernels.hpp), the host's reading of the same words (dense_resolve, join.hip) and the
// two-fetch build (dense_try_two_fetch, join.hip).  No HIP include: host/dense_range_check.cpp compiles it with a host compiler.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define SQLRS_HD __host__ __device__
#else
#define SQLRS_HD
#endif

struct DenseRange {
  bool ok;
  uint64_t range; // hi - lo + 1 (meaningful when ok)
};
// `lo`, `hi`: the smallest and largest valid key as ORDERED images (i64_to_ordered: they differ like the signed values);
// lo > hi: no valid key.  Accepted: 1 <= range <= max_range and range < 2^31.  The test is made on span = hi - lo, which
// cannot wrap for lo <= hi — `hi - lo + 1` is 0 for a key set that holds INT64_MIN and INT64_MAX (lo = 0, hi = ~0), and a
// range of 0 passed `range <= max_range`: a table of no entry addressed with offsets anywhere in 2^64.
SQLRS_HD inline DenseRange dense_range_decide(uint64_t lo, uint64_t hi, uint64_t max_range) {
  const uint64_t span = hi - lo;
  DenseRange d;
  d.ok = lo <= hi && span < max_range && span < (1ull << 31) - 1;
  d.range = span + 1;
  return d;
}

// What a finished attempt says about the build side, for the one-fetch and the two-fetch build alike (dense_apply_verdict)
struct DenseVerdict {
  bool adopt;      // unique keys over an accepted range: the direct-address table becomes the join's table
  bool not_unique; // an accepted range whose keys repeat: `unique = false` is a fact (nothing is known under a refused range)
  bool dup_range;  // ... and none of them NULL: [min, min + range) serves the multiplicities per key (hash_join_dup_mult)
};
// `occupied`: slots that hold a row; `nulls`: build rows with a NULL key (one is kept beside the table, several match each
// other); `had_validity`: the keys came with a bitmap, NULL in it or not.  Fewer occupied slots than valid keys = a key repeats.
SQLRS_HD inline DenseVerdict dense_verdict_decide(DenseRange dr, uint64_t occupied, uint64_t nulls, uint64_t rows, bool had_validity) {
  DenseVerdict v;
  v.adopt = dr.ok && nulls <= 1 && occupied + nulls == rows;
  v.not_unique = dr.ok && !v.adopt;
  v.dup_range = v.not_unique && nulls == 0 && !had_validity;
  return v;
}
