// Whether a build side's key range takes the direct-address table of the join: ONE decision, shared by the device-side
// verdict (dense_dev, join_probe_kernels.hpp), the host's reading of the same words (dense_resolve, join.hip) and the
// two-fetch build (build_table, join.hip).  No HIP include: host/dense_range_check.cpp compiles it with a host compiler.
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
