// Stand-alone check of dense_range_decide (sqlrs_amd/csrc/dense_range.hpp): the one decision whether a build side's key
// range takes the join's direct-address table — and of dense_verdict_decide beside it: what the finished attempt says about the
// build side (adopt / not unique / dup range usable).  No HIP: built by tests/test_join_model_cpu.py with
//   g++ -std=c++17 -fsanitize=address,undefined -I sqlrs_amd/csrc host/dense_range_check.cpp
// and run; exit status 0 = every row of the table below holds.  `lo`, `hi` are ORDERED images (0 = INT64_MIN, ~0 = INT64_MAX).
#include "dense_range.hpp"

#include <cinttypes>
#include <cstdio>

int main() {
  const uint64_t ALL = ~0ull, BIG = 1ull << 40, MR = 4 * 1000 + 1024; // (MR: slots per key x rows + 1024 of a 1 000-row build side)
  const struct {
    const char *what;
    uint64_t lo, hi, max_range;
    bool ok;
    uint64_t range; // (looked at when ok)
  } rows[] = {
      {"INT64_MIN and INT64_MAX: hi - lo + 1 wraps to 0", 0, ALL, MR, false, 0},
      {"the same under the largest max_range", 0, ALL, ALL, false, 0},
      {"INT64_MIN and INT64_MAX - 1: 2^64 - 1 values", 0, ALL - 1, MR, false, 0},
      {"the same under the largest max_range", 0, ALL - 1, ALL, false, 0},
      {"a range of exactly max_range", 500, 500 + MR - 1, MR, true, MR},
      {"a range of max_range + 1", 500, 500 + MR, MR, false, 0},
      {"exactly max_range, ending on INT64_MAX", ALL - (MR - 1), ALL, MR, true, MR},
      {"exactly max_range, starting on INT64_MIN", 0, MR - 1, MR, true, MR},
      {"span 2^31 - 2 (range 2^31 - 1) under a large max_range", 7, 7 + ((1ull << 31) - 2), BIG, true, (1ull << 31) - 1},
      {"span 2^31 - 1 (range 2^31) under a large max_range", 7, 7 + ((1ull << 31) - 1), BIG, false, 0},
      {"no valid key: lo = ~0 > hi = 0", ALL, 0, MR, false, 0},
      {"no valid key, next to each other", 6, 5, MR, false, 0},
      {"one key", 12345, 12345, MR, true, 1},
      {"one key: INT64_MIN", 0, 0, MR, true, 1},
      {"one key: INT64_MAX", ALL, ALL, MR, true, 1},
      {"one key under max_range 1", 9, 9, 1, true, 1},
      {"two keys under max_range 1", 9, 10, 1, false, 0},
      {"anything under max_range 0", 9, 9, 0, false, 0},
  };
  int bad = 0;
  for (const auto &r : rows) {
    const DenseRange d = dense_range_decide(r.lo, r.hi, r.max_range);
    const bool same = d.ok == r.ok && (!r.ok || d.range == r.range);
    if (!same) {
      bad++;
      std::printf("FAIL %s: lo %" PRIu64 " hi %" PRIu64 " max_range %" PRIu64 " -> ok %d range %" PRIu64 ", expected ok %d range %" PRIu64 "\n", r.what,
                  r.lo, r.hi, r.max_range, (int)d.ok, d.range, (int)r.ok, r.range);
    }
  }
  // dense_verdict_decide: what the finished attempt says about a 1 000-row build side whose valid keys lie in [lo, hi]
  const struct {
    const char *what;
    uint64_t lo, hi, occupied, nulls, rows;
    bool had_validity, adopt, not_unique, dup_range;
  } verdicts[] = {
      {"unique, no NULL", 100, 1099, 1000, 0, 1000, false, true, false, false},
      {"unique, a bitmap without NULLs", 100, 1099, 1000, 0, 1000, true, true, false, false},
      {"exactly one NULL key: adopted", 100, 1098, 999, 1, 1000, true, true, false, false},
      {"two NULL keys match each other: not unique, no dup range", 100, 1097, 998, 2, 1000, true, false, true, false},
      {"duplicates, no NULL: dup range", 100, 599, 500, 0, 1000, false, false, true, true},
      {"duplicates under a bitmap with zero NULLs: no dup range", 100, 599, 500, 0, 1000, true, false, true, false},
      {"duplicates and one NULL: no dup range", 100, 598, 499, 1, 1000, true, false, true, false},
      {"range refused (max_range + 1): nothing known", 0, MR, 1000, 0, 1000, false, false, false, false},
      {"range refused, duplicates: nothing known", 0, ALL, 500, 0, 1000, false, false, false, false},
      {"lo > hi (every key NULL, one row): nothing known", ALL, 0, 0, 1, 1, true, false, false, false},
      {"lo > hi, 1 000 NULL keys: nothing known", ALL, 0, 0, 1000, 1000, true, false, false, false},
  };
  for (const auto &r : verdicts) {
    const DenseVerdict v = dense_verdict_decide(dense_range_decide(r.lo, r.hi, MR), r.occupied, r.nulls, r.rows, r.had_validity);
    if (v.adopt != r.adopt || v.not_unique != r.not_unique || v.dup_range != r.dup_range) {
      bad++;
      std::printf("FAIL %s: adopt %d not_unique %d dup_range %d, expected %d %d %d\n", r.what, (int)v.adopt, (int)v.not_unique,
                  (int)v.dup_range, (int)r.adopt, (int)r.not_unique, (int)r.dup_range);
    }
  }
  std::printf("%d of %d rows failed\n", bad, (int)(sizeof(rows) / sizeof(rows[0]) + sizeof(verdicts) / sizeof(verdicts[0])));
  return bad ? 1 : 0;
}
