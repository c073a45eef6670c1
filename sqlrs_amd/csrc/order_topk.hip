// order_topk.hip — ORDER BY ... LIMIT k with a first key the plain route (ops.hip order_topk) leaves out: a Utf8 column, a
// fixed-width column with NULLs, a key expression (SQLRS_ORDER_LIMIT_ALL_KEYS).  The candidates-only idea is the same:
// a threshold T from a sorted sample, the rows at or below T kept in input order, those sorted on all keys.  What differs is
// how a row is compared with T.  A row's WEAK IMAGE is: NULL below every valid row whatever the direction; a valid
// fixed-width key its ordered 64-bit image (i64_to_ordered / f64_to_ordered); a valid Utf8 key its first 64 bytes as eight
// big-endian 64-bit words, zero padded (chunks 0..7 of ops.hip utf8_chunk_key_kernel), compared word by word; DESC
// complements the words.  Truncation and zero padding are monotone: a <= b in the ORDER BY's own order implies
// image(a) <= image(b), so {rows : image <= image(T)} is downward closed in the true order, and once it holds k rows it holds
// the first k of the full result.  Rows that tie with T on all 64 bytes are kept.
//  * the sample: the same 65 536 evenly spaced rows and the same quantile as order_topk, gathered into a small column and
//    sorted as the operator sorts (Utf8: the strings themselves through sort_perm_by_utf8, not their images), NULLs first;
//  * the mask: ONE pass, order_topk_mask_kernel — T travels by value in the kernel arguments, one __ballot word per 64 rows
//    and one count per tile of TILE_ROWS rows; a scan of the counts, one fetch of the total, then the kept rows' u32 ids
//    (selection_rows_u32, range_partition.hip).  The caller gathers and sorts.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.hpp"
#include "device_utils.hpp"
#include "prims.hpp"

namespace sq {

constexpr int TK_WORDS = 8;      // 64-bit words of a Utf8 key's image (its first 64 bytes)
constexpr int TK_CHUNKS_FIXED = 8; // 64-row words per wave and trip, fixed-width keys: 8 independent loads in flight
constexpr int TK_CHUNKS_UTF8 = 4;  // ... Utf8 keys (two offsets per row, then the bytes)

// the threshold row's image in the ASCENDING form (the kernel applies the direction)
struct TopkBound {
  uint64_t w[TK_WORDS]; // fixed width: w[0] only
  uint32_t valid;       // 0: the threshold row is NULL — the candidates are exactly the NULL rows
  uint32_t desc;
};

// KIND: 0 i64, 1 f64, 2 i32, 3 utf8
template <int KIND> __device__ __forceinline__ uint64_t topk_image(const void *vals, int64_t r) {
  if (KIND == 0) return i64_to_ordered(__builtin_nontemporal_load((const int64_t *)vals + r));
  if (KIND == 1) return f64_to_ordered(__builtin_nontemporal_load((const double *)vals + r));
  return i64_to_ordered((int64_t)__builtin_nontemporal_load((const int32_t *)vals + r));
}

// word `c` of the image of the string s[0 .. len): bytes at or past `len` are never read
__device__ __forceinline__ uint64_t topk_utf8_word(const uint8_t *s, int32_t len, int c) {
  const int32_t left = len - 8 * c;
  uint64_t u = 0;
  if (left >= 8) {
    uint64_t x;
    __builtin_memcpy(&x, s + 8 * c, 8);
    u = __builtin_bswap64(x);
  } else {
    for (int k = 0; k < left; k++) u |= (uint64_t)s[8 * c + k] << (56 - 8 * k);
  }
  return u;
}

// image(string) <= image(T) in the requested direction; stops at the first differing word (almost every row: chunk 0, or
// the first chunk past a shared prefix); equal through the last word is a tie: kept
__device__ __forceinline__ bool topk_utf8_keep(const uint8_t *s, int32_t len, const TopkBound &T) {
  const uint64_t flip = T.desc ? ~0ull : 0ull;
#pragma unroll
  for (int c = 0; c < TK_WORDS; c++) {
    const uint64_t u = topk_utf8_word(s, len, c);
    if (u != T.w[c]) return (u ^ flip) < (T.w[c] ^ flip);
  }
  return true;
}

// keep[j] of row r0 + 64 j.  FULL: every row of the trip exists, the loads are unconditional (all of them in flight
// together).  Otherwise (the last trip of the column) rows past the end are not kept and touch no memory.
template <int KIND, bool NULLABLE, bool FULL, int CH>
__device__ __forceinline__ void topk_trip(const void *__restrict__ vals, const int32_t *__restrict__ off,
                                          const uint64_t *__restrict__ validity, const TopkBound &T, int64_t r0, int64_t n,
                                          bool (&keep)[CH]) {
  const int lane = (int)(r0 & 63);
  uint64_t vw[CH];
#pragma unroll
  for (int j = 0; j < CH; j++) {
    const int64_t r = r0 + 64 * j;
    vw[j] = (NULLABLE && (FULL || r < n)) ? validity[r >> 6] : ~0ull;
  }
  if (KIND != 3) {
    uint64_t raw[CH];
    const uint64_t flip = T.desc ? ~0ull : 0ull, bound = T.w[0] ^ flip;
#pragma unroll
    for (int j = 0; j < CH; j++) {
      const int64_t r = r0 + 64 * j;
      raw[j] = (FULL || r < n) ? topk_image<KIND == 3 ? 0 : KIND>(vals, r) : 0ull;
    }
#pragma unroll
    for (int j = 0; j < CH; j++) {
      const bool in = FULL || r0 + 64 * j < n, v = (vw[j] >> lane) & 1;
      keep[j] = in && (!v || (T.valid && (raw[j] ^ flip) <= bound));
    }
  } else {
    int32_t a[CH], b[CH];
#pragma unroll
    for (int j = 0; j < CH; j++) {
      const int64_t r = r0 + 64 * j;
      const bool in = FULL || r < n;
      a[j] = in ? off[r] : 0;
      b[j] = in ? off[r + 1] : 0;
    }
#pragma unroll
    for (int j = 0; j < CH; j++) {
      const bool in = FULL || r0 + 64 * j < n, v = (vw[j] >> lane) & 1;
      bool k = in && !v; // a NULL row: below every valid row, its bytes are not read
      if (in && v && T.valid) k = topk_utf8_keep((const uint8_t *)vals + a[j], b[j] - a[j], T);
      keep[j] = k;
    }
  }
}

// one wave = one tile of TILE_ROWS rows (grid-stride), CH 64-row words per trip; lane j stores word j of its trip, lane 0
// the tile's kept rows (range_select_mask_kernel's layout: selection_rows_u32 reads it)
template <int KIND, bool NULLABLE>
__global__ __launch_bounds__(BLOCK) void order_topk_mask_kernel(const void *__restrict__ vals, const int32_t *__restrict__ off,
                                                                const uint64_t *__restrict__ validity, const TopkBound T,
                                                                int64_t n, int64_t nwords, int64_t ntiles,
                                                                uint64_t *__restrict__ bits, uint32_t *__restrict__ tile_cnt) {
  constexpr int CH = KIND == 3 ? TK_CHUNKS_UTF8 : TK_CHUNKS_FIXED;
  static_assert(TILE_WORDS % CH == 0, "a trip stays inside its tile");
  const int lane = lane_id();
  const int64_t wave = (blockIdx.x * (int64_t)BLOCK + threadIdx.x) >> 6, waves = ((int64_t)gridDim.x * BLOCK) >> 6;
  for (int64_t tile = wave; tile < ntiles; tile += waves) {
    uint32_t cnt = 0;
    for (int64_t w0 = tile * TILE_WORDS; w0 < min((tile + 1) * TILE_WORDS, nwords); w0 += CH) {
      const int64_t r0 = w0 * 64 + lane;
      bool keep[CH];
      if ((w0 + CH) * 64 <= n) topk_trip<KIND, NULLABLE, true, CH>(vals, off, validity, T, r0, n, keep);
      else topk_trip<KIND, NULLABLE, false, CH>(vals, off, validity, T, r0, n, keep);
      uint64_t mine = 0;
#pragma unroll
      for (int j = 0; j < CH; j++) {
        const uint64_t b = __ballot(keep[j]);
        mine = lane == j ? b : mine;
        cnt += (uint32_t)__popcll(b);
      }
      if (lane < CH && w0 + lane < nwords) bits[w0 + lane] = mine;
    }
    if (lane == 0) tile_cnt[tile] = cnt;
  }
}

// ---- the sample (S rows: cheap kernels, one thread per row)
__global__ void topk_sample_rows_kernel(int64_t n, int64_t step, int64_t S, uint32_t *__restrict__ rows) {
  const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (s < S) rows[s] = (uint32_t)min(s * step, n - 1);
}
// sort keys of the gathered sample, as ops.hip sort_key_kernel over an identity permutation: NULL rows tie with key 0
template <int KIND>
__global__ void topk_sample_key_kernel(const void *__restrict__ vals, const uint64_t *__restrict__ validity, int64_t S, int desc,
                                       uint64_t *__restrict__ keys) {
  const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (s >= S) return;
  uint64_t u = 0;
  if (!validity || ((validity[s >> 6] >> (s & 63)) & 1)) {
    u = topk_image<KIND>(vals, s);
    if (desc) u = ~u;
  }
  keys[s] = u;
}
__global__ void topk_sample_valid_kernel(const uint64_t *__restrict__ validity, const uint32_t *__restrict__ perm, int64_t S,
                                         uint64_t *__restrict__ keys) {
  const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (s >= S) return;
  const uint32_t r = perm[s];
  keys[s] = (validity[r >> 6] >> (r & 63)) & 1; // NULL (0) first
}
// the q-th sorted sample's validity and image -> out[0], out[1 .. 1 + TK_WORDS)  (one wave; lane c writes word c)
template <int KIND>
__global__ void topk_bound_kernel(const void *__restrict__ vals, const int32_t *__restrict__ off,
                                  const uint64_t *__restrict__ validity, const uint32_t *__restrict__ perm, int64_t q,
                                  uint64_t *__restrict__ out) {
  const int c = (int)threadIdx.x;
  if (c >= TK_WORDS) return;
  const uint32_t r = perm[q];
  const bool v = !validity || ((validity[r >> 6] >> (r & 63)) & 1);
  uint64_t u = 0;
  if (v) {
    if (KIND == 3) u = topk_utf8_word((const uint8_t *)vals + off[r], off[r + 1] - off[r], c);
    else if (c == 0) u = topk_image<KIND == 3 ? 0 : KIND>(vals, (int64_t)r);
  }
  out[1 + c] = u;
  if (c == 0) out[0] = v ? 1ull : 0ull;
}

// `key`: the first ORDER BY key over all n rows (Int32 / Int64 / Float64 / Utf8, materialised); `limit` rows will be read.
// true: *idx holds the u32 ids of the *count candidate rows in input order (limit <= *count <= n / 2).  false: a guard
// ignored the hint — fewer candidates than `limit` (the sample misjudged the column), or more than n / 2 (NULLs are the
// majority, or the strings agree on their first 64 bytes: nothing is gathered, the full sort is the cheaper way).
bool order_topk_keys_select(Ctx *ctx, const DCol &key, int desc, int64_t n, int64_t limit, BufP *idx, int64_t *count) {
  const int kind = key.dtype == SQLRS_INT64 ? 0 : key.dtype == SQLRS_FLOAT64 ? 1 : key.dtype == SQLRS_INT32 ? 2 : 3;
  if (kind == 3 && key.dtype != SQLRS_UTF8) fail(SQLRS_ERR_INTERNAL, "order top-k: unsupported first key type");
  const uint64_t *valid = (key.validity && key.null_count != 0) ? key.validity : nullptr;
  // 1. the threshold: the q-th of S sampled rows in the ORDER BY's own order of the first key, NULLs first
  const int64_t S = 65536, step = n / S;
  const int64_t q = std::min<int64_t>(S - 1, (int64_t)std::ceil((double)limit * (double)S / (double)n * 2.0) + 64);
  TopkBound T{};
  T.desc = desc ? 1u : 0u;
  {
    ProfScope ps(ctx, "order_topk_keys_sample");
    dim3 g((unsigned)ceil_div(S, 256)), b(256);
    BufP rows = ctx->alloc(4 * (size_t)S), perm = ctx->alloc(4 * (size_t)S), keys = ctx->alloc(8 * (size_t)S);
    topk_sample_rows_kernel<<<g, b, 0, ctx->stream>>>(n, step, S, rows->as<uint32_t>());
    SQ_HIP(hipGetLastError());
    // (a small column of its own: sort_perm_by_utf8 sizes its passes by the first S offsets of the column it is given)
    const DCol sc = gather_column(ctx, key, rows->p, false, nullptr, S);
    const uint64_t *sv = sc.validity;
    iota_u32(ctx, perm->as<uint32_t>(), S);
    if (kind == 3) {
      sort_perm_by_utf8(ctx, sc, sv, desc, perm->as<uint32_t>(), keys->as<uint64_t>(), S);
    } else {
      if (kind == 0) topk_sample_key_kernel<0><<<g, b, 0, ctx->stream>>>(sc.values, sv, S, desc, keys->as<uint64_t>());
      else if (kind == 1) topk_sample_key_kernel<1><<<g, b, 0, ctx->stream>>>(sc.values, sv, S, desc, keys->as<uint64_t>());
      else topk_sample_key_kernel<2><<<g, b, 0, ctx->stream>>>(sc.values, sv, S, desc, keys->as<uint64_t>());
      SQ_HIP(hipGetLastError());
      radix_sort_pairs(ctx, keys->as<uint64_t>(), perm->as<uint32_t>(), S, 0, 64);
    }
    if (sv) { // nulls first whatever the direction
      topk_sample_valid_kernel<<<g, b, 0, ctx->stream>>>(sv, perm->as<uint32_t>(), S, keys->as<uint64_t>());
      SQ_HIP(hipGetLastError());
      radix_sort_pairs(ctx, keys->as<uint64_t>(), perm->as<uint32_t>(), S, 0, 8);
    }
    BufP bound = ctx->alloc(8 * (1 + TK_WORDS));
    if (kind == 0) topk_bound_kernel<0><<<1, 64, 0, ctx->stream>>>(sc.values, sc.offsets, sv, perm->as<uint32_t>(), q, bound->as<uint64_t>());
    else if (kind == 1) topk_bound_kernel<1><<<1, 64, 0, ctx->stream>>>(sc.values, sc.offsets, sv, perm->as<uint32_t>(), q, bound->as<uint64_t>());
    else if (kind == 2) topk_bound_kernel<2><<<1, 64, 0, ctx->stream>>>(sc.values, sc.offsets, sv, perm->as<uint32_t>(), q, bound->as<uint64_t>());
    else topk_bound_kernel<3><<<1, 64, 0, ctx->stream>>>(sc.values, sc.offsets, sv, perm->as<uint32_t>(), q, bound->as<uint64_t>());
    SQ_HIP(hipGetLastError());
    const uint64_t *h = (const uint64_t *)ctx->fetch(bound->p, 8 * (1 + TK_WORDS));
    T.valid = h[0] ? 1u : 0u;
    for (int c = 0; c < TK_WORDS; c++) T.w[c] = h[1 + c];
  }
  // 2. the candidates' bits and their number
  const int64_t nwords = ceil_div(n, 64), ntiles = ceil_div(n, TILE_ROWS);
  BufP bits = ctx->alloc(8 * (size_t)nwords), cnt = ctx->alloc(4 * (size_t)ntiles), total = ctx->alloc(8);
  BufP tile_off = ctx->alloc(8 * (size_t)ntiles);
  {
    ProfScope ps(ctx, "order_topk_keys_mask");
    const dim3 g((unsigned)std::min<int64_t>(ceil_div(ntiles, WAVES_PER_BLOCK), 2048)), b(BLOCK);
    uint64_t *bp = bits->as<uint64_t>();
    uint32_t *cp = cnt->as<uint32_t>();
#define SQ_TOPK_MASK(K, NV) \
  order_topk_mask_kernel<K, NV><<<g, b, 0, ctx->stream>>>(key.values, key.offsets, valid, T, n, nwords, ntiles, bp, cp)
    switch (kind * 2 + (valid ? 1 : 0)) {
    case 0: SQ_TOPK_MASK(0, false); break;
    case 1: SQ_TOPK_MASK(0, true); break;
    case 2: SQ_TOPK_MASK(1, false); break;
    case 3: SQ_TOPK_MASK(1, true); break;
    case 4: SQ_TOPK_MASK(2, false); break;
    case 5: SQ_TOPK_MASK(2, true); break;
    case 6: SQ_TOPK_MASK(3, false); break;
    default: SQ_TOPK_MASK(3, true); break;
    }
#undef SQ_TOPK_MASK
    SQ_HIP(hipGetLastError());
    exclusive_scan_u32(ctx, cnt->as<uint32_t>(), ntiles, tile_off->as<uint64_t>(), nullptr, total->as<uint64_t>());
  }
  const int64_t kept = (int64_t)ctx->fetch_value(total->as<uint64_t>()); // the one count fetch
  if (kept < limit || kept > n / 2) return false;
  // 3. the kept rows' ids
  *idx = ctx->alloc(4 * (size_t)std::max<int64_t>(kept, 1));
  if (kept) selection_rows_u32(ctx, bits->as<uint64_t>(), tile_off->as<uint64_t>(), n, (*idx)->as<uint32_t>());
  *count = kept;
  return true;
}

} // namespace sq
