// range_partition.hip — range partitioning of a batch for the multi-GPU ORDER BY (a sample sort over the exchange):
// sample (sqlrs_range_sample) -> splitters on the host (sqlrs_range_splitters) -> stable range partition
// (sqlrs_range_partition) -> the hash exchange's all-to-all -> the ordinary Order on every rank.
//
// A row's tuple is its ORDER BY image followed by its global position (include/sqlrs_hip.h): per key a validity word
// (0 = NULL) and the key encoded exactly as the local Order sorts it (ops.hip sort_key_kernel: i64_to_ordered,
// f64_to_ordered, int32 widened to int64, BOOLEAN 0 / 1, complemented for DESC, 0 for NULL), then row_base + row.
// Compared word by word as unsigned integers, the tuples of a table are all distinct and ordered like the rows of
// sqlrs_order's result (NULLs first, ties in input order), so concatenating every rank's sorted part in rank order IS
// that result.
//  * general path (any key list of fixed-width types, any payload): the tuples are written to HBM (one kernel per key +
//    the positions), a search kernel finds every row's part against the splitters and counts per part in LDS, then one
//    stable 8-bit radix pass on the part gives the permutation and every column is gathered (sqlrs_hash_partition's tail);
//  * fast path (one int64 / float64 key column without NULLs, <= 3 carried 8-byte columns without NULLs, >= 2^16 rows):
//    the multi-split of split_kernels.hpp with RangePart: the histogram pass binary-searches the splitters in LDS and
//    leaves the part of every row as a byte, the scatter reads it back; every column is read once and written once,
//    8 + 16 * columns + 2 bytes per row.
#include <algorithm>
#include <cmath>
#include <numeric>

#include "common.hpp"
#include "device_utils.hpp"
#include "prims.hpp"
#include "split_kernels.hpp"

namespace sq {

// kind: 0 i64, 1 f64, 2 i32, 3 bool.  Output row i reads source row i * n / m (m = n: every row in order).
template <int KIND>
__global__ void range_key_words_kernel(const void *__restrict__ vals, const uint64_t *__restrict__ validity, int64_t m,
                                       int64_t n, uint64_t flip, int word, int tw, uint64_t *__restrict__ tup) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= m) return;
  const int64_t r = m == n ? i : i * n / m;
  uint64_t v = 0, u = 0;
  if (!validity || ((validity[r >> 6] >> (r & 63)) & 1)) {
    v = 1;
    if (KIND == 0) u = i64_to_ordered(((const int64_t *)vals)[r]);
    else if (KIND == 1) u = f64_to_ordered(((const double *)vals)[r]);
    else if (KIND == 2) u = i64_to_ordered((int64_t)((const int32_t *)vals)[r]);
    else u = (((const uint64_t *)vals)[r >> 6] >> (r & 63)) & 1;
    u ^= flip;
  }
  tup[i * tw + word] = v;
  tup[i * tw + word + 1] = u;
}

__global__ void range_pos_kernel(int64_t m, int64_t n, int64_t row_base, int tw, uint64_t *__restrict__ tup) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= m) return;
  tup[i * tw + tw - 1] = (uint64_t)(row_base + (m == n ? i : i * n / m));
}

// part of every row = number of splitters <= its tuple (binary search over p2 - 1 padded splitters, in LDS when they
// fit); per-part counts through an LDS histogram, like part_ids_kernel (partition.hip)
__global__ __launch_bounds__(BLOCK) void range_part_ids_kernel(const uint64_t *__restrict__ tup, int tw, int64_t n,
                                                               const uint64_t *__restrict__ spl, uint32_t parts,
                                                               uint32_t p2, int spl_in_lds, uint64_t *__restrict__ pid,
                                                               unsigned long long *__restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rp_smem[];
  __shared__ unsigned int h[256];
  uint64_t *s = (uint64_t *)rp_smem;
  h[threadIdx.x] = 0;
  if (spl_in_lds)
    for (int64_t t = threadIdx.x; t < (int64_t)(p2 - 1) * tw; t += BLOCK) s[t] = spl[t];
  const uint64_t *sp = spl_in_lds ? s : spl;
  __syncthreads();
  for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
    const uint64_t *t = tup + i * tw;
    uint32_t at = 0;
    for (uint32_t step = p2 >> 1; step; step >>= 1) {
      const uint64_t *c = sp + (int64_t)(at + step - 1) * tw;
      bool le = true; // splitter <= row tuple
      for (int w = 0; w < tw; w++) {
        const uint64_t a = c[w], b = t[w];
        if (a != b) {
          le = a < b;
          break;
        }
      }
      if (le) at += step;
    }
    pid[i] = at;
    atomicAdd(&h[at], 1u);
  }
  __syncthreads();
  if (threadIdx.x < parts && h[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

// the fast path's part starts: part p begins where its first tile's run begins (one fetch instead of one copy per part)
__global__ void range_starts_kernel(const uint32_t *__restrict__ offs, int64_t ntiles, uint32_t parts,
                                    uint32_t *__restrict__ starts) {
  const uint32_t p = threadIdx.x;
  if (p < parts) starts[p] = offs[(int64_t)p * ntiles];
}

// ---- range select (ORDER BY ... LIMIT k over ranks): the rows whose tuple is strictly below ONE bound tuple, in input
// order.  The tuple is never written: the mask kernel encodes every key on the fly (the helpers of range_key_words_kernel)
// and compares it with the bound word by word; one __ballot word per 64 rows and the kept rows per tile, then a scan of
// those, the kept rows' ids and one gather per column.
constexpr int RS_MAXK = 16;  // keys the kernel arguments hold (more: the tuples are written and compared, range_below_kernel)
constexpr int RS_CHUNKS = 8; // 64-row words per wave and trip: 8 independent 512-byte loads in flight per key
struct RsKey {
  const void *vals;
  const uint64_t *validity; // nullptr: no NULLs
  uint64_t flip;            // ~0 for DESC
  int kind;                 // 0 i64, 1 f64, 2 i32, 3 bool (as range_key_words_kernel)
};
struct RsArgs {
  RsKey key[RS_MAXK];
  uint64_t bound[2 * RS_MAXK]; // per key the bound's validity word and key word
  uint64_t pos;                // the bound's position word
  int nk;
};

template <int KIND> __device__ __forceinline__ uint64_t rs_encode(const void *vals, int64_t r) {
  if (KIND == 0) return i64_to_ordered(__builtin_nontemporal_load((const int64_t *)vals + r));
  if (KIND == 1) return f64_to_ordered(__builtin_nontemporal_load((const double *)vals + r));
  if (KIND == 2) return i64_to_ordered((int64_t)__builtin_nontemporal_load((const int32_t *)vals + r));
  return (((const uint64_t *)vals)[r >> 6] >> (r & 63)) & 1;
}

// st[j] of row r0 + 64 j: 0 = equal to the bound so far, 1 = below it, 2 = above it (or past the end).  The loads are
// unconditional (rows past the end read row n - 1) so that all RS_CHUNKS of them are in flight together: loads under a
// per-row branch were issued one at a time, each behind a wait (0.30 ms for 1e8 int64 keys).
template <int KIND, bool HASV>
__device__ __forceinline__ void rs_compare_key(const RsKey &kd, uint64_t bv, uint64_t bu, int64_t r0, int64_t n,
                                               uint32_t (&st)[RS_CHUNKS]) {
  uint64_t raw[RS_CHUNKS], vw[RS_CHUNKS];
#pragma unroll
  for (int j = 0; j < RS_CHUNKS; j++) {
    const int64_t r = min(r0 + 64 * j, n - 1);
    vw[j] = HASV ? kd.validity[r >> 6] : ~0ull;
    raw[j] = rs_encode<KIND>(kd.vals, r);
  }
#pragma unroll
  for (int j = 0; j < RS_CHUNKS; j++)
    if (st[j] == 0) {
      const int64_t r = r0 + 64 * j;
      const uint64_t v = (vw[j] >> (r & 63)) & 1, u = v ? raw[j] ^ kd.flip : 0ull; // NULL: validity word 0, key 0
      if (v != bv) st[j] = v < bv ? 1 : 2;
      else if (u != bu) st[j] = u < bu ? 1 : 2;
    }
}

// one wave = one tile of TILE_ROWS rows (grid-stride), RS_CHUNKS 64-row words per trip; lane j stores word j of its trip,
// lane 0 the tile's kept rows (a plain scan of them gives the compaction's tile offsets)
__global__ __launch_bounds__(BLOCK) void range_select_mask_kernel(const RsArgs a, int64_t n, int64_t row_base, int64_t nwords,
                                                                  int64_t ntiles, uint64_t *__restrict__ bits,
                                                                  uint32_t *__restrict__ tile_cnt) {
  const int lane = lane_id();
  const int64_t wave = (blockIdx.x * (int64_t)BLOCK + threadIdx.x) >> 6, waves = ((int64_t)gridDim.x * BLOCK) >> 6;
  for (int64_t tile = wave; tile < ntiles; tile += waves) {
    uint32_t cnt = 0;
    for (int64_t w0 = tile * TILE_WORDS; w0 < min((tile + 1) * TILE_WORDS, nwords); w0 += RS_CHUNKS) {
      const int64_t r0 = w0 * 64 + lane;
      uint32_t st[RS_CHUNKS];
#pragma unroll
      for (int j = 0; j < RS_CHUNKS; j++) st[j] = r0 + 64 * j < n ? 0u : 2u;
      for (int k = 0; k < a.nk; k++) {
        bool open = false;
#pragma unroll
        for (int j = 0; j < RS_CHUNKS; j++) open |= st[j] == 0;
        if (__ballot(open) == 0) break; // every row of the trip decided by the earlier keys: the later ones are not read
        const RsKey &kd = a.key[k];
        const uint64_t bv = a.bound[2 * k], bu = a.bound[2 * k + 1];
        switch (kd.kind * 2 + (kd.validity ? 1 : 0)) {
        case 0: rs_compare_key<0, false>(kd, bv, bu, r0, n, st); break;
        case 1: rs_compare_key<0, true>(kd, bv, bu, r0, n, st); break;
        case 2: rs_compare_key<1, false>(kd, bv, bu, r0, n, st); break;
        case 3: rs_compare_key<1, true>(kd, bv, bu, r0, n, st); break;
        case 4: rs_compare_key<2, false>(kd, bv, bu, r0, n, st); break;
        case 5: rs_compare_key<2, true>(kd, bv, bu, r0, n, st); break;
        case 6: rs_compare_key<3, false>(kd, bv, bu, r0, n, st); break;
        default: rs_compare_key<3, true>(kd, bv, bu, r0, n, st); break;
        }
      }
      uint64_t mine = 0;
#pragma unroll
      for (int j = 0; j < RS_CHUNKS; j++) {
        const bool keep = st[j] == 1 || (st[j] == 0 && (uint64_t)(row_base + r0 + 64 * j) < a.pos); // equal keys: position
        const uint64_t b = __ballot(keep);
        mine = lane == j ? b : mine;
        cnt += (uint32_t)__popcll(b);
      }
      if (lane < RS_CHUNKS && w0 + lane < nwords) bits[w0 + lane] = mine;
    }
    if (lane == 0) tile_cnt[tile] = cnt;
  }
}

// u32 ids of the kept rows, one wave per tile of TILE_ROWS rows (grid-stride): a tile without a kept row costs one load.
// (select.hip's compaction runs one workgroup per tile: 57 us per column for 1e8 rows, almost all of it on empty tiles.)
__global__ __launch_bounds__(BLOCK) void range_select_rows_kernel(const uint64_t *__restrict__ bits,
                                                                  const uint64_t *__restrict__ tile_off, int64_t nwords,
                                                                  int64_t ntiles, uint32_t *__restrict__ out) {
  const int lane = lane_id();
  const int64_t wave = (blockIdx.x * (int64_t)BLOCK + threadIdx.x) >> 6, waves = ((int64_t)gridDim.x * BLOCK) >> 6;
  for (int64_t tile = wave; tile < ntiles; tile += waves) {
    const int64_t wi = tile * TILE_WORDS + lane;
    const uint64_t m = wi < nwords ? bits[wi] : 0ull;
    if (__ballot(m != 0) == 0) continue;
    const uint32_t pc = (uint32_t)__popcll(m);
    const uint32_t excl = wave_iscan_u32(pc) - pc;
    const uint64_t base = tile_off[tile];
    for (int W = 0; W < TILE_WORDS; W++) {
      const uint64_t mw = shfl_u64(m, W);
      if (mw == 0) continue;
      const uint32_t off = (uint32_t)__shfl((int)excl, W, 64);
      if ((mw >> lane) & 1) out[base + off + mbcnt(mw)] = (uint32_t)((tile * TILE_WORDS + W) * 64 + lane);
    }
  }
}

void selection_rows_u32(Ctx *ctx, const uint64_t *bits, const uint64_t *tile_off, int64_t rows, uint32_t *out) {
  ProfScope ps(ctx, "range_select_rows");
  const int64_t nwords = ceil_div(std::max<int64_t>(rows, 1), 64), ntiles = ceil_div(rows, TILE_ROWS);
  const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(ntiles, WAVES_PER_BLOCK), 1024);
  range_select_rows_kernel<<<dim3(blocks), dim3(BLOCK), 0, ctx->stream>>>(bits, tile_off, nwords, ntiles, out);
  SQ_HIP(hipGetLastError());
}

// range_select_mask_kernel's bits over tuples written to HBM (more than RS_MAXK keys); the bound in LDS
__global__ __launch_bounds__(BLOCK) void range_below_kernel(const uint64_t *__restrict__ tup, int tw, int64_t n,
                                                            const uint64_t *__restrict__ bound, uint64_t *__restrict__ bits) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rb_smem[];
  uint64_t *b = (uint64_t *)rb_smem;
  for (int w = threadIdx.x; w < tw; w += BLOCK) b[w] = bound[w];
  __syncthreads();
  const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
  bool keep = false;
  if (i < n)
    for (int w = 0; w < tw; w++) {
      const uint64_t x = tup[i * tw + w];
      if (x != b[w]) {
        keep = x < b[w];
        break;
      }
    }
  const uint64_t m = __ballot(keep);
  if (lane_id() == 0 && i < n) bits[i >> 6] = m;
}

inline int range_tuple_words(int num_keys) { return 2 * num_keys + 1; }

// lexicographic unsigned comparison of two tuples of `tw` words
inline bool tuple_less(const uint64_t *a, const uint64_t *b, int tw) {
  for (int w = 0; w < tw; w++)
    if (a[w] != b[w]) return a[w] < b[w];
  return false;
}

struct RangeKeys {
  std::vector<Expr> exprs;
  std::vector<int> desc;
};

RangeKeys range_keys(int num_keys, const sqlrs_order_by_t *order_by, const char *what = "range partition") {
  if (num_keys < 1 || !order_by) fail(SQLRS_ERR_INTERNAL, std::string(what) + ": at least one ORDER BY key is needed");
  RangeKeys k;
  for (int i = 0; i < num_keys; i++) {
    k.exprs.push_back(expr_from_abi(&order_by[i].expr));
    k.desc.push_back(order_by[i].asc ? 0 : 1);
  }
  return k;
}

// the ORDER BY keys evaluated over the batch; every key is checked (and evaluated) before the first launch of the caller: a
// refused key type leaves nothing queued
std::vector<DCol> range_eval_keys(Ctx *ctx, InBatch &ib, const RangeKeys &rk, const char *what = "range partition") {
  const int64_t n = ib.rows();
  auto colfn = [&](int i) -> const DCol & {
    if (i < 0 || i >= ib.num_columns()) fail(SQLRS_ERR_INTERNAL, "input ref out of range");
    return ib.col(i);
  };
  std::vector<DCol> keys;
  for (size_t k = 0; k < rk.exprs.size(); k++) {
    DCol c = eval_expr(ctx, rk.exprs[k], colfn, n, true);
    if (c.dtype == SQLRS_UTF8)
      fail(SQLRS_ERR_INTERNAL, std::string(what) + ": Utf8 ORDER BY keys are not supported (fixed-width keys only)");
    if (c.dtype != SQLRS_INT64 && c.dtype != SQLRS_FLOAT64 && c.dtype != SQLRS_INT32 && c.dtype != SQLRS_BOOLEAN)
      fail(SQLRS_ERR_INTERNAL, std::string(what) + ": unsupported ORDER BY key type");
    keys.push_back(std::move(c));
  }
  return keys;
}

// writes the m tuples of the rows i * n / m (i < m; m = n: every row) to `tup` (m * tw words, device)
void range_tuples_of(Ctx *ctx, const std::vector<DCol> &keys, const RangeKeys &rk, int64_t n, int64_t m, int64_t row_base,
                     uint64_t *tup) {
  const int tw = range_tuple_words((int)rk.exprs.size());
  if (m == 0) return;
  dim3 g((unsigned)ceil_div(m, 256)), b(256);
  for (size_t k = 0; k < keys.size(); k++) {
    const DCol &c = keys[k];
    const uint64_t *valid = (c.validity && c.null_count != 0) ? c.validity : nullptr;
    const uint64_t flip = rk.desc[k] ? ~0ull : 0ull;
    const int word = 2 * (int)k;
    switch (c.dtype) {
    case SQLRS_INT64: range_key_words_kernel<0><<<g, b, 0, ctx->stream>>>(c.values, valid, m, n, flip, word, tw, tup); break;
    case SQLRS_FLOAT64: range_key_words_kernel<1><<<g, b, 0, ctx->stream>>>(c.values, valid, m, n, flip, word, tw, tup); break;
    case SQLRS_INT32: range_key_words_kernel<2><<<g, b, 0, ctx->stream>>>(c.values, valid, m, n, flip, word, tw, tup); break;
    default: range_key_words_kernel<3><<<g, b, 0, ctx->stream>>>(c.values, valid, m, n, flip, word, tw, tup); break;
    }
    SQ_HIP(hipGetLastError());
  }
  range_pos_kernel<<<g, b, 0, ctx->stream>>>(m, n, row_base, tw, tup);
  SQ_HIP(hipGetLastError());
}

void range_tuples(Ctx *ctx, InBatch &ib, const RangeKeys &rk, int64_t m, int64_t row_base, uint64_t *tup) {
  range_tuples_of(ctx, range_eval_keys(ctx, ib, rk), rk, ib.rows(), m, row_base, tup);
}

} // namespace sq

using namespace sq;

extern "C" int sqlrs_range_tuple_words(int num_keys) { return num_keys < 1 ? -1 : range_tuple_words(num_keys); }

extern "C" int sqlrs_range_sample(sqlrs_ctx_t *ctx, const sqlrs_batch_t *in, int num_keys, const sqlrs_order_by_t *order_by,
                                  int64_t row_base, int num_samples, uint64_t *tuples, int *written) {
  return guard(ctx, [&] {
    SQ_HIP(hipSetDevice(ctx->device));
    RangeKeys rk = range_keys(num_keys, order_by);
    if (num_samples < 0) fail(SQLRS_ERR_INTERNAL, "range sample: num_samples must be >= 0");
    if (row_base < 0) fail(SQLRS_ERR_INTERNAL, "range sample: row_base must be >= 0");
    if (!written || (num_samples > 0 && !tuples)) fail(SQLRS_ERR_INTERNAL, "range sample: null output pointer");
    InBatch ib(ctx, in);
    const int64_t m = std::min<int64_t>(num_samples, ib.rows());
    const int tw = range_tuple_words(num_keys);
    BufP t = ctx->alloc(8 * (size_t)tw * (size_t)std::max<int64_t>(m, 1));
    range_tuples(ctx, ib, rk, m, row_base, t->as<uint64_t>());
    if (m) SQ_HIP(hipMemcpyAsync(tuples, t->p, 8 * (size_t)tw * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    *written = (int)m;
  });
}

extern "C" int sqlrs_range_splitters(int num_keys, int64_t num_tuples, const uint64_t *tuples, int num_parts,
                                     uint64_t *splitters) {
  if (num_keys < 1 || num_tuples < 0 || (num_tuples > 0 && !tuples)) return SQLRS_ERR_INTERNAL;
  if (num_parts < 1 || num_parts > 256 || (num_parts > 1 && !splitters)) return SQLRS_ERR_INTERNAL;
  const int tw = range_tuple_words(num_keys);
  try {
    std::vector<int64_t> idx((size_t)num_tuples);
    std::iota(idx.begin(), idx.end(), (int64_t)0);
    std::stable_sort(idx.begin(), idx.end(),
                     [&](int64_t a, int64_t b) { return tuple_less(tuples + a * tw, tuples + b * tw, tw); });
    for (int j = 1; j < num_parts; j++) {
      uint64_t *dst = splitters + (size_t)(j - 1) * tw;
      if (num_tuples == 0) { // the maximum tuple: every row goes to part 0
        std::fill(dst, dst + tw, ~0ull);
        continue;
      }
      const uint64_t *src = tuples + idx[(size_t)((int64_t)j * num_tuples / num_parts)] * tw; // (j * T / W)-th smallest
      std::copy(src, src + tw, dst);
    }
  } catch (const std::exception &) {
    return SQLRS_ERR_INTERNAL;
  }
  return SQLRS_OK;
}

extern "C" int sqlrs_range_partition(sqlrs_ctx_t *ctx, const sqlrs_batch_t *in, int num_keys, const sqlrs_order_by_t *order_by,
                                     int64_t row_base, int num_parts, const uint64_t *splitters, int out_mem,
                                     sqlrs_batch_t **out, int64_t *offsets) {
  return guard(ctx, [&] {
    SQ_HIP(hipSetDevice(ctx->device));
    RangeKeys rk = range_keys(num_keys, order_by);
    if (num_parts < 1 || num_parts > 256) fail(SQLRS_ERR_INTERNAL, "range partition: num_parts must be in [1, 256]");
    if (num_parts > 1 && !splitters) fail(SQLRS_ERR_INTERNAL, "range partition: splitters is NULL with num_parts > 1");
    if (row_base < 0) fail(SQLRS_ERR_INTERNAL, "range partition: row_base must be >= 0");
    if (!out || !offsets) fail(SQLRS_ERR_INTERNAL, "range partition: null output pointer");
    const int tw = range_tuple_words(num_keys);
    for (int j = 1; j + 1 < num_parts; j++)
      if (tuple_less(splitters + (size_t)j * tw, splitters + (size_t)(j - 1) * tw, tw))
        fail(SQLRS_ERR_INTERNAL, "range partition: splitters are not nondecreasing (splitter " + std::to_string(j) +
                                     " < splitter " + std::to_string(j - 1) + ")");
    InBatch ib(ctx, in);
    const int64_t n = ib.rows();
    const int nc = ib.num_columns();
    // ---- fast path: one int64 / float64 key column without NULLs among <= 3 carried 8-byte columns without NULLs
    {
      const char *gen_e = hook("SQLRS_RANGE_PART_GENERAL"); // test / A-B hook, read per call: 1 = the general path
      bool fast = !(gen_e && gen_e[0] == '1') && n >= (1 << 16) && nc >= 1 && nc <= 3 && num_keys == 1 && num_parts > 1 &&
                  rk.exprs[0].nodes.size() == 1 && rk.exprs[0].nodes[0].op == SQLRS_EXPR_INPUT_REF &&
                  rk.exprs[0].nodes[0].index >= 0 && rk.exprs[0].nodes[0].index < nc;
      for (int c = 0; fast && c < nc; c++) {
        const DCol &col = ib.col(c);
        fast = width_of(col.dtype) == 8 && !(col.validity && col.null_count != 0) && col.stride != 0;
      }
      const int kcol = fast ? rk.exprs[0].nodes[0].index : -1;
      if (fast) fast = ib.col(kcol).dtype == SQLRS_INT64 || ib.col(kcol).dtype == SQLRS_FLOAT64;
      if (fast) {
        ProfScope ps(ctx, "range_partition");
        // the splitters as (encoded key, position) for rows whose key is valid: a NULL-key splitter (validity word 0)
        // is below every such row, a validity word above 1 above every row
        std::vector<uint64_t> sp2(2 * (size_t)(num_parts - 1));
        for (int j = 0; j + 1 < num_parts; j++) {
          const uint64_t *s = splitters + (size_t)j * tw;
          const uint64_t k = s[0] == 0 ? 0ull : (s[0] == 1 ? s[1] : ~0ull), p = s[0] == 0 ? 0ull : (s[0] == 1 ? s[2] : ~0ull);
          sp2[2 * (size_t)j] = k;
          sp2[2 * (size_t)j + 1] = p;
        }
        BufP dspl = ctx->alloc(8 * sp2.size());
        SQ_HIP(hipMemcpyAsync(dspl->p, sp2.data(), 8 * sp2.size(), hipMemcpyHostToDevice, ctx->stream));
        uint32_t p2 = 1;
        while (p2 < (uint32_t)num_parts) p2 <<= 1;
        const int64_t ntiles = ceil_div(n, SP_TILE);
        BufP hist = ctx->alloc(4 * (size_t)(num_parts * ntiles)), offs = ctx->alloc(4 * (size_t)(num_parts * ntiles));
        BufP total = ctx->alloc(8), starts = ctx->alloc(4 * 256);
        // the histogram pass stores every row's part as a byte that the scatter reads back instead of searching again:
        // +2 B per row of traffic, measured 0.84 against 1.14 ms for 1e8 rows into 8 parts
        const char *ids_e = hook("SQLRS_RANGE_PART_IDS"); // A/B hook, read per call: 0 = the scatter searches again
        const bool write_ids = !(ids_e && ids_e[0] == '0');
        BufP ids = write_ids ? ctx->alloc((size_t)n) : nullptr;
        DBatch o;
        o.rows = n;
        uint64_t *outp[3] = {nullptr, nullptr, nullptr};
        const uint64_t *inp[3] = {nullptr, nullptr, nullptr};
        for (int c = 0; c < nc; c++) {
          DCol oc;
          oc.dtype = ib.col(c).dtype;
          oc.length = n;
          oc.null_count = 0;
          oc.own_values = ctx->alloc(8 * (size_t)n + 16);
          oc.values = oc.own_values->p;
          outp[c] = oc.own_values->as<uint64_t>();
          inp[c] = ib.col(c).v<uint64_t>();
          o.cols.push_back(std::move(oc));
        }
        const size_t lds = (size_t)SP_TILE * (8 * (size_t)nc + 1);
        dim3 g((unsigned)ntiles), b(SP_WG);
        const uint64_t flip = rk.desc[0] ? ~0ull : 0ull;
        auto run = [&](auto pf) {
          using P = decltype(pf);
          if (write_ids)
            split_hist_kernel<P, true><<<g, b, 0, ctx->stream>>>(inp[kcol], n, pf, ntiles, hist->as<uint32_t>(), ids->as<uint8_t>());
          else
            split_hist_kernel<P, false><<<g, b, 0, ctx->stream>>>(inp[kcol], n, pf, ntiles, hist->as<uint32_t>(), nullptr);
          SQ_HIP(hipGetLastError());
          exclusive_scan_u32(ctx, hist->as<uint32_t>(), (int64_t)num_parts * ntiles, nullptr, offs->as<uint32_t>(),
                             total->as<uint64_t>());
          auto launch = [&](auto kfn) {
            allow_big_lds(ctx, kfn, 112 * 1024); // (+ ~15 KiB of static LDS: counters, run starts, the splitters)
            kfn<<<g, b, lds, ctx->stream>>>(inp[0], inp[1], inp[2], kcol, n, pf, ntiles, offs->as<uint32_t>(), outp[0], outp[1],
                                            outp[2], write_ids ? ids->as<uint8_t>() : nullptr);
          };
          if (write_ids) {
            if (nc == 1) launch(split_scatter_kernel<P, 1, true>);
            else if (nc == 2) launch(split_scatter_kernel<P, 2, true>);
            else launch(split_scatter_kernel<P, 3, true>);
          } else {
            if (nc == 1) launch(split_scatter_kernel<P, 1, false>);
            else if (nc == 2) launch(split_scatter_kernel<P, 2, false>);
            else launch(split_scatter_kernel<P, 3, false>);
          }
          SQ_HIP(hipGetLastError());
        };
        if (ib.col(kcol).dtype == SQLRS_INT64)
          run(RangePart<0>{(uint32_t)num_parts, p2, flip, row_base, dspl->as<u64x2>()});
        else
          run(RangePart<1>{(uint32_t)num_parts, p2, flip, row_base, dspl->as<u64x2>()});
        range_starts_kernel<<<dim3(1), dim3(256), 0, ctx->stream>>>(offs->as<uint32_t>(), ntiles, (uint32_t)num_parts,
                                                                    starts->as<uint32_t>());
        SQ_HIP(hipGetLastError());
        const uint32_t *st = (const uint32_t *)ctx->fetch(starts->p, 4 * (size_t)num_parts);
        for (int p = 0; p < num_parts; p++) offsets[p] = (int64_t)st[p];
        offsets[num_parts] = n;
        *out = emit_batch(ctx, std::move(o), out_mem);
        return;
      }
    }
    // ---- general path
    const int64_t n1 = std::max<int64_t>(n, 1);
    BufP tup = ctx->alloc(8 * (size_t)tw * (size_t)n1);
    range_tuples(ctx, ib, rk, n, row_base, tup->as<uint64_t>()); // (checks the key types even for an empty batch)
    BufP pid = ctx->alloc(8 * (size_t)n1), perm = ctx->alloc(4 * (size_t)n1);
    BufP counts = ctx->alloc_zero(8 * 256);
    if (n) {
      ProfScope ps(ctx, "range_partition");
      uint32_t p2 = 1;
      while (p2 < (uint32_t)num_parts) p2 <<= 1;
      // the splitters padded with all-ones tuples to p2 - 1 (no row tuple reaches one: its validity words are 0 / 1)
      std::vector<uint64_t> sp((size_t)std::max<uint32_t>(p2 - 1, 1) * tw, ~0ull);
      if (num_parts > 1) std::copy(splitters, splitters + (size_t)(num_parts - 1) * tw, sp.begin());
      BufP dspl = ctx->alloc(8 * sp.size());
      SQ_HIP(hipMemcpyAsync(dspl->p, sp.data(), 8 * sp.size(), hipMemcpyHostToDevice, ctx->stream));
      const size_t spl_bytes = 8 * (size_t)(p2 - 1) * tw;
      const bool in_lds = spl_bytes <= 48 * 1024;
      unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(n, BLOCK), 4096);
      range_part_ids_kernel<<<dim3(blocks), dim3(BLOCK), in_lds ? spl_bytes : 0, ctx->stream>>>(
          tup->as<uint64_t>(), tw, n, dspl->as<uint64_t>(), (uint32_t)num_parts, p2, in_lds ? 1 : 0, pid->as<uint64_t>(),
          counts->as<unsigned long long>());
      SQ_HIP(hipGetLastError());
      iota_u32(ctx, perm->as<uint32_t>(), n);
      if (num_parts > 1) radix_sort_pairs(ctx, pid->as<uint64_t>(), perm->as<uint32_t>(), n, 0, 8);
      ctx->sync(); // (the host copy of the padded splitters is read by the copy above)
    }
    std::vector<uint64_t> hc(256);
    SQ_HIP(hipMemcpyAsync(hc.data(), counts->p, 8 * 256, hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    offsets[0] = 0;
    for (int p = 0; p < num_parts; p++) offsets[p + 1] = offsets[p] + (int64_t)hc[(size_t)p];
    DBatch o;
    o.rows = n;
    for (int c = 0; c < nc; c++) o.cols.push_back(gather_column(ctx, ib.col(c), perm->p, false, nullptr, n));
    *out = emit_batch(ctx, std::move(o), out_mem);
  });
}

// j-th smallest gathered tuple as the bound of attempt `a`: j + 1 = (c + ceil(2 sqrt(c)) + 2) * 4^a with c = ceil(k T / N);
// -1 = past the last tuple (the all-ones bound)
static int64_t range_bound_index(int64_t T, int64_t N, int64_t k, int attempt) {
  const unsigned __int128 c = ((unsigned __int128)k * (unsigned __int128)T + (unsigned __int128)(N - 1)) / (unsigned __int128)N;
  if (c >= (unsigned __int128)T) return -1;
  unsigned __int128 r = (unsigned __int128)std::ceil(2.0 * std::sqrt((double)(uint64_t)c)); // smallest r with r * r >= 4 c
  while (r * r < 4 * c) r++;
  while (r > 0 && (r - 1) * (r - 1) >= 4 * c) r--;
  unsigned __int128 j1 = c + r + 2;
  for (int i = 0; i < attempt; i++) {
    j1 *= 4;
    if (j1 > (unsigned __int128)T) return -1;
  }
  return j1 > (unsigned __int128)T ? -1 : (int64_t)(j1 - 1);
}

extern "C" int sqlrs_range_bound(int num_keys, int64_t num_tuples, const uint64_t *tuples, int64_t total_rows, int64_t k,
                                 int attempt, uint64_t *bound) {
  if (num_keys < 1 || num_tuples < 0 || (num_tuples > 0 && !tuples) || total_rows < 0 || attempt < 0 || !bound)
    return SQLRS_ERR_INTERNAL;
  const int tw = range_tuple_words(num_keys);
  if (k <= 0) { // keeps nothing
    std::fill(bound, bound + tw, 0ull);
    return SQLRS_OK;
  }
  const int64_t j = (k >= total_rows || num_tuples == 0) ? -1 : range_bound_index(num_tuples, total_rows, k, attempt);
  if (j < 0) { // keeps every row: a row tuple's validity words are 0 / 1
    std::fill(bound, bound + tw, ~0ull);
    return SQLRS_OK;
  }
  try {
    std::vector<int64_t> idx((size_t)num_tuples);
    std::iota(idx.begin(), idx.end(), (int64_t)0);
    std::nth_element(idx.begin(), idx.begin() + j, idx.end(),
                     [&](int64_t a, int64_t b) { return tuple_less(tuples + a * tw, tuples + b * tw, tw); });
    const uint64_t *src = tuples + idx[(size_t)j] * tw;
    std::copy(src, src + tw, bound);
  } catch (const std::exception &) {
    return SQLRS_ERR_INTERNAL;
  }
  return SQLRS_OK;
}

extern "C" int sqlrs_range_select(sqlrs_ctx_t *ctx, const sqlrs_batch_t *in, int num_keys, const sqlrs_order_by_t *order_by,
                                  int64_t row_base, const uint64_t *bound, int out_mem, sqlrs_batch_t **out) {
  if (!ctx) return SQLRS_ERR_INTERNAL;
  return guard(ctx, [&] {
    SQ_HIP(hipSetDevice(ctx->device));
    RangeKeys rk = range_keys(num_keys, order_by, "range select");
    if (row_base < 0) fail(SQLRS_ERR_INTERNAL, "range select: row_base must be >= 0");
    if (!in || !bound || !out) fail(SQLRS_ERR_INTERNAL, "range select: null pointer");
    InBatch ib(ctx, in);
    const int64_t n = ib.rows();
    const int nc = ib.num_columns();
    const int tw = range_tuple_words(num_keys);
    std::vector<DCol> keys = range_eval_keys(ctx, ib, rk, "range select");
    Selection s;
    s.rows = n;
    const int64_t nwords = ceil_div(std::max<int64_t>(n, 1), 64);
    s.own_bits = ctx->alloc(8 * (size_t)nwords);
    s.bits = s.own_bits->as<uint64_t>();
    if (n && num_keys <= RS_MAXK) {
      ProfScope ps(ctx, "range_select");
      RsArgs a{};
      a.nk = num_keys;
      for (int k = 0; k < num_keys; k++) {
        const DCol &c = keys[(size_t)k];
        a.key[k].vals = c.values;
        a.key[k].validity = (c.validity && c.null_count != 0) ? c.validity : nullptr;
        a.key[k].flip = rk.desc[(size_t)k] ? ~0ull : 0ull;
        a.key[k].kind = c.dtype == SQLRS_INT64 ? 0 : c.dtype == SQLRS_FLOAT64 ? 1 : c.dtype == SQLRS_INT32 ? 2 : 3;
        a.bound[2 * k] = bound[2 * k];
        a.bound[2 * k + 1] = bound[2 * k + 1];
      }
      a.pos = bound[tw - 1];
      // the tile offsets from the kernel's per-tile counts: selection_finish's chained look-back over 4096-row tiles
      // took 0.30 ms for 1e8 rows, as long as the mask itself
      const int64_t ntiles = ceil_div(n, TILE_ROWS);
      BufP cnt = ctx->alloc(4 * (size_t)ntiles), total = ctx->alloc(8);
      s.tile_off = ctx->alloc(8 * (size_t)ntiles);
      const unsigned blocks = (unsigned)ceil_div(ntiles, WAVES_PER_BLOCK);
      range_select_mask_kernel<<<dim3(blocks), dim3(BLOCK), 0, ctx->stream>>>(a, n, row_base, nwords, ntiles,
                                                                            s.own_bits->as<uint64_t>(), cnt->as<uint32_t>());
      SQ_HIP(hipGetLastError());
      exclusive_scan_u32(ctx, cnt->as<uint32_t>(), ntiles, s.tile_off->as<uint64_t>(), nullptr, total->as<uint64_t>());
      s.count = (int64_t)ctx->fetch_value(total->as<uint64_t>()); // the one count fetch
    } else {
      if (n) { // more keys than the kernel arguments hold
        ProfScope ps(ctx, "range_select");
        BufP tup = ctx->alloc(8 * (size_t)tw * (size_t)n), dbound = ctx->alloc(8 * (size_t)tw);
        range_tuples_of(ctx, keys, rk, n, n, row_base, tup->as<uint64_t>());
        SQ_HIP(hipMemcpyAsync(dbound->p, bound, 8 * (size_t)tw, hipMemcpyHostToDevice, ctx->stream));
        range_below_kernel<<<dim3((unsigned)ceil_div(n, BLOCK)), dim3(BLOCK), 8 * (size_t)tw, ctx->stream>>>(
            tup->as<uint64_t>(), tw, n, dbound->as<uint64_t>(), s.own_bits->as<uint64_t>());
        SQ_HIP(hipGetLastError());
      }
      selection_finish(ctx, s); // tile offsets + the one count fetch (syncs: the caller's `bound` has been read)
    }
    // the kept rows' ids, then every column gathered by them (what compact_column does for Utf8)
    BufP idx = ctx->alloc(4 * (size_t)std::max<int64_t>(s.count, 1));
    if (s.count) selection_rows_u32(ctx, s.bits, s.tile_off->as<uint64_t>(), n, idx->as<uint32_t>());
    DBatch o;
    o.rows = s.count;
    for (int c = 0; c < nc; c++) o.cols.push_back(gather_column(ctx, ib.col(c), idx->p, false, nullptr, s.count));
    *out = emit_batch(ctx, std::move(o), out_mem);
  });
}
