// join_async.hip — sqlrs_hash_join_probe_push_async: one small HOST probe batch, one launch, no copy call (small_async.hpp).
// The two one-launch probe kernels, what admits a batch to them, and the join's four switches; every other batch goes to the
// synchronous operator in join.hip (hash_join_probe_sync).
#include "common.hpp"
#include "device_utils.hpp"
#include "prims.hpp"
#include "small_async.hpp"
#include "join_table.hpp"
#include "key_hash.hpp"
#include "join_state.hpp"

using namespace sq;

namespace sq {
// ---- one small HOST probe batch, one launch, no copy call (small_async.hpp) ------------------------------------------
// Inner join over unique build keys: one lookup per probe row (the direct-address table or the 16-byte-slot table), the
// rows with a partner compacted in probe-row order (= the reference's pair order, hash_join.rs:225-234), the build
// columns gathered by the build row, the probe columns copied — the joined batch (build_batch, hash_join.rs:25-45)
// written straight into the pinned slot.
struct SaProbeParams {
  SaLayout lay;
  int nleft, key_col, key_is32, dense;
  const void *lvals[SA_MAX_COLS];
  const uint64_t *lvalid[SA_MAX_COLS];
  const Slot *table;
  uint64_t mask;
  DenseTable dt;
  const uint8_t *in;
  uint8_t *out;
  unsigned long long seq;
};
// sqlrs_hash_join_set_async_utf8: the same with Utf8 payload columns on either side (UTF8 = true; batches without one keep the
// instantiation they always had).  Per Utf8 column the Filter's scheme (ops.hip, sa_filter_kernel): the kept rows' lengths by
// output position in LDS, a block exclusive scan that is the output offsets, then the bytes row by row — from the build
// column in HBM (loffs / lvals by the build row) or from the batch's own bytes in the slot.  The column's bytes are compared
// with what the host reserved (SaCol::out_cap) before one of them is stored.
struct SaProbeUtf8Params : SaProbeParams {
  const int32_t *loffs[SA_MAX_COLS]; // build columns: the offsets of a Utf8 column (lvals = its bytes) or null
};
// sqlrs_hash_join_set_async_filter (FILTER = true; joins without a filter keep the instantiations they always had): the join
// filter as a postfix program over the JOINED row, compiled once per join (sa_probe_filter_ready) and read from HBM into LDS
// at kernel start.  The operand loader of sa_eval_row for the joined row {build row, probe row}: a build column comes from HBM
// (NULL when the row has no partner, else the column's 64-bit-word bitmap), a probe column from the slot.
template <class Base> struct SaWithFilter : Base {
  const SaProgram *prog; // HBM
  SaWithFilter() = default;
  SaWithFilter(const Base &b, const SaProgram *pr) : Base(b), prog(pr) {}
};
template <class P> struct SaJoinedLoad {
  const P &p;
  uint32_t r, brow;
  __device__ __forceinline__ unsigned long long operator()(uint32_t c, bool *ok) const {
    if ((int)c >= p.nleft) return SaSlotLoad{p.lay, p.in, r}(c, ok);
    if (brow == DENSE_EMPTY) {
      *ok = false;
      return 0ull;
    }
    const uint64_t *lv = p.lvalid[c];
    *ok = !lv || ((lv[brow >> 6] >> (brow & 63)) & 1);
    return p.lay.c[c].width == 8 ? ((const unsigned long long *)p.lvals[c])[brow] : (unsigned long long)(long long)((const int32_t *)p.lvals[c])[brow];
  }
};
// the program from HBM into LDS (every thread of the workgroup calls it; the caller's next barrier makes it readable)
__device__ __forceinline__ void sa_load_program(const SaProgram *from, unsigned char *s_raw) {
  static_assert(sizeof(SaProgram) % 4 == 0, "copied in words");
  for (uint32_t i = threadIdx.x; i < (uint32_t)(sizeof(SaProgram) / 4); i += blockDim.x) ((uint32_t *)s_raw)[i] = ((const uint32_t *)from)[i];
}
// sqlrs_hash_join_set_async_keys (KEYS = true, only together with UTF8 = true; a batch that needs neither a NULL key nor a hashed
// key keeps the instantiation it always had): the key of a probe row through sa_probe_key.  nkeys = 0, EXACT mode (j->exact: one
// fixed-width key column, key_col): the value as always, and a row whose validity bit is clear is a NULL key — it takes the NULL
// build row(s): table[cap] of the slot table (probe_slot(.., is_null)), dt.null_head of the direct-address table, nothing on
// dd_table (only built without a NULL build key).  nkeys = 1 .. 4, HASH mode (!j->exact: a Utf8 key, or several key columns): the
// u64 normalize_keys (keys.hip) gives the row, by key_hash.hpp's arithmetic over the columns staged in the slot (key column k =
// byte k of key_cols) — a NULL leaves the running hash alone, the tag follows the probe column's own dtype — looked up as a
// value: match-by-hash, the synchronous route's rule and the reference's (hash_join.rs:222-232).
template <class Base> struct SaWithKeys : Base {
  int nkeys;
  uint32_t key_cols;
};
template <bool KEYS, class P> __device__ __forceinline__ uint64_t sa_probe_key(const P &p, const SaCol &kc, uint32_t r, bool *is_null) {
  *is_null = false;
  if constexpr (KEYS) {
    if (p.nkeys) {
      uint64_t acc = 0;
      for (int k = 0; k < p.nkeys; k++) {
        const SaCol &c = p.lay.c[p.nleft + (int)((p.key_cols >> (8 * k)) & 0xffu)];
        if (c.in_voff != SA_NONE && !((p.in[c.in_voff + (r >> 3)] >> (r & 7)) & 1)) continue;
        uint64_t v;
        if (c.dtype == SQLRS_UTF8) { // (the bytes sit at in_data from offsets[0] on)
          const int32_t *off = (const int32_t *)(p.in + c.in_off);
          v = key_hash_utf8(p.in + c.in_data, (int64_t)((uint32_t)off[r] - c.data_base), (int64_t)((uint32_t)off[r + 1] - c.data_base));
        } else if (c.width == 8)
          v = key_hash_fixed(((const uint64_t *)(p.in + c.in_off))[r], KEY_TAG_64);
        else
          v = key_hash_fixed((uint64_t)((const uint32_t *)(p.in + c.in_off))[r], KEY_TAG_32);
        acc = key_fold(v, acc, p.nkeys > 1);
      }
      return acc;
    }
    *is_null = kc.in_voff != SA_NONE && !((p.in[kc.in_voff + (r >> 3)] >> (r & 7)) & 1);
  }
  return p.key_is32 ? (uint64_t)(int64_t)((const int32_t *)(p.in + kc.in_off))[r] : ((const uint64_t *)(p.in + kc.in_off))[r];
}
template <bool UTF8, bool FILTER, bool KEYS> using SaProbeBaseP = std::conditional_t<KEYS, SaWithKeys<SaProbeUtf8Params>, std::conditional_t<UTF8, SaProbeUtf8Params, SaProbeParams>>;
template <bool UTF8, bool FILTER, bool KEYS = false> using SaProbeP = std::conditional_t<FILTER, SaWithFilter<SaProbeBaseP<UTF8, FILTER, KEYS>>, SaProbeBaseP<UTF8, FILTER, KEYS>>;
template <bool UTF8, bool FILTER, bool KEYS = false>
__global__ __launch_bounds__(1024) void sa_probe_kernel(SaGroup<SaProbeP<UTF8, FILTER, KEYS>> grp) {
  static_assert(!KEYS || UTF8, "the key loader is instantiated with the Utf8 kernels only");
  const auto &p = grp.p[blockIdx.x]; // (one workgroup per batch of the group)
  __shared__ uint32_t s_w[17], s_nulls[SA_MAX_COLS];
  __shared__ uint8_t s_v[SA_MAX_ROWS];
  if (threadIdx.x < SA_MAX_COLS) s_nulls[threadIdx.x] = 0;
  [[maybe_unused]] __shared__ __attribute__((aligned(8))) unsigned char s_prog_raw[FILTER ? sizeof(SaProgram) : 8]; // (SaProgram has member initialisers)
  [[maybe_unused]] __shared__ uint32_t s_div0;
  if constexpr (FILTER) {
    sa_load_program(p.prog, s_prog_raw);
    if (threadIdx.x == 0) s_div0 = 0;
    __syncthreads();
  }
  const SaCol &kc = p.lay.c[p.nleft + p.key_col]; // (the first key column)
  uint32_t m[4] = {DENSE_EMPTY, DENSE_EMPTY, DENSE_EMPTY, DENSE_EMPTY}, pos[4], total;
  const uint32_t bits = sa_positions(
      p.lay.rows,
      [&](uint32_t r, int t) {
        bool is_null;
        const uint64_t key = sa_probe_key<KEYS>(p, kc, r, &is_null);
        uint32_t h = DENSE_EMPTY;
        if (p.dense) {
          const uint64_t d = key - p.dt.kmin;
          if (KEYS && is_null) h = p.dt.null_head;
          else h = dense_get(p.dt, d < p.dt.range ? d : p.dt.range + 1);
        } else {
          const Slot sl = probe_slot(p.table, p.mask, key, KEYS && is_null);
          if (sl.count) h = sl.head;
        }
        if constexpr (FILTER) {
          if (h != DENSE_EMPTY) { // a candidate pair: kept iff the filter is valid and TRUE on the joined row (a NULL drops it)
            bool valid, div0 = false;
            const unsigned long long v = sa_eval_row(*(const SaProgram *)s_prog_raw, SaJoinedLoad<SaProbeP<UTF8, FILTER, KEYS>>{p, r, h}, &valid, &div0);
            if (div0) s_div0 = 1u;
            if (!(valid && v != 0)) h = DENSE_EMPTY;
          }
        }
        m[t] = h;
        return h != DENSE_EMPTY;
      },
      pos, s_w, &total);
  [[maybe_unused]] bool failed = false;
  for (int c = 0; c < p.lay.ncols; c++) {
    const SaCol &col = p.lay.c[c];
    const bool left = c < p.nleft;
    const uint8_t *rvalid = !left && col.in_voff != SA_NONE ? p.in + col.in_voff : nullptr;
    const uint64_t *lvalid = left ? p.lvalid[c] : nullptr;
    const uint8_t *src = left ? (const uint8_t *)p.lvals[c] : p.in + col.in_off;
    if constexpr (UTF8) {
      if (col.dtype == SQLRS_UTF8) { // (uniform: the layout is a kernel argument)
        __shared__ uint32_t s_len[SA_MAX_ROWS + 4]; // lengths of the kept rows in output order, then their exclusive prefix
        const int32_t *off = left ? p.loffs[c] : (const int32_t *)(p.in + col.in_off);
        int32_t *ooff = (int32_t *)(p.out + col.out_off);
#pragma unroll
        for (int t = 0; t < 4; t++) {
          if (!((bits >> t) & 1)) continue;
          const uint32_t r = left ? m[t] : (uint32_t)t * 1024u + threadIdx.x;
          s_len[pos[t]] = (uint32_t)(off[r + 1] - off[r]);
          if (lvalid) s_v[pos[t]] = (uint8_t)((lvalid[r >> 6] >> (r & 63)) & 1);
          else if (rvalid) s_v[pos[t]] = (rvalid[r >> 3] >> (r & 7)) & 1;
        }
        __syncthreads();
        { // thread i owns entries 4 i .. 4 i + 3 of the (<= 4096) lengths
          uint32_t a[4], sum = 0;
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const uint32_t i = threadIdx.x * 4 + q;
            a[q] = i < total ? s_len[i] : 0u;
            sum += a[q];
          }
          const uint32_t inc = wave_iscan_u32(sum);
          if (lane_id() == 63) s_w[wave_id()] = inc;
          __syncthreads();
          uint32_t base = inc - sum, all = 0;
#pragma unroll
          for (int q = 0; q < 16; q++) {
            const uint32_t wsum = s_w[q];
            base += q < wave_id() ? wsum : 0;
            all += wsum;
          }
          failed = all > col.out_cap; // (uniform; cannot happen while the host's reservation is right)
          if (!failed) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
              const uint32_t i = threadIdx.x * 4 + q;
              if (i <= total) { // (entry `total` = the end of the last string)
                s_len[i] = base;
                ooff[i] = (int32_t)base;
              }
              base += a[q];
            }
            if (total == SA_MAX_ROWS && threadIdx.x == 1023) ooff[SA_MAX_ROWS] = (int32_t)base; // (a full batch kept whole: its end offset has no owner above)
          }
        }
        __syncthreads();
        if (failed) break; // (nothing of this column's bytes is stored, zero rows are published, the wait reports it)
        const uint8_t *bytes = left ? (const uint8_t *)p.lvals[c] : p.in + col.in_data;
        const uint32_t data_base = left ? 0u : col.data_base;
#pragma unroll
        for (int t = 0; t < 4; t++) {
          if (!((bits >> t) & 1)) continue;
          const uint32_t r = left ? m[t] : (uint32_t)t * 1024u + threadIdx.x;
          const uint32_t beg = (uint32_t)off[r], len = (uint32_t)off[r + 1] - beg;
          const uint8_t *from = bytes + (beg - data_base);
          uint8_t *dst = p.out + col.out_data + s_len[pos[t]];
          for (uint32_t b = 0; b < len; b++) dst[b] = from[b];
        }
        if (lvalid || rvalid) sa_pack_validity(s_v, total, p.out + col.out_voff, &s_nulls[c]);
        else __syncthreads(); // (s_len is reused by the next Utf8 column)
        continue;
      }
    }
#pragma unroll
    for (int t = 0; t < 4; t++) {
      if (!((bits >> t) & 1)) continue;
      const uint32_t r = left ? m[t] : (uint32_t)t * 1024u + threadIdx.x;
      if (col.width == 8) ((uint64_t *)(p.out + col.out_off))[pos[t]] = ((const uint64_t *)src)[r];
      else ((uint32_t *)(p.out + col.out_off))[pos[t]] = ((const uint32_t *)src)[r];
      if (lvalid) s_v[pos[t]] = (uint8_t)((lvalid[r >> 6] >> (r & 63)) & 1);
      else if (rvalid) s_v[pos[t]] = (rvalid[r >> 3] >> (r & 7)) & 1;
    }
    if (lvalid || rvalid) sa_pack_validity(s_v, total, p.out + col.out_voff, &s_nulls[c]);
  }
  if constexpr (UTF8 && FILTER) { // (s_div0: every keep_of ran in front of sa_positions' barriers; 1 = the evaluator's error at the wait)
    __shared__ uint32_t s_err;
    if (threadIdx.x == 0) s_err = failed ? 2u : s_div0;
    sa_publish((SaHeader *)p.out, p.seq, failed ? 0u : total, s_nulls, p.lay.ncols, &s_err);
  } else if constexpr (FILTER) {
    sa_publish((SaHeader *)p.out, p.seq, total, s_nulls, p.lay.ncols, &s_div0);
  } else if constexpr (UTF8) {
    __shared__ uint32_t s_err;
    if (threadIdx.x == 0) s_err = failed ? 2u : 0u;
    sa_publish((SaHeader *)p.out, p.seq, failed ? 0u : total, s_nulls, p.lay.ncols, &s_err);
  } else
    sa_publish((SaHeader *)p.out, p.seq, total, s_nulls, p.lay.ncols);
}
// Lmax of every Utf8 build column: the longest string in bytes, NULL slots included — what one output row can cost at the most
__global__ void sa_utf8_lmax_kernel(const int32_t *__restrict__ off, int64_t n, uint32_t *__restrict__ out) {
  uint32_t m = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    m = max(m, (uint32_t)(off[i + 1] - off[i]));
  for (int s = 32; s >= 1; s >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, s, 64));
  if (lane_id() == 0 && m) atomicMax(out, m);
}
// once per join, when the first batch needs it: one kernel and one fetch per Utf8 build column
static const std::vector<int64_t> &hash_join_utf8_lmax(sqlrs_hash_join *j) {
  if (!j->utf8_lmax_known) {
    Ctx *ctx = j->ctx;
    j->utf8_lmax.assign(j->left.cols.size(), -1);
    for (size_t c = 0; c < j->left.cols.size(); c++) {
      const DCol &lc = j->left.cols[c];
      if (lc.dtype != SQLRS_UTF8) continue;
      const int64_t n = lc.length;
      BufP out = ctx->alloc_zero(8);
      if (n > 0) {
        const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, 256 * 4), 4 * (int64_t)ctx->num_cus));
        sa_utf8_lmax_kernel<<<dim3(blocks), dim3(256), 0, ctx->stream>>>(lc.offsets, n, out->as<uint32_t>());
        SQ_HIP(hipGetLastError());
      }
      j->utf8_lmax[c] = (int64_t)ctx->fetch_value(out->as<uint32_t>());
    }
    j->utf8_lmax_known = true;
  }
  return j->utf8_lmax;
}
// the build columns of a batch for the async kernels: dtypes, and whether they are columns the kernels carry.  *any_utf8: one is Utf8
static bool sa_probe_build_cols(sqlrs_hash_join *j, int32_t *ldt, bool *any_utf8) {
  const int nleft = (int)j->left.cols.size();
  for (int c = 0; c < nleft; c++) {
    const DCol &lc = j->left.cols[(size_t)c];
    if (lc.stride == 0) return false;
    if (lc.dtype == SQLRS_UTF8) {
      if (!j->async_utf8 || !lc.offsets) return false;
      *any_utf8 = true;
    } else if (lc.dtype != SQLRS_INT32 && lc.dtype != SQLRS_INT64 && lc.dtype != SQLRS_FLOAT64)
      return false;
    ldt[c] = lc.dtype;
  }
  return true;
}
static bool sa_batch_has_utf8(const sqlrs_batch_t *b) {
  for (int c = 0; c < b->num_columns; c++)
    if (b->columns[c].dtype == SQLRS_UTF8) return true;
  return false;
}
// bytes to reserve per Utf8 build column for `out_rows` output rows (others 0)
static void sa_probe_front_bytes(sqlrs_hash_join *j, uint64_t out_rows, uint64_t *front_bytes) {
  const std::vector<int64_t> &lmax = hash_join_utf8_lmax(j);
  for (size_t c = 0; c < lmax.size(); c++) front_bytes[c] = lmax[c] > 0 ? out_rows * (uint64_t)lmax[c] : 0;
}
// sqlrs_hash_join_set_async_filter: true = the join's filter runs inside the probe kernels for `right`.  The program is compiled
// once per join over the joined schema — the build side's dtypes, then the right_dtypes of sqlrs_hash_join_create — with
// sa_compile's rule (<= SA_PROG_MAX nodes, stack <= SA_STACK_MAX, int32 / int64 / float64 columns, Boolean result); a batch
// whose dtypes are not right_dtypes keeps the synchronous operator
static bool sa_probe_filter_ready(sqlrs_hash_join *j, const sqlrs_batch_t *right) {
  if (!j->has_filter || !j->async_filter || !right) return false;
  if (!j->filter_prog_state) {
    std::vector<int32_t> dt;
    for (const DCol &c : j->left.cols) dt.push_back(c.dtype);
    dt.insert(dt.end(), j->right_dtypes.begin(), j->right_dtypes.end());
    SaProgram prog;
    const bool ok = !j->right_dtypes.empty() && sa_compile(j->filter, dt.data(), (int)dt.size(), &prog) && prog.result_dtype == SQLRS_BOOLEAN;
    if (ok) {
      j->filter_prog_host.assign(sizeof(SaProgram), 0);
      std::memcpy(j->filter_prog_host.data(), &prog, sizeof(SaProgram));
    }
    j->filter_prog_state = ok ? 1 : -1;
  }
  if (j->filter_prog_state != 1 || (size_t)right->num_columns != j->right_dtypes.size()) return false;
  for (int c = 0; c < right->num_columns; c++)
    if (right->columns[c].dtype != j->right_dtypes[(size_t)c]) return false;
  return true;
}
// the program in HBM (uploaded once, on the ctx stream) and, `pairs`: the general kernel's list regions, one per ring slot
// (allocated once, from the ctx pool; freed with the join, whose destruction drains the side streams first).  Called before a
// slot is taken (it may throw) and only by a join's fast batches, so the first batch that is enqueued — the one that orders the
// side streams behind the ctx stream (async_ordered) — comes after the upload
static void sa_probe_filter_device(sqlrs_hash_join *j, bool pairs) {
  Ctx *ctx = j->ctx;
  if (!j->filter_prog) {
    BufP prog = ctx->alloc(sizeof(SaProgram));
    SQ_HIP(hipMemcpyAsync(prog->p, j->filter_prog_host.data(), sizeof(SaProgram), hipMemcpyHostToDevice, ctx->stream));
    j->filter_prog = prog;
  }
  if (pairs && !j->filter_pairs) j->filter_pairs = ctx->alloc((size_t)SA_SLOTS * SA_MAX_OUT_ROWS * sizeof(uint2));
}
// The key columns of `right` for the async kernels; false = the synchronous operator takes the batch.  Without
// sqlrs_hash_join_set_async_keys: ONE exactly compared INPUT_REF key of int32 / int64 / float64 without a NULL in the batch.  With
// it (the header's rule): 1 .. 4 INPUT_REF keys of int32 / int64 / float64 / Utf8 (Utf8: the Utf8 switch as well), NULLs allowed;
// kd->loader = the batch needs sa_probe_key (a NULL key in exact mode, any batch in hash mode).  A batch whose keys the
// synchronous operator refuses (exact on one side only, another exact dtype) stays with it: it raises what there is to raise.
struct SaKeyDesc {
  int key_col = 0, key_is32 = 0, nkeys = 0;
  uint32_t key_cols = 0;
  bool loader = false;
};
static bool sa_probe_keys(sqlrs_hash_join *j, const sqlrs_batch_t *right, SaKeyDesc *kd) {
  const size_t nk = j->rkeys.size();
  if (j->comp.on || !right || nk < 1 || nk != j->lkeys.size() || right->num_columns > SA_MAX_COLS) return false;
  if (!j->async_keys && (!j->exact || nk != 1)) return false;
  if (nk > 4 || (j->exact && nk != 1)) return false;
  bool any_null = false;
  for (size_t k = 0; k < nk; k++) {
    const Expr &e = j->rkeys[k];
    if (e.nodes.size() != 1 || e.nodes[0].op != SQLRS_EXPR_INPUT_REF) return false;
    const int kc = e.nodes[0].index;
    if (kc < 0 || kc >= right->num_columns) return false;
    const sqlrs_column_t &kcol = right->columns[kc];
    const bool fixed = kcol.dtype == SQLRS_INT64 || kcol.dtype == SQLRS_FLOAT64 || kcol.dtype == SQLRS_INT32;
    if (j->exact ? (!fixed || kcol.dtype != j->key_dtype) : !(fixed || (kcol.dtype == SQLRS_UTF8 && j->async_utf8))) return false;
    if (!j->exact && nk == 1 && fixed) return false; // (one fixed-width probe key against a hashed build key: the operator's error)
    any_null |= kcol.validity && kcol.null_count != 0;
    kd->key_cols |= (uint32_t)kc << (8 * k);
    if (k == 0) {
      kd->key_col = kc;
      kd->key_is32 = kcol.dtype == SQLRS_INT32;
    }
  }
  if (j->exact && any_null && !j->async_keys) return false; // (NULL probe keys match NULL build keys: the key loader)
  kd->nkeys = j->exact ? 0 : (int)nk;
  kd->loader = !j->exact || any_null;
  return true;
}
// ---- admission: what sa_probe_try and sa_probe_general_try (below) share -------------------------------------------------------
// The checks both kernels' batches pass first, in this order; false = not a fast batch.  Leaves the join's table resolved
// (dense_resolve, hash_join_ensure_table: either may throw, no slot is taken yet).
struct SaProbeBatch {
  SaKeyDesc kd;
  bool filt = false, utf8 = false; // the join's filter runs in the kernel; a Utf8 payload column on either side
  int nleft = 0;
  int32_t ldt[SA_MAX_COLS]; // the build columns' dtypes
};
static bool sa_probe_prelude(sqlrs_hash_join *j, const sqlrs_batch_t *right, SaProbeBatch *b) {
  if (!sa_probe_keys(j, right, &b->kd)) return false;
  b->filt = sa_probe_filter_ready(j, right);
  if (j->has_filter && !b->filt) return false;
  b->nleft = (int)j->left.cols.size();
  if (b->nleft + right->num_columns > SA_MAX_COLS) return false;
  if (!sa_probe_build_cols(j, b->ldt, &b->utf8)) return false;
  if (j->async_utf8 && !b->utf8) b->utf8 = sa_batch_has_utf8(right);
  dense_resolve(j);
  if (!j->dense) hash_join_ensure_table(j); // (a build side that established itself on the LDS route has its table built here)
  return true;
}
// Takes a slot, stages `right` in it (output laid out for `out_rows` rows, SA_NONE: the batch's own) and fills the fields both
// kernels' parameters carry; the slot, or -1 = not a fast batch (no slot is held).  Everything of the admission that can throw
// comes before this call, except sa_order_after_ctx behind the slot (ADVICE.md's open item).
template <class P>
static int sa_probe_fill(P &p, sqlrs_hash_join *j, SaRing *r, const sqlrs_batch_t *right, const SaProbeBatch &b, uint32_t out_rows,
                         const uint64_t *front_bytes) {
  const int slot = r ? sa_take_slot(r) : -1;
  if (slot < 0) return -1;
  if (!sa_stage_input(right, r->in_area(slot), &p.lay, b.nleft, b.ldt, b.utf8, out_rows, b.utf8 ? front_bytes : nullptr)) { // (the byte bound: checked before anything is written)
    r->busy[slot] = false;
    return -1;
  }
  p.nleft = b.nleft;
  p.key_col = b.kd.key_col;
  p.key_is32 = b.kd.key_is32;
  p.nkeys = b.kd.nkeys;
  p.key_cols = b.kd.key_cols;
  for (int c = 0; c < SA_MAX_COLS; c++) {
    p.lvals[c] = c < b.nleft ? j->left.cols[(size_t)c].values : nullptr;
    p.lvalid[c] = c < b.nleft && j->left.cols[(size_t)c].has_nulls() ? j->left.cols[(size_t)c].validity : nullptr;
    p.loffs[c] = c < b.nleft && j->left.cols[(size_t)c].dtype == SQLRS_UTF8 ? j->left.cols[(size_t)c].offsets : nullptr;
  }
  p.table = j->table ? j->table->as<Slot>() : nullptr;
  p.mask = j->mask;
  p.dt = dense_table_of(j);
  p.in = r->in_area(slot);
  p.out = r->out_area(slot);
  p.seq = ++r->seq;
  if (!j->async_ordered) { // the table, the build columns and the cleared `visited` (and the filter's program) were queued on the ctx stream: the side streams wait for them, once
    sa_order_after_ctx(j->ctx, r);
    j->async_ordered = true;
  }
  return slot;
}
// Queues the batch for the instantiation <UTF8, FILTER, KEYS> it needs — `p` is the widest parameter block of the family `Fam`
// (its P<..> and launch<..>), sliced to the kernel's own; `filter_args`: what the family's FILTER blocks carry behind the base
// (the program, the general kernel's list region) — and describes the slot in *t.
template <class Fam, class Full, class... FilterArgs>
static void sa_probe_enqueue(sqlrs_hash_join *j, SaRing *r, const Full &p, const SaProbeBatch &b, int slot, sqlrs_ticket *t, FilterArgs... filter_args) {
  const auto enqueue = [&](auto launch, const auto &q) { sa_enqueue(j->ctx, r, j, launch, q, slot); };
  if (b.filt && b.kd.loader) enqueue(Fam::template launch<true, true, true>, typename Fam::template P<true, true, true>(p, filter_args...));
  else if (b.kd.loader) enqueue(Fam::template launch<true, false, true>, p);
  else if (b.filt && b.utf8) enqueue(Fam::template launch<true, true, false>, typename Fam::template P<true, true, false>(p, filter_args...));
  else if (b.filt) enqueue(Fam::template launch<false, true, false>, typename Fam::template P<false, true, false>(p, filter_args...));
  else if (b.utf8) enqueue(Fam::template launch<true, false, false>, (const typename Fam::template P<true, false, false> &)p);
  else enqueue(Fam::template launch<false, false, false>, (const typename Fam::template P<false, false, false> &)p);
  t->slot = slot;
  t->seq = p.seq;
  t->lay = p.lay;
}
struct SaInnerKernels {
  template <bool UTF8, bool FILTER, bool KEYS> using P = SaProbeP<UTF8, FILTER, KEYS>;
  template <bool UTF8, bool FILTER, bool KEYS> static constexpr auto launch = sa_launch_group<P<UTF8, FILTER, KEYS>, sa_probe_kernel<UTF8, FILTER, KEYS>>;
};
// true = sa_probe_kernel was queued for `right` and *t describes its slot
static bool sa_probe_try(sqlrs_hash_join *j, const sqlrs_batch_t *right, sqlrs_ticket *t) {
  SaProbeBatch b;
  if (sa_fast_off() || j->join_type != SQLRS_JOIN_INNER || !sa_probe_prelude(j, right, &b)) return false;
  if (!j->unique || (!j->dense && !j->table)) return false;
  uint64_t front_bytes[SA_MAX_COLS] = {};
  if (b.utf8 && right->num_rows >= 0 && right->num_rows <= (int64_t)SA_MAX_ROWS) sa_probe_front_bytes(j, (uint64_t)right->num_rows, front_bytes);
  if (b.filt) sa_probe_filter_device(j, false); // (may throw: before a slot is taken)
  SaWithKeys<SaProbeUtf8Params> p;
  SaRing *r = sa_ring(j->ctx);
  const int slot = sa_probe_fill(p, j, r, right, b, SA_NONE, front_bytes);
  if (slot < 0) return false;
  p.dense = j->dense ? 1 : 0;
  sa_probe_enqueue<SaInnerKernels>(j, r, p, b, slot, t, b.filt ? j->filter_prog->as<SaProgram>() : nullptr);
  return true;
}

// ---- the same for Left / Right / Full joins and build sides with duplicate keys (sqlrs_hash_join_set_async_general) -------------
// A probe row emits as many joined rows as its key has build rows (Right / Full: one when it has none, hash_join.rs:241-246), so
// the batch is not compacted but EXPANDED: every probe row is looked up once ({run start, rows}: the direct-address table, the
// 16-byte-slot table, or dd_table), the emit counts are scanned over the batch in row order (wave scans + one LDS step per 1024
// rows), and then one thread per OUTPUT row finds its probe row by binary search in the scanned offsets (LDS) — stores stay
// coalesced and a hot key does not serialise one thread.  Output row o of probe row r is build row rows_by_slot[start_r + o -
// off_r]: probe-row major, build insertion order minor, the reference's pair order (hash_join.rs:225-234) and that of
// join_fill_expand_kernel.  A wave's 64 consecutive output rows are one aligned 8-byte word of a column's validity bitmap: the
// bitmaps are the waves' ballots (no per-row flags in LDS, no pack pass).  Left / Full: the matched build rows are marked in
// `visited` (mark_bits_kernel's form) — sqlrs_hash_join_finish drains the side streams before it reads them.
// Static LDS: 2 x 16 KiB (offsets, run starts) + 116 bytes.  The host admits a batch only when rows x M fits `cap`.
struct SaProbeGenParams {
  SaLayout lay;
  int nleft, key_col, key_is32;
  int mode; // 0: direct-address table (unique keys), 1: 16-byte-slot table, 2: dd_table (duplicate keys over a dense range)
  int unique, outer_right, mark;
  uint32_t cap; // output rows the slot is laid out for
  const void *lvals[SA_MAX_COLS];
  const uint64_t *lvalid[SA_MAX_COLS];
  const Slot *table;
  uint64_t mask;
  DenseTable dt;
  const uint32_t *dd;
  uint64_t dup_min, dup_range;
  const uint32_t *rows_by_slot;
  unsigned long long *visited;
  const uint8_t *in;
  uint8_t *out;
  unsigned long long seq;
};
// sqlrs_hash_join_set_async_utf8 (UTF8 = true; batches without a Utf8 column keep the instantiation they always had): inside a
// 1024-row chunk of output every thread takes its row's length per Utf8 column (a build column: of the build row, 0 for a row
// without partner; a probe column: of the probe row), a wave scan and the 16 wave totals in s_w give the chunk-local offsets, a
// running byte base per column (s_ubase, LDS) carries across chunks; the chunk's bytes are compared with what the host
// reserved (SaCol::out_cap) before one of them is stored.
struct SaProbeGenUtf8Params : SaProbeGenParams {
  const int32_t *loffs[SA_MAX_COLS]; // build columns: the offsets of a Utf8 column (lvals = its bytes) or null
};
// sqlrs_hash_join_set_async_filter (FILTER = true; joins without a filter keep the instantiations they always had) — the join
// filter with apply_join_filter's semantics (hash_join.rs:47-127), two phases inside the one launch.  Phase A walks the
// CANDIDATES — the rows the kernel would emit without a filter, Right / Full: a (NULL, r) row per probe row without partner
// included — one thread each, evaluates the program on the joined row and compacts the kept ones stably (ballot + mbcnt + a
// running base across the 1024-candidate chunks) into a list of {probe row, build row | DENSE_EMPTY} in HBM (`pairs`: a region
// per ring slot; 16384 x 8 bytes do not fit LDS next to s_off / s_start), setting a bit per probe row that kept a candidate
// (s_kept, LDS); Right / Full: the probe rows whose bit stayed clear are appended as {r, DENSE_EMPTY}, ascending.  Phase B is
// the emit loop over the list instead of the search.  A workgroup's writes of phase A are ordered before its reads of phase B
// by the barrier between them.  `visited` is marked in phase B only: by kept pairs, and not at all when a valid candidate
// divided by zero (the batch's wait raises the evaluator's error, SaHeader::pad = 1).
template <class Base> struct SaGenWithFilter : Base {
  const SaProgram *prog; // HBM
  uint2 *pairs;          // HBM: room for `cap` entries
  SaGenWithFilter() = default;
  SaGenWithFilter(const Base &b, const SaProgram *pr, uint2 *pl) : Base(b), prog(pr), pairs(pl) {}
};
// sqlrs_hash_join_set_async_keys (KEYS = true): sa_probe_key, as in sa_probe_kernel
template <bool UTF8, bool FILTER, bool KEYS> using SaProbeGenBaseP = std::conditional_t<KEYS, SaWithKeys<SaProbeGenUtf8Params>, std::conditional_t<UTF8, SaProbeGenUtf8Params, SaProbeGenParams>>;
template <bool UTF8, bool FILTER, bool KEYS = false> using SaProbeGenP = std::conditional_t<FILTER, SaGenWithFilter<SaProbeGenBaseP<UTF8, FILTER, KEYS>>, SaProbeGenBaseP<UTF8, FILTER, KEYS>>;
template <bool UTF8, bool FILTER, bool KEYS = false>
__global__ __launch_bounds__(1024) void sa_probe_general_kernel(SaGroup<SaProbeGenP<UTF8, FILTER, KEYS>> grp) {
  static_assert(!KEYS || UTF8, "the key loader is instantiated with the Utf8 kernels only");
  const auto &p = grp.p[blockIdx.x]; // (one workgroup per batch of the group)
  __shared__ uint32_t s_off[SA_MAX_ROWS], s_start[SA_MAX_ROWS]; // per probe row: first output row; run start / build row / DENSE_EMPTY
  __shared__ uint32_t s_w[16], s_nulls[SA_MAX_COLS], s_err;
  [[maybe_unused]] __shared__ uint32_t s_ubase[SA_MAX_COLS]; // Utf8: bytes of the column emitted by the chunks so far
  [[maybe_unused]] __shared__ __attribute__((aligned(8))) unsigned char s_prog_raw[FILTER ? sizeof(SaProgram) : 8]; // (SaProgram has member initialisers)
  [[maybe_unused]] __shared__ uint32_t s_kept[FILTER ? SA_MAX_ROWS / 32 : 1], s_div0; // FILTER: bit r = probe row r has a kept candidate
  [[maybe_unused]] bool failed = false;
  const int lane = lane_id(), w = wave_id();
  if (threadIdx.x < SA_MAX_COLS) s_nulls[threadIdx.x] = 0;
  if constexpr (UTF8)
    if (threadIdx.x < SA_MAX_COLS) s_ubase[threadIdx.x] = 0;
  if (threadIdx.x == 0) s_err = 0;
  if constexpr (FILTER) { // (the lookup loop below has barriers: all of this is in place before phase A)
    sa_load_program(p.prog, s_prog_raw);
    if (threadIdx.x < SA_MAX_ROWS / 32) s_kept[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_div0 = 0;
  }
  const uint32_t rows = p.lay.rows;
  const SaCol &kc = p.lay.c[p.nleft + p.key_col]; // (the first key column)
  uint32_t base = 0;
  for (uint32_t t = 0; t * 1024u < rows; t++) { // (uniform)
    const uint32_t r = t * 1024u + threadIdx.x;
    uint32_t e = 0, start = DENSE_EMPTY;
    if (r < rows) {
      bool is_null;
      const uint64_t key = sa_probe_key<KEYS>(p, kc, r, &is_null);
      uint32_t cnt = 0;
      if (p.mode == 0) {
        const uint64_t d = key - p.dt.kmin;
        if (KEYS && is_null) start = p.dt.null_head;
        else start = dense_get(p.dt, d < p.dt.range ? d : p.dt.range + 1);
        cnt = start != DENSE_EMPTY;
      } else if (p.mode == 1) {
        const Slot sl = probe_slot(p.table, p.mask, key, KEYS && is_null);
        start = sl.head;
        cnt = sl.count;
      } else if (KEYS && is_null) { // (dd_table is only built without a NULL build key: no partner)
        cnt = 0;
      } else {
        const uint64_t d = key - p.dup_min;
        const uint32_t *en = p.dd + (d < p.dup_range ? d : p.dup_range + 1); // (a key outside the range reads the empty run behind it)
        start = en[0];
        cnt = en[1] - start;
      }
      if (!cnt) start = DENSE_EMPTY;
      e = cnt ? cnt : (uint32_t)p.outer_right;
    }
    const uint32_t inc = wave_iscan_u32(e);
    uint32_t before, all;
    sa_block_prefix(s_w, lane == 63, inc, &before, &all);
    if (r < rows) {
      s_off[r] = base + before + inc - e;
      s_start[r] = start;
    }
    base += all;
    __syncthreads();
  }
  uint32_t total = base;
  if (total > p.cap) { // (cannot happen while the host's M is right: nothing is written past the slot, the wait reports it)
    total = 0;
    if (threadIdx.x == 0) s_err = 2;
  }
  if constexpr (FILTER) {
    __syncthreads(); // (rows = 0: the loop above had no barrier)
    const SaProgram &prog = *(const SaProgram *)s_prog_raw;
    uint32_t kbase = 0; // entries of the list so far
    for (uint32_t o0 = 0; o0 < total; o0 += 1024u) { // phase A (uniform): candidate o of the batch
      const uint32_t o = o0 + threadIdx.x;
      uint32_t r = 0, brow = DENSE_EMPTY;
      bool keep = false;
      if (o < total) {
        r = sa_output_row(s_off, rows, o); // (candidate o)
        const uint32_t st = s_start[r];
        if (st != DENSE_EMPTY) brow = p.unique ? st : p.rows_by_slot[st + (o - s_off[r])];
        bool valid, div0 = false;
        const unsigned long long v = sa_eval_row(prog, SaJoinedLoad<SaProbeGenP<UTF8, FILTER, KEYS>>{p, r, brow}, &valid, &div0);
        if (div0) s_div0 = 1u;
        keep = valid && v != 0;
      }
      const uint64_t bm = __ballot(keep);
      uint32_t before, all;
      sa_block_prefix(s_w, lane == 0, (uint32_t)__popcll(bm), &before, &all);
      if (keep) { // (kbase + all <= o0 + 1024, at most `total` <= cap: inside the slot's region)
        p.pairs[kbase + before + mbcnt(bm)] = make_uint2(r, brow);
        atomicOr(&s_kept[r >> 5], 1u << (r & 31));
      }
      kbase += all;
      __syncthreads();
    }
    if (p.outer_right) // the probe rows that kept no candidate come back as (NULL, r) behind the kept ones, in row order (:73-121)
      for (uint32_t t = 0; t * 1024u < rows; t++) { // (uniform)
        const uint32_t r = t * 1024u + threadIdx.x;
        const bool lost = total && r < rows && !((s_kept[r >> 5] >> (r & 31)) & 1); // (total = 0 with rows > 0: the slot was too small, nothing is written)
        const uint64_t bm = __ballot(lost);
        uint32_t before, all;
        sa_block_prefix(s_w, lane == 0, (uint32_t)__popcll(bm), &before, &all);
        if (lost) p.pairs[kbase + before + mbcnt(bm)] = make_uint2(r, DENSE_EMPTY); // (a row that lost all <= one candidate each: the list stays <= total)
        kbase += all;
        __syncthreads();
      }
    total = s_div0 ? 0u : kbase; // (uniform: every write of s_div0 and of the list has a barrier behind it) a division by zero emits and marks nothing
  }
  for (uint32_t o0 = 0; o0 < total; o0 += 1024u) { // (uniform)
    const uint32_t o = o0 + threadIdx.x;
    const bool act = o < total;
    uint32_t r = 0, brow = DENSE_EMPTY;
    if constexpr (FILTER) {
      if (act) {
        const uint2 pr = p.pairs[o];
        r = pr.x;
        brow = pr.y;
      }
    }
    if (act) {
      if constexpr (!FILTER) {
        r = sa_output_row(s_off, rows, o);
        const uint32_t st = s_start[r];
        if (st != DENSE_EMPTY) brow = p.unique ? st : p.rows_by_slot[st + (o - s_off[r])];
      }
      if (p.mark && brow != DENSE_EMPTY) { // (bits only ever get set: a plain read decides whether the atomic is needed, mark_bits_kernel)
        const unsigned long long bit = 1ull << (brow & 63);
        if (!(__hip_atomic_load(&p.visited[brow >> 6], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(&p.visited[brow >> 6], bit);
      }
    }
    const uint64_t actm = __ballot(act);
    for (int c = 0; c < p.lay.ncols; c++) {
      const SaCol &col = p.lay.c[c];
      const bool left = c < p.nleft;
      const uint8_t *rvalid = !left && col.in_voff != SA_NONE ? p.in + col.in_voff : nullptr;
      const uint64_t *lvalid = left ? p.lvalid[c] : nullptr;
      const uint8_t *src = left ? (const uint8_t *)p.lvals[c] : p.in + col.in_off;
      bool valid = true;
      bool is_utf8 = false;
      if constexpr (UTF8) is_utf8 = col.dtype == SQLRS_UTF8; // (uniform: the layout is a kernel argument)
      if constexpr (UTF8) {
        if (is_utf8) {
          const int32_t *off = left ? p.loffs[c] : (const int32_t *)(p.in + col.in_off);
          const uint32_t s = left ? brow : r;
          valid = !act || s != DENSE_EMPTY; // (a probe row without partner: NULL and no bytes in every build column)
          uint32_t beg = 0, len = 0;
          if (act && valid) {
            beg = (uint32_t)off[s];
            len = (uint32_t)off[s + 1] - beg;
          }
          const uint32_t inc = wave_iscan_u32(len);
          uint32_t before, all;
          sa_block_prefix(s_w, lane == 63, inc, &before, &all);
          const uint32_t cbase = s_ubase[c];
          failed = all > col.out_cap || cbase > col.out_cap - all; // (uniform; cannot happen while the host's reservation is right)
          if (act && !failed) {
            const uint32_t at = cbase + before + inc - len;
            ((int32_t *)(p.out + col.out_off))[o] = (int32_t)at;
            const uint8_t *from = left ? (const uint8_t *)p.lvals[c] + beg : p.in + col.in_data + (beg - col.data_base);
            uint8_t *dst = p.out + col.out_data + at;
            for (uint32_t b = 0; b < len; b++) dst[b] = from[b];
          }
          __syncthreads(); // (s_w and s_ubase[c] have been read by everyone: the next column / chunk may write them)
          if (threadIdx.x == 0) s_ubase[c] = cbase + all;
          if (failed) break; // (nothing of this chunk's bytes was stored; zero rows are published, the wait reports it)
          if (act && valid) {
            if (lvalid) valid = (lvalid[s >> 6] >> (s & 63)) & 1;
            else if (rvalid) valid = (rvalid[s >> 3] >> (s & 7)) & 1;
          }
        }
      }
      if (act && !is_utf8) {
        const uint32_t s = left ? brow : r;
        valid = s != DENSE_EMPTY; // (a probe row without partner: NULL in every build column)
        if (col.width == 8) ((uint64_t *)(p.out + col.out_off))[o] = valid ? ((const uint64_t *)src)[s] : 0ull;
        else ((uint32_t *)(p.out + col.out_off))[o] = valid ? ((const uint32_t *)src)[s] : 0u;
        if (valid && lvalid) valid = (lvalid[s >> 6] >> (s & 63)) & 1;
        else if (rvalid) valid = (rvalid[s >> 3] >> (s & 7)) & 1;
      }
      if (lvalid || rvalid || (left && p.outer_right)) { // (uniform) the column may hold NULLs: 64 output rows = one word of its bitmap
        const uint64_t bm = __ballot(act && valid);
        if (lane == 0 && actm) {
          *(uint64_t *)(p.out + col.out_voff + ((o0 + 64u * (uint32_t)w) >> 3)) = bm;
          const uint32_t nulls = (uint32_t)__popcll(actm & ~bm);
          if (nulls) atomicAdd(&s_nulls[c], nulls);
        }
      }
    }
    if constexpr (UTF8)
      if (failed) break;
  }
  if constexpr (UTF8) {
    __syncthreads();
    if (failed) {
      total = 0;
      if (threadIdx.x == 0) s_err = 2;
    }
    if (threadIdx.x == 0) // the end of the last string (zero rows: the one offset there is)
      for (int c = 0; c < p.lay.ncols; c++)
        if (p.lay.c[c].dtype == SQLRS_UTF8) ((int32_t *)(p.out + p.lay.c[c].out_off))[total] = (int32_t)(failed ? 0u : s_ubase[c]);
  }
  if constexpr (FILTER)
    if (threadIdx.x == 0 && s_div0 && !s_err) s_err = 1; // (thread 0 reads both behind phase A's last barrier; sa_publish reads s_err behind its own)
  sa_publish((SaHeader *)p.out, p.seq, total, s_nulls, p.lay.ncols, &s_err);
}
// M: the most build rows that share one key — the largest Slot.count of the 16-byte-slot table (its NULL-key slot included) or
// the longest run of dd_table
__global__ void sa_max_run_kernel(const Slot *__restrict__ table, const uint32_t *__restrict__ dd, int64_t n, uint32_t *__restrict__ out) {
  uint32_t m = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    m = max(m, table ? table[i].count : dd[i + 1] - dd[i]);
  for (int s = 32; s >= 1; s >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, s, 64));
  if (lane_id() == 0 && m) atomicMax(out, m);
}
// once per join, on first need: unique build keys need no kernel
static uint32_t hash_join_max_run(sqlrs_hash_join *j) {
  if (j->unique) return 1;
  if (!j->max_run) {
    Ctx *ctx = j->ctx;
    const int64_t n = j->dd_table ? (int64_t)j->dup_range : (int64_t)j->mask + 3; // (dd_table[range] = rows ends the last run; cap + 2 slots)
    BufP out = ctx->alloc_zero(8);
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, 256 * 4), 4 * (int64_t)ctx->num_cus));
    sa_max_run_kernel<<<dim3(blocks), dim3(256), 0, ctx->stream>>>(j->dd_table ? nullptr : j->table->as<Slot>(),
                                                                  j->dd_table ? j->dd_table->as<uint32_t>() : nullptr, n, out->as<uint32_t>());
    SQ_HIP(hipGetLastError());
    j->max_run = std::max(1u, ctx->fetch_value(out->as<uint32_t>()));
  }
  return j->max_run;
}
struct SaGeneralKernels {
  template <bool UTF8, bool FILTER, bool KEYS> using P = SaProbeGenP<UTF8, FILTER, KEYS>;
  template <bool UTF8, bool FILTER, bool KEYS>
  static constexpr auto launch = sa_launch_group<P<UTF8, FILTER, KEYS>, sa_probe_general_kernel<UTF8, FILTER, KEYS>>;
};
// true = sa_probe_general_kernel was queued for `right` and *t describes its slot.  The rule is the header's
// (sqlrs_hash_join_set_async_general): sa_probe_try's conditions without "Inner" and "unique build keys", plus the output bound.
static bool sa_probe_general_try(sqlrs_hash_join *j, const sqlrs_batch_t *right, sqlrs_ticket *t) {
  SaProbeBatch b;
  if (!j->async_general || sa_fast_off()) return false;
  if (!right || right->num_rows < 0 || right->num_rows > (int64_t)SA_MAX_ROWS || !sa_probe_prelude(j, right, &b)) return false;
  if (j->unique && j->join_type == SQLRS_JOIN_INNER) return false; // (sa_probe_kernel's own: it declined for a reason that holds here too)
  const int mode = j->dense ? 0 : (j->dd_table ? 2 : 1);
  if (mode == 1 && !j->table) return false;
  if (!j->unique && !j->rows_by_slot) return false;
  const uint64_t out_rows = (uint64_t)right->num_rows * hash_join_max_run(j);
  if (out_rows > SA_MAX_OUT_ROWS) return false;
  uint64_t front_bytes[SA_MAX_COLS] = {};
  if (b.utf8) sa_probe_front_bytes(j, out_rows, front_bytes);
  if (b.filt) sa_probe_filter_device(j, true); // (may throw: before a slot is taken)
  SaWithKeys<SaProbeGenUtf8Params> p;
  SaRing *r = sa_ring(j->ctx);
  const int slot = sa_probe_fill(p, j, r, right, b, (uint32_t)out_rows, front_bytes);
  if (slot < 0) return false;
  p.mode = mode;
  p.unique = j->unique ? 1 : 0;
  p.outer_right = (j->join_type == SQLRS_JOIN_RIGHT || j->join_type == SQLRS_JOIN_FULL) ? 1 : 0;
  p.mark = (j->join_type == SQLRS_JOIN_LEFT || j->join_type == SQLRS_JOIN_FULL) ? 1 : 0;
  p.cap = (uint32_t)out_rows;
  p.dd = j->dd_table ? j->dd_table->as<uint32_t>() : nullptr;
  p.dup_min = j->dup_min;
  p.dup_range = j->dup_range;
  p.rows_by_slot = j->rows_by_slot ? j->rows_by_slot->as<uint32_t>() : nullptr;
  p.visited = p.mark ? j->visited->as<unsigned long long>() : nullptr;
  sa_probe_enqueue<SaGeneralKernels>(j, r, p, b, slot, t, b.filt ? j->filter_prog->as<SaProgram>() : nullptr,
                                     b.filt ? j->filter_pairs->as<uint2>() + (size_t)slot * SA_MAX_OUT_ROWS : nullptr); // (a slot is reused only after its ticket was waited for)
  return true;
}
} // namespace sq

static int sa_probe_set(sqlrs_hash_join_t *j, bool sqlrs_hash_join::*sw, int on, const char *name) {
  if (!j) return SQLRS_ERR_INTERNAL;
  return guard(j->ctx, [&] {
    if (j->probe_started) fail(SQLRS_ERR_INTERNAL, std::string(name) + ": after the first probe call");
    j->*sw = on != 0;
  });
}

extern "C" {
// sqlrs_hash_join_probe_push without the wait (small_async.hpp): *ticket stands for the HOST batch
// sqlrs_hash_join_probe_push(j, right, SQLRS_MEM_HOST, ..) would return — NULL for an empty build side.
int sqlrs_hash_join_probe_push_async(sqlrs_hash_join_t *j, const sqlrs_batch_t *right, sqlrs_ticket_t **ticket) {
  if (ticket) *ticket = nullptr;
  return guard(j->ctx, [&] {
    Ctx *ctx = j->ctx;
    if (!ticket) fail(SQLRS_ERR_INTERNAL, "push_async: null ticket");
    SQ_HIP(hipSetDevice(ctx->device));
    if (!j->finished) fail(SQLRS_ERR_INTERNAL, "probe before build_finish");
    j->probe_started = true;
    auto t = std::unique_ptr<sqlrs_ticket>(new sqlrs_ticket());
    t->ctx = ctx;
    if (!j->empty_build && !sa_probe_try(j, right, t.get()) && !sa_probe_general_try(j, right, t.get())) {
      sa_flush(ctx); // (tickets complete in issue order)
      t->done = hash_join_probe_sync(j, right);
    }
    *ticket = t.release();
  });
}
// The join's four switches (small_async.hpp: what each admits), each before the first probe call of any kind: the general kernel
// (outer joins, duplicate build keys), the join filter inside both kernels, the key loader (NULL probe keys, Utf8 keys, 2 .. 4
// key columns), Utf8 payload columns.
int sqlrs_hash_join_set_async_general(sqlrs_hash_join_t *j, int on) { return sa_probe_set(j, &sqlrs_hash_join::async_general, on, "sqlrs_hash_join_set_async_general"); }
int sqlrs_hash_join_set_async_filter(sqlrs_hash_join_t *j, int on) { return sa_probe_set(j, &sqlrs_hash_join::async_filter, on, "sqlrs_hash_join_set_async_filter"); }
int sqlrs_hash_join_set_async_keys(sqlrs_hash_join_t *j, int on) { return sa_probe_set(j, &sqlrs_hash_join::async_keys, on, "sqlrs_hash_join_set_async_keys"); }
int sqlrs_hash_join_set_async_utf8(sqlrs_hash_join_t *j, int on) { return sa_probe_set(j, &sqlrs_hash_join::async_utf8, on, "sqlrs_hash_join_set_async_utf8"); }
} // extern "C"
