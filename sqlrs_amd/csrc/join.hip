// join.hip — HashJoinExecutor on device (src/executor/join/hash_join.rs:146-323).
//
// Build (left child): integer keys that cover a small range (a dimension table's surrogate keys)
// get a direct-address table heads[key - min] = row, verified to be duplicate-free; anything
// else an open-addressing table in HBM, 16-byte slots {key, head, count}, linear probing, slots
// claimed with one 64-bit CAS on the key.  Unique build keys (the PK-FK case) store the build
// row directly; otherwise rows of one key are laid out CSR-style in insertion order (stable
// radix sort by slot), which is what makes the output pair order equal to the reference's
// Vec<usize> per hash (:172-177).
//
// Probe (right child): unique build keys -> one lookup per probe row, hits compacted with ballots
// and a decoupled look-back in a single pass; duplicates -> count matches per probe row ->
// exclusive scan -> fill.  Either way pairs come out probe-row major / build-insertion minor
// exactly like the reference loop (:225-248).
// Algorithmic HBM bytes: 8 B per build row + 8 B per probe row + 12 B per emitted pair.
// The random-access working set is the table: 4 B x key range (direct-address, 4 MiB for 1e6
// keys = one XCD's L2, ~265 G lookups/s) or 16 B x 2 x build rows (hash table, ~56-66 G
// lookups/s once it exceeds the L2; profiles/r01_ubench_mi355x.txt).
#include <cstdlib>

#include "common.hpp"
#include "device_utils.hpp"
#include "prims.hpp"
#include "small_async.hpp"
#include "join_kernels.hpp"
#include "key_hash.hpp"
#include "join_state.hpp"
#include "radix_part.hpp"

#include "join_probe_kernels.hpp" // every kernel of this operator (namespace sq)

using namespace sq;

extern "C" void sqlrs_batch_release(sqlrs_batch_t *batch);

namespace sq {

struct Pairs {
  int64_t m = 0;
  BufP left, right;   // u64[m], u32[m]
  BufP left_validity; // bitmap or null (Right/Full only)
  // pair i = (some build row, probe row i) for EVERY probe row (the all-hit attempt succeeded): the probe side of the
  // joined batch is the probe batch itself, nothing to gather
  bool right_identity = false;
};
// the index pairs as two columns: u64 build rows (NULL where an outer join's probe row has no partner), u32 probe rows
static void pairs_as_columns(const Pairs &p, DCol *l, DCol *r) {
  l->dtype = SQLRS_UINT64;
  l->length = p.m;
  l->values = p.left->p;
  l->own_values = p.left;
  if (p.left_validity) {
    l->validity = p.left_validity->as<uint64_t>();
    l->own_validity = p.left_validity;
    l->null_count = -1;
  }
  r->dtype = SQLRS_UINT32;
  r->length = p.m;
  r->values = p.right->p;
  r->own_values = p.right;
}

static Slot *slots_of(const sqlrs_hash_join *j) { return j->table ? j->table->as<Slot>() : nullptr; }
static bool is_outer_right(const sqlrs_hash_join *j) { return j->join_type == SQLRS_JOIN_RIGHT || j->join_type == SQLRS_JOIN_FULL; }
// (both take the RESULT of hook("SQLRS_..."))
static bool hook_is_zero(const char *e) { return e && std::atoi(e) == 0; }
static int hook_int(const char *e, int unset) { return e ? std::atoi(e) : unset; }

static std::vector<DCol> eval_key_cols(Ctx *ctx, const std::vector<Expr> &exprs, const std::function<const DCol &(int)> &col,
                                       int64_t rows) {
  std::vector<DCol> kc;
  for (const Expr &e : exprs) kc.push_back(eval_expr(ctx, e, col, rows, true));
  return kc;
}
static NKeys eval_keys(Ctx *ctx, const std::vector<Expr> &exprs,
                       const std::function<const DCol &(int)> &col, int64_t rows) {
  return normalize_keys(ctx, eval_key_cols(ctx, exprs, col, rows), rows);
}

// ---- several integer key columns as ONE exact key (sqlrs_hash_join::Composite) ----------------------------------------
// The reference hashes the key columns into 64 bits and matches by hash alone (hash_join.rs:161-232) — and its fold of the
// column hashes collides readily: on a 1000 x 1000 grid of (x, y) build keys, 3e6 probe rows find 3.71e6 partners where
// 2.96e6 exist.  The default of this library reproduces exactly that (normalize_keys, hash mode: same pairs, same order as the
// reference, false matches included).  This is the OPT-IN alternative for callers who want the SQL answer: an exact
// composite key, which also makes dense key grids eligible for the direct-address table and sparse ones for the LDS route.
// NULL in a key column never matches here; the composite is taken only when no build key is NULL, and a probe row with a NULL
// key, a value outside the build side's ranges, or a key column of another integer type gets a key that matches nothing.
// build side: ranges of the key columns over all build batches -> j->comp, and the composite key of every build row
static BufP composite_build_keys(sqlrs_hash_join *j) {
  Ctx *ctx = j->ctx;
  const size_t nk = j->lkeys.size();
  // OPT-IN (SQLRS_JOIN_COMPOSITE=1, read per build): exact equality is NOT what the reference computes — see the note above
  const char *e = std::getenv("SQLRS_JOIN_COMPOSITE");
  if (!e || e[0] != '1') return nullptr;
  if (nk < 2 || nk > 4 || j->lazy_table || j->nB < 1 || j->left_keycol_parts.size() != j->left_batches.size()) return nullptr;
  for (const std::vector<DCol> &part : j->left_keycol_parts) {
    if (part.size() != nk) return nullptr;
    for (size_t c = 0; c < nk; c++) {
      const DCol &k = part[c];
      if ((k.dtype != SQLRS_INT64 && k.dtype != SQLRS_INT32) || k.dtype != j->left_keycol_parts[0][c].dtype || k.stride == 0 ||
          (k.validity && count_nulls(ctx, k) != 0))
        return nullptr;
    }
  }
  BufP mm = ctx->alloc(16 * nk);
  std::vector<long long> init;
  for (size_t c = 0; c < nk; c++) {
    init.push_back(INT64_MAX);
    init.push_back(INT64_MIN);
  }
  SQ_HIP(hipMemcpyAsync(mm->p, init.data(), 16 * nk, hipMemcpyHostToDevice, ctx->stream));
  SQ_HIP(hipStreamSynchronize(ctx->stream)); // (`init` is pageable host memory)
  for (const std::vector<DCol> &part : j->left_keycol_parts)
    for (size_t c = 0; c < nk; c++) {
      const int64_t rows = part[c].length;
      if (rows == 0) continue;
      const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(rows, 256), 4 * (int64_t)ctx->num_cus);
      comp_join_minmax_kernel<<<dim3(blocks), dim3(256), 0, ctx->stream>>>(part[c].values, part[c].dtype == SQLRS_INT32, rows,
                                                                         mm->as<long long>() + 2 * c);
    }
  SQ_HIP(hipGetLastError());
  const long long *h = (const long long *)ctx->fetch(mm->p, 16 * nk);
  sqlrs_hash_join::Composite cp;
  cp.nk = (int)nk;
  unsigned __int128 total = 1;
  for (size_t c = 0; c < nk; c++) {
    if (h[2 * c] > h[2 * c + 1]) return nullptr;
    cp.dtype[c] = j->left_keycol_parts[0][c].dtype;
    cp.min[c] = h[2 * c];
    cp.range[c] = (uint64_t)h[2 * c + 1] - (uint64_t)h[2 * c] + 1; // (0 = all 2^64 values: caught by the product below)
    if (cp.range[c] == 0) return nullptr;
    total *= cp.range[c];
    if (total >= ((unsigned __int128)1 << 62)) return nullptr; // the composite does not fit: hashes
  }
  uint64_t stride = 1;
  for (size_t c = nk; c-- > 0;) {
    cp.stride[c] = stride;
    stride *= cp.range[c];
  }
  cp.on = true;
  j->comp = cp;
  BufP keys = ctx->alloc(8 * (size_t)std::max<int64_t>(j->nB, 1));
  int64_t off = 0;
  ProfScope ps(ctx, "normalize_keys");
  for (const std::vector<DCol> &part : j->left_keycol_parts) {
    const int64_t rows = part[0].length;
    if (rows == 0) continue;
    CompJoinKeys ck{};
    ck.nk = (int)nk;
    for (size_t c = 0; c < nk; c++) {
      ck.vals[c] = part[c].values;
      ck.valid[c] = nullptr;
      ck.min[c] = cp.min[c];
      ck.range[c] = cp.range[c];
      ck.stride[c] = cp.stride[c];
      ck.is32[c] = cp.dtype[c] == SQLRS_INT32;
    }
    comp_join_keys_kernel<<<dim3((unsigned)ceil_div(rows, 256)), dim3(256), 0, ctx->stream>>>(ck, rows, keys->as<uint64_t>() + off);
    off += rows;
  }
  SQ_HIP(hipGetLastError());
  return keys;
}
// probe side: the same composite, the no-match key for rows that cannot have a partner
static NKeys composite_probe_keys(sqlrs_hash_join *j, const std::function<const DCol &(int)> &col, int64_t rows) {
  Ctx *ctx = j->ctx;
  std::vector<DCol> kc = eval_key_cols(ctx, j->rkeys, col, rows);
  NKeys k;
  k.rows = rows;
  k.exact = true;
  k.dtype = SQLRS_INT64;
  k.keys = ctx->alloc(8 * (size_t)std::max<int64_t>(rows, 1));
  if (rows == 0) return k;
  const sqlrs_hash_join::Composite &cp = j->comp;
  CompJoinKeys ck{};
  ck.nk = cp.nk;
  for (int c = 0; c < cp.nk; c++) {
    const DCol &d = kc[(size_t)c];
    if (d.dtype != cp.dtype[c]) ck.nk = -1; // (the reference's hashes differ by type: nothing matches)
    ck.vals[c] = d.values;
    ck.valid[c] = (d.validity && d.null_count != 0) ? d.validity : nullptr;
    ck.min[c] = cp.min[c];
    ck.range[c] = cp.range[c];
    ck.stride[c] = cp.stride[c];
    ck.is32[c] = cp.dtype[c] == SQLRS_INT32;
  }
  ProfScope ps(ctx, "normalize_keys");
  comp_join_keys_kernel<<<dim3((unsigned)ceil_div(rows, 256)), dim3(256), 0, ctx->stream>>>(ck, rows, k.keys->as<uint64_t>());
  SQ_HIP(hipGetLastError());
  return k;
}

// ---- build: key parts -> j->bkeys, j->bkeys_validity (kept for the fused join+aggregate route, hashagg_op.hip), j->exact, j->key_dtype
static void concat_build_keys(sqlrs_hash_join *j) {
  Ctx *ctx = j->ctx;
  int64_t n = j->nB;
  // one build batch (the usual case): its normalised keys ARE the key array, no concat copy
  BufP ckeys = composite_build_keys(j); // several integer key columns: one exact key (or null: as normalised per batch)
  j->left_keycol_parts.clear();
  const bool single = !ckeys && j->left_key_parts.size() == 1 && j->left_key_parts[0].keys && j->left_key_parts[0].keys->owned;
  BufP keys = ckeys ? ckeys : (single ? j->left_key_parts[0].keys : ctx->alloc(8 * (size_t)std::max<int64_t>(n, 1)));
  BufP validity;
  bool any_null = false;
  for (const NKeys &p : j->left_key_parts) any_null |= (p.validity != nullptr);
  j->exact = ckeys ? true : j->left_key_parts[0].exact;
  j->key_dtype = ckeys ? SQLRS_INT64 : j->left_key_parts[0].dtype;
  if (!ckeys) {
    size_t off = 0;
    for (const NKeys &p : j->left_key_parts) {
      if (p.exact != j->exact || p.dtype != j->key_dtype)
        fail(SQLRS_ERR_ARROW, "join key type changed between build batches");
      if (p.rows && !single)
        SQ_HIP(hipMemcpyAsync(keys->as<uint8_t>() + off, p.keys->p, 8 * (size_t)p.rows,
                              hipMemcpyDeviceToDevice, ctx->stream));
      off += 8 * (size_t)p.rows;
    }
    if (any_null) { // reuse the bitmap concat of concat_columns through BOOLEAN pseudo columns
      std::vector<DCol> tmp(j->left_key_parts.size());
      std::vector<const DCol *> ptrs;
      for (size_t i = 0; i < tmp.size(); i++) {
        const NKeys &p = j->left_key_parts[i];
        tmp[i].dtype = SQLRS_INT64;
        tmp[i].length = p.rows;
        tmp[i].values = p.keys->p;
        tmp[i].validity = p.validity;
        tmp[i].null_count = p.validity ? -1 : 0;
        ptrs.push_back(&tmp[i]);
      }
      DCol c = concat_columns(ctx, ptrs);
      if (tmp.size() == 1) {
        validity = j->left_key_parts[0].own_validity;
        if (!validity) { // borrowed bitmap: copy it
          validity = ctx->alloc(bitmap_bytes(n));
          SQ_HIP(hipMemcpyAsync(validity->p, tmp[0].validity, bitmap_bytes(n),
                                hipMemcpyDeviceToDevice, ctx->stream));
        }
      } else
        validity = c.own_validity;
    }
  }
  j->bkeys = keys;
  j->bkeys_validity = validity;
}

static void build_hash_table(sqlrs_hash_join *j);
static bool build_dense_dup(sqlrs_hash_join *j);
// a build side without a direct-address table (not tried, or refused)
static void build_after_refusal(sqlrs_hash_join *j) {
  if (j->lazy_table) return; // built by hash_join_ensure_table when something probes it
  if (build_dense_dup(j)) return; // duplicate keys over a dense range: runs by key, no general table
  if (lds_build_first(j)) return; // general keys on LDS tables: uniqueness from there, the global table on first need only
  build_hash_table(j);
}
// direct-address slots per build key (a join owned by a HashJoin+HashAgg takes the table up to 16 slots per key: its fused route
// then partitions by key range and needs only the existence bitmap of the range — a filtered dimension, or the hash-partitioned
// shard of one that a rank of the multi-GPU plan receives, 1/8 of the keys of the range for 8 ranks)
static uint64_t dense_slots_per_key(const sqlrs_hash_join *j) {
  if (j->lazy_table) return DENSE_SLOTS_PER_KEY_OWNED;
  return (uint64_t)std::max(1, hook_int(hook("SQLRS_DENSE_JOIN_SLOTS_PLAIN"), 4)); // tuning hook, read per call
}
// the table of a direct-address attempt over [dmin, dmin + range) (empty: the range was refused before one was built)
struct DenseBuilt {
  uint64_t dmin = 0, range = 0;
  BufP dense, packed;
  uint32_t bits = 0, null_head = 0xffffffffu;
};
// A verdict (dense_verdict_decide, dense_range.hpp) -> the join's state and ONE of JR_DENSE_ADOPTED / JR_DENSE_REFUSED per
// attempt.  true = adopted, the build is done; false: the caller goes on with build_after_refusal.
static bool dense_apply_verdict(sqlrs_hash_join *j, const DenseVerdict &v, const DenseBuilt &t) {
  j->ctx->join_route[v.adopt ? Ctx::JR_DENSE_ADOPTED : Ctx::JR_DENSE_REFUSED]++;
  if (v.adopt) {
    j->unique = j->unique_known = j->table_built = true;
    j->dense = t.dense;
    j->dense_min = t.dmin;
    j->dense_range = t.range;
    j->dense_null_head = t.null_head;
    j->dense_packed = t.packed;
    j->dense_pbits = t.bits;
    return true;
  }
  if (v.not_unique) {
    // fewer occupied slots than valid keys (or several NULL keys, which match each other): the build keys are NOT
    // unique — a fact the fused join+aggregate need not discover again by inserting them into its bucket tables
    j->unique = false;
    j->unique_known = true;
  }
  if (v.dup_range) { // (no NULL key: the fused join+aggregate can take multiplicities per key, hash_join_dup_mult)
    j->dup_min = t.dmin;
    j->dup_range = t.range;
  }
  return false;
}
// The one-fetch build's verdict (dense_pack_count_kernel: st[0 .. 35)) -> the join's state.  `h`: the words when the caller
// has fetched them already (with its own answer, in one round trip), else they are fetched here.
void dense_resolve(sqlrs_hash_join *j, const uint64_t *h) { // (join_state.hpp: join_async.hip resolves too)
  if (!j->dense_pending) return;
  j->dense_pending = false;
  uint64_t hw[DENSE_ST_WORDS];
  std::memcpy(hw, h ? h : (const uint64_t *)j->ctx->fetch(j->pend_st->p, 8 * DENSE_ST_WORDS), sizeof(hw)); // (later fetches reuse the staging buffer)
  j->pend_st = nullptr;
  uint64_t nlo = 0, hi = 0;
  for (int i = 0; i < DENSE_MM; i++) nlo = std::max(nlo, hw[i]), hi = std::max(hi, hw[DENSE_MM + i]);
  const uint64_t lo = ~nlo, occupied = hw[2 * DENSE_MM], nulls = hw[2 * DENSE_MM + 1];
  const DenseRange dr = dense_range_decide(lo, hi, j->pend_max_range); // (what dense_dev decided)
  const DenseVerdict v = dense_verdict_decide(dr, occupied, nulls, (uint64_t)j->nB, j->pend_validity);
  const DenseBuilt t{lo ^ (1ull << 63), dr.range, std::move(j->pend_dense), std::move(j->pend_packed), j->pend_bits, (uint32_t)hw[2 * DENSE_MM + 2]};
  if (!dense_apply_verdict(j, v, t)) build_after_refusal(j);
}
// 1. dense surrogate keys (range <= 4 x rows — 16 x for a join+aggregate's join — and < 2^31) -> direct-address table.  It is tried
//    first: when the build keys turn out unique nothing else is needed, and the 16-byte-slot hash table (1.1 ms for 1e7 keys) is never built.
// One fetch (see dense_pack_count_kernel): the table is sized for the largest range that takes the route.  false: not taken.
static bool dense_try_one_fetch(sqlrs_hash_join *j) {
  Ctx *ctx = j->ctx;
  const int64_t n = j->nB;
  // (the one-fetch form allocates the table of the LARGEST admissible range before it has looked at a key: only while that
  //  stays under 1 GiB — advisor r05; beyond, the two-fetch sequence sizes the table from the range it has seen)
  const uint64_t spk1 = j->lazy_table ? DENSE_SLOTS_PER_KEY_OWNED : 4;
  if (n > (1ll << 24) || 4 * (spk1 * (uint64_t)n + 1024) > (1ull << 30)) return false;
  if (hook_is_zero(hook("SQLRS_DENSE_BUILD_ONE_FETCH"))) return false; // A/B hook, read per call (0 = the two-fetch sequence below)
  ProfScope ps(ctx, "join_build_dense");
  const uint64_t max_range = dense_slots_per_key(j) * (uint64_t)n + 1024;
  uint32_t bits = 1;
  while (((1ull << bits) - 1) < (uint64_t)n) bits++; // all ones = empty must not be a build row
  if (bits < 8) bits = 8;
  if (bits > 25 || (max_range + 2) * bits >= (1ull << 32) || j->lazy_table) bits = 0;
  if (hook_is_zero(hook("SQLRS_DENSE_PACKED"))) bits = 0; // A/B hook, read per call (0 = the probe reads the 4-byte table)
  BufP st = ctx->alloc_zero(8 * (DENSE_ST_WORDS + 1)); // (+ the miss flag of a first probe that runs before the verdict is fetched)
  BufP dense = ctx->alloc(4 * (size_t)max_range + 64);
  BufP packed = bits ? ctx->alloc(4 * (size_t)((max_range + 2 + 31) / 32) * bits + 16) : nullptr;
  const uint64_t *keys = j->bkeys->as<uint64_t>(), *vp = j->bkeys_validity ? j->bkeys_validity->as<uint64_t>() : nullptr;
  unsigned long long *stp = st->as<unsigned long long>();
  const unsigned mblocks = (unsigned)std::min<int64_t>(ceil_div(n, 256 * 8), 4 * (int64_t)ctx->num_cus);
  const bool init_fused = max_range + 2 <= (8ull << 20); // (entries: <= 32 MiB of table)
  key_minmax_inv_kernel<<<dim3(mblocks), dim3(256), 0, ctx->stream>>>(keys, vp, n, stp, init_fused ? dense->as<uint4>() : nullptr,
                                                                      (int64_t)((max_range + 2 + 3) / 4));
  if (!init_fused) {
    const unsigned iblocks = (unsigned)std::min<int64_t>(ceil_div((int64_t)max_range + 2, 256 * 4 * 4), 4 * (int64_t)ctx->num_cus);
    dense_init_dev_kernel<<<dim3(iblocks), dim3(256), 0, ctx->stream>>>(stp, max_range, dense->as<uint4>());
  }
  if (n < (1ll << 21))
    dense_fill_dev_kernel<4><<<dim3((unsigned)ceil_div(n, 256 * 4)), dim3(256), 0, ctx->stream>>>(keys, vp, n, stp, max_range,
                                                                                                dense->as<uint32_t>(), stp + 2 * DENSE_MM);
  else
    dense_fill_dev_kernel<1><<<dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, ctx->stream>>>(keys, vp, n, stp, max_range,
                                                                                            dense->as<uint32_t>(), stp + 2 * DENSE_MM);
  if (bits) {
    const unsigned pblocks = (unsigned)std::min<int64_t>(ceil_div(ceil_div((int64_t)max_range + 2, 32), 256), 8 * (int64_t)ctx->num_cus);
    dense_pack_count_kernel<<<dim3(pblocks), dim3(256), 0, ctx->stream>>>(dense->as<uint32_t>(), stp, max_range, bits,
                                                                        packed->as<uint32_t>(), stp + 2 * DENSE_MM);
  } else {
    const unsigned cblocks = (unsigned)std::min<int64_t>(ceil_div((int64_t)max_range, 256 * 8), 4 * (int64_t)ctx->num_cus);
    dense_count_dev_kernel<<<dim3(cblocks), dim3(256), 0, ctx->stream>>>(dense->as<uint32_t>(), stp, max_range, stp + 2 * DENSE_MM);
  }
  SQ_HIP(hipGetLastError());
  ctx->join_route[Ctx::JR_DENSE_ONE_FETCH]++;
  ctx->join_route[bits ? Ctx::JR_DENSE_PACKED : Ctx::JR_DENSE_PLAIN]++;
  j->dense_pending = true;
  j->pend_st = st;
  j->pend_dense = dense;
  j->pend_packed = packed;
  j->pend_bits = bits;
  j->pend_max_range = max_range;
  j->pend_validity = j->bkeys_validity != nullptr;
  // The verdict stays on the device when the first probe can take it from there (dense_resolve): a plain join whose probe
  // kernels read the packed table.  SQLRS_DENSE_BUILD_DEFER=0 (read per call): decide here.
  if (hook_is_zero(hook("SQLRS_DENSE_BUILD_DEFER")) || !bits || j->lazy_table) dense_resolve(j); // A/B hook, read per call
  return true;
}
// Two fetches: the key range first, then a table of exactly that range and its fill / count.  true = adopted, the build is done.
static bool dense_try_two_fetch(sqlrs_hash_join *j) {
  Ctx *ctx = j->ctx;
  const int64_t n = j->nB;
  BufP mm = ctx->alloc(16); // {min = ~0, max = 0} without a host round trip
  SQ_HIP(hipMemsetAsync(mm->p, 0xff, 8, ctx->stream));
  SQ_HIP(hipMemsetAsync(mm->as<uint8_t>() + 8, 0, 8, ctx->stream));
  const uint64_t *keys = j->bkeys->as<uint64_t>(), *vp = j->bkeys_validity ? j->bkeys_validity->as<uint64_t>() : nullptr;
  unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(n, 256 * 8), 4 * (int64_t)ctx->num_cus);
  key_minmax_kernel<<<dim3(blocks), dim3(256), 0, ctx->stream>>>(keys, vp, n, mm->as<unsigned long long>(),
                                                                mm->as<unsigned long long>() + 1);
  SQ_HIP(hipGetLastError());
  const uint64_t *h = (const uint64_t *)ctx->fetch(mm->p, 16);
  const uint64_t lo = h[0], hi = h[1]; // ordered images differ like the signed values; lo > hi: no valid key
  ctx->join_route[Ctx::JR_DENSE_TWO_FETCH]++;
  const DenseRange dr = lo <= hi ? dense_range_decide(lo, hi, dense_slots_per_key(j) * (uint64_t)n + 1024) : DenseRange{false, 0};
  if (!dr.ok) return dense_apply_verdict(j, dense_verdict_decide(dr, 0, 0, (uint64_t)n, vp != nullptr), DenseBuilt{}); // refused: no table, nothing known
  const uint64_t range = dr.range, dmin = lo ^ (1ull << 63); // (back from the ordered image to the two's complement bits)
  ProfScope ps(ctx, "join_build_dense");
  BufP dense = ctx->alloc(4 * (size_t)range + 8);
  SQ_HIP(hipMemsetAsync(dense->p, 0xff, 4 * (size_t)range + 8, ctx->stream));
  uint32_t *null_head = dense->as<uint32_t>() + range; // spare slot after the table
  BufP cnt = ctx->alloc_zero(24); // {occupied slots, NULL keys, copy of the NULL row's head (u32)}
  dense_fill_kernel<<<dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, ctx->stream>>>(
      keys, vp, n, dmin, dense->as<uint32_t>(), null_head, cnt->as<unsigned long long>());
  unsigned cblocks = (unsigned)std::min<int64_t>(ceil_div((int64_t)range, 256 * 8), 4 * (int64_t)ctx->num_cus);
  dense_count_kernel<<<dim3(cblocks), dim3(256), 0, ctx->stream>>>(dense->as<uint32_t>(), (int64_t)range,
                                                                  cnt->as<unsigned long long>());
  SQ_HIP(hipMemcpyAsync(cnt->as<uint64_t>() + 2, null_head, 4, hipMemcpyDeviceToDevice, ctx->stream));
  SQ_HIP(hipGetLastError());
  const uint64_t *hc = (const uint64_t *)ctx->fetch(cnt->p, 24); // one round trip for all three
  ctx->join_route[Ctx::JR_DENSE_PLAIN]++;
  return dense_apply_verdict(j, dense_verdict_decide(dr, hc[0], hc[1], (uint64_t)n, vp != nullptr), {dmin, range, dense, nullptr, 0, (uint32_t)hc[2]});
}
static void build_table(sqlrs_hash_join *j) {
  concat_build_keys(j);
  if (j->exact && j->nB > 0 && j->key_dtype != SQLRS_FLOAT64) {
    if (dense_try_one_fetch(j)) return; // verdict pending on the device, or resolved (dense_resolve goes on after a refusal)
    if (dense_try_two_fetch(j)) return; // adopted
  }
  build_after_refusal(j);
}

// 1b. (round 6) DUPLICATE build keys over a dense range — a foreign key joined to a foreign key, a dimension attribute: the direct-
// address attempt above has found the range and that some key repeats.  The general table (32 MiB of slots for 1e6 rows, a CAS
// insert per row, a stable radix sort by SLOT for the runs, then — for the LDS route — its distinct keys partitioned again: 0.56 ms
// of small launches and six host round trips for 1e6 rows) is not needed: the rows counted per key of the range
// (hash_join_dup_mult), an exclusive scan, and the rows stably sorted by (key - min) ARE the runs; the probe's count pass reads
// {run start, rows} with one 8-byte load per probe row from a table the size of the range (L2-resident for C3's shapes) instead
// of three passes over LDS tables.  1e8 x 1e6 rows, every key ~4 times (4e8 pairs), build + probe: 3.76 -> 2.57 ms.
static bool build_dense_dup(sqlrs_hash_join *j) {
  Ctx *ctx = j->ctx;
  if (!j->dup_range || !j->exact || !j->bkeys || j->bkeys_validity || j->nB <= 0 ||
      j->nB > 0x7fffffffll || j->dup_range >= (1ull << 31))
    return false;
  const uint32_t *mult = hash_join_dup_mult(j);
  if (!mult) return false;
  ProfScope ps(ctx, "join_build_dense_dup");
  const int64_t range = (int64_t)j->dup_range, n = j->nB;
  BufP start = ctx->alloc(4 * (size_t)range + 8), total = ctx->alloc(8);
  exclusive_scan_u32(ctx, mult, range, nullptr, start->as<uint32_t>(), total->as<uint64_t>());
  j->dd_table = ctx->alloc(4 * (size_t)range + 16);
  dd_table_kernel<<<dim3((unsigned)ceil_div(range + 3, 256)), dim3(256), 0, ctx->stream>>>(start->as<uint32_t>(), range, (uint32_t)n, j->dd_table->as<uint32_t>());
  BufP k64 = ctx->alloc(8 * (size_t)n);
  j->rows_by_slot = ctx->alloc(4 * (size_t)n);
  dd_sort_keys_kernel<<<dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, ctx->stream>>>(j->bkeys->as<uint64_t>(), n, j->dup_min, k64->as<uint64_t>());
  iota_u32(ctx, j->rows_by_slot->as<uint32_t>(), n);
  SQ_HIP(hipGetLastError());
  int bits = 1;
  while ((1ull << bits) < (uint64_t)range) bits++;
  radix_sort_pairs(ctx, k64->as<uint64_t>(), j->rows_by_slot->as<uint32_t>(), n, 0, bits); // (stable: a run keeps build insertion order, hash_join.rs:172-177)
  j->unique = false;
  j->table_built = j->unique_known = true; // (no general table: every probe of this join counts on dd_table)
  return true;
}

// 2. open-addressing table over the key hash (any key type, duplicates allowed)
static void build_hash_table(sqlrs_hash_join *j) {
  Ctx *ctx = j->ctx;
  const int64_t n = j->nB;
  BufP keys = j->bkeys, validity = j->bkeys_validity;
  j->table_built = j->unique_known = true;
  uint64_t cap = 64;
  while (2 * cap < 3 * (uint64_t)n) cap <<= 1; // load factor <= 2/3
  j->mask = cap - 1;
  int64_t nslots = (int64_t)cap + 2;
  j->table = ctx->alloc(sizeof(Slot) * (size_t)nslots);
  BufP row_slot = ctx->alloc(4 * (size_t)std::max<int64_t>(n, 1));
  BufP dup = ctx->alloc_zero(8);
  {
    ProfScope ps(ctx, "join_build");
    table_init_kernel<<<dim3((unsigned)ceil_div(nslots, 256)), dim3(256), 0, ctx->stream>>>(
        slots_of(j), nslots);
    if (n)
      join_insert_kernel<<<dim3((unsigned)ceil_div(n, BLOCK)), dim3(BLOCK), 0, ctx->stream>>>(
          keys->as<uint64_t>(), validity ? validity->as<uint64_t>() : nullptr, n,
          slots_of(j), j->mask, row_slot->as<uint32_t>(), dup->as<int>());
    SQ_HIP(hipGetLastError());
  }
  j->unique = ctx->fetch_value(dup->as<int>()) == 0;
  if (!j->unique) {
    // CSR: head = exclusive scan of counts in slot order; rows stably sorted by slot
    ProfScope ps(ctx, "join_build_csr");
    BufP counts = ctx->alloc(4 * (size_t)nslots), heads = ctx->alloc(4 * (size_t)nslots);
    BufP total = ctx->alloc(8);
    slot_counts_kernel<<<dim3((unsigned)ceil_div(nslots, 256)), dim3(256), 0, ctx->stream>>>(
        slots_of(j), nslots, counts->as<uint32_t>());
    exclusive_scan_u32(ctx, counts->as<uint32_t>(), nslots, nullptr, heads->as<uint32_t>(),
                       total->as<uint64_t>());
    slot_heads_kernel<<<dim3((unsigned)ceil_div(nslots, 256)), dim3(256), 0, ctx->stream>>>(
        slots_of(j), nslots, heads->as<uint32_t>());
    BufP k64 = ctx->alloc(8 * (size_t)n);
    j->rows_by_slot = ctx->alloc(4 * (size_t)n);
    u32_to_u64_kernel<<<dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, ctx->stream>>>(
        row_slot->as<uint32_t>(), n, k64->as<uint64_t>());
    iota_u32(ctx, j->rows_by_slot->as<uint32_t>(), n);
    SQ_HIP(hipGetLastError());
    int bits = 1;
    while ((1ull << bits) < (uint64_t)nslots) bits++;
    radix_sort_pairs(ctx, k64->as<uint64_t>(), j->rows_by_slot->as<uint32_t>(), n, 0, bits);
  }
}

void hash_join_ensure_table(sqlrs_hash_join *j) {
  dense_resolve(j);
  if (!j->table_built && j->finished && !j->empty_build && !build_dense_dup(j)) {
    j->ctx->join_route[Ctx::JR_TABLE_LATE]++;
    build_hash_table(j);
  }
}

DenseTable dense_table_of(const sqlrs_hash_join *j) { // (join_state.hpp)
  DenseTable dt;
  dt.heads = j->dense ? j->dense->as<uint32_t>() : nullptr;
  dt.kmin = j->dense_min;
  dt.range = j->dense_range;
  dt.null_head = j->dense_null_head;
  if (j->dense && j->dense_packed) {
    dt.packed = j->dense_packed->as<uint8_t>();
    dt.bits = j->dense_pbits;
    dt.pmask = (1u << j->dense_pbits) - 1;
  }
  return dt;
}

// ---- probe: one function per route, probe_pairs chooses -------------------------------------------------------------------
// The optimistic all-hit attempt of the direct-address probe.  SQLRS_PROBE_ALLHIT=0 (read per call): never.
static bool allhit_wanted(const NKeys &pk) {
  return !hook_is_zero(hook("SQLRS_PROBE_ALLHIT")) && !pk.validity && pk.rows >= (1 << 16); // A/B hook, read per call
}
// its launches: a sample of rows first (a batch with misses raises `miss` early), then every row
static void launch_allhit(Ctx *ctx, const NKeys &pk, int64_t n, const DenseTable &dt, uint64_t *left, uint32_t *right, unsigned int *miss) {
  const uint64_t *keys = pk.keys->as<uint64_t>();
  const int64_t every = std::max<int64_t>(1, n >> 14); // ~16 K sampled rows
  join_probe_dense_sample_kernel<<<dim3((unsigned)ceil_div(ceil_div(n, every), 256)), dim3(256), 0, ctx->stream>>>(keys, n, every, dt, miss);
  if (dt.packed) { // wave-contiguous chunks over the bit-packed table
    const unsigned pblocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n / JAP_ROWS, 4), JAP_GRID * (int64_t)ctx->num_cus));
    if (((uintptr_t)pk.keys->p & 15) == 0)
      join_probe_dense_allhit_packed_kernel<true><<<dim3(pblocks), dim3(256), 0, ctx->stream>>>(keys, n, dt, left, right, miss);
    else
      join_probe_dense_allhit_packed_kernel<false><<<dim3(pblocks), dim3(256), 0, ctx->stream>>>(keys, n, dt, left, right, miss);
  } else {
    const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(n, 256 * JA_ILP), 16 * (int64_t)ctx->num_cus);
    join_probe_dense_allhit_kernel<<<dim3(blocks), dim3(256), 0, ctx->stream>>>(keys, n, dt, left, right, miss);
  }
  SQ_HIP(hipGetLastError());
}
// its outcome: kept, or redone by the compacting kernel, as later batches of this join then are at once
static bool allhit_kept(sqlrs_hash_join *j, bool kept) {
  j->ctx->join_route[kept ? Ctx::JR_ALLHIT_KEPT : Ctx::JR_ALLHIT_REDONE]++;
  if (!kept && j->dense) j->probe_miss_seen = true;
  return kept;
}
// The first probe of a direct-address build whose verdict is still on the device: the all-hit kernel takes key range and
// uniqueness from the device-side words and ONE fetch brings back the build's verdict and the probe's — a host round trip
// less per join (C3: 8 MB of build keys cost 0.07 ms, a third of it that round trip).  true: `out` holds the pairs — a unique
// dense key set and every probe row found its partner; false: the build is resolved, the batch is still to be probed.
static bool probe_allhit_pending(sqlrs_hash_join *j, const NKeys &pk, Pairs *out) {
  Ctx *ctx = j->ctx;
  const int64_t n = pk.rows;
  ProfScope ps(ctx, "join_probe_dense");
  Pairs p;
  p.left = ctx->alloc(8 * (size_t)n);
  p.right = ctx->alloc(4 * (size_t)n);
  unsigned long long *stp = j->pend_st->as<unsigned long long>();
  unsigned int *miss = (unsigned int *)(stp + DENSE_ST_WORDS);
  DenseTable dt;
  dt.heads = j->pend_dense->as<uint32_t>();
  dt.packed = j->pend_packed->as<uint8_t>();
  dt.bits = j->pend_bits;
  dt.pmask = (1u << j->pend_bits) - 1;
  dt.st = stp;
  dt.st_max_range = j->pend_max_range;
  dt.st_rows = (uint64_t)j->nB;
  launch_allhit(ctx, pk, n, dt, p.left->as<uint64_t>(), p.right->as<uint32_t>(), miss);
  ctx->join_route[Ctx::JR_PROBE_PENDING]++;
  uint64_t hw[DENSE_ST_WORDS + 1];
  std::memcpy(hw, ctx->fetch(j->pend_st->p, 8 * (DENSE_ST_WORDS + 1)), sizeof(hw));
  dense_resolve(j, hw);
  if (!allhit_kept(j, j->dense && (unsigned int)hw[DENSE_ST_WORDS] == 0)) return false;
  p.m = n;
  p.right_identity = true;
  *out = p;
  return true;
}
// unique build keys, Inner / Left: hits compacted with look-back over the LDS route's match (`lm`), the dense or the slot table
static Pairs probe_unique_inner(sqlrs_hash_join *j, const NKeys &pk, const LdsJoinMatch &lm) {
  Ctx *ctx = j->ctx;
  const int64_t n = pk.rows;
  Pairs p;
  int64_t tiles = lm.ok ? lds_join_tiles(n) : ceil_div(n, j->dense ? JD_TILE : JP_TILE);
  p.left = ctx->alloc(8 * (size_t)n);
  p.right = ctx->alloc(4 * (size_t)n);
  // the all-hit attempt first (join_probe_dense_allhit_kernel); its miss flag is a word of its own (a zeroed slab: no memset)
  // and is NOT cleared by a look-back rerun.  The look-back descriptors are allocated (and cleared: a memset) only when the
  // compacting kernel runs.
  unsigned int *miss = nullptr;
  BufP miss_buf;
  if (allhit_wanted(pk) && j->dense && !lm.ok && !j->probe_miss_seen) {
    miss_buf = ctx->alloc_zero(8);
    miss = miss_buf->as<unsigned int>();
    ProfScope ps(ctx, "join_probe_dense");
    launch_allhit(ctx, pk, n, dense_table_of(j), p.left->as<uint64_t>(), p.right->as<uint32_t>(), miss);
    if (allhit_kept(j, ctx->fetch_value(miss) == 0)) {
      p.m = n;
      p.right_identity = true;
      return p;
    }
  }
  BufP desc = ctx->alloc_zero(8 * (size_t)tiles + 24);
  unsigned *ticket = (unsigned *)(desc->as<uint64_t>() + tiles);
  uint64_t *tot = desc->as<uint64_t>() + tiles + 1;
  if (!lm.ok) ctx->join_route[j->dense ? Ctx::JR_COMPACT_DENSE : Ctx::JR_COMPACT_SLOTS]++;
  for (int use_ticket = lookback_start_mode(ctx), attempt = 0; use_ticket < 2; use_ticket++, attempt++) {
    if (attempt) SQ_HIP(hipMemsetAsync(desc->p, 0, 8 * (size_t)tiles + 16, ctx->stream)); // rerun after a timeout
    {
      ProfScope ps(ctx, lm.ok ? "join_match_compact" : (j->dense ? "join_probe_dense" : "join_probe_unique"));
      dim3 gt((unsigned)tiles);
      DenseTable dt = dense_table_of(j);
      if (lm.ok) {
        lds_join_restore(ctx, lm, n, p.left->as<uint64_t>(), p.right->as<uint32_t>(), desc->as<uint64_t>(), ticket, tot, use_ticket);
      } else if (j->dense && pk.validity)
        join_probe_dense_kernel<true><<<gt, dim3(JD_BLOCK), 0, ctx->stream>>>(
            pk.keys->as<uint64_t>(), pk.validity, n, tiles, dt, p.left->as<uint64_t>(), p.right->as<uint32_t>(),
            desc->as<uint64_t>(), ticket, tot, use_ticket);
      else if (j->dense)
        join_probe_dense_kernel<false><<<gt, dim3(JD_BLOCK), 0, ctx->stream>>>(
            pk.keys->as<uint64_t>(), pk.validity, n, tiles, dt, p.left->as<uint64_t>(), p.right->as<uint32_t>(),
            desc->as<uint64_t>(), ticket, tot, use_ticket, miss);
      else
        join_probe_unique_kernel<false><<<gt, dim3(BLOCK), 0, ctx->stream>>>(
            pk.keys->as<uint64_t>(), pk.validity, n, tiles, slots_of(j), j->mask, dt,
            p.left->as<uint64_t>(), p.right->as<uint32_t>(), desc->as<uint64_t>(), ticket, tot, use_ticket);
      SQ_HIP(hipGetLastError());
    }
    const uint64_t *h = (const uint64_t *)ctx->fetch(ticket, 16); // {ticket|timeout, total}
    p.m = (int64_t)h[1];
    if (use_ticket || (h[0] >> 32) == 0) break;
    lookback_timed_out(ctx);
  }
  // unique build keys, pairs in probe-row order: as many pairs as probe rows = every row matched once = pair i is (.., i)
  p.right_identity = p.m == n;
  return p;
}
// unique build keys, Right / Full: exactly one pair per probe row, pair i = (build row | NULL, probe row i)
static Pairs probe_unique_outer(sqlrs_hash_join *j, const NKeys &pk) {
  Ctx *ctx = j->ctx;
  const int64_t n = pk.rows;
  Pairs p;
  p.m = n;
  p.right_identity = true;
  p.left = ctx->alloc(8 * (size_t)n);
  p.right = ctx->alloc(4 * (size_t)n);
  p.left_validity = ctx->alloc(bitmap_bytes(n));
  ProfScope ps(ctx, "join_probe_unique");
  ctx->join_route[Ctx::JR_UNIQUE_OUTER]++;
  int64_t n64 = (int64_t)round_up((size_t)n, 64);
  DenseTable dt = dense_table_of(j);
  if (j->dense)
    join_probe_unique_outer_kernel<true><<<dim3((unsigned)ceil_div(n64, BLOCK)), dim3(BLOCK), 0, ctx->stream>>>(
        pk.keys->as<uint64_t>(), pk.validity, n, slots_of(j), j->mask, dt, p.left->as<uint64_t>(),
        p.right->as<uint32_t>(), p.left_validity->as<uint64_t>());
  else
    join_probe_unique_outer_kernel<false><<<dim3((unsigned)ceil_div(n64, BLOCK)), dim3(BLOCK), 0, ctx->stream>>>(
        pk.keys->as<uint64_t>(), pk.validity, n, slots_of(j), j->mask, dt, p.left->as<uint64_t>(),
        p.right->as<uint32_t>(), p.left_validity->as<uint64_t>());
  SQ_HIP(hipGetLastError());
  return p;
}
// duplicate build keys, and Right / Full joins over general keys: count matches per probe row -> exclusive scan -> fill.  The
// count comes from the LDS route's match (`lmg`, un-permuted into {run, pairs}), from dd_table, or from the slot table.
static Pairs probe_counted(sqlrs_hash_join *j, const NKeys &pk, const LdsJoinMatch &lmg) {
  Ctx *ctx = j->ctx;
  const int64_t n = pk.rows;
  const int outer_right = is_outer_right(j);
  Pairs p;
  dim3 g((unsigned)ceil_div(n, BLOCK)), b(BLOCK);
  // The fill pass scans the pair counts of its 64 probe rows itself, so only one sum per 64-row group is scanned globally
  // (round 6: per-row counts + offsets were 0.4 + 0.8 GB written and 1.2 GB read for 1e8 probe rows, 0.45 ms of scan).  A build
  // side of >= 2^26 rows — 64 runs of that length overflow a 32-bit sum — keeps per-row counts.
  const bool per_row = hook_is_zero(hook("SQLRS_JOIN_GROUPED")); // test hook, read per call: 0 = per-row counts whatever the build side's size
  const int grouped = (j->nB < (1ll << 26) && !per_row) ? 1 : 0;
  ctx->join_route[grouped ? Ctx::JR_COUNTS_GROUPED : Ctx::JR_COUNTS_PER_ROW]++;
  const int64_t nscan = grouped ? ceil_div(n, 64) : n;
  BufP counts = ctx->alloc(4 * (size_t)nscan), offsets = ctx->alloc(8 * (size_t)nscan), total = ctx->alloc(8);
  BufP match = ctx->alloc(8 * (size_t)n);
  if (lmg.ok) {
    ProfScope ps(ctx, "join_match_unpermute");
    lds_join_unpermute(j, lmg, n, outer_right, match->as<uint2>(), counts->as<uint32_t>(), grouped);
  } else if (j->dd_table) { // duplicate keys over a dense range: {run, rows} by direct address
    ProfScope ps(ctx, "join_probe_count_dense_dup");
    const bool stream = !pk.validity && n >= JAP_ROWS && ((uintptr_t)pk.keys->p & 15) == 0;
    ctx->join_route[stream ? Ctx::JR_DD_STREAM : Ctx::JR_DD_ROWS]++;
    if (stream) {
      const unsigned pblocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(n / JAP_ROWS, 4), JAP_GRID * (int64_t)ctx->num_cus));
      dd_count_stream_kernel<<<dim3(pblocks), dim3(256), 0, ctx->stream>>>(pk.keys->as<uint64_t>(), n, j->dup_min, j->dup_range, j->dd_table->as<uint32_t>(),
                                                                         outer_right, counts->as<uint32_t>(), match->as<uint2>(), grouped);
    } else
      dd_count_kernel<<<dim3((unsigned)ceil_div(n, (int64_t)BLOCK * DD_U)), b, 0, ctx->stream>>>(pk.keys->as<uint64_t>(), pk.validity, n, j->dup_min, j->dup_range, j->dd_table->as<uint32_t>(), outer_right,
                                                counts->as<uint32_t>(), match->as<uint2>(), grouped);
    SQ_HIP(hipGetLastError());
  } else {
    ProfScope ps(ctx, "join_probe_count");
    join_count_kernel<<<g, b, 0, ctx->stream>>>(pk.keys->as<uint64_t>(), pk.validity, n, slots_of(j), j->mask, outer_right,
                                                counts->as<uint32_t>(), match->as<uint2>(), grouped);
    SQ_HIP(hipGetLastError());
  }
  exclusive_scan_u32(ctx, counts->as<uint32_t>(), nscan, offsets->as<uint64_t>(), nullptr,
                     total->as<uint64_t>());
  p.m = (int64_t)ctx->fetch_value(total->as<uint64_t>());
  int64_t m1 = std::max<int64_t>(p.m, 1);
  p.left = ctx->alloc(8 * (size_t)m1);
  p.right = ctx->alloc(4 * (size_t)m1);
  BufP lvb;
  if (outer_right) lvb = ctx->alloc((size_t)m1);
  if (p.m) {
    ProfScope ps(ctx, "join_probe_fill");
    join_fill_expand_kernel<<<g, b, 0, ctx->stream>>>(
        match->as<uint2>(), n, j->unique ? 1 : 0, outer_right, j->rows_by_slot ? j->rows_by_slot->as<uint32_t>() : nullptr,
        offsets->as<uint64_t>(), p.left->as<uint64_t>(), p.right->as<uint32_t>(), lvb ? lvb->as<uint8_t>() : nullptr, grouped);
    SQ_HIP(hipGetLastError());
  }
  if (outer_right) {
    p.left_validity = ctx->alloc(bitmap_bytes(m1));
    int64_t m64 = (int64_t)round_up((size_t)m1, 64);
    bytes_to_bits_kernel<<<dim3((unsigned)ceil_div(m64, 256)), dim3(256), 0, ctx->stream>>>(
        lvb->as<uint8_t>(), p.m, p.left_validity->as<uint64_t>());
    SQ_HIP(hipGetLastError());
  }
  return p;
}
// which route a probe batch takes (tests/test_gpu_join_edges.py, Plan.probe, restates this order of conditions)
static Pairs probe_pairs(sqlrs_hash_join *j, const NKeys &pk) {
  Ctx *ctx = j->ctx;
  if (pk.exact != j->exact || (pk.exact && pk.dtype != j->key_dtype))
    fail(SQLRS_ERR_INTERNAL, "join keys of different types on the two sides are not supported");
  Pairs p;
  const int64_t n = pk.rows;
  const bool outer_right = is_outer_right(j);
  if (j->dense_pending && allhit_wanted(pk) && !outer_right && n <= 0xffffffffll && j->pend_bits)
    if (probe_allhit_pending(j, pk, &p)) return p; // (false: the build is resolved, the batch still to be probed)
  // (a build side whose uniqueness came from lds_build_first has no global table yet: built only when this batch needs it)
  LdsJoinMatch lm;
  dense_resolve(j);
  if (j->lds_first && !j->table_built && j->unique && !outer_right && !j->dense && n > 0) lm = lds_join_match(j, pk);
  if (!lm.ok) hash_join_ensure_table(j);
  if (n == 0) {
    p.left = ctx->alloc(8);
    p.right = ctx->alloc(8);
    return p;
  }
  if (n > 0xffffffffll) fail(SQLRS_ERR_INTERNAL, "probe batch larger than 2^32 rows");
  // general keys, build side beyond an L2-resident table: LDS tables over a blocked partition (see lds_join_probe_kernel)
  if (!lm.ok && j->unique && !outer_right && !j->dense) lm = lds_join_match(j, pk);
  if (j->unique && !outer_right) return probe_unique_inner(j, pk, lm);
  // duplicate build keys, and Right / Full joins over general keys: matched on the LDS tables too
  LdsJoinMatch lmg;
  if (!j->dense && !j->dd_table && (!j->unique || outer_right)) lmg = lds_join_match(j, pk, !j->unique);
  if (j->unique && outer_right && !lmg.ok) return probe_unique_outer(j, pk);
  return probe_counted(j, pk, lmg);
}

static DBatch gather_pairs(sqlrs_hash_join *j, const DBatch &right, const Pairs &p) {
  Ctx *ctx = j->ctx;
  DBatch out;
  out.rows = p.m;
  const uint64_t *lv = p.left_validity ? p.left_validity->as<uint64_t>() : nullptr;
  // Join-key equivalence: with one exactly-compared key `left[c] = right[rc]` every emitted pair
  // carries equal key values on both sides (NULL = NULL included, hash_utils.rs:91-104), so for
  // Inner/Left the gathered build key column is the gathered probe key column: the random
  // gather over the build side is skipped.
  int lkey_col = -1, rkey_col = -1;
  if (!is_outer_right(j) && j->exact && j->lkeys.size() == 1 && j->lkeys[0].nodes.size() == 1 &&
      j->rkeys[0].nodes.size() == 1 && j->lkeys[0].nodes[0].op == SQLRS_EXPR_INPUT_REF &&
      j->rkeys[0].nodes[0].op == SQLRS_EXPR_INPUT_REF) {
    lkey_col = j->lkeys[0].nodes[0].index;
    rkey_col = j->rkeys[0].nodes[0].index;
    if (lkey_col < 0 || (size_t)lkey_col >= j->left.cols.size() || rkey_col < 0 ||
        (size_t)rkey_col >= right.cols.size() ||
        j->left.cols[(size_t)lkey_col].dtype != right.cols[(size_t)rkey_col].dtype)
      lkey_col = rkey_col = -1;
  }
  std::vector<DCol> rcols;
  for (const DCol &c : right.cols)
    rcols.push_back(p.right_identity ? c : gather_column(ctx, c, p.right->p, false, nullptr, p.m));
  for (size_t c = 0; c < j->left.cols.size(); c++) {
    if ((int)c == lkey_col)
      out.cols.push_back(rcols[(size_t)rkey_col]);
    else
      out.cols.push_back(gather_column(ctx, j->left.cols[c], p.left->p, true, lv, p.m));
  }
  for (DCol &c : rcols) out.cols.push_back(std::move(c));
  return out;
}

// apply_join_filter  (hash_join.rs:47-127)
static void apply_filter(sqlrs_hash_join *j, const DBatch &right, Pairs &p) {
  Ctx *ctx = j->ctx;
  DBatch inter = gather_pairs(j, right, p); // intermediate batch (:256-262)
  auto colfn = [&](int i) -> const DCol & {
    if (i < 0 || (size_t)i >= inter.cols.size()) fail(SQLRS_ERR_INTERNAL, "input ref out of range");
    return inter.cols[(size_t)i];
  };
  DCol mask = eval_expr(ctx, j->filter, colfn, inter.rows, false);
  mask.length = inter.rows;
  Selection sel = selection_from_mask(ctx, mask);
  DCol lcol, rcol;
  pairs_as_columns(p, &lcol, &rcol);
  DCol lf = compact_column(ctx, lcol, sel), rf = compact_column(ctx, rcol, sel);
  if (!is_outer_right(j)) {
    p.m = sel.count;
    p.left = lf.own_values;
    p.right = rf.own_values;
    p.left_validity = lf.own_validity; // always all-valid here
    return;
  }
  // keep every right row: rows that lost all their matches come back as (NULL, row) (:73-121)
  int64_t nr = right.rows;
  BufP visited = ctx->alloc_zero(bitmap_bytes(std::max<int64_t>(nr, 1)));
  if (sel.count)
    mark_bits_kernel<uint32_t><<<dim3((unsigned)ceil_div(sel.count, 256)), dim3(256), 0, ctx->stream>>>(
        rf.v<uint32_t>(), nullptr, sel.count, visited->as<unsigned long long>());
  SQ_HIP(hipGetLastError());
  Selection unv = selection_from_clear_bits(ctx, visited->as<uint64_t>(), nr);
  BufP uidx = selection_indices_u32(ctx, unv);
  DCol ucol;
  ucol.dtype = SQLRS_UINT32;
  ucol.length = unv.count;
  ucol.values = uidx->p;
  ucol.own_values = uidx;
  DCol lnull = make_null_column(ctx, SQLRS_UINT64, unv.count);
  if (!lf.validity) lf.null_count = 0;
  DCol l2 = concat_columns(ctx, {&lf, &lnull});
  DCol r2 = concat_columns(ctx, {&rf, &ucol});
  p.m = sel.count + unv.count;
  p.left = l2.own_values;
  p.right = r2.own_values;
  p.left_validity = l2.own_validity;
  if (!p.left_validity && unv.count == 0 && lf.own_validity) p.left_validity = lf.own_validity;
}

const uint32_t *hash_join_dup_mult(sqlrs_hash_join *j) {
  dense_resolve(j);
  if (!j->dup_range || !j->bkeys || j->bkeys_validity) return nullptr;
  if (!j->dup_mult) {
    Ctx *ctx = j->ctx;
    j->dup_mult = ctx->alloc_zero(4 * (size_t)j->dup_range + 8);
    dup_mult_kernel<<<dim3((unsigned)ceil_div(j->nB, 256)), dim3(256), 0, ctx->stream>>>(j->bkeys->as<uint64_t>(), j->nB, j->dup_min,
                                                                                      j->dup_mult->as<uint32_t>());
    SQ_HIP(hipGetLastError());
  }
  return j->dup_mult->as<uint32_t>();
}

const uint64_t *hash_join_dense_bits(sqlrs_hash_join *j) {
  dense_resolve(j);
  if (!j->dense || !j->dense_range) return nullptr;
  if (!j->dense_bits) {
    Ctx *ctx = j->ctx;
    const int64_t words = ceil_div((int64_t)j->dense_range, 64);
    j->dense_bits = ctx->alloc(8 * (size_t)words + 8);
    dense_bits_kernel<<<dim3((unsigned)ceil_div(words * 64, 256)), dim3(256), 0, ctx->stream>>>(
        j->dense->as<uint32_t>(), (int64_t)j->dense_range, j->dense_bits->as<uint64_t>());
    SQ_HIP(hipGetLastError());
  }
  return j->dense_bits->as<uint64_t>();
}

// Key-only build side (see dense_bits_kernel): true = `out` holds the joined batch
static bool semi_join_probe(sqlrs_hash_join *j, InBatch &ib, const NKeys &pk, DBatch *out) {
  Ctx *ctx = j->ctx;
  if (j->dense_pending && j->join_type == SQLRS_JOIN_INNER && !j->has_filter && j->left.cols.size() == 1) dense_resolve(j); // (a candidate: decide now)
  if (j->join_type != SQLRS_JOIN_INNER || j->has_filter || !j->unique || !j->dense || !j->exact || pk.validity ||
      j->left.cols.size() != 1 || j->lkeys.size() != 1 || j->lkeys[0].nodes.size() != 1 || j->rkeys[0].nodes.size() != 1 ||
      j->lkeys[0].nodes[0].op != SQLRS_EXPR_INPUT_REF || j->rkeys[0].nodes[0].op != SQLRS_EXPR_INPUT_REF ||
      j->lkeys[0].nodes[0].index != 0)
    return false;
  const int rkey_col = j->rkeys[0].nodes[0].index;
  const int64_t n = ib.rows();
  if (rkey_col < 0 || rkey_col >= ib.num_columns() || n < (1 << 16)) return false;
  if (j->left.cols[0].dtype != ib.col(rkey_col).dtype) return false;
  // Unique build keys that FILL their range (as many rows as the range has values, none NULL: a dimension's surrogate keys) —
  // a probe key inside the range has its partner, no table says more: the mask is a range test over the key stream (5e8 probe
  // rows: 2.55 -> ms of lookups in the 1.25 MB bitmap gone; the fused route takes the same shortcut, hashagg_op.hip)
  const bool full_range = j->unique && j->unique_known && !j->bkeys_validity && j->dense_range == (uint64_t)j->nB;
  if (!full_range) hash_join_dense_bits(j);
  Selection sel;
  sel.rows = n;
  const int64_t nwords = ceil_div(n, 64);
  sel.own_bits = ctx->alloc(8 * (size_t)nwords + 64);
  sel.bits = sel.own_bits->as<uint64_t>();
  {
    ProfScope ps(ctx, "join_semi_mask");
    const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(nwords, WAVES_PER_BLOCK * SM_U), 8 * (int64_t)ctx->num_cus);
    BufP hits = ctx->alloc_zero(8);
    semi_mask_kernel<<<dim3(std::max(blocks, 1u)), dim3(BLOCK), 0, ctx->stream>>>(
        pk.keys->as<uint64_t>(), n, full_range ? nullptr : j->dense_bits->as<uint64_t>(), j->dense_min, j->dense_range, sel.own_bits->as<uint64_t>(),
        hits->as<unsigned long long>());
    SQ_HIP(hipGetLastError());
    sel.count = (int64_t)ctx->fetch_value(hits->as<uint64_t>());
  }
  if (sel.count != n) selection_finish(ctx, sel); // (tile offsets are only needed to compact: 1.4 ms per 5e8 rows)
  // (all rows kept: the output SHARES the probe columns — library-owned buffers by reference, a caller's borrowed
  //  device buffers as private copies, since a batch is only borrowed for the call)
  DBatch right = ib.materialize(sel.count == n);
  out->rows = sel.count;
  std::vector<DCol> rcols;
  if (sel.count == n) { // every probe row has its partner (PK-FK): the probe columns ARE the joined rows
    rcols = right.cols;
  } else {
    for (const DCol &c : right.cols) rcols.push_back(compact_column(ctx, c, sel));
  }
  out->cols.push_back(rcols[(size_t)rkey_col]); // the build key column = the probe key column of the matched rows
  for (DCol &c : rcols) out->cols.push_back(std::move(c));
  return true;
}

// `also` (optional): the joined batch AND its pairs (probe_push_many cuts the batch at probe-row boundaries)
static DBatch probe_batch(sqlrs_hash_join *j, InBatch &ib, Pairs *pairs_only, Pairs *also = nullptr) {
  Ctx *ctx = j->ctx;
  auto colfn = [&](int i) -> const DCol & { return ib.col(i); };
  NKeys pk = j->comp.on ? composite_probe_keys(j, colfn, ib.rows()) : eval_keys(ctx, j->rkeys, colfn, ib.rows());
  if (!pairs_only && !also) {
    DBatch semi;
    if (semi_join_probe(j, ib, pk, &semi)) return semi;
  }
  Pairs p = probe_pairs(j, pk);
  if (also) *also = p;
  if (pairs_only) {
    *pairs_only = p;
    return DBatch();
  }
  if (j->has_filter) p.right_identity = false; // (the join filter selects among the pairs)
  // every probe row matched exactly once: the joined batch takes the probe columns as they are — shared when they
  // are this library's own buffers (an upstream operator's output), copied once when the caller only lent them
  DBatch right = ib.materialize(p.right_identity);
  if (j->has_filter) apply_filter(j, right, p);
  if ((j->join_type == SQLRS_JOIN_LEFT || j->join_type == SQLRS_JOIN_FULL) && p.m) {
    mark_bits_kernel<uint64_t><<<dim3((unsigned)ceil_div(p.m, 256)), dim3(256), 0, ctx->stream>>>(
        p.left->as<uint64_t>(), p.left_validity ? p.left_validity->as<uint64_t>() : nullptr, p.m,
        j->visited->as<unsigned long long>()); // :274-282
    SQ_HIP(hipGetLastError());
  }
  return gather_pairs(j, right, p); // :284-291
}
// (join_state.hpp) the synchronous operator's HOST batch for one probe batch: what push_async parks in a ticket (join_async.hip)
sqlrs_batch_t *hash_join_probe_sync(sqlrs_hash_join *j, const sqlrs_batch_t *right) {
  InBatch ib(j->ctx, right);
  return emit_batch(j->ctx, probe_batch(j, ib, nullptr), SQLRS_MEM_HOST);
}

} // namespace sq

extern "C" {

int sqlrs_hash_join_create(sqlrs_ctx_t *ctx, int join_type, int num_keys,
                           const sqlrs_expr_t *left_keys, const sqlrs_expr_t *right_keys,
                           const sqlrs_expr_t *filter, int num_right_columns,
                           const int32_t *right_dtypes, sqlrs_hash_join_t **out) {
  return guard(ctx, [&] {
    if (num_keys < 1) fail(SQLRS_ERR_INTERNAL, "HashJoin must has on condition"); // :132
    if (join_type < SQLRS_JOIN_INNER || join_type > SQLRS_JOIN_FULL)
      fail(SQLRS_ERR_INTERNAL, "bad join type");
    auto j = std::unique_ptr<sqlrs_hash_join>(new sqlrs_hash_join());
    j->ctx = ctx;
    j->join_type = join_type;
    for (int i = 0; i < num_keys; i++) {
      j->lkeys.push_back(expr_from_abi(&left_keys[i]));
      j->rkeys.push_back(expr_from_abi(&right_keys[i]));
    }
    if (filter && filter->num_nodes > 0) {
      j->has_filter = true;
      j->filter = expr_from_abi(filter);
    }
    if (num_right_columns > 0) j->right_dtypes.assign(right_dtypes, right_dtypes + num_right_columns);
    j->hstage.all_types = stage_all_types_flag(num_keys, left_keys); // SQLRS_EXPR_STAGE_ALL_TYPES: the build side's stage (host_stage.hpp)
    *out = j.release();
  });
}

static int hash_join_build_push_device(sqlrs_hash_join_t *j, const sqlrs_batch_t *left);
static int hash_join_flush_host(sqlrs_hash_join_t *j) {
  if (!j->hstage.has_schema) return SQLRS_OK;
  sqlrs_batch_t *dev = nullptr;
  int st = guard(j->ctx, [&] {
    SQ_HIP(hipSetDevice(j->ctx->device));
    dev = j->hstage.take();
  });
  if (st != SQLRS_OK) return st;
  st = hash_join_build_push_device(j, dev);
  sqlrs_batch_release(dev);
  return st;
}
int sqlrs_hash_join_build_push(sqlrs_hash_join_t *j, const sqlrs_batch_t *left) {
  j->hstage.ctx = j->ctx;
  if (!j->finished && j->hstage.accepts(left)) {
    int st = j->hstage.flush_before(left) ? hash_join_flush_host(j) : SQLRS_OK;
    if (st == SQLRS_OK) st = guard(j->ctx, [&] { j->hstage.append(left); });
    if (st != SQLRS_OK || j->hstage.rows < HOST_STAGE_FLUSH_ROWS) return st;
    return hash_join_flush_host(j);
  }
  int st = hash_join_flush_host(j);
  return st != SQLRS_OK ? st : hash_join_build_push_device(j, left);
}
static int hash_join_build_push_device(sqlrs_hash_join_t *j, const sqlrs_batch_t *left) {
  return guard(j->ctx, [&] {
    SQ_HIP(hipSetDevice(j->ctx->device));
    if (j->finished) fail(SQLRS_ERR_INTERNAL, "build_push after build_finish");
    InBatch ib(j->ctx, left);
    DBatch b = ib.materialize(true);
    auto colfn = [&](int i) -> const DCol & {
      if (i < 0 || (size_t)i >= b.cols.size()) fail(SQLRS_ERR_INTERNAL, "input ref out of range");
      return b.cols[(size_t)i];
    };
    // (the evaluated key columns are kept only for the opt-in composite key, concat_build_keys: 8 B x rows x keys of device memory
    //  otherwise held until build_finish for nothing)
    const char *ck_e = std::getenv("SQLRS_JOIN_COMPOSITE");
    if (j->lkeys.size() >= 2 && j->lkeys.size() <= 4 && !j->lazy_table && ck_e && std::atoi(ck_e) == 1) {
      std::vector<DCol> kc = eval_key_cols(j->ctx, j->lkeys, colfn, b.rows);
      j->left_key_parts.push_back(normalize_keys(j->ctx, kc, b.rows));
      j->left_keycol_parts.push_back(std::move(kc));
    } else
      j->left_key_parts.push_back(eval_keys(j->ctx, j->lkeys, colfn, b.rows));
    j->left_batches.push_back(std::move(b));
    j->empty_build = false;
  });
}

int sqlrs_hash_join_build_finish(sqlrs_hash_join_t *j) {
  int stf = hash_join_flush_host(j);
  if (stf != SQLRS_OK) return stf;
  return guard(j->ctx, [&] {
    SQ_HIP(hipSetDevice(j->ctx->device));
    if (j->finished) return;
    j->finished = true;
    if (j->empty_build) return; // the join emits nothing (:183-185)
    Ctx *ctx = j->ctx;
    size_t nc = j->left_batches[0].cols.size();
    for (size_t c = 0; c < nc; c++) {
      std::vector<const DCol *> parts;
      for (DBatch &b : j->left_batches) {
        if (b.cols.size() != nc) fail(SQLRS_ERR_ARROW, "concat_batches: schema mismatch");
        parts.push_back(&b.cols[c]);
      }
      j->left.cols.push_back(concat_columns(ctx, parts));
    }
    for (DBatch &b : j->left_batches) j->nB += b.rows;
    j->left.rows = j->nB;
    if (j->nB > 0xffffffffll) fail(SQLRS_ERR_INTERNAL, "build side larger than 2^32 rows");
    build_table(j);
    j->left_batches.clear();
    j->left_key_parts.clear();
    if (j->join_type == SQLRS_JOIN_LEFT || j->join_type == SQLRS_JOIN_FULL)
      j->visited = ctx->alloc_zero(bitmap_bytes(std::max<int64_t>(j->nB, 1)));
  });
}

int sqlrs_hash_join_probe_push(sqlrs_hash_join_t *j, const sqlrs_batch_t *right, int out_mem,
                               sqlrs_batch_t **out) {
  return guard(j->ctx, [&] {
    SQ_HIP(hipSetDevice(j->ctx->device));
    if (!j->finished) fail(SQLRS_ERR_INTERNAL, "probe before build_finish");
    j->probe_started = true;
    *out = nullptr;
    if (j->empty_build) return;
    InBatch ib(j->ctx, right);
    DBatch r = probe_batch(j, ib, nullptr);
    *out = emit_batch(j->ctx, std::move(r), out_mem);
  });
}

// n probe batches in one call: out[i] is what sqlrs_hash_join_probe_push(right[i]) returns [ref: hash_join.rs:207-292: one
// joined batch per probe batch] — for the reference's batch shape, 1024-row HOST batches (storage/csv.rs:105), where one
// upload + probe + download per batch is ~80 us a call (12 Mrows/s).  Inner / Left joins without a join filter whose
// batches are small HOST batches of fixed-width columns (and whose joined columns are fixed width): the batches are
// uploaded together and probed as ONE batch — the pairs come out probe-row major (hash_join.rs:225-234), so input batch
// i's joined rows are one contiguous range, found by searching the pairs' probe rows for the batch boundaries — and
// every range is handed out as a HOST batch of its own.  Anything else runs batch by batch.
int sqlrs_hash_join_probe_push_many(sqlrs_hash_join_t *j, int n, const sqlrs_batch_t *const *right, int out_mem,
                                    sqlrs_batch_t **out) {
  return guard(j->ctx, [&] {
    Ctx *ctx = j->ctx;
    SQ_HIP(hipSetDevice(ctx->device));
    if (!j->finished) fail(SQLRS_ERR_INTERNAL, "probe before build_finish");
    j->probe_started = true;
    for (int i = 0; i < n; i++) out[i] = nullptr;
    if (n <= 0 || j->empty_build) return;
    if (!j->probe_stage) {
      j->probe_stage.reset(new HostStage());
      j->probe_stage->ctx = ctx;
    }
    HostStage &st = *j->probe_stage;
    bool stageable = out_mem == SQLRS_MEM_HOST && n > 1 && !j->has_filter && !st.has_schema &&
                     (j->join_type == SQLRS_JOIN_INNER || j->join_type == SQLRS_JOIN_LEFT) && all_fixed_width(j->left);
    int64_t total_rows = 0;
    for (int i = 0; i < n && stageable; i++) {
      stageable = st.accepts(right[i]) && right[i]->num_columns == right[0]->num_columns;
      for (int c = 0; c < right[i]->num_columns && stageable; c++) stageable = right[i]->columns[c].dtype == right[0]->columns[c].dtype;
      total_rows += right[i] ? right[i]->num_rows : 0;
    }
    if (!stageable || total_rows == 0 || total_rows > (1ll << 30)) {
      int i = 0;
      try {
        for (; i < n; i++) {
          InBatch ib(ctx, right[i]);
          out[i] = emit_batch(ctx, probe_batch(j, ib, nullptr), out_mem);
        }
      } catch (...) {
        for (int k = 0; k < i; k++) {
          sqlrs_batch_release(out[k]);
          out[k] = nullptr;
        }
        throw;
      }
      return;
    }
    std::vector<int64_t> bounds((size_t)n + 1, 0);
    try {
      for (int i = 0; i < n; i++) {
        st.append(right[i]);
        bounds[(size_t)i + 1] = bounds[(size_t)i] + right[i]->num_rows;
      }
    } catch (...) {
      j->probe_stage.reset(); // (a half-staged call must not leave its schema and rows behind: the staged path would stay off)
      throw;
    }
    sqlrs_batch_t *dev = st.take();
    struct Rel {
      sqlrs_batch_t *b;
      ~Rel() { if (b) sqlrs_batch_release(b); }
    } rel{dev};
    Pairs p;
    DBatch o;
    {
      InBatch ib(ctx, dev);
      o = probe_batch(j, ib, nullptr, &p);
    }
    std::vector<int64_t> cut = bounds; // every probe row matched exactly once: pair i = probe row i
    if (!p.right_identity) {
      BufP dbounds = ctx->alloc(8 * ((size_t)n + 1)), dcut = ctx->alloc(8 * ((size_t)n + 1));
      SQ_HIP(hipMemcpyAsync(dbounds->p, bounds.data(), 8 * ((size_t)n + 1), hipMemcpyHostToDevice, ctx->stream));
      pairs_before_kernel<<<dim3((unsigned)ceil_div(n + 1, 256)), dim3(256), 0, ctx->stream>>>(
          p.right->as<uint32_t>(), p.m, dbounds->as<int64_t>(), n + 1, dcut->as<int64_t>());
      SQ_HIP(hipGetLastError());
      SQ_HIP(hipMemcpyAsync(cut.data(), dcut->p, 8 * ((size_t)n + 1), hipMemcpyDeviceToHost, ctx->stream));
      ctx->sync();
    }
    if (!all_fixed_width(o)) fail(SQLRS_ERR_INTERNAL, "probe_push_many: joined columns are fixed width");
    split_rows_to_host(ctx, o, cut, &j->pin_out, &j->pin_cap, n, out);
  });
}

int sqlrs_hash_join_probe_indices(sqlrs_hash_join_t *j, const sqlrs_batch_t *right, int out_mem,
                                  sqlrs_batch_t **out) {
  return guard(j->ctx, [&] {
    SQ_HIP(hipSetDevice(j->ctx->device));
    if (!j->finished) fail(SQLRS_ERR_INTERNAL, "probe before build_finish");
    j->probe_started = true;
    *out = nullptr;
    if (j->empty_build) return;
    InBatch ib(j->ctx, right);
    Pairs p;
    probe_batch(j, ib, &p);
    DBatch b;
    b.rows = p.m;
    DCol l, r;
    pairs_as_columns(p, &l, &r);
    b.cols.push_back(std::move(l));
    b.cols.push_back(std::move(r));
    *out = emit_batch(j->ctx, std::move(b), out_mem);
  });
}

int sqlrs_hash_join_finish(sqlrs_hash_join_t *j, int out_mem, sqlrs_batch_t **out) {
  return guard(j->ctx, [&] {
    SQ_HIP(hipSetDevice(j->ctx->device));
    if (!j->finished) fail(SQLRS_ERR_INTERNAL, "finish before build_finish");
    *out = nullptr;
    if (j->empty_build) return;
    if (j->join_type != SQLRS_JOIN_LEFT && j->join_type != SQLRS_JOIN_FULL) return;
    Ctx *ctx = j->ctx;
    // the general async probe kernels mark `visited` on the ring's side streams: what is pending is launched and the side
    // streams are waited for — with tickets still outstanding too (their batches stay in their slots until they are waited for)
    if (j->async_ordered) sa_drain(ctx);
    Selection sel = selection_from_clear_bits(ctx, j->visited->as<uint64_t>(), j->nB); // :298-301
    DBatch b;
    b.rows = sel.count;
    for (const DCol &c : j->left.cols) b.cols.push_back(compact_column(ctx, c, sel));
    for (int32_t dt : j->right_dtypes) b.cols.push_back(make_null_column(ctx, dt, sel.count));
    *out = emit_batch(ctx, std::move(b), out_mem);
  });
}

void sqlrs_hash_join_destroy(sqlrs_hash_join_t *j) {
  if (j && j->async_ordered) sa_drain(j->ctx); // (probe kernels of the async path may still read the table on a side stream)
  delete j;
}

} // extern "C"
