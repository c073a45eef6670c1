// prims.hpp — host-callable device primitives shared by the operators.
#pragma once

#include <functional>

#include "common.hpp"

namespace sq {

// ---- scans (scan.hip) --------------------------------------------------------------
// Exclusive prefix sum of n u32 values (single pass, decoupled look-back).  Writes u64
// and/or u32 outputs (either may be null) and the grand total to *total (device u64).
void exclusive_scan_u32(Ctx *ctx, const uint32_t *in, int64_t n, uint64_t *out64, uint32_t *out32,
                        uint64_t *total);

// ---- selections / compaction (select.hip) ------------------------------------------
// A row selection over `rows` rows: bit i of `bits` set = keep row i.  tile_off[t] is the
// number of kept rows before tile t (TILE_ROWS rows per tile); `count` kept rows total.
struct Selection {
  int64_t rows = 0;
  int64_t count = 0;
  const uint64_t *bits = nullptr;
  BufP own_bits;
  BufP tile_off; // u64[num_tiles]
};
// keep rows whose BOOLEAN mask is valid AND true (arrow filter semantics, filter.rs:23)
Selection selection_from_mask(Ctx *ctx, const DCol &mask);
// keep rows whose bit is CLEAR in `bits` (unvisited rows, hash_join.rs:298-301)
Selection selection_from_clear_bits(Ctx *ctx, const uint64_t *bits, int64_t rows);
// keep rows whose bit is SET in `bits` (a copy with the padding bits behind row `rows` cleared: Arrow leaves them unspecified)
Selection selection_from_set_bits(Ctx *ctx, const uint64_t *bits, int64_t rows);
// finishes a Selection whose bits are given (computes tile offsets + count; syncs)
void selection_finish(Ctx *ctx, Selection &s);
DCol compact_column(Ctx *ctx, const DCol &c, const Selection &s);
// u32 row ids of the kept rows
BufP selection_indices_u32(Ctx *ctx, const Selection &s);
BufP selection_indices_u64(Ctx *ctx, const Selection &s);
// range_partition.hip: u32 ids of the set bits of `bits` over `rows` rows into out[tile_off[t] ...) — tile_off = the exclusive
// scan of the kept rows per TILE_ROWS tile; one wave per tile, a tile without a kept row costs one load
void selection_rows_u32(Ctx *ctx, const uint64_t *bits, const uint64_t *tile_off, int64_t rows, uint32_t *out);

// Fused C2 fast path: predicate `col OP constant` + order-preserving compaction of that
// column in one pass.  Returns the Selection (bits + tile offsets) so that further columns
// can be compacted, and the compacted predicate column itself.
bool filter_fast_path(Ctx *ctx, const Expr &e, const std::function<const DCol &(int)> &col,
                      int64_t rows, int *col_index, Selection *sel, DCol *out_col);

// ---- gather (gather.hip) ------------------------------------------------------------
// out[i] = src[idx[i]]; NULL index (idx_validity bit clear) or NULL source row => NULL.
DCol gather_column(Ctx *ctx, const DCol &src, const void *idx, bool idx_is_u64,
                   const uint64_t *idx_validity, int64_t n);
// 2..4 plain 8-byte columns by one u32 permutation, through packed rows (gather.hip); false = shape not taken
bool gather_columns_packed(Ctx *ctx, std::vector<DCol> &cols, int64_t src_rows, const uint32_t *idx, int64_t n);
DCol concat_columns(Ctx *ctx, const std::vector<const DCol *> &parts); // one part: returned as is (no copy)
DCol copy_column(Ctx *ctx, const DCol &c); // deep copy into buffers owned by the result
// ops.hip: stable sort of the rows in `perm` by a Utf8 column (NULL rows tie); keys = n-element scratch
void sort_perm_by_utf8(Ctx *ctx, const DCol &c, const uint64_t *valid, int desc, uint32_t *perm, uint64_t *keys,
                       int64_t n);
// order_topk.hip: the ORDER BY ... LIMIT candidates of a first key of any sortable type (Utf8, NULLs): u32 ids of the rows at
// or below a sampled threshold, in input order; false = a guard ignored the hint (fewer than `limit`, or more than n / 2)
bool order_topk_keys_select(Ctx *ctx, const DCol &key, int desc, int64_t n, int64_t limit, BufP *idx, int64_t *count);
DCol materialize_scalar(Ctx *ctx, const DCol &c, int64_t rows);
// number of clear validity bits among the first `rows` rows
int64_t count_clear_bits(Ctx *ctx, const uint64_t *bits, int64_t rows);

// ---- expressions (expr.hip) ---------------------------------------------------------
// BoundExpr::eval_column (evaluator.rs:13-28).  The result may be a broadcast scalar
// (stride 0) when the expression is a bare constant; pass materialize=true to expand it.
DCol eval_expr(Ctx *ctx, const Expr &e, const std::function<const DCol &(int)> &col, int64_t rows,
               bool materialize);

// ---- whole expressions in one pass (expr_fused.hip; SQLRS_EXPR_FUSED_EVAL) ------------
// The Filter's predicate `e` over `ib` as ONE kernel that writes the selection's mask words; true = `sel` is finished
// (selection_finish ran).  false = the predicate is not a program (nothing launched): the caller takes eval_expr.
bool fused_filter_selection(Ctx *ctx, const Expr &e, InBatch &ib, Selection *sel);
// The computed columns of a projection (every expression that is not a bare InputRef / constant) by the program kernel:
// true = (*out)[i] is column i for every i with (*computed)[i] set, the others are left to the caller.  false = some computed
// column is not a program (nothing launched): the caller takes eval_expr for all of them.
bool fused_project_columns(Ctx *ctx, const std::vector<Expr> &exprs, InBatch &ib, std::vector<DCol> *out, std::vector<uint8_t> *computed);

// ---- key normalisation (keys.hip) ---------------------------------------------------
// Join / group keys as one u64 per row.  Single fixed-width key column: the value itself
// (sign-extended / bit pattern), compared exactly, NULL tracked in `validity`.  Utf8 or
// multi-column keys: a 64-bit hash folded exactly like create_hashes/combine_hashes
// (hash_utils.rs:13-16,161-220: NULL leaves the running hash unchanged) and matched by
// hash only, which is the reference's own matching rule (hash_join.rs:222-232).
struct NKeys {
  int64_t rows = 0;
  BufP keys;                          // u64[rows]
  const uint64_t *validity = nullptr; // exact mode only: NULL key rows
  BufP own_validity;
  bool exact = true;
  int32_t dtype = SQLRS_INT64;        // exact mode: dtype of the single key column
};
NKeys normalize_keys(Ctx *ctx, const std::vector<DCol> &cols, int64_t rows);
// library-internal de-duplication keys: asymmetric strong hash, NULL is a value (keys.hip)
NKeys normalize_keys_strong(Ctx *ctx, const std::vector<DCol> &cols, int64_t rows);

// ---- radix sort (sort.hip) ----------------------------------------------------------
// Stable LSD radix sort of (u64 key, u32 value) pairs on bits [begin_bit, end_bit).
// Results are left in keys/vals (temporaries come from the pool).  `keys_below_end_bit`: the caller guarantees that no
// key has a bit at or above end_bit set (row numbers below a known count) — the question "on which bytes do the keys
// differ" (a pass over the keys + a host round trip) is then not asked: every byte of [begin_bit, end_bit) is sorted.
void radix_sort_pairs(Ctx *ctx, uint64_t *keys, uint32_t *vals, int64_t n, int begin_bit,
                      int end_bit, bool keys_below_end_bit = false);
// perm[0 .. n) = the indices 0 .. n-1 in the stable order of their u32 keys (all below 2^bits)
void radix_sort_index_u32(Ctx *ctx, const uint32_t *keys, int64_t n, int bits, uint32_t *perm);
// The same passes, but the last one writes no permutation: output position g receives the columns of row perm[g] of `rows`,
// 32-byte group rows {key, cell 0, cell 1, first row} (agg_partition.hpp PartAggOutput::grow): key[g] = the key and
// agg[c][g] = cell cell[c] (agg[1] may be null).  COUNT / SUM cells are final as they are stored (agg_finalize_raw copies them).
struct SortedRowsOut {
  const uint64_t *rows = nullptr;
  uint64_t *key = nullptr;
  uint64_t *agg[2] = {nullptr, nullptr};
  int cell[2] = {0, 0};
};
void radix_sort_gather_rows_u32(Ctx *ctx, const uint32_t *keys, int64_t n, int bits, const SortedRowsOut &ro);
void iota_u32(Ctx *ctx, uint32_t *out, int64_t n);
// order_fast.hip: ORDER BY one fixed-width key without NULLs, rows (key, one carried 8-byte column, row id)
// travel through <= 2 HBM passes + an in-LDS finish; false = shape / data do not fit (general path)
bool order_fast(Ctx *ctx, const DCol &key, int desc, const DCol *carry, int64_t n, DCol *key_out, DCol *carry_out,
                BufP *perm, bool want_perm, bool *in_order = nullptr);
// 2..4 plain int64 / int32 key columns, or 1..4 when one has NULLs (NULLs first: a valid bit in front of the value), whose
// fields together fit 64 bits: ordered by one composite key through order_fast; keys_out = the key columns in output order
// (values and validity decoded from the sorted composite).  carry_out stays empty when the
// row ids travelled instead (want_perm with wide composites): the caller gathers that column like the others
bool order_composite(Ctx *ctx, const std::vector<const DCol *> &keys, const std::vector<int> &desc, const DCol *carry, int64_t n,
                     std::vector<DCol> *keys_out, DCol *carry_out, BufP *perm, bool want_perm, bool *in_order);

} // namespace sq
