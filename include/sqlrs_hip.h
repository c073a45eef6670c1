/*
 * sqlrs_hip.h — C ABI of the MI355X (gfx950) execution backend for the sqlrs
 * `src/executor` hot path: Filter -> HashJoin (build + probe) -> HashAgg
 * (update + finalize) -> Order.
 *
 * This is the drop-in boundary.  Every entry point replaces one
 * piece of a reference operator; the reference interface it stands in for is
 * cited as  [ref: file:line]  relative to the sqlrs source tree.
 *
 * Data model = Arrow column buffers, passed as plain pointers + sizes:
 *   - fixed-width columns: `values` = length * sizeof(T) little-endian
 *   - BOOLEAN columns:     `values` = Arrow bitmap (LSB-first), ceil(length/8) B
 *   - UTF8 columns:        `values` = bytes, `offsets` = (length+1) int32, non-decreasing; offsets[0] need not
 *                            be 0, for HOST and DEVICE columns alike: the column is the rows it describes
 *                            (bytes [offsets[0], offsets[length]) of `values`), so `offsets` may point into
 *                            the offsets of a longer array.  Batches the library returns have offsets[0] = 0.
 *   - `validity`           = Arrow validity bitmap (LSB-first) or NULL (= all
 *                            valid); array offset must be 0 (slice on the host)
 *   - `mem`                = where the three pointers live (host or HBM)
 * An arrow-rs `ArrayData` maps 1:1 (buffers()[i].as_ptr(), null_buffer()); the
 * Rust shim a sqlrs maintainer would add is shown in INTEGRATION.md.
 *
 * Threading: one ctx = one HIP stream on one GPU; calls on a ctx are not
 * re-entrant (the reference executor is single-threaded: executor/mod.rs:58-64).
 * Distinct ctxs may be used from distinct threads / processes / GPUs.
 *
 * No CPU fallback exists in this library: without a usable gfx950 device
 * sqlrs_ctx_create fails with SQLRS_ERR_DEVICE.
 *
 * Environment.  Three deployment settings are read when a ctx / operator is created: SQLRS_POOL_RESERVE_GB (one up-front
 * device allocation that the ctx pool carves its blocks from), SQLRS_POOL_VMM=<MiB> (pool blocks of that size and more are
 * backed through hipMemCreate / hipMemMap), SQLRS_JOIN_COMPOSITE=1 (several integer join keys compared exactly instead of
 * by the reference's combined hash).  Every other SQLRS_* name (tools/HOOKS.md) is a test / tuning hook and is looked at
 * only in a process started with SQLRS_HOOKS=1; without it the library never calls getenv on an operator's path.
 */
#ifndef SQLRS_HIP_H
#define SQLRS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- status -- */
/* [ref: src/executor/mod.rs:67-85  enum ExecutorError {Storage, Arrow, InternalError}] */
typedef enum sqlrs_status {
  SQLRS_OK = 0,
  SQLRS_ERR_ARROW = 1,    /* ExecutorError::Arrow          (bad buffers, divide by zero, ...) */
  SQLRS_ERR_INTERNAL = 2, /* ExecutorError::InternalError  (unsupported dtype / shape)        */
  SQLRS_ERR_STORAGE = 3,  /* ExecutorError::Storage        (never produced by this path)      */
  SQLRS_ERR_DEVICE = 4    /* HIP runtime failure / no gfx950 device (no reference analogue)   */
} sqlrs_status_t;

/* ----------------------------------------------------------------- types -- */
/* [ref: src/types/mod.rs:23-36  ScalarValue lattice: Null/Boolean/Float64/Int32/Int64/String]
 * UINT32/UINT64 exist only for the join index pair arrays (hash_join.rs:218-219). */
typedef enum sqlrs_dtype {
  SQLRS_NULLTYPE = 0,
  SQLRS_INT32 = 1,
  SQLRS_INT64 = 2,
  SQLRS_FLOAT64 = 3,
  SQLRS_BOOLEAN = 4,
  SQLRS_UTF8 = 5,
  SQLRS_UINT32 = 6,
  SQLRS_UINT64 = 7
} sqlrs_dtype_t;

typedef enum sqlrs_mem { SQLRS_MEM_HOST = 0, SQLRS_MEM_DEVICE = 1 } sqlrs_mem_t;

/* One Arrow array.  [ref: arrow::array::ArrayRef as used by executor/evaluator.rs:13-28] */
typedef struct sqlrs_column {
  int32_t dtype;           /* sqlrs_dtype_t */
  int32_t mem;             /* sqlrs_mem_t: address space of values/validity/offsets */
  int64_t length;          /* rows */
  int64_t null_count;      /* -1 = unknown (library counts bits when it needs to) */
  const void *values;
  const uint8_t *validity; /* NULL = no nulls */
  const int32_t *offsets;  /* UTF8 only */
} sqlrs_column_t;

/* One RecordBatch.  [ref: arrow::record_batch::RecordBatch, the item type of
 * BoxedExecutor, executor/mod.rs:34].  Batches returned by the library are
 * owned by it until sqlrs_batch_release.  A DEVICE batch returned by the library
 * may be pushed, unchanged, into another operator of the same ctx: an operator
 * that retains its input (join build side, HashAgg) then shares the batch's
 * reference-counted buffers instead of copying them, and sqlrs_batch_release
 * only drops the caller's reference (the Arc<RecordBatch> clone of the reference).
 *
 * Borrowing rules for caller-built batches:
 *   - SQLRS_MEM_HOST columns are read completely before the call returns.
 *   - SQLRS_MEM_DEVICE columns are used STREAM-ORDERED on the ctx stream: the call queues kernels that read
 *     them (and operators that retain input queue a private copy) but does not wait for those kernels.
 *     The buffers must (a) hold their data before the ctx stream reaches the call — data produced on
 *     another stream: sqlrs_ctx_wait_stream(ctx, that_stream) first, or synchronise that stream — and
 *     (b) stay valid and unmodified until the work queued by the call has completed:
 *     sqlrs_ctx_synchronize, or sqlrs_ctx_release_to_stream(ctx, s) before stream s reuses / frees them.
 *     (A stream-ordered allocator on another stream — e.g. torch's caching allocator — may hand a freed
 *     block to later work of ITS stream: order that stream behind the ctx with release_to_stream.)
 *   - A DEVICE column may describe a window of a longer device array: `values` / `validity` advanced to the
 *     window's first row (bitmaps by whole 8-byte words, i.e. a multiple of 64 rows), UTF8 `offsets` advanced
 *     with `values` unchanged.  The library re-bases such offsets on the ctx stream and reads the bytes from
 *     offsets[0] on; both ends of the offsets are fetched under the one synchronisation a DEVICE UTF8 column
 *     already costs.
 *   - Device bitmaps (validity, BOOLEAN values) must be 8-byte aligned and readable up to the next multiple
 *     of 8 bytes (kernels read whole 64-bit words); host bitmaps have no such requirement.
 * Size limit, the same for every operator: 0 <= num_rows < 2^31 per batch (row ids travel as 32-bit words); a batch
 * outside that range is refused by every call that takes one with SQLRS_ERR_ARROW, before any column is read.  Larger
 * inputs arrive as several batches — the reference's own batches are 1024 rows (src/storage/csv.rs:105). */
typedef struct sqlrs_batch {
  int64_t num_rows;
  int32_t num_columns;
  int32_t reserved;
  sqlrs_column_t *columns;
  void *owner; /* private; NULL for caller-built batches */
} sqlrs_batch_t;

/* ----------------------------------------------------------- expressions -- */
/* Postfix encoding of the BoundExpr subset evaluated on this path.
 * [ref: src/executor/evaluator.rs:13-28 (eval_column), src/executor/array_compute.rs:70-90
 *  (binary_op), src/binder/expression/mod.rs:18-27 (BoundExpr)] */
typedef enum sqlrs_expr_op {
  SQLRS_EXPR_INPUT_REF = 1, /* BoundExpr::InputRef  -> column `index`                       */
  SQLRS_EXPR_CONSTANT = 2,  /* BoundExpr::Constant  -> dtype + (i | f | s), is_null         */
  SQLRS_EXPR_TYPE_CAST = 3, /* BoundExpr::TypeCast  -> cast top of stack to `dtype`         */
  /* BoundExpr::BinaryOp, sqlparser BinaryOperator names (array_compute.rs:75-88) */
  SQLRS_EXPR_PLUS = 10,
  SQLRS_EXPR_MINUS = 11,
  SQLRS_EXPR_MULTIPLY = 12,
  SQLRS_EXPR_DIVIDE = 13,
  SQLRS_EXPR_GT = 14,
  SQLRS_EXPR_LT = 15,
  SQLRS_EXPR_GTEQ = 16,
  SQLRS_EXPR_LTEQ = 17,
  SQLRS_EXPR_EQ = 18,
  SQLRS_EXPR_NOTEQ = 19,
  SQLRS_EXPR_AND = 20, /* and_kleene */
  SQLRS_EXPR_OR = 21   /* or_kleene  */
} sqlrs_expr_op_t;

typedef struct sqlrs_expr_node {
  int32_t op;      /* sqlrs_expr_op_t */
  int32_t dtype;   /* CONSTANT: value type; TYPE_CAST: target type */
  int32_t index;   /* INPUT_REF: column index in the input batch */
  int32_t is_null; /* CONSTANT: ScalarValue::X(None) */
  int64_t i;       /* CONSTANT int32/int64/boolean payload */
  double f;        /* CONSTANT float64 payload */
  const char *s;   /* CONSTANT utf8 payload (NUL-terminated), else NULL */
} sqlrs_expr_node_t;

typedef struct sqlrs_expr {
  const sqlrs_expr_node_t *nodes; /* postfix order */
  int32_t num_nodes;
  int32_t reserved; /* 0, or on the first key expression of a blocking operator's create call: SQLRS_EXPR_STAGE_ALL_TYPES (see sqlrs_hash_agg_push);
                     * on the predicate of sqlrs_filter_create / exprs[0] of sqlrs_project_create: SQLRS_EXPR_FUSED_EVAL (see sqlrs_filter_push) */
} sqlrs_expr_t;

/* [ref: src/binder/table/join.rs:18-24  enum JoinType] (Cross never reaches HashJoin:
 *  optimizer/physical_rewriter.rs:20-31) */
typedef enum sqlrs_join_type {
  SQLRS_JOIN_INNER = 0,
  SQLRS_JOIN_LEFT = 1,
  SQLRS_JOIN_RIGHT = 2,
  SQLRS_JOIN_FULL = 3
} sqlrs_join_type_t;

/* [ref: src/binder/expression/agg_func.rs:10-15 AggFunc, :29-34 BoundAggFunc] */
typedef enum sqlrs_agg_kind {
  SQLRS_AGG_COUNT = 0,
  SQLRS_AGG_SUM = 1,
  SQLRS_AGG_MIN = 2,
  SQLRS_AGG_MAX = 3
} sqlrs_agg_kind_t;

typedef struct sqlrs_agg_func {
  int32_t func;         /* sqlrs_agg_kind_t */
  int32_t distinct;     /* BoundAggFunc.distinct */
  int32_t return_dtype; /* BoundAggFunc.return_type (SUM accumulates in this type, sum.rs:54) */
  int32_t reserved;     /* 0, or in sqlrs_simple_agg_create: SQLRS_SIMPLE_AGG_REDUCE (first entry) / SQLRS_SIMPLE_AGG_FILTER (last entry) */
  sqlrs_expr_t arg;     /* BoundAggFunc.exprs[0]  (only exprs[0] is read: hash_agg.rs:65) */
} sqlrs_agg_func_t;

/* [ref: src/binder/statement/mod.rs:26-29  BoundOrderBy {expr, asc}] */
typedef struct sqlrs_order_by {
  sqlrs_expr_t expr;
  int32_t asc;
  int32_t reserved; /* 0, or on the first key of sqlrs_order_create: SQLRS_ORDER_LIMIT_ALL_KEYS (see sqlrs_order_set_limit) */
} sqlrs_order_by_t;

/* ---------------------------------------------------------------- context -- */
typedef struct sqlrs_ctx sqlrs_ctx_t;

/* Opens GPU `device_id`, creates the ctx stream and the device memory pool.
 * Replaces nothing in the reference (it has no device); it is the handle a
 * replacement ExecutorBuilder would hold [ref: src/executor/mod.rs:36-56]. */
int sqlrs_ctx_create(int device_id, sqlrs_ctx_t **out);
/* Operators (and timers) of the ctx must be destroyed first; batches the ctx returned may be released
 * before or after (their device blocks then go straight back to the driver). */
void sqlrs_ctx_destroy(sqlrs_ctx_t *ctx);
/* Message of the last failed call on this ctx (valid until the next call). */
const char *sqlrs_last_error(const sqlrs_ctx_t *ctx);
/* Blocks until all work queued on the ctx stream is done. */
int sqlrs_ctx_synchronize(sqlrs_ctx_t *ctx);
/* The hipStream_t of the ctx as an opaque pointer (event timing, stream ordering by callers). */
void *sqlrs_ctx_stream(sqlrs_ctx_t *ctx);
/* Stream-ordered hand-over of DEVICE buffers without blocking the host (`stream` = a hipStream_t):
 * wait_stream: work queued on the ctx AFTER this call starts only when everything queued on
 *   `producer_stream` BEFORE it has finished (inputs produced there are complete);
 * release_to_stream: work queued on `consumer_stream` AFTER this call starts only when everything queued
 *   on the ctx BEFORE it has finished (borrowed inputs may be reused, outputs may be read there). */
int sqlrs_ctx_wait_stream(sqlrs_ctx_t *ctx, void *producer_stream);
int sqlrs_ctx_release_to_stream(sqlrs_ctx_t *ctx, void *consumer_stream);
/* Bytes currently held by the ctx memory pool (live + cached). */
int64_t sqlrs_ctx_pool_bytes(const sqlrs_ctx_t *ctx);
/* Frees cached (not live) pool blocks back to the driver. */
void sqlrs_ctx_pool_trim(sqlrs_ctx_t *ctx);

/* Releases a batch returned by any call below (host or device resident). */
void sqlrs_batch_release(sqlrs_batch_t *batch);
/* Copies a batch (host or device) into freshly allocated memory of `out_mem`;
 * this is the "Arrow column buffers move to HBM once per pipeline" step. */
int sqlrs_batch_copy(sqlrs_ctx_t *ctx, const sqlrs_batch_t *in, int out_mem, sqlrs_batch_t **out);

/* --------------------------------------------------- Arrow C Data Interface -- */
/* [ref: src/executor/mod.rs:34  BoxedExecutor = BoxStream<'static, Result<RecordBatch, ExecutorError>> — the item every
 *  operator of the reference consumes and yields is an arrow RecordBatch]  The two structs of the Arrow C Data Interface,
 * exactly as the specification defines them (the guard is the specification's own, so this header coexists with
 * arrow/c/abi.h); arrow-rs binds them as arrow::ffi::{FFI_ArrowArray, FFI_ArrowSchema}, pyarrow as _export_to_c /
 * _import_from_c. */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
#define ARROW_FLAG_DICTIONARY_ORDERED 1
#define ARROW_FLAG_NULLABLE 2
#define ARROW_FLAG_MAP_KEYS_SORTED 4
struct ArrowSchema {
  const char *format;
  const char *name;
  const char *metadata;
  int64_t flags;
  int64_t n_children;
  struct ArrowSchema **children;
  struct ArrowSchema *dictionary;
  void (*release)(struct ArrowSchema *);
  void *private_data;
};
struct ArrowArray {
  int64_t length;
  int64_t null_count;
  int64_t offset;
  int64_t n_buffers;
  int64_t n_children;
  const void **buffers;
  struct ArrowArray **children;
  struct ArrowArray *dictionary;
  void (*release)(struct ArrowArray *);
  void *private_data;
};
#endif
/* A RecordBatch exported as a struct array ("+s": what RecordBatch::into / pyarrow's RecordBatch._export_to_c produce) ->
 * a HOST batch of this library WITHOUT copying its buffers: both structures are MOVED into the call (their `release`
 * fields are NULL afterwards, as the specification's move rule says; the schema is released before the call returns, the
 * array when the batch is: sqlrs_batch_release).  Children of type int32 "i", int64 "l", float64 "g", bool "b", utf8 "u";
 * anything else, a dictionary, or NULLs at the struct level: SQLRS_ERR_ARROW and nothing is consumed.  A child whose
 * offset is not a multiple of eight has its bitmaps re-packed (the only copy). */
int sqlrs_batch_import_arrow(sqlrs_ctx_t *ctx, struct ArrowArray *array, struct ArrowSchema *schema, sqlrs_batch_t **out);
/* The reverse: `batch` (produced by this library; HOST or DEVICE resident — device columns are downloaded first) is MOVED
 * into `out_array` / `out_schema` and must not be used or released by the caller afterwards: the consumer's `release`
 * callbacks give the memory back.  `names`: num_columns field names or NULL ("c0", "c1", ...).  A caller-built batch
 * (owner == NULL) is copied, since its buffers are only borrowed. */
int sqlrs_batch_export_arrow(sqlrs_ctx_t *ctx, sqlrs_batch_t *batch, const char *const *names, struct ArrowArray *out_array,
                             struct ArrowSchema *out_schema);

/* ----------------------------------------------------------------- Filter -- */
/* [ref: src/executor/filter.rs:7-25  FilterExecutor{expr, child}::execute]
 * One output batch per input batch, row order preserved, rows whose predicate
 * is false or NULL dropped, empty batches still returned. */
typedef struct sqlrs_filter sqlrs_filter_t;
int sqlrs_filter_create(sqlrs_ctx_t *ctx, const sqlrs_expr_t *expr, sqlrs_filter_t **out);
/* Opt-in, SQLRS_EXPR_FUSED_EVAL in `reserved` of the predicate handed to sqlrs_filter_create, or of exprs[0] handed to
 * sqlrs_project_create (0, the default, leaves every decision as it is; a flag of the create calls like
 * SQLRS_EXPR_STAGE_ALL_TYPES, not a setter: the set of entry points is unchanged): whole expressions are evaluated in one
 * pass.  Results never depend on it.  It affects only sqlrs_filter_push and sqlrs_project_push — the synchronous single-batch
 * calls, HOST or DEVICE input, any out_mem.  *_push_many, *_push_async, sqlrs_eval_expr and the inner Filters of HashAgg /
 * join_agg / the join filter are out of scope and run as without it.
 *
 * Filter: the two existing one-pass routes (`column OP constant`; a conjunction of up to four such terms over int64 / float64
 * columns without NULLs) are tried first, unchanged.  A predicate that then compiles (below) is evaluated row by row by ONE
 * kernel that writes the selection's mask words; tile offsets and the compaction of the columns follow as for any mask.
 * Anything else takes the per-node evaluator as without the flag.
 * Project: a bare column reference and a bare constant keep their handling (a reference shares the input's buffers); every
 * other expression is a computed column.  If every computed column compiles they are evaluated by the program kernel, up to
 * four per launch; if even one does not, the whole push takes the per-node evaluator, so the first error raised is the same.
 * What compiles: int32 / int64 / float64 / boolean columns and constants as operands, an int32 / int64 / float64 / boolean
 * result, at most 24 expression nodes, 8 operands in flight and 16 distinct referenced columns per launch.  utf8 operands,
 * operands of two different types, unsupported casts and longer expressions do not: the per-node evaluator runs and raises
 * whatever there is to raise.  A batch of 0 rows takes the per-node evaluator as well.
 * Results are those without the flag: row order, validity, and the values bit for bit on every valid row (the value under a
 * NULL of a computed column is 0; a computed column always carries a validity bitmap, null_count -1).  A valid row that divides by
 * zero makes the push return SQLRS_ERR_ARROW "Divide by zero error" and no batch; the operator stays usable.
 * Witnesses (sqlrs_ctx_profile_read): "fused_eval_filter_batches" — pushes whose mask the program kernel wrote —
 * and "fused_eval_project_columns" — computed columns it wrote; "expr_binary" / "expr_cast" do not move on such a push. */
#define SQLRS_EXPR_FUSED_EVAL 2
int sqlrs_filter_push(sqlrs_filter_t *f, const sqlrs_batch_t *in, int out_mem, sqlrs_batch_t **out);
/* n iterations of the loop in ONE call: out[i] (n entries) is what sqlrs_filter_push(in[i]) returns — one output batch
 * per input batch, in order, empty ones included [ref: filter.rs:15-24] — for the reference's batch shape, 1024-row
 * HOST batches [ref: src/storage/csv.rs:105]: small HOST batches of fixed-width columns are uploaded together, filtered
 * by one launch sequence and the kept rows of every input batch handed out as a batch of its own (out_mem = HOST); any
 * other input runs through sqlrs_filter_push batch by batch.  On error no output batch is left allocated. */
int sqlrs_filter_push_many(sqlrs_filter_t *f, int n, const sqlrs_batch_t *const *in, int out_mem, sqlrs_batch_t **out);
/* The reference's own calling shape — ONE batch per poll (filter.rs:15-24; 1024 rows, storage/csv.rs:105) — without a stream
 * synchronisation per call: push_async queues the batch and returns a TICKET for the HOST batch sqlrs_filter_push(f, in,
 * SQLRS_MEM_HOST, ..) would have returned; sqlrs_batch_wait(ticket, &out) blocks until that batch exists, hands it out and
 * consumes the ticket (also after an error).  `in` is read completely before push_async returns.  Tickets of one ctx
 * complete in issue order; a caller that waits a few batches behind (the stream adaptor of the Rust / C++ mirrors keeps
 * `depth` tickets in flight) never blocks on the device.  HOST batches of <= 4096 rows and <= 12 int32 / int64 / float64 /
 * utf8 columns under ANY predicate over their int32 / int64 / float64 columns (comparisons, + - * / with the evaluator's wrapping
 * and its "Divide by zero error" — reported by sqlrs_batch_wait of that ticket —, casts between the three types, NULL
 * constants, AND / OR; <= 24 expression nodes) share ONE launch with up to three neighbours and take no copy call (pinned,
 * device-mapped ring); every other batch (DEVICE input, more rows or columns, and — unless
 * sqlrs_filter_set_async_all_types is on, below — a predicate that reads a utf8 / boolean column or a batch that carries a
 * boolean column) runs the synchronous operator inside push_async: same batches, no speed-up.  Tickets must be waited for
 * before their ctx is destroyed. */
typedef struct sqlrs_ticket sqlrs_ticket_t;
int sqlrs_filter_push_async(sqlrs_filter_t *f, const sqlrs_batch_t *in, sqlrs_ticket_t **ticket);
/* on != 0: the one-launch path of sqlrs_filter_push_async takes every column type.  Default 0: exactly the behaviour
 * described above.  f == NULL: SQLRS_ERR_INTERNAL.  May be called at any time between calls on the filter and affects the
 * batches pushed afterwards; results never depend on it (the stream of HOST batches is the synchronous operator's, batch
 * for batch; "Divide by zero error" still arrives at the wait of its own ticket), so there is no ordering rule.
 *
 * With the switch on the predicate may also read
 *   - utf8 columns and utf8 constants (the empty string and a NULL constant included), as operands of the six comparisons
 *     against another utf8 operand: bytes compare unsigned and lexicographically, a proper prefix is less, a NULL operand
 *     gives NULL.  A utf8 cast, utf8 arithmetic or a utf8 result is not a program: the synchronous evaluator runs and
 *     raises whatever there is to raise.  The utf8 constants of one expression may total at most 1024 bytes; more runs the
 *     synchronous operator;
 *   - boolean columns, as operands of comparisons (false < true) and of AND / OR, as the source of a cast to int32 / int64 /
 *     float64, or as the whole predicate (WHERE p);
 * and the batch may carry boolean columns (compacted like a validity bitmap).  What still sends a HOST batch to the
 * synchronous operator is size alone: more than 4096 rows, 12 columns, 24 expression nodes or 8 operands in flight, more
 * than 1024 bytes of utf8 constants, columns (plus constants) that do not fit the 512 KiB of a ring slot's input or output
 * area, comparison operands of two different types.  A batch with nothing of this in it takes the same kernel as with
 * the switch off. */
int sqlrs_filter_set_async_all_types(sqlrs_filter_t *f, int on);
int sqlrs_batch_wait(sqlrs_ticket_t *ticket, sqlrs_batch_t **out);
void sqlrs_filter_destroy(sqlrs_filter_t *f);

/* Evaluates one expression on a batch -> one-column batch.
 * [ref: src/executor/evaluator.rs:13-28  BoundExpr::eval_column] */
int sqlrs_eval_expr(sqlrs_ctx_t *ctx, const sqlrs_expr_t *expr, const sqlrs_batch_t *in,
                    int out_mem, sqlrs_batch_t **out);

/* --------------------------------------------------------------- HashJoin -- */
/* [ref: src/executor/join/hash_join.rs:16-23  HashJoinExecutor{left_child, right_child,
 *  join_type, join_condition, join_output_schema}; execute :146-323]
 * left = build side, right = probe side (hash_join.rs:162,208). */
typedef struct sqlrs_hash_join sqlrs_hash_join_t;
int sqlrs_hash_join_create(sqlrs_ctx_t *ctx, int join_type, int num_keys,
                           const sqlrs_expr_t *left_keys,  /* JoinCondition::On.on[i].0 */
                           const sqlrs_expr_t *right_keys, /* JoinCondition::On.on[i].1 */
                           const sqlrs_expr_t *filter,     /* JoinCondition::On.filter or NULL */
                           int num_right_columns,          /* right part of join_output_schema */
                           const int32_t *right_dtypes,    /* (types of the all-NULL tail columns) */
                           sqlrs_hash_join_t **out);
/* build phase, one call per left batch  [ref: hash_join.rs:161-181] */
int sqlrs_hash_join_build_push(sqlrs_hash_join_t *j, const sqlrs_batch_t *left);
/* end of left stream: concat + finish the table  [ref: hash_join.rs:183-187] */
int sqlrs_hash_join_build_finish(sqlrs_hash_join_t *j);
/* probe phase, one call per right batch -> one joined batch (possibly 0 rows).
 * If the build side received no batch, *out = NULL ("emit nothing", hash_join.rs:183-185).
 * [ref: hash_join.rs:207-292] */
int sqlrs_hash_join_probe_push(sqlrs_hash_join_t *j, const sqlrs_batch_t *right, int out_mem,
                               sqlrs_batch_t **out);
/* n probe batches in ONE call: out[i] (n entries) is what sqlrs_hash_join_probe_push(right[i]) returns — one joined batch
 * per probe batch, in order [ref: hash_join.rs:207-292] — for the reference's batch shape, 1024-row HOST batches
 * [ref: src/storage/csv.rs:105]: Inner / Left joins without a join filter over small HOST batches of fixed-width columns
 * are probed as one batch (pairs are probe-row major, hash_join.rs:225-234: every input batch's joined rows are one
 * contiguous range) and cut back into n HOST batches; anything else runs batch by batch.  On error no output batch is
 * left allocated. */
int sqlrs_hash_join_probe_push_many(sqlrs_hash_join_t *j, int n, const sqlrs_batch_t *const *right, int out_mem,
                                    sqlrs_batch_t **out);
/* sqlrs_hash_join_probe_push without the wait (see sqlrs_filter_push_async; hash_join.rs:207-292 polled one batch at a
 * time): the fast path takes Inner joins without a join filter over ONE exactly compared INPUT_REF key (int32 / int64 /
 * float64, no NULL probe keys), unique build keys and fixed-width columns on both sides; *out of the wait is NULL for an
 * empty build side, as for probe_push. */
int sqlrs_hash_join_probe_push_async(sqlrs_hash_join_t *j, const sqlrs_batch_t *right, sqlrs_ticket_t **ticket);
/* on != 0: sqlrs_hash_join_probe_push_async also serves, in one launch per batch, Left / Right / Full joins and build
 * sides with duplicate keys (below).  Default 0: exactly today's behaviour.  Call after sqlrs_hash_join_create and before
 * the first probe call of any kind (later: SQLRS_ERR_INTERNAL).  The contract of probe_push_async is unchanged: the
 * ticket stands for the HOST batch sqlrs_hash_join_probe_push(j, right, SQLRS_MEM_HOST, ..) would have returned.
 *
 * Eligibility of a probe batch with the switch on.  Everything the fast path above requires except "Inner" and "unique
 * build keys": no join filter; ONE exactly compared INPUT_REF key of int32 / int64 / float64 (no composite key, no
 * match-by-hash); no NULL probe key in the batch; HOST input of at most 4096 rows; int32 / int64 / float64 columns on
 * both sides, at most 12 output columns; a free ring slot.  In place of the two dropped conditions, the OUTPUT BOUND: let
 * M be the largest number of build rows that share one key (1 for unique build keys; build rows with a NULL key count as
 * sharing one key) — a batch of `rows` rows emits at most rows x M joined rows (a Right / Full probe row without a
 * partner emits one) — and the batch is eligible iff
 *   rows x M <= 16384 (SA_MAX_OUT_ROWS), and
 *   64 + sum over the output columns of (round64(width x rows x M) + round64(ceil(rows x M / 8))) <= 524288 (SA_AREA):
 *   the 64-byte header, every output column (width 4 or 8) and its validity bitmap laid out for rows x M rows, each
 *   piece rounded up to 64 bytes — and the staged input, round64(width x rows) per probe column plus
 *   round64(ceil(rows / 8) + 8) per probe column with NULLs, fits 524288 bytes as well (it always does at <= 4096 rows
 *   and <= 12 columns).
 * M is computed once per join (one small kernel, one fetch) when it is first needed.  The decision is made on the host
 * before a slot is taken; there is no overflow and no re-run.  An Inner join over unique build keys keeps the kernel of
 * the fast path above.  Every other batch — join filters, Utf8 / Boolean columns on either side, DEVICE input, more than
 * 4096 rows, the bound exceeded, and (unless sqlrs_hash_join_set_async_keys is on, below) NULL probe keys, Utf8 keys and
 * keys of several columns — runs the synchronous operator
 * inside push_async, as with the switch off.  Left / Full: sqlrs_hash_join_finish may be called with tickets still
 * outstanding; it waits for the queued probe kernels (which mark the visited build rows) before it reads the marks. */
int sqlrs_hash_join_set_async_general(sqlrs_hash_join_t *j, int on);
/* on != 0: both one-launch kernels of sqlrs_hash_join_probe_push_async also carry Utf8 PAYLOAD columns, on the build side
 * and in the probe batch.  Default 0: exactly today's behaviour.  Calling rules as for sqlrs_hash_join_set_async_general
 * (after create, before the first probe call of any kind; later: SQLRS_ERR_INTERNAL); the contract of probe_push_async is
 * unchanged.  The key column stays int32 / int64 / float64.
 *
 * Eligibility of a probe batch with the switch on: every condition of the fast path of probe_push_async — or of the
 * general path above when sqlrs_hash_join_set_async_general is on as well — except "fixed-width columns only": any
 * non-key column of the build side or of the probe batch may be Utf8.  A Utf8 column of the probe batch has non-NULL
 * `offsets`, offsets[rows] >= offsets[0], and non-NULL `values` when that range is not empty.  Let out_rows = rows on the
 * Inner / unique route and rows x M on the general route; the batch is eligible iff out_rows <= 16384 and
 *   64 + sum over the output columns of piece(c) <= 524288 (SA_AREA), where
 *     a fixed-width column: round64(width x out_rows) + round64(ceil(out_rows / 8)), as above;
 *     a Utf8 column: round64(4 x (out_rows + 1)) + round64(ceil(out_rows / 8)) + round64(bytes_c), with
 *       bytes_c = out_rows x Lmax_c for a build column — Lmax_c the largest offsets[i + 1] - offsets[i] of that build
 *       column, NULL slots included — and
 *       bytes_c = B_c x (out_rows / rows) for a probe column, B_c = offsets[rows] - offsets[0] (the factor is 1 or M; a
 *       0-row batch has 0 bytes),
 *   and the staged input fits 524288 bytes: per probe column round64(width x rows), for Utf8
 *   round64(4 x (rows + 1)) + round64(B_c), plus round64(ceil(rows / 8) + 8) per column with NULLs.
 * Lmax_c is computed once per join (one small kernel over the build column's offsets and one fetch) when it is first
 * needed.  The host decides before it takes a slot; nothing overflows and nothing is re-run (the kernels compare every
 * column's bytes with its reservation before they store one, and sqlrs_batch_wait reports SQLRS_ERR_INTERNAL should that
 * ever fail).  Everything else — the bound exceeded, Boolean columns, a Utf8 key (unless sqlrs_hash_join_set_async_keys is
 * on as well), and the rest of the lists above — runs
 * the synchronous operator inside push_async, as with the switch off. */
int sqlrs_hash_join_set_async_utf8(sqlrs_hash_join_t *j, int on);
/* on != 0: both one-launch kernels of sqlrs_hash_join_probe_push_async also serve a join that HAS a join filter
 * (JoinCondition::On { on, filter }): the filter is evaluated on the joined row inside the kernel, with
 * apply_join_filter's semantics (hash_join.rs:47-127).  Default 0: exactly today's behaviour (a filtered join takes no
 * fast batch).  Calling rules as for sqlrs_hash_join_set_async_general (after create, before the first probe call of any
 * kind; later: SQLRS_ERR_INTERNAL; j == NULL: SQLRS_ERR_INTERNAL); the contract of probe_push_async is unchanged.  A join
 * without a filter is not affected by the switch.
 *
 * Eligibility of a probe batch of a join that has a filter, with the switch on: every condition the batch would have to
 * meet without the filter, except "no join filter" — the Inner / unique-build-keys fast path; or the general path when
 * sqlrs_hash_join_set_async_general is on; with Utf8 payload columns when sqlrs_hash_join_set_async_utf8 is on — and the
 * same OUTPUT BOUND with the same formulas, taken over the CANDIDATES, rows x M: the filter never makes a batch emit more
 * rows than it has candidates (a Right / Full probe row emits max(passing pairs, 1) <= max(matches, 1) rows).  In
 * addition the FILTER MUST COMPILE for the in-kernel evaluator, over the joined schema (the build side's columns, then
 * the num_right_columns right_dtypes given to sqlrs_hash_join_create): at most 24 nodes, an evaluation stack of at most
 * 8; every referenced column int32 / int64 / float64; constants int32 / int64 / float64 / Boolean (NULL allowed); casts
 * between those types; both operands of an arithmetic or comparison node of one type; a Boolean result — the rule of
 * sqlrs_filter_push_async's general predicates.  It is compiled once per join; a probe batch whose column dtypes are not
 * right_dtypes is not eligible.  A filter that does not compile (it reads a Utf8 / Boolean column, is too long, mixes
 * operand types) runs the synchronous operator inside push_async, as with the switch off.
 *
 * Semantics, bit for bit those of the synchronous operator.  Inner / Left: the candidates are the matched pairs (probe-row
 * major, build insertion order minor); a pair is kept iff the filter is valid and TRUE on it (NULL drops it).  Right /
 * Full: the candidates also hold one (NULL, r) row per probe row r without partner, the filter is evaluated on those too
 * (every build column NULL); the batch is the kept candidates in candidate order, followed by one (NULL, r) row for every
 * probe row that appears in no kept candidate, in ascending r.  Left / Full: only build rows of KEPT pairs count as
 * visited for the tail batch of sqlrs_hash_join_finish.  A valid candidate row that divides by zero makes that ticket's
 * sqlrs_batch_wait return SQLRS_ERR_ARROW "Divide by zero error"; the batch marks no build row visited, later tickets
 * are unaffected. */
int sqlrs_hash_join_set_async_filter(sqlrs_hash_join_t *j, int on);
/* on != 0: both one-launch kernels of sqlrs_hash_join_probe_push_async load the KEY of a probe row themselves: NULL probe
 * keys, Utf8 keys and keys of 2 to 4 columns take a kernel too.  Default 0: exactly today's behaviour.  Calling rules as
 * for sqlrs_hash_join_set_async_general (after create, before the first probe call of any kind; later: SQLRS_ERR_INTERNAL;
 * j == NULL: SQLRS_ERR_INTERNAL); it composes with the three switches above; the contract of probe_push_async is unchanged
 * (the ticket stands for the HOST batch sqlrs_hash_join_probe_push would have returned, bit for bit, the visited marks
 * behind the Left / Full tail included).
 *
 * Eligibility of a probe batch with the switch on: every condition of the fast path of probe_push_async — or of the
 * general path when sqlrs_hash_join_set_async_general is on; with Utf8 payload columns when
 * sqlrs_hash_join_set_async_utf8 is on; with a join filter when sqlrs_hash_join_set_async_filter is on — except "ONE
 * exactly compared INPUT_REF key of int32 / int64 / float64" and "no NULL probe key in the batch".  In their place:
 *   KEY COUNT AND TYPE: the join has 1 to 4 key pairs, and every right key expression is a bare INPUT_REF to a column of
 *   the batch of dtype int32 / int64 / float64 / Utf8;
 *   UTF8 KEYS: a Utf8 key column needs sqlrs_hash_join_set_async_utf8 on as well — it travels as the payload column it
 *   already is, under that switch's conditions on `offsets` / `values` and its byte bounds;
 *   NULLS: probe key columns may hold NULLs.
 * A join over ONE fixed-width key is compared exactly, as before: the batch's key column has the build key's dtype (any
 * other stays with the synchronous operator, which refuses it), and a NULL probe key finds the build rows whose key is
 * NULL (hash_utils.rs:91-104).  A Utf8 key and keys of 2 to 4 columns are matched BY HASH: the kernel computes, per probe
 * row, the 64-bit value the synchronous operator computes (a NULL column leaves the running hash alone; a value is hashed
 * under its own column's dtype, so an int32 probe column against an int64 build column finds nothing) and looks it up —
 * the synchronous route's rule and the reference's (hash_join.rs:222-232), false matches by hash collision included.
 * Everything else is unchanged: the Inner / unique route versus the general route, the output bound rows x M (M counts
 * NULL-key build rows as sharing one key; for hashed keys, build rows that share one hash), the byte bounds, the
 * filter's compile rule.  Still synchronous: Boolean keys, key expressions that are not bare column references, more
 * than four key columns, the opt-in composite key (SQLRS_JOIN_COMPOSITE=1), and the rest of the lists above. */
int sqlrs_hash_join_set_async_keys(sqlrs_hash_join_t *j, int on);
/* The index-pair form of one probe batch, before any gather: 2 columns
 * (UINT64 left index, nullable; UINT32 right index), in the reference's order
 * (probe-row major, build insertion order minor), join filter NOT applied.
 * [ref: hash_join.rs:218-253  left_indices / right_indices] */
int sqlrs_hash_join_probe_indices(sqlrs_hash_join_t *j, const sqlrs_batch_t *right, int out_mem,
                                  sqlrs_batch_t **out);
/* end of right stream: the unvisited-left tail batch for Left/Full (always a
 * batch, possibly 0 rows), *out = NULL for Inner/Right or an empty build side.
 * [ref: hash_join.rs:296-322] */
int sqlrs_hash_join_finish(sqlrs_hash_join_t *j, int out_mem, sqlrs_batch_t **out);
void sqlrs_hash_join_destroy(sqlrs_hash_join_t *j);

/* ---------------------------------------------------------------- HashAgg -- */
/* [ref: src/executor/aggregate/hash_agg.rs:15-19  HashAggExecutor{agg_funcs, group_by, child};
 *  execute :32-150; accumulators aggregate/{count,sum,min_max}.rs]
 * Output = one batch [group keys..., aggs...], groups in first-seen order.
 * COUNT accumulates across batches (the reference assigns, count.rs:22: see DESIGN.md). */
typedef struct sqlrs_hash_agg sqlrs_hash_agg_t;
int sqlrs_hash_agg_create(sqlrs_ctx_t *ctx, int num_group_by, const sqlrs_expr_t *group_by,
                          int num_aggs, const sqlrs_agg_func_t *aggs, sqlrs_hash_agg_t **out);
/* [ref: hash_agg.rs:44-122]
 * BLOCKING operators (this one, sqlrs_join_agg_probe_push, sqlrs_order_push, sqlrs_hash_join_build_push) decide when
 * to work: small HOST batches of fixed-width columns — the reference's 1024-row CSV batches — are appended to a host
 * staging area (one memcpy) and uploaded together once per 2^22 rows or at *_finish; device batches are staged by
 * reference.  Consequence for error reporting: an error that only the evaluation of a batch reveals (an expression
 * over a column of the wrong type, "Divide by zero error", a schema that differs from the first batch's) is returned
 * by the call that works on the staged rows — a LATER push or *_finish — not necessarily by the push that delivered
 * the batch; the operator is unusable after an error either way (destroy it), exactly like the reference's stream,
 * which ends at its first Err.  A wide aggregate list (more than two argument columns) runs as several internal
 * operators that each see every batch.
 *
 * Opt-in, SQLRS_EXPR_STAGE_ALL_TYPES in `reserved` of the FIRST key expression handed to the create call — group_by[0] of
 * sqlrs_hash_agg_create, left_keys[0] of sqlrs_hash_join_create, left_keys[0] of sqlrs_join_agg_create (its probe-side stage
 * and the build side it owns), order_by[0].expr of sqlrs_order_create; 0, the default, leaves every decision as it is, and
 * an aggregate without GROUP BY has no place for the flag: the staging area also takes small HOST batches with Utf8 and
 * Boolean columns and with NULLs — what every table of the reference's own tests holds.  A batch is staged when it has at
 * most 2^20 rows, every column is Int32 / Int64 / Float64 / Boolean / Utf8 (or an unsigned fixed-width type) of the staged
 * schema's type, and every Utf8 column has offsets with 0 <= offsets[0] <= offsets[num_rows]; any other batch flushes the
 * stage and is handled as without the flag, with the same status and message.  A push copies the batch's buffers as they are
 * (no loop over rows); the flush — per 2^22 rows, before any Utf8 column would hold more than 2^30 staged bytes, or at
 * *_finish — uploads every staged array once and builds each offsets array and bitmap with one kernel launch.  Results are
 * those without the flag, bit for bit.  The caller's null_count is not trusted (it may be -1): the NULLs are counted on the
 * staged validity bytes.  The error-reporting consequence above now applies to these batches too, which is why this is a
 * flag.  sqlrs_ctx_profile_read reports the batches staged this way as "stage_all_types_batches" and the flushes that ran the
 * kernels as "stage_stitch_flushes". */
#define SQLRS_EXPR_STAGE_ALL_TYPES 1
int sqlrs_hash_agg_push(sqlrs_hash_agg_t *a, const sqlrs_batch_t *in);
/* [ref: hash_agg.rs:124-149]; with no pushed batch the reference panics (:125):
 * here that is SQLRS_ERR_INTERNAL. */
int sqlrs_hash_agg_finish(sqlrs_hash_agg_t *a, int out_mem, sqlrs_batch_t **out);
/* Group order of the output batch.  SQLRS_GROUP_ORDER_FIRST_SEEN (default) is the reference's
 * (hash_agg.rs:98,132).  SQLRS_GROUP_ORDER_ANY is for PARTIAL aggregates that are exchanged and
 * merged again (multi-GPU): the sort of the groups by first row and the gathers
 * that follow it are skipped; the set of groups and every value are unchanged. */
#define SQLRS_GROUP_ORDER_FIRST_SEEN 0
#define SQLRS_GROUP_ORDER_ANY 1
int sqlrs_hash_agg_set_group_order(sqlrs_hash_agg_t *a, int group_order);
/* A FilterExecutor sitting directly below the operator — PhysicalHashAgg(PhysicalFilter(child)), the shape of
 * `SELECT k, sum(v) FROM t WHERE t.col > c GROUP BY k` [ref: filter.rs:13-25 feeding hash_agg.rs:44].  `filter`
 * indexes the columns of the pushed batches.  Results are identical to sqlrs_filter_push on every batch followed
 * by sqlrs_hash_agg_push of its output (groups in first-seen order of the FILTERED rows).  When the predicate is
 * `column OP constant` over an int64 / float64 column without NULLs, the batch is one that is aggregated in
 * place (>= 2^26 rows, first batch) and neither the keys nor the aggregate arguments contain a division, the
 * first partition pass evaluates the predicate itself (no filtered copy of any column is written); otherwise
 * the library runs the Filter operator first.  Must be called before the first batch; NULL / empty = none. */
int sqlrs_hash_agg_set_filter(sqlrs_hash_agg_t *a, const sqlrs_expr_t *filter);
/* batches whose filter was evaluated inside the first partition pass (diagnostics / tests) */
int64_t sqlrs_hash_agg_filter_fused_batches(const sqlrs_hash_agg_t *a);
void sqlrs_hash_agg_destroy(sqlrs_hash_agg_t *a);

/* ------------------------------------------------------------------ Order -- */
/* [ref: src/executor/order.rs:8-67  OrderExecutor{order_by, child}::execute]
 * NULLs first (SortOptions::default().nulls_first, order.rs:37-40), stable. */
typedef struct sqlrs_order sqlrs_order_t;
int sqlrs_order_create(sqlrs_ctx_t *ctx, int num_keys, const sqlrs_order_by_t *order_by,
                       sqlrs_order_t **out);
int sqlrs_order_push(sqlrs_order_t *o, const sqlrs_batch_t *in);
/* The reference's Order keeps the child's batches themselves (order.rs:19-26: Arc'd arrays in a Vec, no copy).
 * sqlrs_order_push must copy device columns it does not own, because a batch is only borrowed for the call
 * (1.6 GB, 0.64 ms for 1e8 rows x 2 columns); with this entry point the CALLER keeps every buffer of `in` alive
 * and unchanged until sqlrs_order_finish has returned (or the operator is destroyed), the stream rules of
 * sqlrs_batch_t apply until then, and nothing is copied.  Host columns are uploaded as usual. */
int sqlrs_order_push_retained(sqlrs_order_t *o, const sqlrs_batch_t *in);
int sqlrs_order_finish(sqlrs_order_t *o, int out_mem, sqlrs_batch_t **out);
/* ORDER BY ... LIMIT k — PhysicalLimit(PhysicalOrder(child)) [ref: limit.rs:12-80 slicing what order.rs:27-66 sorted]:
 * the caller promises to read only the first `rows` (= offset + limit) rows of the result.  sqlrs_order_finish may then
 * return a PREFIX of the sorted result with at least `rows` rows (or everything): it keeps the rows whose key cannot be
 * beyond position `rows` — a threshold from a sample of the keys, ties at the threshold included — and sorts only those,
 * so the prefix is exactly what the full sort would put first, stable ties and all.  Applies when the FIRST key is a plain
 * fixed-width column without NULLs (the threshold is taken on it; further keys only order the candidates) and `rows` is a
 * small part of the input; ignored otherwise (0 = no hint).  The LimitExecutor above
 * slices either result the same way. */
int sqlrs_order_set_limit(sqlrs_order_t *o, int64_t rows);
/* Opt-in, SQLRS_ORDER_LIMIT_ALL_KEYS in `reserved` of the FIRST sqlrs_order_by_t handed to sqlrs_order_create (0, the
 * default, leaves every decision of sqlrs_order_finish as it is): the hint of sqlrs_order_set_limit — under the same
 * conditions on `rows` and the input size — also applies when the FIRST key is an Int32 / Int64 / Float64 column WITH NULLs,
 * a Utf8 column (with or without NULLs), or an expression that is not a bare column reference and evaluates to one of those
 * types (evaluated once over the whole input; an evaluation error is the one the full sort raises, same status and text).
 * The contract is the same: the caller reads only the first `rows` rows; the result is a PREFIX of the full sorted result
 * with at least `rows` rows, or everything; ties are stable and NULLs come first in either direction.  The threshold is a
 * sampled row of the first key; a row is compared with it through a weak image — NULL below every valid row, a fixed-width
 * key its value, a Utf8 key its first 64 bytes (zero padded) — and rows that tie with the threshold's image are kept, so no
 * row that belongs to the prefix is lost.  The hint is ignored (everything is sorted) when fewer than `rows` rows qualify or
 * more than half of the input does.  A Boolean first key, a constant first key and a first key sqlrs_order_set_limit serves
 * by itself keep their routes.  (A flag of the create call, not an entry point of its own: the set of functions is
 * unchanged.) */
#define SQLRS_ORDER_LIMIT_ALL_KEYS 1
/* rows the last finish sorted because of the hint; 0 = the hint did not apply (diagnostics / tests) */
int64_t sqlrs_order_topk_candidates(const sqlrs_order_t *o);
void sqlrs_order_destroy(sqlrs_order_t *o);

/* ---------------------------------------------------- HashJoin + HashAgg fused -- */
/* A HashAggExecutor sitting directly on an Inner HashJoinExecutor without join filter
 * [ref: hash_agg.rs:32-150 consuming hash_join.rs:146-323] — what a physical rewrite of
 * PhysicalHashAgg(PhysicalHashJoin(left, right)) instantiates.  Results are identical to running
 * the two operators back to back: group_by / aggregate argument expressions index the JOIN
 * OUTPUT schema (left columns, then right columns), groups come out in first-seen order of the
 * join output.  When the join has one exactly-compared key with unique build keys, the group key
 * is that key and the aggregate arguments only read probe-side columns, the joined batch is never
 * materialised (probe rows are partitioned once, each LDS bucket table is pre-filled with the
 * build keys); otherwise the library composes the two operators on the device itself. */
typedef struct sqlrs_join_agg sqlrs_join_agg_t;
int sqlrs_join_agg_create(sqlrs_ctx_t *ctx, int num_keys, const sqlrs_expr_t *left_keys,
                          const sqlrs_expr_t *right_keys, int num_left_columns, int num_right_columns,
                          const int32_t *right_dtypes, int num_group_by, const sqlrs_expr_t *group_by,
                          int num_aggs, const sqlrs_agg_func_t *aggs, sqlrs_join_agg_t **out);
int sqlrs_join_agg_build_push(sqlrs_join_agg_t *ja, const sqlrs_batch_t *left);
int sqlrs_join_agg_build_finish(sqlrs_join_agg_t *ja);
int sqlrs_join_agg_probe_push(sqlrs_join_agg_t *ja, const sqlrs_batch_t *right);
int sqlrs_join_agg_finish(sqlrs_join_agg_t *ja, int out_mem, sqlrs_batch_t **out);
int sqlrs_join_agg_set_group_order(sqlrs_join_agg_t *ja, int group_order); /* see sqlrs_hash_agg_set_group_order */
/* probe inputs that took the non-materialising route so far (small probe batches are staged and
 * processed together: they count once) */
int64_t sqlrs_join_agg_fused_batches(const sqlrs_join_agg_t *ja);
/* A FilterExecutor sitting directly below the probe side — PhysicalHashAgg(PhysicalHashJoin(left,
 * PhysicalFilter(right))), the shape of `... FROM fact JOIN dim ... WHERE fact.col > k GROUP BY ...`
 * [ref: filter.rs:13-25 feeding hash_join.rs:207].  `filter` indexes the PROBE batch's columns.  Results
 * are identical to sqlrs_filter_push on every probe batch followed by sqlrs_join_agg_probe_push of its
 * output; when the predicate is `column OP constant` over an int64 / float64 column without NULLs and the
 * non-materialising route applies, the first partition pass evaluates it itself (the filtered copies of
 * the probe columns are never written), otherwise the library runs the Filter operator first.  Must be
 * called before the first probe batch; NULL / empty removes the filter. */
int sqlrs_join_agg_set_probe_filter(sqlrs_join_agg_t *ja, const sqlrs_expr_t *filter);
/* probe batches whose filter was evaluated inside the first partition pass (diagnostics / tests) */
int64_t sqlrs_join_agg_filter_fused_batches(const sqlrs_join_agg_t *ja);
/* GROUP BY over columns of the BUILD side (`... FROM fact JOIN dim ON fact.k = dim.k GROUP BY dim.region`,
 * PhysicalHashAgg over PhysicalHashJoin with group_by = InputRefs below num_left_columns) with unique build keys:
 * every build column is a function of the join key, so the operator groups the probe rows by JOIN KEY first (its
 * non-materialising route), finds the build row of every distinct key once, and re-aggregates those partial rows by
 * the requested columns (COUNT -> sum of counts; SUM / MIN / MAX of partials).  Same groups, same first-seen group
 * order [ref: hash_agg.rs:98] and the same aggregates as HashAgg over the materialised join [ref: hash_join.rs:284-291
 * feeding hash_agg.rs:44-122]; SUM(double) within the summation-order tolerance.  Returns the number of partial
 * groups (distinct join keys) the last finish re-aggregated; 0 = the route did not run (diagnostics / tests). */
int64_t sqlrs_join_agg_eager_groups(const sqlrs_join_agg_t *ja);
void sqlrs_join_agg_destroy(sqlrs_join_agg_t *ja);

/* ---------------------------------------- operators either side of the hot path -- */
/* [ref: src/executor/project.rs:6-29  ProjectExecutor{exprs, child}]  One output batch per input batch,
 * column i = exprs[i].eval_column(batch). */
typedef struct sqlrs_project sqlrs_project_t;
int sqlrs_project_create(sqlrs_ctx_t *ctx, int num_exprs, const sqlrs_expr_t *exprs, sqlrs_project_t **out);
int sqlrs_project_push(sqlrs_project_t *p, const sqlrs_batch_t *in, int out_mem, sqlrs_batch_t **out);
/* n input batches in ONE call: out[i] (n entries) is what sqlrs_project_push(in[i]) returns — one output batch per input
 * batch, in order [ref: project.rs:15-27] — for the reference's batch shape, 1024-row HOST batches
 * [ref: src/storage/csv.rs:105]: small HOST batches of fixed-width columns are uploaded together and projected by one
 * launch sequence (an expression's row i depends on row i alone); anything else runs batch by batch.  On error no output
 * batch is left allocated. */
int sqlrs_project_push_many(sqlrs_project_t *p, int n, const sqlrs_batch_t *const *in, int out_mem, sqlrs_batch_t **out);
/* sqlrs_project_push without the wait (see sqlrs_filter_push_async; project.rs:15-27 polled one batch at a time): the fast
 * path takes HOST batches of <= 4096 rows whose output columns are bare column references (int32 / int64 / float64 /
 * boolean / utf8) or expressions over int32 / int64 / float64 columns with an int32 / int64 / float64 / boolean result
 * (<= 6 computed columns, <= 12 columns in and out); sqlrs_batch_wait reports a division by zero of that batch.  An
 * expression that reads a utf8 / boolean column runs the synchronous operator inside push_async unless
 * sqlrs_project_set_async_all_types is on. */
int sqlrs_project_push_async(sqlrs_project_t *p, const sqlrs_batch_t *in, sqlrs_ticket_t **ticket);
/* on != 0: the computed columns of sqlrs_project_push_async may read utf8 and boolean columns and utf8 constants, under the
 * rules of sqlrs_filter_set_async_all_types (utf8 only as comparison operands, <= 1024 bytes of utf8 constants per
 * expression, boolean columns in comparisons, AND / OR and casts; a computed column is still int32 / int64 / float64 /
 * boolean).  Default 0: exactly the behaviour described above.  p == NULL: SQLRS_ERR_INTERNAL.  May be called at any time
 * between calls on the projection; affects the batches pushed afterwards, never their contents. */
int sqlrs_project_set_async_all_types(sqlrs_project_t *p, int on);
void sqlrs_project_destroy(sqlrs_project_t *p);

/* [ref: src/executor/limit.rs:4-81  LimitExecutor{limit, offset, child}]  limit / offset are the constants
 * of the two BoundExpr::Constant (has_* = 0: None).  One call per child batch, in stream order, with the
 * reference's arithmetic across batches: *out = NULL when the batch contributes nothing, otherwise the
 * batch itself or its slice; *done = 1 once no later batch can contribute (the reference `break`s, or
 * returned before polling the child when limit = 0) — the caller stops pulling the child then. */
typedef struct sqlrs_limit sqlrs_limit_t;
int sqlrs_limit_create(sqlrs_ctx_t *ctx, int has_limit, int64_t limit, int has_offset, int64_t offset,
                       sqlrs_limit_t **out);
int sqlrs_limit_push(sqlrs_limit_t *l, const sqlrs_batch_t *in, int out_mem, sqlrs_batch_t **out, int *done);
void sqlrs_limit_destroy(sqlrs_limit_t *l);

/* [ref: src/executor/join/cross_join.rs:8-58  CrossJoinExecutor{left_child, right_child, join_output_schema};
 *  instantiated at src/executor/mod.rs:116-125]  What the binder rewrites an uncorrelated scalar subquery to
 * (src/binder/table/subquery.rs:120-167: base table CROSS JOIN the one-row subquery).  The left child is collected and
 * concatenated (cross_join.rs:30-36); for every right batch and every LEFT ROW the reference yields one batch = that
 * row's values repeated right.num_rows times | the right columns (cross_join.rs:39-55).  probe_push returns those
 * batches of ONE right batch as a single batch in the same row order (left row 0 x right rows, left row 1 x right
 * rows, ...); the host mirrors slice it back into left_rows batches of right.num_rows rows.  *out = NULL when the left
 * child yielded no batch (cross_join.rs:32-34) or no row. */
typedef struct sqlrs_cross_join sqlrs_cross_join_t;
int sqlrs_cross_join_create(sqlrs_ctx_t *ctx, sqlrs_cross_join_t **out);
int sqlrs_cross_join_build_push(sqlrs_cross_join_t *j, const sqlrs_batch_t *left);
int sqlrs_cross_join_probe_push(sqlrs_cross_join_t *j, const sqlrs_batch_t *right, int out_mem, sqlrs_batch_t **out);
/* The same for the left rows [left_begin, left_begin + left_rows) only: a library batch holds < 2^31 rows, the reference's
 * one-batch-per-left-row stream has no such limit, so a caller whose left rows x right rows exceed it takes the left rows in
 * ranges (sqlrs_cross_join_left_rows = rows pushed so far) and gets the same stream, range after range. */
int sqlrs_cross_join_probe_push_range(sqlrs_cross_join_t *j, const sqlrs_batch_t *right, int64_t left_begin, int64_t left_rows,
                                      int out_mem, sqlrs_batch_t **out);
int64_t sqlrs_cross_join_left_rows(const sqlrs_cross_join_t *j);
void sqlrs_cross_join_destroy(sqlrs_cross_join_t *j);

/* [ref: src/executor/aggregate/simple_agg.rs:10-66  SimpleAggExecutor{agg_funcs, child}]  Aggregates
 * without GROUP BY: one accumulator per aggregate over all rows, exactly one output row (COUNT = 0 and
 * NULL for the others when no row arrived); finish without any pushed batch is SQLRS_ERR_INTERNAL (the
 * reference unwraps a None, :63). */
typedef struct sqlrs_simple_agg sqlrs_simple_agg_t;
int sqlrs_simple_agg_create(sqlrs_ctx_t *ctx, int num_aggs, const sqlrs_agg_func_t *aggs, sqlrs_simple_agg_t **out);
int sqlrs_simple_agg_push(sqlrs_simple_agg_t *a, const sqlrs_batch_t *in);
int sqlrs_simple_agg_finish(sqlrs_simple_agg_t *a, int out_mem, sqlrs_batch_t **out);
void sqlrs_simple_agg_destroy(sqlrs_simple_agg_t *a);
/* Two opt-in flags of sqlrs_simple_agg_create, in `reserved` of its sqlrs_agg_func_t entries (0, the default, leaves the operator
 * as it is; flags of the create call, not entry points of their own: the set of functions is unchanged).
 *
 * SQLRS_SIMPLE_AGG_REDUCE in `reserved` of the FIRST entry: the reduce route [ref: simple_agg.rs:27-65, one accumulator per
 * aggregate updated batch by batch].  Without it the operator is a HashAgg over one constant key: it keeps copies of the
 * pushed key and argument columns until finish and resolves every row through the group table.  With it every pushed batch
 * is consumed by one grid-stride kernel that reads each referenced column once, evaluates the filter (below) and the argument
 * expressions row by row in registers and reduces into one partial record per workgroup, and a second launch that folds
 * those records, in a fixed tree, into a few persistent cells; the operator keeps nothing of the batch (DEVICE columns
 * are read stream-ordered, as the borrowing rules say).  Results are those of the default route; SUM over Float64 within the
 * summation-order tolerance, and bit for bit the same for the same sequence of batches on one device (no floating-point
 * atomics).  Small fixed-width HOST batches are staged as for sqlrs_hash_agg_push (the referenced columns only) and reduced
 * together per 2^22 rows or at finish.
 * Admitted — decided once, from the column types of the FIRST pushed batch, for the operator's whole life: every aggregate is
 * a non-DISTINCT COUNT / SUM / MIN / MAX whose argument (cast to the return type for SUM) is an expression over Int32 /
 * Int64 / Float64 columns and constants with casts and + - * / (<= 24 nodes, stack <= 8) and an Int32 / Int64 / Float64
 * result; the filter, if any, is such an expression with comparisons and AND / OR and a Boolean result; at most 4 distinct
 * (argument, cast) pairs — any number of aggregates over them — and between 1 and 16 referenced columns.  Anything else (a
 * Utf8 / Boolean operand, DISTINCT, MIN / MAX over Utf8, a fifth argument, a longer expression) falls back: the operator
 * behaves exactly as without the flag.  A later batch whose referenced columns differ in type from the first batch's is
 * refused at its push with the status the inner operator has for batches of different schemas (SQLRS_ERR_ARROW).
 * Errors: a division by zero on a kept row with valid operands is recorded on the device and reported by
 * sqlrs_simple_agg_finish (SQLRS_ERR_ARROW, the evaluator's text), not by the push that met it.
 * Witness: the count `simple_reduce_batches` of sqlrs_ctx_profile_read — pushes the reduce route consumed on this ctx, empty
 * batches included, counted at the push; an operator that is not admitted does not move it.
 *
 * SQLRS_SIMPLE_AGG_FILTER in `reserved` of the LAST entry (num_aggs >= 2): that entry is not an aggregate — its `arg` is the
 * predicate of a FilterExecutor sitting directly below the operator, PhysicalSimpleAgg(PhysicalFilter(child)), the shape of
 * `SELECT sum(x) FROM t WHERE ...` [ref: filter.rs:13-25 feeding simple_agg.rs:27-65]; its other fields are not read and the
 * output has num_aggs - 1 columns.  Results are identical to sqlrs_filter_push on every batch followed by
 * sqlrs_simple_agg_push of its output: rows whose mask is false or NULL are dropped; when every row is dropped but a batch
 * was pushed the result is COUNT = 0 and NULL for the others; no batch pushed is the error it is without the flag.  With the
 * reduce route the predicate is evaluated inside the reducing kernel (the filtered columns are never written); otherwise it
 * is handed to the inner operator (sqlrs_hash_agg_set_filter).  An empty `arg` means no filter. */
#define SQLRS_SIMPLE_AGG_REDUCE 1
#define SQLRS_SIMPLE_AGG_FILTER 2

/* [ref: src/util/mod.rs:53-80  record_batch_to_string]  The sqllogictest text form of a batch (host or
 * device resident): one line per row, one blank between columns, NULL -> "NULL", empty string ->
 * "(empty)", other values as arrow's array_value_to_string prints them (floats: Rust's Display).
 * *out is a NUL-terminated string owned by the library until sqlrs_string_free. */
int sqlrs_batch_to_string(sqlrs_ctx_t *ctx, const sqlrs_batch_t *in, char **out);
void sqlrs_string_free(char *s);

/* CSV ingest [ref: src/storage/csv.rs:92-106 CsvConfig (header, ',', infer over 10 records, batches of
 * 1024 rows), :124-133 schema inference, :190-241 CsvTransaction::next_batch].  Parsed on the host (on the device after
 * sqlrs_csv_set_device_parse); with out_mem = SQLRS_MEM_DEVICE the scan's output is HBM resident.
 * Inferred types: INT64, FLOAT64, BOOLEAN, else UTF8 (date-like columns stay UTF8: the path has no date
 * type); a missing value is NULL in a typed column and the empty string in a UTF8 column. */
typedef struct sqlrs_csv sqlrs_csv_t;
int sqlrs_csv_open(sqlrs_ctx_t *ctx, const char *path, int has_header, char delimiter, int64_t batch_size,
                   int64_t infer_max_records, sqlrs_csv_t **out);
int sqlrs_csv_num_columns(const sqlrs_csv_t *r);
const char *sqlrs_csv_column_name(const sqlrs_csv_t *r, int i);
int sqlrs_csv_column_dtype(const sqlrs_csv_t *r, int i);
/* Bounds (offset, limit) of the scan over the data records, limit < 0 = none [ref: csv.rs:207-223]; a file
 * WITHOUT a header yields limit + 1 records, as the reference does (its (offset, offset + limit + 1) line bounds meet
 * arrow-csv's line counter, which starts one later only when there is a header); call before the first next_batch */
int sqlrs_csv_set_bounds(sqlrs_csv_t *r, int64_t offset, int64_t limit);
/* Projections: indices into the file's columns [ref: csv.rs:224] */
int sqlrs_csv_set_projection(sqlrs_csv_t *r, int num_columns, const int32_t *columns);
/* *out = NULL at the end of the scan */
int sqlrs_csv_next_batch(sqlrs_csv_t *r, int out_mem, sqlrs_batch_t **out);
void sqlrs_csv_close(sqlrs_csv_t *r);
/* The device form of the scan: the bytes -> columns work of sqlrs_csv_next_batch done by gfx950 kernels (csv_device.hip).
 * chunk_bytes = 0: host parser (the default); > 0: parse on the device, the file read in pieces of this many bytes (at most
 * 2^31 - 65); < 0: on, with the library's piece size (32 MiB).  Call before the first sqlrs_csv_next_batch.
 * Contract: the sequence of sqlrs_csv_next_batch results — number of batches, rows per batch, dtypes, values bit for bit,
 * validity, Utf8 offsets and bytes, *out = NULL at the end, and for bad input the status, the sqlrs_last_error text and the
 * batch at which it is raised (every earlier batch still delivered) — is the host parser's for the same file, bounds,
 * projection, batch_size, has_header, delimiter and out_mem.  That is: records end at '\n', one trailing '\r' is stripped,
 * a line that is empty after that is skipped, a last record without '\n' counts, the delimiter is any single byte; an empty
 * field is the empty string in a Utf8 column and NULL in a typed one; Int64 and Float64 are std::from_chars (Float64 in
 * general format, correctly rounded; "inf", "nan", "1e+5", "1.", ".5" are read), Boolean is true / false in any case; a
 * record with another field count than the schema and an unparsable typed field are SQLRS_ERR_ARROW with the host parser's
 * text and line number.
 * What the device does not decide it hands back, and counts: a piece with a '"' byte anywhere, a record longer than a piece
 * and the batch in which the device met an error are read by the host parser (whole batches, from the first record of the
 * batch under construction: host_rows); a Float64 field that is not -?digits[.digits][(e|E)[-]digits] with fewer than 2^53
 * as its digits and a decimal exponent within +-22 — where one IEEE multiply or divide of two exact doubles is the correctly
 * rounded value — is written by the host with std::from_chars (patched_fields).  More than 32 projected columns: host parser. */
int sqlrs_csv_set_device_parse(sqlrs_csv_t *r, int64_t chunk_bytes);
/* on != 0: pieces that contain '"' bytes are parsed on the device too, as long as every quote in the piece is regular
 * (below); any other piece is handed back exactly as without the switch.  Needs sqlrs_csv_set_device_parse; either order;
 * before the first sqlrs_csv_next_batch (later: SQLRS_ERR_INTERNAL).  Default 0.  The contract of
 * sqlrs_csv_set_device_parse holds unchanged: the stream of batches is the host parser's, errors included.
 * With every '"' toggling "inside quotes" from the start of a piece (a piece starts at a record's start, outside), a quote
 * that opens is regular iff it is the piece's first byte or follows the delimiter, a '\n' or a quote (which then closed:
 * the "" of an escaped quote); a quote that closes is regular iff the delimiter, '\n', "\r\n" or a quote follows.  Then the
 * separators are the delimiters and record-ending '\n' outside quotes, a field that starts with '"' also ends in one, and
 * its value is what lies between them with "" read as '"' (a typed field: parsed from that; "" is NULL).  A piece is cut at
 * its last '\n' outside quotes.  Handed back (host_rows): a piece with an irregular quote in front of that cut — a quote in
 * the middle of an unquoted field, text behind a closing quote, "x"\r followed by the delimiter — a piece without such a cut
 * (a record longer than a piece, also through quoted line breaks; a quote left open at the end of the file), and, as ever,
 * the batch with an error.  A delimiter that is '"', '\n' or '\r' leaves the switch without effect. */
int sqlrs_csv_set_device_quotes(sqlrs_csv_t *r, int on);
/* rows delivered by the device parser / by the host parser since the switch was set / typed fields the device left to the host */
int sqlrs_csv_device_stats(const sqlrs_csv_t *r, int64_t *device_rows, int64_t *host_rows, int64_t *patched_fields);

/* --------------------------------------------------------------- exchange -- */
/* Hash-partitions a batch on one key expression for the multi-GPU partitioned join /
 * group-by (no reference analogue: sqlrs is single process).  The output batch
 * holds the input rows permuted so that partition p = rows [offsets[p], offsets[p+1]), input
 * order preserved inside a partition; `offsets` (host, num_parts + 1 entries) is filled by the
 * call.  Rows with equal keys always land in the same partition; NULL keys go to partition 0.
 * The caller exchanges the slices (RCCL all-to-all over xGMI) and feeds what it receives to
 * the ordinary operators above. */
int sqlrs_hash_partition(sqlrs_ctx_t *ctx, const sqlrs_batch_t *in, const sqlrs_expr_t *key,
                         int num_parts, int out_mem, sqlrs_batch_t **out, int64_t *offsets);
/* Filter + hash partition in one pass: the rows of `in` that pass `predicate` (FilterExecutor semantics,
 * [ref: src/executor/filter.rs:13-25]: rows whose mask is false or NULL are dropped; NULL / zero nodes =
 * no predicate) distributed like sqlrs_hash_partition.  Partition p = rows
 * [part_start[p], part_start[p] + part_rows[p]) of the output batch (both arrays: host, num_parts
 * entries, filled by the call); rows outside those ranges are unspecified padding and the row order
 * inside a partition is unspecified — what the equi-join / group-by exchange needs, nothing more.
 * `column OP constant` predicates over an int64 / float64 column without NULLs on batches of <= 3
 * fixed-width 8-byte columns (the filtered fact rows of the partitioned hash join) run as ONE kernel:
 * every row is read once, every kept row written once, into per-partition regions of num_rows rows each
 * (num_parts x the input's size of device memory).  Any other shape = sqlrs_filter_* followed by
 * sqlrs_hash_partition inside the library (same rows per partition). */
int sqlrs_hash_partition_filter(sqlrs_ctx_t *ctx, const sqlrs_batch_t *in, const sqlrs_expr_t *key,
                                const sqlrs_expr_t *predicate, int num_parts, int out_mem,
                                sqlrs_batch_t **out, int64_t *part_start, int64_t *part_rows);

/* The exchange itself: an all-to-all of hash partitions over RCCL (xGMI) on the ctx stream, one process per GPU
 * (no reference analogue: sqlrs is a single process; it slots under the executors the builder instantiates
 * for a partitioned join / aggregate [ref: src/executor/mod.rs:103-114,163-174]: their children are wrapped in an
 * exchange of the children's hash partitions).  RCCL is dlopen'ed at the first call; none of this needs torch.
 *   sqlrs_exchange_unique_id   one rank makes the 128-byte id (ncclGetUniqueId) and hands it to the others out of band;
 *   sqlrs_exchange_create      collective: every rank calls it with the same id, its rank and the world size;
 *   sqlrs_exchange_all_to_all  collective: `in` is a DEVICE batch of fixed-width columns (NULLs allowed: validity travels
 *       as a byte per row beside the values) whose rows [part_start[p], part_start[p] + part_rows[p]) go to rank p (what
 *       sqlrs_hash_partition / _filter return; host arrays of `world` entries); *out = the rows received from rank 0, 1,
 *       ... in this order (DEVICE); recv_rows (optional, host, `world` entries) = rows received per rank.  All columns of
 *       the call travel in ONE ncclGroupStart/End.  A rank whose arguments are unusable (Utf8 / Boolean column, partition
 *       outside the batch) says so in the count all-gather: EVERY rank then returns SQLRS_ERR_INTERNAL from this call and
 *       nothing is sent (*out = NULL).  `in` is read stream-ordered: keep it alive until the ctx stream has passed
 *       (sqlrs_ctx_synchronize / release_to_stream), like every borrowed device batch;
 *   sqlrs_exchange_begin / _send_chunk / _finish  the same exchange for a SEQUENCE of chunks into ONE received batch (the
 *       fact rows of the partitioned join, filtered and partitioned chunk by chunk): begin names the column types (and a
 *       capacity hint in rows; the receive batch grows as needed), every send_chunk is a collective like all_to_all, finish
 *       returns the rows of all chunks (per chunk: from rank 0, 1, ...).  send_chunk(k) puts the count words of chunk k on the
 *       wire and sends the payload of chunk k - 1, whose words reached the host while chunk k was being produced: the
 *       host does not wait for the device inside the loop, and the transfer of chunk k - 1 overlaps the partitioning of
 *       chunk k + 1 on the stream.  A batch this library produced is retained by reference until its payload is queued;
 *       any other DEVICE batch is copied once;
 *   sqlrs_exchange_plan        the receive side's bookkeeping as plain host arithmetic (no device): send_rows_all[q * world
 *       + p] = rows rank q sends to rank p -> rows / start offsets this rank receives per source rank. */
/* Range partitioning for a multi-GPU ORDER BY (a sample sort over the exchange above; no reference analogue, the
 * reference sorts in one process [ref: src/executor/order.rs:27-66]).  For a table T cut into W slices held by ranks
 * 0 .. W-1 in this order, with row_base = the rows on lower ranks:
 *   1. every rank samples its slice (sqlrs_range_sample), the tuples are all-gathered (any transport);
 *   2. every rank computes the same W - 1 splitters from all tuples (sqlrs_range_splitters, host arithmetic);
 *   3. every rank range-partitions its slice (sqlrs_range_partition) and sends part p to rank p
 *      (sqlrs_exchange_all_to_all: received in source-rank order);
 *   4. every rank runs sqlrs_order_* (the same ORDER BY list) over what it received.
 * The rank outputs concatenated in rank order are bit-identical to sqlrs_order over T, ties included.  No call here is a
 * collective.  ORDER BY keys: any list sqlrs_order_create accepts whose keys evaluate to Int32 / Int64 / Float64 /
 * Boolean (a Utf8 key is refused with SQLRS_ERR_INTERNAL); payload columns may be of any type.
 * TUPLE LAYOUT (sqlrs_range_tuple_words(K) = 2 K + 1 uint64 words, compared as unsigned integers word by word): per key,
 * in ORDER BY order, a validity word (0 = NULL, 1 = valid) and the key encoded as the Order sorts it (0 for NULL; Int64:
 * value ^ 2^63, Int32: widened to Int64 first, Float64: IEEE total order (bits ^ 2^63 when the sign is clear, ~bits when
 * it is set: -0.0 < +0.0, NaNs outside the infinities), Boolean: 0 / 1; all of it complemented when asc = 0), then the
 * row's global position row_base + i.  NULLs come first whatever the direction, equal keys in position order.
 *   sqlrs_range_sample      min(num_samples, rows) tuples of the rows i * rows / min(num_samples, rows) (evenly spaced,
 *       deterministic, in row order) into `tuples` (host, num_samples * words); *written = their number;
 *   sqlrs_range_splitters   host arithmetic only (no ctx, no device, like sqlrs_exchange_plan): sorts the num_tuples
 *       gathered tuples and writes num_parts - 1 splitters (splitter j - 1 = the (j * num_tuples / num_parts)-th smallest
 *       tuple, counting from 0; nondecreasing) to `splitters` (host); with no tuples every splitter is the all-ones
 *       tuple, so every row goes to part 0.  Returns SQLRS_ERR_INTERNAL on bad arguments (num_parts outside [1, 256],
 *       NULL pointers);
 *   sqlrs_range_partition   stable range partition: the part of a row = the number of splitters <= its tuple; the
 *       output batch holds the input rows permuted so that part p = rows [offsets[p], offsets[p+1]) (`offsets`: host,
 *       num_parts + 1 entries), input order kept inside a part.  `splitters`: host, num_parts - 1 tuples, nondecreasing
 *       (checked; may be NULL when num_parts = 1).  One Int64 / Float64 key column without NULLs among <= 3 8-byte
 *       columns without NULLs (>= 65536 rows, num_parts > 1) runs as one histogram + one scatter pass that read and
 *       write every column once; other shapes sort part ids and gather every column.
 *       (All three: SQLRS_ERR_INTERNAL with sqlrs_last_error set for a Utf8 key, num_parts outside [1, 256],
 *       splitters that are not nondecreasing, NULL splitters with num_parts > 1.) */
int sqlrs_range_tuple_words(int num_keys); /* -1 when num_keys < 1 */
int sqlrs_range_sample(sqlrs_ctx_t *ctx, const sqlrs_batch_t *in, int num_keys, const sqlrs_order_by_t *order_by,
                       int64_t row_base, int num_samples, uint64_t *tuples, int *written);
int sqlrs_range_splitters(int num_keys, int64_t num_tuples, const uint64_t *tuples, int num_parts, uint64_t *splitters);
int sqlrs_range_partition(sqlrs_ctx_t *ctx, const sqlrs_batch_t *in, int num_keys, const sqlrs_order_by_t *order_by,
                          int64_t row_base, int num_parts, const uint64_t *splitters, int out_mem,
                          sqlrs_batch_t **out, int64_t *offsets);
/* ORDER BY ... LIMIT k over the same W ranks (a distributed selection by tuple bound; the reference's
 * PhysicalLimit(PhysicalOrder) [ref: src/executor/limit.rs:12-80 over src/executor/order.rs:27-66]).  Only the rows that can
 * still be among the global first k travel, to ONE root rank:
 *   1. all-gather the row counts (row_base, N); every rank samples its slice (sqlrs_range_sample, in proportion to its
 *      share) and the tuples are all-gathered;
 *   2. every rank computes the same bound tuple B from the samples, N, k = offset + limit and an attempt number a
 *      (sqlrs_range_bound, host arithmetic);
 *   3. every rank keeps its rows whose tuple is strictly below B, in input order (sqlrs_range_select) and all-gathers how
 *      many it kept; below min(k, N) in all, every rank repeats 2-3 with a + 1 (the counts are the same everywhere, so all
 *      ranks agree; the last attempt's bound is the all-ones tuple, which keeps every row);
 *   4. the candidates go to the root (sqlrs_exchange_all_to_all, part_rows = the candidates for the root, 0 for every other
 *      rank: received in source-rank order), which runs sqlrs_order_* with sqlrs_order_set_limit(k); its first min(k, N)
 *      rows are the first min(k, N) rows of sqlrs_order over the whole table, ties included; the caller applies OFFSET /
 *      LIMIT to them.  Every other rank's result is empty.
 * Why: at least k tuples lie below B and the first k rows are the k smallest tuples, so the candidates are a superset of
 * them; inside a rank the candidates keep input order and they arrive in rank order, i.e. in global position order, so
 * the stable Order breaks ties exactly as the global one; and because the position is part of the tuple, a run of equal
 * keys is cut at a position instead of being sent whole.
 *   sqlrs_range_bound       host arithmetic only (no ctx, no device): k <= 0 -> the all-zero tuple (keeps nothing);
 *       k >= total_rows, no tuples, or j past the last tuple -> the all-ones tuple (keeps every row); otherwise the j-th
 *       smallest of the num_tuples gathered tuples, counting from 0, with
 *           j = (c + ceil(2 sqrt(c)) + 2) * 4^attempt - 1,   c = ceil(k * num_tuples / total_rows)
 *       (nondecreasing in attempt; all-ones once 4^attempt > num_tuples).  The slack grows with sqrt(c), the deviation of
 *       the number of rows below a sample quantile: random keys need a second attempt in <= 2.5 % of the cases for
 *       k = 1e3 .. 1e6 of 1e7 rows with 8192 samples, against 6 - 49 % for a constant slack of 2.
 *       SQLRS_ERR_INTERNAL on bad arguments (num_keys < 1, num_tuples < 0, total_rows < 0, attempt < 0, NULL pointers);
 *   sqlrs_range_select      the rows of `in` whose tuple (row_base + i as position) is strictly below `bound` (host, one
 *       tuple of sqlrs_range_tuple_words(num_keys) words), in input order, every column carried (any type, NULLs
 *       included).  Keys as sqlrs_range_partition (a Utf8 key: SQLRS_ERR_INTERNAL naming Utf8, nothing queued); row_base
 *       < 0 and NULL pointers are errors.  No tuple is written: one kernel reads each key column once, encodes it on the fly
 *       and leaves one selection bit per row, then the kept rows' ids (one count fetch) and one gather per column.  More than
 *       16 keys: the tuples are written and compared instead.  Measured on one MI355X (tools/range_topk_bench.py): 0.248 ms
 *       for 1e8 rows of (int64 key, f64) keeping 6 897 of them, against 0.84 ms for sqlrs_range_partition into 8 parts
 *       (DESIGN.md §4.6).  No top-k exchange has run on more than one GPU. */
int sqlrs_range_bound(int num_keys, int64_t num_tuples, const uint64_t *tuples, int64_t total_rows, int64_t k, int attempt,
                      uint64_t *bound);
int sqlrs_range_select(sqlrs_ctx_t *ctx, const sqlrs_batch_t *in, int num_keys, const sqlrs_order_by_t *order_by,
                       int64_t row_base, const uint64_t *bound, int out_mem, sqlrs_batch_t **out);

#define SQLRS_EXCHANGE_ID_BYTES 128
typedef struct sqlrs_exchange sqlrs_exchange_t;
int sqlrs_exchange_unique_id(sqlrs_ctx_t *ctx, void *id_out);
int sqlrs_exchange_create(sqlrs_ctx_t *ctx, const void *unique_id, int rank, int world, sqlrs_exchange_t **out);
int sqlrs_exchange_all_to_all(sqlrs_exchange_t *x, const sqlrs_batch_t *in, const int64_t *part_start, const int64_t *part_rows,
                              sqlrs_batch_t **out, int64_t *recv_rows);
int sqlrs_exchange_begin(sqlrs_exchange_t *x, int num_columns, const int32_t *dtypes, int64_t capacity_rows);
int sqlrs_exchange_send_chunk(sqlrs_exchange_t *x, const sqlrs_batch_t *in, const int64_t *part_start, const int64_t *part_rows);
int sqlrs_exchange_finish(sqlrs_exchange_t *x, sqlrs_batch_t **out);
int sqlrs_exchange_plan(int world, int rank, const int64_t *send_rows_all, int64_t *recv_rows, int64_t *recv_start, int64_t *total);
int64_t sqlrs_exchange_bytes_off_rank(const sqlrs_exchange_t *x);
void sqlrs_exchange_destroy(sqlrs_exchange_t *x);

/* ------------------------------------------------- timing of device work -- */
/* HIP-event timing on the ctx stream (bench.py measures the dominant kernel
 * with these: torch.cuda.Event only sees torch's own stream). */
typedef struct sqlrs_timer sqlrs_timer_t;
int sqlrs_timer_create(sqlrs_ctx_t *ctx, sqlrs_timer_t **out);
int sqlrs_timer_start(sqlrs_timer_t *t);
int sqlrs_timer_stop(sqlrs_timer_t *t);
/* synchronises on the stop event */
int sqlrs_timer_elapsed_ms(sqlrs_timer_t *t, double *ms);
void sqlrs_timer_destroy(sqlrs_timer_t *t);

/* Per-kernel-class accumulated device time since the last reset, measured with
 * HIP events around each launch group when profiling is enabled (off by
 * default; enabling it serialises nothing but adds two event records per group). */
int sqlrs_ctx_profile_enable(sqlrs_ctx_t *ctx, int on);
int sqlrs_ctx_profile_reset(sqlrs_ctx_t *ctx);
/* Writes up to `cap` entries; returns the number of classes. Names are static strings. */
int sqlrs_ctx_profile_read(sqlrs_ctx_t *ctx, int cap, const char **names, double *total_ms,
                           int64_t *launches);

/* Rows one workgroup of the fused `col OP const` filter takes at a time (its tile): the row counts around which that
 * kernel changes shape — for tests that must straddle it. */
int64_t sqlrs_filter_tile_rows(void);

/* Library version string ("sqlrs-hip <semver> gfx950"). */
const char *sqlrs_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SQLRS_HIP_H */
