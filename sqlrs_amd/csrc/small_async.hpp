// small_async.hpp — push_async: the reference's calling shape, ONE 1024-row HOST batch per poll (storage/csv.rs:105,
// filter.rs:15-24, hash_join.rs:284-291), without a stream synchronisation per call (round 6, review r05 #6).
//
// Mechanism.  A synchronous `push` of such a batch is a chain of round trips — upload, two to four launches, the count, the
// download, a stream synchronisation: ~47 us for 8 KB of rows, 21 Mrows/s (Filter) / 11 Mrows/s (HashJoin probe).  `push_async`
// hands back a TICKET and `sqlrs_batch_wait(ticket)` the batch; a caller that waits a few batches behind never blocks on the
// device.  The fast path is ONE launch per batch and no copy call at all:
//   * the batch's columns are copied (memcpy, 8 KB per column) into a slot of a pinned, device-mapped ring (sa_stage_input);
//   * one 1024-thread workgroup reads them over PCIe and does the operator's work.  Filter: the predicate — a conjunction of
//     `column OP constant` terms directly, anything else as a postfix program (SaProgram, sa_eval_row: the evaluator's semantics
//     row by row) — and the kept rows of every column compacted with ballots (sa_positions).  Project: a
//     program per computed column.  HashJoin probe: one lookup per row in the join's table, the build columns gathered;
//   * it writes the output columns + validity bitmaps + a header {sequence number, rows, NULL counts} back into the slot
//     (sa_publish); `wait` polls the header's sequence number (a system-scope release store behind __threadfence_system), falls
//     back to a stream synchronisation when it does not show up, and copies the rows into an ordinary HOST batch.
// Up to SA_GROUP_MAX consecutive batches of one operator leave with one launch (sa_enqueue, sa_launch_group), on SA_STREAMS side streams.
// Without a switch the path takes batches of int32 / int64 / float64 columns (the Filter: Utf8 payload columns too) and programs
// over them; the join: Inner, unique build keys, ONE exactly compared key column without a NULL in the batch, no join filter.
//
// Switches (off by default; the join's are set before its first probe call), what each admits, and the kernel that serves it:
//   sqlrs_hash_join_set_async_general   Left / Right / Full joins and duplicate build keys.  A batch of `rows` rows against a
//     sa_probe_general_kernel           build side whose most frequent key has M rows emits <= rows x M rows: taken when that
//                                       is <= SA_MAX_OUT_ROWS and the output laid out for it fits the slot — the host decides
//                                       before it takes a slot, nothing overflows.
//   sqlrs_hash_join_set_async_utf8      Utf8 PAYLOAD columns on both sides of the join.  The host reserves out_rows x Lmax bytes
//     UTF8 = true of both probe         for a build column (Lmax: its longest string, one kernel and one fetch per join) and
//     kernels                           B x (out_rows / rows) for a probe column of B bytes, admits the batch when that fits;
//                                       the kernels check a column's bytes against SaCol::out_cap before they store one.
//   sqlrs_hash_join_set_async_filter    a join WITH a join filter: compiled once per join into an SaProgram over the joined
//     FILTER = true of both             schema, uploaded once, copied into LDS at kernel start, evaluated on the joined row
//                                       (build columns from HBM, probe columns from the slot).  sa_probe_kernel keeps a pair
//                                       iff the filter is valid and TRUE; sa_probe_general_kernel follows apply_join_filter
//                                       (kept candidates as a list in HBM, then the Right / Full rows that kept none).  A
//                                       valid candidate that divides by zero: SaHeader::pad = 1, the evaluator's error at the wait.
//   sqlrs_hash_join_set_async_keys      NULL probe keys (they take the NULL build rows), a Utf8 key (with the Utf8 switch), 2 - 4
//     KEYS = true of both (only with    key columns: the kernel loads a row's key itself (sa_probe_key), the hashed forms as the
//     UTF8 = true)                      u64 normalize_keys computes (key_hash.hpp), looked up as a value: match-by-hash.
//   sqlrs_filter_set_async_all_types    programs that read Utf8 / Boolean columns and Utf8 constants (sa_compile with `wide`,
//   sqlrs_project_set_async_all_types   SaSlotLoadWide; constants in a pool of <= SA_POOL_MAX bytes staged behind the columns),
//     WIDE = true of sa_filter_kernel   Boolean payload columns (compacted like a validity bitmap, sa_pack_bits).  Chosen per
//     / sa_project_kernel               batch: one with nothing wide in it keeps the narrow kernel.  A join's filter stays narrow.
//
// Everything else — DEVICE input, more than SA_MAX_ROWS rows or SA_MAX_COLS columns, a program past SA_PROG_MAX nodes / SA_STACK_MAX
// stack words, Boolean join keys, the opt-in composite key, a batch that does not fit its slot, no free slot — runs the synchronous
// operator inside push_async and parks the finished batch in the ticket: same results, one output per input, no speed-up.
#pragma once

#include <cstring>

#include "common.hpp"

namespace sq {

constexpr int SA_SLOTS = 32, SA_MAX_COLS = 12;
constexpr uint32_t SA_MAX_ROWS = 4096, SA_NONE = 0xffffffffu;
constexpr size_t SA_AREA = 512 * 1024; // bytes of a slot's input area and of its output area
constexpr uint32_t SA_MAX_OUT_ROWS = 16384; // rows one batch of the general probe kernel may emit (rows x M, see above)

struct SaHeader { // at the start of a slot's output area
  unsigned long long seq; // written LAST by the kernel: the ticket's sequence number
  uint32_t count, pad;
  uint32_t nulls[SA_MAX_COLS];
};
struct SaCol {
  uint32_t in_off, in_voff;   // values / validity bitmap in the input area (in_voff = SA_NONE: no NULLs); build columns: unused
  uint32_t out_off, out_voff; // values / validity bitmap in the output area (always reserved)
  uint32_t width;             // 4 or 8; Utf8: 4 (in_off / out_off are the int32 offsets, rows + 1 of them)
  int32_t dtype;
  // Utf8: the bytes [offsets[0], offsets[rows]) of the input column sit at in_data (a join's build columns: in HBM, in_data
  // unused); the emitted rows' bytes go to out_data, which has out_cap bytes reserved — the kernel stores none past them
  uint32_t in_data, out_data, data_base; // data_base = offsets[0] of the input column
  uint32_t out_cap;
};
struct SaLayout {
  int ncols = 0;
  uint32_t rows = 0;
  SaCol c[SA_MAX_COLS];
};

constexpr int SA_STREAMS = 4, SA_GROUP_MAX = 4;
constexpr size_t SA_PARAM_MAX = 1024; // bytes of one batch's kernel parameters
struct SaRing {
  uint8_t *pin = nullptr; // SA_SLOTS x (input area | output area), pinned + device mapped
  bool busy[SA_SLOTS] = {};
  int next = 0;
  unsigned long long seq = 0;
  // The one-workgroup kernels of consecutive batches are independent of each other; on ONE stream they run back to back
  // (launch latency + a PCIe read round trip + the write-back: ~9 us per batch, 111 Mrows/s measured), on SA_STREAMS side
  // streams they overlap.  A kernel that reads operator state built on the ctx stream (the join's table) is ordered behind
  // it with one event per operator (sa_order_after_ctx), and an operator that is destroyed drains the side streams first.
  hipStream_t side[SA_STREAMS] = {};
  hipEvent_t order_ev = nullptr;
  bool dirty = false; // a kernel was queued on a side stream since the last drain
  // Grouped launches: the parameters of up to `group` consecutive batches of ONE operator wait here and leave with ONE launch
  // (grid = batches, a workgroup each) — the launch call is the largest part of the host's ~6 us per batch.  Flushed when the
  // group is full, when another operator (or the synchronous path) comes, and by whoever waits for a ticket of the group.
  unsigned char pend_buf[SA_GROUP_MAX * SA_PARAM_MAX];
  int pend_n = 0, pend_first_slot = 0, group = SA_GROUP_MAX;
  const void *pend_owner = nullptr;
  void (*pend_launch)(SaRing *, Ctx *) = nullptr;
  unsigned long long launched_seq = 0; // the kernels of all tickets up to this sequence number are queued
  unsigned long long pend_last_seq = 0; // the newest ticket of the pending group (NOT `seq`: the ticket whose push flushes another
                                        // operator's group has its number already and joins the NEXT group)
  ~SaRing() {
    for (hipStream_t s : side)
      if (s) {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
      }
    if (order_ev) (void)hipEventDestroy(order_ev);
    if (pin) (void)hipHostFree(pin);
  }
  hipStream_t stream_of(int slot) const { return side[slot % SA_STREAMS]; }
  uint8_t *in_area(int s) const { return pin + (size_t)s * 2 * SA_AREA; }
  uint8_t *out_area(int s) const { return pin + (size_t)s * 2 * SA_AREA + SA_AREA; }
};
SaRing *sa_ring(Ctx *ctx);  // the ctx's ring, created on first use
int sa_take_slot(SaRing *r); // -1: every slot has a ticket outstanding
void sa_order_after_ctx(Ctx *ctx, SaRing *r); // every side stream waits for what the ctx stream holds now
void sa_drain(Ctx *ctx);                      // flushes, then waits for the side streams (operator teardown); no-op without a ring
void sa_flush(Ctx *ctx);                      // launches the pending group, if any
template <class P> struct SaGroup { P p[SA_GROUP_MAX]; };
// appends one batch's parameters to the pending group of `owner` (launching what another operator left there first)
template <class P> inline void sa_enqueue(Ctx *ctx, SaRing *r, const void *owner, void (*launch)(SaRing *, Ctx *), const P &p, int slot) {
  static_assert(sizeof(P) <= SA_PARAM_MAX, "parameter block too large");
  if (r->pend_n && (r->pend_owner != owner || r->pend_launch != launch)) sa_flush(ctx);
  if (!r->pend_n) r->pend_first_slot = slot;
  std::memcpy(r->pend_buf + (size_t)r->pend_n * SA_PARAM_MAX, &p, sizeof(P));
  r->pend_owner = owner;
  r->pend_launch = launch;
  r->pend_last_seq = p.seq;
  r->pend_n++;
  ctx->async_fast_batches++;
  if (r->pend_n >= r->group) sa_flush(ctx);
}

// Lays `in` (HOST columns of int32 / int64 / float64 — Utf8 when `allow_utf8`, Boolean when `allow_bool` — <= SA_MAX_ROWS rows) out in `area` and describes it in `lay`;
// `first_out_col` output columns are reserved in front of the batch's own (the join's build columns).  `out_rows`: the rows
// the OUTPUT columns and their bitmaps are laid out for (SA_NONE: as many as the batch has; more for a kernel that emits more
// rows than it reads — a Utf8 column of the batch then has (its bytes) x (out_rows / rows) reserved: every row emitted equally
// often at the most).  `front_bytes` (may be null: no Utf8 column in front): the bytes to reserve for the data of front column c
// when it is Utf8.  A Boolean column (width 0) is its value bitmap at in_off and, compacted, at out_off: whole 64-bit words.
// `extra_bytes` are reserved behind the columns in the input area (a program's constant pool) and *extra_off is where.
// false = not a batch for the fast path (nothing written that matters).
bool sa_stage_input(const sqlrs_batch_t *in, uint8_t *area, SaLayout *lay, int first_out_col, const int32_t *front_dtypes,
                    bool allow_utf8 = false, uint32_t out_rows = SA_NONE, const uint64_t *front_bytes = nullptr, bool allow_bool = false,
                    uint32_t extra_bytes = 0, uint32_t *extra_off = nullptr);

// ---- a postfix program over the batch's fixed-width columns, evaluated per row INSIDE the one-launch kernels -----------------
// BoundExpr::eval_column (evaluator.rs:13-28, array_compute.rs:70-90) restated for one row: the same arithmetic (integers wrap,
// x / 0 on a valid row is the Arrow error), the same comparisons (doubles in IEEE total order), Kleene AND / OR, the same casts
// (out of range -> NULL), NULL = an operand was NULL — expr.hip does this column by column with one launch per node.
constexpr int SA_PROG_MAX = 24, SA_STACK_MAX = 8;
enum SaOp : uint8_t { SAO_COL = 0, SAO_CONST, SAO_CAST, SAO_ADD, SAO_SUB, SAO_MUL, SAO_DIV, SAO_GT, SAO_LT, SAO_GE, SAO_LE, SAO_EQ, SAO_NE, SAO_AND, SAO_OR };
struct SaInstr {
  uint8_t op, dtype, from, is_null; // dtype: operand type of an arithmetic / comparison, target of a cast, type of a constant / column
  uint32_t col;                     // SAO_COL: column of the batch
  unsigned long long imm;           // SAO_CONST: the value's bits (int32 sign-extended, bool 0 / 1)
};
struct SaProgram {
  int n = 0;
  int32_t result_dtype = 0;
  SaInstr ins[SA_PROG_MAX];
};
// The Utf8 constants of ONE expression, staged once per batch in the slot's input area: at most SA_POOL_MAX bytes in all (more: the
// synchronous path).  `wide`: the program has an operand only sa_eval_row<true> knows (a Utf8 / Boolean column, a Utf8 constant).
constexpr uint32_t SA_POOL_MAX = 1024;
struct SaPool {
  uint32_t nbytes = 0;
  bool wide = false;
  uint8_t bytes[SA_POOL_MAX];
};
// Expr -> program over the columns of `in`; false = not expressible here (a Utf8 / Boolean column or Utf8 constant unless `wide`,
// mixed operand types, an unsupported cast, too long): the synchronous evaluator takes the batch and raises whatever error there
// is to raise.  With `wide` (and a pool) a Utf8 column / constant may be an operand of the six comparisons against another Utf8
// operand — a Utf8 result, cast or arithmetic stays not expressible — and a Boolean column an operand of comparisons, AND / OR and
// casts, or the whole program.  A Utf8 constant's imm is {length << 32 | offset in the pool}: sa_place_pool makes it a slot offset.
bool sa_compile(const Expr &e, const sqlrs_batch_t *in, SaProgram *out, bool wide = false, SaPool *pool = nullptr);
// the same over a list of column dtypes (a join's filter: the build side's columns, then the probe side's — never `wide`)
bool sa_compile(const Expr &e, const int32_t *dtypes, int ncols, SaProgram *out, bool wide = false, SaPool *pool = nullptr);
inline void sa_place_pool(SaProgram *pr, uint32_t pool_off) {
  for (int k = 0; k < pr->n; k++)
    if (pr->ins[k].op == SAO_CONST && pr->ins[k].dtype == SQLRS_UTF8) pr->ins[k].imm += pool_off;
}
inline bool sa_fast_off() {
  const char *e = hook("SQLRS_ASYNC_FAST"); // test hook, read per call: 0 = every batch through the synchronous operator
  return e && e[0] == '0';
}

} // namespace sq

// what push_async returns and sqlrs_batch_wait consumes
struct sqlrs_ticket {
  sq::Ctx *ctx = nullptr;
  int slot = -1; // -1: the slow path ran, `done` is the batch (may be NULL: an operator that emits nothing)
  unsigned long long seq = 0;
  sqlrs_batch_t *done = nullptr;
  sq::SaLayout lay; // (output side: offsets, widths, dtypes of the columns the kernel writes)
};

#if defined(__HIPCC__)
#include "device_utils.hpp"
namespace sq {
// the operand loader of a batch in its slot: column `c` of row `r` (int32 sign-extended), *ok = the value is not NULL
struct SaSlotLoad {
  const SaLayout &lay;
  const uint8_t *in;
  uint32_t r;
  __device__ __forceinline__ unsigned long long operator()(uint32_t col, bool *ok) const {
    const SaCol &c = lay.c[col];
    *ok = c.in_voff == SA_NONE || ((in[c.in_voff + (r >> 3)] >> (r & 7)) & 1);
    return c.width == 8 ? ((const unsigned long long *)(in + c.in_off))[r] : (unsigned long long)(long long)((const int32_t *)(in + c.in_off))[r];
  }
};
// the same with the all-types operand kinds: a Boolean column is bit r of its value bitmap (0 / 1), a Utf8 column the word
// {length << 32 | offset of its bytes in the input area}; bytes() is what sa_eval_row<true> compares Utf8 operands through
struct SaSlotLoadWide {
  const SaLayout &lay;
  const uint8_t *in;
  uint32_t r;
  __device__ __forceinline__ const uint8_t *bytes() const { return in; }
  __device__ __forceinline__ unsigned long long operator()(uint32_t col, bool *ok) const {
    const SaCol &c = lay.c[col];
    *ok = c.in_voff == SA_NONE || ((in[c.in_voff + (r >> 3)] >> (r & 7)) & 1);
    if (c.dtype == SQLRS_BOOLEAN) return (unsigned long long)((in[c.in_off + (r >> 3)] >> (r & 7)) & 1);
    if (c.dtype == SQLRS_UTF8) {
      const int32_t *off = (const int32_t *)(in + c.in_off);
      const uint32_t o0 = (uint32_t)off[r], o1 = (uint32_t)off[r + 1];
      return ((unsigned long long)(o1 - o0) << 32) | (unsigned long long)(c.in_data + (o0 - c.data_base));
    }
    return c.width == 8 ? ((const unsigned long long *)(in + c.in_off))[r] : (unsigned long long)(long long)((const int32_t *)(in + c.in_off))[r];
  }
};
// Utf8 operands `a`, `b` ({length << 32 | offset from `base`}) in cmp_utf8_kernel's order: bytes compare unsigned, the shorter string
// is less when it is a prefix.  `both_valid` false (a NULL operand: the result is NULL whatever the bytes are): no byte is read.
__device__ __forceinline__ void sa_cmp_utf8(const uint8_t *base, unsigned long long a, unsigned long long b, bool both_valid, bool *lt, bool *eq) {
  const uint32_t la = (uint32_t)(a >> 32), lb = (uint32_t)(b >> 32), m = both_valid ? (la < lb ? la : lb) : 0u;
  const uint8_t *pa = base + (uint32_t)a, *pb = base + (uint32_t)b;
  int c = 0;
  for (uint32_t i = 0; i < m && c == 0; i++) c = (int)pa[i] - (int)pb[i];
  if (c == 0) c = (la > lb) - (la < lb);
  *lt = c < 0;
  *eq = c == 0;
}
// one row of the program: *valid = the result is not NULL; *div0 raised when a valid row divides by zero.  `load(column, &ok)`
// fetches an operand: SaSlotLoad for the Filter / Project kernels, the joined-row loader of the probe kernels (join_async.hip).
// WIDE (a compile-time flag: the other instantiations keep their code): Utf8 comparisons, through load.bytes() (SaSlotLoadWide)
template <bool WIDE = false, class Load>
__device__ __forceinline__ unsigned long long sa_eval_row(const SaProgram &pr, const Load &load, bool *valid, bool *div0) {
  unsigned long long v[SA_STACK_MAX];
  bool ok[SA_STACK_MAX];
  int sp = 0;
  for (int k = 0; k < pr.n; k++) {
    const SaInstr I = pr.ins[k];
    if (I.op == SAO_COL) {
      bool o;
      v[sp] = load(I.col, &o);
      ok[sp] = o;
      sp++;
    } else if (I.op == SAO_CONST) {
      ok[sp] = !I.is_null;
      v[sp] = I.imm;
      sp++;
    } else if (I.op == SAO_CAST) {
      unsigned long long x = v[sp - 1];
      bool o = ok[sp - 1];
      if (I.from == SQLRS_BOOLEAN || I.from == SQLRS_INT32 || (I.from == SQLRS_INT64 && I.dtype != SQLRS_INT32)) { // widening / exact sources
        const long long iv = (long long)x;
        if (I.dtype == SQLRS_FLOAT64) x = (unsigned long long)__double_as_longlong((double)iv);
      } else if (I.from == SQLRS_INT64) { // -> int32: out of range = NULL
        const long long iv = (long long)x;
        const bool in_range = iv <= 2147483647ll && iv >= -2147483648ll;
        x = in_range ? x : 0ull;
        o = o && in_range;
      } else { // float64 -> integer
        const double f = __longlong_as_double((long long)x);
        const double lim = I.dtype == SQLRS_INT32 ? 2147483648.0 : 9223372036854775808.0;
        const bool in_range = (I.dtype == SQLRS_INT32 ? f > -lim - 1 : f >= -lim) && (f < lim); // (-2^63 is INT64_MIN: inclusive, expr.hip cast_kernel)
        x = in_range ? (I.dtype == SQLRS_INT32 ? (unsigned long long)(long long)(int32_t)f : (unsigned long long)(long long)f) : 0ull;
        o = o && in_range;
      }
      v[sp - 1] = x;
      ok[sp - 1] = o;
    } else {
      const unsigned long long b = v[sp - 1], a = v[sp - 2];
      const bool bo = ok[sp - 1], ao = ok[sp - 2];
      sp -= 2;
      unsigned long long res = 0;
      bool ro = ao && bo;
      if (I.op >= SAO_ADD && I.op <= SAO_DIV) {
        if (I.dtype == SQLRS_FLOAT64) {
          const double x = __longlong_as_double((long long)a), y = __longlong_as_double((long long)b);
          double q = 0;
          if (I.op == SAO_DIV) {
            if (ro && y == 0.0) *div0 = true;
            else if (ro) q = x / y;
          } else
            q = I.op == SAO_ADD ? x + y : I.op == SAO_SUB ? x - y : x * y;
          res = (unsigned long long)__double_as_longlong(q);
        } else if (I.dtype == SQLRS_INT64) {
          if (I.op == SAO_DIV) {
            if (ro && b == 0) *div0 = true;
            else if (ro) res = (long long)b == -1 ? 0ull - a : (unsigned long long)((long long)a / (long long)b);
          } else
            res = I.op == SAO_ADD ? a + b : I.op == SAO_SUB ? a - b : a * b;
        } else { // int32: wraps at 32 bits, kept sign-extended
          const uint32_t x = (uint32_t)a, y = (uint32_t)b;
          uint32_t q = 0;
          if (I.op == SAO_DIV) {
            if (ro && y == 0) *div0 = true;
            else if (ro) q = (int32_t)y == -1 ? 0u - x : (uint32_t)((int32_t)x / (int32_t)y);
          } else
            q = I.op == SAO_ADD ? x + y : I.op == SAO_SUB ? x - y : x * y;
          res = (unsigned long long)(long long)(int32_t)q;
        }
      } else if (I.op >= SAO_GT && I.op <= SAO_NE) {
        bool lt, eq;
        if (WIDE && I.dtype == SQLRS_UTF8) {
          lt = eq = false;
          if constexpr (WIDE) sa_cmp_utf8(load.bytes(), a, b, ro, &lt, &eq);
        } else if (I.dtype == SQLRS_FLOAT64) {
          const unsigned long long x = f64_to_ordered(__longlong_as_double((long long)a)), y = f64_to_ordered(__longlong_as_double((long long)b));
          lt = x < y;
          eq = x == y;
        } else { // int32 (sign-extended), int64, bool (0 / 1)
          lt = (long long)a < (long long)b;
          eq = a == b;
        }
        res = I.op == SAO_GT ? (!lt && !eq) : I.op == SAO_LT ? lt : I.op == SAO_GE ? !lt : I.op == SAO_LE ? (lt || eq) : I.op == SAO_EQ ? eq : !eq;
      } else if (I.op == SAO_AND) { // Kleene (bool_words_kernel, mode 6)
        const bool kf = (ao && !a) || (bo && !b), kt = ao && a && bo && b;
        res = kt;
        ro = kf || kt;
      } else { // SAO_OR (mode 7)
        const bool kt = (ao && a) || (bo && b), kf = ao && !a && bo && !b;
        res = kt;
        ro = kf || kt;
      }
      v[sp] = res;
      ok[sp] = ro;
      sp++;
    }
  }
  *valid = ok[0];
  return v[0];
}
__device__ __forceinline__ unsigned long long sa_eval_row(const SaProgram &pr, const SaLayout &lay, const uint8_t *in, uint32_t r, bool *valid,
                                                          bool *div0) {
  return sa_eval_row(pr, SaSlotLoad{lay, in, r}, valid, div0);
}

// The block step of a scan over the 16 waves of ONE 1024-thread workgroup: the lane that holds its wave's total (`owner`: lane 0
// behind a ballot, lane 63 behind wave_iscan_u32) stores it into s_w[wave]; *before = the totals of the waves in front of this
// one, *all = those of all 16.  The ONE barrier is between the store and the loads: the caller places the barrier that lets s_w
// be written again.  `s_w`: 16 words of LDS.
__device__ __forceinline__ void sa_block_prefix(uint32_t *s_w, bool owner, uint32_t wave_total, uint32_t *before, uint32_t *all) {
  const int w = wave_id();
  if (owner) s_w[w] = wave_total;
  __syncthreads();
  uint32_t b = 0, a = 0;
#pragma unroll
  for (int q = 0; q < 16; q++) {
    const uint32_t c = s_w[q];
    b += q < w ? c : 0;
    a += c;
  }
  *before = b;
  *all = a;
}
// Output positions of the kept rows of <= 4096 rows on ONE 1024-thread workgroup: pos[t] for row t * 1024 + tid, bit t of
// the return value = kept; *total = kept rows.  `s_w`: 17 words of LDS.
template <class KeepFn>
__device__ __forceinline__ uint32_t sa_positions(uint32_t rows, KeepFn keep_of, uint32_t (&pos)[4], uint32_t *s_w, uint32_t *total) {
  uint32_t base = 0, bits = 0;
#pragma unroll
  for (int t = 0; t < 4; t++) {
    if ((uint32_t)t * 1024u >= rows) break; // (uniform)
    const uint32_t r = (uint32_t)t * 1024u + threadIdx.x;
    const bool k = r < rows && keep_of(r, t);
    const uint64_t bm = __ballot(k);
    uint32_t before, all;
    sa_block_prefix(s_w, lane_id() == 0, (uint32_t)__popcll(bm), &before, &all);
    pos[t] = base + before + mbcnt(bm);
    bits |= k ? 1u << t : 0u;
    base += all;
    __syncthreads();
  }
  *total = base;
  return bits;
}
// the validity bitmap of one output column from per-row flags in LDS (`s_v[pos]` = 1 valid / 0 NULL, written by the kept
// rows before the call's first barrier); returns nothing, adds the NULLs to *s_nulls (LDS)
__device__ __forceinline__ void sa_pack_validity(const uint8_t *s_v, uint32_t total, uint8_t *out_bits, uint32_t *s_nulls) {
  __syncthreads();
  uint32_t nulls = 0;
  for (uint32_t i = threadIdx.x; i < (total + 7) / 8; i += blockDim.x) {
    uint32_t byte = 0;
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const uint32_t p = i * 8 + b;
      const uint32_t v = p < total ? s_v[p] : 0u;
      byte |= v << b;
      nulls += p < total && !v;
    }
    out_bits[i] = (uint8_t)byte;
  }
  if (nulls) atomicAdd(s_nulls, nulls);
  __syncthreads();
}
// the same without the count: the VALUE bitmap of a Boolean column the Filter compacts (`s_v[pos]` = the kept row's bit)
__device__ __forceinline__ void sa_pack_bits(const uint8_t *s_v, uint32_t total, uint8_t *out_bits) {
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < (total + 7) / 8; i += blockDim.x) {
    uint32_t byte = 0;
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const uint32_t p = i * 8 + b;
      byte |= (p < total ? (uint32_t)s_v[p] : 0u) << b;
    }
    out_bits[i] = (uint8_t)byte;
  }
  __syncthreads();
}
// the probe row of output row `o` of a batch whose row r emits the rows [s_off[r], s_off[r + 1]): the last of the `rows` probe
// rows whose first output row is <= o (s_off[0] = 0)
__device__ __forceinline__ uint32_t sa_output_row(const uint32_t *s_off, uint32_t rows, uint32_t o) {
  uint32_t lo = 0, hi = rows;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (s_off[mid] <= o) lo = mid;
    else hi = mid;
  }
  return lo;
}
// The launch function of a kernel over SaGroup<P> for sa_enqueue: the pending parameters, one workgroup per batch, on the side
// stream of the group's first slot.  One function address per kernel instantiation, which is how sa_enqueue tells groups apart.
template <class P, auto Kernel> void sa_launch_group(SaRing *r, Ctx *ctx) {
  static_assert(sizeof(P) <= SA_PARAM_MAX, "parameter block too large");
  SaGroup<P> g;
  for (int i = 0; i < r->pend_n; i++) std::memcpy(&g.p[i], r->pend_buf + (size_t)i * SA_PARAM_MAX, sizeof(P));
  Kernel<<<dim3((unsigned)r->pend_n), dim3(1024), 0, r->stream_of(r->pend_first_slot)>>>(g);
  SQ_HIP(hipGetLastError());
}
// the last step of a fast-path kernel: every thread's stores to the pinned output are pushed out, then ONE thread
// publishes the header.  `s_error` (LDS, may be null) is read BEHIND the barrier like `s_nulls`: any wave may have raised it
// last (passed by value it was thread 0's view in front of the barrier, and a division by zero seen by another wave of the
// Project kernel, which has no barrier of its own after the rows, could be lost)
__device__ __forceinline__ void sa_publish(SaHeader *hdr, unsigned long long seq, uint32_t total, const uint32_t *s_nulls, int ncols,
                                           const uint32_t *s_error = nullptr) {
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    hdr->count = total;
    hdr->pad = s_error ? *s_error : 0u; // (1: a valid row divided by zero — sqlrs_batch_wait turns it into the evaluator's Arrow error)
    for (int c = 0; c < ncols; c++) hdr->nulls[c] = s_nulls[c];
    __threadfence_system();
    __hip_atomic_store(&hdr->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
} // namespace sq
#endif
