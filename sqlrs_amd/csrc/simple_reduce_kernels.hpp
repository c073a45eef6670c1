// simple_reduce_kernels.hpp — the two kernels of SimpleAgg's reduce route (simple_reduce.hip; SQLRS_SIMPLE_AGG_REDUCE).
//
// sr_reduce_kernel   256-thread workgroups, <= SR_MAX_BLOCKS of them, grid-stride.  A wave owns SR_UNROLL consecutive 64-row
//                    groups per iteration (lane = row inside the group: 8 B per lane, coalesced; the validity word of a group
//                    is one load for the wave), a workgroup 4 x SR_UNROLL groups = 1024 rows, the full grid 2^21 rows.  Per
//                    row: the filter (a conjunction of `column OP constant` terms directly, anything else as a postfix
//                    program: sa_eval_row, small_async.hpp) -> kept iff valid and TRUE; for a kept row each distinct argument
//                    once (a bare column directly, anything else sa_eval_row) into per-lane cells {non-NULL count, SUM, MIN
//                    image, MAX image} — agg.hip's ordered images; SUM and MIN / MAX only where an aggregate reads them —
//                    and a flag for a division by zero.  The direct forms load a column's SR_UNROLL rows together
//                    (sr_load_rows: 4 x 8 B per lane in flight, 48 KiB per CU at 6 workgroups); rows the filter dropped
//                    and columns no program names are never read.  The cells are reduced over the wave (__shfl_xor), over
//                    the 4 waves through LDS in wave order, and stored — plain stores — as ONE partial record per workgroup.
// sr_fold_kernel     one wave folds the partial records (stored field major) into the operator's persistent record: per field,
//                    lane j the records j, j + 64, ... in order, then the lanes by butterflies.
//
// No atomics: every addition happens in a tree fixed by (rows, grid), so SUM(Float64) has the same bits on every run.  (A strictly
// sequential fold of 2048 records by one lane was measured first: ~0.45 us per record, 1 ms per push — five times the reduce kernel.)
#pragma once

#include "small_async.hpp"

namespace sq {

constexpr int SR_MAX_ARGS = 4, SR_MAX_COLS = 16, SR_MAX_TERMS = 4;
constexpr int SR_THREADS = 256, SR_UNROLL = 4, SR_MAX_BLOCKS = 2048;
constexpr int SR_BLOCK_ROWS = SR_THREADS * SR_UNROLL;                      // 1024
constexpr int64_t SR_SWEEP_ROWS = (int64_t)SR_MAX_BLOCKS * SR_BLOCK_ROWS; // 2^21
constexpr int SR_FIELDS = 4 * SR_MAX_ARGS + 1;
enum { SR_CNT = 0, SR_SUM = 1, SR_MIN = 2, SR_MAX = 3 };
enum { SR_NEED_SUM = 1, SR_NEED_MINMAX = 2 };

// cells of argument a at w[4 a + {SR_CNT, SR_SUM, SR_MIN, SR_MAX}] (SUM: the u64 wrapping sum, or the bits of a double),
// w[16] != 0: a kept row with valid operands divided by zero
struct SrRecord {
  unsigned long long w[SR_FIELDS];
};
inline void sr_init_record(SrRecord *r) {
  for (int a = 0; a < SR_MAX_ARGS; a++) {
    r->w[4 * a + SR_CNT] = 0;
    r->w[4 * a + SR_SUM] = 0; // (+0.0 as a double)
    r->w[4 * a + SR_MIN] = ~0ull;
    r->w[4 * a + SR_MAX] = 0;
  }
  r->w[4 * SR_MAX_ARGS] = 0;
}

// one term `column OP constant` of a conjunction: kept iff the column is valid and the comparison holds
struct SrTerm {
  uint32_t col, op;       // op: SAO_GT .. SAO_NE
  uint32_t is_f64, pad;   // doubles compare in IEEE total order, as the evaluator's do
  unsigned long long imm; // is_f64: the constant's ordered image; else the (sign-extended) integer
};
// what the operator compiled at its first batch; lives in HBM for the operator's life, copied into LDS per workgroup
struct SrPlan {
  int nargs;
  int filter_mode; // 0 none, 1 terms, 2 program
  int nterms;
  int pad;
  int arg_col[SR_MAX_ARGS];  // >= 0: the argument is this column as it is (no program)
  int arg_f64[SR_MAX_ARGS];  // the argument's value (and its SUM) is a double
  int arg_c0[SR_MAX_ARGS], arg_c1[SR_MAX_ARGS]; // a program that names one or two columns: those (c1 < 0: one); c0 < 0: more
  int arg_op[SR_MAX_ARGS], arg_opdt[SR_MAX_ARGS]; // != 0: the argument is `column c0 OP column c1`, OP = SAO_ADD / SUB / MUL over this dtype
  int arg_need[SR_MAX_ARGS]; // SR_NEED_*: the cells some aggregate reads beside the count (the others are not computed)
  SrTerm terms[SR_MAX_TERMS];
  SaProgram arg[SR_MAX_ARGS];
  SaProgram filter;
};
// one batch: the referenced columns, in the plan's numbering
struct SrBatch {
  const void *values[SR_MAX_COLS];
  const uint64_t *validity[SR_MAX_COLS]; // null: no NULLs
  uint32_t width8;                       // bit c: column c is 8 bytes wide (else an int32)
  int ncols;
  long long rows;
};

#if defined(__HIPCC__)
// operand loader of the interpreter over the batch's global columns: row r, validity words by 64-row group
struct SrLoad {
  const SrBatch &b;
  long long r;
  __device__ __forceinline__ unsigned long long operator()(uint32_t col, bool *ok) const {
    const uint64_t *v = b.validity[col];
    *ok = !v || ((v[r >> 6] >> (r & 63)) & 1);
    return ((b.width8 >> col) & 1) ? ((const unsigned long long *)b.values[col])[r]
                                   : (unsigned long long)(long long)((const int32_t *)b.values[col])[r];
  }
};

// Column `col` of the SR_UNROLL rows rc[u] of this lane, the loads issued together (no branch between them: they are all in
// flight before the first is used); rows with want[u] false are not read.  ok[u] = wanted and not NULL; the validity word of
// group grp[u] (uniform over the wave) is one scalar load.
__device__ __forceinline__ void sr_load_rows(const SrBatch &b, int col, const long long (&rc)[SR_UNROLL], const long long (&grp)[SR_UNROLL],
                                             const bool (&want)[SR_UNROLL], unsigned long long (&x)[SR_UNROLL], bool (&ok)[SR_UNROLL]) {
  const void *vals = b.values[col];
  const uint64_t *valid = b.validity[col];
  if ((b.width8 >> col) & 1) {
#pragma unroll
    for (int u = 0; u < SR_UNROLL; u++) x[u] = want[u] ? ((const unsigned long long *)vals)[rc[u]] : 0ull;
  } else {
#pragma unroll
    for (int u = 0; u < SR_UNROLL; u++) x[u] = want[u] ? (unsigned long long)(long long)((const int32_t *)vals)[rc[u]] : 0ull;
  }
#pragma unroll
  for (int u = 0; u < SR_UNROLL; u++) ok[u] = want[u] && (!valid || ((valid[grp[u]] >> (rc[u] & 63)) & 1));
}

// the interpreter's loader of an argument: `regs` (uniform) — the program names one or two columns and this row's values are
// held in registers (x0: column c0, x1: the other; okbits: bit 0 / 1 = not NULL) — or, for more columns, out of memory
struct SrRegLoad {
  const SrBatch &b;
  long long r;
  unsigned long long x0, x1;
  uint32_t c0, okbits;
  bool regs;
  __device__ __forceinline__ unsigned long long operator()(uint32_t col, bool *ok) const {
    if (!regs) return SrLoad{b, r}(col, ok);
    *ok = ((col == c0 ? okbits : okbits >> 1) & 1u) != 0;
    return col == c0 ? x0 : x1;
  }
};
__device__ __forceinline__ bool sr_term_holds(const SrTerm &t, unsigned long long x) {
  bool lt, eq;
  if (t.is_f64) {
    const unsigned long long u = f64_to_ordered(__longlong_as_double((long long)x));
    lt = u < t.imm;
    eq = u == t.imm;
  } else {
    lt = (long long)x < (long long)t.imm;
    eq = x == t.imm;
  }
  return t.op == SAO_GT ? (!lt && !eq) : t.op == SAO_LT ? lt : t.op == SAO_GE ? !lt : t.op == SAO_LE ? (lt || eq) : t.op == SAO_EQ ? eq : !eq;
}

__device__ __forceinline__ unsigned long long sr_combine(int kind, bool f64, unsigned long long a, unsigned long long b) {
  if (kind == SR_MIN) return a < b ? a : b;
  if (kind == SR_MAX) return a > b ? a : b;
  if (kind == SR_SUM && f64) return (unsigned long long)__double_as_longlong(__longlong_as_double((long long)a) + __longlong_as_double((long long)b));
  return a + b;
}

// `column OP column` for + - *, as sa_eval_row computes it: doubles one IEEE operation, int64 wrapping, int32 wrapping at 32 bits
// and kept sign-extended (no division here: nothing to raise)
__device__ __forceinline__ unsigned long long sr_binop(int op, int dtype, unsigned long long a, unsigned long long b) {
  if (dtype == SQLRS_FLOAT64) {
    const double x = __longlong_as_double((long long)a), y = __longlong_as_double((long long)b);
    return (unsigned long long)__double_as_longlong(op == SAO_ADD ? x + y : op == SAO_SUB ? x - y : x * y);
  }
  const unsigned long long q = op == SAO_ADD ? a + b : op == SAO_SUB ? a - b : a * b;
  return dtype == SQLRS_INT32 ? (unsigned long long)(long long)(int32_t)(uint32_t)q : q;
}

// PROGRAMS false: the filter is absent or a conjunction of terms and every argument a bare column or `column OP column` — the instantiation holds no
// interpreter (fewer registers, more waves per SIMD: the streaming shapes `sum(x)`, `count / sum / min / max (x) WHERE a < c`)
template <int NARGS, bool PROGRAMS>
__global__ void __launch_bounds__(SR_THREADS) sr_reduce_kernel(const SrPlan *__restrict__ plan_g, SrBatch b, unsigned long long *__restrict__ partial) {
  __shared__ __attribute__((aligned(8))) unsigned char s_plan_raw[sizeof(SrPlan)]; // (SaProgram has member initialisers)
  __shared__ unsigned long long s_rec[SR_THREADS / 64][SR_FIELDS];
  {
    const uint32_t *src = (const uint32_t *)plan_g;
    uint32_t *dst = (uint32_t *)s_plan_raw;
    for (uint32_t k = threadIdx.x; k < sizeof(SrPlan) / 4; k += SR_THREADS) dst[k] = src[k];
  }
  __syncthreads();
  const SrPlan &plan = *(const SrPlan *)s_plan_raw;
  unsigned long long sum[NARGS], mn[NARGS], mx[NARGS];
  uint32_t cnt[NARGS]; // (a batch has < 2^31 rows)
#pragma unroll
  for (int a = 0; a < NARGS; a++) {
    cnt[a] = 0;
    sum[a] = 0;
    mn[a] = ~0ull;
    mx[a] = 0;
  }
  bool div0 = false;
  const long long groups = (b.rows + 63) >> 6;
  const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(wave_id());
  const int fmode = plan.filter_mode, nterms = plan.nterms;
  // group of (iteration, workgroup, wave, u): consecutive groups of a wave, consecutive waves, consecutive workgroups
  for (long long g0 = ((long long)blockIdx.x * (SR_THREADS / 64) + wave) * SR_UNROLL; g0 < groups;
       g0 += (long long)gridDim.x * (SR_THREADS / 64) * SR_UNROLL) {
    long long rc[SR_UNROLL], grp[SR_UNROLL];
    bool keep[SR_UNROLL];
#pragma unroll
    for (int u = 0; u < SR_UNROLL; u++) {
      grp[u] = g0 + u < groups ? g0 + u : groups - 1; // (uniform; a group past the end: nothing kept, addresses stay inside)
      const long long r = ((g0 + u) << 6) + lane;
      keep[u] = r < b.rows;
      rc[u] = keep[u] ? r : b.rows - 1;
    }
    if (fmode == 1) { // the conjunction: the columns of all terms requested first (a column named twice in a row: once), then the compares
      unsigned long long tx[SR_MAX_TERMS][SR_UNROLL];
      bool tok[SR_MAX_TERMS][SR_UNROLL];
#pragma unroll
      for (int t = 0; t < SR_MAX_TERMS; t++) {
        if (t >= nterms) continue; // (uniform)
        if (t > 0 && plan.terms[t].col == plan.terms[t - 1].col) {
#pragma unroll
          for (int u = 0; u < SR_UNROLL; u++) {
            tx[t][u] = tx[t > 0 ? t - 1 : 0][u];
            tok[t][u] = tok[t > 0 ? t - 1 : 0][u];
          }
        } else
          sr_load_rows(b, (int)plan.terms[t].col, rc, grp, keep, tx[t], tok[t]);
      }
#pragma unroll
      for (int t = 0; t < SR_MAX_TERMS; t++) {
        if (t >= nterms) continue;
        const SrTerm T = plan.terms[t];
#pragma unroll
        for (int u = 0; u < SR_UNROLL; u++) keep[u] = keep[u] && tok[t][u] && sr_term_holds(T, tx[t][u]);
      }
    } else if (PROGRAMS && fmode == 2) {
#pragma unroll
      for (int u = 0; u < SR_UNROLL; u++) {
        if (!keep[u]) continue;
        bool valid, d0 = false;
        const unsigned long long m = sa_eval_row<false>(plan.filter, SrLoad{b, rc[u]}, &valid, &d0);
        div0 |= d0;
        keep[u] = valid && m != 0;
      }
    }
#pragma unroll
    for (int a = 0; a < NARGS; a++) {
      unsigned long long x[SR_UNROLL];
      bool ok[SR_UNROLL];
      if (plan.arg_col[a] >= 0) sr_load_rows(b, plan.arg_col[a], rc, grp, keep, x, ok);
      else if (!PROGRAMS || plan.arg_op[a]) { // column OP column: both columns' kept rows requested together
        unsigned long long y[SR_UNROLL];
        bool oky[SR_UNROLL];
        sr_load_rows(b, plan.arg_c0[a], rc, grp, keep, x, ok);
        sr_load_rows(b, plan.arg_c1[a], rc, grp, keep, y, oky);
        const int op = plan.arg_op[a], dt = plan.arg_opdt[a];
#pragma unroll
        for (int u = 0; u < SR_UNROLL; u++) {
          x[u] = sr_binop(op, dt, x[u], y[u]);
          ok[u] = ok[u] && oky[u];
        }
      } else { // a program: the kept rows of its columns requested together when it names one or two, then evaluated from registers
        unsigned long long x1[SR_UNROLL];
        bool ok1[SR_UNROLL];
        const int c0 = plan.arg_c0[a], c1 = plan.arg_c1[a];
        const bool regs = c0 >= 0;
        if (regs) {
          sr_load_rows(b, c0, rc, grp, keep, x, ok);
          sr_load_rows(b, c1 >= 0 ? c1 : c0, rc, grp, keep, x1, ok1);
        }
#pragma unroll
        for (int u = 0; u < SR_UNROLL; u++) {
          const bool k = keep[u];
          bool valid = false, d0 = false;
          unsigned long long v = 0;
          if (k) {
            const uint32_t okbits = regs ? (ok[u] ? 1u : 0u) | (ok1[u] ? 2u : 0u) : 0u;
            v = sa_eval_row<false>(plan.arg[a], SrRegLoad{b, rc[u], regs ? x[u] : 0ull, regs ? x1[u] : 0ull, (uint32_t)c0, okbits, regs}, &valid, &d0);
          }
          div0 |= d0;
          x[u] = v;
          ok[u] = k && valid;
        }
      }
      const int need = plan.arg_need[a];
      const bool f64 = plan.arg_f64[a] != 0;
#pragma unroll
      for (int u = 0; u < SR_UNROLL; u++) { // (in row order: the order of a lane's additions is fixed)
        cnt[a] += ok[u] ? 1u : 0u;
        if (need & SR_NEED_SUM) {
          const unsigned long long s = f64 ? (unsigned long long)__double_as_longlong(__longlong_as_double((long long)sum[a]) + __longlong_as_double((long long)x[u])) : sum[a] + x[u];
          sum[a] = ok[u] ? s : sum[a];
        }
        if (need & SR_NEED_MINMAX) {
          const unsigned long long img = f64 ? f64_to_ordered(__longlong_as_double((long long)x[u])) : i64_to_ordered((long long)x[u]);
          mn[a] = ok[u] && img < mn[a] ? img : mn[a];
          mx[a] = ok[u] && img > mx[a] ? img : mx[a];
        }
      }
    }
  }
  // wave: butterflies, the same tree on every run
#pragma unroll
  for (int a = 0; a < NARGS; a++) {
    const bool f64 = plan.arg_f64[a] != 0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      cnt[a] += (uint32_t)__shfl_xor((int)cnt[a], m, 64);
      sum[a] = sr_combine(SR_SUM, f64, sum[a], shfl_xor_u64(sum[a], m));
      mn[a] = sr_combine(SR_MIN, false, mn[a], shfl_xor_u64(mn[a], m));
      mx[a] = sr_combine(SR_MAX, false, mx[a], shfl_xor_u64(mx[a], m));
    }
  }
  const bool wave_div0 = __ballot(div0) != 0;
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < NARGS; a++) {
      s_rec[wave][4 * a + SR_CNT] = cnt[a];
      s_rec[wave][4 * a + SR_SUM] = sum[a];
      s_rec[wave][4 * a + SR_MIN] = mn[a];
      s_rec[wave][4 * a + SR_MAX] = mx[a];
    }
    s_rec[wave][4 * SR_MAX_ARGS] = wave_div0 ? 1ull : 0ull;
  }
  __syncthreads();
  // workgroup: thread f folds field f of the 4 waves in wave order and stores it
  const int f = (int)threadIdx.x;
  if (f < 4 * NARGS || f == 4 * SR_MAX_ARGS) {
    const bool flag = f == 4 * SR_MAX_ARGS;
    const int kind = flag ? SR_MAX : (f & 3);
    const bool f64 = !flag && plan.arg_f64[f >> 2] != 0;
    unsigned long long v = s_rec[0][f];
#pragma unroll
    for (int w = 1; w < SR_THREADS / 64; w++) v = sr_combine(kind, f64, v, s_rec[w][f]);
    partial[(size_t)f * SR_MAX_BLOCKS + blockIdx.x] = v; // (field major: the fold reads a field of consecutive workgroups as one line)
  }
}

// `nblocks` partial records into `state`.  Field by field (the fields some argument owns, and the flag): lane j folds the
// records j, j + 64, j + 128, ... in that order — every lane's loads are independent and contiguous across the wave — then the 64
// lanes are combined by butterflies and lane 0 folds the result into the state cell: one fixed tree per (field, nblocks).
__global__ void __launch_bounds__(64) sr_fold_kernel(const SrPlan *__restrict__ plan, const unsigned long long *__restrict__ partial, int nblocks,
                                                     SrRecord *__restrict__ state) {
  const int lane = (int)threadIdx.x;
  const int nargs = plan->nargs;
  for (int f = 0; f < SR_FIELDS; f++) {
    const bool flag = f == 4 * SR_MAX_ARGS;
    if (!(f < 4 * nargs || flag)) continue;
    const int kind = flag ? SR_MAX : (f & 3);
    const bool f64 = !flag && plan->arg_f64[f >> 2] != 0;
    const unsigned long long *p = partial + (size_t)f * SR_MAX_BLOCKS;
    unsigned long long v = kind == SR_MIN ? ~0ull : 0ull; // (the neutral cell: a lane without a record changes nothing; +0.0 for a sum of doubles)
#pragma unroll 8
    for (int k = lane; k < nblocks; k += 64) v = sr_combine(kind, f64, v, p[k]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = sr_combine(kind, f64, v, shfl_xor_u64(v, m));
    if (lane == 0) state->w[f] = sr_combine(kind, f64, state->w[f], v);
  }
}
#endif

} // namespace sq
