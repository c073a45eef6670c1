// simple_reduce.hip — SimpleAgg's reduce route (SQLRS_SIMPLE_AGG_REDUCE in sqlrs_simple_agg_create): aggregates without GROUP BY as ONE streaming
// pass per pushed batch, the WHERE below them fused in [ref: simple_agg.rs:27-65 over filter.rs:13-25].
//
// The default SimpleAgg is a HashAgg over one constant key: it copies the key and argument columns of every batch, evaluates
// expression arguments and the filter node by node with temporaries, and resolves every row through the group table with
// global atomics on one group.  Here a push is two launches (simple_reduce_kernels.hpp) that read the bytes of the referenced
// columns once and leave the result in one SrRecord; the operator keeps that record, one partial record per workgroup and
// its compiled plan — nothing of a batch.
//
// The route is decided once, at the first batch (sr_decide): the arguments and the filter are compiled with sa_compile over
// the batch's Int32 / Int64 / Float64 columns — only the referenced columns, renumbered 0 .. n-1, which is also the batch a
// HostStage of the operator's own sees for small HOST batches.  A SUM's cast to its return type is part of the argument
// unless it changes nothing a register holds (the type itself, or Int32 -> Int64: the loader sign-extends), so
// `count(j), sum(j), min(j), max(j)` over an Int32 column is one argument with four cells.
#include "common.hpp"
#include "host_stage.hpp"
#include "device_utils.hpp"
#include "simple_agg_state.hpp"
#include "simple_reduce_kernels.hpp"

extern "C" {
void sqlrs_hash_agg_destroy(sqlrs_hash_agg_t *);
void sqlrs_batch_release(sqlrs_batch_t *);
}

namespace sq {

struct SrState {
  std::vector<int> ref_cols;       // plan column k = column ref_cols[k] of a pushed batch
  std::vector<int32_t> ref_dtypes; // ... and the type the first batch had there
  SrPlan plan;
  SrRecord init;
  BufP plan_d, state_d, partial_d;
  struct Out {
    int arg, cell;
    int32_t dtype;
  };
  std::vector<Out> outs; // per aggregate: the cell it reads and the type of its column
  HostStage stage;       // small HOST batches: the referenced columns only
};
void sr_destroy(SrState *s) { delete s; }

static bool numeric(int32_t d) { return d == SQLRS_INT32 || d == SQLRS_INT64 || d == SQLRS_FLOAT64; }
static bool same_nodes(const Expr &a, const Expr &b) {
  if (a.nodes.size() != b.nodes.size()) return false;
  for (size_t k = 0; k < a.nodes.size(); k++) {
    const sqlrs_expr_node_t &x = a.nodes[k], &y = b.nodes[k];
    if (x.op != y.op || x.dtype != y.dtype || x.index != y.index || x.is_null != y.is_null || x.i != y.i || std::memcmp(&x.f, &y.f, 8) != 0)
      return false;
  }
  return true;
}
// t1 [t2 AND [t3 AND [t4 AND]]] with every term COL CONST CMP (a non-NULL constant): the conjunction the kernel evaluates directly
static bool filter_terms(const SaProgram &pr, SrPlan *plan) {
  if (pr.n < 3 || (pr.n - 3) % 4 != 0) return false;
  const int nterms = 1 + (pr.n - 3) / 4;
  if (nterms > SR_MAX_TERMS) return false;
  for (int k = 0; k < nterms; k++) {
    const int at = k == 0 ? 0 : 3 + (k - 1) * 4;
    const SaInstr &c = pr.ins[at], &v = pr.ins[at + 1], &o = pr.ins[at + 2];
    if (k > 0 && pr.ins[at + 3].op != SAO_AND) return false;
    if (c.op != SAO_COL || v.op != SAO_CONST || v.is_null || o.op < SAO_GT || o.op > SAO_NE || !numeric(o.dtype)) return false;
    SrTerm &t = plan->terms[k];
    t.col = c.col;
    t.op = o.op;
    t.is_f64 = o.dtype == SQLRS_FLOAT64;
    t.pad = 0;
    t.imm = t.is_f64 ? ((v.imm >> 63) ? ~v.imm : (v.imm | (1ull << 63))) : v.imm; // (f64_to_ordered, device_utils.hpp)
  }
  plan->nterms = nterms;
  return true;
}

bool sr_decide(sqlrs_simple_agg *a, const sqlrs_batch_t *first) {
  if (!a->reduce || !first || first->num_columns <= 0 || a->funcs.empty()) return false;
  for (size_t i = 0; i < a->funcs.size(); i++)
    if (a->distinct[i] || a->funcs[i] < SQLRS_AGG_COUNT || a->funcs[i] > SQLRS_AGG_MAX) return false;
  auto s = std::unique_ptr<SrState>(new SrState());
  // the referenced columns, renumbered in order of first mention
  std::vector<int> plan_col((size_t)first->num_columns, -1);
  auto renumber = [&](Expr e, Expr *out) {
    for (sqlrs_expr_node_t &nd : e.nodes) {
      if (nd.op != SQLRS_EXPR_INPUT_REF) continue;
      if (nd.index < 0 || nd.index >= first->num_columns || !numeric(first->columns[nd.index].dtype)) return false;
      if (plan_col[(size_t)nd.index] < 0) {
        if (s->ref_cols.size() >= (size_t)SR_MAX_COLS) return false;
        plan_col[(size_t)nd.index] = (int)s->ref_cols.size();
        s->ref_cols.push_back(nd.index);
        s->ref_dtypes.push_back(first->columns[nd.index].dtype);
      }
      nd.index = plan_col[(size_t)nd.index];
    }
    *out = std::move(e);
    return true;
  };
  std::vector<Expr> args(a->args.size());
  for (size_t i = 0; i < a->args.size(); i++)
    if (!renumber(a->args[i], &args[i])) return false;
  Expr filter;
  if (!a->filter.empty() && !renumber(a->filter, &filter)) return false;
  if (s->ref_cols.empty()) return false;
  const int32_t *dt = s->ref_dtypes.data();
  const int nc = (int)s->ref_dtypes.size();
  SrPlan &plan = s->plan;
  std::memset((void *)&plan, 0, sizeof(plan));
  std::vector<Expr> arg_expr; // of the plan's arguments, before the cast
  std::vector<int32_t> arg_cast;
  for (size_t i = 0; i < args.size(); i++) {
    SaProgram natural;
    if (!sa_compile(args[i], dt, nc, &natural) || !numeric(natural.result_dtype)) return false;
    const int32_t nat = natural.result_dtype;
    int32_t cast = a->funcs[i] == SQLRS_AGG_SUM ? a->return_dtypes[i] : 0;
    if (cast == nat || (cast == SQLRS_INT64 && nat == SQLRS_INT32)) cast = 0;
    if (cast && !numeric(cast)) return false;
    const int32_t value_dtype = cast ? cast : nat;
    if ((a->funcs[i] == SQLRS_AGG_MIN || a->funcs[i] == SQLRS_AGG_MAX) && a->return_dtypes[i] != value_dtype) return false;
    int found = -1;
    for (size_t k = 0; k < arg_expr.size(); k++)
      if (arg_cast[k] == cast && same_nodes(arg_expr[k], args[i])) found = (int)k;
    if (found < 0) {
      if (arg_expr.size() >= (size_t)SR_MAX_ARGS) return false;
      found = (int)arg_expr.size();
      Expr e = args[i];
      if (cast) {
        sqlrs_expr_node_t cn;
        std::memset(&cn, 0, sizeof(cn));
        cn.op = SQLRS_EXPR_TYPE_CAST;
        cn.dtype = cast;
        e.nodes.push_back(cn);
        e.strings.emplace_back();
      }
      if (!sa_compile(e, dt, nc, &plan.arg[found]) || plan.arg[found].result_dtype != value_dtype) return false;
      const SaProgram &pr = plan.arg[found];
      plan.arg_col[found] = pr.n == 1 && pr.ins[0].op == SAO_COL ? (int)pr.ins[0].col : -1;
      plan.arg_f64[found] = value_dtype == SQLRS_FLOAT64;
      plan.arg_c0[found] = plan.arg_c1[found] = -1;
      bool few = true;
      for (int k = 0; k < pr.n && few; k++) {
        if (pr.ins[k].op != SAO_COL) continue;
        const int c = (int)pr.ins[k].col;
        if (plan.arg_c0[found] < 0 || plan.arg_c0[found] == c) plan.arg_c0[found] = c;
        else if (plan.arg_c1[found] < 0 || plan.arg_c1[found] == c) plan.arg_c1[found] = c;
        else few = false;
      }
      if (!few) plan.arg_c0[found] = plan.arg_c1[found] = -1;
      if (pr.n == 3 && pr.ins[0].op == SAO_COL && pr.ins[1].op == SAO_COL && pr.ins[2].op >= SAO_ADD && pr.ins[2].op <= SAO_MUL) {
        plan.arg_op[found] = pr.ins[2].op; // column OP column: evaluated without the interpreter
        plan.arg_opdt[found] = pr.ins[2].dtype;
        plan.arg_c0[found] = (int)pr.ins[0].col;
        plan.arg_c1[found] = (int)pr.ins[1].col;
      }
      arg_expr.push_back(args[i]);
      arg_cast.push_back(cast);
    }
    SrState::Out o;
    o.arg = found;
    o.cell = a->funcs[i] == SQLRS_AGG_COUNT ? SR_CNT : a->funcs[i] == SQLRS_AGG_SUM ? SR_SUM : a->funcs[i] == SQLRS_AGG_MIN ? SR_MIN : SR_MAX;
    o.dtype = a->funcs[i] == SQLRS_AGG_COUNT ? SQLRS_INT64 : a->funcs[i] == SQLRS_AGG_SUM ? a->return_dtypes[i] : value_dtype;
    if (a->funcs[i] == SQLRS_AGG_SUM && o.dtype != (plan.arg_f64[found] ? SQLRS_FLOAT64 : SQLRS_INT64)) return false;
    plan.arg_need[found] |= o.cell == SR_SUM ? SR_NEED_SUM : o.cell == SR_CNT ? 0 : SR_NEED_MINMAX;
    s->outs.push_back(o);
  }
  plan.nargs = (int)arg_expr.size();
  if (!filter.empty()) {
    if (!sa_compile(filter, dt, nc, &plan.filter) || plan.filter.result_dtype != SQLRS_BOOLEAN) return false;
    plan.filter_mode = filter_terms(plan.filter, &plan) ? 1 : 2;
  }
  Ctx *ctx = a->ctx;
  SQ_HIP(hipSetDevice(ctx->device));
  sr_init_record(&s->init);
  s->plan_d = ctx->alloc(sizeof(SrPlan));
  s->state_d = ctx->alloc(sizeof(SrRecord));
  s->partial_d = ctx->alloc(sizeof(SrRecord) * (size_t)SR_MAX_BLOCKS);
  SQ_HIP(hipMemcpyAsync(s->plan_d->p, &s->plan, sizeof(SrPlan), hipMemcpyHostToDevice, ctx->stream));
  SQ_HIP(hipMemcpyAsync(s->state_d->p, &s->init, sizeof(SrRecord), hipMemcpyHostToDevice, ctx->stream));
  s->stage.ctx = ctx;
  a->sr = s.release();
  return true;
}

// `cols`: the referenced columns of one batch, device resident, in the plan's numbering
static void sr_reduce_device(sqlrs_simple_agg *a, int64_t rows, const DCol *const *cols) {
  if (rows <= 0) return;
  Ctx *ctx = a->ctx;
  SrState *s = a->sr;
  SrBatch b;
  std::memset(&b, 0, sizeof(b));
  b.ncols = (int)s->ref_cols.size();
  b.rows = rows;
  for (int k = 0; k < b.ncols; k++) {
    const DCol &c = *cols[k];
    if (c.dtype != s->ref_dtypes[(size_t)k] || c.length != rows || c.stride != 1) fail(SQLRS_ERR_ARROW, "concat_batches: schema mismatch");
    b.values[k] = c.values;
    b.validity[k] = c.has_nulls() ? c.validity : nullptr;
    if (width_of(c.dtype) == 8) b.width8 |= 1u << k;
  }
  const int blocks = (int)std::min<int64_t>(SR_MAX_BLOCKS, ceil_div(rows, SR_BLOCK_ROWS));
  const SrPlan *plan = s->plan_d->as<SrPlan>();
  unsigned long long *partial = s->partial_d->as<unsigned long long>(); // [SR_FIELDS][SR_MAX_BLOCKS]
  ProfScope prof(ctx, "simple_reduce");
  bool programs = s->plan.filter_mode == 2;
  for (int k = 0; k < s->plan.nargs; k++) programs = programs || (s->plan.arg_col[k] < 0 && !s->plan.arg_op[k]);
  const dim3 grid((unsigned)blocks), wg(SR_THREADS);
#define SR_LAUNCH(N)                                                                       \
  if (programs) sr_reduce_kernel<N, true><<<grid, wg, 0, ctx->stream>>>(plan, b, partial); \
  else sr_reduce_kernel<N, false><<<grid, wg, 0, ctx->stream>>>(plan, b, partial)
  switch (s->plan.nargs) {
  case 1: SR_LAUNCH(1); break;
  case 2: SR_LAUNCH(2); break;
  case 3: SR_LAUNCH(3); break;
  default: SR_LAUNCH(4); break;
  }
#undef SR_LAUNCH
  SQ_HIP(hipGetLastError());
  sr_fold_kernel<<<dim3(1), dim3(64), 0, ctx->stream>>>(plan, partial, blocks, s->state_d->as<SrRecord>());
  SQ_HIP(hipGetLastError());
}

static void sr_flush_stage(sqlrs_simple_agg *a) {
  SrState *s = a->sr;
  if (!s->stage.has_schema) return;
  sqlrs_batch_t *dev = s->stage.take();
  if (!dev) return;
  try {
    InBatch ib(a->ctx, dev);
    std::vector<const DCol *> cols;
    for (int k = 0; k < ib.num_columns(); k++) cols.push_back(&ib.col(k));
    sr_reduce_device(a, ib.rows(), cols.data());
  } catch (...) {
    sqlrs_batch_release(dev);
    throw;
  }
  sqlrs_batch_release(dev);
}

void sr_push(sqlrs_simple_agg *a, const sqlrs_batch_t *in) {
  Ctx *ctx = a->ctx;
  SrState *s = a->sr;
  SQ_HIP(hipSetDevice(ctx->device));
  if (!in || in->num_rows < 0 || in->num_rows >= (1ll << 31)) fail(SQLRS_ERR_ARROW, "batch of a row count outside [0, 2^31)");
  const size_t nc = s->ref_cols.size();
  // the projected view: the referenced columns under the plan's numbering
  std::vector<sqlrs_column_t> view_cols(nc);
  for (size_t k = 0; k < nc; k++) {
    const int c = s->ref_cols[k];
    if (c >= in->num_columns || in->columns[c].dtype != s->ref_dtypes[k]) fail(SQLRS_ERR_ARROW, "concat_batches: schema mismatch");
    view_cols[k] = in->columns[c];
  }
  sqlrs_batch_t view = *in;
  view.num_columns = (int32_t)nc;
  view.columns = view_cols.data();
  view.owner = nullptr;
  ctx->simple_reduce_batches++;
  if (s->stage.accepts(&view)) {
    s->stage.append(&view);
    if (s->stage.rows >= HOST_STAGE_FLUSH_ROWS) sr_flush_stage(a);
    return;
  }
  sr_flush_stage(a); // (batches fold in push order)
  if (in->num_rows == 0) return;
  InBatch ib(ctx, &view); // HOST columns: uploaded once, read before the call returns
  std::vector<const DCol *> cols;
  for (size_t k = 0; k < nc; k++) cols.push_back(&ib.col((int)k));
  sr_reduce_device(a, ib.rows(), cols.data());
}

void sr_finish(sqlrs_simple_agg *a, int out_mem, sqlrs_batch_t **out) {
  Ctx *ctx = a->ctx;
  SrState *s = a->sr;
  SQ_HIP(hipSetDevice(ctx->device));
  if (out_mem != SQLRS_MEM_HOST && out_mem != SQLRS_MEM_DEVICE) fail(SQLRS_ERR_INTERNAL, "bad out_mem");
  sr_flush_stage(a);
  SrRecord r = *(const SrRecord *)ctx->fetch(s->state_d->p, sizeof(SrRecord));
  if (r.w[4 * SR_MAX_ARGS]) fail(SQLRS_ERR_ARROW, "Divide by zero error"); // (what the evaluator raises, expr.hip)
  const size_t n = s->outs.size();
  std::vector<unsigned long long> vals(n, 0);
  std::vector<uint8_t> valid(n, 1);
  std::vector<int32_t> dtypes(n);
  std::vector<int64_t> nulls(n, 0);
  std::vector<const void *> vptr(n);
  std::vector<const uint8_t *> bptr(n);
  for (size_t i = 0; i < n; i++) {
    const SrState::Out &o = s->outs[i];
    const unsigned long long cnt = r.w[4 * o.arg + SR_CNT], cell = r.w[4 * o.arg + o.cell];
    dtypes[i] = o.dtype;
    if (o.cell == SR_CNT) vals[i] = cnt;
    else if (!cnt) {
      valid[i] = 0;
      nulls[i] = 1;
    } else if (o.cell == SR_SUM) vals[i] = cell;
    else if (s->plan.arg_f64[o.arg]) vals[i] = (cell >> 63) ? (cell & ~(1ull << 63)) : ~cell; // ordered_to_f64
    else {
      const long long v = (long long)(cell ^ (1ull << 63)); // ordered_to_i64
      if (o.dtype == SQLRS_INT32) {
        const int32_t v32 = (int32_t)v;
        std::memcpy(&vals[i], &v32, 4);
      } else vals[i] = (unsigned long long)v;
    }
    vptr[i] = &vals[i];
    bptr[i] = valid[i] ? nullptr : &valid[i];
  }
  if (out_mem == SQLRS_MEM_HOST) {
    *out = emit_host_copy(ctx, (int)n, dtypes.data(), 1, vptr.data(), bptr.data(), nulls.data());
    return;
  }
  DBatch o;
  o.rows = 1;
  for (size_t i = 0; i < n; i++) {
    sqlrs_column_t c;
    std::memset(&c, 0, sizeof(c));
    c.dtype = dtypes[i];
    c.mem = SQLRS_MEM_HOST;
    c.length = 1;
    c.null_count = nulls[i];
    c.values = vptr[i];
    c.validity = bptr[i];
    o.cols.push_back(upload_column(ctx, c, true));
  }
  ctx->sync(); // (the uploads read this frame's vectors)
  *out = emit_batch(ctx, std::move(o), out_mem);
}

} // namespace sq

sqlrs_simple_agg::~sqlrs_simple_agg() {
  if (inner) sqlrs_hash_agg_destroy(inner);
  if (sr) sq::sr_destroy(sr);
}
