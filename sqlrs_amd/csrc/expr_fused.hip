// expr_fused.hip — the fused-evaluation route of the synchronous Filter / Project (SQLRS_EXPR_FUSED_EVAL in `reserved` of the
// expression handed to sqlrs_filter_create / of exprs[0] of sqlrs_project_create; off by default).
//
// eval_expr (expr.hip) runs an expression node by node: a launch, a full-length temporary and — per constant — a full-length
// array per node, an and_words / bool_words launch per validity bitmap, and for a Filter the mask conversion on top.  Here the
// whole expression is compiled per push with sa_compile (small_async.hpp: the program the one-launch kernels of push_async,
// the async probe's join filter and sr_reduce_kernel already run) and evaluated row by row by ONE kernel
// (expr_fused_kernels.hpp) that reads the referenced columns once and writes the selection's mask words (Filter) or the
// computed columns and their validity bitmaps (Project, <= FE_MAX_PROGS columns per launch) directly.
//
// What compiles: sa_compile with `wide` over the batch's dtypes — Int32 / Int64 / Float64 / Boolean columns and constants as
// operands, an Int32 / Int64 / Float64 / Boolean result, <= SA_PROG_MAX nodes, <= SA_STACK_MAX operands in flight — minus
// anything with a Utf8 operand or constant (sa_cmp_utf8 reads both operands relative to ONE base pointer, the slot of a staged
// batch; over device columns every Utf8 column would need its own), and <= FE_MAX_COLS distinct columns per launch.  Whatever
// does not compile — and a referenced column that is not a plain column of the batch's length — returns false here: the caller
// takes the per-node route, which also raises whatever error there is to raise.
#include "common.hpp"
#include "device_utils.hpp"
#include "prims.hpp"
#include "expr_fused_kernels.hpp"

namespace sq {

namespace {

bool fe_result_type(int32_t d) { return d == SQLRS_INT32 || d == SQLRS_INT64 || d == SQLRS_FLOAT64 || d == SQLRS_BOOLEAN; }

// the columns one launch reads, renumbered in order of first mention
struct FeColumns {
  std::vector<int> plan_col; // batch column -> column of the launch, or -1
  std::vector<int> ref;      // column of the launch -> batch column
  explicit FeColumns(int ncols) : plan_col((size_t)ncols, -1) {}
};

// e -> *out over the batch's own column numbers; *has_div: the program holds a division
bool fe_compile(const Expr &e, InBatch &ib, SaProgram *out, bool *has_div) {
  const int nc = ib.num_columns();
  std::vector<int32_t> dt((size_t)nc);
  for (int c = 0; c < nc; c++) dt[(size_t)c] = ib.dtype(c);
  SaPool pool;
  if (!sa_compile(e, dt.data(), nc, out, true, &pool) || !fe_result_type(out->result_dtype)) return false;
  for (int k = 0; k < out->n; k++) {
    const SaInstr &I = out->ins[k];
    if (I.dtype == SQLRS_UTF8 || I.from == SQLRS_UTF8) return false;
    if (I.op == SAO_DIV) *has_div = true;
  }
  return true;
}

// the columns `pr` names join `cols` and the program is rewritten to the launch's numbering; false: more than FE_MAX_COLS
// columns, or a column the kernels cannot read as it is.  (`cols` may have grown when false comes back: the caller drops it.)
bool fe_bind(SaProgram *pr, InBatch &ib, FeColumns *cols) {
  for (int k = 0; k < pr->n; k++) {
    SaInstr &I = pr->ins[k];
    if (I.op != SAO_COL) continue;
    const int c = (int)I.col;
    if (cols->plan_col[(size_t)c] < 0) {
      if (cols->ref.size() >= (size_t)FE_MAX_COLS) return false;
      const DCol &d = ib.col(c);
      if (d.length != ib.rows() || d.stride != 1 || !d.values) return false;
      cols->plan_col[(size_t)c] = (int)cols->ref.size();
      cols->ref.push_back(c);
    }
    I.col = (uint32_t)cols->plan_col[(size_t)c];
  }
  return true;
}

FeBatch fe_batch(InBatch &ib, const FeColumns &cols) {
  FeBatch b;
  std::memset(&b, 0, sizeof(b));
  b.rows = ib.rows();
  for (size_t k = 0; k < cols.ref.size(); k++) {
    const DCol &d = ib.col(cols.ref[k]);
    b.c[k].values = d.values;
    b.c[k].validity = d.has_nulls() ? d.validity : nullptr;
    b.c[k].kind = d.dtype == SQLRS_BOOLEAN ? FE_KBOOL : width_of(d.dtype) == 8 ? FE_K64 : FE_K32;
  }
  return b;
}

unsigned fe_grid(int64_t rows) { return (unsigned)std::min<int64_t>(FE_MAX_BLOCKS, ceil_div(rows, FE_BLOCK_ROWS)); }

void fe_raise_div0(Ctx *ctx, const BufP &flag) {
  if (flag && ctx->fetch_value(flag->as<uint32_t>())) fail(SQLRS_ERR_ARROW, "Divide by zero error"); // (the evaluator's, expr.hip)
}

template <int N> void fe_launch_project(Ctx *ctx, const SaProgram *progs, const FeBatch &b, const FeOut *outs, uint32_t *flag) {
  FePrograms<N> pp;
  FeOuts<N> oo;
  for (int k = 0; k < N; k++) {
    pp.p[k] = progs[k];
    oo.o[k] = outs[k];
  }
  fe_project_kernel<N><<<dim3(fe_grid(b.rows)), dim3(FE_THREADS), 0, ctx->stream>>>(pp, b, oo, flag);
  SQ_HIP(hipGetLastError());
}

} // namespace

bool fused_filter_selection(Ctx *ctx, const Expr &e, InBatch &ib, Selection *sel) {
  const int64_t rows = ib.rows();
  if (rows <= 0 || rows >= (1ll << 31) || ib.num_columns() <= 0) return false;
  FePrograms<1> pp;
  bool has_div = false;
  FeColumns cols(ib.num_columns());
  if (!fe_compile(e, ib, &pp.p[0], &has_div) || pp.p[0].result_dtype != SQLRS_BOOLEAN || !fe_bind(&pp.p[0], ib, &cols)) return false;
  const FeBatch b = fe_batch(ib, cols);
  const int64_t nwords = ceil_div(rows, 64);
  sel->rows = rows;
  sel->own_bits = ctx->alloc(8 * (size_t)nwords + 8);
  sel->bits = sel->own_bits->as<uint64_t>();
  BufP flag = has_div ? ctx->alloc_zero(8) : nullptr;
  {
    ProfScope ps(ctx, "fused_eval_mask");
    fe_mask_kernel<<<dim3(fe_grid(rows)), dim3(FE_THREADS), 0, ctx->stream>>>(pp, b, sel->own_bits->as<uint64_t>(),
                                                                             flag ? flag->as<uint32_t>() : nullptr);
    SQ_HIP(hipGetLastError());
  }
  ctx->fused_eval_filter_batches++;
  fe_raise_div0(ctx, flag);
  selection_finish(ctx, *sel);
  return true;
}

bool fused_project_columns(Ctx *ctx, const std::vector<Expr> &exprs, InBatch &ib, std::vector<DCol> *out, std::vector<uint8_t> *computed) {
  const int64_t rows = ib.rows();
  if (rows <= 0 || rows >= (1ll << 31) || ib.num_columns() <= 0) return false;
  const size_t ne = exprs.size();
  std::vector<SaProgram> progs;
  std::vector<size_t> owner; // expression of program k
  bool has_div = false;
  for (size_t i = 0; i < ne; i++) {
    const Expr &e = exprs[i];
    if (e.nodes.size() == 1) { // a bare InputRef / constant keeps today's handling: nothing of it may fail behind a launch
      const sqlrs_expr_node_t &n = e.nodes[0];
      if (n.op == SQLRS_EXPR_INPUT_REF) {
        if (n.index < 0 || n.index >= ib.num_columns() || ib.col(n.index).length != rows) return false;
      } else if (n.op != SQLRS_EXPR_CONSTANT || !(fe_result_type(n.dtype) || n.dtype == SQLRS_UTF8))
        return false;
      continue;
    }
    SaProgram pr;
    if (!fe_compile(e, ib, &pr, &has_div)) return false;
    progs.push_back(pr);
    owner.push_back(i);
  }
  if (progs.empty()) return false;
  // launches of <= FE_MAX_PROGS programs over <= FE_MAX_COLS columns, all bound before the first one leaves
  struct Launch {
    size_t first, n;
    FeColumns cols;
  };
  std::vector<Launch> launches;
  for (size_t k = 0; k < progs.size(); k++) {
    if (!launches.empty() && launches.back().n < (size_t)FE_MAX_PROGS) {
      FeColumns trial = launches.back().cols;
      SaProgram pr = progs[k];
      if (fe_bind(&pr, ib, &trial)) {
        launches.back().cols = std::move(trial);
        launches.back().n++;
        progs[k] = pr;
        continue;
      }
    }
    Launch l{k, 1, FeColumns(ib.num_columns())};
    if (!fe_bind(&progs[k], ib, &l.cols)) return false;
    launches.push_back(std::move(l));
  }
  out->assign(ne, DCol());
  computed->assign(ne, 0);
  const int64_t nwords = ceil_div(rows, 64);
  std::vector<FeOut> outs(progs.size());
  for (size_t k = 0; k < progs.size(); k++) {
    DCol &o = (*out)[owner[k]];
    o.dtype = progs[k].result_dtype;
    o.length = rows;
    o.null_count = -1; // (as cast_col leaves it: counted by whoever needs it)
    const size_t w = width_of(o.dtype);
    o.own_values = ctx->alloc(w ? w * (size_t)rows + 16 : 8 * (size_t)nwords);
    o.values = o.own_values->p;
    o.own_validity = ctx->alloc(8 * (size_t)nwords);
    o.validity = o.own_validity->as<uint64_t>();
    outs[k].values = o.own_values->p;
    outs[k].validity = o.own_validity->as<uint64_t>();
    outs[k].kind = o.dtype == SQLRS_BOOLEAN ? FE_KBOOL : w == 8 ? FE_K64 : FE_K32;
    outs[k].pad = 0;
    (*computed)[owner[k]] = 1;
  }
  BufP flag = has_div ? ctx->alloc_zero(8) : nullptr;
  uint32_t *fp = flag ? flag->as<uint32_t>() : nullptr;
  for (const Launch &l : launches) {
    ProfScope ps(ctx, "fused_eval_project"); // (one scope per launch: the profile counts them)
    const FeBatch b = fe_batch(ib, l.cols);
    switch (l.n) {
    case 1: fe_launch_project<1>(ctx, &progs[l.first], b, &outs[l.first], fp); break;
    case 2: fe_launch_project<2>(ctx, &progs[l.first], b, &outs[l.first], fp); break;
    case 3: fe_launch_project<3>(ctx, &progs[l.first], b, &outs[l.first], fp); break;
    default: fe_launch_project<4>(ctx, &progs[l.first], b, &outs[l.first], fp); break;
    }
  }
  ctx->fused_eval_project_columns += (int64_t)progs.size();
  fe_raise_div0(ctx, flag);
  return true;
}

} // namespace sq
