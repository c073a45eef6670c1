// fused_eval_check.cpp — PhysicalProject(PhysicalFilter(scan)) through ExecutorBuilder, once as the builder makes it by default
// (every expression node by node) and once with `fused_eval` (SQLRS_EXPR_FUSED_EVAL: the predicate and the computed columns as
// one program kernel each per batch):
//
//   select i, i * v - i, f * 2 + cast(v as double), i + v > 5000 from t where i + v > 4000 or f < 10
//
// over 200 003 rows in 1024-row batches [ref: src/storage/csv.rs:105].  Every value is a small integer — the doubles too — and
// both routes compute a row the same way, so the two outputs must be equal as text.  The profile counts say which route ran.
//
// Build: make -C host fused_eval_check.  Run on a machine with an MI355X (pytest -m gpu does both).
#include <cstdio>

#include "sqlrs_executor.hpp"

using namespace sqlrs;

static int64_t count_of(sqlrs_ctx_t *c, const char *name) {
  const char *names[1024]; double ms[1024]; int64_t count[1024];
  const int n = sqlrs_ctx_profile_read(c, 1024, names, ms, count);
  for (int i = 0; i < n && i < 1024; i++) if (std::string(names[i]) == name) return count[i];
  return 0;
}

int main() {
  HipCtxRef ctx;
  try {
    ctx = std::make_shared<HipCtx>(0);
  } catch (const ExecutorError &e) {
    std::printf("no device: %s\n", e.what());
    return 2;
  }
  auto sch = std::make_shared<Schema>(Schema{{"i", DataType::Int64, false}, {"v", DataType::Int64, false}, {"f", DataType::Float64, false}});
  const int64_t n = 200003, batch = 1024;
  std::vector<RecordBatch> scan;
  uint64_t x = 88172645463325252ull;
  auto rnd = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  for (int64_t at = 0; at < n; at += batch) {
    const int64_t m = std::min(batch, n - at);
    std::vector<int64_t> i((size_t)m), v((size_t)m);
    std::vector<double> f((size_t)m);
    for (int64_t r = 0; r < m; r++) {
      i[(size_t)r] = (int64_t)(rnd() % 10000);
      v[(size_t)r] = (int64_t)(rnd() % 2001) - 1000;
      f[(size_t)r] = (double)(int64_t)(rnd() % 100);
    }
    scan.push_back(RecordBatch::try_new(sch, {Int64Array(i), Int64Array(v), Float64Array(f)}));
  }
  auto col = [](int c) { return build_bound_input_ref((size_t)c); };
  auto bin = [](BinaryOperator op, BoundExpr l, BoundExpr r) { return BoundExpr::binary_op(op, std::move(l), std::move(r)); };
  auto make_plan = [&] {
    BoundExpr where = bin(BinaryOperator::Or, bin(BinaryOperator::Gt, bin(BinaryOperator::Plus, col(0), col(1)), BoundExpr::constant(ScalarValue::Int64(4000))),
                          bin(BinaryOperator::Lt, col(2), BoundExpr::constant(ScalarValue::Float64(10.0))));
    std::vector<BoundExpr> exprs = {
        col(0), bin(BinaryOperator::Minus, bin(BinaryOperator::Multiply, col(0), col(1)), col(0)),
        bin(BinaryOperator::Plus, bin(BinaryOperator::Multiply, col(2), BoundExpr::constant(ScalarValue::Float64(2.0))), BoundExpr::type_cast(col(1), DataType::Float64)),
        bin(BinaryOperator::Gt, bin(BinaryOperator::Plus, col(0), col(1)), BoundExpr::constant(ScalarValue::Int64(5000)))};
    return PlanNode::project(exprs, PlanNode::filter(where, PlanNode::table_scan(scan)), {"i", "i * v - i", "f * 2 + v", "i + v > 5000"});
  };
  int failures = 0;
  try {
    ExecutorBuilder off{ctx}, on{ctx};
    on.fused_eval = true;
    const int64_t f0 = count_of(ctx->raw, "fused_eval_filter_batches"), p0 = count_of(ctx->raw, "fused_eval_project_columns");
    auto a = try_collect(off.build(make_plan()));
    const int64_t f1 = count_of(ctx->raw, "fused_eval_filter_batches"), p1 = count_of(ctx->raw, "fused_eval_project_columns");
    auto b = try_collect(on.build(make_plan()));
    const int64_t f2 = count_of(ctx->raw, "fused_eval_filter_batches"), p2 = count_of(ctx->raw, "fused_eval_project_columns");
    const std::string ta = pretty_format_batches(a), tb = pretty_format_batches(b);
    int64_t rows = 0;
    for (auto &r : b) rows += r.num_rows();
    std::printf("%lld rows in %zu batches\n", (long long)rows, b.size());
    if (a.size() != scan.size() || b.size() != scan.size() || rows <= 0 || rows >= n || ta != tb) {
      failures++;
      std::printf("FAIL the two routes differ (%zu / %zu batches, %zu / %zu characters)\n", a.size(), b.size(), ta.size(), tb.size());
    }
    if (f1 != f0 || p1 != p0) { failures++; std::printf("FAIL the program kernels ran without fused_eval\n"); }
    if (f2 - f1 != (int64_t)scan.size() || p2 - p1 != 3 * (int64_t)scan.size()) {
      failures++;
      std::printf("FAIL fused batches %lld, columns %lld, expected %zu and %zu\n", (long long)(f2 - f1), (long long)(p2 - p1), scan.size(), 3 * scan.size());
    }
  } catch (const ExecutorError &e) {
    failures++;
    std::printf("FAIL %s\n", e.what());
  }
  std::printf("%s (%d failure%s)\n", failures ? "FAILED" : "PASSED", failures, failures == 1 ? "" : "s");
  return failures ? 1 : 0;
}
