// simple_agg_reduce_check.cpp — PhysicalSimpleAgg(PhysicalFilter(scan)) through ExecutorBuilder, once as the builder makes it
// by default (the Filter's expression handed to SimpleAggExecutor, the operator a HashAgg over one constant key) and once with
// `simple_agg_reduce` (SQLRS_SIMPLE_AGG_REDUCE: one streaming kernel per batch, the predicate inside it):
//
//   select count(v), sum(v), min(v), max(v), sum(i * v), sum(f), min(f) from t where i >= 100 and i < 9000 and f < 50
//
// over 200 003 rows in 1024-row batches [ref: src/storage/csv.rs:105].  Every value is a small integer — the doubles too — so every
// sum is exact in any order and the two one-row results must be equal as text.
//
// Build: make -C host simple_agg_reduce_check.  Run on a machine with an MI355X (pytest -m gpu does both).
#include <cstdio>

#include "sqlrs_executor.hpp"

using namespace sqlrs;

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
  auto cmp = [](BinaryOperator op, int col, ScalarValue c) { return BoundExpr::binary_op(op, build_bound_input_ref((size_t)col), BoundExpr::constant(std::move(c))); };
  auto make_plan = [&] {
    BoundExpr where = BoundExpr::binary_op(
        BinaryOperator::And,
        BoundExpr::binary_op(BinaryOperator::And, cmp(BinaryOperator::GtEq, 0, ScalarValue::Int64(100)), cmp(BinaryOperator::Lt, 0, ScalarValue::Int64(9000))),
        cmp(BinaryOperator::Lt, 2, ScalarValue::Float64(50.0)));
    BoundExpr iv = BoundExpr::binary_op(BinaryOperator::Multiply, build_bound_input_ref(0), build_bound_input_ref(1));
    return PlanNode::simple_agg({BoundAggFunc{AggFunc::Count, {build_bound_input_ref(1)}, DataType::Int64, false},
                                 BoundAggFunc{AggFunc::Sum, {build_bound_input_ref(1)}, DataType::Int64, false},
                                 BoundAggFunc{AggFunc::Min, {build_bound_input_ref(1)}, DataType::Int64, false},
                                 BoundAggFunc{AggFunc::Max, {build_bound_input_ref(1)}, DataType::Int64, false},
                                 BoundAggFunc{AggFunc::Sum, {iv}, DataType::Int64, false},
                                 BoundAggFunc{AggFunc::Sum, {build_bound_input_ref(2)}, DataType::Float64, false},
                                 BoundAggFunc{AggFunc::Min, {build_bound_input_ref(2)}, DataType::Float64, false}},
                                PlanNode::filter(where, PlanNode::table_scan(scan)),
                                {"Count(v)", "Sum(v)", "Min(v)", "Max(v)", "Sum(i * v)", "Sum(f)", "Min(f)"});
  };
  int failures = 0;
  try {
    ExecutorBuilder off{ctx}, on{ctx};
    on.simple_agg_reduce = true;
    auto a = try_collect(off.build(make_plan()));
    auto b = try_collect(on.build(make_plan()));
    const std::string ta = pretty_format_batches(a), tb = pretty_format_batches(b);
    std::printf("%s\n", tb.c_str());
    if (a.size() != 1 || b.size() != 1 || a[0].num_rows() != 1 || b[0].num_rows() != 1 || ta != tb) {
      failures++;
      std::printf("FAIL the two routes differ; without simple_agg_reduce:\n%s\n", ta.c_str());
    }
    if (off.rewrites != 1 || on.rewrites != 1) { failures++; std::printf("FAIL peephole: rewrites %d / %d\n", off.rewrites, on.rewrites); }
    if (off.last_reduced_batches != 0 || on.last_reduced_batches != (int64_t)scan.size()) {
      failures++;
      std::printf("FAIL reduced batches %lld / %lld, expected 0 / %zu\n", (long long)off.last_reduced_batches, (long long)on.last_reduced_batches, scan.size());
    }
  } catch (const ExecutorError &e) {
    failures++;
    std::printf("FAIL %s\n", e.what());
  }
  std::printf("%s (%d failure%s)\n", failures ? "FAILED" : "PASSED", failures, failures == 1 ? "" : "s");
  return failures ? 1 : 0;
}
