// simple_agg_state.hpp — the SimpleAgg operator (plumbing.hip: its entry points) and the hooks of its reduce route
// (simple_reduce.hip: SQLRS_SIMPLE_AGG_REDUCE).
#pragma once

#include "common.hpp"

namespace sq {
struct SrState; // simple_reduce.hip
}

struct sqlrs_simple_agg {
  sq::Ctx *ctx = nullptr;
  sqlrs_hash_agg_t *inner = nullptr; // HashAgg over one constant key: same accumulators, one group
  std::vector<int32_t> funcs, return_dtypes;
  bool saw_batch = false;
  // the reduce route: the switch, what it needs of the create call, and — once the first batch has decided — its state
  bool reduce = false, decided = false;
  std::vector<int32_t> distinct;
  std::vector<sq::Expr> args;
  sq::Expr filter; // the SQLRS_SIMPLE_AGG_FILTER entry of the create call (empty: none); with the route off it lives in `inner`
  sq::SrState *sr = nullptr; // non-null: the route serves the operator
  ~sqlrs_simple_agg();
};

namespace sq {
// decides at the first batch; true: a->sr is set and every push / the finish go through the two calls below
bool sr_decide(sqlrs_simple_agg *a, const sqlrs_batch_t *first);
void sr_push(sqlrs_simple_agg *a, const sqlrs_batch_t *in);
void sr_finish(sqlrs_simple_agg *a, int out_mem, sqlrs_batch_t **out);
void sr_destroy(SrState *s);
} // namespace sq
