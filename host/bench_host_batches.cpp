// bench_host_batches.cpp — HashAgg fed the reference's batch shape by a NATIVE caller: 19 532 pageable host batches
// of 1024 rows (storage/csv.rs:105) through sqlrs_hash_agg_push, result on the host.  What a Rust drop-in pays per
// batch — a C call, no interpreter — next to bench.py's `C4_host_batches_1024`, whose wall clock includes one Python
// ctypes call per batch.  Prints one JSON object; `bench.py` adds it to the line as `C4_host_batches_1024_native`.
//   ./bench_host_batches [rows = 2e7] [groups = 1e6] [batch = 1024]
//   ./bench_host_batches filter ... | probe ...   the streaming operators at the same batch shape (see bench_filter / bench_probe)
//   ./bench_host_batches probe_general ...         outer joins / duplicate build keys through push_async (see bench_probe_general)
//   ./bench_host_batches probe_keys ...            Utf8 keys, two-column keys, NULL probe keys through push_async (see bench_probe_keys)
//   ./bench_host_batches filter_all_types ...      Utf8 / Boolean predicates through push_async (see bench_filter_all_types)
//   ./bench_host_batches stage_types ...           the blocking operators over Utf8 / Boolean / NULL-bearing batches, SQLRS_EXPR_STAGE_ALL_TYPES off and on (see bench_stage_types)
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sqlrs_hip.h"

static uint64_t splitmix64(uint64_t seed, uint64_t i) { // the generator of sqlrs_amd/datagen.py
  uint64_t z = seed * 0x9E3779B97F4A7C15ull + (i + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
#define CHECK(x)                                                                                  \
  do {                                                                                            \
    int st_ = (x);                                                                                \
    if (st_ != SQLRS_OK) {                                                                        \
      std::fprintf(stderr, "%s failed (%d): %s\n", #x, st_, ctx ? sqlrs_last_error(ctx) : "");    \
      return 1;                                                                                   \
    }                                                                                             \
  } while (0)

static void host_col(sqlrs_column_t &c, int32_t dtype, const void *values, int64_t m) {
  std::memset(&c, 0, sizeof(c));
  c.dtype = dtype;
  c.mem = SQLRS_MEM_HOST;
  c.length = m;
  c.values = values;
}

// ./bench_host_batches filter [rows = 2e7] [batch = 1024] [group = 1024]
// FilterExecutor (C2's query: SELECT v1 FROM t WHERE v1 > k, selectivity 0.5) fed pageable 1024-row host batches by a native
// caller, result batches on the host: (a) one sqlrs_filter_push per batch, (b) sqlrs_filter_push_many over groups of batches.
static int bench_filter(int argc, char **argv) {
  const int64_t n = argc > 2 ? (int64_t)std::atof(argv[2]) : 20000000, B = argc > 3 ? std::atoll(argv[3]) : 1024;
  const int group = argc > 4 ? std::atoi(argv[4]) : 1024;
  sqlrs_ctx_t *ctx = nullptr;
  if (sqlrs_ctx_create(0, &ctx) != SQLRS_OK) {
    std::printf("{\"error\": \"no device\"}\n");
    return 2;
  }
  std::vector<int64_t> v((size_t)n);
  int64_t expect = 0;
  const int64_t k = (1ll << 30);
  for (int64_t i = 0; i < n; i++) {
    v[(size_t)i] = (int64_t)(splitmix64(0xC2, (uint64_t)i) % (1ull << 31));
    expect += v[(size_t)i] > k;
  }
  sqlrs_expr_node_t nodes[3] = {};
  nodes[0].op = SQLRS_EXPR_INPUT_REF;
  nodes[0].index = 0;
  nodes[1].op = SQLRS_EXPR_CONSTANT;
  nodes[1].dtype = SQLRS_INT64;
  nodes[1].i = k;
  nodes[2].op = SQLRS_EXPR_GT;
  sqlrs_expr_t pred{nodes, 3, 0};
  const int64_t nb = (n + B - 1) / B;
  std::vector<sqlrs_column_t> cols((size_t)nb);
  std::vector<sqlrs_batch_t> batches((size_t)nb);
  std::vector<const sqlrs_batch_t *> ptrs((size_t)nb);
  for (int64_t b = 0; b < nb; b++) {
    const int64_t m = std::min<int64_t>(B, n - b * B);
    host_col(cols[(size_t)b], SQLRS_INT64, v.data() + b * B, m);
    std::memset(&batches[(size_t)b], 0, sizeof(sqlrs_batch_t));
    batches[(size_t)b].num_rows = m;
    batches[(size_t)b].num_columns = 1;
    batches[(size_t)b].columns = &cols[(size_t)b];
    ptrs[(size_t)b] = &batches[(size_t)b];
  }
  double best[3] = {1e30, 1e30, 1e30};
  int64_t kept[3] = {0, 0, 0};
  bool order_ok = true;
  const int DEPTH = 8; // tickets in flight of the async mode (the caller waits that many batches behind)
  for (int mode = 0; mode < 3; mode++) {
    for (int rep = 0; rep < 3; rep++) {
      auto t0 = std::chrono::steady_clock::now();
      sqlrs_filter_t *f = nullptr;
      CHECK(sqlrs_filter_create(ctx, &pred, &f));
      int64_t got = 0;
      std::vector<sqlrs_batch_t *> outs((size_t)group);
      if (mode == 0) {
        for (int64_t b = 0; b < nb; b++) {
          sqlrs_batch_t *o = nullptr;
          CHECK(sqlrs_filter_push(f, ptrs[(size_t)b], SQLRS_MEM_HOST, &o));
          got += o->num_rows;
          sqlrs_batch_release(o);
        }
      } else if (mode == 2) { // one batch per call, no synchronisation per call: sqlrs_filter_push_async + sqlrs_batch_wait
        std::vector<sqlrs_ticket_t *> q((size_t)DEPTH, nullptr);
        auto take = [&](int64_t b) { // the batch of input batch b
          sqlrs_batch_t *o = nullptr;
          CHECK(sqlrs_batch_wait(q[(size_t)(b % DEPTH)], &o));
          const int64_t m = o->num_rows;
          if (rep == 0 && m) {
            const int64_t *ov = (const int64_t *)o->columns[0].values;
            const int64_t *iv = v.data() + b * B;
            int64_t j = 0;
            for (int64_t r = 0; r < batches[(size_t)b].num_rows && j < m; r++)
              if (iv[r] > k) order_ok = order_ok && ov[j++] == iv[r];
            order_ok = order_ok && j == m;
          }
          got += m;
          sqlrs_batch_release(o);
          return 0;
        };
        for (int64_t b = 0; b < nb; b++) {
          if (b >= DEPTH && take(b - DEPTH)) return 1;
          CHECK(sqlrs_filter_push_async(f, ptrs[(size_t)b], &q[(size_t)(b % DEPTH)]));
        }
        for (int64_t b = std::max<int64_t>(0, nb - DEPTH); b < nb; b++)
          if (take(b)) return 1;
      } else {
        for (int64_t b0 = 0; b0 < nb; b0 += group) {
          const int g = (int)std::min<int64_t>(group, nb - b0);
          CHECK(sqlrs_filter_push_many(f, g, ptrs.data() + b0, SQLRS_MEM_HOST, outs.data()));
          for (int i = 0; i < g; i++) {
            const int64_t m = outs[(size_t)i]->num_rows;
            if (rep == 0 && m) { // one output batch per input batch, rows in input order
              const int64_t *ov = (const int64_t *)outs[(size_t)i]->columns[0].values;
              const int64_t *iv = v.data() + (b0 + i) * B;
              int64_t j = 0;
              for (int64_t r = 0; r < batches[(size_t)(b0 + i)].num_rows && j < m; r++)
                if (iv[r] > k) order_ok = order_ok && ov[j++] == iv[r];
              order_ok = order_ok && j == m;
            }
            got += m;
            sqlrs_batch_release(outs[(size_t)i]);
          }
        }
      }
      sqlrs_filter_destroy(f);
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      kept[mode] = got;
      if (rep > 0 && ms < best[mode]) best[mode] = ms;
    }
  }
  const bool ok = kept[0] == expect && kept[1] == expect && kept[2] == expect && order_ok;
  std::printf("{\"rows\": %lld, \"batches\": %lld, \"batch_rows\": %lld, \"kept\": %lld, \"ms_push\": %.1f, \"Mrows_s_push\": %.1f, "
              "\"group\": %d, \"ms_push_many\": %.1f, \"Mrows_s_push_many\": %.1f, \"depth\": %d, \"ms_push_async\": %.1f, "
              "\"Mrows_s_push_async\": %.1f, \"check\": \"%s\", \"note\": \"native caller (C ABI): "
              "pageable %lld-row host batches, one result batch per input batch on the host; push = sqlrs_filter_push per batch, "
              "push_many = sqlrs_filter_push_many over groups of batches, push_async = sqlrs_filter_push_async per batch with `depth` "
              "tickets in flight + sqlrs_batch_wait; best of 2 after a warm-up\"}\n",
              (long long)n, (long long)nb, (long long)B, (long long)kept[1], best[0], (double)n / best[0] / 1e3, group, best[1],
              (double)n / best[1] / 1e3, DEPTH, best[2], (double)n / best[2] / 1e3, ok ? "OK" : "mismatch", (long long)B);
  sqlrs_ctx_destroy(ctx);
  return ok ? 0 : 1;
}

// ./bench_host_batches probe [rows = 2e7] [build = 1e6] [batch = 1024]
// HashJoinExecutor (C3's join: fact x dim on an int64 key, Inner, every probe row matches) with the PROBE side fed as pageable
// 1024-row host batches, joined batches (dim key, dim payload, fact key, fact val) on the host: sqlrs_hash_join_probe_push per batch.
static int bench_probe(int argc, char **argv) {
  const int64_t n = argc > 2 ? (int64_t)std::atof(argv[2]) : 20000000, nB = argc > 3 ? (int64_t)std::atof(argv[3]) : 1000000;
  const int64_t B = argc > 4 ? std::atoll(argv[4]) : 1024;
  sqlrs_ctx_t *ctx = nullptr;
  if (sqlrs_ctx_create(0, &ctx) != SQLRS_OK) {
    std::printf("{\"error\": \"no device\"}\n");
    return 2;
  }
  std::vector<int64_t> dk((size_t)nB), dp((size_t)nB), fk((size_t)n);
  std::vector<double> fv((size_t)n);
  for (int64_t i = 0; i < nB; i++) {
    dk[(size_t)i] = (i * 7919) % nB; // a permutation when gcd(7919, nB) = 1
    dp[(size_t)i] = dk[(size_t)i] * 3 + 1;
  }
  for (int64_t i = 0; i < n; i++) {
    fk[(size_t)i] = (int64_t)(splitmix64(0xF1, (uint64_t)i) % (uint64_t)nB);
    fv[(size_t)i] = (double)(splitmix64(0xF2, (uint64_t)i) >> 11) * (1.0 / 9007199254740992.0);
  }
  sqlrs_expr_node_t k0{};
  k0.op = SQLRS_EXPR_INPUT_REF;
  k0.index = 0;
  sqlrs_expr_t key{&k0, 1, 0};
  const int32_t right_dtypes[2] = {SQLRS_INT64, SQLRS_FLOAT64};
  double best = 1e30, best_many = 1e30;
  int64_t joined = 0, joined_many = 0;
  bool ok = true;
  { // the same probe batches through sqlrs_hash_join_probe_push_many, 1024 batches per call
    const int64_t nb = (n + B - 1) / B;
    const int group = 1024;
    std::vector<sqlrs_column_t> cols((size_t)nb * 2);
    std::vector<sqlrs_batch_t> batches((size_t)nb);
    std::vector<const sqlrs_batch_t *> ptrs((size_t)nb);
    for (int64_t b = 0; b < nb; b++) {
      const int64_t m = std::min<int64_t>(B, n - b * B);
      host_col(cols[(size_t)b * 2], SQLRS_INT64, fk.data() + b * B, m);
      host_col(cols[(size_t)b * 2 + 1], SQLRS_FLOAT64, fv.data() + b * B, m);
      std::memset(&batches[(size_t)b], 0, sizeof(sqlrs_batch_t));
      batches[(size_t)b].num_rows = m;
      batches[(size_t)b].num_columns = 2;
      batches[(size_t)b].columns = &cols[(size_t)b * 2];
      ptrs[(size_t)b] = &batches[(size_t)b];
    }
    for (int rep = 0; rep < 3; rep++) {
      auto t0 = std::chrono::steady_clock::now();
      sqlrs_hash_join_t *j = nullptr;
      CHECK(sqlrs_hash_join_create(ctx, SQLRS_JOIN_INNER, 1, &key, &key, nullptr, 2, right_dtypes, &j));
      sqlrs_column_t lc[2];
      host_col(lc[0], SQLRS_INT64, dk.data(), nB);
      host_col(lc[1], SQLRS_INT64, dp.data(), nB);
      sqlrs_batch_t lb{};
      lb.num_rows = nB;
      lb.num_columns = 2;
      lb.columns = lc;
      CHECK(sqlrs_hash_join_build_push(j, &lb));
      CHECK(sqlrs_hash_join_build_finish(j));
      joined_many = 0;
      std::vector<sqlrs_batch_t *> outs((size_t)group);
      for (int64_t b0 = 0; b0 < nb; b0 += group) {
        const int g = (int)std::min<int64_t>(group, nb - b0);
        CHECK(sqlrs_hash_join_probe_push_many(j, g, ptrs.data() + b0, SQLRS_MEM_HOST, outs.data()));
        for (int i = 0; i < g; i++) {
          sqlrs_batch_t *o = outs[(size_t)i];
          if (!o) continue;
          if (rep == 0 && o->num_rows == batches[(size_t)(b0 + i)].num_rows) {
            const int64_t *k = (const int64_t *)o->columns[0].values, *p = (const int64_t *)o->columns[1].values;
            const int64_t *rk = (const int64_t *)o->columns[2].values;
            for (int64_t r = 0; r < o->num_rows; r += 97)
              ok = ok && k[r] == fk[(size_t)((b0 + i) * B + r)] && p[r] == 3 * k[r] + 1 && rk[r] == k[r];
          } else if (rep == 0) {
            ok = false;
          }
          joined_many += o->num_rows;
          sqlrs_batch_release(o);
        }
      }
      sqlrs_hash_join_destroy(j);
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (rep > 0 && ms < best_many) best_many = ms;
    }
    ok = ok && joined_many == n;
  }
  for (int rep = 0; rep < 3; rep++) {
    auto t0 = std::chrono::steady_clock::now();
    sqlrs_hash_join_t *j = nullptr;
    CHECK(sqlrs_hash_join_create(ctx, SQLRS_JOIN_INNER, 1, &key, &key, nullptr, 2, right_dtypes, &j));
    sqlrs_column_t lc[2];
    host_col(lc[0], SQLRS_INT64, dk.data(), nB);
    host_col(lc[1], SQLRS_INT64, dp.data(), nB);
    sqlrs_batch_t lb{};
    lb.num_rows = nB;
    lb.num_columns = 2;
    lb.columns = lc;
    CHECK(sqlrs_hash_join_build_push(j, &lb));
    CHECK(sqlrs_hash_join_build_finish(j));
    joined = 0;
    for (int64_t lo = 0; lo < n; lo += B) {
      const int64_t m = std::min<int64_t>(B, n - lo);
      sqlrs_column_t rc[2];
      host_col(rc[0], SQLRS_INT64, fk.data() + lo, m);
      host_col(rc[1], SQLRS_FLOAT64, fv.data() + lo, m);
      sqlrs_batch_t rb{};
      rb.num_rows = m;
      rb.num_columns = 2;
      rb.columns = rc;
      sqlrs_batch_t *o = nullptr;
      CHECK(sqlrs_hash_join_probe_push(j, &rb, SQLRS_MEM_HOST, &o));
      if (o) {
        if (rep == 0 && o->num_rows == m) { // PK-FK: one joined row per probe row, probe order; payload = 3 * key + 1
          const int64_t *k = (const int64_t *)o->columns[0].values, *p = (const int64_t *)o->columns[1].values;
          for (int64_t r = 0; r < m; r += 97) ok = ok && k[r] == fk[(size_t)(lo + r)] && p[r] == 3 * k[r] + 1;
        }
        joined += o->num_rows;
        sqlrs_batch_release(o);
      }
    }
    sqlrs_hash_join_destroy(j);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rep > 0 && ms < best) best = ms;
  }
  ok = ok && joined == n;
  // one probe batch per call without a synchronisation per call: sqlrs_hash_join_probe_push_async + sqlrs_batch_wait
  const int DEPTH = 8;
  double best_async = 1e30;
  int64_t joined_async = 0;
  for (int rep = 0; rep < 3; rep++) {
    auto t0 = std::chrono::steady_clock::now();
    sqlrs_hash_join_t *j = nullptr;
    CHECK(sqlrs_hash_join_create(ctx, SQLRS_JOIN_INNER, 1, &key, &key, nullptr, 2, right_dtypes, &j));
    sqlrs_column_t lc[2];
    host_col(lc[0], SQLRS_INT64, dk.data(), nB);
    host_col(lc[1], SQLRS_INT64, dp.data(), nB);
    sqlrs_batch_t lb{};
    lb.num_rows = nB;
    lb.num_columns = 2;
    lb.columns = lc;
    CHECK(sqlrs_hash_join_build_push(j, &lb));
    CHECK(sqlrs_hash_join_build_finish(j));
    joined_async = 0;
    const int64_t nb = (n + B - 1) / B;
    std::vector<sqlrs_ticket_t *> q((size_t)DEPTH, nullptr);
    auto take = [&](int64_t b) {
      sqlrs_batch_t *o = nullptr;
      CHECK(sqlrs_batch_wait(q[(size_t)(b % DEPTH)], &o));
      if (o) {
        const int64_t m = std::min<int64_t>(B, n - b * B);
        if (rep == 0 && o->num_rows == m) {
          const int64_t *k = (const int64_t *)o->columns[0].values, *p = (const int64_t *)o->columns[1].values;
          const int64_t *rk = (const int64_t *)o->columns[2].values;
          const double *rv = (const double *)o->columns[3].values;
          for (int64_t r = 0; r < m; r += 97)
            ok = ok && k[r] == fk[(size_t)(b * B + r)] && p[r] == 3 * k[r] + 1 && rk[r] == k[r] && rv[r] == fv[(size_t)(b * B + r)];
        } else if (rep == 0)
          ok = false;
        joined_async += o->num_rows;
        sqlrs_batch_release(o);
      }
      return 0;
    };
    for (int64_t b = 0; b < nb; b++) {
      if (b >= DEPTH && take(b - DEPTH)) return 1;
      const int64_t lo = b * B, m = std::min<int64_t>(B, n - lo);
      sqlrs_column_t rc[2];
      host_col(rc[0], SQLRS_INT64, fk.data() + lo, m);
      host_col(rc[1], SQLRS_FLOAT64, fv.data() + lo, m);
      sqlrs_batch_t rb{};
      rb.num_rows = m;
      rb.num_columns = 2;
      rb.columns = rc;
      CHECK(sqlrs_hash_join_probe_push_async(j, &rb, &q[(size_t)(b % DEPTH)]));
    }
    for (int64_t b = std::max<int64_t>(0, nb - DEPTH); b < nb; b++)
      if (take(b)) return 1;
    sqlrs_hash_join_destroy(j);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rep > 0 && ms < best_async) best_async = ms;
  }
  ok = ok && joined_async == n;
  std::printf("{\"depth\": %d, \"ms_push_async\": %.1f, \"Mrows_s_push_async\": %.1f, ", DEPTH, best_async, (double)n / best_async / 1e3);
  std::printf("\"probe_rows\": %lld, \"build_rows\": %lld, \"batch_rows\": %lld, \"joined\": %lld, \"ms_push\": %.1f, \"Mrows_s_push\": %.1f, "
              "\"group\": 1024, \"ms_push_many\": %.1f, \"Mrows_s_push_many\": %.1f, "
              "\"check\": \"%s\", \"note\": \"native caller (C ABI): build side one host batch, probe side pageable %lld-row host batches, "
              "joined batches (4 columns) on the host, one per probe batch; push = sqlrs_hash_join_probe_push per batch, push_many = "
              "sqlrs_hash_join_probe_push_many over groups of batches; build included; best of 2 after a warm-up\"}\n",
              (long long)n, (long long)nB, (long long)B, (long long)joined, best, (double)n / best / 1e3, best_many, (double)n / best_many / 1e3,
              ok ? "OK" : "mismatch", (long long)B);
  sqlrs_ctx_destroy(ctx);
  return ok ? 0 : 1;
}

// ./bench_host_batches project [rows = 2e7] [batch = 1024]
// ProjectExecutor `SELECT v, v * 3 + 1, v > 2^30` over pageable 1024-row host batches (one bare column, two computed ones):
// sqlrs_project_push per batch against sqlrs_project_push_async with DEPTH tickets in flight.
static int bench_project(int argc, char **argv) {
  const int64_t n = argc > 2 ? (int64_t)std::atof(argv[2]) : 20000000, B = argc > 3 ? std::atoll(argv[3]) : 1024;
  sqlrs_ctx_t *ctx = nullptr;
  if (sqlrs_ctx_create(0, &ctx) != SQLRS_OK) {
    std::printf("{\"error\": \"no device\"}\n");
    return 2;
  }
  std::vector<int64_t> v((size_t)n);
  for (int64_t i = 0; i < n; i++) v[(size_t)i] = (int64_t)(splitmix64(0xC2, (uint64_t)i) % (1ull << 31));
  const int64_t k = (1ll << 30);
  sqlrs_expr_node_t e0[1] = {}, e1[5] = {}, e2[3] = {};
  e0[0].op = SQLRS_EXPR_INPUT_REF;
  e1[0].op = SQLRS_EXPR_INPUT_REF;
  e1[1].op = SQLRS_EXPR_CONSTANT; e1[1].dtype = SQLRS_INT64; e1[1].i = 3;
  e1[2].op = SQLRS_EXPR_MULTIPLY;
  e1[3].op = SQLRS_EXPR_CONSTANT; e1[3].dtype = SQLRS_INT64; e1[3].i = 1;
  e1[4].op = SQLRS_EXPR_PLUS;
  e2[0].op = SQLRS_EXPR_INPUT_REF;
  e2[1].op = SQLRS_EXPR_CONSTANT; e2[1].dtype = SQLRS_INT64; e2[1].i = k;
  e2[2].op = SQLRS_EXPR_GT;
  sqlrs_expr_t exprs[3] = {{e0, 1, 0}, {e1, 5, 0}, {e2, 3, 0}};
  const int64_t nb = (n + B - 1) / B;
  std::vector<sqlrs_column_t> cols((size_t)nb);
  std::vector<sqlrs_batch_t> batches((size_t)nb);
  for (int64_t b = 0; b < nb; b++) {
    const int64_t m = std::min<int64_t>(B, n - b * B);
    host_col(cols[(size_t)b], SQLRS_INT64, v.data() + b * B, m);
    std::memset(&batches[(size_t)b], 0, sizeof(sqlrs_batch_t));
    batches[(size_t)b].num_rows = m;
    batches[(size_t)b].num_columns = 1;
    batches[(size_t)b].columns = &cols[(size_t)b];
  }
  const int DEPTH = 8;
  double best[2] = {1e30, 1e30};
  bool ok = true;
  int64_t rows_out[2] = {0, 0};
  for (int mode = 0; mode < 2; mode++)
    for (int rep = 0; rep < 3; rep++) {
      auto t0 = std::chrono::steady_clock::now();
      sqlrs_project_t *pj = nullptr;
      CHECK(sqlrs_project_create(ctx, 3, exprs, &pj));
      int64_t got = 0;
      auto consume = [&](sqlrs_batch_t *o, int64_t b) {
        const int64_t m = o->num_rows;
        if (rep == 0) { // every row of every column
          const int64_t *iv = v.data() + b * B, *c0 = (const int64_t *)o->columns[0].values, *c1 = (const int64_t *)o->columns[1].values;
          const uint8_t *c2 = (const uint8_t *)o->columns[2].values;
          ok = ok && m == batches[(size_t)b].num_rows && o->num_columns == 3;
          for (int64_t r = 0; ok && r < m; r++)
            ok = c0[r] == iv[r] && c1[r] == iv[r] * 3 + 1 && (((c2[r >> 3] >> (r & 7)) & 1) != 0) == (iv[r] > k);
        }
        got += m;
        sqlrs_batch_release(o);
      };
      if (mode == 0) {
        for (int64_t b = 0; b < nb; b++) {
          sqlrs_batch_t *o = nullptr;
          CHECK(sqlrs_project_push(pj, &batches[(size_t)b], SQLRS_MEM_HOST, &o));
          consume(o, b);
        }
      } else {
        std::vector<sqlrs_ticket_t *> q((size_t)DEPTH, nullptr);
        for (int64_t b = 0; b < nb + DEPTH; b++) {
          if (b >= DEPTH) {
            sqlrs_batch_t *o = nullptr;
            CHECK(sqlrs_batch_wait(q[(size_t)(b % DEPTH)], &o));
            consume(o, b - DEPTH);
          }
          if (b < nb) CHECK(sqlrs_project_push_async(pj, &batches[(size_t)b], &q[(size_t)(b % DEPTH)]));
        }
      }
      sqlrs_project_destroy(pj);
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      rows_out[mode] = got;
      if (rep > 0 && ms < best[mode]) best[mode] = ms;
    }
  ok = ok && rows_out[0] == n && rows_out[1] == n;
  std::printf("{\"rows\": %lld, \"batches\": %lld, \"batch_rows\": %lld, \"ms_push\": %.1f, \"Mrows_s_push\": %.1f, \"depth\": %d, "
              "\"ms_push_async\": %.1f, \"Mrows_s_push_async\": %.1f, \"check\": \"%s\", \"note\": \"native caller (C ABI): SELECT v, v * 3 + 1, "
              "v > 2^30 over pageable %lld-row host batches, one result batch per input batch on the host; best of 2 after a warm-up\"}\n",
              (long long)n, (long long)nb, (long long)B, best[0], (double)n / best[0] / 1e3, DEPTH, best[1], (double)n / best[1] / 1e3,
              ok ? "OK" : "mismatch", (long long)B);
  sqlrs_ctx_destroy(ctx);
  return ok ? 0 : 1;
}

// ./bench_host_batches probe_general [rows = 2e7] [build = 1e6] [batch = 1024] [join = left|right|full|inner] [dup = 1|4]
// The probe stream of bench_probe against a build side whose every key is carried by `dup` rows (build / dup distinct keys;
// a fifth of the probe keys has no partner), joined as `join`, through three paths: sqlrs_hash_join_probe_push per batch,
// sqlrs_hash_join_probe_push_async with sqlrs_hash_join_set_async_general off (the synchronous operator inside push_async) and
// on (one launch per batch), DEPTH tickets in flight.  The off and on runs alternate; best of 2 after a warm-up each; the
// joined rows (tail batch of Left / Full included) of the three paths must agree.
//
// ./bench_host_batches probe_utf8 [the same arguments]
// The same with one Utf8 column of 8-16 byte strings on each side (build: chosen by the key; probe: by the probe key, each
// batch's offsets a window into one array, so offsets[0] != 0).  sqlrs_hash_join_set_async_general is on in both push_async
// paths; what alternates is sqlrs_hash_join_set_async_utf8: off = the synchronous operator inside push_async (today's
// behaviour with a Utf8 column around the join), on = one launch per batch.
static int bench_probe_general(int argc, char **argv, bool utf8) {
  const int64_t n = argc > 2 ? (int64_t)std::atof(argv[2]) : 20000000, nB = argc > 3 ? (int64_t)std::atof(argv[3]) : 1000000;
  const int64_t B = argc > 4 ? std::atoll(argv[4]) : 1024;
  const char *jname = argc > 5 ? argv[5] : "left";
  const int64_t dup = argc > 6 ? std::max<int64_t>(1, std::atoll(argv[6])) : 1;
  const int jt = std::strcmp(jname, "inner") == 0 ? SQLRS_JOIN_INNER : std::strcmp(jname, "right") == 0 ? SQLRS_JOIN_RIGHT
                 : std::strcmp(jname, "full") == 0 ? SQLRS_JOIN_FULL : SQLRS_JOIN_LEFT;
  sqlrs_ctx_t *ctx = nullptr;
  if (sqlrs_ctx_create(0, &ctx) != SQLRS_OK) {
    std::printf("{\"error\": \"no device\"}\n");
    return 2;
  }
  const int64_t nkeys = std::max<int64_t>(1, nB / dup);
  std::vector<int64_t> dk((size_t)nB), dp((size_t)nB), fk((size_t)n);
  std::vector<double> fv((size_t)n);
  for (int64_t i = 0; i < nB; i++) {
    dk[(size_t)i] = ((i * 7919) % nB) % nkeys;
    dp[(size_t)i] = dk[(size_t)i] * 3 + 1;
  }
  for (int64_t i = 0; i < n; i++) {
    fk[(size_t)i] = (int64_t)(splitmix64(0xF1, (uint64_t)i) % (uint64_t)(nkeys + nkeys / 4));
    fv[(size_t)i] = (double)(splitmix64(0xF2, (uint64_t)i) >> 11) * (1.0 / 9007199254740992.0);
  }
  // Utf8: key k carries 8 + k % 9 bytes of the letter 'a' + k % 26 (build) / 'A' + k % 26 (probe)
  std::vector<int32_t> doff, foff;
  std::vector<char> dbytes, fbytes;
  auto strings = [](const std::vector<int64_t> &keys, char first, std::vector<int32_t> &off, std::vector<char> &bytes) {
    off.resize(keys.size() + 1);
    off[0] = 0;
    for (size_t i = 0; i < keys.size(); i++) off[i + 1] = off[i] + 8 + (int32_t)(keys[i] % 9);
    bytes.resize((size_t)off[keys.size()] + 1);
    for (size_t i = 0; i < keys.size(); i++) std::memset(bytes.data() + off[i], first + (int)(keys[i] % 26), (size_t)(off[i + 1] - off[i]));
  };
  if (utf8) {
    if (n * 16 > 2000000000ll) {
      std::printf("{\"error\": \"probe_utf8: at most 1.25e8 probe rows\"}\n");
      return 2;
    }
    strings(dk, 'a', doff, dbytes);
    strings(fk, 'A', foff, fbytes);
  }
  const int ncl = utf8 ? 3 : 2; // columns per side
  sqlrs_expr_node_t k0{};
  k0.op = SQLRS_EXPR_INPUT_REF;
  k0.index = 0;
  sqlrs_expr_t key{&k0, 1, 0};
  const int32_t right_dtypes[3] = {SQLRS_INT64, SQLRS_FLOAT64, SQLRS_UTF8};
  const int DEPTH = 8;
  const int64_t nb = (n + B - 1) / B;
  double best[3] = {1e30, 1e30, 1e30}; // push, push_async switch off, push_async switch on
  int64_t joined[3] = {0, 0, 0};
  bool ok = true;
  auto run = [&](int path, int rep) -> int { // 0 ok
    auto t0 = std::chrono::steady_clock::now();
    sqlrs_hash_join_t *j = nullptr;
    CHECK(sqlrs_hash_join_create(ctx, jt, 1, &key, &key, nullptr, ncl, right_dtypes, &j));
    if (path == 2 || (utf8 && path == 1)) CHECK(sqlrs_hash_join_set_async_general(j, 1));
    if (utf8 && path == 2) CHECK(sqlrs_hash_join_set_async_utf8(j, 1));
    sqlrs_column_t lc[3];
    host_col(lc[0], SQLRS_INT64, dk.data(), nB);
    host_col(lc[1], SQLRS_INT64, dp.data(), nB);
    if (utf8) {
      host_col(lc[2], SQLRS_UTF8, dbytes.data(), nB);
      lc[2].offsets = doff.data();
    }
    sqlrs_batch_t lb{};
    lb.num_rows = nB;
    lb.num_columns = ncl;
    lb.columns = lc;
    CHECK(sqlrs_hash_join_build_push(j, &lb));
    CHECK(sqlrs_hash_join_build_finish(j));
    int64_t got = 0;
    auto consume = [&](sqlrs_batch_t *o) { // a matched row carries payload 3 * key + 1 beside the probe row's key
      if (!o) return;
      if (rep == 0 && o->num_rows) {
        const int64_t *p = (const int64_t *)o->columns[1].values, *rk = (const int64_t *)o->columns[ncl].values;
        const uint8_t *pv = (const uint8_t *)o->columns[1].validity;
        for (int64_t r = 0; r < o->num_rows; r += 97) {
          const bool matched = rk[r] < nkeys;
          const bool valid = !pv || !o->columns[1].null_count || ((pv[r >> 3] >> (r & 7)) & 1);
          ok = ok && matched == valid && (!matched || p[r] == 3 * rk[r] + 1);
          for (int side = 0; utf8 && side < 2; side++) { // the strings: length and letter by the key, first and last byte
            const sqlrs_column_t &sc = o->columns[side ? 2 * ncl - 1 : 2];
            const int32_t *so = (const int32_t *)sc.offsets;
            const char *sb = (const char *)sc.values;
            const uint8_t *sv = (const uint8_t *)sc.validity;
            const bool svalid = !sv || !sc.null_count || ((sv[r >> 3] >> (r & 7)) & 1);
            const int32_t len = so[r + 1] - so[r], want = (side || matched) ? 8 + (int32_t)(rk[r] % 9) : 0;
            const char letter = (char)((side ? 'A' : 'a') + (int)(rk[r] % 26));
            ok = ok && svalid == (side || matched) && len == want && (!want || (sb[so[r]] == letter && sb[so[r + 1] - 1] == letter));
          }
        }
      }
      got += o->num_rows;
      sqlrs_batch_release(o);
    };
    std::vector<sqlrs_ticket_t *> q((size_t)DEPTH, nullptr);
    for (int64_t b = 0; b < nb + (path ? DEPTH : 0); b++) {
      if (path && b >= DEPTH) {
        sqlrs_batch_t *o = nullptr;
        CHECK(sqlrs_batch_wait(q[(size_t)(b % DEPTH)], &o));
        consume(o);
      }
      if (b >= nb) continue;
      const int64_t lo = b * B, m = std::min<int64_t>(B, n - lo);
      sqlrs_column_t rc[3];
      host_col(rc[0], SQLRS_INT64, fk.data() + lo, m);
      host_col(rc[1], SQLRS_FLOAT64, fv.data() + lo, m);
      if (utf8) {
        host_col(rc[2], SQLRS_UTF8, fbytes.data(), m);
        rc[2].offsets = foff.data() + lo;
      }
      sqlrs_batch_t rb{};
      rb.num_rows = m;
      rb.num_columns = ncl;
      rb.columns = rc;
      if (path) {
        CHECK(sqlrs_hash_join_probe_push_async(j, &rb, &q[(size_t)(b % DEPTH)]));
      } else {
        sqlrs_batch_t *o = nullptr;
        CHECK(sqlrs_hash_join_probe_push(j, &rb, SQLRS_MEM_HOST, &o));
        consume(o);
      }
    }
    sqlrs_batch_t *tail = nullptr;
    CHECK(sqlrs_hash_join_finish(j, SQLRS_MEM_HOST, &tail));
    if (tail) {
      got += tail->num_rows;
      sqlrs_batch_release(tail);
    }
    sqlrs_hash_join_destroy(j);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    joined[path] = got;
    if (rep > 0 && ms < best[path]) best[path] = ms;
    return 0;
  };
  for (int rep = 0; rep < 3; rep++)
    if (run(0, rep)) return 1;
  for (int rep = 0; rep < 3; rep++) // off and on alternate
    for (int path = 1; path <= 2; path++)
      if (run(path, rep)) return 1;
  ok = ok && joined[0] == joined[1] && joined[1] == joined[2] && joined[0] > 0;
  std::printf("{\"mode\": \"%s\", \"join\": \"%s\", \"dup\": %lld, \"probe_rows\": %lld, \"build_rows\": %lld, \"batch_rows\": %lld, "
              "\"joined\": %lld, \"depth\": %d, \"ms_push\": %.1f, \"Mrows_s_push\": %.1f, \"ms_push_async_off\": %.1f, \"Mrows_s_push_async_off\": %.1f, "
              "\"ms_push_async_on\": %.1f, \"Mrows_s_push_async_on\": %.1f, \"on_over_off\": %.2f, \"check\": \"%s\", \"note\": \"native caller "
              "(C ABI): build side one host batch (every key %lld times), probe side pageable %lld-row host batches (a fifth of the keys "
              "without partner), joined batches on the host; push = sqlrs_hash_join_probe_push per batch, push_async_off / _on = "
              "sqlrs_hash_join_probe_push_async with %s 0 / 1 (alternating runs); Mrows/s = probe rows; "
              "build included; best of 2 after a warm-up\"}\n",
              utf8 ? "probe_utf8" : "probe_general", jname, (long long)dup, (long long)n, (long long)nB, (long long)B, (long long)joined[0], DEPTH, best[0], (double)n / best[0] / 1e3,
              best[1], (double)n / best[1] / 1e3, best[2], (double)n / best[2] / 1e3, best[1] / best[2], ok ? "OK" : "mismatch", (long long)dup,
              (long long)B,
              utf8 ? "one Utf8 column of 8-16 byte strings per side, sqlrs_hash_join_set_async_general 1 and sqlrs_hash_join_set_async_utf8"
                   : "sqlrs_hash_join_set_async_general");
  sqlrs_ctx_destroy(ctx);
  return ok ? 0 : 1;
}


// ./bench_host_batches probe_keys [rows = 2e6] [build = 1e6] [batch = 1024] [leg = utf8|pair|nulls|all]
// sqlrs_hash_join_set_async_keys: three legs over keys the one-launch probe kernels load themselves, each through three paths —
// sqlrs_hash_join_probe_push per batch, sqlrs_hash_join_probe_push_async with the switch off (the synchronous operator inside
// push_async: what such a batch cost before) and on (one launch per batch) — DEPTH tickets in flight, off and on alternating in one
// process, best of 2 after a warm-up each; the joined rows of the three paths must agree.
//   utf8:  Inner join over unique Utf8 keys of 8-16 bytes (8 hex digits of the key, then 0-8 letters); build (s, p), probe (t, k)
//   pair:  Left join over a two-column (int64, int64) key (k, 7 k + 3); build (a, b, p), probe (a, b, v)
//   nulls: Inner join over an int64 key, 5 % of the probe keys NULL (the build side has no NULL key); build (k, p), probe (k, v)
// A fifth of the probe keys has no partner.  sqlrs_hash_join_set_async_general and _utf8 are on in both push_async paths.  The
// setter is looked up at run time, so the tool also links against a library that does not have it yet (the other modes).
static int bench_probe_keys(int argc, char **argv) {
  const int64_t n = argc > 2 ? (int64_t)std::atof(argv[2]) : 2000000, nB = argc > 3 ? (int64_t)std::atof(argv[3]) : 1000000;
  const int64_t B = argc > 4 ? std::atoll(argv[4]) : 1024;
  const char *which = argc > 5 ? argv[5] : "all";
  sqlrs_ctx_t *ctx = nullptr;
  typedef int (*setter_t)(sqlrs_hash_join_t *, int);
  const setter_t set_keys = (setter_t)dlsym(RTLD_DEFAULT, "sqlrs_hash_join_set_async_keys");
  if (!set_keys || B % 8 != 0 || n * 16 > 2000000000ll) {
    std::printf("{\"error\": \"probe_keys: needs sqlrs_hash_join_set_async_keys, a batch size that is a multiple of 8 and at most 1.25e8 probe rows\"}\n");
    return 2;
  }
  if (sqlrs_ctx_create(0, &ctx) != SQLRS_OK) {
    std::printf("{\"error\": \"no device\"}\n");
    return 2;
  }
  std::vector<int64_t> dk((size_t)nB), dk2((size_t)nB), dp((size_t)nB), fk((size_t)n), fk2((size_t)n);
  std::vector<double> fv((size_t)n);
  std::vector<uint8_t> fvalid((size_t)(n + 7) / 8 + 8, 0);
  std::vector<int64_t> fnulls((size_t)((n + B - 1) / B), 0);
  for (int64_t i = 0; i < nB; i++) {
    dk[(size_t)i] = (i * 7919) % nB;
    dk2[(size_t)i] = dk[(size_t)i] * 7 + 3;
    dp[(size_t)i] = dk[(size_t)i] * 3 + 1;
  }
  for (int64_t i = 0; i < n; i++) {
    fk[(size_t)i] = (int64_t)(splitmix64(0xF1, (uint64_t)i) % (uint64_t)(nB + nB / 4));
    fk2[(size_t)i] = fk[(size_t)i] * 7 + 3;
    fv[(size_t)i] = (double)(splitmix64(0xF2, (uint64_t)i) >> 11) * (1.0 / 9007199254740992.0);
    const bool null = splitmix64(0xF3, (uint64_t)i) % 20 == 0;
    if (!null) fvalid[(size_t)(i >> 3)] |= (uint8_t)(1u << (i & 7));
    else fnulls[(size_t)(i / B)]++;
  }
  std::vector<int32_t> doff, foff;
  std::vector<char> dbytes, fbytes;
  auto strings = [](const std::vector<int64_t> &keys, std::vector<int32_t> &off, std::vector<char> &bytes) {
    off.resize(keys.size() + 1);
    off[0] = 0;
    for (size_t i = 0; i < keys.size(); i++) off[i + 1] = off[i] + 8 + (int32_t)(keys[i] % 9);
    bytes.resize((size_t)off[keys.size()] + 16);
    for (size_t i = 0; i < keys.size(); i++) {
      char hex[17];
      std::snprintf(hex, sizeof(hex), "%08llx", (unsigned long long)keys[i]);
      std::memset(bytes.data() + off[i], 'a' + (int)(keys[i] % 26), (size_t)(off[i + 1] - off[i]));
      std::memcpy(bytes.data() + off[i], hex, 8);
    }
  };
  strings(dk, doff, dbytes);
  strings(fk, foff, fbytes);
  sqlrs_expr_node_t k0{}, k1{};
  k0.op = k1.op = SQLRS_EXPR_INPUT_REF;
  k0.index = 0;
  k1.index = 1;
  sqlrs_expr_t keys2[2] = {{&k0, 1, 0}, {&k1, 1, 0}};
  const int DEPTH = 8;
  const int64_t nb = (n + B - 1) / B;
  int rc_all = 0;
  for (int leg = 0; leg < 3; leg++) {
    const char *lname = leg == 0 ? "utf8" : leg == 1 ? "pair" : "nulls";
    if (std::strcmp(which, "all") != 0 && std::strcmp(which, lname) != 0) continue;
    const int jt = leg == 1 ? SQLRS_JOIN_LEFT : SQLRS_JOIN_INNER;
    const int nkey = leg == 1 ? 2 : 1, nlc = leg == 1 ? 3 : 2, nrc = leg == 1 ? 3 : 2;
    const int32_t rd_utf8[2] = {SQLRS_UTF8, SQLRS_INT64}, rd_pair[3] = {SQLRS_INT64, SQLRS_INT64, SQLRS_FLOAT64}, rd_nulls[2] = {SQLRS_INT64, SQLRS_FLOAT64};
    const int32_t *rd = leg == 0 ? rd_utf8 : leg == 1 ? rd_pair : rd_nulls;
    double best[3] = {1e30, 1e30, 1e30}; // push, push_async switch off, push_async switch on
    int64_t joined[3] = {0, 0, 0};
    bool ok = true;
    auto run = [&](int path, int rep) -> int { // 0 ok
      auto t0 = std::chrono::steady_clock::now();
      sqlrs_hash_join_t *j = nullptr;
      CHECK(sqlrs_hash_join_create(ctx, jt, nkey, keys2, keys2, nullptr, nrc, rd, &j));
      if (path) {
        CHECK(sqlrs_hash_join_set_async_general(j, 1));
        CHECK(sqlrs_hash_join_set_async_utf8(j, 1));
      }
      if (path == 2) CHECK(set_keys(j, 1));
      sqlrs_column_t lc[3];
      if (leg == 0) {
        host_col(lc[0], SQLRS_UTF8, dbytes.data(), nB);
        lc[0].offsets = doff.data();
        host_col(lc[1], SQLRS_INT64, dp.data(), nB);
      } else {
        host_col(lc[0], SQLRS_INT64, dk.data(), nB);
        if (leg == 1) host_col(lc[1], SQLRS_INT64, dk2.data(), nB);
        host_col(lc[nlc - 1], SQLRS_INT64, dp.data(), nB);
      }
      sqlrs_batch_t lb{};
      lb.num_rows = nB;
      lb.num_columns = nlc;
      lb.columns = lc;
      CHECK(sqlrs_hash_join_build_push(j, &lb));
      CHECK(sqlrs_hash_join_build_finish(j));
      int64_t got = 0;
      auto consume = [&](sqlrs_batch_t *o) { // a matched row carries payload 3 * key + 1 beside the probe row's key
        if (!o) return;
        if (rep == 0 && o->num_rows) {
          const int pc = nlc - 1, kc = leg == 0 ? nlc + 1 : nlc; // payload; the probe row's int64 key
          const int64_t *p = (const int64_t *)o->columns[pc].values, *rk = (const int64_t *)o->columns[kc].values;
          const uint8_t *pv = (const uint8_t *)o->columns[pc].validity, *kv = (const uint8_t *)o->columns[kc].validity;
          for (int64_t r = 0; r < o->num_rows; r += 97) {
            const bool knull = kv && o->columns[kc].null_count && !((kv[r >> 3] >> (r & 7)) & 1);
            const bool matched = !knull && rk[r] < nB;
            const bool valid = !pv || !o->columns[pc].null_count || ((pv[r >> 3] >> (r & 7)) & 1);
            ok = ok && matched == valid && (!matched || p[r] == 3 * rk[r] + 1) && (jt == SQLRS_JOIN_LEFT || matched);
          }
        }
        got += o->num_rows;
        sqlrs_batch_release(o);
      };
      std::vector<sqlrs_ticket_t *> q((size_t)DEPTH, nullptr);
      for (int64_t b = 0; b < nb + (path ? DEPTH : 0); b++) {
        if (path && b >= DEPTH) {
          sqlrs_batch_t *o = nullptr;
          CHECK(sqlrs_batch_wait(q[(size_t)(b % DEPTH)], &o));
          consume(o);
        }
        if (b >= nb) continue;
        const int64_t lo = b * B, m = std::min<int64_t>(B, n - lo);
        sqlrs_column_t rc[3];
        if (leg == 0) {
          host_col(rc[0], SQLRS_UTF8, fbytes.data(), m);
          rc[0].offsets = foff.data() + lo;
          host_col(rc[1], SQLRS_INT64, fk.data() + lo, m);
        } else {
          host_col(rc[0], SQLRS_INT64, fk.data() + lo, m);
          if (leg == 1) host_col(rc[1], SQLRS_INT64, fk2.data() + lo, m);
          host_col(rc[nrc - 1], SQLRS_FLOAT64, fv.data() + lo, m);
          if (leg == 2) {
            rc[0].validity = fvalid.data() + lo / 8;
            rc[0].null_count = fnulls[(size_t)b];
          }
        }
        sqlrs_batch_t rb{};
        rb.num_rows = m;
        rb.num_columns = nrc;
        rb.columns = rc;
        if (path) {
          CHECK(sqlrs_hash_join_probe_push_async(j, &rb, &q[(size_t)(b % DEPTH)]));
        } else {
          sqlrs_batch_t *o = nullptr;
          CHECK(sqlrs_hash_join_probe_push(j, &rb, SQLRS_MEM_HOST, &o));
          consume(o);
        }
      }
      sqlrs_batch_t *tail = nullptr;
      CHECK(sqlrs_hash_join_finish(j, SQLRS_MEM_HOST, &tail));
      if (tail) {
        got += tail->num_rows;
        sqlrs_batch_release(tail);
      }
      sqlrs_hash_join_destroy(j);
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      joined[path] = got;
      if (rep > 0 && ms < best[path]) best[path] = ms;
      return 0;
    };
    for (int rep = 0; rep < 3; rep++)
      if (run(0, rep)) return 1;
    for (int rep = 0; rep < 3; rep++) // off and on alternate
      for (int path = 1; path <= 2; path++)
        if (run(path, rep)) return 1;
    ok = ok && joined[0] == joined[1] && joined[1] == joined[2] && joined[0] > 0;
    std::printf("{\"mode\": \"probe_keys\", \"leg\": \"%s\", \"join\": \"%s\", \"probe_rows\": %lld, \"build_rows\": %lld, \"batch_rows\": %lld, "
                "\"joined\": %lld, \"depth\": %d, \"ms_push\": %.1f, \"Mrows_s_push\": %.1f, \"ms_push_async_off\": %.1f, \"Mrows_s_push_async_off\": %.1f, "
                "\"ms_push_async_on\": %.1f, \"Mrows_s_push_async_on\": %.1f, \"on_over_off\": %.2f, \"check\": \"%s\", \"note\": \"native caller "
                "(C ABI): build side one host batch of unique keys, probe side pageable %lld-row host batches (a fifth of the keys without partner%s), "
                "joined batches on the host; push = sqlrs_hash_join_probe_push per batch, push_async_off / _on = sqlrs_hash_join_probe_push_async with "
                "sqlrs_hash_join_set_async_keys 0 / 1 (alternating runs; _general and _utf8 on in both); Mrows/s = probe rows; build included; best of 2 "
                "after a warm-up\"}\n",
                lname, jt == SQLRS_JOIN_LEFT ? "left" : "inner", (long long)n, (long long)nB, (long long)B, (long long)joined[0], DEPTH, best[0],
                (double)n / best[0] / 1e3, best[1], (double)n / best[1] / 1e3, best[2], (double)n / best[2] / 1e3, best[1] / best[2], ok ? "OK" : "mismatch",
                (long long)B, leg == 2 ? ", 5 % of them NULL" : "");
    std::fflush(stdout);
    if (!ok) rc_all = 1;
  }
  sqlrs_ctx_destroy(ctx);
  return rc_all;
}

// ./bench_host_batches probe_filter [rows = 2e7] [build = 1e6] [batch = 1024] [join = inner|left|right|full] [dup = 1|4]
// The probe stream of probe_general with a join filter, ON l.k = r.k AND l.x > r.v over two float64 payload columns (uniform in
// [0, 1): about half the pairs pass), through three paths: sqlrs_hash_join_probe_push per batch, and
// sqlrs_hash_join_probe_push_async with sqlrs_hash_join_set_async_filter off (the synchronous operator inside push_async: what
// a filtered join always took) and on (one launch per batch, the filter inside the kernel); sqlrs_hash_join_set_async_general
// is on in both push_async paths.  The off and on runs alternate; best of 2 after a warm-up each.  Its own check: the joined
// rows of every path (tail batch of Left / Full included) must equal the count the host works out from the keys and the two
// payload columns, and on every 97th row of the first run a matched row carries l.k = r.k and l.x > r.v.
// Compiled with -DSQLRS_BENCH_NO_ASYNC_FILTER the one call of the new setter is left out and the on path is not run: the tool
// then builds against a library that has no such entry point.
static int bench_probe_filter(int argc, char **argv) {
  const int64_t n = argc > 2 ? (int64_t)std::atof(argv[2]) : 20000000, nB = argc > 3 ? (int64_t)std::atof(argv[3]) : 1000000;
  const int64_t B = argc > 4 ? std::atoll(argv[4]) : 1024;
  const char *jname = argc > 5 ? argv[5] : "inner";
  const int64_t dup = argc > 6 ? std::max<int64_t>(1, std::atoll(argv[6])) : 1;
  const int jt = std::strcmp(jname, "left") == 0 ? SQLRS_JOIN_LEFT : std::strcmp(jname, "right") == 0 ? SQLRS_JOIN_RIGHT
                 : std::strcmp(jname, "full") == 0 ? SQLRS_JOIN_FULL : SQLRS_JOIN_INNER;
#ifdef SQLRS_BENCH_NO_ASYNC_FILTER
  const int npaths = 2;
#else
  const int npaths = 3;
#endif
  sqlrs_ctx_t *ctx = nullptr;
  if (sqlrs_ctx_create(0, &ctx) != SQLRS_OK) {
    std::printf("{\"error\": \"no device\"}\n");
    return 2;
  }
  const int64_t nkeys = std::max<int64_t>(1, nB / dup);
  std::vector<int64_t> dk((size_t)nB), fk((size_t)n);
  std::vector<double> dx((size_t)nB), fv((size_t)n);
  auto unit = [](uint64_t seed, uint64_t i) { return (double)(splitmix64(seed, i) >> 11) * (1.0 / 9007199254740992.0); };
  for (int64_t i = 0; i < nB; i++) {
    dk[(size_t)i] = ((i * 7919) % nB) % nkeys;
    dx[(size_t)i] = unit(0xD3, (uint64_t)i);
  }
  for (int64_t i = 0; i < n; i++) {
    fk[(size_t)i] = (int64_t)(splitmix64(0xF1, (uint64_t)i) % (uint64_t)(nkeys + nkeys / 4));
    fv[(size_t)i] = unit(0xF2, (uint64_t)i);
  }
  // the count the paths must reach, from the inputs alone: the build rows by key (counting sort), every probe row against its key's rows
  int64_t expect = 0;
  {
    std::vector<int64_t> start((size_t)nkeys + 1, 0), rows((size_t)nB);
    for (int64_t i = 0; i < nB; i++) start[(size_t)dk[(size_t)i] + 1]++;
    for (int64_t k = 0; k < nkeys; k++) start[(size_t)k + 1] += start[(size_t)k];
    std::vector<int64_t> at(start.begin(), start.end() - 1);
    for (int64_t i = 0; i < nB; i++) rows[(size_t)at[(size_t)dk[(size_t)i]]++] = i;
    std::vector<char> kept((size_t)nB, 0);
    const bool outer_right = jt == SQLRS_JOIN_RIGHT || jt == SQLRS_JOIN_FULL, outer_left = jt == SQLRS_JOIN_LEFT || jt == SQLRS_JOIN_FULL;
    for (int64_t i = 0; i < n; i++) {
      int64_t pass = 0;
      if (fk[(size_t)i] < nkeys)
        for (int64_t q = start[(size_t)fk[(size_t)i]]; q < start[(size_t)fk[(size_t)i] + 1]; q++)
          if (dx[(size_t)rows[(size_t)q]] > fv[(size_t)i]) {
            pass++;
            kept[(size_t)rows[(size_t)q]] = 1;
          }
      expect += outer_right ? std::max<int64_t>(pass, 1) : pass;
    }
    if (outer_left)
      for (int64_t i = 0; i < nB; i++) expect += !kept[(size_t)i];
  }
  sqlrs_expr_node_t k0{};
  k0.op = SQLRS_EXPR_INPUT_REF;
  k0.index = 0;
  sqlrs_expr_t key{&k0, 1, 0};
  sqlrs_expr_node_t fn[3] = {}; // joined schema: l.k 0, l.x 1, r.k 2, r.v 3
  fn[0].op = SQLRS_EXPR_INPUT_REF;
  fn[0].index = 1;
  fn[1].op = SQLRS_EXPR_INPUT_REF;
  fn[1].index = 3;
  fn[2].op = SQLRS_EXPR_GT;
  sqlrs_expr_t filter{fn, 3, 0};
  const int32_t right_dtypes[2] = {SQLRS_INT64, SQLRS_FLOAT64};
  const int DEPTH = 8;
  const int64_t nb = (n + B - 1) / B;
  double best[3] = {1e30, 1e30, 1e30}; // push, push_async switch off, push_async switch on
  int64_t joined[3] = {0, 0, 0};
  bool ok = true;
  auto run = [&](int path, int rep) -> int { // 0 ok
    auto t0 = std::chrono::steady_clock::now();
    sqlrs_hash_join_t *j = nullptr;
    CHECK(sqlrs_hash_join_create(ctx, jt, 1, &key, &key, &filter, 2, right_dtypes, &j));
    if (path) CHECK(sqlrs_hash_join_set_async_general(j, 1));
#ifndef SQLRS_BENCH_NO_ASYNC_FILTER
    if (path == 2) CHECK(sqlrs_hash_join_set_async_filter(j, 1));
#endif
    sqlrs_column_t lc[2];
    host_col(lc[0], SQLRS_INT64, dk.data(), nB);
    host_col(lc[1], SQLRS_FLOAT64, dx.data(), nB);
    sqlrs_batch_t lb{};
    lb.num_rows = nB;
    lb.num_columns = 2;
    lb.columns = lc;
    CHECK(sqlrs_hash_join_build_push(j, &lb));
    CHECK(sqlrs_hash_join_build_finish(j));
    int64_t got = 0;
    auto consume = [&](sqlrs_batch_t *o) { // a row with a build side passed the filter on equal keys
      if (!o) return;
      if (rep == 0 && o->num_rows) {
        const int64_t *lk = (const int64_t *)o->columns[0].values, *rk = (const int64_t *)o->columns[2].values;
        const double *lx = (const double *)o->columns[1].values, *rv = (const double *)o->columns[3].values;
        const uint8_t *xv = (const uint8_t *)o->columns[1].validity;
        for (int64_t r = 0; r < o->num_rows; r += 97) {
          const bool matched = !xv || !o->columns[1].null_count || ((xv[r >> 3] >> (r & 7)) & 1);
          ok = ok && (matched ? lk[r] == rk[r] && lx[r] > rv[r] : (jt == SQLRS_JOIN_RIGHT || jt == SQLRS_JOIN_FULL));
        }
      }
      got += o->num_rows;
      sqlrs_batch_release(o);
    };
    std::vector<sqlrs_ticket_t *> q((size_t)DEPTH, nullptr);
    for (int64_t b = 0; b < nb + (path ? DEPTH : 0); b++) {
      if (path && b >= DEPTH) {
        sqlrs_batch_t *o = nullptr;
        CHECK(sqlrs_batch_wait(q[(size_t)(b % DEPTH)], &o));
        consume(o);
      }
      if (b >= nb) continue;
      const int64_t lo = b * B, m = std::min<int64_t>(B, n - lo);
      sqlrs_column_t rc[2];
      host_col(rc[0], SQLRS_INT64, fk.data() + lo, m);
      host_col(rc[1], SQLRS_FLOAT64, fv.data() + lo, m);
      sqlrs_batch_t rb{};
      rb.num_rows = m;
      rb.num_columns = 2;
      rb.columns = rc;
      if (path) {
        CHECK(sqlrs_hash_join_probe_push_async(j, &rb, &q[(size_t)(b % DEPTH)]));
      } else {
        sqlrs_batch_t *o = nullptr;
        CHECK(sqlrs_hash_join_probe_push(j, &rb, SQLRS_MEM_HOST, &o));
        consume(o);
      }
    }
    sqlrs_batch_t *tail = nullptr;
    CHECK(sqlrs_hash_join_finish(j, SQLRS_MEM_HOST, &tail));
    if (tail) {
      got += tail->num_rows;
      sqlrs_batch_release(tail);
    }
    sqlrs_hash_join_destroy(j);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    joined[path] = got;
    if (rep > 0 && ms < best[path]) best[path] = ms;
    return 0;
  };
  for (int rep = 0; rep < 3; rep++)
    if (run(0, rep)) return 1;
  for (int rep = 0; rep < 3; rep++) // off and on alternate
    for (int path = 1; path < npaths; path++)
      if (run(path, rep)) return 1;
  for (int path = 0; path < npaths; path++) ok = ok && joined[path] == expect;
  std::printf("{\"mode\": \"probe_filter\", \"join\": \"%s\", \"dup\": %lld, \"probe_rows\": %lld, \"build_rows\": %lld, \"batch_rows\": %lld, "
              "\"joined\": %lld, \"expected\": %lld, \"depth\": %d, \"ms_push\": %.1f, \"Mrows_s_push\": %.1f, \"ms_push_async_off\": %.1f, "
              "\"Mrows_s_push_async_off\": %.1f, ",
              jname, (long long)dup, (long long)n, (long long)nB, (long long)B, (long long)joined[0], (long long)expect, DEPTH, best[0],
              (double)n / best[0] / 1e3, best[1], (double)n / best[1] / 1e3);
  if (npaths == 3)
    std::printf("\"ms_push_async_on\": %.1f, \"Mrows_s_push_async_on\": %.1f, \"on_over_off\": %.2f, ", best[2], (double)n / best[2] / 1e3, best[1] / best[2]);
  std::printf("\"check\": \"%s\", \"note\": \"native caller (C ABI): build side one host batch (every key %lld times, a float64 payload), probe side "
              "pageable %lld-row host batches (a fifth of the keys without partner, a float64 payload), join filter l.x > r.v (about half the pairs "
              "pass), joined batches on the host; push = sqlrs_hash_join_probe_push per batch, push_async_off / _on = "
              "sqlrs_hash_join_probe_push_async with sqlrs_hash_join_set_async_general 1 and sqlrs_hash_join_set_async_filter 0 / 1 (alternating "
              "runs)%s; Mrows/s = probe rows; build included; best of 2 after a warm-up\"}\n",
              ok ? "OK" : "mismatch", (long long)dup, (long long)B, npaths == 3 ? "" : "; built without the setter: no on path");
  sqlrs_ctx_destroy(ctx);
  return ok ? 0 : 1;
}

// ./bench_host_batches filter_all_types [rows = 2e6] [batch = 1024]
// FilterExecutor over the shape of the reference's CSV tables — {int64 k, float64 v, Utf8 s of 4-16 bytes, Boolean p} in pageable
// 1024-row HOST batches (every batch's offsets a window into one array, so offsets[0] != 0; its bitmap a window of whole bytes) —
// under `s = <constant> AND v > c` and `p AND v > c`: sqlrs_filter_push per batch, sqlrs_filter_push_async with
// sqlrs_filter_set_async_all_types off (the synchronous operator inside push_async: what these predicates always took) and on
// (one launch per batch, the operands read inside the kernel).  The three paths alternate; best of 2 after a warm-up; one JSON
// line per predicate, `on_over_off` = ms off / ms on.
static int bench_filter_all_types(int argc, char **argv) {
  const int64_t n = argc > 2 ? (int64_t)std::atof(argv[2]) : 2000000;
  const int64_t B = ((argc > 3 ? std::atoll(argv[3]) : 1024) + 7) / 8 * 8; // (whole bytes of bitmap per batch)
  sqlrs_ctx_t *ctx = nullptr;
  if (sqlrs_ctx_create(0, &ctx) != SQLRS_OK) {
    std::printf("{\"error\": \"no device\"}\n");
    return 2;
  }
  static const char *NAMES[16] = {"utah", "texas", "oregon", "alabama", "new york", "minnesota", "california", "mississippi",
                                  "pennsylvania", "massachusetts", "north carolina", "west virginia x", "district of col.", "ohio", "idaho", "nevada"};
  const char *WANT = "california";
  const double c = 0.5;
  std::vector<int64_t> k((size_t)n);
  std::vector<double> v((size_t)n);
  std::vector<int32_t> offs((size_t)n + 1);
  std::vector<char> data;
  std::vector<uint8_t> pbits((size_t)(n + 7) / 8 + 8, 0);
  int64_t expect[2] = {0, 0};
  offs[0] = 0;
  for (int64_t i = 0; i < n; i++) {
    k[(size_t)i] = (int64_t)(splitmix64(0xA7, (uint64_t)i) % 1000);
    v[(size_t)i] = (double)(splitmix64(0xF2, (uint64_t)i) >> 11) * (1.0 / 9007199254740992.0);
    const char *name = NAMES[splitmix64(0x57, (uint64_t)i) % 16];
    data.insert(data.end(), name, name + std::strlen(name));
    offs[(size_t)i + 1] = (int32_t)data.size();
    const bool p = splitmix64(0xB0, (uint64_t)i) & 1;
    if (p) pbits[(size_t)(i >> 3)] |= (uint8_t)(1u << (i & 7));
    expect[0] += std::strcmp(name, WANT) == 0 && v[(size_t)i] > c;
    expect[1] += p && v[(size_t)i] > c;
  }
  sqlrs_expr_node_t utf8_pred[7] = {}, bool_pred[5] = {};
  utf8_pred[0].op = SQLRS_EXPR_INPUT_REF;
  utf8_pred[0].index = 2;
  utf8_pred[1].op = SQLRS_EXPR_CONSTANT;
  utf8_pred[1].dtype = SQLRS_UTF8;
  utf8_pred[1].s = WANT;
  utf8_pred[2].op = SQLRS_EXPR_EQ;
  utf8_pred[3].op = SQLRS_EXPR_INPUT_REF;
  utf8_pred[3].index = 1;
  utf8_pred[4].op = SQLRS_EXPR_CONSTANT;
  utf8_pred[4].dtype = SQLRS_FLOAT64;
  utf8_pred[4].f = c;
  utf8_pred[5].op = SQLRS_EXPR_GT;
  utf8_pred[6].op = SQLRS_EXPR_AND;
  bool_pred[0].op = SQLRS_EXPR_INPUT_REF;
  bool_pred[0].index = 3;
  bool_pred[1] = utf8_pred[3];
  bool_pred[2] = utf8_pred[4];
  bool_pred[3] = utf8_pred[5];
  bool_pred[4].op = SQLRS_EXPR_AND;
  const sqlrs_expr_t preds[2] = {{utf8_pred, 7, 0}, {bool_pred, 5, 0}};
  const char *pred_names[2] = {"s = 'california' AND v > 0.5", "p AND v > 0.5"};
  const int64_t nb = (n + B - 1) / B;
  std::vector<sqlrs_column_t> cols((size_t)nb * 4);
  std::vector<sqlrs_batch_t> batches((size_t)nb);
  for (int64_t b = 0; b < nb; b++) {
    const int64_t m = std::min<int64_t>(B, n - b * B);
    sqlrs_column_t *cc = &cols[(size_t)b * 4];
    host_col(cc[0], SQLRS_INT64, k.data() + b * B, m);
    host_col(cc[1], SQLRS_FLOAT64, v.data() + b * B, m);
    host_col(cc[2], SQLRS_UTF8, data.data(), m);
    cc[2].offsets = offs.data() + b * B;
    host_col(cc[3], SQLRS_BOOLEAN, pbits.data() + b * B / 8, m);
    std::memset(&batches[(size_t)b], 0, sizeof(sqlrs_batch_t));
    batches[(size_t)b].num_rows = m;
    batches[(size_t)b].num_columns = 4;
    batches[(size_t)b].columns = cc;
  }
  const int DEPTH = 8; // tickets in flight, as in the other legs
  bool all_ok = true;
  for (int q = 0; q < 2; q++) {
    double best[3] = {1e30, 1e30, 1e30};
    int64_t kept[3] = {0, 0, 0};
    for (int rep = 0; rep < 3; rep++) { // (the first repetition warms the pool and the ring; the paths alternate)
      for (int path = 0; path < 3; path++) { // 0: push, 1: push_async with the switch off, 2: with it on
        auto t0 = std::chrono::steady_clock::now();
        sqlrs_filter_t *f = nullptr;
        CHECK(sqlrs_filter_create(ctx, &preds[q], &f));
        if (path == 2) CHECK(sqlrs_filter_set_async_all_types(f, 1));
        int64_t got = 0;
        if (path == 0) {
          for (int64_t b = 0; b < nb; b++) {
            sqlrs_batch_t *o = nullptr;
            CHECK(sqlrs_filter_push(f, &batches[(size_t)b], SQLRS_MEM_HOST, &o));
            got += o->num_rows;
            sqlrs_batch_release(o);
          }
        } else {
          std::vector<sqlrs_ticket_t *> tq((size_t)DEPTH, nullptr);
          auto take = [&](int64_t b) {
            sqlrs_batch_t *o = nullptr;
            CHECK(sqlrs_batch_wait(tq[(size_t)(b % DEPTH)], &o));
            got += o->num_rows;
            sqlrs_batch_release(o);
            return 0;
          };
          for (int64_t b = 0; b < nb; b++) {
            if (b >= DEPTH && take(b - DEPTH)) return 1;
            CHECK(sqlrs_filter_push_async(f, &batches[(size_t)b], &tq[(size_t)(b % DEPTH)]));
          }
          for (int64_t b = std::max<int64_t>(0, nb - DEPTH); b < nb; b++)
            if (take(b)) return 1;
        }
        sqlrs_filter_destroy(f);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        kept[path] = got;
        if (rep > 0 && ms < best[path]) best[path] = ms;
      }
    }
    const bool ok = kept[0] == expect[q] && kept[1] == expect[q] && kept[2] == expect[q];
    all_ok = all_ok && ok;
    std::printf("{\"leg\": \"filter_all_types\", \"predicate\": \"%s\", \"rows\": %lld, \"batches\": %lld, \"batch_rows\": %lld, \"kept\": %lld, "
                "\"depth\": %d, \"ms_push\": %.1f, \"Mrows_s_push\": %.1f, \"ms_async_off\": %.1f, \"Mrows_s_async_off\": %.1f, "
                "\"ms_async_on\": %.1f, \"Mrows_s_async_on\": %.1f, \"on_over_off\": %.2f, \"check\": \"%s\", \"note\": \"native caller (C ABI): "
                "pageable %lld-row host batches {int64, float64, utf8 of 4-16 bytes, boolean}, one result batch per input batch on the host; "
                "sqlrs_filter_push, then sqlrs_filter_push_async with sqlrs_filter_set_async_all_types 0 / 1 (alternating), best of 2 after a warm-up\"}\n",
                pred_names[q], (long long)n, (long long)nb, (long long)B, (long long)kept[2], DEPTH, best[0], (double)n / best[0] / 1e3, best[1],
                (double)n / best[1] / 1e3, best[2], (double)n / best[2] / 1e3, best[1] / best[2], ok ? "OK" : "mismatch", (long long)B);
  }
  sqlrs_ctx_destroy(ctx);
  return all_ok ? 0 : 1;
}

// ./bench_host_batches stage_types [rows = 2e6] [batch = 1024]
// SQLRS_EXPR_STAGE_ALL_TYPES: the three blocking operators fed pageable host batches of {int64 k, float64 v, Utf8 s of 4-16 bytes
// (about 1000 distinct), Boolean p}, 2 % NULLs in v and in s, each batch's offsets and bitmaps a window into one array.  Legs:
//   hash_agg   GROUP BY s: sum(v), count(p)
//   order      ORDER BY s, k
//   join_build Inner join, build side = the batches, key s; then ONE probe batch of 4096 strings (one in 64 has partners)
// Each leg runs with the flag off (the ordinary path: one upload per batch and buffer) and on, alternating in one process; after
// a warm-up each, the median of 5; the wall clock ends when the operator's finish has put the result on the host.  The two
// results of a leg must agree bit for bit (v is a multiple of 1/8: a SUM is exact in any order).  One JSON line per leg;
// "faster" = on_ms < off_ms - off_spread_ms.
static uint64_t digest_batch(const sqlrs_batch_t *o, uint64_t h) {
  auto mix = [&](uint64_t x) { h = (h ^ x) * 0x100000001b3ull; };
  if (!o) return h;
  mix((uint64_t)o->num_rows);
  for (int c = 0; c < o->num_columns; c++) {
    const sqlrs_column_t &col = o->columns[c];
    const uint8_t *valid = col.null_count ? (const uint8_t *)col.validity : nullptr;
    mix((uint64_t)col.null_count);
    for (int64_t r = 0; r < o->num_rows; r++) {
      if (valid && !((valid[r >> 3] >> (r & 7)) & 1)) {
        mix(0x6e756c6cull);
        continue;
      }
      if (col.dtype == SQLRS_UTF8) {
        const int32_t *off = (const int32_t *)col.offsets;
        const uint8_t *b = (const uint8_t *)col.values;
        mix((uint64_t)(off[r + 1] - off[r]));
        for (int32_t k = off[r]; k < off[r + 1]; k++) mix(b[k]);
      } else if (col.dtype == SQLRS_BOOLEAN)
        mix((((const uint8_t *)col.values)[r >> 3] >> (r & 7)) & 1);
      else
        mix(((const uint64_t *)col.values)[r]); // (the 8-byte types of this mode)
    }
  }
  return h;
}

static int bench_stage_types(int argc, char **argv) {
  const int64_t n = argc > 2 ? (int64_t)std::atof(argv[2]) : 2000000, B = argc > 3 ? std::atoll(argv[3]) : 1024;
  if (B % 8 != 0 || n < 1 || n * 16 > 2000000000ll) {
    std::printf("{\"error\": \"stage_types: needs a batch size that is a multiple of 8 and at most 1.25e8 rows\"}\n");
    return 2;
  }
  sqlrs_ctx_t *ctx = nullptr;
  if (sqlrs_ctx_create(0, &ctx) != SQLRS_OK) {
    std::printf("{\"error\": \"no device\"}\n");
    return 2;
  }
  const int64_t IDS = 1000, nb = (n + B - 1) / B;
  auto text_of = [](int64_t id, char *out) -> int32_t { // 4 hex digits of the id, then 0-12 letters
    const int32_t len = 4 + (int32_t)(id % 13);
    std::memset(out, 'a' + (int)(id % 26), (size_t)len);
    char hex[8];
    std::snprintf(hex, sizeof(hex), "%04llx", (unsigned long long)(id & 0xffff));
    std::memcpy(out, hex, 4);
    return len;
  };
  std::vector<int64_t> k((size_t)n);
  std::vector<double> v((size_t)n);
  std::vector<int32_t> soff((size_t)n + 1, 0);
  std::vector<char> sbytes((size_t)n * 16 + 16);
  std::vector<uint8_t> vvalid((size_t)(n + 7) / 8 + 8, 0), svalid((size_t)(n + 7) / 8 + 8, 0), p((size_t)(n + 7) / 8 + 8, 0);
  for (int64_t i = 0; i < n; i++) {
    k[(size_t)i] = i;
    v[(size_t)i] = (double)(splitmix64(0xB2, (uint64_t)i) % 8000) / 8.0;
    const uint8_t bit = (uint8_t)(1u << (i & 7));
    if (splitmix64(0xB3, (uint64_t)i) % 50 != 0) vvalid[(size_t)(i >> 3)] |= bit;
    if (splitmix64(0xB4, (uint64_t)i) & 1) p[(size_t)(i >> 3)] |= bit;
    int32_t len = 0;
    if (splitmix64(0xB5, (uint64_t)i) % 50 != 0) {
      svalid[(size_t)(i >> 3)] |= bit;
      len = text_of((int64_t)(splitmix64(0xB6, (uint64_t)i) % (uint64_t)IDS), sbytes.data() + soff[(size_t)i]);
    }
    soff[(size_t)i + 1] = soff[(size_t)i] + len;
  }
  // the batches, built once: 4 columns each
  std::vector<sqlrs_column_t> cols((size_t)nb * 4);
  std::vector<sqlrs_batch_t> batches((size_t)nb);
  for (int64_t b = 0; b < nb; b++) {
    const int64_t lo = b * B, m = std::min<int64_t>(B, n - lo);
    sqlrs_column_t *c = &cols[(size_t)b * 4];
    host_col(c[0], SQLRS_INT64, k.data() + lo, m);
    host_col(c[1], SQLRS_FLOAT64, v.data() + lo, m);
    c[1].validity = vvalid.data() + lo / 8;
    c[1].null_count = -1;
    host_col(c[2], SQLRS_UTF8, sbytes.data(), m);
    c[2].offsets = soff.data() + lo; // a window: offsets[0] != 0
    c[2].validity = svalid.data() + lo / 8;
    c[2].null_count = -1;
    host_col(c[3], SQLRS_BOOLEAN, p.data() + lo / 8, m);
    std::memset(&batches[(size_t)b], 0, sizeof(sqlrs_batch_t));
    batches[(size_t)b].num_rows = m;
    batches[(size_t)b].num_columns = 4;
    batches[(size_t)b].columns = c;
  }
  // the join's probe batch: 4096 strings over 64 x the ids of the build side
  const int64_t NP = 4096;
  std::vector<int32_t> poff((size_t)NP + 1, 0);
  std::vector<char> pbytes((size_t)NP * 16 + 16);
  for (int64_t i = 0; i < NP; i++)
    poff[(size_t)i + 1] = poff[(size_t)i] + text_of((int64_t)(splitmix64(0xB7, (uint64_t)i) % (uint64_t)(64 * IDS)), pbytes.data() + poff[(size_t)i]);
  sqlrs_column_t pcol;
  host_col(pcol, SQLRS_UTF8, pbytes.data(), NP);
  pcol.offsets = poff.data();
  sqlrs_batch_t probe{};
  probe.num_rows = NP;
  probe.num_columns = 1;
  probe.columns = &pcol;

  sqlrs_expr_node_t ref[4] = {};
  for (int i = 0; i < 4; i++) {
    ref[i].op = SQLRS_EXPR_INPUT_REF;
    ref[i].index = i;
  }
  int rc_all = 0;
  const char *leg_names[3] = {"hash_agg", "order", "join_build"};
  for (int leg = 0; leg < 3; leg++) {
    std::vector<double> ms[2];
    uint64_t dig[2] = {0, 0};
    int64_t out_rows[2] = {0, 0};
    auto run = [&](int on, bool timed) -> int { // 0 ok
      const int32_t flag = on ? SQLRS_EXPR_STAGE_ALL_TYPES : 0;
      std::vector<sqlrs_batch_t *> outs;
      auto t0 = std::chrono::steady_clock::now();
      if (leg == 0) {
        sqlrs_expr_t gb{&ref[2], 1, flag};
        sqlrs_agg_func_t aggs[2] = {};
        aggs[0].func = SQLRS_AGG_SUM;
        aggs[0].return_dtype = SQLRS_FLOAT64;
        aggs[0].arg = sqlrs_expr_t{&ref[1], 1, 0};
        aggs[1].func = SQLRS_AGG_COUNT;
        aggs[1].return_dtype = SQLRS_INT64;
        aggs[1].arg = sqlrs_expr_t{&ref[3], 1, 0};
        sqlrs_hash_agg_t *a = nullptr;
        CHECK(sqlrs_hash_agg_create(ctx, 1, &gb, 2, aggs, &a));
        for (int64_t b = 0; b < nb; b++) CHECK(sqlrs_hash_agg_push(a, &batches[(size_t)b]));
        sqlrs_batch_t *o = nullptr;
        CHECK(sqlrs_hash_agg_finish(a, SQLRS_MEM_HOST, &o));
        outs.push_back(o);
        sqlrs_hash_agg_destroy(a);
      } else if (leg == 1) {
        sqlrs_order_by_t ob[2] = {{sqlrs_expr_t{&ref[2], 1, flag}, 1, 0}, {sqlrs_expr_t{&ref[0], 1, 0}, 1, 0}};
        sqlrs_order_t *od = nullptr;
        CHECK(sqlrs_order_create(ctx, 2, ob, &od));
        for (int64_t b = 0; b < nb; b++) CHECK(sqlrs_order_push(od, &batches[(size_t)b]));
        sqlrs_batch_t *o = nullptr;
        CHECK(sqlrs_order_finish(od, SQLRS_MEM_HOST, &o));
        outs.push_back(o);
        sqlrs_order_destroy(od);
      } else {
        sqlrs_expr_t lk{&ref[2], 1, flag}, rk{&ref[0], 1, 0};
        const int32_t right_dtypes[1] = {SQLRS_UTF8};
        sqlrs_hash_join_t *j = nullptr;
        CHECK(sqlrs_hash_join_create(ctx, SQLRS_JOIN_INNER, 1, &lk, &rk, nullptr, 1, right_dtypes, &j));
        for (int64_t b = 0; b < nb; b++) CHECK(sqlrs_hash_join_build_push(j, &batches[(size_t)b]));
        CHECK(sqlrs_hash_join_build_finish(j));
        sqlrs_batch_t *o = nullptr, *tail = nullptr;
        CHECK(sqlrs_hash_join_probe_push(j, &probe, SQLRS_MEM_HOST, &o));
        CHECK(sqlrs_hash_join_finish(j, SQLRS_MEM_HOST, &tail));
        outs.push_back(o);
        outs.push_back(tail);
        sqlrs_hash_join_destroy(j);
      }
      const double t = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (timed) ms[on].push_back(t);
      uint64_t h = 0xcbf29ce484222325ull;
      out_rows[on] = 0;
      for (sqlrs_batch_t *o : outs) {
        h = digest_batch(o, h);
        if (o) out_rows[on] += o->num_rows;
        sqlrs_batch_release(o);
      }
      if (timed && h != dig[on]) dig[on] = ~0ull; // (a run that differs from its own warm-up)
      if (!timed) dig[on] = h;
      return 0;
    };
    for (int on = 0; on < 2; on++)
      if (run(on, false)) return 1;
    for (int rep = 0; rep < 5; rep++) // off and on alternate
      for (int on = 0; on < 2; on++)
        if (run(on, true)) return 1;
    double med[2], spread[2];
    for (int on = 0; on < 2; on++) {
      std::sort(ms[on].begin(), ms[on].end());
      med[on] = ms[on][2];
      spread[on] = ms[on][4] - ms[on][0];
    }
    const bool ok = dig[0] == dig[1] && dig[0] != ~0ull && out_rows[0] == out_rows[1] && out_rows[0] > 0;
    std::printf("{\"mode\": \"stage_types\", \"leg\": \"%s\", \"rows\": %lld, \"batches\": %lld, \"batch_rows\": %lld, \"out_rows\": %lld, "
                "\"off_ms\": %.1f, \"off_spread_ms\": %.1f, \"on_ms\": %.1f, \"on_spread_ms\": %.1f, \"Mrows_s_off\": %.1f, \"Mrows_s_on\": %.1f, "
                "\"on_over_off\": %.2f, \"faster\": %s, \"check\": \"%s\", \"note\": \"native caller (C ABI): pageable %lld-row host batches "
                "{int64, float64, utf8 of 4-16 bytes, boolean}, 2 %% NULLs in the float64 and the utf8 column, result on the host; "
                "SQLRS_EXPR_STAGE_ALL_TYPES off / on (alternating), median of 5 after a warm-up each, spread = max - min; on_over_off = "
                "off_ms / on_ms; faster = on_ms < off_ms - off_spread_ms\"}\n",
                leg_names[leg], (long long)n, (long long)nb, (long long)B, (long long)out_rows[1], med[0], spread[0], med[1], spread[1],
                (double)n / med[0] / 1e3, (double)n / med[1] / 1e3, med[0] / med[1], med[1] < med[0] - spread[0] ? "true" : "false",
                ok ? "OK" : "mismatch", (long long)B);
    std::fflush(stdout);
    if (!ok) rc_all = 1;
  }
  sqlrs_ctx_destroy(ctx);
  return rc_all;
}

int main(int argc, char **argv) {
  if (argc > 1 && std::strcmp(argv[1], "stage_types") == 0) return bench_stage_types(argc, argv);
  if (argc > 1 && std::strcmp(argv[1], "filter_all_types") == 0) return bench_filter_all_types(argc, argv);
  if (argc > 1 && std::strcmp(argv[1], "probe_filter") == 0) return bench_probe_filter(argc, argv);
  if (argc > 1 && std::strcmp(argv[1], "probe_keys") == 0) return bench_probe_keys(argc, argv);
  if (argc > 1 && std::strcmp(argv[1], "probe_general") == 0) return bench_probe_general(argc, argv, false);
  if (argc > 1 && std::strcmp(argv[1], "probe_utf8") == 0) return bench_probe_general(argc, argv, true);
  if (argc > 1 && std::strcmp(argv[1], "filter") == 0) return bench_filter(argc, argv);
  if (argc > 1 && std::strcmp(argv[1], "project") == 0) return bench_project(argc, argv);
  if (argc > 1 && std::strcmp(argv[1], "probe") == 0) return bench_probe(argc, argv);
  const int64_t n = argc > 1 ? (int64_t)std::atof(argv[1]) : 20000000, G = argc > 2 ? (int64_t)std::atof(argv[2]) : 1000000;
  const int64_t B = argc > 3 ? std::atoll(argv[3]) : 1024;
  sqlrs_ctx_t *ctx = nullptr;
  if (sqlrs_ctx_create(0, &ctx) != SQLRS_OK) {
    std::printf("{\"error\": \"no device\"}\n");
    return 2;
  }
  std::vector<int64_t> key((size_t)n);
  std::vector<double> val((size_t)n);
  for (int64_t i = 0; i < n; i++) {
    key[(size_t)i] = (int64_t)(splitmix64(0xA1, (uint64_t)i) % (uint64_t)G);
    val[(size_t)i] = (double)(splitmix64(0xF2, (uint64_t)i) >> 11) * (1.0 / 9007199254740992.0);
  }
  sqlrs_expr_node_t k0{}, v1{};
  k0.op = SQLRS_EXPR_INPUT_REF;
  k0.index = 0;
  v1.op = SQLRS_EXPR_INPUT_REF;
  v1.index = 1;
  sqlrs_expr_t gb{&k0, 1, 0};
  sqlrs_agg_func_t aggs[2] = {};
  aggs[0].func = SQLRS_AGG_COUNT;
  aggs[0].return_dtype = SQLRS_INT64;
  aggs[0].arg = sqlrs_expr_t{&v1, 1, 0};
  aggs[1].func = SQLRS_AGG_SUM;
  aggs[1].return_dtype = SQLRS_FLOAT64;
  aggs[1].arg = sqlrs_expr_t{&v1, 1, 0};
  double best = 1e30, sum_check = 0;
  int64_t groups = 0, count_check = 0, batches = 0;
  for (int rep = 0; rep < 3; rep++) { // (the first repetition warms the pool and the staging area)
    auto t0 = std::chrono::steady_clock::now();
    sqlrs_hash_agg_t *a = nullptr;
    CHECK(sqlrs_hash_agg_create(ctx, 1, &gb, 2, aggs, &a));
    batches = 0;
    for (int64_t lo = 0; lo < n; lo += B) {
      const int64_t m = std::min<int64_t>(B, n - lo);
      sqlrs_column_t cols[2] = {};
      cols[0].dtype = SQLRS_INT64;
      cols[0].mem = SQLRS_MEM_HOST;
      cols[0].length = m;
      cols[0].values = key.data() + lo;
      cols[1].dtype = SQLRS_FLOAT64;
      cols[1].mem = SQLRS_MEM_HOST;
      cols[1].length = m;
      cols[1].values = val.data() + lo;
      sqlrs_batch_t b{};
      b.num_rows = m;
      b.num_columns = 2;
      b.columns = cols;
      CHECK(sqlrs_hash_agg_push(a, &b));
      batches++;
    }
    sqlrs_batch_t *out = nullptr;
    CHECK(sqlrs_hash_agg_finish(a, SQLRS_MEM_HOST, &out));
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    groups = out->num_rows;
    count_check = 0;
    sum_check = 0;
    const int64_t *cnt = (const int64_t *)out->columns[1].values;
    const double *sm = (const double *)out->columns[2].values;
    for (int64_t g = 0; g < groups; g++) {
      count_check += cnt[g];
      sum_check += sm[g];
    }
    sqlrs_batch_release(out);
    sqlrs_hash_agg_destroy(a);
    if (rep > 0 && ms < best) best = ms;
  }
  double exp_sum = 0;
  for (int64_t i = 0; i < n; i++) exp_sum += val[(size_t)i];
  const bool ok = count_check == n && std::abs(sum_check - exp_sum) <= 1e-9 * exp_sum;
  std::printf("{\"rows\": %lld, \"batches\": %lld, \"batch_rows\": %lld, \"groups\": %lld, \"ms\": %.1f, \"Mrows_s\": %.1f, "
              "\"pcie_GBps\": %.2f, \"check\": \"%s\", \"note\": \"native caller (C ABI, no interpreter): pageable %lld-row host "
              "batches through sqlrs_hash_agg_push's host staging, result on the host, best of 2 after a warm-up\"}\n",
              (long long)n, (long long)batches, (long long)B, (long long)groups, best, (double)n / best / 1e3,
              16.0 * (double)n / best / 1e6, ok ? "OK" : "mismatch", (long long)B);
  sqlrs_ctx_destroy(ctx);
  return ok ? 0 : 1;
}
