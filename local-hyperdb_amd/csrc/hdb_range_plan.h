// hdb_range_plan.h -- how hdb_range_host cuts a call: queries per chunk, tiles per query, and the call its score pass plans with.
//
// Pure host functions of plain numbers, in the spirit of hdb_maxsim_plan.h: no HIP call, no hdb_index, so tests/range_plan_check.hip
// runs them over a grid.  A call of nq queries over n rows:
//   chunk   cq consecutive queries, scored into sbuf[cq][ld_n] (4 bytes per query and row) by the exact score pass; cq is the most
//           queries whose scores stay inside exact_bytes, at most cq_cap -- and 1 where one query's scores alone exceed the budget
//           (the workspace is then what it must be);
//   tile    HDB_RANGE_TILE consecutive rows of one query: one workgroup of the count pass and of the emit pass, one counter.
// The result has no plan: its size is a fact of the data, known per chunk once the counts are back (hdb_range_result_bytes per entry
// against the budget range_bytes).
#pragma once
#include "hdb_maxsim_plan.h"
#include "../../include/hyperdb_hip.h"

struct RangePlan {
    int cq = 1;                                   // queries per chunk, at most cq_cap
    int64_t ld_n = 0;                             // leading dimension of sbuf
    int64_t ntiles = 0;                           // tiles per query
};

// cq_cap: the most queries the score pass takes per launch (256; 128 in K slices -- TopkPlan::ksplit)
static inline RangePlan range_plan(int64_t n, int32_t nq, int cq_cap, int64_t exact_bytes) {
    RangePlan r;
    r.ld_n = (int64_t)align_up((size_t)std::max<int64_t>(n, 1), 4);
    r.cq = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(std::max<int32_t>(nq, 1), std::min(cq_cap, 256)), exact_bytes / (r.ld_n * 4)));
    r.ntiles = (n + HDB_RANGE_TILE - 1) / HDB_RANGE_TILE;
    return r;
}
// Chunks of a call under a plan (the stat range_chunks).
static inline int64_t range_chunks(const RangePlan& r, int32_t nq) { return ((int64_t)nq + r.cq - 1) / r.cq; }

// Device bytes one returned entry costs: its packed 64-bit key, its int64 index and its float32 score.
static inline int64_t hdb_range_result_bytes(int64_t total) { return total * 20; }

// The call the score pass hands to plan_topk: the multi-vector call's (hdb_maxsim_plan.h) -- the exact shape on every matrix size,
// all rows, never a row list, never matrix-core euclidean: ||v||^2 + ||q||^2 - 2 v.q cancels exactly on the near-duplicates a high
// threshold selects.  k does not matter to that pass (nothing is selected): 1.
static inline TopkCall range_call(int32_t nq, int metric) { return maxsim_call(nq, 1, metric); }
static inline bool range_shape(const TopkPlan& p) { return maxsim_shape(p); }
