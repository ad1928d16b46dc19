// hdb_group_plan.h -- how hdb_topk_grouped_host runs: the schedule of its fast rounds and the call its exact pass plans with.
//
// Pure host functions of plain numbers, in the spirit of hdb_plan.h: no HIP call, no hdb_index, so tests/group_plan_check.hip runs
// them over a grid.  A grouped call of k groups:
//   fast round 1   hdb_topk of k1 = min(n, HDB_MAX_K, k * group_oversample) rows per query -- whatever path that call takes -- and one
//                  collapse launch (hdb_group.hip) that keeps each group's first occurrence;
//   fast round 2   for the queries whose list ended before k groups were seen (HDB_Q_GROUPS_SHORT): the same at
//                  k2 = min(n, HDB_MAX_K, 4 * k1), where that is more than k1;
//   exact pass     for the queries still short after the last round, for those whose sampled call failed (HDB_Q_UNDERFLOW /
//                  HDB_Q_OVERFLOW), and for every query when group_fast_rounds = 0: the exact shape of run_pipeline with the group
//                  best and demote launches between the score pass and the selection (group_exact_call below).
// A list of n rows is the whole ranking: a round at k' = n is never short, so no round follows it.
#pragma once
#include "hdb_plan.h"          // (HDB_GROUP_OVERSAMPLE_MAX and HDB_GROUP_ROUNDS_MAX: beside the option table that clamps to them)

struct GroupRounds {
    int rounds = 0;                               // fast rounds the call may run (0: the exact pass answers every query)
    int32_t kr[HDB_GROUP_ROUNDS_MAX] = {0, 0};    // rows per query of each round, strictly increasing, never above min(n, HDB_MAX_K)
};

static inline GroupRounds group_rounds(int64_t n, int32_t k, int64_t oversample, int64_t fast_rounds) {
    GroupRounds g;
    if (n <= 0 || k < 1 || fast_rounds <= 0) return g;
    const int64_t os = std::max<int64_t>(1, std::min<int64_t>(oversample, HDB_GROUP_OVERSAMPLE_MAX));
    const int64_t cap = std::min<int64_t>(n, HDB_MAX_K);
    const int64_t k1 = std::min<int64_t>(cap, (int64_t)k * os);
    g.kr[g.rounds++] = (int32_t)k1;
    const int64_t k2 = std::min<int64_t>(cap, 4 * k1);
    if (fast_rounds >= 2 && k2 > k1) g.kr[g.rounds++] = (int32_t)k2;
    return g;
}

// The call the exact grouped pass hands to plan_topk: the exact selection over all rows with the per-group maxima in the workspace.
static inline TopkCall group_exact_call(int32_t nq, int32_t k, int metric, int64_t n_groups) {
    return TopkCall{nq, k, metric, true, true, n_groups};
}
// Does a plan have the shape that pass runs?  (hamming / jaccard and k > HDB_MAX_K are refused before anything is planned.)
static inline bool group_exact_shape(const TopkPlan& p) {
    return p.path == HDB_PATH_PIPELINE && p.exact && !p.small && !p.subset && p.n_best > 0 && p.ld_scores == p.ld_n;
}
