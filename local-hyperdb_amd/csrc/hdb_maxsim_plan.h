// hdb_maxsim_plan.h -- how hdb_maxsim_host cuts a call: sets per block, vectors per chunk, and the call its score pass plans with.
//
// Pure host functions of plain numbers, in the spirit of hdb_group_plan.h: no HIP call, no hdb_index, so tests/maxsim_plan_check.hip
// runs them over a grid.  A call of ns sets (nv flat vectors, set s = vectors off[s] .. off[s + 1]):
//   block   sb consecutive sets whose running sums acc[sb][ld_g] (4 bytes per set and group) stay in the workspace together; the
//           selection runs once per block, over acc, so sb is at most 256 (one finalize workgroup per set);
//   chunk   cq consecutive vectors of a block's flat range, scored into sbuf[cq][ld_n] (4 bytes per vector and row) by the exact
//           score pass and reduced into acc by one launch.  A chunk may cut across set boundaries -- one pass over V serves several
//           sets -- and never across a block's end.
// Both count against exact_bytes: acc gets at most half of it while more than one set is in a block, and never so much that one
// vector's scores no longer fit; the rest is sbuf's.  Where one vector and one set fit together, sbuf + acc stay inside exact_bytes;
// where they do not, the plan is sb = cq = 1 and the workspace is what it must be.
#pragma once
#include "hdb_plan.h"

struct MaxsimPlan {
    int sb = 1;                                   // sets per block
    int cq = 1;                                   // vectors per chunk, at most cq_cap
    int64_t ld_n = 0, ld_g = 0;                   // leading dimensions of sbuf and acc
};

// cq_cap: the most vectors the score pass takes per launch (256; 128 in K slices -- TopkPlan::ksplit)
static inline MaxsimPlan maxsim_plan(int64_t n, int64_t n_groups, int32_t ns, int cq_cap, int64_t exact_bytes) {
    MaxsimPlan m;
    m.ld_n = (int64_t)align_up((size_t)std::max<int64_t>(n, 1), 4);
    m.ld_g = (int64_t)align_up((size_t)std::max<int64_t>(n_groups, 1), 4);
    const int64_t vec = m.ld_n * 4, set = m.ld_g * 4;
    const int64_t for_acc = std::min<int64_t>(exact_bytes / 2, exact_bytes - vec);
    m.sb = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(ns, 256), for_acc / set));
    const int64_t for_sbuf = exact_bytes - (int64_t)m.sb * set;
    m.cq = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int>(cq_cap, 256), for_sbuf / vec));
    return m;
}

// Chunks of a call under a plan: per block, the block's vectors in pieces of cq (the stat maxsim_chunks).
static inline int64_t maxsim_chunks(const MaxsimPlan& m, const int32_t* off, int32_t ns) {
    int64_t chunks = 0;
    for (int32_t s0 = 0; s0 < ns; s0 += m.sb) {
        const int32_t s1 = std::min<int32_t>(ns, s0 + m.sb);
        chunks += ((int64_t)off[s1] - off[s0] + m.cq - 1) / m.cq;
    }
    return chunks;
}

// The call the score pass hands to plan_topk: the exact selection's score pass over all rows for the call's nv flat vectors, on
// matrices of up to HDB_CAND_CAP rows too (the VALU scan), never through a row list (the reduction indexes sbuf by row).
static inline TopkCall maxsim_call(int32_t nv, int32_t k, int metric) {
    TopkCall c{nv, k, metric, true, true, 0};
    c.maxsim = true;
    return c;
}
// Does a plan have the shape that pass runs?  (hamming / jaccard and k > HDB_MAX_K are refused before anything is planned.)
static inline bool maxsim_shape(const TopkPlan& p) {
    return p.path == HDB_PATH_PIPELINE && p.exact && !p.small && !p.subset && p.n_best == 0 && p.ld_scores == p.ld_n;
}
