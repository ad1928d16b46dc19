// hdb_emit.h -- the shared epilogue of the row scans (hdb_scan.hip, hdb_bscan.hip): raw row sum -> final score, then store / filter,
// and the per-block survivor stage behind the filter.  One text for both units, so a row's score is finished the same way whatever
// kernel summed it.
#pragma once
#include "hdb_common.h"
#include "../../include/hyperdb_hip.h"

// Survivors of a filter pass (MODE 1) wait in LDS, per block and query slot, and reach the global candidate lists with ONE atomic
// per block and query at the end of the block's tiles.  A returning atomic per survivor on the per-query counters (one cache line:
// ~88 per us) was what small matrices spent their time in: n = 200k x 100 float32, 16 queries, ~2 k survivors each -- 374 us of
// filter pass for 11 us of matrix; the N <= 8192 path, where every row survives, likewise (tools/diag_small_valu.py).
#define HDB_STAGE_CAP 128
struct HdbStage {
    unsigned long long buf[4][HDB_STAGE_CAP];      // up to four query slots per block (QT, QH <= 4)
    unsigned int cnt[4];
    unsigned int base;
};
__device__ __forceinline__ void hdb_stage_init(HdbStage& st) { if (threadIdx.x < 4) st.cnt[threadIdx.x] = 0u; }   // (before a block barrier)
// every thread of the block, after its last tile; slot s holds the survivors of local query ql0 + s
__device__ __forceinline__ void hdb_stage_flush(const ScanArgs& a, HdbStage& st, int ql0, int nslots) {
    __syncthreads();
    for (int s = 0; s < nslots; ++s) {
        const unsigned int have = min(st.cnt[s], (unsigned int)HDB_STAGE_CAP);        // (block-uniform)
        if (have == 0u) continue;
        if (threadIdx.x == 0) st.base = atomicAdd(&a.cnt[(ql0 + s) * HDB_CNT_STRIDE], have);
        __syncthreads();
        const unsigned int base = st.base;
        for (unsigned int e = threadIdx.x; e < have; e += blockDim.x)
            if (base + e < a.cap) a.cand[(int64_t)(ql0 + s) * a.cap + base + e] = st.buf[s][e];
        __syncthreads();
    }
}

// Shared epilogue: raw row sum -> final score of hyperDB_ranking_algorithm_sort, then store / filter.
template <int MODE, typename Acc>
__device__ __forceinline__ void hdb_emit(const ScanArgs& a, int q, int64_t row, int64_t out_i, Acc sum, HdbStage* stg = nullptr, int slot = 0) {
    float s;
    if (a.metric == HDB_EUCLIDEAN) {
        s = (float)(Acc(1) / (Acc(1) + sqrt(sum)));                       // 1/(1+||v-q||), :49-51
    } else if (a.metric == HDB_MANHATTAN) {
        s = (float)(Acc(1) / (Acc(1) + sum));                             // 1/(1+sum|v-q|), :59-60
    } else if (a.metric == HDB_EUCLIDEAN_DIST) {
        s = (float)sqrt(sum);
    } else if (a.metric == HDB_COSINE) {
        s = (float)sum * a.inv_norm[row] * a.qinv[q];                      // :37-41 with cached norms
    } else {
        s = (float)sum;                                                    // dot / hamming
    }
    if (a.bias) s += a.bias[row];                                          // recency, :186
    const bool masked = a.mask && !a.mask[row];                            // filtered-out row
    if (masked) s = -INFINITY;
    if (!a.raw) s = hdb_canon(s);                                          // NaN -> -inf, :174
    if (MODE == 0) {
        a.scores[(int64_t)(q - a.q0) * a.ld + out_i] = s;
    } else {
        const int ql = q - a.q0;
        if (!masked && s >= a.thr[ql]) {
            const unsigned long long ent = hdb_pack(s, (uint32_t)row);
            if (stg) {
                const unsigned int lp = atomicAdd(&stg->cnt[slot], 1u);              // LDS
                if (lp < HDB_STAGE_CAP) { stg->buf[slot][lp] = ent; return; }
            }
            const uint32_t pos = atomicAdd(&a.cnt[ql * HDB_CNT_STRIDE], 1u);         // the slot is full: straight to the global list
            if (pos < a.cap) a.cand[(int64_t)ql * a.cap + pos] = ent;
        }
    }
}
