// hdb_group.hip -- grouped top-k (hdb_topk_grouped_host, hdb_collapse_groups; include/hyperdb_hip.h) for gfx950.
//
// Every row may carry a group id (a document whose chunks are rows).  The grouped top-k of a query is the first k rows of the
// ungrouped ranking (score descending, row ascending) that open a group: one row per group, k distinct groups.  Two ways there:
//
//   hdb_group_collapse_kernel  the fast rounds and the primitive.  A ranked list [m <= 2048] of one query -> its first k first
//                              occurrences.  One workgroup per query: keys (group id, list position) sorted in LDS (16 KiB), a key
//                              that opens a run of equal group ids marks its list position, the marks are prefix-summed in list
//                              order and the first k marked entries are copied out, then the -1 / -inf tail and the status word.
//   hdb_group_best_kernel      the exact pass, between the score pass into sbuf and the radix selection of run_pipeline's exact
//   hdb_group_demote_kernel    shape.  best[q][g] = max over the rows of group g of hdb_pack(score, row) -- the 64-bit key whose
//                              maximum is "highest score, lowest row" -- by 64-bit atomicMax; lanes of a wave that hold a run of
//                              equal ids combine their keys first (a segmented max by shuffles) and only the run's last lane
//                              issues the atomic: a document's chunks are adjacent rows.  Then every row that is not its group's
//                              best gets -inf in sbuf, the state a masked row is in, and the selection runs unchanged with the
//                              caller's k.
//   hdb_group_finish_kernel    behind the exact pass's finalize: an entry that came out at -inf (k exceeds the groups that can be
//                              returned) becomes the -1 padding, and HDB_Q_BADROW is OR-ed in where the demote pass met a bad id.
//
// The library does not trust the ids: every kernel compares an id against [0, n_groups) before an address is formed from it.  A
// row with an id outside is treated as masked and reported (HDB_Q_BADROW); nothing is indexed with it.
#include "hdb_common.h"
#include "hdb_first_occ.h"
#include "../../include/hyperdb_hip.h"
#include <algorithm>

#define HDB_GROUP_MAXM 2048
#define HDB_GROUP_NONE HDB_FIRST_NONE

// ------------------------------------------------------------------------------------------------------------------------
// Collapse.  idx / score: [nq][m] as hdb_topk writes them (row_base added; -1 = padding).  An entry at -inf is an excluded row
// that an exact selection handed out because nothing else was left: padding as well.  carry: the bits of status_in that the
// output keeps (HDB_Q_NAN for the public entry; the host schedule also keeps the sampled call's failure bits).
// A list is exhaustive -- nothing eligible is missing from it -- when it holds padding or when m >= n.
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void hdb_group_collapse_kernel(const int64_t* idx, const float* score, int m, uint32_t k,
                                                                  const int32_t* groups, int32_t n_groups, int64_t n, int64_t row_base,
                                                                  int64_t* idx_out, float* score_out, const int32_t* status_in,
                                                                  int32_t* status_out, int32_t carry) {
    __shared__ unsigned long long key[HDB_GROUP_MAXM];
    __shared__ uint8_t first[HDB_GROUP_MAXM];
    __shared__ uint32_t wsum[16];
    __shared__ int s_bad, s_pad;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { s_bad = 0; s_pad = 0; }
    int P = 64;
    while (P < m) P <<= 1;                                    // m <= HDB_GROUP_MAXM, so P <= HDB_GROUP_MAXM
    __syncthreads();
    const int64_t* my_idx = idx + (int64_t)q * m;
    const float* my_score = score + (int64_t)q * m;
    for (int i = tid; i < P; i += 1024) {
        unsigned long long kx = HDB_GROUP_NONE;
        if (i < m) {
            const int64_t id = my_idx[i];
            if (id < 0 || my_score[i] == -INFINITY) {
                atomicOr(&s_pad, 1);
            } else {
                const uint64_t loc = (uint64_t)id - (uint64_t)row_base;       // the true difference when id >= row_base
                if (id < row_base || loc >= (uint64_t)n) {
                    atomicOr(&s_bad, 1);                      // out of range: nothing is read for it
                } else {
                    const int32_t g = groups[loc];
                    if ((uint32_t)g >= (uint32_t)n_groups) atomicOr(&s_bad, 1);
                    else kx = ((unsigned long long)(uint32_t)g << 32) | (unsigned long long)(uint32_t)i;
                }
            }
        }
        key[i] = kx;
        first[i] = 0;
    }
    __syncthreads();
    // a key that opens a run of equal group ids is its group's first occurrence in the list: its list position gets marked
    hdb_mark_first_occurrences(key, first, P, tid, 1024);
    // the marks, prefix-summed in list order: thread t owns positions [t per, (t + 1) per)
    const int per = (P + 1023) / 1024;
    const int i0 = tid * per;
    uint32_t mine = 0;
    for (int i = i0; i < i0 + per && i < P; ++i) mine += first[i];
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t v = __shfl_up(incl, o, 64); if (lane >= o) incl += v; }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t pos = incl - mine, total = 0;
    for (int w = 0; w < 16; ++w) { if (w < wave) pos += wsum[w]; total += wsum[w]; }
    int64_t* out_i = idx_out + (int64_t)q * k;
    float* out_s = score_out + (int64_t)q * k;
    for (int i = i0; i < i0 + per && i < P; ++i)
        if (first[i]) {
            if (pos < k) { out_i[pos] = my_idx[i]; out_s[pos] = my_score[i]; }
            ++pos;
        }
    for (uint32_t i = total + tid; i < k; i += 1024) { out_i[i] = -1; out_s[i] = -INFINITY; }
    if (tid == 0 && status_out) {
        int32_t st = status_in ? (status_in[q] & carry) : 0;
        if (s_bad) st |= HDB_Q_BADROW;
        if (total < k && !s_pad && (int64_t)m < n) st |= HDB_Q_GROUPS_SHORT;
        status_out[q] = st;
    }
}

extern "C" int hdb_launch_group_collapse(const int64_t* idx, const float* score, int nq, int m, int k, const int32_t* groups,
                                         int64_t n_groups, int64_t n, int64_t row_base, int64_t* idx_out, float* score_out,
                                         const int32_t* status_in, int32_t* status_out, int carry, void* stream) {
    if (m < 1 || m > HDB_GROUP_MAXM || k < 1 || k > HDB_GROUP_MAXM || nq < 1 || n_groups < 1 || n_groups > 0x7FFFFFFFll || n < 0)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(hdb_group_collapse_kernel, dim3(nq), dim3(1024), 0, (hipStream_t)stream, idx, score, m, (uint32_t)k, groups,
                       (int32_t)n_groups, n, row_base, idx_out, score_out, status_in, status_out, (int32_t)carry);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------------
// Group best.  scores: [nq][ld] (the exact shape's sbuf: bias added, masked rows and NaN at -inf), best: [nq][n_groups], zero --
// below every real key -- on entry.  grid = (blocks, queries of the chunk), 256 threads; a wave takes 64 consecutive rows.
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hdb_group_best_kernel(const float* scores, int64_t n, int64_t ld, const int32_t* groups,
                                                             int32_t n_groups, unsigned long long* best) {
    const int q = blockIdx.y, lane = threadIdx.x & 63;
    const float* sq = scores + (int64_t)q * ld;
    unsigned long long* bq = best + (int64_t)q * n_groups;
    for (int64_t r0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63); r0 < n; r0 += (int64_t)gridDim.x * 256) {      // (wave-uniform)
        const int64_t r = r0 + lane;
        int32_t g = -1;
        unsigned long long kx = 0ull;
        if (r < n) {
            const int32_t gr = groups[r];
            if ((uint32_t)gr < (uint32_t)n_groups) { g = gr; kx = hdb_pack(hdb_canon(sq[r]), (uint32_t)r); }      // the id check comes before the address
        }
        // segmented inclusive max over runs of equal ids: after the steps the last lane of a run holds the run's maximum (a lane
        // further away with the same id adds a key of the same group: harmless)
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int32_t og = __shfl_up(g, o, 64);
            const unsigned long long ok = __shfl_up(kx, o, 64);
            if (lane >= o && og == g && ok > kx) kx = ok;
        }
        const int32_t ng = __shfl_down(g, 1, 64);
        const bool last = lane == 63 || ng != g;
        if (g >= 0 && last) atomicMax(&bq[g], kx);
    }
}

// Demote.  Row r keeps its score only where best[q][group[r]] names r; a row with a bad id gets -inf too and raises *bad.
// Four rows per thread: sbuf's leading dimension is a multiple of 4 floats and its queries start 16-byte aligned, so the scores
// move as 16-byte pieces; the ids do where the caller's array is 16-byte aligned (VEC) and the quad lies inside the matrix.
template <bool VEC>
__global__ __launch_bounds__(256) void hdb_group_demote_kernel(float* scores, int64_t n, int64_t ld, const int32_t* groups, int32_t n_groups,
                                                               const unsigned long long* best, int* bad) {
    const int q = blockIdx.y;
    float* sq = scores + (int64_t)q * ld;
    const unsigned long long* bq = best + (int64_t)q * n_groups;
    const int64_t quads = (n + 3) >> 2;
    bool any_bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < quads; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i << 2;
        float4 s = *reinterpret_cast<const float4*>(sq + r);         // (r + 3 < ld: the pad behind row n - 1 exists)
        int32_t g[4] = {-1, -1, -1, -1};
        if (VEC && r + 3 < n) {
            const int4 gv = *reinterpret_cast<const int4*>(groups + r);
            g[0] = gv.x; g[1] = gv.y; g[2] = gv.z; g[3] = gv.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (r + e < n) g[e] = groups[r + e];
        }
        float v[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (r + e >= n) continue;
            bool keep = false;
            if ((uint32_t)g[e] < (uint32_t)n_groups) keep = (0xFFFFFFFFu - (uint32_t)(bq[g[e]] & 0xFFFFFFFFull)) == (uint32_t)(r + e);
            else any_bad = true;
            if (!keep) v[e] = -INFINITY;
        }
        *reinterpret_cast<float4*>(sq + r) = make_float4(v[0], v[1], v[2], v[3]);
    }
    if (any_bad) atomicOr(bad, 1);
}

// Behind the finalize of the exact pass: entries at -inf are padding, and a bad id anywhere in the index marks every query.
__global__ __launch_bounds__(256) void hdb_group_finish_kernel(int64_t* idx, const float* score, int nq, uint32_t k, int32_t* status, const int* bad) {
    const int64_t total = (int64_t)nq * k;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
        if (score[i] == -INFINITY) idx[i] = -1;
    if (status && blockIdx.x == 0 && (int)threadIdx.x < nq && *bad) status[threadIdx.x] |= HDB_Q_BADROW;
}

extern "C" int hdb_launch_group_best(const float* scores, int64_t n, int64_t ld, int nq, const int32_t* groups, int64_t n_groups,
                                     unsigned long long* best, void* stream) {
    if (n < 1 || ld < n || nq < 1 || n_groups < 1 || n_groups > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
    const dim3 grid(hdb_grid_for(n, 256, std::max(4, 2048 / nq)), nq);
    hipLaunchKernelGGL(hdb_group_best_kernel, grid, dim3(256), 0, (hipStream_t)stream, scores, n, ld, groups, (int32_t)n_groups, best);
    return (int)hipGetLastError();
}

extern "C" int hdb_launch_group_demote(float* scores, int64_t n, int64_t ld, int nq, const int32_t* groups, int64_t n_groups,
                                       const unsigned long long* best, int* bad, void* stream) {
    if (n < 1 || ld < n || (ld & 3) != 0 || (reinterpret_cast<uintptr_t>(scores) & 15) != 0 || nq < 1 || n_groups < 1 || n_groups > 0x7FFFFFFFll)
        return (int)hipErrorInvalidValue;
    const dim3 grid(hdb_grid_for((n + 3) / 4, 256, std::max(4, 2048 / nq)), nq);
    if ((reinterpret_cast<uintptr_t>(groups) & 15) == 0)
        hipLaunchKernelGGL(hdb_group_demote_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, scores, n, ld, groups, (int32_t)n_groups, best, bad);
    else
        hipLaunchKernelGGL(hdb_group_demote_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, scores, n, ld, groups, (int32_t)n_groups, best, bad);
    return (int)hipGetLastError();
}

extern "C" int hdb_launch_group_finish(int64_t* idx, const float* score, int nq, int k, int32_t* status, const int* bad, void* stream) {
    if (nq < 1 || nq > 256 || k < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(hdb_group_finish_kernel, dim3(hdb_grid_for((int64_t)nq * k, 256, 256)), dim3(256), 0, (hipStream_t)stream, idx, score, nq,
                       (uint32_t)k, status, bad);
    return (int)hipGetLastError();
}
