// hdb_rerank.hip -- exact scores of per-query candidate lists (hdb_rerank, include/hyperdb_hip.h) for gfx950.
//
// Every other scoring entry scores all rows, or one row set shared by the queries of the call.  Here query q comes with ITS OWN
// list of up to HDB_CAND_CAP row ids (the output of a cheaper index, a keyword index, a per-query filter) and the answer is the
// exact top-k among them.  Two launches of this unit sit between the query preparation and the finalize of the multi-kernel pipeline:
//
//   hdb_rerank_prep_kernel   one workgroup per query: ids -> local rows, sorted ascending in LDS.  Negative ids (padding) are
//                            dropped, ids outside [row_base, row_base + n) are dropped and flagged (HDB_Q_BADROW) -- an id is
//                            compared against the bounds before anything is indexed with it, the mask byte included --, masked
//                            rows and repeats are dropped.  The compact list, its count and the query's status word are written.
//                            Ascending rows give the gather its locality; distinct rows are what the finalize's rank sort needs
//                            (two equal packed entries would land in one output slot).
//   hdb_rerank_score_kernel  grid = (tiles of list positions, queries of the chunk), the query in LDS.  A 16-lane group takes one
//                            candidate and reads its row as contiguous 256-byte pieces -- the shape the row-list scan gathers
//                            whole rows with at the streaming rate.  The pass is bound by the latency of the gather, so for rows
//                            of 256 / 384 / 512 / 768 / 1536 bytes every load of a group's candidates is issued before the first
//                            use, 6-8 loads of 16 bytes per lane.  Workgroups past the query's count leave at once: the work is
//                            that of the valid candidates, not of m.
//
// The score contract.  A (query, row) pair gets the float32 bits the VALU scan (hdb_scan.hip) gives that row: the lane split and
// chunk order of hdb_scan_kernel (16-byte pieces l16 + 16 j, a dead piece adds 0 * q) or hdb_scan_generic_kernel (elements
// l16 + 16 i), the same accumulate expressions for the product, the squared and the absolute difference, hdb_rows4_sum with the
// candidate in all four row slots and the lane that owns slot row & 3 -- the slot the row has in its dense tile --, then hdb_emit's
// epilogue.  hdb_quant_rescore_kernel (hdb_quant.hip) does the same for three dtypes and three metrics from lists the shadow's
// filter wrote; this unit serves the six byte-addressed dtypes and manhattan, and pearson as cosine on centred queries with the
// row scale 1/(sd d) in the place of 1/||v||.  Nothing depends on the position of a row in the list or on the other candidates.
// The squared differences are accumulated with explicit fma, element by element in order.  Written as acc += df * df, the first two
// squares of an unrolled chain are a sum of two products, and the compiler is free to fuse either one: it rounded the SECOND square
// and fused the first, where the scan's kernels fuse in element order -- one float32 step apart on 1-2 % of the rows (measured
// against the masked exact call, 20 001 Gaussian rows).  The explicit form is the scan's chain whatever the unrolling.
#include "hdb_common.h"
#include "hdb_unpack.h"
#include "../../include/hyperdb_hip.h"
#include <algorithm>

// ------------------------------------------------------------------------------------------------------------------------
// List preparation.  LDS: the keys (32 KiB).  The sentinel 0xFFFFFFFF is no row: an index holds at most 2^32 - 2 rows.
// ------------------------------------------------------------------------------------------------------------------------
#define HDB_RR_NONE 0xFFFFFFFFu
__global__ __launch_bounds__(1024) void hdb_rerank_prep_kernel(const int64_t* cand, int m, int64_t n, int64_t row_base, const uint8_t* mask,
                                                               const int* qnan, int64_t* rows, uint32_t* cnt, int32_t* status) {
    __shared__ uint32_t key[HDB_CAND_CAP];
    __shared__ uint32_t wsum[16];
    __shared__ int s_bad;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_bad = 0;
    int P = 64;
    while (P < m) P <<= 1;                                    // m <= HDB_CAND_CAP, so P <= HDB_CAND_CAP
    __syncthreads();
    for (int i = tid; i < P; i += 1024) {
        uint32_t kx = HDB_RR_NONE;
        if (i < m) {
            const int64_t id = cand[(int64_t)q * m + i];
            if (id >= 0) {                                    // (a negative id is padding)
                const uint64_t loc = (uint64_t)id - (uint64_t)row_base;       // the true difference when id >= row_base
                if (id < row_base || loc >= (uint64_t)n) atomicOr(&s_bad, 1);  // out of range: nothing is read for it
                else if (!mask || mask[loc]) kx = (uint32_t)loc;
            }
        }
        key[i] = kx;
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {               // bitonic network, ascending: the sentinels end up behind the rows
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (P >> 1); t += 1024) {
                const int i = ((t / stride) * (stride << 1)) + (t % stride), j = i + stride;
                const bool asc = (i & size) == 0;
                const uint32_t x = key[i], y = key[j];
                if (asc ? (x > y) : (x < y)) { key[i] = y; key[j] = x; }
            }
            __syncthreads();
        }
    }
    // first occurrences, compacted in order: thread t owns positions [t per, (t + 1) per)
    const int per = (P + 1023) / 1024;
    const int i0 = tid * per;
    uint32_t mine = 0;
    for (int i = i0; i < i0 + per && i < P; ++i) mine += (key[i] != HDB_RR_NONE && (i == 0 || key[i] != key[i - 1])) ? 1u : 0u;
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t v = __shfl_up(incl, o, 64); if (lane >= o) incl += v; }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t pos = incl - mine, total = 0;
    for (int w = 0; w < 16; ++w) { if (w < wave) pos += wsum[w]; total += wsum[w]; }
    int64_t* out = rows + (int64_t)q * m;                     // total <= m: every kept key is one of the m ids
    for (int i = i0; i < i0 + per && i < P; ++i)
        if (key[i] != HDB_RR_NONE && (i == 0 || key[i] != key[i - 1])) out[pos++] = (int64_t)key[i];
    if (tid == 0) {
        cnt[q * HDB_CNT_STRIDE] = total;
        if (status) status[q] = ((qnan[q] & 1) ? HDB_Q_NAN : 0) | (s_bad ? HDB_Q_BADROW : 0);
    }
}

extern "C" int hdb_launch_rerank_prep(const int64_t* cand, int m, int nq, int64_t n, int64_t row_base, const uint8_t* mask, const int* qnan,
                                      int64_t* rows, uint32_t* cnt, int32_t* status, void* stream) {
    if (m < 1 || m > HDB_CAND_CAP || nq < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(hdb_rerank_prep_kernel, dim3(nq), dim3(1024), 0, (hipStream_t)stream, cand, m, n, row_base, mask, qnan, rows, cnt, status);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------------
// Scoring.  ScanArgs as for the VALU scan; rows = the prepared lists [query of the chunk][m], cnt their counts, cand / cap the
// packed entries out (entry i of a query is the row at list position i).  grid = (blocks, queries of the chunk), 256 threads,
// LDS = d accumulate-type values.  A wave step takes 4 U candidates: group g the positions base + 4 u + g.
// NC > 0: rows of exactly NC 16-byte pieces, unrolled -- all U * ceil(NC / 16) loads of a group ahead of the first use;
// NC == 0: rows of whole 16-byte pieces, runtime loop; NC < 0: element loop (any d, any alignment).
// ------------------------------------------------------------------------------------------------------------------------
template <typename T, int ACC, int NC, int U>
__global__ __launch_bounds__(256) void hdb_rerank_score_kernel(ScanArgs a) {
    using Acc = typename Elem<T>::Acc;
    constexpr int EPC = Elem<T>::EPC;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Acc* qs = reinterpret_cast<Acc*>(smem);
    const int ql = blockIdx.y, q = a.q0 + ql;
    const uint32_t total = min(a.cnt[ql * HDB_CNT_STRIDE], (uint32_t)a.m);
    if ((uint32_t)blockIdx.x * 16u * U >= total) return;                        // (workgroup-uniform: nothing left of this list)
    for (int i = threadIdx.x; i < a.d; i += 256) qs[i] = reinterpret_cast<const Acc*>(a.Q)[(int64_t)q * a.d + i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, l16 = lane & 15;
    const int64_t* list = a.rows + (int64_t)ql * a.m;
    const char* Vb = reinterpret_cast<const char*>(a.V);
    const T* Vt = reinterpret_cast<const T*>(a.V);
    for (uint32_t base = ((uint32_t)blockIdx.x * 4 + wave) * 4u * U; base < total; base += gridDim.x * 16u * U) {      // (wave-uniform)
        uint32_t row[U];
        Acc acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            row[u] = (uint32_t)list[min(base + 4u * u + g, total - 1u)];        // (a position past the end re-reads the last row)
            acc[u] = Acc(0);
        }
        if constexpr (NC > 0) {
            constexpr int NJ = (NC + 15) / 16;
            uint4 raw[U][NJ];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int c = l16 + 16 * j;
                    const int cc = NC == 16 * NJ ? c : min(c, NC - 1);          // (idle lanes of a ragged step re-read the last piece)
                    raw[u][j] = *reinterpret_cast<const uint4*>(Vb + (int64_t)row[u] * a.row_bytes + (int64_t)cc * 16);
                }
            __builtin_amdgcn_sched_barrier(0);              // keep the loads ahead of every use
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int c = l16 + 16 * j;
                    const bool live = NC == 16 * NJ ? true : c < NC;
                    const int cc = NC == 16 * NJ ? c : min(c, NC - 1);
                    Acc x[EPC];
                    hdb_unpack(raw[u][j], x, (T*)nullptr);
#pragma unroll
                    for (int e = 0; e < EPC; ++e) {
                        const Acc qe = qs[cc * EPC + e];
                        if (ACC == 1) { const Acc df = live ? x[e] - qe : Acc(0); acc[u] = fma(df, df, acc[u]); }
                        else if (ACC == 2) { const Acc df = live ? x[e] - qe : Acc(0); acc[u] += df < Acc(0) ? -df : df; }
                        else acc[u] += (live ? x[e] : Acc(0)) * qe;
                    }
                }
        } else if constexpr (NC == 0) {
            const int nj = (a.nchunks + 15) >> 4;
            for (int j = 0; j < nj; ++j) {
                const int c = l16 + 16 * j;
                const bool live = c < a.nchunks;
                const int cc = live ? c : a.nchunks - 1;
                uint4 raw[U];
#pragma unroll
                for (int u = 0; u < U; ++u) raw[u] = *reinterpret_cast<const uint4*>(Vb + (int64_t)row[u] * a.row_bytes + (int64_t)cc * 16);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    Acc x[EPC];
                    hdb_unpack(raw[u], x, (T*)nullptr);
#pragma unroll
                    for (int e = 0; e < EPC; ++e) {
                        const Acc qe = qs[cc * EPC + e];
                        if (ACC == 1) { const Acc df = live ? x[e] - qe : Acc(0); acc[u] = fma(df, df, acc[u]); }
                        else if (ACC == 2) { const Acc df = live ? x[e] - qe : Acc(0); acc[u] += df < Acc(0) ? -df : df; }
                        else acc[u] += (live ? x[e] : Acc(0)) * qe;
                    }
                }
            }
        } else {
            for (int e = l16; e < a.d; e += 16) {
                const Acc qe = qs[e];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const Acc x = (Acc)hdb_to_f(Vt[(int64_t)row[u] * a.d + e]);
                    if (ACC == 1) { const Acc df = x - qe; acc[u] = fma(df, df, acc[u]); }
                    else if (ACC == 2) { const Acc df = x - qe; acc[u] += df < Acc(0) ? -df : df; }
                    else acc[u] += x * qe;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t i = base + 4u * u + g;
            const Acc sum = hdb_rows4_sum(acc[u], acc[u], acc[u], acc[u], l16);
            if (i < total && (l16 & 3) == 0 && hdb_owned_row(l16) == (int)(row[u] & 3u)) {
                const uint32_t r = row[u];
                float s;                                      // hdb_emit's epilogue
                if (a.metric == HDB_EUCLIDEAN) {
                    s = (float)(Acc(1) / (Acc(1) + sqrt(sum)));
                } else if (a.metric == HDB_MANHATTAN) {
                    s = (float)(Acc(1) / (Acc(1) + sum));
                } else if (a.metric == HDB_COSINE) {
                    s = (float)sum * a.inv_norm[r] * a.qinv[q];
                } else {
                    s = (float)sum;
                }
                if (a.bias) s += a.bias[r];
                s = hdb_canon(s);
                a.cand[(int64_t)ql * a.cap + i] = hdb_pack(s, r);
            }
        }
    }
}

// one workgroup iteration covers 16 U list positions; blocks along x: the positions of the longest possible list, at most `cap`
template <typename T, int ACC, int NC, int U>
static void rerank_launch(const ScanArgs& a, int nq_launch, hipStream_t st) {
    using Acc = typename Elem<T>::Acc;
    const int cap = std::max(4, 2048 / std::max(nq_launch, 1));
    const dim3 grid(hdb_grid_for(a.m, 16 * U, cap), nq_launch);
    hipLaunchKernelGGL((hdb_rerank_score_kernel<T, ACC, NC, U>), grid, dim3(256), (size_t)a.d * sizeof(Acc), st, a);
}
template <typename T, int ACC>
static void rerank_launch_acc(const ScanArgs& a, bool vec, int nq_launch, hipStream_t st) {
    if (!vec) { rerank_launch<T, ACC, -1, 2>(a, nq_launch, st); return; }
    switch (a.nchunks) {                                      // 256 / 384 / 512 / 768 / 1536-byte rows: 6-8 loads per lane in flight
    case 16: rerank_launch<T, ACC, 16, 4>(a, nq_launch, st); return;
    case 24: rerank_launch<T, ACC, 24, 4>(a, nq_launch, st); return;
    case 32: rerank_launch<T, ACC, 32, 4>(a, nq_launch, st); return;
    case 48: rerank_launch<T, ACC, 48, 2>(a, nq_launch, st); return;
    case 96: rerank_launch<T, ACC, 96, 1>(a, nq_launch, st); return;
    default: rerank_launch<T, ACC, 0, 2>(a, nq_launch, st); return;
    }
}
template <typename T>
static void rerank_launch_t(const ScanArgs& a, bool vec, int nq_launch, hipStream_t st) {
    if (a.metric == HDB_EUCLIDEAN) rerank_launch_acc<T, 1>(a, vec, nq_launch, st);
    else if (a.metric == HDB_MANHATTAN) rerank_launch_acc<T, 2>(a, vec, nq_launch, st);
    else rerank_launch_acc<T, 0>(a, vec, nq_launch, st);
}

extern "C" int hdb_launch_rerank_score(const ScanArgs* args, int dtype, int nq_launch, void* stream) {
    ScanArgs a = *args;
    hipStream_t st = (hipStream_t)stream;
    if (!a.rows || a.m < 1 || a.m > (int64_t)a.cap || nq_launch < 1) return (int)hipErrorInvalidValue;
    if (a.metric != HDB_DOT && a.metric != HDB_COSINE && a.metric != HDB_EUCLIDEAN && a.metric != HDB_MANHATTAN) return (int)hipErrorInvalidValue;
    const int elem = hdb_elem_bytes(dtype);
    if (elem == 0) return (int)hipErrorInvalidValue;          // (packed bits have no byte-addressed elements)
    a.row_bytes = (int32_t)hdb_row_bytes(dtype, a.d);
    a.nchunks = a.row_bytes / 16;
    // the scan's own rule for its 16-byte flavour (hdb_launch_scan)
    const bool vec = (a.row_bytes % 16 == 0) && ((reinterpret_cast<uintptr_t>(a.V) & 15) == 0) && ((size_t)a.d * (elem == 8 ? 8 : 4) <= 60 * 1024);
    if (dtype == HDB_F16) rerank_launch_t<__half>(a, vec, nq_launch, st);
    else if (dtype == HDB_F32) rerank_launch_t<float>(a, vec, nq_launch, st);
    else if (dtype == HDB_BF16) rerank_launch_t<hdb_bf16>(a, vec, nq_launch, st);
    else if (dtype == HDB_F8E4M3) rerank_launch_t<hdb_f8>(a, vec, nq_launch, st);
    else if (dtype == HDB_I8) rerank_launch_t<hdb_i8>(a, vec, nq_launch, st);
    else if (dtype == HDB_F64) rerank_launch_t<double>(a, vec, nq_launch, st);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}
