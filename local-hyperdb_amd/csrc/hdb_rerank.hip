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
// epilogue (hdb_sum_score, hdb_emit.h).  It is the only kernel that scores listed rows on this contract, and it has two callers:
// hdb_rerank (rerank_impl, hdb_api.hip) with the prepared lists -- the six byte-addressed dtypes, manhattan, and pearson as cosine
// on centred queries with the row scale 1/(sd d) in the place of 1/||v|| --, and the explicit int8 shadow (quant_topk, hdb_api.hip),
// whose filter pass left packed entries: the kernel then takes each row from its entry and rewrites the entry in place (float16,
// bfloat16 and float32 rows; dot, cosine, euclidean).  Nothing depends on the position of a row in the list or on the other candidates.
// The squared differences are accumulated with explicit fma, element by element in order.  Written as acc += df * df, the first two
// squares of an unrolled chain are a sum of two products, and the compiler is free to fuse either one: it rounded the SECOND square
// and fused the first, where the scan's kernels fuse in element order -- one float32 step apart on 1-2 % of the rows (measured
// against the masked exact call, 20 001 Gaussian rows).  The explicit form is the scan's chain whatever the unrolling.
#include "hdb_common.h"
#include "hdb_unpack.h"
#include "hdb_emit.h"        // hdb_sum_score
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
// Scoring.  ScanArgs as for the VALU scan; cnt the lists' counts, cand / cap the packed entries out.  The rows come from
//   ENT false: rows = the prepared lists [query of the chunk][m]: entry i of a query is the row at list position i;
//   ENT true:  the entries themselves, as a filter pass left them (row of entry i = 0xFFFFFFFF - its low word), min(cnt, cap) of
//              them; entry i is rewritten in place.
// grid = (blocks, queries of the chunk), 256 threads, LDS = d accumulate-type values.  A wave step takes 4 U candidates: group g
// the positions base + 4 u + g.
// NC > 0: rows of exactly NC 16-byte pieces, unrolled -- all U * ceil(NC / 16) loads of a group ahead of the first use;
// NC == 0: rows of whole 16-byte pieces, runtime loop; NC < 0: element loop (any d, any alignment).
// ------------------------------------------------------------------------------------------------------------------------
// one element's term: ACC 0 the product, 1 the squared difference (explicit fma, see above), 2 the absolute difference; a dead
// piece (live == false) adds 0 * q or 0, as in hdb_scan_kernel
template <int ACC, typename Acc>
__device__ __forceinline__ void hdb_gather_acc(Acc& acc, bool live, Acc x, Acc qe) {
    if (ACC == 1) { const Acc df = live ? x - qe : Acc(0); acc = fma(df, df, acc); }
    else if (ACC == 2) { const Acc df = live ? x - qe : Acc(0); acc += df < Acc(0) ? -df : df; }
    else acc += (live ? x : Acc(0)) * qe;
}

template <typename T, int ACC, int NC, int U, bool ENT>
__global__ __launch_bounds__(256) void hdb_rerank_score_kernel(ScanArgs a) {
    using Acc = typename Elem<T>::Acc;
    constexpr int EPC = Elem<T>::EPC;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Acc* qs = reinterpret_cast<Acc*>(smem);
    const int ql = blockIdx.y, q = a.q0 + ql;
    const uint32_t total = min(a.cnt[ql * HDB_CNT_STRIDE], ENT ? a.cap : (uint32_t)a.m);
    if ((uint32_t)blockIdx.x * 16u * U >= total) return;                        // (workgroup-uniform: nothing left of this list)
    for (int i = threadIdx.x; i < a.d; i += 256) qs[i] = reinterpret_cast<const Acc*>(a.Q)[(int64_t)q * a.d + i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, l16 = lane & 15;
    const int64_t* list = ENT ? nullptr : a.rows + (int64_t)ql * a.m;      // (ENT: there is no list, a.rows is null)
    unsigned long long* ent = a.cand + (int64_t)ql * a.cap;
    const char* Vb = reinterpret_cast<const char*>(a.V);
    const T* Vt = reinterpret_cast<const T*>(a.V);
    for (uint32_t base = ((uint32_t)blockIdx.x * 4 + wave) * 4u * U; base < total; base += gridDim.x * 16u * U) {      // (wave-uniform)
        uint32_t row[U];
        Acc acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            // A position past the end re-reads the last one.  ENT: the group that owns that entry may be storing it at this moment.
            // That is sound because a rewrite never changes an entry's low word -- the row -- and is one aligned 64-bit store:
            // the 32-bit load below sees the same word before, during and after it.  Nothing else of an entry is read here.
            const uint32_t pos = min(base + 4u * u + g, total - 1u);
            if constexpr (ENT) row[u] = 0xFFFFFFFFu - reinterpret_cast<const uint32_t*>(ent + pos)[0];
            else row[u] = (uint32_t)list[pos];
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
                    for (int e = 0; e < EPC; ++e) hdb_gather_acc<ACC>(acc[u], live, x[e], qs[cc * EPC + e]);
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
                    for (int e = 0; e < EPC; ++e) hdb_gather_acc<ACC>(acc[u], live, x[e], qs[cc * EPC + e]);
                }
            }
        } else {
            for (int e = l16; e < a.d; e += 16) {
                const Acc qe = qs[e];
#pragma unroll
                for (int u = 0; u < U; ++u) hdb_gather_acc<ACC>(acc[u], true, (Acc)hdb_to_f(Vt[(int64_t)row[u] * a.d + e]), qe);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t i = base + 4u * u + g;
            const Acc sum = hdb_rows4_sum(acc[u], acc[u], acc[u], acc[u], l16);
            if (i < total && (l16 & 3) == 0 && hdb_owned_row(l16) == (int)(row[u] & 3u)) {
                const uint32_t r = row[u];
                float s = hdb_sum_score(a.metric, sum, a.inv_norm, r, a.qinv, q);      // the rest as hdb_emit finishes a score
                if (a.bias) s += a.bias[r];
                if (a.mask && !a.mask[r]) s = -INFINITY;    // (per-query lists come without masked rows; a filter pass keeps them)
                ent[i] = hdb_pack(hdb_canon(s), r);
            }
        }
    }
}

// The entry source is built for what the int8 shadow serves: float16, bfloat16 and float32 rows, products and squared differences.
template <typename T, int ACC>
constexpr bool hdb_gather_ent_built = ACC != 2 && (std::is_same_v<T, __half> || std::is_same_v<T, hdb_bf16> || std::is_same_v<T, float>);

// one workgroup iteration covers 16 U positions; blocks along x: the positions of the longest possible list, at most `cap`.
// The query sits in LDS for both row sources, d accumulate-type values: hdb_index_create admits d <= 7680, i.e. 30 KiB of float32
// (60 KiB of float64) -- inside the 64 KiB a launch gets without an attribute, the bound of hdb_scan_generic_kernel's launch as well.
template <typename T, int ACC, int NC, int U, bool ENT>
static void rerank_launch(const ScanArgs& a, int nq_launch, hipStream_t st) {
    using Acc = typename Elem<T>::Acc;
    const int cap = std::max(4, 2048 / std::max(nq_launch, 1));
    const dim3 grid(hdb_grid_for(ENT ? (int64_t)a.cap : a.m, 16 * U, cap), nq_launch);
    hipLaunchKernelGGL((hdb_rerank_score_kernel<T, ACC, NC, U, ENT>), grid, dim3(256), (size_t)a.d * sizeof(Acc), st, a);
}
template <typename T, int ACC, bool ENT>
static bool rerank_launch_acc(const ScanArgs& a, bool vec, int nq_launch, hipStream_t st) {
    if constexpr (ENT && !hdb_gather_ent_built<T, ACC>) return false;
    else if (!vec) rerank_launch<T, ACC, -1, 2, ENT>(a, nq_launch, st);
    else switch (a.nchunks) {                                 // 256 / 384 / 512 / 768 / 1536-byte rows: 6-8 loads per lane in flight
    // (256-byte rows from entries: one candidate per group and step.  A one-query shadow call leaves ~2 000 entries -- 33 workgroups
    //  at U = 4, 131 at U = 1 -- and measured 1.5 us slower per call at U = 4: bf16 2M x 128, profiles/gather_scorer_time.txt)
    case 16: rerank_launch<T, ACC, 16, ENT ? 1 : 4, ENT>(a, nq_launch, st); break;
    case 24: rerank_launch<T, ACC, 24, 4, ENT>(a, nq_launch, st); break;
    case 32: rerank_launch<T, ACC, 32, 4, ENT>(a, nq_launch, st); break;
    case 48: rerank_launch<T, ACC, 48, 2, ENT>(a, nq_launch, st); break;
    case 96: rerank_launch<T, ACC, 96, 1, ENT>(a, nq_launch, st); break;
    default: rerank_launch<T, ACC, 0, 2, ENT>(a, nq_launch, st); break;
    }
    return true;
}
template <typename T, bool ENT>
static bool rerank_launch_t(const ScanArgs& a, bool vec, int nq_launch, hipStream_t st) {
    if (a.metric == HDB_EUCLIDEAN) return rerank_launch_acc<T, 1, ENT>(a, vec, nq_launch, st);
    if (a.metric == HDB_MANHATTAN) return rerank_launch_acc<T, 2, ENT>(a, vec, nq_launch, st);
    return rerank_launch_acc<T, 0, ENT>(a, vec, nq_launch, st);
}

// a.rows set: per-query lists of a.m positions (hdb_rerank); a.rows null: the entries a filter pass left in a.cand (the int8 shadow)
extern "C" int hdb_launch_rerank_score(const ScanArgs* args, int dtype, int nq_launch, void* stream) {
    ScanArgs a = *args;
    hipStream_t st = (hipStream_t)stream;
    if (!a.cand || !a.cnt || a.cap < 1 || nq_launch < 1 || (a.rows && (a.m < 1 || a.m > (int64_t)a.cap))) return (int)hipErrorInvalidValue;
    if (a.metric != HDB_DOT && a.metric != HDB_COSINE && a.metric != HDB_EUCLIDEAN && a.metric != HDB_MANHATTAN) return (int)hipErrorInvalidValue;
    a.row_bytes = (int32_t)hdb_row_bytes(dtype, a.d);
    a.nchunks = a.row_bytes / 16;
    const bool vec = hdb_scan_rows_in_pieces(a.row_bytes, a.V, a.d, hdb_elem_bytes(dtype));
    bool built = false;
    const bool known = hdb_with_elem(dtype, [&](auto* tag) {      // (packed bits have no byte-addressed elements)
        using T = hdb_elem_of<decltype(tag)>;
        built = a.rows ? rerank_launch_t<T, false>(a, vec, nq_launch, st) : rerank_launch_t<T, true>(a, vec, nq_launch, st);
    });
    return known && built ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}
