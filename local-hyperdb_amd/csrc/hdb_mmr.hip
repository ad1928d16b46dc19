// hdb_mmr.hip -- diverse top-k: maximal marginal relevance over a call's candidates (hdb_mmr, hdb_mmr_host; include/hyperdb_hip.h)
// for gfx950.
//
// Every other scoring kernel scores rows against queries.  Here the rows of ONE query's candidate list are scored against each
// other, and k of them are picked one after the other: a pick is paid for its relevance and charged for its similarity to the
// closest pick before it.  Three launches per chunk of queries, separate on purpose -- the kernel boundary is what makes the pair
// matrix of one launch visible to the next on every XCD; nothing waits on a flag:
//
//   hdb_mmr_prep_kernel    one workgroup per query: the list [m <= 2048] -> its candidates.  Padding (id < 0, score -inf) is dropped,
//                          an id outside [row_base, row_base + n) is dropped and flagged (HDB_Q_BADROW) -- compared against the
//                          bounds before anything is indexed with it --, a repeat is dropped: keys (local row, list position) are
//                          sorted in LDS and a key that opens a run marks its position (hdb_first_occ.h, the routine of
//                          hdb_group_collapse_kernel).  The survivors are compacted IN LIST ORDER into rows[mp] / rel[mp] with their
//                          count and the status word; mp = m rounded up to the pair tile.
//   hdb_mmr_pairs_kernel   grid = (tile pairs ti <= tj, queries of the chunk), 256 threads, one pair of candidates per thread.  A
//                          16-lane group gathers one candidate row of each tile in 16-byte pieces (rows that are not whole pieces: an
//                          element loop), widened through hdb_unpack.h into LDS, a slice of 256 row bytes at a time; the LDS pitch
//                          is the slice plus 16 bytes, so the 16 rows a ds_read_b128 lane group reads at one element index lie in 16
//                          different 16-byte slots of the bank row.  A thread walks the slice in element order with explicit fma.
//                          Diagonal tiles compute i < j only.  P[mp][mp] float32 gets the value twice, mirrored, so the selection
//                          reads contiguous rows.  Workgroups past the query's count leave at once.  No atomics.
//   hdb_mmr_select_kernel  one workgroup of 256 threads per query, min(k, count) steps.  Candidate c belongs to thread c mod 256,
//                          which keeps its relevance, its penalty and its selected flag in registers (8 candidates at most).  A
//                          step: val, the argmax of the 64-bit key (ordered value bits, inverted position) by wave shuffles and one
//                          LDS exchange between the four waves, then the winner's row of P -- one coalesced load -- raises the
//                          penalties by max, and one output slot is written.  The loop is bounded by k.
//
// The pair value p(a, b) depends on the two rows only: products (or squared differences) accumulated in element order e = 0 .. d - 1
// in the accumulate type (float32; double for a float64 index), the scan's epilogue without bias (hdb_emit), NaN -> -inf.  Cosine
// multiplies by the cached 1/||v|| of the LOWER row first, so the value does not depend on which of the two stands first in a list.
#include "hdb_common.h"
#include "hdb_unpack.h"
#include "hdb_first_occ.h"
#include "../../include/hyperdb_hip.h"
#include <algorithm>

#define HDB_MMR_MAXM 2048

// ------------------------------------------------------------------------------------------------------------------------
// List preparation.  idx / score: [nq][m]; rows / rel: [nq][mp]; cnt: [nq].  LDS: the keys (16 KiB) and the marks (2 KiB).
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void hdb_mmr_prep_kernel(const int64_t* idx, const float* score, int m, int mp, int64_t n, int64_t row_base,
                                                            uint32_t* rows, float* rel, int32_t* cnt, const int32_t* status_in,
                                                            int32_t* status_out) {
    __shared__ unsigned long long key[HDB_MMR_MAXM];
    __shared__ uint8_t first[HDB_MMR_MAXM];
    __shared__ uint32_t wsum[16];
    __shared__ int s_bad;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_bad = 0;
    int P = 64;
    while (P < m) P <<= 1;                                    // m <= HDB_MMR_MAXM, so P <= HDB_MMR_MAXM
    __syncthreads();
    const int64_t* my_idx = idx + (int64_t)q * m;
    const float* my_score = score + (int64_t)q * m;
    for (int i = tid; i < P; i += 1024) {
        unsigned long long kx = HDB_FIRST_NONE;
        if (i < m) {
            const int64_t id = my_idx[i];
            if (id >= 0 && my_score[i] != -INFINITY) {        // (a negative id and an entry at -inf are padding)
                const uint64_t loc = (uint64_t)id - (uint64_t)row_base;       // the true difference when id >= row_base
                if (id < row_base || loc >= (uint64_t)n) atomicOr(&s_bad, 1);  // out of range: nothing is read for it
                else kx = ((unsigned long long)(uint32_t)loc << 32) | (unsigned long long)(uint32_t)i;
            }
        }
        key[i] = kx;
        first[i] = 0;
    }
    __syncthreads();
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
    uint32_t* out_r = rows + (int64_t)q * mp;                 // total <= m <= mp: every mark is one of the m positions
    float* out_s = rel + (int64_t)q * mp;
    for (int i = i0; i < i0 + per && i < P; ++i)
        if (first[i]) {
            out_r[pos] = (uint32_t)((uint64_t)my_idx[i] - (uint64_t)row_base);
            out_s[pos] = my_score[i];
            ++pos;
        }
    if (tid == 0) {
        cnt[q] = (int32_t)total;
        if (status_out) status_out[q] = (status_in ? (status_in[q] & HDB_Q_NAN) : 0) | (s_bad ? HDB_Q_BADROW : 0);
    }
}

extern "C" int hdb_launch_mmr_prep(const int64_t* idx, const float* score, int nq, int m, int mp, int64_t n, int64_t row_base, uint32_t* rows,
                                   float* rel, int32_t* cnt, const int32_t* status_in, int32_t* status_out, void* stream) {
    if (m < 1 || m > HDB_MMR_MAXM || mp != hdb_mmr_mp(m) || nq < 1 || n < 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(hdb_mmr_prep_kernel, dim3(nq), dim3(1024), 0, (hipStream_t)stream, idx, score, m, mp, n, row_base, rows, rel, cnt,
                       status_in, status_out);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------------
// Pairs.  ACC 0: products, 1: squared differences.  VEC: rows of whole 16-byte pieces at a 16-byte aligned base.
// A slice is 16 pieces = 16 EPC elements; a b128 LDS access moves VW accumulate-type values.
// ------------------------------------------------------------------------------------------------------------------------
template <typename Acc> struct alignas(16) MmrVec { Acc v[16 / sizeof(Acc)]; };

template <typename T, int ACC, bool VEC>
__global__ __launch_bounds__(HDB_MMR_TILE * HDB_MMR_TILE) void hdb_mmr_pairs_kernel(const void* V, int d, int64_t row_bytes, int metric,
                                                                                   const float* inv_norm, const uint32_t* rows,
                                                                                   const int32_t* cnt, int mp, float* P) {
    using Acc = typename Elem<T>::Acc;
    using Vec = MmrVec<Acc>;
    constexpr int EPC = Elem<T>::EPC, SLICE = 16 * EPC, VW = 16 / (int)sizeof(Acc), PITCH = SLICE + VW;
    static_assert(HDB_MMR_TILE == 16, "a 16-lane group gathers one row of a tile");
    __shared__ __attribute__((aligned(16))) Acc sA[HDB_MMR_TILE * PITCH];
    __shared__ __attribute__((aligned(16))) Acc sB[HDB_MMR_TILE * PITCH];
    const int q = blockIdx.y, tid = threadIdx.x;
    const int count = cnt[q];
    // blockIdx.x = tj (tj + 1) / 2 + ti, ti <= tj
    const int t = blockIdx.x;
    int tj = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while ((tj + 1) * (tj + 2) / 2 <= t) ++tj;
    while (tj * (tj + 1) / 2 > t) --tj;
    const int ti = t - tj * (tj + 1) / 2;
    if (tj * HDB_MMR_TILE >= count) return;                   // (workgroup-uniform; ti <= tj: nothing of this tile pair exists)
    const bool diag = ti == tj;
    const uint32_t* list = rows + (int64_t)q * mp;
    const int g = tid >> 4, l16 = tid & 15;
    // what this 16-lane group gathers: candidate g of each tile (past the count: the last candidate again, never written out)
    const uint32_t ga = list[min(ti * HDB_MMR_TILE + g, count - 1)], gb = list[min(tj * HDB_MMR_TILE + g, count - 1)];
    // what this thread computes: the pair (ci, cj)
    const int ci = ti * HDB_MMR_TILE + g, cj = tj * HDB_MMR_TILE + l16;
    const bool active = ci < count && cj < count && (!diag || ci < cj);
    const Acc* pa = sA + g * PITCH;
    const Acc* pb = (diag ? sA : sB) + l16 * PITCH;
    const char* Vb = reinterpret_cast<const char*>(V);
    const T* Vt = reinterpret_cast<const T*>(V);
    const int nchunks = (int)(row_bytes >> 4);
    Acc acc = Acc(0);
    for (int s0 = 0; s0 < d; s0 += SLICE) {
        if (s0) __syncthreads();                              // the slice before this one has been read
        if constexpr (VEC) {
            const int c = s0 / EPC + l16;
            if (c < nchunks) {                                // (a piece past the row's end is never read below: ne stops before it)
                Acc x[EPC];
                hdb_unpack(*reinterpret_cast<const uint4*>(Vb + (int64_t)ga * row_bytes + (int64_t)c * 16), x, (T*)nullptr);
#pragma unroll
                for (int e = 0; e < EPC; e += VW) {
                    Vec v;
#pragma unroll
                    for (int w = 0; w < VW; ++w) v.v[w] = x[e + w];
                    *reinterpret_cast<Vec*>(sA + g * PITCH + l16 * EPC + e) = v;
                }
                if (!diag) {
                    hdb_unpack(*reinterpret_cast<const uint4*>(Vb + (int64_t)gb * row_bytes + (int64_t)c * 16), x, (T*)nullptr);
#pragma unroll
                    for (int e = 0; e < EPC; e += VW) {
                        Vec v;
#pragma unroll
                        for (int w = 0; w < VW; ++w) v.v[w] = x[e + w];
                        *reinterpret_cast<Vec*>(sB + g * PITCH + l16 * EPC + e) = v;
                    }
                }
            }
        } else {
            for (int e = l16; e < SLICE; e += 16) {           // (elements past d: zero, a term that changes no sum)
                const bool in = s0 + e < d;
                sA[g * PITCH + e] = in ? (Acc)hdb_to_f(Vt[(int64_t)ga * d + s0 + e]) : Acc(0);
                if (!diag) sB[g * PITCH + e] = in ? (Acc)hdb_to_f(Vt[(int64_t)gb * d + s0 + e]) : Acc(0);
            }
        }
        __syncthreads();
        const int ne = (min(SLICE, d - s0) + VW - 1) / VW * VW;
        if (active) {
            for (int e = 0; e < ne; e += VW) {
                const Vec a = *reinterpret_cast<const Vec*>(pa + e), b = *reinterpret_cast<const Vec*>(pb + e);
#pragma unroll
                for (int w = 0; w < VW; ++w) {
                    if (ACC == 1) { const Acc df = a.v[w] - b.v[w]; acc = fma(df, df, acc); }
                    else acc = fma(a.v[w], b.v[w], acc);
                }
            }
        }
    }
    if (!active) return;
    const uint32_t ra = list[ci], rb = list[cj];
    float s;                                                  // hdb_emit's epilogue, without bias
    if (metric == HDB_EUCLIDEAN) s = (float)(Acc(1) / (Acc(1) + sqrt(acc)));
    else if (metric == HDB_COSINE) s = (float)acc * inv_norm[min(ra, rb)] * inv_norm[max(ra, rb)];
    else s = (float)acc;
    s = hdb_canon(s);
    float* Pq = P + (int64_t)q * mp * mp;
    Pq[(int64_t)ci * mp + cj] = s;
    Pq[(int64_t)cj * mp + ci] = s;
}

template <typename T>
static void mmr_pairs_launch(const void* V, int d, int64_t row_bytes, int metric, const float* inv_norm, const uint32_t* rows, const int32_t* cnt,
                             int nq, int mp, float* P, hipStream_t st) {
    const int tiles = mp / HDB_MMR_TILE;
    const dim3 grid(tiles * (tiles + 1) / 2, nq), block(HDB_MMR_TILE * HDB_MMR_TILE);
    const bool vec = (row_bytes % 16 == 0) && ((reinterpret_cast<uintptr_t>(V) & 15) == 0);
    const bool sq = metric == HDB_EUCLIDEAN;
    if (vec && sq) hipLaunchKernelGGL((hdb_mmr_pairs_kernel<T, 1, true>), grid, block, 0, st, V, d, row_bytes, metric, inv_norm, rows, cnt, mp, P);
    else if (vec) hipLaunchKernelGGL((hdb_mmr_pairs_kernel<T, 0, true>), grid, block, 0, st, V, d, row_bytes, metric, inv_norm, rows, cnt, mp, P);
    else if (sq) hipLaunchKernelGGL((hdb_mmr_pairs_kernel<T, 1, false>), grid, block, 0, st, V, d, row_bytes, metric, inv_norm, rows, cnt, mp, P);
    else hipLaunchKernelGGL((hdb_mmr_pairs_kernel<T, 0, false>), grid, block, 0, st, V, d, row_bytes, metric, inv_norm, rows, cnt, mp, P);
}

extern "C" int hdb_launch_mmr_pairs(const void* V, int dtype, int d, int pair_metric, const float* inv_norm, const uint32_t* rows,
                                    const int32_t* cnt, int nq, int mp, float* P, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!V || d < 1 || nq < 1 || nq > 65535 || mp < HDB_MMR_TILE || mp > HDB_MMR_MAXM || mp % HDB_MMR_TILE != 0) return (int)hipErrorInvalidValue;
    if (pair_metric != HDB_DOT && pair_metric != HDB_COSINE && pair_metric != HDB_EUCLIDEAN) return (int)hipErrorInvalidValue;
    if (pair_metric == HDB_COSINE && !inv_norm) return (int)hipErrorInvalidValue;
    if (hdb_elem_bytes(dtype) == 0) return (int)hipErrorInvalidValue;      // (packed bits have no byte-addressed elements)
    const int64_t row_bytes = hdb_row_bytes(dtype, d);
    if (dtype == HDB_F16) mmr_pairs_launch<__half>(V, d, row_bytes, pair_metric, inv_norm, rows, cnt, nq, mp, P, st);
    else if (dtype == HDB_F32) mmr_pairs_launch<float>(V, d, row_bytes, pair_metric, inv_norm, rows, cnt, nq, mp, P, st);
    else if (dtype == HDB_BF16) mmr_pairs_launch<hdb_bf16>(V, d, row_bytes, pair_metric, inv_norm, rows, cnt, nq, mp, P, st);
    else if (dtype == HDB_F8E4M3) mmr_pairs_launch<hdb_f8>(V, d, row_bytes, pair_metric, inv_norm, rows, cnt, nq, mp, P, st);
    else if (dtype == HDB_I8) mmr_pairs_launch<hdb_i8>(V, d, row_bytes, pair_metric, inv_norm, rows, cnt, nq, mp, P, st);
    else if (dtype == HDB_F64) mmr_pairs_launch<double>(V, d, row_bytes, pair_metric, inv_norm, rows, cnt, nq, mp, P, st);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------------
// Selection.  val = canon(lam * r - oml * pen): two rounded products and one rounded subtraction, never contracted into an fma.
// ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float hdb_mmr_val(float lam, float r, float oml, float pen) {
#pragma clang fp contract(off)
    const float a = lam * r;
    const float b = oml * pen;
    return hdb_canon(a - b);
}

__global__ __launch_bounds__(HDB_MMR_SELECT_THREADS) void hdb_mmr_select_kernel(const uint32_t* rows, const float* rel, const int32_t* cnt, int mp,
                                                                                const float* P, float lam, float oml, uint32_t k,
                                                                                int64_t row_base, int64_t* idx_out, float* score_out) {
    constexpr int NT = HDB_MMR_SELECT_THREADS, CPT = HDB_MMR_MAXM / NT, NW = NT / 64;
    __shared__ unsigned long long s_key[2][NW];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int count = min(cnt[q], mp);
    const uint32_t steps = min(k, (uint32_t)count);
    const uint32_t* list = rows + (int64_t)q * mp;
    const float* my_rel = rel + (int64_t)q * mp;
    const float* Pq = P + (int64_t)q * mp * mp;
    int64_t* out_i = idx_out + (int64_t)q * k;
    float* out_s = score_out + (int64_t)q * k;
    float r[CPT], pen[CPT];
    uint32_t open = 0;                                        // bit u: candidate tid + NT u exists and has not been picked
#pragma unroll
    for (int u = 0; u < CPT; ++u) {
        const int c = tid + NT * u;
        r[u] = -INFINITY; pen[u] = -INFINITY;
        if (c < count) { r[u] = hdb_canon(my_rel[c]); open |= 1u << u; }
    }
    uint32_t t = 0;
    for (; t < steps; ++t) {
        unsigned long long best = 0ull;                       // below every key: hdb_pack(-inf, .) > 0
#pragma unroll
        for (int u = 0; u < CPT; ++u)
            if (open & (1u << u)) {
                const float val = t == 0 ? r[u] : hdb_mmr_val(lam, r[u], oml, pen[u]);
                const unsigned long long kx = hdb_pack(val, (uint32_t)(tid + NT * u));      // highest value, lowest position
                best = kx > best ? kx : best;
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const unsigned long long v = __shfl_xor(best, o, 64); best = v > best ? v : best; }
        if (lane == 0) s_key[t & 1][wave] = best;
        __syncthreads();                                      // (one barrier per step: the two key rows alternate)
#pragma unroll
        for (int w = 0; w < NW; ++w) { const unsigned long long v = s_key[t & 1][w]; best = v > best ? v : best; }
        if (best == 0ull) break;                              // (never: steps <= count candidates are open; uniform)
        const uint32_t s = 0xFFFFFFFFu - (uint32_t)best;      // the winner's position among the candidates, < count
        if ((int)(s & (NT - 1)) == tid) {
            open &= ~(1u << (s / NT));
            out_i[t] = (int64_t)list[s] + row_base;
            out_s[t] = hdb_canon(my_rel[s]);
        }
        const float* prow = Pq + (int64_t)s * mp;
#pragma unroll
        for (int u = 0; u < CPT; ++u)
            if (open & (1u << u)) pen[u] = fmaxf(pen[u], prow[tid + NT * u]);
    }
    for (uint32_t i = t + tid; i < k; i += NT) { out_i[i] = -1; out_s[i] = -INFINITY; }
}

extern "C" int hdb_launch_mmr_select(const uint32_t* rows, const float* rel, const int32_t* cnt, int nq, int mp, const float* P, float lam,
                                     int k, int64_t row_base, int64_t* idx_out, float* score_out, void* stream) {
    if (nq < 1 || mp < HDB_MMR_TILE || mp > HDB_MMR_MAXM || mp % HDB_MMR_TILE != 0 || k < 1 || k > mp || !(lam >= 0.0f && lam <= 1.0f))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(hdb_mmr_select_kernel, dim3(nq), dim3(HDB_MMR_SELECT_THREADS), 0, (hipStream_t)stream, rows, rel, cnt, mp, P, lam,
                       1.0f - lam, (uint32_t)k, row_base, idx_out, score_out);
    return (int)hipGetLastError();
}
