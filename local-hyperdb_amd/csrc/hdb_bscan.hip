// hdb_bscan.hip -- float32 queries against packed-bit rows (HDB_B1) for gfx950: dot / cosine / pearson / euclidean / manhattan.
//
// The matrix is the 0/1 matrix the bits stand for (element e of a row = bit e & 31 of word e >> 5), so a row's raw sum is
//     sum_e (b_e ? A_e : B_e)       with the two per-element terms of the query
//     dot, cosine, pearson (the centred query):  A = 1 * q,      B = 0 * q
//     euclidean, euclidean distance:             A = (1 - q)^2,  B = (0 - q)^2
//     manhattan:                                 A = |1 - q|,    B = |0 - q|
// -- the terms themselves, never ||q||^2 + pop - 2 q.b: a query close to a stored row cancels there to hundreds of 1e-5 bands.
//
// One thread per row; work items are the 16 rows of each 16-row tile, so the strided tile sample of the float scans is available
// (ScanArgs::tile_stride) and a sampled score lands where hdb_scan_kernel puts it.  A thread reads its row front to back in 16-byte
// pieces (4-byte pieces where a row is no multiple of 16 bytes or V is not 16-byte aligned), eight pieces in flight at a time.
//
// Queries live in LDS as nibble tables: T[j][m][q], j < d / 4, m < 16, q < QT, = ((x0 + x1) + x2) + x3 with x_i = bit i of m ? A : B
// of element 4 j + i of query q.  The QT queries of a pass are interleaved, so ONE read (ds_read_b32 / b64 / b128 for 1 / 2 / 4
// queries) serves them all: a row costs d / 4 reads whatever QT is, and d / 4 adds per query.  All lanes of a wave are at the same
// j at the same time, so a wave-level read touches one line of 64 x QT bytes: sixteen distinct entries over distinct banks and
// same-address broadcasts.
//
// ONE summation order per row, whatever the mode, the grid and the number of queries of the pass: nibble sums as above, even
// nibbles into one accumulator and odd nibbles into another, in element order, the two added at the end.  The fallback for rows
// whose tables do not fit (hdb_bscan_qt == 0: d > 3840) keeps {A, B} of every element in LDS and forms the same nibble sums in
// registers, so it follows the same order.
#include "hdb_common.h"
#include "hdb_emit.h"
#include "../../include/hyperdb_hip.h"

// the two terms of element e for bit = 1 (A) and bit = 0 (B); acc as in hdb_scan.hip: 0 dot, 1 squared difference, 2 absolute
// difference (a run-time value: only the prologue reads it, the pass over the rows is the same code for every metric)
__device__ __forceinline__ void hdb_b1_terms(int acc, float q, float& A, float& B) {
    if (acc == 1) { const float da = 1.f - q, db = 0.f - q; A = da * da; B = db * db; }
    else if (acc == 2) { A = fabsf(1.f - q); B = fabsf(0.f - q); }
    else { A = 1.f * q; B = 0.f * q; }          // (0 * q: a NaN or infinite query element reaches every row, as in the reference's product)
}

// QT > 0: nibble tables of QT queries; QT == 0: the fallback, one query.  VEC: 16-byte row pieces.
template <int QT, int MODE, bool VEC>
__global__ __launch_bounds__(256) void hdb_bscan_kernel(ScanArgs a, int nq_end, int acc) {
    constexpr int NQ = QT > 0 ? QT : 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* tab = reinterpret_cast<float*>(smem);
    __shared__ HdbStage stage;
    if (MODE == 1) hdb_stage_init(stage);

    const int d = a.d, W = d >> 5, nnib = d >> 2;
    const int qbase = a.q0 + blockIdx.y * NQ;
    const float* Q = reinterpret_cast<const float*>(a.Q);
    if constexpr (QT > 0) {
        // T[j][m][qt]: 16 d bytes per query
        for (int i = threadIdx.x; i < QT * nnib * 16; i += 256) {
            const int qt = i % QT, r = i / QT, j = r >> 4, m = r & 15;
            const float* qp = Q + (int64_t)min(qbase + qt, nq_end - 1) * d + 4 * j;
            float x[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float A, B;
                hdb_b1_terms(acc, qp[e], A, B);
                x[e] = ((m >> e) & 1) ? A : B;
            }
            tab[i] = ((x[0] + x[1]) + x[2]) + x[3];
        }
    } else {
        // {A, B} of every element: 8 d bytes
        const float* qp = Q + (int64_t)min(qbase, nq_end - 1) * d;
        for (int e = threadIdx.x; e < d; e += 256) {
            float A, B;
            hdb_b1_terms(acc, qp[e], A, B);
            tab[2 * e] = A; tab[2 * e + 1] = B;
        }
    }
    __syncthreads();

    const uint32_t* Vw = reinterpret_cast<const uint32_t*>(a.V);
    const int64_t nitems = a.ntiles * 16;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < nitems; j += (int64_t)gridDim.x * 256) {
        const int64_t row = hdb_tile_index(j >> 4, a.tile_stride) * 16 + (j & 15);
        if (row >= a.n) continue;                                          // ragged last tile: nothing is read, nothing is written
        const uint32_t* p = Vw + row * (int64_t)W;
        float acc0[NQ], acc1[NQ];
#pragma unroll
        for (int qt = 0; qt < NQ; ++qt) { acc0[qt] = 0.f; acc1[qt] = 0.f; }
        // one 32-bit word = eight nibbles, elements 32 w .. 32 w + 31
        auto word = [&](int w, uint32_t bits) {
            if constexpr (QT > 0) {
                typedef float fq_t __attribute__((ext_vector_type(QT)));
                const fq_t* t0 = reinterpret_cast<const fq_t*>(tab) + (w * 8) * 16;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const uint32_t m = (bits >> (4 * i)) & 15u;
                    const fq_t v = t0[i * 16 + m];                        // the QT queries' entries in one read
#pragma unroll
                    for (int qt = 0; qt < QT; ++qt) {
                        if (i & 1) acc1[qt] += v[qt]; else acc0[qt] += v[qt];
                    }
                }
            } else {
                const float4* ab = reinterpret_cast<const float4*>(tab) + w * 16;      // {A, B, A, B} of two elements
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float4 e01 = ab[2 * i], e23 = ab[2 * i + 1];
                    const uint32_t m = bits >> (4 * i);
                    const float x0 = (m & 1u) ? e01.x : e01.y, x1 = (m & 2u) ? e01.z : e01.w;
                    const float x2 = (m & 4u) ? e23.x : e23.y, x3 = (m & 8u) ? e23.z : e23.w;
                    const float v = ((x0 + x1) + x2) + x3;
                    if (i & 1) acc1[0] += v; else acc0[0] += v;
                }
            }
        };
        // A lane's row is read in segments of up to 128 bytes, ALL loads of a segment issued before its first use: the lanes of a wave
        // read 64 different rows, so every load instruction touches 64 cache lines, and a line's pieces must be asked for back to
        // back -- with one load per loop step each 128-byte line came from HBM once per piece (10M x 1024 bits: 8 x the bytes).
        if constexpr (VEC) {
            typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
            constexpr int NB = QT == 4 ? 4 : 8;          // pieces in flight: 64 bytes beside four queries' sums (136 -> 120 registers: four waves per SIMD), else 128
            for (int w0 = 0; w0 < W; w0 += 4 * NB) {
                u32x4 v[NB];
#pragma unroll
                for (int c = 0; c < NB; ++c)             // (W is uniform: a scalar branch per piece, nothing is loaded past the row)
                    if (w0 + 4 * c < W) v[c] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + w0 + 4 * c));      // (V is streamed once per pass)
#pragma unroll
                for (int c = 0; c < NB; ++c) {
                    const int w = w0 + 4 * c;
                    if (w < W) { word(w, v[c].x); word(w + 1, v[c].y); word(w + 2, v[c].z); word(w + 3, v[c].w); }
                }
            }
        } else {
            for (int w0 = 0; w0 < W; w0 += 8) {
                uint32_t v[8];
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (w0 + c < W) v[c] = __builtin_nontemporal_load(p + w0 + c);
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (w0 + c < W) word(w0 + c, v[c]);
            }
        }
#pragma unroll
        for (int qt = 0; qt < NQ; ++qt) {
            const int q = qbase + qt;
            if (q < nq_end) hdb_emit<MODE>(a, q, row, j, acc0[qt] + acc1[qt], MODE == 1 ? &stage : nullptr, qt);
        }
    }
    if (MODE == 1) hdb_stage_flush(a, stage, (int)blockIdx.y * NQ, min(NQ, nq_end - qbase));
}

template <int QT, int MODE, bool VEC>
static int bscan_launch(const ScanArgs& a, int nq_launch, int blocks, hipStream_t st) {
    constexpr int NQ = QT > 0 ? QT : 1;
    auto kern = hdb_bscan_kernel<QT, MODE, VEC>;
    const int lds = hdb_bscan_lds_bytes(a.d, QT);
    const int acc = (a.metric == HDB_EUCLIDEAN || a.metric == HDB_EUCLIDEAN_DIST) ? 1 : (a.metric == HDB_MANHATTAN ? 2 : 0);
    static unsigned long long attr_done = 0;
    // (set once per device and instantiation: the most any width asks for, not this call's)
    const hipError_t e = hdb_lds_attr_once(reinterpret_cast<const void*>(kern), HDB_BSCAN_TABLE_BYTES, &attr_done);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kern, dim3(blocks, (nq_launch + NQ - 1) / NQ), dim3(256), (size_t)lds, st, a, a.q0 + nq_launch, acc);
    return (int)hipGetLastError();
}
template <int QT, int MODE>
static int bscan_metric(const ScanArgs& a, int nq_launch, int blocks, bool vec, hipStream_t st) {
    return vec ? bscan_launch<QT, MODE, true>(a, nq_launch, blocks, st) : bscan_launch<QT, MODE, false>(a, nq_launch, blocks, st);
}

// Entry used by hdb_launch_scan for dtype == HDB_B1.  mode: 0 = write scores, 1 = threshold filter.
extern "C" int hdb_launch_bscan(const ScanArgs* args, int mode, int nq_launch, int max_blocks, void* stream) {
    ScanArgs a = *args;
    hipStream_t st = (hipStream_t)stream;
    if (a.rows || nq_launch < 1 || (mode != 0 && mode != 1)) return (int)hipErrorInvalidValue;      // (no list flavour: the plan never asks)
    if (a.metric == HDB_HAMMING || a.metric == HDB_JACCARD) return (int)hipErrorInvalidValue;       // (the bit kernels on the sign cache)
    const int qt_max = hdb_bscan_qt(a.d);
    if (qt_max < 0 || (reinterpret_cast<uintptr_t>(a.V) & 3) != 0) return (int)hipErrorInvalidValue;
    a.row_bytes = (int32_t)hdb_row_bytes(HDB_B1, a.d);
    a.nchunks = a.row_bytes / 16;
    const bool vec = a.row_bytes % 16 == 0 && (reinterpret_cast<uintptr_t>(a.V) & 15) == 0;
    // queries per pass: the rule's, but no more tables than the launch has queries (1, 2 or 4)
    const int want = nq_launch >= 3 ? 4 : nq_launch;
    const int qt = qt_max == 0 ? 0 : (qt_max < want ? qt_max : want);
    const int auto_blocks = hdb_bscan_auto_blocks(a.d, qt, hdb_cu_count());
    const int blocks = hdb_grid_for(a.ntiles * 16, 256, max_blocks > 0 ? max_blocks : auto_blocks);
#define HDB_BSCAN_QT(QT_) (mode == 0 ? bscan_metric<QT_, 0>(a, nq_launch, blocks, vec, st) : bscan_metric<QT_, 1>(a, nq_launch, blocks, vec, st))
    if (qt == 4) return HDB_BSCAN_QT(4);
    if (qt == 2) return HDB_BSCAN_QT(2);
    if (qt == 1) return HDB_BSCAN_QT(1);
    return HDB_BSCAN_QT(0);
#undef HDB_BSCAN_QT
}
