// hdb_f4scan.hip -- float32 queries against MXFP4 rows (HDB_MXF4) for gfx950: dot / cosine / pearson / euclidean / manhattan.
//
// A stored row is [d / 2 code bytes][d / 32 scale bytes][zero padding] at pitch hdb_row_bytes(HDB_MXF4, d), a multiple of 16 bytes.
// The 16-byte code chunk c of a row is MX block c: 32 e2m1 elements (element e of the row = nibble e & 1 of byte e >> 1, the even
// element in the low nibble) that share scale byte c, an e8m0 power of two.  Every element widens to float32 exactly, so the scores
// are the float32 contract's on the widened matrix: the terms themselves, never ||v||^2 + ||q||^2 - 2 q.v.
//
// The tile is hdb_scan_kernel's: a wave covers 16 consecutive rows, lane group g = lane >> 4 owns rows 4g .. 4g + 3, lane l16 of the
// group takes chunk l16 + 16 j of each of them, and the row sums finish with hdb_rows4_sum -- so the sample, the candidate packing
// and the epilogue (hdb_emit.h) are shared.  A 16-lane group reads the code bytes of a row as one contiguous piece.
//
// The query lives in REGISTERS where the row allows it (NJ = 1: d <= 512, NJ = 2: d <= 1024): a lane only ever meets chunk l16
// (+ 16), so its 32 (64) query elements per query are loop-invariant -- loaded once per workgroup, and the grid-stride loop reads
// no LDS.  A 16-byte load carries 32 elements here; a query in LDS costs 128 bytes of reads per lane, chunk and query, twice int8's
// ratio ("MXFP4 matrices").  Wider rows take the runtime loop with the query in LDS (NJ = 0), one query per pass: larger
// LDS passes were built and measured slower than several small ones (hdb_f4scan_qt, hdb_caps.h).
//
// The inner step of a chunk: the scale float is scale byte << 23, v_cvt_scalef32_pk_f32_fp4 widens two elements with the scale
// applied (16 per chunk, four byte selects per word), and the 16 pairs meet the 16 query pairs in packed float32 arithmetic.
//
// ONE summation order per row, whatever the mode, the grid, the number of queries of the pass and the flavour: a lane keeps two
// partial sums per row and query -- the even elements of its chunks and the odd ones, chunk after chunk, element pair after element
// pair, every term added with one explicit fma (dot, euclidean) or one add (manhattan) -- adds the two, and the sixteen lanes
// of a row are added by hdb_rows4_sum.  Lanes without a chunk, and the padding, take no part: they contribute exactly 0.
#include "hdb_common.h"
#include "hdb_emit.h"
#include "../../include/hyperdb_hip.h"

typedef float hdb_f2 __attribute__((ext_vector_type(2)));

// one MX block -> its 32 float32 values as 16 pairs in element order (pair 4 w + b = byte b of word w: low nibble, high nibble)
#define HDB_F4_WORD(w)                                                                    \
    x[4 * (w) + 0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(raw[w], scale, 0);          \
    x[4 * (w) + 1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(raw[w], scale, 1);          \
    x[4 * (w) + 2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(raw[w], scale, 2);          \
    x[4 * (w) + 3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(raw[w], scale, 3);
__device__ __forceinline__ void hdb_f4_widen(const hdb_u32x4 raw, uint32_t scale_byte, hdb_f2 (&x)[16]) {
    const float scale = __uint_as_float(scale_byte << 23);      // 2^(s - 127): one shift per chunk (255: the exponent of inf / NaN)
    HDB_F4_WORD(0) HDB_F4_WORD(1) HDB_F4_WORD(2) HDB_F4_WORD(3)
}
#undef HDB_F4_WORD

// 32 terms of one row and one query into the row's two partial sums.  ACC as in hdb_scan.hip: 0 dot, 1 squared difference, 2 absolute
// difference.  Explicit fma / add per pair: the bits do not depend on what the compiler would contract.
template <int ACC>
__device__ __forceinline__ void hdb_f4_step(hdb_f2& acc, const hdb_f2 (&x)[16], const hdb_f2 (&q)[16]) {
#pragma unroll
    for (int p = 0; p < 16; ++p) {
        if (ACC == 0) acc = __builtin_elementwise_fma(x[p], q[p], acc);
        else {
            const hdb_f2 df = x[p] - q[p];
            if (ACC == 1) acc = __builtin_elementwise_fma(df, df, acc);
            else acc = acc + __builtin_elementwise_abs(df);
        }
    }
}

// grid = (blocks, ceil(nq_launch / QT)); block = 256 threads = 4 waves.  NJ > 0: the queries in registers, NJ chunk steps per row;
// NJ == 0: the queries in LDS (QT * d floats; built for QT = 1), any number of steps.
template <int QT, int MODE, int ACC, int NJ>
__global__ __launch_bounds__(256) void hdb_f4scan_kernel(ScanArgs a, int nq_end) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* qs = reinterpret_cast<float*>(smem);
    __shared__ HdbStage stage;
    if (MODE == 1) hdb_stage_init(stage);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, l16 = lane & 15;
    const int d = a.d, nblk = d >> 5, code_bytes = d >> 1;
    const int qbase = a.q0 + blockIdx.y * QT;
    const float* Q = reinterpret_cast<const float*>(a.Q);

    hdb_f2 qr[NJ > 0 ? NJ : 1][QT][16];
    if constexpr (NJ > 0) {
        // this lane's fragments: elements 32 c .. 32 c + 31 of every query of the pass, c = l16 + 16 j (none: zeros, never used)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = l16 + 16 * j;
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                const float* qp = Q + (int64_t)min(qbase + qt, nq_end - 1) * d + 32 * min(c, nblk - 1);
#pragma unroll
                for (int p = 0; p < 16; ++p) qr[j][qt][p] = hdb_f2{qp[2 * p], qp[2 * p + 1]};
            }
        }
    } else {
        for (int i = threadIdx.x; i < QT * d; i += 256) {
            const int qt = i / d, e = i - qt * d;
            qs[i] = Q[(int64_t)min(qbase + qt, nq_end - 1) * d + e];
        }
    }
    __syncthreads();

    const char* Vb = reinterpret_cast<const char*>(a.V);
    const int nj = NJ > 0 ? NJ : (nblk + 15) >> 4;
    for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < a.ntiles; t += (int64_t)gridDim.x * 4) {
        const int64_t r0 = hdb_tile_index(t, a.tile_stride) * 16 + 4 * g;
        const char* p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] = Vb + min(r0 + u, a.n - 1) * (int64_t)a.row_bytes;
        hdb_f2 acc[4][QT];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) acc[u][qt] = hdb_f2{0.f, 0.f};

        // chunk c of the four rows: the code chunk non-temporal (V is streamed once per pass), its scale byte from the same row --
        // the line it sits in is the row's last code line or the one behind it, in flight for this very wave
        auto load4 = [&](int c, hdb_u32x4 (&raw)[4], uint32_t (&sb)[4]) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                raw[u] = __builtin_nontemporal_load(reinterpret_cast<const hdb_u32x4*>(p[u] + (int64_t)c * 16));
                sb[u] = *reinterpret_cast<const uint8_t*>(p[u] + code_bytes + c);
            }
        };
        if constexpr (NJ > 0) {
            hdb_u32x4 raw[NJ][4];
            uint32_t sb[NJ][4];
            // every load of the tile before the first use; a lane without chunk c loads nothing
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                if (l16 + 16 * j < nblk) load4(l16 + 16 * j, raw[j], sb[j]);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (l16 + 16 * j < nblk) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        hdb_f2 x[16];
                        hdb_f4_widen(raw[j][u], sb[j][u], x);
#pragma unroll
                        for (int qt = 0; qt < QT; ++qt) hdb_f4_step<ACC>(acc[u][qt], x, qr[j][qt]);
                    }
                }
            }
        } else {
            for (int j = 0; j < nj; ++j) {
                const int c = l16 + 16 * j;
                if (c < nblk) {
                    hdb_u32x4 raw[4];
                    uint32_t sb[4];
                    load4(c, raw, sb);
                    hdb_f2 x[4][16];
#pragma unroll
                    for (int u = 0; u < 4; ++u) hdb_f4_widen(raw[u], sb[u], x[u]);
#pragma unroll
                    for (int qt = 0; qt < QT; ++qt) {
                        hdb_f2 q[16];                        // the chunk's 32 query elements: read once for the four rows
                        const hdb_f2* ql = reinterpret_cast<const hdb_f2*>(qs + qt * d + 32 * c);
#pragma unroll
                        for (int e = 0; e < 16; ++e) q[e] = ql[e];
#pragma unroll
                        for (int u = 0; u < 4; ++u) hdb_f4_step<ACC>(acc[u][qt], x[u], q);
                    }
                }
            }
        }
        // finish the 16-lane row sums; lane l16 == u keeps row u of its group (as hdb_scan_kernel)
        const int u_own = hdb_owned_row(l16);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            const float mine = hdb_rows4_sum(acc[0][qt].x + acc[0][qt].y, acc[1][qt].x + acc[1][qt].y, acc[2][qt].x + acc[2][qt].y,
                                             acc[3][qt].x + acc[3][qt].y, l16);
            const int64_t row = r0 + u_own;
            const int q = qbase + qt;
            if ((l16 & 3) == 0 && row < a.n && q < nq_end)
                hdb_emit<MODE>(a, q, row, t * 16 + 4 * g + u_own, mine, MODE == 1 ? &stage : nullptr, qt);
        }
    }
    if (MODE == 1) hdb_stage_flush(a, stage, (int)blockIdx.y * QT, min(QT, nq_end - qbase));
}

template <int QT, int MODE, int ACC, int NJ>
static int f4scan_launch(const ScanArgs& a, int nq_launch, int blocks, hipStream_t st) {
    const size_t lds = NJ > 0 ? 0 : (size_t)hdb_f4scan_lds_bytes(a.d);
    hipLaunchKernelGGL((hdb_f4scan_kernel<QT, MODE, ACC, NJ>), dim3(blocks, (nq_launch + QT - 1) / QT), dim3(256), lds, st, a, a.q0 + nq_launch);
    return (int)hipGetLastError();
}
// the flavours that are built (hdb_f4scan_qt never asks for another): one step 1 / 2 / 4 queries, two steps 1 / 2, the LDS loop 1
template <int QT, int MODE, int ACC>
static int f4scan_nj(const ScanArgs& a, int nj, int nq_launch, int blocks, hipStream_t st) {
    if (nj == 1) return f4scan_launch<QT, MODE, ACC, 1>(a, nq_launch, blocks, st);
    if constexpr (QT <= 2) {
        if (nj == 2) return f4scan_launch<QT, MODE, ACC, 2>(a, nq_launch, blocks, st);
    }
    if constexpr (QT == 1) {
        if (nj == 0) return f4scan_launch<QT, MODE, ACC, 0>(a, nq_launch, blocks, st);
    }
    return (int)hipErrorInvalidValue;
}
template <int QT, int MODE>
static int f4scan_metric(const ScanArgs& a, int nj, int nq_launch, int blocks, hipStream_t st) {
    if (a.metric == HDB_EUCLIDEAN || a.metric == HDB_EUCLIDEAN_DIST) return f4scan_nj<QT, MODE, 1>(a, nj, nq_launch, blocks, st);
    if (a.metric == HDB_MANHATTAN) return f4scan_nj<QT, MODE, 2>(a, nj, nq_launch, blocks, st);
    return f4scan_nj<QT, MODE, 0>(a, nj, nq_launch, blocks, st);
}

// Entry used by hdb_launch_scan for dtype == HDB_MXF4.  mode: 0 = write scores, 1 = threshold filter.
extern "C" int hdb_launch_f4scan(const ScanArgs* args, int mode, int nq_launch, int max_blocks, void* stream) {
    ScanArgs a = *args;
    hipStream_t st = (hipStream_t)stream;
    if (a.rows || nq_launch < 1 || (mode != 0 && mode != 1)) return (int)hipErrorInvalidValue;      // (no list flavour: the plan never asks)
    if (a.metric == HDB_HAMMING || a.metric == HDB_JACCARD) return (int)hipErrorInvalidValue;       // (the bit kernels on the sign cache)
    a.row_bytes = (int32_t)hdb_row_bytes(HDB_MXF4, a.d);
    if (a.row_bytes <= 0 || (reinterpret_cast<uintptr_t>(a.V) & 15) != 0) return (int)hipErrorInvalidValue;
    a.nchunks = a.d / 32;                                                                           // code chunks = MX blocks
    // queries per pass: 1, 2 or 4 -- as many as the launch has, and as the flavour of this width takes (more: several passes, grid.y)
    const int qt = hdb_f4scan_qt(a.d, nq_launch >= 3 ? 4 : nq_launch);
    if (qt < 1) return (int)hipErrorInvalidValue;
    const int nj = hdb_f4scan_nj(a.d);
    const int blocks = hdb_grid_for(a.ntiles, 4, max_blocks > 0 ? max_blocks : hdb_f4scan_auto_blocks(qt, nj, hdb_cu_count()));
#define HDB_F4SCAN_QT(QT_) (mode == 0 ? f4scan_metric<QT_, 0>(a, nj, nq_launch, blocks, st) : f4scan_metric<QT_, 1>(a, nj, nq_launch, blocks, st))
    if (qt == 4) return HDB_F4SCAN_QT(4);
    if (qt == 2) return HDB_F4SCAN_QT(2);
    return HDB_F4SCAN_QT(1);
#undef HDB_F4SCAN_QT
}
