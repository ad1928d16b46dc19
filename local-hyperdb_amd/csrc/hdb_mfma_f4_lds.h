// hdb_mfma_f4_lds.h -- MXFP4 rows (HDB_MXF4) on the bf16 matrix pipe for LARGE BATCHES: the rows stationary in registers, the query
// parts stationary in LDS.  The kernel behind hdb_mfma_f4_lds*.hip; opt-in (f8_lds_min_q beside b1_mfma_min_q, ScanArgs::f8_lds = 1).
//
// The arithmetic and the bits are hdb_mfma_f4_kernel's (hdb_mfma_f4.h): a float32 query as three exact bf16 parts (hdb_split3_finite),
// a row element as ONE bf16 (v_cvt_scalef32_pk_bf16_fp4 with the block scale), the K permutation of that kernel -- k slot 8 h + e of
// k-step 4 j + i is element 128 j + 32 h + 8 i + e -- k-steps in order, p2, p1, p0 per step on one float32 accumulator per (row,
// query), and that kernel's epilogue (hdb_f8_tile_finish).  A row's score has the same bits in both flavours.
//
// What differs is who holds what.  The register kernel keeps the parts of ONE group of 16 queries in a wave's registers (3 D / 8 of
// them) and streams tiles past it: every further group of 16 queries is another wave that loads and converts the tile again, and
// each wave walks K on one accumulator, a chain of 3 D / 32 dependent matrix instructions.  Half-byte rows turn the sizes round: the
// queries are the large operand (6 bytes per element), a converted 16-row tile the small one (D / 8 registers per lane).  So here
//   * a workgroup of four waves serves a BLOCK of G groups of 16 queries (hdb_mfma_f4_lds_groups: 4, at d = 512 3; blockIdx.y picks
//     the block).  Its waves split the three parts of those queries once, at kernel start, and store them to LDS lane-major: the
//     fragment of (k-step s, group g, part p) is the 1 KiB at ((s G + g) 3 + p) 1024, lane l's 16 bytes at + 16 l -- exactly what
//     lane l hands the matrix instruction, so every later read is one ds_read_b128 at consecutive addresses, free of bank conflicts.
//     D / 32 x G x 3 KiB: 48 / 96 / 144 / 144 KiB of the 160.  ONE barrier after the fill, none in the tile loop;
//   * every wave owns its tiles, TWO 16-row tiles per step (the workgroup takes eight per step, the grid is persistent in x).  It
//     loads them with the register kernel's loads -- one uint4 per group of four MX blocks, one scale word per j, all issued before
//     the first conversion -- and converts each tile ONCE into A fragments that stay in registers: 2 x D / 32 x 4 of them.  The next
//     pair's loads are issued before this pair is multiplied;
//   * for k-step s and group g the three parts are read from LDS once and multiplied with BOTH tiles into acc[tile][g]: 2 G
//     independent accumulators, so consecutive matrix instructions do not wait for each other, and one 3-KiB read feeds six of them
//     (one tile per read would ask 3 KiB of LDS per three matrix instructions and wave: at or above what the LDS port delivers).
// Queries past nq_end are zero parts; a group wholly past nq_end is neither filled nor multiplied (`ng`, uniform in the workgroup:
// the multiply is compiled once per count so that its straight line is not cut by branches).  An odd tile count clamps the second
// tile of the last pair to the last tile and skips its epilogue; a ragged last tile re-reads the last row.
// One wave per SIMD, within the 512 registers a wave has there (profiles/f4_lds_kernel_resources.txt has every instantiation).
#pragma once
#include "hdb_mfma_f4.h"

// K steps x NG groups: the fragments of (s, g + 1) are read while those of (s, g) are multiplied
template <int D, int G, int NG>
__device__ __forceinline__ void hdb_f4_lds_multiply(const unsigned char* __restrict__ qp, const u32x4 (&A)[2][D / 32], f32x4 (&acc)[2][G]) {
    constexpr int NF = D / 32 * NG;
    auto part = [&](int f, int p) { return *reinterpret_cast<const u32x4*>(qp + (((f / NG) * G + f % NG) * 3 + p) * 1024); };
    u32x4 c0 = part(0, 0), c1 = part(0, 1), c2 = part(0, 2);
    __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);        // (the order is pinned: left alone the scheduler sinks every read to its
#pragma unroll                                                //  first use, one register quad and a full LDS round trip per two MFMAs)
    for (int f = 0; f < NF; ++f) {
        const int s = f / NG, g = f % NG;
        u32x4 n0 = c0, n1 = c1, n2 = c2;
        if (f + 1 < NF) { n2 = part(f + 1, 2); n1 = part(f + 1, 1); n0 = part(f + 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 3, 0); }
        __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
#define HDB_BF(x) __builtin_bit_cast(hdb_bf16x8, x)
        acc[0][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(HDB_BF(A[0][s]), HDB_BF(c2), acc[0][g], 0, 0, 0);
        acc[1][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(HDB_BF(A[1][s]), HDB_BF(c2), acc[1][g], 0, 0, 0);
        acc[0][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(HDB_BF(A[0][s]), HDB_BF(c1), acc[0][g], 0, 0, 0);
        acc[1][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(HDB_BF(A[1][s]), HDB_BF(c1), acc[1][g], 0, 0, 0);
        acc[0][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(HDB_BF(A[0][s]), HDB_BF(c0), acc[0][g], 0, 0, 0);
        acc[1][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(HDB_BF(A[1][s]), HDB_BF(c0), acc[1][g], 0, 0, 0);
#undef HDB_BF
        c0 = n0; c1 = n1; c2 = n2;
    }
}

template <int D, int MODE, int METRIC, bool HAS_BIAS>
__global__ __launch_bounds__(256, 1) void hdb_mfma_f4_lds_kernel(ScanArgs a, const float* __restrict__ Qf, const float* __restrict__ aux0,
                                                                 const float* __restrict__ qsq, int nq_end) {
    static_assert(hdb_mfma_f4_lds_supported(D) && (MODE == 0 || MODE == 1), "128 / 256 / 384 / 512; MODE 0 / 1");
    constexpr int NJ = D / 128, KS = D / 32, G = hdb_mfma_f4_lds_groups(D);
    constexpr int PITCH = HdbF4Row<D>::pitch;
    constexpr bool FILT = MODE == 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char hdb_f4_qparts[];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int rl = lane & 15, h = lane >> 4;
    const int qb0 = a.q0 + (int)blockIdx.y * 16 * G;
    const int ng = min(G, (nq_end - qb0 + 15) / 16);          // groups of this block that hold a query
    if (ng < 1) return;                                       // (uniform in the workgroup, before the barrier)

    // the query parts of the block -> LDS: the (k-step, group) pairs go round the four waves
    for (int f = w; f < KS * ng; f += 4) {
        const int s = f / ng, g = f - s * ng;
        const int q = qb0 + 16 * g + rl;
        const bool ok = q < nq_end;
        const float4* qf = reinterpret_cast<const float4*>(Qf + (int64_t)(ok ? q : nq_end - 1) * D) + 8 * h;
        float4 x0 = qf[32 * (s >> 2) + 2 * (s & 3)], x1 = qf[32 * (s >> 2) + 2 * (s & 3) + 1];      // k-step 4 j + i: query elements 128 j + 32 h + 8 i .. + 7
        if (!ok) { x0 = make_float4(0.f, 0.f, 0.f, 0.f); x1 = x0; }
        const HdbParts3 b = hdb_split3_finite(HdbRaw8{f32x4{x0.x, x0.y, x0.z, x0.w}, f32x4{x1.x, x1.y, x1.z, x1.w}});
        unsigned char* dst = hdb_f4_qparts + (s * G + g) * 3 * 1024 + lane * 16;
        *reinterpret_cast<u32x4*>(dst) = b.p0;
        *reinterpret_cast<u32x4*>(dst + 1024) = b.p1;
        *reinterpret_cast<u32x4*>(dst + 2048) = b.p2;
    }
    // what the epilogue knows of query rl of each group
    bool q_ok[G];
    int ql[G];
    float qinv_l[G], qsq_l[G], thr_cmp[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int q = qb0 + 16 * g + rl;
        q_ok[g] = q < nq_end;
        ql[g] = q - a.q0;
        qinv_l[g] = 1.f; qsq_l[g] = 0.f; thr_cmp[g] = INFINITY;
        if (q_ok[g]) {
            if (METRIC == 1) qinv_l[g] = a.qinv[q];
            if (METRIC == 2) qsq_l[g] = qsq[q];
            if (FILT) {
                const float thr = a.thr[ql[g]];
                if (METRIC != 2 && !HAS_BIAS) { const float tc = thr / qinv_l[g]; thr_cmp[g] = tc - fabsf(tc) * 1e-6f; }
                else thr_cmp[g] = thr;
            }
        }
    }
    __syncthreads();                                          // the only barrier: the parts are read-only from here on

    const char* const Vb = reinterpret_cast<const char*>(a.V);
    const int64_t n_rows = a.n;
    const int sh = 8 * h;
    // the blocks 4 j + h of a lane's row of tile t and the scale words that hold their scale bytes (hdb_mfma_f4_kernel's loads)
    auto load_tile = [&](int64_t t, uint4 (&raw)[NJ], uint32_t (&sw)[NJ]) {
        const int64_t ra = min(hdb_tile_index(t, a.tile_stride) * 16 + rl, n_rows - 1);
        const char* src = Vb + ra * (int64_t)PITCH;
#pragma unroll
        for (int j = 0; j < NJ; ++j) raw[j] = *reinterpret_cast<const uint4*>(src + 64 * j + 16 * h);
#pragma unroll
        for (int j = 0; j < NJ; ++j) sw[j] = *reinterpret_cast<const uint32_t*>(src + D / 2 + 4 * j);
    };
    const int64_t last = a.ntiles - 1;
    const int64_t t_step = (int64_t)gridDim.x * 8;
    int64_t t = ((int64_t)blockIdx.x * 4 + w) * 2;            // this wave's pair: tiles t and t + 1
    if (t > last) return;
    uint4 raw[2][NJ];
    uint32_t sw[2][NJ];
    load_tile(t, raw[0], sw[0]);
    load_tile(min(t + 1, last), raw[1], sw[1]);
    const unsigned char* const qp = hdb_f4_qparts + lane * 16;
    for (; t <= last; t += t_step) {
        u32x4 A[2][KS];                                       // both tiles as bf16, converted once
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const float scale = hdb_mxf4_scale_f(__builtin_amdgcn_ubfe(sw[u][j], (uint32_t)sh, 8u));
                const uint32_t word[4] = {raw[u][j].x, raw[u][j].y, raw[u][j].z, raw[u][j].w};
#pragma unroll
                for (int i = 0; i < 4; ++i) A[u][4 * j + i] = hdb_f4x8_to_bf16x8(word[i], scale);
            }
        }
        // the next pair's loads, in flight while this pair is multiplied (the last step re-reads the last tile: never past it)
        load_tile(min(t + t_step, last), raw[0], sw[0]);
        load_tile(min(t + t_step + 1, last), raw[1], sw[1]);
        f32x4 acc[2][G];
#pragma unroll
        for (int g = 0; g < G; ++g) { acc[0][g] = hdb_f8_acc_start<false>(a, q_ok[g], 0, 0, n_rows); acc[1][g] = acc[0][g]; }
        if (ng == 1) hdb_f4_lds_multiply<D, G, 1>(qp, A, acc);
        else if (ng == 2) hdb_f4_lds_multiply<D, G, 2>(qp, A, acc);
        else if (G == 3 || ng == 3) hdb_f4_lds_multiply<D, G, 3>(qp, A, acc);
        else hdb_f4_lds_multiply<D, G, G>(qp, A, acc);
        // C register j of lane (rl, h) = row 4 h + j of the tile x query rl of the group
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int64_t tu = t + u;
            if (tu > last) break;                             // (an odd tile count: the clamped copy of the last tile)
            const int64_t rowg = hdb_tile_index(tu, a.tile_stride) * 16 + 4 * h;
#pragma unroll
            for (int g = 0; g < G; ++g)
                if (g < ng) hdb_f8_tile_finish<MODE, METRIC, HAS_BIAS, false>(a, acc[u][g], aux0, tu, h, rowg, n_rows, q_ok[g], ql[g], qinv_l[g], qsq_l[g], thr_cmp[g], 0);
        }
    }
}

// l.blocks: the workgroups of the launch in x (hdb_mfma_f4_lds_blocks); grid.y: the blocks of 16 G queries, each of which reads the matrix
template <int D, int MODE, int METRIC, bool HAS_BIAS>
static int launch_f4_lds_one(const ScanArgs& a, const MfmaLaunch& l, const float* aux0) {
    auto kern = hdb_mfma_f4_lds_kernel<D, MODE, METRIC, HAS_BIAS>;
    static unsigned long long attr_done = 0;          // per instantiation, one bit per device
    const hipError_t e = hdb_lds_attr_once(reinterpret_cast<const void*>(kern), hdb_mfma_f4_lds_bytes(D), &attr_done);      // (d >= 256: beyond 64 KiB)
    if (e != hipSuccess) return (int)e;
    constexpr int QB = 16 * hdb_mfma_f4_lds_groups(D);
    const dim3 grid(l.blocks, (l.nq_launch + QB - 1) / QB);
    hipLaunchKernelGGL(kern, grid, dim3(256), (size_t)hdb_mfma_f4_lds_bytes(D), (hipStream_t)l.stream, a, (const float*)l.q, aux0, l.qsq, a.q0 + l.nq_launch);
    return (int)hipGetLastError();
}
template <int D>
static int launch_f4_lds(const ScanArgs& a, const MfmaLaunch& l) {
    // 16-byte block loads: base and pitch; a mask arrives folded into the bias
    static_assert(HdbF4Row<D>::pitch % 16 == 0 && (D / 2) % 64 == 0 && hdb_mfma_f4_lds_bytes(D) <= 160 * 1024, "16-byte blocks, aligned scale words, the LDS of a CU");
    if ((reinterpret_cast<uintptr_t>(a.V) & 15) != 0 || a.d != D || hdb_row_bytes(HDB_MXF4, a.d) != HdbF4Row<D>::pitch || a.mask || a.n < 1 || a.ntiles < 1 ||
        l.blocks < 1 || l.nq_launch < 1)
        return (int)hipErrorNotSupported;
    return hdb_mode_ladder<1, 0>(a, l.mode, l.sqnorm, [&](auto mode, auto metric, auto bias, const float* aux0) {
        return launch_f4_lds_one<D, mode.value, metric.value, bias.value != 0>(a, l, aux0);
    });
}
