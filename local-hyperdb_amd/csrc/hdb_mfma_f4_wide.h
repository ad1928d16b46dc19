// hdb_mfma_f4_wide.h -- MXFP4 rows (HDB_MXF4) WIDER than 512 elements on the bf16 matrix pipe, in ONE launch: the kernel behind
// hdb_mfma_f4_wide*.hip (opt-in: b1_mfma_min_q >= 1 together with f8_ks_min_q != 0; hdb_mfma_f4_wide_geom, hdb_caps.h).
//
// The arithmetic, the row loads and the K permutation are the whole-row kernel's (hdb_mfma_f4.h): one 16-byte load per MX block, one
// scale byte per load, four v_cvt_scalef32_pk_bf16_fp4 per fragment, three v_mfma_f32_16x16x32_bf16 per k-step against the query's
// three exact bf16 parts, smallest part first.  What a wave cannot do beyond 512 elements is HOLD the query parts: 3 d / 8 registers.
// The other row types cut such rows into K slices, one launch per slice with the raw partial sums in a float32 workspace between
// the launches.  For half-byte rows that is the wrong trade: one extra slice costs 8 bytes per row and query, at 64 queries 512
// bytes per row against the 544 of a 1024-element row itself.  So here the WAVES OF ONE WORKGROUP split K and the partial sums never
// leave the CU:
//   * a workgroup is S = d / W waves (2 .. 8; W = 128 / 256 / 384 / 512, the template parameter; S is blockDim.x / 64, a run-time
//     value, so the kernels of a W serve every d = S W).  All S waves work on the same 16-row tile and the same 16 queries;
//   * wave s owns elements [s W, (s + 1) W) of every row: lane (rl, h) loads the uint4 at byte s W / 2 + 64 j + 16 h of the stored
//     row for j < W / 128 -- MX blocks 4 (s W / 128 + j) + h -- and the scale word at byte d / 2 + s W / 32 + 4 j (4-byte aligned: W
//     is a multiple of 128), of which it selects byte h.  The pitch is hdb_row_bytes(HDB_MXF4, d);
//   * its query parts are those of elements s W + 128 j + 32 h + 8 i .. + 7, built once before the tile loop: 3 W / 8 registers;
//   * every wave's accumulator starts from zero; after the K walk the waves other than the tile's reducer store theirs to LDS, one
//     float4 per lane (1 KiB per wave), the workgroup meets at ONE barrier, and the reducer adds the S partial sums IN SLICE ORDER
//     0, 1 .. S - 1 -- its own from its registers at its own position -- and runs the shared epilogue (hdb_f8_tile_finish).  The
//     order is fixed, so a row's score has the same float32 bits in every mode, grid and batch size, as in the whole-row kernel;
//   * two LDS buffers alternate by tile, which is why one barrier per tile is enough: whoever writes tile i + 2 into the buffer of
//     tile i has passed the barrier of tile i + 1, and the reducer of tile i reaches that barrier only after it has read;
//   * the reducer ROTATES: step i of a workgroup is reduced by wave i mod S, so the epilogue's per-row loads (aux0, bias), its
//     stores and atomics, and the wait for S - 1 KiB of LDS are spread over the waves instead of making one wave the straggler of
//     every barrier.  (A fixed reducer was not built; the choice is by that argument, not by a measurement.)
// The barrier makes the control flow a contract: every exit before the loop is workgroup-uniform (a workgroup serves ONE query
// group; its tile walk depends on blockIdx alone), every wave walks t = blockIdx.x, + gridDim.x .. the same number of times, and a
// ragged last tile or query group is clamped (min(row, n - 1), q_ok), never left.
// From W <= 384 the next tile's loads are issued before this tile is converted (the whole-row kernel's finding); at W = 512 the 192
// registers of query parts leave no room for a second tile's 20, and the second wave per SIMD is what hides the latency there.
// Grid: x = workgroups over tiles (hdb_mfma_f4_wide_blocks), y = one 16-query group per workgroup; the groups of a larger batch
// re-read the tile through the caches, as the whole-row kernel's query groups do.
// MODE 0 = store the scores, MODE 1 = filter against a.thr; METRIC 0 dot, 1 cosine / pearson, 2 euclidean: hdb_mfma_f4.h.
// The matrix must be finite (the plan asks), for the whole-row kernel's reason.
#pragma once
#include "hdb_mfma_f4.h"

// (512 threads at most: two waves per SIMD, 256 registers per lane, accumulator included -- the bound W = 512 has to meet.
//  profiles/f4_wide_kernel_resources.txt has every instantiation.)
template <int W, int MODE, int METRIC, bool HAS_BIAS>
__global__ __launch_bounds__(512) void hdb_mfma_f4_wide_kernel(ScanArgs a, const float* __restrict__ Qf, const float* __restrict__ aux0,
                                                               const float* __restrict__ qsq, int nq_end, int pitch) {
    static_assert(W % 128 == 0 && W >= 128 && W <= 512 && (MODE == 0 || MODE == 1), "whole groups of four MX blocks; MODE 0 / 1");
    constexpr int NJ = W / 128, KS = W / 32;
    constexpr bool FILT = MODE == 1;
    extern __shared__ float4 hdb_f4w_part[];         // [2 buffers][S waves][64 lanes]
    const int lane = threadIdx.x & 63;
    const int s = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int S = (int)(blockDim.x >> 6);
    const int rl = lane & 15, h = lane >> 4;
    const int d = a.d;
    const int qw0 = a.q0 + (int)blockIdx.y * 16;
    if (qw0 >= nq_end || (int64_t)blockIdx.x >= a.ntiles) return;      // (workgroup-uniform: before any barrier)
    const int q = qw0 + rl;
    const bool q_ok = q < nq_end;
    const int ql = q - a.q0;
    const int qq = q_ok ? q : nq_end - 1;
    HdbParts3 Bq[KS];                                // k-step 4 j + i of the slice: query elements s W + 128 j + 32 h + 8 i .. + 7
    {
        const float4* qf = reinterpret_cast<const float4*>(Qf + (int64_t)qq * d + s * W) + 8 * h;
#pragma unroll
        for (int c = 0; c < KS; ++c) {
            float4 x0 = qf[32 * (c >> 2) + 2 * (c & 3)], x1 = qf[32 * (c >> 2) + 2 * (c & 3) + 1];
            if (!q_ok) { x0 = make_float4(0.f, 0.f, 0.f, 0.f); x1 = x0; }
            Bq[c] = hdb_split3_finite(HdbRaw8{f32x4{x0.x, x0.y, x0.z, x0.w}, f32x4{x1.x, x1.y, x1.z, x1.w}});
        }
    }
    float qinv_l = 1.f, qsq_l = 0.f, thr_cmp = INFINITY;
    if (q_ok) {
        if (METRIC == 1) qinv_l = a.qinv[q];
        if (METRIC == 2) qsq_l = qsq[q];
        if (FILT) {
            const float thr = a.thr[ql];
            if (METRIC != 2 && !HAS_BIAS) { const float tc = thr / qinv_l; thr_cmp = tc - fabsf(tc) * 1e-6f; }
            else thr_cmp = thr;
        }
    }
    // the slice of a lane's row: its codes from byte s W / 2 + 16 h, its scale words from byte d / 2 + s W / 32
    const char* const Vb = reinterpret_cast<const char*>(a.V) + s * (W / 2) + 16 * h;
    const int sc_off = d / 2 + s * (W / 32) - s * (W / 2) - 16 * h;
    const int64_t n_rows = a.n;
    const int sh = 8 * h;
    auto load_tile = [&](int64_t t, uint4 (&raw)[NJ], uint32_t (&sw)[NJ]) {      // (a ragged last tile re-reads the last row)
        const int64_t ra = min(hdb_tile_index(t, a.tile_stride) * 16 + rl, n_rows - 1);
        const char* src = Vb + ra * (int64_t)pitch;
#pragma unroll
        for (int j = 0; j < NJ; ++j) raw[j] = *reinterpret_cast<const uint4*>(src + 64 * j);
#pragma unroll
        for (int j = 0; j < NJ; ++j) sw[j] = *reinterpret_cast<const uint32_t*>(src + sc_off + 4 * j);
    };
    constexpr bool AHEAD = W < 512;
    const int64_t t_step = gridDim.x;
    uint4 raw[NJ];
    uint32_t sw[NJ];
    if constexpr (AHEAD) load_tile(blockIdx.x, raw, sw);
    int red = 0, buf = 0;                            // this step's reducer and LDS buffer: the same in every wave
    for (int64_t t = blockIdx.x; t < a.ntiles; t += t_step) {
        uint4 nraw[NJ];
        uint32_t nsw[NJ];
        if constexpr (AHEAD) load_tile(min(t + t_step, a.ntiles - 1), nraw, nsw);      // (the last step re-reads a tile: t never leaves [0, ntiles))
        else load_tile(t, raw, sw);
        const int64_t row0 = hdb_tile_index(t, a.tile_stride) * 16;
        const int64_t rowg = row0 + 4 * h;
        // C register j of lane (rl, h) = row 4 h + j of the tile x query rl, over this wave's slice of K
        f32x4 acc = hdb_f8_acc_start<false>(a, q_ok, 0, rowg, n_rows);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const float scale = hdb_mxf4_scale_f(__builtin_amdgcn_ubfe(sw[j], (uint32_t)sh, 8u));
            const uint32_t word[4] = {raw[j].x, raw[j].y, raw[j].z, raw[j].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const u32x4 av = hdb_f4x8_to_bf16x8(word[i], scale);
                const HdbParts3& b = Bq[4 * j + i];
#define HDB_BF(x) __builtin_bit_cast(hdb_bf16x8, x)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(HDB_BF(av), HDB_BF(b.p2), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(HDB_BF(av), HDB_BF(b.p1), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(HDB_BF(av), HDB_BF(b.p0), acc, 0, 0, 0);
#undef HDB_BF
            }
        }
        float4* const part = hdb_f4w_part + buf * S * 64 + lane;
        if (s != red) part[s * 64] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        __syncthreads();
        if (s == red) {                              // slice order 0, 1 .. S - 1, whoever adds
            f32x4 sum = acc;
            if (s != 0) { const float4 p = part[0]; sum = f32x4{p.x, p.y, p.z, p.w}; }
            for (int u = 1; u < S; ++u) {
                f32x4 pu = acc;
                if (u != s) { const float4 p = part[u * 64]; pu = f32x4{p.x, p.y, p.z, p.w}; }
                sum += pu;
            }
            hdb_f8_tile_finish<MODE, METRIC, HAS_BIAS, false>(a, sum, aux0, t, h, rowg, n_rows, q_ok, ql, qinv_l, qsq_l, thr_cmp, 0);
        }
        red = red + 1 == S ? 0 : red + 1;
        buf ^= 1;
        if constexpr (AHEAD) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) { raw[j] = nraw[j]; sw[j] = nsw[j]; }
        }
    }
}

// One launch: S x 64 threads, 2 S KiB of LDS, grid (l.blocks workgroups over the tiles, 16-query groups)
template <int W>
static int launch_f4_wide(const ScanArgs& a, const MfmaLaunch& l) {
    const HdbF4WideGeom g = hdb_mfma_f4_wide_geom(a.d);
    const int gw = g.w, gs = g.s;
    const int pitch = (int)hdb_row_bytes(HDB_MXF4, a.d);
    // 16-byte block loads: base and pitch; the slices make up the row; a mask arrives folded into the bias
    if ((reinterpret_cast<uintptr_t>(a.V) & 15) != 0 || pitch <= 0 || (pitch & 15) != 0 || gw != W || gs < 2 || gs > 8 || a.d != gs * W || a.mask ||
        a.n < 1 || l.blocks < 1 || l.nq_launch < 1)
        return (int)hipErrorNotSupported;
    const dim3 grid(l.blocks, (l.nq_launch + 15) / 16), block(64 * gs);
    const size_t lds = (size_t)2 * gs * 64 * sizeof(float4);
    return hdb_mode_ladder<1, 0>(a, l.mode, l.sqnorm, [&](auto mode, auto metric, auto bias, const float* aux0) {
        hipLaunchKernelGGL((hdb_mfma_f4_wide_kernel<W, mode.value, metric.value, bias.value != 0>), grid, block, lds, (hipStream_t)l.stream, a,
                           (const float*)l.q, aux0, l.qsq, a.q0 + l.nq_launch, pitch);
        return (int)hipGetLastError();
    });
}
