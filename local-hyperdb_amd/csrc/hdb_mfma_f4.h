// hdb_mfma_f4.h -- MXFP4 rows (HDB_MXF4) on the bf16 matrix pipe: the kernel behind hdb_mfma_f4*.hip (opt-in, b1_mfma_min_q).
//
// The arithmetic is the float8 / int8 / packed-bit register kernels' (hdb_mfma_f8.h), which is the bfloat16 flavour's: a float32 query
// travels as three bf16 parts that add up to it exactly (hdb_split3_finite, built once per launch), a row element is ONE bf16 -- an
// e2m1 code has two significant bits and its block scale is a power of two, so while the matrix is finite the scaled value IS a bf16
// number -- and a k-step of 32 elements is three v_mfma_f32_16x16x32_bf16, v p2 + v p1 + v p0 on one accumulator, every product
// exact, float32 accumulation.  The epilogue (hdb_f8_acc_start / hdb_f8_tile_finish), the mode ladder and the launch
// (launch_reg_kernel: grid, the wq rule) are those kernels', reused as they are.
//
// What differs is how the rows reach the A fragments, and with it WHICH elements a k-step multiplies.  A dot product does not care
// which K slot an element sits in as long as A and B agree, and an MXFP4 row is made of 16-byte MX blocks (32 codes, one scale byte):
//   * lane (rl = lane & 15, h = lane >> 4) of a wave loads block 4 j + h of row rl of its 16-row tile for j = 0 .. D / 128 - 1: one
//     uint4 at byte 16 (4 j + h) of the stored row.  The four lanes of a row read 64 contiguous bytes per j; the wave's D / 128 loads
//     cover the row's codes exactly once;
//   * the four words of that load are the lane's A fragments of k-steps 4 j + 0 .. 4 j + 3: word i holds elements
//     32 (4 j + h) + 8 i .. + 7, so k slot 8 h + e of k-step 4 j + i is element 128 j + 32 h + 8 i + e of the row;
//   * ONE scale per load: byte 4 j + h of the row's scale bytes (offset D / 2, 64-byte aligned at these widths: one aligned 4-byte
//     load per j, the lane selects byte h), as the float byte << 23 (hdb_mxf4_scale_f);
//   * four v_cvt_scalef32_pk_bf16_fp4 per fragment -- byte select 0 .. 3 of the word -- give the four packed bf16 words directly: the
//     low nibble is the even element and lands in the low half, the order hdb_split3_finite packs the query parts in.  No permute;
//   * the query fragments follow the same permutation: for k-step 4 j + i lane (ql, h) holds query elements 128 j + 32 h + 8 i .. + 7.
// K is walked k-step 0, 1, 2 .. in that (permuted) order, smallest part first, whatever the grid, the batch size and the mode: a row's
// score has the same float32 bits in every call.
// All loads of a tile -- D / 128 code loads and as many scale words -- are issued before the first conversion, and from D = 256 on the
// NEXT tile's loads are issued before this tile is converted and multiplied (the packed-bit kernel's finding at the same register
// counts: with one to three waves per SIMD and no LDS ring nothing else hides the latency).  No LDS and no barrier: a 256-thread
// workgroup is `wq` query groups of 16 queries x 4 / wq tile lanes.
// MODE 0 = store the scores (row sample, exact path), MODE 1 = filter against a.thr into the candidate lists.  METRIC: 0 dot,
// 1 cosine (aux0 = 1 / ||v|| or pearson's row scale), 2 euclidean similarity through ||v||^2 + ||q||^2 - 2 v.q (aux0 = ||v||^2;
// near-duplicates are re-scored from the widened row by hdb_rescore_euclid_f4_kernel below).
// The matrix must be finite (the plan asks): a block whose values overflow to inf would meet zero query parts, inf x 0 = NaN.
#pragma once
#include "hdb_mfma_f8.h"

// one word of a block (eight codes) and the block's scale -> the A fragment's eight bf16, element 2 j in the low half of word j
__device__ __forceinline__ u32x4 hdb_f4x8_to_bf16x8(uint32_t word, float scale) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    u32x4 o;
    o[0] = __builtin_bit_cast(uint32_t, (bf16x2_t)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 0));
    o[1] = __builtin_bit_cast(uint32_t, (bf16x2_t)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 1));
    o[2] = __builtin_bit_cast(uint32_t, (bf16x2_t)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 2));
    o[3] = __builtin_bit_cast(uint32_t, (bf16x2_t)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 3));
    return o;
}

// the pitch of a stored row of D elements: hdb_row_bytes(HDB_MXF4, D)
template <int D> struct HdbF4Row { static constexpr int pitch = (D / 2 + D / 32 + 15) / 16 * 16; };

// (D = 512: 192 registers of query parts, 2 x 20 of row codes and scale words, the accumulator and the addressing: 248-256 VGPRs plus
//  4 AGPRs, so nothing is asked beyond one workgroup per CU -- the four filter kernels that end above 256 run one wave per SIMD, the
//  float8 kernel's situation -- and the next tile's loads in flight are what hides the latency.  Two workgroups per CU were not
//  tried.  profiles/f4_mfma_kernel_resources.txt has every instantiation.)
template <int D, int MODE, int METRIC, bool HAS_BIAS>
__global__ __launch_bounds__(256, 1) void hdb_mfma_f4_kernel(ScanArgs a, const float* __restrict__ Qf, const float* __restrict__ aux0,
                                                             const float* __restrict__ qsq, int nq_end, int wq) {
    static_assert(D % 128 == 0 && D >= 128 && D <= 512 && (MODE == 0 || MODE == 1), "whole groups of four MX blocks; MODE 0 / 1");
    constexpr int NJ = D / 128, KS = D / 32;
    constexpr int PITCH = HdbF4Row<D>::pitch;
    constexpr bool FILT = MODE == 1;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int rl = lane & 15, h = lane >> 4;
    const int qg = w % wq, tl = w / wq, ntl = 4 / wq;
    const int qw0 = a.q0 + ((int)blockIdx.y * wq + qg) * 16;
    if (qw0 >= nq_end) return;                       // (wave-uniform; the kernel has no barrier)
    const int q = qw0 + rl;
    const bool q_ok = q < nq_end;
    const int ql = q - a.q0;
    const int qq = q_ok ? q : nq_end - 1;
    HdbParts3 Bq[KS];                                // k-step 4 j + i: query elements 128 j + 32 h + 8 i .. + 7
    {
        const float4* qf = reinterpret_cast<const float4*>(Qf + (int64_t)qq * D) + 8 * h;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            float4 x0 = qf[32 * (s >> 2) + 2 * (s & 3)], x1 = qf[32 * (s >> 2) + 2 * (s & 3) + 1];
            if (!q_ok) { x0 = make_float4(0.f, 0.f, 0.f, 0.f); x1 = x0; }
            Bq[s] = hdb_split3_finite(HdbRaw8{f32x4{x0.x, x0.y, x0.z, x0.w}, f32x4{x1.x, x1.y, x1.z, x1.w}});
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
    const char* const Vb = reinterpret_cast<const char*>(a.V);
    const int64_t n_rows = a.n;
    const int sh = 8 * h;
    // the blocks 4 j + h of a lane's row of tile t and the scale words that hold their scale bytes (a ragged last tile re-reads the last row)
    auto load_tile = [&](int64_t t, uint4 (&raw)[NJ], uint32_t (&sw)[NJ]) {
        const int64_t ra = min(hdb_tile_index(t, a.tile_stride) * 16 + rl, n_rows - 1);
        const char* src = Vb + ra * (int64_t)PITCH;
#pragma unroll
        for (int j = 0; j < NJ; ++j) raw[j] = *reinterpret_cast<const uint4*>(src + 64 * j + 16 * h);      // (cached: the waves that share the tile find it in L1 / L2)
#pragma unroll
        for (int j = 0; j < NJ; ++j) sw[j] = *reinterpret_cast<const uint32_t*>(src + D / 2 + 4 * j);
    };
    constexpr bool AHEAD = D > 128;
    const int64_t t_step = (int64_t)gridDim.x * ntl;
    int64_t t = (int64_t)blockIdx.x * ntl + tl;
    if (t >= a.ntiles) return;
    uint4 raw[NJ];
    uint32_t sw[NJ];
    if constexpr (AHEAD) load_tile(t, raw, sw);
    for (; t < a.ntiles; t += t_step) {
        uint4 nraw[NJ];
        uint32_t nsw[NJ];
        if constexpr (AHEAD) load_tile(min(t + t_step, a.ntiles - 1), nraw, nsw);      // (the last step re-reads its own tile: t never leaves [0, ntiles))
        else load_tile(t, raw, sw);
        const int64_t row0 = hdb_tile_index(t, a.tile_stride) * 16;
        const int64_t rowg = row0 + 4 * h;
        // C register j of lane (rl, h) = row 4 h + j of the tile x query rl
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
        hdb_f8_tile_finish<MODE, METRIC, HAS_BIAS, false>(a, acc, aux0, t, h, rowg, n_rows, q_ok, ql, qinv_l, qsq_l, thr_cmp, 0);
        if constexpr (AHEAD) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) { raw[j] = nraw[j]; sw[j] = nsw[j]; }
        }
    }
}

// (the grid and the launch are the float8 register kernel's: launch_reg_kernel, hdb_mfma_f8.h)
template <int D>
static int launch_f4(const ScanArgs& a, const MfmaLaunch& l) {
    // 16-byte block loads: base and pitch; a mask arrives folded into the bias
    static_assert(HdbF4Row<D>::pitch % 16 == 0 && (D / 2) % 64 == 0, "16-byte blocks, aligned scale words");
    if ((reinterpret_cast<uintptr_t>(a.V) & 15) != 0 || a.d != D || hdb_row_bytes(HDB_MXF4, a.d) != HdbF4Row<D>::pitch || a.mask || a.n < 1 || l.blocks < 1)
        return (int)hipErrorNotSupported;
    return hdb_mode_ladder<1, 0>(a, l.mode, l.sqnorm, [&](auto mode, auto metric, auto bias, const float* aux0) {
        return launch_reg_kernel(hdb_mfma_f4_kernel<D, mode.value, metric.value, bias.value != 0>, a, l, aux0);
    });
}

// The euclidean re-score of the matrix-core scan (hdb_rescore_euclid_kernel, hdb_mfma.hip) for MXFP4 rows: candidates whose squared
// distance is below 5 % of ||q||^2 are re-scored from the stored row with the direct difference.  One wave per entry; lane l widens
// the MX blocks l, l + 64 .. of the row with the conversion the VALU scan uses (block load, scale byte, v_cvt_scalef32_pk_f32_fp4)
// and sums (v - q)^2 in float32; the lanes' sums are added by the butterfly of the other row types.
template <bool HAS_BIAS>
__global__ __launch_bounds__(256) void hdb_rescore_euclid_f4_kernel(unsigned long long* cand, const uint32_t* cnt, uint32_t cap, const char* V, int d,
                                                                    int pitch, const float* Q, const float* qsq, int q0, const float* bias) {
    typedef float f2_t __attribute__((ext_vector_type(2)));
    const int ql = blockIdx.y, lane = threadIdx.x & 63;
    const uint32_t n = cnt[ql * HDB_CNT_STRIDE] < cap ? cnt[ql * HDB_CNT_STRIDE] : cap;
    const float* qv = Q + (int64_t)(q0 + ql) * d;
    const float close2 = 0.05f * qsq[q0 + ql];
    const int nblk = d >> 5;
    for (uint32_t e = blockIdx.x * 4 + (threadIdx.x >> 6); e < n; e += gridDim.x * 4) {
        const unsigned long long ent = cand[(int64_t)ql * cap + e];
        const uint32_t row = 0xFFFFFFFFu - (uint32_t)(ent & 0xFFFFFFFFull);
        float s = hdb_key2f((uint32_t)(ent >> 32));
        const float b = HAS_BIAS ? bias[row] : 0.f;
        const float sim = s - b;                                   // 1 / (1 + dist) in (0, 1]; -inf for an excluded row
        const float dist = 1.f / sim - 1.f;
        if (sim > 0.f && dist * dist < close2) {                   // wave-uniform: one entry per wave
            const char* p = V + (int64_t)row * pitch;
            float acc = 0.f;
            for (int c = lane; c < nblk; c += 64) {
                const uint4 raw = *reinterpret_cast<const uint4*>(p + 16 * c);
                const float scale = hdb_mxf4_scale_f(*reinterpret_cast<const uint8_t*>(p + (d >> 1) + c));
                const uint32_t word[4] = {raw.x, raw.y, raw.z, raw.w};
                const float2* qc = reinterpret_cast<const float2*>(qv + 32 * c);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f2_t x[4] = {__builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word[i], scale, 0), __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word[i], scale, 1),
                                       __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word[i], scale, 2), __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word[i], scale, 3)};
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float2 qe = qc[4 * i + u];
                        const float d0 = x[u][0] - qe.x, d1 = x[u][1] - qe.y;
                        acc = fmaf(d0, d0, acc);
                        acc = fmaf(d1, d1, acc);
                    }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
            s = hdb_canon(1.f / (1.f + sqrtf(acc)) + b);
            if (lane == 0) cand[(int64_t)ql * cap + e] = hdb_pack(s, row);
        }
    }
}
