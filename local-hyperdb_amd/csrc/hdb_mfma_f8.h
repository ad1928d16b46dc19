// hdb_mfma_f8.h -- float8 e4m3 rows (HDB_F8E4M3) on the bf16 matrix pipe: the kernel behind hdb_mfma_f8.hip / hdb_mfma_f8_b.hip.
//
// The arithmetic is the bfloat16 flavour's (MfmaShape<16, hdb_bf16>, hdb_mfma_kernel.h): a float32 query travels as three bf16 parts that
// add up to it exactly (hdb_split3_finite, built once per launch), a row element is ONE bf16 -- a float8 code has four significant
// bits, so the upper half of its float32 widening is the value itself -- and a k-step of 32 elements is three
// v_mfma_f32_16x16x32_bf16, v p2 + v p1 + v p0, every product exact, float32 accumulation.  Fragment map, K walk (k-steps in order,
// smallest part first) and epilogue are that flavour's, so the scores equal those of a bfloat16 index over the widened matrix bit
// for bit.
//
// What differs is how the rows reach the A fragments: CONVERTED PER FRAGMENT IN REGISTERS, and read straight from global memory.
// Lane (rl = lane & 15, h = lane >> 4) of a wave owns the k slots 32 s + 8 h .. + 7 of row rl of its 16-row tile: eight bytes, one
// 8-byte load per k-step (the four lanes of a row read 32 contiguous bytes, the wave's D / 32 loads cover whole rows), four
// v_cvt_pk_f32_fp8 and four v_perm to pack the upper halves.  All D / 32 loads of a tile are issued before the first conversion.
// There is no LDS ring: a 256-thread workgroup is `wq` query groups of 16 queries x 4 / wq tile lanes, the waves that share a tile
// issue the same addresses together and meet in L1 / L2.  A one-byte row of 128 or 384 bytes is no multiple of the 256 bytes the
// ring's XOR swizzle works on, which is why the bfloat16 kernel's staging was not instantiated for it.
// MODE 0 = store the scores (row sample, exact path), MODE 1 = filter against a.thr into the candidate lists (one returning atomic per
// survivor: ~2 k survivors per query and pass).  METRIC: 0 dot, 1 cosine (aux0 = 1/||v|| or pearson's row scale), 2 euclidean
// similarity through ||v||^2 + ||q||^2 - 2 v.q (aux0 = ||v||^2; near-duplicates are re-scored by hdb_rescore_euclid_kernel).
// Tiles are 16 rows (hdb_mfma_tile_rows): a.ntiles / a.tile_stride count 16-row tiles, as for the VALU scan.
// KSL: the launch covers ONE K slice of D elements of rows that are wider (hdb_mfma_ksplit.hip, ks_geom_f8; opt-in, f8_ks_min_q): rows
// at pitch a.ks_pitch from byte a.ks_off, the query at pitch a.ks_dfull from element a.ks_off (one byte per element: the same number),
// accumulators started from a.ks_partial_in (nullptr = zero) and, MODE 3, stored raw to a.ks_partial_out for the next slice; the last
// slice runs the epilogue, MODE 0 / 1.  The sums are indexed like MODE 0's scores -- [query][compact tile sequence x 16 + row], pitch
// a.ks_ld -- which is the bfloat16 slice kernel's layout (hdb_mfma_kernel.h); a lane reads the four elements it later writes, so the
// two buffers and MODE 0's scores may alias.  With ks_geom_bf16's slice list the K walk is that kernel's, partial sum by partial sum.
#pragma once
#include "hdb_mfma_kernel.h"

__device__ __forceinline__ u32x4 hdb_f8x8_to_bf16x8(const uint2& raw) {
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw.x, true);
    const f32x2_t c = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw.y, false), e = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw.y, true);
    u32x4 o;        // element 2 j in the low half of word j (the order hdb_split3_finite packs the query parts in)
    o[0] = __builtin_amdgcn_perm(hdb_fbits(a[1]), hdb_fbits(a[0]), 0x07060302u);
    o[1] = __builtin_amdgcn_perm(hdb_fbits(b[1]), hdb_fbits(b[0]), 0x07060302u);
    o[2] = __builtin_amdgcn_perm(hdb_fbits(c[1]), hdb_fbits(c[0]), 0x07060302u);
    o[3] = __builtin_amdgcn_perm(hdb_fbits(e[1]), hdb_fbits(e[0]), 0x07060302u);
    return o;
}

// int8 rows (HDB_I8, hdb_mfma_i8.hip): eight signed bytes -> eight bf16, element 2 j in the low half of word j.  |x| <= 128 has at
// most 8 significant bits, so the upper half of the float32 widening is the value itself: one v_cvt_f32_i32 with a sign-extending
// byte select per element (hdb_i8_cvt) and one v_perm per pair -- 12 instructions per 8 bytes against float8's 8, and fewer than
// the 2 v_xor + 8 v_cvt_f32_ubyteN + 8 v_sub_f32 + 4 v_perm of the unsigned recipe.
__device__ __forceinline__ u32x4 hdb_i8x8_to_bf16x8(const uint2& raw) {
    const int lo = (int)raw.x, hi = (int)raw.y;
    u32x4 o;
    o[0] = __builtin_amdgcn_perm(hdb_fbits(hdb_i8_cvt<1>(lo)), hdb_fbits(hdb_i8_cvt<0>(lo)), 0x07060302u);
    o[1] = __builtin_amdgcn_perm(hdb_fbits(hdb_i8_cvt<3>(lo)), hdb_fbits(hdb_i8_cvt<2>(lo)), 0x07060302u);
    o[2] = __builtin_amdgcn_perm(hdb_fbits(hdb_i8_cvt<1>(hi)), hdb_fbits(hdb_i8_cvt<0>(hi)), 0x07060302u);
    o[3] = __builtin_amdgcn_perm(hdb_fbits(hdb_i8_cvt<3>(hi)), hdb_fbits(hdb_i8_cvt<2>(hi)), 0x07060302u);
    return o;
}
// The row converter of hdb_mfma_f8_kernel, a compile-time parameter: eight stored bytes -> the A fragment's eight bf16.  Everything
// else of the kernel -- fragment map, K walk, epilogue, grid, the wq rule -- is shared; the float8 instantiations take the default
// and compile to what they were.
struct HdbRowCvtF8 { static __device__ __forceinline__ u32x4 to_bf16x8(const uint2& raw) { return hdb_f8x8_to_bf16x8(raw); } };
struct HdbRowCvtI8 { static __device__ __forceinline__ u32x4 to_bf16x8(const uint2& raw) { return hdb_i8x8_to_bf16x8(raw); } };

// What the register kernel below and the LDS kernel (hdb_mfma_f8_lds.h) do with a tile's accumulator, in ONE place so that the two
// cannot drift: lane (rl, h) holds rows rowg = row0 + 4 h .. + 3 of tile sequence number t against query rl.
// ... its start: zero, or the sums of the K slices before this one
template <bool KSL>
__device__ __forceinline__ f32x4 hdb_f8_acc_start(const ScanArgs& a, bool q_ok, int64_t ks_at, int64_t rowg, int64_t n_rows) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if constexpr (KSL) {
        if (a.ks_partial_in && q_ok) {           // the sums of the slices before this one
            const float* pin = a.ks_partial_in + ks_at;
            if (rowg + 3 < n_rows) { const float4 pv = *reinterpret_cast<const float4*>(pin); acc[0] = pv.x; acc[1] = pv.y; acc[2] = pv.z; acc[3] = pv.w; }
            else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (rowg + j < n_rows) acc[j] = pin[j];
            }
        }
    }
    return acc;
}
// ... and its end: MODE 3 stores the raw sums for the next slice, MODE 0 / 1 run the metric's epilogue and store or filter
template <int MODE, int METRIC, bool HAS_BIAS, bool KSL>
__device__ __forceinline__ void hdb_f8_tile_finish(const ScanArgs& a, const f32x4& acc, const float* __restrict__ aux0, int64_t t, int h, int64_t rowg,
                                                   int64_t n_rows, bool q_ok, int ql, float qinv_l, float qsq_l, float thr_cmp, int64_t ks_at) {
    constexpr bool FILT = MODE == 1;
    if constexpr (MODE == 3) {                   // raw partial sums for the next K slice
        if (q_ok) {
            float* pout = a.ks_partial_out + ks_at;
            if (rowg + 3 < n_rows) *reinterpret_cast<float4*>(pout) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (rowg + j < n_rows) pout[j] = acc[j];
            }
        }
        return;
    }
    // epilogue: the bfloat16 flavour's arithmetic, term by term
    float x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t rr = min(rowg + j, n_rows - 1);
        const float aj = METRIC != 0 ? aux0[rr] : 1.f;
        const float bj = HAS_BIAS ? a.bias[rr] : 0.f;
        const float dot = acc[j];
        if (METRIC != 0 || HAS_BIAS || MODE == 0) {
            if (METRIC == 0) x[j] = HAS_BIAS ? fmaf(dot, qinv_l, bj) : dot * qinv_l;
            else if (METRIC == 1) {
                if (FILT && !HAS_BIAS) x[j] = dot * aj;
                else x[j] = HAS_BIAS ? fmaf(dot * aj, qinv_l, bj) : dot * aj * qinv_l;
            } else {
                const float d2 = fmaxf(fmaf(-2.f * qinv_l, dot, aj + qsq_l), 0.f);
                x[j] = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_sqrtf(d2)) + (HAS_BIAS ? bj : 0.f);
            }
        } else x[j] = dot;
    }
    if (MODE == 0) {
        if (q_ok) {
            float* dst = a.scores + (int64_t)ql * a.ld + (t * 16 + 4 * h);          // sample passes store compactly
#pragma unroll
            for (int j = 0; j < 4; ++j) if (rowg + j < n_rows) dst[j] = hdb_canon(x[j]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool hit = x[j] >= thr_cmp && rowg + j < n_rows && !(HAS_BIAS && x[j] == -INFINITY);      // bias -inf = masked row
            if (hit) {
                const float sc = hdb_canon((METRIC != 2 && !HAS_BIAS) ? x[j] * qinv_l : x[j]);
                const uint32_t pos = atomicAdd(&a.cnt[ql * HDB_CNT_STRIDE], 1u);
                if (pos < a.cap) a.cand[(int64_t)ql * a.cap + pos] = hdb_pack(sc, (uint32_t)(rowg + j));
            }
        }
    }
}

// (the filter flavour of a 512-element slice holds 192 registers of query parts, 32 of raw row bytes, the partial sums and the slice
//  addressing: left alone it takes 254-256 VGPRs plus 4 AGPRs for the accumulator -- 264 allocated, one wave per SIMD.  Asked for two
//  workgroups per CU it keeps the accumulator in the 256 VGPRs, without scratch: two waves per SIMD like the other 512-element kernels)
template <int D, int MODE, int METRIC, bool HAS_BIAS, bool KSL = false, typename CVT = HdbRowCvtF8>
__global__ __launch_bounds__(256, (KSL && D == 512 && MODE == 1) ? 2 : 1) void hdb_mfma_f8_kernel(ScanArgs a, const float* __restrict__ Qf, const float* __restrict__ aux0,
                                                          const float* __restrict__ qsq, int nq_end, int wq) {
    static_assert(D % 32 == 0 && (MODE == 0 || MODE == 1 || (KSL && MODE == 3 && METRIC == 0 && !HAS_BIAS)), "whole k-steps; MODE 0 / 1, a K slice also 3");
    constexpr int KS = D / 32;
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
    HdbParts3 Bq[KS];
    {
        const float4* qf = reinterpret_cast<const float4*>(KSL ? Qf + (int64_t)qq * a.ks_dfull + a.ks_off : Qf + (int64_t)qq * D) + 2 * h;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            float4 x0 = qf[8 * s], x1 = qf[8 * s + 1];
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
    const int64_t pitch = KSL ? a.ks_pitch : (int64_t)D;
    for (int64_t t = (int64_t)blockIdx.x * ntl + tl; t < a.ntiles; t += (int64_t)gridDim.x * ntl) {
        const int64_t row0 = hdb_tile_index(t, a.tile_stride) * 16;
        const int64_t ra = min(row0 + rl, n_rows - 1);                         // (a ragged last tile re-reads the last row)
        const uint2* src = reinterpret_cast<const uint2*>(Vb + ra * pitch + (KSL ? a.ks_off : 0)) + h;
        uint2 raw[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) raw[s] = src[4 * s];            // (cached: the waves that share the tile find it in L1 / L2)
        const int64_t rowg = row0 + 4 * h;
        // C register j of lane (rl, h) = row 4 h + j of the tile x query rl; a K slice keeps it at [query][t * 16 + 4 h + j]
        const int64_t ks_at = KSL ? (int64_t)(q_ok ? ql : 0) * a.ks_ld + (t * 16 + 4 * h) : 0;
        f32x4 acc = hdb_f8_acc_start<KSL>(a, q_ok, ks_at, rowg, n_rows);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const u32x4 av = CVT::to_bf16x8(raw[s]);
#define HDB_BF(x) __builtin_bit_cast(hdb_bf16x8, x)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(HDB_BF(av), HDB_BF(Bq[s].p2), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(HDB_BF(av), HDB_BF(Bq[s].p1), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(HDB_BF(av), HDB_BF(Bq[s].p0), acc, 0, 0, 0);
#undef HDB_BF
        }
        hdb_f8_tile_finish<MODE, METRIC, HAS_BIAS, KSL>(a, acc, aux0, t, h, rowg, n_rows, q_ok, ql, qinv_l, qsq_l, thr_cmp, ks_at);
    }
}

// One launch of a register kernel -- this one, its int8 flavour, the packed-bit one (hdb_mfma_b1.h): the same arguments and the
// same grid, (workgroups, query-group rows) with wq query groups per workgroup; the other waves take further tiles
template <typename K>
static int launch_reg_kernel(K kern, const ScanArgs& a, const MfmaLaunch& l, const float* aux0) {
    const int tq = (l.nq_launch + 15) / 16;
    const int wq = tq <= 1 ? 1 : tq <= 2 ? 2 : 4;
    const dim3 grid(l.blocks, (tq + wq - 1) / wq);
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, (hipStream_t)l.stream, a, (const float*)l.q, aux0, l.qsq, a.q0 + l.nq_launch, wq);
    return (int)hipGetLastError();
}
template <int D, typename CVT = HdbRowCvtF8>
static int launch_f8(const ScanArgs& a, const MfmaLaunch& l) {
    if ((reinterpret_cast<uintptr_t>(a.V) & 7) != 0 || a.d != D || a.mask) return (int)hipErrorNotSupported;      // 8-byte fragment loads; a mask arrives folded into the bias
    return hdb_mode_ladder<1, 0>(a, l.mode, l.sqnorm, [&](auto mode, auto metric, auto bias, const float* aux0) {
        return launch_reg_kernel(hdb_mfma_f8_kernel<D, mode.value, metric.value, bias.value != 0, false, CVT>, a, l, aux0);
    });
}
// One K slice of a wide float8 row (hdb_mfma_ksplit.hip): mode 3 = raw partial sums out, 0 / 1 = the last slice with the metric's epilogue
template <int D>
static int launch_f8_kslice(const ScanArgs& a, const MfmaLaunch& l) {
    // 8-byte fragment loads: base, pitch and slice offset; float4 query and partial-sum accesses; the slice lies inside the row
    if ((reinterpret_cast<uintptr_t>(a.V) & 7) != 0 || (a.ks_pitch & 7) != 0 || (a.ks_off & 7) != 0 || a.ks_off < 0 || a.ks_off + D > a.ks_pitch ||
        a.ks_dfull != a.ks_pitch || (a.ks_ld & 3) != 0 || a.mask) return (int)hipErrorNotSupported;
    if ((reinterpret_cast<uintptr_t>(a.ks_partial_in) & 15) != 0 || (reinterpret_cast<uintptr_t>(a.ks_partial_out) & 15) != 0 || (l.mode == 3 && !a.ks_partial_out)) return (int)hipErrorNotSupported;
    return hdb_mode_ladder<1, 0, 3>(a, l.mode, l.sqnorm, [&](auto mode, auto metric, auto bias, const float* aux0) {
        return launch_reg_kernel(hdb_mfma_f8_kernel<D, mode.value, metric.value, bias.value != 0, true>, a, l, aux0);
    });
}
