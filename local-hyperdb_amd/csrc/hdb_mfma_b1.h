// hdb_mfma_b1.h -- packed-bit rows (HDB_B1) on the bf16 matrix pipe: the kernel behind hdb_mfma_b1*.hip (opt-in, b1_mfma_min_q).
//
// The arithmetic is the float8 / int8 register kernel's (hdb_mfma_f8.h), which is the bfloat16 flavour's: a float32 query travels as
// three bf16 parts that add up to it exactly (hdb_split3_finite, built once per launch), a row element is ONE bf16 -- a bit is 0.0 or
// 1.0, 0x0000 or 0x3F80 -- and a k-step of 32 elements is three v_mfma_f32_16x16x32_bf16, v p2 + v p1 + v p0 on one accumulator,
// every product exact, float32 accumulation.  Fragment map, K walk and epilogue (hdb_f8_acc_start / hdb_f8_tile_finish, reused as
// they are) are that kernel's, so the scores of dot, cosine and euclidean equal those of a bfloat16 index over the unpacked 0/1
// matrix bit for bit; inv_norm / sqnorm already carry an int8 index's bits (hdb_b1_rownorm_kernel).
//
// What differs is how the rows reach the A fragments.  Lane (rl = lane & 15, h = lane >> 4) owns the k slots 32 s + 8 h .. + 7 of
// row rl of its 16-row tile.  The device holds the little bit order (element e = bit e & 31 of word e >> 5), so those eight elements
// are BYTE h of WORD s of the row: a lane loads the row's words (the four lanes of a row read the same words; 16-byte loads where
// the base is 16-byte aligned -- the row pitch D / 8 and every slice offset are multiples of 16 bytes by construction -- and 4-byte
// loads otherwise: hdb_index_create guarantees a packed matrix 4-byte alignment only, and the launcher refuses no such base),
// extracts its byte b and expands it arithmetically:
//     u = b | (b << 15)                       bit i of b at bits i and 15 + i
//     word_j = (u & (0x10001 << 2 j)) * (0x3F80 >> 2 j)     element 2 j in the low half, 2 j + 1 in the high half, j = 0 .. 3
// (the shift of ((u >> 2 j) & 0x10001) * 0x3F80 folded into the two constants: 0x3F80 = 0x7F << 7 shifts right by up to 6 bits
// exactly, the factors stay below 24 bits and the product below 32): one v_bfe, a shift and an or for u, and per word one and (or a
// v_bitop3 that takes the or with it) and one v_mul_u32_u24 -- 10-11 VALU instructions per k-step.
// The words of the next tile are loaded while the current one is multiplied (D >= 256).  No LDS and no barrier: a 256-thread
// workgroup is `wq` query groups of 16 queries x 4 / wq tile lanes, as in hdb_mfma_f8_kernel.
// MODE 0 = store the scores, MODE 1 = filter against a.thr, a K slice (KSL) also MODE 3 = raw partial sums for the next slice.
// KSL: the launch covers one K slice of D elements of rows that are wider (hdb_mfma_ksplit.hip, ks_geom_b1): rows at pitch
// a.ks_pitch BYTES from byte a.ks_off / 8, the query at pitch a.ks_dfull from ELEMENT a.ks_off; the partial sums use the float8
// slices' layout and workspace, [query][compact tile sequence x 16 + row], pitch a.ks_ld.
#pragma once
#include "hdb_mfma_f8.h"

// byte b (eight elements, element i = bit i) -> the A fragment's eight bf16, element 2 j in the low half of word j
__device__ __forceinline__ u32x4 hdb_b1x8_to_bf16x8(uint32_t b) {
    const uint32_t u = b | (b << 15);
    u32x4 o;
    o[0] = __umul24(u & 0x00010001u, 0x3F80u);          // bits 2 j and 16 + 2 j times 0x3F80 >> 2 j: 0x3F80 in either half, no carry
    o[1] = __umul24(u & 0x00040004u, 0x0FE0u);
    o[2] = __umul24(u & 0x00100010u, 0x03F8u);
    o[3] = __umul24(u & 0x00400040u, 0x00FEu);
    return o;
}

template <int D, int MODE, int METRIC, bool HAS_BIAS, bool KSL = false>
__global__ __launch_bounds__(256, (KSL && D == 512 && MODE == 1) ? 2 : 1) void hdb_mfma_b1_kernel(ScanArgs a, const float* __restrict__ Qf, const float* __restrict__ aux0,
                                                          const float* __restrict__ qsq, int nq_end, int wq) {
    static_assert(D % 128 == 0 && (MODE == 0 || MODE == 1 || (KSL && MODE == 3 && METRIC == 0 && !HAS_BIAS)), "whole 16-byte pieces of a row; MODE 0 / 1, a K slice also 3");
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
    const char* const Vb = reinterpret_cast<const char*>(a.V) + (KSL ? (a.ks_off >> 3) : 0);
    const int64_t n_rows = a.n;
    const int64_t pitch = KSL ? a.ks_pitch : (int64_t)(D / 8);
    // 16-byte loads where every row piece is 16-byte aligned (wave-uniform): the pitch and the slice offset are by construction, the base may not be
    const bool wide = ((reinterpret_cast<uintptr_t>(Vb) | (uintptr_t)pitch) & 15) == 0;
    const int sh = 8 * h;
    // the words of a lane's row of tile t (a ragged last tile re-reads the last row)
    auto load_tile = [&](int64_t t, uint32_t (&raw)[KS]) {
        const int64_t ra = min(hdb_tile_index(t, a.tile_stride) * 16 + rl, n_rows - 1);
        const char* src = Vb + ra * pitch;
        if (wide) {
#pragma unroll
            for (int s = 0; s < KS; s += 4) {
                const uint4 v = *reinterpret_cast<const uint4*>(src + 4 * s);
                raw[s] = v.x; raw[s + 1] = v.y; raw[s + 2] = v.z; raw[s + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int s = 0; s < KS; ++s) raw[s] = *reinterpret_cast<const uint32_t*>(src + 4 * s);
        }
    };
    // A tile is D / 32 registers of words, so the NEXT tile's loads are in flight while this one is expanded and multiplied (the last
    // step re-reads its own tile: t never leaves [0, ntiles)).  With two or three waves per SIMD and no LDS ring nothing else hides the
    // latency.  Not at D = 128: those kernels run four to six waves per SIMD without it and three with it, and measured slower with it.
    constexpr bool AHEAD = D > 128;
    const int64_t t_step = (int64_t)gridDim.x * ntl;
    int64_t t = (int64_t)blockIdx.x * ntl + tl;
    if (t >= a.ntiles) return;
    uint32_t raw[KS];
    if constexpr (AHEAD) load_tile(t, raw);
    for (; t < a.ntiles; t += t_step) {
        uint32_t nxt[KS];
        if constexpr (AHEAD) load_tile(min(t + t_step, a.ntiles - 1), nxt);
        else load_tile(t, raw);
        const int64_t row0 = hdb_tile_index(t, a.tile_stride) * 16;
        const int64_t rowg = row0 + 4 * h;
        // C register j of lane (rl, h) = row 4 h + j of the tile x query rl; a K slice keeps it at [query][t * 16 + 4 h + j]
        const int64_t ks_at = KSL ? (int64_t)(q_ok ? ql : 0) * a.ks_ld + (t * 16 + 4 * h) : 0;
        f32x4 acc = hdb_f8_acc_start<KSL>(a, q_ok, ks_at, rowg, n_rows);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const u32x4 av = hdb_b1x8_to_bf16x8(__builtin_amdgcn_ubfe(raw[s], (uint32_t)sh, 8u));
#define HDB_BF(x) __builtin_bit_cast(hdb_bf16x8, x)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(HDB_BF(av), HDB_BF(Bq[s].p2), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(HDB_BF(av), HDB_BF(Bq[s].p1), acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(HDB_BF(av), HDB_BF(Bq[s].p0), acc, 0, 0, 0);
#undef HDB_BF
        }
        hdb_f8_tile_finish<MODE, METRIC, HAS_BIAS, KSL>(a, acc, aux0, t, h, rowg, n_rows, q_ok, ql, qinv_l, qsq_l, thr_cmp, ks_at);
        if constexpr (AHEAD) {
#pragma unroll
            for (int s = 0; s < KS; ++s) raw[s] = nxt[s];
        }
    }
}

// (the grid and the launch are the float8 register kernel's: launch_reg_kernel, hdb_mfma_f8.h)
template <int D>
static int launch_b1(const ScanArgs& a, const MfmaLaunch& l) {
    // 4-byte row words (what hdb_index_create guarantees); a mask arrives folded into the bias
    if ((reinterpret_cast<uintptr_t>(a.V) & 3) != 0 || a.d != D || a.mask || a.n < 1 || l.blocks < 1) return (int)hipErrorNotSupported;
    return hdb_mode_ladder<1, 0>(a, l.mode, l.sqnorm, [&](auto mode, auto metric, auto bias, const float* aux0) {
        return launch_reg_kernel(hdb_mfma_b1_kernel<D, mode.value, metric.value, bias.value != 0, false>, a, l, aux0);
    });
}
// One K slice of a wide packed-bit row (hdb_mfma_ksplit.hip): mode 3 = raw partial sums out, 0 / 1 = the last slice with the metric's epilogue
template <int D>
static int launch_b1_kslice(const ScanArgs& a, const MfmaLaunch& l) {
    // 4-byte row words: base, pitch (bytes) and slice offset (elements: whole words); float4 query and partial-sum accesses; the slice lies inside the row
    if ((reinterpret_cast<uintptr_t>(a.V) & 3) != 0 || (a.ks_pitch & 3) != 0 || (a.ks_off & 31) != 0 || a.ks_off < 0 ||
        a.ks_off + D > a.ks_dfull || (int64_t)a.ks_dfull != a.ks_pitch * 8 || (a.ks_dfull & 3) != 0 || (a.ks_ld & 3) != 0 || a.mask || a.n < 1 || l.blocks < 1) return (int)hipErrorNotSupported;
    if ((reinterpret_cast<uintptr_t>(a.ks_partial_in) & 15) != 0 || (reinterpret_cast<uintptr_t>(a.ks_partial_out) & 15) != 0 || (l.mode == 3 && !a.ks_partial_out)) return (int)hipErrorNotSupported;
    return hdb_mode_ladder<1, 0, 3>(a, l.mode, l.sqnorm, [&](auto mode, auto metric, auto bias, const float* aux0) {
        return launch_reg_kernel(hdb_mfma_b1_kernel<D, mode.value, metric.value, bias.value != 0, true>, a, l, aux0);
    });
}
