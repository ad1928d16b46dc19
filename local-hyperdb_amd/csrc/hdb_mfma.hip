// hdb_mfma.hip -- the Q.V^T row scan of fp16 matrices on the gfx950 matrix cores (fp32 accumulate), 1..256 queries
// per pass over V.
//
// Replaces "np.dot(vectors, query.T)" (hyperdb/ranking_algorithm.py:29,:41) and, through
// ||v-q||^2 = ||v||^2 + ||q||^2 - 2 v.q, "np.linalg.norm(vectors - query, axis=1)" (:49).  The reference takes one
// query per call; here up to 8*MF*QT queries ride on ONE pass over V, and a single query takes the same kernel (one
// wave multiplies, the kernel is then a pure HBM streaming kernel: 6.9-7.1 TB/s at N=10M, d=384).
//
// Work decomposition (one workgroup = 8 waves = 512 threads, one workgroup per CU, persistent):
//   * wave w owns MF*QT queries of the batch (MF = 16: v_mfma_f32_16x16x32_f16, QT = 1 or 2 query tiles per wave;
//     MF = 32: v_mfma_f32_32x32x16_f16, kept for A/B runs); their scaled fp16 values (hdb_q16_scale) for ALL k
//     live in its registers as MFMA B fragments (QT*d/8 VGPRs for MF=16), loaded once;
//   * the workgroup streams tiles of R rows of V through a 3-deep LDS ring filled by LDS-DMA
//     (global_load_lds_dwordx4, 1 KiB per wave-instruction, source-side XOR swizzle so that the
//     lane-linear LDS image is bank-conflict-free for the ds_read_b128 A-fragment reads), together with
//     the per-row aux values (1/||v|| or ||v||^2, bias);
//   * every wave multiplies the whole tile by its queries, one ds_read_b128 per QT MFMAs, issued 2-3 k-steps
//     ahead from inline asm with counted lgkmcnt waits; accumulators never leave registers;
//   * epilogue in registers: scale / bias / threshold compare behind a group-max prefilter; survivors go
//     to a wave-private segment of a small LDS list (slot = running count + ballot rank, no atomic), which each wave
//     empties into the per-query candidate lists with global atomics when it fills.  The N x Q score matrix is never
//     written (10 GB at N=10M, Q=256).
// Synchronisation: one raw s_barrier per tile; tile t+2 is in flight while tile t is multiplied (counted
// s_waitcnt vmcnt, never 0 in the steady state).
// Algorithmic bytes per row: d*2 (V read exactly once per pass); FLOPs: 2*Q*d per row.
#include "hdb_mfma_kernel.h"

// fp32 -> scaled fp16 queries for the matrix pipe (hdb_q16_scale, hdb_common.h); qscl[q] = 1 / scale.  One wave per
// query.  The prep kernel does the same for plain queries; this one serves the centred copies of pearson.
__global__ __launch_bounds__(64) void hdb_q_to_f16_kernel(const float* Q, int nq, int d, _Float16* out, float* qscl) {
    const int q = blockIdx.x;
    if (q >= nq) return;
    float amax = 0.f;
    for (int e = threadIdx.x; e < d; e += 64) amax = fmaxf(amax, fabsf(Q[(int64_t)q * d + e]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    const float scale = hdb_q16_scale(amax);
    for (int e = threadIdx.x; e < d; e += 64) out[(int64_t)q * d + e] = (_Float16)(Q[(int64_t)q * d + e] * scale);
    if (threadIdx.x == 0) qscl[q] = 1.f / scale;
}

// Euclidean scores from the MFMA path come from ||v||^2 + ||q||^2 - 2 v.q, which cancels when v ~ q (an exact
// duplicate scores 1/(1+~0.01) instead of 1).  Candidates whose squared distance is below 5 % of ||q||^2 -- where
// the rounding of the expansion, ~1e-6 (||v||^2 + ||q||^2), exceeds 4e-5 of the distance itself -- are re-scored
// from the stored row with the direct difference, like the reference (:49); beyond that the expansion is good to
// 5e-6 in the similarity.  One wave per entry.
__device__ __forceinline__ float hdb_row_f(_Float16 v) { return (float)v; }
__device__ __forceinline__ float hdb_row_f(float v) { return v; }
__device__ __forceinline__ float hdb_row_f(hdb_bf16 v) { return hdb_bf16_to_f(v); }
__device__ __forceinline__ float hdb_row_f(hdb_f8 v) { return __builtin_amdgcn_cvt_f32_fp8((int)v.bits, 0); }
__device__ __forceinline__ float hdb_row_f(hdb_i8 v) { return hdb_i8_to_f(v); }
// element k of a stored row; packed bits (HdbB1Word rows of d / 32 words, element e = bit e & 31 of word e >> 5) yield 0.f / 1.f
struct HdbB1Word { uint32_t w; };
template <typename T>
__device__ __forceinline__ float hdb_row_at(const T* V, uint32_t row, int d, int k) { return hdb_row_f(V[(int64_t)row * d + k]); }
__device__ __forceinline__ float hdb_row_at(const HdbB1Word* V, uint32_t row, int d, int k) {
    return (float)((V[(int64_t)row * (d >> 5) + (k >> 5)].w >> (k & 31)) & 1u);
}
template <typename T, bool HAS_BIAS>
__global__ __launch_bounds__(256) void hdb_rescore_euclid_kernel(unsigned long long* cand, const uint32_t* cnt, uint32_t cap,
                                                                 const T* V, int d, const float* Q, const float* qsq, int q0,
                                                                 const float* bias) {
    const int ql = blockIdx.y, lane = threadIdx.x & 63;
    const uint32_t n = cnt[ql * HDB_CNT_STRIDE] < cap ? cnt[ql * HDB_CNT_STRIDE] : cap;
    const float* qv = Q + (int64_t)(q0 + ql) * d;
    const float close2 = 0.05f * qsq[q0 + ql];
    for (uint32_t e = blockIdx.x * 4 + (threadIdx.x >> 6); e < n; e += gridDim.x * 4) {
        const unsigned long long ent = cand[(int64_t)ql * cap + e];
        const uint32_t row = 0xFFFFFFFFu - (uint32_t)(ent & 0xFFFFFFFFull);
        float s = hdb_key2f((uint32_t)(ent >> 32));
        const float b = HAS_BIAS ? bias[row] : 0.f;
        const float sim = s - b;                                   // 1 / (1 + dist) in (0, 1]; -inf for an excluded row
        const float dist = 1.f / sim - 1.f;
        if (sim > 0.f && dist * dist < close2) {                   // wave-uniform: one entry per wave
            float acc = 0.f;
            for (int k = lane; k < d; k += 64) { const float df = hdb_row_at(V, row, d, k) - qv[k]; acc += df * df; }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
            s = hdb_canon(1.f / (1.f + sqrtf(acc)) + b);
            if (lane == 0) cand[(int64_t)ql * cap + e] = hdb_pack(s, row);
        }
    }
}

// bytes of the control block of the single-launch batched call for a grid of `wgs` workgroups
extern "C" size_t hdb_mfma_batch_ctl_bytes(int wgs) { return (size_t)HDB_BATCH_GRAN_BYTE + (size_t)HDB_BATCH_MAXQ * (size_t)wgs * 8 * 8; }

// d=384, more than 128 queries: 16 = 16x16x32 with two query tiles per wave (default: the same FLOPs and LDS
// traffic as the 32x32x16 form, but the chip holds a higher clock on this shape: 1.78-1.85 ms against 2.07-2.25 ms
// for N=10M, Q=256), 32 = 32x32x16 with one query tile per wave (kept for A/B measurements).
// (per index: hdb_set_option(ix, "mfma_variant", 16 | 32), passed down as `variant`)

// The router: picks the shard and hands it the scan and ONE launch record (MfmaLaunch, hdb_common.h); every shard has the same
// signature and reads what it needs.  The grids are rules of hdb_caps.h or the few lines below.
// a.ntiles / a.tile_stride are in units of hdb_mfma_tile_rows(dtype, d) rows here.  q: the query fragments' source --
// scaled fp16 copies (+ qscl) for fp16 matrices, the float32 queries themselves for every other row type (the record's qscl is nullptr).
// mode 2 = the whole call in one launch (hdb_mfma_kernel.h): f != nullptr, nq_launch <= hdb_mfma_batch_capacity(), grid = one
// workgroup per CU at most (the in-kernel exchange needs the grid co-resident)
extern "C" int hdb_launch_mfma_scan(const ScanArgs* args, int dtype, int mode, int nq_launch, const void* q16, const float* sqnorm,
                                    const float* qsq, const float* qscl, int max_blocks, int variant, void* stream, const BatchArgs* f) {
    const int g_mfma_variant = variant == 32 ? 32 : variant == 64 ? 64 : 16;
    const ScanArgs& a = *args;
    if (a.mask) return (int)hipErrorNotSupported;
    const int cus = hdb_cu_count();                      // one persistent workgroup per CU ...
    // ... or, with max_blocks < 0, -max_blocks workgroups per CU: the hardware dispatcher then hands the next workgroup
    // to whichever CU finishes first (CUs differ by up to 40 % in streaming speed, see hdb_mfma_fused.h)
    const int64_t want = max_blocks < 0 ? (int64_t)cus * (-max_blocks) : cus;
    int blocks = (int)(a.ntiles < want ? a.ntiles : want);
    if (max_blocks > 0 && max_blocks < blocks) blocks = max_blocks;
    if (blocks < 1) blocks = 1;
    if (mode == 2 && blocks > cus) blocks = cus;
    MfmaLaunch l = {mode, nq_launch, q16, sqnorm, qsq, dtype == HDB_F16 ? qscl : nullptr, blocks, g_mfma_variant, 0, stream, f};
    if (hdb_mfma_ksplit_slices(dtype, a.d) > 0) return mode == 2 ? (int)hipErrorNotSupported : hdb_launch_mfma_ksplit(args, dtype, &l);
    if (const int pad = hdb_mfma_anyd_pad(dtype, a.d)) {               // a width without a geometry of its own: one slice of the next wider one
        if (mode == 2) return (int)hipErrorNotSupported;
        l.width = pad;
        if (dtype == HDB_F16) return pad <= 384 ? hdb_launch_mfma_anyd_a(args, &l) : hdb_launch_mfma_anyd_b(args, &l);
        if (a.f32_split) return pad <= 384 ? hdb_launch_mfma_anyd_e(args, &l) : hdb_launch_mfma_anyd_f(args, &l);
        return pad <= 384 ? hdb_launch_mfma_anyd_c(args, &l) : hdb_launch_mfma_anyd_d(args, &l);
    }
    if (dtype == HDB_F32) return (a.f32_split > 0 && hdb_mfma_f32_split_min_q(a.d) > 0) ? hdb_launch_mfma_scan_f32s(args, &l) : hdb_launch_mfma_scan_f32(args, &l);
    if (dtype == HDB_F8E4M3 || dtype == HDB_I8 || dtype == HDB_B1) {
        // one-byte and packed-bit rows: the register kernels (hdb_mfma_f8.h; int8 with another row converter, hdb_mfma_i8.hip; packed
        // bits when the plan asked, b1_mfma_min_q, hdb_mfma_b1.h) -- no LDS ring and 16-row tiles, a wave per tile, hdb_mfma_reg_blocks
        if (mode == 2) return (int)hipErrorNotSupported;
        l.blocks = hdb_mfma_reg_blocks(a.ntiles, cus, max_blocks);
        if (dtype == HDB_I8) return hdb_launch_mfma_scan_i8(args, &l);
        if (dtype == HDB_B1) return hdb_mfma_b1_ks_slices(a.d) > 0 ? hdb_launch_mfma_ksplit(args, dtype, &l) : hdb_launch_mfma_scan_b1(args, &l);
        // float8 with the rows expanded in LDS once per workgroup (the plan asked, f8_lds_min_q, hdb_mfma_f8_lds.h): a grid of stages,
        // one or two workgroups per CU at most; every launcher takes min(its stages, this limit)
        if (a.f8_lds) l.blocks = max_blocks > 0 ? max_blocks : hdb_mfma_f8_lds_wg_per_cu(a.d, a.f8_lds) * cus;
        // rows wider than 512 elements: the plan asked for K slices (f8_ks_min_q) -- it alone hands such a call a partial-sum buffer
        if (a.ks_partial_out && hdb_mfma_f8_ks_slices(a.d) > 0) return hdb_launch_mfma_ksplit(args, dtype, &l);
        return a.f8_lds ? hdb_launch_mfma_scan_f8_lds(args, &l) : hdb_launch_mfma_scan_f8(args, &l);
    }
    if (dtype == HDB_BF16) return mode == 2 ? (int)hipErrorNotSupported : hdb_launch_mfma_scan_bf16(args, &l);
    if (dtype != HDB_F16) return (int)hipErrorNotSupported;
    // (mode 2 promises hdb_mfma_batch_capacity() queries in ONE launch: only the two-tile launcher holds more than 128, whatever the variant)
    if (nq_launch > 128 && hdb_mfma_qt2_supported(a.d) && (g_mfma_variant != 32 || (mode == 2 && a.d != 384))) return hdb_launch_mfma_scan_f16_qt2(args, &l);
    switch (a.d) {
        case 128: case 256: return hdb_launch_mfma_scan_f16_narrow(args, &l);
        case 384: return hdb_launch_mfma_scan_f16_d384(args, &l);
        case 512: case 640: case 768: return hdb_launch_mfma_scan_f16_mid(args, &l);
        case 1024: case 1536: return hdb_launch_mfma_scan_f16_1k(args, &l);
        default: return hdb_launch_mfma_scan_f16_wide(args, &l);     // 896, 1152, 1280, 1408
    }
}

extern "C" int hdb_launch_q_to_f16(const float* Q, int nq, int d, void* q16, float* qscl, void* stream) {
    hipLaunchKernelGGL(hdb_q_to_f16_kernel, dim3(nq), dim3(64), 0, (hipStream_t)stream, Q, nq, d, (_Float16*)q16, qscl);
    return (int)hipGetLastError();
}

// one row type of the re-score: the bias flavour, the launch
template <typename T>
static int launch_rescore_euclid(unsigned long long* cand, const uint32_t* cnt, uint32_t cap, int nq_launch, const void* V, int d, const float* Q,
                                 const float* qsq, int q0, const float* bias, void* stream) {
    auto kern = bias ? hdb_rescore_euclid_kernel<T, true> : hdb_rescore_euclid_kernel<T, false>;
    hipLaunchKernelGGL(kern, dim3(64, nq_launch), dim3(256), 0, (hipStream_t)stream, cand, cnt, cap, (const T*)V, d, Q, qsq, q0, bias);
    return (int)hipGetLastError();
}
extern "C" int hdb_launch_rescore_euclid(unsigned long long* cand, const uint32_t* cnt, uint32_t cap, int nq_launch, const void* V,
                                         int dtype, int d, const float* Q, const float* qsq, int q0, const float* bias, void* stream) {
    switch (dtype) {                    // (the dtypes of the matrix-core scan)
        case HDB_B1: return launch_rescore_euclid<HdbB1Word>(cand, cnt, cap, nq_launch, V, d, Q, qsq, q0, bias, stream);
        case HDB_I8: return launch_rescore_euclid<hdb_i8>(cand, cnt, cap, nq_launch, V, d, Q, qsq, q0, bias, stream);
        case HDB_F8E4M3: return launch_rescore_euclid<hdb_f8>(cand, cnt, cap, nq_launch, V, d, Q, qsq, q0, bias, stream);
        case HDB_F16: return launch_rescore_euclid<_Float16>(cand, cnt, cap, nq_launch, V, d, Q, qsq, q0, bias, stream);
        case HDB_BF16: return launch_rescore_euclid<hdb_bf16>(cand, cnt, cap, nq_launch, V, d, Q, qsq, q0, bias, stream);
        case HDB_F32: return launch_rescore_euclid<float>(cand, cnt, cap, nq_launch, V, d, Q, qsq, q0, bias, stream);
        default: return (int)hipErrorNotSupported;
    }
}
