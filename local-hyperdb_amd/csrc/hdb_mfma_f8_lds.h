// hdb_mfma_f8_lds.h -- float8 e4m3 rows (HDB_F8E4M3) on the bf16 matrix pipe, EXPANDED TO BF16 IN LDS ONCE PER WORKGROUP: the kernel
// behind hdb_mfma_f8_lds*.hip.  Opt-in (the planner's f8_lds_min_q; ScanArgs::f8_lds = waves per workgroup).
//
// The arithmetic and the bits are hdb_mfma_f8_kernel's (hdb_mfma_f8.h), which are the bfloat16 flavour's: the float32 query as three
// exact bf16 parts (hdb_split3_finite) in registers, one group of 16 queries per wave; lane (rl = lane & 15, h = lane >> 4) owns
// the k slots 32 s + 8 h .. + 7 of row rl of a 16-row tile; k-steps in order, p2, p1, p0 per step, float32 accumulation; the
// accumulator's start and end are that kernel's own functions (hdb_f8_acc_start, hdb_f8_tile_finish).  MODE, METRIC, HAS_BIAS and
// KSL (one K slice of a wider row: ks_pitch, ks_off, ks_dfull, ks_partial_in / _out, the alias rule) mean what they mean there.
//
// What differs is how the rows reach the A fragments.  That kernel converts every fragment in the wave that multiplies it, so a
// batch of 64 queries converts every row four times and a batch of 128 reads it twice as well.  Here a workgroup of NW = 4 or 8
// waves (blockDim.x / 64; d = 512: 4, hdb_caps.h) takes a STAGE of TR rows -- TR / 16 consecutive tile sequence numbers t, each with its own row0 =
// hdb_tile_index(t, tile_stride) x 16: a sample pass is strided, a stage is not contiguous in memory -- and
//   * loads it once, coalesced: thread i takes the 16-byte pieces g = i, i + NT, ... (CPT of them, hdb_mfma_f8_lds_chunks; piece g is
//     bytes 16 (g % (D / 16)) .. + 15 of stage row g / (D / 16)), so TR = CPT x NT x 16 / D (hdb_mfma_f8_lds_stage_rows);
//   * converts a piece with v_cvt_pk_f32_fp8 + v_perm (hdb_f8x8_to_bf16x8, twice) and writes the 32 bytes of bf16 to LDS;
//   * every wave reads its A fragments from that image, one 16-byte read per lane and k-step, and multiplies with its own queries.
// Two LDS buffers: the loads of stage i + 1 are issued into registers before stage i is multiplied, converted and stored after it;
// ONE barrier per stage (the buffer a stage is stored to was last read before the barrier that ended the stage before).
// Queries beyond 16 NW go to grid.y and read the matrix again.
//
// The LDS image and its banks.  Row r of a stage is 2 D bytes = D / 8 chunks of 16 bytes, chunk c = the k slots 8 c .. 8 c + 7 (what
// lane h of k-step s reads: c = 4 s + h); the pitch is a multiple of 256 bytes, so in a linear image chunk c of EVERY row lies on the
// same 16-byte slot of the 64 banks and the 16 lanes of a ds_read_b128 group would hit it 16 ways.  Chunk c of row r is therefore
// stored at chunk c ^ (r & 15) (the XOR stays inside the row's own 256-byte segment).  The groups of ds_read_b128 are {0-3, 12-15,
// 20-27}, {4-11, 16-19, 28-31} and the same + 32: eight lanes of one h and eight of the next, sixteen distinct rl.  With b = 4 s + h of
// the group's first half, its slots are b ^ {0-3, 12-15} and (b ^ 1) ^ {4-11} = b ^ {4-11} permuted (second group: b ^ {4-11} and
// (b ^ 1) ^ {0-3, 12-15}): all 16 slots, once each, at every k-step -- conflict-free.  The stores are ds_write_b128, eight contiguous
// lanes at a time over 32 banks: eight consecutive pieces of one row store their first halves to chunks (2 cc) ^ x, four distinct
// slots of the eight -- 2-way, 16 LDS cycles against the 13 the instruction's operand transfer takes anyway.
//
// Barriers: no wave leaves early.  A wave whose query group lies beyond nq_end loads, converts, stores and meets every barrier; it
// skips its multiplies and its stores to global memory.  The stage loop's trip count depends on blockIdx.x, gridDim.x, blockDim.x
// and a.ntiles only.  A ragged last stage re-reads the last tile, a ragged last tile the last row (n - 1); neither is multiplied.
#pragma once
#include "hdb_mfma_f8.h"

template <int D, int MODE, int METRIC, bool HAS_BIAS, bool KSL = false>
__global__ __launch_bounds__(D == 512 ? 256 : 512) void hdb_mfma_f8_lds_kernel(ScanArgs a, const float* __restrict__ Qf, const float* __restrict__ aux0,
                                                              const float* __restrict__ qsq, int nq_end) {
    static_assert(hdb_mfma_f8_lds_supported(D) && (MODE == 0 || MODE == 1 || (KSL && MODE == 3 && METRIC == 0 && !HAS_BIAS)), "128 / 256 / 384 / 512; MODE 0 / 1, a K slice also 3");
    constexpr int KS = D / 32, GC = D / 16, CPT = hdb_mfma_f8_lds_chunks(D), PITCH = 2 * D;
    constexpr bool FILT = MODE == 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char hdb_f8_stage[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rl = lane & 15, h = lane >> 4;
    const int tps = CPT * nt / GC / 16;                       // tiles per stage
    const int stage_bytes = tps * 16 * PITCH;
    const int qw0 = a.q0 + ((int)blockIdx.y * (nt >> 6) + w) * 16;
    const bool wave_on = qw0 < nq_end;                       // (wave-uniform; a wave without queries still stages and meets the barriers)
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
    const char* const Vb = reinterpret_cast<const char*>(a.V) + (KSL ? a.ks_off : 0);
    const int64_t n_rows = a.n;
    const int64_t pitch = KSL ? a.ks_pitch : (int64_t)D;
    const int64_t nstages = (a.ntiles + tps - 1) / tps;

    // the stage's pieces of this thread -> registers
    auto load_stage = [&](int64_t sg, uint4 (&raw)[CPT]) {
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
            const int g = tid + i * nt, r = g / GC, cc = g - r * GC;
            const int64_t t = min(sg * tps + (r >> 4), a.ntiles - 1);                      // (a ragged last stage re-reads the last tile)
            const int64_t ra = min(hdb_tile_index(t, a.tile_stride) * 16 + (r & 15), n_rows - 1);     // (a ragged last tile the last row)
            raw[i] = *reinterpret_cast<const uint4*>(Vb + ra * pitch + cc * 16);
        }
    };
    // ... -> bf16 -> the swizzled image at byte `buf` of the LDS
    auto store_stage = [&](int buf, const uint4 (&raw)[CPT]) {
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
            const int g = tid + i * nt, r = g / GC, cc = g - r * GC;
            const int at = buf + r * PITCH, x = r & 15;
            *reinterpret_cast<u32x4*>(hdb_f8_stage + at + (((2 * cc) ^ x) << 4)) = hdb_f8x8_to_bf16x8(make_uint2(raw[i].x, raw[i].y));
            *reinterpret_cast<u32x4*>(hdb_f8_stage + at + (((2 * cc + 1) ^ x) << 4)) = hdb_f8x8_to_bf16x8(make_uint2(raw[i].z, raw[i].w));
        }
    };
    // this wave's 16 queries x the stage's tiles.  Chunk 4 s + h of row rl lies at chunk (4 s + h) ^ rl = (4 s) ^ (h ^ rl): four
    // addresses, one per s & 3, and a constant 256 bytes per four k-steps
    const int hx = h ^ rl;
    auto multiply = [&](int buf, int64_t sg) {
        for (int j = 0; j < tps; ++j) {
            const int64_t t = sg * tps + j;
            if (t >= a.ntiles) break;
            const int64_t row0 = hdb_tile_index(t, a.tile_stride) * 16;
            const int64_t rowg = row0 + 4 * h;
            const int64_t ks_at = KSL ? (int64_t)(q_ok ? ql : 0) * a.ks_ld + (t * 16 + 4 * h) : 0;
            f32x4 acc = hdb_f8_acc_start<KSL>(a, q_ok, ks_at, rowg, n_rows);
            const int at = buf + (j * 16 + rl) * PITCH;
            const unsigned char* const ap[4] = {hdb_f8_stage + at + ((0 ^ hx) << 4), hdb_f8_stage + at + ((4 ^ hx) << 4),
                                                hdb_f8_stage + at + ((8 ^ hx) << 4), hdb_f8_stage + at + ((12 ^ hx) << 4)};
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const u32x4 av = *reinterpret_cast<const u32x4*>(ap[s & 3] + (s >> 2) * 256);
#define HDB_BF(x) __builtin_bit_cast(hdb_bf16x8, x)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(HDB_BF(av), HDB_BF(Bq[s].p2), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(HDB_BF(av), HDB_BF(Bq[s].p1), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(HDB_BF(av), HDB_BF(Bq[s].p0), acc, 0, 0, 0);
#undef HDB_BF
            }
            hdb_f8_tile_finish<MODE, METRIC, HAS_BIAS, KSL>(a, acc, aux0, t, h, rowg, n_rows, q_ok, ql, qinv_l, qsq_l, thr_cmp, ks_at);
        }
    };

    int64_t sg = blockIdx.x;
    if (sg >= nstages) return;                                // (block-uniform, before the first barrier)
    uint4 raw[CPT];
    load_stage(sg, raw);
    store_stage(0, raw);
    __syncthreads();
    for (int cur = 0; sg < nstages; sg += gridDim.x, cur ^= 1) {
        const int64_t nx = sg + gridDim.x;
        if (nx < nstages) load_stage(nx, raw);               // in flight while this stage is multiplied
        if (wave_on) multiply(cur * stage_bytes, sg);
        if (nx < nstages) store_stage((cur ^ 1) * stage_bytes, raw);
        __syncthreads();                                      // the next stage is whole; this one has been read by every wave
    }
}

// blocks: the most workgroups the launch may take (max_blocks, or workgroups per CU x CUs); the grid is one workgroup per stage up to it
template <int D, int MODE, int METRIC, bool HAS_BIAS, bool KSL>
static int launch_f8_lds_one(const ScanArgs& a, const MfmaLaunch& l, const float* aux0) {
    auto kern = hdb_mfma_f8_lds_kernel<D, MODE, METRIC, HAS_BIAS, KSL>;
    static unsigned long long attr_done = 0;          // per instantiation, one bit per device
    const hipError_t e = hdb_lds_attr_once(reinterpret_cast<const void*>(kern), hdb_mfma_f8_lds_bytes(D, 8), &attr_done);      // (eight waves at d >= 384: beyond 64 KiB)
    if (e != hipSuccess) return (int)e;
    const int waves = hdb_mfma_f8_lds_waves(a.f8_lds, D);          // (d = 512: four waves whatever was asked for)
    const int tq = (l.nq_launch + 15) / 16;
    const dim3 grid(hdb_mfma_f8_lds_blocks(a.ntiles, D, waves, l.blocks), (tq + waves - 1) / waves);
    hipLaunchKernelGGL(kern, grid, dim3(64 * waves), (size_t)hdb_mfma_f8_lds_bytes(D, waves), (hipStream_t)l.stream, a, (const float*)l.q, aux0, l.qsq, a.q0 + l.nq_launch);
    return (int)hipGetLastError();
}
template <int D>
static int launch_f8_lds(const ScanArgs& a, const MfmaLaunch& l) {
    // 16-byte pieces of whole rows; a mask arrives folded into the bias
    if ((reinterpret_cast<uintptr_t>(a.V) & 15) != 0 || a.d != D || a.mask || a.ntiles < 1 || a.n < 1 || l.blocks < 1) return (int)hipErrorNotSupported;
    return hdb_mode_ladder<1, 0>(a, l.mode, l.sqnorm, [&](auto mode, auto metric, auto bias, const float* aux0) {
        return launch_f8_lds_one<D, mode.value, metric.value, bias.value != 0, false>(a, l, aux0);
    });
}
// One K slice of a wide float8 row (hdb_mfma_ksplit.hip): mode 3 = raw partial sums out, 0 / 1 = the last slice with the metric's epilogue
template <int D>
static int launch_f8_lds_kslice(const ScanArgs& a, const MfmaLaunch& l) {
    // 16-byte pieces: base, pitch and slice offset; float4 query and partial-sum accesses; the slice lies inside the row
    if ((reinterpret_cast<uintptr_t>(a.V) & 15) != 0 || (a.ks_pitch & 15) != 0 || (a.ks_off & 15) != 0 || a.ks_off < 0 || a.ks_off + D > a.ks_pitch ||
        a.ks_dfull != a.ks_pitch || (a.ks_ld & 3) != 0 || a.mask || a.ntiles < 1 || a.n < 1 || l.blocks < 1) return (int)hipErrorNotSupported;
    if ((reinterpret_cast<uintptr_t>(a.ks_partial_in) & 15) != 0 || (reinterpret_cast<uintptr_t>(a.ks_partial_out) & 15) != 0 || (l.mode == 3 && !a.ks_partial_out)) return (int)hipErrorNotSupported;
    return hdb_mode_ladder<1, 0, 3>(a, l.mode, l.sqnorm, [&](auto mode, auto metric, auto bias, const float* aux0) {
        return launch_f8_lds_one<D, mode.value, metric.value, bias.value != 0, true>(a, l, aux0);
    });
}
