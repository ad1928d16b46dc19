// hdb_quant_mfma.hip -- batches of 5-256 dot / cosine queries through the int8 shadow (hdb_quant.hip): the filter pass on the int8
// matrix cores (v_mfma_i32_16x16x64_i8), the threshold of a batch and the block-diagonal exact rescoring (gfx950).
//
// Pipeline of one chunk of up to 256 queries (hdb_api.hip, quant_batch_topk):
//   hdb_quant_qprep_m_kernel (1/||q||, scaled fp16 copy, codes of the rounded query)
//   -> hdb_qb_scan_kernel<0> over a strided row sample: per-subset maxima of the LOWER bounds
//   -> hdb_qb_thr_kernel: T_s = m-th largest of them per query
//   -> hdb_qb_scan_kernel<1> over all rows: (row, query) pairs whose UPPER bound reaches T_s go to the query's candidate list
//   -> hdb_qb_rescore_kernel: every list entry scored from the fp16 matrix with the default batched path's instruction and epilogue
//   -> hdb_quant_finalize_kernel with the floor T_s.
// Bounds (1)-(3) and the completeness argument are those of hdb_quant.hip; nothing here changes them.
//
// ---- The filter kernel ----------------------------------------------------------------------------------------------------
// C[row][query] = sum_j c_rj c_qj with v_mfma_i32_16x16x64_i8: A = 16 rows x 64 codes, B = 16 queries x 64 codes, one k-step is 64
// bytes of the row pitch P (P % 64 == 0).  Lane l supplies, for BOTH operands, the 16 contiguous code bytes [64 s + 16 (l >> 4), + 16)
// of row / query (l & 15): whatever order the hardware gives those bytes inside the step, rows and queries use the same one, and an
// exact integer sum does not care about the order.  C/D: lane l, register e -> row 4 (l >> 4) + e, query l & 15.
// The queries are the stationary operand: a wave keeps NQT query tiles (16 queries each) for all k-steps in registers
// (NQT * P / 16 VGPRs, 128 at most).  The four waves of a workgroup form `wq` groups over the queries (1: up to 64 queries, every
// wave holds all of them and the waves split the row tiles; 2: up to 128; 4: up to 256, every wave multiplies every row tile by
// its own quarter of the queries).  Row fragments come straight from global memory (a tile is one contiguous piece of 16 P
// bytes; waves of one workgroup that read the same tile meet in the vector L1), the next tile's loads are issued before the
// current tile is multiplied.
//
// ---- The cheap candidate test -----------------------------------------------------------------------------------------------
// hdb_quant_scan_kernel evaluates, per pair, with kappa = 1/||q|| and rho = 1/||v|| (both 1 for the dot product), b = bias:
//     A = fl(fl(s_q s_r) fl(C)),  B = (N_q E_r + D_q T_r)(1 + 2^-10) + |A| 2^-10 + a0,   a0 = 2^-100 (d + 8)
//     hi = fl(fl(fl(A + B) rho) kappa) + b, pushed outward by |hi| 2^-20 + 1e-30,         and emits the pair when hi >= T_s.
// With alpha = s_q s_r C rho kappa and beta = (N_q E_r + D_q T_r) rho kappa (real numbers), every float operation above perturbs
// its result by a factor within (1 +- u), u = 2^-24; at most ten of them and the push act on any constituent, and an error
// relative to a partial result is at most that fraction of the sum of the constituents' magnitudes, so
//     hi <= alpha + (2^-10 + 2^-18) |alpha| + beta (1 + 2^-10 + 2^-18) + b + 2^-19 |b| + a0 rho kappa (1 + 2^-19) + 2e-30.   (4)
// The kernel evaluates instead, with per-query and per-row values formed once outside the pair loop,
//     cs = fl(s_q kappa), cn = fl(fl(N_q kappa)(1 + 2^-9)), cd = fl(fl(D_q kappa)(1 + 2^-9)),
//     ar = fl(s_r rho),   er = fl(E_r rho),  tr = fl(T_r rho),  b' = fl(b + 2^-18 |b|)   (-inf for a masked row or one past n),
//     m = fl(ar fl(C))  (|C| <= 127^2 * 512 < 2^24: the conversion is exact),  m2 = fl(m + 2^-9 |m|),
//     y = fl(cd tr + fl(cn er + fl(cs m2 + b')))                                       -- convert, multiply, four fma, compare.
// Term by term (theta: a product of at most four factors within (1 +- u)):
//     cs m2 = alpha (1 +- 2^-9) theta, the sign being that of alpha, >= alpha + (2^-10 + 2^-18) |alpha| + 2^-11 |alpha|;
//     cn er >= N_q E_r rho kappa (1 + 2^-9)(1 - 3u) >= N_q E_r rho kappa (1 + 2^-10 + 2^-18) + 2^-11 (the same); cd tr likewise;
//     b' >= b + 2^-19 |b| + 2^-20 |b|.
// The three roundings of y cost at most 3u (|cs m2| + cn er + cd tr + |b'|) <= 2^-22 (|alpha| + beta + |b|), which the spare
// 2^-11 |alpha| + 2^-11 beta + 2^-20 |b| covers; products that underflow lose less than 2^-120 in all.  Hence
//     y >= [right-hand side of (4)] - c0,   c0 = 1.001 a0 R K + 4e-30,
// where R and K bound rho and kappa: 1 for the dot product; for cosine R = 2^24 (an fp16 row has ||v|| >= 2^-24 unless it is zero,
// and then 1/||v|| is stored as 1) and K = 2^40, i.e. c0 = 1.001 (d + 8) 2^-36.  A row whose 1/||v|| exceeds R gets b' = +inf and a
// query whose 1/||q|| exceeds K gets the threshold -inf: they always pass.  So with
//     ct = fl(fl(T_s - 2^-18 |T_s|) - c0)  <=  T_s - c0,
// hi >= T_s implies y >= ct.  The test is written !(y < ct), so a NaN (an infinite b' meeting an infinite product) passes as well.
// Pairs that pass are then held against the exact hi of hdb_quant_scan_kernel, evaluated for them alone: the lists are those of
// the VALU scan, and the cheap test can only cost time, never a row.  Masked rows and rows past n never pass the second test.
//
// ---- MODE 0 -----------------------------------------------------------------------------------------------------------------
// The sample pass evaluates the exact lower bound of every sampled pair (the sample is a tenth of the rows) and keeps ONE running
// maximum per lane and query tile; at the end every quarter-wave (16 lanes = 16 queries, 4 rows of each tile) writes its maxima:
// wstat[query][4 * (workgroup * (4 / wq) + row part of the wave) + (lane >> 4)].  Every slot of the grid is written (-inf: nothing seen), nothing is
// initialized by the host, and nq x sample scores are never stored.  T_s = the m-th largest of a query's slots: a lower bound of
// the m-th largest sampled lower bound (order statistic of a subset), equal to it unless two of the top m fell to one slot.
#include "hdb_mfma_kernel.h"
#include "hdb_quant.h"
#include "../../include/hyperdb_hip.h"

typedef int hqb_i32x4 __attribute__((ext_vector_type(4)));

struct QbArgs {
    QuantArgs q;              // codes, caches, queries, thresholds and lists (scores / wmax / nsub unused)
    float* wstat;             // MODE 0: [nq][wld] per-slot maxima of the lower bounds
    int64_t wld;
    int32_t wq;               // wave groups over the queries: 1, 2 or 4
};

__device__ __forceinline__ hqb_i32x4 hqb_load_nt(const int8_t* p) {
    return __builtin_nontemporal_load(reinterpret_cast<const hqb_i32x4*>(p));
}

template <int MODE, int KS, int NQT>
__global__ __launch_bounds__(256) void hdb_qb_scan_kernel(QbArgs g) {
    const QuantArgs& a = g.q;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rl = lane & 15, h = lane >> 4;
    const int WQ = g.wq, WR = 4 / WQ;
    const int wq_id = wave % WQ, wr_id = wave / WQ;
    const bool cosine = a.metric == HDB_COSINE;
    const float absmin = 0x1p-100f * (float)(a.d + 8);

    // ---- this wave's queries: B fragments for every k-step, per-query values of lane column rl ----
    hqb_i32x4 Bq[NQT][KS];
    int qi[NQT];
    bool q_ok[NQT];
    float c_s[NQT], c_n[NQT], c_d[NQT], c_t[NQT];        // MODE 1: cs, cn, cd, ct of the cheap test; MODE 0: s_q, N_q, D_q, kappa
#pragma unroll
    for (int t = 0; t < NQT; ++t) {
        const int q = (wq_id * NQT + t) * 16 + rl;
        const float* o = a.qaux + (int64_t)(q < a.nq ? q : 0) * HDB_QQ_WORDS;
        q_ok[t] = q < a.nq && o[HDB_QQ_BAD] == 0.f;
        qi[t] = q < a.nq ? q : 0;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            Bq[t][s] = hqb_i32x4{0, 0, 0, 0};
            if (q < a.nq) Bq[t][s] = *reinterpret_cast<const hqb_i32x4*>(a.qcodes + (int64_t)q * a.P + 64 * s + 16 * h);
        }
        const float kappa = cosine ? a.qinv[qi[t]] : 1.f;
        if (MODE == 0) {
            c_s[t] = o[HDB_QQ_S]; c_n[t] = o[HDB_QQ_N]; c_d[t] = o[HDB_QQ_D]; c_t[t] = kappa;
        } else {
            const float T = a.thr[qi[t]];
            const float c0 = cosine ? 1.001f * (float)(a.d + 8) * 0x1p-36f : 1.001f * absmin + 4e-30f;
            c_s[t] = o[HDB_QQ_S] * kappa;
            c_n[t] = (o[HDB_QQ_N] * kappa) * (1.f + 0x1p-9f);
            c_d[t] = (o[HDB_QQ_D] * kappa) * (1.f + 0x1p-9f);
            c_t[t] = (T - fabsf(T) * 0x1p-18f) - c0;
            if (!(kappa <= 0x1p40f)) c_t[t] = -INFINITY;             // (also a NaN kappa)
            if (!q_ok[t]) c_t[t] = INFINITY;                         // a query the call leaves to the exact re-run: nothing passes
        }
    }
    float wbest[NQT];
#pragma unroll
    for (int t = 0; t < NQT; ++t) wbest[t] = -INFINITY;

    const int64_t step = (int64_t)gridDim.x * WR;
    int64_t t_cur = (int64_t)blockIdx.x * WR + wr_id;
    auto load_tile = [&](int64_t t, hqb_i32x4 (&f)[KS]) {
        const int64_t r = min(hdb_tile_index(t, a.tile_stride) * 16 + rl, a.n - 1);
        const int8_t* p = a.codes + r * (int64_t)a.P + 16 * h;
#pragma unroll
        for (int s = 0; s < KS; ++s) f[s] = hqb_load_nt(p + 64 * s);
    };
    hqb_i32x4 cur[KS];
    if (t_cur < a.ntiles) load_tile(t_cur, cur);
    for (; t_cur < a.ntiles; t_cur += step) {
        const int64_t r0 = hdb_tile_index(t_cur, a.tile_stride) * 16 + 4 * h;     // first of this lane's four rows
        hqb_i32x4 nxt[KS];
        const bool more = t_cur + step < a.ntiles;
        if (more) load_tile(t_cur + step, nxt);
        // per-row values of rows r0 .. r0 + 3: vector loads while all four rows exist, clamped scalar loads in the ragged last tile
        float s_r[4], e_r[4], t_r[4];
        float rho[4] = {1.f, 1.f, 1.f, 1.f};
        if (r0 + 3 < a.n) {
            const float4 x0 = *reinterpret_cast<const float4*>(a.aux + 3 * r0);
            const float4 x1 = *reinterpret_cast<const float4*>(a.aux + 3 * r0 + 4);
            const float4 x2 = *reinterpret_cast<const float4*>(a.aux + 3 * r0 + 8);
            s_r[0] = x0.x; s_r[1] = x0.w; s_r[2] = x1.z; s_r[3] = x2.y;
            e_r[0] = x0.y; e_r[1] = x1.x; e_r[2] = x1.w; e_r[3] = x2.z;
            t_r[0] = x0.z; t_r[1] = x1.y; t_r[2] = x2.x; t_r[3] = x2.w;
            if (cosine) { const float4 iv = *reinterpret_cast<const float4*>(a.inv_norm + r0); rho[0] = iv.x; rho[1] = iv.y; rho[2] = iv.z; rho[3] = iv.w; }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t rr = min(r0 + e, a.n - 1);
                s_r[e] = a.aux[3 * rr + HDB_QROW_S]; e_r[e] = a.aux[3 * rr + HDB_QROW_E]; t_r[e] = a.aux[3 * rr + HDB_QROW_T];
                if (cosine) rho[e] = a.inv_norm[rr];
            }
        }
        float bs[4];
        bool dead[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t rr = min(r0 + e, a.n - 1);
            bs[e] = a.bias ? a.bias[rr] : 0.f;
            dead[e] = r0 + e >= a.n || (a.mask && !a.mask[rr]);
        }
        int acc[NQT][4];
#pragma unroll
        for (int t = 0; t < NQT; ++t) {
            hqb_i32x4 c = {0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < KS; ++s) c = __builtin_amdgcn_mfma_i32_16x16x64_i8(cur[s], Bq[t][s], c, 0, 0, 0);
            acc[t][0] = c[0]; acc[t][1] = c[1]; acc[t][2] = c[2]; acc[t][3] = c[3];
        }
        if (MODE == 0) {
#pragma unroll
            for (int t = 0; t < NQT; ++t) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // the lower bound as hdb_quant_scan_kernel forms it
                    const float A = (c_s[t] * s_r[e]) * (float)acc[t][e];
                    const float B = (c_n[t] * e_r[e] + c_d[t] * t_r[e]) * (1.f + 0x1p-10f) + fabsf(A) * 0x1p-10f + absmin;
                    float lo = A - B;
                    if (cosine) lo = lo * rho[e] * c_t[t];
                    if (a.bias) lo += bs[e];
                    lo = lo - fabsf(lo) * 0x1p-20f - 1e-30f;
                    if (lo != lo || dead[e] || !q_ok[t]) lo = -INFINITY;
                    wbest[t] = fmaxf(wbest[t], lo);
                }
            }
        } else {
            float ar[4], er[4], tr[4], bp[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ar[e] = s_r[e] * rho[e]; er[e] = e_r[e] * rho[e]; tr[e] = t_r[e] * rho[e];
                bp[e] = fmaf(fabsf(bs[e]), 0x1p-18f, bs[e]);
                if (!(rho[e] <= 0x1p24f)) bp[e] = INFINITY;
                if (dead[e]) bp[e] = -INFINITY;
            }
#pragma unroll
            for (int t = 0; t < NQT; ++t) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float m = ar[e] * (float)acc[t][e];
                    const float m2 = fmaf(fabsf(m), 0x1p-9f, m);
                    const float y = fmaf(c_d[t], tr[e], fmaf(c_n[t], er[e], fmaf(c_s[t], m2, bp[e])));
                    const bool pass = !(y < c_t[t]);
                    if (__ballot(pass) != 0ull) {
                        if (pass && q_ok[t] && !dead[e]) {
                            // the exact upper bound of hdb_quant_scan_kernel for the survivors of the cheap test
                            const float* o = a.qaux + (int64_t)qi[t] * HDB_QQ_WORDS;
                            const float A = (o[HDB_QQ_S] * s_r[e]) * (float)acc[t][e];
                            const float B = (o[HDB_QQ_N] * e_r[e] + o[HDB_QQ_D] * t_r[e]) * (1.f + 0x1p-10f) + fabsf(A) * 0x1p-10f + absmin;
                            float hi = A + B;
                            if (cosine) hi = hi * rho[e] * a.qinv[qi[t]];
                            if (a.bias) hi += bs[e];
                            hi = hi + fabsf(hi) * 0x1p-20f + 1e-30f;
                            if (hi != hi) hi = INFINITY;
                            if (hi >= a.thr[qi[t]]) {
                                const uint32_t pos = atomicAdd(&a.cnt[qi[t] * HDB_CNT_STRIDE], 1u);
                                if (pos < a.cap) a.cand[(int64_t)qi[t] * a.cap + pos] = hdb_pack(hi, (uint32_t)(r0 + e));
                            }
                        }
                    }
                }
            }
        }
        if (more) {
#pragma unroll
            for (int s = 0; s < KS; ++s) cur[s] = nxt[s];
        }
    }
    if (MODE == 0) {
        // a query's slots: one per quarter-wave of every wave that holds it -- (workgroup, row part, lane >> 4)
        const int64_t slot = ((int64_t)blockIdx.x * WR + wr_id) * 4 + h;
#pragma unroll
        for (int t = 0; t < NQT; ++t) {
            const int q = (wq_id * NQT + t) * 16 + rl;
            if (q < a.nq) g.wstat[(int64_t)q * g.wld + slot] = wbest[t];
        }
    }
}

// T_s = the m-th largest of n values per query (m <= 64): every thread keeps the maximum of its strided share, then m rounds of
// "largest of the 1024 maxima, remove one copy".  A lower bound of the m-th largest value (order statistic of a subset), equal to
// it unless two of the top m fell to one thread.  thr[q] = -inf when fewer than m values above -inf exist.
__global__ __launch_bounds__(1024) void hdb_qb_thr_kernel(const float* vals, int64_t n, int64_t ld, uint32_t m, float* thr) {
    __shared__ uint32_t wmaxs[16];
    __shared__ int owner;
    const int q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* v = vals + (int64_t)q * ld;
    uint32_t best = 0u;                                   // key 0 is below every float, -inf included
    for (int64_t i = threadIdx.x; i < n; i += 1024) { const float x = v[i]; if (x == x && x != -INFINITY) best = max(best, hdb_f2key(x)); }
    uint32_t kth = 0u;
    for (uint32_t r = 0; r < m; ++r) {
        uint32_t wm = best;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) wm = max(wm, (uint32_t)__shfl_xor((int)wm, o, 64));
        if (lane == 0) wmaxs[wave] = wm;
        if (threadIdx.x == 0) owner = 1024;
        __syncthreads();
        uint32_t bm = 0u;
#pragma unroll
        for (int w = 0; w < 16; ++w) bm = max(bm, wmaxs[w]);
        if (best == bm) atomicMin(&owner, (int)threadIdx.x);
        __syncthreads();
        if ((int)threadIdx.x == owner) best = 0u;
        kth = bm;
        __syncthreads();
    }
    if (threadIdx.x == 0) thr[q] = kth == 0u ? -INFINITY : hdb_key2f(kth);
}

// ------------------------------------------------------------------------------------------------------------------------
// Block-diagonal exact rescoring: query q against its own list only.  One wave takes 16 list entries: their rows, fetched from the
// fp16 matrix by index, are the A operand and the query's scaled fp16 copy (every column the same query) the B operand of
// v_mfma_f32_16x16x32_f16, lane l supplying elements [32 s + 8 (l >> 4), + 8) of row / query for k-step s = 0 .. d/32 - 1 in order
// -- the instruction, fragment map and K walk of hdb_mfma_kernel<_Float16, 16, QT, D, ...> (MfmaShape<16, _Float16>::mma), which is
// what hdb_launch_mfma_scan gives every fp16 call of d = 128 / 256 / 384 / 512 with mfma_variant = 16, whatever the query count.
// A score depends on its own row and query only, so the position in the tile does not matter (the 1-4-query flavour relies on
// the same when it gathers).  Epilogue: the MODE 0 one of that kernel -- dot: dot * qscl, cosine: dot * (1/||v||) * (1/||q|| * qscl),
// with a bias fmaf(.., .., bias) and the row mask as a bias of -inf (hdb_maskbias_kernel) -- then hdb_canon.
// ------------------------------------------------------------------------------------------------------------------------
struct QbRescoreArgs {
    const _Float16* V; const _Float16* q16; const float* qscl; const float* qinv; const float* inv_norm; const float* bias;
    const uint8_t* mask; unsigned long long* cand; const uint32_t* cnt; uint32_t cap;
};

template <int D, int METRIC, bool HAS_BIAS>
__global__ __launch_bounds__(256) void hdb_qb_rescore_kernel(QbRescoreArgs a) {
    using Shape = MfmaShape<16, _Float16>;
    constexpr int KS = D / 32;
    const int q = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rl = lane & 15, h = lane >> 4;
    const uint32_t total = min(a.cnt[q * HDB_CNT_STRIDE], a.cap);
    if (total == 0u) return;
    half8 Bq[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) Bq[s] = *reinterpret_cast<const half8*>(a.q16 + (int64_t)q * D + 32 * s + 8 * h);
    const float qs = a.qscl[q];
    const float qinv_l = METRIC == 1 ? a.qinv[q] * qs : qs;
    unsigned long long* list = a.cand + (int64_t)q * a.cap;
    for (uint32_t base = ((uint32_t)blockIdx.x * 4 + wave) * 16; base < total; base += gridDim.x * 64) {       // (wave-uniform)
        const uint32_t i = min(base + (uint32_t)rl, total - 1);
        const uint32_t row = 0xFFFFFFFFu - (uint32_t)(list[i] & 0xFFFFFFFFull);
        const _Float16* pr = a.V + (int64_t)row * D + 8 * h;
        half8 af[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) af[s] = *reinterpret_cast<const half8*>(pr + 32 * s);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) acc = Shape::mma(af[s], Bq[s], acc);
        // lane (rl, h) holds entries base + 4 h + e, e = 0 .. 3, in every column: lanes rl < 4 write entry e = rl
        const uint32_t row_e = (uint32_t)__shfl((int)row, 4 * h + (rl & 3), 64);
        const float dot = rl == 0 ? acc[0] : rl == 1 ? acc[1] : rl == 2 ? acc[2] : acc[3];
        const uint32_t ie = base + 4 * h + rl;
        if (rl < 4 && ie < total) {
            float bj = 0.f;
            if (HAS_BIAS) bj = a.mask ? (a.mask[row_e] ? (a.bias ? a.bias[row_e] : 0.f) : -INFINITY) : a.bias[row_e];
            float x;
            if (METRIC == 0) x = HAS_BIAS ? fmaf(dot, qinv_l, bj) : dot * qinv_l;
            else { const float aj = a.inv_norm[row_e]; x = HAS_BIAS ? fmaf(dot * aj, qinv_l, bj) : dot * aj * qinv_l; }
            list[ie] = hdb_pack(hdb_canon(x), row_e);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// host-side launchers
// ------------------------------------------------------------------------------------------------------------------------
template <int MODE, int KS>
static void qb_launch_ks(const QbArgs& g, int nqt, int blocks, hipStream_t st) {
    switch (nqt) {
    case 1: hipLaunchKernelGGL((hdb_qb_scan_kernel<MODE, KS, 1>), dim3(blocks), dim3(256), 0, st, g); break;
    case 2: hipLaunchKernelGGL((hdb_qb_scan_kernel<MODE, KS, 2>), dim3(blocks), dim3(256), 0, st, g); break;
    case 3: hipLaunchKernelGGL((hdb_qb_scan_kernel<MODE, KS, 3>), dim3(blocks), dim3(256), 0, st, g); break;
    default: hipLaunchKernelGGL((hdb_qb_scan_kernel<MODE, KS, 4>), dim3(blocks), dim3(256), 0, st, g); break;
    }
}
template <int MODE>
static int qb_launch_mode(const QbArgs& g, int nqt, int blocks, hipStream_t st) {
    switch (g.q.P) {
    case 128: qb_launch_ks<MODE, 2>(g, nqt, blocks, st); break;
    case 256: qb_launch_ks<MODE, 4>(g, nqt, blocks, st); break;
    case 384: qb_launch_ks<MODE, 6>(g, nqt, blocks, st); break;
    case 512: qb_launch_ks<MODE, 8>(g, nqt, blocks, st); break;
    default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}
// mode 0: per-slot maxima of the sampled lower bounds -> wstat[nq][wld] (wld >= hdb_qb_slots(blocks, nq)); mode 1: candidate emission.
// 1 <= a.nq <= 256; a.cnt zeroed by the caller (hdb_quant_qprep_m_kernel).
extern "C" int hdb_launch_qb_scan(const QuantArgs* args, int mode, float* wstat, int64_t wld, int max_blocks, void* stream) {
    QbArgs g;
    g.q = *args; g.wstat = wstat; g.wld = wld;
    const QuantArgs& a = g.q;
    if (a.nq < 1 || a.nq > 256 || !hdb_qb_supported(a.d) || a.P != a.d || (a.metric != HDB_DOT && a.metric != HDB_COSINE)) return (int)hipErrorInvalidValue;
    int nqt; qb_shape(a.nq, g.wq, nqt);
    const int blocks = hdb_qb_scan_blocks(a.ntiles, a.nq, hdb_cu_count(), max_blocks);
    if (mode == 0 && (!wstat || wld < hdb_qb_slots(blocks, a.nq))) return (int)hipErrorInvalidValue;
    return mode == 0 ? qb_launch_mode<0>(g, nqt, blocks, (hipStream_t)stream) : qb_launch_mode<1>(g, nqt, blocks, (hipStream_t)stream);
}

extern "C" int hdb_launch_qb_thr(const float* vals, int64_t n, int64_t ld, int nq, uint32_t m, float* thr, void* stream) {
    if (m < 1 || m > 64) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(hdb_qb_thr_kernel, dim3(nq), dim3(1024), 0, (hipStream_t)stream, vals, n, ld, m, thr);
    return (int)hipGetLastError();
}

extern "C" int hdb_launch_qb_rescore(const void* V, int d, const void* q16, const float* qscl, const float* qinv, const float* inv_norm,
                                     const float* bias, const uint8_t* mask, int metric, unsigned long long* cand, const uint32_t* cnt,
                                     uint32_t cap, int nq, void* stream) {
    if (!hdb_qb_supported(d) || (reinterpret_cast<uintptr_t>(V) & 15) != 0 || (metric != HDB_DOT && metric != HDB_COSINE)) return (int)hipErrorInvalidValue;
    QbRescoreArgs a;
    a.V = (const _Float16*)V; a.q16 = (const _Float16*)q16; a.qscl = qscl; a.qinv = qinv; a.inv_norm = inv_norm; a.bias = bias; a.mask = mask;
    a.cand = cand; a.cnt = cnt; a.cap = cap;
    const dim3 grid(32, nq);
    hipStream_t st = (hipStream_t)stream;
    const bool hb = bias != nullptr || mask != nullptr;
#define HQB_RS(D_)                                                                                                             \
    do {                                                                                                                       \
        if (metric == HDB_DOT) { if (hb) hipLaunchKernelGGL((hdb_qb_rescore_kernel<D_, 0, true>), grid, dim3(256), 0, st, a);   \
                                 else hipLaunchKernelGGL((hdb_qb_rescore_kernel<D_, 0, false>), grid, dim3(256), 0, st, a); }   \
        else { if (hb) hipLaunchKernelGGL((hdb_qb_rescore_kernel<D_, 1, true>), grid, dim3(256), 0, st, a);                     \
               else hipLaunchKernelGGL((hdb_qb_rescore_kernel<D_, 1, false>), grid, dim3(256), 0, st, a); }                     \
    } while (0)
    switch (d) {
    case 128: HQB_RS(128); break;
    case 256: HQB_RS(256); break;
    case 384: HQB_RS(384); break;
    default: HQB_RS(512); break;
    }
#undef HQB_RS
    return (int)hipGetLastError();
}
