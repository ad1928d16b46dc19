// hdb_quant.hip -- the opt-in int8 shadow of the stored matrix: quantized row scan with exact rescoring (gfx950).
//
// The index may keep an int8 copy of its N x d matrix (hdb_index_quantize): one code byte per element at a row pitch
// P = round_up(d, 16) bytes (zero-padded, so every row streams in 16-byte pieces whatever d is) and three floats per row.
// A top-k call of 1-4 dot / cosine / euclidean queries then reads P + 12 bytes per row instead of 2d or 4d, scores every row
// approximately with v_dot4_i32_i8 (exact int32 sums), keeps the rows whose UPPER bound can still reach a sampled threshold,
// rescores those from the original matrix with the VALU scan's own float32 arithmetic and selects.  The answer is the same
// bits as the VALU scan (hdb_scan_kernel / hdb_scan_generic_kernel + hdb_emit) gives, not an approximation of it.
//
// ---- The bound ---------------------------------------------------------------------------------------------------------
// Row r (values v_rj, j < d):   s_r = max_j |v_rj| / 127 (float32),  c_rj = rne(v_rj / s_r) in [-127, 127],
//                               eps_r = v_r - s_r c_r (float64 at quantization time).
// Query q (float32):            s_q, c_q, delta_q = q - s_q c_q, formed the same way.
// C_qr = sum_j c_qj c_rj is exact in int32 (|C| <= 127^2 d < 2^31 for every d the index takes).
// Since q.v_r = s_r (s_q C_qr + delta_q.c_r) + q.eps_r, Cauchy-Schwarz gives
//     |q.v_r - s_q s_r C_qr| <= ||q|| ||eps_r|| + ||delta_q|| (s_r ||c_r||)  =: B_qr.                              (1)
// The target is not the real dot product but the float32 sum S_f the VALU scan forms: per lane an fma chain of ceil(d/16)
// steps, then a 4-level DPP tree (hdb_rows4_sum).  Each product enters at most d/16 + 5 <= d + 8 roundings, so
//     |S_f - q.v_r| <= gamma ||q|| ||v_r||,  gamma = gamma_{d+8} = (d+8) u / (1 - (d+8) u),  u = 2^-24                (2)
// (an absolute 2^-100 (d+8) covers underflow).  The per-row cache holds (all rounded UP from float64):
//     aux[r] = { s_r,  E_r = ||eps_r|| + gamma ||v_r||,  T_r = s_r ||c_r|| }                 (12 bytes per row)
// and the query prep: s_q, N_q = ||q|| (up), D_q = ||delta_q|| (up), ||q||^2.  With A = fl(fl(s_q s_r) fl(C)):
//     B = (N_q E_r + D_q T_r)(1 + 2^-10) + |A| 2^-10 + 2^-100 (d+8)                                               (3)
// bounds |S_f - A| by (1) + (2): the 2^-10 terms dominate every float32 rounding of A (<= 3u |A|, fl(C) adds u when
// |C| >= 2^24) and of B itself (a few u relative), and later the rounding of A -/+ B (u (|A| + B)).
// dot / cosine: the raw-sum interval is [A - B, A + B].
// euclidean: the scan sums fl(x - q)^2 directly; with D2 = ||v||^2 + ||q||^2 - 2 q.v (real), E_f (its float sum) lies in
//     D2 (1 -/+ 2 gamma) (one more rounding per element than (2)).  ||v||^2 comes from the float32 row cache sqnorm, itself within
//     gamma of the real value: ||v||^2 in sq (1 -/+ 2 gamma).  So with c = sq + ||q||^2 - 2A and
//     err = 2 gamma sq + 2B + 2^-10 (sq + ||q||^2 + 2|A|) + 2^-100 (d+8):
//     E_f in [max(0, c - err)(1 - 2 gamma - 2^-10), (c + err)(1 + 2 gamma + 2^-10)].
// Score domain: every map of hdb_emit is monotone in the raw sum (x -> fl(fl(x a) b) with a, b > 0 for cosine, x -> 1/(1+sqrt x)
// non-increasing for euclidean, then + bias), so the same float operations applied to the raw bounds bound the final score.  The
// compiler may contract hdb_emit's multiply and bias add into one fma, i.e. round once less than the bound's evaluation: the
// bounds are pushed outward by |s| 2^-20 + 1e-30 (many ulps) to cover that.  NaN never reaches a bound (finite matrix, finite
// query; a NaN upper bound would count as +inf).
//
// ---- bfloat16 rows (opt-in: bf16_quant) ------------------------------------------------------------------------------------------
// Nothing above depends on the element type of the matrix.  A bfloat16 element widens to float32 exactly (a shift), so v_rj is a
// float32 number as for the other types; the row quantizer forms s_r, eps_r, ||v_r|| from the widened values in float64, and E_r
// takes max(gamma, gamma_m) like every shadow.  The target is the float32 sum of the VALU scan, bound (2): hdb_scan_kernel /
// hdb_scan_generic_kernel instantiated for hdb_bf16 run the same fma chain per lane and the same tree on the widened values (the
// products of an 8-bit and a 24-bit significand are not exact in float32, as for float32 rows; (2) counts every rounding).  The
// euclidean interval reads the float32 sqnorm cache, which hdb_rownorm_kernel<hdb_bf16> fills with the same chain and tree as for
// the other types (squares of bfloat16 numbers are exact in float32: within gamma a fortiori).  The rescoring kernel's bfloat16
// instantiation unpacks a 16-byte piece as hdb_scan.hip's hdb_unpack does -- even element the low half of its word, odd element the
// high half -- so the lanes' partial sums are the scan's.  A default bfloat16 index answers 1-4 queries on that scan: the shadow
// returns the default path's bits.
//
// ---- The matrix-core flavour (automatic shadow of an fp16 index, hdb_api.hip) --------------------------------------------
// A default fp16 index answers 1-4-query calls on the matrix cores, so the shadow it builds for itself must return THOSE bits.
// The rescoring then gathers the candidate rows (with their 1/||v|| and bias) into a compact matrix and scores it with the
// MODE 0 launch of hdb_mfma_kernel.h -- the launch hdb_topk_exact uses for every row.  Its target sum S_m is the matrix-core
// sum of the ROUNDED query q' = fp16(q * scale) / scale (scale a power of two, hdb_q16_scale), so the query prep quantizes q'
// (hdb_quant_qprep_m_kernel: N_q = ||q'||, delta_q = q' - s_q c_q, exact for what is multiplied) and (1) holds for q'.  For (2):
// fp16 x fp16 products are exact in float32; v_mfma_f32_16x16x32_f16 adds 32 of them and the accumulator per step, d/32 steps in a
// chain, in an order and with a rounding (possibly truncation, unit 2^-23) the hardware does not document.  Whatever the order,
// at most d + d/32 additions each err by at most 2^-23 of a partial sum of magnitude <= sum_j |q'_j v_rj| <= ||q'|| ||v_r||, so
//     |S_m - q'.v_r| <= gamma_m ||q'|| ||v_r||,  gamma_m = (d + 8) 2^-22                                            (2m)
// with a factor two to spare.  Measured on MI355X (tests/test_auto_quant.py::test_gamma_m_measured: random and adversarial rows
// against float64 dot products of the same fp16 values): the largest |S_m - q'.v| / (||q'|| ||v||) is 2.7e-7 at d = 128, 4.3e-7 at
// d = 384, 8.2e-7 at d = 768, i.e. 0.8 %, 0.5 %, 0.4 % of gamma_m; the test asserts it stays at or below gamma_m / 4.
// E_r is built with the larger of gamma and gamma_m, so one shadow serves both flavours; the int8 error ||eps_r|| ~ 7e-3 ||v_r||
// dwarfs either.  The epilogue (x qscl, a power of two; cosine x 1/||v|| x 1/||q||; + bias, possibly fused) is the same monotone
// map up to the contraction the outward push of the bounds already covers.
//
// ---- The pipeline (hdb_api.hip, quant_topk) ----------------------------------------------------------------------------
//   query prep (hdb_qprep_kernel: 1/||q||, NaN flags) -> quantized query prep (codes, s_q, N_q, D_q)
//   -> int8 scan over a strided row sample (MODE 0: lower bounds)  -> T_s = m-th largest sampled lower bound (hdb_sample_thr)
//   -> int8 scan over all rows (MODE 1: row r is a candidate of q when its upper bound >= T_s)
//   -> exact rescoring of the candidates from the original matrix -> finalize with the floor T_s.
// (matrix-core flavour: ONE query prep launch; the threshold rides in the two passes -- QuantArgs::nsub, hdb_quant.h -- when the
//  sample is large enough; the kernel that emits a candidate copies its row into the compact matrix, so rescoring = the MODE 0
//  launch of hdb_mfma_kernel.h.)
// Completeness: every row that was not emitted has exact score <= its upper bound < T_s.  The finalize checks that the kk-th
// best rescored candidate scores ABOVE T_s (hdb_finalize_fast's floor); then every row missing from the list scores strictly
// below the kk-th best, so the top kk, ties at the kk-th score included, are all in the list.  If the check fails (HDB_Q_UNDERFLOW)
// or the list overflowed (HDB_Q_OVERFLOW) the status word says so and hdb_topk_host re-runs that query through the exact path.
//
// ---- The 5-bit plane (one dot / cosine query; hdb_quant_plane_scan_kernel) -----------------------------------------------------
// The MODE 1 pass rejects all but a few thousand rows at full int8 resolution.  Beside the codes the index keeps their high five
// bits: for a code c in [-127, 127], h = c >> 3 (arithmetic), u = h + 16 in [0, 31], rho = c - (8h + 4) in [-4, 3].  Per row, in
// units of 32 elements (U = ceil(P / 32) units): a 16-byte piece of nibbles u >> 1 (byte b of word i = elements 8i + b | 8i + 4 + b
// << 4, so w & 0x0F0F0F0F and (w >> 4) & 0x0F0F0F0F pair with consecutive query-code words), one word of bits u & 1 (element
// 4g + b at bit 8b + g, so (w >> g) & 0x01010101 pairs with query word g), both as arrays of their own (a 16-row tile is
// contiguous), and 16 bytes of row terms, laid out per 16-row tile as two 64-byte HOT BLOCKS (one for dot-product calls, one for
// cosine calls; hdb_caps.h) and 128 reserved bytes.  Pass 1 reads one block: 4 bytes per row, where the float32 terms
// {s_r, E_r, T_r, R_r} and 1 / ||v_r|| took 20.  With w_r = 1 (dot) or 1 / ||v_r|| (cosine: the cached float32 inv_norm[r]) a block holds
//     k_hi[16]   bfloat16: the smallest bfloat16 >= s_r w_r (the float64 product of two float32 numbers is exact);
//                the lower side is derived, k_lo = k_hi (1 - 2^-7) <= s_r w_r (bfloat16 spacing; 0 below 2^-126);
//     rc[16]     bytes: ceil(2 R_r), R_r = ||rho_r||_2 over j < d (an integer sum of squares of at most 16 d <= 8192, so rc <= 182);
//                R = 0.5 rc >= R_r exactly;
//     E*, T*, F* float32, the maxima over the tile's rows (rows < n) of E_r w_r, T_r w_r and absmin w_r, each rounded up,
//                absmin = 2^-100 (d + 8) the absolute floor of (3).  For cosine E_r w_r and T_r w_r are scale-free (about 7e-3 for every
//                row), so the maxima are tight; a dot-product call on a tile whose norms differ widely passes more of its rows.
// Pass 1 only filters: every row it keeps is evaluated again with MODE 1's own bits, so these terms need to be conservative and
// nothing else -- no bit of them reaches an answer.
// The bound.  c = 8u - 124 + rho, so with C5 = sum_j c_qj (8 u_rj - 124) = 8 sum_j c_qj u_rj - 124 sum_j c_qj (exact in int32)
//     |C - C5| = |sum_j c_qj rho_rj| <= ||c_q|| ||rho_r|| <= N_c R =: U                                              (4)
// (Cauchy-Schwarz on integers; the query prep leaves N_c = ||c_q|| rounded up and sum_j c_qj in qaux).  In float32:
//     ch = fl(fl(C5) + fl(N_c R)) + (|.| 2^-20 + 1) >= C5 + U >= C, and ch is a float, so ch >= fl(C);  cl likewise <= fl(C)
// (fl(C5) errs by 2^-24 |C5|, the product and the sum by 2^-24 (|C5| + 2U), U <= 508 d: the absolute 1 covers what the relative term
// does not).  MODE 1 forms A = fl(k8 fl(C)), k8 = fl(s_q s_r) >= 0, and, for cosine, multiplies by w_r after the sum A + B; pass 1
// works in the scaled domain from the start, A' = A w_r (a real number), k' = s_q s_r w_r.  |A - s_q s_r fl(C)| <= 2.1u |A|, so
// A' lies within 2.1u |A'| of k' fl(C).  The two sides of k':
//     k_up = fl(s_q k_hi) pushed up by 2^-20   >= k' (1 + 2^-21),        k_dn = fl(s_q k_lo) pushed down by 2^-20   <= k' (1 - 2^-21)
// (the pushes, 16u, cover the three roundings of each WHILE THE PRODUCTS ARE NORMAL NUMBERS.  A product s_q k below 2^-126 errs by an
// absolute 2^-150 instead -- by up to 2^-126 if denormals were flushed -- which |ch| < 2^23 turns into at most 2^-103 of A5; MODE 1's
// own k8 = fl(s_q s_r) errs by 2^-150 likewise, 2^-127 of A, and its multiply by w_r scales that.  Neither is relative to anything,
// so the cover is the absolute 1e-30 > 2^-100 in X below, ahead of the multiply by 1 / ||q|| in both kernels.  It holds for
// w_r <= 2^24, i.e. rows of norm 2^-24 or more: every non-zero float16 row.  The assumption is therefore about float32 rows of
// smaller norm: for those s_q s_r must be a normal number, at least 2^-126.  A dot-product call needs none, see "monotone" below.)
// The upper side of k' fl(C) takes k_up where ch >= 0 and k_dn where ch < 0:
//     ch >= 0:  A5 = fl(k_up ch) >= k' (1 + 2^-22) ch >= k' (1 + 2^-22) fl(C) >= A' for fl(C) >= 0, and A5 >= 0 > A' for fl(C) < 0;
//     ch <  0:  fl(C) <= ch < 0 and A5 = fl(k_dn ch) >= k' (1 - 2^-22) ch >= k' (1 - 2^-22) fl(C) = k' fl(C) + 4u |k' fl(C)| >= A'.
// Al = fl(k_dn cl) for cl >= 0, fl(k_up cl) for cl < 0, is <= A' in the same way, and |A'| <= Amax = max(|A5|, |Al|).  (For dot, where
// w_r = 1, fl(s_q k_hi) >= k8 >= fl(s_q k_lo) already by monotone rounding.)  The raw upper bound of (3), times w_r, is at most
//     g(A') = A' + c0 + |A'| 2^-10 + F*,   c0 = (N_q E* + D_q T*)(1 + 2^-10) >= (N_q E_r + D_q T_r)(1 + 2^-10) w_r,   F* >= absmin w_r
// in real numbers: non-decreasing in A'.  MODE 1's float32 evaluation F(A) of (3), whatever the compiler contracts, errs by at most
// 8u (|A| + B(A)), and its multiply by w_r by one more u: y = fl(F(A) w_r) <= g(A') + 9.1u (|A'| + B'(A')) <= g(A5) + 9.1u Mx,
// Mx = Amax + Bmax, Bmax = c0 + Amax 2^-10 + F*.  ANY float32 evaluation F5 of g errs by at most 8u Mx.  Hence
//     X = F5(A5) + Mx 2^-18 >= g(A5) - 8u Mx + 64u Mx - (own roundings, < 4u Mx) >= g(A5) + 52u Mx >= y.
// What is left of the cosine scaling is one multiply by 1 / ||q|| > 0 in both kernels: y5 = fl(X / ||q||) >= fl(y / ||q||) = y8, and
// both magnitudes are at most mM = fl(Mx (1 + 2^-17) / ||q||).  (MODE 1 associates (F w_r) / ||q||, pass 1 folds w_r into k', c0 and
// F*: a few ulps, inside the 52u above.)  The bias add may be contracted into the last multiply in either kernel: each side errs by at
// most 2u (|y| + |bias|) <= 2u Z, Z = mM + |bias|; MODE 1 then pushes its value by |hi| 2^-20 + 1e-30 <= Z 2^-20 (1 + 4u) + 1e-30.  With
//     hi5 = fl(y5 + bias) + Z 2^-18 + 4e-30
// the sum of all of that (< Z 2^-20 x 1.5 + 1e-30) is covered: hi5 >= hi for every row, hi as MODE 1 computes it, and hi5 is finite
// where the terms are.  A row pass 1 drops (hi5 < T_s; a NaN never drops) would have been dropped by MODE 1: the candidate set, and
// every later stage, is unchanged.  The pushes are relative to magnitudes that do not cancel.  What the block costs in width: k_up
// and k_dn are 2^-7 |A'| apart -- about 0.03 of a score's standard deviation at d = 384, against a width B of about 1.15 -- R grows by
// at most 0.5 in about 45, and E*, T* are the tile's largest instead of the row's own.
// The rows pass 1 keeps are finished by pass 1 itself: 16 at a time they go through MODE 1's own evaluation (hq_rows4_bounds, compiled
// with contraction off: the uncontracted form is one of the evaluations F(A) above, and both kernels get the same bits from it).
// The sampled tiles are not streamed a second time.  The sample pass has already put their rows through that evaluation, so it stores
// hi beside the lower bound it is after (QuantArgs::pl_hi, one float per sample slot), and pass 1 walks the other tiles only
// (hdb_plane_skip_*, hdb_caps.h) and queues the sampled rows with !(hi < T_s) from the list.  Streamed, such a row was queued because
// hi5 >= hi; a sampled row with hi < T_s that hi5 let through was queued for nothing (the drain drops it).  The drain evaluates and
// emits on the same condition either way: the candidate set is unchanged, plane_survivors counts at most what it counted.
#include "hdb_common.h"
#include "hdb_quant.h"
#include "hdb_finalize.h"
#include "../../include/hyperdb_hip.h"

// Float32 of a non-negative float64, rounded up (the double itself carries a relative margin of 2^-40 for its own sums).
__device__ __forceinline__ float hq_up(double x) {
    x = x * (1.0 + 0x1p-40);
    float f = (float)x;
    if ((double)f < x) f = nextafterf(f, INFINITY);
    return f;
}

__device__ __forceinline__ float hq_f(__half v) { return __half2float(v); }
__device__ __forceinline__ float hq_f(hdb_bf16 v) { return hdb_bf16_to_f(v); }
__device__ __forceinline__ float hq_f(float v) { return v; }

template <typename T> struct HqElem;
template <> struct HqElem<__half> { static constexpr int EPC = 8; };
template <> struct HqElem<hdb_bf16> { static constexpr int EPC = 8; };
template <> struct HqElem<float> { static constexpr int EPC = 4; };

__device__ __forceinline__ void hq_unpack(const uint4& raw, float (&x)[8], __half*) {
    const __half2* h = reinterpret_cast<const __half2*>(&raw);
#pragma unroll
    for (int i = 0; i < 4; ++i) { float2 f = __half22float2(h[i]); x[2 * i] = f.x; x[2 * i + 1] = f.y; }
}
// bfloat16 pairs in the order of hdb_scan.hip's hdb_unpack: the even element is the low half of its word, the odd one the high half
__device__ __forceinline__ void hq_unpack(const uint4& raw, float (&x)[8], hdb_bf16*) {
    const unsigned int w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { x[2 * i] = __uint_as_float(w[i] << 16); x[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u); }
}
__device__ __forceinline__ void hq_unpack(const uint4& raw, float (&x)[4], float*) {
    x[0] = __uint_as_float(raw.x); x[1] = __uint_as_float(raw.y);
    x[2] = __uint_as_float(raw.z); x[3] = __uint_as_float(raw.w);
}

// code of one element: rne(x / s) clamped to [-127, 127] (|x| <= 127 s up to the rounding of s), 0 for s == 0
__device__ __forceinline__ int hq_code(double x, float s) {
    if (!(s > 0.f)) return 0;
    double c = rint(x / (double)s);
    c = c > 127.0 ? 127.0 : (c < -127.0 ? -127.0 : c);
    return (int)c;
}

// ------------------------------------------------------------------------------------------------------------------------
// Row quantization: one wave per row.  codes[r][0..P) (zero past d), aux[r] = {s_r, E_r, T_r}; non-finite rows raise the
// index's NaN flag (1: a NaN, 2: an infinity), as hdb_rownorm_kernel does -- the quantized path is declined on such matrices.
// ------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void hdb_quant_rows_kernel(const T* V, int64_t n, int d, int P, int8_t* codes, float* aux,
                                                             int* nan_flag, double gamma) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t r = wave; r < n; r += nwaves) {
        const T* row = V + r * (int64_t)d;
        float amax = 0.f;
        double ss = 0.0;
        bool has_nan = false, has_inf = false;
        for (int e = lane; e < d; e += 64) {
            const float x = hq_f(row[e]);
            if (x != x) has_nan = true;
            else if (x - x != 0.f) has_inf = true;
            amax = fmaxf(amax, fabsf(x));
            ss += (double)x * (double)x;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { amax = fmaxf(amax, __shfl_xor(amax, o, 64)); ss += __shfl_xor(ss, o, 64); }
        const bool nanr = __ballot(has_nan) != 0ull, infr = __ballot(has_inf) != 0ull;
        const bool bad = nanr || infr;
        const float s = bad ? 0.f : amax / 127.f;
        double ee = 0.0, cc = 0.0;
        for (int e = lane; e < P; e += 64) {
            int c = 0;
            if (e < d && !bad) {
                const double x = (double)hq_f(row[e]);
                c = hq_code(x, s);
                const double eps = x - (double)s * (double)c;       // exact in float64: s has 24 bits, c 8
                ee += eps * eps;
                cc += (double)c * (double)c;
            }
            codes[r * (int64_t)P + e] = (int8_t)c;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { ee += __shfl_xor(ee, o, 64); cc += __shfl_xor(cc, o, 64); }
        if (lane == 0) {
            if (nanr) atomicOr(nan_flag, 1);
            else if (infr) atomicOr(nan_flag, 2);
            aux[3 * r + HDB_QROW_S] = s;
            aux[3 * r + HDB_QROW_E] = bad ? 0.f : hq_up(sqrt(ee) + gamma * sqrt(ss));
            aux[3 * r + HDB_QROW_T] = bad ? 0.f : hq_up((double)s * sqrt(cc));
        }
    }
}

// Compaction: codes and caches travel with their rows (hdb_index_gather).  One wave per kept row.
__global__ __launch_bounds__(256) void hdb_quant_gather_kernel(const int8_t* codes, const float* aux, const int64_t* rows, int64_t m,
                                                               int P, int8_t* codes_out, float* aux_out) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t j = wave; j < m; j += nwaves) {
        const int64_t r = rows[j];
        for (int c = lane * 16; c < P; c += 64 * 16)
            *reinterpret_cast<uint4*>(codes_out + j * (int64_t)P + c) = *reinterpret_cast<const uint4*>(codes + r * (int64_t)P + c);
        if (lane < 3) aux_out[3 * j + lane] = aux[3 * r + lane];
    }
}

// Quantized query prep: one wave per query (float32 queries).  qcodes[q][0..P), qaux[q] = {s_q, N_q, D_q, ||q||^2, bad}.
// Word 0 of `stat` (the largest candidate count of the call) is reset here, ahead of the finalize that raises it.
__global__ __launch_bounds__(64) void hdb_quant_qprep_kernel(const float* Q, int nq, int d, int P, int8_t* qcodes, float* qaux, int* stat,
                                                             uint32_t* pl_cnt) {
    const int q = blockIdx.x, lane = threadIdx.x;
    if (q >= nq) return;
    if (q == 0 && lane == 0 && stat) stat[0] = 0;
    if (q == 0 && lane == 0 && pl_cnt) pl_cnt[0] = 0u;     // no survivor of the 5-bit plane yet
    const float* qr = Q + (int64_t)q * d;
    float amax = 0.f;
    bool bad = false;
    for (int e = lane; e < d; e += 64) {
        const float x = qr[e];
        if (!(x - x == 0.f)) bad = true;
        amax = fmaxf(amax, fabsf(x));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    bad = __ballot(bad) != 0ull;
    const float s = bad ? 0.f : amax / 127.f;
    double nn = 0.0, dd = 0.0;
    int cs = 0, c2 = 0;                                     // sum c, sum c^2 (exact: at most 127^2 d < 2^31)
    for (int e = lane; e < P; e += 64) {
        int c = 0;
        if (e < d && !bad) {
            const double x = (double)qr[e];
            c = hq_code(x, s);
            const double del = x - (double)s * (double)c;
            nn += x * x;
            dd += del * del;
        }
        qcodes[(int64_t)q * P + e] = (int8_t)c;
        cs += c; c2 += c * c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nn += __shfl_xor(nn, o, 64); dd += __shfl_xor(dd, o, 64);
        cs += __shfl_xor(cs, o, 64); c2 += __shfl_xor(c2, o, 64);
    }
    if (lane == 0) {
        float* o = qaux + (int64_t)q * HDB_QQ_WORDS;
        const float sq = (float)nn;
        const bool big = !(sq - sq == 0.f);                 // ||q||^2 overflows float32: leave the query to the exact re-run
        o[HDB_QQ_S] = s;
        o[HDB_QQ_N] = bad ? 0.f : hq_up(sqrt(nn));
        o[HDB_QQ_D] = bad ? 0.f : hq_up(sqrt(dd));
        o[HDB_QQ_SQ] = sq;
        o[HDB_QQ_BAD] = (bad || big) ? 1.f : 0.f;
        o[HDB_QQ_CN] = hq_up(sqrt((double)c2));
        o[HDB_QQ_CS] = (float)cs;                           // |sum| <= 127 d < 2^24: exact
        o[7] = 0.f;
    }
}

// The same for the matrix-core flavour, and the whole query preparation of that call in ONE launch: 1/||q||, ||q||^2 and the NaN
// flags with hdb_qprep_kernel's own operations (same fma chain per lane, same butterfly: the cosine epilogue multiplies by these
// bits), the scaled fp16 copy q16 / qscl the matrix cores multiply with, and codes / norms of the ROUNDED query q' = q16 * qscl.
__global__ __launch_bounds__(64) void hdb_quant_qprep_m_kernel(const float* Q, int nq, int d, int P, float* qinv, float* qsq, int* qnan,
                                                               _Float16* q16, float* qscl, int8_t* qcodes, float* qaux, int* stat,
                                                               uint32_t* cnt_init, uint32_t* pl_cnt) {
    const int q = blockIdx.x, lane = threadIdx.x;
    if (q >= nq) return;
    if (q == 0 && lane == 0 && stat) stat[0] = 0;
    if (q == 0 && lane == 0 && pl_cnt) pl_cnt[0] = 0u;     // no survivor of the 5-bit plane yet
    if (lane == 0 && cnt_init) cnt_init[q * HDB_CNT_STRIDE] = 0u;     // an empty candidate list (the folded threshold has no kernel that would do it)
    const float* qr = Q + (int64_t)q * d;
    float s = 0.f, amax = 0.f;
    bool bad = false;
    for (int e = lane; e < d; e += 64) {
        const float x = qr[e];
        s = fma(x, x, s);
        amax = fmaxf(amax, fabsf(x));
        if (!(x - x == 0.f)) bad = true;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    const float scale = hdb_q16_scale(amax);
    const float inv_scale = 1.f / scale;
    float amax2 = 0.f;
    for (int e = lane; e < d; e += 64) {
        const _Float16 h = (_Float16)(qr[e] * scale);
        q16[(int64_t)q * d + e] = h;
        const float xr = (float)h * inv_scale;              // exact: a power of two
        if (!(xr - xr == 0.f)) bad = true;
        amax2 = fmaxf(amax2, fabsf(xr));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); amax2 = fmaxf(amax2, __shfl_xor(amax2, o, 64)); }
    bad = __ballot(bad) != 0ull;
    const float sq_ = bad ? 0.f : amax2 / 127.f;
    double nn = 0.0, dd = 0.0;
    int cs = 0, c2 = 0;                                     // sum c, sum c^2 (exact: at most 127^2 d < 2^31)
    for (int e = lane; e < P; e += 64) {
        int c = 0;
        if (e < d && !bad) {
            const double x = (double)((float)(_Float16)(qr[e] * scale) * inv_scale);
            c = hq_code(x, sq_);
            const double del = x - (double)sq_ * (double)c;
            nn += x * x;
            dd += del * del;
        }
        qcodes[(int64_t)q * P + e] = (int8_t)c;
        cs += c; c2 += c * c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nn += __shfl_xor(nn, o, 64); dd += __shfl_xor(dd, o, 64);
        cs += __shfl_xor(cs, o, 64); c2 += __shfl_xor(c2, o, 64);
    }
    if (lane == 0) {
        const float ss = s;
        qsq[q] = ss;
        qinv[q] = (s == 0.f) ? 1.0f : (float)(1.f / sqrt(s));
        qnan[q] = (ss != ss) ? 1 : (ss - ss != 0.f) ? 2 : 0;
        qscl[q] = inv_scale;
        float* o = qaux + (int64_t)q * HDB_QQ_WORDS;
        const float sq = (float)nn;
        const bool big = !(sq - sq == 0.f);
        o[HDB_QQ_S] = sq_;
        o[HDB_QQ_N] = bad ? 0.f : hq_up(sqrt(nn));
        o[HDB_QQ_D] = bad ? 0.f : hq_up(sqrt(dd));
        o[HDB_QQ_SQ] = sq;
        o[HDB_QQ_BAD] = (bad || big) ? 1.f : 0.f;
        o[HDB_QQ_CN] = hq_up(sqrt((double)c2));
        o[HDB_QQ_CS] = (float)cs;                           // |sum| <= 127 d < 2^24: exact
        o[7] = 0.f;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// int8 scan.  Tiling as hdb_scan_kernel: a wave covers 16 consecutive rows, lane group g = lane >> 4 owns rows 4g..4g+3 and its
// 16 lanes stride over the row's 16-byte pieces (non-temporal loads; the shadow is streamed once per call).  The NQ queries'
// codes sit in LDS; sums are exact int32 (v_dot4_i32_i8), so the 16-lane reduction may take any order.
// MODE 0: lower bounds of the sampled rows -> scores[q][ld];  MODE 1: rows whose upper bound reaches thr[q] -> candidate lists.
// NJ > 0: rows of at most NJ * 256 bytes, all loads of a tile issued before the first dot product; NJ == 0: any width.
// ------------------------------------------------------------------------------------------------------------------------
#define HQ_STAGE_CAP 128
struct HqStage {
    unsigned long long buf[4][HQ_STAGE_CAP];
    unsigned int cnt[4];
    unsigned int base;
};

__device__ __forceinline__ int hq_dpp_i(int x, int ctrl_id) {
    switch (ctrl_id) {
    case 0: return __builtin_amdgcn_update_dpp(0, x, HDB_DPP_MIRROR, 0xF, 0xF, false);
    case 1: return __builtin_amdgcn_update_dpp(0, x, HDB_DPP_HALF_MIRROR, 0xF, 0xF, false);
    case 2: return __builtin_amdgcn_update_dpp(0, x, HDB_DPP_XOR2, 0xF, 0xF, false);
    default: return __builtin_amdgcn_update_dpp(0, x, HDB_DPP_XOR1, 0xF, 0xF, false);
    }
}
// hdb_rows4_sum for int32 partial sums: on return lane l16 holds the sum of row hdb_owned_row(l16) of its group
__device__ __forceinline__ int hq_rows4_sum(int a0, int a1, int a2, int a3, int l16) {
    const bool b3 = (l16 & 8) != 0, b2 = (l16 & 4) != 0;
    const int v01 = (b3 ? a1 : a0) + hq_dpp_i(b3 ? a0 : a1, 0);
    const int v23 = (b3 ? a3 : a2) + hq_dpp_i(b3 ? a2 : a3, 0);
    int w = (b2 ? v23 : v01) + hq_dpp_i(b2 ? v01 : v23, 1);
    w += hq_dpp_i(w, 2);
    w += hq_dpp_i(w, 3);
    return w;
}

// The threshold folded into the passes (QuantArgs::nsub > 0), every thread of a 256-thread workgroup calls it.  Every workgroup of
// the filter pass runs it at its head with no load of the stream in flight, so the 32 wave maxima are DPP reductions
// (hdb_wave_max_dpp: a scalar, no LDS crossbar) and the owner of a maximum is found by comparing with that scalar:
template <int NQ>
__device__ __forceinline__ void hq_fold_thr(const QuantArgs& a, float (&q_thr)[NQ]) {
    // T_s = 16th largest of the per-wave maxima of the sample pass: every wave extracts the 16 largest of its quarter, wave 0
    // the 16 largest of those 64 (hdb_sample_thr_kernel's scheme; exact for the nsub keys)
    __shared__ uint32_t s_top[4 * 16];
    __shared__ float s_thr[NQ];
    const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int q = 0; q < NQ; ++q) {
        uint32_t c[HDB_QUANT_NSUB_MAX / 256];
#pragma unroll
        for (int j = 0; j < HDB_QUANT_NSUB_MAX / 256; ++j) {
            const int e = (int)threadIdx.x + 256 * j;
            c[j] = e < a.nsub ? a.wmax[(int64_t)q * a.nsub + e] : 0u;
        }
        for (int r = 0; r < 16; ++r) {
            uint32_t lm = 0u;
#pragma unroll
            for (int j = 0; j < HDB_QUANT_NSUB_MAX / 256; ++j) lm = max(lm, c[j]);
            const uint32_t wm = hdb_wave_max_dpp(lm);        // (scalar: DPP inside the rows, v_readlane across them -- no LDS crossbar)
            const unsigned long long who = __ballot(lm == wm);
            if (ln == (int)__ffsll((long long)who) - 1) {
                bool gone = false;
#pragma unroll
                for (int j = 0; j < HDB_QUANT_NSUB_MAX / 256; ++j)
                    if (!gone && c[j] == wm) { c[j] = 0u; gone = true; }
            }
            if (ln == 0) s_top[wv * 16 + r] = wm;
        }
        __syncthreads();
        if (wv == 0) {
            uint32_t v = s_top[ln];
            uint32_t kth = 0u;
            for (int r = 0; r < 16; ++r) {
                const uint32_t wm = hdb_wave_max_dpp(v);
                const unsigned long long who = __ballot(v == wm);
                if (ln == (int)__ffsll((long long)who) - 1) v = 0u;
                kth = wm;
            }
            if (ln == 0) {
                const float t = kth == 0u ? -INFINITY : hdb_key2f(kth);
                s_thr[q] = t;
                if (blockIdx.x == 0) a.thr_out[q] = t;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) q_thr[q] = s_thr[q];
}

// What the scan needs of its NQ queries (the quantized query prep's record, 1/||q|| for cosine).
template <int NQ>
struct HqQuery {
    float s[NQ], n[NQ], d[NQ], sq[NQ], inv[NQ];
    bool bad[NQ];
};
template <int NQ>
__device__ __forceinline__ void hq_query_load(const QuantArgs& a, HqQuery<NQ>& qc) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const float* o = a.qaux + (int64_t)q * HDB_QQ_WORDS;
        qc.s[q] = o[HDB_QQ_S]; qc.n[q] = o[HDB_QQ_N]; qc.d[q] = o[HDB_QQ_D]; qc.sq[q] = o[HDB_QQ_SQ]; qc.bad[q] = o[HDB_QQ_BAD] != 0.f;
        qc.inv[q] = a.metric == HDB_COSINE ? a.qinv[q] : 1.f;
    }
}

// One group of four rows rr[0..3] (a.n or more: no row) through the int8 evaluation, called by the 16 lanes of the group: the code
// loads, the v_dot4 sums against the NQ queries in LDS (qs[q * nch + piece]), hq_rows4_sum, and in the lane that then owns a row
// (`row` = rr[hdb_owned_row(l16)]; the function returns whether that is a row of the matrix) the row terms and the bounds lo <= score <= hi
// of the header -- -inf both for a masked row or a query the prep declined -- handed to sink(q, lo, hi, masked) query by query, so that
// no caller holds NQ pairs of bounds at once (the dense kernels keep the parent's registers that way).  The dense passes (hdb_quant_scan_kernel) and the pass over
// the 5-bit plane (hdb_quant_plane_scan_kernel, for the rows it keeps) both call it, and the candidate set must not depend on which:
// the float arithmetic is compiled with contraction OFF, so both instantiations round after every multiply and every add and give
// the same bits (G, the 16-byte pieces of a row in flight per lane, only orders exact int32 sums).  That is one of the evaluations F(A) the plane's derivation (header, "The 5-bit plane") covers -- it holds for
// whatever the compiler contracts, the uncontracted form included -- so hi5 >= hi stands as derived there.
template <int NQ, int NJ, int G, typename Sink>
__device__ __forceinline__ bool hq_rows4_bounds(const QuantArgs& a, const int4* qs, const HqQuery<NQ>& qc, const int64_t (&rr)[4], int l16,
                                                int64_t row, Sink&& sink) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const int nch = a.P >> 4;
    const int nj = NJ > 0 ? NJ : (nch + 15) >> 4;
    const int8_t* p[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) p[u] = a.codes + min(rr[u], a.n - 1) * (int64_t)a.P;
    int acc[4][NQ];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[u][q] = 0;
    for (int j0 = 0; j0 < nj; j0 += G) {
        uint4 raw[G][4];
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const int c = l16 + 16 * (j0 + j);
            const bool live = (j0 + j) < nj && c < nch;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (live) {
                    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p[u] + (int64_t)c * 16));
                    raw[j][u] = make_uint4(v.x, v.y, v.z, v.w);
                } else {
                    raw[j][u] = make_uint4(0u, 0u, 0u, 0u);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);           // loads ahead of every use
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const int c = l16 + 16 * (j0 + j);
            const int cc = c < nch ? c : 0;          // (dead pieces are zero: any query piece gives 0)
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int4 qv = qs[q * nch + cc];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    int s = acc[u][q];
                    s = __builtin_amdgcn_sdot4((int)raw[j][u].x, qv.x, s, false);
                    s = __builtin_amdgcn_sdot4((int)raw[j][u].y, qv.y, s, false);
                    s = __builtin_amdgcn_sdot4((int)raw[j][u].z, qv.z, s, false);
                    s = __builtin_amdgcn_sdot4((int)raw[j][u].w, qv.w, s, false);
                    acc[u][q] = s;
                }
            }
        }
    }
    int C[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) C[q] = hq_rows4_sum(acc[0][q], acc[1][q], acc[2][q], acc[3][q], l16);
    if ((l16 & 3) != 0 || row >= a.n) return false;
    const float s_r = a.aux[3 * row + HDB_QROW_S], e_r = a.aux[3 * row + HDB_QROW_E], t_r = a.aux[3 * row + HDB_QROW_T];
    const bool masked = a.mask && !a.mask[row];
    const float bias = a.bias ? a.bias[row] : 0.f;
    const float invn = a.metric == HDB_COSINE ? a.inv_norm[row] : 1.f;
    const float sqv = a.metric == HDB_EUCLIDEAN ? a.sqnorm[row] : 0.f;
    {
#pragma clang fp contract(off)
        const float absmin = 0x1p-100f * (float)(a.d + 8);
        const float g2 = 2.f * a.gamma;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            float lo = -INFINITY, hi = -INFINITY;
            if (!qc.bad[q] && !masked) {
                const float A = (qc.s[q] * s_r) * (float)C[q];
                const float aA = fabsf(A);
                const float B = (qc.n[q] * e_r + qc.d[q] * t_r) * (1.f + 0x1p-10f) + aA * 0x1p-10f + absmin;
                float l, h;
                if (a.metric == HDB_EUCLIDEAN) {
                    const float ctr = sqv + qc.sq[q] - 2.f * A;
                    const float err = g2 * sqv + 2.f * B + 0x1p-10f * (sqv + qc.sq[q] + 2.f * aA) + absmin;
                    const float elo = fmaxf(ctr - err, 0.f) * (1.f - g2 - 0x1p-10f);
                    const float ehi = (ctr + err) * (1.f + g2 + 0x1p-10f);
                    h = (float)(1.f / (1.f + sqrt(elo)));
                    l = (float)(1.f / (1.f + sqrt(ehi)));
                } else {
                    l = A - B; h = A + B;
                    if (a.metric == HDB_COSINE) { l = l * invn * qc.inv[q]; h = h * invn * qc.inv[q]; }
                }
                if (a.bias) { l += bias; h += bias; }
                l = l - fabsf(l) * 0x1p-20f - 1e-30f;
                h = h + fabsf(h) * 0x1p-20f + 1e-30f;
                if (l != l) l = -INFINITY;
                if (h != h) h = INFINITY;
                lo = l; hi = h;
            }
            sink(q, lo, hi, masked);
        }
    }
    return true;
}

// The argument block where the launch left it, in the kernarg segment.  QuantArgs MUST stay the first (and only) parameter of every
// kernel that reaches this function -- hdb_quant_scan_kernel and hdb_quant_plane_scan_kernel -- so that it lies at offset 0: a
// parameter put in front of it would make this read something else without a compiler error.  Code that runs rarely -- a stage that is full, a drain of the plane pass, the flush -- reads its fields through this
// reference when it gets there, so that the streaming loop around it does not hold two dozen pointers in registers for it.  The
// empty asm keeps the loads from being moved back in front of the loop.
__device__ __forceinline__ const QuantArgs& hq_args_in_memory() {
    typedef const __attribute__((address_space(4))) QuantArgs* ArgPtr;
    const uint64_t v = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    asm volatile("" : "+v"(lo), "+v"(hi));
    lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo); hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)hi);      // (scalar again: scalar loads)
    return *(const QuantArgs*)(ArgPtr)(((uint64_t)hi << 32) | lo);
}

// Matrix-core flavour (a.G non-null): candidate `row` of list slot `slot` goes to row `slot` of the compact matrix, its 1/||v|| and
// bias beside it -- the bias as the matrix-core scan takes it, the row mask folded in (hdb_maskbias_kernel).  The lanes `l` of `nl`
// share the row's 16-byte pieces.  Slots past a query's count are left as they are: the MODE 0 launch scores them too (its grid is
// set by the host, which does not know the counts) and nobody reads those scores.
__device__ __forceinline__ void hq_copy_row(const QuantArgs& a, int64_t slot, uint32_t row, int l, int nl) {
    const char* src = a.V + (int64_t)row * a.row_bytes;
    char* dst = a.G + slot * a.row_bytes;
    for (int c = l * 16; c < a.row_bytes; c += nl * 16) *reinterpret_cast<uint4*>(dst + c) = *reinterpret_cast<const uint4*>(src + c);
    if (l == 0) {
        if (a.ginv) a.ginv[slot] = a.inv_norm[row];
        if (a.gbias) a.gbias[slot] = a.mask ? (a.mask[row] ? (a.bias ? a.bias[row] : 0.f) : -INFINITY) : a.bias[row];
    }
}
// A row whose upper bound reaches the threshold of query q: into the workgroup's stage, or straight to the list when that is full.
__device__ __forceinline__ void hq_emit(HqStage& stage, int q, float hi, int64_t row) {
    const unsigned long long ent = hdb_pack(hi, (uint32_t)row);
    const unsigned int lp = atomicAdd(&stage.cnt[q], 1u);                    // LDS
    if (lp < HQ_STAGE_CAP) stage.buf[q][lp] = ent;
    else {
        const QuantArgs& a = hq_args_in_memory();
        const uint32_t pos = atomicAdd(&a.cnt[q * HDB_CNT_STRIDE], 1u);      // the stage is full: straight to the list
        if (pos < a.cap) {
            a.cand[(int64_t)q * a.cap + pos] = ent;
            if (a.G) hq_copy_row(a, (int64_t)q * a.cap + pos, (uint32_t)row, 0, 1);
        }
    }
}
// The stage to the lists: one atomic per workgroup and query (hdb_stage_flush), then one wave per entry for the row copies.
template <int NQ>
__device__ __forceinline__ void hq_stage_flush(HqStage& stage) {
    __syncthreads();
    const QuantArgs& a = hq_args_in_memory();
    for (int q = 0; q < NQ; ++q) {
        const unsigned int have = min(stage.cnt[q], (unsigned int)HQ_STAGE_CAP);
        if (have == 0u) continue;
        if (threadIdx.x == 0) stage.base = atomicAdd(&a.cnt[q * HDB_CNT_STRIDE], have);
        __syncthreads();
        const unsigned int base = stage.base;
        for (unsigned int e = threadIdx.x; e < have; e += blockDim.x)
            if (base + e < a.cap) a.cand[(int64_t)q * a.cap + base + e] = stage.buf[q][e];
        if (a.G)
            for (unsigned int e = threadIdx.x >> 6; e < have; e += blockDim.x >> 6)
                if (base + e < a.cap)
                    hq_copy_row(a, (int64_t)q * a.cap + base + e, 0xFFFFFFFFu - (uint32_t)(stage.buf[q][e] & 0xFFFFFFFFull), threadIdx.x & 63, 64);
        __syncthreads();
    }
}

// MODE 0: lower bounds of the sampled rows -> scores[q][ld], or (nsub > 0) the per-wave maxima -> wmax, and for one query ahead of the
// plane pass (pl_hi non-null) their upper bounds -> pl_hi[sample slot];  MODE 1: rows whose upper bound
// reaches the threshold (thr[q], or nsub > 0: folded, hq_fold_thr) -> candidate lists;  MODE 2 (tests): MODE 1's upper bound of every
// row -> dbg[row], nothing emitted.
// (QuantArgs stays the first parameter: hq_args_in_memory.)
template <int MODE, int NQ, int NJ>
__global__ __launch_bounds__(256) void hdb_quant_scan_kernel(QuantArgs a) {
    static_assert(sizeof(QuantArgs) % 8 == 0, "the argument block is read back from the kernarg segment as laid out here");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int4* qs = reinterpret_cast<int4*>(smem);                       // [NQ][nch]
    __shared__ HqStage stage;
    const int nch = a.P >> 4;
    if (MODE == 1 && threadIdx.x < 4) stage.cnt[threadIdx.x] = 0u;
    for (int i = threadIdx.x; i < NQ * nch; i += 256) qs[i] = reinterpret_cast<const int4*>(a.qcodes)[i];
    HqQuery<NQ> qc;
    hq_query_load<NQ>(a, qc);
    float q_thr[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) q_thr[q] = (MODE == 1 && a.nsub == 0) ? a.thr[q] : 0.f;
    __syncthreads();
    if (MODE == 1 && a.nsub > 0) hq_fold_thr<NQ>(a, q_thr);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, l16 = lane & 15;
    uint32_t wbest[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) wbest[q] = 0u;

    const int64_t ntiles = a.ntiles;
    for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < ntiles; t += (int64_t)gridDim.x * 4) {
        const int64_t r0 = hdb_tile_index(t, a.tile_stride) * 16 + 4 * g;
        const int64_t rr[4] = {r0, r0 + 1, r0 + 2, r0 + 3};
        const int u_own = hdb_owned_row(l16);
        const int64_t row = r0 + u_own;
        const int64_t out_i = t * 16 + 4 * g + u_own;
        const bool live = hq_rows4_bounds<NQ, NJ, (NJ > 0 ? NJ : 2)>(a, qs, qc, rr, l16, row, [&](int q, float lo, float hi, bool masked) {
            if (MODE == 2) {
                a.dbg[row] = hi;
            } else if (MODE == 0) {
                if (a.nsub > 0) wbest[q] = max(wbest[q], hdb_f2key(lo));
                else a.scores[(int64_t)q * a.ld + out_i] = lo;
                if (NQ == 1 && a.pl_hi) a.pl_hi[out_i] = hi;          // (pass 1 over the plane takes the sampled rows from here)
            } else if (!masked && !qc.bad[q] && hi >= q_thr[q]) {
                hq_emit(stage, q, hi, row);
            }
        });
        if (MODE == 0 && a.nsub == 0 && !live && (l16 & 3) == 0)
#pragma unroll
            for (int q = 0; q < NQ; ++q) a.scores[(int64_t)q * a.ld + out_i] = -INFINITY;
        if (MODE == 0 && NQ == 1 && a.pl_hi && !live && (l16 & 3) == 0) a.pl_hi[out_i] = -INFINITY;
    }
    if (MODE == 0 && a.nsub > 0) {                       // (every wave of the grid writes its slot: a wave without tiles writes 0)
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            uint32_t wm = wbest[q];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) wm = max(wm, (uint32_t)__shfl_xor((int)wm, o, 64));
            if (lane == 0) a.wmax[(int64_t)q * a.nsub + blockIdx.x * 4 + wave] = wm;
        }
    }
    if (MODE == 1) hq_stage_flush<NQ>(stage);
}

// ------------------------------------------------------------------------------------------------------------------------
// The 5-bit plane.  Derivation from the codes of the 16-row tiles [t0, t1), rows below n: a wave per tile, four rows at a time, 16
// lanes per row; lane l16 packs unit l16 (32 elements: one 16-byte piece of nibbles, one word of bits), the group sums the squared
// residuals of the elements below d.  Lanes 0-15 then hold one row of the tile each and write its two hot blocks (hdb_caps.h): the
// maxima E*, T*, F* are tile state, so a tile is always derived whole, from all of its rows (plane_rows, hdb_api.hip, rounds to
// tiles), and the rows at or beyond n take no part in them.  inv_norm must hold the tile's rows already.
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hdb_quant_plane_rows_kernel(const int8_t* codes, const float* aux, const float* inv_norm, int64_t t0,
                                                                   int64_t t1, int64_t n, int d, int P, int U, uint8_t* nib,
                                                                   uint32_t* bitw, float* rec) {
    const int lane = threadIdx.x & 63, g = lane >> 4, l16 = lane & 15;
    const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t t = t0 + wave; t < t1; t += nwaves) {                       // (wave-uniform)
        int ssr[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int64_t r = t * 16 + 4 * it + g;
            int ss = 0;
            if (r < n && l16 < U) {
                const int8_t* src = codes + r * (int64_t)P + 32 * l16;
                uint4 raw[2];
                raw[0] = *reinterpret_cast<const uint4*>(src);
                raw[1] = (32 * l16 + 16 < P) ? *reinterpret_cast<const uint4*>(src + 16) : make_uint4(0u, 0u, 0u, 0u);
                const uint32_t* cw = reinterpret_cast<const uint32_t*>(raw);      // query-aligned words: word w holds elements 4w .. 4w + 3
                uint32_t nw[4] = {0u, 0u, 0u, 0u}, bw = 0u;
#pragma unroll
                for (int w = 0; w < 8; ++w) {
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int c = (int)(int8_t)((cw[w] >> (8 * b)) & 0xFFu);
                        const int h = c >> 3;
                        const uint32_t u5 = (uint32_t)(h + 16);
                        const int rho = c - (8 * h + 4);
                        if (32 * l16 + 4 * w + b < d) ss += rho * rho;
                        nw[w >> 1] |= (u5 >> 1) << (8 * b + 4 * (w & 1));
                        bw |= (u5 & 1u) << (8 * b + w);
                    }
                }
                *reinterpret_cast<uint4*>(nib + (r * (int64_t)U + l16) * 16) = make_uint4(nw[0], nw[1], nw[2], nw[3]);
                bitw[r * (int64_t)U + l16] = bw;
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
            ssr[it] = ss;                                                    // (every lane of group g: row 4 it + g; at most 16 d, exact)
        }
        // lane e < 16 takes row e = 4 it + g of the tile from group g = e & 3, pass it = e >> 2
        int ss = 0;
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int v = __shfl(ssr[it], 16 * (lane & 3), 64);
            if (((lane >> 2) & 3) == it) ss = v;
        }
        const int64_t r = t * 16 + l16;
        const bool valid = lane < 16 && r < n;
        const double absmin = 0x1p-100 * (double)(d + 8);
        double kd = 0.0, kc = 0.0;
        float ed = 0.f, td = 0.f, fd = 0.f, ec = 0.f, tc = 0.f, fc = 0.f;
        uint32_t rcode = 0u;
        if (valid) {
            const float s = aux[3 * r + HDB_QROW_S], e = aux[3 * r + HDB_QROW_E], tt = aux[3 * r + HDB_QROW_T];
            const double inv = (double)inv_norm[r];
            kd = (double)s; kc = (double)s * inv;                            // (products of two float32 numbers: exact in float64)
            ed = e; td = tt; fd = hdb_plane_up(absmin);
            ec = hdb_plane_up((double)e * inv); tc = hdb_plane_up((double)tt * inv); fc = hdb_plane_up(absmin * inv * (1.0 + 0x1p-40));
            rcode = hdb_plane_rc_encode((uint32_t)ss);
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {                                    // (a NaN of a non-finite row is dropped or kept: such an index takes no quantized call)
            ed = fmaxf(ed, __shfl_xor(ed, o, 64)); td = fmaxf(td, __shfl_xor(td, o, 64)); fd = fmaxf(fd, __shfl_xor(fd, o, 64));
            ec = fmaxf(ec, __shfl_xor(ec, o, 64)); tc = fmaxf(tc, __shfl_xor(tc, o, 64)); fc = fmaxf(fc, __shfl_xor(fc, o, 64));
        }
        if (lane < 16) {
            char* tile = reinterpret_cast<char*>(rec) + hdb_plane_block_off(t, 0);
#pragma unroll
            for (int fl = 0; fl < 2; ++fl) {
                char* blk = tile + fl * HDB_PLANE_BLOCK_BYTES;
                reinterpret_cast<uint16_t*>(blk + HDB_PLANE_BLOCK_K)[l16] = hdb_plane_k_encode(fl == HDB_PLANE_BLOCK_COSINE ? kc : kd);
                reinterpret_cast<uint8_t*>(blk + HDB_PLANE_BLOCK_RC)[l16] = (uint8_t)rcode;
                if (l16 == 0)
                    *reinterpret_cast<float4*>(blk + HDB_PLANE_BLOCK_TILE) =
                        fl == HDB_PLANE_BLOCK_COSINE ? make_float4(ec, tc, fc, 0.f) : make_float4(ed, td, fd, 0.f);
            }
            if (l16 < 8) *reinterpret_cast<uint4*>(tile + 2 * HDB_PLANE_BLOCK_BYTES + 16 * l16) = make_uint4(0u, 0u, 0u, 0u);      // reserved
        }
    }
}

// Pass 1: the coarse upper bound hi5 (header, "The 5-bit plane") of every row; a row with hi5 >= T_s is finished here, by the wave
// that found it.
// A wave takes two 16-row tiles per step.  A tile of the nibble plane is 16 U contiguous 16-byte pieces and lane l takes pieces
// l + 64 j, j < J = ceil(U / 4), i.e. whole-wave contiguous loads with every lane busy (U = 12 at d = 384: exactly 3 per lane); piece
// f belongs to row f / U, unit f % U -- the same for every tile, so a lane keeps one LDS offset per j and reads the eight query words
// of a unit from qs as it decodes that piece (the words themselves, 8 J registers held through the loop, cost J = 3 two waves per
// SIMD and J = 2, 4 one: profiles/plane_occupancy_kernel_resources.txt; the pass is no slower for the LDS reads at any grid and needs
// no reload after a drain: profiles/plane_occupancy_time.txt, "Attribution").
// The per-piece sums meet in LDS (wave-private), lanes 0-31 add the U pieces of one row each and evaluate the bound.
// Survivors wait in a wave-private queue of row numbers (LDS; appended by ballot and popcount, no atomics).  Once it holds 16 the wave
// takes 16 of them as one MODE 1 tile -- 16 lanes per 4 rows, hq_rows4_bounds with the row numbers from the queue -- and emits the
// candidates through the workgroup's stage exactly as MODE 1 does; what is left after the last step goes as a ragged tile (empty
// slots: "no row" = a.n).  The gather's latency chain (row number -> code row -> row terms) hides behind the other waves' streams.
// A step appends at most 32 rows to fewer than 16, and a drain leaves fewer than 16: 48 entries per wave.
// Behind the stream the wave takes its share of the sampled rows from the list of the sample pass, 32 at a time into the same queue.
// (96 scalar registers: the drain's nest of branches and its argument loads would otherwise take the kernel past 96, which costs the
//  narrow widths a wave per SIMD; with the cap the allocator keeps a handful of scalars in vector lanes around the drain instead.
//  QuantArgs stays the first parameter: hq_args_in_memory.  The empty asm statements here and in the drain only steer the register
//  allocator; the figures they buy are in profiles/quant_inpass_kernel_resources.txt with the compiler they were taken with.)
#define HQ_PL_QUEUE 48
template <int J, bool DBG>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(96))) void hdb_quant_plane_scan_kernel(QuantArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int4* qs = reinterpret_cast<int4*>(smem);                       // [2 U] query codes, zero past P: MODE 1's layout for one query
    __shared__ int part[4][2][64 * J];
    __shared__ HqStage stage;
    __shared__ uint32_t queue[4][HQ_PL_QUEUE];
    __shared__ uint32_t surv_cnt;
    const int U = a.pl_units, nch = a.P >> 4;
    if (threadIdx.x < 4) stage.cnt[threadIdx.x] = 0u;
    if (threadIdx.x == 0) surv_cnt = 0u;
    for (int i = threadIdx.x; i < 2 * U; i += 256) qs[i] = i < nch ? reinterpret_cast<const int4*>(a.qcodes)[i] : make_int4(0, 0, 0, 0);
    const float* qo = a.qaux;
    const float q_s = qo[HDB_QQ_S], q_n = qo[HDB_QQ_N], q_d = qo[HDB_QQ_D], q_cn = qo[HDB_QQ_CN];
    const int q_cs = (int)qo[HDB_QQ_CS];
    const bool q_bad = qo[HDB_QQ_BAD] != 0.f;
    const bool cosine = a.metric == HDB_COSINE;
    const float q_inv = cosine ? a.qinv[0] : 1.f;
    float thr1[1] = {(!DBG && a.nsub == 0) ? a.thr[0] : 0.f};
    __syncthreads();
    if (!DBG && a.nsub > 0) hq_fold_thr<1>(a, thr1);
    const float q_thr = thr1[0];

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // (the tile number stays scalar)
    const int npieces = 16 * U;
    // where the query words of piece lane + 64 j lie in qs: the decode reads them there, piece by piece, and holds one offset per j
    int qoff[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int f = lane + 64 * j;
        qoff[j] = f < npieces ? 2 * (f % U) : 0;
    }
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    typedef float f32x3 __attribute__((ext_vector_type(3)));
    const int64_t ntiles = a.ntiles;
    const int et = lane >> 4, er = lane & 15;                       // epilogue lanes 0-31: tile et of the pair, row er
    int qn = 0;                                                     // rows in this wave's queue (wave-uniform)
    uint32_t nsurv = 0u;                                            // rows this wave kept (wave-uniform)
    // `m` queued rows from entry `base` on as one MODE 1 tile (m <= 16)
    auto drain = [&](int base, int m) {
        const QuantArgs& a = hq_args_in_memory();
        HqQuery<1> qc;
        qc.s[0] = q_s; qc.n[0] = q_n; qc.d[0] = q_d; qc.sq[0] = 0.f; qc.inv[0] = q_inv; qc.bad[0] = q_bad;      // (dot / cosine: no ||q||^2)
        int ln = lane;
        asm volatile("" : "+v"(ln));                     // (nothing of the tile is computed ahead of the loop and held through the stream)
        const int g = ln >> 4, l16 = ln & 15;
        int64_t rr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) rr[u] = 4 * g + u < m ? (int64_t)queue[wave][base + 4 * g + u] : a.n;
        const int own = 4 * g + hdb_owned_row(l16);
        const int64_t row = own < m ? (int64_t)queue[wave][base + own] : a.n;
        hq_rows4_bounds<1, 0, 1>(a, qs, qc, rr, l16, row, [&](int, float, float hi, bool masked) {     // (one piece in flight: few registers)
            if (!masked && !q_bad && hi >= q_thr) hq_emit(stage, 0, hi, row);
        });
    };

    // The walk: position tp of the tiles the sample pass did not take (hdb_caps.h; DBG, or no list: every tile), two positions per
    // step.  The two tiles of a step need not be adjacent -- a sampled tile may lie between them -- so every address and every
    // epilogue row comes from the mapped tile number tl[tt] (scalar; ntiles: no tile).
    const uint32_t s_tiles = DBG ? 0u : a.pl_s_tiles, s_stride = DBG ? 1u : a.pl_s_stride;
    const uint32_t nwalk = hdb_plane_skip_count((uint32_t)ntiles, s_tiles);
    const uint32_t tp0 = ((uint32_t)blockIdx.x * 4u + (uint32_t)wave) * 2u;
    const HdbSkipStep sk_step = hdb_plane_skip_step((uint32_t)gridDim.x * 8u, s_stride), sk_next = {0u, 1u, 1u};
    HdbSkipPos pos = hdb_plane_skip_start(tp0 < nwalk ? tp0 : 0u, s_tiles, s_stride);
    for (uint32_t tp = tp0; tp < nwalk; tp += (uint32_t)gridDim.x * 8u, hdb_plane_skip_advance(pos, sk_step, s_tiles, s_stride)) {
        int64_t tl[2];
        {
            HdbSkipPos p1 = pos;
            hdb_plane_skip_advance(p1, sk_next, s_tiles, s_stride);
            tl[0] = hdb_plane_skip_tile(pos, s_tiles, s_stride);
            tl[1] = tp + 1u < nwalk ? hdb_plane_skip_tile(p1, s_tiles, s_stride) : ntiles;
        }
        u32x4 nv[2][J];
        uint32_t bv[2][J];
        int ln = lane;
        asm volatile("" : "+v"(ln));                     // (piece numbers and lane offsets are formed per step, from one register held across steps)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            // pieces of this tile's own rows: 0 past the last tile, the ragged tile loads its rows only (piece f is of row f / U)
            const int pieces_left = (int)min((int64_t)16, max((int64_t)0, a.n - tl[tt] * 16)) * U;
            const uint8_t* nb = a.pl_nib + tl[tt] * (int64_t)npieces * 16;
            const uint32_t* bb = a.pl_bit + tl[tt] * (int64_t)npieces;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                if (ln < pieces_left - 64 * j) {
                    nv[tt][j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(nb + (uint32_t)ln * 16u) + 64 * j);     // (piece ln + 64 j: scalar base, 32-bit lane offset)
                    bv[tt][j] = __builtin_nontemporal_load(bb + (uint32_t)ln + 64 * j);
                } else {
                    nv[tt][j] = u32x4{0u, 0u, 0u, 0u};
                    bv[tt][j] = 0u;
                }
            }
        }
        // the row terms of the epilogue lanes, issued with the plane loads
        const int64_t row = (et ? tl[1] : tl[0]) * 16 + er;
        const bool rvalid = lane < 32 && row < a.n;      // (no tile: row = 16 ntiles >= n)
        // (the hot block of the lane's tile, hdb_caps.h: its own k_hi and rc, and the tile's {E*, T*, F*, 0} -- 64 bytes per tile)
        f32x3 tm = f32x3{0.f, 0.f, 0.f};                 // (three words, not the block's four: a fourth register nobody reads is reused at once, and that write waits for every load in flight)
        uint32_t kcode = 0u, rcode = 0u;
        float bias = 0.f;
        bool masked = false;
        if (rvalid) {
            const char* blk = reinterpret_cast<const char*>(a.pl_rec) + hdb_plane_block_off(et ? tl[1] : tl[0], cosine ? HDB_PLANE_BLOCK_COSINE : HDB_PLANE_BLOCK_DOT);
            // (plain loads: the three pieces of a lane, and the 16 lanes of a tile, share one 64-byte block, and the streaming hint on them
            //  cost the headline 13 us against these -- profiles/plane_block_time.txt, "variant")
            kcode = reinterpret_cast<const uint16_t*>(blk + HDB_PLANE_BLOCK_K)[er];
            rcode = reinterpret_cast<const uint8_t*>(blk + HDB_PLANE_BLOCK_RC)[er];
            tm = *reinterpret_cast<const f32x3*>(blk + HDB_PLANE_BLOCK_TILE);
            if (a.bias) bias = a.bias[row];
            if (a.mask) masked = !a.mask[row];
        }
        __builtin_amdgcn_sched_barrier(0);               // loads ahead of every use
        // piece j of both tiles against the eight query words of its unit, read from qs (two 16-byte LDS reads per j, in flight with
        // nothing but themselves: the barrier keeps the words of the next j from being read, and held, ahead of their piece)
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int4 x = qs[qoff[j]], y = qs[qoff[j] + 1];
            const int qw[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                const uint32_t bw = bv[tt][j];
                const uint32_t w4[4] = {nv[tt][j].x, nv[tt][j].y, nv[tt][j].z, nv[tt][j].w};
                int s = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint32_t lo = ((w4[i] << 1) & 0x1E1E1E1Eu) | ((bw >> (2 * i)) & 0x01010101u);
                    const uint32_t hi = ((w4[i] >> 3) & 0x1E1E1E1Eu) | ((bw >> (2 * i + 1)) & 0x01010101u);
                    s = __builtin_amdgcn_sdot4((int)lo, qw[2 * i], s, false);
                    s = __builtin_amdgcn_sdot4((int)hi, qw[2 * i + 1], s, false);
                }
                part[wave][tt][lane + 64 * j] = s;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        int S = 0;
        if (lane < 32)
            for (int i = 0; i < U; ++i) S += part[wave][et][er * U + i];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                 // (the next step's stores stay behind these loads)
        float hi5 = -INFINITY;
        const bool dead = !rvalid || masked || q_bad;
        if (!dead) {
            const float fc = (float)(8 * S - 124 * q_cs);
            const float Uf = q_cn * hdb_plane_rc_decode(rcode);
            float ch = fc + Uf, cl = fc - Uf;
            ch = ch + (fabsf(ch) * 0x1p-20f + 1.f);
            cl = cl - (fabsf(cl) * 0x1p-20f + 1.f);
            const float k_hi = hdb_plane_k_hi(kcode), k_lo = hdb_plane_k_lo(k_hi);
            float k_up = q_s * k_hi, k_dn = q_s * k_lo;
            k_up = k_up + k_up * 0x1p-20f;
            k_dn = k_dn - k_dn * 0x1p-20f;
            const float A5 = (ch >= 0.f ? k_up : k_dn) * ch, Al = (cl >= 0.f ? k_dn : k_up) * cl;
            const float Amax = fmaxf(fabsf(A5), fabsf(Al));
            const float c0 = (q_n * tm.x + q_d * tm.y) * (1.f + 0x1p-10f);
            const float B5 = c0 + fabsf(A5) * 0x1p-10f + tm.z;
            const float Bmax = c0 + Amax * 0x1p-10f + tm.z;
            const float Mx = Amax + Bmax;
            float X = (A5 + B5) + (Mx * 0x1p-18f + 1e-30f);
            float mM = Mx * (1.f + 0x1p-17f);
            if (cosine) { X = X * q_inv; mM = mM * q_inv; }            // (1 / ||v_r|| is in k_hi, E*, T*, F* already)
            const float Z = mM + fabsf(bias);
            float h = X;
            if (a.bias) h += bias;
            hi5 = h + (Z * 0x1p-18f + 4e-30f);
            if (hi5 != hi5) hi5 = INFINITY;
        }
        if (DBG) {
            if (rvalid) a.dbg[row] = hi5;
            continue;
        }
        const bool keep = !dead && !(hi5 < q_thr);
        const unsigned long long km = __ballot(keep);
        if (km == 0ull) continue;                        // (wave-uniform)
        if (keep) queue[wave][qn + __popcll(km & ((1ull << lane) - 1ull))] = (uint32_t)row;
        const int nk = __popcll(km);
        qn += nk; nsurv += (uint32_t)nk;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (qn >= 16) {
            do { qn -= 16; drain(qn, 16); } while (qn >= 16);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();             // (the next append stays behind the drain's loads)
        }
    }
    if (!DBG) {
        // The sampled rows: their upper bounds are in the list the sample pass left, slot 16 w + r for row r of window w's tile.  A wave
        // loads 64 slots at a time (the next 64 in flight behind them) and appends the rows with !(hi < T_s) half by half -- at most 32 to
        // fewer than 16, as a step of the stream does -- and drains as the stream does.  hi is MODE 1's own (hq_rows4_bounds, same
        // bits), and hi5 >= hi had every such row queued when the tile was streamed: the drain emits what it emitted then.
        if (s_tiles != 0u) {
            const QuantArgs& am = hq_args_in_memory();
            const uint32_t nslots = s_tiles * 16u, dslot = (uint32_t)gridDim.x * 256u;
            uint32_t cbase = ((uint32_t)blockIdx.x * 4u + (uint32_t)wave) * 64u;             // (scalar)
            float hnext = cbase + lane < nslots ? am.pl_hi[cbase + lane] : 0.f;
#pragma unroll 1
            for (; cbase < nslots; cbase += dslot) {
                const uint32_t slot = cbase + lane;
                const float hi = hnext;
                hnext = slot + dslot < nslots ? am.pl_hi[slot + dslot] : 0.f;
                const int64_t row = hdb_tile_index((int64_t)(slot >> 4), (int64_t)s_stride) * 16 + (slot & 15u);
                bool keep = slot < nslots && !q_bad && !(hi < q_thr);
                if (keep && am.mask) keep = am.mask[row] != 0;                               // (a masked row is in no queue, as in the stream)
                const unsigned long long km = __ballot(keep);
#pragma unroll 1
                for (int h = 0; h < 2; ++h) {
                    const uint32_t kh = (uint32_t)(km >> (32 * h));
                    if (kh == 0u) continue;                                                  // (wave-uniform)
                    if (keep && (lane >> 5) == h) queue[wave][qn + __popc(kh & ((1u << (lane & 31)) - 1u))] = (uint32_t)row;
                    const int nk = __popc(kh);
                    qn += nk; nsurv += (uint32_t)nk;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    while (qn >= 16) { qn -= 16; drain(qn, 16); }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();                                         // (the next append stays behind the drain's loads)
                }
            }
        }
        if (qn > 0) drain(0, qn);
        if (lane == 0 && nsurv != 0u) atomicAdd(&surv_cnt, nsurv);                       // LDS
        hq_stage_flush<1>(stage);
        if (threadIdx.x == 0 && surv_cnt != 0u) {                                        // one atomic per workgroup (stat plane_survivors)
            const QuantArgs& a = hq_args_in_memory();
            const uint32_t before = atomicAdd(&a.pl_cnt[0], surv_cnt);
            // the count passes plane_cap_rows in exactly one workgroup's add (stat plane_overflows: the plane kept more than it is worth)
            if (before <= a.pl_cap && before + surv_cnt > a.pl_cap) atomicAdd(&a.pl_cnt[1], 1u);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// Exact rescoring of the candidates from the ORIGINAL matrix.  A 16-lane group takes one candidate and forms its lanes' partial
// sums exactly as hdb_scan_kernel (VEC: 16-byte pieces, lane l16 takes pieces l16 + 16 j, a dead piece adds (0 * q)) or
// hdb_scan_generic_kernel (elements l16 + 16 i) does, then runs hdb_rows4_sum with the candidate in all four row slots and keeps
// the lane that owns row slot (row & 3) -- the slot the row has in its dense tile -- so the same tree adds the same partials in the
// same order.  hdb_emit's epilogue follows; the packed key is rewritten.
// ------------------------------------------------------------------------------------------------------------------------
struct RescoreArgs {
    const void* V; int32_t d; int32_t row_bytes; int32_t nchunks;
    const float* Q;           // [nq][d] float32, as the caller passed them
    int32_t metric;
    const float* inv_norm; const float* qinv; const float* bias; const uint8_t* mask;
    unsigned long long* cand; const uint32_t* cnt; uint32_t cap;
};

template <typename T, int ACC, bool VEC>
__global__ __launch_bounds__(256) void hdb_quant_rescore_kernel(RescoreArgs a) {
    using Acc = float;
    constexpr int EPC = HqElem<T>::EPC;
    const int q = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, l16 = lane & 15;
    const uint32_t total = min(a.cnt[q * HDB_CNT_STRIDE], a.cap);
    const float* qv = a.Q + (int64_t)q * a.d;
    const char* Vb = reinterpret_cast<const char*>(a.V);
    const T* Vt = reinterpret_cast<const T*>(a.V);
    for (uint32_t base = ((uint32_t)blockIdx.x * 4 + wave) * 4; base < total; base += gridDim.x * 16) {     // (wave-uniform)
        const uint32_t i = base + g;
        const bool valid = i < total;
        const unsigned long long ent = valid ? a.cand[(int64_t)q * a.cap + i] : 0ull;
        const uint32_t row = valid ? 0xFFFFFFFFu - (uint32_t)(ent & 0xFFFFFFFFull) : 0u;
        Acc acc = Acc(0);
        if constexpr (VEC) {
            const char* pr = Vb + (int64_t)row * a.row_bytes;
            const int nj = (a.nchunks + 15) >> 4;
            for (int j = 0; j < nj; ++j) {
                const int c = l16 + 16 * j;
                const bool live = c < a.nchunks;
                const int cc = live ? c : a.nchunks - 1;
                const uint4 raw = *reinterpret_cast<const uint4*>(pr + (int64_t)cc * 16);
                Acc x[EPC];
                hq_unpack(raw, x, (T*)nullptr);
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    const Acc qe = qv[cc * EPC + e];
                    if (ACC == 1) {
                        const Acc df = live ? x[e] - qe : Acc(0);
                        acc += df * df;
                    } else {
                        acc += (live ? x[e] : Acc(0)) * qe;
                    }
                }
            }
        } else {
            for (int e = l16; e < a.d; e += 16) {
                const Acc qe = qv[e];
                const Acc x = (Acc)hq_f(Vt[(int64_t)row * a.d + e]);
                if (ACC == 1) { const Acc df = x - qe; acc += df * df; }
                else acc += x * qe;
            }
        }
        const Acc sum = hdb_rows4_sum(acc, acc, acc, acc, l16);
        if (valid && (l16 & 3) == 0 && hdb_owned_row(l16) == (int)(row & 3u)) {
            float s;                                      // hdb_emit, MODE 1
            if (a.metric == HDB_EUCLIDEAN) {
                s = (float)(Acc(1) / (Acc(1) + sqrt(sum)));
            } else if (a.metric == HDB_COSINE) {
                s = (float)sum * a.inv_norm[row] * a.qinv[q];
            } else {
                s = (float)sum;
            }
            if (a.bias) s += a.bias[row];
            const bool masked = a.mask && !a.mask[row];
            if (masked) s = -INFINITY;
            s = hdb_canon(s);
            a.cand[(int64_t)q * a.cap + i] = hdb_pack(s, row);
        }
    }
}

// Finalize: hdb_finalize_fast over the rescored list with the floor T_s (see "Completeness" above).  A query with an infinite
// element, or one the quantized prep could not take, is reported as HDB_Q_UNDERFLOW: hdb_topk_host re-runs it exactly.
__global__ __launch_bounds__(1024) void hdb_quant_finalize_kernel(const unsigned long long* cand, const uint32_t* cnt, uint32_t cap, uint32_t k,
                                                                  uint32_t kk, int64_t row_base, int64_t* idx_out, float* score_out,
                                                                  int32_t* status, const int* qnan, const float* qaux, const float* thr,
                                                                  int* stat, unsigned long long* cand_rw, const float* sc, int64_t ld) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long buf[];
    const int q = blockIdx.x;
    const uint32_t total = cnt[q * HDB_CNT_STRIDE];
    if (sc) {          // matrix-core flavour, second half: the MODE 0 launch left the score of list entry i at sc[q][q cap + i]
        const uint32_t nc = min(total, cap);
        for (uint32_t i = threadIdx.x; i < nc; i += blockDim.x) {
            const int64_t slot = (int64_t)q * cap + i;
            const uint32_t row = 0xFFFFFFFFu - (uint32_t)(cand_rw[slot] & 0xFFFFFFFFull);
            cand_rw[slot] = hdb_pack(sc[(int64_t)q * ld + slot], row);
        }
        __threadfence_block();
        __syncthreads();
    }
    if (threadIdx.x == 0 && stat) atomicMax(stat, (int)min(total, 0x7FFFFFFFu));
    const int qn = qnan[q];
    const bool bad = qaux[(int64_t)q * HDB_QQ_WORDS + HDB_QQ_BAD] != 0.f;
    hdb_finalize_fast(buf, cand + (int64_t)q * cap, total, q, cap, k, kk, row_base, idx_out, score_out, status,
                      qn & 1, ((qn & 2) || bad) ? (int32_t)HDB_Q_UNDERFLOW : 0, thr + q, 1.f);
}

// ------------------------------------------------------------------------------------------------------------------------
// host-side launchers
// ------------------------------------------------------------------------------------------------------------------------
extern "C" int hdb_launch_quant_rows(const void* V, int64_t n, int d, int dtype, int P, int8_t* codes, float* aux, int* nan_flag,
                                     double gamma, void* stream) {
    if (n <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = hdb_grid_for(n, 4, 8192);
    // (every element type has an instantiation of its own: a type that is not built is an error, never another type's kernel)
    if (dtype == HDB_F16) hipLaunchKernelGGL(hdb_quant_rows_kernel<__half>, dim3(blocks), dim3(256), 0, st, (const __half*)V, n, d, P, codes, aux, nan_flag, gamma);
    else if (dtype == HDB_BF16) hipLaunchKernelGGL(hdb_quant_rows_kernel<hdb_bf16>, dim3(blocks), dim3(256), 0, st, (const hdb_bf16*)V, n, d, P, codes, aux, nan_flag, gamma);
    else if (dtype == HDB_F32) hipLaunchKernelGGL(hdb_quant_rows_kernel<float>, dim3(blocks), dim3(256), 0, st, (const float*)V, n, d, P, codes, aux, nan_flag, gamma);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

extern "C" int hdb_launch_quant_gather(const int8_t* codes, const float* aux, const int64_t* rows, int64_t m, int P, int8_t* codes_out,
                                       float* aux_out, void* stream) {
    if (m <= 0) return 0;
    hipLaunchKernelGGL(hdb_quant_gather_kernel, dim3(hdb_grid_for(m, 4, 8192)), dim3(256), 0, (hipStream_t)stream, codes, aux, rows, m, P,
                       codes_out, aux_out);
    return (int)hipGetLastError();
}

extern "C" int hdb_launch_quant_qprep(const float* Q, int nq, int d, int P, int8_t* qcodes, float* qaux, int* stat, uint32_t* pl_cnt,
                                      void* stream) {
    hipLaunchKernelGGL(hdb_quant_qprep_kernel, dim3(nq), dim3(64), 0, (hipStream_t)stream, Q, nq, d, P, qcodes, qaux, stat, pl_cnt);
    return (int)hipGetLastError();
}

extern "C" int hdb_launch_quant_qprep_m(const float* Q, int nq, int d, int P, float* qinv, float* qsq, int* qnan, void* q16, float* qscl,
                                        int8_t* qcodes, float* qaux, int* stat, uint32_t* cnt_init, uint32_t* pl_cnt, void* stream) {
    hipLaunchKernelGGL(hdb_quant_qprep_m_kernel, dim3(nq), dim3(64), 0, (hipStream_t)stream, Q, nq, d, P, qinv, qsq, qnan, (_Float16*)q16,
                       qscl, qcodes, qaux, stat, cnt_init, pl_cnt);
    return (int)hipGetLastError();
}

template <int MODE, int NQ>
static void hq_launch_scan_nq(const QuantArgs& a, int blocks, size_t lds, hipStream_t st) {
    const int nch = a.P >> 4;
    const int nj = (nch + 15) >> 4;
    if (nj == 1) hipLaunchKernelGGL((hdb_quant_scan_kernel<MODE, NQ, 1>), dim3(blocks), dim3(256), lds, st, a);
    else if (nj == 2) hipLaunchKernelGGL((hdb_quant_scan_kernel<MODE, NQ, 2>), dim3(blocks), dim3(256), lds, st, a);
    else if (nj == 3) hipLaunchKernelGGL((hdb_quant_scan_kernel<MODE, NQ, 3>), dim3(blocks), dim3(256), lds, st, a);
    else hipLaunchKernelGGL((hdb_quant_scan_kernel<MODE, NQ, 0>), dim3(blocks), dim3(256), lds, st, a);
}
template <int MODE>
static void hq_launch_scan_mode(const QuantArgs& a, int blocks, size_t lds, hipStream_t st) {
    switch (a.nq) {
    case 1: hq_launch_scan_nq<MODE, 1>(a, blocks, lds, st); break;
    case 2: hq_launch_scan_nq<MODE, 2>(a, blocks, lds, st); break;
    case 3: hq_launch_scan_nq<MODE, 3>(a, blocks, lds, st); break;
    default: hq_launch_scan_nq<MODE, 4>(a, blocks, lds, st); break;
    }
}
// the row copies of the matrix-core flavour move 16-byte pieces
static bool hq_copy_args_ok(const QuantArgs& a) {
    return !a.G || (a.V && a.row_bytes > 0 && a.row_bytes % 16 == 0 && (reinterpret_cast<uintptr_t>(a.V) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.G) & 15) == 0);
}
// mode 0: lower bounds of the sampled tiles; mode 1: candidate emission over a.ntiles dense tiles.  1 <= a.nq <= 4.
extern "C" int hdb_launch_quant_scan(const QuantArgs* args, int mode, int max_blocks, void* stream) {
    const QuantArgs& a = *args;
    if (a.nq < 1 || a.nq > 4 || (a.P & 15) != 0) return (int)hipErrorInvalidValue;
    const size_t lds = (size_t)a.nq * a.P;
    const int blocks = hdb_quant_scan_blocks(a.ntiles, max_blocks);
    if (a.nsub != 0 && (a.nsub > HDB_QUANT_NSUB_MAX || !a.wmax || (mode == 0 ? a.nsub != 4 * blocks : !a.thr_out))) return (int)hipErrorInvalidValue;
    if (mode == 0) hq_launch_scan_mode<0>(a, blocks, lds, (hipStream_t)stream);
    else {
        if (!hq_copy_args_ok(a)) return (int)hipErrorInvalidValue;
        hq_launch_scan_mode<1>(a, blocks, lds, (hipStream_t)stream);
    }
    return (int)hipGetLastError();
}

// The 5-bit plane: derivation and pass 1 (one query; dot / cosine).
// the tiles [t0, t1) of the plane, whole, from the codes, caches and 1/||v|| of their rows below n
extern "C" int hdb_launch_quant_plane_rows(const int8_t* codes, const float* aux, const float* inv_norm, int64_t t0, int64_t t1, int64_t n, int d,
                                           int P, uint8_t* nib, uint32_t* bitw, float* rec, void* stream) {
    if (t1 <= t0) return 0;
    const int U = hdb_quant_plane_units(P);
    if (U > 16 || (P & 15) != 0 || t0 < 0 || (t1 - 1) * 16 >= n) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(hdb_quant_plane_rows_kernel, dim3(hdb_grid_for(t1 - t0, 4, 8192)), dim3(256), 0, (hipStream_t)stream, codes, aux, inv_norm,
                       t0, t1, n, d, P, U, nib, bitw, rec);
    return (int)hipGetLastError();
}
// dbg = false: pass 1 (candidates of the rows the plane keeps; the threshold as MODE 1 takes it, folded or a.thr); dbg = true: hi5 of every row -> a.dbg (tests)
// blocks: the grid, from the plan (hdb_quant_plane_blocks; dbg: hdb_quant_plane_dbg_blocks).  Any count gives the same candidates --
// only gridDim.x enters the kernel, as the walk's step and the list phase's stride.
extern "C" int hdb_launch_quant_plane_scan(const QuantArgs* args, int dbg, int blocks, void* stream) {
    const QuantArgs& a = *args;
    const int U = a.pl_units;
    if (blocks < 1 || blocks > (1 << 22)) return (int)hipErrorInvalidValue;           // (blocks x 256 list slots per round fit 32 bits)
    if (a.nq != 1 || U < 1 || U > 16 || U != hdb_quant_plane_units(a.P) || (a.metric != HDB_DOT && a.metric != HDB_COSINE)) return (int)hipErrorInvalidValue;
    if (!dbg && a.nsub != 0 && (a.nsub > HDB_QUANT_NSUB_MAX || !a.wmax || !a.thr_out)) return (int)hipErrorInvalidValue;
    if (!dbg && (!a.cnt || !a.cand || !a.pl_cnt || !hq_copy_args_ok(a))) return (int)hipErrorInvalidValue;
    // the tiles the sample pass took are not walked (dbg: every tile is): its windows lie inside the matrix and its list is there
    if (a.ntiles < 0 || a.ntiles > 0x10000000) return (int)hipErrorInvalidValue;      // (a row number has 32 bits: hdb_pack)
    if (!dbg && a.pl_s_tiles != 0u && (!a.pl_hi || a.pl_s_stride < 1u || (uint64_t)a.pl_s_tiles * a.pl_s_stride > (uint64_t)a.ntiles)) return (int)hipErrorInvalidValue;
    const size_t lds = (size_t)U * 32;
    hipStream_t st = (hipStream_t)stream;
    const int J = hdb_quant_plane_j(U);
#define HQ_PLANE(J_) do { if (dbg) hipLaunchKernelGGL((hdb_quant_plane_scan_kernel<J_, true>), dim3(blocks), dim3(256), lds, st, a); \
                          else hipLaunchKernelGGL((hdb_quant_plane_scan_kernel<J_, false>), dim3(blocks), dim3(256), lds, st, a); } while (0)
    if (J == 1) HQ_PLANE(1); else if (J == 2) HQ_PLANE(2); else if (J == 3) HQ_PLANE(3); else HQ_PLANE(4);
#undef HQ_PLANE
    return (int)hipGetLastError();
}
// MODE 1's upper bound of every row of a.ntiles dense tiles for one query -> a.dbg (tests)
extern "C" int hdb_launch_quant_scan_one(const QuantArgs* args, int mode, int max_blocks, void* stream) {
    const QuantArgs& a = *args;
    if (a.nq != 1 || (a.P & 15) != 0 || a.nsub != 0 || mode != 2 || !a.dbg) return (int)hipErrorInvalidValue;
    const size_t lds = (size_t)a.P;
    const int blocks = hdb_quant_scan_blocks(a.ntiles, max_blocks);
    const int nj = ((a.P >> 4) + 15) >> 4;
    hipStream_t st = (hipStream_t)stream;
#define HQ_ONE(NJ_) hipLaunchKernelGGL((hdb_quant_scan_kernel<2, 1, NJ_>), dim3(blocks), dim3(256), lds, st, a)
    if (nj == 1) HQ_ONE(1); else if (nj == 2) HQ_ONE(2); else if (nj == 3) HQ_ONE(3); else HQ_ONE(0);
#undef HQ_ONE
    return (int)hipGetLastError();
}

extern "C" int hdb_launch_quant_rescore(const void* V, int d, int dtype, const float* Q, int nq, int metric, const float* inv_norm,
                                        const float* qinv, const float* bias, const uint8_t* mask, unsigned long long* cand,
                                        const uint32_t* cnt, uint32_t cap, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    RescoreArgs a;
    a.V = V; a.d = d; a.Q = Q; a.metric = metric; a.inv_norm = inv_norm; a.qinv = qinv; a.bias = bias; a.mask = mask;
    a.cand = cand; a.cnt = cnt; a.cap = cap;
    if (dtype != HDB_F16 && dtype != HDB_F32 && dtype != HDB_BF16) return (int)hipErrorInvalidValue;      // (the dtypes that have a shadow)
    a.row_bytes = (int32_t)hdb_row_bytes(dtype, d);
    a.nchunks = a.row_bytes / 16;
    // the same choice as hdb_launch_scan: 16-byte pieces when rows are whole pieces of an aligned matrix
    const bool vec = (a.row_bytes % 16 == 0) && ((reinterpret_cast<uintptr_t>(V) & 15) == 0) && ((size_t)d * 4 <= 60 * 1024);
    const bool euc = metric == HDB_EUCLIDEAN;
    const dim3 grid((cap + 15) / 16 < 128 ? (cap + 15) / 16 : 128, nq);
#define HQ_RESCORE(T_, ACC_, VEC_) hipLaunchKernelGGL((hdb_quant_rescore_kernel<T_, ACC_, VEC_>), grid, dim3(256), 0, st, a)
    if (dtype == HDB_F16) {
        if (vec) { if (euc) HQ_RESCORE(__half, 1, true); else HQ_RESCORE(__half, 0, true); }
        else { if (euc) HQ_RESCORE(__half, 1, false); else HQ_RESCORE(__half, 0, false); }
    } else if (dtype == HDB_BF16) {
        if (vec) { if (euc) HQ_RESCORE(hdb_bf16, 1, true); else HQ_RESCORE(hdb_bf16, 0, true); }
        else { if (euc) HQ_RESCORE(hdb_bf16, 1, false); else HQ_RESCORE(hdb_bf16, 0, false); }
    } else if (dtype == HDB_F32) {
        if (vec) { if (euc) HQ_RESCORE(float, 1, true); else HQ_RESCORE(float, 0, true); }
        else { if (euc) HQ_RESCORE(float, 1, false); else HQ_RESCORE(float, 0, false); }
    } else {
        return (int)hipErrorInvalidValue;
    }
#undef HQ_RESCORE
    return (int)hipGetLastError();
}

extern "C" int hdb_launch_quant_finalize(const unsigned long long* cand, const uint32_t* cnt, uint32_t cap, int nq, uint32_t k, uint32_t kk,
                                         int64_t row_base, int64_t* idx_out, float* score_out, int32_t* status, const int* qnan,
                                         const float* qaux, const float* thr, int* stat, unsigned long long* cand_rw, const float* sc,
                                         int64_t ld, void* stream) {
    const size_t lds = (size_t)cap * 16 + 2048 * 4 + 64;
    static unsigned long long attr_done = 0;
    hipError_t e = hdb_lds_attr_once(reinterpret_cast<const void*>(hdb_quant_finalize_kernel), (int)lds, &attr_done);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(hdb_quant_finalize_kernel, dim3(nq), dim3(1024), lds, (hipStream_t)stream, cand, cnt, cap, k, kk, row_base,
                       idx_out, score_out, status, qnan, qaux, thr, stat, cand_rw, sc, ld);
    return (int)hipGetLastError();
}
