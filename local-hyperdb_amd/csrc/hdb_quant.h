// hdb_quant.h -- arguments of the int8 shadow kernels (hdb_quant.hip), shared with hdb_api.hip.
#pragma once
#include <stdint.h>

// Per-row cache of the shadow: three floats per row, [row][3].
#define HDB_QROW_S 0      // s_r = max_j |v_rj| / 127
#define HDB_QROW_E 1      // ||eps_r||_2 + gamma_d ||v_r||_2, rounded up
#define HDB_QROW_T 2      // s_r ||c_r||_2, rounded up
// Per-query record written by the quantized query prep: eight floats per query.
#define HDB_QQ_S 0        // s_q
#define HDB_QQ_N 1        // ||q||_2, rounded up
#define HDB_QQ_D 2        // ||delta_q||_2, rounded up
#define HDB_QQ_SQ 3       // ||q||^2 (float64 sum rounded to nearest)
#define HDB_QQ_BAD 4      // non-zero: the query is not finite (the call leaves it to the exact re-run)
#define HDB_QQ_CN 5       // ||c_q||_2, rounded up (the 5-bit plane's residual bound)
#define HDB_QQ_CS 6       // sum_j c_qj (an integer, exact in float32)
#define HDB_QQ_WORDS 8

struct QuantArgs {
    const int8_t* codes;      // [n][P] int8 codes of the rows, zero-padded
    int64_t n;
    int32_t d;
    int32_t P;                // code pitch in bytes: d rounded up to 16
    const float* aux;         // [n][3] per-row cache
    const float* sqnorm;      // [n] ||v||^2 of the float32 row cache (euclidean)
    const float* inv_norm;    // [n] 1/||v|| (cosine)
    const int8_t* qcodes;     // [nq][P]
    const float* qaux;        // [nq][HDB_QQ_WORDS]
    const float* qinv;        // [nq] 1/||q|| as the VALU scan's query prep computes it
    const float* bias;        // [n] or nullptr
    const uint8_t* mask;      // [n] or nullptr
    int32_t metric;
    int32_t nq;
    float gamma;              // rounding-error factor of the float32 VALU scan, gamma_{d+8}
    int64_t ntiles;           // 16-row tiles to visit
    int64_t tile_stride;      // 1 = dense; > 1 = strided sample (hdb_tile_index)
    float* scores; int64_t ld;                            // MODE 0: lower bounds of the sampled rows
    const float* thr; uint32_t* cnt; unsigned long long* cand; uint32_t cap;   // MODE 1: candidate lists
    // Threshold folded into the two passes (nsub > 0; matrix-core flavour): MODE 0 leaves, instead of the scores, the largest lower
    // bound every WAVE of its grid saw -- wmax[q][nsub], nsub = 4 x workgroups, as orderable keys (0: nothing seen) -- and every
    // workgroup of the filter pass starts by taking the 16th largest of those (a lower bound of the 16th largest sampled lower bound,
    // equal to it unless two of the top 16 fell to one wave: hdb_sample_thr_kernel's argument with 4x the subsets) and workgroup 0
    // stores it to thr_out for the finalize.  No launch in between, nothing to wait for.  (Selecting once, by the workgroup of the
    // sample pass that arrives last on a ticket, was measured and made the call longer: DESIGN.md.)
    uint32_t* wmax; int32_t nsub; float* thr_out;
    // Matrix-core flavour (G non-null): the workgroup that stores a candidate to cand[slot] also copies its row of the matrix V
    // (row_bytes each, a multiple of 16) to row `slot` of the compact matrix G and leaves 1/||v|| and the bias (row mask folded in, as
    // hdb_maskbias_kernel does) in ginv[slot] / gbias[slot] (either may be null) for the MODE 0 launch of hdb_mfma_kernel.h.
    const char* V; int32_t row_bytes; char* G; float* ginv; float* gbias;
    // The 5-bit plane (hdb_quant.hip, "The 5-bit plane"): pass 1 (hdb_quant_plane_scan_kernel) streams the plane, and the rows whose
    // coarse upper bound reaches T_s go through MODE 1's evaluation in the same kernel, 16 at a time, into the candidate lists.
    // pl_cnt[0] counts those rows; a call that kept more than pl_cap of them adds one to pl_cnt[1] (the plane let more through than it
    // is worth; the answer is complete either way).  dbg: test-only output of one upper bound per row (hdb_debug_quant_bounds).
    const uint8_t* pl_nib; const uint32_t* pl_bit; const float* pl_rec; int32_t pl_units;
    uint32_t* pl_cnt; uint32_t pl_cap;
    // The sampled tiles are evaluated once: the sample pass of a one-query call that takes the plane (MODE 0, pl_hi non-null) stores
    // MODE 1's upper bound of every sampled row to pl_hi[sample slot] (-inf: masked row, declined query), and pass 1 walks the
    // tiles the sample did not take (pl_s_tiles windows of pl_s_stride tiles, hdb_plane_skip_tile; 0 windows: every tile) and
    // queues the sampled rows with !(pl_hi < T_s) for the evaluation it gives the rows its own bound keeps.
    float* pl_hi; uint32_t pl_s_tiles; uint32_t pl_s_stride;
    float* dbg;
};
#define HDB_QUANT_NSUB_MAX 4096      // (MODE 1 holds nsub / 256 keys per thread)
