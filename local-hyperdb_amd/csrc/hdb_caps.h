// hdb_caps.h -- what each kernel unit can take and the grids its launcher uses, as plain inline functions of plain numbers.
//
// Two readers: the launchers (each calls the rule of its own unit from here) and the planner of hdb_topk (hdb_plan.h), which
// must reach the same answers without a launch.  Nothing here touches HIP: the grid rules take the CU count as an argument, so a
// host program without a GPU can call every function (tests/test_topk_plan.py).  The constants a rule reads live beside it.
// Included at the end of hdb_common.h (hdb_elem_bytes, hdb_grid_for).
#pragma once
#include "../../include/hyperdb_hip.h"

// ---- hdb_scan.hip: the VALU row scan ----
// Workgroups of a scan launch when the caller sets no limit.  A wave keeps one 16-row tile in flight, so the bytes in flight per CU
// are workgroups per CU x 4 x 16 x row bytes: 2 workgroups per CU (512) with the 12-KiB tiles of 768-byte rows, 1 (256) with the
// unrolled 1536-byte-row kernel -- ~100 KiB either way, the measured optimum of the fp16 / float32 scans.  The float8 kernels of
// 256- / 384- / 512-byte rows have 4- / 6- / 8-KiB tiles: their grid grows by 768 / row bytes, up to the 4 workgroups per CU that
// the registers of the ONE-query kernels allow (88-124 per lane: 4 waves per SIMD) -- 1024 / 1024 / 768 workgroups, 64 / 96 / 96 KiB
// in flight per CU.  The four-query kernel takes the same grid; its dot flavour (116-118 registers) is resident four times per CU as
// well, its euclidean / manhattan flavours (154-162: 3 waves per SIMD) three times -- the fourth workgroup of a CU waits its turn.
// int8 rows (HDB_I8) are the same bytes and take the same kernels' unrolled flavours, so the same grid.
static inline int hdb_scan_auto_blocks(int dtype, int row_bytes, bool vec, bool wide_rows) {
    if ((dtype == HDB_F8E4M3 || dtype == HDB_I8) && vec && (row_bytes == 256 || row_bytes == 384 || row_bytes == 512)) {
        const int b = 512 * 768 / row_bytes;
        return b < 1024 ? b : 1024;
    }
    return wide_rows ? 256 : 512;
}

// ---- hdb_bscan.hip: float32 queries against packed-bit rows (HDB_B1) ----
// One thread per row.  A query lives in LDS as a NIBBLE TABLE, T[d / 4][16] floats = 16 d bytes: entry [j][m] is the sum of the four
// per-element terms of elements 4 j .. 4 j + 3 for the bit pattern m, so a row costs d / 4 reads.  QT queries per pass have all
// their tables resident; the rule below takes the largest QT of 4 / 2 / 1 whose tables fit HDB_BSCAN_TABLE_BYTES, the 60 KiB every
// scan kernel allows its queries -- with the 4-KiB survivor stage beside them two workgroups fit the 160 KiB of a CU:
//   d <= 960: 4 queries per pass, d <= 1920: 2, d <= 3840: 1.
// Wider rows (up to the 7680 hdb_index_create admits) keep the two terms of every element in LDS instead, 8 d bytes <= 60 KiB, one
// query per pass, and select per bit in registers (QT = 0 here: the fallback; it forms the same nibble sums in the same order).
#define HDB_BSCAN_TABLE_BYTES (60 * 1024)
static inline int hdb_bscan_qt(int d) {
    if (d <= 0 || d % 32 != 0) return -1;                                 // no such row
    for (int qt = 4; qt >= 1; qt >>= 1)
        if ((int64_t)qt * 16 * d <= HDB_BSCAN_TABLE_BYTES) return qt;
    return (int64_t)8 * d <= HDB_BSCAN_TABLE_BYTES ? 0 : -1;
}
// dynamic LDS of a launch: the tables of the queries of one pass, or the fallback's pairs of terms
static inline int hdb_bscan_lds_bytes(int d, int qt) { return qt > 0 ? qt * 16 * d : 8 * d; }
// workgroups (256 threads, one row each) of a launch when the caller sets no limit: as many per CU as the LDS holds beside the
// 4-KiB stage, eight at most (the waves a SIMD takes)
static inline int hdb_bscan_auto_blocks(int d, int qt, int cus) {
    int per_cu = (160 * 1024) / (hdb_bscan_lds_bytes(d, qt) + 5 * 1024);
    per_cu = per_cu < 1 ? 1 : per_cu > 8 ? 8 : per_cu;
    return per_cu * (cus > 0 ? cus : 1);
}

// ---- hdb_mfma_ksplit.hip: K slices of rows too wide for one wave's query fragments ----
// The slice list of a width: slice s covers `width[s]` elements of every row from byte `off[s]` of the stored row on; the widths
// add up to d and every one of them is a slice geometry that is instantiated for the dtype (float32 512 / 768, fp16 1024 / 1536,
// bfloat16 256 / 384 / 512).
#define HDB_KS_MAX_SLICES 8
struct KsGeom {
    int slices;                           // 0: the width has no K slices
    int width[HDB_KS_MAX_SLICES];
    int off[HDB_KS_MAX_SLICES];
};
// n0 slices of w0 elements, then n1 of w1
static inline KsGeom ks_list(int elem_bytes, int n0, int w0, int n1 = 0, int w1 = 0) {
    KsGeom g = {};
    int at = 0;
    for (int s = 0; s < n0 + n1 && s < HDB_KS_MAX_SLICES; ++s) {
        g.width[s] = s < n0 ? w0 : w1; g.off[s] = at * elem_bytes;
        at += g.width[s];
    }
    g.slices = n0 + n1;
    return g;
}
// bfloat16 (hdb_mfma_bf16_ks.hip): the query fragments of 16 queries take 3/8 of a register per element (three bf16 parts), so a
// slice is 512 elements at most -- every multiple of 128 from 640 to 1536 as the fewest slices of 512 / 384 / 256, the widest first,
// and 2048 / 3072 / 4096 as slices of 512
static inline KsGeom ks_geom_bf16(int d) {
    switch (d) {
        case 640: return ks_list(2, 1, 384, 1, 256);
        case 768: return ks_list(2, 2, 384);
        case 896: return ks_list(2, 1, 512, 1, 384);
        case 1024: return ks_list(2, 2, 512);
        case 1152: return ks_list(2, 3, 384);
        case 1280: return ks_list(2, 1, 512, 2, 384);
        case 1408: return ks_list(2, 2, 512, 1, 384);
        case 1536: return ks_list(2, 3, 512);
        case 2048: return ks_list(2, 4, 512);
        case 3072: return ks_list(2, 6, 512);
        case 4096: return ks_list(2, 8, 512);
        default: return ks_list(2, 0, 0);
    }
}
// ... and the number of queries of a call from which the bfloat16 slices are used (the planner's bf16_ks_min_q = -1).  Up to 8 queries
// are two VALU passes at HBM speed; the slices read the matrix once, but in 16-row stages of 8-16 KiB (two tiles in flight per CU)
// and with one launch per slice and pass.  Measured, one box, the two paths alternating call by call, cosine top-100, p50 in us, slices vs
// VALU scan at 5 / 8 / 16 queries on ~1.5 GB of rows (profiles/bf16_wide_time.txt):
//   640: 591 vs 515, 621 vs 534, 653 vs 1035     768: 547 vs 510, 576 vs 524, 593 vs 1017     896: 521 vs 517, 539 vs 516, 566 vs 1008
//  1024: 621 vs 669, 641 vs 668, 678 vs 1318    1152: 613 vs 510, 630 vs 510, 654 vs 1000    1280: 595 vs 517, 615 vs 522, 647 vs 1015
//  1408: 574 vs 523, 594 vs 530, 616 vs 1029    1536: 556 vs 522, 578 vs 531, 595 vs 1026    2048: 632 vs 593, 654 vs 586, 676 vs 1093
//  3072: 654 vs 652, 684 vs 653, 700 vs 1067    4096: 746 vs 1386, 785 vs 2144, 790 vs 4196
// The slices win from 5 queries at d = 1024 and 4096 and lose by 1-19 % at 5 and 8 queries everywhere else; at 16 they win 1.5-5.3x
// at every width.  9-15 queries were not measured: a third VALU pass is 1.5 x the two-pass figure (>= 765 us), above every slice time
// at 8 and 16 queries, so the other widths start at 9.
static inline int hdb_mfma_bf16_ks_min_q(int d) { return (d == 1024 || d == 4096) ? 5 : 9; }
static inline KsGeom ks_geom(int dtype, int d) {
    if (dtype == HDB_F32 && d == 1024) return ks_list(4, 2, 512);
    if (dtype == HDB_F32 && d == 1536) return ks_list(4, 2, 768);
    if (dtype == HDB_F16 && d == 2048) return ks_list(2, 2, 1024);
    if (dtype == HDB_F16 && d == 3072) return ks_list(2, 2, 1536);
    if (dtype == HDB_F16 && d == 4096) return ks_list(2, 4, 1024);
    if (dtype == HDB_BF16) return ks_geom_bf16(d);
    return ks_list(1, 0, 0);
}
static inline int hdb_mfma_ksplit_slices(int dtype, int d) { return ks_geom(dtype, d).slices; }
// float8 e4m3 (hdb_mfma_f8_ks.hip): OPT-IN slices (the planner's f8_ks_min_q, 0 = never by default), so they are no part of
// ks_geom / hdb_mfma_ksplit_slices / hdb_mfma_tile_rows / hdb_mfma_supported, which describe the default dispatch.  The query
// fragments are bfloat16's (three bf16 parts, 3/8 of a register per element), so the widths and the slices of a width are
// ks_geom_bf16's; an element is one byte, so off[s] is the byte offset into the stored row and the element offset into the query.
static inline KsGeom ks_geom_f8(int d) {
    const KsGeom b = ks_geom_bf16(d);
    KsGeom g = {};
    g.slices = b.slices;
    for (int s = 0; s < b.slices && s < HDB_KS_MAX_SLICES; ++s) { g.width[s] = b.width[s]; g.off[s] = b.off[s] / 2; }
    return g;
}
static inline int hdb_mfma_f8_ks_slices(int d) { return ks_geom_f8(d).slices; }
// ... and the number of queries of a call from which the float8 slices are used when f8_ks_min_q = -1.  Measured, one box, the
// contenders alternating call by call, cosine top-100, p50 in us, slices vs VALU scan at 5 / 8 / 16 queries on ~1.5 GB of rows, the
// two p50s of the repeated slice contender at most 1.9 % apart (tools/time_f8_wide.py -> profiles/f8_wide_time.txt):
//   768: 483 vs 1149, 501 vs 1187, 526 vs 2251    1024: 513 vs 1160, 517 vs 1181, 535 vs 2242
//  1536: 553 vs 1177, 560 vs 1186, 580 vs 2238    4096: 732 vs 1239, 750 vs 1956, 771 vs 3815
// The slices win 1.7-2.4x at 5 queries at every measured width (two VALU passes of one-byte rows run at ~2.7 TB/s, far from HBM
// speed), so the rule is 5, the first batch size the matrix cores are offered; the widths between were not measured.
static inline int hdb_mfma_f8_ks_min_q(int d) { (void)d; return 5; }

// ---- hdb_mfma_bf16.hip ----
// rows per LDS stage (hdb_mfma_tile_rows): the query fragments of 16 queries take 3 d / 8 registers, so the wider the row the fewer
// row tiles a wave keeps in flight beside them -- 64 rows up to d = 256, 32 at d = 384, 16 at d = 512
static inline int hdb_mfma_bf16_tile_rows(int d) { return (d == 128 || d == 256) ? 64 : d == 384 ? 32 : d == 512 ? 16 : 0; }

// ---- hdb_mfma_f8.hip ----
// float8 e4m3 rows (hdb_mfma_f8.h): d = 128, 256, 384 and 512, the bfloat16 flavour's widths (three bf16 query parts: 3 d / 8
// registers per 16 queries).  A wave takes one 16-row tile at a time and reads its fragments from global memory, so the tile height
// is the VALU scan's 16 rows at every width
static inline int hdb_mfma_f8_tile_rows(int d) { return (d == 128 || d == 256 || d == 384 || d == 512) ? 16 : 0; }
// workgroups of a launch of the register kernels (float8, int8, packed bits: no LDS ring, 256 threads) over `ntiles` 16-row tiles:
// max_blocks when the caller set one, else four workgroups per CU; never more than there are tiles, never fewer than one
static inline int hdb_mfma_reg_blocks(int64_t ntiles, int cus, int max_blocks) {
    const int64_t want = max_blocks > 0 ? max_blocks : 4 * (int64_t)cus;
    return (int)(ntiles < want ? (ntiles < 1 ? 1 : ntiles) : want);
}

// ---- hdb_mfma_f8_lds*.hip: float8 rows expanded to bf16 in LDS once per workgroup (hdb_mfma_f8_lds.h; opt-in, f8_lds_min_q) ----
// Whole rows of 128 / 256 / 384 / 512 elements and the K slices of 256 / 384 / 512.  A workgroup of `waves` waves (4 or 8, 16
// queries each) takes a STAGE of rows at a time: every thread loads hdb_mfma_f8_lds_chunks(d) 16-byte pieces of it, so a stage is
// chunks x 64 x waves x 16 bytes of float8 -- 8 / 8 / 12 / 16 KiB with four waves, twice that with eight -- and twice as many
// bytes of bf16 in LDS, in two buffers:
//   d        128    256    384    512
//   rows      64     32     32     32     (four waves; eight: 128 / 64 / 64 / --)
//   LDS    32 KiB 32 KiB 48 KiB 64 KiB    (four waves; eight: 64 / 64 / 96 KiB / --, dynamic LDS beyond 64 KiB)
// Four waves leave room for two workgroups per CU (128 KiB at most, 256 registers per lane), eight for one.  d = 512 is built for four
// waves and one workgroup per CU only: 192 registers of query parts, the stage's pieces and the A fragments in flight do not fit the
// 256 registers that two waves per SIMD leave a lane (the build spilled 44-124 bytes), so those kernels take what they need.
static constexpr int hdb_mfma_f8_lds_supported(int d) { return d == 128 || d == 256 || d == 384 || d == 512; }
// waves per workgroup: ScanArgs::f8_lds carries 4 or 8.  Measured at 10M x 384, cosine top-100, p50 in us, LDS flavour with four waves
// (profiles/f8_lds_time.txt) vs eight (profiles/f8_lds_time_w8.txt; runs of their own, the repeated contender 4-12 % apart at this
// shape): 64 queries 1 855 vs 2 310, 128 queries 3 566 vs 2 800, 256 queries 6 994 vs 5 453 -- four waves (two workgroups per CU: one
// converts while the other multiplies) win while one workgroup holds the launch's queries, eight win 1.27x once four would read the
// matrix twice.  So a launch of up to 64 queries takes four waves and a larger one eight (the option f8_lds_waves = 4 | 8 fixes it).
#define HDB_F8_LDS_WAVES 4
static constexpr int hdb_mfma_f8_lds_waves(int waves, int d = 0) { return d == 512 ? 4 : waves == 8 ? 8 : waves == 4 ? 4 : HDB_F8_LDS_WAVES; }
static constexpr int hdb_mfma_f8_lds_auto_waves(int nq_launch) { return nq_launch > 64 ? 8 : 4; }
static constexpr int hdb_mfma_f8_lds_chunks(int d) { return d == 128 || d == 256 ? 2 : d == 384 ? 3 : d == 512 ? 4 : 0; }
static constexpr int hdb_mfma_f8_lds_stage_rows(int d, int waves = HDB_F8_LDS_WAVES) {
    return hdb_mfma_f8_lds_supported(d) ? hdb_mfma_f8_lds_chunks(d) * 64 * hdb_mfma_f8_lds_waves(waves, d) * 16 / d : 0;
}
static constexpr int hdb_mfma_f8_lds_bytes(int d, int waves = HDB_F8_LDS_WAVES) { return 2 * hdb_mfma_f8_lds_stage_rows(d, waves) * 2 * d; }
static constexpr int hdb_mfma_f8_lds_wg_per_cu(int d, int waves) { return (d == 512 || hdb_mfma_f8_lds_waves(waves, d) == 8) ? 1 : 2; }
// workgroups of a launch over `ntiles` 16-row tiles: one per stage, at most `limit` (max_blocks, or workgroups per CU x CUs)
static inline int hdb_mfma_f8_lds_blocks(int64_t ntiles, int d, int waves, int limit) {
    const int tps = hdb_mfma_f8_lds_stage_rows(d, waves) / 16;
    const int64_t stages = tps > 0 ? (ntiles + tps - 1) / tps : 0;
    const int64_t b = stages < limit ? stages : limit;
    return b < 1 ? 1 : (int)b;
}
// ... and the number of queries of a call from which the LDS flavour is used when f8_lds_min_q = -1; 0 = never.  d: the stored row
// width -- a whole row or, under f8_ks_min_q, a sliced one.  The rule is the smallest measured batch size from which the LDS flavour
// beats the register flavour by more than the repeated contender's spread at every larger measured size.  Measured, one box, the
// contenders alternating call by call, cosine top-100, p50 in us, LDS (four waves) vs registers at 16 / 32 / 64 / 128 / 256 queries,
// the two p50s of the repeated LDS contender at most 1.6 % apart (10M x 384: 0.2 / 2.3 / 3.7 / 9.5 / 5.6 %)
// (tools/time_f8_lds.py -> profiles/f8_lds_time.txt):
//   10M x 384: 1 480 vs 1 095, 1 575 vs 2 061, 1 855 vs 4 138, 3 566 vs 8 155, 6 994 vs 15 830     -> 32 (1.31x; 16 queries 0.74x)
//    2M x 128:   223 vs   118,   231 vs   177,   260 vs   308,   431 vs   558,   701 vs  1 055     -> 64 (1.18x; 32 queries 0.77x)
//    2M x 256:   367 vs   242,   387 vs   384,   421 vs   665,   772 vs 1 117, 1 191 vs  2 078     -> 64 (1.58x; 32 queries 0.99x)
//    2M x 512:   799 vs   334,   801 vs   563,   845 vs 1 001, 1 616 vs 1 947, 3 185 vs  3 812     -> 64 (1.19x; 32 queries 0.70x)
//    2M x 768:   808 vs   554,   859 vs   932,   964 vs 1 689, 1 831 vs 3 286, 3 611 vs  6 541     -> 32 (1.08x; 16 queries 0.69x)
//  375k x 4096: 1 455 vs   801, 1 520 vs 1 242, 1 663 vs 2 068, 3 199 vs 3 812, 6 268 vs  7 510     -> 64 (1.24x; 32 queries 0.82x)
// The other sliced widths were not measured: 0.  (The option is 0 by default: the rule is used only where a caller sets -1.)
static inline int hdb_mfma_f8_lds_min_q(int d) { return (d == 384 || d == 768) ? 32 : (d == 128 || d == 256 || d == 512 || d == 4096) ? 64 : 0; }

// ---- hdb_mfma_b1*.hip: packed-bit rows on the bf16 matrix pipe (hdb_mfma_b1.h; OPT-IN, the planner's b1_mfma_min_q, 0 = never by default) ----
// Like the float8 slices these rules are no part of hdb_mfma_supported / hdb_mfma_tile_rows / hdb_mfma_ksplit_slices /
// hdb_mfma_batch_capacity / hdb_mfma_fused_supported, which describe the default dispatch and keep answering "no" for HDB_B1.
// Whole rows of 128 / 256 / 384 / 512 elements (the query fragments are bfloat16's: three bf16 parts, 3 d / 8 registers per 16
// queries), 16-row tiles read straight from global memory, as in the float8 register kernel.
static inline int hdb_mfma_b1_tile_rows(int d) { return (d == 128 || d == 256 || d == 384 || d == 512) ? 16 : 0; }
// Wider rows in K slices: the widths and the slices of a width are ks_geom_bf16's; off[s] is the BYTE offset into the stored row
// (an eighth of the element offset into the query: a slice starts on a whole 32-bit word, in fact on a multiple of 16 bytes).
static inline KsGeom ks_geom_b1(int d) {
    const KsGeom b = ks_geom_bf16(d);
    KsGeom g = {};
    g.slices = b.slices;
    for (int s = 0; s < b.slices && s < HDB_KS_MAX_SLICES; ++s) { g.width[s] = b.width[s]; g.off[s] = b.off[s] / 16; }
    return g;
}
static inline int hdb_mfma_b1_ks_slices(int d) { return ks_geom_b1(d).slices; }
// ... and the number of queries of a call from which a packed-bit index takes the matrix cores when b1_mfma_min_q = -1; 0 = never
// (a width nobody measured).  The rule is the smallest measured batch size from which the matrix cores beat the bit scan
// (hdb_bscan.hip: four queries per pass) by more than the repeated contender's spread, for cosine AND euclidean, at every larger
// measured size and at every measured row count of the width.  Measured, one box, the contenders alternating call by call, top-100
// through rank_batch, p50 of 60 calls in us, matrix cores vs bit scan on the same handle at 5 / 8 / 16 / 64 / 128 queries, cosine
// (euclidean in brackets where it decides); spread = the two p50s of the repeated matrix-core contender, up to 14 % at 2M rows, where
// its second turn of a round is the slower one throughout (tools/time_b1_mfma.py -> profiles/b1_mfma_time.txt):
//   10M x 384:  475 vs 472 (517 vs 474), 480 vs 533 (522 vs 533), 504 vs 963, 1 710 vs 3 689, 3 355 vs 7 466      -> 8 (5 queries: 0.99 / 0.92)
//    2M x 384:  139 vs 158, 142 vs 173, 165 vs 287, 396 vs 902, 719 vs 1 724                                      -> 5; the width takes 8
//    2M x 128:  109 vs 113 (94 vs 103, spread 5.9 %), 90 vs 119, 97 vs 191, 219 vs 574, 353 vs 1 085               -> 5 (1.03, spread 1.5 % / 1.09)
//    2M x 256:  114 vs 139 (121 vs 134, spread 8.8 %), 116 vs 149, 123 vs 237, 305 vs 750, 503 vs 1 429           -> 5 (1.21 / 1.10)
//    2M x 512:  161 vs 180 (165 vs 178, spread 6.8 %), 164 vs 188, 187 vs 328, 469 vs 1 077, 863 vs 2 109         -> 5 (1.12 / 1.07)
//    2M x 768:  268 vs 280 (284 vs 275), 305 vs 307 (315 vs 309), 361 vs 542, 1 134 vs 1 944, 2 170 vs 3 862      -> 16 (5 and 8 queries: 0.97-1.04, inside the spread)
//   10M x 1024: 1 633 vs 2 043, 1 633 vs 2 709, 1 695 vs 5 355, 7 573 vs 21 170, 14 834 vs 41 861                 -> 5 (1.25 / 1.21)
//    2M x 1024: 405 vs 481 (410 vs 447), 416 vs 616, 439 vs 1 150, 1 317 vs 4 498, 2 528 vs 8 937                 -> 5 (1.19 / 1.09)
//  375k x 4096: 510 vs 881, 527 vs 1 317, 559 vs 2 481, 1 304 vs 9 336, 2 485 vs 18 219                           -> 5 (1.73)
// The other sliced widths were not measured: 0.  (The option is 0 by default: the rule is used only where a caller sets -1.)
static inline int hdb_mfma_b1_min_q(int d) {
    return d == 384 ? 8 : (d == 128 || d == 256 || d == 512 || d == 1024 || d == 4096) ? 5 : d == 768 ? 16 : 0;
}

// ---- hdb_mfma_qt2.hip: two query tiles per wave ----
static inline int hdb_mfma_qt2_supported(int d) { return d == 128 || d == 256 || d == 512 || d == 640; }

// ---- hdb_mfma.hip: the matrix-core scan ----
// Geometry: rows per LDS stage = the largest of 64 / 32 / 16 whose stage (R * row bytes) fits 48 KiB (three stages + lists
// <= 160 KiB).  Rows are multiples of 256 bytes (the XOR swizzle works on 16 chunks of 16 bytes), so every d that is a
// multiple of 128 (fp16) / 64 (fp32) works; the upper limits are the query fragments a wave holds in registers: d/8
// (fp16) or d/4 (fp32) registers for 16 queries, 192 at most.
// fp16: 16x16x32 MFMAs, 128 queries per pass (d <= 640 with more than 128 queries: two query tiles per wave, 256 per pass).
// fp32: 16x16x4 MFMAs, 128 queries per pass; the matrix pipe (157 TFLOP/s) binds from ~16 queries on, so the VALU scan
// keeps the calls of up to 4 queries (one pass at HBM speed) and this path takes the batches.
// bfloat16 rows (hdb_mfma_bf16.hip): d = 128, 256, 384 and 512 -- the query fragments of 16 queries take 48, 96, 144 and 192
// registers (three bf16 parts); the d = 512 kernels build with 241-256 registers and no scratch, so the width is admitted.  Wider
// bfloat16 rows (640 .. 1536 in steps of 128, 2048 / 3072 / 4096) are cut into K slices of those widths (ks_geom_bf16)

static inline int mfma_exact_tile_rows(int dtype, int d) {
    if (dtype == HDB_BF16 && d > 0 && hdb_mfma_ksplit_slices(dtype, d) > 0) return 16;     // 640 .. 4096: K slices of 16-row stages (hdb_mfma_bf16_ks.hip)
    if (dtype == HDB_BF16) return d > 0 ? hdb_mfma_bf16_tile_rows(d) : 0;
    if (dtype == HDB_F8E4M3 || dtype == HDB_I8) return d > 0 ? hdb_mfma_f8_tile_rows(d) : 0;      // (int8: the float8 kernel with another row converter, hdb_mfma_i8.hip)
    if ((dtype != HDB_F16 && dtype != HDB_F32) || d <= 0) return 0;       // (packed bits, float64: no matrix cores)
    if (hdb_mfma_ksplit_slices(dtype, d) > 0) return 16;                  // wide rows: K slices of 16-row stages (hdb_mfma_ksplit.hip)
    const int row_bytes = (int)hdb_row_bytes(dtype, d);
    if (row_bytes % 256 != 0 || row_bytes > 3072) return 0;          // d <= 1536 (fp16) / 768 (fp32)
    if (dtype == HDB_F32 && d != 128 && d != 256 && d != 384 && d != 512 && d != 768) return 0;     // instantiated fp32 widths
    for (int r = 64; r >= 16; r >>= 1)
        if (r * row_bytes <= 48 * 1024) return r;
    return 0;
}

// Rows of any width that is a multiple of 16 bytes and has no geometry of its own ride the next wider one as a single K slice
// (hdb_mfma_anyd.h): -> that width, or 0.  fp16 d % 8 == 0 up to 1024, float32 d % 4 == 0 up to 768.
static inline int hdb_mfma_anyd_pad(int dtype, int d) {
    if (dtype != HDB_F16 && dtype != HDB_F32) return 0;      // (bfloat16: its own widths only)
    if (d <= 0 || hdb_row_bytes(dtype, d) % 16 != 0 || mfma_exact_tile_rows(dtype, d) > 0) return 0;
    static const int w16[] = {128, 256, 384, 512, 768, 1024}, w32[] = {128, 256, 384, 512, 768};
    if (dtype == HDB_F16) { for (int w : w16) if (w >= d) return w; }
    else { for (int w : w32) if (w >= d) return w; }
    return 0;
}

static inline int hdb_mfma_tile_rows(int dtype, int d) {
    const int pad = hdb_mfma_anyd_pad(dtype, d);
    return mfma_exact_tile_rows(dtype, pad ? pad : d);
}

// queries ONE launch of the MFMA scan covers (grid.y == 1): what a single-launch (mode 2) call can take
static inline int hdb_mfma_batch_capacity(int dtype, int d) {
    if (hdb_mfma_tile_rows(dtype, d) <= 0 || hdb_mfma_ksplit_slices(dtype, d) > 0 || hdb_mfma_anyd_pad(dtype, d) > 0) return 0;      // (K slices, odd widths: the multi-kernel pipeline)
    if (dtype == HDB_BF16 || dtype == HDB_F8E4M3 || dtype == HDB_I8) return 0;      // (bfloat16, float8 and int8 rows likewise: no single launch is built)
    if (dtype == HDB_F32) return (d == 512 || d == 768) ? 64 : 128;      // (d = 512 / 768: the bf16-part flavour pairs its waves over K, hdb_mfma_kernel.h KP)
    return (d == 384 || d == 128 || d == 256 || d == 512 || d == 640) ? 256 : 128;      // two query tiles per wave (hdb_mfma_qt2.hip)
}

static inline int hdb_mfma_supported(int dtype, int d, int metric) {
    return hdb_mfma_tile_rows(dtype, d) > 0 && (metric == HDB_DOT || metric == HDB_COSINE || metric == HDB_EUCLIDEAN);
}

// float32 widths whose scan also exists in bf16 parts (hdb_mfma_f32s.hip) -> the number of queries of a CALL from which that
// flavour is used (0: no such flavour; the API decides per call, ScanArgs::f32_split).  d <= 384: measured from 16 queries up, never
// slower than the float32 MFMAs and 1.5-1.7x faster from 48 (profiles/r4_f32_bf16_parts.txt); d = 512 / 768: one wave cannot hold the
// query fragments of a whole row, the float32 flavour runs 16-row tiles on one SIMD per 16 queries (2x a pass at any batch size), the
// bf16-part flavour splits K over two waves.
// Other float32 widths ride these geometries (any multiple of 4 up to 768 as one padded slice, hdb_mfma_anyd.h; 1024 / 1536 as two
// slices of 512 / 768, hdb_mfma_ksplit.hip) and follow the geometry's rule.
// ... and the largest call that flavour takes (d = 1024: the paired waves hold 64 queries per launch row, so 65-128 queries read the
// two slices twice -- 2 650 against 2 350 us at 128 queries on 1M rows, profiles/r4_f32_bf16_parts.txt)
static inline int hdb_mfma_f32_split_max_q(int d) { return d == 1024 ? 64 : 1 << 30; }
static inline int hdb_mfma_f32_split_min_q(int d) {
    if (d == 1024 || d == 1536) return 1;
    const int g = (d == 128 || d == 256 || d == 384 || d == 512 || d == 768) ? d : hdb_mfma_anyd_pad(HDB_F32, d);
    return (g == 128 || g == 256 || g == 384) ? 9 : (g == 512 || g == 768) ? 1 : 0;
}

// ---- hdb_mfma_fused*.hip: the single launch of 1-4 queries ----
#define HDB_FUSED_MAXQ 4            // queries per fused call
#define HDB_FUSED_MAX_WG 1024
static inline int hdb_mfma_fused_supported(int dtype, int d, int metric, int nq, uint32_t kk) {
    // fp16: every width the batched scan takes (multiples of 128 up to 1536); beyond d = 768 the query fragments (d/8
    // registers) leave no room for the selectors' state: they stay in LDS, up to 2 queries (hdb_mfma_fused_wide.hip)
    // (d = 896: 28-KiB tiles of 28 k-steps keep the one multiplying wave busier than the stream: five kernels are 6 % faster)
    // (d = 128: 16-KiB tiles -- a round of this kernel costs ~1 us whatever the tile holds: 660 vs 400 us at 10 M rows)
    const bool shape = (dtype == HDB_F16 && hdb_mfma_tile_rows(dtype, d) > 0 && d % 128 == 0 && d != 896 && d != 128 && d <= 1536) ||
                       (dtype == HDB_F32 && (d == 128 || d == 256 || d == 384 || d == 512 || d == 768));   // float32: VALU flavour
    // float32 queries live in registers as d/4 floats per lane group: 48 registers = 2 queries up to d = 384, 1 beyond
    const int maxq = dtype == HDB_F32 ? (d <= 384 ? 2 : 1) : (d <= 768 ? HDB_FUSED_MAXQ : 2);
    // euclidean (the MFMA expansion + direct re-score of near-duplicates in the last workgroup): fp16 matrices only -- the
    // float32 VALU pipelines compute the direct difference, which this kernel's float32 flavour does not; d = 768 would spill
    // three registers (those calls take the batched single launch, hdb_mfma_kernel.h MODE 2)
    // (euclidean, 2-4 queries: wave 0 pays sqrt + rcp on all 16 MFMA columns -- 199 vs 182 us at N=1.25M d=384 with four queries; those
    // calls take the batched single launch, where eight waves share the epilogue)
    // float32 (round 3): the VALU flavour accumulates (v - q)^2 directly, as hdb_scan.hip does -- no cancellation, nothing to
    // re-score, one or two queries like dot / cosine
    const bool euclid = metric == HDB_EUCLIDEAN && ((dtype == HDB_F16 && d != 768 && nq == 1) || dtype == HDB_F32);
    return shape && (metric == HDB_DOT || metric == HDB_COSINE || metric == HDB_PEARSON || euclid) && nq >= 1 && nq <= maxq && kk <= 128;
}

// Local flavour (FusedArgs::local, hdb_mfma_fused.h): how many tiles of a workgroup fit its parking area -- 0 where the kernel
// does not park at all (fp16 d = 768; euclidean d = 640: the parking state would spill there).  Mirrors PARK / pend_max.
static inline int hdb_mfma_fused_local_tiles(int dtype, int d, int metric, int nq) {
    if (dtype == HDB_F32) return nq <= 1 || d > 384 ? 16 : 8;
    const bool park = (d <= 640 && !(metric == HDB_EUCLIDEAN && d > 512)) || d > 768;
    if (!park) return 0;
    return nq <= 2 ? 16 : 32 / nq;
}
// workgroups of hdb_launch_mfma_fused over `ntiles` tiles: one per CU at most
static inline int hdb_mfma_fused_blocks(int64_t ntiles, int cus, int max_blocks) {
    int blocks = (int)(ntiles < cus ? ntiles : cus);
    if (max_blocks > 0 && max_blocks < blocks) blocks = max_blocks;
    if (blocks > HDB_FUSED_MAX_WG) blocks = HDB_FUSED_MAX_WG;
    if (blocks < 1) blocks = 1;
    return blocks;
}

// ---- hdb_bits_fused.hip: the single launch of the bit metrics ----
#ifndef HDB_BITS_THREADS
#define HDB_BITS_THREADS 1024
#endif
#define HDB_BITS_MAXW 512
static inline int hdb_bits_fused_supported(int metric, int nq, int W, uint32_t kk) {
    return (metric == HDB_HAMMING || metric == HDB_JACCARD) && nq >= 1 && nq <= 4 && W <= HDB_BITS_MAXW && kk <= 128;
}
// workgroups of hdb_launch_bits_fused over `ntiles` 16-row tiles
static inline int hdb_bits_fused_blocks(int64_t ntiles, int cus, int max_blocks) {
    int blocks = cus;
    const int64_t items = ntiles * 4;
    if ((int64_t)blocks * HDB_BITS_THREADS > items) blocks = (int)((items + HDB_BITS_THREADS - 1) / HDB_BITS_THREADS);
    if (max_blocks > 0 && max_blocks < blocks) blocks = max_blocks;
    if (blocks < 1) blocks = 1;
    return blocks;
}
// the local flavour needs every workgroup's share of the k best rows far below the 8 it emits at least: grids of 2 k workgroups
// and more (k = 100: matrices of 820k rows and more; P(Poisson(0.5) >= 8) = 2e-7 per workgroup), else the exchange flavour
static inline bool hdb_bits_fused_local(int blocks, uint32_t kk) { return (int64_t)blocks >= 2 * (int64_t)kk; }

// ---- hdb_l1_tile.hip: dense manhattan passes ----
// rows that are multiples of 256 bytes up to 1536 bytes (fp16 d <= 768, float32 d <= 384: two or four float32 queries per wave in registers)
// Measured against the 4-query scan in one process (profiles/r3_manhattan_tile_vs_scan.txt): fp16 d=384, 5 M rows: 800 vs 1 372 us
// (2 queries), 1 187 vs 2 558 (5), 1 390 vs 2 728 (8); fp16 d=128: 559 vs 986 (5); float32 d=384, 2 M rows: 594 vs 1 083 (5).
// One query: equal (the single-query scan keeps it).  fp16 d = 512 keeps two queries per wave, d = 640 / 768 one (two copies of a
// 768-element query are 96 registers next to the tile chunks: spills); they still share the staged tile between the waves:
// d = 768, 2.5 M rows: 589 vs 1 231 us (2 queries), 1 531 vs 2 484 (5), 3 674 vs 4 813 (16); d = 512, 4 M rows: 1 275 vs 2 686 (5).
static inline int hdb_l1_tile_supported(int dtype, int d) {
    if (dtype == HDB_F16) return d == 128 || d == 256 || d == 384 || d == 512 || d == 640 || d == 768;      // (512: two queries per wave; 640 / 768: one)
    if (dtype == HDB_F32) return d == 128 || d == 256 || d == 384 || d == 512 || d == 768;      // (512: two queries per wave, 16-row tiles; 768: one)
    return 0;
}
// The packed-fp16 flavour of that kernel (fp16 rows, queries that are fp16 numbers) rounds v - q to fp16: a difference beyond 65504
// becomes inf, the row's sum inf and its score 0 where the float32 flavour and the reference stay finite.  It is taken only where no
// difference can leave fp16 range: every stored element and every query element within HDB_L1_PK_MAX = 65504 / 2 in magnitude.
//   the matrix: bit HDB_FLAG_L1_WIDE of the index's flag word, set by the row-norm kernels for a row whose sum of squares exceeds
//     HDB_L1_PK_MAX^2 -- no element of a row below that can exceed HDB_L1_PK_MAX (a sufficient test that costs the build nothing;
//     a matrix of many moderately large elements loses the packed flavour with it and keeps the float32 one);
//   the queries: the kernel's own wave-uniform test beside "is an fp16 number".
#define HDB_L1_PK_MAX 32752.0f
#define HDB_FLAG_NAN 1            // bits of hdb_index::nan_flag: a NaN row,
#define HDB_FLAG_INF 2            // a row with an infinite sum of squares,
#define HDB_FLAG_L1_WIDE 4        // a row that may hold an element beyond HDB_L1_PK_MAX
static inline bool hdb_l1_packed_ok(int dtype, int64_t l1_packed_opt, int flags) {
    return dtype == HDB_F16 && l1_packed_opt != 0 && flags >= 0 && (flags & HDB_FLAG_L1_WIDE) == 0;      // (flags < 0: not fetched)
}

// ---- hdb_quant.hip: the int8 shadow and its 5-bit plane ----
// workgroups a launch over `ntiles` tiles takes (the folded threshold keeps 4 x that many per-wave maxima of the sample pass)
static inline int hdb_quant_scan_blocks(int64_t ntiles, int max_blocks) { return hdb_grid_for(ntiles, 4, max_blocks > 0 ? max_blocks : 1024); }
// The 5-bit plane: units of a row
static inline int hdb_quant_plane_units(int P) { return (P + 31) / 32; }
// ... and 16-byte pieces a lane takes of a tile: the J of hdb_quant_plane_scan_kernel<J, DBG> (1 .. 4 for rows of up to 512 elements)
static constexpr int hdb_quant_plane_j(int U) { return (U + 3) / 4; }
// The grid of the plane pass (hdb_quant_plane_scan_kernel<J, false>): workgroups of four waves, a wave takes two tiles per step, so
// one workgroup per four step-pairs of the `nwalk` tiles it walks, at most wg_per_cu per CU.  Every workgroup of the grid is resident
// while wg_per_cu does not exceed the waves per SIMD the kernel is compiled for (four waves of a workgroup: one per SIMD), and the
// static split of the walk is balanced only then.  HDB_PLANE_WAVES: what the compiler gives <J, false>, J = 1 .. 4
// (profiles/plane_occupancy_kernel_resources.txt; the figures move with the compiler, and so must this line).
// HDB_PLANE_WG_PER_CU: the default per J.  An entry moves off 4 (the grid the pass had on 256 CUs) only where another grid won in
// both of two runs at every measured size from 2M rows up (profiles/plane_occupancy_time.txt, DESIGN.md section 4, "The 5-bit
// plane"; tools/time_quant.py --auto --plane-grid, one handle, the settings alternating call by call, p50 of a call in us, run 1 /
// run 2).  More waves than four per SIMD bought nothing at any width; FEWER win where a wave has three or four pieces in flight:
//   J = 3 (d = 384), 3 against 4: 2M 141.6 / 141.3 vs 143.1 / 143.2, 2.5M 167.6 / 168.3 vs 170.8 / 170.3, 3M 189.4 / 188.5 vs 191.4 /
//     190.7, 5M 274.7 / 274.6 vs 279.5 / 279.0, 10M 464.1 / 481.8 vs 481.3 / 493.5 (2 loses: 487.7 / 496.9; 5 .. 7: 482.6 .. 505.6)   -> 3
//   J = 4 (d = 512), 2 against 4: 2M 181.3 / 181.2 vs 184.4 / 184.5, 3M 239.7 / 239.2 vs 245.5 / 245.9, 10M 597.9 / 596.7 vs 622.2 /
//     621.9 (3: 614.4 / 615.9; 5: 626.4 / 618.9; 1 was not measured)                                                            -> 2
//   J = 2 (d = 256): 3 wins at 10M (344.0 / 343.4 vs 347.8 / 349.0) and loses at 2M (115.3 / 115.6 vs 114.4 / 114.8); 6 and 8 lose  -> 4
//   J = 1 (d = 128): 5 .. 7 win at 5M and 10M (10M: 223.8 / 223.3 vs 235.5 / 236.1) and do not at 2M (90.2 / 90.3 vs 89.8 / 90.0)      -> 4
// The option plane_wg_per_cu (1 .. 8) puts any value in the table's place for A/B runs -- more than the compiled waves only queues
// workgroups behind the resident ones.
#define HDB_PLANE_WAVES {8, 8, 7, 5}
#define HDB_PLANE_WG_PER_CU {4, 4, 3, 2}
static constexpr int hdb_quant_plane_waves(int J) { constexpr int t[4] = HDB_PLANE_WAVES; return t[J < 1 ? 0 : J > 4 ? 3 : J - 1]; }
static constexpr int hdb_quant_plane_wg_per_cu(int J) { constexpr int t[4] = HDB_PLANE_WG_PER_CU; return t[J < 1 ? 0 : J > 4 ? 3 : J - 1]; }
static_assert(hdb_quant_plane_wg_per_cu(1) >= 1 && hdb_quant_plane_wg_per_cu(1) <= hdb_quant_plane_waves(1) &&
              hdb_quant_plane_wg_per_cu(2) >= 1 && hdb_quant_plane_wg_per_cu(2) <= hdb_quant_plane_waves(2) &&
              hdb_quant_plane_wg_per_cu(3) >= 1 && hdb_quant_plane_wg_per_cu(3) <= hdb_quant_plane_waves(3) &&
              hdb_quant_plane_wg_per_cu(4) >= 1 && hdb_quant_plane_wg_per_cu(4) <= hdb_quant_plane_waves(4),
              "a default grid of the plane pass asks for more waves per SIMD than its kernel is compiled for");
// wg_per_cu: 0 = the table, 1 .. 8 = that many; max_blocks > 0 caps the result as it caps every grid
static inline int hdb_quant_plane_blocks(int64_t nwalk, int J, int cus, int wg_per_cu, int max_blocks) {
    const int per_cu = wg_per_cu >= 1 ? (wg_per_cu < 8 ? wg_per_cu : 8) : hdb_quant_plane_wg_per_cu(J);
    int64_t limit = (int64_t)per_cu * (cus > 0 ? cus : 1);
    if (max_blocks > 0 && max_blocks < limit) limit = max_blocks;
    return hdb_grid_for((nwalk + 1) / 2, 4, (int)limit);
}
// ... and of the test entry (DBG: every tile, no list): the 1024 workgroups the pass had before its grid followed the device
static inline int hdb_quant_plane_dbg_blocks(int64_t ntiles, int max_blocks) { return hdb_grid_for((ntiles + 1) / 2, 4, max_blocks > 0 ? max_blocks : 1024); }
// The plane pass of a one-query call does not stream the tiles the sample pass evaluated (it takes their upper bounds from the
// list that pass left, QuantArgs::pl_hi): it walks a dense index t' over the OTHER tiles.  The sample takes one tile of each
// window w < s_tiles of `stride` tiles, hdb_tile_index(w, stride); the tiles from s_tiles x stride on (the ragged last one among
// them) are in no window.  A position is (w, o): w < s_tiles and o < stride - 1 counts the window's tiles with the sampled one
// left out, or w == s_tiles and o counts the tiles behind the last window.  s_tiles == 0: no sample, every tile is walked.
// One division where a walk starts; a step of `step` positions adds (step / (stride - 1), step % (stride - 1)), which the walker
// forms once, so that nothing divides per step but hdb_tile_index itself.  (stride == 1: the sample is a dense prefix, no window
// has a tile of its own and every position is in the tail.)  Tile numbers fit 32 bits: a row number does (hdb_pack).
// (__host__ __device__: the kernel walks with these very functions, tests/plane_skip_check.hip walks them on the host.)
struct HdbSkipPos { uint32_t w, o; };
struct HdbSkipStep { uint32_t dw, dn, step; };        // (windows, positions inside a window, positions) of one step
__host__ __device__ __forceinline__ uint32_t hdb_plane_skip_count(uint32_t ntiles, uint32_t s_tiles) { return ntiles - s_tiles; }
__host__ __device__ __forceinline__ HdbSkipStep hdb_plane_skip_step(uint32_t step, uint32_t stride) {
    const uint32_t m = stride - 1u;
    HdbSkipStep s;
    s.dw = m ? step / m : 0u; s.dn = m ? step % m : 0u; s.step = step;
    return s;
}
__host__ __device__ __forceinline__ HdbSkipPos hdb_plane_skip_start(uint32_t tp, uint32_t s_tiles, uint32_t stride) {
    const uint32_t m = stride - 1u;
    HdbSkipPos p;
    const uint32_t w = m ? tp / m : s_tiles;
    if (w < s_tiles) { p.w = w; p.o = tp - w * m; }
    else { p.w = s_tiles; p.o = tp - s_tiles * m; }
    return p;
}
// (the step must come from hdb_plane_skip_step with the same stride, or be {0, 1, 1}: the next position)
__host__ __device__ __forceinline__ void hdb_plane_skip_advance(HdbSkipPos& p, const HdbSkipStep& s, uint32_t s_tiles, uint32_t stride) {
    if (p.w >= s_tiles) { p.o += s.step; return; }
    const uint32_t m = stride - 1u;
    p.w += s.dw; p.o += s.dn;
    if (p.o >= m) { p.o -= m; ++p.w; }
    if (p.w >= s_tiles) { p.o += (p.w - s_tiles) * m; p.w = s_tiles; }
}
__host__ __device__ __forceinline__ int64_t hdb_plane_skip_tile(const HdbSkipPos& p, uint32_t s_tiles, uint32_t stride) {
    if (p.w >= s_tiles) return (int64_t)s_tiles * stride + p.o;
    const uint32_t jit = (uint32_t)(hdb_tile_index((int64_t)p.w, (int64_t)stride) - (int64_t)p.w * stride);
    return (int64_t)p.w * stride + p.o + (p.o >= jit ? 1u : 0u);
}
// The row terms of the plane pass (hdb_quant.hip, "The 5-bit plane": the hot block).  The record array keeps 16 bytes per row, laid
// out per 16-row tile: 256 bytes = [0, 64) the hot block of dot-product calls, [64, 128) that of cosine calls, [128, 256) reserved
// (zero).  A hot block: 16 bfloat16 k_hi (row r's scale -- s_r, cosine: s_r / ||v_r|| -- rounded UP), 16 bytes rc = ceil(2 R_r),
// then four float32 words of the tile: E*, T* (the maxima of E_r and T_r over the tile's rows, cosine: of E_r / ||v_r|| and
// T_r / ||v_r||, rounded up), F* (the bound's absolute floor 2^-100 (d + 8), cosine: times the largest 1 / ||v_r||, rounded up)
// and a zero.  Pass 1 reads one block per tile; the numbers only ever widen its bound, and no bit of them reaches an answer.
// (__host__ __device__: hdb_quant_plane_rows_kernel writes with these functions, hdb_quant_plane_scan_kernel reads with them and
// tests/plane_block_check.hip runs them on the host.)
#define HDB_PLANE_TILE_BYTES 256
#define HDB_PLANE_BLOCK_BYTES 64
#define HDB_PLANE_BLOCK_DOT 0
#define HDB_PLANE_BLOCK_COSINE 1
#define HDB_PLANE_BLOCK_K 0           // byte offsets inside a hot block: 16 x bf16 k_hi,
#define HDB_PLANE_BLOCK_RC 32         // 16 x u8 rc,
#define HDB_PLANE_BLOCK_TILE 48       // {E*, T*, F*, 0} float32
// bytes of the record array for `rows` rows: whole tiles (16 bytes per row all the same)
__host__ __device__ __forceinline__ int64_t hdb_plane_rec_bytes(int64_t rows) { return (rows + 15) / 16 * HDB_PLANE_TILE_BYTES; }
__host__ __device__ __forceinline__ int64_t hdb_plane_block_off(int64_t tile, int flavour) {
    return tile * HDB_PLANE_TILE_BYTES + (int64_t)flavour * HDB_PLANE_BLOCK_BYTES;
}
__host__ __device__ __forceinline__ float hdb_plane_bits_f(uint32_t u) { union { uint32_t u; float f; } c; c.u = u; return c.f; }
__host__ __device__ __forceinline__ uint32_t hdb_plane_f_bits(float f) { union { uint32_t u; float f; } c; c.f = f; return c.u; }
// The smallest bfloat16 at or above the non-negative float64 k (the high half of a float32; infinity where k is beyond the largest
// finite bfloat16, which no scale of a finite row reaches; a NaN stays one).  Exact: a bfloat16 is a float32 is a float64.
__host__ __device__ __forceinline__ uint16_t hdb_plane_k_encode(double k) {
    if (!(k > 0.0)) return k == k ? (uint16_t)0 : (uint16_t)0x7FC0;
    float f = (float)k;                                   // (rne: at most half a float32 ulp below k, then the truncation is at or below k)
    if (f != f || f - f != 0.f) return (uint16_t)0x7F80;
    uint32_t h = hdb_plane_f_bits(f) >> 16;               // truncated: at or below f
    if ((double)hdb_plane_bits_f(h << 16) < k) ++h;       // next bfloat16 (carries into the exponent, up to infinity, as the bits do)
    return (uint16_t)h;
}
__host__ __device__ __forceinline__ float hdb_plane_k_hi(uint32_t code) { return hdb_plane_bits_f(code << 16); }
// The lower side is derived: bfloat16 numbers from 2^-126 on are at most a factor 1 + 2^-7 apart, so the k that rounded up to k_hi
// is above k_hi (1 - 2^-7) (an exact float32 product: 8 x 7 bits); below that the spacing is absolute and the lower side is 0, as
// it is for an infinite k_hi.
__host__ __device__ __forceinline__ float hdb_plane_k_lo(float k_hi) {
    return k_hi >= 0x1p-126f && k_hi <= 0x1.fep127f ? k_hi * (1.f - 0x1p-7f) : 0.f;
}
// rc = ceil(2 R) for R = sqrt(ss), ss the integer sum of squared residuals of a row (at most 16 x 512, so rc <= 182): the smallest
// integer with rc^2 >= 4 ss, in integers.  It decodes as 0.5 rc >= R, exactly.
__host__ __device__ __forceinline__ uint32_t hdb_plane_rc_encode(uint32_t ss) {
    const uint32_t t = 4u * ss;
    uint32_t rc = (uint32_t)sqrtf((float)t);
    while (rc * rc < t) ++rc;
    while (rc > 0u && (rc - 1u) * (rc - 1u) >= t) --rc;
    return rc < 255u ? rc : 255u;
}
__host__ __device__ __forceinline__ float hdb_plane_rc_decode(uint32_t rc) { return 0.5f * (float)rc; }
// float32 at or above the non-negative float64 x (a NaN or an overflow: infinity, which keeps every row of the tile)
__host__ __device__ __forceinline__ float hdb_plane_up(double x) {
    if (!(x > 0.0)) return x == x ? 0.f : hdb_plane_bits_f(0x7F800000u);
    float f = (float)x;
    if (f != f || f - f != 0.f) return hdb_plane_bits_f(0x7F800000u);
    if ((double)f < x) f = hdb_plane_bits_f(hdb_plane_f_bits(f) + 1u);
    return f;
}

// ---- hdb_quant_mfma.hip: batches through the shadow on the int8 matrix cores ----
// widths the int8 matrix-core filter and the block-diagonal rescoring take: whole 64-byte k-steps and a geometry of the fp16 scan
static inline int hdb_qb_supported(int d) { return d == 128 || d == 256 || d == 384 || d == 512; }
// wave groups over the queries and query tiles per wave for a chunk of nq queries
static inline void qb_shape(int nq, int& wq, int& nqt) {
    const int tq = (nq + 15) / 16;
    wq = tq <= 4 ? 1 : tq <= 8 ? 2 : 4;
    nqt = (tq + wq - 1) / wq;
}
static inline int hdb_qb_scan_blocks(int64_t ntiles, int nq, int cus, int max_blocks) {
    int wq, nqt; qb_shape(nq, wq, nqt);
    const int64_t lim = max_blocks > 0 ? max_blocks : 2 * (int64_t)cus;
    return hdb_grid_for(ntiles, 4 / wq, (int)(lim < 512 ? lim : 512));
}
// slots of wstat every query has after a MODE 0 launch of that many workgroups
static inline int64_t hdb_qb_slots(int blocks, int nq) { int wq, nqt; qb_shape(nq, wq, nqt); return (int64_t)blocks * (4 / wq) * 4; }

// ---- hdb_maxsim.hip: multi-vector queries ----
// Lanes that own one group in the reduction (hdb_maxsim_reduce_kernel<TEAM>), from the mean group size n / n_groups: a team reads
// its group's rows TEAM at a time, so a team wider than the group idles lanes and a team far narrower walks it alone.  The steps were
// derived -- a lane takes about four rows of a mean group -- and then measured (tools/time_maxsim.py, profiles/maxsim_time.txt, one
// device, cosine top-10, p50 of 60 calls in us, team 1 / 4 / 16 / 64; the rule's choice in brackets):
//   10M x 128 fp16, groups of 100, 32 vectors:      2 518 / 1 798 / [1 659] / 1 874        8 sets: 16 717 / 10 743 / [9 682] / 11 283
//   2M x 384 fp32, groups of 4, 4 vectors:          [602] / 614 / 651 / 804
//   2M x 384 fp16, every row a group, 8 vectors:    [399] / 458 / 705 / 1 776
//   2M x 384 fp16, groups of 4 shuffled, 4 vectors: [464] / 479 / 484 / 644
//   200k x 384 fp16, ONE group, 4 vectors:          50 924 / 15 361 / 6 909 / [1 928]      (one team walks all rows: not split, see the header's Not-built list)
// In every measured shape the rule's team is the fastest; sizes between the steps (mean 5 .. 50, 100 .. 200k) are
// not measured.  The option maxsim_team fixes the team for such runs.
static inline int hdb_maxsim_team_rule(int64_t n, int64_t n_groups) {
    const int64_t mean = n_groups > 0 ? n / n_groups : n;
    return mean <= 4 ? 1 : mean <= 32 ? 4 : mean <= 256 ? 16 : 64;
}

// ---- hdb_mmr.hip: diverse top-k (maximal marginal relevance) ----
// The pair pass works on tiles of HDB_MMR_TILE candidates: a workgroup of HDB_MMR_TILE^2 threads, one pair each.  Every extent
// that depends on a list length m uses m rounded up to the tile.
#define HDB_MMR_TILE 16
#define HDB_MMR_SELECT_THREADS 256        // hdb_mmr_select_kernel: candidate c belongs to thread c mod 256, HDB_MAX_K / 256 = 8 per thread
static inline int hdb_mmr_mp(int m) { return (m + HDB_MMR_TILE - 1) / HDB_MMR_TILE * HDB_MMR_TILE; }
