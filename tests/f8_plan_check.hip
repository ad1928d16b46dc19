// f8_plan_check.hip -- what the host side of the library says about float8 e4m3 matrices (HDB_F8E4M3 = 5): a stand-alone program,
// no GPU call.
// 1) the element: hdb_elem_bytes(5) == 1, code 4 has no size; hdb_f8_to_f widens each of the 256 codes to the value its fields spell
//    (sign, exponent - 7, mantissa / 8; exponent 0 = subnormal; 0x7F / 0xFF = NaN), computed here with ldexp;
// 2) the capability rules (csrc/hdb_caps.h): the matrix cores take d = 128 / 256 / 384 / 512 in 16-row tiles and nothing else (no
//    padded widths, no K slices), no single launch, no LDS tile kernel for any width; the grid of the VALU scan grows for 256- /
//    384- / 512-byte rows and is what it was for every other dtype and width; the register kernels' grid (hdb_mfma_reg_blocks) is
//    max_blocks or four workgroups per CU, at most the tiles, at least one;
// 3) plan_topk (csrc/hdb_plan.h) over n x d x nq x k x metric x bias / mask x finite x exact x options: never the shadow, the plane,
//    a matrix-core single launch or the tile kernel; the matrix cores EXACTLY for 5 or more dot / cosine / euclidean / pearson
//    queries on a finite matrix of the four widths above 8 192 rows with use_mfma on (the finiteness is asked exactly where it
//    decides); the bit metrics may take their single launch; every other plan -- small, sampled, exact, full sort, row list -- is
//    field for field the plan of a bfloat16 matrix of the same shape with use_mfma = 0; sample tile heights are
//    hdb_mfma_tile_rows on the matrix cores and the VALU scan's 16 rows elsewhere.
// Prints "plans N" and "F failures"; exit status 1 on any failure.
#include "plan_check.h"
#include <cmath>
#include <cstdio>

int main() {
    // ---- 1: the element ----
    CHECK(HDB_F8E4M3 == 5 && hdb_elem_bytes(HDB_F8E4M3) == 1, "one byte per element");
    CHECK(hdb_elem_bytes(4) == 0 && hdb_elem_bytes(6) == 0 && hdb_elem_bytes(-1) == 0, "unassigned codes have no size");
    CHECK(hdb_elem_bytes(HDB_F16) == 2 && hdb_elem_bytes(HDB_F32) == 4 && hdb_elem_bytes(HDB_F64) == 8 && hdb_elem_bytes(HDB_BF16) == 2, "the other sizes stay");
    CHECK(sizeof(hdb_f8) == 1, "hdb_f8 is one byte");
    int finite = 0;
    for (int code = 0; code < 256; ++code) {
        const float got = hdb_f8_to_f(hdb_f8{(unsigned char)code});
        const int e = (code >> 3) & 15, m = code & 7;
        if ((code & 0x7F) == 0x7F) { CHECK(got != got, "code %d is NaN", code); continue; }
        ++finite;
        const float mag = e == 0 ? std::ldexp((float)m, -9) : std::ldexp(1.f + (float)m / 8.f, e - 7);
        const float want = (code & 0x80) ? -mag : mag;
        CHECK(got == want && std::signbit(got) == std::signbit(want), "code %d widens to %g, its fields spell %g", code, (double)got, (double)want);
    }
    CHECK(finite == 254, "254 finite codes");
    CHECK(hdb_f8_to_f(hdb_f8{0x7E}) == 448.f && hdb_f8_to_f(hdb_f8{0xFE}) == -448.f && hdb_f8_to_f(hdb_f8{0x01}) == 0.001953125f, "the ends of the range");

    // ---- 2: the capability rules ----
    for (int d = 1; d <= 4096; ++d) {
        const bool wd = d == 128 || d == 256 || d == 384 || d == 512;
        CHECK(hdb_mfma_tile_rows(HDB_F8E4M3, d) == (wd ? 16 : 0) && hdb_mfma_f8_tile_rows(d) == (wd ? 16 : 0), "d %d", d);
        CHECK(hdb_mfma_anyd_pad(HDB_F8E4M3, d) == 0 && hdb_mfma_ksplit_slices(HDB_F8E4M3, d) == 0, "d %d", d);
        CHECK(hdb_mfma_batch_capacity(HDB_F8E4M3, d) == 0 && !hdb_l1_tile_supported(HDB_F8E4M3, d), "d %d", d);
        for (int metric = HDB_DOT; metric <= HDB_PEARSON; ++metric) {
            const bool mm = metric == HDB_DOT || metric == HDB_COSINE || metric == HDB_EUCLIDEAN;     // (pearson asks as cosine)
            CHECK((hdb_mfma_supported(HDB_F8E4M3, d, metric) != 0) == (wd && mm), "d %d metric %d", d, metric);
            CHECK(!hdb_mfma_fused_supported(HDB_F8E4M3, d, metric, 1, 100), "d %d metric %d", d, metric);
        }
    }
    // blocks x tile bytes is what it is for 768-byte rows, up to four workgroups per CU
    CHECK(hdb_scan_auto_blocks(HDB_F8E4M3, 256, true, false) == 1024, "256-byte rows");
    CHECK(hdb_scan_auto_blocks(HDB_F8E4M3, 384, true, false) == 1024, "384-byte rows");
    CHECK(hdb_scan_auto_blocks(HDB_F8E4M3, 512, true, false) == 768, "512-byte rows");
    CHECK(hdb_scan_auto_blocks(HDB_F8E4M3, 384, false, false) == 512 && hdb_scan_auto_blocks(HDB_F8E4M3, 768, true, false) == 512 &&
          hdb_scan_auto_blocks(HDB_F8E4M3, 272, true, false) == 512 && hdb_scan_auto_blocks(HDB_F8E4M3, 100, false, false) == 512, "other float8 rows");
    for (int dt : {(int)HDB_F16, (int)HDB_F32, (int)HDB_F64, (int)HDB_BF16}) for (int rb : {256, 384, 512, 768, 1536, 3072})
        CHECK(hdb_scan_auto_blocks(dt, rb, true, false) == 512 && hdb_scan_auto_blocks(dt, rb, true, true) == 256, "dtype %d, %d-byte rows", dt, rb);

    // the grid of the register kernels (float8, int8, packed bits): the rule against the expression the router spelled out three times
    for (int cus : {1, 256}) for (int max_blocks : {-2, 0, 1, 7, 5000})
    for (int64_t ntiles : {(int64_t)0, (int64_t)1, (int64_t)3, (int64_t)4 * cus - 1, (int64_t)4 * cus, (int64_t)4 * cus + 1, (int64_t)10000000}) {
        const int64_t want8 = max_blocks > 0 ? max_blocks : 4 * (int64_t)cus;
        const int blocks8 = (int)(ntiles < want8 ? (ntiles < 1 ? 1 : ntiles) : want8);
        CHECK(hdb_mfma_reg_blocks(ntiles, cus, max_blocks) == blocks8 && blocks8 >= 1, "ntiles %lld cus %d max_blocks %d", (long long)ntiles, cus, max_blocks);
    }

    // ---- 3: the planner ----
    long plans = 0;
    const int ds[] = {7, 100, 128, 256, 272, 384, 512, 768, 1024};
    const int nqs[] = {1, 2, 4, 5, 8, 16, 130, 300};
    const int64_t ns[] = {1, 300, 8192, 8193, 20003, 60001, 1000000, 10000000};
    const int ks[] = {1, 100, 128, 129, 2049, 9000};
    for (int variant = 0; variant < 4; ++variant) for (int d : ds) for (int64_t n : ns) for (int nq : nqs) for (int k : ks)
    for (int metric = HDB_DOT; metric <= HDB_PEARSON; ++metric) for (int aux = 0; aux < 4; ++aux) for (int fin = 0; fin < 2; ++fin) for (int exact = 0; exact < 2; ++exact) {
        hdb_options o;
        if (variant == 1) o.quant_min_n = 0;                                   // "a shadow for every size": still none
        if (variant == 2) { o.subset_min_n = 0; }                              // the row list wherever the ratio admits it
        if (variant == 3) { o.use_mfma = 0; o.use_fused = 0; o.use_l1_tile = 0; }
        TopkFacts f{};
        f.n = n; f.d = d; f.dtype = HDB_F8E4M3; f.cus = 256; f.qmode = HDB_QUANT_NONE; f.has_bias = (aux & 1) != 0; f.has_mask = (aux & 2) != 0;
        if (variant == 2 && f.has_mask) f.subset_m = n / 3 > 1000 ? 1000 : n / 3;
        const TopkCall c{nq, k, metric, true, exact != 0};
        int asked = 0;
        const TopkPlan p = plan_topk(f, o, c, [&] { ++asked; return fin != 0; });
        ++plans;
#define WHERE "variant %d d %d n %lld nq %d k %d metric %d aux %d finite %d exact %d", variant, d, (long long)n, nq, k, metric, aux, fin, exact
        CHECK(!p.shadow() && !p.build_needed && !p.plane_wanted && p.stats.quant == 0 && p.stats.plane == 0, WHERE);
        CHECK(p.path != HDB_PATH_FUSED && p.path != HDB_PATH_BATCH1 && !p.local && p.stats.local == (p.path == HDB_PATH_BITS1 ? p.stats.local : 0), WHERE);
        CHECK(p.path != HDB_PATH_BITS1 || (is_bits_metric(metric) && nq <= 4 && o.use_fused), WHERE);
        CHECK(p.stats.fused == (p.path == HDB_PATH_BITS1 ? 3 : 0), WHERE);
        const bool wd = d == 128 || d == 256 || d == 384 || d == 512;
        const bool mm = metric == HDB_DOT || metric == HDB_COSINE || metric == HDB_EUCLIDEAN || metric == HDB_PEARSON;
        // what decides but the finiteness: the batch, the metric, the width, more rows than the candidate list, the switch -- and no row list taken
        const bool eligible = o.use_mfma && mm && nq >= 5 && wd && n > HDB_CAND_CAP && !p.subset;
        const bool want = eligible && fin;
        const bool sorted = p.path == HDB_PATH_FULL_SORT;
        CHECK(p.mfma == want && p.stats.mfma == (want && !sorted ? 1 : 0), WHERE);
        CHECK(asked == (eligible ? 1 : 0), WHERE);                             // the question is asked exactly where it decides
        CHECK(!p.l1tile && !p.ksplit && !p.f32s && !p.f16_queries && !p.q16_in_prep && p.ld_ks == 0, WHERE);
        CHECK(p.tile_rows == (want ? hdb_mfma_tile_rows(HDB_F8E4M3, d) : 16) && p.tile_rows == 16, WHERE);
        CHECK(p.path == HDB_PATH_PIPELINE || sorted || p.path == HDB_PATH_BITS1, WHERE);
        CHECK(p.cq_max >= 1 && p.cq_max <= std::min(nq, 256), WHERE);
        CHECK(p.mask_fold == (want && f.has_mask && !sorted), WHERE);
        const int64_t rows = p.subset ? f.subset_m : n;                        // a list call plans a matrix of the listed rows
        CHECK(p.small == (rows <= HDB_CAND_CAP) && sorted == (k > HDB_MAX_K && rows > HDB_CAND_CAP), WHERE);
        if (!p.small && !p.exact && !sorted) CHECK(p.s_rows == p.s_tiles * p.tile_rows && p.s_tiles > 0 && p.s_tiles * p.s_stride * p.tile_rows <= rows, WHERE);
        if (variant == 2 && p.subset) CHECK(f.subset_m > 0 && subset_metric(metric) && p.stats.subset == 1 && p.path == HDB_PATH_PIPELINE, WHERE);
        // the same plan as a bfloat16 matrix of this shape whose matrix cores are switched off: always but for the matrix-core flags
        TopkFacts fb = f; fb.dtype = HDB_BF16;
        hdb_options ob = o; ob.use_mfma = 0;
        TopkPlan b = plan_topk(fb, ob, c, [&] { return fin != 0; });
        if (want) { b.mfma = true; b.stats.mfma = sorted ? 0 : 1; b.mask_fold = f.has_mask && !sorted; }      // (16-row tiles either way: same sample, same chunks)
        CHECK_SAME_PLAN(p, b, WHERE);
    }
    // an index that claims a shadow it cannot have (the library refuses hdb_index_quantize for the dtype) still plans none
    for (int nq : {1, 4, 16}) {
        TopkFacts f{};
        f.n = 5000000; f.d = 384; f.dtype = HDB_F8E4M3; f.cus = 256; f.qmode = HDB_QUANT_I8; f.qauto = nq > 1; f.plane_present = true;
        hdb_options o; o.quant_min_n = 0;
        const TopkPlan p = plan_topk(f, o, TopkCall{nq, 100, HDB_COSINE, true, false}, [] { return true; });
        ++plans;
        CHECK(!p.shadow() && p.stats.quant == 0 && p.path == HDB_PATH_PIPELINE && p.mfma == (nq >= 5), "qmode set, %d queries", nq);
    }
    std::printf("plans %ld\n", plans);
    return check_done();
}
