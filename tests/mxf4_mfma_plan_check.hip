// mxf4_mfma_plan_check.hip -- the plans of an MXFP4 matrix (HDB_MXF4) under the opt-in b1_mfma_min_q: a stand-alone host program, no GPU call.
// d = 32 .. 1024 in steps of 32, every metric, n in {300, 8192, 8389, 10M}, nq in {1, 4, 5, 16, 64}, with and without bias and mask,
// a finite matrix and one that is not.  With the option at 5 and 16 the plan takes the matrix cores exactly for whole rows of 128 /
// 256 / 384 / 512 elements, dot / cosine / euclidean / pearson, at least that many queries, more than HDB_CAND_CAP rows and a finite
// matrix -- 16-row tiles, the multi-kernel pipeline, no K slices, LDS flavour, parts of float32 rows, shadow, row list or local launch;
// everywhere else, and with the option at 0 or -1, the plan equals the plan under default options member for member.
// Prints "plans N", "mfma plans M" and "F failures"; exit status 1 on any failure.
#include "plan_check.h"

int main() {
    for (int d = 1; d <= 8192; ++d) {
        CHECK(hdb_mfma_f4_tile_rows(d) == (whole_width(d) ? 16 : 0) && hdb_mfma_f4_min_q(d) == 0, "d %d", d);
        CHECK(hdb_mfma_tile_rows(HDB_MXF4, d) == 0 && hdb_mfma_ksplit_slices(HDB_MXF4, d) == 0 && hdb_mfma_batch_capacity(HDB_MXF4, d) == 0, "d %d", d);
        for (int metric = HDB_DOT; metric <= HDB_PEARSON; ++metric) CHECK(!hdb_mfma_supported(HDB_MXF4, d, metric), "d %d metric %d", d, metric);
    }
    long plans = 0, on = 0;
    const int nqs[] = {1, 4, 5, 16, 64};
    const int64_t ns[] = {300, 8192, 8389, 10000000};
    const int vs[] = {0, -1, 5, 16};
    for (int v : vs) for (int d = 32; d <= 1024; d += 32) for (int metric = HDB_DOT; metric <= HDB_PEARSON; ++metric) for (int64_t n : ns)
    for (int nq : nqs) for (int aux = 0; aux < 4; ++aux) for (int fin = 0; fin < 2; ++fin) {
        hdb_options o;
        o.b1_mfma_min_q = v;
        TopkFacts f{};
        f.n = n; f.d = d; f.dtype = HDB_MXF4; f.cus = 256; f.qmode = HDB_QUANT_NONE; f.has_bias = (aux & 1) != 0; f.has_mask = (aux & 2) != 0;
        const TopkCall c{nq, 10, metric, true, false};
        const TopkPlan p = plan_topk(f, o, c, [&] { return fin != 0; });
        const TopkPlan today = plan_topk(f, hdb_options{}, c, [&] { return fin != 0; });
        ++plans;
#define WHERE "option %d d %d n %lld nq %d metric %d aux %d finite %d", v, d, (long long)n, nq, metric, aux, fin
        const int64_t T = (v > 0 && whole_width(d)) ? std::max<int64_t>(v, 5) : 0;
        CHECK(b1_mfma_first_q(o, HDB_MXF4, d) == T, WHERE);
        const bool mm = metric == HDB_DOT || metric == HDB_COSINE || metric == HDB_EUCLIDEAN || metric == HDB_PEARSON;
        const bool want = T > 0 && mm && nq >= T && n > HDB_CAND_CAP && fin != 0;
        CHECK(p.mfma == want, WHERE);
        if (!want) { CHECK_SAME_PLAN(p, today, WHERE); continue; }
        ++on;
        CHECK(p.tile_rows == 16 && p.path == HDB_PATH_PIPELINE && p.stats.mfma == 1 && p.stats.fused == 0 && p.mask_fold == f.has_mask && !p.f16_queries, WHERE);
        CHECK(!p.ksplit && p.ld_ks == 0 && !p.f8_lds && !p.f32s && !p.shadow() && !p.subset && !p.local && !p.l1tile && !p.plane_wanted && !p.build_needed, WHERE);
    }
    CHECK(on > 500, "the grid reaches the matrix cores (%ld plans)", on);
    std::printf("plans %ld\nmfma plans %ld\n", plans, on);
    return check_done();
}
