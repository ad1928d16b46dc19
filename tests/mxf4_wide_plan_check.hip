// mxf4_wide_plan_check.hip -- the plans of an MXFP4 matrix (HDB_MXF4) wider than 512 elements under b1_mfma_min_q and f8_ks_min_q
// together (csrc/hdb_plan.h, hdb_mfma_f4_wide_geom in csrc/hdb_caps.h): a stand-alone host program, no GPU call.
// At a width with a wide geometry the threshold is max(5, b1_mfma_min_q, f8_ks_min_q or the width's rule) when b1_mfma_min_q >= 1
// and f8_ks_min_q != 0, and the plan takes the matrix cores for that many dot / cosine / euclidean / pearson queries on a finite
// matrix of more than HDB_CAND_CAP rows: 16-row tiles, the multi-kernel pipeline, NO K slices and no partial-sum workspace.  The
// whole rows of 128 .. 512 elements keep b1_mfma_min_q's own rule; everywhere else the plan equals the default-options plan.
// Prints "plans N", "wide plans M" and "F failures"; exit status 1 on any failure.
#include "plan_check.h"

int main() {
    for (int d = 1; d <= 8192; ++d) {
        const HdbF4WideGeom g = hdb_mfma_f4_wide_geom(d);
        if (g.w || g.s) CHECK(g.s * g.w == d && g.s >= 2 && g.s <= 8 && g.w % 128 == 0 && g.w >= 128 && g.w <= 512 && d >= 640 && d <= 4096, "d %d = %d x %d", d, g.s, g.w);
        if (d <= 512 || d == 1408 || d % 128 != 0 || d > 4096) CHECK(g.w == 0 && g.s == 0, "d %d has a geometry", d);
        CHECK(hdb_mfma_f4_wide_min_q(d) >= 5, "d %d", d);
    }
    const int required[][3] = {{768, 256, 3}, {1024, 256, 4}, {1152, 384, 3}, {1280, 256, 5}, {1536, 384, 4}, {2048, 512, 4}, {3072, 384, 8}};
    for (const auto& r : required) CHECK(hdb_mfma_f4_wide_geom(r[0]).w == r[1] && hdb_mfma_f4_wide_geom(r[0]).s == r[2], "d %d", r[0]);
    long plans = 0, on = 0;
    const int nqs[] = {1, 4, 5, 16, 64};
    const int64_t ns[] = {300, 8192, 8389, 10000000};
    const int opts[][2] = {{5, 0}, {0, 5}, {-1, -1}, {5, -1}, {5, 16}, {16, 5}};
    for (const auto& v : opts) for (int d = 32; d <= 4224; d += 32) for (int metric = HDB_DOT; metric <= HDB_PEARSON; ++metric) for (int64_t n : ns)
    for (int nq : nqs) for (int mask = 0; mask < 2; ++mask) for (int fin = 0; fin < 2; ++fin) {
        hdb_options o;
        o.b1_mfma_min_q = v[0]; o.f8_ks_min_q = v[1];
        TopkFacts f{};
        f.n = n; f.d = d; f.dtype = HDB_MXF4; f.cus = 256; f.qmode = HDB_QUANT_NONE; f.has_mask = mask != 0;
        const TopkCall c{nq, 10, metric, true, false};
        const TopkPlan p = plan_topk(f, o, c, [&] { return fin != 0; });
        const TopkPlan today = plan_topk(f, hdb_options{}, c, [&] { return fin != 0; });
        ++plans;
#define WHERE "options %d %d d %d n %lld nq %d metric %d mask %d finite %d", v[0], v[1], d, (long long)n, nq, metric, mask, fin
        const bool wide = hdb_mfma_f4_wide_geom(d).s > 0;
        int64_t T = 0;
        if (wide && v[0] >= 1 && v[1] != 0) T = std::max<int64_t>(std::max<int64_t>(5, v[0]), v[1] > 0 ? v[1] : hdb_mfma_f4_wide_min_q(d));
        if (whole_width(d) && v[0] >= 1) T = std::max<int64_t>(5, v[0]);
        CHECK(b1_mfma_first_q(o, HDB_MXF4, d) == T, WHERE);
        const bool mm = metric == HDB_DOT || metric == HDB_COSINE || metric == HDB_EUCLIDEAN || metric == HDB_PEARSON;
        const bool want = T > 0 && mm && nq >= T && n > HDB_CAND_CAP && fin != 0;
        CHECK(p.mfma == want, WHERE);
        if (!want) { CHECK_SAME_PLAN(p, today, WHERE); continue; }
        if (wide) ++on;
        CHECK(p.tile_rows == 16 && p.path == HDB_PATH_PIPELINE && p.stats.mfma == 1 && p.stats.fused == 0 && p.mask_fold == f.has_mask && !p.f16_queries, WHERE);
        CHECK(!p.ksplit && p.ld_ks == 0 && !p.f8_lds && !p.f32s && !p.shadow() && !p.subset && !p.local && !p.l1tile && !p.plane_wanted && !p.build_needed, WHERE);
    }
    std::printf("plans %ld\nwide plans %ld\n", plans, on);
    return check_done();
}
