// topk_plan_check.hip -- plan_topk (csrc/hdb_plan.h) on the host: a stand-alone program, no GPU call.
//
// usage: topk_plan_check tests/golden/dispatch_table.jsonl
// 1) every row of the recorded dispatch table: the plan's statistics equal the row's, field by field; a statistic the row leaves
//    out (the parent left it stale on that path) is zero in the plan;
// 2) properties of the plan, for every row and over a synthetic grid (see check_props).
// Prints "rows N" and "failures F"; exit status 1 on any failure.
#include "plan_check.h"
#include <cstring>
#include <fstream>

// The properties every plan has.  `fin`: what the finiteness callable answers.  -> the plan, for the caller's own checks.
static TopkPlan check_props(const TopkFacts& f, const hdb_options& o, const TopkCall& c, bool fin, const char* tag) {
    int asked = 0;
    auto finite = [&] { ++asked; return fin; };
    const TopkPlan p = plan_topk(f, o, c, finite);
#define WHERE "%s dtype %d d %d n %lld nq %d k %d metric %d status %d exact %d qmode %d", tag, f.dtype, f.d, (long long)f.n, c.nq, c.k, c.metric, (int)c.has_status, (int)c.exact, f.qmode
    CHECK(p.cq_max >= 1 && p.cq_max <= std::min(c.nq, 256), WHERE);
    if (p.single_launch()) CHECK(c.has_status && c.k <= 128, WHERE);
    if (p.path == HDB_PATH_BATCH1 || p.path == HDB_PATH_FUSED) CHECK(p.cq_max <= hdb_mfma_batch_capacity(f.dtype, f.d), WHERE);
    if (p.path == HDB_PATH_BITS1) CHECK(p.stats.chunks == (c.nq + 3) / 4, WHERE);
    if (f.n > 0 && !p.shadow()) {
        // the TopkWs extents: the layout's size against the same sum in floating point (a wrapped product would be far off)
        const size_t bytes = ws_bytes_for<TopkWs>((int)c.nq, (int)f.d, p.W, p.cq_max, p.ld_scores, p.ld_ks, p.sort_n, (size_t)0);
        const long double nq = c.nq, d = f.d, cq = p.cq_max;
        const long double want = 16.0L * nq + 4.0L * nq * p.W + 10.0L * nq * d + cq * (4.0L + 4 * HDB_CNT_STRIDE + 16.0L * HDB_RADIX_BINS + 16 + 8.0L * HDB_CAND_CAP) + 256 +
                                 4.0L * cq * (long double)p.ld_scores + 4.0L * cq * (long double)p.ld_ks + 20.0L * (long double)p.sort_n;
        CHECK(p.ld_scores >= 4 && p.ld_ks >= 0 && p.sort_n >= 0, WHERE);
        CHECK((long double)bytes >= want && (long double)bytes <= want + 256.0L * 24 && bytes < ((size_t)1 << 46), WHERE);
        CHECK(p.exact && !p.small ? p.ld_scores >= f.n : p.ld_scores >= p.s_rows, WHERE);
        CHECK(p.s_tiles * p.tile_rows * p.s_stride <= std::max<int64_t>(f.n, p.tile_rows), WHERE);      // the sample's last tile exists
    }
    // the finiteness question: once on a shadow path (the answer was yes), at most once at all (the plan keeps the answer for the
    // rules that read it later: an explicit shadow that declined, a padded width, the bf16 parts), never where no rule reads it
    CHECK(asked <= 1, WHERE);
    if (p.shadow()) CHECK(asked == 1 && fin, WHERE);
    if (f.dtype == HDB_F64 || is_bits_metric(c.metric) || f.n <= HDB_CAND_CAP) CHECK(asked == 0, WHERE);
    if (p.shadow()) CHECK(p.build_needed == (f.qmode != HDB_QUANT_I8), WHERE);
    // a declined build is final: the second plan names a path that needs none
    TopkFacts f2 = f; f2.qauto_declined = true;
    const TopkPlan p2 = plan_topk(f2, o, c, [&] { return fin; });
    CHECK(!(p2.shadow() && p2.build_needed), WHERE);
    if (p.shadow() && p.build_needed) CHECK(!p2.shadow(), WHERE);
    return p;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: topk_plan_check TABLE.jsonl\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::printf("cannot open %s\n", argv[1]); return 2; }
    std::string line, stat_names;
    long rows = 0, lines = 0;
    int cus = 0;
    std::map<int, long> paths;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        ++lines;
        Row r;
        if (!parse_row(line, r)) { CHECK(false, "line %ld does not parse", lines); continue; }
        if (r.str.count("header")) { CHECK(lines == 1, "header on line %ld", lines); cus = (int)r.num["cus"]; stat_names = r.str["stats"]; continue; }
        ++rows;
        TopkFacts f; TopkCall c; hdb_options o;
        row_inputs(r, cus, lines, f, c, o);
        char tag[32]; std::snprintf(tag, sizeof(tag), "line %ld", lines);
        const TopkPlan p = check_props(f, o, c, r.num["nonfinite"] == 0, tag);
        paths[(int)p.path]++;
        // "stats": in the header's order; "-" = the parent left the statistic stale on this path: the plan's value is its zero
        const long long qa = (f.qmode == HDB_QUANT_I8 && f.qauto) || (p.shadow() && p.build_needed) ? 1 : 0;
        check_row_stats(r, stat_names, p, qa, lines);
    }
    for (int pth = HDB_PATH_EMPTY; pth <= HDB_PATH_PIPELINE; ++pth) CHECK(paths[pth] >= 3, "path %d occurs in %ld rows of the table", pth, paths[pth]);

    // ---- the synthetic grid: default options, the three shadow states ----
    const int nqs[] = {1, 2, 4, 5, 24, 129, 256, 300}, ds[] = {1, 40, 128, 384, 512, 768, 1024, 2048}, ks[] = {1, 128, 129, 2049};
    const int64_t ns[] = {0, 1, 8192, 8193, 70001, 2000000, 10000000};
    long plans = 0;
    for (int dtype = HDB_F16; dtype <= HDB_BF16; ++dtype) for (int d : ds) for (int64_t n : ns) for (int shadow = 0; shadow < 3; ++shadow) {
        if (shadow && (dtype == HDB_F64 || dtype == HDB_BF16)) continue;          // (no shadow exists for these)
        TopkFacts f{};
        f.n = n; f.d = d; f.dtype = dtype; f.cus = 256;
        f.qmode = shadow ? HDB_QUANT_I8 : HDB_QUANT_NONE; f.qauto = shadow == 2; f.plane_present = shadow == 2 && d <= 512;
        const hdb_options o;
        for (int nq : nqs) for (int k : ks) for (int metric = HDB_DOT; metric <= HDB_PEARSON; ++metric)
            for (int status = 0; status < 2; ++status) for (int exact = 0; exact < 2; ++exact) for (int fin = 0; fin < 2; ++fin) {
                check_props(f, o, TopkCall{nq, k, metric, status != 0, exact != 0}, fin != 0, "grid");
                ++plans;
            }
    }

    // ---- the rules that keep the score contract on low-score rows and at the infinities ----
    // (1) float32 batches: dot_product never multiplies as bf16 parts -- its plan is the plan of the same call with f32_split = 0,
    //     statistic by statistic, exact selection included; cosine, euclidean and pearson keep the parts wherever the width has them,
    //     on a finite matrix
    long rules = 0;
    {
        const int fds[] = {100, 128, 256, 300, 384, 512, 768, 1024, 1536}, fnq[] = {5, 8, 9, 16, 40, 64, 65, 128, 256};
        const int64_t fns[] = {20005, 70001, 2000000};
        for (int d : fds) for (int64_t n : fns) for (int nq : fnq) for (int k : {50, 2048}) {
            TopkFacts f{};
            f.n = n; f.d = d; f.dtype = HDB_F32; f.cus = 256;
            hdb_options o, o0; o0.f32_split = 0;
            auto yes = [] { return true; };
            const TopkPlan dot = plan_topk(f, o, TopkCall{nq, k, HDB_DOT, true, false}, yes);
            const TopkPlan dot0 = plan_topk(f, o0, TopkCall{nq, k, HDB_DOT, true, false}, yes);
#define WHERE2 "f32 d %d n %lld nq %d k %d", d, (long long)n, nq, k
            CHECK(!dot.f32s && dot.stats.f32s == 0 && dot.mfma && dot.stats.mfma == 1, WHERE2);
            CHECK(!plan_topk(f, o, TopkCall{nq, k, HDB_DOT, true, true}, yes).f32s, WHERE2);
            CHECK(dot.path == dot0.path && dot.cq_max == dot0.cq_max && dot.tile_rows == dot0.tile_rows && dot.stats.fused == dot0.stats.fused &&
                  dot.stats.chunks == dot0.stats.chunks && dot.stats.sample_rows == dot0.stats.sample_rows && dot.stats.path == dot0.stats.path, WHERE2);
            const int smin = hdb_mfma_f32_split_min_q(d);
            const bool parts = smin > 0 && nq >= smin && nq <= hdb_mfma_f32_split_max_q(d);
            for (int metric : {(int)HDB_COSINE, (int)HDB_EUCLIDEAN, (int)HDB_PEARSON}) {
                const TopkPlan p = plan_topk(f, o, TopkCall{nq, k, metric, true, false}, yes);
                CHECK(p.mfma && p.f32s == parts && p.stats.f32s == (parts ? 1 : 0), WHERE2);
                CHECK(!plan_topk(f, o, TopkCall{nq, k, metric, true, false}, [] { return false; }).f32s, WHERE2);
                // a call that asks for the exact selection keeps the parts (and the default call's bits) and says that it asked: the
                // executor drops them when a query holds an infinity
                const TopkPlan e = plan_topk(f, o, TopkCall{nq, k, metric, true, true}, yes);
                CHECK(e.exact && e.exact_req && !p.exact_req && e.f32s == parts && e.stats.path == 2 && e.path == HDB_PATH_PIPELINE, WHERE2);
                ++rules;
            }
        }
        // the shapes of tests/test_low_score_contract.py by name: parts for cosine, float32 for dot_product
        const int sd[] = {384, 384, 300, 768, 1024}, sq[] = {16, 64, 16, 8, 16};
        for (int i = 0; i < 5; ++i) {
            TopkFacts f{};
            f.n = 20005; f.d = sd[i]; f.dtype = HDB_F32; f.cus = 256;
            const hdb_options o;
            CHECK(plan_topk(f, o, TopkCall{sq[i], 50, HDB_COSINE, true, false}, [] { return true; }).f32s, "cosine d %d nq %d", sd[i], sq[i]);
            CHECK(!plan_topk(f, o, TopkCall{sq[i], 50, HDB_DOT, true, false}, [] { return true; }).f32s, "dot d %d nq %d", sd[i], sq[i]);
        }
    }
    // (2) padded widths (fp16 / float32 rows that ride the next wider geometry): the matrix cores on a finite matrix only, and the
    //     question is asked once whatever reads the answer afterwards
    {
        const struct { int dtype, d; } pw[] = {{HDB_F16, 96}, {HDB_F16, 200}, {HDB_F16, 1000}, {HDB_F32, 100}, {HDB_F32, 300}, {HDB_F32, 700}};
        for (const auto& w : pw) for (int nq : {6, 40, 128}) for (int metric : {(int)HDB_DOT, (int)HDB_COSINE, (int)HDB_EUCLIDEAN, (int)HDB_PEARSON}) {
            TopkFacts f{};
            f.n = 20005; f.d = w.d; f.dtype = w.dtype; f.cus = 256;
            const hdb_options o;
            CHECK(hdb_mfma_anyd_pad(w.dtype, w.d) > 0, "dtype %d d %d is a padded width", w.dtype, w.d);
            for (int fin = 0; fin < 2; ++fin) {
                int asked = 0;
                const TopkPlan p = plan_topk(f, o, TopkCall{nq, 50, metric, true, false}, [&] { ++asked; return fin != 0; });
                CHECK(asked == 1 && p.mfma == (fin != 0) && p.stats.mfma == fin && !(p.f32s && !fin) && p.path == HDB_PATH_PIPELINE,
                      "padded dtype %d d %d nq %d metric %d finite %d: asked %d mfma %d", w.dtype, w.d, nq, metric, fin, asked, (int)p.mfma);
                ++rules;
            }
        }
        // widths with a geometry of their own do not ask on fp16, and fp16 d = 100 (no multiple of 16 bytes) has no matrix cores at all
        for (int d : {128, 384, 100}) {
            TopkFacts f{};
            f.n = 20005; f.d = d; f.dtype = HDB_F16; f.cus = 256;
            int asked = 0;
            const TopkPlan p = plan_topk(f, hdb_options(), TopkCall{6, 50, HDB_DOT, true, false}, [&] { ++asked; return false; });
            CHECK(asked == 0 && p.mfma == (d != 100), "fp16 d %d: asked %d mfma %d", d, asked, (int)p.mfma);
        }
    }
    // (3) the packed-fp16 manhattan flavour: fp16 rows, the option on, the flag word fetched and without the "wide element" bit
    CHECK(hdb_l1_packed_ok(HDB_F16, 1, 0) && hdb_l1_packed_ok(HDB_F16, 1, HDB_FLAG_NAN) && hdb_l1_packed_ok(HDB_F16, 1, HDB_FLAG_INF), "packed: allowed");
    CHECK(!hdb_l1_packed_ok(HDB_F16, 1, HDB_FLAG_L1_WIDE) && !hdb_l1_packed_ok(HDB_F16, 1, HDB_FLAG_INF | HDB_FLAG_L1_WIDE) && !hdb_l1_packed_ok(HDB_F16, 1, -1) &&
          !hdb_l1_packed_ok(HDB_F16, 0, 0) && !hdb_l1_packed_ok(HDB_F32, 1, 0) && !hdb_l1_packed_ok(HDB_BF16, 1, 0), "packed: refused");
    CHECK(2.0f * HDB_L1_PK_MAX <= 65504.0f && (float)(_Float16)HDB_L1_PK_MAX == HDB_L1_PK_MAX, "HDB_L1_PK_MAX is an fp16 number of at most half the range");
    std::printf("rule plans %ld\n", rules);
    std::printf("rows %ld\ngrid plans %ld\n", rows, plans);
    return check_done();
}
