// subset_plan_check.hip -- the row-list rule of plan_topk (csrc/hdb_plan.h) on the host: a stand-alone program, no GPU call.
//
// usage: subset_plan_check tests/golden/dispatch_table.jsonl
// Over dtype x d x n x m x nq x k x metric x exact:
//   taken     -- a plan with `subset` is the multi-kernel pipeline, mfma = fused = quant = 0, and every extent and statistic equals
//                plan_topk of the m-row facts with use_mfma = use_fused = use_quant = use_l1_tile = 0;
//   never     -- hamming / jaccard, use_subset = 0, subset_m = 0, a violated ratio rule, n < subset_min_n, or an inner plan that
//                is a full sort: the plan is the masked call's, field by field;
//   unchanged -- every row of the recorded dispatch table: facts without a list give the recorded statistics, and the same
//                plan as facts that carry a list with use_subset = 0.
// Prints "rows N", "grid plans P", "taken T" and " F failures"; exit status 1 on any failure.
#include "plan_check.h"
#include <fstream>

static_assert(HDB_SUBSET_MIN_ROWS >= 32768, "the measured rule of subset_min_n never goes below 32 768 rows");
static_assert(HDB_SUBSET_RATIO >= 1, "subset_ratio is an integer >= 1");

static bool listed_metric(int metric) {
    return metric == HDB_DOT || metric == HDB_COSINE || metric == HDB_EUCLIDEAN || metric == HDB_MANHATTAN || metric == HDB_PEARSON;
}
static auto fin = [] { return true; };
// "equal except the list": the two plans are compared with `subset` and stats.subset reset on both sides
static TopkPlan no_list(TopkPlan p) { p.subset = false; p.stats.subset = 0; return p; }

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: subset_plan_check TABLE.jsonl\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::printf("cannot open %s\n", argv[1]); return 2; }

    // ---- unchanged: the recorded dispatch table ----
    std::string line, stat_names;
    long rows = 0, lines = 0;
    int cus = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        ++lines;
        Row r;
        if (!parse_row(line, r)) { CHECK(false, "line %ld does not parse", lines); continue; }
        if (r.str.count("header")) { cus = (int)r.num["cus"]; stat_names = r.str["stats"]; continue; }
        ++rows;
        TopkFacts f; TopkCall c; hdb_options o;
        row_inputs(r, cus, lines, f, c, o);
        const bool finite_m = r.num["nonfinite"] == 0;
        const TopkPlan p = plan_topk(f, o, c, [&] { return finite_m; });
        CHECK(!p.subset && p.stats.subset == 0, "line %ld: a plan without a list says subset", lines);
        check_row_stats(r, stat_names, p, -1, lines);          // (quant_auto is the index's: not compared here)
        // ... and the same plan from facts that carry a list the options switch off, or a list of no rows
        TopkFacts fl = f; fl.subset_m = std::max<int64_t>(1, f.n / 64); fl.has_mask = true;
        TopkFacts fm = f; fm.has_mask = true;
        hdb_options off = o; off.use_subset = 0; off.subset_min_n = 0; off.subset_ratio = 1;
        const TopkPlan pm = plan_topk(fm, o, c, [&] { return finite_m; });
        const TopkPlan pl = plan_topk(fl, off, c, [&] { return finite_m; });
        CHECK(!pl.subset && pl.stats.subset == 0, "line %ld: use_subset = 0 takes the list", lines);
        CHECK_SAME_PLAN(pl, pm, "line %ld: use_subset = 0 changes the plan", lines);
    }

    // ---- the grid ----
    const int ds[] = {40, 96, 100, 384, 768}, nqs[] = {1, 4, 6, 64}, ks[] = {10, 128, 3000};
    const int64_t ns[] = {20000, 60000, 3000000};
    long plans = 0, taken = 0, taken_default = 0;
    for (int dtype = HDB_F16; dtype <= HDB_BF16; ++dtype) for (int d : ds) for (int64_t n : ns) {
        const int64_t ms[] = {5, 1000, 8192, 8193, 20001, n / 2};
        for (int64_t m : ms) for (int nq : nqs) for (int k : ks) for (int metric = HDB_DOT; metric <= HDB_PEARSON; ++metric) for (int exact = 0; exact < 2; ++exact) {
#define WHERE "dtype %d d %d n %lld m %lld nq %d k %d metric %d exact %d", dtype, d, (long long)n, (long long)m, nq, k, metric, exact
            const TopkCall c{nq, k, metric, true, exact != 0};
            TopkFacts f{};
            f.n = n; f.d = d; f.dtype = dtype; f.cus = 256; f.has_mask = true; f.has_bias = (k == 128); f.subset_m = m;
            TopkFacts fmask = f; fmask.subset_m = 0;                                 // the masked call of the same handle
            TopkFacts fin_m{}; fin_m.n = m; fin_m.d = d; fin_m.dtype = dtype; fin_m.cus = 256; fin_m.has_bias = f.has_bias;      // the same call on m rows
            hdb_options on; on.subset_min_n = 0; on.subset_ratio = 1;
            hdb_options in_o = on; in_o.use_mfma = 0; in_o.use_fused = 0; in_o.use_quant = 0; in_o.use_l1_tile = 0;
            const TopkPlan inner = plan_topk(fin_m, in_o, c, fin);
            const TopkPlan masked = plan_topk(fmask, on, c, fin);
            const int64_t groups = (nq + 3) / 4;
            CHECK(!masked.subset && masked.stats.subset == 0, WHERE);
            for (int64_t ratio : {(int64_t)1, (int64_t)2, (int64_t)8}) {
                hdb_options o = on; o.subset_ratio = ratio;
                const bool want = listed_metric(metric) && m * groups * ratio <= n && inner.path == HDB_PATH_PIPELINE;
                const TopkPlan p = plan_topk(f, o, c, fin);
                ++plans;
                CHECK(p.subset == want, WHERE);
                if (p.subset) {
                    ++taken;
                    CHECK(p.path == HDB_PATH_PIPELINE && p.stats.mfma == 0 && p.stats.fused == 0 && p.stats.quant == 0 && p.stats.subset == 1, WHERE);
                    CHECK(p.stats.path >= 0 && p.stats.path <= 2 && !p.mfma && !p.mask_fold && !p.l1tile && !p.ksplit && p.tile_rows == 16, WHERE);
                    CHECK_SAME_PLAN(no_list(p), no_list(inner), WHERE);
                    CHECK(p.kk == (uint32_t)std::min<int64_t>(k, m) && p.ld_n >= m && p.small == (m <= HDB_CAND_CAP), WHERE);
                    CHECK(!(k > HDB_MAX_K && m > HDB_CAND_CAP), WHERE);
                    if (!p.small && !p.exact) CHECK(p.s_tiles * 16 * p.s_stride <= m, WHERE);      // the sample's last list tile exists
                } else {
                    CHECK_SAME_PLAN(p, masked, WHERE);
                }
            }
            // never: the bit metrics, a full sort inside, the switches
            if (is_bits_metric(metric) || inner.path == HDB_PATH_FULL_SORT) CHECK(!plan_topk(f, on, c, fin).subset, WHERE);
            if (k > HDB_MAX_K && m > HDB_CAND_CAP) CHECK(inner.path == HDB_PATH_FULL_SORT, WHERE);
            hdb_options off = on; off.use_subset = 0;
            const TopkPlan p_off = plan_topk(f, off, c, fin);
            CHECK_SAME_PLAN(p_off, masked, WHERE);
            hdb_options big = on; big.subset_min_n = n + 1;
            const TopkPlan p_big = plan_topk(f, big, c, fin);
            CHECK_SAME_PLAN(p_big, masked, WHERE);
            hdb_options at = on; at.subset_min_n = n;                                       // n >= subset_min_n is inclusive
            CHECK(plan_topk(f, at, c, fin).subset == plan_topk(f, on, c, fin).subset, WHERE);
            // the measured rule (-1 / -1): never below HDB_SUBSET_MIN_ROWS rows, HDB_SUBSET_RATIO in the inequality
            const hdb_options dflt;
            const bool want_d = listed_metric(metric) && n >= HDB_SUBSET_MIN_ROWS && m * groups * HDB_SUBSET_RATIO <= n && inner.path == HDB_PATH_PIPELINE;
            const TopkPlan p_d = plan_topk(f, dflt, c, fin);
            CHECK(p_d.subset == want_d, WHERE);
            if (n < 32768) CHECK(!p_d.subset, WHERE);
            hdb_options in_d = dflt; in_d.use_mfma = 0; in_d.use_fused = 0; in_d.use_quant = 0; in_d.use_l1_tile = 0;
            if (p_d.subset) { ++taken_default; CHECK_SAME_PLAN(no_list(p_d), no_list(plan_topk(fin_m, in_d, c, fin)), WHERE); }
            else CHECK_SAME_PLAN(p_d, plan_topk(fmask, dflt, c, fin), WHERE);
            plans += 4;
        }
    }
    CHECK(taken > 1000 && taken_default > 100, "the grid takes the list in %ld / %ld plans", taken, taken_default);
    std::printf("rows %ld\ngrid plans %ld\ntaken %ld (default rule %ld)\n", rows, plans, taken, taken_default);
    return check_done();
}
