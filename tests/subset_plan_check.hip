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
#include "hdb_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <string>

static long g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 40) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static_assert(HDB_SUBSET_MIN_ROWS >= 32768, "the measured rule of subset_min_n never goes below 32 768 rows");
static_assert(HDB_SUBSET_RATIO >= 1, "subset_ratio is an integer >= 1");

static bool same_stats(const TopkStats& a, const TopkStats& b) {
    return a.sample_rows == b.sample_rows && a.sample_m == b.sample_m && a.path == b.path && a.chunks == b.chunks && a.mfma == b.mfma &&
           a.fused == b.fused && a.local == b.local && a.f32s == b.f32s && a.quant == b.quant && a.plane == b.plane;
}
// every member of the plan but `subset` and stats.subset
static bool same_plan(const TopkPlan& a, const TopkPlan& b) {
    return a.path == b.path && a.kk == b.kk && a.W == b.W && a.bits == b.bits && a.pearson == b.pearson && a.exact == b.exact &&
           a.small == b.small && a.mfma == b.mfma && a.f32s == b.f32s && a.ksplit == b.ksplit && a.l1tile == b.l1tile && a.local == b.local &&
           a.prep == b.prep && a.fold_small == b.fold_small && a.q16_in_prep == b.q16_in_prep && a.f16_queries == b.f16_queries &&
           a.mask_fold == b.mask_fold && a.tile_rows == b.tile_rows && a.s_tiles == b.s_tiles && a.s_stride == b.s_stride &&
           a.s_rows == b.s_rows && a.ld_s == b.ld_s && a.ld_n == b.ld_n && a.m == b.m && a.cq_max == b.cq_max &&
           a.ld_scores == b.ld_scores && a.ld_ks == b.ld_ks && a.sort_n == b.sort_n && a.local_slot == b.local_slot &&
           a.local_m == b.local_m && a.bits_local == b.bits_local && a.npass == b.npass && a.mflavour == b.mflavour &&
           a.build_needed == b.build_needed && a.plane_wanted == b.plane_wanted && a.qb_int8 == b.qb_int8 && a.P == b.P &&
           a.nsub == b.nsub && a.pl_cap == b.pl_cap && a.qs.s_tiles == b.qs.s_tiles && a.qs.s_stride == b.qs.s_stride &&
           a.qs.s_rows == b.qs.s_rows && a.qs.ld_s == b.qs.ld_s && same_stats(a.stats, b.stats);
}
static bool listed_metric(int metric) {
    return metric == HDB_DOT || metric == HDB_COSINE || metric == HDB_EUCLIDEAN || metric == HDB_MANHATTAN || metric == HDB_PEARSON;
}
static auto fin = [] { return true; };

// one flat JSON object: "key": integer | "string"
struct Row { std::map<std::string, long long> num; std::map<std::string, std::string> str; };
static bool parse_row(const std::string& s, Row& r) {
    size_t i = 0;
    while ((i = s.find('"', i)) != std::string::npos) {
        const size_t e = s.find('"', i + 1);
        if (e == std::string::npos) return false;
        const std::string key = s.substr(i + 1, e - i - 1);
        size_t v = e + 1;
        while (v < s.size() && (s[v] == ':' || s[v] == ' ')) ++v;
        if (v >= s.size()) return false;
        if (s[v] == '"') {
            const size_t ve = s.find('"', v + 1);
            if (ve == std::string::npos) return false;
            r.str[key] = s.substr(v + 1, ve - v - 1);
            i = ve + 1;
        } else {
            char* end = nullptr;
            r.num[key] = std::strtoll(s.c_str() + v, &end, 10);
            if (end == s.c_str() + v) return false;
            i = (size_t)(end - s.c_str());
        }
    }
    return true;
}
struct OptName { const char* name; int64_t hdb_options::*field; };
static const OptName OPTS[] = {
    {"max_blocks", &hdb_options::max_blocks}, {"force_exact", &hdb_options::force_exact}, {"sample_target", &hdb_options::sample_target},
    {"mfma_min_q", &hdb_options::mfma_min_q}, {"use_mfma", &hdb_options::use_mfma}, {"exact_bytes", &hdb_options::exact_bytes},
    {"bits_fused", &hdb_options::bits_fused}, {"bits_local", &hdb_options::bits_local}, {"fused_max_q", &hdb_options::fused_max_q},
    {"f32_min_q", &hdb_options::f32_min_q}, {"f32_split", &hdb_options::f32_split}, {"f32_split_min_q", &hdb_options::f32_split_min_q},
    {"bits_max_q", &hdb_options::bits_max_q}, {"use_fused", &hdb_options::use_fused}, {"use_local", &hdb_options::use_local},
    {"local_m", &hdb_options::local_m}, {"local_max_tiles", &hdb_options::local_max_tiles}, {"local_small", &hdb_options::local_small},
    {"local_max_q", &hdb_options::local_max_q}, {"use_l1_tile", &hdb_options::use_l1_tile}, {"use_batch1", &hdb_options::use_batch1},
    {"mfma_variant", &hdb_options::mfma_variant}, {"use_quant", &hdb_options::use_quant}, {"quant_min_n", &hdb_options::quant_min_n},
    {"quant_max_k", &hdb_options::quant_max_k}, {"auto_quant", &hdb_options::auto_quant}, {"quant_batch_min_n", &hdb_options::quant_batch_min_n},
    {"quant_batch_kernel", &hdb_options::quant_batch_kernel}, {"use_plane", &hdb_options::use_plane}, {"plane_min_n", &hdb_options::plane_min_n},
    {"plane_cap_rows", &hdb_options::plane_cap_rows},
};
static int dtype_of(const std::string& s) { return s == "f16" ? HDB_F16 : s == "f32" ? HDB_F32 : s == "f64" ? HDB_F64 : s == "bf16" ? HDB_BF16 : -1; }
static int metric_of(const std::string& s) {
    return s == "dot" ? HDB_DOT : s == "cosine" ? HDB_COSINE : s == "euclidean" ? HDB_EUCLIDEAN : s == "hamming" ? HDB_HAMMING :
           s == "manhattan" ? HDB_MANHATTAN : s == "jaccard" ? HDB_JACCARD : s == "pearson" ? HDB_PEARSON : -1;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: subset_plan_check TABLE.jsonl\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::printf("cannot open %s\n", argv[1]); return 2; }

    // ---- unchanged: the recorded dispatch table ----
    std::string line;
    long rows = 0, lines = 0;
    int cus = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        ++lines;
        Row r;
        if (!parse_row(line, r)) { CHECK(false, "line %ld does not parse", lines); continue; }
        if (r.str.count("header")) { cus = (int)r.num["cus"]; continue; }
        ++rows;
        char dt[8] = "", me[16] = ""; long long n = -1; int d = 0, nq = 0, k = 0;
        CHECK(std::sscanf(r.str["call"].c_str(), "%7s %d %lld %d %d %15s", dt, &d, &n, &nq, &k, me) == 6, "line %ld: call", lines);
        TopkFacts f{};                   // (no list: the member is not set)
        f.n = n; f.d = d; f.dtype = dtype_of(dt);
        f.qmode = r.num["pre_shadow"] ? HDB_QUANT_I8 : HDB_QUANT_NONE; f.qauto = r.num["pre_auto"] != 0;
        f.plane_present = r.num["pre_plane"] != 0; f.has_mask = r.num["mask"] != 0; f.has_bias = r.num["bias"] != 0; f.cus = cus;
        const TopkCall c{nq, k, metric_of(me), true, r.num["exact"] != 0};
        hdb_options o;
        for (const auto& kv : r.num) {
            if (kv.first.compare(0, 4, "opt.") != 0) continue;
            for (const OptName& on : OPTS) if (kv.first.substr(4) == on.name) o.*(on.field) = kv.second;
        }
        const bool finite_m = r.num["nonfinite"] == 0;
        const TopkPlan p = plan_topk(f, o, c, [&] { return finite_m; });
        CHECK(!p.subset && p.stats.subset == 0, "line %ld: a plan without a list says subset", lines);
        // the recorded statistics ("-" = stale in the table: zero in the plan, quant_auto is the index's)
        const struct { const char* name; long long got; bool plan; } st[] = {
            {"path", p.stats.path, true}, {"fused", p.stats.fused, true}, {"local", p.stats.local, true}, {"mfma", p.stats.mfma, true},
            {"f32_split", p.stats.f32s, true}, {"quant", p.stats.quant, true}, {"quant_auto", 0, false}, {"plane", p.stats.plane, true},
            {"chunks", p.stats.chunks, true}, {"sample_rows", p.stats.sample_rows, true}, {"sample_m", p.stats.sample_m, true},
        };
        const char* tok = r.str["stats"].c_str();
        for (const auto& s : st) {
            char* end = nullptr;
            while (*tok == ' ') ++tok;
            if (*tok == '-') { ++tok; if (s.plan) CHECK(s.got == 0, "line %ld: %s is stale in the table, the plan says %lld", lines, s.name, s.got); continue; }
            const long long want = std::strtoll(tok, &end, 10);
            CHECK(end != tok, "line %ld: stats has no %s", lines, s.name);
            if (s.plan) CHECK(want == s.got, "line %ld: %s is %lld in the table, %lld in the plan", lines, s.name, want, s.got);
            tok = end;
        }
        // ... and the same plan from facts that carry a list the options switch off, or a list of no rows
        TopkFacts fl = f; fl.subset_m = std::max<int64_t>(1, n / 64); fl.has_mask = true;
        TopkFacts fm = f; fm.has_mask = true;
        hdb_options off = o; off.use_subset = 0; off.subset_min_n = 0; off.subset_ratio = 1;
        const TopkPlan pm = plan_topk(fm, o, c, [&] { return finite_m; });
        const TopkPlan pl = plan_topk(fl, off, c, [&] { return finite_m; });
        CHECK(!pl.subset && pl.stats.subset == 0 && same_plan(pl, pm), "line %ld: use_subset = 0 changes the plan", lines);
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
                    CHECK(same_plan(p, inner), WHERE);
                    CHECK(p.kk == (uint32_t)std::min<int64_t>(k, m) && p.ld_n >= m && p.small == (m <= HDB_CAND_CAP), WHERE);
                    CHECK(!(k > HDB_MAX_K && m > HDB_CAND_CAP), WHERE);
                    if (!p.small && !p.exact) CHECK(p.s_tiles * 16 * p.s_stride <= m, WHERE);      // the sample's last list tile exists
                } else {
                    CHECK(p.stats.subset == 0 && same_plan(p, masked), WHERE);
                }
            }
            // never: the bit metrics, a full sort inside, the switches
            if (is_bits_metric(metric) || inner.path == HDB_PATH_FULL_SORT) CHECK(!plan_topk(f, on, c, fin).subset, WHERE);
            if (k > HDB_MAX_K && m > HDB_CAND_CAP) CHECK(inner.path == HDB_PATH_FULL_SORT, WHERE);
            hdb_options off = on; off.use_subset = 0;
            const TopkPlan p_off = plan_topk(f, off, c, fin);
            CHECK(!p_off.subset && same_plan(p_off, masked), WHERE);
            hdb_options big = on; big.subset_min_n = n + 1;
            const TopkPlan p_big = plan_topk(f, big, c, fin);
            CHECK(!p_big.subset && same_plan(p_big, masked), WHERE);
            hdb_options at = on; at.subset_min_n = n;                                       // n >= subset_min_n is inclusive
            CHECK(plan_topk(f, at, c, fin).subset == plan_topk(f, on, c, fin).subset, WHERE);
            // the measured rule (-1 / -1): never below HDB_SUBSET_MIN_ROWS rows, HDB_SUBSET_RATIO in the inequality
            const hdb_options dflt;
            const bool want_d = listed_metric(metric) && n >= HDB_SUBSET_MIN_ROWS && m * groups * HDB_SUBSET_RATIO <= n && inner.path == HDB_PATH_PIPELINE;
            const TopkPlan p_d = plan_topk(f, dflt, c, fin);
            CHECK(p_d.subset == want_d, WHERE);
            if (n < 32768) CHECK(!p_d.subset, WHERE);
            if (p_d.subset) { ++taken_default; CHECK(same_plan(p_d, plan_topk(fin_m, [&] { hdb_options x = dflt; x.use_mfma = 0; x.use_fused = 0; x.use_quant = 0; x.use_l1_tile = 0; return x; }(), c, fin)), WHERE); }
            else CHECK(same_plan(p_d, plan_topk(fmask, dflt, c, fin)), WHERE);
            plans += 4;
        }
    }
    CHECK(taken > 1000 && taken_default > 100, "the grid takes the list in %ld / %ld plans", taken, taken_default);
    std::printf("rows %ld\ngrid plans %ld\ntaken %ld (default rule %ld)\n %ld failures\n", rows, plans, taken, taken_default, g_fail);
    return g_fail ? 1 : 0;
}
