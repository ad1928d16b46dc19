// plan_check.h -- what the stand-alone host check programs (tests/*_check.hip) share: the failure count and its closing line, the
// widths the matrix-core kernels of one-byte and packed rows take, and the replay of tests/golden/dispatch_table.jsonl rows.  Plans
// are compared with plan_diff (csrc/hdb_plan.h): every member, by the one list kept below the struct.
#pragma once
#include "hdb_plan.h"
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>

// CHECK(condition, printf arguments that say where): counts a failure and prints the first 40
static long g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 40) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)
// CHECK_SAME_PLAN(a, b, where): the two plans are equal member for member; the failure names the first member that differs
#define CHECK_SAME_PLAN(a, b, ...) do { const char* diff_ = plan_diff(a, b); if (diff_) { if (++g_fail <= 40) { std::printf("FAIL %s differs between %s and %s: ", diff_, #a, #b); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)
// the last line of every program and its exit status
static inline int check_done() { std::printf(" %ld failures\n", g_fail); return g_fail ? 1 : 0; }

// float8 / int8 / packed-bit rows on the matrix cores: whole rows of these widths, K slices of those
static inline bool whole_width(int d) { return d == 128 || d == 256 || d == 384 || d == 512; }
static inline bool sliced_width(int d) { return (d >= 640 && d <= 1536 && d % 128 == 0) || d == 2048 || d == 3072 || d == 4096; }

// one flat JSON object: "key": integer | "string"
struct Row { std::map<std::string, long long> num; std::map<std::string, std::string> str; };
static inline bool parse_row(const std::string& s, Row& r) {
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
static inline int dtype_of(const std::string& s) { return s == "f16" ? HDB_F16 : s == "f32" ? HDB_F32 : s == "f64" ? HDB_F64 : s == "bf16" ? HDB_BF16 : -1; }
static inline int metric_of(const std::string& s) {
    return s == "dot" ? HDB_DOT : s == "cosine" ? HDB_COSINE : s == "euclidean" ? HDB_EUCLIDEAN : s == "hamming" ? HDB_HAMMING :
           s == "manhattan" ? HDB_MANHATTAN : s == "jaccard" ? HDB_JACCARD : s == "pearson" ? HDB_PEARSON : -1;
}
// The recorded statistics of a row against the plan's.  `names`: the header's "stats", the names of hdb_get_stat in the order of every
// row's "stats" -- looked up in HDB_STATS.  "-" = the parent left the statistic stale on that path: zero in the plan.  quant_auto is
// the index's, not the plan's: compared with `quant_auto` unless that is negative.
static inline void check_row_stats(Row& r, const std::string& names, const TopkPlan& p, long long quant_auto, long line) {
    CHECK(!names.empty(), "line %ld: no header with the names of the statistics before it", line);
    const char* tok = r.str["stats"].c_str();
    for (size_t at = 0, e; at < names.size(); at = e + 1) {
        if ((e = names.find(' ', at)) == std::string::npos) e = names.size();
        const std::string name = names.substr(at, e - at);
        long long got = quant_auto; bool plan = false;
        for (const hdb_stat_entry& s : HDB_STATS) if (name == s.name) { got = p.stats.*s.member; plan = true; }
        CHECK(plan || name == "quant_auto", "line %ld: %s is no statistic of the plan", line, name.c_str());
        while (*tok == ' ') ++tok;
        if (*tok == '-') { ++tok; if (plan) CHECK(got == 0, "line %ld: %s is stale in the table, the plan says %lld", line, name.c_str(), got); continue; }
        char* end = nullptr;
        const long long want = std::strtoll(tok, &end, 10);
        CHECK(end != tok, "line %ld: stats has no %s", line, name.c_str());
        if (plan || quant_auto >= 0) CHECK(want == got, "line %ld: %s is %lld in the table, %lld in the plan", line, name.c_str(), want, got);
        tok = end;
    }
}

// One row of the dispatch table -> what plan_topk is told.  "call": "dtype d n nq k metric"; flags and facts that are zero are left
// out of the line; the "opt.NAME" keys are set the way hdb_set_option sets them (hdb_option_set: the library's names and clamps).
static inline void row_inputs(Row& r, int cus, long line, TopkFacts& f, TopkCall& c, hdb_options& o) {
    char dt[8] = "", me[16] = ""; long long n = -1; int d = 0, nq = 0, k = 0;
    CHECK(std::sscanf(r.str["call"].c_str(), "%7s %d %lld %d %d %15s", dt, &d, &n, &nq, &k, me) == 6, "line %ld: call", line);
    f = TopkFacts{};                 // (no row list: subset_m stays 0)
    f.n = n; f.d = d; f.dtype = dtype_of(dt);
    f.qmode = r.num["pre_shadow"] ? HDB_QUANT_I8 : HDB_QUANT_NONE; f.qauto = r.num["pre_auto"] != 0;
    f.plane_present = r.num["pre_plane"] != 0; f.has_mask = r.num["mask"] != 0; f.has_bias = r.num["bias"] != 0; f.cus = cus;
    c = TopkCall{nq, k, metric_of(me), true, r.num["exact"] != 0};
    CHECK(f.dtype >= 0 && c.metric >= 0 && f.cus > 0 && f.d > 0 && c.nq > 0 && c.k > 0, "line %ld: bad inputs", line);
    o = hdb_options();
    for (const auto& kv : r.num)
        if (kv.first.compare(0, 4, "opt.") == 0) CHECK(hdb_option_set(o, kv.first.c_str() + 4, kv.second), "line %ld: option %s", line, kv.first.c_str());
}
