// bf16_quant_plan_check.hip -- the opt-in int8 shadow of a bfloat16 index on the host: plan_topk (csrc/hdb_plan.h) for bfloat16
// facts with and without a shadow.  A stand-alone program, no GPU call.
// A) facts {dtype = HDB_BF16, qmode = HDB_QUANT_I8, qauto = false} (an index whose caller set bf16_quant and called
//    hdb_index_quantize): the plan is HDB_PATH_QUANT with mflavour == false, build_needed == false, stats.quant == 1,
//    stats.mfma == 0 EXACTLY for 1-4 dot / cosine / euclidean queries, k <= 128, status words present, not exact, a finite matrix
//    of more than HDB_CAND_CAP rows and at least the rule's (quant_min_rows(HDB_BF16), or quant_min_n); plane_wanted EXACTLY for
//    one dot / cosine query, d <= 512, n >= the plane rule (HDB_PLANE_MIN_ROWS, or plane_min_n); P = round_up(d, 16); the
//    finiteness is asked at most once per plan, and exactly once where everything else admits the shadow; with use_quant = 0
//    nothing takes the shadow and the plan is the plan of the same index without one.
// B) facts with qmode = HDB_QUANT_NONE under default options and under quant_min_n = 0: never a shadow, never build_needed (the
//    automatic build stays an fp16 rule), and field for field the plan the same facts get with use_quant = 0 -- the library
//    before the option, where no bfloat16 call could reach the shadow rules.
// Prints "plans N" and "F failures"; exit status 1 on any failure.
#include "plan_check.h"
#include <cstdio>

int main() {
    CHECK(hdb_options().bf16_quant == 0, "the option is off by default");
    CHECK(quant_min_rows(HDB_BF16) == 1000000, "the measured rule of bfloat16");
    CHECK(quant_min_rows(HDB_F16) == 1250000 && quant_min_rows(HDB_F32) == 500000, "the other types keep their rules");

    long plans = 0, taken = 0, planes = 0;
    const int64_t ns[] = {8192, 8193, 70001, 999999, 1000000, 1249999, 1250000, 2000000, 10000000};      // (both sides of the measured rule and of fp16's)
    const int ds[] = {40, 128, 384, 512, 520, 768};
    const int nqs[] = {1, 2, 4, 5, 24};
    const int ks[] = {1, 128, 129};
    // option variants: 0 defaults, 1 quant_min_n = 0, 2 quant_min_n = 0 and plane_min_n = 0, 3 use_quant = 0, 4 use_plane = 0 with quant_min_n = 0
    for (int variant = 0; variant < 5; ++variant)
    for (int64_t n : ns) for (int d : ds) for (int nq : nqs) for (int k : ks)
    for (int metric = HDB_DOT; metric <= HDB_PEARSON; ++metric) for (int status = 0; status < 2; ++status) for (int exact = 0; exact < 2; ++exact) for (int fin = 0; fin < 2; ++fin) {
        hdb_options o;
        if (variant == 1 || variant == 2 || variant == 4) o.quant_min_n = 0;
        if (variant == 2) o.plane_min_n = 0;
        if (variant == 3) o.use_quant = 0;
        if (variant == 4) o.use_plane = 0;
        const TopkCall c{nq, k, metric, status != 0, exact != 0};
#define WHERE "variant %d n %lld d %d nq %d k %d metric %d status %d exact %d finite %d", variant, (long long)n, d, nq, k, metric, status, exact, fin

        // ---- A: the index holds an explicit shadow ----
        TopkFacts f{};
        f.n = n; f.d = d; f.dtype = HDB_BF16; f.cus = 256; f.qmode = HDB_QUANT_I8; f.qauto = false; f.plane_present = d <= 512 && o.use_plane;
        int asked = 0;
        const TopkPlan p = plan_topk(f, o, c, [&] { ++asked; return fin != 0; });
        ++plans;
        const int64_t rule = o.quant_min_n >= 0 ? o.quant_min_n : (int64_t)1000000;      // (the measured rule, profiles/bf16_quant_time.txt, as a literal)
        const bool call_ok = nq >= 1 && nq <= 4 && (metric == HDB_DOT || metric == HDB_COSINE || metric == HDB_EUCLIDEAN) && k <= 128 &&
                             status && !exact && n > HDB_CAND_CAP && n >= rule && o.use_quant;
        const bool want = call_ok && fin;
        const bool is_quant = p.path == HDB_PATH_QUANT;
        CHECK(is_quant == want, WHERE);
        CHECK(p.path != HDB_PATH_QUANT_BATCH && !p.build_needed, WHERE);
        CHECK((p.stats.quant == 1) == want && (p.stats.quant == 0) == !want, WHERE);
        CHECK(asked <= 1, WHERE);
        if (call_ok) CHECK(asked == 1, WHERE);
        if (want) {
            ++taken;
            CHECK(!p.mflavour && !p.build_needed && p.stats.mfma == 0 && p.stats.fused == 0 && p.stats.path == 1 && p.stats.chunks == 1, WHERE);
            CHECK(p.P == (d + 15) / 16 * 16 && p.nsub == 0 && p.kk == (uint32_t)k, WHERE);
            const int64_t plane_rule = o.plane_min_n >= 0 ? o.plane_min_n : (int64_t)2000000;
            const bool plane = nq == 1 && (metric == HDB_DOT || metric == HDB_COSINE) && d <= 512 && n >= plane_rule && o.use_plane;
            CHECK(p.plane_wanted == plane && p.stats.plane == (plane ? 1 : 0), WHERE);
            planes += plane ? 1 : 0;
            CHECK(p.qs.s_rows > 0 && p.stats.sample_rows == p.qs.s_rows && p.stats.sample_m == 16, WHERE);
        } else {
            CHECK(!p.plane_wanted && p.stats.plane == 0 && !p.mflavour, WHERE);
            // a bfloat16 call the shadow does not take is the call of the index without one
            TopkFacts f0 = f; f0.qmode = HDB_QUANT_NONE; f0.plane_present = false;
            const TopkPlan p0 = plan_topk(f0, o, c, [&] { return fin != 0; });
            CHECK_SAME_PLAN(p, p0, WHERE);
        }

        // ---- B: no shadow (variants 0 and 1: default options and quant_min_n = 0) ----
        if (variant <= 1) {
            TopkFacts g{};
            g.n = n; g.d = d; g.dtype = HDB_BF16; g.cus = 256; g.qmode = HDB_QUANT_NONE;
            int asked_b = 0;
            const TopkPlan b = plan_topk(g, o, c, [&] { ++asked_b; return fin != 0; });
            ++plans;
            CHECK(!b.shadow() && !b.build_needed && !b.mflavour && !b.plane_wanted && b.stats.quant == 0 && b.stats.plane == 0, WHERE);
            CHECK(asked_b <= 1, WHERE);
            hdb_options off = o;
            off.use_quant = 0; off.auto_quant = 0;
            const TopkPlan b0 = plan_topk(g, off, c, [&] { return fin != 0; });
            CHECK_SAME_PLAN(b, b0, WHERE);
            // 1-4 queries stay on the VALU scan, whatever the matrix holds
            if (nq <= 4) CHECK(!b.mfma && b.stats.mfma == 0 && asked_b == 0, WHERE);
        }
    }
    // the explicit rule of the other types is untouched by the new one: fp16 / fp32 facts with a shadow at the bf16 rule's edge
    for (int dtype : {(int)HDB_F16, (int)HDB_F32}) for (int64_t n : {(int64_t)499999, (int64_t)500000, (int64_t)1249999, (int64_t)1250000}) {
        TopkFacts f{};
        f.n = n; f.d = 384; f.dtype = dtype; f.cus = 256; f.qmode = HDB_QUANT_I8;
        const TopkPlan p = plan_topk(f, hdb_options(), TopkCall{1, 100, HDB_COSINE, true, false}, [] { return true; });
        ++plans;
        CHECK((p.path == HDB_PATH_QUANT) == (n >= (dtype == HDB_F16 ? 1250000 : 500000)), "dtype %d n %lld", dtype, (long long)n);
    }
    // float8 and float64 facts never plan the explicit shadow, whatever qmode says
    for (int dtype : {(int)HDB_F8E4M3, (int)HDB_F64}) {
        TopkFacts f{};
        f.n = 2000000; f.d = 384; f.dtype = dtype; f.cus = 256; f.qmode = HDB_QUANT_I8;
        hdb_options o; o.quant_min_n = 0;
        const TopkPlan p = plan_topk(f, o, TopkCall{1, 100, HDB_COSINE, true, false}, [] { return true; });
        ++plans;
        CHECK(!p.shadow() && p.stats.quant == 0, "dtype %d", dtype);
    }
    CHECK(taken > 1000 && planes > 50, "the grid reached the shadow %ld times, the plane %ld times", taken, planes);
    std::printf("plans %ld\n shadow %ld plane %ld\n", plans, taken, planes);
    return check_done();
}
