// b1_mfma_plan_check.hip -- the plans of a packed-bit matrix (HDB_B1) under the opt-in b1_mfma_min_q: a stand-alone host program, no GPU call.
// 1) the rules (csrc/hdb_caps.h): hdb_mfma_b1_tile_rows is 16 at d = 128 / 256 / 384 / 512 and 0 elsewhere; ks_geom_b1 has
//    ks_geom_bf16's slice list at every width, every slice's BYTE offset is a multiple of 4 (of 16, in fact), equals an eighth of the
//    elements before it and the slice lies inside the row of d / 8 bytes; the default-dispatch rules keep answering "no";
// 2) plan_topk (csrc/hdb_plan.h) over the grid of b1_plan_check.hip widened by d in {640, 1152, 2048, 4096, 544, 4128} and nq in {9, 64}:
//    with b1_mfma_min_q = 0 every plan equals today's -- the int8 plan with use_mfma = 0 for the float metrics, the int8 plan for the
//    bit metrics; with the option at -1 / 1 / 5 / 16 (threshold in force T = max(option or hdb_mfma_b1_min_q(d), 5, mfma_min_q), 0 =
//    never) the plan equals, field for field, at the four whole widths the int8 plan made with mfma_min_q = T and a matrix that is
//    finite, at the sliced widths the float8 plan made with f8_ks_min_q = T and f8_lds_min_q = 0, and at every other width, for
//    manhattan and the bit metrics, for 1-4 queries and with use_mfma = 0 today's plan;
// 3) the finiteness callback is never called for a packed-bit plan.
// Prints "plans N", "mfma plans M" and "F failures"; exit status 1 on any failure.
#include "plan_check.h"
#include <cstdio>
#include <cstring>

int main() {
    // ---- 1: the rules ----
    for (int d = 1; d <= 8192; ++d) {
        CHECK(hdb_mfma_b1_tile_rows(d) == (whole_width(d) ? 16 : 0), "d %d", d);
        const KsGeom g = ks_geom_b1(d), b = ks_geom_bf16(d);
        CHECK(g.slices == b.slices && hdb_mfma_b1_ks_slices(d) == g.slices && (g.slices > 0) == sliced_width(d) && g.slices <= HDB_KS_MAX_SLICES, "d %d: %d slices", d, g.slices);
        int at = 0;
        for (int s = 0; s < g.slices; ++s) {
            CHECK(g.width[s] == b.width[s] && (g.width[s] == 256 || g.width[s] == 384 || g.width[s] == 512), "d %d slice %d: %d elements", d, s, g.width[s]);
            CHECK(g.off[s] % 4 == 0 && g.off[s] % 16 == 0 && g.off[s] * 8 == at && g.off[s] >= 0, "d %d slice %d: byte offset %d after %d elements", d, s, g.off[s], at);
            CHECK((int64_t)g.off[s] + g.width[s] / 8 <= hdb_row_bytes(HDB_B1, d), "d %d slice %d leaves the row", d, s);
            at += g.width[s];
        }
        if (g.slices) CHECK(at == d, "d %d: the slices cover %d elements", d, at);
        CHECK(!(whole_width(d) && g.slices), "d %d: whole and sliced", d);
        // the default dispatch knows nothing of it
        CHECK(hdb_mfma_tile_rows(HDB_B1, d) == 0 && hdb_mfma_ksplit_slices(HDB_B1, d) == 0 && hdb_mfma_batch_capacity(HDB_B1, d) == 0, "d %d", d);
        for (int metric = HDB_DOT; metric <= HDB_PEARSON; ++metric) {
            CHECK(!hdb_mfma_supported(HDB_B1, d, metric), "d %d metric %d", d, metric);
            for (int nq = 1; nq <= 4; ++nq) CHECK(!hdb_mfma_fused_supported(HDB_B1, d, metric, nq, 100), "d %d metric %d", d, metric);
        }
        CHECK(b1_mfma_first_q(hdb_options{}, HDB_B1, d) == 0, "d %d: the default is never", d);
        hdb_options o5; o5.b1_mfma_min_q = 5;
        CHECK(b1_mfma_first_q(o5, HDB_B1, d) == ((whole_width(d) || sliced_width(d)) ? 5 : 0), "d %d", d);
        CHECK(b1_mfma_first_q(o5, HDB_I8, d) == 0 && b1_mfma_first_q(o5, HDB_F8E4M3, d) == 0 && b1_mfma_first_q(o5, HDB_BF16, d) == 0, "d %d: other dtypes", d);
        CHECK(hdb_mfma_b1_min_q(d) >= 0 && (hdb_mfma_b1_min_q(d) == 0 || whole_width(d) || sliced_width(d)), "d %d: a rule for a width without a kernel", d);
    }

    // ---- 2, 3: the planner ----
    long plans = 0, on = 0, on_ks = 0, fin_calls = 0;
    const int ds[] = {32, 96, 128, 256, 384, 512, 768, 1024, 4128, 640, 1152, 2048, 4096, 544};
    const int nqs[] = {1, 2, 4, 5, 8, 16, 130, 300, 9, 64};
    const int64_t ns[] = {1, 300, 8192, 8193, 20003, 60001, 1000000, 10000000};
    const int ks[] = {1, 100, 129, 2049, 9000};
    const int vs[] = {0, -1, 1, 5, 16};
    for (int v : vs) for (int variant = 0; variant < 4; ++variant) for (int d : ds) for (int64_t n : ns) for (int nq : nqs) for (int k : ks)
    for (int metric = HDB_DOT; metric <= HDB_PEARSON; ++metric) for (int aux = 0; aux < 4; ++aux) for (int exact = 0; exact < 2; ++exact) {
        hdb_options o;
        o.b1_mfma_min_q = v;
        if (variant == 1) o.use_mfma = 0;
        if (variant == 2) o.mfma_min_q = 7;
        if (variant == 3) { o.subset_min_n = 0; o.f8_ks_min_q = -1; o.f8_lds_min_q = -1; o.max_blocks = 300; }       // (options of other dtypes and a row list: nothing to a packed-bit plan)
        TopkFacts f{};
        f.n = n; f.d = d; f.dtype = HDB_B1; f.cus = 256; f.qmode = HDB_QUANT_NONE; f.has_bias = (aux & 1) != 0; f.has_mask = (aux & 2) != 0;
        if (variant == 3 && f.has_mask) f.subset_m = n / 3 > 1000 ? 1000 : n / 3;
        const TopkCall c{nq, k, metric, true, exact != 0};
        const TopkPlan p = plan_topk(f, o, c, [&] { ++fin_calls; return true; });
        ++plans;
#define WHERE "option %d variant %d d %d n %lld nq %d k %d metric %d aux %d exact %d", v, variant, d, (long long)n, nq, k, metric, aux, exact
        const bool bitm = is_bits_metric(metric);
        // today's plan: the int8 plan (no row list), without the matrix cores for the float metrics
        TopkFacts f8 = f; f8.dtype = HDB_I8; f8.subset_m = 0;
        hdb_options o8 = o; o8.b1_mfma_min_q = 0; o8.f8_ks_min_q = 0; o8.f8_lds_min_q = 0;
        if (!bitm) o8.use_mfma = 0;
        const TopkPlan today = plan_topk(f8, o8, c, [&] { return true; });
        // the threshold in force, by the issue's words
        const int64_t rule = v > 0 ? v : v < 0 ? hdb_mfma_b1_min_q(d) : 0;
        const int64_t T = (rule > 0 && (whole_width(d) || sliced_width(d))) ? std::max<int64_t>(std::max<int64_t>(rule, 5), o.mfma_min_q) : 0;
        CHECK(b1_mfma_first_q(o, HDB_B1, d) == T, WHERE);
        const bool offered = T > 0 && !bitm && metric != HDB_MANHATTAN && o.use_mfma && nq >= 5;
        if (!offered) { CHECK_SAME_PLAN(p, today, WHERE); CHECK(!p.mfma && p.stats.mfma == 0 && !p.ksplit, WHERE); continue; }
        TopkPlan want;
        if (whole_width(d)) {
            hdb_options oi = o; oi.b1_mfma_min_q = 0; oi.f8_ks_min_q = 0; oi.f8_lds_min_q = 0; oi.mfma_min_q = T;
            want = plan_topk(f8, oi, c, [&] { return true; });
        } else {
            TopkFacts ff = f; ff.dtype = HDB_F8E4M3; ff.subset_m = 0;
            hdb_options of = o; of.b1_mfma_min_q = 0; of.f8_ks_min_q = T; of.f8_lds_min_q = 0;
            want = plan_topk(ff, of, c, [&] { return true; });
        }
        CHECK_SAME_PLAN(p, want, WHERE);
        CHECK(!p.shadow() && !p.plane_wanted && !p.build_needed && !p.l1tile && !p.subset && !p.f8_lds && !p.f32s && !p.local && p.stats.fused == 0, WHERE);
        if (nq < T) CHECK_SAME_PLAN(p, today, WHERE);
        if (p.mfma) {
            ++on;
            CHECK(nq >= T && n > HDB_CAND_CAP && p.tile_rows == 16 && p.ksplit == sliced_width(d) && (p.ld_ks > 0) == sliced_width(d), WHERE);
            CHECK(p.path == HDB_PATH_PIPELINE || (p.path == HDB_PATH_FULL_SORT && k > HDB_MAX_K), WHERE);      // (the full sort scores one query at a time on the bit scan)
            if (p.path == HDB_PATH_PIPELINE) CHECK(p.stats.mfma == 1 && p.mask_fold == f.has_mask, WHERE);
            if (p.ksplit) ++on_ks;
        }
    }
    CHECK(fin_calls == 0, "the finiteness callback was asked %ld times for packed-bit plans", fin_calls);
    CHECK(on > 10000 && on_ks > 10000, "the grid reaches the matrix cores (%ld plans) and the slices (%ld)", on, on_ks);
    std::printf("plans %ld\nmfma plans %ld\n", plans, on);
    return check_done();
}
