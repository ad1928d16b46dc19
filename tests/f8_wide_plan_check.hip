// f8_wide_plan_check.hip -- the opt-in K slices of float8 e4m3 rows wider than 512 elements on the host: the slice lists
// (ks_geom_f8, csrc/hdb_caps.h) and plan_topk (csrc/hdb_plan.h) under the option f8_ks_min_q.  A stand-alone program, no GPU call.
// 1) ks_geom_f8(d) for d = 1 .. 4096: slices exactly at bfloat16's widths, every slice 256 / 384 / 512 elements, widths add up to
//    d and equal ks_geom_bf16's slice by slice, offsets cumulative (one byte per element: byte offset = element offset) and
//    multiples of 8;
// 2) the caps that describe the default dispatch do not know the slices: hdb_mfma_ksplit_slices, hdb_mfma_tile_rows and
//    hdb_mfma_supported are 0 for float8 beyond 512 elements;
// 3) default options (f8_ks_min_q = 0): no float8 plan has ksplit, none beyond 512 elements has mfma;
// 4) f8_ks_min_q = 5: ksplit and mfma EXACTLY for 5+ dot / cosine / euclidean / pearson queries on a finite matrix of a sliced width
//    above HDB_CAND_CAP rows with use_mfma on and no row list taken; such a plan has ld_ks = ld_n, at most 128 queries per chunk,
//    16-row tiles, the pipeline or the full sort, and asked for the finiteness once; every plan is field for field the bfloat16
//    plan of the same shape under bf16_ks_min_q = 5;
// 5) other values: 9 starts at 9 queries, -1 at hdb_mfma_f8_ks_min_q(d), 3 is clamped to 5.
// Prints "plans N" and "F failures"; exit status 1 on any failure.
#include "plan_check.h"
#include <cstdio>

// bfloat16's sliced widths, as literals: 640 .. 1536 in steps of 128, 2048, 3072, 4096

int main() {
    // ---- 1, 2: the slice lists and the caps of the default dispatch ----
    int with_slices = 0;
    for (int d = 1; d <= 4096; ++d) {
        const KsGeom g = ks_geom_f8(d), b = ks_geom_bf16(d);
        CHECK((g.slices > 0) == sliced_width(d) && g.slices == b.slices && g.slices <= HDB_KS_MAX_SLICES && hdb_mfma_f8_ks_slices(d) == g.slices, "d %d: %d slices", d, g.slices);
        int sum = 0;
        for (int s = 0; s < g.slices && s < HDB_KS_MAX_SLICES; ++s) {
            CHECK(g.width[s] == 256 || g.width[s] == 384 || g.width[s] == 512, "d %d slice %d: width %d", d, s, g.width[s]);
            CHECK(g.width[s] == b.width[s], "d %d slice %d: width %d, bfloat16's %d", d, s, g.width[s], b.width[s]);
            CHECK(s == 0 || g.width[s] <= g.width[s - 1], "d %d slice %d: the widest first", d, s);
            CHECK(g.off[s] == sum && g.off[s] % 8 == 0 && 2 * g.off[s] == b.off[s], "d %d slice %d: offset %d, %d elements before it", d, s, g.off[s], sum);
            sum += g.width[s];
        }
        if (g.slices > 0) { ++with_slices; CHECK(sum == d, "d %d: the slices cover %d elements", d, sum); }
        // fewest slices: one fewer could not cover the row with 512 elements each
        if (g.slices > 0) CHECK((g.slices - 1) * 512 < d, "d %d: %d slices", d, g.slices);
        if (d > 512) {
            CHECK(hdb_mfma_ksplit_slices(HDB_F8E4M3, d) == 0 && ks_geom(HDB_F8E4M3, d).slices == 0, "d %d", d);
            CHECK(hdb_mfma_tile_rows(HDB_F8E4M3, d) == 0 && hdb_mfma_f8_tile_rows(d) == 0 && hdb_mfma_anyd_pad(HDB_F8E4M3, d) == 0, "d %d", d);
            for (int metric = HDB_DOT; metric <= HDB_PEARSON; ++metric) CHECK(!hdb_mfma_supported(HDB_F8E4M3, d, metric), "d %d metric %d", d, metric);
        }
        CHECK(hdb_mfma_f8_ks_min_q(d) >= 5, "d %d: the rule starts at %d queries", d, hdb_mfma_f8_ks_min_q(d));
    }
    CHECK(with_slices == 11, "%d widths have slices", with_slices);
    CHECK(hdb_mfma_tile_rows(HDB_F8E4M3, 512) == 16 && hdb_mfma_supported(HDB_F8E4M3, 512, HDB_COSINE) && hdb_mfma_f8_ks_slices(512) == 0, "d = 512 is a whole row");
    CHECK(hdb_options().f8_ks_min_q == 0, "the option is off by default");

    // ---- 3, 4, 5: the planner ----
    long plans = 0;
    const int ds[] = {512, 640, 768, 1024, 1536, 4096, 600, 520};
    const int nqs[] = {1, 2, 4, 5, 8, 9, 16, 130, 300};
    const int64_t ns[] = {1, 300, 8192, 8193, 20003, 60001, 1000000, 10000000};
    const int ks[] = {1, 100, 128, 129, 2049, 9000};
    const int64_t opts[] = {0, 5, 9, -1, 3};
    for (int64_t opt : opts) for (int variant = 0; variant < 4; ++variant) {
        if (opt != 0 && opt != 5 && variant != 0) continue;                        // (the variants under the default and under 5; the other values on plain options)
        for (int d : ds) for (int64_t n : ns) for (int nq : nqs) for (int k : ks)
        for (int metric = HDB_DOT; metric <= HDB_PEARSON; ++metric) for (int aux = 0; aux < 4; ++aux) for (int fin = 0; fin < 2; ++fin) for (int exact = 0; exact < 2; ++exact) {
            hdb_options o;
            o.f8_ks_min_q = opt;
            if (variant == 1) o.quant_min_n = 0;
            if (variant == 2) o.subset_min_n = 0;                                  // the row list wherever the ratio admits it
            if (variant == 3) { o.use_mfma = 0; o.use_fused = 0; o.use_l1_tile = 0; }
            TopkFacts f{};
            f.n = n; f.d = d; f.dtype = HDB_F8E4M3; f.cus = 256; f.qmode = HDB_QUANT_NONE; f.has_bias = (aux & 1) != 0; f.has_mask = (aux & 2) != 0;
            if (variant == 2 && f.has_mask) f.subset_m = n / 3 > 1000 ? 1000 : n / 3;
            const TopkCall c{nq, k, metric, true, exact != 0};
            int asked = 0;
            const TopkPlan p = plan_topk(f, o, c, [&] { ++asked; return fin != 0; });
            ++plans;
#define WHERE "f8_ks_min_q %lld variant %d d %d n %lld nq %d k %d metric %d aux %d finite %d exact %d", (long long)opt, variant, d, (long long)n, nq, k, metric, aux, fin, exact
            const bool mm = metric == HDB_DOT || metric == HDB_COSINE || metric == HDB_EUCLIDEAN || metric == HDB_PEARSON;
            const bool sorted = p.path == HDB_PATH_FULL_SORT;
            CHECK(!p.shadow() && p.path != HDB_PATH_FUSED && p.path != HDB_PATH_BATCH1 && !p.l1tile && !p.f32s && !p.f16_queries && p.stats.quant == 0, WHERE);
            CHECK(p.path == HDB_PATH_PIPELINE || sorted || p.path == HDB_PATH_BITS1, WHERE);
            CHECK(p.tile_rows == 16 && p.cq_max >= 1 && p.cq_max <= std::min(nq, 256), WHERE);
            // the whole-row rule, unchanged: d = 512 from 5 queries on
            const bool whole = d == 512 && o.use_mfma && mm && nq >= 5 && n > HDB_CAND_CAP && !p.subset;
            if (opt == 0) {                        // the default: the library before the slices
                CHECK(!p.ksplit && p.ld_ks == 0, WHERE);
                if (d > 512) CHECK(!p.mfma && p.stats.mfma == 0 && asked == 0, WHERE);
                else CHECK(p.mfma == (whole && fin) && asked == (whole ? 1 : 0), WHERE);
                TopkFacts fb = f; fb.dtype = HDB_BF16;
                hdb_options ob = o; ob.use_mfma = 0;
                TopkPlan b = plan_topk(fb, ob, c, [&] { return fin != 0; });
                if (p.mfma) { b.mfma = true; b.stats.mfma = sorted ? 0 : 1; b.mask_fold = f.has_mask && !sorted; }
                CHECK_SAME_PLAN(p, b, WHERE);
                continue;
            }
            const int first = opt == 5 ? 5 : opt == 9 ? 9 : opt == 3 ? 5 : hdb_mfma_f8_ks_min_q(d);
            CHECK(first >= 5, WHERE);
            const bool eligible = sliced_width(d) && nq >= first && mm && n > HDB_CAND_CAP && o.use_mfma && !p.subset;
            const bool want = eligible && fin;
            CHECK(p.ksplit == want, WHERE);
            CHECK(p.mfma == (want || (whole && fin)) && p.stats.mfma == (p.mfma && !sorted ? 1 : 0), WHERE);
            CHECK(asked == ((eligible || whole) ? 1 : 0), WHERE);              // asked once, and only where it decides
            CHECK(p.mask_fold == (p.mfma && f.has_mask && !sorted), WHERE);
            if (want) {
                CHECK(p.ld_ks == p.ld_n && p.ld_n == (int64_t)align_up((size_t)n, 4), WHERE);
                CHECK(p.cq_max <= 128 && (int64_t)p.cq_max * p.ld_ks * 4 <= std::max<int64_t>(o.exact_bytes, p.ld_ks * 4), WHERE);
                CHECK(p.path == HDB_PATH_PIPELINE || sorted, WHERE);
                CHECK(sorted == (k > HDB_MAX_K), WHERE);
                CHECK(p.stats.chunks == (sorted ? nq : (nq + p.cq_max - 1) / p.cq_max) && p.stats.fused == 0 && p.stats.subset == 0, WHERE);
                if (!p.exact && !sorted) CHECK(p.s_rows == p.s_tiles * 16 && p.s_tiles > 0 && p.s_tiles * p.s_stride * 16 <= n, WHERE);
            } else CHECK(p.ld_ks == 0, WHERE);
            // the bfloat16 plan of the same shape under the same threshold: equal field for field (a bfloat16 row of 512 elements is a
            // 16-row tile as well; 600 and 520 have no geometry for either)
            TopkFacts fb = f; fb.dtype = HDB_BF16;
            hdb_options ob = o; ob.bf16_ks_min_q = first;
            const TopkPlan b = plan_topk(fb, ob, c, [&] { return fin != 0; });
            CHECK_SAME_PLAN(p, b, WHERE);
        }
    }
    // the option reaches the sliced widths only: whole rows keep their 5 whatever it says
    for (int64_t opt : {(int64_t)0, (int64_t)40}) for (int d : {128, 256, 384, 512}) {
        hdb_options o;
        o.f8_ks_min_q = opt;
        TopkFacts f{};
        f.n = 20003; f.d = d; f.dtype = HDB_F8E4M3; f.cus = 256; f.qmode = HDB_QUANT_NONE;
        const TopkPlan p = plan_topk(f, o, TopkCall{5, 50, HDB_COSINE, true, false}, [] { return true; });
        ++plans;
        CHECK(p.mfma && !p.ksplit && p.ld_ks == 0, "f8 d %d, 5 queries, f8_ks_min_q %lld", d, (long long)opt);
    }
    // mfma_min_q holds for the slices as well
    {
        hdb_options o; o.f8_ks_min_q = 5; o.mfma_min_q = 12;
        TopkFacts f{};
        f.n = 20003; f.d = 768; f.dtype = HDB_F8E4M3; f.cus = 256; f.qmode = HDB_QUANT_NONE;
        const TopkPlan p8 = plan_topk(f, o, TopkCall{8, 50, HDB_COSINE, true, false}, [] { return true; });
        const TopkPlan p12 = plan_topk(f, o, TopkCall{12, 50, HDB_COSINE, true, false}, [] { return true; });
        plans += 2;
        CHECK(!p8.ksplit && !p8.mfma && p12.ksplit && p12.mfma, "mfma_min_q = 12");
    }
    std::printf("plans %ld\n", plans);
    return check_done();
}
