// bf16_wide_plan_check.hip -- the K-slice lists (ks_geom, csrc/hdb_caps.h) and plan_topk (csrc/hdb_plan.h) for bfloat16 rows wider
// than 512 elements, on the host: a stand-alone program, no GPU call.
// 1) bfloat16: every width of the slice table against the table as literals; widths add up to d, offsets are cumulative (in bytes
//    of the stored row), every slice is 256, 384 or 512 elements wide; 100, 384 and 520 have no slices;
// 2) fp16 / float32: the slice lists they had before the lists could be mixed, as literals;
// 3) plan_topk over nq x n x k x metric x bias / mask for every bfloat16 width: with bf16_ks_min_q = 5, 5+ dot / cosine / euclidean /
//    pearson queries on a finite matrix take the matrix cores through K slices, everything else keeps the VALU scan; with the default
//    (-1) the slices start at the width's measured threshold (hdb_mfma_bf16_ks_min_q: 5 at d = 1024 / 4096, 9 elsewhere).
// Prints "plans N" and "F failures"; exit status 1 on any failure.
#include "plan_check.h"
#include <cstdio>

struct Want { int dtype, d, slices; int width[HDB_KS_MAX_SLICES]; };
static const Want WANT[] = {
    {HDB_BF16, 640, 2, {384, 256}},
    {HDB_BF16, 768, 2, {384, 384}},
    {HDB_BF16, 896, 2, {512, 384}},
    {HDB_BF16, 1024, 2, {512, 512}},
    {HDB_BF16, 1152, 3, {384, 384, 384}},
    {HDB_BF16, 1280, 3, {512, 384, 384}},
    {HDB_BF16, 1408, 3, {512, 512, 384}},
    {HDB_BF16, 1536, 3, {512, 512, 512}},
    {HDB_BF16, 2048, 4, {512, 512, 512, 512}},
    {HDB_BF16, 3072, 6, {512, 512, 512, 512, 512, 512}},
    {HDB_BF16, 4096, 8, {512, 512, 512, 512, 512, 512, 512, 512}},
    // what the uniform table gave: {slices, dslice} = {2, 512}, {2, 768}, {2, 1024}, {2, 1536}, {4, 1024}, offset s * dslice * element bytes
    {HDB_F32, 1024, 2, {512, 512}},
    {HDB_F32, 1536, 2, {768, 768}},
    {HDB_F16, 2048, 2, {1024, 1024}},
    {HDB_F16, 3072, 2, {1536, 1536}},
    {HDB_F16, 4096, 4, {1024, 1024, 1024, 1024}},
};
// ... and their byte offsets, written out
static const int OFF_F32_1024[] = {0, 2048}, OFF_F32_1536[] = {0, 3072}, OFF_F16_2048[] = {0, 2048}, OFF_F16_3072[] = {0, 3072},
                 OFF_F16_4096[] = {0, 2048, 4096, 6144};

static void check_offsets(int dtype, int d, const int* off, int count) {
    const KsGeom g = ks_geom(dtype, d);
    CHECK(g.slices == count, "dtype %d d %d", dtype, d);
    for (int s = 0; s < count && s < g.slices; ++s) CHECK(g.off[s] == off[s], "dtype %d d %d slice %d: offset %d", dtype, d, s, g.off[s]);
}

int main() {
    // ---- 1, 2: the slice lists ----
    for (const Want& w : WANT) {
        const KsGeom g = ks_geom(w.dtype, w.d);
        const int es = w.dtype == HDB_F32 ? 4 : 2;
        CHECK(g.slices == w.slices && g.slices <= HDB_KS_MAX_SLICES, "dtype %d d %d: %d slices", w.dtype, w.d, g.slices);
        CHECK(hdb_mfma_ksplit_slices(w.dtype, w.d) == w.slices, "dtype %d d %d", w.dtype, w.d);
        int sum = 0;
        for (int s = 0; s < w.slices && s < g.slices; ++s) {
            CHECK(g.width[s] == w.width[s], "dtype %d d %d slice %d: width %d", w.dtype, w.d, s, g.width[s]);
            CHECK(g.off[s] == sum * es, "dtype %d d %d slice %d: offset %d, %d elements before it", w.dtype, w.d, s, g.off[s], sum);
            if (w.dtype == HDB_BF16) CHECK(g.width[s] == 256 || g.width[s] == 384 || g.width[s] == 512, "d %d slice %d: width %d", w.d, s, g.width[s]);
            sum += g.width[s];
        }
        CHECK(sum == w.d, "dtype %d d %d: the slices cover %d elements", w.dtype, w.d, sum);
        CHECK(mfma_exact_tile_rows(w.dtype, w.d) == 16 && hdb_mfma_tile_rows(w.dtype, w.d) == 16, "dtype %d d %d", w.dtype, w.d);
        CHECK(hdb_mfma_batch_capacity(w.dtype, w.d) == 0, "dtype %d d %d", w.dtype, w.d);
    }
    check_offsets(HDB_F32, 1024, OFF_F32_1024, 2);
    check_offsets(HDB_F32, 1536, OFF_F32_1536, 2);
    check_offsets(HDB_F16, 2048, OFF_F16_2048, 2);
    check_offsets(HDB_F16, 3072, OFF_F16_3072, 2);
    check_offsets(HDB_F16, 4096, OFF_F16_4096, 4);
    const int none[] = {100, 128, 256, 384, 512, 520, 576, 1600, 2560, 8192};
    for (int d : none) {
        CHECK(ks_geom(HDB_BF16, d).slices == 0 && hdb_mfma_ksplit_slices(HDB_BF16, d) == 0, "bf16 d %d has slices", d);
        CHECK(hdb_mfma_anyd_pad(HDB_BF16, d) == 0, "bf16 d %d is padded", d);
    }
    CHECK(hdb_mfma_tile_rows(HDB_BF16, 100) == 0 && hdb_mfma_tile_rows(HDB_BF16, 520) == 0, "odd bf16 widths stay off the matrix cores");
    CHECK(hdb_mfma_tile_rows(HDB_BF16, 384) == 32 && hdb_mfma_tile_rows(HDB_BF16, 512) == 16 && hdb_mfma_tile_rows(HDB_BF16, 256) == 64, "whole-row bf16 geometries");
    // widths the other dtypes take whole keep doing so
    CHECK(ks_geom(HDB_F16, 768).slices == 0 && ks_geom(HDB_F16, 1536).slices == 0 && ks_geom(HDB_F32, 768).slices == 0 && ks_geom(HDB_F64, 1024).slices == 0, "slices of other dtypes");

    // ---- 3: the planner ----
    long plans = 0;
    const int nqs[] = {1, 2, 4, 5, 8, 16, 33, 128, 129, 130, 300};
    const int64_t ns[] = {8193, 20003, 1000000, 5000000};
    const int ks[] = {1, 50, 128, 2049};
    // bf16_ks_min_q = 5: the slices from 5 queries on at every width; -1 (the default): from the width's measured crossover with the
    // two VALU passes of 5-8 queries -- 5 at d = 1024 and 4096, 9 elsewhere; a larger fixed number holds; never fewer than 5
    for (const Want& w : WANT) {
        if (w.dtype != HDB_BF16) continue;
        CHECK(hdb_mfma_bf16_ks_min_q(w.d) == ((w.d == 1024 || w.d == 4096) ? 5 : 9), "d %d: the slices start at %d queries", w.d, hdb_mfma_bf16_ks_min_q(w.d));
    }
    const int64_t rules[] = {5, -1, 1, 40};
    for (int64_t rule : rules) for (const Want& w : WANT) {
        if (w.dtype != HDB_BF16) continue;
        hdb_options o;
        o.bf16_ks_min_q = rule;
        const int first = (int)std::max<int64_t>(5, rule >= 0 ? rule : hdb_mfma_bf16_ks_min_q(w.d));
        for (int64_t n : ns) for (int nq : nqs) for (int k : ks) for (int metric = HDB_DOT; metric <= HDB_PEARSON; ++metric) for (int aux = 0; aux < 4; ++aux)
        for (int fin = 0; fin < 2; ++fin) for (int exact = 0; exact < 2; ++exact) {
            TopkFacts f{};
            f.n = n; f.d = w.d; f.dtype = HDB_BF16; f.cus = 256; f.qmode = HDB_QUANT_NONE; f.has_bias = (aux & 1) != 0; f.has_mask = (aux & 2) != 0;
            const TopkCall c{nq, k, metric, true, exact != 0};
            int asked = 0;
            const TopkPlan p = plan_topk(f, o, c, [&] { ++asked; return fin != 0; });
            ++plans;
#define WHERE "d %d n %lld nq %d k %d metric %d aux %d finite %d exact %d bf16_ks_min_q %lld", w.d, (long long)n, nq, k, metric, aux, fin, exact, (long long)rule
            const bool mm = metric == HDB_DOT || metric == HDB_COSINE || metric == HDB_EUCLIDEAN || metric == HDB_PEARSON;
            const bool want = mm && nq >= first && fin;
            const bool sorted = p.path == HDB_PATH_FULL_SORT;            // k > HDB_MAX_K: one VALU pass and a sort per query, whatever the plan's flags
            CHECK(sorted == (k > HDB_MAX_K), WHERE);
            CHECK(p.mfma == want && p.stats.mfma == (want && !sorted ? 1 : 0), WHERE);
            CHECK(p.ksplit == want, WHERE);
            CHECK(!p.f32s && !p.f16_queries && !p.q16_in_prep && p.stats.fused == (p.path == HDB_PATH_BITS1 ? 3 : 0) && p.stats.quant == 0, WHERE);
            CHECK(p.path == HDB_PATH_PIPELINE || p.path == HDB_PATH_FULL_SORT || (p.path == HDB_PATH_BITS1 && is_bits_metric(metric)), WHERE);
            CHECK(p.tile_rows == 16, WHERE);
            CHECK(p.cq_max >= 1 && p.cq_max <= std::min(nq, 256), WHERE);
            if (want) {
                CHECK(p.ld_ks == (int64_t)align_up((size_t)n, 4), WHERE);
                CHECK(p.cq_max <= 128 && (int64_t)p.cq_max * p.ld_ks * 4 <= std::max<int64_t>(o.exact_bytes, p.ld_ks * 4), WHERE);
                CHECK(p.stats.chunks == (sorted ? nq : (nq + p.cq_max - 1) / p.cq_max), WHERE);
                CHECK(p.mask_fold == (f.has_mask && p.path != HDB_PATH_FULL_SORT), WHERE);
                CHECK(asked == 1, WHERE);
            } else {
                CHECK(p.ld_ks == 0, WHERE);
                if (nq < first || !mm) CHECK(asked == 0, WHERE);        // the question is not asked where it decides nothing
            }
            // use_mfma = 0 is the plan of the library before the slices: same sample, same chunking up to the 128-query rows
            hdb_options off = o; off.use_mfma = 0;
            const TopkPlan v = plan_topk(f, off, c, [&] { return fin != 0; });
            CHECK(!v.mfma && !v.ksplit && v.ld_ks == 0 && v.tile_rows == 16, WHERE);
            CHECK(v.s_tiles == p.s_tiles && v.s_stride == p.s_stride && v.m == p.m && v.exact == p.exact && v.path == p.path, WHERE);
        }
    }
    // the option reaches the sliced widths only: whole rows (d <= 512) keep their 5
    for (int d : {128, 256, 384, 512}) {
        hdb_options o;
        o.bf16_ks_min_q = 40;
        TopkFacts f{};
        f.n = 20003; f.d = d; f.dtype = HDB_BF16; f.cus = 256; f.qmode = HDB_QUANT_NONE;
        const TopkPlan p = plan_topk(f, o, TopkCall{5, 50, HDB_COSINE, true, false}, [] { return true; });
        CHECK(p.mfma && !p.ksplit && p.ld_ks == 0, "bf16 d %d, 5 queries", d);
    }
    std::printf("plans %ld\n", plans);
    return check_done();
}
