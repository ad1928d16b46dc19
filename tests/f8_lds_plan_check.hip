// f8_lds_plan_check.hip -- the opt-in LDS flavour of the float8 matrix-core scan on the host: its geometry (csrc/hdb_caps.h) and
// plan_topk (csrc/hdb_plan.h) under the option f8_lds_min_q.  A stand-alone program, no GPU call.
// 1) geometry: for d = 128 / 256 / 384 / 512 and 4 / 8 waves the stage height is a multiple of 16 rows, a whole number of 16-byte
//    pieces per thread, both buffers fit 160 KiB and the workgroups of a CU fit it together; other widths have no stage;
// 2) f8_lds_min_q = 0 (the default): no plan has f8_lds;
// 3) f8_lds_min_q = n or -1: f8_lds EXACTLY where the plan is on the float8 matrix cores outside the full sort -- a whole row of 128 /
//    256 / 384 / 512 elements or, with f8_ks_min_q, the K slices -- and the call has max(n, 5, mfma_min_q) queries (-1:
//    hdb_mfma_f8_lds_min_q(d), 0 = never); never for another dtype, matrices of up to 8192 rows, a row-list call, a matrix that is
//    not finite, manhattan or the bit metrics;
// 4) every other field of the plan equals the plan with the option off.
// Prints "plans N" and "F failures"; exit status 1 on any failure.
#include "plan_check.h"
#include <cstdio>

int main() {
    // ---- 1: the geometry ----
    for (int d = 1; d <= 4096; ++d) {
        CHECK((hdb_mfma_f8_lds_supported(d) != 0) == whole_width(d), "d %d", d);
        if (!whole_width(d)) { CHECK(hdb_mfma_f8_lds_stage_rows(d) == 0 && hdb_mfma_f8_lds_stage_rows(d, 8) == 0, "d %d has a stage", d); continue; }
        CHECK(hdb_mfma_f8_lds_stage_rows(d) % 16 == 0 && hdb_mfma_f8_lds_stage_rows(d) > 0 && hdb_mfma_f8_lds_bytes(d) <= 160 * 1024, "d %d: the default waves", d);
        for (int waves : {4, 8}) {
            const int rows = hdb_mfma_f8_lds_stage_rows(d, waves), bytes = hdb_mfma_f8_lds_bytes(d, waves);
            CHECK(rows > 0 && rows % 16 == 0, "d %d, %d waves: %d rows", d, waves, rows);
            CHECK(bytes == 2 * rows * 2 * d && bytes <= 160 * 1024, "d %d, %d waves: %d bytes", d, waves, bytes);
            const int w = hdb_mfma_f8_lds_waves(waves, d);                         // (d = 512: four waves whatever is asked for)
            CHECK(w == (d == 512 ? 4 : waves), "d %d, %d waves asked: %d", d, waves, w);
            CHECK(hdb_mfma_f8_lds_wg_per_cu(d, waves) * bytes <= 160 * 1024 && hdb_mfma_f8_lds_wg_per_cu(d, waves) * w <= 8, "d %d, %d waves: the workgroups of a CU", d, waves);
            CHECK(rows * (d / 16) == hdb_mfma_f8_lds_chunks(d) * 64 * w, "d %d, %d waves: whole pieces per thread", d, waves);
            CHECK(hdb_mfma_f8_lds_blocks(1251, d, waves, 8) == 8 && hdb_mfma_f8_lds_blocks(1, d, waves, 512) == 1 &&
                  hdb_mfma_f8_lds_blocks(1251, d, waves, 1 << 20) == (1251 + rows / 16 - 1) / (rows / 16), "d %d, %d waves: the grid", d, waves);
        }
        CHECK(hdb_mfma_f8_lds_waves(4) == 4 && hdb_mfma_f8_lds_waves(8) == 8 && hdb_mfma_f8_lds_waves(0) == HDB_F8_LDS_WAVES && hdb_mfma_f8_lds_waves(5) == HDB_F8_LDS_WAVES, "waves");
    }
    CHECK(hdb_options().f8_lds_min_q == 0, "the option is off by default");

    // ---- 2, 3, 4: the planner ----
    long plans = 0, taken = 0;
    const int ds[] = {128, 256, 384, 512, 640, 1280, 4096, 600, 96};
    const int nqs[] = {1, 4, 5, 8, 9, 16, 33, 130, 300};
    const int64_t ns[] = {300, 8192, 8193, 20003, 1000000, 10000000};
    const int ks[] = {1, 100, 129, 2049};
    const int64_t opts[] = {0, 5, 9, 33, 3, -1};
    const int dtypes[] = {HDB_F8E4M3, HDB_BF16, HDB_F16, HDB_F32};
    for (int64_t opt : opts) for (int variant = 0; variant < 5; ++variant) for (int dtype : dtypes) {
        if (dtype != HDB_F8E4M3 && (opt != 5 || variant > 1)) continue;             // (the other dtypes under 5, plain and with the slices' option)
        for (int d : ds) for (int64_t n : ns) for (int nq : nqs) for (int k : ks)
        for (int metric = HDB_DOT; metric <= HDB_PEARSON; ++metric) for (int aux = 0; aux < 4; ++aux) for (int fin = 0; fin < 2; ++fin) for (int exact = 0; exact < 2; ++exact) {
            hdb_options o;
            if (variant == 1) o.f8_ks_min_q = 5;                                   // the K slices, from 5 queries on
            if (variant == 2) { o.f8_ks_min_q = 16; o.mfma_min_q = 9; }            // ... from 16, the matrix cores from 9
            if (variant == 3) { o.subset_min_n = 0; o.f8_ks_min_q = 5; }           // the row list wherever the ratio admits it
            if (variant == 4) { o.use_mfma = 0; o.use_fused = 0; o.use_l1_tile = 0; o.f8_ks_min_q = 5; }
            TopkFacts f{};
            f.n = n; f.d = d; f.dtype = dtype; f.cus = 256; f.qmode = HDB_QUANT_NONE; f.has_bias = (aux & 1) != 0; f.has_mask = (aux & 2) != 0;
            if (variant == 3 && f.has_mask) f.subset_m = n / 3 > 1000 ? 1000 : n / 3;
            const TopkCall c{nq, k, metric, true, exact != 0};
            const TopkPlan off = plan_topk(f, o, c, [&] { return fin != 0; });
            o.f8_lds_min_q = opt;
            int asked = 0, asked_off = 0;
            const TopkPlan p = plan_topk(f, o, c, [&] { ++asked; return fin != 0; });
            { hdb_options o0 = o; o0.f8_lds_min_q = 0; (void)plan_topk(f, o0, c, [&] { ++asked_off; return fin != 0; }); }
            plans += 2;
#define WHERE "f8_lds_min_q %lld variant %d dtype %d d %d n %lld nq %d k %d metric %d aux %d finite %d exact %d", (long long)opt, variant, dtype, d, (long long)n, nq, k, metric, aux, fin, exact
            CHECK(!off.f8_lds && off.stats.f8_lds == 0, WHERE);
            const bool mm = metric == HDB_DOT || metric == HDB_COSINE || metric == HDB_EUCLIDEAN || metric == HDB_PEARSON;
            const int64_t mq = std::max<int64_t>(o.mfma_min_q, 5);
            const int64_t rule = opt > 0 ? opt : opt < 0 ? hdb_mfma_f8_lds_min_q(d) : 0;
            const int64_t first = rule > 0 ? std::max<int64_t>(mq, rule) : 0;
            const int64_t ks_first = o.f8_ks_min_q > 0 ? std::max<int64_t>(mq, o.f8_ks_min_q) : 0;
            // where the float8 matrix cores run at all, spelled out from the facts: the widths, the batch size, the metric, the rows
            const bool cores = dtype == HDB_F8E4M3 && o.use_mfma && mm && n > HDB_CAND_CAP && fin && !p.subset &&
                               ((whole_width(d) && nq >= mq) || (sliced_width(d) && ks_first > 0 && nq >= ks_first));
            CHECK(p.mfma == cores || dtype != HDB_F8E4M3, WHERE);
            const bool want = cores && first > 0 && nq >= first && k <= HDB_MAX_K;
            CHECK(p.f8_lds == want && p.stats.f8_lds == (want ? 1 : 0), WHERE);
            if (want) { ++taken; CHECK(p.path == HDB_PATH_PIPELINE && p.mfma && p.stats.mfma == 1 && p.tile_rows == 16 && !p.small && !p.subset, WHERE); }
            if (dtype != HDB_F8E4M3 || n <= HDB_CAND_CAP || p.subset || !fin || metric == HDB_MANHATTAN || metric == HDB_HAMMING || metric == HDB_JACCARD || nq < 5)
                CHECK(!p.f8_lds, WHERE);
            TopkPlan q = p; q.f8_lds = false; q.stats.f8_lds = 0;
            CHECK_SAME_PLAN(q, off, WHERE);                                        // nothing else changes (f8_lds and stats.f8_lds: reset above) ...
            CHECK(asked == asked_off, WHERE);                                      // ... and the matrix is asked about as often
        }
    }
    CHECK(taken > 1000, "the sweep reached the LDS flavour %ld times", taken);
    // -1 follows the rule of the width: never where it returns 0
    for (int d : {128, 256, 384, 512, 768}) {
        hdb_options o; o.f8_lds_min_q = -1; o.f8_ks_min_q = 5;
        TopkFacts f{};
        f.n = 20003; f.d = d; f.dtype = HDB_F8E4M3; f.cus = 256; f.qmode = HDB_QUANT_NONE;
        const int r = hdb_mfma_f8_lds_min_q(d);
        CHECK(r == 0 || r >= 5, "d %d: the rule is %d", d, r);
        CHECK(f8_lds_first_q(o, HDB_F8E4M3, d) == (r > 0 ? std::max(5, r) : 0) && f8_lds_first_q(o, HDB_BF16, d) == 0, "d %d: the stat", d);
        for (int nq : {5, 64, 256}) {
            const TopkPlan p = plan_topk(f, o, TopkCall{nq, 50, HDB_COSINE, true, false}, [] { return true; });
            ++plans;
            CHECK(p.mfma && p.f8_lds == (r > 0 && nq >= std::max(5, r)), "d %d, %d queries under the measured rule %d", d, nq, r);
        }
    }
    std::printf("plans %ld\n", plans);
    return check_done();
}
