// mxf4_lds_plan_check.hip -- the plans of an MXFP4 matrix (HDB_MXF4) under f8_lds_min_q beside b1_mfma_min_q (csrc/hdb_plan.h, the
// hdb_mfma_f4_lds_* rules of csrc/hdb_caps.h): a stand-alone host program, no GPU call.
// The threshold is max(5, b1_mfma_min_q, f8_lds_min_q) where both options are >= 1 and the row is a whole row of 128 / 256 / 384 / 512
// elements, else 0.  p.f8_lds is true exactly where the plan WITHOUT the option is on the whole-row matrix cores, outside the full sort,
// with at least that many queries; every other member equals that plan's, and the matrix is asked whether it is finite equally often.
// Prints "plans N", "lds plans M" and "F failures"; exit status 1 on any failure.
#include "plan_check.h"

int main() {
    for (int d = 1; d <= 8192; ++d) {
        CHECK(hdb_mfma_f4_lds_supported(d) == whole_width(d) && hdb_mfma_f4_lds_min_q(d) == 0, "d %d", d);
        CHECK(hdb_mfma_f4_lds_groups(d) == (!whole_width(d) ? 0 : d == 512 ? 3 : 4), "d %d", d);
        if (!whole_width(d)) continue;
        CHECK(hdb_mfma_f4_lds_bytes(d) == d / 32 * hdb_mfma_f4_lds_groups(d) * 3072 && hdb_mfma_f4_lds_bytes(d) <= 160 * 1024, "d %d: %d bytes of LDS", d, hdb_mfma_f4_lds_bytes(d));
    }
    const int64_t tiles[] = {1, 7, 8, 9, 525, 2047, 2048, 2049, 625000};
    for (int64_t nt : tiles) for (int limit : {0, 1, 64, 1000}) {
        const int b = hdb_mfma_f4_lds_blocks(nt, 256, limit);
        CHECK(b >= 1 && b <= (limit > 0 ? limit : 256) && b <= (nt + 7) / 8 && (b == (nt + 7) / 8 || b == (limit > 0 ? limit : 256)), "tiles %lld limit %d: %d", (long long)nt, limit, b);
    }
    long plans = 0, on = 0;
    const int nqs[] = {1, 4, 5, 15, 16, 64};
    const int64_t ns[] = {300, 8192, 8389, 10000000};
    const int ks[] = {10, 3000};
    const int opts[][3] = {{5, 5, 0}, {5, 0, 0}, {0, 5, 0}, {5, -1, 0}, {-1, 5, 0}, {5, 16, 0}, {16, 5, 0}, {5, 3, 0}, {5, 5, 5}};      // b1_mfma_min_q, f8_lds_min_q, f8_ks_min_q
    for (const auto& v : opts) for (int d = 32; d <= 1024; d += 32) for (int metric = HDB_DOT; metric <= HDB_PEARSON; ++metric) for (int64_t n : ns)
    for (int nq : nqs) for (int k : ks) for (int aux = 0; aux < 4; ++aux) for (int fin = 0; fin < 2; ++fin) {
        hdb_options o, o_off;
        o.b1_mfma_min_q = o_off.b1_mfma_min_q = v[0]; o.f8_ks_min_q = o_off.f8_ks_min_q = v[2];
        o.f8_lds_min_q = v[1];
        TopkFacts f{};
        f.n = n; f.d = d; f.dtype = HDB_MXF4; f.cus = 256; f.qmode = HDB_QUANT_NONE; f.has_bias = (aux & 1) != 0; f.has_mask = (aux & 2) != 0;
        const TopkCall c{nq, k, metric, true, false};
        int asked = 0, asked_off = 0;
        TopkPlan p = plan_topk(f, o, c, [&] { ++asked; return fin != 0; });
        const TopkPlan off = plan_topk(f, o_off, c, [&] { ++asked_off; return fin != 0; });
        ++plans;
#define WHERE "options %d %d %d d %d n %lld nq %d k %d metric %d aux %d finite %d", v[0], v[1], v[2], d, (long long)n, nq, k, metric, aux, fin
        const int64_t T = (v[0] >= 1 && v[1] >= 1 && whole_width(d)) ? std::max<int64_t>(std::max<int64_t>(5, v[0]), v[1]) : 0;
        CHECK(f8_lds_first_q(o, HDB_MXF4, d) == T && f8_lds_first_q(o_off, HDB_MXF4, d) == 0, WHERE);
        const bool want = T > 0 && nq >= T && off.mfma && whole_width(d) && off.path != HDB_PATH_FULL_SORT;
        CHECK(p.f8_lds == want && p.stats.f8_lds == (want ? 1 : 0) && !off.f8_lds && off.stats.f8_lds == 0, WHERE);
        CHECK(asked == asked_off, WHERE);
        if (want) { ++on; CHECK(p.tile_rows == 16 && p.path == HDB_PATH_PIPELINE && !p.ksplit && p.stats.mfma == 1, WHERE); }
        p.f8_lds = false; p.stats.f8_lds = 0;
        CHECK_SAME_PLAN(p, off, WHERE);
    }
    CHECK(on > 500, "the grid reaches the LDS flavour (%ld plans)", on);
    std::printf("plans %ld\nlds plans %ld\n", plans, on);
    return check_done();
}
