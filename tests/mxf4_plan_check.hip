// mxf4_plan_check.hip -- MXFP4 matrices (HDB_MXF4 = 13) on the host, no GPU call: the row pitch by hand (0 for d % 32 != 0, 11 and 12
// unassigned) and plan_topk for every d <= 8192 and metric: never the matrix cores, a float single launch, the tile kernel, the row list or a shadow.
#include "plan_check.h"

int main() {
    CHECK(HDB_MXF4 == 13 && hdb_elem_bytes(HDB_MXF4) == 0 && hdb_elem_bytes(11) == 0 && hdb_elem_bytes(12) == 0, "sub-byte, and 11 / 12 unassigned");
    CHECK(hdb_row_bytes(13, 32) == 32 && hdb_row_bytes(13, 384) == 208 && hdb_row_bytes(13, 512) == 272 && hdb_row_bytes(13, 1024) == 544, "pitches by hand");
    for (int d = -1; d <= 8192; ++d) {
        CHECK(hdb_row_bytes(11, d) == 0 && hdb_row_bytes(12, d) == 0, "unassigned codes, d %d", d);
        if (d <= 0 || d % 32 != 0) { CHECK(hdb_row_bytes(13, d) == 0 && hdb_f4scan_qt(d, 4) < 0, "d %d is no row", d); continue; }
        const int64_t rb = hdb_row_bytes(13, d);
        CHECK(rb % 16 == 0 && rb >= d / 2 + d / 32 && rb < d / 2 + d / 32 + 16, "d %d: pitch %lld", d, (long long)rb);
    }
    long plans = 0;
    const int nqs[] = {1, 4, 5, 64};
    const int64_t ns[] = {300, 20003, 10000000};
    const int ks[] = {100, 3000};
    for (int d = 32; d <= 8192; d += 32) for (int metric = HDB_DOT; metric <= HDB_PEARSON; ++metric)
    for (int64_t n : ns) for (int nq : nqs) for (int k : ks) for (int aux = 0; aux < 4; ++aux) for (int variant = 0; variant < 2; ++variant) {
        hdb_options o;
        if (variant == 1) { o.quant_min_n = 0; o.subset_min_n = 0; o.b1_mfma_min_q = -1; o.f8_ks_min_q = -1; o.f8_lds_min_q = -1; o.bf16_quant = 1; o.mfma_min_q = 1; }
        TopkFacts f{};
        f.n = n; f.d = d; f.dtype = HDB_MXF4; f.cus = 256; f.qmode = HDB_QUANT_NONE; f.has_bias = (aux & 1) != 0; f.has_mask = (aux & 2) != 0;
        if (f.has_mask) f.subset_m = n / 64;
        const TopkPlan p = plan_topk(f, o, TopkCall{nq, k, metric, true, false}, [] { return true; });
        ++plans;
#define WHERE "variant %d d %d n %lld nq %d k %d metric %d aux %d", variant, d, (long long)n, nq, k, metric, aux
        CHECK(!p.mfma && !p.shadow() && !p.plane_wanted && !p.build_needed && !p.l1tile && !p.subset && !p.ksplit && !p.f8_lds && !p.f32s && !p.local, WHERE);
        CHECK(p.path != HDB_PATH_FUSED && p.path != HDB_PATH_BATCH1 && p.path != HDB_PATH_QUANT && (p.path != HDB_PATH_BITS1 || is_bits_metric(metric)), WHERE);
        CHECK(p.stats.mfma == 0 && p.stats.quant == 0 && p.stats.subset == 0 && (p.stats.fused == 0 || p.stats.fused == 3), WHERE);
    }
    std::printf("plans %ld\n", plans);
    return check_done();
}
