// b1_plan_check.hip -- what the host side of the library says about packed-bit matrices (HDB_B1 = 10): a stand-alone program, no GPU call.
// 1) the row pitch: hdb_row_bytes(dtype, d) equals d * hdb_elem_bytes(dtype) wherever that is non-zero, is d / 8 for dtype 10 at
//    whole 32-bit words, and 0 for unassigned codes and for d % 32 != 0; hdb_elem_bytes(10) stays 0 (a bit has no whole-byte size);
// 2) the capability rules (csrc/hdb_caps.h): no matrix cores, no padded widths, no K slices, no single launch, no tile kernel at any
//    width; the QT rule of hdb_bscan.hip keeps the tables of a pass inside the LDS it claims at every width hdb_index_create
//    admits (d % 32 == 0, 8 d <= 60 KiB), with two workgroups per CU beside their survivor stages;
// 3) plan_topk (csrc/hdb_plan.h) over the int8 check's grid of n x d (multiples of 32) x nq x k x metric x bias / mask x exact x
//    options: every HDB_B1 plan has mfma = quant = plane = l1tile = subset = 0 and fused in {0, 3}; for the bit metrics it equals,
//    field for field, the plan of an int8 matrix of the same shape; for the other metrics it equals the int8 plan made with
//    use_mfma = 0.  (A row list set on the index changes nothing: the B1 plan is compared with the int8 plan WITHOUT a list.)
// Prints "plans N" and "F failures"; exit status 1 on any failure.
#include "plan_check.h"
#include <cstdio>
#include <cstring>

int main() {
    // ---- 1: the row pitch ----
    CHECK(HDB_B1 == 10 && hdb_elem_bytes(HDB_B1) == 0, "a bit has no whole-byte size");
    CHECK(hdb_elem_bytes(4) == 0 && hdb_elem_bytes(6) == 0 && hdb_elem_bytes(8) == 0 && hdb_elem_bytes(9) == 0 && hdb_elem_bytes(-1) == 0, "unassigned codes have no size");
    for (int dtype = -1; dtype <= 12; ++dtype) for (int d = 1; d <= 8192; ++d) {
        const int64_t rb = hdb_row_bytes(dtype, d);
        if (dtype == HDB_B1) CHECK(rb == (d % 32 == 0 ? d / 8 : 0), "dtype 10 d %d: %lld", d, (long long)rb);
        else CHECK(rb == (int64_t)d * hdb_elem_bytes(dtype), "dtype %d d %d: %lld", dtype, d, (long long)rb);
        if (dtype == 4 || dtype == 6 || dtype == 8 || dtype == 9 || dtype < 0 || dtype > 10) CHECK(rb == 0, "unassigned code %d d %d", dtype, d);
    }
    CHECK(hdb_row_bytes(HDB_F16, 384) == 768 && hdb_row_bytes(HDB_F64, 3) == 24 && hdb_row_bytes(HDB_I8, 100) == 100 && hdb_row_bytes(HDB_B1, 384) == 48 &&
          hdb_row_bytes(HDB_B1, 32) == 4 && hdb_row_bytes(HDB_B1, 96) == 12 && hdb_row_bytes(HDB_B1, 48) == 0 && hdb_row_bytes(HDB_B1, 0) == 0 &&
          hdb_row_bytes(HDB_F32, -4) == 0, "pitches by hand");

    // ---- 2: the capability rules ----
    for (int d = 1; d <= 8192; ++d) {
        CHECK(hdb_mfma_tile_rows(HDB_B1, d) == 0 && hdb_mfma_anyd_pad(HDB_B1, d) == 0 && hdb_mfma_ksplit_slices(HDB_B1, d) == 0, "d %d", d);
        CHECK(hdb_mfma_batch_capacity(HDB_B1, d) == 0 && !hdb_l1_tile_supported(HDB_B1, d), "d %d", d);
        for (int metric = HDB_DOT; metric <= HDB_PEARSON; ++metric) {
            CHECK(!hdb_mfma_supported(HDB_B1, d, metric), "d %d metric %d", d, metric);
            for (int nq = 1; nq <= 4; ++nq) CHECK(!hdb_mfma_fused_supported(HDB_B1, d, metric, nq, 100), "d %d metric %d", d, metric);
        }
        CHECK(f8_lds_first_q(hdb_options{}, HDB_B1, d) == 0, "d %d: no LDS flavour", d);
        // the QT rule: a width hdb_index_create admits has a kernel, and that kernel's tables fit the LDS the rule claims
        const bool admitted = d % 32 == 0 && (int64_t)d * 8 <= 60 * 1024;
        const int qt = hdb_bscan_qt(d);
        if (!admitted) { CHECK(d % 32 != 0 ? qt < 0 : true, "d %d is no row", d); continue; }
        CHECK(qt == 0 || qt == 1 || qt == 2 || qt == 4, "d %d: %d queries per pass", d, qt);
        const int lds = hdb_bscan_lds_bytes(d, qt);
        CHECK(lds == (qt > 0 ? qt * 16 * d : 8 * d) && lds <= HDB_BSCAN_TABLE_BYTES, "d %d qt %d: %d bytes of tables", d, qt, lds);
        CHECK(2 * (lds + 5 * 1024) <= 160 * 1024, "d %d: two workgroups per CU", d);
        // the largest QT that fits is the one taken; every smaller launch (fewer queries than QT) fits a fortiori
        if (qt > 0 && qt < 4) CHECK((int64_t)(2 * qt) * 16 * d > HDB_BSCAN_TABLE_BYTES, "d %d: %d queries per pass leave room for more", d, qt);
        if (qt == 0) CHECK((int64_t)16 * d > HDB_BSCAN_TABLE_BYTES, "d %d: one table would fit", d);
        const int blocks = hdb_bscan_auto_blocks(d, qt, 256);
        CHECK(blocks >= 256 && blocks <= 8 * 256 && (int64_t)(blocks / 256) * (lds + 5 * 1024) <= 160 * 1024, "d %d: %d workgroups", d, blocks);
    }
    CHECK(hdb_bscan_qt(32) == 4 && hdb_bscan_qt(384) == 4 && hdb_bscan_qt(960) == 4 && hdb_bscan_qt(992) == 2 && hdb_bscan_qt(1024) == 2 &&
          hdb_bscan_qt(1920) == 2 && hdb_bscan_qt(1952) == 1 && hdb_bscan_qt(3840) == 1 && hdb_bscan_qt(3872) == 0 && hdb_bscan_qt(4128) == 0 &&
          hdb_bscan_qt(7680) == 0 && hdb_bscan_qt(7712) < 0 && hdb_bscan_qt(48) < 0, "the cuts of the QT rule");

    // ---- 3: the planner ----
    long plans = 0, sampled = 0, fused3 = 0;
    const int ds[] = {32, 96, 128, 256, 384, 512, 768, 1024, 4128};
    const int nqs[] = {1, 2, 4, 5, 8, 16, 130, 300};
    const int64_t ns[] = {1, 300, 8192, 8193, 20003, 60001, 1000000, 10000000};
    const int ks[] = {1, 100, 128, 129, 2049, 9000};
    for (int variant = 0; variant < 5; ++variant) for (int d : ds) for (int64_t n : ns) for (int nq : nqs) for (int k : ks)
    for (int metric = HDB_DOT; metric <= HDB_PEARSON; ++metric) for (int aux = 0; aux < 4; ++aux) for (int fin = 0; fin < 2; ++fin) for (int exact = 0; exact < 2; ++exact) {
        hdb_options o;
        if (variant == 1) o.quant_min_n = 0;                                   // "a shadow for every size": still none
        if (variant == 2) { o.subset_min_n = 0; }                              // the row list wherever the ratio admits it: never here
        if (variant == 3) { o.use_mfma = 0; o.use_fused = 0; o.use_l1_tile = 0; }
        if (variant == 4) { o.f8_ks_min_q = -1; o.f8_lds_min_q = -1; o.bf16_quant = 1; o.auto_quant = 1; }
        TopkFacts f{};
        f.n = n; f.d = d; f.dtype = HDB_B1; f.cus = 256; f.qmode = HDB_QUANT_NONE; f.has_bias = (aux & 1) != 0; f.has_mask = (aux & 2) != 0;
        if (variant == 2 && f.has_mask) f.subset_m = n / 3 > 1000 ? 1000 : n / 3;
        const TopkCall c{nq, k, metric, true, exact != 0};
        const TopkPlan p = plan_topk(f, o, c, [&] { return fin != 0; });
        TopkFacts f8 = f; f8.dtype = HDB_I8; f8.subset_m = 0;
        hdb_options o8 = o;
        const bool bitm = is_bits_metric(metric);
        if (!bitm) o8.use_mfma = 0;
        const TopkPlan b = plan_topk(f8, o8, c, [&] { return fin != 0; });
        ++plans;
#define WHERE "variant %d d %d n %lld nq %d k %d metric %d aux %d finite %d exact %d", variant, d, (long long)n, nq, k, metric, aux, fin, exact
        CHECK(!p.mfma && !p.shadow() && !p.plane_wanted && !p.build_needed && !p.l1tile && !p.subset && !p.ksplit && !p.f8_lds && !p.f32s && !p.local, WHERE);
        CHECK(p.stats.mfma == 0 && p.stats.quant == 0 && p.stats.plane == 0 && p.stats.subset == 0 && p.stats.f8_lds == 0, WHERE);
        CHECK(p.stats.fused == 0 || p.stats.fused == 3, WHERE);
        CHECK(p.path != HDB_PATH_FUSED && p.path != HDB_PATH_BATCH1 && p.path != HDB_PATH_QUANT && (p.path != HDB_PATH_BITS1 || bitm), WHERE);
        CHECK_SAME_PLAN(p, b, WHERE);
        if (p.stats.path == 1 && !bitm) ++sampled;
        if (p.stats.fused == 3) ++fused3;
    }
    CHECK(sampled > 1000 && fused3 > 1000, "the grid reaches the sampled pipeline (%ld plans) and the bit metrics' single launch (%ld)", sampled, fused3);
    std::printf("plans %ld\n", plans);
    return check_done();
}
