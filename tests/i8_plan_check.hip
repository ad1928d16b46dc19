// i8_plan_check.hip -- what the host side of the library says about int8 matrices (HDB_I8 = 7): a stand-alone program, no GPU call.
// 1) the element: hdb_elem_bytes(7) == 1, codes 4 / 6 / 9 have no size; hdb_i8_to_f and hdb_i8_cvt widen each of the 256 codes to
//    its integer, and the upper 16 bits of that float32 -- a bfloat16 -- carry the whole value (the low 16 are zero), which is what
//    lets the matrix-core kernel take the upper halves as its A fragment;
// 2) the capability rules (csrc/hdb_caps.h) answer for int8 what they answer for float8 at every width: matrix cores at d = 128 /
//    256 / 384 / 512 in 16-row tiles, no padded widths, no K slices, no single launch, no tile kernel, the byte-sized scan grid;
// 3) plan_topk (csrc/hdb_plan.h) over the float8 check's grid of n x d x nq x k x metric x bias / mask x finite x exact x options:
//    every int8 plan equals, field for field, the plan of a float8 matrix of the same shape whose two opt-ins (f8_ks_min_q,
//    f8_lds_min_q) are 0 -- whatever the int8 index's own values of those two options are; never K slices, never the LDS flavour.
// Prints "plans N" and "F failures"; exit status 1 on any failure.
#include "plan_check.h"
#include <cstdio>
#include <cstring>

int main() {
    // ---- 1: the element ----
    CHECK(HDB_I8 == 7 && hdb_elem_bytes(HDB_I8) == 1 && sizeof(hdb_i8) == 1, "one byte per element");
    CHECK(hdb_elem_bytes(4) == 0 && hdb_elem_bytes(6) == 0 && hdb_elem_bytes(9) == 0 && hdb_elem_bytes(8) == 0 && hdb_elem_bytes(-1) == 0, "unassigned codes have no size");
    CHECK(hdb_elem_bytes(HDB_F16) == 2 && hdb_elem_bytes(HDB_F32) == 4 && hdb_elem_bytes(HDB_F64) == 8 && hdb_elem_bytes(HDB_BF16) == 2 &&
          hdb_elem_bytes(HDB_F8E4M3) == 1, "the other sizes stay");
    for (int code = 0; code < 256; ++code) {
        const int want = code < 128 ? code : code - 256;
        hdb_i8 e;
        const unsigned char byte = (unsigned char)code;
        std::memcpy(&e, &byte, 1);
        const float got = hdb_i8_to_f(e);
        CHECK(got == (float)want, "code %d widens to %g, not %d", code, (double)got, want);
        uint32_t bits;
        std::memcpy(&bits, &got, 4);
        CHECK((bits & 0xFFFFu) == 0u, "code %d: the low 16 bits of its float32 are %04x", code, bits & 0xFFFFu);
        const uint32_t upper = bits & 0xFFFF0000u;
        float back;
        std::memcpy(&back, &upper, 4);
        CHECK(back == (float)want, "code %d: the upper half alone is %g", code, (double)back);
        CHECK(hdb_bf16_to_f(hdb_bf16{(unsigned short)(bits >> 16)}) == (float)want, "code %d as a bfloat16", code);
        // the word form the kernels convert with, at each of the four byte positions, whatever the other bytes hold
        const uint32_t fill = 0xA55A3CC3u;
        const int w0 = (int)((fill & ~0xFFu) | (uint32_t)code), w1 = (int)((fill & ~0xFF00u) | ((uint32_t)code << 8));
        const int w2 = (int)((fill & ~0xFF0000u) | ((uint32_t)code << 16)), w3 = (int)((fill & ~0xFF000000u) | ((uint32_t)code << 24));
        CHECK(hdb_i8_cvt<0>(w0) == (float)want && hdb_i8_cvt<1>(w1) == (float)want && hdb_i8_cvt<2>(w2) == (float)want && hdb_i8_cvt<3>(w3) == (float)want,
              "code %d at the four byte positions", code);
    }

    // ---- 2: the capability rules: float8's answers ----
    for (int d = 1; d <= 4096; ++d) {
        const bool wd = d == 128 || d == 256 || d == 384 || d == 512;
        CHECK(hdb_mfma_tile_rows(HDB_I8, d) == (wd ? 16 : 0) && hdb_mfma_tile_rows(HDB_I8, d) == hdb_mfma_tile_rows(HDB_F8E4M3, d), "d %d", d);
        CHECK(hdb_mfma_anyd_pad(HDB_I8, d) == 0 && hdb_mfma_ksplit_slices(HDB_I8, d) == 0, "d %d", d);
        CHECK(hdb_mfma_batch_capacity(HDB_I8, d) == 0 && !hdb_l1_tile_supported(HDB_I8, d), "d %d", d);
        for (int metric = HDB_DOT; metric <= HDB_PEARSON; ++metric) {
            CHECK(hdb_mfma_supported(HDB_I8, d, metric) == hdb_mfma_supported(HDB_F8E4M3, d, metric), "d %d metric %d", d, metric);
            CHECK(!hdb_mfma_fused_supported(HDB_I8, d, metric, 1, 100), "d %d metric %d", d, metric);
        }
        for (int vec = 0; vec < 2; ++vec)
            CHECK(hdb_scan_auto_blocks(HDB_I8, d, vec != 0, false) == hdb_scan_auto_blocks(HDB_F8E4M3, d, vec != 0, false), "%d-byte rows", d);
    }
    CHECK(hdb_scan_auto_blocks(HDB_I8, 256, true, false) == 1024 && hdb_scan_auto_blocks(HDB_I8, 384, true, false) == 1024 &&
          hdb_scan_auto_blocks(HDB_I8, 512, true, false) == 768 && hdb_scan_auto_blocks(HDB_I8, 272, true, false) == 512, "the byte-sized grid");
    CHECK(f8_lds_first_q(hdb_options{}, HDB_I8, 384) == 0, "no LDS flavour");
    { hdb_options o; o.f8_lds_min_q = -1; o.f8_ks_min_q = -1; CHECK(f8_lds_first_q(o, HDB_I8, 384) == 0, "no LDS flavour on request either"); }

    // ---- 3: the planner: the float8 plan with the two float8 opt-ins at 0 ----
    long plans = 0, on_mfma = 0;
    const int ds[] = {7, 100, 128, 256, 272, 384, 512, 768, 1024};
    const int nqs[] = {1, 2, 4, 5, 8, 16, 130, 300};
    const int64_t ns[] = {1, 300, 8192, 8193, 20003, 60001, 1000000, 10000000};
    const int ks[] = {1, 100, 128, 129, 2049, 9000};
    for (int variant = 0; variant < 5; ++variant) for (int d : ds) for (int64_t n : ns) for (int nq : nqs) for (int k : ks)
    for (int metric = HDB_DOT; metric <= HDB_PEARSON; ++metric) for (int aux = 0; aux < 4; ++aux) for (int fin = 0; fin < 2; ++fin) for (int exact = 0; exact < 2; ++exact) {
        hdb_options o;
        if (variant == 1) o.quant_min_n = 0;                                   // "a shadow for every size": still none
        if (variant == 2) { o.subset_min_n = 0; }                              // the row list wherever the ratio admits it
        if (variant == 3) { o.use_mfma = 0; o.use_fused = 0; o.use_l1_tile = 0; }
        if (variant == 4) { o.f8_ks_min_q = -1; o.f8_lds_min_q = -1; }         // the float8 opt-ins set on the int8 index: ignored
        TopkFacts f{};
        f.n = n; f.d = d; f.dtype = HDB_I8; f.cus = 256; f.qmode = HDB_QUANT_NONE; f.has_bias = (aux & 1) != 0; f.has_mask = (aux & 2) != 0;
        if (variant == 2 && f.has_mask) f.subset_m = n / 3 > 1000 ? 1000 : n / 3;
        const TopkCall c{nq, k, metric, true, exact != 0};
        int asked = 0, asked8 = 0;
        const TopkPlan p = plan_topk(f, o, c, [&] { ++asked; return fin != 0; });
        TopkFacts f8 = f; f8.dtype = HDB_F8E4M3;
        hdb_options o8 = o; o8.f8_ks_min_q = 0; o8.f8_lds_min_q = 0;
        const TopkPlan b = plan_topk(f8, o8, c, [&] { ++asked8; return fin != 0; });
        ++plans;
#define WHERE "variant %d d %d n %lld nq %d k %d metric %d aux %d finite %d exact %d", variant, d, (long long)n, nq, k, metric, aux, fin, exact
        CHECK_SAME_PLAN(p, b, WHERE);
        CHECK(asked == asked8, WHERE);
        CHECK(!p.shadow() && !p.ksplit && !p.f8_lds && !p.l1tile && p.ld_ks == 0 && p.path != HDB_PATH_FUSED && p.path != HDB_PATH_BATCH1, WHERE);
        const bool wd = d == 128 || d == 256 || d == 384 || d == 512;
        const bool mm = metric == HDB_DOT || metric == HDB_COSINE || metric == HDB_EUCLIDEAN || metric == HDB_PEARSON;
        CHECK(p.mfma == (o.use_mfma && mm && nq >= 5 && wd && n > HDB_CAND_CAP && !p.subset && fin), WHERE);
        if (p.mfma) ++on_mfma;
    }
    CHECK(on_mfma > 1000, "the grid reaches the matrix cores (%ld plans)", on_mfma);
    std::printf("plans %ld\n", plans);
    return check_done();
}
