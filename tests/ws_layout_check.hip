// ws_layout_check.hip -- host program of tests/test_ws_layout.py: runs the workspace layouts of csrc/hdb_ws.h over a grid of shapes.
// No GPU call is made.  The program states, for every pointer of a layout, the bytes its users need there (the kernels' extents);
// the region of a pointer runs to the next pointer placed (or to the reported size).  For every point and layout: each region is
// 256-byte aligned, holds the bytes stated, regions follow one another without overlap inside the size the dry run reported, the
// shadow layouts are sized by plans that do not depend on k and hold the sample of every k, and no layout needs more bytes than the
// byte formula it replaced (the formulas of the previous hdb_api.hip, copied below as the reference number).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <utility>
#include <sys/mman.h>

#include "hdb_ws.h"
#include "../include/hyperdb_hip.h"
#include "plan_check.h"

static long g_points = 0;

static const size_t RESERVE = (size_t)64 << 30;     // address space only: never touched
static char* g_base = nullptr;

// ---- the byte formulas the layouts replaced ---------------------------------------------------------------------------------
static size_t old_scores_need(int d, int W) { return 8192 + (size_t)W * 4 + (size_t)d * 8; }
static size_t old_topk_need(int nq, int d, int W, int cq_max, int64_t ld_scores, int64_t ld_ks, int64_t sort_n, size_t tb) {
    size_t need = 0;
    need += 4 * align_up((size_t)nq * 4, 256) + 1024;
    need += align_up((size_t)nq * W * 4, 256);
    need += align_up((size_t)nq * d * 2, 256);
    need += align_up((size_t)nq * d * 8, 256);
    need += align_up((size_t)cq_max * 4, 256) + align_up((size_t)cq_max * 4 * HDB_CNT_STRIDE, 256) + 256;
    need += align_up((size_t)cq_max * 4 * HDB_RADIX_BINS * 4, 256);
    need += align_up((size_t)cq_max * 16, 256);
    need += align_up((size_t)cq_max * HDB_CAND_CAP * 8, 256);
    need += align_up((size_t)cq_max * ld_scores * 4, 256) + 4096;
    if (ld_ks > 0) need += align_up((size_t)cq_max * ld_ks * 4, 256);
    if (sort_n > 0) need += align_up((size_t)sort_n * 4, 256) + align_up((size_t)sort_n * 16, 256) + align_up(tb, 256) + 4096;
    return need;
}
static size_t old_quant_need(int nq, int P, int d, int64_t ld_s, uint32_t pl_cap, bool mflavour) {
    size_t need = 8 * align_up((size_t)nq * 4, 256) + 4096;
    need += align_up((size_t)nq * P, 256) + align_up((size_t)nq * HDB_QQ_WORDS * 4, 256);
    need += align_up((size_t)nq * 4 * HDB_CNT_STRIDE, 256) + 256;
    need += align_up((size_t)nq * HDB_CAND_CAP * 8, 256) + align_up((size_t)nq * ld_s * 4, 256);
    if (pl_cap) need += align_up((size_t)pl_cap * 4, 256) + 256;
    if (mflavour) {
        const size_t crow = (size_t)nq * HDB_CAND_CAP;
        need += align_up((size_t)nq * d * 2, 256) + 256;
        need += align_up((size_t)nq * HDB_QUANT_NSUB_MAX * 4, 256);
        need += align_up(crow * d * 2, 256) + 2 * align_up(crow * 4, 256) + align_up((size_t)nq * crow * 4, 256);
    }
    return need;
}
static size_t old_quant_batch_need(int cq, int P, int d, int64_t ld_s, int64_t wld) {
    size_t need = 8 * align_up((size_t)cq * 4, 256) + 4096;
    need += align_up((size_t)cq * P, 256) + align_up((size_t)cq * HDB_QQ_WORDS * 4, 256);
    need += align_up((size_t)cq * 4 * HDB_CNT_STRIDE, 256) + 256;
    need += align_up((size_t)cq * HDB_CAND_CAP * 8, 256);
    need += align_up((size_t)cq * d * 2, 256);
    need += align_up(std::max((size_t)cq * wld, (size_t)4 * ld_s) * 4, 256);
    return need;
}

// ---- extents --------------------------------------------------------------------------------------------------------------------
// The shadow layouts take theirs from the sample plans of hdb_ws.h itself.  The main pipeline's plan needs the index (sample_plan,
// hdb_api.hip); TopkWs must hold for any extents, so a stand-in of the same shape picks representative ones.
static int64_t ld_of_rows(int64_t rows) { return (int64_t)align_up((size_t)std::max<int64_t>(rows, 4), 4); }
static int64_t topk_sample_rows(int64_t n, uint32_t kk, int nq, int tile_rows) {
    const int64_t T = kk <= 128 ? (nq >= 32 ? 1024 : 2048) : 4096;
    const uint32_t m = kk <= 128 ? 8u : (kk <= 512 ? 64u : 256u);
    int64_t rows = std::max<int64_t>((int64_t)((double)m * (double)n / (double)T), 16 * (int64_t)m);
    const int64_t tiles = std::min((rows + tile_rows - 1) / tile_rows, n / tile_rows);
    return tiles * tile_rows;
}

// ---- one layout at one point ------------------------------------------------------------------------------------------------
// `need`: (pointer the layout placed, bytes its users need there), in the order of the takes; nullptr = a region this flag combination
// does not take (then no bytes may be needed).
typedef std::vector<std::pair<const void*, size_t>> Needs;
template <typename WS, typename Collect, typename... Ext>
static size_t check_layout(const char* what, size_t old_need, Collect collect, Ext... ext) {
    const size_t size = ws_bytes_for<WS>(ext...);
    CHECK(size <= old_need, "%s: %zu bytes, the formula it replaces needs %zu", what, size, old_need);
    CHECK(size <= RESERVE, "%s: %zu bytes exceed the test's address-space reservation", what, size);
    if (size > RESERVE) return size;
    WS w; Bump b(g_base, size);
    w.lay(b, ext...);
    CHECK(b.off == size && b.off <= b.cap, "%s: the placing run ends at %zu, the dry run at %zu", what, b.off, size);
    Needs need;
    collect(w, need);
    size_t end = 0, placed = 0;          // end of the bytes needed so far
    for (size_t i = 0; i < need.size(); ++i) {
        if (!need[i].first) { CHECK(need[i].second == 0, "%s: pointer %zu is null, %zu bytes are needed there", what, i, need[i].second); continue; }
        const size_t off = (size_t)((const char*)need[i].first - g_base), bytes = need[i].second;
        CHECK((const char*)need[i].first >= g_base && off % 256 == 0, "%s: region %zu at offset %zu is not 256-byte aligned", what, i, off);
        CHECK(bytes > 0, "%s: region %zu is empty", what, i);
        CHECK(off >= end, "%s: region %zu at %zu overlaps its predecessor, which needs the bytes up to %zu", what, i, off, end);
        CHECK(off + bytes <= size, "%s: region %zu needs the bytes up to %zu, past the reported size %zu", what, i, off + bytes, size);
        end = off + bytes;
        ++placed;
    }
    CHECK(placed > 0, "%s: no region placed", what);
    return size;
}

int main() {
    g_base = (char*)mmap(nullptr, RESERVE, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (g_base == (char*)MAP_FAILED) { std::printf("mmap failed\n"); return 2; }
    CHECK(((uintptr_t)g_base & 255) == 0, "base not aligned");
    const int nqs[] = {1, 4, 5, 256, 300};
    const int64_t ns[] = {1, 8192, 8193, 70001, 10000000};
    const int ds[] = {1, 40, 384, 4096};
    const int ks[] = {1, 128, 2049};
    const int64_t exact_bytes = (int64_t)1 << 30;
    const int64_t wld = 8192;            // slots of the batch's sample pass per query: 512 workgroups x 16
    for (int nq : nqs) for (int64_t n : ns) for (int d : ds) {
        const int W = (d + 31) / 32, P = (int)align_up((size_t)d, 16);
        const int64_t ld_n = (int64_t)align_up((size_t)n, 4);
        ++g_points;
        check_layout<ScoresWs>("scores", old_scores_need(d, W),
                               [=](const ScoresWs& w, Needs& p) { p = {{w.qinv, 4}, {w.qsq, 4}, {w.qnan, 4}, {w.qbits, (size_t)W * 4}, {w.qc, (size_t)d * 8}}; }, d, W);
        // shadow layouts: the score buffer takes the largest sample any k takes (quant_ld_max, as hdb_api.hip sizes it)
        const int64_t q_ld = quant_ld_max(n, d);
        const int64_t qb_ld = quant_batch_sample(n).ld_s;
        size_t q_size[2][2] = {{0, 0}, {0, 0}};
        for (int k : ks) {
            const uint32_t kk = (uint32_t)std::min<int64_t>(k, n);
            const bool small = n <= HDB_CAND_CAP;
            const bool full_sort = k > HDB_MAX_K && !small;
            // ---- main pipeline: exact x ksplit x matrix-core tile x full sort (small comes with n)
            for (int exact = 0; exact < 2; ++exact) for (int ksplit = 0; ksplit < 2; ++ksplit) for (int tile_rows : {16, 64}) {
                const bool ex = exact && !small;
                const int64_t ld_s = ld_of_rows((small || exact) ? 0 : topk_sample_rows(n, kk, nq, tile_rows));
                int cq = 256;
                if (ex) cq = (int)std::max<int64_t>(1, std::min<int64_t>(256, exact_bytes / (ld_n * 4)));
                if (ksplit && !small) cq = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(cq, 128), exact_bytes / (ld_n * 4)));
                cq = std::min(cq, nq);
                const int64_t ld_scores = ex ? ld_n : ld_s, ld_ks = ksplit ? ld_n : 0, sort_n = full_sort ? n : 0;
                const size_t tb = full_sort ? (size_t)n * 8 + 777 : 0;
                ++g_points;
                check_layout<TopkWs>("topk", old_topk_need(nq, d, W, cq, ld_scores, ld_ks, sort_n, tb),
                                     [=](const TopkWs& w, Needs& p) {
                                         const size_t q = (size_t)nq, c = (size_t)cq;
                                         p = {{w.qinv, q * 4}, {w.qsq, q * 4}, {w.qnan, q * 4}, {w.qscl, q * 4}, {w.qbits, q * W * 4},
                                              {w.q16, q * d * 2}, {w.qc, q * d * 8}, {w.thr, c * 4}, {w.cnt, c * HDB_CNT_STRIDE * 4},
                                              {w.tile_ctr, 256}, {w.hist, c * 4 * HDB_RADIX_BINS * 4}, {w.tie_info, c * 16},
                                              {w.cand, c * HDB_CAND_CAP * 8}, {w.sbuf, c * (size_t)ld_scores * 4}, {w.kbuf, c * (size_t)ld_ks * 4},
                                              {w.sc1, (size_t)sort_n * 4}, {w.work, (size_t)sort_n * 16}, {w.temp, tb}};
                                     },
                                     nq, d, W, cq, ld_scores, ld_ks, sort_n, tb);
            }
            // ---- 1-4-query shadow: matrix-core flavour x plane
            const QuantSample qs = quant_call_sample(n, d, kk);         // the call's own sample: its ld_s is the leading dimension in sbuf
            CHECK(qs.ld_s <= q_ld && qs.s_rows <= qs.ld_s, "the sample of k = %d (ld %ld) is larger than the one the layout is sized for (%ld)", k, (long)qs.ld_s, (long)q_ld);
            CHECK(qs.s_tiles >= 1 && (qs.s_tiles - 1) * qs.s_stride + qs.s_stride <= std::max<int64_t>(n / 16, 1), "the sample of k = %d leaves the matrix", k);
            for (int mfl = 0; mfl < 2; ++mfl) for (int plane = 0; plane < 2; ++plane) {
                const uint32_t pl_cap = plane ? (uint32_t)std::max<int64_t>(n / 8, 16) : 0;
                ++g_points;
                const size_t size = check_layout<QuantWs>("quant", old_quant_need(nq, P, d, q_ld, pl_cap, mfl != 0),
                                                          [=](const QuantWs& w, Needs& p) {
                                                              const size_t q = (size_t)nq, crow = mfl ? q * HDB_CAND_CAP : 0, mq = mfl ? q : 0;
                                                              p = {{w.qinv, q * 4}, {w.qsq, q * 4}, {w.qnan, q * 4}, {w.qcodes, q * P}, {w.qaux, q * HDB_QQ_WORDS * 4},
                                                                   {w.thr, q * 4}, {w.cnt, q * HDB_CNT_STRIDE * 4}, {w.cand, q * HDB_CAND_CAP * 8},
                                                                   {w.sbuf, q * (size_t)qs.ld_s * 4}, {w.pl_list, (size_t)pl_cap * 4},
                                                                   {w.q16, mq * d * 2}, {w.qscl, mq * 4}, {w.G, crow * d * 2}, {w.ginv, crow * 4}, {w.gbias, crow * 4},
                                                                   {w.gsc, mq * crow * 4}, {w.wmax, mq * HDB_QUANT_NSUB_MAX * 4}};
                                                          },
                                                          nq, P, d, q_ld, pl_cap, mfl != 0);
                if (k == 1) q_size[mfl][plane] = size;
                CHECK(size == q_size[mfl][plane], "quant: %zu bytes at k = %d, %zu at k = 1", size, k, q_size[mfl][plane]);
            }
        }
        // ---- shadow batch: one chunk of up to 256 queries; nothing of it depends on k
        ++g_points;
        check_layout<QuantBatchWs>("quant batch", old_quant_batch_need(std::min(nq, 256), P, d, qb_ld, wld),
                                   [=](const QuantBatchWs& w, Needs& p) {
                                       const size_t c = (size_t)std::min(nq, 256);
                                       p = {{w.qinv, c * 4}, {w.qsq, c * 4}, {w.qnan, c * 4}, {w.qscl, c * 4}, {w.qcodes, c * P}, {w.qaux, c * HDB_QQ_WORDS * 4},
                                            {w.thr, c * 4}, {w.cnt, c * HDB_CNT_STRIDE * 4}, {w.cand, c * HDB_CAND_CAP * 8}, {w.q16, c * d * 2},
                                            {w.wbuf, std::max(c * (size_t)wld, (size_t)4 * qb_ld) * 4}};       // slot maxima, or four queries' sampled bounds
                                   },
                                   std::min(nq, 256), P, d, qb_ld, wld);
    }
    std::printf("%ld layouts checked\n", g_points);
    return check_done();
}
