// mmr_plan_check.hip -- host program of tests/test_mmr_host.py: how hdb_mmr cuts a call (csrc/hdb_mmr_plan.h) and the workspace of a
// chunk (MmrWs, csrc/hdb_ws.h) over a grid.  No GPU call is made.
//   plan       over (nq, m, exact_bytes): mp is m rounded up to the pair tile, tiles = mp / tile, tile pairs = tiles (tiles + 1) / 2
//              and every pair ti <= tj has one index tj (tj + 1) / 2 + ti below that count; cq = clamp(exact_bytes / (mp^2 4), 1,
//              min(nq, 256)); a chunk of more than one query keeps its pair matrices inside exact_bytes; the chunks cover nq;
//   workspace  the size the dry run reports is where the placing run ends; rows, rel, cnt and P are 256-byte aligned, hold their
//              bytes, do not overlap and lie inside the reported size.
#include <cstdio>
#include <cstdlib>
#include <sys/mman.h>

#include "hdb_mmr_plan.h"
#include "../include/hyperdb_hip.h"
#include "plan_check.h"

static long g_points = 0;

int main() {
    const size_t RESERVE = (size_t)64 << 30;     // address space only: never touched
    char* base = (char*)mmap(nullptr, RESERVE, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (base == (char*)MAP_FAILED) { std::printf("mmap failed\n"); return 2; }
    const int32_t nqs[] = {1, 2, 5, 16, 255, 256, 257, 1000};
    const int32_t ms[] = {1, 5, 15, 16, 17, 128, 257, 600, 2047, 2048};
    const int64_t ebs[] = {(int64_t)1 << 20, (int64_t)3 << 20, (int64_t)1 << 24, (int64_t)1 << 30, (int64_t)1 << 34};
    for (int32_t nq : nqs) for (int32_t m : ms) for (int64_t eb : ebs) {
        ++g_points;
        const MmrPlan p = mmr_plan(nq, m, eb);
        CHECK(p.mp >= m && p.mp < m + HDB_MMR_TILE && p.mp % HDB_MMR_TILE == 0 && p.mp == hdb_mmr_mp(m), "m %d: mp %d", m, p.mp);
        CHECK(p.tiles * HDB_MMR_TILE == p.mp && p.tile_pairs == p.tiles * (p.tiles + 1) / 2, "m %d: %d tiles, %d tile pairs", m, p.tiles, p.tile_pairs);
        // the grid's x extent: the last pair (tiles - 1, tiles - 1) has the last index
        const int last = (p.tiles - 1) * p.tiles / 2 + (p.tiles - 1);
        CHECK(last == p.tile_pairs - 1, "m %d: the last tile pair has index %d of %d", m, last, p.tile_pairs);
        const int64_t per_query = (int64_t)p.mp * p.mp * 4;
        const int64_t want = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nq, 256), eb / per_query));
        CHECK(p.cq == want, "nq %d m %d eb %ld: cq %d, the rule gives %ld", nq, m, (long)eb, p.cq, (long)want);
        CHECK(p.cq >= 1 && p.cq <= std::min(nq, 256), "nq %d m %d: chunk of %d queries", nq, m, p.cq);
        CHECK(p.cq == 1 || (int64_t)p.cq * per_query <= eb, "nq %d m %d: a chunk of %d queries exceeds exact_bytes %ld", nq, m, p.cq, (long)eb);
        CHECK(p.chunks == (nq + p.cq - 1) / p.cq && p.chunks * p.cq >= nq && (p.chunks - 1) * p.cq < nq, "nq %d m %d: %ld chunks of %d", nq, m, (long)p.chunks, p.cq);
        // the workspace of a chunk
        const size_t size = ws_bytes_for<MmrWs>(p.cq, p.mp);
        CHECK(size <= RESERVE, "%zu bytes exceed the reservation", size);
        if (size > RESERVE) continue;
        MmrWs w; Bump b(base, size);
        w.lay(b, p.cq, p.mp);
        CHECK(b.off == size && b.off <= b.cap, "nq %d m %d: the placing run ends at %zu, the dry run at %zu", nq, m, b.off, size);
        const size_t o_rows = (size_t)((char*)w.rows - base), o_rel = (size_t)((char*)w.rel - base), o_cnt = (size_t)((char*)w.cnt - base),
                     o_P = (size_t)((char*)w.P - base);
        const size_t list_bytes = (size_t)p.cq * p.mp * 4;
        CHECK(o_rows % 256 == 0 && o_rel % 256 == 0 && o_cnt % 256 == 0 && o_P % 256 == 0, "nq %d m %d: a region is not 256-byte aligned", nq, m);
        CHECK(o_rel >= o_rows + list_bytes && o_cnt >= o_rel + list_bytes && o_P >= o_cnt + (size_t)p.cq * 4, "nq %d m %d: regions overlap", nq, m);
        CHECK(o_P + (size_t)p.cq * (size_t)per_query == size, "nq %d m %d: P ends at %zu, the size is %zu", nq, m, o_P + (size_t)p.cq * (size_t)per_query, size);
    }
    // no query: no chunk; the pair metrics
    CHECK(mmr_plan(0, 10, (int64_t)1 << 30).chunks == 0, "a call without queries has chunks");
    CHECK(mmr_pair_metric_ok(HDB_DOT) && mmr_pair_metric_ok(HDB_COSINE) && mmr_pair_metric_ok(HDB_EUCLIDEAN), "a pair metric is refused");
    CHECK(!mmr_pair_metric_ok(HDB_HAMMING) && !mmr_pair_metric_ok(HDB_MANHATTAN) && !mmr_pair_metric_ok(HDB_JACCARD) && !mmr_pair_metric_ok(HDB_PEARSON) &&
          !mmr_pair_metric_ok(HDB_EUCLIDEAN_DIST) && !mmr_pair_metric_ok(-1) && !mmr_pair_metric_ok(99), "a metric that is no pair metric passes");
    std::printf("%ld points checked\n", g_points);
    return check_done();
}
