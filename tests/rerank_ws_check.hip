// rerank_ws_check.hip -- host program of tests/test_rerank_host.py: the workspace layout of hdb_rerank (RerankWs, csrc/hdb_ws.h) over
// a grid of shapes, in the manner of ws_layout_check.hip.  No GPU call is made.  For every point: the size the dry run reports is
// where the placing run ends, every region is 256-byte aligned, holds the bytes its users need (the kernels' extents, stated
// below), follows its predecessor without overlap and lies inside the reported size; the centred queries exist only for pearson.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <utility>
#include <sys/mman.h>

#include "hdb_ws.h"
#include "../include/hyperdb_hip.h"
#include "plan_check.h"

static long g_points = 0;

int main() {
    const size_t RESERVE = (size_t)8 << 30;      // address space only: never touched
    char* base = (char*)mmap(nullptr, RESERVE, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (base == (char*)MAP_FAILED) { std::printf("mmap failed\n"); return 2; }
    const int nqs[] = {1, 9, 256, 300};
    const int cqs[] = {1, 4, 256};
    const int ms[] = {1, 5, 16, 17, 1000, 8192};
    const int ds[] = {1, 40, 384, 4096};
    for (int nq : nqs) for (int cq_opt : cqs) for (int m : ms) for (int d : ds) for (int pearson = 0; pearson < 2; ++pearson) {
        const int cq = std::min(cq_opt, nq);
        ++g_points;
        const size_t size = ws_bytes_for<RerankWs>(nq, d, cq, m, pearson != 0);
        CHECK(size <= RESERVE, "%zu bytes exceed the reservation", size);
        if (size > RESERVE) continue;
        RerankWs w; Bump b(base, size);
        w.lay(b, nq, d, cq, m, pearson != 0);
        CHECK(b.off == size && b.off <= b.cap, "nq %d cq %d m %d d %d: the placing run ends at %zu, the dry run at %zu", nq, cq, m, d, b.off, size);
        const size_t q = (size_t)nq, c = (size_t)cq;
        const std::vector<std::pair<const void*, size_t>> need = {
            {w.qinv, q * 4}, {w.qsq, q * 4}, {w.qnan, q * 4}, {w.qc, pearson ? q * d * 8 : 0}, {w.cnt, c * HDB_CNT_STRIDE * 4},
            {w.rows, c * (size_t)m * 8}, {w.cand, c * HDB_CAND_CAP * 8}};
        size_t end = 0;
        for (size_t i = 0; i < need.size(); ++i) {
            if (!need[i].first) { CHECK(need[i].second == 0, "pointer %zu is null, %zu bytes are needed there", i, need[i].second); continue; }
            const size_t off = (size_t)((const char*)need[i].first - base), bytes = need[i].second;
            CHECK(bytes > 0, "region %zu is placed and nobody needs it", i);
            CHECK(off % 256 == 0, "region %zu at offset %zu is not 256-byte aligned", i, off);
            CHECK(off >= end, "region %zu at %zu overlaps its predecessor, which needs the bytes up to %zu", i, off, end);
            CHECK(off + bytes <= size, "region %zu needs the bytes up to %zu, past the reported size %zu", i, off + bytes, size);
            end = off + bytes;
        }
        // nothing but the regions and their alignment: the size is the sum of the needs, each rounded to 256 bytes at most
        size_t sum = 0;
        for (const auto& r : need) sum += align_up(r.second, 256);
        CHECK(size <= sum, "nq %d cq %d m %d d %d: %zu bytes for regions of %zu", nq, cq, m, d, size, sum);
    }
    std::printf("%ld layouts checked\n", g_points);
    return check_done();
}
