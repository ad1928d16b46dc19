// plane_grid_check.hip -- the grid of the plane pass (hdb_quant_plane_blocks, csrc/hdb_caps.h) on the host: a stand-alone program, no
// GPU call.
//
// The plane pass (hdb_quant_plane_scan_kernel, csrc/hdb_quant.hip) runs workgroups of four waves, a wave takes two tiles per step: one
// workgroup per four step-pairs of the tiles it walks, at most wg_per_cu per CU (0: the table HDB_PLANE_WG_PER_CU, an entry per
// J = ceil(U / 4)), and max_blocks > 0 caps it further.  For
//   n in {16, 17, 8193, 70001, 2 000 000, 10 000 000}, J = 1 .. 4 (d = 128 J, the call's own sample quant_call_sample(n, d, 128)),
//   cus in {1, 64, 256}, wg_per_cu = 0 .. 8, max_blocks in {0, 1, 3, 5000}
// the program checks that
//   1 <= blocks <= cap, cap = wg_per_cu x cus (the table's entry for 0), and <= max_blocks where that is set,
//   blocks never exceed the work, ceil(ceil(nwalk / 2) / 4) workgroups (one where nothing is walked), and equal min(cap, work),
//   wg_per_cu = 0 gives what the table's entry gives, and no entry exceeds the waves per SIMD its kernel is compiled for,
//   the walk at that grid -- exactly as the kernel walks, see tests/plane_skip_check.hip -- visits the complement of the sample once.
// (A walk is repeated only for a grid not yet seen with that sample.)
// It prints "table J WG WAVES" for J = 1 .. 4, "rules R", "walks W", "tiles T" and " F failures"; exit status 1 on any failure.
#include "hdb_ws.h"
#include "plan_check.h"
#include <cstdio>
#include <set>
#include <vector>

static long g_tiles = 0;

static void walk(int64_t n, uint32_t s_tiles, uint32_t stride, int grid) {
#define WHERE "n %lld s_tiles %u stride %u grid %d", (long long)n, s_tiles, stride, grid
    const int64_t ntiles = (n + 15) / 16;
    CHECK((int64_t)s_tiles * stride <= ntiles, WHERE);
    if ((int64_t)s_tiles * stride > ntiles) return;
    std::vector<unsigned char> sampled((size_t)ntiles, 0), seen((size_t)ntiles, 0);
    for (uint32_t w = 0; w < s_tiles; ++w) {
        const int64_t t = hdb_tile_index((int64_t)w, (int64_t)stride);
        CHECK(t >= 0 && t < ntiles, WHERE);
        if (t < 0 || t >= ntiles) return;
        sampled[(size_t)t] = 1;
    }
    const uint32_t nwalk = hdb_plane_skip_count((uint32_t)ntiles, s_tiles);
    const HdbSkipStep step = hdb_plane_skip_step((uint32_t)grid * 8u, stride), next = {0u, 1u, 1u};
    long visited = 0;
    for (int block = 0; block < grid; ++block) for (int wave = 0; wave < 4; ++wave) {
        const uint32_t tp0 = ((uint32_t)block * 4u + (uint32_t)wave) * 2u;
        HdbSkipPos pos = hdb_plane_skip_start(tp0 < nwalk ? tp0 : 0u, s_tiles, stride);
        for (uint32_t tp = tp0; tp < nwalk; tp += (uint32_t)grid * 8u, hdb_plane_skip_advance(pos, step, s_tiles, stride)) {
            HdbSkipPos p1 = pos;
            hdb_plane_skip_advance(p1, next, s_tiles, stride);
            for (int tt = 0; tt < 2; ++tt) {
                if (tp + (uint32_t)tt >= nwalk) continue;
                const int64_t t = hdb_plane_skip_tile(tt ? p1 : pos, s_tiles, stride);
                CHECK(t >= 0 && t < ntiles, WHERE);
                if (t < 0 || t >= ntiles) continue;
                CHECK(!sampled[(size_t)t] && !seen[(size_t)t], WHERE);
                seen[(size_t)t] = 1; ++visited;
            }
        }
    }
    long missing = 0;
    for (int64_t t = 0; t < ntiles; ++t) if (!sampled[(size_t)t] && !seen[(size_t)t]) ++missing;
    CHECK(missing == 0 && visited == (long)ntiles - (long)s_tiles, WHERE);
    g_tiles += visited;
#undef WHERE
}

int main() {
    const int64_t ns[] = {16, 17, 8193, 70001, 2000000, 10000000};
    const int cuss[] = {1, 64, 256};
    const int mbs[] = {0, 1, 3, 5000};
    long rules = 0, walks = 0;
    for (int J = 1; J <= 4; ++J) {
        const int wg = hdb_quant_plane_wg_per_cu(J), waves = hdb_quant_plane_waves(J);
        std::printf("table %d %d %d\n", J, wg, waves);
        CHECK(wg >= 1 && wg <= waves && waves <= 8, "J %d", J);
        CHECK(hdb_quant_plane_j(4 * J) == J && hdb_quant_plane_j(4 * J - 3) == J && hdb_quant_plane_j(hdb_quant_plane_units(128 * J)) == J, "J %d", J);
    }
    for (int64_t n : ns) for (int J = 1; J <= 4; ++J) {
        const int d = 128 * J;
        const QuantSample qs = quant_call_sample(n, d, 128);
        const int64_t ntiles = (n + 15) / 16, nwalk = ntiles - qs.s_tiles;
        CHECK(qs.s_tiles >= 1 && nwalk >= 0, "n %lld J %d", (long long)n, J);
        const int64_t work = std::max<int64_t>(1, ((nwalk + 1) / 2 + 3) / 4);
        std::set<int> walked;
        for (int cus : cuss) for (int wg = 0; wg <= 8; ++wg) for (int mb : mbs) {
#define WHERE "n %lld J %d cus %d wg_per_cu %d max_blocks %d", (long long)n, J, cus, wg, mb
            const int blocks = hdb_quant_plane_blocks(nwalk, J, cus, wg, mb);
            int64_t cap = (int64_t)(wg ? wg : hdb_quant_plane_wg_per_cu(J)) * cus;
            CHECK(blocks >= 1 && blocks <= cap, WHERE);
            if (mb > 0) { CHECK(blocks <= mb, WHERE); cap = std::min<int64_t>(cap, mb); }
            CHECK(blocks <= work, WHERE);
            CHECK(blocks == std::min(cap, work), WHERE);
            if (wg == 0) CHECK(blocks == hdb_quant_plane_blocks(nwalk, J, cus, hdb_quant_plane_wg_per_cu(J), mb), WHERE);
            ++rules;
            if (blocks >= 1 && walked.insert(blocks).second) { walk(n, (uint32_t)qs.s_tiles, (uint32_t)qs.s_stride, blocks); ++walks; }
#undef WHERE
        }
    }
    // out-of-range arguments fall back to something launchable
    CHECK(hdb_quant_plane_blocks(0, 3, 256, 0, 0) == 1 && hdb_quant_plane_blocks(1000000, 3, 0, 0, 0) >= 1, "edges");
    CHECK(hdb_quant_plane_blocks(1000000, 3, 256, 99, 0) == 8 * 256 && hdb_quant_plane_blocks(1000000, 3, 256, -5, 0) == hdb_quant_plane_wg_per_cu(3) * 256, "edges");
    CHECK(hdb_quant_plane_dbg_blocks(625000, 0) == 1024 && hdb_quant_plane_dbg_blocks(625000, 3) == 3 && hdb_quant_plane_dbg_blocks(9, 0) == 2, "dbg");
    std::printf("rules %ld\nwalks %ld\ntiles %ld\n", rules, walks, g_tiles);
    return check_done();
}
