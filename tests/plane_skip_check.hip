// plane_skip_check.hip -- the walk of the plane pass over the tiles the sample pass did not take (hdb_plane_skip_*, csrc/hdb_caps.h)
// on the host: a stand-alone program, no GPU call.
//
// The sample of a one-query shadow call takes tile hdb_tile_index(w, stride) of every window w < s_tiles (csrc/hdb_common.h); the
// plane pass (hdb_quant_plane_scan_kernel, csrc/hdb_quant.hip) walks a dense index over the other tiles.  For
//   n in {16, 17, 8193, 8217, 70001, 1 000 003, 10 000 000} with the call's own sample quant_call_sample(n, 384, 128) (csrc/hdb_ws.h),
//   forced plans (stride 1: a dense prefix; stride 2: one walked tile per window; every tile sampled; no sample; a long tail)
// and grids of 1, 3 and 1024 workgroups the program walks the tiles exactly as the kernel does -- wave (block, wave) starts at position
// (block * 4 + wave) * 2, takes that position and the next, steps by grid * 8, one hdb_plane_skip_start and then
// hdb_plane_skip_advance only -- and checks that
//   every visited tile is inside the matrix and visited once,
//   the visited tiles are exactly the tiles that are not hdb_tile_index(w, stride) of a window w < s_tiles,
//   the incremental position equals hdb_plane_skip_start of the same dense index (the closed form), step by step,
//   the sampled tiles are distinct, ascending, inside their windows and never the ragged last tile.
// It prints "index W STRIDE VALUE" for a fixed list of (w, stride) -- tests/test_plane_skip_plan.py compares them with the Python
// restatement of hdb_tile_index that tests/test_plane_skip.py plants its rows with -- then "plans P", "tiles T" and " F failures";
// exit status 1 on any failure.
#include "hdb_ws.h"
#include "plan_check.h"
#include <cstdio>
#include <vector>

static long g_tiles = 0;

static void walk(int64_t n, uint32_t s_tiles, uint32_t stride, int grid) {
#define WHERE "n %lld s_tiles %u stride %u grid %d", (long long)n, s_tiles, stride, grid
    const int64_t ntiles = (n + 15) / 16;
    CHECK((int64_t)s_tiles * stride <= ntiles, WHERE);
    if ((int64_t)s_tiles * stride > ntiles) return;
    std::vector<unsigned char> sampled((size_t)ntiles, 0), seen((size_t)ntiles, 0);
    int64_t prev = -1;
    for (uint32_t w = 0; w < s_tiles; ++w) {
        const int64_t t = hdb_tile_index((int64_t)w, (int64_t)stride);
        CHECK(t >= (int64_t)w * stride && t < (int64_t)(w + 1) * stride && t > prev && t < n / 16, WHERE);
        if (t < 0 || t >= ntiles) return;
        sampled[(size_t)t] = 1; prev = t;
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
            const HdbSkipPos c0 = hdb_plane_skip_start(tp, s_tiles, stride);
            CHECK(c0.w == pos.w && c0.o == pos.o, WHERE);
            for (int tt = 0; tt < 2; ++tt) {
                if (tp + (uint32_t)tt >= nwalk) continue;
                if (tt == 1) { const HdbSkipPos c1 = hdb_plane_skip_start(tp + 1u, s_tiles, stride); CHECK(c1.w == p1.w && c1.o == p1.o, WHERE); }
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
    CHECK(s_tiles == 0 || !sampled[(size_t)ntiles - 1] || n % 16 == 0, WHERE);       // (the ragged last tile is walked)
    g_tiles += visited;
#undef WHERE
}

int main() {
    const int64_t ns[] = {16, 17, 8193, 8217, 70001, 1000003, 10000000};
    const int grids[] = {1, 3, 1024};
    long plans = 0;
    for (int64_t n : ns) {
        const QuantSample qs = quant_call_sample(n, 384, 128);
        CHECK(qs.s_tiles >= 1 && qs.s_stride >= 1 && qs.s_rows == qs.s_tiles * 16 && qs.s_rows <= quant_ld_max(n, 384), "n %lld", (long long)n);
        for (int grid : grids) { walk(n, (uint32_t)qs.s_tiles, (uint32_t)qs.s_stride, grid); ++plans; }
    }
    // forced plans: {n, s_tiles, stride}
    const struct { int64_t n; uint32_t s_tiles, stride; } forced[] = {
        {323, 5, 1}, {320, 20, 1}, {8217, 137, 1},          // stride 1: a dense prefix, every tile sampled, a long tail
        {8217, 200, 2}, {70001, 1458, 3},                   // one and two walked tiles per window
        {70001, 0, 1}, {17, 0, 1},                          // no sample: every tile
        {70001, 7, 31}, {1000003, 61, 1024}, {70001, 4375, 1},
    };
    for (const auto& f : forced) for (int grid : grids) { walk(f.n, f.s_tiles, f.stride, grid); ++plans; }
    // what the Python restatement is compared with
    const int64_t strides[] = {1, 2, 3, 7, 31, 32, 1000};
    const int64_t ws[] = {0, 1, 2, 3, 17, 136, 1000, 19531, 4000000};
    for (int64_t s : strides) for (int64_t w : ws) std::printf("index %lld %lld %lld\n", (long long)w, (long long)s, (long long)hdb_tile_index(w, s));
    std::printf("plans %ld\ntiles %ld\n", plans, g_tiles);
    return check_done();
}
