// hdb_mmr_plan.h -- how hdb_mmr cuts a call: queries per chunk, and the extents its launches and its workspace (MmrWs, hdb_ws.h) take.
//
// Pure host functions of plain numbers, in the spirit of hdb_group_plan.h and hdb_maxsim_plan.h: no HIP call, no hdb_index, so
// tests/mmr_plan_check.hip runs them over a grid.  A call of nq lists of m entries:
//   mp          m rounded up to the pair tile (HDB_MMR_TILE, hdb_caps.h): the leading dimension of rows, rel and P;
//   tiles       mp / HDB_MMR_TILE, and tile_pairs = tiles (tiles + 1) / 2 pairs ti <= tj: the x extent of the pair launch's grid;
//   chunk       cq consecutive queries whose pair matrices P [cq][mp][mp] (4 bytes per pair) stay in the workspace together:
//               cq = clamp(exact_bytes / (mp^2 4), 1, min(nq, 256)).  One query's matrix is at most 16 MiB (m = 2048): where
//               exact_bytes is less, the plan is cq = 1 and the workspace is what it must be.
// Per chunk: three launches -- prep (cq workgroups), pairs (tile_pairs x cq), select (cq).
#pragma once
#include "hdb_plan.h"

struct MmrPlan {
    int mp = 0, tiles = 0, tile_pairs = 0;
    int cq = 1;                                   // queries per chunk
    int64_t chunks = 0;                           // the stat mmr_chunks
};

static inline MmrPlan mmr_plan(int32_t nq, int32_t m, int64_t exact_bytes) {
    MmrPlan p;
    p.mp = hdb_mmr_mp(m);
    p.tiles = p.mp / HDB_MMR_TILE;
    p.tile_pairs = p.tiles * (p.tiles + 1) / 2;
    const int64_t per_query = (int64_t)p.mp * p.mp * 4;
    p.cq = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nq, 256), exact_bytes / per_query));
    p.chunks = nq > 0 ? ((int64_t)nq + p.cq - 1) / p.cq : 0;
    return p;
}

// The pair metrics: the three whose value two stored rows have without a query.
static inline bool mmr_pair_metric_ok(int metric) { return metric == HDB_DOT || metric == HDB_COSINE || metric == HDB_EUCLIDEAN; }
