// hdb_plan.h -- plan_topk: the ONE place where hdb_topk chooses its path.
//
// A pure function of plain facts -- the index (rows, width, dtype, what shadow it holds), the device (CU count), the options, the
// call -- to one TopkPlan: the path, everything its executor in hdb_api.hip consumes, and the statistics of the call.  It makes
// no HIP call and does not see hdb_index, so tests/test_topk_plan.py runs it on the host over a recorded dispatch table
// (tests/golden/dispatch_table.jsonl) and a synthetic grid.  The one question it cannot answer from numbers -- is every row of the
// matrix finite? -- it asks through a callable, and only where the answer decides something (the answer costs a device round trip
// the first time).  What a kernel unit can take comes from hdb_caps.h, the shadow's sample plans from hdb_ws.h.
#pragma once
#include "hdb_ws.h"
#include <algorithm>
#include <cstring>

// ---- options (hdb_set_option), embedded in the index as ix->opt ----------------------------------------------------------------
struct hdb_options {
    int64_t max_blocks = 0;           // 0 = automatic (row scan: 2-4 workgroups per CU, see hdb_launch_scan)
    int64_t force_exact = 0;
    int64_t sample_target = 0;        // 0 = automatic
    int64_t mfma_min_q = 1;
    int64_t use_mfma = 1;
    int64_t exact_bytes = (int64_t)1 << 30;
    int64_t bits_fused = 1;           // hamming / jaccard: try the sampled-threshold path first (exact path when it fails)
    int64_t bits_local = 1;           // ... its single launch without row sample and exchange: every workgroup its own threshold (hdb_bits_fused.hip, round 4)
    // knobs of the dispatch: -1 = the measured rule (tools/sweep_dispatch.py, profiles/r3_dispatch_few_queries.txt), else a fixed limit
    int64_t fused_max_q = -1;         // hdb_mfma_fused_kernel takes calls of up to this many queries
    int64_t f32_min_q = -1;           // float32 matrices: the matrix-core scan from this many queries on
    int64_t f32_split = 1;            // ... as bf16 parts (hdb_mfma_f32s.hip) where that flavour exists, the matrix is finite and the call has at least
    int64_t f32_split_min_q = -1;     //     this many queries (-1: hdb_mfma_f32_split_min_q(d), the measured crossover)
    int64_t bf16_ks_min_q = -1;       // bfloat16 rows in K slices (d > 512): from this many queries on, never fewer than 5 (-1: hdb_mfma_bf16_ks_min_q(d), measured per width)
    int64_t f8_ks_min_q = 0;          // float8 rows in K slices (d > 512, hdb_mfma_f8_ks.hip): 0 = never (the default: opt-in), n >= 1 = from max(n, 5, mfma_min_q) queries on, -1 = hdb_mfma_f8_ks_min_q(d)
    int64_t f8_lds_min_q = 0;         // float8 batches on the matrix cores with the rows expanded to bf16 in LDS once per workgroup (hdb_mfma_f8_lds.h): 0 = never (the default: opt-in), n >= 1 = from max(n, 5, mfma_min_q) queries on, -1 = hdb_mfma_f8_lds_min_q(d) (0 there: never)
    int64_t b1_mfma_min_q = 0;        // packed-bit batches on the bf16 matrix cores (hdb_mfma_b1.h; d = 128 .. 512 whole, 640 .. 4096 in K slices): 0 = never (the default: opt-in), n >= 1 = from max(n, 5, mfma_min_q) queries on, -1 = hdb_mfma_b1_min_q(d) (0 there: never)
    int64_t bf16_quant = 0;           // bfloat16 matrices: hdb_index_quantize(HDB_QUANT_I8) builds an explicit int8 shadow (0, the default: the call is refused; opt-in).  Means nothing on other types; the plan does not read it
    int64_t f8_lds_waves = 0;         // ... in workgroups of this many waves: 0 = by the launch's queries (hdb_mfma_f8_lds_auto_waves), 4 | 8 = fixed (A/B runs)
    int64_t bits_max_q = -1;          // hamming / jaccard: the single launch (four queries at a time) up to this many queries
    int64_t host_direct = 1;          // hdb_topk_host: kernels write a pinned host record themselves (no D2H copy)
    int64_t dyn_tiles = 1;            // MFMA filter pass: hand tiles out from a counter (0: static split)
    int64_t dyn_min_mb = 16;          // ... for passes of at least this many MiB of V per workgroup
    int64_t dyn_heavy = 0;            // ... also when all eight waves multiply (measured: 1.3-5 % slower at 256 queries, profiles/r3_q256_clock.json)
    int64_t host_poll = 1;            // hdb_topk_host + single-launch pipeline + pinned record: poll the status words instead of the stream
    int64_t use_fused = 1;            // 1-4 dot / cosine queries on an fp16 matrix: the whole call in ONE kernel (hdb_mfma_fused.h)
    int64_t use_local = 1;            // ... short matrices: its local flavour (no row sample, no exchange; every workgroup its own threshold)
    int64_t local_m = 0;              // ... rows every workgroup emits at least (0 = automatic: ~3072 / workgroups, 8 .. 32)
    int64_t local_max_tiles = 4;      // ... while a workgroup has at most this many tiles (the parking area holds 16)
    int64_t local_small = 0;          // ... 1: also for matrices of up to 8192 rows (measured slower than the three launches)
    int64_t local_max_q = 1;          // ... for calls of up to this many queries (two to four: the batched single launch is faster -- 36 vs 45 us at 20k rows, profiles/r4_latency_map.txt)
    int64_t use_l1_tile = 1;          // manhattan: dense passes through the LDS-staged tile kernel (hdb_l1_tile.hip)
    int64_t l1_packed = 1;            // ... fp16 rows and fp16-valued queries: packed fp16 differences (0: always float32, for A/B runs)
    int64_t use_batch1 = 1;           // 5+ queries (euclidean: 1+) on the matrix cores, k <= 128: the whole call in ONE launch per <= 256 queries (needs use_fused)
    int64_t fused_timeout_us = 2000;  // bound of every in-kernel spin of those kernels
    int64_t finalize_threads = 1024;  // workgroup size of hdb_finalize_kernel (256 | 512 | 1024)
    int64_t mfma_variant = 16;        // MFMA shape of the d=384 256-query pass (16 | 32)
    int64_t use_quant = 1;            // 0: never the int8 shadow, even where one exists
    int64_t quant_min_n = -1;         // ... from this many rows on (-1: the measured rule, quant_min_rows)
    int64_t quant_max_k = 128;        // ... for k up to this (<= 128)
    int64_t auto_quant = 1;           // fp16 matrix, 1-4 dot / cosine queries on the matrix cores: build the shadow on the first eligible call of a large index
    int64_t quant_batch_min_n = -1;   // ... batches of 5+ queries: from this many rows on (-1: the measured rule, quant_batch_rule)
    int64_t quant_batch_kernel = 1;   // ... their filter pass: 1 = int8 matrix cores (hdb_quant_mfma.hip), 0 = the v_dot4 scan, four queries per pass
    int64_t use_plane = 1;            // one dot / cosine query: pre-filter the shadow's rows through the 5-bit plane (0: never -- the manual switch)
    int64_t plane_min_n = -1;         // ... from this many rows on (-1: the measured rule, HDB_PLANE_MIN_ROWS)
    int64_t plane_cap_rows = 0;       // ... kept rows beyond which a call counts in the stat plane_overflows (0: n / 8); changes no answer
    int64_t plane_wg_per_cu = 0;      // ... workgroups per CU of its pass: 0 = the measured table (HDB_PLANE_WG_PER_CU, hdb_caps.h), 1 .. 8 = fixed (A/B runs); changes no answer
    int64_t use_subset = 1;           // a row list beside the mask (hdb_index_set_row_subset): score only the listed rows where the rule says so (0: never -- the mask)
    int64_t subset_min_n = -1;        // ... on matrices of at least this many rows (-1: the measured rule, HDB_SUBSET_MIN_ROWS)
    int64_t subset_ratio = -1;        // ... while m * ceil(nq / 4) * subset_ratio <= n (-1: the measured rule, HDB_SUBSET_RATIO; else an integer >= 1)
    int64_t rerank_chunk = 0;         // hdb_rerank: queries per chunk (0: up to HDB_RERANK_MAXQ); the plan of hdb_topk does not read it
    int64_t group_oversample = 4;     // hdb_topk_grouped_host: the first fast round collapses the top k * group_oversample (1 .. 64; rank_two_stage's default, not measured)
    int64_t group_fast_rounds = 2;    // ... fast rounds at most (0 .. 2); 0: always the exact grouped pass.  The plan of hdb_topk reads neither (hdb_group_plan.h)
    int64_t maxsim_team = 0;          // hdb_maxsim_host: lanes that own one group in its reduction (0: the rule, hdb_maxsim_team_rule; 1 | 4 | 16 | 64 = fixed, A/B runs and tests); changes no answer
};
#define HDB_RERANK_MAXQ 256
#define HDB_GROUP_OVERSAMPLE_MAX 64
#define HDB_GROUP_ROUNDS_MAX 2

// The ONE list of the option names: every member of hdb_options with the rule hdb_set_option applies to a value before it stores it.
//   HDB_OPT_CLAMP  max(lo, min(value, hi)) -- plain assignment where the bounds are the type's, "negative becomes -1" where lo is -1
//   HDB_OPT_SET    one of `set` (its first `hi` entries); any other value is ignored and the call still succeeds
//   HDB_OPT_RATIO  negative becomes -1, otherwise at least 1
//   HDB_OPT_BOOL   0 or 1
// hdb_set_option (hdb_api.hip), the host check programs (tests/plan_check.h) and the documentation guard (tests/test_abi.py) all read it.
enum { HDB_OPT_CLAMP, HDB_OPT_SET, HDB_OPT_RATIO, HDB_OPT_BOOL };
struct hdb_option_entry { const char* name; int64_t hdb_options::*member; int rule; int64_t lo, hi; int64_t set[5]; };
#define HDB_OPT(n)               {#n, &hdb_options::n, HDB_OPT_CLAMP, INT64_MIN, INT64_MAX, {}}
#define HDB_OPT_MIN(n, lo)       {#n, &hdb_options::n, HDB_OPT_CLAMP, lo, INT64_MAX, {}}
#define HDB_OPT_RANGE(n, lo, hi) {#n, &hdb_options::n, HDB_OPT_CLAMP, lo, hi, {}}
#define HDB_OPT_IN(n, cnt, ...)  {#n, &hdb_options::n, HDB_OPT_SET, 0, cnt, {__VA_ARGS__}}
#define HDB_OPT_FLAG(n)          {#n, &hdb_options::n, HDB_OPT_BOOL, 0, 1, {}}
static constexpr hdb_option_entry HDB_OPTIONS[] = {
    HDB_OPT(max_blocks), HDB_OPT(force_exact), HDB_OPT(sample_target), HDB_OPT(mfma_min_q), HDB_OPT(use_mfma),
    HDB_OPT_MIN(exact_bytes, 1 << 20), HDB_OPT(bits_fused), HDB_OPT(bits_local), HDB_OPT(fused_max_q), HDB_OPT(f32_min_q),
    HDB_OPT(f32_split), HDB_OPT(f32_split_min_q), HDB_OPT(bf16_ks_min_q), HDB_OPT_MIN(f8_ks_min_q, -1), HDB_OPT_MIN(f8_lds_min_q, -1),
    HDB_OPT_MIN(b1_mfma_min_q, -1), HDB_OPT_FLAG(bf16_quant), HDB_OPT_IN(f8_lds_waves, 3, 0, 4, 8),
    HDB_OPT(bits_max_q), HDB_OPT(host_direct), HDB_OPT(dyn_tiles), HDB_OPT_MIN(dyn_min_mb, 0), HDB_OPT(dyn_heavy), HDB_OPT(host_poll),
    HDB_OPT(use_fused), HDB_OPT(use_local), HDB_OPT_RANGE(local_m, 0, 64), HDB_OPT_MIN(local_max_tiles, 1), HDB_OPT(local_small),
    HDB_OPT(local_max_q), HDB_OPT(use_l1_tile), HDB_OPT(l1_packed), HDB_OPT(use_batch1), HDB_OPT_MIN(fused_timeout_us, 1),
    HDB_OPT_IN(finalize_threads, 3, 256, 512, 1024), HDB_OPT_IN(mfma_variant, 3, 16, 32, 64), HDB_OPT(use_quant), HDB_OPT(quant_min_n),
    HDB_OPT_RANGE(quant_max_k, 1, 128), HDB_OPT(auto_quant), HDB_OPT(quant_batch_min_n), HDB_OPT_FLAG(quant_batch_kernel),
    HDB_OPT(use_plane), HDB_OPT(plane_min_n), HDB_OPT_MIN(plane_cap_rows, 0), HDB_OPT_RANGE(plane_wg_per_cu, 0, 8), HDB_OPT(use_subset),
    HDB_OPT_MIN(subset_min_n, -1), {"subset_ratio", &hdb_options::subset_ratio, HDB_OPT_RATIO, -1, INT64_MAX, {}}, HDB_OPT_RANGE(rerank_chunk, 0, HDB_RERANK_MAXQ),
    HDB_OPT_RANGE(group_oversample, 1, HDB_GROUP_OVERSAMPLE_MAX), HDB_OPT_RANGE(group_fast_rounds, 0, HDB_GROUP_ROUNDS_MAX),
    HDB_OPT_IN(maxsim_team, 5, 0, 1, 4, 16, 64),
};
#undef HDB_OPT
#undef HDB_OPT_MIN
#undef HDB_OPT_RANGE
#undef HDB_OPT_IN
#undef HDB_OPT_FLAG
static_assert(sizeof(HDB_OPTIONS) / sizeof(HDB_OPTIONS[0]) == sizeof(hdb_options) / sizeof(int64_t), "every member of hdb_options has one entry in HDB_OPTIONS");
// -> whether `name` is an option; the value is stored under the entry's rule
static inline bool hdb_option_set(hdb_options& o, const char* name, int64_t value) {
    for (const hdb_option_entry& e : HDB_OPTIONS) {
        if (std::strcmp(name, e.name) != 0) continue;
        switch (e.rule) {
        case HDB_OPT_CLAMP: o.*e.member = std::max(e.lo, std::min(value, e.hi)); break;
        case HDB_OPT_SET:   for (int64_t i = 0; i < e.hi; ++i) if (value == e.set[i]) o.*e.member = value; break;
        case HDB_OPT_RATIO: o.*e.member = value < 0 ? -1 : std::max<int64_t>(1, value); break;
        default:            o.*e.member = value ? 1 : 0; break;
        }
        return true;
    }
    return false;
}

// ---- what the planner is told ---------------------------------------------------------------------------------------------------
struct TopkFacts {
    int64_t n; int32_t d; int dtype;
    int qmode;                        // HDB_QUANT_I8: the index holds a shadow ...
    bool qauto;                       // ... that it built for itself
    bool qauto_declined;              // ... or could not build (memory): no shadow path asks for a build
    bool plane_present, plane_declined;
    bool has_mask, has_bias;
    int cus;                          // compute units of the device
    int64_t subset_m;                 // rows of the list set beside the mask (hdb_index_set_row_subset), 0 = none
};
// n_groups > 0: the exact grouped pass of hdb_topk_grouped_host (exact is set as well); 0 for every other call
// maxsim: the score pass of hdb_maxsim_host (hdb_maxsim_plan.h; exact is set as well): the exact shape on every matrix size, all rows
struct TopkCall { int32_t nq, k; int metric; bool has_status, exact; int64_t n_groups; bool maxsim = false; };

// ---- what it answers ------------------------------------------------------------------------------------------------------------
enum TopkPath {
    HDB_PATH_EMPTY,                   // no rows: padding
    HDB_PATH_QUANT,                   // 1-4 queries through the int8 shadow (explicit: VALU bits; automatic: the matrix cores' bits)
    HDB_PATH_QUANT_BATCH,             // 5+ queries through the automatic shadow
    HDB_PATH_FUSED,                   // the single launch of 1-4 queries (exchange or local flavour)
    HDB_PATH_BITS1,                   // the single launch of the bit metrics, four queries at a time
    HDB_PATH_BATCH1,                  // the batched single launch, cq_max queries at a time
    HDB_PATH_FULL_SORT,               // k > HDB_MAX_K: all scores of a query, sorted
    HDB_PATH_PIPELINE                 // the multi-kernel pipeline: small, sampled or exact
};
// statistics of one call (hdb_get_stat); every call writes all of them
struct TopkStats { int64_t sample_rows = 0, sample_m = 0, path = 0, chunks = 0, mfma = 0, fused = 0, local = 0, f32s = 0, quant = 0, plane = 0, subset = 0, f8_lds = 0, plane_blocks = 0, rerank = 0;
                   int64_t grouped = 0, group_k = 0, group_rounds = 0, group_exact = 0;        // hdb_topk_grouped_host writes these four behind its last inner call
                   int64_t maxsim = 0, maxsim_chunks = 0, maxsim_team = 0, maxsim_sorted = 0;        // hdb_maxsim_host writes these four behind its plan's
                   int64_t mmr = 0, mmr_chunks = 0; };                                                // hdb_mmr / hdb_mmr_host write these two behind the calls inside them
// The ONE list of its members: X(name of the stat in hdb_get_stat, member).  hdb_get_stat answers these names from the table,
// plan_diff compares them, the documentation guard (tests/test_abi.py) reads the names.
#define HDB_STAT_FIELDS(X) \
    X(sample_rows, sample_rows) X(sample_m, sample_m) X(path, path) X(chunks, chunks) X(mfma, mfma) X(fused, fused) X(local, local) \
    X(f32_split, f32s) X(quant, quant) X(plane, plane) X(subset, subset) X(f8_lds, f8_lds) X(plane_blocks, plane_blocks) X(rerank, rerank) \
    X(grouped, grouped) X(group_k, group_k) X(group_rounds, group_rounds) X(group_exact, group_exact) \
    X(maxsim, maxsim) X(maxsim_chunks, maxsim_chunks) X(maxsim_team, maxsim_team) X(maxsim_sorted, maxsim_sorted) \
    X(mmr, mmr) X(mmr_chunks, mmr_chunks)
struct hdb_stat_entry { const char* name; int64_t TopkStats::*member; };
#define X(name, member) {#name, &TopkStats::member},
static constexpr hdb_stat_entry HDB_STATS[] = { HDB_STAT_FIELDS(X) };
#undef X
static_assert(sizeof(HDB_STATS) / sizeof(HDB_STATS[0]) == sizeof(TopkStats) / sizeof(int64_t), "every member of TopkStats has one entry in HDB_STAT_FIELDS");

struct TopkPlan {
    TopkPath path = HDB_PATH_EMPTY;
    uint32_t kk = 0; int W = 0;
    bool bits = false, pearson = false;                 // the metric's family
    bool exact = false, small = false, mfma = false, f32s = false, ksplit = false, l1tile = false, local = false;
    bool exact_req = false;                             // the caller asked for the exact selection (f32s: only while no query holds an infinity, run_pipeline)
    bool f8_lds = false;                                // float8 rows: every matrix-core launch of the call expands its rows in LDS (hdb_mfma_f8_lds.h)
    bool subset = false;                                // the pipeline scores the rows of the index's list: every extent below is that of a matrix of subset_m rows
    // prologue of the paths that prepare their queries with launches of their own (full sort, pipeline)
    bool prep = false, fold_small = false, q16_in_prep = false, f16_queries = false, mask_fold = false;
    int tile_rows = 16;
    int64_t s_tiles = 0, s_stride = 1, s_rows = 0, ld_s = 0, ld_n = 0; uint32_t m = 0;      // the row sample
    int cq_max = 1;
    int64_t ld_scores = 0, ld_ks = 0, sort_n = 0;      // extents of TopkWs beside (nq, d, W, cq_max)
    int64_t n_best = 0;                                 // ... and its per-group maxima: the exact grouped pass (TopkCall::n_groups), 0 otherwise
    uint32_t local_slot = 0, local_m = 0;               // single launch, local flavour
    int bits_local = 0;                                 // bits single launch: the local flavour is allowed
    int npass = 4;                                      // radix passes of the exact selection
    // shadow paths
    bool mflavour = false, build_needed = false, plane_wanted = false;
    bool qb_int8 = false;                               // batches: the int8 matrix-core filter (0: the v_dot4 scan, four queries per pass)
    int P = 0, nsub = 0; uint32_t pl_cap = 0;           // pl_cap: rows the plane may keep before the call counts in plane_overflows
    int pl_blocks = 0;                                  // workgroups of the plane pass (hdb_quant_plane_blocks), 0: the call does not take the plane
    QuantSample qs = {0, 1, 0, 0};
    TopkStats stats;
    bool shadow() const { return path == HDB_PATH_QUANT || path == HDB_PATH_QUANT_BATCH; }
    bool single_launch() const { return path == HDB_PATH_FUSED || path == HDB_PATH_BITS1 || path == HDB_PATH_BATCH1; }
};
// The ONE list of its members (qs and stats: member by member below).  A member that is not listed here does not compile:
#define TOPK_PLAN_FIELDS(X) \
    X(path) X(kk) X(W) X(bits) X(pearson) X(exact) X(small) X(mfma) X(f32s) X(ksplit) X(l1tile) X(local) X(exact_req) X(f8_lds) X(subset) \
    X(prep) X(fold_small) X(q16_in_prep) X(f16_queries) X(mask_fold) X(tile_rows) X(s_tiles) X(s_stride) X(s_rows) X(ld_s) X(ld_n) X(m) \
    X(cq_max) X(ld_scores) X(ld_ks) X(sort_n) X(n_best) X(local_slot) X(local_m) X(bits_local) X(npass) X(mflavour) X(build_needed) \
    X(plane_wanted) X(qb_int8) X(P) X(nsub) X(pl_cap) X(pl_blocks) X(qs.s_tiles) X(qs.s_stride) X(qs.s_rows) X(qs.ld_s)
// (members of an aggregate: the most initializers T{...} takes; hdb_any converts to every member's type, so each stands for one member)
struct hdb_any { template <class T> operator T() const; };
template <class T, class = void, class... A> struct hdb_arity { static constexpr size_t value = sizeof...(A) - 1; };
template <class T, class... A> struct hdb_arity<T, decltype(void(T{A{}...})), A...> : hdb_arity<T, void, A..., hdb_any> {};
#define X(f) +1
static_assert(hdb_arity<TopkPlan>::value == (0 TOPK_PLAN_FIELDS(X)) - 4 + 2 && hdb_arity<QuantSample>::value == 4,
              "every member of TopkPlan is listed in TOPK_PLAN_FIELDS (qs as its four members, stats through HDB_STAT_FIELDS)");
#undef X
// -> the name of the first member in which two plans differ, nullptr when they are equal.  A check that means "equal except X" resets
// X on both sides first.
static inline const char* plan_diff(const TopkPlan& a, const TopkPlan& b) {
#define X(f) if (!(a.f == b.f)) return #f;
    TOPK_PLAN_FIELDS(X)
#undef X
#define X(name, f) if (a.stats.f != b.stats.f) return "stats." #f;
    HDB_STAT_FIELDS(X)
#undef X
    return nullptr;
}

#define HDB_FUSED_MAXQ_RULE 4
static inline bool is_bits_metric(int metric) { return metric == HDB_HAMMING || metric == HDB_JACCARD; }

// Row sample for the threshold estimate: `tiles` tiles of `tile_rows` rows, evenly strided over V.
// The m-th largest of the sampled scores is exceeded by about T rows of the full matrix (Gamma(m)
// spread), T >= 8k..16k and <= CAP/2, so both "fewer than k pass" and "more than CAP pass" are
// < 1e-9 events for exchangeable row orders; either one only costs the exact-path re-run.
// coarse: the scores take few distinct values (bit metrics), so the rows at the threshold's own level all survive; aim lower.
// Batches of 32+ queries aim at 1024 survivors per query instead of 2048: every survivor costs the filter's slow path
// (d=384, 64 queries: 1.28 -> 1.20 ms per call; 256 queries: -1 %), the sample doubles to 0.8 % of the rows, and
// P(fewer than k=100 pass) = P(Gamma(8) < 0.78) = 1.7e-6 per query, paid with one exact re-run of that query.
static inline void sample_plan(int64_t n, int64_t sample_target, uint32_t kk, int nq, int tile_rows, bool coarse, int64_t& tiles, int64_t& stride, uint32_t& m) {
    int64_t T = sample_target > 0 ? sample_target : (kk <= 128 ? (nq >= 32 ? 1024 : 2048) : 4096);
    if (coarse && sample_target <= 0) T /= 2;
    m = kk <= 128 ? 8u : (kk <= 512 ? 64u : 256u);
    int64_t rows = (int64_t)((double)m * (double)n / (double)T);
    rows = std::max<int64_t>(rows, 16 * (int64_t)m);         // at least 16 m sample rows
    tiles = (rows + tile_rows - 1) / tile_rows;
    const int64_t all_tiles = n / tile_rows;                 // full tiles only: sample rows always exist
    tiles = std::min(tiles, all_tiles);
    stride = std::max<int64_t>(1, all_tiles / std::max<int64_t>(tiles, 1));
}

// Smallest matrix that takes the int8 shadow when quant_min_n is -1 (measured): below it the extra launches
// of the quantized pipeline cost more than the bytes it saves.
// bfloat16 (the opt-in shadow, bf16_quant): the smallest measured n at d = 384 from which the shadow beats the same handle with
// use_quant = 0 (the VALU scan) by at least 5 % in both of two runs, at that size and every larger one, for 1 and for 4 queries --
// the criterion of HDB_PLANE_MIN_ROWS (profiles/bf16_quant_time.txt, tools/time_bf16_quant.py; cosine top-100, p50 in us, VALU scan
// -> shadow, both runs): one query 500k 107 -> 108 / 105 -> 106 (0.99: no), 1M 165 -> 136 / 164 -> 133 (1.22x / 1.23x), 1.25M 1.31x /
// 1.34x, 2M (plane) 1.69x / 1.67x, 10M 1 222 -> 541 / 1 223 -> 527 (2.26x / 2.32x); four queries 500k 1.33x / 1.37x, 1M 1.69x / 1.77x,
// 10M 2 058 -> 738 / 2 028 -> 736 (2.79x / 2.75x).  It lies below fp16's because the bf16 default is the VALU scan, not the matrix cores.
static inline int64_t quant_min_rows(int dtype) {
    return dtype == HDB_F16 ? 1250000 : dtype == HDB_BF16 ? 1000000 : 500000;
}

// ... and the smallest fp16 matrix that builds a shadow for itself (auto_quant; measured, profiles/auto_quant_time.txt, DESIGN.md
// section 4.9).  It lies above the sizes at which the suite pins the default path's statistics (up to 1.6M rows).
#define HDB_QUANT_AUTO_MIN_ROWS 2000000
// Smallest matrix whose one-query calls go through the 5-bit plane when plane_min_n is -1: the smallest measured size from which the
// plane column of profiles/quant_plane_time.txt beats the plane-off column by at least 5 % in both runs, at that size and every
// larger one (2M: 1.10x / 1.09x, 10M: 1.29x / 1.30x).  It is also the smallest size that has an automatic shadow.
#define HDB_PLANE_MIN_ROWS 2000000
// rows the plane may keep before a call counts in plane_overflows: an eighth of the matrix (the plane keeps under 5 % of Gaussian
// rows), or what the option asks for
static inline uint32_t plane_list_cap(const hdb_options& o, int64_t n) {
    return (uint32_t)(o.plane_cap_rows > 0 ? std::min<int64_t>(o.plane_cap_rows, n) : std::max<int64_t>(n / 8, 16));
}
// The 5-bit plane of the shadow (hdb_quant.hip): 20 bytes per 32-element unit and 16 bytes of row terms per row (hot blocks per 16-row tile, hdb_caps.h), for rows of up to 512
// elements (the widths the plane path takes).
static inline bool plane_possible(int d) { return d <= 512; }
// an index whose caller switched the path off (use_plane = 0) before the shadow was built does not pay for a plane
static inline bool plane_wanted(int d, const hdb_options& o) { return plane_possible(d) && o.use_plane; }

// The measured rule of quant_batch_min_n = -1: the smallest matrix from which a batch of nq queries is at least 1.10x faster through
// the shadow than through the fp16 single launch, 0 = never (profiles/quant_batch_time.txt, one box, interleaved, p50 in us, parent ->
// shadow).  The filter kernel reads its row fragments straight from global memory, so a workgroup has one tile per wave in flight:
// it wins while one query tile per wave keeps the pass near the shadow's bytes and loses once the waves share tiles.
//   d = 384, 5-16 queries: 2M 269 -> 261 (1.03), 3M 373 -> 336 (1.11) / 430 -> 378 (1.14), 4M 1.16 / 1.13, 5M 1.18-1.19, 10M 1.18-1.21
//   d = 384, 24 queries: 5M 674 -> 568 (1.19), 10M 1167 -> 1002 (1.17); 32 queries: 1.03 / 1.13, at 3M-4M 0.93 / 1.00; 48: 0.94 / 1.03
//   d = 384, 64 / 128 / 256 queries at 10M: 1137 -> 1776 (0.64), 1342 -> 3485 (0.39), 2292 -> 6545 (0.35): excluded
//   d = 512, 5 / 8 / 16 queries: 10M 1.21 / 1.18 / 1.11; 5M 1.10 / 1.09 / 0.99; 2M 0.98 and below
//   d = 128: 0.78-0.91 at every size (the fp16 pass over 256-byte rows is short already); d = 256: not measured, so not admitted
static inline int64_t quant_batch_rule(int d, int nq) {
    int64_t rows = 0;
    if (d == 384) rows = nq <= 16 ? 3000000 : nq <= 24 ? 5000000 : 0;
    else if (d == 512) rows = nq <= 16 ? 10000000 : 0;
    return rows > 0 ? std::max<int64_t>(rows, HDB_QUANT_AUTO_MIN_ROWS) : 0;
}
// wld of QuantBatchWs: the most slots any launch of the batch's sample pass leaves per query
static inline int64_t quant_batch_wld() { return (int64_t)align_up((size_t)hdb_qb_slots(512, 1), 4); }

// What the two automatic-shadow tests of plan_topk share (auto_quant): a call the matrix cores would answer on an fp16 matrix that
// has no shadow or an automatic one, sampled path, status words, k within the shadow's limits, dot or cosine.
static inline bool auto_quant_call(const TopkFacts& ix, const hdb_options& o, const TopkCall& c, bool mfma, bool exact, bool small) {
    return o.auto_quant && o.use_quant && mfma && ix.dtype == HDB_F16 && (ix.qmode == HDB_QUANT_NONE || ix.qauto) && !exact && !small &&
           c.has_status && c.k <= o.quant_max_k && c.k <= 128 && (c.metric == HDB_DOT || c.metric == HDB_COSINE) &&
           !(ix.qmode == HDB_QUANT_NONE && ix.qauto_declined);      // (a build the device had no memory for is not asked for again)
}

// 1-4 queries through the shadow (quant_topk).  mflavour: the automatic shadow of an fp16 index, rescored on the matrix cores.
static inline void plan_quant(TopkPlan& p, const TopkFacts& ix, const hdb_options& o, const TopkCall& c, bool mflavour) {
    p.path = HDB_PATH_QUANT; p.mflavour = mflavour; p.build_needed = ix.qmode != HDB_QUANT_I8;
    p.P = (int)align_up((size_t)ix.d, 16);
    p.qs = quant_call_sample(ix.n, ix.d, p.kk);
    // (a shadow that was built without a plane -- use_plane was off then -- gets it on the first call that asks for the path)
    p.plane_wanted = c.nq == 1 && (c.metric == HDB_DOT || c.metric == HDB_COSINE) && plane_wanted(ix.d, o) && !ix.plane_declined &&
                     ix.n >= (o.plane_min_n >= 0 ? o.plane_min_n : (int64_t)HDB_PLANE_MIN_ROWS);
    p.pl_cap = plane_list_cap(o, ix.n);
    // the plane pass walks the tiles the sample did not take; its grid follows the device and the measured table (hdb_caps.h)
    if (p.plane_wanted)
        p.pl_blocks = hdb_quant_plane_blocks((ix.n + 15) / 16 - p.qs.s_tiles, hdb_quant_plane_j(hdb_quant_plane_units(p.P)), ix.cus,
                                             (int)o.plane_wg_per_cu, (int)o.max_blocks);
    if (mflavour) {
        // the threshold folded into the two passes (QuantArgs::nsub) while the sample's grid has at least the 1024 subsets
        // hdb_sample_thr_kernel works with; smaller samples keep that kernel
        p.nsub = 4 * hdb_quant_scan_blocks(p.qs.s_tiles, (int)o.max_blocks);
        if (p.nsub < 1024 || p.nsub > HDB_QUANT_NSUB_MAX) p.nsub = 0;
    }
    p.stats.quant = 1; p.stats.path = 1; p.stats.mfma = mflavour ? 1 : 0; p.stats.plane = p.plane_wanted ? 1 : 0;
    p.stats.plane_blocks = p.pl_blocks;
    p.stats.sample_rows = p.qs.s_rows; p.stats.sample_m = 16; p.stats.chunks = 1;
}
// batches of 5+ queries through the automatic shadow (quant_batch_topk): chunks of up to 256 queries
static inline void plan_quant_batch(TopkPlan& p, const TopkFacts& ix, const hdb_options& o, const TopkCall& c) {
    p.path = HDB_PATH_QUANT_BATCH; p.mflavour = true; p.build_needed = ix.qmode != HDB_QUANT_I8;
    p.P = (int)align_up((size_t)ix.d, 16);
    p.qs = quant_batch_sample(ix.n);
    p.cq_max = std::min<int>(c.nq, 256);
    p.qb_int8 = o.quant_batch_kernel != 0;
    p.stats.quant = 1; p.stats.path = 1; p.stats.mfma = 1;
    p.stats.sample_rows = p.qs.s_rows; p.stats.sample_m = HDB_QB_SAMPLE_M; p.stats.chunks = (c.nq + p.cq_max - 1) / p.cq_max;
}

// ---- the row list (hdb_index_set_row_subset): when a filtered call scores only the rows it keeps ---------------------------------
// A list call is the VALU scan, four queries per pass, over m gathered rows plus the launches of the multi-kernel pipeline; the
// masked call streams all n rows on whatever path it has.  The two knobs of the rule, subset_ratio = -1 / subset_min_n = -1:
// (profiles/subset_time.txt, one box, the same handle with use_subset = 0 and with the list, alternating call by call, p50 of 200 calls
// in us, cosine top-100, masked -> list; share = m / n exactly, random ascending rows):
//   10M x 384 fp16, 1 / 4 / 16 queries:
//     share 1/2: 521 -> 688 (0.76), 799 -> 1171 (0.68), 1301 -> not eligible
//     share 1/4: 516 -> 369 (1.40), 795 -> 617 (1.29), 1325 -> 1595 (0.83)
//     share 1/8: 507 -> 211 (2.40), 778 -> 339 (2.30), 1296 -> 834 (1.55)
//     share 1/16: 507 -> 130 (3.89), 748 -> 196 (3.81), 1295 -> 457 (2.83)
//     share 1/64: 495 -> 69 (7.18), 716 -> 92 (7.78), 1289 -> 170 (7.58)
//     share 1/1024: 489 -> 46 (10.53), 708 -> 60 (11.90), 1283 -> 74 (17.27)
//   2M x 384 fp32, 1 / 4 / 16 queries:
//     share 1/2: 471 -> 288 (1.64), 523 -> 392 (1.33), 528 -> not eligible
//     share 1/4: 465 -> 167 (2.78), 522 -> 219 (2.38), 516 -> 574 (0.90)
//     share 1/8: 465 -> 111 (4.20), 521 -> 140 (3.73), 515 -> 320 (1.61)
//     share 1/16: 465 -> 79 (5.89), 522 -> 98 (5.31), 530 -> 200 (2.65)
//     share 1/64: 465 -> 54 (8.57), 523 -> 71 (7.41), 516 -> 110 (4.67)
//     share 1/1024: 467 -> 37 (12.75), 523 -> 46 (11.27), 534 -> 60 (8.89)
//   1M x 768 bf16, 1 / 4 / 16 queries:
//     share 1/2: 287 -> 177 (1.62), 400 -> 236 (1.69), 606 -> not eligible
//     share 1/4: 278 -> 116 (2.38), 400 -> 155 (2.58), 603 -> 324 (1.86)
//     share 1/8: 277 -> 88 (3.16), 400 -> 112 (3.58), 602 -> 208 (2.90)
//     share 1/16: 276 -> 72 (3.82), 397 -> 89 (4.48), 602 -> 147 (4.09)
//     share 1/64: 274 -> 60 (4.61), 389 -> 74 (5.23), 594 -> 95 (6.27)
//     share 1/1024: 274 -> 44 (6.18), 379 -> 54 (6.99), 622 -> 63 (9.91)
//   ladder, rows x 384 fp16, share 1/64, one query: 50k 43 -> 33 (1.30), 100k 56 -> 35 (1.58), 250k 64 -> 35 (1.82), 500k 91 -> 36 (2.53), 1000k 145 -> 46 (3.12)
//   HDB_SUBSET_RATIO: the smallest power of two R such that every measured cell with m * ceil(nq / 4) * R <= n is at least 1.10x
//   faster through the list.  R = 1 and R = 2 admit share 1/2 of the 10M x 384 fp16 index, where the masked call streams the int8
//   shadow (4 GB) and the list gathers 3.84 GB of fp16 rows through the VALU: it loses.  R = 4 admits share 1/4 with up to four
//   queries and share 1/16 with sixteen, every cell of which wins by 1.29x or more.
//   HDB_SUBSET_MIN_ROWS: the smallest ladder size from which the list wins by 1.10x at that size and every larger one: 50 000, the
//   smallest size measured (below it: not measured).  It is never below 32 768 rows whatever a measurement says: under a few tens of
//   thousands of rows every call is launch-bound and there is nothing to win.
#define HDB_SUBSET_RATIO 4
#define HDB_SUBSET_MIN_ROWS 50000
static inline bool subset_metric(int metric) {
    return metric == HDB_DOT || metric == HDB_COSINE || metric == HDB_EUCLIDEAN || metric == HDB_MANHATTAN || metric == HDB_PEARSON;
}
// the call's side of the rule: m * ceil(nq / 4) * ratio <= n on a matrix of at least min_n rows
static inline bool subset_rule(const TopkFacts& ix, const hdb_options& o, const TopkCall& c) {
    if (ix.subset_m <= 0 || !o.use_subset || !subset_metric(c.metric) || c.nq < 1) return false;
    if (ix.dtype == HDB_B1) return false;       // packed-bit rows have no list flavour (hdb_bscan.hip): the mask serves, bit for bit
    if (ix.n < (o.subset_min_n >= 0 ? o.subset_min_n : (int64_t)HDB_SUBSET_MIN_ROWS)) return false;
    const int64_t ratio = o.subset_ratio >= 1 ? std::min<int64_t>(o.subset_ratio, (int64_t)1 << 30) : (int64_t)HDB_SUBSET_RATIO;
    return ix.subset_m <= ix.n / (((int64_t)c.nq + 3) / 4 * ratio);
}

// The number of queries of a call from which a float8 index expands its rows in LDS (f8_lds_min_q; the stat of the same name): the
// option, or the measured rule of the width, never below 5 or mfma_min_q; 0 = never
static inline int64_t f8_lds_first_q(const hdb_options& o, int dtype, int d) {
    if (dtype != HDB_F8E4M3) return 0;
    const int64_t rule = o.f8_lds_min_q > 0 ? o.f8_lds_min_q : o.f8_lds_min_q < 0 ? (int64_t)hdb_mfma_f8_lds_min_q(d) : 0;
    return rule > 0 ? std::max<int64_t>(std::max<int64_t>(o.mfma_min_q, 5), rule) : 0;
}

// The number of queries of a call from which a packed-bit index takes the matrix cores (b1_mfma_min_q; the stat of the same name):
// the option, or the measured rule of the width, never below 5 or mfma_min_q; 0 = never (the default, and every width without a kernel)
static inline int64_t b1_mfma_first_q(const hdb_options& o, int dtype, int d) {
    if (dtype != HDB_B1 || (hdb_mfma_b1_tile_rows(d) <= 0 && hdb_mfma_b1_ks_slices(d) <= 0)) return 0;
    const int64_t rule = o.b1_mfma_min_q > 0 ? o.b1_mfma_min_q : o.b1_mfma_min_q < 0 ? (int64_t)hdb_mfma_b1_min_q(d) : 0;
    return rule > 0 ? std::max<int64_t>(std::max<int64_t>(o.mfma_min_q, 5), rule) : 0;
}

// finite(): "are all rows of the matrix finite with a finite sum of squares?"
template <typename Finite>
static inline TopkPlan plan_topk(const TopkFacts& ix, const hdb_options& o, const TopkCall& c, Finite&& finite_fn) {
    int fin_known = -1;                                      // several rules below read the answer: the question is asked once
    auto finite = [&]() -> bool { if (fin_known < 0) fin_known = finite_fn() ? 1 : 0; return fin_known == 1; };
    // A list call is the same call on a matrix of the m listed rows with the matrix cores and the single launches off: the plan of
    // those facts, taken while it is the multi-kernel pipeline (k > HDB_MAX_K on more than HDB_CAND_CAP listed rows keeps the mask).
    // Its extents, sample plan and statistics are the inner plan's; the executor reads the rows through the list.
    // (the exact grouped pass indexes its score buffer by row: it keeps the mask; the multi-vector reduction likewise)
    if (c.n_groups <= 0 && !c.maxsim && subset_rule(ix, o, c)) {
        TopkFacts in{};
        in.n = ix.subset_m; in.d = ix.d; in.dtype = ix.dtype; in.qmode = HDB_QUANT_NONE; in.has_bias = ix.has_bias; in.cus = ix.cus;
        hdb_options oin = o;
        oin.use_mfma = 0; oin.use_fused = 0; oin.use_quant = 0; oin.use_l1_tile = 0;
        TopkPlan pin = plan_topk(in, oin, c, finite_fn);     // (the caller's callable, not the lambda: one instantiation)
        if (pin.path == HDB_PATH_PIPELINE) { pin.subset = true; pin.stats.subset = 1; return pin; }
    }
    TopkPlan p;
    const int64_t n = ix.n;
    const int nq = c.nq, k = c.k, metric = c.metric;
    const uint32_t kk = (uint32_t)std::min<int64_t>(k, n);
    const int W = (ix.d + 31) / 32;
    p.kk = kk; p.W = W;
    const bool is_ham = is_bits_metric(metric), is_pearson = metric == HDB_PEARSON;
    p.bits = is_ham; p.pearson = is_pearson;
    if (n == 0) return p;            // nothing stored: all -1 / -inf
    const bool full_sort = k > HDB_MAX_K && n > HDB_CAND_CAP;
    const bool f64 = ix.dtype == HDB_F64;
    // The exact grouped pass needs every score in a buffer, so a matrix of up to HDB_CAND_CAP rows takes the exact shape too -- on
    // the VALU scan, which is what such a matrix runs on in every other call (`tiny`).  small == tiny wherever n_groups is 0.
    const bool tiny = n <= HDB_CAND_CAP;
    const bool small = tiny && c.n_groups <= 0 && !c.maxsim;      // (the multi-vector score pass: the same, hdb_maxsim_plan.h)
    // bit metrics tie massively by construction; the sampled threshold still works while the rows at and above its
    // level fit the candidate list (random data: yes), and the status word sends the rest through the exact path
    const bool exact_req = c.exact;                          // the caller asked for the exact selection (tests; the re-run of a failed call)
    bool exact = c.exact;
    if (is_ham && !small && !o.bits_fused) exact = true;
    if (o.force_exact && !small) exact = true;
    if (!small && (int64_t)kk * 32 > n) exact = true;        // k is a large share of the rows: a sampled threshold cannot help
    // the int8 shadow (hdb_index_quantize): 1-4 dot / cosine / euclidean queries on a finite float16 / float32 matrix; same answer
    // (bfloat16 likewise: such an index holds a shadow only where its caller set bf16_quant and asked for one.  A bfloat16 call of
    //  1-4 queries never reaches the matrix cores below, so a matrix that is not finite is still asked about once per plan.)
    if (ix.qmode == HDB_QUANT_I8 && !ix.qauto && o.use_quant && !exact && !small && c.has_status && nq >= 1 && nq <= 4 &&
        k <= o.quant_max_k && k <= 128 && (metric == HDB_DOT || metric == HDB_COSINE || metric == HDB_EUCLIDEAN) &&
        (ix.dtype == HDB_F16 || ix.dtype == HDB_F32 || ix.dtype == HDB_BF16) && n >= (o.quant_min_n >= 0 ? o.quant_min_n : quant_min_rows(ix.dtype))) {
        if (finite()) { plan_quant(p, ix, o, c, false); return p; }
    }
    // fp32 matrices: the VALU scan serves up to 4 queries in one pass at HBM speed; the fp32 MFMA scan (matrix-pipe
    // bound at 157 TFLOP/s) takes over where a second VALU pass would start
    // (rows that need K slices -- float32 d >= 1024, fp16 d >= 2048 -- likewise: up to 4 queries are one VALU pass at HBM speed, the
    // slices pay a second launch and the partial sums)
    // float32: up to 4 queries are one VALU pass at HBM speed and the float32 matrix pipe binds early -- but three or four queries on
    // rows of up to 384 elements are faster through the batched single launch from ~300k rows on (n = 2M x 384: 595 / 640 -> 510 us;
    // d = 768: 1 030 vs 1 714, the VALU pass stays)
    const int64_t f32_min_q = o.f32_min_q >= 0 ? o.f32_min_q : ((ix.d <= 384 && n >= 300000) ? 3 : 5);
    // (widths without a geometry of their own ride the next wider one through the multi-kernel pipeline: like the K slices, from five queries on)
    // (bfloat16 rows, hdb_mfma_bf16.hip, likewise: up to 4 queries are one VALU pass with unrounded float32 queries)
    // (... and in K slices, d > 512, from the width's measured crossover with the two VALU passes that 5-8 queries cost: hdb_mfma_bf16_ks_min_q)
    const int64_t bf16_ks_min_q = (ix.dtype == HDB_BF16 && hdb_mfma_ksplit_slices(ix.dtype, ix.d) > 0)
                                      ? (o.bf16_ks_min_q >= 0 ? o.bf16_ks_min_q : (int64_t)hdb_mfma_bf16_ks_min_q(ix.d)) : 0;
    // (float8 rows, hdb_mfma_f8.hip, join bfloat16's rule: up to 4 queries are one VALU pass over one byte per element.  Two such
    //  passes cost half of bfloat16's bytes, so the crossover could have lain above 5 -- measured, it does not: cosine top-100, matrix
    //  cores vs use_mfma = 0 on the same tensor, alternating, p50 in us, spread <= 5 % (profiles/f8_time.txt): 5 queries 10M x 384 1 070
    //  vs 2 902, 2M x 384 260 vs 616, 2M x 128 121 vs 285, 2M x 256 231 vs 421, 2M x 512 307 vs 772; 8 queries 1 073 vs 2 992, 264 vs 637,
    //  123 vs 331, 234 vs 439, 312 vs 793 -- the matrix cores win 1.8-2.8x from the first batch size they are offered)
    // (int8 rows, hdb_mfma_i8.hip: the same bytes through the same kernel with another row converter -- float8's rule; an int8 index
    //  plans like a float8 index whose two opt-ins, f8_ks_min_q and f8_lds_min_q, are 0)
    const int64_t min_q = (hdb_mfma_ksplit_slices(ix.dtype, ix.d) > 0 || hdb_mfma_anyd_pad(ix.dtype, ix.d) > 0 || ix.dtype == HDB_BF16 || ix.dtype == HDB_F8E4M3 || ix.dtype == HDB_I8) ? std::max<int64_t>(std::max<int64_t>(o.mfma_min_q, 5), bf16_ks_min_q)
                        : ix.dtype == HDB_F32 ? std::max<int64_t>(o.mfma_min_q, f32_min_q) : o.mfma_min_q;
    // hdb_mfma_fused_kernel is built around ONE multiplying wave and two selector waves: with 2-4 fp16 queries its sample phase and
    // epilogue cost more than the batched single launch (eight multiplying waves) until the pass itself dominates -- n = 100k x 384,
    // three queries: 124 vs 57 us; 500k: 128 vs 97; 1M: 162 vs 149; 2M: 267 vs 268; 5M: 591 vs 608 (four queries never win).
    // float32 (VALU flavour, two queries): the single launch wins at every size.
    const int64_t fused_max_q = o.fused_max_q >= 0 ? o.fused_max_q
                              : ix.dtype == HDB_F32 ? HDB_FUSED_MAXQ_RULE : (n >= 1500000 ? 3 : 1);
    // (float8 rows wider than 512 elements reach the matrix cores through K slices on request only, f8_ks_min_q != 0: the caps above
    //  answer for the default dispatch, where such rows keep the VALU scan, so the slices have a rule of their own here)
    const int64_t f8_ks_first = (ix.dtype == HDB_F8E4M3 && o.f8_ks_min_q != 0 && hdb_mfma_f8_ks_slices(ix.d) > 0)
                                    ? std::max<int64_t>(std::max<int64_t>(o.mfma_min_q, 5), o.f8_ks_min_q > 0 ? o.f8_ks_min_q : (int64_t)hdb_mfma_f8_ks_min_q(ix.d)) : 0;
    const int metric_mm = is_pearson ? (int)HDB_COSINE : metric;
    const bool f8ks_call = f8_ks_first > 0 && nq >= f8_ks_first && (metric_mm == HDB_DOT || metric_mm == HDB_COSINE || metric_mm == HDB_EUCLIDEAN);
    // (packed-bit rows reach the matrix cores on request only as well, b1_mfma_min_q != 0 -- whole rows of up to 512 elements and the
    //  K slices of wider ones, hdb_mfma_b1.h.  The matrix is always finite -- its flag word is never written -- so nothing is asked.)
    const int64_t b1_first = b1_mfma_first_q(o, ix.dtype, ix.d);
    const bool b1_call = b1_first > 0 && nq >= b1_first && (metric_mm == HDB_DOT || metric_mm == HDB_COSINE || metric_mm == HDB_EUCLIDEAN);
    bool mfma = o.use_mfma && !is_ham && !small && !tiny && ((nq >= min_q && hdb_mfma_supported(ix.dtype, ix.d, metric_mm)) || f8ks_call || b1_call);
    // The matrix cores score euclidean through ||v||^2 + ||q||^2 - 2 v.q, which cancels where v is close to q; every other call
    // re-scores its few candidates directly (hdb_launch_rescore_euclid).  The multi-vector reduction consumes EVERY score of the pass,
    // and the near-duplicate of a query vector is exactly the row a group's maximum picks: its euclidean score pass stays on the VALU
    // scan, which sums the differences themselves.
    if (c.maxsim && metric == HDB_EUCLIDEAN) mfma = false;
    // bfloat16 rows meet three query parts, two of them zero where the query is a bf16 number: a row holding inf would give
    // inf x 0 = NaN where np.dot gives inf, so a matrix that is not finite stays on the VALU scan
    // (float8 rows: a NaN code times a zero part is NaN where the VALU scan's NaN -> -inf ranking is the contract; same rule)
    // (int8 rows are always finite -- 512 x 128^2 is far from overflow -- and the flag their row norms leave says so: the same question, always yes)
    if (mfma && (ix.dtype == HDB_BF16 || ix.dtype == HDB_F8E4M3 || ix.dtype == HDB_I8)) mfma = finite();
    // fp16 / float32 rows narrower than the geometry they ride (hdb_mfma_anyd.h): the chunks past the end of a row are chunk 0 of
    // the row again and meet zero query fragments -- an infinite element in a row's first 16 bytes gives inf x 0 = NaN there where
    // np.dot gives the infinity.  Same rule: a matrix that is not finite stays on the VALU scan.
    if (mfma && hdb_mfma_anyd_pad(ix.dtype, ix.d) > 0) mfma = finite();
    // The automatic int8 shadow (auto_quant): a call of 1-4 dot / cosine queries that the matrix cores would answer on a large finite
    // fp16 matrix reads the shadow instead and rescoring returns the matrix cores' bits (quant_topk, mflavour).  The index builds
    // the shadow on its first such call (build_needed); an explicit shadow (hdb_index_quantize) keeps its own rule and the VALU bits above.
    const bool f8ks = mfma && f8ks_call;
    const bool b1mm = mfma && b1_call, b1ks = b1mm && hdb_mfma_b1_ks_slices(ix.d) > 0;
    const bool auto_q = auto_quant_call(ix, o, c, mfma, exact, small);
    if (auto_q && nq >= 1 && nq <= 4 &&
        // (rows wider than 512 elements join only on request: their bounds pass too many candidates on large matrices, see quant_sample_target)
        (o.quant_min_n >= 0 ? n >= o.quant_min_n : (n >= (int64_t)HDB_QUANT_AUTO_MIN_ROWS && ix.d <= 512))) {
        if (finite()) { plan_quant(p, ix, o, c, true); return p; }
    }
    // ... and batches of 5+ queries (hdb_quant_mfma.hip): the same conditions under a row rule of their own (quant_batch_min_n), for the
    // widths the int8 matrix-core pass takes and the 16x16x32 form of the fp16 scan, whose bits the rescoring returns
    if (auto_q && nq >= 5 && hdb_qb_supported(ix.d) && o.mfma_variant == 16 &&
        (o.quant_batch_min_n >= 0 ? n >= o.quant_batch_min_n : (quant_batch_rule(ix.d, nq) > 0 && n >= quant_batch_rule(ix.d, nq)))) {
        if (finite()) { plan_quant_batch(p, ix, o, c); return p; }
    }
    // 1-4 dot / cosine queries, k <= 128: one launch does everything (hdb_mfma_fused.h; fp16 on the matrix cores,
    // float32 in the VALU from the same staged tiles)
    // Short matrices: the single launch in its LOCAL flavour -- no row sample, no exchange; every workgroup parks the scores of all
    // its tiles and emits the rows at or above its own local_m-th best (hdb_mfma_fused.h).  Possible while a workgroup's tiles fit
    // its parking area (up to 16); used, by measurement (profiles/r4_latency_map.txt, same box, interleaved), up to local_max_tiles =
    // 4 tiles per workgroup (fp16 d = 384: 65 536 rows): 35 vs 37 us at 20k rows, 45 vs 45 at 100k, 62 vs 59 at 250k -- beyond that
    // the exchange flavour filters while it streams and the local one selects after its last tile.  Matrices of up to 8192 rows keep
    // the three launches (thr = -inf, scan, finalize): 26 us at 1000 rows against 31 for this kernel's launch ramp and last workgroup.
    const int fl_rows = hdb_mfma_tile_rows(ix.dtype, ix.d);
    const int64_t fl_tiles = fl_rows > 0 ? (n + fl_rows - 1) / fl_rows : 0;
    const int64_t fl_grid = fl_rows > 0 ? hdb_mfma_fused_blocks(fl_tiles, ix.cus, (int)o.max_blocks) : 0;
    const int fl_cap = fl_rows > 0 && nq >= 1 && nq <= HDB_FUSED_MAXQ_RULE && nq <= o.local_max_q ? hdb_mfma_fused_local_tiles(ix.dtype, ix.d, metric, nq) : 0;
    const bool local_ok = fl_grid * 32 <= HDB_CAND_CAP && o.use_fused && o.use_local && !o.force_exact && !exact_req && (ix.dtype == HDB_F32 || (o.use_mfma && nq >= o.mfma_min_q)) && fl_grid > 0 && fl_cap > 0 && (fl_tiles + fl_grid - 1) / fl_grid <= std::min<int64_t>(fl_cap, o.local_max_tiles) && (!small || o.local_small) &&
                          !is_ham && kk <= 128 && c.has_status && hdb_mfma_fused_supported(ix.dtype, ix.d, metric, nq, kk);
    if (local_ok) exact = false;                       // (k a large share of the rows: every workgroup then emits all its rows)
    const bool fused_shape = o.use_fused && !exact && (!small || local_ok) && k <= HDB_MAX_K && c.has_status && !is_ham &&
                             hdb_mfma_fused_supported(ix.dtype, ix.d, metric, nq, kk) && (ix.dtype == HDB_F32 || mfma || local_ok) && (nq <= fused_max_q || local_ok) &&
                             // float32 d = 512 streams 32-KiB tiles (16 rows): below ~3 GB the five-kernel VALU pipeline is
                             // 2-5 % faster end to end (200 vs 210 us at 0.5 M rows, 376 vs 385 at 1 M; 728 vs 687 at 2 M)
                             !(ix.dtype == HDB_F32 && ix.d == 512 && n < 1500000) &&
                             // fp16 d = 1024 (32-KiB tiles, 32 k-steps in one wave): 189 vs 195 us at 0.5 M rows, 619 vs 627 at 2 M,
                             // but 1 491 vs 1 466 at 5 M -- the single launch up to 4 M rows
                             !(ix.dtype == HDB_F16 && ix.d == 1024 && n > 4000000);
    const int tile_rows = (f8ks || b1mm) ? 16 : (mfma || fused_shape) ? hdb_mfma_tile_rows(ix.dtype, ix.d) : 16;      // (float8 slices, packed bits: the 16-row tiles of the register kernels)
    // float32 rows on the matrix cores multiply in three bf16 parts (hdb_mfma_f32s.hip: 2.7x the rate of the float32 MFMAs, same
    // 1e-5 contract) -- on finite matrices: the parts of an infinite element would cancel to NaN where np.dot keeps the infinity
    // Two parts keep 16 mantissa bits of a row value, so the product's error is up to 2^-17 |v| |q| whatever the score:
    //   cosine / pearson divide it by |v| |q| (2^-17 = 7.6e-6 at the very worst, measured 3e-7: inside 1e-5 for every row);
    //   euclidean adds |v|^2 + |q|^2 before the root and 1 / (1 + .): a score error below 2^-17 as well;
    //   dot_product keeps it as it is: a row whose score is small against |v| |q| (a selective filter, a large k, data that share a
    //   dominant direction) misses 1e-5 * max(1, |s|) -- |v| = 20, |q| = 2, |s| < 1: up to 2.3 bands (tests/test_low_score_contract.py).
    // So dot_product runs on the float32 MFMAs, which exist for every shape the parts have.
    // The parts of an infinite QUERY element cancel to NaN too, which the parts flavour reports as HDB_Q_UNDERFLOW -- to the exact
    // re-run.  A call that asks for the exact selection (hdb_topk_exact, exact_req) is that last resort and keeps the parts, and with
    // them the default call's bits, only while no query of the call holds an infinity: a fact of the queries, so the executor looks
    // (run_pipeline reads the flags its query preparation left) and multiplies in float32 otherwise.
    bool f32s = false;
    const int f32s_auto = hdb_mfma_f32_split_min_q(ix.d);
    const int f32s_min = f32s_auto > 0 ? (int)(o.f32_split_min_q > 0 ? o.f32_split_min_q : f32s_auto) : 0;       // queries of the CALL (every launch of a call multiplies the same way)
    if (mfma && ix.dtype == HDB_F32 && o.f32_split && metric != HDB_DOT && f32s_min > 0 && nq >= f32s_min && nq <= hdb_mfma_f32_split_max_q(ix.d)) f32s = finite();
    // anything else the matrix-core scan takes (5-256 dot / cosine queries, 1-256 euclidean ones), k <= 128: one launch per
    // <= bcap queries does preparation, sample, thresholds, the pass and every query's final sort (hdb_mfma_kernel.h, MODE 2)
    const int bcap = mfma ? hdb_mfma_batch_capacity(ix.dtype, ix.d) : 0;
    const bool batch1 = o.use_fused && o.use_batch1 && mfma && !fused_shape && !exact && !small && !full_sort && kk <= 128 &&
                        c.has_status && bcap > 0;

    // ---- plan the chunking --------------------------------------------------------------------
    int64_t s_tiles = 0, s_stride = 1; uint32_t m = 0;
    if (!small && !exact) sample_plan(n, o.sample_target, kk, nq, tile_rows, is_ham, s_tiles, s_stride, m);
    const int64_t s_rows = s_tiles * tile_rows;
    const int64_t ld_s = align_up((size_t)std::max<int64_t>(s_rows, 4), 4);
    const int64_t ld_n = align_up((size_t)n, 4);
    int cq_max = batch1 ? bcap : 256;
    // (the per-group maxima of the exact grouped pass, 8 bytes per query and group, count against exact_bytes beside the scores)
    const int64_t n_best = c.n_groups > 0 ? c.n_groups : 0;
    if (exact && !small) cq_max = (int)std::max<int64_t>(1, std::min<int64_t>(256, o.exact_bytes / (ld_n * 4 + n_best * 8)));
    // wide rows on the matrix cores go through K slices with a [query][rows] buffer of partial sums (hdb_mfma_ksplit.hip)
    const bool ksplit = mfma && (hdb_mfma_ksplit_slices(ix.dtype, ix.d) > 0 || f8ks || b1ks);
    if (ksplit && !small) cq_max = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(cq_max, 128), o.exact_bytes / (ld_n * 4 + n_best * 8)));
    cq_max = std::min(cq_max, (int)nq);
    const bool fused = fused_shape && !full_sort && (m == 8 || local_ok);           // (no prep kernel either)
    // hamming / jaccard: the single launch for every call (with the two-level hand-out of the pass: one query 120-124 vs 125-132 us
    // for the six launches at N=10M, 78 vs 77 at 5M, 60 vs 63 at 1.25M, 44 vs 52 at 250k rows; four queries 135 vs 172 at N=10M --
    // profiles/r3_bits_variants.txt; bits_fused = 3 keeps one-query calls on 1M+ rows with the six launches, for comparison)
    const bool bits1 = o.use_fused && o.bits_fused && is_ham && !exact && !small && !full_sort && !f64 && c.has_status &&
                       hdb_bits_fused_supported(metric, 1, W, kk) && (nq >= 2 || n < 1000000 || o.bits_fused != 3) &&
                       // (more than four queries: the six launches take them all in one go, grid.y = query groups -- 16 queries on
                       // 100k rows 50 vs 148 us for four single launches in a row, 64 queries 67 vs 642; 10M rows 464 vs 524)
                       nq <= (o.bits_max_q >= 0 ? o.bits_max_q : 4);
    // float8 batches with the rows expanded in LDS once per workgroup (f8_lds_min_q, opt-in): whatever the float8 matrix cores take --
    // a whole row or the K slices -- from the threshold's number of queries on; sample, filter and exact pass alike.  Nothing else of
    // the plan changes: the tiles stay 16 rows, so the sample rows, the thresholds and with them the answers are the register flavour's
    const int64_t f8_lds_first = f8_lds_first_q(o, ix.dtype, ix.d);
    p.f8_lds = mfma && ix.dtype == HDB_F8E4M3 && !full_sort && (f8ks || hdb_mfma_f8_lds_supported(ix.d)) && f8_lds_first > 0 && nq >= f8_lds_first;
    p.stats.f8_lds = p.f8_lds ? 1 : 0;
    p.exact = exact; p.exact_req = exact_req; p.small = small; p.mfma = mfma; p.f32s = f32s; p.ksplit = ksplit; p.local = local_ok;
    p.tile_rows = tile_rows; p.s_tiles = s_tiles; p.s_stride = s_stride; p.m = m; p.s_rows = s_rows; p.ld_s = ld_s; p.ld_n = ld_n;
    p.cq_max = cq_max; p.n_best = n_best;
    // full sort (k > HDB_MAX_K): all scores of one query, the sort's work array and its scratch live in the same layout
    p.ld_scores = exact && !small ? ld_n : ld_s; p.ld_ks = ksplit ? ld_n : 0; p.sort_n = full_sort ? n : 0;
    p.path = fused ? HDB_PATH_FUSED : bits1 ? HDB_PATH_BITS1 : batch1 ? HDB_PATH_BATCH1 : full_sort ? HDB_PATH_FULL_SORT : HDB_PATH_PIPELINE;
    // the single launches prepare (sign, centre) their queries themselves; the other two paths with launches of their own:
    p.prep = !p.single_launch();
    // the MFMA scan multiplies with fp16 queries: written by the same kernel (pearson converts its centred copy later)
    p.f16_queries = mfma && ix.dtype == HDB_F16;          // fp32 matrices multiply with the float32 queries as they are
    p.q16_in_prep = p.f16_queries && !is_pearson && !full_sort;
    // matrices of up to 8192 rows, one chunk of queries: the prep kernel also sets thr = -inf / an empty list and packs the query sign
    // bits -- four (five) launches become three; the reference's own sizes live here (151 .. 10 000 documents)
    p.fold_small = small && p.path == HDB_PATH_PIPELINE && nq <= cq_max;
    // the MFMA scan has no mask input: excluded rows get a bias of -inf instead (never appended, like the VALU scan)
    // (run_scan hands manhattan calls of two or more queries to the tile kernel; a single query keeps the VALU scan and its mask input)
    p.l1tile = metric == HDB_MANHATTAN && o.use_l1_tile && !small && !tiny && nq >= 2 && hdb_l1_tile_supported(ix.dtype, ix.d);
    p.mask_fold = (mfma || fused || p.l1tile) && ix.has_mask && !full_sort;
    p.stats.f32s = f32s ? 1 : 0; p.stats.sample_rows = s_rows; p.stats.sample_m = m; p.stats.path = 1;
    switch (p.path) {
    case HDB_PATH_FUSED:
        // local flavour: rows every workgroup emits at least: ~3072 candidates in all (8 .. 32 per workgroup); a grid too small to hold 4 k rows
        // that way emits everything (64 = every lane maximum of a tile)
        // slots of a workgroup in the (slotted) lists: 64 while the grid leaves room for them, else 32; never fewer than twice local_m
        if (local_ok) {
            p.local_slot = fl_grid * 64 <= HDB_CAND_CAP ? 64u : 32u;
            p.local_m = o.local_m > 0 ? (uint32_t)o.local_m
                      : fl_grid * 32 >= 4 * (int64_t)kk ? (uint32_t)std::min<int64_t>(p.local_slot / 2, std::max<int64_t>(8, (3072 + fl_grid - 1) / fl_grid)) : 64u;
        }
        p.stats.local = local_ok ? 1 : 0; p.stats.chunks = 1; p.stats.mfma = ix.dtype == HDB_F16 ? 1 : 0; p.stats.fused = 1;
        break;
    case HDB_PATH_BITS1:
        p.bits_local = o.bits_local ? 1 : 0;
        p.stats.fused = 3; p.stats.chunks = (nq + 3) / 4;
        p.stats.local = (p.bits_local && hdb_bits_fused_local(hdb_bits_fused_blocks((n + 15) / 16, ix.cus, (int)o.max_blocks), kk)) ? 1 : 0;
        break;
    case HDB_PATH_BATCH1:
        p.stats.fused = 2; p.stats.mfma = 1; p.stats.chunks = (nq + cq_max - 1) / cq_max;
        break;
    case HDB_PATH_FULL_SORT:
        // cold path for huge k: one query at a time, all scores -> stable radix sort (hdb_sort.hip)
        p.stats.path = 3; p.stats.chunks = nq; p.stats.sample_rows = 0; p.stats.sample_m = 0;
        break;
    default:
        p.stats.path = small ? 0 : (exact ? 2 : 1); p.stats.mfma = mfma ? 1 : 0; p.stats.chunks = (nq + cq_max - 1) / cq_max;
        // hamming scores are integers in [0, d]: their float keys are zero below the top 8 + bits(d) bits, so the
        // last radix pass (the last two for d < 128) would only re-read the scores to find every key in bin 0
        if (metric == HDB_HAMMING && !ix.has_bias && !ix.has_mask) {
            int bits = 0;
            while ((ix.d >> bits) != 0) ++bits;
            p.npass = std::min(4, (8 + bits + 7) / 8);
        }
        break;
    }
    return p;
}
