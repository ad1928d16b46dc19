// hdb_ws.h -- the layouts of the per-index scratch workspace (hdb_index::ws), each written ONCE.
//
// A layout is a struct of pointers with one member, lay(Bump&, extents...), that takes its regions in order.  The same
// function sizes the workspace (a Bump without a base only advances its offset) and places the pointers (a Bump on the real
// buffer), so the size and the pointers cannot drift apart.  Plain extents in, no hdb_index: tests/test_ws_layout.py runs the
// layouts on the host over a grid of shapes.
// The sample plans of the shadow paths, which give those layouts their extents, are here for the same reason.
#pragma once
#include "hdb_common.h"
#include "hdb_quant.h"
#include <algorithm>

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Regions of 256-byte alignment, one after the other.  base == nullptr: sizing mode, take() returns nullptr.
struct Bump {
    char* base; size_t cap, off = 0;
    Bump(char* b, size_t c) : base(b), cap(c) {}
    template <typename T> T* take(size_t count) {
        off = align_up(off, 256);
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
};

// bytes a layout needs for these extents
template <typename WS, typename... Ext>
static inline size_t ws_bytes_for(Ext... ext) {
    WS w; Bump dry(nullptr, 0);
    w.lay(dry, ext...);
    return dry.off;
}

// hdb_scores: one query
struct ScoresWs {
    float* qinv; float* qsq; int* qnan; uint32_t* qbits; void* qc;
    void lay(Bump& b, int d, int W) {
        qinv = b.take<float>(1); qsq = b.take<float>(1); qnan = b.take<int>(1);
        qbits = b.take<uint32_t>((size_t)W);
        qc = b.take<double>((size_t)d);
    }
};

// The main pipeline (topk_impl): per-query words of the whole call, then the buffers of one chunk of cq queries.
// ld_scores: leading dimension of the score buffer (the sample's, or all rows on the exact path); ld_ks: of the partial sums of
// the K slices (0: none); sort_n > 0: the three buffers of the full sort (k > HDB_MAX_K), sort_temp bytes of radix-sort scratch.
// n_best > 0 (the exact grouped pass, hdb_topk_grouped_host): the per-group maxima of a chunk, [cq][n_best] 64-bit keys, and the
// word its demote launch raises on a bad group id; every other call passes 0 and gets neither.
struct TopkWs {
    float* qinv; float* qsq; int* qnan; float* qscl; uint32_t* qbits; void* q16; void* qc;
    float* thr; uint32_t* cnt; uint32_t* tile_ctr; uint32_t* hist; uint32_t* tie_info; unsigned long long* cand;
    float* sbuf; float* kbuf;
    float* sc1; uint32_t* work; void* temp;
    unsigned long long* best; int* gbad;
    void lay(Bump& b, int nq, int d, int W, int cq, int64_t ld_scores, int64_t ld_ks, int64_t sort_n, size_t sort_temp, int64_t n_best = 0) {
        qinv = b.take<float>(nq); qsq = b.take<float>(nq); qnan = b.take<int>(nq); qscl = b.take<float>(nq);
        qbits = b.take<uint32_t>((size_t)nq * W);
        q16 = b.take<uint16_t>((size_t)nq * d);                         // fp16 queries (MFMA)
        qc = b.take<double>((size_t)nq * d);                            // centred queries (pearson)
        thr = b.take<float>(cq);
        cnt = b.take<uint32_t>((size_t)cq * HDB_CNT_STRIDE);            // a cache line per query; hist follows it (one memset clears both)
        tile_ctr = b.take<uint32_t>(64);
        hist = b.take<uint32_t>((size_t)cq * 4 * HDB_RADIX_BINS);
        tie_info = b.take<uint32_t>((size_t)cq * 4);
        cand = b.take<unsigned long long>((size_t)cq * HDB_CAND_CAP);
        sbuf = b.take<float>((size_t)cq * ld_scores);
        kbuf = ld_ks > 0 ? b.take<float>((size_t)cq * ld_ks) : nullptr;
        sc1 = nullptr; work = nullptr; temp = nullptr;
        if (sort_n > 0) {
            sc1 = b.take<float>(align_up((size_t)sort_n, 4));
            work = b.take<uint32_t>((size_t)sort_n * 4);
            temp = b.take<char>(sort_temp);
        }
        best = nullptr; gbad = nullptr;
        if (n_best > 0) {
            best = b.take<unsigned long long>((size_t)cq * (size_t)n_best);
            gbad = b.take<int>(1);
        }
    }
};

// hdb_maxsim_host: the main pipeline's layout for the call's nq flat vectors in chunks of cq (exact shape: ld_scores = all rows), then
// the running sums of a block of sb sets, acc [sb][ld_g], the call's set offsets and per-set NaN words on the device, and the
// selection's buffers for sb sets (cnt and hist neighbours, as in TopkWs: one memset clears both).
struct MaxsimWs {
    TopkWs t;
    float* acc; int32_t* voff; int* snan;
    uint32_t* cnt; uint32_t* hist; uint32_t* tie_info; unsigned long long* cand;
    void lay(Bump& b, int nq, int d, int W, int cq, int64_t ld_scores, int64_t ld_ks, int sb, int64_t ld_g, int ns) {
        t.lay(b, nq, d, W, cq, ld_scores, ld_ks, 0, 0, 0);
        acc = b.take<float>((size_t)sb * (size_t)ld_g);
        voff = b.take<int32_t>((size_t)ns + 1);
        snan = b.take<int>((size_t)ns);
        cnt = b.take<uint32_t>((size_t)sb * HDB_CNT_STRIDE);
        hist = b.take<uint32_t>((size_t)sb * 4 * HDB_RADIX_BINS);
        tie_info = b.take<uint32_t>((size_t)sb * 4);
        cand = b.take<unsigned long long>((size_t)sb * HDB_CAND_CAP);
    }
};

// hdb_mmr: the buffers of one chunk of cq queries (hdb_mmr_plan.h).  mp: the list length rounded up to the pair tile -- the
// candidates' local rows and relevances in list order, their counts, and the pair matrix P [cq][mp][mp].
struct MmrWs {
    uint32_t* rows; float* rel; int32_t* cnt; float* P;
    void lay(Bump& b, int cq, int mp) {
        rows = b.take<uint32_t>((size_t)cq * mp);
        rel = b.take<float>((size_t)cq * mp);
        cnt = b.take<int32_t>((size_t)cq);
        P = b.take<float>((size_t)cq * mp * mp);
    }
};

// hdb_rerank: per-query words of the whole call, then the buffers of one chunk of cq queries.  m: the caller's list length -- the
// prepared lists (valid, ascending, unique local rows) have that leading dimension; the packed entries keep the leading dimension
// HDB_CAND_CAP the finalize kernel is launched with.  pearson: the centred queries.
struct RerankWs {
    float* qinv; float* qsq; int* qnan; void* qc; uint32_t* cnt; int64_t* rows; unsigned long long* cand;
    void lay(Bump& b, int nq, int d, int cq, int m, bool pearson) {
        qinv = b.take<float>(nq); qsq = b.take<float>(nq); qnan = b.take<int>(nq);
        qc = pearson ? b.take<double>((size_t)nq * d) : nullptr;
        cnt = b.take<uint32_t>((size_t)cq * HDB_CNT_STRIDE);
        rows = b.take<int64_t>((size_t)cq * m);
        cand = b.take<unsigned long long>((size_t)cq * HDB_CAND_CAP);
    }
};

// ---- sample plans of the shadow paths -----------------------------------------------------------------------------------------
// The strided row sample: s_tiles 16-row tiles spread evenly over the matrix, one score per sampled row and query in a buffer of
// leading dimension ld_s.
struct QuantSample { int64_t s_tiles, s_stride, s_rows, ld_s; };
static inline QuantSample quant_sample(int64_t n, int64_t s_tiles) {
    QuantSample p;
    p.s_tiles = s_tiles;
    p.s_stride = std::max<int64_t>(1, (n / 16) / s_tiles);
    p.s_rows = s_tiles * 16;
    p.ld_s = (int64_t)align_up((size_t)std::max<int64_t>(p.s_rows, 4), 4);
    return p;
}
// Rows of the whole matrix the sampled threshold T_s aims to leave with a LOWER bound above it: 512 (a sample of 16 keeps P(fewer
// than k = 128 such rows) near 1e-5).  The UPPER bounds let exp(z delta - delta^2 / 2) times as many through, delta = 2B / sigma =
// 0.029 sqrt(d) standard deviations of the scores for Gaussian rows: ~8x at d = 384, 10-14x at d = 768, where 512 would overflow
// the candidate list.  Rows wider than 512 elements therefore aim at 4k (at least 256: the sample is 16 n / target rows).
static inline int64_t quant_sample_target(int d, uint32_t kk) {
    return d > 512 ? std::min<int64_t>(512, std::max<int64_t>(256, 4 * (int64_t)kk)) : 512;
}
static inline int64_t quant_sample_tiles(int64_t n, int64_t target) {
    const int64_t all_tiles = n / 16;
    int64_t s_tiles = ((std::max<int64_t>((int64_t)(16.0 * (double)n / (double)target), 256)) + 15) / 16;
    return std::max<int64_t>(1, std::min(s_tiles, all_tiles));
}
// the sample of a 1-4-query call, and the largest one any k takes (k = 1: the smallest target): the extent QuantWs is sized for
static inline QuantSample quant_call_sample(int64_t n, int d, uint32_t kk) { return quant_sample(n, quant_sample_tiles(n, quant_sample_target(d, kk))); }
static inline int64_t quant_ld_max(int64_t n, int d) { return quant_call_sample(n, d, 1).ld_s; }
// Sample plan of a batch.  T_s is the m-th largest sampled lower bound; the rows of the whole matrix with a LOWER bound above it
// number about target x Gamma(m) / m.  A batch pays for its worst query on both sides (too few: the floor check fails; too many: the
// upper bounds, exp(z delta) times as many, overflow the list), so the batch plan narrows the spread with m = 32 instead of 16 and
// aims lower, at 320 rows: P(fewer than k = 128 such rows) = P(Gamma(32) < 12.8) ~ 1e-5 per query, and the +3 sigma query of 256
// stands at 320 x 49 / 32 = 490 rows where the 1-4-query plan's would stand at 512 x 28 / 16 = 896.  The sample is m / target = a
// tenth of the rows (the CPU model's m = 64 / target 256 would read a quarter of the shadow a second time).
#define HDB_QB_SAMPLE_M 32
#define HDB_QB_SAMPLE_TARGET 320
static inline QuantSample quant_batch_sample(int64_t n) {
    const int64_t rows = std::max<int64_t>((int64_t)((double)HDB_QB_SAMPLE_M * (double)n / (double)HDB_QB_SAMPLE_TARGET), 16 * HDB_QB_SAMPLE_M);
    return quant_sample(n, std::max<int64_t>(1, std::min((rows + 15) / 16, n / 16)));
}

// 1-4 queries through the int8 shadow (quant_topk, hdb_debug_quant_bounds).  ld_s: the score buffer's extent per query -- the
// largest sample any k takes, so that calls that differ in k never regrow the workspace; pl_cap: 4-byte entries of a list beside
// the score buffer (0: none) -- the upper bounds of the sampled rows, which the sample pass of a one-query call leaves for the pass
// over the 5-bit plane (QuantArgs::pl_hi; one per sample slot, so the same extent as ld_s); mflavour: the compact matrix and the
// score block of the matrix-core rescoring.
struct QuantWs {
    float* qinv; float* qsq; int* qnan; int8_t* qcodes; float* qaux; float* thr; uint32_t* cnt; unsigned long long* cand; float* sbuf;
    uint32_t* pl_list;
    void* q16; float* qscl; char* G; float* ginv; float* gbias; float* gsc; uint32_t* wmax;
    void lay(Bump& b, int nq, int P, int d, int64_t ld_s, uint32_t pl_cap, bool mflavour) {
        qinv = b.take<float>(nq); qsq = b.take<float>(nq); qnan = b.take<int>(nq);
        qcodes = b.take<int8_t>((size_t)nq * P);
        qaux = b.take<float>((size_t)nq * HDB_QQ_WORDS);
        thr = b.take<float>(nq);
        cnt = b.take<uint32_t>((size_t)nq * HDB_CNT_STRIDE);
        cand = b.take<unsigned long long>((size_t)nq * HDB_CAND_CAP);
        sbuf = b.take<float>((size_t)nq * ld_s);
        pl_list = pl_cap ? b.take<uint32_t>(pl_cap) : nullptr;
        q16 = nullptr; qscl = nullptr; G = nullptr; ginv = nullptr; gbias = nullptr; gsc = nullptr; wmax = nullptr;
        if (mflavour) {
            const size_t crow = (size_t)nq * HDB_CAND_CAP;              // rows of the compact matrix
            q16 = b.take<uint16_t>((size_t)nq * d); qscl = b.take<float>(nq);
            G = b.take<char>(crow * d * 2); ginv = b.take<float>(crow); gbias = b.take<float>(crow); gsc = b.take<float>((size_t)nq * crow);
            wmax = b.take<uint32_t>((size_t)nq * HDB_QUANT_NSUB_MAX);   // per-wave maxima of the sample pass
        }
    }
};

// One chunk of cq <= 256 queries of a batch through the shadow (quant_batch_topk).  wld: slots the sample pass leaves per query.
struct QuantBatchWs {
    float* qinv; float* qsq; int* qnan; float* qscl; int8_t* qcodes; float* qaux; float* thr; uint32_t* cnt; unsigned long long* cand;
    void* q16; float* wbuf;
    void lay(Bump& b, int cq, int P, int d, int64_t ld_s, int64_t wld) {
        qinv = b.take<float>(cq); qsq = b.take<float>(cq); qnan = b.take<int>(cq); qscl = b.take<float>(cq);
        qcodes = b.take<int8_t>((size_t)cq * P);
        qaux = b.take<float>((size_t)cq * HDB_QQ_WORDS);
        thr = b.take<float>(cq);
        cnt = b.take<uint32_t>((size_t)cq * HDB_CNT_STRIDE);
        cand = b.take<unsigned long long>((size_t)cq * HDB_CAND_CAP);
        q16 = b.take<uint16_t>((size_t)cq * d);
        wbuf = b.take<float>(std::max((size_t)cq * wld, (size_t)4 * ld_s));     // slot maxima (kernel 1) / sampled lower bounds of four queries (kernel 0)
    }
};
