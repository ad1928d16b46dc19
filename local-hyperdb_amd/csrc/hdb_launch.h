// hdb_launch.h -- every function that crosses a translation unit of the library and is not part of the public ABI
// (include/hyperdb_hip.h): the launchers of the kernel units and the size helpers beside them.  (What a unit can take and the grid
// its launcher uses are inline rules in hdb_caps.h: definitions, not prototypes.)
//
// The names are extern "C", so a call through a stale prototype would still link and the callee would read the wrong
// registers.  Each function is therefore declared HERE ONLY, and every unit that defines one sees this header (through
// hdb_common.h): a definition that drifts from its declaration fails to compile with "conflicting types".
// tests/test_launchers_declared_once.py keeps both halves of that true.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct ScanArgs;        // hdb_common.h
struct FusedArgs;
struct BatchArgs;
struct MfmaLaunch;
struct BitsArgs;
struct QuantArgs;       // hdb_quant.h

// shards of the matrix-core scan: one launcher per geometry, all with ONE signature -- the scan and the launch record
#define HDB_GEOM_DECL(name) int name(const ScanArgs* args, const MfmaLaunch* l)

extern "C" {
// ---- hdb_scan.hip: the VALU row scan, per-row caches, query prep ----
int hdb_launch_scan(const ScanArgs* args, int dtype, int mode, int nq_launch, int max_blocks, void* stream);
int hdb_launch_list_rows(unsigned long long* cand, const uint32_t* cnt, uint32_t cap, int nq, const int64_t* rows, int64_t m, void* stream);
int hdb_launch_rownorm(const void* V, int64_t n, int d, int dtype, float* inv_norm, float* sqnorm, int* nan_flag, void* stream);
int hdb_launch_qprep(const void* Q, int nq, int d, bool f64, float* qinv, float* qsq, int* qnan, void* q16, float* qscl, void* stream);
int hdb_launch_qprep2(const void* Q, int nq, int d, bool f64, float* qinv, float* qsq, int* qnan, void* q16, float* qscl,
                      float* thr_init, uint32_t* cnt_init, uint32_t* qbits, int W, void* stream);
int hdb_launch_signpack(const void* V, int64_t n, int d, int dtype, int64_t row0, uint32_t* bits, void* stream);
int hdb_launch_qsign(const void* Q, int nq, int d, bool f64, int W, uint32_t* qbits, void* stream);
int hdb_launch_hamming(const ScanArgs* args, int mode, int nq_launch, const uint32_t* bits, int64_t npad, int W,
                       const uint32_t* qbits, void* stream);
int hdb_launch_maskbias(const uint8_t* mask, const float* bias, int64_t n, float* out, void* stream);
int hdb_launch_recency(const double* ts, int64_t n, double rb, double ts_max, float* out, void* stream);
int hdb_launch_recency2(const double* ts, const uint8_t* mask, int64_t n, double rb, double ts_max, double first_max, float* out, void* stream);
int hdb_launch_rowstats(const void* V, int64_t n, int d, int dtype, float* pscale, void* stream);
int hdb_launch_qcentre(const void* Q, int nq, int d, bool f64, void* Qc, float* qscale, void* stream);

// ---- hdb_bscan.hip: float32 queries against packed-bit rows (HDB_B1); reached from hdb_launch_scan ----
int hdb_launch_bscan(const ScanArgs* args, int mode, int nq_launch, int max_blocks, void* stream);

// ---- hdb_select.hip: thresholds, collection, finalize, merge ----
int hdb_launch_hist(const float* scores, int64_t n, int64_t ld, int nq, uint32_t* hist, int pass, uint32_t k, void* stream);
int hdb_launch_thr(const uint32_t* hist, int nq, int npass, uint32_t m, uint32_t sample_n, float* thr, uint32_t* cnt, void* stream);
int hdb_launch_fill_thr(float* thr, uint32_t* cnt, int nq, float v, void* stream);
int hdb_launch_sample_thr(const float* scores, int64_t n, int64_t ld, int nq, uint32_t m, float* thr, uint32_t* cnt, uint32_t* tile_ctr, void* stream);
int hdb_launch_collect(const float* scores, int64_t n, int64_t ld, int nq, const uint32_t* hist, int npass, uint32_t k, uint32_t* cnt,
                       unsigned long long* cand, uint32_t cap, uint32_t* tie_info, void* stream);
int hdb_launch_finalize(const unsigned long long* cand, const uint32_t* cnt, uint32_t cap, int nq, uint32_t k, uint32_t kk,
                        int64_t row_base, int64_t* idx_out, float* score_out, int32_t* status, const int* qnan, int threads, int inf_status, void* stream);
int hdb_launch_status_nan(const int* qnan, int nq, int32_t* status, void* stream);
int hdb_launch_merge(const void* idx_base, int64_t idx_stride, const void* score_base, int64_t score_stride,
                     const void* status_base, int64_t status_stride, int parts, int nq, uint32_t k, int64_t* idx_out,
                     float* score_out, int32_t* status_out, void* stream);

// ---- hdb_sort.hip, hdb_rows.hip ----
int hdb_sort_temp_bytes(int64_t n, size_t* bytes);
int hdb_launch_full_sort(const float* scores, const uint8_t* mask, int64_t n, int64_t k, int64_t row_base, uint32_t* work, void* temp, size_t temp_bytes,
                         int64_t* idx_out, float* score_out, void* stream);
int hdb_launch_gather_rows(const void* V, const int64_t* rows, int64_t m, int row_bytes, void* out, const float* inv_in,
                           const float* sq_in, float* inv_out, float* sq_out, int* nan_flag, void* stream);

// ---- hdb_mfma.hip: the matrix-core scan ----
size_t hdb_mfma_batch_ctl_bytes(int wgs);
int hdb_launch_mfma_scan(const ScanArgs* args, int dtype, int mode, int nq_launch, const void* q16, const float* sqnorm,
                         const float* qsq, const float* qscl, int max_blocks, int variant, void* stream, const BatchArgs* f);
int hdb_launch_q_to_f16(const float* Q, int nq, int d, void* q16, float* qscl, void* stream);
int hdb_launch_rescore_euclid(unsigned long long* cand, const uint32_t* cnt, uint32_t cap, int nq_launch, const void* V, int dtype, int d,
                              const float* Q, const float* qsq, int q0, const float* bias, void* stream);
// ... its shards (hdb_mfma_<geometry>.hip): what a shard reads of the record is its own business (MfmaLaunch, hdb_common.h)
HDB_GEOM_DECL(hdb_launch_mfma_scan_f16_d384);           // fp16 rows: the only shards that read qscl, d384 the only one that reads variant
HDB_GEOM_DECL(hdb_launch_mfma_scan_f16_narrow);
HDB_GEOM_DECL(hdb_launch_mfma_scan_f16_mid);
HDB_GEOM_DECL(hdb_launch_mfma_scan_f16_1k);
HDB_GEOM_DECL(hdb_launch_mfma_scan_f16_wide);
HDB_GEOM_DECL(hdb_launch_mfma_scan_f16_qt2);
HDB_GEOM_DECL(hdb_launch_mfma_scan_f32);                // float32 rows, and as bf16 parts (f32s)
HDB_GEOM_DECL(hdb_launch_mfma_scan_f32_wide);
HDB_GEOM_DECL(hdb_launch_mfma_scan_f32s);
HDB_GEOM_DECL(hdb_launch_mfma_scan_f32s_wide);
HDB_GEOM_DECL(hdb_launch_mfma_scan_bf16);
HDB_GEOM_DECL(hdb_launch_mfma_scan_bf16_wide);
HDB_GEOM_DECL(hdb_launch_mfma_scan_f8);
HDB_GEOM_DECL(hdb_launch_mfma_scan_f8_wide);
HDB_GEOM_DECL(hdb_launch_mfma_scan_i8);                 // int8 rows: the float8 kernel with the int8 row converter (hdb_mfma_i8.hip)
HDB_GEOM_DECL(hdb_launch_mfma_scan_i8_wide);
HDB_GEOM_DECL(hdb_launch_mfma_scan_b1);                 // packed-bit rows: bits expanded to bf16 0.0 / 1.0 per fragment in registers (hdb_mfma_b1.h; opt-in, b1_mfma_min_q)
HDB_GEOM_DECL(hdb_launch_mfma_scan_b1_wide);
HDB_GEOM_DECL(hdb_launch_mfma_scan_f8_lds);             // float8 rows expanded to bf16 in LDS (hdb_mfma_f8_lds.h; ScanArgs::f8_lds = waves per workgroup); blocks: the most workgroups the launch may take
HDB_GEOM_DECL(hdb_launch_mfma_scan_f8_lds_wide);
// the K-slice driver (hdb_mfma_ksplit.hip) and one slice of l->width elements (args: the slice's ks_* fields set)
int hdb_launch_mfma_ksplit(const ScanArgs* args, int dtype, const MfmaLaunch* l);
HDB_GEOM_DECL(hdb_launch_mfma_kslice_f32s);
HDB_GEOM_DECL(hdb_launch_mfma_kslice_bf16);
HDB_GEOM_DECL(hdb_launch_mfma_kslice_bf16_wide);
HDB_GEOM_DECL(hdb_launch_mfma_kslice_f8);
HDB_GEOM_DECL(hdb_launch_mfma_kslice_f8_wide);
HDB_GEOM_DECL(hdb_launch_mfma_kslice_f8_lds);
HDB_GEOM_DECL(hdb_launch_mfma_kslice_f8_lds_wide);
HDB_GEOM_DECL(hdb_launch_mfma_kslice_b1);
HDB_GEOM_DECL(hdb_launch_mfma_kslice_b1_wide);
// a width without a geometry of its own as one slice of the next wider one, l->width (hdb_mfma_anyd.h)
HDB_GEOM_DECL(hdb_launch_mfma_anyd_a); HDB_GEOM_DECL(hdb_launch_mfma_anyd_b);       // fp16 rows
HDB_GEOM_DECL(hdb_launch_mfma_anyd_c); HDB_GEOM_DECL(hdb_launch_mfma_anyd_d);       // float32 rows
HDB_GEOM_DECL(hdb_launch_mfma_anyd_e); HDB_GEOM_DECL(hdb_launch_mfma_anyd_f);       // float32 rows as bf16 parts

// ---- the single launches: hdb_mfma_fused*.hip, hdb_bits_fused.hip; hdb_l1_tile.hip ----
size_t hdb_mfma_fused_ctl_bytes(void);
int hdb_launch_mfma_fused(const ScanArgs* args, int dtype, const FusedArgs* fa, int max_blocks, void* stream);
int hdb_launch_mfma_fused_wide(const ScanArgs* args, const FusedArgs* fa, int blocks, void* stream);
int hdb_launch_bits_fused(const BitsArgs* args, int jaccard, int max_blocks, void* stream);
int hdb_launch_l1_tile(const ScanArgs* args, int dtype, int mode, int nq_launch, int max_blocks, void* stream);

// ---- hdb_quant.hip: the int8 shadow and its 5-bit plane ----
int hdb_launch_quant_rows(const void* V, int64_t n, int d, int dtype, int P, int8_t* codes, float* aux, int* nan_flag, double gamma,
                          void* stream);
int hdb_launch_quant_gather(const int8_t* codes, const float* aux, const int64_t* rows, int64_t m, int P, int8_t* codes_out,
                            float* aux_out, void* stream);
int hdb_launch_quant_qprep(const float* Q, int nq, int d, int P, int8_t* qcodes, float* qaux, int* stat, uint32_t* pl_cnt, void* stream);
int hdb_launch_quant_qprep_m(const float* Q, int nq, int d, int P, float* qinv, float* qsq, int* qnan, void* q16, float* qscl,
                             int8_t* qcodes, float* qaux, int* stat, uint32_t* cnt_init, uint32_t* pl_cnt, void* stream);
int hdb_launch_quant_plane_rows(const int8_t* codes, const float* aux, const float* inv_norm, int64_t t0, int64_t t1, int64_t n, int d, int P,
                                uint8_t* nib, uint32_t* bitw, float* rec, void* stream);
int hdb_launch_quant_plane_scan(const QuantArgs* args, int dbg, int blocks, void* stream);
int hdb_launch_quant_scan(const QuantArgs* args, int mode, int max_blocks, void* stream);
int hdb_launch_quant_scan_one(const QuantArgs* args, int mode, int max_blocks, void* stream);
int hdb_launch_quant_rescore(const void* V, int d, int dtype, const float* Q, int nq, int metric, const float* inv_norm,
                             const float* qinv, const float* bias, const uint8_t* mask, unsigned long long* cand,
                             const uint32_t* cnt, uint32_t cap, void* stream);
int hdb_launch_quant_finalize(const unsigned long long* cand, const uint32_t* cnt, uint32_t cap, int nq, uint32_t k, uint32_t kk,
                              int64_t row_base, int64_t* idx_out, float* score_out, int32_t* status, const int* qnan,
                              const float* qaux, const float* thr, int* stat, unsigned long long* cand_rw, const float* sc, int64_t ld,
                              void* stream);

// ---- hdb_rerank.hip: exact scores of per-query candidate lists ----
// prep: cand [nq][m] caller ids -> rows [nq][m] valid, ascending, unique local rows, cnt[q * HDB_CNT_STRIDE] of them, status[q]
// score: ScanArgs as for the VALU scan, with rows = those lists, m = their leading dimension, cnt / cand / cap the packed lists out
int hdb_launch_rerank_prep(const int64_t* cand, int m, int nq, int64_t n, int64_t row_base, const uint8_t* mask, const int* qnan,
                           int64_t* rows, uint32_t* cnt, int32_t* status, void* stream);
int hdb_launch_rerank_score(const ScanArgs* args, int dtype, int nq_launch, void* stream);

// ---- hdb_group.hip: grouped top-k (one row per group) ----
// collapse: a ranked list [nq][m <= 2048] -> the first k first occurrences of a group per query; status_in / status_out may be the
// same array, `carry` = the bits of status_in that survive.  best / demote: the two launches of the exact grouped pass over the
// score buffer [nq][ld] (best: [nq][n_groups], zero on entry; *bad is raised by an id outside [0, n_groups)).  finish: behind the
// finalize of that pass, nq <= 256.
int hdb_launch_group_collapse(const int64_t* idx, const float* score, int nq, int m, int k, const int32_t* groups, int64_t n_groups,
                              int64_t n, int64_t row_base, int64_t* idx_out, float* score_out, const int32_t* status_in,
                              int32_t* status_out, int carry, void* stream);
int hdb_launch_group_best(const float* scores, int64_t n, int64_t ld, int nq, const int32_t* groups, int64_t n_groups,
                          unsigned long long* best, void* stream);
int hdb_launch_group_demote(float* scores, int64_t n, int64_t ld, int nq, const int32_t* groups, int64_t n_groups,
                            const unsigned long long* best, int* bad, void* stream);
int hdb_launch_group_finish(int64_t* idx, const float* score, int nq, int k, int32_t* status, const int* bad, void* stream);

// ---- hdb_maxsim.hip: multi-vector queries (sum over a set's vectors of the per-group maxima) ----
// keys / sort / offsets: the inverted index of the group ids -- keys [n] (an id outside [0, n_groups) becomes n_groups and raises
// flags[0]; keys that decrease somewhere raise flags[1]), iota: rows = 0 .. n - 1, the stable sort of the pairs, and
// grp_off [n_groups + 1].  reduce: one launch per chunk of cq vectors (v0 = the first one, s_first = its set, s_base = the first set
// of acc [sets][ld_g]); team = 1 | 4 | 16 | 64 lanes per group.  setnan: snan[s] = a vector of set s holds a NaN.
int hdb_maxsim_sort_temp_bytes(int64_t n, int64_t n_groups, size_t* bytes);
int hdb_launch_maxsim_keys(const int32_t* groups, int64_t n, int64_t n_groups, uint32_t* keys, int* flags, void* stream);
int hdb_launch_maxsim_iota(uint32_t* rows, int64_t n, void* stream);
int hdb_launch_maxsim_sort(void* temp, size_t temp_bytes, uint32_t* keys_in, uint32_t* keys_out, uint32_t* rows_in, uint32_t* rows_out,
                           int64_t n, int64_t n_groups, void* stream);
int hdb_launch_maxsim_offsets(const uint32_t* keys, int64_t n, int64_t n_groups, uint32_t* grp_off, void* stream);
int hdb_launch_maxsim_setnan(const int* qnan, const int32_t* voff, int ns, int* snan, void* stream);
int hdb_launch_maxsim_reduce(const float* sbuf, int64_t ld_n, int cq, int32_t v0, const int32_t* voff, int32_t s_first, int32_t s_base,
                             const uint32_t* grp_off, const uint32_t* grp_rows, int sorted, int64_t n_groups, float* acc, int64_t ld_g,
                             int team, void* stream);

// ---- hdb_mmr.hip: diverse top-k (maximal marginal relevance over a call's candidates) ----
// Three launches per chunk of nq queries, mp = hdb_mmr_mp(m) (hdb_caps.h).  prep: the lists [nq][m] -> candidates in list order, rows /
// rel [nq][mp] and cnt [nq]; status_in / status_out may be the same array or NULL (HDB_Q_NAN is carried, HDB_Q_BADROW set, the rest
// cleared).  pairs: P [nq][mp][mp] float32, the similarity of every two candidates under dot / cosine / euclidean, mirrored; the
// diagonal is not written.  select: min(k, count) picks per query into idx_out / score_out [nq][k], then the -1 / -inf tail.
int hdb_launch_mmr_prep(const int64_t* idx, const float* score, int nq, int m, int mp, int64_t n, int64_t row_base, uint32_t* rows,
                        float* rel, int32_t* cnt, const int32_t* status_in, int32_t* status_out, void* stream);
int hdb_launch_mmr_pairs(const void* V, int dtype, int d, int pair_metric, const float* inv_norm, const uint32_t* rows,
                         const int32_t* cnt, int nq, int mp, float* P, void* stream);
int hdb_launch_mmr_select(const uint32_t* rows, const float* rel, const int32_t* cnt, int nq, int mp, const float* P, float lam,
                          int k, int64_t row_base, int64_t* idx_out, float* score_out, void* stream);

// ---- hdb_quant_mfma.hip: batches through the shadow on the int8 matrix cores ----
int hdb_launch_qb_scan(const QuantArgs* args, int mode, float* wstat, int64_t wld, int max_blocks, void* stream);
int hdb_launch_qb_thr(const float* vals, int64_t n, int64_t ld, int nq, uint32_t m, float* thr, void* stream);
int hdb_launch_qb_rescore(const void* V, int d, const void* q16, const float* qscl, const float* qinv, const float* inv_norm,
                          const float* bias, const uint8_t* mask, int metric, unsigned long long* cand, const uint32_t* cnt,
                          uint32_t cap, int nq, void* stream);
}
