/* hyperdb_hip.h -- C ABI of the MI355X (gfx950) brute-force ranking engine.
 *
 * Drop-in boundary for the hot path of AdamCodd/local-hyperDB.  The reference has no FFI
 * layer: its boundary is the Python function table of hyperdb/ranking_algorithm.py, called
 * from hyperdb/hyperdb.py:1556.  Every entry point below cites the reference interface it
 * replaces; the Python side (local-hyperdb_amd/hyperdb/ranking_algorithm.py) keeps the
 * reference's names and signatures and reaches these symbols through ctypes.
 *
 * Conventions
 *   - All pointers named dev_* are device (HBM) pointers owned by the caller (PyTorch-ROCm
 *     tensors on the Python side).  The library BORROWS them; it owns only its workspace.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls only
 *     enqueue work; they do not synchronise unless stated.
 *   - Return value: 0 (HDB_OK) or a negative hdb_status; the message of the last failure on
 *     the calling thread is returned by hdb_last_error().
 *   - One in-flight call per handle (the reference is single-threaded, hyperdb.py:1381-1388).
 *   - Scores leave the device as float32; the Python shim widens to float64 like
 *     ranking_algorithm.py:171.  Indices are int64 like numpy's argpartition output (:199).
 */
#ifndef HYPERDB_HIP_H
#define HYPERDB_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hdb_index hdb_index;

/* dtype of the stored matrix: HyperDB(fp_precision=...) accepts float16/32/64 (hyperdb.py:65-66); bfloat16 (the upper 16 bits of
 * a float32, 2 bytes per element) is this library's addition for embedding models that emit it, and so is OCP float8 e4m3
 * (torch.float8_e4m3fn: 1 sign, 4 exponent, 3 mantissa bits, bias 7, no infinities, 0x7F / 0xFF = NaN; one byte per element).
 * HDB_I8 = 7 is a matrix of signed 8-bit integers (np.int8 / torch.int8, two's complement, one byte per element): the integers ARE
 * the matrix -- no scale, no zero point, no NaN code, every value in [-128, 127] widens to float32 exactly.
 * HDB_B1 = 10 is a matrix of packed bits, one bit per element: `d` counts bits and is a multiple of 32, a row is d / 32 uint32 words
 * (row-major, 4-byte aligned) and element e of a row is bit e & 31 of word e >> 5 -- np.packbits(.., bitorder="little") read as
 * little-endian words, the bit order of the sign cache.  The matrix is the 0/1 matrix the bits stand for: 1.0 where the bit is set.
 * Codes 4, 6, 8 and 9 are unassigned and refused by hdb_index_create, like every other value not listed here. */
enum hdb_dtype { HDB_F16 = 0, HDB_F32 = 1, HDB_F64 = 2, HDB_BF16 = 3, HDB_F8E4M3 = 5, HDB_I8 = 7, HDB_B1 = 10 };

/* metric strings of hyperDB_ranking_algorithm_sort's dispatch table (ranking_algorithm.py:155-163). */
enum hdb_metric {
    HDB_DOT = 0,        /* dot_product          ranking_algorithm.py:24-30   */
    HDB_COSINE = 1,     /* cosine_similarity    ranking_algorithm.py:32-42   */
    HDB_EUCLIDEAN = 2,  /* euclidean_metric     ranking_algorithm.py:44-52   (similarity 1/(1+dist)) */
    HDB_HAMMING = 3,    /* hamming_distance     ranking_algorithm.py:128-147 (d - popcount(xor of x>0)) */
    HDB_MANHATTAN = 4,  /* manhattan_distance   ranking_algorithm.py:54-61   */
    HDB_JACCARD = 5,    /* jaccard_similarity   ranking_algorithm.py:63-75   */
    HDB_PEARSON = 6,    /* pearson_correlation  ranking_algorithm.py:77-113  */
    HDB_EUCLIDEAN_DIST = 7 /* euclidean_metric(get_similarity_score=False): raw distance, hdb_scores only */
};

enum hdb_status {
    HDB_OK = 0,
    HDB_ERR_ARG = -1,          /* bad shape / dtype / k / null pointer  -> ValueError in the shim  */
    HDB_ERR_HIP = -2,          /* a HIP runtime call failed             -> RuntimeError            */
    HDB_ERR_UNSUPPORTED = -3,  /* metric/dtype combination not built    -> NotImplementedError     */
    HDB_ERR_NOMEM = -4
};

/* per-query status bits written by hdb_topk (device int32 per query) */
enum hdb_query_status {
    HDB_Q_OK = 0,
    HDB_Q_UNDERFLOW = 1,  /* sampled threshold too high: fewer than k candidates passed */
    HDB_Q_OVERFLOW = 2,   /* candidate buffer overflowed (massive ties or skewed sample) */
    HDB_Q_NAN = 4,        /* the query vector contains a NaN (ValueError of ranking_algorithm.py:150-151) */
    HDB_Q_BADROW = 8,     /* hdb_rerank: a candidate id outside [row_base, row_base + n) other than a negative one: skipped, never read;
                             grouped calls: also a row whose group id is outside [0, n_groups): treated as masked, never used as an index */
    HDB_Q_GROUPS_SHORT = 16 /* hdb_collapse_groups: fewer than k groups were found and the list was not exhaustive */
};

/* Library/ABI version (major*100+minor). */
int hdb_version(void);

/* Message of the last error on this thread ("" if none). */
const char* hdb_last_error(void);

/* Register a resident N x d row-major matrix (C-contiguous, like HyperDB.vectors, hyperdb.py:80,:911).
 * One pass over V builds the per-row caches that the reference recomputes on every query:
 * 1/||v|| (get_norm_vector, ranking_algorithm.py:8-21, zero norm -> 1), ||v||^2, and the NaN
 * flag (the np.isnan(vectors).any() of ranking_algorithm.py:150).  `row_base` is added to every
 * returned index (global row id of local row 0 when the matrix is one shard of a larger one).
 * Enqueues on `stream`; the index is usable on the same stream immediately. */
int hdb_index_create(hdb_index** out, const void* dev_V, int64_t n, int32_t d, int dtype,
                     int device, int64_t row_base, void* stream);

/* Re-point an index at a (possibly grown / rewritten) matrix and rebuild the row caches;
 * matrix lifecycle counterpart of commit_pending / remove_document (hyperdb.py:503-509,:721-728). */
int hdb_index_update(hdb_index* ix, const void* dev_V, int64_t n, void* stream);

/* Growable matrix (HyperDB.add, hyperdb.py:503-509 grows self.vectors by np.concatenate on every commit):
 * hdb_index_rebase -- the caller moved the SAME rows to another allocation (capacity doubling); only the borrowed
 *                     pointer changes, every cache stays valid.
 * hdb_index_extend -- rows [n_old, new_n) were appended behind the existing rows of the current allocation; the
 *                     1/||v||, ||v||^2 and NaN caches are extended over the new rows only (O(new rows), not O(N));
 *                     the sign bits and the pearson row scales are extended the same way on their next use (lazy caches:
 *                     the appended rows only). */
int hdb_index_rebase(hdb_index* ix, const void* dev_V);
int hdb_index_extend(hdb_index* ix, int64_t new_n, void* stream);

/* Global row id of local row 0 (see hdb_index_create): a shard's base moves when an earlier shard grows or is compacted. */
int hdb_index_set_row_base(hdb_index* ix, int64_t row_base);

/* Compaction after HyperDB.remove_document (hyperdb.py:691-766; the reference rebuilds self.vectors on the host with
 * np.vstack / a boolean mask, :721-728): the m kept rows dev_rows[0..m) (ascending local row ids, int64, device) are
 * gathered into dev_V_out (m x d, caller-owned, must not alias the current matrix) in one pass at HBM speed, and the
 * 1/||v||, ||v||^2 and NaN caches travel with their rows -- nothing is recomputed.  On return (the call synchronises
 * `stream`) the index borrows dev_V_out with n = m and the caller may release the old matrix; bias and mask are
 * cleared, sign-bit / pearson caches are rebuilt lazily. */
int hdb_index_gather(hdb_index* ix, const int64_t* dev_rows, int64_t m, void* dev_V_out, void* stream);

void hdb_index_destroy(hdb_index* ix);

/* Opt-in int8 shadow of the matrix: quantized row scan with exact rescoring (local-hyperdb_amd/csrc/hdb_quant.hip).
 * HDB_QUANT_I8 builds, next to the float16 / float32 matrix, an owned int8 copy -- one code per element at a row pitch
 * P = round_up(d, 16) bytes -- and 12 bytes of per-row caches: N x (P + 12) bytes of device memory.  HDB_QUANT_NONE frees it.
 * float64, float8 and int8 matrices return HDB_ERR_UNSUPPORTED, and so does a bfloat16 matrix unless the option bf16_quant is set on the
 * index (opt-in: then the call builds the same explicit shadow, codes, caches and 5-bit plane, from the two-byte rows; the calls it
 * serves return the bits of the VALU scan, which is the default path of a bfloat16 index for 1-4 queries; a bfloat16 index never
 * builds a shadow for itself, with or without the option).  The shadow follows the matrix: hdb_index_extend quantizes the appended rows,
 * hdb_index_gather moves codes and caches with the kept rows, hdb_index_update rebuilds it, hdb_index_rebase leaves it alone.
 *
 * The bound.  Row r: s_r = max_j |v_rj| / 127, c_rj = rne(v_rj / s_r), eps_r = v_r - s_r c_r; the query likewise (s_q, c_q,
 * delta_q = q - s_q c_q).  C_qr = c_q . c_r is exact in int32, and
 *     |q.v_r - s_q s_r C_qr| <= ||q|| ||eps_r|| + ||delta_q|| s_r ||c_r||  (Cauchy-Schwarz),
 * widened by the float32 rounding of the VALU scan's own sum (gamma_{d+8} ||q|| ||v_r||) and of the bound's evaluation; cosine
 * and euclidean (through d^2 = ||v||^2 + ||q||^2 - 2 q.v) map the interval through the scan's epilogue, which is monotone, and the
 * bias is added to both ends.  hdb_quant.hip derives it line by line.
 *
 * Dispatch.  hdb_topk takes the shadow for 1-4 dot / cosine / euclidean queries with k <= quant_max_k (<= 128) on a finite
 * matrix of more than HDB_CAND_CAP rows, at least quant_min_n of them (-1: the measured rule), when use_quant is on, the call is
 * not exact and force_exact is off.  Every row whose upper bound reaches T_s (the 16th largest lower bound of a strided row
 * sample) is rescored from the original matrix in the lane split, chunk order and reduction order of the VALU scan, so the top-k
 * -- indices and float32 score bits -- is the one hdb_scores / hdb_topk with use_mfma = 0 return.  A query whose list
 * overflowed, or whose k-th rescored candidate does not score above T_s, gets HDB_Q_OVERFLOW / HDB_Q_UNDERFLOW like any sampled
 * call (hdb_topk_host re-runs it exactly).  hdb_topk_exact never takes the shadow.
 * Stats: quant (the last call took it), quant_cands (largest candidate list of that call; synchronises), quant_bytes.
 *
 * The automatic shadow (option auto_quant, default 1).  A float16 index answers 1-4 dot / cosine queries on the matrix cores, and
 * those float32 score bits differ from the VALU scan's.  When auto_quant, use_quant and use_mfma are on, the index has no explicit
 * shadow, the matrix is float16 and finite, and a call is eligible -- 1-4 queries the matrix cores would take, dot or cosine,
 * k <= quant_max_k, not exact, no force_exact, a status pointer, and at least 2 000 000 rows of at most 512 elements (quant_min_n
 * >= 0 replaces that rule: any row count from there on, any width the matrix cores take) -- the index builds the shadow on the
 * first such call and answers it, and every later one, from it.  The candidates are then rescored on the matrix cores (gathered
 * into a compact matrix and scored by the launch hdb_topk_exact uses for all rows), so indices and score bits are those of the
 * default path and of hdb_topk_exact; the bound targets the matrix-core sum of the fp16-rounded query with gamma_m = (d + 8) 2^-22
 * (hdb_quant.hip, bound (2m)).  Stats of such a call: quant = 1, mfma = 1 (the arithmetic the scores come from), path = 1,
 * fused = 0; quant_auto = 1 while the index holds a shadow it built itself.
 * Cost: the index grows by n x (round_up(d, 16) + 12) bytes of device memory (10M x 384: 3.96 GB beside 7.68 GB) and the first
 * eligible call also pays the allocation and one pass over the matrix (10M x 384: 11.8 ms, 2.5M: 3.1 ms).  The build is skipped, silently
 * and for good (until hdb_index_update), when hipMemGetInfo does not show room for the shadow, the call's workspace and 1 GiB
 * beside them, or when an allocation fails.  hdb_index_quantize(HDB_QUANT_NONE) drops the shadow AND sets auto_quant = 0 for the
 * handle; hdb_index_quantize(HDB_QUANT_I8) turns it into an explicit one (VALU bits, the rule above).  An index that only serves
 * other metrics or small matrices never builds one.
 *
 * Batches through the automatic shadow (local-hyperdb_amd/csrc/hdb_quant_mfma.hip).  A call of 5 or more dot / cosine queries under
 * the same conditions, on rows of 128, 256, 384 or 512 elements with mfma_variant = 16, is answered from the shadow as well, in
 * chunks of up to 256 queries: quantized query prep, an int8 matrix-core pass (v_mfma_i32_16x16x64_i8) over a tenth of the rows
 * that leaves per-slot maxima of the lower bounds, T_s = the 32nd largest of them per query, an int8 matrix-core pass over all
 * rows that emits the (row, query) pairs whose upper bound reaches T_s, rescoring of every list from the fp16 matrix with the
 * instruction, K walk and epilogue of the default batched path (query q against its own list only), finalize with the floor T_s.
 * Indices and score bits are those of the default path and of hdb_topk_exact; a query whose floor check fails or whose list
 * overflows says so in its status word.  The pass tests every pair with a cheap conservative form of the bound -- convert,
 * multiply, four fma, compare, on per-row and per-query values folded outside the pair loop; it passes every pair whose upper
 * bound (bound (3) of hdb_quant.hip, score-domain map and outward push included) reaches T_s - c0, c0 = 1.001 (d + 8) 2^-36 for
 * cosine and 1.001 (d + 8) 2^-100 + 4e-30 for the dot product -- and holds the survivors against the exact bound, so the lists
 * are those the v_dot4 scan would emit (derivation in the kernel's header comment).
 * Row rule: quant_batch_min_n (-1: the measured rule -- d = 384: 5-16 queries from 3 000 000 rows, 17-24 from 5 000 000; d = 512:
 * 5-16 queries from 10 000 000 rows; nothing else, DESIGN.md section 4.9 has the table -- never below 2 000 000 rows; >= 0: every
 * query count from that many rows on).  It is separate from quant_min_n, which keeps governing 1-4-query calls only.  quant_batch_kernel
 * (default 1) = 0 runs the filter with the v_dot4 scan of the 1-4-query flavour, four queries per pass over the shadow: the A/B
 * switch for timing and an independent kernel for the tests.  Stats as above (quant = 1, quant_auto = 1, mfma = 1, path = 1,
 * fused = 0), chunks = launches of up to 256 queries, quant_cands = the largest list of the call, quant_cands_min /
 * quant_cands_median = the smallest / median list of its last chunk (both synchronise).
 * Workspace of a chunk of cq queries: the lists, cq x HDB_CAND_CAP x 8 bytes (16 MiB at 256 queries), at most cq x 8192 floats of
 * sample maxima, cq x d fp16 query values and the per-query words; no compact matrix and no score block.  A batch call can be
 * the one that builds the shadow and pays for it.
 *
 * The 5-bit plane (one dot / cosine query; hdb_quant.hip, "The 5-bit plane").  Beside the codes the index keeps their high five
 * bits -- a nibble plane, a bit plane and 16 bytes of row terms per row, 20 bytes per 32 elements + 16 (10M x 384: 2.56 GB) --
 * derived from the codes wherever the shadow's rows are written (build, extend, update, gather) for rows of up to 512 elements.
 * The row terms are laid out per 16-row tile: 256 bytes = a 64-byte hot block for dot-product calls, one for cosine calls, and 128
 * reserved bytes (zero).  A hot block holds 16 bfloat16 row scales rounded up (cosine: divided by the row's norm), 16 bytes
 * ceil(2 ||residual||) and the tile's largest error terms {E*, T*, F*, 0} as float32; a call reads the one block of its metric,
 * 4 bytes per row.  The maxima are tile state: whatever writes a row derives its whole tile again, from all of the tile's rows.  A
 * one-query call of at least plane_min_n rows (-1: the measured rule, 2 000 000) with use_plane on streams the plane and, in the
 * same launch, runs the int8 evaluation on the rows whose coarse upper bound hi5 reaches T_s, 16 at a time.  hi5 >= the int8
 * pass's own upper bound for every row, so the candidate list, and the answer, are those of the call without the plane.
 * plane_cap_rows (0: n / 8) is a mark, not a capacity: a call that keeps more rows than that is counted in plane_overflows -- the
 * plane let more through than it is worth, the call read the plane AND the codes of those rows -- and its answer is complete all
 * the same (there is no automatic switch-off: use_plane = 0 is the manual one).  Euclidean calls, 2-4 queries and batches never
 * take the plane.  The plane is under the automatic build's memory guard: when the shadow fits and the plane does not, the shadow
 * is built alone.  Stats: plane (the last call took it), plane_bytes, plane_survivors (rows the plane kept in the last call) and
 * plane_overflows (calls of this index that kept more than plane_cap_rows); the last two synchronise. */
enum hdb_quant { HDB_QUANT_NONE = 0, HDB_QUANT_I8 = 1 };
int hdb_index_quantize(hdb_index* ix, int mode, void* stream);
/* Test entry: the upper bound of every row for ONE float32 query (dot or cosine) as the int8 pass computes it (dev_hi, n floats)
 * and as pass 1 over the 5-bit plane computes it (dev_hi5, n floats).  Needs a shadow with its plane; nothing is selected. */
int hdb_debug_quant_bounds(hdb_index* ix, const float* dev_q, int metric, float* dev_hi, float* dev_hi5, void* stream);

/* 1 if the matrix contains a NaN (synchronises `stream` of the create/update call). */
int hdb_index_has_nan(hdb_index* ix, int* out_flag);

/* Additive per-row term applied before top-k: the recency_scores of ranking_algorithm.py:180-186.
 * dev_bias: n floats or NULL to clear.  Borrowed until replaced/cleared. */
int hdb_index_set_bias(hdb_index* ix, const float* dev_bias);

/* Device-side builder of that term: dev_out[i] = recency_bias * exp(dev_ts[i] - ts_max), evaluated in
 * float64 and stored as float32 (ranking_algorithm.py:183; ts_max = max(timestamps), which the caller
 * already knows from the host-side timestamp list, hyperdb.py:1341-1344). */
int hdb_recency_bias(const double* dev_ts, int64_t n, double recency_bias, double ts_max, float* dev_out,
                     int device, void* stream);

/* Both decays a HyperDB.query() call applies (hyperdb.py:1344 over the FILTERED documents, then ranking_algorithm.py:183 on
 * those values): dev_out[i] = rb * exp(first_i - max first), first_i = rb * exp(-ts_max + dev_ts[i]), for the rows dev_mask keeps
 * (NULL: all rows; dropped rows get 0).  ts_max / ts_min = newest / oldest timestamp among the kept rows (the maximum of
 * `first` sits at one of them).  float64 arithmetic, float32 result: the whole recency term of the facade without a host pass. */
int hdb_recency_bias_twice(const double* dev_ts, const uint8_t* dev_mask, int64_t n, double recency_bias, double ts_max,
                           double ts_min, float* dev_out, int device, void* stream);

/* Optional row subset (filters / skip_doc, hyperdb.py:1119-1134,:1258-1308): dev_mask is n bytes,
 * non-zero = row takes part; NULL clears.  Excluded rows score -inf and are never returned:
 * with fewer than k rows included the tail is -1 / -inf on every path. */
int hdb_index_set_row_mask(hdb_index* ix, const uint8_t* dev_mask);

/* Row mask plus the ascending list of the rows it keeps: a selective filter reads only the rows it keeps (hdb_scan.hip, the list
 * flavour of the VALU scan).  dev_mask: n bytes as for hdb_index_set_row_mask.  dev_rows: the m local row ids with
 * dev_mask[r] != 0, strictly ascending, int64, device, borrowed like the mask (m >= 1; NULL = a plain mask).  The caller
 * guarantees that list and mask describe the same rows; the library does not check it on the device.  Eligible calls score
 * only the listed rows, every other call uses the mask.  Both NULL clears.  hdb_index_set_row_mask drops the list;
 * hdb_index_extend, hdb_index_update and hdb_index_gather drop it with mask and bias; hdb_index_rebase keeps it.
 *
 * Dispatch.  A hdb_topk / hdb_topk_exact / hdb_topk_host call takes the list when use_subset is on (default 1), the metric is
 * dot, cosine, euclidean, manhattan or pearson (hamming and jaccard read the packed sign bits and keep the mask), the matrix has
 * at least subset_min_n rows (-1: the rule of hdb_plan.h, never below 32 768), m * ceil(nq / 4) * subset_ratio <= n (-1: the
 * rule of hdb_plan.h; else an integer >= 1) and the same call on a matrix of m rows is the multi-kernel pipeline: k > 2048 on
 * more than 8192 listed rows keeps the mask.  Every dtype is served.  The call then runs the plan of that m-row matrix with
 * use_mfma = 0, use_fused = 0, use_quant = 0, use_l1_tile = 0 -- small (m <= 8192), sampled or exact -- over the listed rows:
 * ceil(m / 16) tiles of list positions, position j in the place of row j, 1/||v||, the pearson scale and the bias taken from the
 * true row, the true row in every candidate.  hdb_topk_host re-runs a failed sampled list call exactly over the list.
 *
 * Contract.  Indices, float32 score bits and status words equal those of the same call on a fresh index registered over
 * V[rows] with bias[rows] and those four options off, indices mapped through rows and row_base added; with fewer than k listed
 * rows the tail is -1 / -inf.  Against the masked call of the same handle the result is the same modulo ties within the
 * dtype's tolerance (1e-3 float16, 1e-5 otherwise); the bits may differ because a default float16 index rounds float32 queries
 * to float16 for the matrix cores and the list path does not, and because a row's slot in the reduction tree is j & 3 instead
 * of row & 3.  A call that does not take the list is the masked call, bit for bit.
 * Stats: subset (the last call scored from the list), subset_rows (m of the list currently set, 0 = none); path, chunks,
 * sample_rows and sample_m are those of the plan that ran, mfma = fused = quant = 0. */
int hdb_index_set_row_subset(hdb_index* ix, const uint8_t* dev_mask, const int64_t* dev_rows, int64_t m);

/* Full score vector of one query: the per-metric functions dot_product / cosine_similarity /
 * euclidean_metric / hamming_distance (... :24,:32,:44,:128).  dev_q: d elements, float32 for
 * F16/F32/BF16/F8E4M3/I8 matrices, float64 for F64 matrices.  dev_out: n floats.  The bias is NOT added. */
int hdb_scores(hdb_index* ix, const void* dev_q, int metric, float* dev_out, void* stream);

/* Top-k of nq independent queries: metric scoring + NaN->-inf + bias + argpartition/argsort of
 * hyperDB_ranking_algorithm_sort (ranking_algorithm.py:168-204), for nq queries at once (the
 * reference takes one query per call).  dev_Q: nq x d row-major (float32, or float64 for F64
 * matrices).  Outputs: dev_idx [nq][k] int64 (row_base added; -1 where fewer than k rows exist),
 * dev_score [nq][k] float32, sorted by (score descending, index ascending).
 * dev_status [nq] int32 receives hdb_query_status bits; queries with a non-zero status must be
 * re-run with hdb_topk_exact (the threshold estimate from the row sample failed for them).
 * On fp16 matrices (d any multiple of 128 up to 1536; dot, cosine, euclidean, pearson) the
 * scores come from the matrix cores with fp16 copies of the queries (scaled per query by a power of two, so any
 * float32 magnitude is safe) and float32 accumulation: nothing is lost when the query has the matrix's dtype, a
 * float32 query is rounded to 11 significant bits per element (score error ~1e-4 relative, inside the 1e-3
 * contract for fp16 data).  hdb_set_option(ix, "use_mfma", 0) keeps float32 queries unrounded (VALU scan).
 * float32 matrices (d in {128,256,384,512,768}) take batches of 5+ queries through fp32 MFMAs: exact fp32 products.
 * Larger cosine / euclidean / pearson batches on a finite float32 matrix multiply the rows as two bf16 parts instead (option
 * f32_split, default 1; stat f32_split): 16 mantissa bits of a row value, a product error of up to 2^-17 |v| |q| that those
 * metrics divide by |v| |q| or bury under |v|^2 + |q|^2 -- inside 1e-5 * max(1, |s|) for every row.  dot_product never does:
 * nothing scales its error down, and a row whose score is small against |v| |q| would miss the band (|v| = 20, |q| = 2,
 * |s| < 1: up to 2.3e-5), so dot_product batches run on the fp32 MFMAs at every size.  The parts of an infinite query element
 * cancel to NaN: such a query gets HDB_Q_UNDERFLOW from hdb_topk and its answer from hdb_topk_exact.
 * fp16 / float32 rows of a width without a geometry of its own (any multiple of 16 bytes) ride the next wider one on the matrix
 * cores while the matrix is finite; a matrix with an infinite or NaN element keeps the VALU scan at those widths.
 * Calls of 1-4 dot / cosine queries with k <= 128 on an fp16 matrix (d = 256 .. 768; 1-2 queries for d = 1024 .. 1536), or of 1-2 on a float32 matrix
 * (d in {128,256,384}; one query at d = 768 and, from 1.5 M rows on, at d = 512), run as ONE kernel launch (query preparation, row sample, threshold exchange between the
 * workgroups, filter pass, final sort: hdb_mfma_fused.h); everything else is the same pipeline as separate launches.
 * Results are bit-identical either way.
 * bfloat16 matrices (HDB_BF16).  Queries are float32.  Every stored value widens to float32 exactly, and the contract is the
 * float32 one: scores within 1e-5 of the reference's arithmetic on the widened matrix (hamming exact, jaccard 1e-6), on every path.
 *   - 1-4 queries, every metric, any d, any k, bias and row mask: the VALU scan (float32 arithmetic on the widened values, unrounded
 *     float32 queries), through the small, sampled, exact and full-sort pipelines, as separate launches.  hamming / jaccard calls
 *     of 1-4 queries may take their single launch (it reads the packed sign bits only).  Manhattan batches stay on the
 *     4-queries-per-pass scan (no LDS tile kernel).
 *     On request (option bf16_quant = 1, then hdb_index_quantize(HDB_QUANT_I8)): 1-4 dot / cosine / euclidean queries with k <= 128
 *     on a finite matrix of at least quant_min_n rows (-1: 1 000 000, measured) filter on the int8 shadow and rescore the candidates
 *     from the bfloat16 rows with this scan's arithmetic -- the same indices and float32 score bits.
 *   - 5+ dot / cosine / euclidean / pearson queries on a FINITE matrix of d = 128, 256, 384 or 512 with use_mfma on: the matrix
 *     cores (hdb_mfma_bf16.hip), multi-kernel pipeline.  A float32 query travels as three bf16 parts that add up to it exactly,
 *     a row is one bf16: three v_mfma_f32_16x16x32_bf16 per k-step, every product exact, float32 accumulation.  A query element
 *     that is not finite keeps its first part only, so no inf - inf is formed and the status words stay 0.  A matrix with an
 *     infinite (or overflowing) row stays on the VALU scan (inf x 0 would be NaN where np.dot gives inf).
 *   - the same calls on wider rows -- d = 640, 768, 896, 1024, 1152, 1280, 1408, 1536, 2048, 3072 or 4096 -- take the matrix cores
 *     through K slices (hdb_mfma_bf16_ks.hip): a wave holds the three query parts of 512 elements at most, so a row is cut into the
 *     fewest slices of 512 / 384 / 256 elements, the widest first (768 = 2 x 384, 1024 = 2 x 512, 1280 = 512 + 2 x 384, 1536 = 3 x 512,
 *     4096 = 8 x 512), one launch per slice and pass, at most 128 queries per chunk.  The matrix is still read once per pass; the
 *     partial sums travel through a [query][rows] float32 workspace: +8 bytes per row, query and extra slice.  Same arithmetic, same
 *     treatment of non-finite values, pearson as cosine on centred queries.  The slices start where they were measured to beat
 *     the two VALU passes that 5-8 queries cost: from 5 queries at d = 1024 and 4096, from 9 at the other widths (option
 *     bf16_ks_min_q: -1 = that rule, else a fixed number of queries, never fewer than 5).  Other widths stay on the VALU scan.
 *   - never: the single launches of the matrix-core paths (fused = 0 always), the int8 shadow (hdb_index_quantize returns
 *     HDB_ERR_UNSUPPORTED, auto_quant does not apply).
 * Stats: mfma = 1 on the matrix-core path, fused = 0 (3 for the bit metrics' single launch), path as for the other dtypes.
 * float8 e4m3 matrices (HDB_F8E4M3).  Queries are float32.  Each of the 254 finite codes (largest magnitude 448, smallest 2^-9)
 * widens to float32 exactly (v_cvt_pk_f32_fp8), and the contract is the float32 one: scores within 1e-5 of the reference's
 * arithmetic on the widened matrix (hamming exact, jaccard 1e-6).  No approximate filter, no rescoring, no second copy.
 *   - 1-4 queries, every metric, any d, any k, bias, row mask and row list, and every batch no other path takes: the VALU scan
 *     (float32 arithmetic on the widened values, unrounded float32 queries), four queries per pass, through the small, sampled,
 *     exact and full-sort pipelines, as separate launches.  Rows of 256, 384 and 512 bytes have a fully unrolled ONE-query kernel on
 *     a grid sized by bytes (hdb_scan.hip); the four-query kernel keeps the runtime loop on that grid -- an unrolled four-query
 *     flavour that keeps ~100 KiB in flight per CU is not built (it needs all 256 registers), and four queries reach 1.2-1.4x over
 *     bfloat16 instead of the 2x the bytes allow.  hamming / jaccard calls of 1-4 queries may take their single launch (it reads
 *     the packed sign bits only).  Manhattan batches stay on the 4-queries-per-pass scan.
 *   - 5+ dot / cosine / euclidean / pearson queries on a matrix without a NaN code, d = 128, 256, 384 or 512, use_mfma on: the matrix
 *     cores (hdb_mfma_f8.hip), multi-kernel pipeline.  The rows are converted to bf16 per fragment in registers (exact: a code has
 *     four significant bits), a float32 query travels as three bf16 parts that add up to it exactly: three v_mfma_f32_16x16x32_bf16
 *     per k-step, every product exact, float32 accumulation, the bfloat16 flavour's K walk and epilogue -- the scores are those of
 *     a bfloat16 index over the widened matrix bit for bit.  A query element that is not finite keeps its first part only (status
 *     words stay 0).  A matrix holding a NaN code stays on the VALU scan.  Other widths stay on the VALU scan.
 *   - on request (option f8_ks_min_q, 0 = never by default): the same calls on wider rows -- d = 640, 768, 896, 1024, 1152, 1280,
 *     1408, 1536, 2048, 3072 or 4096 -- take the matrix cores through K slices (hdb_mfma_f8_ks.hip), multi-kernel pipeline.  The
 *     slice list is bfloat16's (the fewest slices of 512 / 384 / 256 elements, the widest first), one launch per slice and pass, at
 *     most 128 queries per chunk, partial sums in a [query][rows] float32 workspace (+8 bytes per row, query and extra slice); rows
 *     are still converted per fragment in registers.  Same K walk, same epilogue: the scores are those of a bfloat16 index over the
 *     widened matrix going through ITS K slices, bit for bit.  f8_ks_min_q = n >= 1: from max(n, 5, mfma_min_q) queries on; -1: from
 *     hdb_mfma_f8_ks_min_q(d) queries on (hdb_caps.h).  A matrix holding a NaN code, manhattan batches, matrices of up to 8192 rows
 *     and row-list calls stay on the VALU scan; k > 2048 is the full sort as for every dtype.  Off by default: the default dispatch
 *     of float8 rows beyond 512 elements is pinned as "VALU scan" (tests/f8_plan_check.hip), and every 16 queries of a batch convert
 *     a tile's fragments again, so large batches lose to a bfloat16 index -- turning a measured rule on is a change of its own.
 *   - on request (option f8_lds_min_q, 0 = never by default): every matrix-core launch of such a call -- whole rows of 128 .. 512
 *     elements or, under f8_ks_min_q, the K slices; sample, filter and exact pass -- expands its rows to bf16 in LDS once per workgroup
 *     of 4 waves (launches of more than 64 queries: 8; f8_lds_waves fixes it) instead of once per wave (hdb_mfma_f8_lds.h): a stage of rows is loaded with 16-byte loads,
 *     converted and stored to a swizzled, double-buffered image that every wave reads its fragments from.  Same query parts, K walk
 *     and epilogue, same plan otherwise: indices, score bits and status words are those of the call with the option off.
 *     f8_lds_min_q = n >= 1: from max(n, 5, mfma_min_q) queries on; -1: from hdb_mfma_f8_lds_min_q(d) queries on (hdb_caps.h: 32 at
 *     d = 384 / 768, 64 at d = 128 / 256 / 512 / 4096, 0 = never at the widths not measured; profiles/f8_lds_time.txt).  Whatever stays off the float8 matrix cores stays off this flavour.
 *   - a matrix holding a NaN code raises the NaN flag (hdb_index_has_nan) like a NaN of any other dtype.
 *   - never: the single launches of the matrix-core paths (fused = 0 always), the LDS tile kernel of manhattan batches, the int8 shadow
 *     and its 5-bit plane (hdb_index_quantize returns HDB_ERR_UNSUPPORTED, auto_quant does not apply: one byte per element already
 *     is the shadow's stream); K slices for wider rows unless f8_ks_min_q asks for them.
 * Stats: mfma = 1 on the matrix-core path, fused = 0 (3 for the bit metrics' single launch); f8_lds = 1 when the last call's
 * matrix-core launches expanded the rows in LDS; f8_lds_min_q = the threshold in force for this index, 0 = never.
 * int8 matrices (HDB_I8).  Queries are float32.  Every stored integer widens to float32 exactly (one v_cvt_f32_i32 with a
 * sign-extending byte select per element), all arithmetic is float32 on unrounded float32 queries, and the contract is the float32
 * one: scores within 1e-5 of the reference's arithmetic on the widened matrix (hamming exact with the sign bit x > 0, jaccard 1e-6).
 * The matrix is always finite: hdb_index_has_nan is 0.  An int8 index plans exactly like a float8 index of the same shape with
 * f8_ks_min_q = 0 and f8_lds_min_q = 0:
 *   - 1-4 queries, every metric, any d, any k, bias, row mask and row list, and every batch no other path takes: the VALU scan, four
 *     queries per pass, through the small, sampled, exact and full-sort pipelines.  Rows of 256, 384 and 512 bytes take the float8
 *     flavour's unrolled ONE-query kernels on its grid sized by bytes.  Manhattan batches stay on the 4-queries-per-pass scan.
 *   - 5+ dot / cosine / euclidean / pearson queries, d = 128, 256, 384 or 512, use_mfma on: the matrix cores (hdb_mfma_i8.hip), the
 *     float8 flavour's kernel with another row converter: eight signed bytes become eight bf16 in registers (exact: |x| <= 128 has
 *     at most 8 significant bits), the query travels as three exact bf16 parts, same K walk and epilogue -- indices, score bits and
 *     status words are those of a bfloat16 index over the widened matrix.  Other widths stay on the VALU scan.
 *   - never: the single launches of the matrix-core paths, the manhattan tile kernel, K slices, the LDS flavour, the int8 shadow and
 *     its plane (hdb_index_quantize returns HDB_ERR_UNSUPPORTED: one byte per element already).
 * Stats: mfma = 1 on the matrix-core path, fused = 0 (3 for the bit metrics' single launch).
 * packed-bit matrices (HDB_B1).  Layout: n x d / 32 uint32 words, element e of a row = bit e & 31 of word e >> 5; d % 32 == 0
 * (HDB_ERR_ARG otherwise) and d <= 7680.  Queries are float32 x d.  Contract: every metric is the reference's arithmetic on the 0/1
 * float32 matrix the bits stand for -- scores within 1e-5 * max(1, |s|), hamming exact (x > 0 is the bit itself), jaccard 1e-6; no
 * scale, no +-1 reading, no centring; hdb_index_has_nan is 0.  Row caches: ||v||^2 is the row's popcount, 1/||v|| = 1/sqrt(pop)
 * (0 -> 1), the pearson scale comes from pop and d (an all-0 or all-1 row is a constant row: NaN), the sign cache is a re-layout
 * of the words.
 *   - dot / cosine / pearson / euclidean / manhattan: hdb_bscan.hip, one thread per row, through the small, sampled, exact and
 *     full-sort pipelines.  The score of a row is sum_j (b_j ? A_j : B_j) over the per-element terms themselves (A = q, B = 0 q;
 *     (1 - q)^2, q^2; |1 - q|, |q|), four elements at a time from a per-query table in LDS, in ONE summation order per row: the
 *     sample pass, the filter pass, hdb_topk_exact and hdb_scores return the same float32 bits for a row, whatever the grid.
 *   - hamming / jaccard: the bit kernels that every dtype uses, on the sign cache; such calls plan exactly as on an int8 index.
 *   - on request (option b1_mfma_min_q, 0 = never by default): batches of 5+ dot / cosine / euclidean / pearson queries on rows of
 *     d = 128, 256, 384 or 512 bits, and in K slices (bfloat16's slice list) on d = 640 .. 1536 in steps of 128, 2048, 3072 and 4096,
 *     run on the bf16 matrix cores (hdb_mfma_b1.h), multi-kernel pipeline: a bit is exactly one bf16 number, expanded per fragment in
 *     registers; float32 queries as three exact bf16 parts, the bfloat16 flavour's K walk and epilogue.  Dot, cosine and euclidean
 *     return the indices, score bits and status words of a bfloat16 index over the unpacked 0/1 matrix (wider rows: going through
 *     ITS K slices); pearson takes the cosine epilogue with its own row scale and keeps the 1e-5 contract.  b1_mfma_min_q = n >= 1:
 *     from max(n, 5, mfma_min_q) queries on; -1: from hdb_mfma_b1_min_q(d) queries on (hdb_caps.h, 0 there = never).  Manhattan, the
 *     bit metrics, 1-4 queries, other widths, matrices of up to 8192 rows and use_mfma = 0 stay on the bit scan; a base that is only
 *     4-byte aligned is served.  Off by default: the default dispatch of packed-bit rows is pinned (tests/b1_plan_check.hip).
 *   - never: the 1-4-query and batched single launches, the manhattan tile kernel, the int8 shadow and its plane
 *     (hdb_index_quantize returns HDB_ERR_UNSUPPORTED), the row list (a call with a list set is the masked call, bit for bit); the
 *     matrix cores unless b1_mfma_min_q asks for them.
 * Stats: mfma = 0 (1 on the matrix-core path of b1_mfma_min_q), quant = 0, plane = 0, subset = 0, fused = 0 (3 for the bit metrics'
 * single launch); b1_mfma_min_q = the threshold in force for this index, 0 = never. */
int hdb_topk(hdb_index* ix, const void* dev_Q, int32_t nq, int32_t k, int metric,
             int64_t* dev_idx, float* dev_score, int32_t* dev_status, void* stream);

/* hdb_topk + copy of the packed result record ([nq*k int64][nq*k f32][nq i32], hdb_packed_bytes) into host memory
 * (pinned memory recommended) + stream synchronisation, in one call: what one HyperDB.query() needs.  Queries whose
 * sampled threshold failed are re-run through the exact path before returning; on return every status word is 0
 * except HDB_Q_NAN.  Saves the caller-side allocations and the extra host round trips of doing this in Python. */
int hdb_topk_host(hdb_index* ix, const void* dev_Q, int32_t nq, int32_t k, int metric, void* host_record, void* stream);

/* Same contract, but by materialising all n scores per query and radix-selecting them:
 * always exact, any tie pattern, any k <= HDB_MAX_K; dev_status is written as 0 (HDB_Q_NAN apart) whatever the queries hold --
 * an infinite query element included.  The scores are hdb_topk's own bits; where hdb_topk would multiply float32 rows as bf16
 * parts, this call does so only while no query of the call holds an infinity (it reads the query flags back: one stream
 * synchronisation, on float32 cosine / euclidean / pearson batches only) and uses the fp32 MFMAs otherwise. */
int hdb_topk_exact(hdb_index* ix, const void* dev_Q, int32_t nq, int32_t k, int metric,
                   int64_t* dev_idx, float* dev_score, int32_t* dev_status, void* stream);

/* Rerank: the exact top-k of every query among ITS OWN list of rows (local-hyperdb_amd/csrc/hdb_rerank.hip) -- the second half of
 * a two-stage search (candidates from a cheap index, rescored against this one), of hybrid search and of per-query filters.
 * dev_cand: [nq][m] int64, row-major, device; ids as hdb_topk returns them (row_base added), so the output of one index feeds
 * another with the same base.  1 <= m <= HDB_CAND_CAP (8192) and 1 <= k <= m, anything else is HDB_ERR_ARG.
 * The list of query q:
 *   - a negative id is padding (the -1 tail of a short first stage) and is skipped silently;
 *   - an id outside [row_base, row_base + n) is skipped and sets HDB_Q_BADROW in the query's status word.  The id is compared
 *     against the bounds before any address is formed from it: no row, cache or mask byte of such an id is read;
 *   - an id listed twice counts once;
 *   - the rest are scored with the handle's bias added and its row mask applied (a masked row is never returned; a row list set
 *     with hdb_index_set_row_subset is ignored);
 *   - the result is ordered by (score descending, id ascending); where fewer than k rows remain the tail is -1 / -inf.
 * Status: 0, HDB_Q_NAN, HDB_Q_BADROW.  Nothing is sampled, so nothing is ever re-run.
 * Served: HDB_F16, HDB_F32, HDB_F64 (float64 queries), HDB_BF16, HDB_F8E4M3, HDB_I8 matrices; dot, cosine, euclidean, manhattan,
 * pearson; any d.  Rows that are whole 16-byte pieces of a 16-byte aligned matrix are read with 16-byte loads, everything else
 * element by element.  HDB_B1 matrices, hamming and jaccard return HDB_ERR_UNSUPPORTED: a bits index is a FIRST stage.
 * Scores: a returned row carries the float32 bits the VALU scan gives that row on this handle -- the indices and score bits of
 * hdb_topk_exact with use_mfma = use_fused = use_quant = use_l1_tile = 0 under a row mask that keeps exactly the query's valid
 * candidates.  The score of a (query, row) pair does not depend on the row's place in the list, on the other candidates or on
 * the other queries.  The 1e-5 band (1e-3 float16) against the reference's arithmetic on V[cand[q]] follows.
 * Launches per chunk of queries: query preparation (pearson: and centring), list preparation (one workgroup per query sorts the
 * list in LDS, drops padding, out-of-range, masked and repeated ids and writes the status word), the scoring pass (a 16-lane
 * group per candidate, the query in LDS) and the finalize of the multi-kernel pipeline.  Option rerank_chunk: queries per chunk
 * (0: up to 256).  Stats: rerank = 1, chunks; hdb_topk sets rerank = 0.
 * hdb_rerank_host: the same, then the packed record (hdb_packed_bytes(nq, k)) in host memory and one stream synchronisation.
 * Not built: rerank onto an HDB_B1 index and the bit metrics, lists longer than 8192, groups and sharded indexes (ids would need
 * routing to shards), one launch that scores and selects a short list, the matrix cores (a gather of a few hundred rows per
 * query is bound by latency). */
int hdb_rerank(hdb_index* ix, const void* dev_Q, int32_t nq, const int64_t* dev_cand, int32_t m, int32_t k, int metric,
               int64_t* dev_idx, float* dev_score, int32_t* dev_status, void* stream);
int hdb_rerank_host(hdb_index* ix, const void* dev_Q, int32_t nq, const int64_t* dev_cand, int32_t m, int32_t k, int metric,
                    void* host_record, void* stream);

/* Two-stage search in one call: hdb_topk of k1 on `first` (any dtype and metric, HDB_B1 and hamming included; dev_Q1 are ITS
 * queries), kept on the device, then hdb_rerank of those [nq][k1] ids on `second` with dev_Q2 and metric2, top k, as one packed
 * record in host memory.  Stage one's status words are read back (one small copy and a synchronisation) and its failed queries
 * re-run exactly, as hdb_topk_host does, before their ids are used; the record's status words are the rerank's.
 * `first` and `second` must be on the same device with the same n and row_base, 1 <= k1 <= min(8192, n) and 1 <= k <= k1;
 * otherwise HDB_ERR_ARG.  They may be the same handle. */
int hdb_two_stage_host(hdb_index* first, const void* dev_Q1, int metric1, int32_t k1,
                       hdb_index* second, const void* dev_Q2, int metric2, int32_t k,
                       int32_t nq, void* host_record, void* stream);

/* Grouped top-k: the best row of each group, k distinct groups per query ("group by" / "collapse": the rows are chunks, a group is
 * the document they were cut from -- source_indices of the reference's data model).
 * Semantics.  Order the eligible rows of a query -- not masked; bias added; NaN -> -inf -- by (score descending, row ascending), the
 * order of hdb_topk.  A group's representative is its first row in that order; the grouped top-k is the first k representatives, in
 * that order: no group twice, and with fewer than k groups among the eligible rows the tail is -1 / -inf.  A group whose rows are all
 * excluded (or all at -inf) is not returned.  Walking the ungrouped ranking from the top and keeping each group's first occurrence
 * gives exactly this answer as soon as k groups have been seen.
 *
 * hdb_index_set_groups: dev_groups = n int32 ids in [0, n_groups), one per row, device memory, borrowed like bias and mask until
 * replaced or cleared (NULL clears; 1 <= n_groups <= 2^31 - 1).  hdb_index_extend, hdb_index_update and hdb_index_gather drop the
 * ids with mask and bias; hdb_index_rebase keeps them.  The library does not trust them: every kernel compares an id against
 * [0, n_groups) before it forms an address from it; a row whose id is outside counts as masked for that call and sets HDB_Q_BADROW
 * in the status words of the call.
 *
 * hdb_topk_grouped_host: the grouped top-k of nq queries as the packed record of hdb_topk_host (hdb_packed_bytes(nq, k)) in host
 * memory; indices are the representatives' rows (row_base added), scores theirs; the call synchronises `stream`.
 * 1 <= k <= HDB_MAX_K (0 or less: HDB_ERR_ARG; more: HDB_ERR_UNSUPPORTED); no groups set: HDB_ERR_ARG.  The sizes are judged before
 * the handle, the handle before any HIP call.  Served: every dtype (HDB_B1 included) with dot, cosine, euclidean, manhattan and
 * pearson; hamming and jaccard return HDB_ERR_UNSUPPORTED.  Status words on return: 0, HDB_Q_NAN, HDB_Q_BADROW -- never
 * HDB_Q_GROUPS_SHORT, HDB_Q_UNDERFLOW or HDB_Q_OVERFLOW.
 * How it runs (local-hyperdb_amd/csrc/hdb_group_plan.h, hdb_group.hip).  Fast rounds: hdb_topk of k1 = min(n, HDB_MAX_K,
 * k * group_oversample) into a device record -- on whatever path that call takes: single launch, shadow, matrix cores, row list --,
 * one collapse launch, and the nq status words read back (one small copy, one synchronisation).  The queries flagged
 * HDB_Q_GROUPS_SHORT run a second round at k2 = min(n, HDB_MAX_K, 4 * k1) where k2 > k1, one by one.  A query whose sampled call failed
 * (HDB_Q_UNDERFLOW / HDB_Q_OVERFLOW) or that is still short after the last round goes to the exact grouped pass: the exact shape of
 * the multi-kernel pipeline -- all scores of a chunk of queries in the workspace -- with two launches before the radix selection:
 * best[q][g] = max over the group's rows of the packed (score, row) key (64-bit atomicMax, adjacent rows of one group combined in
 * the wave first), then every row that is not its group's best is set to -inf, the state a masked row is in.  best is
 * cq x n_groups x 8 bytes of the call's workspace and counts against exact_bytes when the chunk size cq is chosen.
 * Scores: a fast round returns the float32 bits hdb_topk returns for the row; the exact pass those of hdb_topk_exact.  Where the
 * two differ (a default float16 index rounds float32 queries for the matrix cores) the representative of a group may differ between
 * the two within the dtype's tolerance, as it may between hdb_topk and hdb_topk_exact.
 * Options: group_oversample (1 .. 64, default 4), group_fast_rounds (0 .. 2, default 2; 0 = always the exact pass).
 * Stats: grouped (1 after a grouped call; hdb_topk and hdb_rerank set it to 0), group_k (rows per query of the last fast round
 * run, 0 = none), group_rounds (fast rounds run), group_exact (queries answered by the exact pass); the other stats are those of
 * the last inner call.
 *
 * hdb_collapse_groups: the primitive on its own.  dev_idx / dev_score: any ranked list [nq][m], 1 <= k <= m <= HDB_MAX_K (anything else:
 * HDB_ERR_ARG), ids as hdb_topk, hdb_rerank and hdb_two_stage_host return them (row_base added), so grouping composes with those
 * calls; dev_groups / n_groups / n / row_base describe the rows as for hdb_index_set_groups.  Output [nq][k]: each group's first
 * occurrence in list order, then -1 / -inf.  A negative id, or an entry at -inf, is padding.  An id outside [row_base, row_base + n)
 * is skipped and sets HDB_Q_BADROW -- nothing is read for it --, and so does an id whose group id is outside [0, n_groups).
 * dev_status (nq words, may be NULL) is read and written: HDB_Q_NAN is carried over from the call that ranked the list, every
 * other bit is replaced by HDB_Q_BADROW and HDB_Q_GROUPS_SHORT: fewer than k groups were found and the list was not exhaustive.  A
 * list is exhaustive when it holds padding or when m >= n.  The outputs must not overlap the inputs.
 * Not built: hamming / jaccard grouped calls, k > HDB_MAX_K, several GPUs (a group can span shards: a second collapse after the
 * merge), more than one hit per group, per-group hit counts, a grouped stage inside hdb_two_stage_host (compose it with
 * hdb_collapse_groups), threshold estimation that knows about groups. */
int hdb_index_set_groups(hdb_index* ix, const int32_t* dev_groups, int64_t n_groups);
int hdb_topk_grouped_host(hdb_index* ix, const void* dev_Q, int32_t nq, int32_t k, int metric, void* host_record, void* stream);
int hdb_collapse_groups(const int64_t* dev_idx, const float* dev_score, int32_t nq, int32_t m, int32_t k, const int32_t* dev_groups,
                        int64_t n_groups, int64_t n, int64_t row_base, int64_t* dev_idx_out, float* dev_score_out, int32_t* dev_status,
                        int device, void* stream);

/* Multi-vector queries: a query is a SET of vectors, a document a group of rows, and groups are ranked by the sum over the set's
 * vectors of each vector's best row in the group -- late interaction (ColBERT / ColPali style stores: token or patch vectors) and
 * multi-query fusion (T paraphrases of one question over source_indices groups; every row its own group: the sum of the scores).
 * Semantics.  A call carries ns sets; set s is the vectors dev_Q[host_off[s] .. host_off[s + 1]) of one flat float32 matrix
 * (float64 for an HDB_F64 index), T_s = host_off[s + 1] - host_off[s] >= 1.  x(t, r) is the score every exact call of this handle
 * ranks by: the metric's score with the handle's bias added, -inf where the row mask excludes the row, where the score is NaN or
 * where the row's group id is outside [0, n_groups); its bits are those hdb_topk_exact gives that row in a call of the same vectors.
 * (Euclidean: the score pass stays on the VALU scan, which sums the differences themselves -- the bits hdb_topk_exact gives a row it
 * re-scores.  The matrix cores' ||v||^2 + ||q||^2 - 2 v.q cancels on a row close to a query vector, the row a group's maximum picks.)
 *   score(s, g) = canon(((x_0 + x_1) + ...) + x_{T-1}),  x_i = max over the rows r of g of x(host_off[s] + i, r)
 * in float32, one add per vector, in vector order; canon: NaN -> -inf.  A group without an eligible row, or with a term at -inf,
 * scores -inf.  The answer of set s is the first k groups by (score descending, group id ascending); groups at -inf are never
 * returned: the tail is -1 / -inf.  The bias enters every term, T times in all.  The result does not depend on how the vectors are
 * chunked as long as the vectors' score bits do not; on integer data they never do.
 *
 * hdb_maxsim_host: the answer of ns sets as the packed record of hdb_topk_host (hdb_packed_bytes(ns, k)) in host memory; indices
 * are GROUP ids, scores the group scores; the call synchronises `stream`.  ns >= 1 and 1 <= k (else HDB_ERR_ARG), k <= HDB_MAX_K
 * (else HDB_ERR_UNSUPPORTED), host_off[0] == 0 and strictly increasing (else HDB_ERR_ARG naming the set); then the handle; no groups
 * set: HDB_ERR_ARG.  Served: every dtype (HDB_B1 included) with dot, cosine, euclidean, manhattan and pearson; hamming and jaccard
 * return HDB_ERR_UNSUPPORTED.  Status word of a set: HDB_Q_NAN where one of its vectors holds a NaN, HDB_Q_BADROW for every set
 * where a row's group id is outside [0, n_groups) (such a row counts as masked; nothing is indexed with its id).
 * How it runs (local-hyperdb_amd/csrc/hdb_maxsim_plan.h, hdb_maxsim.hip).  On the first call after hdb_index_set_groups the index
 * builds an inverted index of the ids on the device -- grp_rows, the rows ordered by (group id, row), by a stable radix sort, and
 * grp_off, n_groups + 1 offsets -- and keeps it until the ids are replaced, cleared or dropped (hdb_index_extend / _update / _gather
 * drop it, hdb_index_rebase keeps it).  The index is derived from the ids as they stood at that call: a caller who rewrites the borrowed
 * array in place must call hdb_index_set_groups again (the grouped call reads the ids afresh on every call; this one does not).
 * Ids that are non-decreasing by row -- a document's chunks are adjacent rows -- are their own
 * index: only the offsets are built and the reduction reads the scores contiguously (stat maxsim_sorted).  The sets are handled in
 * blocks of sb whose running sums acc[sb][n_groups] fit the budget; inside a block the flat vector range goes through the exact
 * score pass of the multi-kernel pipeline in chunks of cq <= 256 vectors (128 in K slices) -- VALU scan on matrices of up to 8192
 * rows, the matrix cores where the plan of a call of that many queries says so (never for euclidean, above) -- and chunks may cut across set boundaries: one pass
 * over V serves several sets.  After each chunk one launch reduces sbuf[cq][n] into acc: a team of 1 | 4 | 16 | 64 lanes owns a
 * group, takes the maximum over the group's rows per vector and adds it to the set's running sum -- no atomics, one owner per
 * element, a fixed order of adds.  Per block the radix selection of the exact pipeline runs over acc (n = n_groups, row_base 0).
 * sbuf (4 bytes per vector and row) and acc (4 bytes per set and group) count against exact_bytes.
 * Options: maxsim_team (0 = the rule from n / n_groups, hdb_caps.h; 1 | 4 | 16 | 64 = fixed; no call is answered differently for it).
 * Stats: maxsim (1 after such a call; hdb_topk, hdb_rerank and the grouped call set it to 0; a multi-vector call sets grouped =
 * rerank = 0), maxsim_chunks (score-pass launches' chunks), maxsim_team, maxsim_sorted, maxsim_bytes (the inverted index as held);
 * mfma / path are those of the score pass.
 * Not built: several GPUs / shards; hamming / jaccard; k > 2048; a score pass that reduces in its own epilogue without the
 * [vectors][rows] round trip (the follow-up); per-vector weights; splitting one huge group over teams (one team walks it: correct,
 * slow). */
int hdb_maxsim_host(hdb_index* ix, const void* dev_Q, const int32_t* host_off, int32_t ns, int32_t k, int metric,
                    void* host_record, void* stream);   /* record: hdb_packed_bytes(ns, k); indices are GROUP ids */

/* Diverse top-k: maximal marginal relevance (MMR) over a call's candidates -- a hit is paid for its relevance and charged for being
 * a near copy of a hit already chosen (the search_type "mmr" of retrieval stacks).  Grouping covers "ten chunks of one document"; this
 * covers ten near-identical chunks of ten different documents.
 * Semantics.  Input per query: a list (id_i, r_i), i = 0 .. m - 1, as hdb_topk, hdb_rerank, hdb_two_stage_host and hdb_collapse_groups
 * return it: ids carry row_base, the relevance r_i is the list's float32 score with bias, mask and path already in it; the list need
 * not be sorted.  An id < 0 is padding and so is an entry at -inf; an id outside [row_base, row_base + n) is skipped and sets
 * HDB_Q_BADROW -- it is compared against the bounds before any address is formed from it, nothing is read for it --; an id listed
 * twice counts once, at its first list position.  The surviving entries, in list order, are the query's candidates.  The handle's
 * bias, mask, row list and groups are not read.
 *   p(a, b), the similarity of two stored rows under pair_metric (HDB_DOT, HDB_COSINE, HDB_EUCLIDEAN), no bias, no mask: stored
 *   values widened exactly to the accumulate type (float32; double for an HDB_F64 index, the result cast to float32), products
 *   accumulated with explicit fma in element order e = 0 .. d - 1; euclidean sums the squared differences themselves, as the VALU
 *   scan does, and is 1 / (1 + sqrt(sum)) -- never ||a||^2 + ||b||^2 - 2 a.b, which cancels on the near copies this call exists
 *   for; cosine is dot * inv_norm[lower row] * inv_norm[higher row] from the index's cache (zero norm: 1); NaN -> -inf.  p is
 *   evaluated once per unordered pair and mirrored, and depends on the two rows only: not on list positions, tiles, the other
 *   candidates or the other queries.
 *   Selection, with lam = (float)lambda, oml = 1.0f - lam: step 0 picks the candidate with the largest r_i; step t >= 1 picks the
 *   unselected candidate with the largest val_i = canon(lam * r_i - oml * pen_i), pen_i = max over the selected s of p(i, s) -- two
 *   rounded float32 products and one rounded subtraction, no contraction; canon: NaN -> -inf.  Ties go to the lowest list position.
 *   Every candidate is eligible until it is chosen (one at val = -inf is picked when nothing better is left); the call stops after
 *   min(k, candidates) picks.
 * Output: [nq][k] ids and their relevances r IN PICK ORDER -- not re-sorted by score --, tail -1 / -inf.  Status word: HDB_Q_NAN is
 * carried over from the word that came in, HDB_Q_BADROW is set as above, every other bit is cleared.  lambda = 1 returns the first k
 * candidates by (relevance descending, position ascending); lambda = 0 picks by relevance first and then whatever is least like
 * anything already chosen.
 *
 * hdb_mmr: the primitive; it takes any ranked list, so it composes with hdb_topk, hdb_rerank, two-stage and hdb_collapse_groups.
 * 1 <= k <= m <= HDB_MAX_K and lambda in [0, 1] (anything else, NaN included: HDB_ERR_ARG), a pair_metric other than the three:
 * HDB_ERR_UNSUPPORTED, nq < 0: HDB_ERR_ARG, nq == 0: HDB_OK -- all judged before the handle, and the handle (NULL: HDB_ERR_ARG;
 * HDB_B1: HDB_ERR_UNSUPPORTED, a bits index is a first stage) before any HIP call.  The six byte-addressed dtypes
 * are served, any d.  Outputs must not overlap inputs.  dev_status [nq] is read and written, and may be NULL.
 * hdb_mmr_host: one call for the common case -- hdb_topk of m (<= n, else HDB_ERR_ARG) rows per query under `metric` (any metric
 * hdb_topk takes, the bit metrics included) into a device record, on whatever path that call takes; its status words are read back
 * and failed queries re-run exactly; hdb_mmr over the record; the packed record (hdb_packed_bytes(nq, k)) goes to host memory and
 * `stream` is synchronised.  nq >= 1.
 * How it runs (local-hyperdb_amd/csrc/hdb_mmr_plan.h, hdb_mmr.hip).  Queries go in chunks of cq = clamp(exact_bytes / (mp^2 4), 1,
 * min(nq, 256)), mp = m rounded up to 16: the pair matrices P [cq][mp][mp] of a chunk live in the workspace.  Three launches per
 * chunk: prep (one workgroup per query validates and compacts the list in list order; first occurrences by the sort of
 * hdb_collapse_groups), pairs (grid = tile pairs ti <= tj x queries; 16-lane groups gather candidate rows in 16-byte pieces into LDS,
 * one pair per thread, no atomics) and select (one workgroup per query, min(k, candidates) steps: val, a 64-bit argmax by wave
 * shuffles and one LDS exchange, one coalesced row of P to raise the penalties).  Separate launches: the kernel boundary makes P
 * visible; nothing spins on a flag.
 * Options: none of its own; chunking obeys exact_bytes.
 * Stats: mmr (1 after either call; hdb_topk, hdb_rerank, the grouped call and the multi-vector call set it to 0; an MMR call sets
 * rerank = grouped = maxsim = 0), mmr_chunks; after hdb_mmr_host the other stats are those of its hdb_topk.
 * Not built: a one-workgroup flavour that keeps P in LDS for m up to about 190 and drops two launches; p computed on the fly without
 * the m^2 matrix for large batches; the matrix cores for the pair pass; manhattan / pearson / bit-metric pair similarity and HDB_B1
 * handles; m > 2048; several GPUs / shards; MMR inside the grouped and the multi-vector call (compose through hdb_mmr); returning
 * the val of each pick. */
int hdb_mmr(hdb_index* ix, const int64_t* dev_idx, const float* dev_score, int32_t nq, int32_t m, int32_t k, double lambda,
            int pair_metric, int64_t* dev_idx_out, float* dev_score_out, int32_t* dev_status /* read and written, may be NULL */,
            void* stream);
int hdb_mmr_host(hdb_index* ix, const void* dev_Q, int32_t nq, int32_t m, int32_t k, int metric, double lambda, int pair_metric,
                 void* host_record /* hdb_packed_bytes(nq, k) */, void* stream);

/* Merge `parts` per-shard top-k lists (the all-gathered [parts][nq][k] buffers of the row-sharded
 * index) into the global top-k per query, same ordering rule.  Every part list must be ordered as hdb_topk writes
 * it: score descending, row ascending, unused slots (index -1) at the end. */
int hdb_merge_topk(const int64_t* dev_idx_parts, const float* dev_score_parts, int32_t parts,
                   int32_t nq, int32_t k, int64_t* dev_idx, float* dev_score, int device, void* stream);

/* Packed per-shard result record used for the exchange step (ONE RCCL all-gather per query batch):
 *   [nq*k int64 indices][nq*k float32 scores][nq int32 status], padded to a multiple of 16 bytes.
 * hdb_packed_bytes gives the record size; hdb_topk can write straight into such a record (pass
 * base, base + nq*k*8, base + nq*k*12).  hdb_merge_topk_packed merges `parts` gathered records and
 * ORs their status words per query into dev_status (may be NULL). */
int64_t hdb_packed_bytes(int32_t nq, int32_t k);
int hdb_merge_topk_packed(const void* dev_gathered, int32_t parts, int32_t nq, int32_t k, int64_t* dev_idx,
                          float* dev_score, int32_t* dev_status, int device, void* stream);
/* The same merge on the HOST, for records that are already in host memory (one process per GPU on one node: every rank's
 * hdb_topk_host leaves its record in host memory, the ranks swap the 1.2 KB records through a shared-memory segment and
 * merge here -- a few microseconds instead of a collective, a merge launch and another synchronisation).  `records` =
 * `parts` packed records back to back (shard p's rows precede shard p+1's), `out_record` = one packed record; same total
 * order (score descending, global row ascending), status words OR-ed per query, missing entries -1 / -inf.  No GPU call. */
int hdb_merge_topk_host(const void* records, int32_t parts, int32_t nq, int32_t k, void* out_record);
/* The swap itself, for `world` processes of one node that have all mapped the same zero-initialised shared-memory segment
 * `shm` of 2 * world * stride bytes (hyperdb/sharded.py HostExchange creates it): slot (parity, rank) = 64-byte header
 * {seq} + record.  Exchange number seq (1, 2, ... in lockstep on every rank) copies `record` (hdb_packed_bytes(nq, k)
 * bytes, <= stride - 64) into this rank's slot of parity seq & 1, publishes seq behind it (release), waits until every
 * rank's slot carries seq (acquire; HDB_ERR_HIP after timeout_s) and merges the `world` records straight out of the
 * segment into out_record like hdb_merge_topk_host.  A slot is rewritten two exchanges later, which no rank can reach
 * before everybody has published the exchange in between, i.e. has finished reading this one.  No GPU call. */
int hdb_host_exchange_merge(void* shm, int64_t stride, int32_t world, int32_t rank, uint64_t seq, const void* record,
                            int32_t nq, int32_t k, void* out_record, double timeout_s);

/* Single-process multi-GPU group: HyperDB.query() (hyperdb.py:1584) is a single-process
 * call, so the row-sharded matrix must be reachable without a launcher.  A group is `parts` row shards, each an hdb_index
 * created on its own device with its row_base (a device may hold several shards).  hdb_group_topk_host copies the
 * queries (HOST memory, nq x d float32, or float64 for F64 matrices) into a pinned staging buffer every device can read,
 * runs hdb_topk_host on every shard concurrently (one worker thread and one stream per shard; between calls a worker spins
 * briefly on the job word, then parks), lets each shard's last kernel store its packed record into a pinned, portable
 * host buffer that every device can write, merges the `parts` records on the host (as hdb_merge_topk_host) and returns
 * the merged packed record (hdb_packed_bytes layout) in host_record.  A shard whose sampled threshold failed re-runs those
 * queries locally through the exact selection before it reports: on return every status word is 0 except HDB_Q_NAN.
 * Bias / mask are set per shard on the shards' own handles (recency: pass the GLOBAL newest timestamp as ts_max to
 * hdb_recency_bias).  Any k the single index takes is accepted (the merge runs on the host).
 * The group borrows the shard handles: destroy the group first, then the shards. */
typedef struct hdb_group hdb_group;
int hdb_group_create(hdb_group** out, hdb_index* const* shards, int32_t parts);
int hdb_group_topk_host(hdb_group* g, const void* host_Q, int32_t nq, int32_t k, int metric, void* host_record);
void hdb_group_destroy(hdb_group* g);

/* Largest k served by the selection kernels.  hdb_topk / hdb_topk_exact accept any k: above HDB_MAX_K (on a
 * matrix of more than 8192 rows) they materialise the scores of each query and radix-sort them (cold path,
 * "top_k > N returns all rows sorted", ranking_algorithm.py:195-200).
 * The two DEVICE merges, hdb_merge_topk and hdb_merge_topk_packed, rank parts*k entries per query in LDS and return
 * HDB_ERR_UNSUPPORTED beyond parts*k = 8192 (8 ranks: k > 1024).  Nothing above the C ABI is limited by that:
 * hdb_merge_topk_host, hdb_host_exchange_merge and hdb_group_topk_host merge on the host with any parts*k, and the
 * one-process-per-GPU path (hyperdb/sharded.py) copies the all-gathered records to the host and calls
 * hdb_merge_topk_host whenever parts*k exceeds the cap, with either exchange transport. */
#define HDB_MAX_K 2048

/* Tuning knobs / introspection (bench and tests): name -> value, returns HDB_ERR_ARG if unknown.
 * Options:  max_blocks (0 = automatic grid of the row scans), force_exact (1: always the exact selection),
 *   sample_target (expected survivors of the sampled threshold, 0 = automatic), use_mfma (0: VALU scans only),
 *   mfma_min_q (smallest batch that takes the MFMA scan on fp16 matrices, default 1), mfma_variant (16 | 32: MFMA
 *   shape of the 256-query pass), bits_fused (0: hamming / jaccard always through the exact selection; 3: one-query calls on 1M+ rows keep the six launches),
 *   host_direct (0: hdb_topk_host always copies through a device record), exact_bytes (score workspace cap of
 *   the exact path), finalize_threads (256 | 512 | 1024), profile (1: HIP events around the pass over V),
 *   use_fused (0: never the single-launch pipeline), fused_timeout_us (bound of its in-kernel spins, default 2000),
 *   host_poll (0: hdb_topk_host always waits on the stream instead of polling the status words of a pinned record),
 *   dyn_tiles (0: the batched MFMA filter pass always splits its tiles statically; default 1 = tiles from a counter for
 *   long passes over rows of >= 768 bytes with up to 64 queries), dyn_min_mb (... for passes of at least this many MiB of V per
 *   workgroup, default 16, >= 0), dyn_heavy (1: also when all eight waves multiply; default 0),
 *   bits_local (0: the bit metrics' single launch never takes its local flavour, every workgroup its own threshold).
 *   The local flavour of the 1-4-query single launch (short matrices: no row sample, no exchange): use_local (0: never), local_m
 *   (rows every workgroup emits at least, 0 = automatic, 0 .. 64), local_max_tiles (tiles per workgroup up to which it is taken,
 *   default 4, >= 1), local_small (1: also on matrices of up to 8192 rows), local_max_q (calls of up to this many queries, default 1).
 *   The row list (hdb_index_set_row_subset, above): use_subset (0: never the list -- the mask), subset_min_n (matrices of at least
 *   this many rows; -1, also for any negative value: the measured rule), subset_ratio (the list while m * ceil(nq / 4) *
 *   subset_ratio <= n; -1, also for any negative value: the measured rule; otherwise at least 1).
 *   Dispatch of few-query calls (-1 = the measured rule): fused_max_q (the 1-4-query single launch takes
 *   calls of up to this many queries), f32_min_q (float32 matrices: the matrix-core scan from this many queries on), bf16_ks_min_q
 *   (bfloat16 rows wider than 512 elements: K slices from this many queries on, never fewer than 5), f8_ks_min_q (float8 rows wider
 *   than 512 elements: 0 = never, the default; n >= 1 = K slices from max(n, 5, mfma_min_q) queries on; -1 = hdb_mfma_f8_ks_min_q(d)), f8_lds_min_q
 *   (float8 batches with the rows expanded to bf16 in LDS once per workgroup: 0 = never, the default; n >= 1 = from max(n, 5, mfma_min_q)
 *   queries on; -1 = hdb_mfma_f8_lds_min_q(d), 0 there = never), f8_lds_waves (waves per workgroup of that flavour: 0 = by the launch's queries, the default; 4 | 8), b1_mfma_min_q
 *   (packed-bit batches on the bf16 matrix cores: 0 = never, the default; n >= 1 = from max(n, 5, mfma_min_q) queries on; -1 =
 *   hdb_mfma_b1_min_q(d), 0 there = never), bits_max_q
 *   (hamming / jaccard: single launches of four queries up to this many queries, more through the six launches in one go);
 *   use_batch1 (0: never the batched single launch), use_l1_tile (0: manhattan batches stay with the 4-query scan),
 *   l1_packed (0: that tile kernel always subtracts in float32; default 1 = packed fp16 differences on fp16 rows while every query
 *   element is an fp16 number and every element of the matrix and of the queries is within 32752 = 65504 / 2 in magnitude, so that
 *   no difference leaves fp16 range), f32_split (0: float32 batches never multiply as bf16 parts), f32_split_min_q.
 *   Int8 shadow (hdb_index_quantize): use_quant (0: never), quant_min_n (-1: the measured rule), quant_max_k (<= 128),
 *   bf16_quant (0, the default: hdb_index_quantize(HDB_QUANT_I8) refuses a bfloat16 matrix; 1: it builds an explicit shadow; means
 *   nothing on other dtypes),
 *   auto_quant (1: a large float16 index builds its own shadow on the first eligible call; 0: never), quant_batch_min_n (batches
 *   of 5+ queries through that shadow: -1 the measured rule, >= 0 from this many rows on), quant_batch_kernel (1: int8 matrix
 *   cores, 0: the v_dot4 scan four queries at a time), use_plane (0: one-query calls never pre-filter through the 5-bit plane),
 *   plane_min_n (-1: the measured rule), plane_cap_rows (0: n / 8; kept rows beyond which a call counts in plane_overflows -- a
 *   statistic: no call is answered differently for it), plane_wg_per_cu (workgroups per CU of the pass over the plane: 0 the
 *   measured table, 1 .. 8 that many -- for A/B runs, no call is answered differently for it).
 *   rerank_chunk (hdb_rerank: queries per chunk, 0 = automatic, up to 256; at most 256).
 *   group_oversample (hdb_topk_grouped_host: rows per wanted group in the first fast round, 1 .. 64, default 4), group_fast_rounds
 *   (0 .. 2, default 2; 0: every query through the exact grouped pass).
 *   maxsim_team (hdb_maxsim_host: lanes per group of its reduction, 0 = the rule, 1 | 4 | 16 | 64).
 *   max_blocks < 0 asks for -max_blocks workgroups per CU in the batched MFMA scan (measured: no gain).
 * Stats:    path (0 small, 1 sampled threshold, 2 exact, 3 full sort), mfma, fused (0 multi-kernel, 1 the 1-4-query single launch,
 *   2 the batched single launch, 3 the bit-metric single launch), local (1: that single launch in its local flavour), f32_split
 *   (1: a float32 batch multiplied as bf16 parts), f8_lds (1: float8 rows expanded in LDS), subset (1: the last call scored from
 *   the row list), host_direct, chunks, sample_rows, sample_m,
 *   scan_launches, scan_time_ns (sum over the profiled launches), cand_cap, n, ws_bytes, quant, quant_cands, quant_cands_min, quant_cands_median,
 *   quant_bytes, quant_auto, plane, plane_bytes, plane_survivors, plane_overflows, plane_blocks (workgroups of the last call's
 *   pass over the plane, 0 when it did not take it), rerank (1: the last call was hdb_rerank / hdb_rerank_host or the second
 *   stage of hdb_two_stage_host; then chunks counts its chunks and every other stat of the call is 0), grouped, group_k,
 *   group_rounds, group_exact (hdb_topk_grouped_host, above), maxsim, maxsim_chunks, maxsim_team, maxsim_sorted, maxsim_bytes
 *   (hdb_maxsim_host, above), mmr, mmr_chunks (hdb_mmr / hdb_mmr_host, above). */
int hdb_set_option(hdb_index* ix, const char* name, int64_t value);
int hdb_get_stat(hdb_index* ix, const char* name, int64_t* value);

#ifdef __cplusplus
}
#endif
#endif /* HYPERDB_HIP_H */
