// hdb_api.hip -- the C ABI of include/hyperdb_hip.h: handle, workspace and the top-k pipeline.
//
// hdb_topk = validate, plan, execute (topk_impl).  Which path a call takes is decided in ONE place, plan_topk (hdb_plan.h), a pure
// function that sees plain facts and no hdb_index; its TopkPlan carries everything the executors here consume and the statistics of
// the call (stats_begin stores plan.stats; nothing else starts a call's statistics).  One executor per path: quant_topk, quant_batch_topk,
// run_fused, run_bits1, run_batch1, run_full_sort, run_pipeline -- launches, workspace layouts and ensure_* calls, no rule.
//
// The multi-kernel pipeline (run_pipeline) for a chunk of queries (everything enqueued on the caller's stream):
//   n <= CAP            : thr = -inf -> scan(filter) -> finalize                (every row is a candidate)
//   otherwise           : scan(scores) over a strided row sample
//                         -> 4 radix-histogram passes -> thr[q] = m-th largest sample score
//                         -> scan(filter) over all rows (the only pass that touches all of V)
//                         -> finalize (sort <= 8192 candidates per query, emit k)
// hdb_topk_exact: scan(scores) over all rows -> 4 histogram passes -> collect (+ordered ties)
//                 -> finalize.  Used for hamming (integer scores, massive ties), for queries whose
//                 sampled threshold failed, and by tests as the on-device cross-check.
// Written once for all ranking calls (tests/test_host_calls_once.py): plan_call + stats_begin, select_exact (the radix selection),
// single_launch (the timing bracket of a one-launch pipeline); for the *_host calls HostRec (the device record and its way back),
// rerun_flagged (the exact re-run of queries whose sampled threshold failed), query_pitch, ranking_metric / ranking_k (argument checks).
#include "hdb_common.h"
#include "hdb_quant.h"
#include "hdb_ws.h"
#include "hdb_plan.h"
#include "hdb_group_plan.h"
#include "hdb_maxsim_plan.h"
#include "hdb_mmr_plan.h"
#include "hdb_devbuf.h"
#include "../../include/hyperdb_hip.h"
#include <string>
#include <cmath>
#include <cstring>
#include <cstdio>
#include <algorithm>
#include <vector>
#include <chrono>
#include <atomic>

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(HDB_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));           \
    } while (0)
#define LAUNCH_TRY(expr)                                                                           \
    do {                                                                                           \
        int e_ = (expr);                                                                           \
        if (e_ != 0) return fail(HDB_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString((hipError_t)e_)); \
    } while (0)

struct hdb_index {
    const void* V = nullptr;
    int64_t n = 0;
    int32_t d = 0;
    int dtype = HDB_F32;
    int device = 0;
    int64_t row_base = 0;
    // Device memory is owned through DevBuf (hdb_devbuf.h); a buffer's capacity is its `cap`, and a field beside it says more than that.
    // per-row caches (owned; the two change together, inv_norm.cap is the capacity in rows of both)
    DevBuf<float> inv_norm, sqnorm;
    DevBuf<int> nan_flag;             // device int
    hipStream_t build_stream = nullptr;
    // hamming sign bits (owned, lazy)
    DevBuf<uint32_t> bits;
    int64_t bits_npad = 0;            // its capacity in rows (bits.cap = bits_npad * W words), and a kernel argument
    int W = 0;
    bool bits_valid = false;
    int64_t bits_done = 0;            // rows [0, bits_done) are packed for the CURRENT matrix (hdb_index_extend keeps them: only the appended rows are packed)
    // pearson per-row scale 1/(sd*d) (owned, lazy)
    DevBuf<float> pscale;
    bool pscale_valid = false;
    int64_t pscale_done = 0;          // likewise
    // borrowed
    const float* bias = nullptr;
    const uint8_t* mask = nullptr;
    // ... and, beside the mask, the ascending list of the rows it keeps (hdb_index_set_row_subset): subset_m > 0 only with both set
    const int64_t* rows = nullptr;
    int64_t subset_m = 0;
    // ... and a group id per row (hdb_index_set_groups): n ids in [0, n_groups), checked by every kernel that reads one
    const int32_t* groups = nullptr;
    int64_t n_groups = 0;
    // ... and their inverted index (owned, lazy: hdb_maxsim_host builds it on its first call after hdb_index_set_groups; hdb_maxsim.hip):
    // grp_rows = the rows ordered by (group id, row) -- not built where the ids are non-decreasing by row (grp_sorted: the identity) --
    // grp_off = n_groups + 1 offsets into it, grp_flags = two device words: [0] an id outside [0, n_groups), [1] ids that decrease
    DevBuf<uint32_t> grp_rows, grp_off;
    DevBuf<int> grp_flags;
    bool grp_valid = false, grp_sorted = false;
    // mask folded into a bias vector for the MFMA scan (owned, rebuilt per call: the mask and bias are borrowed)
    DevBuf<float> mbias;
    // control block of the single-launch pipeline (owned): counters + exchange granules, zero between calls
    DevBuf<char> fctl;
    uint32_t fused_epoch = 0;
    // ... and of the single-launch BATCHED pipeline (hdb_mfma_kernel.h, MODE 2): counters, threshold words, sample granules
    DevBuf<char> bctl;
    // device copy of the result record of hdb_topk_host (owned)
    DevBuf<char> rec;
    // ... and of stage one of hdb_two_stage_host (owned): its ids feed the rerank, which may use `rec` of the same handle
    DevBuf<char> rec1;
    // int8 shadow of the matrix (owned, hdb_index_quantize; hdb_quant.hip): codes [rows][qP], caches [rows][3]
    int qmode = HDB_QUANT_NONE;
    DevBuf<int8_t> qcodes;
    DevBuf<float> qaux;
    int64_t q_rows = 0;               // capacity in rows of the shadow AND its plane: five arrays of different pitch share it
    int32_t qP = 0;                   // code pitch: d rounded up to 16 bytes
    DevBuf<int> qstat;                // device words (HDB_QSTAT_WORDS): [0] largest candidate count of the last quantized call,
                                      // [1] survivors of its pass over the 5-bit plane, [2] calls with more survivors than plane_cap_rows
    // the 5-bit plane beside the shadow (hdb_quant.hip): nibbles [rows][pU][16], bits [rows][pU], records [rows][4]; q_rows rows each
    DevBuf<uint8_t> pnib;
    DevBuf<uint32_t> pbit;
    DevBuf<float> prec;
    int32_t pU = 0;                   // 32-element units per row
    bool plane_declined = false;      // no memory for it (the shadow alone serves): stands until hdb_index_update / hdb_index_quantize
    bool qauto = false;               // the shadow was built by the index itself (auto_quant): its calls return the matrix cores' bits
    bool qauto_declined = false;      // ... or could not be (memory): the decision stands until the matrix changes
    // scratch (owned)
    DevBuf<char> ws;
    hdb_options opt;                  // hdb_set_option (hdb_plan.h)
    int flags_host = -1;              // host copy of *nan_flag (HDB_FLAG_*, hdb_caps.h: 1 = a NaN row, 2 = a row with an infinite sum of squares, 4 = a row that may hold an element beyond half of fp16 range); -1 = not fetched since the last build
    // stats of the last hdb_topk call: the plan's (topk_impl), and whether hdb_topk_host wrote the caller's record directly
    TopkStats st;
    int64_t st_host_direct = 0;
    const uint32_t* qb_cnt = nullptr; // a batch through the shadow: the list counters of its last chunk (in the workspace) and their number
    int qb_cnt_n = 0;
    // host-side timing of hdb_topk_host (always on: four clock reads per call), cumulative since "host_timing_reset":
    // entry -> launch, the launch call itself, launch -> record complete (poll / stream wait), calls
    int64_t ht_pre_ns = 0, ht_launch_ns = 0, ht_wait_ns = 0, ht_calls = 0;
    std::chrono::steady_clock::time_point ht_l0, ht_l1;     // around the launch of the single-launch pipelines (topk_impl)
    int64_t ht_attr_ns = 0;            // ... of which hipSetDevice + hipPointerGetAttributes (is the caller's record pinned?)
    // optional HIP-event timing of the dominant kernel (the pass over all of V)
    int64_t profile = 0;
    std::vector<hipEvent_t> ev_pool;      // pairs: [2i] start, [2i+1] stop
    size_t ev_used = 0;
};

static int ensure_ws(hdb_index* ix, size_t bytes) {
    if (bytes <= ix->ws.cap) return HDB_OK;
    HIP_TRY(ix->ws.alloc(align_up(bytes + (bytes >> 2), 1 << 20)));      // (free first: a failure leaves no workspace, capacity 0)
    return HDB_OK;
}
// Lay a workspace out (hdb_ws.h): a dry run of the layout gives the size, the second run places the pointers.
template <typename WS, typename... Ext>
static int ws_lay(hdb_index* ix, WS& w, Ext... ext) {
    const int rc = ensure_ws(ix, ws_bytes_for<WS>(ext...));
    if (rc) return rc;
    Bump b(ix->ws, ix->ws.cap);
    w.lay(b, ext...);
    if (b.off > b.cap) return fail(HDB_ERR_NOMEM, "workspace: a layout ran past the size it reported");
    return HDB_OK;
}

extern "C" int hdb_version(void) { return 112; }
extern "C" const char* hdb_last_error(void) { return g_err.c_str(); }

// The three arrays of a packed record (hdb_packed_bytes is its size): [nq][k] ids, [nq][k] scores, [nq] status words
struct PackedRec { int64_t* idx; float* score; int32_t* status; };
static PackedRec packed_view(const void* base, int32_t nq, int32_t k) {
    char* b = static_cast<char*>(const_cast<void*>(base));
    return {reinterpret_cast<int64_t*>(b), reinterpret_cast<float*>(b + (size_t)nq * k * 8), reinterpret_cast<int32_t*>(b + (size_t)nq * k * 12)};
}
// a device record of at least `bytes` (hdb_packed_bytes), grown by doubling
static int ensure_record(DevBuf<char>& rec, size_t bytes) {
    if (bytes <= rec.cap) return HDB_OK;
    HIP_TRY(rec.alloc(bytes * 2));
    return HDB_OK;
}
// The record of a *_host call.  open: the device record in `buf` (rec or rec1 of an index), grown as needed, and `view`, the three
// arrays the kernels write; direct (hdb_topk_host alone asks): the caller's record is pinned, device-visible memory and the kernels
// write it themselves -- no device record, no copy.  close: the copy to the caller unless direct, then (wait) the stream's completion.
struct HostRec { void* host_record; char* dev; size_t bytes; bool direct; PackedRec view; };
static int hostrec_open(DevBuf<char>& buf, int32_t nq, int32_t k, void* host_record, bool direct, HostRec& r) {
    r.host_record = host_record; r.dev = static_cast<char*>(host_record); r.bytes = (size_t)hdb_packed_bytes(nq, k); r.direct = direct;
    if (!direct) {
        const int rc = ensure_record(buf, r.bytes); if (rc) return rc;
        r.dev = buf;
    }
    r.view = packed_view(r.dev, nq, k);
    return HDB_OK;
}
static int hostrec_close(const HostRec& r, hipStream_t st, bool wait = true) {
    if (!r.direct) HIP_TRY(hipMemcpyAsync(r.host_record, r.dev, r.bytes, hipMemcpyDeviceToHost, st));
    if (wait) HIP_TRY(hipStreamSynchronize(st));
    return HDB_OK;
}

// What a change of the matrix invalidates, stated once (create, update, extend, gather).  kept_rows: the rows that are the old
// matrix's still -- 0, or the old n of an append, where the next hamming / pearson call packs the appended rows only.
static void matrix_changed(hdb_index* ix, int64_t kept_rows, hipStream_t st) {
    ix->flags_host = -1;
    ix->bits_valid = false; ix->bits_done = std::min(ix->bits_done, kept_rows);
    ix->pscale_valid = false; ix->pscale_done = std::min(ix->pscale_done, kept_rows);
    ix->bias = nullptr; ix->mask = nullptr;            // per-row inputs of the old matrix no longer apply
    ix->rows = nullptr; ix->subset_m = 0;
    ix->groups = nullptr; ix->n_groups = 0; ix->grp_valid = false;
    ix->build_stream = st;
}
// New blocks for the per-row caches.  The two change together: they are built beside the index and swapped in (caches_commit) after
// the last step that can fail; the old blocks go when the CacheBufs does.
struct CacheBufs { DevBuf<float> inv, sq; };
static int caches_alloc(int64_t rows, CacheBufs& c) {
    HIP_TRY(c.inv.alloc((size_t)rows));
    HIP_TRY(c.sq.alloc((size_t)rows));
    return HDB_OK;
}
static void caches_commit(hdb_index* ix, CacheBufs& c) {
    if (!c.inv) return;                                // (the index had the room)
    ix->inv_norm.swap(c.inv); ix->sqnorm.swap(c.sq);
}

// ---- int8 shadow (hdb_quant.hip) --------------------------------------------------------------
// gamma_{d+8} of the float32 VALU scan (hdb_quant.hip, bound (2)), with a relative margin for its own evaluation
static double quant_gamma(int d) {
    const double u = std::ldexp(1.0, -24), m = (double)(d + 8) * u;
    return m / (1.0 - m) * (1.0 + std::ldexp(1.0, -20));
}
// gamma_m of the matrix-core sum (hdb_quant.hip, bound (2m)); the per-row cache E_r takes the larger of the two
static double quant_gamma_m(int d) { return (double)(d + 8) * std::ldexp(1.0, -22); }
static double quant_gamma_rows(int d) { return std::max(quant_gamma(d), quant_gamma_m(d)); }
// bytes of one stored row (hdb_row_bytes, hdb_common.h: the one source of every row pitch)
static size_t row_pitch(const hdb_index* ix) { return (size_t)hdb_row_bytes(ix->dtype, ix->d); }
// bytes of one query: float64 against a float64 matrix, float32 against every other storage
static size_t query_pitch(const hdb_index* ix) { return (size_t)ix->d * (ix->dtype == HDB_F64 ? 8 : 4); }
#define HDB_QSTAT_WORDS 4
// the device words of hdb_index::qstat, zeroed on `st`; qstat stays null when the allocation itself fails
static hipError_t qstat_alloc(hdb_index* ix, hipStream_t st) {
    if (ix->qstat) return hipSuccess;
    const hipError_t e = ix->qstat.alloc(HDB_QSTAT_WORDS);
    return e != hipSuccess ? e : hipMemsetAsync(ix->qstat, 0, HDB_QSTAT_WORDS * sizeof(int), st);
}
static void plane_free(hdb_index* ix) { ix->pnib.reset(); ix->pbit.reset(); ix->prec.reset(); }
static void quant_free(hdb_index* ix) {
    ix->qcodes.reset(); ix->qaux.reset(); ix->q_rows = 0;
    plane_free(ix);
}
// bytes of the 5-bit plane per row: 20 per 32-element unit and 16 of row terms (plane_possible, hdb_plan.h: rows of up to 512 elements).
// The row terms are laid out per 16-row tile (hdb_plane_rec_bytes, hdb_caps.h), so their array is rounded up to a whole tile: up to 240
// bytes more than rows x this figure, which the memory guards below and the stat plane_bytes leave out (the guards keep 1 GiB free).
static size_t plane_row_bytes(int P) { return (size_t)hdb_quant_plane_units(P) * 20 + 16; }
// the plane's three arrays for `rows` rows: all of them, or none and the index as it was
static bool plane_alloc(hdb_index* ix, int64_t rows) {
    const size_t U = (size_t)hdb_quant_plane_units(ix->qP);
    DevBuf<uint8_t> nib; DevBuf<uint32_t> bit; DevBuf<float> rec;
    // (the records are laid out per 16-row tile, hdb_caps.h: whole tiles)
    if (nib.alloc((size_t)rows * U * 16) != hipSuccess || bit.alloc((size_t)rows * U) != hipSuccess ||
        rec.alloc((size_t)hdb_plane_rec_bytes(rows) / sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    ix->pnib.swap(nib); ix->pbit.swap(bit); ix->prec.swap(rec);
    return true;
}
// Derive the plane of rows [row0, row0 + m) from their codes; called wherever the shadow's rows are written.  The plane's arrays
// have the shadow's capacity (q_rows >= n rows; pass 1 loads the rows below n only); a reallocated shadow has dropped
// them (quant_commit), and every row is derived again.  No memory: the index goes on without a plane.
// A tile's hot blocks hold maxima over its rows (hdb_caps.h), so the plane is derived tile by tile: every tile that [row0, row0 + m)
// touches, from all of its rows below the row count -- ix->n, or row0 + m where an extend has not committed its rows yet -- with
// the neighbours' codes, caches and 1/||v|| as they stand.  inv_norm of the rows must be current: every caller fills it first, on
// the same stream (build_caches and extend: hdb_launch_rownorm; gather: hdb_launch_gather_rows, committed before the call).
static int plane_rows(hdb_index* ix, int64_t row0, int64_t m, hipStream_t st) {
    if (!plane_possible(ix->d) || ix->plane_declined) return HDB_OK;
    if (!ix->pnib && !plane_wanted(ix->d, ix->opt)) return HDB_OK;
    if (!ix->pnib) {
        // the automatic build's floor holds for every allocation of the plane (a shadow that grew on extend included): 1 GiB stays free
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); ix->plane_declined = true; return HDB_OK; }
        if (free_b < (size_t)ix->q_rows * plane_row_bytes(ix->qP) + ((size_t)1 << 30)) { ix->plane_declined = true; return HDB_OK; }
        if (!plane_alloc(ix, ix->q_rows)) { ix->plane_declined = true; return HDB_OK; }
        ix->pU = hdb_quant_plane_units(ix->qP);
        m = row0 + m; row0 = 0;
    }
    if (m <= 0) return HDB_OK;
    const int64_t rows = std::max(ix->n, row0 + m);
    LAUNCH_TRY(hdb_launch_quant_plane_rows(ix->qcodes, ix->qaux, ix->inv_norm, row0 / 16, (row0 + m + 15) / 16, rows, ix->d, ix->qP, ix->pnib,
                                           ix->pbit, ix->prec, st));
    return HDB_OK;
}
// New blocks for the shadow's codes and caches.  The two change together: built beside the index and swapped in (quant_commit) after
// the last step that can fail; the old blocks go when the ShadowBufs does.
struct ShadowBufs { DevBuf<int8_t> codes; DevBuf<float> aux; int64_t rows = 0; };
static int quant_alloc(const hdb_index* ix, int64_t rows, ShadowBufs& s) {
    hipError_t e = s.codes.alloc((size_t)rows * ix->qP);
    if (e == hipSuccess) e = s.aux.alloc((size_t)rows * 3);
    if (e != hipSuccess) return fail(HDB_ERR_NOMEM, std::string("the int8 shadow: ") + hipGetErrorString(e));
    s.rows = rows;
    return HDB_OK;
}
// ... for `need` rows where the shadow lacks the room (s stays empty where it has it)
static int quant_room(const hdb_index* ix, int64_t need, bool tight, ShadowBufs& s) {
    if (need <= ix->q_rows && ix->qcodes) return HDB_OK;
    return quant_alloc(ix, tight ? need + 64 : need + need / 2 + 64, s);      // (tight: the automatic build -- no room for appends until one comes)
}
static void quant_commit(hdb_index* ix, ShadowBufs& s) {
    if (!s.rows) return;
    ix->qcodes.swap(s.codes); ix->qaux.swap(s.aux); ix->q_rows = s.rows;
    plane_free(ix);                                    // the plane has the shadow's capacity: plane_rows derives all of it again
}
// room for `need` rows; the first `keep` rows of codes and caches survive a reallocation
static int quant_reserve(hdb_index* ix, int64_t need, int64_t keep, hipStream_t st, bool tight = false) {
    ShadowBufs s;
    const int rc = quant_room(ix, need, tight, s);
    if (rc || !s.rows) return rc;
    if (keep > 0 && ix->qcodes) {
        HIP_TRY(hipMemcpyAsync(s.codes, ix->qcodes, (size_t)keep * ix->qP, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(s.aux, ix->qaux, (size_t)keep * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    quant_commit(ix, s);
    return HDB_OK;
}
// quantize rows [row0, row0 + m) of the current matrix into the shadow, and derive their part of the plane
static int quant_rows(hdb_index* ix, int64_t row0, int64_t m, hipStream_t st) {
    if (m <= 0) return HDB_OK;
    const char* src = (const char*)ix->V + (size_t)row0 * row_pitch(ix);
    LAUNCH_TRY(hdb_launch_quant_rows(src, m, ix->d, ix->dtype, ix->qP, ix->qcodes + (size_t)row0 * ix->qP, ix->qaux + (size_t)row0 * 3,
                                     ix->nan_flag, quant_gamma_rows(ix->d), st));
    return plane_rows(ix, row0, m, st);
}

extern "C" int hdb_index_quantize(hdb_index* ix, int mode, void* stream) {
    if (!ix) return fail(HDB_ERR_ARG, "hdb_index_quantize: null index");
    if (mode != HDB_QUANT_NONE && mode != HDB_QUANT_I8) return fail(HDB_ERR_ARG, "hdb_index_quantize: mode must be HDB_QUANT_NONE or HDB_QUANT_I8");
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    if (mode == HDB_QUANT_NONE) {
        if (ix->qcodes) HIP_TRY(hipStreamSynchronize(st));
        quant_free(ix);
        ix->qmode = HDB_QUANT_NONE;
        ix->qauto = false;
        ix->opt.auto_quant = 0;                            // dropped on request: the index does not build one for itself again
        return HDB_OK;
    }
    // (bfloat16: on request only, option bf16_quant -- an explicit shadow with the VALU scan's bits, never an automatic one)
    if (ix->dtype == HDB_BF16 && !ix->opt.bf16_quant) return fail(HDB_ERR_UNSUPPORTED, "hdb_index_quantize: bfloat16 (bf16) matrices have no int8 shadow");
    if (ix->dtype == HDB_F8E4M3) return fail(HDB_ERR_UNSUPPORTED, "hdb_index_quantize: float8 (e4m3) matrices have no int8 shadow: one byte per element already");
    if (ix->dtype == HDB_I8) return fail(HDB_ERR_UNSUPPORTED, "hdb_index_quantize: int8 matrices have no int8 shadow: one byte per element already");
    if (ix->dtype == HDB_B1) return fail(HDB_ERR_UNSUPPORTED, "hdb_index_quantize: packed-bit matrices have no int8 shadow: one bit per element already");
    if (ix->dtype != HDB_F16 && ix->dtype != HDB_F32 && ix->dtype != HDB_BF16) return fail(HDB_ERR_UNSUPPORTED, "hdb_index_quantize: only float16 / float32 matrices have an int8 shadow");
    HIP_TRY(qstat_alloc(ix, st));
    ix->qP = (int32_t)align_up((size_t)ix->d, 16);
    ix->plane_declined = false;
    int rc = quant_reserve(ix, std::max<int64_t>(ix->n, 1), 0, st);
    if (rc) return rc;
    rc = quant_rows(ix, 0, ix->n, st);
    if (rc) return rc;
    ix->qmode = HDB_QUANT_I8;
    ix->qauto = false;                                 // an explicit shadow: the VALU scan's bits
    ix->build_stream = st;
    return HDB_OK;
}

// The automatic shadow (auto_quant): built on the first eligible call.  Memory guard: the shadow, n x (P + 12) bytes, must fit
// the device's free memory beside the workspace the call is about to take and a floor of 1 GiB for everybody else (the caller's
// own allocations, other indexes); a refusal or a failed allocation is remembered -- no error, no retry on every call.
// The 5-bit plane is under the same guard: where the shadow fits and the plane beside it does not, the shadow is built alone.
static bool quant_auto_build(hdb_index* ix, size_t ws_need, hipStream_t st) {
    if (ix->qauto_declined) return false;
    const int32_t P = (int32_t)align_up((size_t)ix->d, 16);
    const size_t shadow = (size_t)(ix->n + 64) * ((size_t)P + 12);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); ix->qauto_declined = true; return false; }
    const size_t ws_grow = ws_need > ix->ws.cap ? ws_need + (ws_need >> 2) + ((size_t)1 << 20) : 0;
    if (free_b < shadow + ws_grow + ((size_t)1 << 30)) { ix->qauto_declined = true; return false; }
    const size_t plane = plane_possible(ix->d) ? (size_t)(ix->n + 64) * plane_row_bytes(P) : 0;
    ix->plane_declined = plane_wanted(ix->d, ix->opt) && free_b < shadow + plane + ws_grow + ((size_t)1 << 30);
    // (no memory for the words: declined; a failed memset is not this function's to report, the launches behind it do)
    if (qstat_alloc(ix, st) != hipSuccess && !ix->qstat) { (void)hipGetLastError(); ix->qauto_declined = true; return false; }
    ix->qP = P;
    if (quant_reserve(ix, std::max<int64_t>(ix->n, 1), 0, st, true) != HDB_OK || quant_rows(ix, 0, ix->n, st) != HDB_OK) {
        (void)hipGetLastError();
        quant_free(ix);
        ix->qauto_declined = true;
        return false;
    }
    ix->qmode = HDB_QUANT_I8;
    ix->qauto = true;
    return true;
}

// A new matrix (create, update): allocate first, then commit V, n and the buffers together, then fill the caches and the shadow.
// An allocation that fails leaves the index on its old matrix, with its old buffers.
static int build_caches(hdb_index* ix, const void* V, int64_t n, hipStream_t st) {
    CacheBufs c; ShadowBufs s;
    int rc = n > (int64_t)ix->inv_norm.cap ? caches_alloc(n + n / 4 + 64, c) : HDB_OK;
    if (rc == HDB_OK && ix->qmode == HDB_QUANT_I8) rc = quant_room(ix, std::max<int64_t>(n, 1), false, s);      // the whole shadow is rebuilt
    if (rc) return rc;
    ix->V = V; ix->n = n;
    caches_commit(ix, c); quant_commit(ix, s);
    matrix_changed(ix, 0, st);                         // nothing of the lazy caches survives
    HIP_TRY(hipMemsetAsync(ix->nan_flag, 0, sizeof(int), st));
    if (n > 0) LAUNCH_TRY(hdb_launch_rownorm(V, n, ix->d, ix->dtype, ix->inv_norm, ix->sqnorm, ix->nan_flag, st));
    return ix->qmode == HDB_QUANT_I8 ? quant_rows(ix, 0, n, st) : HDB_OK;
}

extern "C" int hdb_index_create(hdb_index** out, const void* dev_V, int64_t n, int32_t d, int dtype, int device,
                                int64_t row_base, void* stream) {
    if (!out) return fail(HDB_ERR_ARG, "hdb_index_create: out is null");
    if (n < 0 || d <= 0) return fail(HDB_ERR_ARG, "hdb_index_create: need n >= 0 and d > 0");
    if (n > 0 && !dev_V) return fail(HDB_ERR_ARG, "hdb_index_create: matrix pointer is null");
    if (dtype != HDB_F16 && dtype != HDB_F32 && dtype != HDB_F64 && dtype != HDB_BF16 && dtype != HDB_F8E4M3 && dtype != HDB_I8 && dtype != HDB_B1) return fail(HDB_ERR_ARG, "hdb_index_create: dtype must be f16/f32/f64/bf16/f8e4m3/i8/b1");
    if (dtype == HDB_B1 && d % 32 != 0) return fail(HDB_ERR_ARG, "hdb_index_create: a packed-bit matrix needs d (bits per row) to be a multiple of 32");
    if (n >= ((int64_t)1 << 32) - 1) return fail(HDB_ERR_ARG, "hdb_index_create: at most 2^32-2 rows per shard");
    if ((int64_t)d * 8 > 60 * 1024) return fail(HDB_ERR_ARG, "hdb_index_create: d too large for the query LDS tile");
    if (dtype == HDB_B1 && n > 0 && (reinterpret_cast<uintptr_t>(dev_V) & 3) != 0) return fail(HDB_ERR_ARG, "hdb_index_create: a packed-bit matrix must be 4-byte aligned");
    HIP_TRY(hipSetDevice(device));
    hdb_index* ix = new hdb_index();
    ix->d = d; ix->dtype = dtype; ix->device = device; ix->row_base = row_base;
    const hipError_t e = ix->nan_flag.alloc(1);
    int rc = e == hipSuccess ? build_caches(ix, dev_V, n, (hipStream_t)stream) : fail(HDB_ERR_HIP, std::string("hdb_index_create: ") + hipGetErrorString(e));
    if (rc != HDB_OK) { hdb_index_destroy(ix); return rc; }
    *out = ix;
    return HDB_OK;
}

extern "C" int hdb_index_update(hdb_index* ix, const void* dev_V, int64_t n, void* stream) {
    if (!ix) return fail(HDB_ERR_ARG, "hdb_index_update: null index");
    if (n < 0 || (n > 0 && !dev_V)) return fail(HDB_ERR_ARG, "hdb_index_update: bad matrix");
    if (n >= ((int64_t)1 << 32) - 1) return fail(HDB_ERR_ARG, "hdb_index_update: at most 2^32-2 rows per shard");
    HIP_TRY(hipSetDevice(ix->device));
    // a new matrix: the memory question is asked again.  Only this call resets the two flags -- an append or a compaction changes
    // no answer (matrix_changed leaves them alone)
    ix->qauto_declined = false;
    ix->plane_declined = false;
    return build_caches(ix, dev_V, n, (hipStream_t)stream);
}

extern "C" int hdb_index_rebase(hdb_index* ix, const void* dev_V) {
    if (!ix) return fail(HDB_ERR_ARG, "hdb_index_rebase: null index");
    if (ix->n > 0 && !dev_V) return fail(HDB_ERR_ARG, "hdb_index_rebase: matrix pointer is null");
    ix->V = dev_V;
    return HDB_OK;
}

extern "C" int hdb_index_set_row_base(hdb_index* ix, int64_t row_base) {
    if (!ix) return fail(HDB_ERR_ARG, "hdb_index_set_row_base: null index");
    if (row_base < 0) return fail(HDB_ERR_ARG, "hdb_index_set_row_base: row_base must be >= 0");
    ix->row_base = row_base;
    return HDB_OK;
}

extern "C" int hdb_index_extend(hdb_index* ix, int64_t new_n, void* stream) {
    if (!ix) return fail(HDB_ERR_ARG, "hdb_index_extend: null index");
    if (new_n < ix->n) return fail(HDB_ERR_ARG, "hdb_index_extend: new_n must not shrink the matrix (use hdb_index_update)");
    if (new_n >= ((int64_t)1 << 32) - 1) return fail(HDB_ERR_ARG, "hdb_index_extend: at most 2^32-2 rows per shard");
    if (new_n == ix->n) return HDB_OK;
    if (!ix->V) return fail(HDB_ERR_ARG, "hdb_index_extend: no matrix registered");
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    const int64_t old_n = ix->n;
    // Room first, for the caches and for the shadow, each keeping its first old_n rows: until n is committed below, a step that
    // fails leaves the index on its old n rows, whose values every buffer still holds.
    if (new_n > (int64_t)ix->inv_norm.cap) {
        CacheBufs c;
        const int rc = caches_alloc(new_n + new_n / 2 + 64, c);
        if (rc) return rc;
        if (old_n > 0) {
            HIP_TRY(hipMemcpyAsync(c.inv, ix->inv_norm, old_n * sizeof(float), hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipMemcpyAsync(c.sq, ix->sqnorm, old_n * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
        caches_commit(ix, c);
    }
    if (ix->qmode == HDB_QUANT_I8) {
        const int rc = quant_reserve(ix, new_n, old_n, st);
        if (rc) return rc;
    }
    const char* tail = (const char*)ix->V + (size_t)old_n * row_pitch(ix);
    LAUNCH_TRY(hdb_launch_rownorm(tail, new_n - old_n, ix->d, ix->dtype, ix->inv_norm + old_n, ix->sqnorm + old_n, ix->nan_flag, st));
    if (ix->qmode == HDB_QUANT_I8) {                   // the shadow: the appended rows only
        const int rc = quant_rows(ix, old_n, new_n - old_n, st);
        if (rc) return rc;
    }
    ix->n = new_n;
    matrix_changed(ix, old_n, st);                     // (the next hamming / pearson call packs the appended rows only)
    return HDB_OK;
}

extern "C" int hdb_index_gather(hdb_index* ix, const int64_t* dev_rows, int64_t m, void* dev_V_out, void* stream) {
    if (!ix) return fail(HDB_ERR_ARG, "hdb_index_gather: null index");
    if (m < 0 || m > ix->n) return fail(HDB_ERR_ARG, "hdb_index_gather: m must be in [0, n]");
    if (m > 0 && (!dev_rows || !dev_V_out)) return fail(HDB_ERR_ARG, "hdb_index_gather: null argument");
    if (m > 0 && dev_V_out == ix->V) return fail(HDB_ERR_ARG, "hdb_index_gather: the gather is out of place");
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    const bool shadow = ix->qmode == HDB_QUANT_I8;     // the shadow travels with its rows too
    // new blocks always (the gather is out of place); the index keeps the old ones until the gathered ones are complete
    CacheBufs c; ShadowBufs s;
    const int64_t rows = m + m / 4 + 64;
    int rc = caches_alloc(rows, c);
    if (rc == HDB_OK && shadow) rc = quant_alloc(ix, rows, s);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(ix->nan_flag, 0, sizeof(int), st));
    LAUNCH_TRY(hdb_launch_gather_rows(ix->V, dev_rows, m, (int)row_pitch(ix), dev_V_out, ix->inv_norm, ix->sqnorm, c.inv, c.sq, ix->nan_flag, st));
    if (shadow) LAUNCH_TRY(hdb_launch_quant_gather(ix->qcodes, ix->qaux, dev_rows, m, ix->qP, s.codes, s.aux, st));
    HIP_TRY(hipStreamSynchronize(st));                 // the caller's old matrix is free after this
    ix->V = dev_V_out; ix->n = m;
    caches_commit(ix, c); quant_commit(ix, s);
    matrix_changed(ix, 0, st);
    return shadow ? plane_rows(ix, 0, m, st) : HDB_OK; // the plane is derived again from the gathered codes
}

extern "C" void hdb_index_destroy(hdb_index* ix) {
    if (!ix) return;
    (void)hipSetDevice(ix->device);
    (void)hipDeviceSynchronize();
    for (hipEvent_t e : ix->ev_pool) (void)hipEventDestroy(e);
    delete ix;                                         // every DevBuf frees its block
}

extern "C" int hdb_index_has_nan(hdb_index* ix, int* out_flag) {
    if (!ix || !out_flag) return fail(HDB_ERR_ARG, "hdb_index_has_nan: null argument");
    HIP_TRY(hipSetDevice(ix->device));
    int h = 0;
    HIP_TRY(hipMemcpyAsync(&h, ix->nan_flag, sizeof(int), hipMemcpyDeviceToHost, ix->build_stream));
    HIP_TRY(hipStreamSynchronize(ix->build_stream));
    ix->flags_host = h;
    *out_flag = h & 1;
    return HDB_OK;
}
// Are all rows of the matrix finite with a finite sum of squares?  One 4-byte copy after each build, cached.
static int matrix_is_finite(hdb_index* ix, bool* out) {
    if (ix->flags_host < 0) { int f = 0; int rc = hdb_index_has_nan(ix, &f); if (rc != HDB_OK) return rc; }
    *out = (ix->flags_host & (HDB_FLAG_NAN | HDB_FLAG_INF)) == 0;
    return HDB_OK;
}
// May a manhattan pass over this fp16 matrix take its differences in packed fp16 (hdb_l1_packed_ok, hdb_caps.h)?  The same cached word.
static int matrix_l1_packed_ok(hdb_index* ix, bool* out) {
    *out = false;
    if (ix->dtype != HDB_F16 || !ix->opt.l1_packed) return HDB_OK;      // (nothing to ask)
    if (ix->flags_host < 0) { int f = 0; int rc = hdb_index_has_nan(ix, &f); if (rc != HDB_OK) return rc; }
    *out = hdb_l1_packed_ok(ix->dtype, ix->opt.l1_packed, ix->flags_host);
    return HDB_OK;
}

extern "C" int hdb_index_set_bias(hdb_index* ix, const float* dev_bias) {
    if (!ix) return fail(HDB_ERR_ARG, "hdb_index_set_bias: null index");
    ix->bias = dev_bias;
    return HDB_OK;
}

extern "C" int hdb_index_set_row_mask(hdb_index* ix, const uint8_t* dev_mask) {
    if (!ix) return fail(HDB_ERR_ARG, "hdb_index_set_row_mask: null index");
    ix->mask = dev_mask;
    ix->rows = nullptr; ix->subset_m = 0;               // a stale list never sits beside a new mask
    return HDB_OK;
}

extern "C" int hdb_index_set_row_subset(hdb_index* ix, const uint8_t* dev_mask, const int64_t* dev_rows, int64_t m) {
    if (!ix) return fail(HDB_ERR_ARG, "hdb_index_set_row_subset: null index");
    if (dev_rows && !dev_mask) return fail(HDB_ERR_ARG, "hdb_index_set_row_subset: a row list needs its mask");
    if (dev_rows && (m < 1 || m > ix->n)) return fail(HDB_ERR_ARG, "hdb_index_set_row_subset: m must be in [1, n]");
    ix->mask = dev_mask;
    ix->rows = dev_rows; ix->subset_m = dev_rows ? m : 0;
    return HDB_OK;
}

extern "C" int hdb_index_set_groups(hdb_index* ix, const int32_t* dev_groups, int64_t n_groups) {
    if (!ix) return fail(HDB_ERR_ARG, "hdb_index_set_groups: null index");
    if (dev_groups && (n_groups < 1 || n_groups > 0x7FFFFFFFll)) return fail(HDB_ERR_ARG, "hdb_index_set_groups: n_groups must be in [1, 2^31 - 1]");
    ix->groups = dev_groups; ix->n_groups = dev_groups ? n_groups : 0;
    ix->grp_valid = false;                              // (the inverted index of the old ids: built again by the next multi-vector call)
    return HDB_OK;
}

extern "C" int hdb_set_option(hdb_index* ix, const char* name, int64_t value) {
    if (!ix || !name) return fail(HDB_ERR_ARG, "hdb_set_option: null argument");
    // (the two names that are no member of hdb_options; every other name and its rule: HDB_OPTIONS, hdb_plan.h)
    if (!strcmp(name, "profile")) { ix->profile = value; ix->ev_used = 0; }
    else if (!strcmp(name, "host_timing_reset")) { ix->ht_pre_ns = ix->ht_launch_ns = ix->ht_wait_ns = ix->ht_calls = ix->ht_attr_ns = 0; }
    else if (!hdb_option_set(ix->opt, name, value)) return fail(HDB_ERR_ARG, std::string("hdb_set_option: unknown option ") + name);
    return HDB_OK;
}

// the statistics that live in device words: wait for the device, then copy `bytes` of them to the host
static int read_device_stat(hdb_index* ix, void* dst, const void* src, size_t bytes) {
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return HDB_OK;
}

extern "C" int hdb_get_stat(hdb_index* ix, const char* name, int64_t* value) {
    if (!ix || !name || !value) return fail(HDB_ERR_ARG, "hdb_get_stat: null argument");
    // the statistics of the last call (TopkStats) by their names: HDB_STATS, hdb_plan.h; below, what is computed or the index's own
    for (const hdb_stat_entry& e : HDB_STATS) if (!strcmp(name, e.name)) { *value = ix->st.*e.member; return HDB_OK; }
    int rc = HDB_OK;
    if (!strcmp(name, "f8_lds_min_q")) *value = f8_lds_first_q(ix->opt, ix->dtype, ix->d);      // the threshold in force for this index, 0 = never
    else if (!strcmp(name, "b1_mfma_min_q")) *value = b1_mfma_first_q(ix->opt, ix->dtype, ix->d);      // likewise, for a packed-bit index
    else if (!strcmp(name, "host_direct")) *value = ix->st_host_direct;
    else if (!strcmp(name, "cand_cap")) *value = HDB_CAND_CAP;
    else if (!strcmp(name, "quant_auto")) *value = (ix->qmode == HDB_QUANT_I8 && ix->qauto) ? 1 : 0;
    else if (!strcmp(name, "quant_bytes")) *value = ix->qmode == HDB_QUANT_I8 ? ix->n * (int64_t)(ix->qP + 12) : 0;
    else if (!strcmp(name, "subset_rows")) *value = ix->subset_m;
    else if (!strcmp(name, "maxsim_bytes")) *value = (int64_t)((ix->grp_rows.cap + ix->grp_off.cap) * sizeof(uint32_t));      // the inverted index of the groups, as held
    else if (!strcmp(name, "plane_bytes")) *value = (ix->qmode == HDB_QUANT_I8 && ix->pnib) ? ix->n * (int64_t)plane_row_bytes(ix->qP) : 0;
    else if (!strcmp(name, "plane_survivors") || !strcmp(name, "plane_overflows")) {      // synchronise the device
        // plane_survivors: rows the last call's pass over the plane kept (0 when it did not take the plane); plane_overflows: calls
        // of this index so far that kept more than plane_cap_rows of them (the plane let more through than it is worth)
        int h[HDB_QSTAT_WORDS] = {0, 0, 0, 0};
        if (ix->qstat && (rc = read_device_stat(ix, h, ix->qstat, sizeof(h))) != HDB_OK) return rc;
        *value = name[6] == 's' ? (ix->st.plane ? (int64_t)(uint32_t)h[1] : 0) : (int64_t)(uint32_t)h[2];
    }
    else if (!strcmp(name, "quant_cands")) {          // synchronises the device
        int h = 0;
        if (ix->st.quant && ix->qstat && (rc = read_device_stat(ix, &h, ix->qstat, sizeof(int))) != HDB_OK) return rc;
        *value = h;
    }
    else if (!strcmp(name, "quant_cands_min") || !strcmp(name, "quant_cands_median")) {     // batches: over the lists of the last chunk; synchronises
        int64_t v = 0;
        if (ix->st.quant && ix->qb_cnt && ix->qb_cnt_n > 0) {
            std::vector<uint32_t> raw((size_t)ix->qb_cnt_n * HDB_CNT_STRIDE), c((size_t)ix->qb_cnt_n);
            if ((rc = read_device_stat(ix, raw.data(), ix->qb_cnt, raw.size() * sizeof(uint32_t))) != HDB_OK) return rc;
            for (int q = 0; q < ix->qb_cnt_n; ++q) c[q] = raw[(size_t)q * HDB_CNT_STRIDE];
            std::sort(c.begin(), c.end());
            v = name[13] == 'i' ? c.front() : c[c.size() / 2];
        }
        *value = v;
    }
    else if (!strcmp(name, "n")) *value = ix->n;
    else if (!strcmp(name, "ws_bytes")) *value = (int64_t)ix->ws.cap;
    else if (!strcmp(name, "scan_launches")) *value = (int64_t)(ix->ev_used / 2);
    else if (!strcmp(name, "host_pre_ns")) *value = ix->ht_pre_ns;
    else if (!strcmp(name, "host_launch_ns")) *value = ix->ht_launch_ns;
    else if (!strcmp(name, "host_wait_ns")) *value = ix->ht_wait_ns;
    else if (!strcmp(name, "host_calls")) *value = ix->ht_calls;
    else if (!strcmp(name, "host_attr_ns")) *value = ix->ht_attr_ns;
    else if (!strcmp(name, "scan_time_ns")) {      // sum over recorded launches; synchronises on the last event
        double total_ms = 0.0;
        for (size_t i = 0; i + 1 < ix->ev_used; i += 2) {
            if (hipEventSynchronize(ix->ev_pool[i + 1]) != hipSuccess) return fail(HDB_ERR_HIP, "hipEventSynchronize failed");
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ix->ev_pool[i], ix->ev_pool[i + 1]) != hipSuccess) return fail(HDB_ERR_HIP, "hipEventElapsedTime failed");
            total_ms += ms;
        }
        *value = (int64_t)(total_ms * 1.0e6);
    }
    else return fail(HDB_ERR_ARG, std::string("hdb_get_stat: unknown stat ") + name);
    return HDB_OK;
}

// Bracket one launch with HIP events on the launch stream (bench.py: roofline.achieved).
static void prof_begin(hdb_index* ix, hipStream_t st) {
    if (!ix->profile) return;
    if (ix->ev_used + 2 > ix->ev_pool.size()) {
        if (ix->ev_pool.size() >= 16384) return;     // bounded
        for (int i = 0; i < 2; ++i) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return; ix->ev_pool.push_back(e); }
    }
    (void)hipEventRecord(ix->ev_pool[ix->ev_used], st);
}
static void prof_end(hdb_index* ix, hipStream_t st) {
    if (!ix->profile || ix->ev_used + 2 > ix->ev_pool.size()) return;
    (void)hipEventRecord(ix->ev_pool[ix->ev_used + 1], st);
    ix->ev_used += 2;
}
// The bracket round the launch of a single-launch pipeline: the profile's events outside, the two clock reads of hdb_topk_host's
// timing tight round the launch call.  `launch` returns the launcher's code, handed on as it stands (a failed launch ends no event pair).
template <typename Launch>
static inline int single_launch(hdb_index* ix, hipStream_t st, Launch&& launch) {
    prof_begin(ix, st);
    ix->ht_l0 = std::chrono::steady_clock::now();
    const int e = launch();
    ix->ht_l1 = std::chrono::steady_clock::now();
    if (e == 0) prof_end(ix, st);
    return e;
}

static bool metric_ok(int metric) { return metric >= HDB_DOT && metric <= HDB_EUCLIDEAN_DIST; }

static int ensure_pscale(hdb_index* ix, hipStream_t st) {
    if (ix->pscale_valid) return HDB_OK;
    int64_t keep = ix->pscale ? std::min(ix->pscale_done, ix->n) : 0;          // rows whose scale is still good (appended matrix)
    if (ix->n > (int64_t)ix->pscale.cap) HIP_TRY(ix->pscale.grow_keep((size_t)(ix->n + ix->n / 4 + 64), (size_t)keep, st));
    if (ix->n > keep)
        LAUNCH_TRY(hdb_launch_rowstats((const char*)ix->V + (size_t)keep * row_pitch(ix), ix->n - keep, ix->d, ix->dtype, ix->pscale + keep, st));
    ix->pscale_done = ix->n;
    ix->pscale_valid = true;
    return HDB_OK;
}

static int ensure_bits(hdb_index* ix, hipStream_t st) {
    if (ix->bits_valid) return HDB_OK;
    const int W = (ix->d + 31) / 32;
    if (W > 512) return fail(HDB_ERR_UNSUPPORTED, "hamming: d > 16384 not supported");
    const int64_t npad = align_up((size_t)std::max<int64_t>(ix->n, 4), 256);      // whole 256-row blocks (hdb_bits_word)
    // rows packed before the matrix grew stay where they are: the layout is a sequence of 256-row blocks, so a bigger buffer takes
    // the old blocks as a prefix (hdb_index_extend / HyperDB.add: the next bit-metric call packs the appended rows only)
    int64_t keep = (ix->bits && ix->W == W) ? std::min(ix->bits_done, ix->n) : 0;
    if (!ix->bits || ix->bits_npad < npad || ix->W != W) {
        const int64_t cap = align_up((size_t)(npad + npad / 4), 256);
        DevBuf<uint32_t> b2;                               // zero-filled, then the kept blocks: swapped in when both are queued
        HIP_TRY(b2.alloc((size_t)cap * W));
        HIP_TRY(hipMemsetAsync(b2, 0, (size_t)cap * W * sizeof(uint32_t), st));
        if (keep > 0) HIP_TRY(hipMemcpyAsync(b2, ix->bits, (size_t)align_up((size_t)keep, 256) * W * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        ix->bits.swap(b2); ix->bits_npad = cap; ix->W = W;
    } else if (keep == 0) {
        HIP_TRY(hipMemsetAsync(ix->bits, 0, (size_t)ix->bits_npad * W * sizeof(uint32_t), st));
    }
    if (ix->n > keep)
        LAUNCH_TRY(hdb_launch_signpack((const char*)ix->V + (size_t)keep * row_pitch(ix), ix->n - keep, ix->d, ix->dtype, keep, ix->bits, st));
    ix->bits_done = ix->n;
    ix->bits_valid = true;
    return HDB_OK;
}

static void base_args(const hdb_index* ix, ScanArgs& a, const void* Q, int metric) {
    memset(&a, 0, sizeof(a));
    a.V = ix->V; a.n = ix->n; a.d = ix->d; a.Q = Q; a.metric = metric;
    a.inv_norm = ix->inv_norm; a.mask = ix->mask;
    a.tile_stride = 1; a.ntiles = (ix->n + 15) / 16;
    a.cap = HDB_CAND_CAP;
    a.dyn_min_bytes = ix->opt.dyn_min_mb << 20; a.dyn_heavy = (int32_t)ix->opt.dyn_heavy;
}

// One scan launch (VALU, hamming or MFMA flavour) for queries [a.q0, a.q0+cq).
struct QueryBufs { const float* qinv; const float* qsq; const uint32_t* qbits; const void* q16; const float* qscl; };
static int run_scan(hdb_index* ix, ScanArgs& a, int mode, int cq, const QueryBufs& qb, bool l1tile, bool mfma, hipStream_t st) {
    a.qinv = qb.qinv;
    if (is_bits_metric(a.metric)) {
        LAUNCH_TRY(hdb_launch_hamming(&a, mode, cq, ix->bits, ix->bits_npad, ix->W, qb.qbits, st));
    } else if (l1tile && cq >= 2 && a.tile_stride == 1) {
        // dense manhattan passes of a call the plan gave to the tile kernel (TopkPlan::l1tile; the mask is folded into the bias):
        // tiles staged once in LDS, queries in registers, 8-16 queries per pass (hdb_l1_tile.hip)
        // (the tile kernel has no use for ScanArgs::dyn_heavy: 77 there = "keep the float32 arithmetic", set_option l1_packed 0)
        // ... and also where an element of the matrix may lie beyond half of fp16 range: a packed difference could round to inf
        bool pk_ok = false;
        const int prc = matrix_l1_packed_ok(ix, &pk_ok); if (prc) return prc;
        ScanArgs al = a; al.dyn_heavy = pk_ok ? 0 : 77;
        LAUNCH_TRY(hdb_launch_l1_tile(&al, ix->dtype, mode, cq, (int)ix->opt.max_blocks, st));
    } else if (mfma) {
        LAUNCH_TRY(hdb_launch_mfma_scan(&a, ix->dtype, mode, cq, qb.q16, ix->sqnorm, qb.qsq, qb.qscl, (int)ix->opt.max_blocks, (int)ix->opt.mfma_variant, st, nullptr));
    } else {
        LAUNCH_TRY(hdb_launch_scan(&a, ix->dtype, mode, cq, (int)ix->opt.max_blocks, st));
    }
    return HDB_OK;
}

extern "C" int hdb_scores(hdb_index* ix, const void* dev_q, int metric, float* dev_out, void* stream) {
    if (!ix || !dev_q || !dev_out) return fail(HDB_ERR_ARG, "hdb_scores: null argument");
    if (!metric_ok(metric)) return fail(HDB_ERR_UNSUPPORTED, "hdb_scores: metric not built");
    if (ix->n == 0) return HDB_OK;
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    const int W = (ix->d + 31) / 32;
    ScoresWs w;
    int rc = ws_lay(ix, w, ix->d, W);
    if (rc) return rc;
    float* qinv = w.qinv; float* qsq = w.qsq; int* qnan = w.qnan; uint32_t* qbits = w.qbits; void* qc = w.qc;
    LAUNCH_TRY(hdb_launch_qprep(dev_q, 1, ix->d, ix->dtype == HDB_F64, qinv, qsq, qnan, nullptr, nullptr, st));
    if (is_bits_metric(metric)) {
        rc = ensure_bits(ix, st); if (rc) return rc;
        LAUNCH_TRY(hdb_launch_qsign(dev_q, 1, ix->d, ix->dtype == HDB_F64, W, qbits, st));
    }
    ScanArgs a; base_args(ix, a, dev_q, metric);
    if (metric == HDB_PEARSON) {        // cosine pipeline on the centred query with 1/(sd*d) row scales
        rc = ensure_pscale(ix, st); if (rc) return rc;
        LAUNCH_TRY(hdb_launch_qcentre(dev_q, 1, ix->d, ix->dtype == HDB_F64, qc, qinv, st));
        a.Q = qc; a.metric = HDB_COSINE; a.inv_norm = ix->pscale;
    }
    a.mask = nullptr;                   // per-metric functions score every row, no bias (reference :24-147)
    a.raw = 1;                          // ... and return NaN where the reference does (pearson, jaccard)
    a.scores = dev_out; a.ld = ix->n;
    QueryBufs qb{qinv, qsq, qbits, nullptr, nullptr};
    return run_scan(ix, a, 0, 1, qb, false, false, st);
}

// ---- hdb_topk: validate, plan (hdb_plan.h), execute -----------------------------------------------------------------------------
// The arguments of one call, as the executors take them, and the index as the planner sees it.
struct TopkArgs { const void* Q; int32_t nq, k; int metric; int64_t* idx; float* score; int32_t* status; hipStream_t st; };
static TopkFacts topk_facts(const hdb_index* ix) {
    return {ix->n, ix->d, ix->dtype, ix->qmode, ix->qauto, ix->qauto_declined, ix->pnib != nullptr, ix->plane_declined,
            ix->mask != nullptr, ix->bias != nullptr, hdb_cu_count(), ix->subset_m};
}

// The workspace of a 1-4-query shadow call (QuantWs, hdb_ws.h): the memory guard of the automatic build sizes with these extents,
// the call lays out with them.  The score buffer takes the extent of the largest sample any k takes (quant_ld_max) -- the call's own
// ld_s is only its leading dimension -- so calls that differ in k never regrow the workspace.  (P from d: the automatic build asks
// before the index has a pitch.)  pl_cap: entries of the list beside the score buffer (hdb_ws.h): quant_hi_cap from every caller.
static int quant_pitch(const hdb_index* ix) { return (int)align_up((size_t)ix->d, 16); }
// The list of the sampled rows' upper bounds (QuantArgs::pl_hi): one query, a width the plane takes; like the score buffer it has
// the extent of the largest sample any k takes.  The memory guard, the call and the test entry all size with it.
static uint32_t quant_hi_cap(const hdb_index* ix, int nq) {
    return nq == 1 && plane_possible((int)ix->d) ? (uint32_t)quant_ld_max(ix->n, ix->d) : 0u;
}
static size_t quant_ws_bytes(const hdb_index* ix, int nq, uint32_t pl_cap, bool mflavour) {
    return ws_bytes_for<QuantWs>(nq, quant_pitch(ix), (int)ix->d, quant_ld_max(ix->n, ix->d), pl_cap, mflavour);
}
static int quant_ws_lay(hdb_index* ix, QuantWs& w, int nq, uint32_t pl_cap, bool mflavour) {
    return ws_lay(ix, w, nq, quant_pitch(ix), (int)ix->d, quant_ld_max(ix->n, ix->d), pl_cap, mflavour);
}
// ... and of one chunk of a batch (QuantBatchWs)
static size_t quant_batch_ws_bytes(const hdb_index* ix, int cq) {
    return ws_bytes_for<QuantBatchWs>(cq, quant_pitch(ix), (int)ix->d, quant_batch_sample(ix->n).ld_s, quant_batch_wld());
}
static int quant_batch_ws_lay(hdb_index* ix, QuantBatchWs& w, int cq) {
    return ws_lay(ix, w, cq, quant_pitch(ix), (int)ix->d, quant_batch_sample(ix->n).ld_s, quant_batch_wld());
}
// The shadow's counterpart of base_args: the index's side and the prepared queries; every pass sets its own tiles, outputs and lists.
static void quant_base_args(const hdb_index* ix, QuantArgs& a, const int8_t* qcodes, const float* qaux, const float* qinv, int metric, int nq) {
    memset(&a, 0, sizeof(a));
    a.codes = ix->qcodes; a.n = ix->n; a.d = ix->d; a.P = ix->qP; a.aux = ix->qaux; a.sqnorm = ix->sqnorm; a.inv_norm = ix->inv_norm;
    a.qcodes = qcodes; a.qaux = qaux; a.qinv = qinv; a.bias = ix->bias; a.mask = ix->mask; a.metric = metric; a.nq = nq;
    a.gamma = (float)quant_gamma(ix->d);
}
// Query prep of a 1-4-query shadow call.  mflavour: one launch (1/||q||, the scaled fp16 copy, codes of the rounded query); otherwise
// 1/||q|| and the NaN flags exactly as every other path computes them (the cosine epilogue multiplies by this 1/||q||), then the codes.
static int quant_query_prep(hdb_index* ix, const float* Q, int nq, const QuantWs& w, bool mflavour, int* stat, uint32_t* cnt_init,
                            uint32_t* pl_cnt, hipStream_t st) {
    if (mflavour) {
        LAUNCH_TRY(hdb_launch_quant_qprep_m(Q, nq, ix->d, ix->qP, w.qinv, w.qsq, w.qnan, w.q16, w.qscl, w.qcodes, w.qaux, stat, cnt_init, pl_cnt, st));
    } else {
        LAUNCH_TRY(hdb_launch_qprep(Q, nq, ix->d, false, w.qinv, w.qsq, w.qnan, nullptr, nullptr, st));
        LAUNCH_TRY(hdb_launch_quant_qprep(Q, nq, ix->d, ix->qP, w.qcodes, w.qaux, stat, pl_cnt, st));
    }
    return HDB_OK;
}

// What a planned shadow path needs before it can run: the shadow itself (the automatic build, on the first eligible call) and
// the plane (a shadow that was built without one -- use_plane was off then -- gets it on the first call that asks for the path).
// Either may be declined for memory: the index remembers that, *declined is set and topk_impl plans once more on the new facts.
static int shadow_prepare(hdb_index* ix, const TopkPlan& p, int nq, hipStream_t st, bool* declined) {
    if (p.build_needed) {
        const size_t ws_need = p.path == HDB_PATH_QUANT ? quant_ws_bytes(ix, nq, quant_hi_cap(ix, nq), true) : quant_batch_ws_bytes(ix, p.cq_max);
        if (!quant_auto_build(ix, ws_need, st)) { *declined = true; return HDB_OK; }
    }
    if (p.plane_wanted && !ix->pnib) {
        const int rc = plane_rows(ix, 0, ix->n, st);
        if (rc) return rc;
        *declined = ix->pnib == nullptr;
    }
    return HDB_OK;
}

// 1-4 dot / cosine / euclidean queries through the int8 shadow (hdb_quant.hip): quantized query prep, lower bounds on a strided row
// sample, T_s = 16th largest of them, the pass over the shadow that keeps rows whose upper bound reaches T_s, exact rescoring of
// those from the matrix, finalize with the floor T_s.  The sample aims at ~512 rows of the whole matrix with a lower bound above
// T_s (the upper bounds let several times that many through; a sample of 16 keeps P(fewer than k = 128 such rows) near 1e-5).
// mflavour (the automatic shadow of an fp16 index): the scores are the matrix cores' -- one launch prepares the queries (1/||q||,
// the scaled fp16 copy, codes of the rounded query), the filter pass copies every candidate's row into a compact matrix as it emits
// it, the MODE 0 launch of the matrix-core scan scores that, the finalize packs those scores into the list before it selects.
// Launches: query prep, sample pass, filter pass, MODE 0, finalize -- five with the threshold folded into the passes (nsub), six
// with hdb_sample_thr_kernel; the explicit shadow has two query prep launches and hdb_quant_rescore_kernel in MODE 0's place.
static int quant_topk(hdb_index* ix, const TopkArgs& c, const TopkPlan& p) {
    const void* dev_Q = c.Q; const int32_t nq = c.nq, k = c.k; const int metric = c.metric; hipStream_t st = c.st;
    int64_t* dev_idx = c.idx; float* dev_score = c.score; int32_t* dev_status = c.status;      // (the call, under the names the body uses)
    const uint32_t kk = p.kk; const bool mflavour = p.mflavour, use_pl = p.plane_wanted;
    const int64_t n = ix->n;
    const uint32_t m = 16;
    const QuantSample sp = p.qs;
    QuantWs w;
    int rc = quant_ws_lay(ix, w, nq, quant_hi_cap(ix, nq), mflavour);
    if (rc) return rc;
    uint32_t* qstat = reinterpret_cast<uint32_t*>(ix->qstat.p);
    uint32_t* pl_cnt = use_pl ? qstat + 1 : nullptr;
    const size_t crow = (size_t)nq * HDB_CAND_CAP;
    const int nsub = p.nsub;
    rc = quant_query_prep(ix, (const float*)dev_Q, nq, w, mflavour, ix->qstat, nsub ? w.cnt : nullptr, pl_cnt, st);
    if (rc) return rc;
    QuantArgs a; quant_base_args(ix, a, w.qcodes, w.qaux, w.qinv, metric, nq);
    a.ntiles = sp.s_tiles; a.tile_stride = sp.s_stride; a.scores = w.sbuf; a.ld = sp.ld_s;
    a.wmax = w.wmax; a.nsub = nsub; a.thr_out = w.thr;
    a.pl_hi = use_pl ? reinterpret_cast<float*>(w.pl_list) : nullptr;      // the plane pass takes the sampled rows from this list
    if (use_pl && (!a.pl_hi || sp.s_rows > (int64_t)quant_hi_cap(ix, nq))) return fail(HDB_ERR_ARG, "quant_topk: no list for the sampled rows");
    LAUNCH_TRY(hdb_launch_quant_scan(&a, 0, (int)ix->opt.max_blocks, st));
    if (!nsub) LAUNCH_TRY(hdb_launch_sample_thr(w.sbuf, sp.s_rows, sp.ld_s, nq, m, w.thr, w.cnt, nullptr, st));
    a.ntiles = (n + 15) / 16; a.tile_stride = 1; a.scores = nullptr; a.ld = 0;
    a.thr = w.thr; a.cnt = w.cnt; a.cand = w.cand; a.cap = HDB_CAND_CAP;
    const bool has_bias = ix->bias != nullptr || ix->mask != nullptr;
    if (mflavour) {                                  // the filter pass fills the compact matrix as it emits
        a.V = (const char*)ix->V; a.row_bytes = ix->d * 2; a.G = w.G;
        a.ginv = metric == HDB_COSINE ? w.ginv : nullptr; a.gbias = has_bias ? w.gbias : nullptr;
    }
    prof_begin(ix, st);
    if (use_pl) {
        // one dot / cosine query: the pass over the 5-bit plane, which finishes the rows it keeps itself (hdb_quant.hip); it takes
        // the threshold the way MODE 1 would (folded or from thr) and leaves it in thr for the finalize.  It does not stream the
        // sample's tiles: their rows come from the list of upper bounds the sample pass left (pl_hi)
        a.pl_nib = ix->pnib; a.pl_bit = ix->pbit; a.pl_rec = ix->prec; a.pl_units = ix->pU;
        a.pl_cnt = pl_cnt; a.pl_cap = p.pl_cap;
        a.pl_s_tiles = (uint32_t)sp.s_tiles; a.pl_s_stride = (uint32_t)sp.s_stride;      // ... and walks the other tiles
        LAUNCH_TRY(hdb_launch_quant_plane_scan(&a, 0, p.pl_blocks, st));      // (the grid is the plan's: stat plane_blocks)
    } else {
        LAUNCH_TRY(hdb_launch_quant_scan(&a, 1, (int)ix->opt.max_blocks, st));
    }
    prof_end(ix, st);
    if (mflavour) {
        ScanArgs s; memset(&s, 0, sizeof(s));
        s.V = w.G; s.n = (int64_t)crow; s.d = ix->d; s.Q = dev_Q; s.metric = metric; s.inv_norm = w.ginv; s.qinv = w.qinv;
        s.bias = has_bias ? w.gbias : nullptr; s.mask = nullptr; s.nq = nq;
        s.tile_stride = 1; s.ntiles = (int64_t)crow / hdb_mfma_tile_rows(ix->dtype, ix->d); s.cap = HDB_CAND_CAP;
        s.scores = w.gsc; s.ld = (int64_t)crow;
        LAUNCH_TRY(hdb_launch_mfma_scan(&s, ix->dtype, 0, nq, w.q16, w.ginv, w.qsq, w.qscl, (int)ix->opt.max_blocks, (int)ix->opt.mfma_variant, st, nullptr));
    } else {
        LAUNCH_TRY(hdb_launch_quant_rescore(ix->V, ix->d, ix->dtype, (const float*)dev_Q, nq, metric, ix->inv_norm, w.qinv, ix->bias, ix->mask,
                                            w.cand, w.cnt, HDB_CAND_CAP, st));
    }
    LAUNCH_TRY(hdb_launch_quant_finalize(w.cand, w.cnt, HDB_CAND_CAP, nq, (uint32_t)k, kk, ix->row_base, dev_idx, dev_score, dev_status, w.qnan,
                                         w.qaux, w.thr, ix->qstat, mflavour ? w.cand : nullptr, w.gsc, (int64_t)crow, st));
    return HDB_OK;
}

// Test entry: the upper bound of every row for ONE float32 query, as the MODE 1 pass computes it (dev_hi[n]) and as pass 1 over the
// 5-bit plane computes it (dev_hi5[n]); masked rows give -inf in both.  The index needs a shadow with its plane.
extern "C" int hdb_debug_quant_bounds(hdb_index* ix, const float* dev_q, int metric, float* dev_hi, float* dev_hi5, void* stream) {
    if (!ix || !dev_q || !dev_hi || !dev_hi5) return fail(HDB_ERR_ARG, "hdb_debug_quant_bounds: null argument");
    if (metric != HDB_DOT && metric != HDB_COSINE) return fail(HDB_ERR_ARG, "hdb_debug_quant_bounds: dot or cosine");
    if (ix->qmode != HDB_QUANT_I8 || !ix->pnib || ix->n < 1) return fail(HDB_ERR_UNSUPPORTED, "hdb_debug_quant_bounds: the index has no 5-bit plane");
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    QuantWs w;
    int rc = quant_ws_lay(ix, w, 1, quant_hi_cap(ix, 1), true);
    if (rc) return rc;
    rc = quant_query_prep(ix, dev_q, 1, w, ix->qauto, nullptr, nullptr, nullptr, st);
    if (rc) return rc;
    QuantArgs a; quant_base_args(ix, a, w.qcodes, w.qaux, w.qinv, metric, 1);
    a.ntiles = (ix->n + 15) / 16; a.tile_stride = 1;
    a.pl_nib = ix->pnib; a.pl_bit = ix->pbit; a.pl_rec = ix->prec; a.pl_units = ix->pU;
    a.dbg = dev_hi;
    LAUNCH_TRY(hdb_launch_quant_scan_one(&a, 2, (int)ix->opt.max_blocks, st));
    a.dbg = dev_hi5;
    LAUNCH_TRY(hdb_launch_quant_plane_scan(&a, 1, hdb_quant_plane_dbg_blocks(a.ntiles, (int)ix->opt.max_blocks), st));
    return HDB_OK;
}

// ---- batches of 5+ queries through the automatic shadow (hdb_quant_mfma.hip) ---------------------------------------------------
// One call: chunks of up to 256 queries, each through query prep, sample pass, thresholds, filter pass, block-diagonal rescoring
// and finalize.  Workspace per chunk: the lists (cq x 8192 x 8 bytes = 16 MiB at 256 queries), the slot maxima of the sample pass
// (cq x 8192 floats at most) and the per-query words; no compact matrix and no nq x nq score block.
static int quant_batch_topk(hdb_index* ix, const TopkArgs& c, const TopkPlan& p) {
    const void* dev_Q = c.Q; const int32_t nq = c.nq, k = c.k; const int metric = c.metric; hipStream_t st = c.st;
    int64_t* dev_idx = c.idx; float* dev_score = c.score; int32_t* dev_status = c.status;      // (the call, under the names the body uses)
    const uint32_t kk = p.kk;
    const int64_t n = ix->n;
    const int P = ix->qP;
    const uint32_t m = HDB_QB_SAMPLE_M;
    const QuantSample sp = p.qs;
    const int64_t s_tiles = sp.s_tiles, s_stride = sp.s_stride, s_rows = sp.s_rows, ld_s = sp.ld_s;
    const int cq_max = p.cq_max;
    QuantBatchWs w;
    const int rc = quant_batch_ws_lay(ix, w, cq_max);
    if (rc) return rc;
    const int64_t wld = quant_batch_wld();
    float* const qinv = w.qinv; float* const qsq = w.qsq; int* const qnan = w.qnan; float* const qscl = w.qscl;
    int8_t* const qcodes = w.qcodes; float* const qaux = w.qaux; float* const thr = w.thr; uint32_t* const cnt = w.cnt;
    unsigned long long* const cand = w.cand; void* const q16 = w.q16; float* const wbuf = w.wbuf;
    for (int q0 = 0; q0 < nq; q0 += cq_max) {
        const int cq = std::min(cq_max, nq - q0);
        const float* Qc = (const float*)dev_Q + (size_t)q0 * ix->d;
        // (the stat word is reset by the first chunk only: quant_cands is the largest list of the CALL)
        LAUNCH_TRY(hdb_launch_quant_qprep_m(Qc, cq, ix->d, P, qinv, qsq, qnan, q16, qscl, qcodes, qaux, q0 == 0 ? ix->qstat : nullptr, cnt, nullptr, st));
        QuantArgs a; quant_base_args(ix, a, qcodes, qaux, qinv, metric, cq);
        a.thr = thr; a.cnt = cnt; a.cand = cand; a.cap = HDB_CAND_CAP;
        if (p.qb_int8) {
            a.ntiles = s_tiles; a.tile_stride = s_stride;
            const int sblocks = hdb_qb_scan_blocks(s_tiles, cq, hdb_cu_count(), (int)ix->opt.max_blocks);
            LAUNCH_TRY(hdb_launch_qb_scan(&a, 0, wbuf, wld, (int)ix->opt.max_blocks, st));
            LAUNCH_TRY(hdb_launch_qb_thr(wbuf, hdb_qb_slots(sblocks, cq), wld, cq, m, thr, st));
            a.ntiles = (n + 15) / 16; a.tile_stride = 1;
            prof_begin(ix, st);
            LAUNCH_TRY(hdb_launch_qb_scan(&a, 1, nullptr, 0, (int)ix->opt.max_blocks, st));
            prof_end(ix, st);
        } else {
            // the v_dot4 scan of the 1-4-query flavour, four queries per pass over the sample and over the shadow
            for (int g0 = 0; g0 < cq; g0 += 4) {
                QuantArgs g = a;
                g.nq = std::min(4, cq - g0);
                g.qcodes = qcodes + (size_t)g0 * P; g.qaux = qaux + (size_t)g0 * HDB_QQ_WORDS; g.qinv = qinv + g0;
                g.thr = thr + g0; g.cnt = cnt + (size_t)g0 * HDB_CNT_STRIDE; g.cand = cand + (size_t)g0 * HDB_CAND_CAP;
                g.ntiles = s_tiles; g.tile_stride = s_stride; g.scores = wbuf; g.ld = ld_s;
                LAUNCH_TRY(hdb_launch_quant_scan(&g, 0, (int)ix->opt.max_blocks, st));
                LAUNCH_TRY(hdb_launch_qb_thr(wbuf, s_rows, ld_s, g.nq, m, thr + g0, st));
                g.ntiles = (n + 15) / 16; g.tile_stride = 1; g.scores = nullptr; g.ld = 0;
                prof_begin(ix, st);
                LAUNCH_TRY(hdb_launch_quant_scan(&g, 1, (int)ix->opt.max_blocks, st));
                prof_end(ix, st);
            }
        }
        LAUNCH_TRY(hdb_launch_qb_rescore(ix->V, ix->d, q16, qscl, qinv, ix->inv_norm, ix->bias, ix->mask, metric, cand, cnt, HDB_CAND_CAP, cq, st));
        LAUNCH_TRY(hdb_launch_quant_finalize(cand, cnt, HDB_CAND_CAP, cq, (uint32_t)k, kk, ix->row_base, dev_idx + (int64_t)q0 * k,
                                             dev_score + (int64_t)q0 * k, dev_status + q0, qnan, qaux, thr, ix->qstat, nullptr, nullptr, 0, st));
    }
    ix->qb_cnt = cnt; ix->qb_cnt_n = nq - (nq - 1) / cq_max * cq_max;
    return HDB_OK;
}

// The single-launch pipelines: a fresh epoch per launch on a control block (31 bits, never 0: bit 31 of a tag is the "final" flag
// of the threshold words), the bound of every in-kernel spin in 100 MHz ticks, and the control block itself, zero when allocated.
static uint32_t next_epoch(hdb_index* ix) {
    ix->fused_epoch = (ix->fused_epoch + 1) & 0x7FFFFFFFu;
    if (ix->fused_epoch == 0) ix->fused_epoch = 1;
    return ix->fused_epoch;
}
static uint32_t timeout_ticks(const hdb_index* ix) { return (uint32_t)std::min<int64_t>(ix->opt.fused_timeout_us * 100, 0x7FFFFFFF); }
static int ensure_ctl(DevBuf<char>& ctl, size_t bytes) {
    if (ctl) return HDB_OK;
    DevBuf<char> c2;                                   // (the index takes the block once it is zero)
    HIP_TRY(c2.alloc(bytes));
    HIP_TRY(hipMemset(c2, 0, bytes));
    ctl.swap(c2);
    return HDB_OK;
}

// nothing stored: all -1 / -inf
static int run_empty(const TopkArgs& c) {
    HIP_TRY(hipMemsetAsync(c.idx, 0xFF, (size_t)c.nq * c.k * sizeof(int64_t), c.st));
    HIP_TRY(hipMemsetAsync(c.score, 0xFF, (size_t)c.nq * c.k * sizeof(float), c.st));   // NaN pattern; no rows exist
    if (c.status) HIP_TRY(hipMemsetAsync(c.status, 0, (size_t)c.nq * sizeof(int32_t), c.st));
    return HDB_OK;
}

// What every path outside the shadow starts with: the workspace (TopkWs, extents from the plan) and the shared prologue -- query
// prep, sign bits, centring, the mask folded into a bias -- each where the plan says so.
struct TopkEnv {
    TopkWs w; size_t sort_temp;
    const void* Qeff; int metric_eff;                  // pearson: the centred queries through the cosine pipeline
    const float* bias_eff; const uint8_t* mask_eff;    // the MFMA scan has no mask input: excluded rows get a bias of -inf instead
};
// (the prologue alone, over a workspace that is laid out already: hdb_maxsim_host lays TopkWs inside its own layout)
static int topk_prologue(hdb_index* ix, const TopkArgs& c, const TopkPlan& p, TopkEnv& e) {
    hipStream_t st = c.st;
    const bool f64 = ix->dtype == HDB_F64;
    const int64_t n = ix->n;
    TopkWs& w = e.w;
    int rc = HDB_OK;
    if (p.prep)
        LAUNCH_TRY(hdb_launch_qprep2(c.Q, c.nq, ix->d, f64, w.qinv, w.qsq, w.qnan, p.q16_in_prep ? w.q16 : nullptr, w.qscl, p.fold_small ? w.thr : nullptr,
                                     p.fold_small ? w.cnt : nullptr, (p.fold_small && p.bits) ? w.qbits : nullptr, p.W, st));
    if (p.bits) {
        rc = ensure_bits(ix, st); if (rc) return rc;
        if (p.prep && !p.fold_small) LAUNCH_TRY(hdb_launch_qsign(c.Q, c.nq, ix->d, f64, p.W, w.qbits, st));
    }
    e.Qeff = c.Q; e.metric_eff = c.metric;
    if (p.pearson) {
        rc = ensure_pscale(ix, st); if (rc) return rc;
        if (p.prep) LAUNCH_TRY(hdb_launch_qcentre(c.Q, c.nq, ix->d, f64, w.qc, w.qinv, st));     // qinv <- 1/sd_q (the single launches centre their queries themselves)
        e.Qeff = w.qc; e.metric_eff = HDB_COSINE;
    }
    e.bias_eff = ix->bias; e.mask_eff = ix->mask;
    if (p.mask_fold) {
        if (n > (int64_t)ix->mbias.cap) HIP_TRY(ix->mbias.alloc((size_t)(n + n / 4 + 64)));
        LAUNCH_TRY(hdb_launch_maskbias(ix->mask, ix->bias, n, ix->mbias, st));
        e.bias_eff = ix->mbias; e.mask_eff = nullptr;
    }
    return HDB_OK;
}
static int topk_begin(hdb_index* ix, const TopkArgs& c, const TopkPlan& p, TopkEnv& e) {
    e.sort_temp = 0;
    if (p.sort_n > 0) LAUNCH_TRY(hdb_sort_temp_bytes(p.sort_n, &e.sort_temp));
    const int rc = ws_lay(ix, e.w, (int)c.nq, (int)ix->d, p.W, p.cq_max, p.ld_scores, p.ld_ks, p.sort_n, e.sort_temp, p.n_best);
    if (rc) return rc;
    return topk_prologue(ix, c, p, e);
}

// k > HDB_MAX_K: one query at a time, all scores -> stable radix sort (hdb_sort.hip)
static int run_full_sort(hdb_index* ix, const TopkArgs& c, const TopkPlan& p) {
    TopkEnv e;
    int rc = topk_begin(ix, c, p, e); if (rc) return rc;
    for (int q0 = 0; q0 < c.nq; ++q0) {
        QueryBufs qb{e.w.qinv, e.w.qsq, e.w.qbits, nullptr, nullptr};
        ScanArgs s2; base_args(ix, s2, e.Qeff, e.metric_eff);
        if (p.pearson) s2.inv_norm = ix->pscale;
        s2.q0 = q0; s2.bias = ix->bias; s2.scores = e.w.sc1; s2.ld = p.ld_n;
        rc = run_scan(ix, s2, 0, 1, qb, false, false, c.st); if (rc) return rc;
        LAUNCH_TRY(hdb_launch_full_sort(e.w.sc1, s2.mask, ix->n, c.k, ix->row_base, e.w.work, e.w.temp, e.sort_temp, c.idx + (int64_t)q0 * c.k,
                                        c.score + (int64_t)q0 * c.k, c.st));
    }
    if (c.status) LAUNCH_TRY(hdb_launch_status_nan(e.w.qnan, c.nq, c.status, c.st));     // HDB_Q_NAN survives on this path too
    return HDB_OK;
}

// 1-4 dot / cosine queries, k <= 128: the whole call in ONE launch (hdb_mfma_fused.h): prep + sample + threshold + filter pass +
// finalize; fp16 on the matrix cores, float32 in the VALU from the same staged tiles.  Exchange or local flavour (p.local).
static int run_fused(hdb_index* ix, const TopkArgs& c, const TopkPlan& p) {
    TopkEnv e;
    int rc = topk_begin(ix, c, p, e); if (rc) return rc;
    rc = ensure_ctl(ix->fctl, hdb_mfma_fused_ctl_bytes()); if (rc) return rc;
    ScanArgs a; base_args(ix, a, c.Q, c.metric);
    a.bias = e.bias_eff; a.mask = nullptr;
    if (c.metric == HDB_EUCLIDEAN) a.inv_norm = ix->sqnorm;        // the per-row aux value of the euclidean expansion
    if (p.pearson) a.inv_norm = ix->pscale;                        // 1/(sd_v d); the kernel centres the queries itself
    a.ntiles = (ix->n + p.tile_rows - 1) / p.tile_rows;
    a.thr = e.w.thr; a.cnt = e.w.cnt; a.cand = e.w.cand; a.nq = c.nq;
    FusedArgs fa; memset(&fa, 0, sizeof(fa));
    fa.Qraw = static_cast<const float*>(c.Q); fa.nq = c.nq;
    fa.s_tiles = p.s_tiles; fa.s_stride = p.s_stride;
    fa.epoch = next_epoch(ix);
    fa.timeout_ticks = timeout_ticks(ix);
    fa.ctl = reinterpret_cast<uint32_t*>(ix->fctl.p);
    fa.cand = e.w.cand; fa.cap = HDB_CAND_CAP; fa.k = (uint32_t)c.k; fa.kk = p.kk; fa.row_base = ix->row_base;
    fa.idx_out = c.idx; fa.score_out = c.score; fa.status = c.status; fa.thr_out = e.w.thr;
    fa.local = p.local ? 1 : 0; fa.local_slot = p.local_slot; fa.local_m = p.local_m;
    LAUNCH_TRY(single_launch(ix, c.st, [&] { return hdb_launch_mfma_fused(&a, ix->dtype, &fa, (int)ix->opt.max_blocks, c.st); }));
    return HDB_OK;
}

// 1-4 hamming / jaccard queries per launch: prep, sample, threshold, the pass over the sign bits and the final sort in ONE
// kernel (hdb_bits_fused.hip); larger batches go through it four queries at a time (as the multi-kernel scan re-reads the bits)
static int run_bits1(hdb_index* ix, const TopkArgs& c, const TopkPlan& p) {
    TopkEnv e;
    int rc = topk_begin(ix, c, p, e); if (rc) return rc;
    rc = ensure_ctl(ix->bctl, hdb_mfma_batch_ctl_bytes(hdb_cu_count())); if (rc) return rc;
    for (int q0 = 0; q0 < c.nq; q0 += 4) {
        const int cq = std::min(4, c.nq - q0);
        BitsArgs ba; memset(&ba, 0, sizeof(ba));
        ba.bits = ix->bits; ba.npad = ix->bits_npad; ba.W = p.W; ba.n = ix->n; ba.d = ix->d;
        ba.Qraw = static_cast<const float*>(c.Q) + (size_t)q0 * ix->d; ba.nq = cq;
        ba.ntiles = (ix->n + 15) / 16; ba.s_tiles = p.s_tiles; ba.s_stride = p.s_stride;
        ba.bias = ix->bias; ba.mask = ix->mask;
        ba.local = p.bits_local;
        ba.epoch = next_epoch(ix);
        ba.timeout_ticks = timeout_ticks(ix);
        ba.ctl = reinterpret_cast<uint32_t*>(ix->bctl.p);
        ba.cand = e.w.cand; ba.cap = HDB_CAND_CAP; ba.k = (uint32_t)c.k; ba.kk = p.kk; ba.row_base = ix->row_base;
        ba.idx_out = c.idx + (int64_t)q0 * c.k; ba.score_out = c.score + (int64_t)q0 * c.k; ba.status = c.status + q0;
        LAUNCH_TRY(single_launch(ix, c.st, [&] { return hdb_launch_bits_fused(&ba, c.metric == HDB_JACCARD ? 1 : 0, (int)ix->opt.max_blocks, c.st); }));
    }
    return HDB_OK;
}

// anything else the matrix-core scan takes (5-256 dot / cosine queries, 1-256 euclidean ones), k <= 128: one launch per
// <= cq_max queries does preparation, sample, thresholds, the pass and every query's final sort (hdb_mfma_kernel.h, MODE 2)
static int run_batch1(hdb_index* ix, const TopkArgs& c, const TopkPlan& p) {
    TopkEnv e;
    int rc = topk_begin(ix, c, p, e); if (rc) return rc;
    rc = ensure_ctl(ix->bctl, hdb_mfma_batch_ctl_bytes(hdb_cu_count())); if (rc) return rc;
    const size_t qrow = (size_t)ix->d * 4;
    for (int q0 = 0; q0 < c.nq; q0 += p.cq_max) {
        const int cq = std::min(p.cq_max, c.nq - q0);
        ScanArgs a; base_args(ix, a, c.Q, e.metric_eff);                                  // pearson: the cosine launch on queries the kernel centres, ...
        if (p.pearson) a.inv_norm = ix->pscale;                                           // ... row scale 1/(sd_v d)
        a.bias = e.bias_eff; a.mask = nullptr; a.q0 = 0; a.nq = cq; a.f32_split = p.f32s ? 1 : 0;
        a.ntiles = (ix->n + p.tile_rows - 1) / p.tile_rows;
        a.cand = e.w.cand;
        a.tile_ctr = ix->opt.dyn_tiles ? reinterpret_cast<uint32_t*>(ix->bctl.p) + HDB_BATCH_CTL_TILE : nullptr;
        BatchArgs fa; memset(&fa, 0, sizeof(fa));
        fa.Qraw = static_cast<const char*>(c.Q) + (size_t)q0 * qrow;
        fa.s_tiles = p.s_tiles; fa.s_stride = p.s_stride; fa.centre = p.pearson ? 1 : 0;
        fa.epoch = next_epoch(ix);
        fa.timeout_ticks = timeout_ticks(ix);
        fa.ctl = reinterpret_cast<uint32_t*>(ix->bctl.p);
        fa.k = (uint32_t)c.k; fa.kk = p.kk; fa.row_base = ix->row_base;
        fa.idx_out = c.idx + (int64_t)q0 * c.k; fa.score_out = c.score + (int64_t)q0 * c.k; fa.status = c.status + q0;
        LAUNCH_TRY(single_launch(ix, c.st, [&] {
            return hdb_launch_mfma_scan(&a, ix->dtype, 2, cq, nullptr, ix->sqnorm, nullptr, nullptr, (int)ix->opt.max_blocks, (int)ix->opt.mfma_variant, c.st, &fa);
        }));
    }
    return HDB_OK;
}

// The multi-kernel pipeline, cq_max queries at a time.  small: thr = -inf -> scan(filter) -> finalize; sampled: scan(scores) over the
// row sample -> threshold -> scan(filter) over all rows -> finalize; exact: scan(scores) over all rows -> radix passes -> collect.
// p.subset: the same three shapes over the m rows of the index's list (ScanArgs::rows / m) -- the plan is that of a matrix of m
// rows, "all rows" are the listed ones, no mask (every listed row is kept), the bias unfolded and indexed by the true row; the
// exact shape collects list positions and rewrites them to rows before finalize.
// What run_pipeline and hdb_maxsim_host share -- "prepare the queries of a chunk and score them into sbuf" -- in three steps:
// exact_parts: float32 rows as bf16 parts in a call that ASKED for the exact selection (hdb_topk_exact: the last resort, status 0
// whatever the queries hold): the parts of an infinite query element cancel to NaN, so the call keeps them -- and the default call's
// bits -- only while no query holds an infinity.  The preparation left that per query (qnan & 2); reading it is a stream
// synchronisation, paid by exact calls of float32 batches and by no other call.
static int exact_parts(hdb_index* ix, const TopkPlan& p, const int* qnan, int32_t nq, hipStream_t st, bool& f32s) {
    f32s = p.f32s;
    if (f32s && p.exact_req) {
        std::vector<int> h_qnan((size_t)nq);
        HIP_TRY(hipMemcpyAsync(h_qnan.data(), qnan, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int q = 0; q < nq; ++q) f32s = f32s && !(h_qnan[q] & 2);
        if (!f32s) ix->st.f32s = 0;
    }
    return HDB_OK;
}
// chunk_args: the query buffers and scan arguments of the chunk [q0, q0 + cq) of a call of nq queries over n rows (the fp16 copies of
// all queries are written by the first chunk that needs them)
static int chunk_args(hdb_index* ix, const TopkPlan& p, const TopkEnv& e, bool f32s, int32_t nq, int q0, int cq, int64_t n, bool& q16_ready,
                      hipStream_t st, QueryBufs& qb, ScanArgs& a) {
    const TopkWs& w = e.w;
    if (p.f16_queries && !q16_ready) { LAUNCH_TRY(hdb_launch_q_to_f16((const float*)e.Qeff, nq, ix->d, w.q16, w.qscl, st)); q16_ready = true; }
    qb = QueryBufs{w.qinv, w.qsq, w.qbits, p.f16_queries ? w.q16 : e.Qeff, p.f16_queries ? w.qscl : nullptr};
    base_args(ix, a, e.Qeff, e.metric_eff);
    if (p.pearson) a.inv_norm = ix->pscale;
    a.q0 = q0; a.bias = e.bias_eff; a.mask = e.mask_eff; a.f32_split = f32s ? 1 : 0;
    a.f8_lds = !p.f8_lds ? 0 : ix->opt.f8_lds_waves ? (int)ix->opt.f8_lds_waves : hdb_mfma_f8_lds_auto_waves(cq);
    a.thr = w.thr; a.cnt = w.cnt; a.cand = w.cand;
    a.ntiles = (n + p.tile_rows - 1) / p.tile_rows;
    if (p.subset) { a.rows = ix->rows; a.m = ix->subset_m; a.mask = nullptr; a.bias = ix->bias; }
    a.ks_partial_out = w.kbuf; a.ks_ld = p.ld_n;       // (K slices only; sample and exact passes index it by their own tile sequence)
    return HDB_OK;
}
// score_chunk: the exact shape's score pass -- every score of the chunk's queries into sbuf[cq][ld_n]
static int score_chunk(hdb_index* ix, const TopkPlan& p, const ScanArgs& a, const QueryBufs& qb, int cq, float* sbuf, hipStream_t st) {
    ScanArgs s = a;
    s.scores = sbuf; s.ld = p.ld_n;
    prof_begin(ix, st);
    const int rc = run_scan(ix, s, 0, cq, qb, p.l1tile, p.mfma, st); if (rc) return rc;
    prof_end(ix, st);
    return HDB_OK;
}
// select_exact: the exact selection over a score matrix -- scores[cq][ld], n entries each -- into cand / cnt: npass radix-histogram
// passes fix each query's kk-th largest score, collect gathers what lies above it and the ordered ties.
// cnt and hist are neighbours in the workspace, cnt first (TopkWs, MaxsimWs; hdb_ws.h): one memset clears both.
static int select_exact(const float* scores, int64_t n, int64_t ld, int cq, int npass, uint32_t kk, uint32_t* cnt, uint32_t* hist, uint32_t* tie_info,
                        unsigned long long* cand, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)((char*)hist - (char*)cnt) + (size_t)cq * 4 * HDB_RADIX_BINS * 4, st));
    for (int ps = 0; ps < npass; ++ps) LAUNCH_TRY(hdb_launch_hist(scores, n, ld, cq, hist, ps, kk, st));
    LAUNCH_TRY(hdb_launch_collect(scores, n, ld, cq, hist, npass, kk, cnt, cand, HDB_CAND_CAP, tie_info, st));
    return HDB_OK;
}

static int run_pipeline(hdb_index* ix, const TopkArgs& c, const TopkPlan& p) {
    TopkEnv e;
    int rc = topk_begin(ix, c, p, e); if (rc) return rc;
    const TopkWs& w = e.w;
    hipStream_t st = c.st; const int32_t k = c.k;
    const int64_t n = p.subset ? ix->subset_m : ix->n;
    bool f32s = false;
    rc = exact_parts(ix, p, w.qnan, c.nq, st, f32s); if (rc) return rc;
    bool q16_ready = p.q16_in_prep;
    for (int q0 = 0; q0 < c.nq; q0 += p.cq_max) {
        const int cq = std::min(p.cq_max, c.nq - q0);
        int64_t* const out_idx = c.idx + (int64_t)q0 * k; float* const out_score = c.score + (int64_t)q0 * k;      // the chunk's slots of the answer
        int32_t* const out_status = c.status ? c.status + q0 : nullptr;
        QueryBufs qb; ScanArgs a;
        rc = chunk_args(ix, p, e, f32s, c.nq, q0, cq, n, q16_ready, st, qb, a); if (rc) return rc;

        if (p.small) {
            if (!p.fold_small) LAUNCH_TRY(hdb_launch_fill_thr(w.thr, w.cnt, cq, -INFINITY, st));
            rc = run_scan(ix, a, 1, cq, qb, p.l1tile, p.mfma, st); if (rc) return rc;
        } else if (!p.exact) {
            // 1) strided row sample -> sample scores
            ScanArgs s = a;
            s.ntiles = p.s_tiles; s.tile_stride = p.s_stride; s.scores = w.sbuf; s.ld = p.ld_s;
            rc = run_scan(ix, s, 0, cq, qb, p.l1tile, p.mfma, st); if (rc) return rc;
            // 2) m-th largest sample score per query
            if (p.m <= 16) {
                LAUNCH_TRY(hdb_launch_sample_thr(w.sbuf, p.s_rows, p.ld_s, cq, p.m, w.thr, w.cnt, w.tile_ctr, st));
                if (p.mfma && ix->opt.dyn_tiles) a.tile_ctr = w.tile_ctr;       // zeroed just now: dynamic tile hand-out in the pass
            } else {
                HIP_TRY(hipMemsetAsync(w.hist, 0, (size_t)cq * 4 * HDB_RADIX_BINS * 4, st));
                for (int ps = 0; ps < 4; ++ps) LAUNCH_TRY(hdb_launch_hist(w.sbuf, p.s_rows, p.ld_s, cq, w.hist, ps, p.m, st));
                LAUNCH_TRY(hdb_launch_thr(w.hist, cq, 4, p.m, (uint32_t)p.s_rows, w.thr, w.cnt, st));
            }
            // 3) the pass over all of V
            prof_begin(ix, st);
            rc = run_scan(ix, a, 1, cq, qb, p.l1tile, p.mfma, st); if (rc) return rc;
            prof_end(ix, st);
        } else {
            rc = score_chunk(ix, p, a, qb, cq, w.sbuf, st); if (rc) return rc;
            if (p.n_best > 0) {
                // the exact grouped pass: each group's best row keeps its score, every other row joins the masked ones at -inf
                HIP_TRY(hipMemsetAsync(w.best, 0, (size_t)cq * (size_t)p.n_best * sizeof(unsigned long long), st));      // key 0 is below every real key
                if (q0 == 0) HIP_TRY(hipMemsetAsync(w.gbad, 0, sizeof(int), st));
                LAUNCH_TRY(hdb_launch_group_best(w.sbuf, n, p.ld_n, cq, ix->groups, p.n_best, w.best, st));
                LAUNCH_TRY(hdb_launch_group_demote(w.sbuf, n, p.ld_n, cq, ix->groups, p.n_best, w.best, w.gbad, st));
            }
            rc = select_exact(w.sbuf, n, p.ld_n, cq, p.npass, p.kk, w.cnt, w.hist, w.tie_info, w.cand, st); if (rc) return rc;
            if (p.subset) LAUNCH_TRY(hdb_launch_list_rows(w.cand, w.cnt, HDB_CAND_CAP, cq, ix->rows, ix->subset_m, st));
        }
        if (p.mfma && c.metric == HDB_EUCLIDEAN)     // the MFMA path scores through ||v||^2+||q||^2-2v.q: redo near-duplicates directly
            LAUNCH_TRY(hdb_launch_rescore_euclid(w.cand, w.cnt, HDB_CAND_CAP, cq, ix->V, ix->dtype, ix->d, (const float*)c.Q, w.qsq, q0, ix->bias, st));
        LAUNCH_TRY(hdb_launch_finalize(w.cand, w.cnt, HDB_CAND_CAP, cq, (uint32_t)k, p.kk, ix->row_base, out_idx, out_score, out_status, w.qnan + q0,
                                       (int)ix->opt.finalize_threads, a.f32_split ? HDB_Q_UNDERFLOW : 0, st));      // (parts of an infinite query element cancel to NaN: exact re-run)
        if (p.n_best > 0)       // (entries the selection handed out at -inf are padding; a bad group id marks the chunk's queries)
            LAUNCH_TRY(hdb_launch_group_finish(out_idx, out_score, cq, k, out_status, w.gbad, st));
    }
    return HDB_OK;
}

// Plan a call (plan_topk, hdb_plan.h).  The planner's one question to the device is the cached flag word of the last build, fetched
// where it decides something; a fetch that failed is the call's error.
static int plan_call(hdb_index* ix, const TopkCall& call, TopkPlan& out) {
    int frc = HDB_OK;
    auto finite = [&] { bool f = false; if (frc == HDB_OK) frc = matrix_is_finite(ix, &f); return f; };
    out = plan_topk(topk_facts(ix), ix->opt, call, finite);
    return frc;
}
// The statistics of a call start here: the plan's (or a fresh set), and no list counters of an earlier batch through the shadow.
static void stats_begin(hdb_index* ix, const TopkStats& stats) {
    ix->st = stats; ix->qb_cnt = nullptr; ix->qb_cnt_n = 0;
}

static int topk_impl(hdb_index* ix, const void* dev_Q, int32_t nq, int32_t k, int metric, int64_t* dev_idx,
                     float* dev_score, int32_t* dev_status, void* stream, bool exact) {
    if (!ix || !dev_idx || !dev_score) return fail(HDB_ERR_ARG, "hdb_topk: null argument");
    if (nq < 0 || k < 0) return fail(HDB_ERR_ARG, "hdb_topk: nq and k must be >= 0");
    if (nq == 0 || k == 0) return HDB_OK;
    if (!dev_Q) return fail(HDB_ERR_ARG, "hdb_topk: query pointer is null");
    if (metric == HDB_EUCLIDEAN_DIST || !metric_ok(metric)) return fail(HDB_ERR_UNSUPPORTED, "hdb_topk: metric not built");
    if (metric == HDB_PEARSON && ix->d < 1) return fail(HDB_ERR_ARG, "hdb_topk: pearson needs d >= 1");
    HIP_TRY(hipSetDevice(ix->device));
    const TopkArgs c{dev_Q, nq, k, metric, dev_idx, dev_score, dev_status, (hipStream_t)stream};
    const TopkCall call{nq, k, metric, dev_status != nullptr, exact};
    TopkPlan p;
    int rc = plan_call(ix, call, p); if (rc) return rc;
    if (p.shadow()) {                // a declined build or plane is a new fact: plan once more, and only once
        bool declined = false;
        rc = shadow_prepare(ix, p, nq, c.st, &declined); if (rc) return rc;
        if (declined) { rc = plan_call(ix, call, p); if (rc) return rc; }
    }
    stats_begin(ix, p.stats);
    switch (p.path) {
    case HDB_PATH_EMPTY: return run_empty(c);
    case HDB_PATH_QUANT: return quant_topk(ix, c, p);
    case HDB_PATH_QUANT_BATCH: return quant_batch_topk(ix, c, p);
    case HDB_PATH_FUSED: return run_fused(ix, c, p);
    case HDB_PATH_BITS1: return run_bits1(ix, c, p);
    case HDB_PATH_BATCH1: return run_batch1(ix, c, p);
    case HDB_PATH_FULL_SORT: return run_full_sort(ix, c, p);
    case HDB_PATH_PIPELINE: return run_pipeline(ix, c, p);
    }
    return fail(HDB_ERR_ARG, "hdb_topk: no path");
}

extern "C" int hdb_topk(hdb_index* ix, const void* dev_Q, int32_t nq, int32_t k, int metric, int64_t* dev_idx,
                        float* dev_score, int32_t* dev_status, void* stream) {
    return topk_impl(ix, dev_Q, nq, k, metric, dev_idx, dev_score, dev_status, stream, false);
}

// k-way merge of `parts` packed records in host memory (recs[p] = record of shard p) into out_record
static void merge_host_records(const char* const* recs, int32_t parts, int32_t nq, int32_t k, void* out_record) {
    const PackedRec out = packed_view(out_record, nq, k);
    int64_t* oi = out.idx; float* os = out.score; int32_t* ost = out.status;
    auto in = [&](int32_t p) { return packed_view(recs[p], nq, k); };
    std::vector<int32_t> pos((size_t)parts);
    for (int32_t q = 0; q < nq; ++q) {
        int32_t st = 0;
        for (int32_t p = 0; p < parts; ++p) {
            st |= in(p).status[q];
            pos[p] = 0;
        }
        for (int32_t i = 0; i < k; ++i) {                // lists sorted by (score descending, row ascending)
            int32_t best = -1; int64_t bi = -1; float bs = 0.f;
            for (int32_t p = 0; p < parts; ++p) {
                if (pos[p] >= k) continue;
                const int64_t ci = in(p).idx[(int64_t)q * k + pos[p]];
                if (ci < 0) { pos[p] = k; continue; }    // padding: this shard has no more rows
                const float cs = in(p).score[(int64_t)q * k + pos[p]];
                if (best < 0 || cs > bs || (cs == bs && ci < bi)) { best = p; bi = ci; bs = cs; }
            }
            if (best < 0) { oi[(int64_t)q * k + i] = -1; os[(int64_t)q * k + i] = -INFINITY; }
            else { oi[(int64_t)q * k + i] = bi; os[(int64_t)q * k + i] = bs; ++pos[best]; }
        }
        ost[q] = st;
    }
}

extern "C" int hdb_merge_topk_host(const void* records, int32_t parts, int32_t nq, int32_t k, void* out_record) {
    if (!records || !out_record || parts <= 0 || nq < 0 || k < 0) return fail(HDB_ERR_ARG, "hdb_merge_topk_host: bad argument");
    const int64_t nb = hdb_packed_bytes(nq, k);
    std::vector<const char*> recs((size_t)parts);
    for (int32_t p = 0; p < parts; ++p) recs[p] = static_cast<const char*>(records) + p * nb;
    merge_host_records(recs.data(), parts, nq, k, out_record);
    return HDB_OK;
}

extern "C" int hdb_host_exchange_merge(void* shm, int64_t stride, int32_t world, int32_t rank, uint64_t seq, const void* record,
                                       int32_t nq, int32_t k, void* out_record, double timeout_s) {
    if (!shm || !record || !out_record || world <= 0 || rank < 0 || rank >= world || stride < 64 || nq < 0 || k < 0)
        return fail(HDB_ERR_ARG, "hdb_host_exchange_merge: bad argument");
    const int64_t nb = hdb_packed_bytes(nq, k);
    if (nb + 64 > stride) return fail(HDB_ERR_ARG, "hdb_host_exchange_merge: record larger than a slot");
    char* base = static_cast<char*>(shm) + (int64_t)(seq & 1) * world * stride;
    char* mine = base + (int64_t)rank * stride;
    memcpy(mine + 64, record, (size_t)nb);
    __atomic_store_n(reinterpret_cast<uint64_t*>(mine), seq, __ATOMIC_RELEASE);          // publish: after the data
    std::vector<const char*> recs((size_t)world);
    const auto t0 = std::chrono::steady_clock::now();
    for (int32_t r = 0; r < world; ++r) {
        const uint64_t* sp = reinterpret_cast<const uint64_t*>(base + (int64_t)r * stride);
        uint32_t spins = 0;
        while (__atomic_load_n(sp, __ATOMIC_ACQUIRE) != seq) {
            __builtin_ia32_pause();
            if ((++spins & 0xFFFFu) == 0 &&
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s)
                return fail(HDB_ERR_HIP, "hdb_host_exchange_merge: a rank did not publish its record in time");
        }
        recs[r] = base + (int64_t)r * stride + 64;
    }
    merge_host_records(recs.data(), world, nq, k, out_record);
    return HDB_OK;
}

// The exact re-run: every query whose status word says that its sampled threshold failed goes once more through the exact selection,
// one by one, straight into its slots of the device view `dv`.  Which queries are flagged is read off `h_st` BEFORE the first re-run:
// with a pinned record the host's words ARE the device's, and every re-run rewrites its own.  *ran: whether anything ran.  Each
// re-run starts the statistics anew; what the call reports afterwards is the caller's rule.
static int rerun_flagged(hdb_index* ix, const void* dev_Q, int32_t nq, int32_t k, int metric, const PackedRec& dv, const int32_t* h_st,
                         hipStream_t st, bool* ran) {
    std::vector<int> bad;                  // (empty, as nearly always: no allocation)
    for (int q = 0; q < nq; ++q) if (h_st[q] & (HDB_Q_UNDERFLOW | HDB_Q_OVERFLOW)) bad.push_back(q);
    *ran = !bad.empty();
    for (int q : bad) {
        const int rc = topk_impl(ix, static_cast<const char*>(dev_Q) + (size_t)q * query_pitch(ix), 1, k, metric, dv.idx + (size_t)q * k,
                                 dv.score + (size_t)q * k, dv.status + q, st, true);
        if (rc) return rc;
    }
    return HDB_OK;
}
extern "C" int hdb_topk_host(hdb_index* ix, const void* dev_Q, int32_t nq, int32_t k, int metric, void* host_record, void* stream) {
    if (!ix || !host_record) return fail(HDB_ERR_ARG, "hdb_topk_host: null argument");
    if (nq <= 0 || k <= 0) return fail(HDB_ERR_ARG, "hdb_topk_host: nq and k must be positive");
    const auto ht0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    // Pinned (device-visible) host memory: the last kernels of the pipeline store the record there themselves and the
    // D2H copy disappears from the critical path; anything else goes through a device record and one hipMemcpyAsync.
    bool direct = false;
    if (ix->opt.host_direct) {
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, host_record) == hipSuccess) direct = attr.type == hipMemoryTypeHost && attr.devicePointer == host_record;
        else (void)hipGetLastError();
        ix->ht_attr_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - ht0).count();
    }
    ix->st_host_direct = direct ? 1 : 0;
    HostRec rec;
    int rc = hostrec_open(ix->rec, nq, k, host_record, direct, rec); if (rc) return rc;
    // Pinned record: the status words are stored last (by the single-launch kernel's final workgroup, or by each query's
    // finalize workgroup), behind a system-scope release, so the host can poll them instead of waiting for the completion
    // signal of the last kernel (end-of-kernel drain, cache write-back, signal, wake-up: ~5-10 us).  The stream stays
    // ordered: the next launch queues behind the kernels.
    constexpr int32_t SENTINEL = 0x7FFFFFFF;
    volatile int32_t* poll = packed_view(host_record, nq, k).status;
    if (direct && ix->opt.host_poll) for (int q = 0; q < nq; ++q) poll[q] = SENTINEL;
    ix->ht_l0 = ix->ht_l1 = std::chrono::steady_clock::now();      // (pipelines of several launches: everything counts as "pre")
    rc = topk_impl(ix, dev_Q, nq, k, metric, rec.view.idx, rec.view.score, rec.view.status, stream, false); if (rc) return rc;
    rc = hostrec_close(rec, st, false); if (rc) return rc;      // (the copy alone: the wait is the poll below, or the stream's where nothing was polled)
    bool polled = false;
    if (direct && ix->opt.host_poll && (ix->st.fused || ix->st.path != 3)) {      // (the k > 2048 full sort writes its status words elsewhere)
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned spins = 0;; ++spins) {
            bool done = true;
            for (int q = 0; q < nq; ++q) done &= poll[q] != SENTINEL;
            if (done) { polled = true; break; }
            if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) break;   // fall back to the signal
            __builtin_ia32_pause();
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (!polled) HIP_TRY(hipStreamSynchronize(st));
    {
        const auto ht3 = std::chrono::steady_clock::now();
        using ns = std::chrono::nanoseconds;
        ix->ht_pre_ns += std::chrono::duration_cast<ns>(ix->ht_l0 - ht0).count();
        ix->ht_launch_ns += std::chrono::duration_cast<ns>(ix->ht_l1 - ix->ht_l0).count();
        ix->ht_wait_ns += std::chrono::duration_cast<ns>(ht3 - ix->ht_l1).count();
        ix->ht_calls++;
    }
    const int64_t quant_first = ix->st.quant;      // rare: the failed queries again, straight into their slots of the record
    bool ran = false;
    rc = rerun_flagged(ix, dev_Q, nq, k, metric, rec.view, packed_view(host_record, nq, k).status, st, &ran);
    if (rc || !ran) return rc;
    ix->st.quant = quant_first;      // the rule of this call: the statistics are the last re-run's, but "quant" reports the first attempt
    return hostrec_close(rec, st);
}

extern "C" int hdb_topk_exact(hdb_index* ix, const void* dev_Q, int32_t nq, int32_t k, int metric, int64_t* dev_idx,
                              float* dev_score, int32_t* dev_status, void* stream) {
    return topk_impl(ix, dev_Q, nq, k, metric, dev_idx, dev_score, dev_status, stream, true);
}

// ---- hdb_rerank: exact top-k of every query among its own list of rows (hdb_rerank.hip) ---------------------------------------------
// What is decided from the numbers alone comes first, before the handle is looked at and before any HIP call.
static int rerank_sizes(const char* who, int32_t nq, int32_t m, int32_t k, bool host) {
    if (m < 1 || m > HDB_CAND_CAP) return fail(HDB_ERR_ARG, std::string(who) + ": m (candidates per query) must be in [1, 8192]");
    if (k < 1 || k > m) return fail(HDB_ERR_ARG, std::string(who) + ": k must be in [1, m]");
    if (host ? nq <= 0 : nq < 0) return fail(HDB_ERR_ARG, std::string(who) + (host ? ": nq must be positive" : ": nq must be >= 0"));
    return HDB_OK;
}
// The metrics a ranking call beside hdb_topk takes (rerank, grouped, multi-vector): the five that score a row against a query.
// what_is: the call's name for itself in the sentence ("rerank is", "grouped calls are").
static int ranking_metric(const char* who, const char* what_is, int metric) {
    if (is_bits_metric(metric)) return fail(HDB_ERR_UNSUPPORTED, std::string(who) + ": hamming / jaccard " + what_is + " not built");
    if (metric != HDB_DOT && metric != HDB_COSINE && metric != HDB_EUCLIDEAN && metric != HDB_MANHATTAN && metric != HDB_PEARSON)
        return fail(HDB_ERR_UNSUPPORTED, std::string(who) + ": metric not built");
    return HDB_OK;
}
// ... and the k of a call that answers in groups (grouped, multi-vector)
static int ranking_k(const char* who, int32_t k) {
    if (k < 1) return fail(HDB_ERR_ARG, std::string(who) + ": k must be at least 1");
    if (k > HDB_MAX_K) return fail(HDB_ERR_UNSUPPORTED, std::string(who) + ": k beyond HDB_MAX_K (2048) is not built");
    return HDB_OK;
}
// Per chunk of queries: list preparation (valid, ascending, unique rows; the status words), the scoring pass, the finalize of the
// multi-kernel pipeline over lists of at most m <= HDB_CAND_CAP entries.  The finalize gets no status pointer: a list shorter than k
// is no underflow here, the tail is -1 / -inf and the status word is the preparation's (HDB_Q_NAN, HDB_Q_BADROW).
static int rerank_impl(const char* who, hdb_index* ix, const void* dev_Q, int32_t nq, const int64_t* dev_cand, int32_t m, int32_t k, int metric,
                       int64_t* dev_idx, float* dev_score, int32_t* dev_status, hipStream_t st) {
    if (!ix) return fail(HDB_ERR_ARG, std::string(who) + ": null index");
    if (nq == 0) return HDB_OK;
    if (!dev_Q || !dev_cand || !dev_idx || !dev_score) return fail(HDB_ERR_ARG, std::string(who) + ": null argument");
    if (ix->dtype == HDB_B1) return fail(HDB_ERR_UNSUPPORTED, std::string(who) + ": a packed-bit index is a first stage: rerank onto packed bits is not built");
    int rc = ranking_metric(who, "rerank is", metric); if (rc) return rc;
    HIP_TRY(hipSetDevice(ix->device));
    const bool f64 = ix->dtype == HDB_F64, pearson = metric == HDB_PEARSON;
    const int cq_max = (int)std::min<int64_t>(nq, ix->opt.rerank_chunk > 0 ? ix->opt.rerank_chunk : HDB_RERANK_MAXQ);
    stats_begin(ix, TopkStats());
    ix->st.rerank = 1;
    RerankWs w;
    rc = ws_lay(ix, w, (int)nq, (int)ix->d, cq_max, (int)m, pearson);
    if (rc) return rc;
    LAUNCH_TRY(hdb_launch_qprep2(dev_Q, nq, ix->d, f64, w.qinv, w.qsq, w.qnan, nullptr, nullptr, nullptr, nullptr, nullptr, 0, st));
    const void* Qeff = dev_Q; int metric_eff = metric;
    if (pearson) {                      // cosine on the centred queries with 1/(sd d) row scales, as topk_begin / run_pipeline prepare them
        rc = ensure_pscale(ix, st); if (rc) return rc;
        LAUNCH_TRY(hdb_launch_qcentre(dev_Q, nq, ix->d, f64, w.qc, w.qinv, st));
        Qeff = w.qc; metric_eff = HDB_COSINE;
    }
    for (int q0 = 0; q0 < nq; q0 += cq_max) {
        const int cq = std::min(cq_max, nq - q0);
        LAUNCH_TRY(hdb_launch_rerank_prep(dev_cand + (int64_t)q0 * m, m, cq, ix->n, ix->row_base, ix->mask, w.qnan + q0, w.rows, w.cnt,
                                          dev_status ? dev_status + q0 : nullptr, st));
        ScanArgs a; base_args(ix, a, Qeff, metric_eff);
        if (pearson) a.inv_norm = ix->pscale;
        a.q0 = q0; a.qinv = w.qinv; a.bias = ix->bias; a.mask = nullptr;      // (the preparation dropped the masked rows)
        a.rows = w.rows; a.m = m; a.cnt = w.cnt; a.cand = w.cand; a.nq = nq;
        LAUNCH_TRY(hdb_launch_rerank_score(&a, ix->dtype, cq, st));
        LAUNCH_TRY(hdb_launch_finalize(w.cand, w.cnt, HDB_CAND_CAP, cq, (uint32_t)k, (uint32_t)k, ix->row_base, dev_idx + (int64_t)q0 * k,
                                       dev_score + (int64_t)q0 * k, nullptr, nullptr, (int)ix->opt.finalize_threads, 0, st));
        ix->st.chunks++;
    }
    return HDB_OK;
}

extern "C" int hdb_rerank(hdb_index* ix, const void* dev_Q, int32_t nq, const int64_t* dev_cand, int32_t m, int32_t k, int metric,
                          int64_t* dev_idx, float* dev_score, int32_t* dev_status, void* stream) {
    const int rc = rerank_sizes("hdb_rerank", nq, m, k, false);
    if (rc) return rc;
    return rerank_impl("hdb_rerank", ix, dev_Q, nq, dev_cand, m, k, metric, dev_idx, dev_score, dev_status, (hipStream_t)stream);
}

extern "C" int hdb_rerank_host(hdb_index* ix, const void* dev_Q, int32_t nq, const int64_t* dev_cand, int32_t m, int32_t k, int metric,
                               void* host_record, void* stream) {
    int rc = rerank_sizes("hdb_rerank_host", nq, m, k, true);
    if (rc) return rc;
    if (!ix || !host_record) return fail(HDB_ERR_ARG, "hdb_rerank_host: null argument");
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    HostRec rec;
    rc = hostrec_open(ix->rec, nq, k, host_record, false, rec); if (rc) return rc;
    rc = rerank_impl("hdb_rerank_host", ix, dev_Q, nq, dev_cand, m, k, metric, rec.view.idx, rec.view.score, rec.view.status, st); if (rc) return rc;
    return hostrec_close(rec, st);
}

// Stage one on `first` into a device record of its own, its status words read back and the failed queries re-run exactly (as
// hdb_topk_host does); the [nq][k1] ids then go straight into the rerank on `second`.
extern "C" int hdb_two_stage_host(hdb_index* first, const void* dev_Q1, int metric1, int32_t k1, hdb_index* second, const void* dev_Q2,
                                  int metric2, int32_t k, int32_t nq, void* host_record, void* stream) {
    int rc = rerank_sizes("hdb_two_stage_host", nq, k1, k, true);      // (k1 is the rerank's m)
    if (rc) return rc;
    if (!first || !second || !dev_Q1 || !dev_Q2 || !host_record) return fail(HDB_ERR_ARG, "hdb_two_stage_host: null argument");
    if (first->device != second->device || first->n != second->n || first->row_base != second->row_base)
        return fail(HDB_ERR_ARG, "hdb_two_stage_host: the two indexes must be on the same device and have the same n and row_base");
    if ((int64_t)k1 > first->n) return fail(HDB_ERR_ARG, "hdb_two_stage_host: k1 must be at most min(8192, n)");
    HIP_TRY(hipSetDevice(first->device));
    hipStream_t st = (hipStream_t)stream;
    HostRec rec1;                                     // (stage one's record stays on the device: opened, never closed)
    rc = hostrec_open(first->rec1, nq, k1, nullptr, false, rec1); if (rc) return rc;
    const PackedRec& r1 = rec1.view;
    rc = topk_impl(first, dev_Q1, nq, k1, metric1, r1.idx, r1.score, r1.status, stream, false); if (rc) return rc;
    std::vector<int32_t> h_st((size_t)nq);
    HIP_TRY(hipMemcpyAsync(h_st.data(), r1.status, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const TopkStats first_stats = first->st;
    bool ran = false;
    rc = rerun_flagged(first, dev_Q1, nq, k1, metric1, r1, h_st.data(), st, &ran); if (rc) return rc;
    if (ran) first->st = first_stats;                 // the rule of this call: `first` reports its first attempt, every statistic of it
    return hdb_rerank_host(second, dev_Q2, nq, r1.idx, k1, k, metric2, host_record, stream);
}

// ---- grouped top-k: one row per group (hdb_group.hip, hdb_group_plan.h) -----------------------------------------------------------
// The exact grouped pass over nq queries: the exact shape of run_pipeline with the per-group maxima in its workspace.
static int grouped_exact(hdb_index* ix, const void* dev_Q, int32_t nq, int32_t k, int metric, int64_t* dev_idx, float* dev_score,
                         int32_t* dev_status, hipStream_t st) {
    const TopkArgs c{dev_Q, nq, k, metric, dev_idx, dev_score, dev_status, st};
    TopkPlan p;
    const int rc = plan_call(ix, group_exact_call(nq, k, metric, ix->n_groups), p); if (rc) return rc;
    if (!group_exact_shape(p)) return fail(HDB_ERR_UNSUPPORTED, "hdb_topk_grouped_host: this call has no exact grouped pass");
    stats_begin(ix, p.stats);
    return run_pipeline(ix, c, p);
}

extern "C" int hdb_topk_grouped_host(hdb_index* ix, const void* dev_Q, int32_t nq, int32_t k, int metric, void* host_record, void* stream) {
    // what the numbers alone decide, then the handle, then the device
    if (nq <= 0) return fail(HDB_ERR_ARG, "hdb_topk_grouped_host: nq must be positive");
    int rc = ranking_k("hdb_topk_grouped_host", k); if (rc) return rc;
    if (!ix || !dev_Q || !host_record) return fail(HDB_ERR_ARG, "hdb_topk_grouped_host: null argument");
    if (!ix->groups) return fail(HDB_ERR_ARG, "hdb_topk_grouped_host: no groups set (hdb_index_set_groups)");
    rc = ranking_metric("hdb_topk_grouped_host", "grouped calls are", metric); if (rc) return rc;
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    HostRec rec;
    rc = hostrec_open(ix->rec, nq, k, host_record, false, rec); if (rc) return rc;
    const PackedRec& out = rec.view;
    const size_t qbytes = query_pitch(ix);
    const GroupRounds gr = group_rounds(ix->n, k, ix->opt.group_oversample, ix->opt.group_fast_rounds);
    int64_t st_k = 0, st_rounds = 0, st_exact = 0;
    std::vector<int32_t> h_st((size_t)nq, 0);
    std::vector<char> todo((size_t)nq, 1);             // queries the exact pass still has to answer
    if (ix->n == 0) {
        rc = run_empty(TopkArgs{dev_Q, nq, k, metric, out.idx, out.score, out.status, st});
        if (rc) return rc;
        std::fill(todo.begin(), todo.end(), 0);
    }
    const int32_t carry = HDB_Q_NAN | HDB_Q_UNDERFLOW | HDB_Q_OVERFLOW;
    for (int r = 0; r < gr.rounds && ix->n > 0; ++r) {
        const int32_t kr = gr.kr[r];
        // round 1: the whole batch in one call; round 2: the flagged queries, one by one, each into the head of the round's record
        HostRec round;
        rc = hostrec_open(ix->rec1, r == 0 ? nq : 1, kr, nullptr, false, round); if (rc) return rc;
        const PackedRec& rr = round.view;
        bool ran = false;
        if (r == 0) {
            rc = topk_impl(ix, dev_Q, nq, kr, metric, rr.idx, rr.score, rr.status, stream, false);
            if (rc) return rc;
            LAUNCH_TRY(hdb_launch_group_collapse(rr.idx, rr.score, nq, kr, k, ix->groups, ix->n_groups, ix->n, ix->row_base, out.idx, out.score,
                                                 rr.status, out.status, carry, st));
            ran = true;
        } else {
            for (int q = 0; q < nq; ++q) {
                if (!todo[q] || (h_st[q] & (HDB_Q_UNDERFLOW | HDB_Q_OVERFLOW))) continue;      // (a failed sampled call: straight to the exact pass)
                rc = topk_impl(ix, static_cast<const char*>(dev_Q) + (size_t)q * qbytes, 1, kr, metric, rr.idx, rr.score, rr.status, stream, false);
                if (rc) return rc;
                LAUNCH_TRY(hdb_launch_group_collapse(rr.idx, rr.score, 1, kr, k, ix->groups, ix->n_groups, ix->n, ix->row_base, out.idx + (size_t)q * k,
                                                     out.score + (size_t)q * k, rr.status, out.status + q, carry, st));
                ran = true;
            }
        }
        if (!ran) break;
        st_k = kr; ++st_rounds;
        HIP_TRY(hipMemcpyAsync(h_st.data(), out.status, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        bool any = false;
        for (int q = 0; q < nq; ++q) {
            todo[q] = (h_st[q] & (HDB_Q_UNDERFLOW | HDB_Q_OVERFLOW | HDB_Q_GROUPS_SHORT)) != 0;
            any |= todo[q] != 0;
        }
        if (!any) break;
    }
    // the exact grouped pass: runs of consecutive queries in one call each
    for (int q = 0; q < nq;) {
        if (!todo[q]) { ++q; continue; }
        int e = q + 1;
        while (e < nq && todo[e]) ++e;
        rc = grouped_exact(ix, static_cast<const char*>(dev_Q) + (size_t)q * qbytes, e - q, k, metric, out.idx + (size_t)q * k, out.score + (size_t)q * k,
                           out.status + q, st);
        if (rc) return rc;
        st_exact += e - q;
        q = e;
    }
    ix->st.grouped = 1; ix->st.group_k = st_k; ix->st.group_rounds = st_rounds; ix->st.group_exact = st_exact;
    return hostrec_close(rec, st);
}

// ---- multi-vector queries: groups ranked by the sum over a set's vectors of the per-group maxima (hdb_maxsim.hip, hdb_maxsim_plan.h) ----
// The inverted index of the group ids, built on the first multi-vector call after hdb_index_set_groups and kept until the ids are
// replaced, cleared or dropped with the matrix.  One synchronisation: the two flag words decide what is built.  Ids that are
// non-decreasing by row are their own index (grp_sorted): only the offsets are built, grp_rows is not touched.
static int maxsim_index(hdb_index* ix, hipStream_t st) {
    if (ix->grp_valid) return HDB_OK;
    const int64_t n = ix->n, ng = ix->n_groups;
    if (n > 0xFFFFFFFFll) return fail(HDB_ERR_UNSUPPORTED, "hdb_maxsim_host: more than 2^32 - 1 rows are not built");
    HIP_TRY(ix->grp_flags.alloc(2));
    if ((size_t)ng + 1 > ix->grp_off.cap) HIP_TRY(ix->grp_off.alloc((size_t)(ng + ng / 4 + 64)));
    DevBuf<uint32_t> keys, keys_out, rows_in;
    DevBuf<char> temp;
    HIP_TRY(keys.alloc((size_t)n));
    HIP_TRY(hipMemsetAsync(ix->grp_flags, 0, 2 * sizeof(int), st));
    LAUNCH_TRY(hdb_launch_maxsim_keys(ix->groups, n, ng, keys, ix->grp_flags, st));
    int flags[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(flags, ix->grp_flags, sizeof(flags), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const bool sorted = flags[1] == 0;
    if (sorted) {
        LAUNCH_TRY(hdb_launch_maxsim_offsets(keys, n, ng, ix->grp_off, st));
    } else {
        size_t temp_bytes = 0;
        LAUNCH_TRY(hdb_maxsim_sort_temp_bytes(n, ng, &temp_bytes));
        if ((size_t)n > ix->grp_rows.cap) HIP_TRY(ix->grp_rows.alloc((size_t)(n + n / 4 + 64)));
        HIP_TRY(keys_out.alloc((size_t)n));
        HIP_TRY(rows_in.alloc((size_t)n));
        HIP_TRY(temp.alloc(std::max<size_t>(temp_bytes, 16)));
        LAUNCH_TRY(hdb_launch_maxsim_iota(rows_in, n, st));       // (the rows enter ascending: the stable sort keeps a group's rows in order)
        LAUNCH_TRY(hdb_launch_maxsim_sort(temp, temp_bytes, keys, keys_out, rows_in, ix->grp_rows, n, ng, st));
        LAUNCH_TRY(hdb_launch_maxsim_offsets(keys_out, n, ng, ix->grp_off, st));
    }
    HIP_TRY(hipStreamSynchronize(st));                 // (the temporaries go when this function returns)
    ix->grp_sorted = sorted; ix->grp_valid = true;
    return HDB_OK;
}

extern "C" int hdb_maxsim_host(hdb_index* ix, const void* dev_Q, const int32_t* host_off, int32_t ns, int32_t k, int metric, void* host_record,
                               void* stream) {
    // what the numbers alone decide, then the handle, then the device
    if (ns < 1) return fail(HDB_ERR_ARG, "hdb_maxsim_host: ns (query sets) must be positive");
    int rc = ranking_k("hdb_maxsim_host", k); if (rc) return rc;
    if (!host_off) return fail(HDB_ERR_ARG, "hdb_maxsim_host: null argument (host_off)");
    if (host_off[0] != 0) return fail(HDB_ERR_ARG, "hdb_maxsim_host: host_off[0] must be 0, got " + std::to_string(host_off[0]));
    for (int32_t s = 0; s < ns; ++s)
        if (host_off[s + 1] <= host_off[s])
            return fail(HDB_ERR_ARG, "hdb_maxsim_host: host_off must be strictly increasing: set " + std::to_string(s) + " is empty (host_off " +
                                         std::to_string(host_off[s]) + " -> " + std::to_string(host_off[s + 1]) + ")");
    if (!ix || !dev_Q || !host_record) return fail(HDB_ERR_ARG, "hdb_maxsim_host: null argument");
    if (!ix->groups) return fail(HDB_ERR_ARG, "hdb_maxsim_host: no groups set (hdb_index_set_groups)");
    rc = ranking_metric("hdb_maxsim_host", "multi-vector calls are", metric); if (rc) return rc;
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    const int32_t nv = host_off[ns];
    HostRec rec;
    rc = hostrec_open(ix->rec, ns, k, host_record, false, rec); if (rc) return rc;
    const PackedRec& out = rec.view;
    if (ix->n == 0) {
        stats_begin(ix, TopkStats()); ix->st.maxsim = 1;
        rc = run_empty(TopkArgs{dev_Q, ns, k, metric, out.idx, out.score, out.status, st}); if (rc) return rc;
        return hostrec_close(rec, st);
    }
    rc = maxsim_index(ix, st);
    if (rc) return rc;
    // the score pass: the exact shape of run_pipeline for the nv flat vectors, cut by the block / chunk plan
    TopkPlan p;
    rc = plan_call(ix, maxsim_call(nv, k, metric), p); if (rc) return rc;
    if (!maxsim_shape(p)) return fail(HDB_ERR_UNSUPPORTED, "hdb_maxsim_host: this call has no exact score pass");
    const int64_t n = ix->n, ng = ix->n_groups;
    const MaxsimPlan mp = maxsim_plan(n, ng, ns, p.ksplit ? 128 : 256, ix->opt.exact_bytes);
    p.cq_max = std::min<int>(mp.cq, nv);
    const int team = ix->opt.maxsim_team ? (int)ix->opt.maxsim_team : hdb_maxsim_team_rule(n, ng);
    stats_begin(ix, p.stats);          // (here, not sooner: the statistics are those of the plan as used)
    ix->st.maxsim = 1; ix->st.maxsim_team = team; ix->st.maxsim_sorted = ix->grp_sorted ? 1 : 0;
    ix->st.maxsim_chunks = maxsim_chunks(mp, host_off, ns); ix->st.chunks = ix->st.maxsim_chunks;
    MaxsimWs w;
    rc = ws_lay(ix, w, (int)nv, (int)ix->d, p.W, p.cq_max, p.ld_scores, p.ld_ks, mp.sb, mp.ld_g, (int)ns);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(w.voff, host_off, ((size_t)ns + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    TopkEnv e; e.w = w.t; e.sort_temp = 0;
    const TopkArgs c{dev_Q, nv, k, metric, out.idx, out.score, out.status, st};
    rc = topk_prologue(ix, c, p, e); if (rc) return rc;
    bool f32s = false;
    rc = exact_parts(ix, p, w.t.qnan, nv, st, f32s); if (rc) return rc;
    LAUNCH_TRY(hdb_launch_maxsim_setnan(w.t.qnan, w.voff, ns, w.snan, st));
    const uint32_t kk = (uint32_t)std::min<int64_t>(k, ng);
    bool q16_ready = p.q16_in_prep;
    for (int32_t s0 = 0; s0 < ns; s0 += mp.sb) {
        const int32_t sbn = std::min<int32_t>(mp.sb, ns - s0), v_end = host_off[s0 + sbn];
        int32_t s_cur = s0;
        for (int32_t v0 = host_off[s0]; v0 < v_end; v0 += p.cq_max) {
            const int cq = std::min<int32_t>(p.cq_max, v_end - v0);
            QueryBufs qb; ScanArgs a;
            rc = chunk_args(ix, p, e, f32s, nv, v0, cq, n, q16_ready, st, qb, a); if (rc) return rc;
            rc = score_chunk(ix, p, a, qb, cq, w.t.sbuf, st); if (rc) return rc;
            while (host_off[s_cur + 1] <= v0) ++s_cur;       // the set that holds vector v0
            LAUNCH_TRY(hdb_launch_maxsim_reduce(w.t.sbuf, p.ld_n, cq, v0, w.voff, s_cur, s0, ix->grp_off, ix->grp_rows, ix->grp_sorted ? 1 : 0, ng,
                                                w.acc, mp.ld_g, team, st));
        }
        // the block's selection: acc is a score matrix of sbn "queries" over n_groups "rows"; ids are group ids (row_base 0)
        rc = select_exact(w.acc, ng, mp.ld_g, sbn, 4, kk, w.cnt, w.hist, w.tie_info, w.cand, st); if (rc) return rc;
        LAUNCH_TRY(hdb_launch_finalize(w.cand, w.cnt, HDB_CAND_CAP, sbn, (uint32_t)k, kk, 0, out.idx + (int64_t)s0 * k, out.score + (int64_t)s0 * k,
                                       out.status + s0, w.snan + s0, (int)ix->opt.finalize_threads, 0, st));
        // (groups at -inf are never returned: padding; a bad group id anywhere in the index marks every set)
        LAUNCH_TRY(hdb_launch_group_finish(out.idx + (int64_t)s0 * k, out.score + (int64_t)s0 * k, sbn, k, out.status + s0, ix->grp_flags, st));
    }
    return hostrec_close(rec, st);
}

extern "C" int hdb_collapse_groups(const int64_t* dev_idx, const float* dev_score, int32_t nq, int32_t m, int32_t k, const int32_t* dev_groups,
                                   int64_t n_groups, int64_t n, int64_t row_base, int64_t* dev_idx_out, float* dev_score_out, int32_t* dev_status,
                                   int device, void* stream) {
    if (m < 1 || m > HDB_MAX_K) return fail(HDB_ERR_ARG, "hdb_collapse_groups: m (entries per query) must be in [1, 2048]");
    if (k < 1 || k > m) return fail(HDB_ERR_ARG, "hdb_collapse_groups: k must be in [1, m]");
    if (nq < 0) return fail(HDB_ERR_ARG, "hdb_collapse_groups: nq must be >= 0");
    if (n_groups < 1 || n_groups > 0x7FFFFFFFll || n < 0 || row_base < 0) return fail(HDB_ERR_ARG, "hdb_collapse_groups: need n_groups in [1, 2^31 - 1], n >= 0 and row_base >= 0");
    if (nq == 0) return HDB_OK;
    if (!dev_idx || !dev_score || !dev_groups || !dev_idx_out || !dev_score_out) return fail(HDB_ERR_ARG, "hdb_collapse_groups: null argument");
    HIP_TRY(hipSetDevice(device));
    LAUNCH_TRY(hdb_launch_group_collapse(dev_idx, dev_score, nq, m, k, dev_groups, n_groups, n, row_base, dev_idx_out, dev_score_out, dev_status,
                                         dev_status, HDB_Q_NAN, stream));
    return HDB_OK;
}

// ---- diverse top-k: maximal marginal relevance over a call's candidates (hdb_mmr.hip, hdb_mmr_plan.h) ---------------------------------
// What is decided from the numbers alone comes first, before the handle is looked at and before any HIP call.
static int mmr_sizes(const char* who, int32_t nq, int32_t m, int32_t k, double lambda, int pair_metric, bool host) {
    if (m < 1 || m > HDB_MAX_K) return fail(HDB_ERR_ARG, std::string(who) + ": m (entries per query) must be in [1, 2048]");
    if (k < 1 || k > m) return fail(HDB_ERR_ARG, std::string(who) + ": k must be in [1, m]");
    if (!(lambda >= 0.0 && lambda <= 1.0)) return fail(HDB_ERR_ARG, std::string(who) + ": lambda must be in [0, 1]");
    if (!mmr_pair_metric_ok(pair_metric)) return fail(HDB_ERR_UNSUPPORTED, std::string(who) + ": pair_metric must be dot, cosine or euclidean; the others are not built");
    if (host ? nq <= 0 : nq < 0) return fail(HDB_ERR_ARG, std::string(who) + (host ? ": nq must be positive" : ": nq must be >= 0"));
    return HDB_OK;
}
static int mmr_handle(const char* who, const hdb_index* ix) {
    if (!ix) return fail(HDB_ERR_ARG, std::string(who) + ": null index");
    if (ix->dtype == HDB_B1) return fail(HDB_ERR_UNSUPPORTED, std::string(who) + ": a packed-bit index is a first stage: pair similarity of packed bits is not built");
    return HDB_OK;
}
// Per chunk of queries: list preparation, the pair matrix, the selection.  status_in / status_out: [nq] or NULL, may be one array.
// The statistics of the call before it stay (hdb_mmr_host: those of its hdb_topk); the ranking flags become this call's.
static int mmr_impl(hdb_index* ix, const int64_t* dev_idx, const float* dev_score, int32_t nq, int32_t m, int32_t k, double lambda,
                    int pair_metric, int64_t* dev_idx_out, float* dev_score_out, const int32_t* status_in, int32_t* status_out, hipStream_t st) {
    const MmrPlan p = mmr_plan(nq, m, ix->opt.exact_bytes);
    MmrWs w;
    const int rc = ws_lay(ix, w, p.cq, p.mp);
    if (rc) return rc;
    ix->st.rerank = ix->st.grouped = ix->st.maxsim = 0;
    ix->st.mmr = 1; ix->st.mmr_chunks = 0;
    for (int q0 = 0; q0 < nq; q0 += p.cq) {
        const int cq = std::min(p.cq, nq - q0);
        LAUNCH_TRY(hdb_launch_mmr_prep(dev_idx + (int64_t)q0 * m, dev_score + (int64_t)q0 * m, cq, m, p.mp, ix->n, ix->row_base, w.rows, w.rel, w.cnt,
                                       status_in ? status_in + q0 : nullptr, status_out ? status_out + q0 : nullptr, st));
        LAUNCH_TRY(hdb_launch_mmr_pairs(ix->V, ix->dtype, ix->d, pair_metric, ix->inv_norm, w.rows, w.cnt, cq, p.mp, w.P, st));
        LAUNCH_TRY(hdb_launch_mmr_select(w.rows, w.rel, w.cnt, cq, p.mp, w.P, (float)lambda, k, ix->row_base, dev_idx_out + (int64_t)q0 * k,
                                         dev_score_out + (int64_t)q0 * k, st));
        ix->st.mmr_chunks++;
    }
    return HDB_OK;
}

extern "C" int hdb_mmr(hdb_index* ix, const int64_t* dev_idx, const float* dev_score, int32_t nq, int32_t m, int32_t k, double lambda,
                       int pair_metric, int64_t* dev_idx_out, float* dev_score_out, int32_t* dev_status, void* stream) {
    int rc = mmr_sizes("hdb_mmr", nq, m, k, lambda, pair_metric, false); if (rc) return rc;
    if (nq == 0) return HDB_OK;
    rc = mmr_handle("hdb_mmr", ix); if (rc) return rc;
    if (!dev_idx || !dev_score || !dev_idx_out || !dev_score_out) return fail(HDB_ERR_ARG, "hdb_mmr: null argument");
    HIP_TRY(hipSetDevice(ix->device));
    return mmr_impl(ix, dev_idx, dev_score, nq, m, k, lambda, pair_metric, dev_idx_out, dev_score_out, dev_status, dev_status, (hipStream_t)stream);
}

// hdb_topk of m rows per query into a device record of its own, its status words read back and the failed queries re-run exactly (as
// hdb_two_stage_host does for its first stage); the [nq][m] record then goes straight into the selection, whose answer is the
// caller's record.
extern "C" int hdb_mmr_host(hdb_index* ix, const void* dev_Q, int32_t nq, int32_t m, int32_t k, int metric, double lambda, int pair_metric,
                            void* host_record, void* stream) {
    int rc = mmr_sizes("hdb_mmr_host", nq, m, k, lambda, pair_metric, true); if (rc) return rc;
    rc = mmr_handle("hdb_mmr_host", ix); if (rc) return rc;
    if (!dev_Q || !host_record) return fail(HDB_ERR_ARG, "hdb_mmr_host: null argument");
    if ((int64_t)m > ix->n) return fail(HDB_ERR_ARG, "hdb_mmr_host: m must be at most min(2048, n)");
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    HostRec rec1;                                     // (the ranked lists stay on the device: opened, never closed)
    rc = hostrec_open(ix->rec1, nq, m, nullptr, false, rec1); if (rc) return rc;
    const PackedRec& r1 = rec1.view;
    rc = topk_impl(ix, dev_Q, nq, m, metric, r1.idx, r1.score, r1.status, stream, false); if (rc) return rc;
    std::vector<int32_t> h_st((size_t)nq);
    HIP_TRY(hipMemcpyAsync(h_st.data(), r1.status, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const TopkStats first_stats = ix->st;
    bool ran = false;
    rc = rerun_flagged(ix, dev_Q, nq, m, metric, r1, h_st.data(), st, &ran); if (rc) return rc;
    if (ran) ix->st = first_stats;                    // the rule of this call: it reports its first attempt, as hdb_two_stage_host does
    HostRec rec;
    rc = hostrec_open(ix->rec, nq, k, host_record, false, rec); if (rc) return rc;
    rc = mmr_impl(ix, r1.idx, r1.score, nq, m, k, lambda, pair_metric, rec.view.idx, rec.view.score, r1.status, rec.view.status, st); if (rc) return rc;
    return hostrec_close(rec, st);
}

extern "C" int hdb_merge_topk(const int64_t* dev_idx_parts, const float* dev_score_parts, int32_t parts, int32_t nq,
                              int32_t k, int64_t* dev_idx, float* dev_score, int device, void* stream) {
    if (!dev_idx_parts || !dev_score_parts || !dev_idx || !dev_score) return fail(HDB_ERR_ARG, "hdb_merge_topk: null argument");
    if (parts <= 0 || nq < 0 || k < 0) return fail(HDB_ERR_ARG, "hdb_merge_topk: bad sizes");
    if (nq == 0 || k == 0) return HDB_OK;
    if ((int64_t)parts * k > HDB_CAND_CAP) return fail(HDB_ERR_UNSUPPORTED, "hdb_merge_topk: parts*k exceeds 8192");
    HIP_TRY(hipSetDevice(device));
    LAUNCH_TRY(hdb_launch_merge(dev_idx_parts, (int64_t)nq * k * 8, dev_score_parts, (int64_t)nq * k * 4, nullptr, 0, parts, nq,
                                (uint32_t)k, dev_idx, dev_score, nullptr, stream));
    return HDB_OK;
}

extern "C" int64_t hdb_packed_bytes(int32_t nq, int32_t k) {
    const int64_t raw = (int64_t)nq * k * 12 + (int64_t)nq * 4;
    return (raw + 15) / 16 * 16;
}

extern "C" int hdb_merge_topk_packed(const void* dev_gathered, int32_t parts, int32_t nq, int32_t k, int64_t* dev_idx,
                                     float* dev_score, int32_t* dev_status, int device, void* stream) {
    if (!dev_gathered || !dev_idx || !dev_score) return fail(HDB_ERR_ARG, "hdb_merge_topk_packed: null argument");
    if (parts <= 0 || nq < 0 || k < 0) return fail(HDB_ERR_ARG, "hdb_merge_topk_packed: bad sizes");
    if (nq == 0 || k == 0) return HDB_OK;
    if ((int64_t)parts * k > HDB_CAND_CAP) return fail(HDB_ERR_UNSUPPORTED, "hdb_merge_topk_packed: parts*k exceeds 8192");
    HIP_TRY(hipSetDevice(device));
    const int64_t stride = hdb_packed_bytes(nq, k);
    const PackedRec r = packed_view(dev_gathered, nq, k);      // the first shard's; the others follow at `stride`
    LAUNCH_TRY(hdb_launch_merge(r.idx, stride, r.score, stride, r.status, stride, parts, nq, (uint32_t)k, dev_idx, dev_score, dev_status, stream));
    return HDB_OK;
}

extern "C" int hdb_recency_bias(const double* dev_ts, int64_t n, double recency_bias, double ts_max, float* dev_out,
                                int device, void* stream) {
    if (n < 0 || (n > 0 && (!dev_ts || !dev_out))) return fail(HDB_ERR_ARG, "hdb_recency_bias: null argument");
    if (n == 0) return HDB_OK;
    HIP_TRY(hipSetDevice(device));
    LAUNCH_TRY(hdb_launch_recency(dev_ts, n, recency_bias, ts_max, dev_out, stream));
    return HDB_OK;
}

extern "C" int hdb_recency_bias_twice(const double* dev_ts, const uint8_t* dev_mask, int64_t n, double recency_bias, double ts_max,
                                      double ts_min, float* dev_out, int device, void* stream) {
    if (n < 0 || (n > 0 && (!dev_ts || !dev_out))) return fail(HDB_ERR_ARG, "hdb_recency_bias_twice: null argument");
    if (n == 0) return HDB_OK;
    HIP_TRY(hipSetDevice(device));
    // max over the kept rows of first_i = rb * exp(-ts_max + ts_i): at the newest row for rb > 0 (exp(0) = 1), at the oldest for rb < 0
    const double first_max = recency_bias >= 0.0 ? recency_bias * std::exp(-ts_max + ts_max) : recency_bias * std::exp(-ts_max + ts_min);
    LAUNCH_TRY(hdb_launch_recency2(dev_ts, dev_mask, n, recency_bias, ts_max, first_max, dev_out, stream));
    return HDB_OK;
}

// ================================================================================================
// Single-process multi-GPU group: one row shard per entry (its own hdb_index, device and stream), queried together
// behind ONE call -- what HyperDB.query() (hyperdb/hyperdb.py:1584, a single-process call) needs to reach several
// GPUs without torchrun.  Per call:
//   calling thread: copies the queries into a pinned, portable staging buffer (every device can read it), publishes the job
//       (an atomic sequence number) and waits for the shards' arrival counter -- spinning first, a condition variable only
//       when a call takes longer than the spin window;
//   worker thread p (one per shard; between calls it spins on the sequence number for a short window, then parks on the
//       condition variable: a query stream never pays a futex wake-up): hdb_topk_host on the shard's own stream -- up to four
//       queries are read by the kernels straight from the staging buffer, larger batches go through one asynchronous copy --
//       which lets the shard's last kernel store its packed record STRAIGHT into slice p of a pinned, portable host buffer,
//       status words last, polls those words instead of waiting for the stream, and re-runs a failed threshold locally
//       through the exact selection (per-shard exactness is all the merge needs);
//   calling thread: k-way merge of the P records on the host (merge_host_records): no merge launch, no collective.
// The exchange unit is the same packed record as the multi-process path (hdb_packed_bytes); it is 1.2 KB per shard at
// nq=1, k=100, so the step is latency-bound and needs no collective library in-process.
// Shards that share a device (a test layout) must not run two single-launch pipelines at once -- each wants every CU for its
// in-kernel exchange -- so their calls take the multi-kernel pipeline; the shards' own handles keep their options.
// ================================================================================================
#include <thread>
#include <mutex>
#include <condition_variable>

struct hdb_group {
    int parts = 0;
    std::vector<hdb_index*> ix;
    std::vector<hipStream_t> st;
    std::vector<DevBuf<char>> qdev;                       // per shard: the device copy of a batch of more than four queries
    std::vector<char> shared_dev;                         // shard p shares its device with another shard of the group
    char* gather = nullptr; size_t gather_bytes = 0;     // pinned + portable host memory: parts records
    char* qpin = nullptr; size_t qpin_bytes = 0;         // pinned + portable host memory: the queries of the current call
    // workers
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable cv_job, cv_done;
    std::atomic<uint64_t> job_seq{0};
    std::atomic<int> pending{0};
    std::atomic<bool> stop{false};
    // current job (written before job_seq moves)
    size_t q_bytes = 0;
    int nq = 0, k = 0, metric = 0; size_t stride = 0;
    std::vector<int> rc;
    std::vector<std::string> err;
};

static constexpr long HDB_GROUP_SPIN_US = 200;           // how long a worker / the caller spins before it parks

static void group_worker(hdb_group* g, int p) {
    (void)hipSetDevice(g->ix[p]->device);
    uint64_t seen = 0;
    for (;;) {
        // wait for a job: spin for a short window (a query stream keeps the workers hot), then park
        bool got = false;
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned spins = 0;; ++spins) {
            if (g->stop.load(std::memory_order_acquire)) return;
            if (g->job_seq.load(std::memory_order_acquire) != seen) { got = true; break; }
            __builtin_ia32_pause();
            if ((spins & 255u) == 255u && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(HDB_GROUP_SPIN_US)) break;
        }
        if (!got) {
            std::unique_lock<std::mutex> lk(g->mu);
            g->cv_job.wait(lk, [&] { return g->stop.load(std::memory_order_acquire) || g->job_seq.load(std::memory_order_acquire) != seen; });
            if (g->stop.load(std::memory_order_acquire)) return;
        }
        seen = g->job_seq.load(std::memory_order_acquire);
        int rc = HDB_OK;
        std::string msg;
        hdb_index* ix = g->ix[p];
        hipStream_t st = g->st[p];
        if (ix->n > 0) {
            const void* dq = g->qpin;                                // up to four queries: the kernels read the pinned staging buffer
            if (g->nq > 4) {
                hipError_t e = hipSuccess;
                if (g->q_bytes > g->qdev[p].cap) e = g->qdev[p].alloc(g->q_bytes * 2);
                if (e == hipSuccess) e = hipMemcpyAsync(g->qdev[p], g->qpin, g->q_bytes, hipMemcpyHostToDevice, st);
                if (e != hipSuccess) { rc = HDB_ERR_HIP; msg = std::string("hdb_group: query upload: ") + hipGetErrorString(e); }
                dq = g->qdev[p];
            }
            if (rc == HDB_OK) {
                const int64_t saved = ix->opt.use_fused;
                if (g->shared_dev[p]) ix->opt.use_fused = 0;             // for this call only (one call in flight per handle)
                rc = hdb_topk_host(ix, dq, g->nq, g->k, g->metric, g->gather + (size_t)p * g->stride, st);
                ix->opt.use_fused = saved;
                if (rc != HDB_OK) msg = hdb_last_error();
            }
        } else {                                                     // an empty shard contributes padding
            const PackedRec r = packed_view(g->gather + (size_t)p * g->stride, g->nq, g->k);
            for (size_t i = 0; i < (size_t)g->nq * g->k; ++i) { r.idx[i] = -1; r.score[i] = -INFINITY; }
            for (int q = 0; q < g->nq; ++q) r.status[q] = 0;
        }
        g->rc[p] = rc; g->err[p] = msg;
        if (g->pending.fetch_sub(1, std::memory_order_acq_rel) == 1) {
            { std::lock_guard<std::mutex> lk(g->mu); }
            g->cv_done.notify_all();
        }
    }
}

extern "C" void hdb_group_destroy(hdb_group* g) {
    if (!g) return;
    g->stop.store(true, std::memory_order_release);
    { std::lock_guard<std::mutex> lk(g->mu); }
    g->cv_job.notify_all();
    for (auto& t : g->th) if (t.joinable()) t.join();
    for (int p = 0; p < (int)g->st.size(); ++p) {
        (void)hipSetDevice(g->ix[p]->device);
        if (g->st[p]) { (void)hipStreamSynchronize(g->st[p]); (void)hipStreamDestroy(g->st[p]); }
        if (p < (int)g->qdev.size()) g->qdev[p].reset();      // (on its own device)
    }
    if (g->gather) (void)hipHostFree(g->gather);
    if (g->qpin) (void)hipHostFree(g->qpin);
    delete g;
}

extern "C" int hdb_group_create(hdb_group** out, hdb_index* const* shards, int32_t parts) {
    if (!out || !shards) return fail(HDB_ERR_ARG, "hdb_group_create: null argument");
    if (parts < 1 || parts > 64) return fail(HDB_ERR_ARG, "hdb_group_create: 1..64 shards");
    for (int p = 0; p < parts; ++p) {
        if (!shards[p]) return fail(HDB_ERR_ARG, "hdb_group_create: null shard");
        if (shards[p]->d != shards[0]->d || shards[p]->dtype != shards[0]->dtype)
            return fail(HDB_ERR_ARG, "hdb_group_create: shards must share d and dtype");
    }
    hdb_group* g = new hdb_group();
    g->parts = parts;
    g->ix.assign(shards, shards + parts);
    g->st.assign(parts, nullptr); g->qdev = std::vector<DevBuf<char>>((size_t)parts);
    g->rc.assign(parts, 0); g->err.assign(parts, std::string());
    g->shared_dev.assign(parts, 0);
    for (int p = 0; p < parts; ++p)
        for (int r = 0; r < parts; ++r)
            if (r != p && g->ix[r]->device == g->ix[p]->device) g->shared_dev[p] = 1;
    hipError_t e = hipSuccess;
    for (int p = 0; p < parts && e == hipSuccess; ++p) {
        e = hipSetDevice(g->ix[p]->device);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&g->st[p], hipStreamNonBlocking);
    }
    if (e != hipSuccess) { hdb_group_destroy(g); return fail(HDB_ERR_HIP, std::string("hdb_group_create: ") + hipGetErrorString(e)); }
    for (int p = 0; p < parts; ++p) g->th.emplace_back(group_worker, g, p);
    *out = g;
    return HDB_OK;
}

static int group_pinned(char** buf, size_t* have, size_t need) {
    if (need <= *have) return HDB_OK;
    if (*buf) { HIP_TRY(hipHostFree(*buf)); *buf = nullptr; *have = 0; }
    need = align_up(need * 2, 4096);
    HIP_TRY(hipHostMalloc((void**)buf, need, hipHostMallocPortable | hipHostMallocMapped));
    *have = need;
    return HDB_OK;
}

extern "C" int hdb_group_topk_host(hdb_group* g, const void* host_Q, int32_t nq, int32_t k, int metric, void* host_record) {
    if (!g || !host_Q || !host_record) return fail(HDB_ERR_ARG, "hdb_group_topk_host: null argument");
    if (nq <= 0 || k <= 0) return fail(HDB_ERR_ARG, "hdb_group_topk_host: nq and k must be positive");
    const size_t bytes = (size_t)hdb_packed_bytes(nq, k);
    const size_t q_bytes = query_pitch(g->ix[0]) * nq;
    if (bytes * g->parts > g->gather_bytes || q_bytes > g->qpin_bytes) {      // (no call is in flight: the previous one returned)
        HIP_TRY(hipSetDevice(g->ix[0]->device));
        int rc = group_pinned(&g->gather, &g->gather_bytes, bytes * g->parts); if (rc) return rc;
        rc = group_pinned(&g->qpin, &g->qpin_bytes, q_bytes); if (rc) return rc;
    }
    memcpy(g->qpin, host_Q, q_bytes);
    g->q_bytes = q_bytes; g->nq = nq; g->k = k; g->metric = metric; g->stride = bytes;
    g->pending.store(g->parts, std::memory_order_release);
    g->job_seq.fetch_add(1, std::memory_order_acq_rel);
    { std::lock_guard<std::mutex> lk(g->mu); }
    g->cv_job.notify_all();
    // wait for the shards: spin (a shard-sized call takes ~0.2 ms), then park
    {
        const auto t0 = std::chrono::steady_clock::now();
        bool done = false;
        for (unsigned spins = 0;; ++spins) {
            if (g->pending.load(std::memory_order_acquire) == 0) { done = true; break; }
            __builtin_ia32_pause();
            if ((spins & 255u) == 255u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5)) break;
        }
        if (!done) {
            std::unique_lock<std::mutex> lk(g->mu);
            g->cv_done.wait(lk, [&] { return g->pending.load(std::memory_order_acquire) == 0; });
        }
    }
    for (int p = 0; p < g->parts; ++p)
        if (g->rc[p] != HDB_OK) return fail(g->rc[p], "shard " + std::to_string(p) + ": " + g->err[p]);
    std::vector<const char*> recs((size_t)g->parts);
    for (int p = 0; p < g->parts; ++p) recs[p] = g->gather + (size_t)p * g->stride;
    merge_host_records(recs.data(), g->parts, nq, k, host_record);
    return HDB_OK;
}
