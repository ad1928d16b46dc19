// hdb_range.hip -- range search (hdb_range_host; include/hyperdb_hip.h) for gfx950: every row at or above a score threshold.
//
// The exact score pass leaves the scores of a chunk of cq queries in sbuf[cq][ld_n] (bias added, masked rows and NaN at -inf).  This
// unit turns them into one variable-length segment per query without an atomic: a row passes when s >= thr[q] and s > -inf, and
// every passing row has ONE slot, computed from counts -- so the segments are row-ascending and the same bits on every run.
//
//   hdb_range_count_kernel    grid (tiles, queries), 256 threads: a workgroup owns HDB_RANGE_TILE = 4096 consecutive rows of one query,
//                             four rounds of one 16-byte load per thread.  Each wave counts with one ballot per element slot of
//                             the load (4 per round), the four wave totals meet in LDS: tcnt[q][tile].
//   hdb_range_offsets_kernel  one workgroup per query: exclusive scan of tcnt[q][*] in place (a run of tiles per thread, the 256 run
//                             totals scanned in LDS), qcnt[q] = the query's count.  The host reads qcnt back, checks the budget,
//                             grows the result buffer and writes the segment starts qoff[q].
//   hdb_range_emit_kernel     the count kernel's grid and tiling, the tile read again: the slot of a passing element is
//                             qoff[q] + tcnt[q][tile] + (passing elements of earlier rounds) + (of earlier waves in its round) +
//                             (of earlier lanes in its wave: the ballots below the lane) + (of earlier elements in its own load).
//                             It stores hdb_pack(s, row) there.
//   hdb_range_sort_kernel     one workgroup per query: a segment of 2 .. HDB_RANGE_LDS_SORT = 8192 keys goes through 64 KiB of LDS
//                             and the bitonic network of the finalize (descending on the packed key = score descending, row
//                             ascending; power-of-two bound, padding key 0 -- below every real key).  Shorter segments are in
//                             order already; longer ones are the cold path: rocPRIM's radix sort of the 64-bit keys, per segment.
//   hdb_range_unpack_kernel   packed keys -> idx (int64, row_base added) and score (float32), once per call over all entries.
//
// The kernels compare and count; they do no float arithmetic: -0 becomes +0 by its bits, NaN fails both comparisons.
#include <cstring>
#include "hdb_common.h"
#include "hdb_finalize.h"
#include "../../include/hyperdb_hip.h"
#include <rocprim/rocprim.hpp>

#define HDB_RANGE_THREADS 256
#define HDB_RANGE_ROUNDS (HDB_RANGE_TILE / (HDB_RANGE_THREADS * 4))
static_assert(HDB_RANGE_ROUNDS * HDB_RANGE_THREADS * 4 == HDB_RANGE_TILE, "a tile is whole rounds of one 16-byte load per thread");
static_assert(HDB_RANGE_LDS_SORT == HDB_CAND_CAP && (HDB_RANGE_LDS_SORT & (HDB_RANGE_LDS_SORT - 1)) == 0, "the LDS sort takes a power of two: the finalize's 8192");

// The four scores of thread `tid`'s load in round r of a tile, and which of them pass: bit e of the result is element e.  Columns
// from n to ld_n (ld_n is a multiple of 4, so a load is inside the row or not at all) and the rows past n never pass.
__device__ __forceinline__ uint32_t hdb_range_load(const float* sq, int64_t row0, int64_t n, int64_t ld_n, float thr, uint32_t (&bits)[4]) {
    uint32_t m = 0;
    bits[0] = bits[1] = bits[2] = bits[3] = 0u;
    if (row0 < ld_n) {
        const uint4 v = *reinterpret_cast<const uint4*>(sq + row0);
        bits[0] = v.x; bits[1] = v.y; bits[2] = v.z; bits[3] = v.w;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (bits[e] == 0x80000000u) bits[e] = 0u;                      // -0 -> +0: equal floats, equal keys
            const float s = __uint_as_float(bits[e]);
            if (row0 + e < n && s >= thr && s > -INFINITY) m |= 1u << e;   // (NaN fails both)
        }
    }
    return m;
}

__global__ __launch_bounds__(HDB_RANGE_THREADS) void hdb_range_count_kernel(const float* sbuf, int64_t ld_n, int64_t n, const float* thr,
                                                                            int64_t ntiles, uint32_t* tcnt) {
    __shared__ uint32_t wsum[HDB_RANGE_THREADS / 64];
    const int q = blockIdx.y, tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const float* sq = sbuf + (int64_t)q * ld_n;
    const float t = thr[q];
    uint32_t wave_total = 0;                                               // (wave-uniform: every lane sees the same ballots)
#pragma unroll
    for (int r = 0; r < HDB_RANGE_ROUNDS; ++r) {
        uint32_t bits[4];
        const uint32_t m = hdb_range_load(sq, tile * HDB_RANGE_TILE + ((int64_t)r * HDB_RANGE_THREADS + tid) * 4, n, ld_n, t, bits);
#pragma unroll
        for (int e = 0; e < 4; ++e) wave_total += (uint32_t)__popcll(__ballot((m >> e) & 1u));
    }
    if ((tid & 63) == 0) wsum[tid >> 6] = wave_total;
    __syncthreads();
    if (tid == 0) {
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < HDB_RANGE_THREADS / 64; ++w) c += wsum[w];
        tcnt[(int64_t)q * ntiles + tile] = c;
    }
}

__global__ __launch_bounds__(256) void hdb_range_offsets_kernel(uint32_t* tcnt, int64_t ntiles, uint32_t* qcnt) {
    __shared__ uint32_t run[256];
    const int q = blockIdx.x, tid = threadIdx.x;
    uint32_t* tq = tcnt + (int64_t)q * ntiles;
    const int64_t per = (ntiles + 255) / 256, lo = tid * per < ntiles ? tid * per : ntiles, hi = lo + per < ntiles ? lo + per : ntiles;
    uint32_t mine = 0;
    for (int64_t i = lo; i < hi; ++i) mine += tq[i];
    run[tid] = mine;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {                                     // inclusive scan of the 256 run totals
        const uint32_t add = tid >= o ? run[tid - o] : 0u;
        __syncthreads();
        run[tid] += add;
        __syncthreads();
    }
    uint32_t at = run[tid] - mine;                                          // exclusive: what lies before this thread's run
    for (int64_t i = lo; i < hi; ++i) { const uint32_t c = tq[i]; tq[i] = at; at += c; }
    if (tid == 255) qcnt[q] = run[255];
}

__global__ __launch_bounds__(HDB_RANGE_THREADS) void hdb_range_emit_kernel(const float* sbuf, int64_t ld_n, int64_t n, const float* thr,
                                                                           int64_t ntiles, const uint32_t* toff, const int64_t* qoff,
                                                                           unsigned long long* keys) {
    constexpr int WAVES = HDB_RANGE_THREADS / 64;
    __shared__ uint32_t part[HDB_RANGE_ROUNDS][WAVES];                      // passing elements of wave w in round r
    const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t tile = blockIdx.x;
    const float* sq = sbuf + (int64_t)q * ld_n;
    const float t = thr[q];
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t bits[HDB_RANGE_ROUNDS][4], pass[HDB_RANGE_ROUNDS], before[HDB_RANGE_ROUNDS];
#pragma unroll
    for (int r = 0; r < HDB_RANGE_ROUNDS; ++r) {
        pass[r] = hdb_range_load(sq, tile * HDB_RANGE_TILE + ((int64_t)r * HDB_RANGE_THREADS + tid) * 4, n, ld_n, t, bits[r]);
        uint32_t total = 0, mine = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned long long b = __ballot((pass[r] >> e) & 1u);
            total += (uint32_t)__popcll(b);
            mine += (uint32_t)__popcll(b & below);
        }
        before[r] = mine;                                                   // of earlier lanes of this wave, this round
        if (lane == 0) part[r][wave] = total;
    }
    __syncthreads();
    const int64_t base = qoff[q] + (int64_t)toff[(int64_t)q * ntiles + tile];
    uint32_t sofar = 0;                                                     // of earlier rounds, and of earlier waves in this one
#pragma unroll
    for (int r = 0; r < HDB_RANGE_ROUNDS; ++r) {
        uint32_t at = sofar + before[r];
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            if (w < wave) at += part[r][w];
            sofar += part[r][w];
        }
        const int64_t row0 = tile * HDB_RANGE_TILE + ((int64_t)r * HDB_RANGE_THREADS + tid) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if ((pass[r] >> e) & 1u) keys[base + at++] = hdb_pack(__uint_as_float(bits[r][e]), (uint32_t)(row0 + e));
    }
}

// qoff: cq + 1 segment starts.  Dynamic LDS: HDB_RANGE_LDS_SORT keys.
__global__ __launch_bounds__(1024) void hdb_range_sort_kernel(unsigned long long* keys, const int64_t* qoff) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long buf[];
    const int64_t lo = qoff[blockIdx.x], cnt = qoff[blockIdx.x + 1] - lo;
    if (cnt < 2 || cnt > HDB_RANGE_LDS_SORT) return;                        // (block-uniform) in order already / the cold path
    int P = 2;
    while (P < (int)cnt) P <<= 1;
    for (int i = threadIdx.x; i < P; i += blockDim.x) buf[i] = i < (int)cnt ? keys[lo + i] : 0ull;
    __syncthreads();
    hdb_bitonic_desc(buf, P);
    for (int i = threadIdx.x; i < (int)cnt; i += blockDim.x) keys[lo + i] = buf[i];
}

__global__ __launch_bounds__(256) void hdb_range_unpack_kernel(const unsigned long long* keys, int64_t total, int64_t row_base, int64_t* idx,
                                                               float* score) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const unsigned long long k = keys[i];
        idx[i] = row_base + (int64_t)(0xFFFFFFFFu - (uint32_t)k);
        score[i] = hdb_key2f((uint32_t)(k >> 32));
    }
}

static bool range_grid_ok(int64_t n, int64_t ld_n, int cq, int64_t ntiles) {
    return n >= 1 && n <= 0xFFFFFFFFll && ld_n >= n && ld_n % 4 == 0 && cq >= 1 && cq <= 65535 && ntiles >= 1 && ntiles <= 0x7FFFFFFFll &&
           ntiles * HDB_RANGE_TILE >= n && (ntiles - 1) * HDB_RANGE_TILE < n;
}

extern "C" int hdb_launch_range_count(const float* sbuf, int64_t ld_n, int64_t n, int cq, const float* thr, int64_t ntiles, uint32_t* tcnt,
                                      void* stream) {
    if (!range_grid_ok(n, ld_n, cq, ntiles) || !sbuf || !thr || !tcnt) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(hdb_range_count_kernel, dim3((unsigned)ntiles, (unsigned)cq), dim3(HDB_RANGE_THREADS), 0, (hipStream_t)stream, sbuf, ld_n, n,
                       thr, ntiles, tcnt);
    return (int)hipGetLastError();
}

extern "C" int hdb_launch_range_offsets(uint32_t* tcnt, int64_t ntiles, int cq, uint32_t* qcnt, void* stream) {
    if (cq < 1 || ntiles < 1 || !tcnt || !qcnt) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(hdb_range_offsets_kernel, dim3((unsigned)cq), dim3(256), 0, (hipStream_t)stream, tcnt, ntiles, qcnt);
    return (int)hipGetLastError();
}

extern "C" int hdb_launch_range_emit(const float* sbuf, int64_t ld_n, int64_t n, int cq, const float* thr, int64_t ntiles, const uint32_t* toff,
                                     const int64_t* qoff, unsigned long long* keys, void* stream) {
    if (!range_grid_ok(n, ld_n, cq, ntiles) || !sbuf || !thr || !toff || !qoff || !keys) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(hdb_range_emit_kernel, dim3((unsigned)ntiles, (unsigned)cq), dim3(HDB_RANGE_THREADS), 0, (hipStream_t)stream, sbuf, ld_n, n,
                       thr, ntiles, toff, qoff, keys);
    return (int)hipGetLastError();
}

extern "C" int hdb_launch_range_sort(unsigned long long* keys, const int64_t* qoff, int cq, void* stream) {
    if (cq < 1 || !keys || !qoff) return (int)hipErrorInvalidValue;
    const size_t lds = (size_t)HDB_RANGE_LDS_SORT * sizeof(unsigned long long);
    static unsigned long long attr_done = 0;
    const hipError_t e = hdb_lds_attr_once(reinterpret_cast<const void*>(hdb_range_sort_kernel), (int)lds, &attr_done);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(hdb_range_sort_kernel, dim3((unsigned)cq), dim3(1024), lds, (hipStream_t)stream, keys, qoff);
    return (int)hipGetLastError();
}

// The cold path: one segment of cnt > HDB_RANGE_LDS_SORT keys, sorted descending through `out` (cnt keys) and copied back.
extern "C" int hdb_range_sort_temp_bytes(int64_t cnt, size_t* bytes) {
    unsigned long long* p = nullptr;
    size_t b = 0;
    const hipError_t e = rocprim::radix_sort_keys_desc(nullptr, b, p, p, (size_t)cnt, 0, 64, (hipStream_t)0);
    *bytes = b;
    return (int)e;
}
extern "C" int hdb_launch_range_sort_long(void* temp, size_t temp_bytes, unsigned long long* keys, unsigned long long* out, int64_t cnt,
                                          void* stream) {
    if (cnt < 1 || !keys || !out) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = rocprim::radix_sort_keys_desc(temp, temp_bytes, keys, out, (size_t)cnt, 0, 64, st);
    if (e != hipSuccess) return (int)e;
    e = hipMemcpyAsync(keys, out, (size_t)cnt * sizeof(unsigned long long), hipMemcpyDeviceToDevice, st);
    return (int)e;
}

extern "C" int hdb_launch_range_unpack(const unsigned long long* keys, int64_t total, int64_t row_base, int64_t* idx, float* score, void* stream) {
    if (total < 1 || !keys || !idx || !score) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(hdb_range_unpack_kernel, dim3(hdb_grid_for(total, 256, 4096)), dim3(256), 0, (hipStream_t)stream, keys, total, row_base, idx,
                       score);
    return (int)hipGetLastError();
}
