// hdb_maxsim.hip -- multi-vector queries (hdb_maxsim_host; include/hyperdb_hip.h) for gfx950.
//
// A query is a set of T vectors, a document a group of rows; score(set, g) = sum over the set's vectors of max over the rows of g
// of the exact score.  The exact score pass leaves the scores of a chunk of vectors in sbuf[cq][ld_n]; this unit turns them into
// acc[set][g] without an atomic: every group has ONE owner, which reads the group's rows through an inverted index of the ids.
//
//   hdb_maxsim_keys_kernel     the inverted index, step 1: key[r] = group id of row r, or n_groups -- behind every group -- where the id
//                              is outside [0, n_groups) (flags[0] is raised: nothing is ever indexed with such an id); flags[1] is
//                              raised where the keys are not non-decreasing by row.  Non-decreasing keys are their own sort: the
//                              index is the identity and only the offsets are built.
//   hdb_maxsim_iota_kernel     other layouts: rows = 0 .. n - 1, the values of the sort.
//   (rocPRIM radix sort)       step 2, other layouts: (key, row) pairs sorted by key; stable and the rows enter ascending, so a
//                              group's rows stay in ascending order -- grp_rows.
//   hdb_maxsim_offsets_kernel  step 3: grp_off[g] = first position whose key is >= g, g = 0 .. n_groups (binary search; an empty
//                              group gets an empty range, the rows with a bad id lie behind grp_off[n_groups]).
//   hdb_maxsim_reduce_kernel   <TEAM, SORTED>: a team of TEAM lanes owns one group.  For every vector of the chunk its lanes stride
//                              over the group's rows and take the maximum (shuffles inside the team); lane 0 adds it to the running
//                              sum of the vector's set: one float32 add per vector, in vector order.  The sum lives in a register
//                              while the set does not change; it is loaded from acc at the chunk's start where the chunk begins
//                              inside a set and stored at set ends (through hdb_canon) and at the chunk's end.  SORTED reads
//                              sbuf[t][grp_off[g] ..] directly, the other flavour through grp_rows.
//   hdb_maxsim_setnan_kernel   snan[s] = 1 where a vector of set s holds a NaN: the finalize turns it into HDB_Q_NAN.
//
// Every TEAM is correct for every group size; a group far larger than its team is slow (one team walks all of it), which is the
// "splitting one huge group over teams" of the header's Not-built list.
#include <cstring>
#include "hdb_common.h"
#include "../../include/hyperdb_hip.h"
#include <rocprim/rocprim.hpp>
#include <algorithm>

__global__ __launch_bounds__(256) void hdb_maxsim_keys_kernel(const int32_t* groups, int64_t n, int32_t n_groups, uint32_t* keys, int* flags) {
    bool bad = false, unsorted = false;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        const int32_t g = groups[r];
        const bool ok = (uint32_t)g < (uint32_t)n_groups;
        const uint32_t key = ok ? (uint32_t)g : (uint32_t)n_groups;
        bad |= !ok;
        if (r > 0) {
            const int32_t pg = groups[r - 1];
            const uint32_t pkey = (uint32_t)pg < (uint32_t)n_groups ? (uint32_t)pg : (uint32_t)n_groups;
            unsorted |= pkey > key;
        }
        keys[r] = key;
    }
    if (bad) atomicOr(flags, 1);
    if (unsorted) atomicOr(flags + 1, 1);
}

__global__ __launch_bounds__(256) void hdb_maxsim_iota_kernel(uint32_t* rows, int64_t n) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) rows[r] = (uint32_t)r;
}

__global__ __launch_bounds__(256) void hdb_maxsim_offsets_kernel(const uint32_t* keys, int64_t n, int32_t n_groups, uint32_t* grp_off) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g <= (int64_t)n_groups; g += (int64_t)gridDim.x * 256) {
        int64_t lo = 0, hi = n;                             // first position with keys[pos] >= g
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)keys[mid] < g) lo = mid + 1; else hi = mid;
        }
        grp_off[g] = (uint32_t)lo;
    }
}

__global__ __launch_bounds__(256) void hdb_maxsim_setnan_kernel(const int* qnan, const int32_t* voff, int ns, int* snan) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= ns) return;
    int any = 0;
    for (int32_t v = voff[s]; v < voff[s + 1]; ++v) any |= qnan[v] & 1;
    snan[s] = any;
}

// sbuf: [cq][ld_n] scores of the vectors v0 .. v0 + cq - 1 of the call (bias added, masked rows and NaN at -inf); voff: the call's set
// offsets [ns + 1] on the device; s_first: the set that holds vector v0; s_base: the first set of acc, [sets][ld_g].  Slots
// [n_groups, ld_g) of a set's row are padding: written as -inf, never read through the index.
template <int TEAM, bool SORTED>
__global__ __launch_bounds__(256) void hdb_maxsim_reduce_kernel(const float* sbuf, int64_t ld_n, int cq, int32_t v0, const int32_t* voff,
                                                                int32_t s_first, int32_t s_base, const uint32_t* grp_off,
                                                                const uint32_t* grp_rows, int32_t n_groups, float* acc, int64_t ld_g) {
    const int64_t slot = ((int64_t)blockIdx.x * 256 + threadIdx.x) / TEAM;
    const int tl = threadIdx.x & (TEAM - 1);
    const bool live = slot < (int64_t)n_groups;            // a group; else padding (slot < ld_g) or nothing
    const bool writer = tl == 0 && slot < ld_g;
    int64_t lo = 0, hi = 0;
    if (live) { lo = grp_off[slot]; hi = grp_off[slot + 1]; }
    int32_t s = s_first;
    int32_t s_end = voff[s + 1];
    bool fresh = v0 == voff[s];                             // the chunk starts a set: the first term is the sum
    float sum = -INFINITY;
    if (!fresh && writer) sum = acc[(int64_t)(s - s_base) * ld_g + slot];
    for (int t = 0; t < cq; ++t) {                          // (uniform: every lane of a team takes part in the shuffles)
        const float* sq = sbuf + (int64_t)t * ld_n;
        float m = -INFINITY;
        for (int64_t i = lo + tl; i < hi; i += TEAM) {
            const int64_t r = SORTED ? i : (int64_t)grp_rows[i];
            m = fmaxf(m, hdb_canon(sq[r]));
        }
#pragma unroll
        for (int o = TEAM >> 1; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        sum = fresh ? m : sum + m;
        fresh = false;
        if (v0 + t + 1 == s_end) {                          // the set is complete
            if (writer) acc[(int64_t)(s - s_base) * ld_g + slot] = live ? hdb_canon(sum) : -INFINITY;
            ++s;
            if (t + 1 < cq) s_end = voff[s + 1];
            fresh = true;
        }
    }
    if (!fresh && writer) acc[(int64_t)(s - s_base) * ld_g + slot] = sum;       // the set goes on in the next chunk
}

static int maxsim_key_bits(int64_t n_groups) {             // keys are 0 .. n_groups
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) <= n_groups) ++bits;
    return bits;
}

extern "C" int hdb_maxsim_sort_temp_bytes(int64_t n, int64_t n_groups, size_t* bytes) {
    uint32_t* p = nullptr;
    size_t b = 0;
    const hipError_t e = rocprim::radix_sort_pairs(nullptr, b, p, p, p, p, (size_t)n, 0, maxsim_key_bits(n_groups), (hipStream_t)0);
    *bytes = b;
    return (int)e;
}

extern "C" int hdb_launch_maxsim_keys(const int32_t* groups, int64_t n, int64_t n_groups, uint32_t* keys, int* flags, void* stream) {
    if (n < 1 || n > 0xFFFFFFFFll || n_groups < 1 || n_groups > 0x7FFFFFFFll || !groups || !keys || !flags) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(hdb_maxsim_keys_kernel, dim3(hdb_grid_for(n, 256, 4096)), dim3(256), 0, (hipStream_t)stream, groups, n, (int32_t)n_groups,
                       keys, flags);
    return (int)hipGetLastError();
}

extern "C" int hdb_launch_maxsim_iota(uint32_t* rows, int64_t n, void* stream) {
    if (n < 1 || n > 0xFFFFFFFFll || !rows) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(hdb_maxsim_iota_kernel, dim3(hdb_grid_for(n, 256, 4096)), dim3(256), 0, (hipStream_t)stream, rows, n);
    return (int)hipGetLastError();
}

extern "C" int hdb_launch_maxsim_sort(void* temp, size_t temp_bytes, uint32_t* keys_in, uint32_t* keys_out, uint32_t* rows_in, uint32_t* rows_out,
                                      int64_t n, int64_t n_groups, void* stream) {
    if (n < 1 || n_groups < 1) return (int)hipErrorInvalidValue;
    return (int)rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, rows_in, rows_out, (size_t)n, 0, maxsim_key_bits(n_groups),
                                          (hipStream_t)stream);
}

extern "C" int hdb_launch_maxsim_offsets(const uint32_t* keys, int64_t n, int64_t n_groups, uint32_t* grp_off, void* stream) {
    if (n < 1 || n_groups < 1 || n_groups > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(hdb_maxsim_offsets_kernel, dim3(hdb_grid_for(n_groups + 1, 256, 4096)), dim3(256), 0, (hipStream_t)stream, keys, n,
                       (int32_t)n_groups, grp_off);
    return (int)hipGetLastError();
}

extern "C" int hdb_launch_maxsim_setnan(const int* qnan, const int32_t* voff, int ns, int* snan, void* stream) {
    if (ns < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(hdb_maxsim_setnan_kernel, dim3((ns + 255) / 256), dim3(256), 0, (hipStream_t)stream, qnan, voff, ns, snan);
    return (int)hipGetLastError();
}

template <int TEAM>
static int maxsim_reduce_launch(bool sorted, dim3 grid, hipStream_t st, const float* sbuf, int64_t ld_n, int cq, int32_t v0, const int32_t* voff,
                                int32_t s_first, int32_t s_base, const uint32_t* grp_off, const uint32_t* grp_rows, int32_t n_groups, float* acc,
                                int64_t ld_g) {
    if (sorted)
        hipLaunchKernelGGL((hdb_maxsim_reduce_kernel<TEAM, true>), grid, dim3(256), 0, st, sbuf, ld_n, cq, v0, voff, s_first, s_base, grp_off,
                           grp_rows, n_groups, acc, ld_g);
    else
        hipLaunchKernelGGL((hdb_maxsim_reduce_kernel<TEAM, false>), grid, dim3(256), 0, st, sbuf, ld_n, cq, v0, voff, s_first, s_base, grp_off,
                           grp_rows, n_groups, acc, ld_g);
    return (int)hipGetLastError();
}

extern "C" int hdb_launch_maxsim_reduce(const float* sbuf, int64_t ld_n, int cq, int32_t v0, const int32_t* voff, int32_t s_first, int32_t s_base,
                                        const uint32_t* grp_off, const uint32_t* grp_rows, int sorted, int64_t n_groups, float* acc, int64_t ld_g,
                                        int team, void* stream) {
    if (cq < 1 || n_groups < 1 || n_groups > 0x7FFFFFFFll || ld_g < n_groups || s_first < s_base || !grp_off || (!sorted && !grp_rows))
        return (int)hipErrorInvalidValue;
    if (team != 1 && team != 4 && team != 16 && team != 64) return (int)hipErrorInvalidValue;
    const int64_t blocks = (ld_g * team + 255) / 256;       // one team per slot of acc's row
    if (blocks > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks);
    hipStream_t st = (hipStream_t)stream;
    const int32_t ng = (int32_t)n_groups;
    switch (team) {
    case 1: return maxsim_reduce_launch<1>(sorted != 0, grid, st, sbuf, ld_n, cq, v0, voff, s_first, s_base, grp_off, grp_rows, ng, acc, ld_g);
    case 4: return maxsim_reduce_launch<4>(sorted != 0, grid, st, sbuf, ld_n, cq, v0, voff, s_first, s_base, grp_off, grp_rows, ng, acc, ld_g);
    case 16: return maxsim_reduce_launch<16>(sorted != 0, grid, st, sbuf, ld_n, cq, v0, voff, s_first, s_base, grp_off, grp_rows, ng, acc, ld_g);
    default: return maxsim_reduce_launch<64>(sorted != 0, grid, st, sbuf, ld_n, cq, v0, voff, s_first, s_base, grp_off, grp_rows, ng, acc, ld_g);
    }
}
