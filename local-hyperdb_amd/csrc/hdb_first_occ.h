// hdb_first_occ.h -- first occurrences in a list, for one workgroup: which list positions hold a value that no earlier position
// holds.  One text for hdb_group_collapse_kernel (the value is a group id) and hdb_mmr_prep_kernel (the value is a local row).
#pragma once
#include "hdb_common.h"

#define HDB_FIRST_NONE 0xFFFFFFFFFFFFFFFFull      // a position that takes no part (padding, a bad id): sorts behind every key

// key[i] = (value << 32) | list position i, or HDB_FIRST_NONE; first[i] = 0; both filled for i < P and a barrier passed.  P: a power
// of two, at least 64; nt: threads of the workgroup.  The keys are sorted ascending in place (bitonic network), and a key that opens
// a run of equal values marks its list position in first[].  Ends behind a barrier: first[] may be read.
__device__ __forceinline__ void hdb_mark_first_occurrences(unsigned long long* key, uint8_t* first, int P, int tid, int nt) {
    for (int size = 2; size <= P; size <<= 1) {               // ascending: the sentinels end up behind the keys
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (P >> 1); t += nt) {
                const int i = ((t / stride) * (stride << 1)) + (t % stride), j = i + stride;
                const bool asc = (i & size) == 0;
                const unsigned long long x = key[i], y = key[j];
                if (asc ? (x > y) : (x < y)) { key[i] = y; key[j] = x; }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < P; i += nt) {
        const unsigned long long kx = key[i];
        if (kx != HDB_FIRST_NONE && (i == 0 || (uint32_t)(key[i - 1] >> 32) != (uint32_t)(kx >> 32))) first[(uint32_t)kx] = 1;
    }
    __syncthreads();
}
