// hdb_mfma_f4.hip -- the row scan of MXFP4 matrices (HDB_MXF4) on the bf16 matrix pipe (hdb_mfma_f4.h; opt-in, b1_mfma_min_q): one
// 16-byte load per MX block, codes converted to bf16 with the block scale applied per fragment in registers, float32 queries as three
// exact bf16 parts in the same K permutation, the bfloat16 flavour's epilogue.  Multi-kernel pipeline only: MODE 0 (scores) and MODE 1
// (filter).  d = 128 / 256 here, 384 / 512 in hdb_mfma_f4_b.hip; and the euclidean re-score of MXFP4 candidates.
#include "hdb_mfma_f4.h"

extern "C" int hdb_launch_mfma_scan_f4(const ScanArgs* args, const MfmaLaunch* l) {
    const ScanArgs& a = *args;
    switch (a.d) {
        case 128: return launch_f4<128>(a, *l);
        case 256: return launch_f4<256>(a, *l);
        default: return hdb_launch_mfma_scan_f4_wide(args, l);
    }
}

// hdb_launch_rescore_euclid's case for HDB_MXF4 rows: any d that is a row (a multiple of 32), the bias flavour
extern "C" int hdb_launch_rescore_euclid_f4(unsigned long long* cand, const uint32_t* cnt, uint32_t cap, int nq_launch, const void* V, int d,
                                            const float* Q, const float* qsq, int q0, const float* bias, void* stream) {
    const int pitch = (int)hdb_row_bytes(HDB_MXF4, d);
    if (pitch <= 0 || (reinterpret_cast<uintptr_t>(V) & 15) != 0 || nq_launch < 1) return (int)hipErrorNotSupported;
    auto kern = bias ? hdb_rescore_euclid_f4_kernel<true> : hdb_rescore_euclid_f4_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(64, nq_launch), dim3(256), 0, (hipStream_t)stream, cand, cnt, cap, (const char*)V, d, pitch, Q, qsq, q0, bias);
    return (int)hipGetLastError();
}
