// hdb_mfma_bf16_ks_b.hip -- the K slices of wide bfloat16 rows (hdb_mfma_bf16_ks.hip), slices of 512 elements.
#include "hdb_mfma_kernel.h"

extern "C" int hdb_launch_mfma_kslice_bf16_wide(const ScanArgs* a, int dslice, int mode, int nq_launch, const void* q, const float* sqnorm,
                                                const float* qsq, int blocks, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (dslice == 512) return launch_kslice<hdb_bf16, 512, 16>(*a, mode, q, sqnorm, qsq, nullptr, nq_launch, blocks, st);
    return (int)hipErrorNotSupported;
}
