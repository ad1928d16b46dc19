// hdb_mfma_f8_ks_b.hip -- the K slices of float8 e4m3 rows (hdb_mfma_f8_ks.hip), slices of 512 elements.
#include "hdb_mfma_f8.h"

extern "C" int hdb_launch_mfma_kslice_f8_wide(const ScanArgs* a, int dslice, int mode, int nq_launch, const void* q, const float* sqnorm,
                                              const float* qsq, int blocks, void* stream) {
    if (dslice != 512) return (int)hipErrorNotSupported;
    return launch_f8_kslice<512>(*a, mode, q, sqnorm, qsq, nq_launch, blocks, (hipStream_t)stream);
}
