// hdb_mfma_f8_lds_ks_b.hip -- the 512-element K slice of float8 e4m3 rows expanded to bf16 in LDS (hdb_mfma_f8_lds.h, KSL; see
// hdb_mfma_f8_lds_ks.hip): 192 registers of query parts.  A translation unit of its own so that the instantiations compile in parallel.
#include "hdb_mfma_f8_lds.h"

extern "C" int hdb_launch_mfma_kslice_f8_lds_wide(const ScanArgs* a, int dslice, int mode, int nq_launch, const void* q, const float* sqnorm,
                                                  const float* qsq, int blocks, void* stream) {
    if (dslice == 512) return launch_f8_lds_kslice<512>(*a, mode, q, sqnorm, qsq, nq_launch, blocks, (hipStream_t)stream);
    return (int)hipErrorNotSupported;
}
