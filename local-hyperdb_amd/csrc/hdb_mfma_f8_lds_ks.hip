// hdb_mfma_f8_lds_ks.hip -- the K slices of float8 e4m3 rows wider than 512 elements (hdb_mfma_ksplit.hip, ks_geom_f8; f8_ks_min_q)
// with every slice expanded to bf16 in LDS once per workgroup (hdb_mfma_f8_lds.h, KSL; f8_lds_min_q): one slice of 256, 384 or 512
// elements per launch, the partial sums indexed by the tile sequence as in hdb_mfma_f8_ks.hip, whatever the slice's stage height.
// Slices of 256 / 384 here, 512 in hdb_mfma_f8_lds_ks_b.hip.
#include "hdb_mfma_f8_lds.h"

extern "C" int hdb_launch_mfma_kslice_f8_lds(const ScanArgs* a, int dslice, int mode, int nq_launch, const void* q, const float* sqnorm,
                                             const float* qsq, int blocks, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (dslice == 256) return launch_f8_lds_kslice<256>(*a, mode, q, sqnorm, qsq, nq_launch, blocks, st);
    if (dslice == 384) return launch_f8_lds_kslice<384>(*a, mode, q, sqnorm, qsq, nq_launch, blocks, st);
    return hdb_launch_mfma_kslice_f8_lds_wide(a, dslice, mode, nq_launch, q, sqnorm, qsq, blocks, stream);
}
