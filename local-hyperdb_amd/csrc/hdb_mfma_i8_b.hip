// hdb_mfma_i8_b.hip -- int8 rows on the bf16 matrix pipe (hdb_mfma_i8.hip), d = 384 and d = 512.
#include "hdb_mfma_f8.h"

extern "C" int hdb_launch_mfma_scan_i8_wide(const ScanArgs* args, int mode, int nq_launch, const void* q, const float* sqnorm,
                                            const float* qsq, int blocks, void* stream) {
    const ScanArgs& a = *args;
    hipStream_t st = (hipStream_t)stream;
    switch (a.d) {
        case 384: return launch_f8<384, HdbRowCvtI8>(a, mode, q, sqnorm, qsq, nq_launch, blocks, st);
        case 512: return launch_f8<512, HdbRowCvtI8>(a, mode, q, sqnorm, qsq, nq_launch, blocks, st);
        default: return (int)hipErrorNotSupported;
    }
}
