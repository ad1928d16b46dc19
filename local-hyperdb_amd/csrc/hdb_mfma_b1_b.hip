// hdb_mfma_b1_b.hip -- the row scan of packed-bit matrices on the bf16 matrix pipe (hdb_mfma_b1.hip), d = 384 / 512.
#include "hdb_mfma_b1.h"

extern "C" int hdb_launch_mfma_scan_b1_wide(const ScanArgs* args, int mode, int nq_launch, const void* q, const float* sqnorm,
                                            const float* qsq, int blocks, void* stream) {
    const ScanArgs& a = *args;
    hipStream_t st = (hipStream_t)stream;
    switch (a.d) {
        case 384: return launch_b1<384>(a, mode, q, sqnorm, qsq, nq_launch, blocks, st);
        case 512: return launch_b1<512>(a, mode, q, sqnorm, qsq, nq_launch, blocks, st);
        default: return (int)hipErrorNotSupported;
    }
}
