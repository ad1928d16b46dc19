// hdb_mfma_1k.hip -- instantiations of the MFMA row scan (hdb_mfma_kernel.h) for fp16 d = 1024 and 1536 (16-row stages): a translation unit of its own so that
// the geometries compile in parallel (each carries 3 modes x 3 metrics x {bias, no bias} kernels).
#include "hdb_mfma_kernel.h"

extern "C" int hdb_launch_mfma_scan_f16_1k(const ScanArgs* args, const MfmaLaunch* l) {
    const ScanArgs& a = *args;
    if (a.d == 1024) return launch_mode<_Float16, 16, 1, 1024, 16>(a, *l);
    if (a.d == 1536) return launch_mode<_Float16, 16, 1, 1536, 16>(a, *l);
    return (int)hipErrorNotSupported;
}
