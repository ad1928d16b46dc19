// hdb_mfma_narrow.hip -- instantiations of the MFMA row scan (hdb_mfma_kernel.h) for fp16 d = 128 and 256, one query tile per wave: a translation unit of its own so that
// the geometries compile in parallel (each carries 3 modes x 3 metrics x {bias, no bias} kernels).
#include "hdb_mfma_kernel.h"

extern "C" int hdb_launch_mfma_scan_f16_narrow(const ScanArgs* args, const MfmaLaunch* l) {
    const ScanArgs& a = *args;
    if (a.d == 128) return launch_mode<_Float16, 16, 1, 128, 64>(a, *l);
    if (a.d == 256) return launch_mode<_Float16, 16, 1, 256, 64>(a, *l);
    return (int)hipErrorNotSupported;
}
