// hdb_mfma_f32b.hip -- the float32 MFMA row scan (hdb_mfma_f32.hip) for d = 384, 512 and 768: a translation unit of its own
// so that the instantiations compile in parallel.
#include "hdb_mfma_kernel.h"

extern "C" int hdb_launch_mfma_scan_f32_wide(const ScanArgs* args, const MfmaLaunch* l) {
    const ScanArgs& a = *args;
    switch (a.d) {
        case 384:
            if (l->nq_launch <= 64) return launch_mode<float, 16, 1, 384, 32, 2>(a, *l);
            return launch_mode<float, 16, 1, 384, 32>(a, *l);
        case 512: return launch_mode<float, 16, 1, 512, 16>(a, *l);
        case 768: return launch_mode<float, 16, 1, 768, 16>(a, *l);
        default: return (int)hipErrorNotSupported;
    }
}
