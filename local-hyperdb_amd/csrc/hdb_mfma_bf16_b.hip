// hdb_mfma_bf16_b.hip -- bfloat16 rows on the bf16 matrix pipe (hdb_mfma_bf16.hip), d = 384 and d = 512.
#include "hdb_mfma_kernel.h"

extern "C" int hdb_launch_mfma_scan_bf16_wide(const ScanArgs* args, const MfmaLaunch* l) {
    const ScanArgs& a = *args;
    switch (a.d) {
        case 384: return launch_mode01<hdb_bf16, 16, 1, 384, 32>(a, *l);
        case 512: return launch_mode01<hdb_bf16, 16, 1, 512, 16>(a, *l);
        default: return (int)hipErrorNotSupported;
    }
}
