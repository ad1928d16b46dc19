// hdb_mfma_b1_b.hip -- the row scan of packed-bit matrices on the bf16 matrix pipe (hdb_mfma_b1.hip), d = 384 / 512.
#include "hdb_mfma_b1.h"

extern "C" int hdb_launch_mfma_scan_b1_wide(const ScanArgs* args, const MfmaLaunch* l) {
    const ScanArgs& a = *args;
    switch (a.d) {
        case 384: return launch_b1<384>(a, *l);
        case 512: return launch_b1<512>(a, *l);
        default: return (int)hipErrorNotSupported;
    }
}
