// hdb_mfma_f4_b.hip -- the row scan of MXFP4 matrices on the bf16 matrix pipe (hdb_mfma_f4.hip), d = 384 / 512.
#include "hdb_mfma_f4.h"

extern "C" int hdb_launch_mfma_scan_f4_wide(const ScanArgs* args, const MfmaLaunch* l) {
    const ScanArgs& a = *args;
    switch (a.d) {
        case 384: return launch_f4<384>(a, *l);
        case 512: return launch_f4<512>(a, *l);
        default: return (int)hipErrorNotSupported;
    }
}
