// hdb_mfma_f8_b.hip -- float8 e4m3 rows on the bf16 matrix pipe (hdb_mfma_f8.hip), d = 384 and d = 512.
#include "hdb_mfma_f8.h"

extern "C" int hdb_launch_mfma_scan_f8_wide(const ScanArgs* args, const MfmaLaunch* l) {
    const ScanArgs& a = *args;
    switch (a.d) {
        case 384: return launch_f8<384>(a, *l);
        case 512: return launch_f8<512>(a, *l);
        default: return (int)hipErrorNotSupported;
    }
}
