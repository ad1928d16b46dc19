// hdb_mfma_i8_b.hip -- int8 rows on the bf16 matrix pipe (hdb_mfma_i8.hip), d = 384 and d = 512.
#include "hdb_mfma_f8.h"

extern "C" int hdb_launch_mfma_scan_i8_wide(const ScanArgs* args, const MfmaLaunch* l) {
    const ScanArgs& a = *args;
    switch (a.d) {
        case 384: return launch_f8<384, HdbRowCvtI8>(a, *l);
        case 512: return launch_f8<512, HdbRowCvtI8>(a, *l);
        default: return (int)hipErrorNotSupported;
    }
}
