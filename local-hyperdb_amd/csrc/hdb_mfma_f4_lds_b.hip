// hdb_mfma_f4_lds_b.hip -- MXFP4 rows with the query parts in LDS (hdb_mfma_f4_lds.h), d = 384 / 512: 96 / 128 registers of
// converted tiles per lane.  A translation unit of its own so that the instantiations compile in parallel.
#include "hdb_mfma_f4_lds.h"

extern "C" int hdb_launch_mfma_scan_f4_lds_wide(const ScanArgs* args, const MfmaLaunch* l) {
    const ScanArgs& a = *args;
    switch (a.d) {
        case 384: return launch_f4_lds<384>(a, *l);
        case 512: return launch_f4_lds<512>(a, *l);
        default: return (int)hipErrorNotSupported;
    }
}
