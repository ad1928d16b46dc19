// hdb_mfma_f4_wide_b.hip -- the row scan of MXFP4 matrices wider than 512 elements (hdb_mfma_f4_wide.hip), slice widths 384 / 512.
#include "hdb_mfma_f4_wide.h"

extern "C" int hdb_launch_mfma_scan_f4_wide_rows_b(const ScanArgs* args, const MfmaLaunch* l) {
    switch (hdb_mfma_f4_wide_geom(args->d).w) {
        case 384: return launch_f4_wide<384>(*args, *l);
        case 512: return launch_f4_wide<512>(*args, *l);
        default: return (int)hipErrorNotSupported;
    }
}
