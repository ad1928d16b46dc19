// hdb_mfma_f4_wide.hip -- the row scan of MXFP4 matrices wider than 512 elements on the bf16 matrix pipe (hdb_mfma_f4_wide.h; opt-in,
// b1_mfma_min_q with f8_ks_min_q): the S = d / W waves of a workgroup each take W elements of every row of a tile and add their
// accumulators through LDS -- one launch, no partial-sum workspace.  Slice widths W = 256 / 128 here, 384 / 512 in
// hdb_mfma_f4_wide_b.hip.
#include "hdb_mfma_f4_wide.h"

extern "C" int hdb_launch_mfma_scan_f4_wide_rows(const ScanArgs* args, const MfmaLaunch* l) {
    switch (hdb_mfma_f4_wide_geom(args->d).w) {
        case 256: return launch_f4_wide<256>(*args, *l);
        case 128: return launch_f4_wide<128>(*args, *l);
        default: return hdb_launch_mfma_scan_f4_wide_rows_b(args, l);
    }
}
