// hdb_mfma_f4_lds.hip -- the row scan of MXFP4 matrices (HDB_MXF4) on the bf16 matrix pipe for large batches (hdb_mfma_f4_lds.h;
// opt-in, f8_lds_min_q beside b1_mfma_min_q): the register flavour's arithmetic and bits (hdb_mfma_f4.h), the query parts of 48 / 64
// queries in LDS, two converted tiles per wave in registers.  Multi-kernel pipeline only: MODE 0 (scores) and MODE 1 (filter).
// d = 128 / 256 here, 384 / 512 in hdb_mfma_f4_lds_b.hip.
#include "hdb_mfma_f4_lds.h"

extern "C" int hdb_launch_mfma_scan_f4_lds(const ScanArgs* args, const MfmaLaunch* l) {
    const ScanArgs& a = *args;
    switch (a.d) {
        case 128: return launch_f4_lds<128>(a, *l);
        case 256: return launch_f4_lds<256>(a, *l);
        default: return hdb_launch_mfma_scan_f4_lds_wide(args, l);
    }
}
