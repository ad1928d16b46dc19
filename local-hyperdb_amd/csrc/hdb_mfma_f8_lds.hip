// hdb_mfma_f8_lds.hip -- the row scan of float8 e4m3 matrices (HDB_F8E4M3) on the bf16 matrix pipe with the rows expanded to bf16 in
// LDS once per workgroup (hdb_mfma_f8_lds.h; opt-in, f8_lds_min_q): the register flavour's arithmetic and bits (hdb_mfma_f8.h), a
// stage of rows loaded and converted once for the 64 or 128 queries of a workgroup.  Multi-kernel pipeline only: MODE 0 (scores) and
// MODE 1 (filter).  d = 128 / 256 here, 384 / 512 in hdb_mfma_f8_lds_b.hip.
#include "hdb_mfma_f8_lds.h"

extern "C" int hdb_launch_mfma_scan_f8_lds(const ScanArgs* args, const MfmaLaunch* l) {
    const ScanArgs& a = *args;
    switch (a.d) {
        case 128: return launch_f8_lds<128>(a, *l);
        case 256: return launch_f8_lds<256>(a, *l);
        default: return hdb_launch_mfma_scan_f8_lds_wide(args, l);
    }
}
