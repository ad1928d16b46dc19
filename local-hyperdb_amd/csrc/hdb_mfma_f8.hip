// hdb_mfma_f8.hip -- the row scan of float8 e4m3 matrices (HDB_F8E4M3) on the bf16 matrix pipe (hdb_mfma_f8.h): rows converted per
// fragment in registers, float32 queries as three exact bf16 parts, the bfloat16 flavour's K walk and epilogue.  Multi-kernel
// pipeline only: MODE 0 (scores) and MODE 1 (filter).  d = 128 / 256 here, 384 / 512 in hdb_mfma_f8_b.hip.
#include "hdb_mfma_f8.h"

extern "C" int hdb_launch_mfma_scan_f8(const ScanArgs* args, const MfmaLaunch* l) {
    const ScanArgs& a = *args;
    switch (a.d) {
        case 128: return launch_f8<128>(a, *l);
        case 256: return launch_f8<256>(a, *l);
        default: return hdb_launch_mfma_scan_f8_wide(args, l);
    }
}
