// hdb_mfma_b1.hip -- the row scan of packed-bit matrices (HDB_B1) on the bf16 matrix pipe (hdb_mfma_b1.h; opt-in, b1_mfma_min_q):
// bits expanded to bf16 0.0 / 1.0 per fragment in registers, float32 queries as three exact bf16 parts, the bfloat16 flavour's K walk
// and epilogue.  Multi-kernel pipeline only: MODE 0 (scores) and MODE 1 (filter).  d = 128 / 256 here, 384 / 512 in hdb_mfma_b1_b.hip.
#include "hdb_mfma_b1.h"

extern "C" int hdb_launch_mfma_scan_b1(const ScanArgs* args, const MfmaLaunch* l) {
    const ScanArgs& a = *args;
    switch (a.d) {
        case 128: return launch_b1<128>(a, *l);
        case 256: return launch_b1<256>(a, *l);
        default: return hdb_launch_mfma_scan_b1_wide(args, l);
    }
}
