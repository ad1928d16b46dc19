// hdb_mfma_i8.hip -- the row scan of int8 matrices (HDB_I8) on the bf16 matrix pipe: hdb_mfma_f8_kernel (hdb_mfma_f8.h) with the int8
// row converter (hdb_i8x8_to_bf16x8: rows converted per fragment in registers, exactly), float32 queries as three exact bf16 parts,
// the bfloat16 flavour's K walk and epilogue.  Multi-kernel pipeline only: MODE 0 (scores) and MODE 1 (filter).  d = 128 / 256
// here, 384 / 512 in hdb_mfma_i8_b.hip.
#include "hdb_mfma_f8.h"

extern "C" int hdb_launch_mfma_scan_i8(const ScanArgs* args, const MfmaLaunch* l) {
    const ScanArgs& a = *args;
    switch (a.d) {
        case 128: return launch_f8<128, HdbRowCvtI8>(a, *l);
        case 256: return launch_f8<256, HdbRowCvtI8>(a, *l);
        default: return hdb_launch_mfma_scan_i8_wide(args, l);
    }
}
