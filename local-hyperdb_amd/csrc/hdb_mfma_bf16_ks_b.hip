// hdb_mfma_bf16_ks_b.hip -- the K slices of wide bfloat16 rows (hdb_mfma_bf16_ks.hip), slices of 512 elements.
#include "hdb_mfma_kernel.h"

extern "C" int hdb_launch_mfma_kslice_bf16_wide(const ScanArgs* a, const MfmaLaunch* l) {
    if (l->width == 512) return launch_kslice<hdb_bf16, 512, 16>(*a, *l);
    return (int)hipErrorNotSupported;
}
