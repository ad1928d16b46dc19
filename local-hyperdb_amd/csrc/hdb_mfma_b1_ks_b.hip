// hdb_mfma_b1_ks_b.hip -- the K slices of packed-bit rows (hdb_mfma_b1_ks.hip), slices of 512 elements.
#include "hdb_mfma_b1.h"

extern "C" int hdb_launch_mfma_kslice_b1_wide(const ScanArgs* a, const MfmaLaunch* l) {
    if (l->width != 512) return (int)hipErrorNotSupported;
    return launch_b1_kslice<512>(*a, *l);
}
