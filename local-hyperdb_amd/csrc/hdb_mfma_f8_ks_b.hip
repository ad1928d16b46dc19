// hdb_mfma_f8_ks_b.hip -- the K slices of float8 e4m3 rows (hdb_mfma_f8_ks.hip), slices of 512 elements.
#include "hdb_mfma_f8.h"

extern "C" int hdb_launch_mfma_kslice_f8_wide(const ScanArgs* a, const MfmaLaunch* l) {
    if (l->width != 512) return (int)hipErrorNotSupported;
    return launch_f8_kslice<512>(*a, *l);
}
