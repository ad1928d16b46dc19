// hdb_mfma_f8_lds_ks_b.hip -- the 512-element K slice of float8 e4m3 rows expanded to bf16 in LDS (hdb_mfma_f8_lds.h, KSL; see
// hdb_mfma_f8_lds_ks.hip): 192 registers of query parts.  A translation unit of its own so that the instantiations compile in parallel.
#include "hdb_mfma_f8_lds.h"

extern "C" int hdb_launch_mfma_kslice_f8_lds_wide(const ScanArgs* a, const MfmaLaunch* l) {
    if (l->width == 512) return launch_f8_lds_kslice<512>(*a, *l);
    return (int)hipErrorNotSupported;
}
