// hdb_mfma_b1_ks.hip -- the K slices of packed-bit rows wider than 512 elements (hdb_mfma_ksplit.hip; the slice lists are ks_geom_b1,
// hdb_caps.h; opt-in through b1_mfma_min_q): one slice of 256, 384 or 512 elements per launch through the slice flavour of
// hdb_mfma_b1_kernel (hdb_mfma_b1.h).  Every slice of a row walks the same tile sequence and indexes its partial sums by it.
// Slices of 256 / 384 here, 512 in hdb_mfma_b1_ks_b.hip (translation units of their own so that the instantiations compile in parallel).
#include "hdb_mfma_b1.h"

extern "C" int hdb_launch_mfma_kslice_b1(const ScanArgs* a, const MfmaLaunch* l) {
    if (l->width == 256) return launch_b1_kslice<256>(*a, *l);
    if (l->width == 384) return launch_b1_kslice<384>(*a, *l);
    return hdb_launch_mfma_kslice_b1_wide(a, l);
}
