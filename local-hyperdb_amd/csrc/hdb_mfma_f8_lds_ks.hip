// hdb_mfma_f8_lds_ks.hip -- the K slices of float8 e4m3 rows wider than 512 elements (hdb_mfma_ksplit.hip, ks_geom_f8; f8_ks_min_q)
// with every slice expanded to bf16 in LDS once per workgroup (hdb_mfma_f8_lds.h, KSL; f8_lds_min_q): one slice of 256, 384 or 512
// elements per launch, the partial sums indexed by the tile sequence as in hdb_mfma_f8_ks.hip, whatever the slice's stage height.
// Slices of 256 / 384 here, 512 in hdb_mfma_f8_lds_ks_b.hip.
#include "hdb_mfma_f8_lds.h"

extern "C" int hdb_launch_mfma_kslice_f8_lds(const ScanArgs* a, const MfmaLaunch* l) {
    if (l->width == 256) return launch_f8_lds_kslice<256>(*a, *l);
    if (l->width == 384) return launch_f8_lds_kslice<384>(*a, *l);
    return hdb_launch_mfma_kslice_f8_lds_wide(a, l);
}
