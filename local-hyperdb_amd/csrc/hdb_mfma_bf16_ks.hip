// hdb_mfma_bf16_ks.hip -- the K slices of bfloat16 rows wider than 512 elements (hdb_mfma_ksplit.hip; the slice lists are
// ks_geom_bf16, hdb_caps.h): one slice of 256, 384 or 512 elements per launch on the bf16 matrix pipe (MfmaShape<16, hdb_bf16>,
// hdb_mfma_kernel.h), 16-row stages whatever the slice's width -- every slice of a row walks the same tile sequence, its partial
// sums are indexed by it.  The float32 queries are split into their three bf16 parts slice by slice (3 x 32 / 48 / 64 k-step
// fragments of 16 queries = 96 / 144 / 192 registers); 128 queries per launch row.
// Slices of 256 / 384 here, 512 in hdb_mfma_bf16_ks_b.hip (translation units of their own so that the instantiations compile in parallel).
#include "hdb_mfma_kernel.h"

extern "C" int hdb_launch_mfma_kslice_bf16(const ScanArgs* a, const MfmaLaunch* l) {
    if (l->width == 256) return launch_kslice<hdb_bf16, 256, 16>(*a, *l);
    if (l->width == 384) return launch_kslice<hdb_bf16, 384, 16>(*a, *l);
    return hdb_launch_mfma_kslice_bf16_wide(a, l);
}
