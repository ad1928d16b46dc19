// hdb_mfma_f8_ks.hip -- the K slices of float8 e4m3 rows wider than 512 elements (hdb_mfma_ksplit.hip; the slice lists are
// ks_geom_f8, hdb_caps.h; opt-in through f8_ks_min_q): one slice of 256, 384 or 512 elements per launch through the slice flavour
// of hdb_mfma_f8_kernel (hdb_mfma_f8.h) -- rows converted per fragment in registers, no LDS ring, 16-row tiles, every slice of a row
// walks the same tile sequence and indexes its partial sums by it.  The float32 queries are split into their three bf16 parts slice
// by slice (96 / 144 / 192 registers for 16 queries); up to 64 queries per launch row.
// Slices of 256 / 384 here, 512 in hdb_mfma_f8_ks_b.hip (translation units of their own so that the instantiations compile in parallel).
#include "hdb_mfma_f8.h"

extern "C" int hdb_launch_mfma_kslice_f8(const ScanArgs* a, const MfmaLaunch* l) {
    if (l->width == 256) return launch_f8_kslice<256>(*a, *l);
    if (l->width == 384) return launch_f8_kslice<384>(*a, *l);
    return hdb_launch_mfma_kslice_f8_wide(a, l);
}
