// hdb_mfma_bf16.hip -- the row scan of bfloat16 matrices (HDB_BF16) on the bf16 matrix pipe (MfmaShape<16, hdb_bf16>,
// hdb_mfma_kernel.h): the rows are the A fragments as they lie in memory (the fp16 flavour's LDS ring, swizzle and fragment map),
// a float32 query travels as three bf16 parts that add up to it exactly, three v_mfma_f32_16x16x32_bf16 per k-step, fp32
// accumulation.  np.dot of the reference (hyperdb/ranking_algorithm.py:29,:41) on the widened matrix within the float32
// contract.  Multi-kernel pipeline only: MODE 0 (scores) and MODE 1 (filter); 128 queries per launch row.
// d = 128 / 256 here, 384 / 512 in hdb_mfma_bf16_b.hip (translation units of their own so that the instantiations compile in parallel);
// wider rows go through K slices of these widths (hdb_mfma_bf16_ks.hip).
#include "hdb_mfma_kernel.h"

extern "C" int hdb_launch_mfma_scan_bf16(const ScanArgs* args, const MfmaLaunch* l) {
    const ScanArgs& a = *args;
    switch (a.d) {
        case 128: return launch_mode01<hdb_bf16, 16, 1, 128, 64>(a, *l);
        case 256: return launch_mode01<hdb_bf16, 16, 1, 256, 64>(a, *l);
        default: return hdb_launch_mfma_scan_bf16_wide(args, l);
    }
}
