// hdb_mfma_f32.hip -- fp32 instantiations of the MFMA row scan (hdb_mfma_kernel.h): v_mfma_f32_16x16x4_f32, exact
// fp32 products and accumulation, so batches on float32 matrices (the reference's default fp_precision,
// hyperdb.py:51) keep the 1e-5 parity contract while up to 128 queries ride on one pass over V instead of 4.
#include "hdb_mfma_kernel.h"

extern "C" int hdb_launch_mfma_scan_f32(const ScanArgs* args, const MfmaLaunch* l) {
    const ScanArgs& a = *args;
    switch (a.d) {
        // up to 64 queries: two waves per query group, each multiplying every other 16-row tile of the stage, so that
        // all four SIMDs issue fp32 MFMAs (N=4M d=384, 16 queries: 1.73 ms with one wave per group)
        case 128:
            if (l->nq_launch <= 64) return launch_mode<float, 16, 1, 128, 64, 2>(a, *l);
            return launch_mode<float, 16, 1, 128, 64>(a, *l);
        case 256:
            if (l->nq_launch <= 64) return launch_mode<float, 16, 1, 256, 32, 2>(a, *l);
            return launch_mode<float, 16, 1, 256, 32>(a, *l);
        default: return hdb_launch_mfma_scan_f32_wide(args, l);     // 384, 512, 768
    }
}
