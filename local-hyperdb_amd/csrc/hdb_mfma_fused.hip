// hdb_mfma_fused.hip -- instantiations of the single-launch top-k (hdb_mfma_fused.h) for the fp16 geometries of
// hdb_mfma.hip: a whole hdb_topk call of 1..4 dot / cosine / pearson queries (one euclidean query) in ONE kernel.
#include "hdb_mfma_fused.h"

// bytes of the persistent control block: 64 words of counters + the granules
extern "C" size_t hdb_mfma_fused_ctl_bytes(void) { return HDB_FUSED_HDR_BYTES + (size_t)HDB_FUSED_MAX_WG * HDB_FUSED_GRAN_PER_WG * 8; }

extern "C" int hdb_launch_mfma_fused(const ScanArgs* args, int dtype, const FusedArgs* fa, int max_blocks, void* stream) {
    const ScanArgs& a = *args;
    FusedArgs f = *fa;
    hipStream_t st = (hipStream_t)stream;
    const int blocks = hdb_mfma_fused_blocks(a.ntiles, hdb_cu_count(), max_blocks);
    f.gran = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(f.ctl) + HDB_FUSED_HDR_BYTES);
    if (dtype == HDB_F32) {
        switch (a.d) {
            case 128: return f.nq == 1 ? launch_fused<float, 1, 128, 64>(a, f, blocks, st) : launch_fused<float, 2, 128, 64>(a, f, blocks, st);
            case 256: return f.nq == 1 ? launch_fused<float, 1, 256, 32>(a, f, blocks, st) : launch_fused<float, 2, 256, 32>(a, f, blocks, st);
            case 384: return f.nq == 1 ? launch_fused<float, 1, 384, 32>(a, f, blocks, st) : launch_fused<float, 2, 384, 32>(a, f, blocks, st);
            case 512: return launch_fused<float, 1, 512, 16>(a, f, blocks, st);
            case 768: return launch_fused<float, 1, 768, 16>(a, f, blocks, st);
            default: return (int)hipErrorNotSupported;
        }
    }
    switch (a.d) {
        case 256: return launch_fused<_Float16, 2, 256, 64>(a, f, blocks, st);
        case 384: return launch_fused<_Float16, 2, 384, 64>(a, f, blocks, st);
        case 512: return launch_fused<_Float16, 2, 512, 32>(a, f, blocks, st);
        case 640: return launch_fused<_Float16, 2, 640, 32>(a, f, blocks, st);
        case 768: return launch_fused<_Float16, 2, 768, 32>(a, f, blocks, st);
        default: return hdb_launch_mfma_fused_wide(&a, &f, blocks, stream);
    }
}

#if HDB_FUSED_STAMPS
extern "C" int hdb_debug_read_fused_stamps(unsigned long long* host_out, int wgs) {
    if (wgs > HDB_CLOCK_WGS_F) wgs = HDB_CLOCK_WGS_F;
    return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(hdb_fused_stamps), (size_t)wgs * 16 * sizeof(unsigned long long));
}
#endif
