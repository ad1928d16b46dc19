// hdb_mfma_anyd_c.hip -- instantiations of the any-width MFMA scan (hdb_mfma_anyd.h): float geometries 128 256 384
#include "hdb_mfma_anyd.h"

extern "C" int hdb_launch_mfma_anyd_c(const ScanArgs* args, const MfmaLaunch* l) {
    const ScanArgs a = anyd_args(*args, 4);
    switch (l->width) {
        case 128: return launch_anyd<float, 128, 64>(a, *l);
        case 256: return launch_anyd<float, 256, 32>(a, *l);
        case 384: return launch_anyd<float, 384, 32>(a, *l);
        default: return (int)hipErrorNotSupported;
    }
}
