// hdb_mfma_anyd_d.hip -- instantiations of the any-width MFMA scan (hdb_mfma_anyd.h): float geometries 512 768
#include "hdb_mfma_anyd.h"

extern "C" int hdb_launch_mfma_anyd_d(const ScanArgs* args, const MfmaLaunch* l) {
    const ScanArgs a = anyd_args(*args, 4);
    switch (l->width) {
        case 512: return launch_anyd<float, 512, 16>(a, *l);
        case 768: return launch_anyd<float, 768, 16>(a, *l);
        default: return (int)hipErrorNotSupported;
    }
}
