// hdb_mfma_anyd_b.hip -- instantiations of the any-width MFMA scan (hdb_mfma_anyd.h): _Float16 geometries 512 768 1024
#include "hdb_mfma_anyd.h"

extern "C" int hdb_launch_mfma_anyd_b(const ScanArgs* args, const MfmaLaunch* l) {
    const ScanArgs a = anyd_args(*args, 2);
    switch (l->width) {
        case 512: return launch_anyd<_Float16, 512, 32>(a, *l);
        case 768: return launch_anyd<_Float16, 768, 32>(a, *l);
        case 1024: return launch_anyd<_Float16, 1024, 16>(a, *l);
        default: return (int)hipErrorNotSupported;
    }
}
