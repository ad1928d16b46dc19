// hdb_mfma_anyd_a.hip -- instantiations of the any-width MFMA scan (hdb_mfma_anyd.h): _Float16 geometries 128 256 384
// (l->width: the geometry the row rides, hdb_mfma_anyd_pad)
#include "hdb_mfma_anyd.h"

extern "C" int hdb_launch_mfma_anyd_a(const ScanArgs* args, const MfmaLaunch* l) {
    const ScanArgs a = anyd_args(*args, 2);
    switch (l->width) {
        case 128: return launch_anyd<_Float16, 128, 64>(a, *l);
        case 256: return launch_anyd<_Float16, 256, 64>(a, *l);
        case 384: return launch_anyd<_Float16, 384, 64>(a, *l);
        default: return (int)hipErrorNotSupported;
    }
}
