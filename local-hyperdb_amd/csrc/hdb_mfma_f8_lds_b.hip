// hdb_mfma_f8_lds_b.hip -- float8 e4m3 rows expanded to bf16 in LDS (hdb_mfma_f8_lds.h), d = 384 / 512: the query parts of 16
// queries take 144 / 192 registers.  A translation unit of its own so that the instantiations compile in parallel.
#include "hdb_mfma_f8_lds.h"

extern "C" int hdb_launch_mfma_scan_f8_lds_wide(const ScanArgs* args, const MfmaLaunch* l) {
    const ScanArgs& a = *args;
    switch (a.d) {
        case 384: return launch_f8_lds<384>(a, *l);
        case 512: return launch_f8_lds<512>(a, *l);
        default: return (int)hipErrorNotSupported;
    }
}
