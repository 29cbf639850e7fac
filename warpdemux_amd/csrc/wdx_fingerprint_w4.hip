// Fast fingerprint kernels of the ODD window widths 21, 23, 25, 27, 29, 31, 33, 35 (exact scores only, fast_body's kExactOnly; no
// streaming form) -- a translation unit of their own so that the build compiles the instantiations side by side.  The
// templates are wdx_fingerprint.hip's; nothing else of it is compiled here.
#define WDX_DEV_KERNELS_ONLY 1
#define WDX_EXTRA_TU 1
#include "wdx_fingerprint.hip"

namespace wdx {

FpKernel resolve_fast_w4(const FpKernelKey &k) {
    switch (k.fw) {
        case 21: return resolve_fast_width<21, 2>(k);
        case 23: return resolve_fast_width<23, 2>(k);
        case 25: return resolve_fast_width<25, 2>(k);
        case 27: return resolve_fast_width<27, 2>(k);
        case 29: return resolve_fast_width<29, 2>(k);
        case 31: return resolve_fast_width<31, 2>(k);
        case 33: return resolve_fast_width<33, 2>(k);
        case 35: return resolve_fast_width<35, 2>(k);
        default: return {};
    }
}

}  // namespace wdx
