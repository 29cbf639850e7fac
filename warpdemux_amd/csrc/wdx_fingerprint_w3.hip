// Fast fingerprint kernels of the ODD window widths 7, 9, 11, 13, 15, 17, 19 (exact scores only, fast_body's kExactOnly; no
// streaming form) -- a translation unit of their own so that the build compiles the instantiations side by side.  The
// templates are wdx_fingerprint.hip's; nothing else of it is compiled here.
#define WDX_DEV_KERNELS_ONLY 1
#define WDX_EXTRA_TU 1
#include "wdx_fingerprint.hip"

namespace wdx {

FpKernel resolve_fast_w3(const FpKernelKey &k) {
    switch (k.fw) {
        case 7: return resolve_fast_width<7, 2>(k);
        case 9: return resolve_fast_width<9, 2>(k);
        case 11: return resolve_fast_width<11, 2>(k);
        case 13: return resolve_fast_width<13, 2>(k);
        case 15: return resolve_fast_width<15, 2>(k);
        case 17: return resolve_fast_width<17, 2>(k);
        case 19: return resolve_fast_width<19, 2>(k);
        default: return {};
    }
}

}  // namespace wdx
