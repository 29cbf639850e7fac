// Fast fingerprint kernels of the window widths 8, 10, 14, 16, 20 (even, not multiples of the tile's six positions per
// lane: exact scores only, fast_body's kExactOnly) -- a translation unit of their own so that the build compiles the
// instantiations side by side.  The templates are wdx_fingerprint.hip's; nothing else of it is compiled here.
#define WDX_DEV_KERNELS_ONLY 1
#define WDX_EXTRA_TU 1
#include "wdx_fingerprint.hip"

namespace wdx {

FpKernel resolve_fast_w1(const FpKernelKey &k) {
    switch (k.fw) {
        case 8: return resolve_fast_width<8, 2>(k);
        case 10: return resolve_fast_width<10, 2>(k);
        case 14: return resolve_fast_width<14, 2>(k);
        case 16: return resolve_fast_width<16, 2>(k);
        case 20: return resolve_fast_width<20, 2>(k);
        default: return {};
    }
}

}  // namespace wdx
