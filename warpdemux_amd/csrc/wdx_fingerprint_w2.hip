// Fast fingerprint kernels of the window widths 22, 26, 28, 32, 34 (even, not multiples of the tile's six positions per
// lane: exact scores only, fast_body's kExactOnly) -- a translation unit of their own so that the build compiles the
// instantiations side by side.  The templates are wdx_fingerprint.hip's; nothing else of it is compiled here.
#define WDX_DEV_KERNELS_ONLY 1
#define WDX_EXTRA_TU 1
#include "wdx_fingerprint.hip"

namespace wdx {

FpKernel resolve_fast_w2(const FpKernelKey &k) {
    switch (k.fw) {
        case 22: return resolve_fast_width<22, 2>(k);
        case 26: return resolve_fast_width<26, 2>(k);
        case 28: return resolve_fast_width<28, 2>(k);
        case 32: return resolve_fast_width<32, 2>(k);
        case 34: return resolve_fast_width<34, 2>(k);
        default: return {};
    }
}

}  // namespace wdx
