// Stand-alone check of the rule in warpdemux_amd/csrc/wdx_window.h that says which product option raises the adapter-window
// cap of a call (tests/test_long_refine_host.py builds it with the system compiler and the address / undefined-behaviour
// sanitizers): a call of the consensus-refinement branch looks at WDX_OPT_LONG_REFINE_WINDOWS only, a plain call at
// WDX_OPT_LONG_WINDOWS only.  stdout: one line per combination, "refine long_windows long_refine_windows long_form cap cut",
// where `cut` is what the live tick's int16 staging keeps of a window of 70 000 samples (the cap of the tick's branch plus
// one sample: that is what reports the window).
#include "wdx_window.h"

#include <stdio.h>

int main() {
    for (int refine = 0; refine < 2; ++refine)
        for (int lw = 0; lw < 2; ++lw)
            for (int lrw = 0; lrw < 2; ++lrw) {
                const bool on = wdx::long_form_on(refine != 0, lw != 0, lrw != 0);
                const int64_t cap = wdx::max_adapter_window(refine != 0, lw != 0, lrw != 0);
                // the live tick's int16 window (wdx_live.hip): no row limit, at most cap + 1 samples
                const wdx::WindowOpts wo{100, 1, cap + 1};
                const wdx::Window w = wdx::adapter_window(100, 69900, wdx::kNoRowLimit, false, wo, 70000);
                if (on != (refine ? lrw != 0 : lw != 0)) return 1;
                if (cap != (on ? (int64_t)WDX_MAX_LONG_ADAPTER_SAMPLES : (int64_t)WDX_MAX_ADAPTER_SAMPLES)) return 1;
                printf("%d %d %d %d %lld %lld\n", refine, lw, lrw, (int)on, (long long)cap, (long long)w.win);
            }
    return 0;
}
