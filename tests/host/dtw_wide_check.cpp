// Stand-alone sweep of warpdemux_amd/csrc/wdx_dtw_wide.h -- which DTW dispatches take the wide-window kernel
// (WDX_OPT_WIDE_DTW) and what a wave of it costs -- built by tests/test_wide_dtw_host.py with the system compiler and the
// address / undefined-behaviour sanitizers.  Every series length 1 .. 300, window 0 .. 303 (0 and anything beyond L: the
// reference's unbanded None) and option 0 / 1.  stdout: one line per case, "L window option eligible strips lds_bytes
// waves_per_cu effective_window".  The program itself checks what must hold of every plan: the strips cover the row, the LDS
// block holds one float64 per row and lane and fits a CU, at least one wave is resident.
#include "wdx_dtw_wide.h"

#include <stdio.h>

int main() {
    long long cases = 0;
    for (int64_t L = 1; L <= 300; ++L)
        for (int64_t window = 0; window <= 303; ++window)
            for (int option = 0; option < 2; ++option) {
                const wdx::WideDtwPlan P = wdx::wide_dtw_plan(L, window, option != 0);
                const int64_t w = wdx::dtw_effective_window(L, window);
                if (w < 1 || w > L) return 1;
                if (P.eligible) {
                    if ((int64_t)P.strips * wdx::kWideDtwStrip < L || (int64_t)(P.strips - 1) * wdx::kWideDtwStrip >= L) return 2;
                    if (P.lds_bytes != 64 * L * 8 || P.lds_bytes > wdx::kWideDtwLdsPerCu) return 3;
                    if (P.waves_per_cu < 1 || (int64_t)P.waves_per_cu * P.lds_bytes > wdx::kWideDtwLdsPerCu) return 4;
                } else if (P.strips != 0 || P.lds_bytes != 0 || P.waves_per_cu != 0) {
                    return 5;
                }
                printf("%lld %lld %d %d %d %lld %d %lld\n", (long long)L, (long long)window, option, (int)P.eligible, P.strips,
                       (long long)P.lds_bytes, P.waves_per_cu, (long long)w);
                ++cases;
            }
    fprintf(stderr, "%lld cases\n", cases);
    return 0;
}
