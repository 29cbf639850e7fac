// Which DTW dispatches take the wide-window kernel (WDX_OPT_WIDE_DTW; wdx_dtw.hip: dtw_wide_kernel) and what a wave of it
// costs -- the one statement of the rule (plain host C++17: no HIP, nothing of the context, so the system compiler builds it
// alone: tests/host/dtw_wide_check.cpp).
//
// The kernel walks the DP matrix in vertical strips of kWideDtwStrip columns: the strip's segment of the previous DP row
// lives in registers, the strip's right-edge column goes to the next strip through LDS, one float64 per row and lane
// (edge[i * 64 + lane]).  One-wave workgroups, so the LDS block of a workgroup is the LDS of a wave.
#pragma once
#include <stdint.h>

#include "../../include/wdx.h"

namespace wdx {

constexpr int kWideDtwMinWindow = 33;            // effective windows up to 32 stay on the register-band kernels
constexpr int kWideDtwStrip = 32;                // columns per strip: 32 float64 = 64 VGPRs of DP state per lane
constexpr int kWideDtwHalo = kWideDtwStrip - 1;  // samples the last strip reads beyond a reference's end (its zero halo)
constexpr int64_t kWideDtwLdsPerCu = 160 * 1024; // LDS of one gfx950 CU
constexpr int64_t kWideDtwLdsGranule = 1280;     // allocation granule of it (profiles/clip5w_lds_granule_probe.txt)

// |i - j| <= w - 1 is vacuous beyond L: window <= 0 (the reference's None) and window > L mean L
inline int64_t dtw_effective_window(int64_t L, int64_t window) { return (window <= 0 || window > L) ? L : window; }

struct WideDtwPlan {
    bool eligible = false;   // the dispatch takes dtw_wide_kernel
    int strips = 0;          // vertical strips per pair: ceil(L / kWideDtwStrip)
    int64_t lds_bytes = 0;   // dynamic LDS of one workgroup (= one wave): 64 lanes x L rows x 8 bytes
    int waves_per_cu = 0;    // resident waves the LDS leaves room for (the kernel's registers allow more)
};

// L: series length; window: as the caller gave it or effective; option: WDX_OPT_WIDE_DTW of the context.
// Not eligible: everything is zero, the dispatch is what it is without the option (scratch rows beyond window 32).
inline WideDtwPlan wide_dtw_plan(int64_t L, int64_t window, bool option) {
    WideDtwPlan P;
    if (!option || L < 1 || L > WDX_DTW_WIDE_MAX_L) return P;
    if (dtw_effective_window(L, window) < kWideDtwMinWindow) return P;
    P.eligible = true;
    P.strips = (int)((L + kWideDtwStrip - 1) / kWideDtwStrip);
    P.lds_bytes = 64 * L * (int64_t)sizeof(double);
    const int64_t alloc = (P.lds_bytes + kWideDtwLdsGranule - 1) / kWideDtwLdsGranule * kWideDtwLdsGranule;
    P.waves_per_cu = (int)(kWideDtwLdsPerCu / alloc);
    return P;
}

}  // namespace wdx
