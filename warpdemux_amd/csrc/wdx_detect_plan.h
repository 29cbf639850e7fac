// Adapter boundary detection (include/wdx.h: wdx_detect_rows states the rule): the domain of wdx_detect_params and the integer
// thresholds the kernel compares against, before anything is launched (plain C++17: no device runtime, nothing of the context).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/wdx.h"

namespace wdx {

// what detect_kernel reads of the parameters
struct DetectQ {
    int32_t max_trace;
    float qpp;
    int32_t find_start, thr1, start_win, max_start, min_ad, max_ad, polya_win, step_win, refine, shift_q;
    int64_t var_q;
};

struct DetectPlan {
    int rc = WDX_SUCCESS;
    char msg[200] = "";
    DetectQ q{};
    int64_t lds_bytes = 0;   // the quantised row: 2 bytes per sample of max_obs_trace, in whole 16-byte pieces
};

#define WDX_DETECT_REFUSE(...)                        \
    do {                                              \
        P.rc = WDX_ERR_INVALID;                       \
        snprintf(P.msg, sizeof P.msg, __VA_ARGS__);   \
        return P;                                     \
    } while (0)

inline DetectPlan detect_plan(const wdx_detect_params *p) {
    DetectPlan P;
    if (!p) WDX_DETECT_REFUSE("detect: the parameters are required (NULL given)");
    if (!isfinite(p->quant_per_pa) || !isfinite(p->open_pore_pa) || !isfinite(p->min_shift_pa) || !isfinite(p->max_polya_var))
        WDX_DETECT_REFUSE("detect: quant_per_pa, open_pore_pa, min_shift_pa and max_polya_var must be finite");
    if (p->max_obs_trace < 1 || p->max_obs_trace > WDX_DETECT_MAX_TRACE)
        WDX_DETECT_REFUSE("detect: max_obs_trace = %d (1..%d)", p->max_obs_trace, WDX_DETECT_MAX_TRACE);
    if (!(p->quant_per_pa > 0.f)) WDX_DETECT_REFUSE("detect: quant_per_pa = %g must be positive", (double)p->quant_per_pa);
    if (p->find_start != 0 && p->find_start != 1) WDX_DETECT_REFUSE("detect: find_start = %d (0 or 1)", p->find_start);
    if (p->step_win < 1 || p->step_win > p->polya_win || p->polya_win > 1024)
        WDX_DETECT_REFUSE("detect: step_win = %d, polya_win = %d (1 <= step_win <= polya_win <= 1024)", p->step_win, p->polya_win);
    if (p->min_obs_adapter < p->step_win || p->max_obs_adapter < p->min_obs_adapter)
        WDX_DETECT_REFUSE("detect: min_obs_adapter = %d, max_obs_adapter = %d (step_win = %d <= min_obs_adapter <= max_obs_adapter)",
                          p->min_obs_adapter, p->max_obs_adapter, p->step_win);
    if (p->start_win < 1 || p->start_win > 256) WDX_DETECT_REFUSE("detect: start_win = %d (1..256)", p->start_win);
    if (p->refine < 0 || p->refine > 4096) WDX_DETECT_REFUSE("detect: refine = %d (0..4096)", p->refine);
    if (p->max_start < 0) WDX_DETECT_REFUSE("detect: max_start = %d must not be negative", p->max_start);
    DetectQ &q = P.q;
    q.max_trace = p->max_obs_trace, q.qpp = p->quant_per_pa, q.find_start = p->find_start;
    q.start_win = p->start_win, q.max_start = p->max_start, q.min_ad = p->min_obs_adapter, q.max_ad = p->max_obs_adapter;
    q.polya_win = p->polya_win, q.step_win = p->step_win, q.refine = p->refine;
    // (volatile: one float32 product each, whatever the host compiler would like to contract or widen)
    volatile float t1 = p->open_pore_pa * p->quant_per_pa, t2 = p->min_shift_pa * p->quant_per_pa;
    q.thr1 = (int32_t)fminf(fmaxf(rintf(t1), -32768.f), 32768.f);
    q.shift_q = (int32_t)fminf(fmaxf(rintf(t2), -65536.f), 65536.f);
    volatile double v1 = (double)p->max_polya_var * (double)p->quant_per_pa;
    volatile double v2 = v1 * (double)p->quant_per_pa;
    q.var_q = (int64_t)fmin(fmax(floor(v2), -1.0), 2147483648.0);
    P.lds_bytes = ((int64_t)2 * q.max_trace + 15) / 16 * 16;
    return P;
}

#undef WDX_DETECT_REFUSE

}  // namespace wdx
