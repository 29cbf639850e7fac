// Accuracy thresholds from probabilities (include/wdx.h: wdx_accuracy_thresholds_device states the rule): what a call does with its
// sizes, before anything is launched (plain C++17: no device runtime, nothing of the context).  wdx_thresholds.hip launches what the
// plan names.
//
//   pass one   one workgroup of 256 threads per (chunk of kThrRows = 4 096 rows, group of classes), one lane per row.  A group is
//              as many predicted classes as fit kThrLdsEntries uint32 LDS counters at 2 (R + 1) counters a class (the bins'
//              row counts and hit counts): all 16 classes up to R = 191 (12.9 KB at k = 16, R = 100), one class at R = 4 096.
//              A workgroup adds at most 4 096 to a counter, then flushes the counters that are not zero to the global int64
//              histograms with 64-bit atomics: integer sums, the same bits in any arrival order.
//   pass two   one wave per class: the suffix sums from the top bin down and, per target, the smallest bin that qualifies.
//
// WORKSPACE (context-owned, grow-only): the two histograms int64 (k, R + 1) each and the skipped count, for the outputs the caller
// did not ask for.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "../../include/wdx.h"

namespace wdx {

constexpr int kThrThreads = 256;
constexpr int kThrRows = 4096;            // rows per pass-one workgroup
constexpr int kThrLdsEntries = 12288;     // uint32 LDS counters of one pass-one workgroup (48 KiB)
static_assert(2 * (WDX_THRESHOLDS_MAX_RESOLUTION + 1) <= kThrLdsEntries, "one class at the largest resolution fits");

struct ThrTargets { int32_t pm[WDX_THRESHOLDS_MAX_TARGETS]; };

struct ThrPlan {
    int rc = WDX_SUCCESS;
    char msg[224] = {0};
    int64_t n = 0;
    int k = 0, R = 0, T = 0;
    int bins = 0;                 // R + 1
    int classes_per_group = 0, groups = 0;
    int64_t chunks = 0;           // row chunks of pass one (0: nothing is launched for it)
    int64_t lds_bytes = 0;
    int64_t hist_entries = 0;     // k * (R + 1)
    int64_t off_kept = 0, off_hit = 0, off_skipped = 0, ws_bytes = 0;
    ThrTargets targets{};
};

inline ThrPlan thresholds_plan(int64_t n, int32_t k, int32_t R, const int32_t *targets_pm, int32_t T, bool have_prob, bool have_y, bool have_thr) {
    ThrPlan P;
#define WDX_THR_REFUSE(code, ...)                      \
    do {                                               \
        P = ThrPlan();                                 \
        snprintf(P.msg, sizeof P.msg, __VA_ARGS__);    \
        P.rc = (code);                                 \
        return P;                                      \
    } while (0)
    if (n < 0) WDX_THR_REFUSE(WDX_ERR_INVALID, "accuracy thresholds: n = %lld must not be negative", (long long)n);
    if (n > WDX_THRESHOLDS_MAX_ROWS)
        WDX_THR_REFUSE(WDX_ERR_UNSUPPORTED, "accuracy thresholds: n = %lld rows, more than WDX_THRESHOLDS_MAX_ROWS = %lld", (long long)n,
                       (long long)WDX_THRESHOLDS_MAX_ROWS);
    if (k < 2 || k > WDX_THRESHOLDS_MAX_CLASSES)
        WDX_THR_REFUSE(WDX_ERR_INVALID, "accuracy thresholds: k = %d classes (2..%d)", k, WDX_THRESHOLDS_MAX_CLASSES);
    if (R < 1 || R > WDX_THRESHOLDS_MAX_RESOLUTION)
        WDX_THR_REFUSE(WDX_ERR_INVALID, "accuracy thresholds: resolution = %d (1..%d)", R, WDX_THRESHOLDS_MAX_RESOLUTION);
    if (T < 1 || T > WDX_THRESHOLDS_MAX_TARGETS)
        WDX_THR_REFUSE(WDX_ERR_INVALID, "accuracy thresholds: %d targets (1..%d)", T, WDX_THRESHOLDS_MAX_TARGETS);
    if (!targets_pm) WDX_THR_REFUSE(WDX_ERR_INVALID, "accuracy thresholds: the targets are required (NULL given)");
    for (int t = 0; t < T; ++t)
        if (targets_pm[t] < 0 || targets_pm[t] > 1000)
            WDX_THR_REFUSE(WDX_ERR_INVALID, "accuracy thresholds: target %d is %d per mille (0..1000)", t, targets_pm[t]);
    if (n > 0 && (!have_prob || !have_y)) WDX_THR_REFUSE(WDX_ERR_INVALID, "accuracy thresholds: the probabilities and the class indices are required (NULL given)");
    if (!have_thr) WDX_THR_REFUSE(WDX_ERR_INVALID, "accuracy thresholds: the threshold table is required (NULL given)");
#undef WDX_THR_REFUSE
    P.n = n, P.k = k, P.R = R, P.T = T, P.bins = R + 1;
    for (int t = 0; t < T; ++t) P.targets.pm[t] = targets_pm[t];
    const int fit = kThrLdsEntries / (2 * P.bins);
    P.classes_per_group = fit < k ? fit : k;
    P.groups = (k + P.classes_per_group - 1) / P.classes_per_group;
    P.chunks = (n + kThrRows - 1) / kThrRows;
    P.lds_bytes = 4 * (int64_t)P.classes_per_group * 2 * P.bins;
    P.hist_entries = (int64_t)k * P.bins;
    P.off_kept = 0;
    P.off_hit = 8 * P.hist_entries;
    P.off_skipped = 16 * P.hist_entries;
    P.ws_bytes = 16 * P.hist_entries + 8;
    return P;
}

}  // namespace wdx
