// An int16 device shard (include/wdx.h: wdx_adc_dev_in) is walked in slices of reads: the adapter windows of one slice are
// decoded into a context-owned float32 staging block, the unchanged chain runs on that block, the next slice reuses it in
// stream order.  This header is the one statement of the slicing arithmetic -- the launcher and the workspace functions
// both read it (plain host C++17 like wdx_window.h, so the system compiler builds it alone: tests/host/adc_dev_check.cpp).
//
// Staging layout of a slice of m reads: m rows of `pitch` floats, then three int32[m] -- the shifted a_start, a_end and the
// packed row lengths.  The chain sees the minibatch layout: row_off NULL, stride = pitch, row_len = the packed length.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "wdx_window.h"

namespace wdx {

// The staging block of a context never grows beyond this, whatever the shard holds: 1 GiB = 43 000 reads of the RNA004
// windows (6 144 samples) per slice, 4 095 reads of 65 536-sample windows (WDX_OPT_LONG_WINDOWS).
constexpr int64_t kAdcDevStagingBudget = (int64_t)1 << 30;
constexpr int64_t kAdcDevAlign = 8;   // a window starts on a multiple of 8 samples: 16-byte groups of int16

// The longest window a slice stages: the call's max_len, no longer than the longest one the call's branch fingerprints
// (a negative max_len counts as 0).  The kernel cuts every window one sample beyond it -- that sample makes the chain report
// the read WDX_READ_FAIL_UNKNOWN, exactly as the float32 twin reports the uncut window.
inline int64_t adc_dev_max_len(int64_t max_len, int64_t max_window) {
    return std::min(std::max<int64_t>(max_len, 0), max_window);
}

// Floats per staged read: a window cut at max_len + 1 samples, whose start was rounded down by at most 7, rounded up to
// whole groups of 8 (the kernel stores whole groups).
inline int64_t adc_dev_pitch(int64_t max_len) { return (max_len + 8 + 7) / 8 * 8; }

inline int64_t adc_dev_read_bytes(int64_t pitch) { return pitch * 4 + 12; }

struct AdcDevPlan {
    int64_t pitch = 0;          // floats per staged read
    int64_t slice_reads = 0;    // reads of every slice but the last
    int64_t n_slices = 0;
    int64_t last_reads = 0;     // reads of the last slice (0 when there is none)
    int64_t staging_bytes = 0;  // of the block that serves every slice; <= kAdcDevStagingBudget
};

// max_len: adc_dev_max_len's answer.  slice_option: WDX_OPT_ADC_DEV_SLICE_READS (0 or less = built-in); it lowers or raises
// the slice, never the staging block beyond the budget.  n_reads up to INT64_MAX / 2 without overflow: only n_slices grows.
inline AdcDevPlan adc_dev_plan(int64_t n_reads, int64_t max_len, int64_t slice_option) {
    AdcDevPlan P;
    P.pitch = adc_dev_pitch(max_len);
    const int64_t fit = std::max<int64_t>(kAdcDevStagingBudget / adc_dev_read_bytes(P.pitch), 1);
    P.slice_reads = slice_option > 0 ? std::min(slice_option, fit) : fit;
    if (n_reads <= 0) return P;
    P.n_slices = (n_reads - 1) / P.slice_reads + 1;
    P.last_reads = n_reads - (P.n_slices - 1) * P.slice_reads;
    P.staging_bytes = std::min(n_reads, P.slice_reads) * adc_dev_read_bytes(P.pitch);
    return P;
}

// Where read r's int16 samples are and which float32 row it stands for (the arithmetic of the contract in include/wdx.h):
//   strided   the row has `stride` samples, row_len clamped to 0 .. stride
//   packed    the row has capacity row_off[r + 1] - row_off[r]; row_len is clamped to it; the float32 row has row_win samples
//             (row_win < 0: none given = row_len), never fewer than row_len
struct AdcDevRow {
    int64_t limit;     // samples of the float32 row: adapter_window's `limit`
    int64_t row_len;   // ADC samples of the read, clamped: adapter_window's `row_len`
};
WDX_HD inline AdcDevRow adc_dev_row(bool packed, int64_t stride_or_capacity, int64_t row_len, int64_t row_win) {
    // (by value, no std::min / std::max of references: on the device those went through private memory)
    const int64_t cap = stride_or_capacity > 0 ? stride_or_capacity : 0;
    const int64_t len = row_len < 0 ? 0 : row_len > cap ? cap : row_len;
    AdcDevRow R;
    R.row_len = len;
    R.limit = !packed ? cap : row_win > len ? row_win : len;
    return R;
}

// The window the kernel stages for a read: adapter_window itself with the alignment of the 16-byte int16 loads and the cut
// one sample beyond max_len.
WDX_HD inline Window adc_dev_window(int32_t a_start, int32_t a_end, const AdcDevRow &R, bool dead, int64_t padding,
                                    int64_t max_len) {
    const WindowOpts o{padding, kAdcDevAlign, max_len + 1};
    return adapter_window(a_start, a_end, R.limit, dead, o, R.row_len);
}

}  // namespace wdx
