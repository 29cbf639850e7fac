// The adapter window of a read as every host way in stages it -- the one statement of the rule (plain host C++17: no HIP,
// nothing of the context, so the system compiler builds it alone: tests/host/window_check.cpp).
//
// The kernels take samples [max(0, a_start - padding), min(row_len, a_end + padding)) of a row (extract_adapter,
// sig_proc.py:382-391).  A host loop that moves only those samples hands the kernels a PACKED row -- samples [first, en)
// of the original one, `first` = the window start rounded down to the alignment of the copy -- with the adapter bounds
// shifted by `first`: the kernels' rule on the packed row selects the same samples, bit for bit.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "../../include/wdx.h"

// The rule is also evaluated per read ON the device (wdx_adc.hip: the int16 device shards), from this very text: hipcc
// compiles the functions below for both sides, the system compiler sees plain inline functions.
#ifdef __HIPCC__
#define WDX_HD __attribute__((host)) __attribute__((device))
#else
#define WDX_HD
#endif

namespace wdx {

// The longest adapter window a call fingerprints -- the one statement of which product option raises it: a call of the
// consensus-refinement branch (rp != NULL) looks at WDX_OPT_LONG_REFINE_WINDOWS only, a plain call at WDX_OPT_LONG_WINDOWS
// only (tests/host/long_cap_check.cpp).
inline bool long_form_on(bool refine, bool long_windows, bool long_refine_windows) {
    return refine ? long_refine_windows : long_windows;
}
inline int64_t max_adapter_window(bool refine, bool long_windows, bool long_refine_windows) {
    return long_form_on(refine, long_windows, long_refine_windows) ? (int64_t)WDX_MAX_LONG_ADAPTER_SAMPLES
                                                                   : (int64_t)WDX_MAX_ADAPTER_SAMPLES;
}

constexpr int64_t kNoRowLimit = INT64_MAX;   // ragged rows whose window may run past the read's end (live int16 chunks)

struct WindowOpts {
    int64_t padding = 0;
    int64_t align = 1;     // `first` is a multiple of it: 1 (DMA / memcpy of floats), 4 (16-byte bus reads of floats), 8 (of int16)
    int64_t max_win = 0;   // > 0: the window keeps at most this many samples (rows without a limit)
};

struct Window {
    int64_t first = 0;   // first sample taken
    int64_t row = 0;     // samples of the packed row: [first, en)
    int64_t valid = 0;   // of them copied; the rest is the NaN tail the device writes (int16 rows)
    int64_t win = 0;     // en - st, what the kernels will see: max_len is the maximum of it
    int32_t a_start = 0, a_end = 0;   // the adapter bounds, shifted by `first`
};

// limit: the samples of the row (stride; row_len or row_win of a caller-packed row; kNoRowLimit).  dead: ok && !ok[r].
// row_len >= 0: the read's own samples, which `valid` is counted against (int16 rows have no NaN tail to end them).
// The start is clamped to the row BEFORE it is aligned: a start beyond the row (a failed detection's garbage) takes
// nothing instead of samples of the next row.  A dead read or an empty window: row = valid = win = 0, bounds unshifted.
WDX_HD inline Window adapter_window(int32_t a_start, int32_t a_end, int64_t limit, bool dead, const WindowOpts &o,
                             int64_t row_len = -1) {
    Window w;
    w.a_start = a_start;
    w.a_end = a_end;
    const int64_t st = std::min(std::max<int64_t>((int64_t)a_start - o.padding, 0), limit);
    int64_t en = std::min((int64_t)a_end + o.padding, limit);
    if (o.max_win > 0) en = std::min(en, st + o.max_win);
    if (dead || en <= st) return w;
    w.first = st & ~(o.align - 1);
    w.row = en - w.first;
    w.valid = row_len < 0 ? w.row : std::min(std::max<int64_t>(row_len - w.first, 0), w.row);
    w.win = en - st;
    w.a_start = (int32_t)((int64_t)a_start - w.first);
    w.a_end = (int32_t)((int64_t)a_end - w.first);
    return w;
}

// What a loop over the reads of a batch keeps of their windows.
struct WindowBatch {
    int64_t max_len = 0;      // FpReads::max_len
    int64_t col0, col1 = 0;   // columns [col0, col1) hold every copied sample of the batch (the 2-D copy)
    int64_t win_total = 0;    // copied samples; against (col1 - col0) * n_reads it chooses between the 2-D copy and the bus pack
    explicit WindowBatch(int64_t stride) : col0(stride) {}
    void add(const Window &w) {
        max_len = std::max(max_len, w.win);
        if (w.valid <= 0) return;
        win_total += w.valid;
        col0 = std::min(col0, w.first);
        col1 = std::max(col1, w.first + w.valid);
    }
};

// Running offset of packed rows that start on multiples of `round` samples (a power of two).
struct PackedOffset {
    int64_t round, next = 0;
    explicit PackedOffset(int64_t round_) : round(round_) {}
    int64_t take(int64_t samples) {
        const int64_t at = next;
        next += (samples + round - 1) & ~(round - 1);
        return at;
    }
};

}  // namespace wdx
