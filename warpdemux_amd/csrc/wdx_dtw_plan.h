// Which kernel a DTW dispatch against the resident reference set takes, in which operand layout, over which grid, and what
// has to be prepared for it -- the one statement of the rule (plain host C++17: no HIP, nothing of the context, so the system
// compiler builds it alone: tests/host/dtw_plan_check.cpp).  wdx_api.hip (dtw_rows_vs_refs) prepares what the plan names,
// wdx_dtw.hip (run_dtw_plan) launches it, and plan.info is what wdx_dtw_last_launch reports afterwards.
#pragma once
#include <stdint.h>

#include "../../include/wdx.h"
#include "wdx_dtw_wide.h"

namespace wdx {

// Largest Sakoe-Chiba window handled by the register-band kernels; wider / unbanded problems with L > this go to the
// scratch-row kernel (or, with WDX_OPT_WIDE_DTW, to the wide kernel: wdx_dtw_wide.h).
constexpr int kMaxRegWindow = 32;
// Zero samples either side of a uniform-operand row (the resident references; the padded reads of the refs-as-lanes
// layout): what the widest register band reads beyond a row's ends.
constexpr int kDtwHalo = kMaxRegWindow - 1;
inline int64_t dtw_padded_length(int64_t L) { return L + 2 * kDtwHalo; }

// Anti-diagonal wavefront kernel: one 16-lane row per pair, 16 pairs per 256-thread block, both series of a pair in LDS.
// It pays where the whole problem fits the machine at once (wdx_dtw.hip): few pairs, a band its 16 lanes cover.
constexpr int kWfPairsPerBlock = 16;  // 256 threads
constexpr int64_t kWfMaxPairs = 16384;
constexpr int kWfMaxWindow = 16;
constexpr int64_t kWfMaxL = 256;
// Batches from this size on go through the DTW kernel's row-major form (no transposed copy of the fingerprints:
// at 10 M reads the copy is 17.6 GB of traffic and 6 ms); below it the launch is latency-bound and the
// read-minor copy (a few MB, two tiny kernels) buys coalesced row loads: live ticks and minibatches measured
// 0.1-0.3 ms faster that way.
constexpr int64_t kRowMajorMinReads = 8192;
// The scratch-row kernel keeps two DP rows per lane in a global block sized for this many lanes: one launch per block.
constexpr int64_t kScratchLanes = 65536;
// Wave slots of the chip for the lane-per-pair kernels: 256 CUs x 4 SIMDs x 3 waves.
constexpr int64_t kDtwWaveSlots = 3072;

enum class DtwEntry {
    kMatrix,  // dtw_dev_locked: every route
    kFused,   // the fused device entries (demux_dev_rows): reads are the lanes, never the wavefront kernel, no scratch rows
};
struct DtwSwitches { bool no_wavefront = false, no_short_dtw = false, wide_dtw = false; };  // the knobs the decision reads
enum class DtwPrep {
    kNone,         // the row-major rows are read in place (and the wavefront kernel's inputs)
    kReadMinor,    // transposed copy (L, ld) of the reads plus one NaN flag per read
    kPaddedReads,  // refs-as-lanes: the reads become the uniform operand, (nX, Lpad) rows with a zero halo, plus NaN flags
};

struct DtwPlan {
    wdx_dtw_launch_info info{};  // what wdx_dtw_last_launch reports after the dispatch; family WDX_DTW_NONE: nothing to launch
    bool unsupported = false;    // a fused entry would need the scratch rows ("demux_dev needs window <= 32")
    int64_t L = 0, lanes = 0, rows = 0;  // series length; series the lanes run over (nA); uniform-operand series (nB)
    DtwPrep prep = DtwPrep::kNone;
    int64_t ld = 0;                         // kReadMinor: leading dimension of the copy; kPaddedReads: padded row length
    int64_t copy_bytes = 0, flag_bytes = 0; // of the copy and of its NaN flags
    bool argmin_after = false;   // the caller asked for the argmin and the kernel does not write it: launch_argmin follows
    int64_t lds_bytes = 0;       // dynamic LDS of a workgroup (wide, wavefront)
    int64_t scratch_bytes = 0;   // the scratch rows' global block
};

// (nX, L) reads against (nY, L) references, window as the caller gave it or effective.
inline DtwPlan dtw_plan(int64_t nX, int64_t nY, int64_t L, int64_t window, bool want_argmin, DtwEntry entry,
                        const DtwSwitches &sw) {
    DtwPlan P;
    if (L <= 0) return P;
    P.L = L;
    const bool matrix = entry == DtwEntry::kMatrix;
    const int32_t w = (int32_t)dtw_effective_window(L, window);
    const WideDtwPlan wide = wide_dtw_plan(L, w, sw.wide_dtw);   // (WDX_OPT_WIDE_DTW: the grid and argmin rules below are its too)
    const bool scratch = w > kMaxRegWindow && !wide.eligible;
    P.unsupported = scratch && !matrix;   // (whatever the batch, an empty one included)
    if (P.unsupported || nX <= 0 || nY <= 0) return P;
    P.argmin_after = want_argmin;   // (unless the kernel folds it in, below)
    // small problems: one launch of the anti-diagonal wavefront kernel straight from the row-major inputs (no transpose), then the argmin
    if (matrix && w <= kWfMaxWindow && L <= kWfMaxL && nX * nY <= kWfMaxPairs && !sw.no_wavefront) {
        P.info = {WDX_DTW_WAVEFRONT, 0, 0, WDX_DTW_LAYOUT_ROW_MAJOR, 0, 1, 1, w, (nX * nY + kWfPairsPerBlock - 1) / kWfPairsPerBlock, 1};
        P.lanes = nX, P.rows = nY;
        P.lds_bytes = kWfPairsPerBlock * 2 * L * (int64_t)sizeof(double);
        return P;
    }
    // lanes = reads unless there are too few of them to fill a wave and there are more refs
    // (few reads, many refs -- live / per-read calls: lanes = refs, the read is the uniform operand)
    const bool lanes_are_reads = !matrix || nX >= 64 || nX >= nY;
    // from kRowMajorMinReads on the kernel reads the row-major fingerprints as they are (a lane owns a row): no transposed copy
    int32_t layout = WDX_DTW_LAYOUT_ROW_MAJOR;
    P.lanes = nX, P.rows = nY;
    if (!lanes_are_reads) {
        layout = WDX_DTW_LAYOUT_REFS_AS_LANES;
        P.lanes = nY, P.rows = nX;
        P.prep = DtwPrep::kPaddedReads;
        P.ld = dtw_padded_length(L);
        P.copy_bytes = nX * P.ld * (int64_t)sizeof(double);
        P.flag_bytes = (nX + 63) / 64 * 64;
    } else if (scratch || nX < kRowMajorMinReads) {
        layout = WDX_DTW_LAYOUT_READ_MINOR;
        P.prep = DtwPrep::kReadMinor;
        P.ld = (nX + 63) / 64 * 64;
        P.copy_bytes = L * P.ld * (int64_t)sizeof(double);
        P.flag_bytes = P.ld;
    }
    const int64_t nA = P.lanes, nB = P.rows;
    if (scratch) {
        const int64_t launches = (nA + kScratchLanes - 1) / kScratchLanes;
        const int64_t last = nA - (launches - 1) * kScratchLanes;
        P.info = {WDX_DTW_SCRATCH, 0, 0, layout, 0, (int32_t)launches, (int32_t)nB, w, (last + 63) / 64, 1};
        P.scratch_bytes = 2 * (L + 1) * kScratchLanes * (int64_t)sizeof(double);
        return P;
    }
    const int64_t gx = (nA + 63) / 64;
    // one block walks `rpb` refs.  With enough a-series to fill 256 CUs x 8 waves a single block
    // walks them all and (if asked) folds the argmin in; otherwise the refs are split over grid.y
    // and the argmin is a second, tiny kernel.  (The kernel's argmin is per lane: only when the lanes are the reads.)
    bool fused = false;
    int64_t rpb = nB;
    if (gx >= 8 * kDtwWaveSlots || nB == 1 || (gx >= 2048 && nB < 32)) {
        fused = want_argmin && lanes_are_reads;
    } else {
        // A wave lives for the whole launch (one block = one wave walking its refs): with about as many waves as
        // the chip has slots (256 CUs x 4 SIMDs x 3 waves of this kernel = 3072) a few stragglers double the
        // launch time -- 1563 x 2 blocks ran at 67 % of the rate of the same kernel on a long grid.  Aim for
        // >= 8 waves per slot (dynamic balancing by the dispatcher), at least 16 refs per block.
        int64_t max_y = (nB + 15) / 16;
        int64_t want_y = (8 * kDtwWaveSlots + gx - 1) / gx;
        if (gx * max_y <= kDtwWaveSlots) {  // fits the chip at once anyway: latency-bound -- as many short blocks as it takes
            want_y = (2048 + gx - 1) / gx;
            max_y = nB;
        }
        if (want_y > max_y) want_y = max_y;
        if (want_y < 1) want_y = 1;
        rpb = (nB + want_y - 1) / want_y;
    }
    P.info = {WDX_DTW_BAND, 0, 0, layout, fused, 1, (int32_t)rpb, w, gx, (nB + rpb - 1) / rpb};
    P.argmin_after = want_argmin && !fused;
    if (wide.eligible) {
        P.info.family = WDX_DTW_WIDE;
        P.lds_bytes = wide.lds_bytes;
    } else if (L == 25 && w == 15 && !sw.no_short_dtw) {  // the shipped models' shape: fully unrolled
        P.info.family = WDX_DTW_SHORT, P.info.band_w = 15, P.info.exact_w = 1;
    } else {  // the band ladder; window 15 has an instantiation of its own without the per-cell window mask
        P.info.band_w = w == 15 ? 15 : (w <= 8 ? 8 : (w <= 16 ? 16 : 32));
        P.info.exact_w = w == 15;
    }
    return P;
}

// ---- the nearest-reference rule behind a dispatch (wdx_nearest_dev, wdx_demux_nearest_dev, wdx_dtw_nearest) ---------------
// Where the rule (label of the nearest reference, margin to the nearest reference of another label, thresholds) is computed:
//   kFused  in the DTW kernel's epilogue, beside what would be its argmin: the plan lets one lane walk all references of a read
//           (today's fused-argmin condition).  Without a `dist` output these launches write no distances at all.
//   kAfter  by nearest_rows_kernel on the (rows, nY) float32 matrix the dispatch wrote: references split over grid.y,
//           references as lanes, the wavefront kernel, the scratch rows -- and every route when a resident reference holds an
//           infinite sample (dtw_settle_inf rewrites entries of the matrix behind the kernels, so the matrix has to exist).
// kAfter without a `dist` output sends the distances through a context-owned block buffer of at most kNearestBlockBytes: the
// call is cut into row blocks of block_rows reads, each dispatched by its own plan.  plan.dtw is the dispatch of one such
// block (of the whole call when block_rows >= nX), and dtw.info.fused_argmin reports the decision: 1 = kFused.
enum class NearestRule { kNone, kFused, kAfter };
constexpr int64_t kNearestBlockBytes = 96ll << 20;
struct NearestPlan {
    DtwPlan dtw;
    NearestRule rule = NearestRule::kNone;  // kNone: nothing to dispatch (no reads, no references) or dtw.unsupported
    bool buffer = false;        // the distances go through the block buffer
    int64_t block_rows = 0;     // reads per dispatch
    int64_t buffer_bytes = 0;   // block_rows * nY * 4 when `buffer`
};

inline NearestPlan nearest_plan(int64_t nX, int64_t nY, int64_t L, int64_t window, bool have_dist, bool refs_any_inf, DtwEntry entry,
                                const DtwSwitches &sw) {
    NearestPlan N;
    N.dtw = dtw_plan(nX, nY, L, window, true, entry, sw);
    if (N.dtw.unsupported || N.dtw.info.family == WDX_DTW_NONE) return N;
    N.block_rows = nX;
    N.dtw.argmin_after = false;   // (the rule's own first-minimum column takes the argmin's place)
    if (N.dtw.info.fused_argmin && !refs_any_inf) {
        N.rule = NearestRule::kFused;
        return N;
    }
    N.rule = NearestRule::kAfter;
    N.dtw.info.fused_argmin = 0;
    if (have_dist) return N;
    N.buffer = true;
    int64_t rows = kNearestBlockBytes / (nY * (int64_t)sizeof(float));
    if (rows >= 64) rows -= rows % 64;
    if (rows < 1) rows = 1;
    if (rows < nX) {   // the plan of a full block; the caller plans the last, shorter one by its own size
        const NearestPlan B = nearest_plan(rows, nY, L, window, false, refs_any_inf, entry, sw);
        if (B.rule != NearestRule::kAfter) return B;   // (a block never fuses where the whole call did not; kept general)
        N = B;
    }
    N.buffer_bytes = N.block_rows * nY * (int64_t)sizeof(float);
    return N;
}

}  // namespace wdx
