// Which kernels one fingerprint call launches, in which order, over which grids, with which capacities and LDS sizes, and which
// device-side list each of them takes, hands over to and retries on -- the one statement of the rule (plain host C++17: no HIP,
// nothing of the context, so the system compiler builds it alone: tests/host/fp_plan_check.cpp replays the recorded route
// table through it and sweeps the parameter domain under the sanitizers).
//   constants, LDS formulae   what the decision reads; the device units use the same constexpr functions
//   fast_combo                which (window width, suppression reach) combinations have fast kernels
//   check_fingerprint_call    what a call is refused for, code and message
//   FpKernelKey, fp_key_exists   the name of a kernel instantiation and the table of the ones that are built
//   plan_fingerprint          the ordered steps of a call; decides everything, launches nothing
//   fp_slices                 how a step's extent is cut into launches
// wdx_fingerprint_launch.inc runs a plan step by step and decides nothing (run_fp_plan); wdx_fingerprint_fast.inc, the width
// units and wdx_clip.hip resolve a key to its kernel.
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/wdx.h"
#include "wdx_window.h"
#include "wdx_work_layout.h"

namespace wdx {

// ---- constants ------------------------------------------------------------------------------------------------------
constexpr int kMaxW = 64;        // cap on running_stat_width
constexpr int kMaxEvents = 253;  // cap on num_events (E + 2 boundaries <= 255)
constexpr int kSegCap = kMaxEvents + 1;
constexpr int kExactTile = 512;  // the exact kernel's t-score tile, positions (kTile: wdx_fingerprint.hip)
// Exact kernel: windows up to kExactLdsCap samples keep their float64 score curve in LDS (12-13 B per sample of the
// 160 KB); longer ones (up to WDX_MAX_ADAPTER_SAMPLES = kBigCap; the reference's RNA002 config allows
// max_obs_trace + 2*padding = 15 200, DEPRECATED/config_files/rna002_70bps@v0.4.4.toml:2) run the SAME code with
// the score curve in a per-workgroup HBM slot (L2-resident: 128 KB per slot) -- fingerprint_big_kernel.
constexpr int kExactLdsCap = 11200;
constexpr int kBigCap = WDX_MAX_ADAPTER_SAMPLES;
constexpr int kBigSlots = 256;  // one workgroup per CU (97 KB of LDS each)
static_assert(kBigCap % 64 == 0 && kBigCap >= 15200, "the exact path must take every window the reference accepts");
// WDX_OPT_LONG_WINDOWS: windows of kBigCap+1 .. kLongCap samples run the SAME code once more with the clipped float32
// samples in the workgroup's HBM slot too (fingerprint_long_kernel): beside the fixed tables LDS holds the peak-state
// bytes only (64 KB of the 160 KB).  A slot is 65 536 x (8 + 4) B = 768 KB; kLongSlots of them are 12 MB per context,
// allocated at the first call that sees such a window with the option on (fingerprint_long_bytes).
constexpr int kLongCap = WDX_MAX_LONG_ADAPTER_SAMPLES;
constexpr int kLongSlots = 16;
constexpr int kRefineMaxQuery = 96;   // LDS budget of the subsequence DP (direction words + three fronts)
constexpr int kRefineMaxSeries = 128;
constexpr int kHBits = 11;       // radix digit of the float32 medians (2048-bin histogram)
constexpr int kHB = 1 << kHBits; // histogram bins
constexpr int kClipWaves = 1;    // reads per workgroup of the one-wave clip kernels (wdx_clip.hip says why one)
constexpr int kClipWaveLongCap = 13312;  // the longest window of the one-wave clip kernel (208 samples per lane)
constexpr int kRouteBlock = 1024;        // route_long_windows_kernel: one thread per read

// Fast kernels' workgroup shape.  Two equivalent configurations were measured in round 1: 256 threads x 4 score
// positions per lane and 512 threads x 2 -- the same VALU instruction count and the same throughput; 256 threads
// keep one wave of a workgroup on each SIMD.
constexpr int kFastBlock = 256;  // threads per workgroup (FB in the kernels' include)
constexpr int kFW = 12;          // the default window width (RNA004); instantiations exist for 12, 18 and 30 (fast_body)
constexpr int kFSeg = 128;       // max segments (num_events + 1)
constexpr int kWideWgPerCu = 5;   // (WDX_WIDE_WG, tied in wdx_fingerprint_fast.inc) EXT main kernels of the NBT = 2 widths (6144 samples): workgroups per CU the registers are budgeted for
constexpr int kCapPMax = 2048;   // largest peak-list capacity
constexpr int kCapPMaxStream = 4 * 4 * kFastBlock;   // ... of the streaming form (fast_body: four 4-peak ownership rounds)
// samples per thread of the instantiations (4096 / 5120: five workgroups per CU, 6144: four, 8192: three)
constexpr int kNptSmall = 4096 / kFastBlock, kNptMid = 5120 / kFastBlock, kNptLarge = 6144 / kFastBlock, kNptHuge = 8192 / kFastBlock;
constexpr int kNptStream = 16384 / kFastBlock;
constexpr int kStreamBuf = 6 * kFastBlock;  // STREAM: samples per tile buffer (six per thread and tile)
constexpr int64_t kSplitSlice = 524288;   // reads per tile-kernel / tail-kernel launch pair (2.4 GB of lists; a pair boundary costs ~25 us: 131 072 -> 100.4, 262 144 -> 99.1, 1 M -> 98.1 ms of main pair per 10 M reads)
constexpr int kSplitWaves = 1;            // reads per workgroup of fingerprint_split_tail_kernel
static_assert(kSplitSlice == kWorkSplitSlice, "workspace layout: wdx_work_layout.h");
// sizeof(FastShared), sizeof(FpShared): the device unit ties them to the structs
constexpr size_t kFastSharedBytes = 488, kFpSharedBytes = 416;
constexpr size_t kLdsMax = 160 * 1024;   // LDS of a CU, and the most one workgroup may ask for

// ---- LDS formulae ---------------------------------------------------------------------------------------------------
constexpr size_t fp_up16(size_t b) { return (b + 15) & ~(size_t)15; }
constexpr size_t fast_sh_offset(int capF, int capP, int nbt = 1) {
    // sig | pad | pk_score capP | pad | pk_pos pad|capP|pad | pk_state pad|capP|pad, rounded up to 16; pad = 4 * nbt
    // entries either side (nbt = neighbour THREADS per side the suppression looks at: 1 for d_eff <= 9, 2 up to 17)
    return (((size_t)(capF + 32) * 4 + (size_t)(capP + 8 * nbt) * 8 + (size_t)(capP + 8 * nbt) * 2 +
             (size_t)(capP + 8 * nbt)) + 15) & ~(size_t)15;
}
constexpr size_t fast_stream_sh_offset(int capP, int nbt = 1) {
    // two tile buffers | pad | pk_score capP | pad | pk_pos | pk_state (as fast_sh_offset)
    return (((size_t)2 * kStreamBuf * 4 + (size_t)(capP + 8 * nbt) * 8 + (size_t)(capP + 8 * nbt) * 2 + (size_t)(capP + 8 * nbt)) +
            15) & ~(size_t)15;
}
constexpr size_t fast_lds_bytes(int capF, int capP, int nbt = 1) { return fp_up16(fast_sh_offset(capF, capP, nbt) + kFastSharedBytes); }
constexpr size_t fast_stream_lds_bytes(int capP, int nbt = 1) { return fp_up16(fast_stream_sh_offset(capP, nbt) + kFastSharedBytes); }
constexpr size_t clip_block_lds_bytes(int cap) { return fp_up16((size_t)(cap + 32) * 4 + (size_t)(kHB + 64) * 4 + kFastSharedBytes); }
constexpr size_t fp_lds_bytes(int cap) {
    size_t b = 0;
    b += (size_t)cap * 8;                        // scores
    b += (size_t)(kExactTile + kMaxW) * 8 * 2;   // Mt, Vt (+ state when it fits)
    b += (size_t)kSegCap * 8 * 3;                // ev, zz, tmp
    b += kFpSharedBytes;
    b += (size_t)cap * 4;                        // sig
    b += (size_t)256 * 4;                        // hist
    b += (size_t)(kSegCap + 1) * 4;              // cpts
    if (cap > (int)((kExactTile + kMaxW) * 16)) b += (size_t)cap;  // dedicated state
    return fp_up16(b);
}
constexpr size_t fp_lds_bytes_big(int cap) { return fp_lds_bytes(cap) - (size_t)cap * 8; }  // no score curve in LDS
// the long form keeps no samples and no score curve in LDS, and always the dedicated state bytes
constexpr size_t fp_lds_bytes_long() { return fp_lds_bytes(kLongCap) - (size_t)kLongCap * (8 + 4); }
static_assert(kLongCap > (kExactTile + kMaxW) * 16, "fp_lds_bytes counts the dedicated state bytes");

// ---- which combinations have fast kernels -----------------------------------------------------------------------------
// The fast kernels exist for three (window width, suppression reach) combinations -- the shipped parameter triples:
//   1: W = 12, d <= 9  (RNA004: 110, 6, 12)      every instantiation of the launch chain
//   2: W = 18, d <= 9  (tRNA triple: 120, 9, 18; the tRNA config itself also refines -> exact kernel)
//   3: W = 30, d <= 17 (RNA002 triple: 110, 15, 30)
// 2 runs the 5120-sample instantiation as main kernel for large batches (then 6144 and 8192 behind it, like 1); 3 the
// 6144-sample one, and the 8192-sample one for longer windows and retries.
//   4 .. 6: W = 6 / 24 / 36, d <= 17 (round 5: the other multiples of the tile's six positions per lane -- configurations
//           nobody ships, but `--export segmentation.running_stat_width=...` is one flag away, and the exact kernel
//           behind this gate runs at a fifteenth of the rate); instantiated like 3 (NBT = 2, 6144-sample main kernel)
//   7, 8: W = 12 / 18 with 9 < d <= 17: the same, for the shipped widths with a longer suppression reach.
inline int fast_combo(const wdx_seg_params &p) {
    if (p.min_obs_per_base < 1) return 0;
    if (p.running_stat_width == 12 && p.min_obs_per_base <= 9) return 1;
    if (p.running_stat_width == 18 && p.min_obs_per_base <= 9) return 2;
    if (p.running_stat_width == 30 && p.min_obs_per_base <= 17) return 3;
    if (p.running_stat_width == 6 && p.min_obs_per_base <= 17) return 4;
    if (p.running_stat_width == 24 && p.min_obs_per_base <= 17) return 5;
    if (p.running_stat_width == 36 && p.min_obs_per_base <= 17) return 6;
    if (p.running_stat_width == 12 && p.min_obs_per_base <= 17) return 7;   // (9 < d <= 17: the NBT = 2 form of the width)
    if (p.running_stat_width == 18 && p.min_obs_per_base <= 17) return 8;
    // 9 .. 37 (round 6): every other width from 7 to 35, d <= 17 -- widths that are not multiples of six, on the fast kernels'
    // EXACT-scores pass (the partner window's statistics come from another slot of a lane one further); no approximate keys,
    // no retry launch.  combo = 9 + (W - 7)
    if (p.min_obs_per_base <= 17 && p.running_stat_width >= 7 && p.running_stat_width <= 35 && p.running_stat_width % 6 != 0)
        return 9 + (p.running_stat_width - 7);
    return 0;
}
inline bool fast_combo_exact_only(int combo) { return combo >= 9; }

// ---- kernel keys ------------------------------------------------------------------------------------------------------
enum FpFamily : int {
    kFamFastMain,     // fingerprint_fast_kernel<npt, prof, fw, nbt, ext, split>
    kFamList1,        // fingerprint_fast_list1_kernel<npt, fw, nbt, split>: one workgroup per list entry
    kFamListStride,   // fingerprint_fast_list_kernel<npt, fw, nbt>: a fixed grid striding over a list
    kFamStream,       // fingerprint_fast_stream_kernel<fw, nbt>
    kFamSplitTail,    // fingerprint_split_tail_kernel<fw, nbt>
    kFamClip,         // clip_bounds_kernel<npl>
    kFamClipList,     // clip_bounds_list_kernel<npl>
    kFamClipBlock,    // clip_bounds_block_kernel
    kFamRoute,        // route_long_windows_kernel
    kFamExactChunks,  // fingerprint_kernel<block, prof>
    kFamExactList,    // fingerprint_list_kernel<block>
    kFamBig,          // fingerprint_big_kernel<block>
    kFamLong,         // fingerprint_long_kernel<block> (a refining call: fingerprint_long_refine_kernel, launch_fp_long_refine)
    // the refinement launchers keep their own grids (wdx_refine_*.hip); a step of these families calls one of them
    kFamRefineTail,     // launch_refine_tail: per slice the subsequence match, then the barcode tails' segmentation
    kFamRefineOptimal,  // the subsequence match per slice, then launch_refine_optimal once
    kFpFamilies
};
struct FpKernelKey {
    FpFamily family = kFamFastMain;
    int npt = 0;         // samples per thread (fast main, list1, striding list)
    bool prof = false;   // diagnostic build (fast main, exact chunks)
    int fw = 0, nbt = 0; // window width, neighbour threads per side (the fast families)
    bool ext = false;    // starts at the clip record (fast main)
    bool split = false;  // tile half of a split pair (fast main, list1)
    int npl = 0;         // samples per lane (clip, clip-list)
    int block = 0;       // workgroup size (the exact families)
};

// The (width, NBT) pairs the fast kernels are built for, and what each pair has:
//   kFull      combinations 1 .. 8: main kernels, both list kernels, the streaming kernel
//   kWide      exact-scores-only even widths: the 6144-sample main kernel, the striding list kernel, the streaming kernel
//   kWideOdd   exact-scores-only odd widths: the same without the streaming kernel
enum FpWidthClass : int { kNoWidth, kFull, kWide, kWideOdd };
constexpr FpWidthClass fp_width_class(int fw, int nbt) {
    if (nbt == 1) return fw == 12 || fw == 18 ? kFull : kNoWidth;
    if (nbt != 2) return kNoWidth;
    if (fw == 30 || fw == 6 || fw == 24 || fw == 36 || fw == 12 || fw == 18) return kFull;
    if (fw < 7 || fw > 35) return kNoWidth;
    return fw % 2 == 0 ? kWide : kWideOdd;
}
// NBT = 1 (reach <= 9): main kernels of 4096 (width 12 only), 5120 and 6144 samples, the diagnostic (PROF) builds for width 12
// only, the split pair of the 5120-sample main kernel and of the 6144-sample list launch.  NBT = 2: the 6144-sample main kernel,
// with a split pair for the widths whose EXT main kernel runs the filtered 512-entry list (multiples of six from 12 up).
constexpr bool fp_has_prof(int fw, int nbt) { return fw == kFW && nbt == 1; }
constexpr bool fp_has_split(int fw, int nbt) { return fp_width_class(fw, nbt) == kFull && (nbt == 1 || (fw >= 12 && fw % 6 == 0)); }
constexpr bool fp_clip_npl_exists(int npl) { return npl == 64 || npl == 80 || npl == 96 || npl == 128 || npl == kClipWaveLongCap / 64; }
// the table of instantiated keys: the resolvers answer for exactly these
constexpr bool fp_key_exists(const FpKernelKey &k) {
    const FpWidthClass wc = fp_width_class(k.fw, k.nbt);
    switch (k.family) {
        case kFamFastMain:
            if (wc == kNoWidth) return false;
            if (wc != kFull) return k.npt == kNptLarge && !k.prof && !k.split;
            if (k.nbt == 2) return k.npt == kNptLarge && !k.prof && (!k.split || (k.ext && fp_has_split(k.fw, 2)));
            if (k.prof && !fp_has_prof(k.fw, 1)) return false;
            if (k.npt == kNptMid) return k.ext;   // (always EXT; the tile half of the split pair exists with and without PROF)
            if (k.split) return false;
            return k.npt == kNptLarge || (k.npt == kNptSmall && fp_has_prof(k.fw, 1));
        case kFamList1: return wc == kFull && k.npt == kNptLarge && (!k.split || k.nbt == 1);
        case kFamListStride: return wc != kNoWidth && k.npt == kNptHuge;
        case kFamStream: return wc == kFull || wc == kWide;
        case kFamSplitTail: return fp_has_split(k.fw, k.nbt);
        case kFamClip: return fp_clip_npl_exists(k.npl);
        case kFamClipList: return k.npl == 96 || k.npl == 128 || k.npl == kClipWaveLongCap / 64;
        case kFamClipBlock: case kFamRoute: case kFamRefineTail: case kFamRefineOptimal: return true;
        case kFamExactChunks: case kFamExactList: return k.block == 512 || k.block == 1024;
        case kFamBig: case kFamLong: return k.block == 1024;
        default: return false;
    }
}
// samples per lane of the one-wave clip kernels for a capacity (0: none)
constexpr int clip_npl(int cap) { return cap <= 4096 ? 64 : (cap <= 5120 ? 80 : (cap <= 6144 ? 96 : (cap <= 8192 ? 128 : (cap <= kClipWaveLongCap ? kClipWaveLongCap / 64 : 0)))); }
constexpr int clip_list_npl(int cap) { return cap == 6144 ? 96 : (cap == 8192 ? 128 : (cap == kClipWaveLongCap ? kClipWaveLongCap / 64 : 0)); }

// ---- slicing ----------------------------------------------------------------------------------------------------------
// A launch over more workgroups than grid.x admits is cut into slices (grid.x * block.x must stay below 2^32).
// WDX_OPT_MAX_LAUNCH_SLICE lowers the built-in limits, so that the tests walk the multi-slice paths on small batches.
enum FpSliceRule : int {
    kOneLaunch,   // a fixed grid: never cut
    kEqualSlices, // EQUAL slices of at most the limit (the fast kernels with one workgroup per read or entry)
    kFullSlices,  // full slices of the limit and a remainder
};
constexpr int64_t fp_slice_limit(int64_t builtin, int64_t max_launch_slice) {
    return max_launch_slice > 0 && max_launch_slice < builtin ? max_launch_slice : builtin;
}
// for (i = 0; i < S.count; ++i): workgroups S.base(i) .. S.base(i) + S.n(i) - 1
struct FpSlices {
    int64_t extent, slice, count;
    int64_t base(int64_t i) const { return i * slice; }
    int64_t n(int64_t i) const { return extent - i * slice < slice ? extent - i * slice : slice; }
};
constexpr FpSlices fp_slices(int64_t extent, FpSliceRule rule, int64_t builtin, int64_t max_launch_slice) {
    if (extent <= 0) return {0, 1, 0};
    if (rule == kOneLaunch) return {extent, extent, 1};
    const int64_t limit = fp_slice_limit(builtin, max_launch_slice);
    int64_t slice = limit;
    if (rule == kEqualSlices) {
        const int64_t n_slices = (extent + limit - 1) / limit;
        slice = (extent + n_slices - 1) / n_slices;
    }
    return {extent, slice, (extent + slice - 1) / slice};
}
constexpr int64_t kFastSliceLimit = (1ll << 31) / kFastBlock;   // kEqualSlices of the fast kernels

// ---- what the decision reads of a call --------------------------------------------------------------------------------
struct FpSwitches {   // of Knobs (Knobs::fp_switches())
    bool exact_path = false;
    int fast_peak_cap = 0, fast_main_cap = 0;
    int64_t fast_chain_min = 0;
    bool fast_exact_scores = false, no_clip_reuse = false, no_wave_clip_long = false, no_peak_filter = false, no_split = false;
    int64_t max_launch_slice = 0;
    bool long_windows = false, long_refine_windows = false, refine_optimal = false;
    bool long_form(bool refine) const { return long_form_on(refine, long_windows, long_refine_windows); }
};
struct PlanFlags {
    bool has_ws;      // the caller gave a workspace
    bool prof;        // diagnostic build (d_prof)
    int stop_phase;
    bool has_big;     // the caller gave the buffer of fingerprint_big_bytes
    bool has_long;    // ... and the one of fingerprint_long_bytes
    bool refine;      // consensus-refinement branch
    bool refine_ws;   // ... with the fast kernels' hand-over records (RefineDev::ws)
};
// what the checks read of a refining call's RefineDev
struct FpRefineView {
    bool has_query;
    int nq, E2, psi1b, psi2b;
};

// ---- refusals ---------------------------------------------------------------------------------------------------------
enum FpRefusal : int {
    kFpOk, kFpTooManyReads, kFpNumEvents, kFpBarcodeEvents, kFpWidth, kFpPadding, kFpRefineQuery, kFpRefineEvents,
    kFpOptimalWithLong, kFpOptimalMinObs, kFpOptimalNorm, kFpLds, kFpNoFastKernels, kFpTooManySteps, kFpRefusals
};
struct FpCheck {   // code != WDX_SUCCESS: refused, and msg is the call's wdx_last_error()
    int code = WDX_SUCCESS;
    FpRefusal why = kFpOk;
    char msg[160] = "";
};
__attribute__((format(printf, 3, 4))) inline FpCheck fp_refuse(FpRefusal why, int code, const char *fmt, ...) {
    FpCheck r;
    r.code = code;
    r.why = why;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(r.msg, sizeof r.msg, fmt, ap);
    va_end(ap);
    return r;
}
inline FpCheck check_fingerprint_call(int64_t n_reads, const wdx_seg_params &p, const FpRefineView *rf, const PlanFlags &f,
                                      const FpSwitches &sw) {
    if (n_reads > 0x7fffffffLL) return fp_refuse(kFpTooManyReads, WDX_ERR_INVALID, "at most 2^31-1 reads per call");
    if (p.num_events < 1 || p.num_events > kMaxEvents)
        return fp_refuse(kFpNumEvents, p.num_events < 1 ? WDX_ERR_INVALID : WDX_ERR_UNSUPPORTED, "num_events must be in [1, %d]", kMaxEvents);
    if (p.barcode_num_events < 1 || p.barcode_num_events > kSegCap)
        return fp_refuse(kFpBarcodeEvents, WDX_ERR_INVALID, "barcode_num_events must be in [1, %d]", kSegCap);
    if (p.running_stat_width < 0 || p.running_stat_width > kMaxW)
        return fp_refuse(kFpWidth, WDX_ERR_UNSUPPORTED, "running_stat_width must be in [0, %d]", kMaxW);
    if (p.padding < 0) return fp_refuse(kFpPadding, WDX_ERR_INVALID, "padding must be >= 0");
    if (rf) {
        if (!rf->has_query || rf->nq < 1 || rf->nq > kRefineMaxQuery || p.num_events + 1 > kRefineMaxSeries)
            return fp_refuse(kFpRefineQuery, WDX_ERR_UNSUPPORTED,
                             "consensus refinement: the query must have 1..%d points and num_events + 1 <= %d", kRefineMaxQuery,
                             kRefineMaxSeries);
        if (rf->E2 < 1 || rf->E2 > kMaxEvents || rf->psi1b < 0 || rf->psi2b < 0)
            return fp_refuse(kFpRefineEvents, WDX_ERR_INVALID,
                             "consensus refinement: barcode_num_events[0] must be in [1, %d], psi >= 0", kMaxEvents);
        if (sw.refine_optimal) {
            if (sw.long_refine_windows)
                return fp_refuse(kFpOptimalWithLong, WDX_ERR_UNSUPPORTED,
                                 "WDX_OPT_REFINE_OPTIMAL_CPTS and WDX_OPT_LONG_REFINE_WINDOWS do not go together");
            if (p.min_obs_per_base < 1)
                return fp_refuse(kFpOptimalMinObs, WDX_ERR_UNSUPPORTED, "optimal change-points: min_obs_per_base must be >= 1");
            if (p.sig_norm != WDX_NORM_NONE || !f.refine_ws)   // (what the record path does not serve: wdx.h)
                return fp_refuse(kFpOptimalNorm, WDX_ERR_UNSUPPORTED,
                                 "optimal change-points: sig_extract.normalization must be \"none\"");
        }
    }
    return FpCheck{};
}

// the two refusals of a plan: the exact kernel's carve-up beyond the LDS, a main kernel that is not built
inline FpCheck check_fp_lds(size_t lds) {
    if (lds > kLdsMax) return fp_refuse(kFpLds, WDX_ERR_INVALID, "fingerprint LDS carve-up (%zu B) exceeds 160 KiB", lds);
    return FpCheck{};
}
inline FpCheck check_fp_main_kernel(const FpKernelKey &k) {
    if (!fp_key_exists(k)) return fp_refuse(kFpNoFastKernels, WDX_ERR_INVALID, "no fast kernels for running_stat_width %d", k.fw);
    return FpCheck{};
}

// ---- plan -------------------------------------------------------------------------------------------------------------
// The read lists of the workspace (wdx_work_layout.h), by the counter that counts each
enum FpCounter : int {
    kCntSlow = 0,   // reads for the exact general kernel
    kCntBig0,       // beyond the main instantiation -> 6144-sample list kernel
    kCntBig1,       // -> 8192-sample list kernel; with the streaming kernel in the chain: its own exact-scores retry list
    kCntRetry,      // an order decision inside the error band of the approximate keys -> redone on exact scores
    kCntBig2,       // windows beyond 6144 samples -> streaming kernel
    kCntBack,       // refinement: barcode tails back from the tail kernel to the exact kernel
    kCntBackTie,    // (diagnostic, back + 1: a run of equal scores across a tile's end)
    kCntBackList,   // (diagnostic, back + 2: beyond the tail kernel's peak list)
    kFpCounters
};
static_assert(kFpCounters == kWorkCounters && kCntBack + 1 == kWorkLists, "workspace layout: wdx_work_layout.h");
constexpr int kNoList = -1;
enum FpEventSlot : int { kEvNone, kEvClip, kEvMain, kEvOptimal };   // the pair of MainEvents that brackets a step

struct FpStep {
    FpKernelKey key;
    int capF = 0, capP = 0;   // the fast families' capacities; clip families and kFamBig: capF = the window capacity
    size_t lds = 0;           // dynamic LDS bytes
    int in = kNoList;         // the list it takes (kNoList: every read of the call) ...
    int64_t in_start = 0;     // ... from this entry on (the striding kernel behind a bounded grid)
    int over = kNoList;       // the list it hands over to
    int retry = kNoList;      // the list it retries on
    bool exact_scores = true;
    bool clip = false;        // the fast families: starts at the reads' clip records; the exact families: takes them where CLIP_OK
    bool routed = false;      // windows beyond capF are on `over` already (the route step ran)
    bool refine_record = false;
    bool defer = false;       // clip-list: leaves what it may not decide to the clip-block step behind it
    int64_t extent = 0;       // workgroups in all ...
    int per_wg = 1;           // ... each of this many reads or entries
    int wg = 0;               // workgroup size
    FpSliceRule rule = kOneLaunch;
    int64_t slice_limit = 0;  // built-in slice limit, workgroups
    bool split_tile = false;  // tile half of a split pair: the next step is its tail, launched slice by slice behind it
    bool counted = false;     // its launches are the ones the call reports (n_launches)
    FpEventSlot ev = kEvNone; // (a split tail under kEvMain: one pooled pair per slice around it too)
};
constexpr int kFpMaxSteps = 24;
struct FpPlan {
    enum Path { kProfExact, kChain, kExact } path = kExact;
    // the exact general kernel (every path ends in it)
    int cap = 0;          // samples of its LDS carve-up
    bool with_huge = false;   // fingerprint_big_kernel behind it
    bool with_long = false;   // fingerprint_long_kernel behind that (WDX_OPT_LONG_WINDOWS)
    // the chain
    bool approx = false;      // approximate score keys first (else exact scores from the first attempt)
    bool filt = false;        // threshold filter of the peak appends
    bool ext = false;         // clip-ahead: clip_bounds_kernel runs ahead of the main kernel (EXT instantiations)
    bool clip_reuse = false;  // the exact kernel behind the chain takes the reads' clip records
    bool refine = false;
    bool with_stream = false; // (what kCntBig1 counts: print_chain_counters)
    int n_steps = 0;
    FpStep steps[kFpMaxSteps];
    FpCheck refused;          // code != WDX_SUCCESS: nothing to run
    FpStep &add(FpFamily fam) {   // (beyond the capacity: the plan is refused, nothing of it runs)
        if (n_steps == kFpMaxSteps) {
            refused = fp_refuse(kFpTooManySteps, WDX_ERR_INVALID, "fingerprint plan: more than %d steps", kFpMaxSteps);
            --n_steps;
        }
        FpStep &s = steps[n_steps++];
        s = FpStep{};
        s.key.family = fam;
        return s;
    }
};

// clip_bounds_kernel over a whole batch: one wave per read
inline FpStep fp_clip_step(int cap, int64_t n_reads) {
    FpStep s;
    s.key.family = kFamClip, s.key.npl = clip_npl(cap);
    s.capF = cap;
    s.extent = (n_reads + kClipWaves - 1) / kClipWaves, s.per_wg = kClipWaves, s.wg = kClipWaves * 64;
    s.rule = kFullSlices, s.slice_limit = 1ll << 22;
    return s;
}
inline int64_t fp_min(int64_t a, int64_t b) { return a < b ? a : b; }
inline int64_t fp_max(int64_t a, int64_t b) { return a > b ? a : b; }

// p and n_reads as check_fingerprint_call accepted them
inline FpPlan plan_fingerprint(const wdx_seg_params &p, int64_t max_len, int64_t n_reads, const FpSwitches &knobs, const PlanFlags &f) {
    FpPlan pl;
    int64_t cap64 = max_len;
    if (cap64 > kExactLdsCap) cap64 = kExactLdsCap;
    if (cap64 < 64) cap64 = 64;
    const int cap = pl.cap = (int)((cap64 + 63) / 64 * 64);
    const size_t lds = fp_lds_bytes(cap);
    if ((pl.refused = check_fp_lds(lds)).code) return pl;
    const int block = lds <= 80 * 1024 ? 512 : 1024;   // the exact kernels' workgroup
    // windows of kExactLdsCap+1 .. kBigCap samples: left alone by every launch below and taken by
    // fingerprint_big_kernel at the end (needs the caller's fingerprint_big_bytes(max_len) buffer; without it they
    // are reported WDX_READ_FAIL_UNKNOWN as windows beyond WDX_MAX_ADAPTER_SAMPLES always are)
    pl.with_huge = max_len > kExactLdsCap && f.has_big && !f.prof;
    // WDX_OPT_LONG_WINDOWS (the refinement branch: WDX_OPT_LONG_REFINE_WINDOWS): windows of kBigCap+1 .. kLongCap samples are
    // left alone in the same way and taken by fingerprint_long_kernel behind that (the caller's
    // fingerprint_long_bytes(max_len) buffer), which refines in place where the call refines
    pl.with_long = knobs.long_form(f.refine) && max_len > kBigCap && f.has_long && pl.with_huge;
    const bool optimal = f.refine && knobs.refine_optimal;
    // the steps every path ends in
    auto exact_chunks = [&](bool prof, bool clip, bool record) {
        FpStep &s = pl.add(kFamExactChunks);
        s.key.block = block, s.key.prof = prof;
        s.lds = lds, s.clip = clip, s.refine_record = record;
        s.extent = n_reads, s.wg = block, s.counted = true;
        // HIP drops work when grid.x * block.x reaches 2^32: launch in slices of 2^21 reads
        s.rule = kFullSlices, s.slice_limit = 1 << 21;
    };
    auto exact_list = [&](int list, bool clip, bool record, int max_grid) {
        FpStep &s = pl.add(kFamExactList);
        s.key.block = block;
        s.lds = lds, s.in = list, s.clip = clip, s.refine_record = record, s.exact_scores = !pl.approx;
        s.extent = fp_min(n_reads, max_grid), s.wg = block;
    };
    auto big = [&](int list, bool clip, bool record) {   // a fixed grid of <= kBigSlots workgroups strides over the list (or over all reads)
        FpStep &s = pl.add(kFamBig);
        s.key.block = 1024;
        s.capF = cap, s.lds = fp_lds_bytes_big(kBigCap), s.in = list, s.clip = clip, s.refine_record = record, s.exact_scores = !pl.approx;
        s.extent = fp_min(n_reads, kBigSlots), s.wg = 1024;
    };
    auto long_form = [&](int list) {
        FpStep &s = pl.add(kFamLong);
        s.key.block = 1024;
        s.lds = fp_lds_bytes_long(), s.in = list, s.exact_scores = !pl.approx;
        s.extent = fp_min(n_reads, kLongSlots), s.wg = 1024;
    };
    // WDX_OPT_REFINE_OPTIMAL_CPTS: every read of the call has left a record by now (the fast kernels, the exact kernel and its big
    // form alike); the subsequence match for all of them, then the optimal change-points of their barcode tails -- one launch
    // whose workgroups stride over the reads, each with its slot of the context's scratch buffer (WDX_K_REFINE_OPTIMAL)
    auto refine_optimal = [&](bool clip) {
        FpStep &s = pl.add(kFamRefineOptimal);
        s.clip = clip, s.exact_scores = !pl.approx;
        s.extent = n_reads, s.wg = 64, s.rule = kFullSlices, s.slice_limit = 1 << 22, s.ev = kEvOptimal;
    };
    auto clip_ahead = [&](int capc, FpEventSlot ev) {
        FpStep &s = pl.add(kFamClip);
        s = fp_clip_step(capc, n_reads);
        s.exact_scores = !pl.approx, s.ev = ev;
    };
    if (f.prof && !f.has_ws) {
        pl.path = FpPlan::kProfExact;
        exact_chunks(true, false, false);
        return pl;
    }
    const int64_t chain_min = knobs.fast_chain_min > 0 ? knobs.fast_chain_min : 2048;
    const bool large_batch = n_reads >= chain_min;
    const int combo = fast_combo(p);
    // fast path for the common case + exact slow path for whatever it declines
    // (the fast kernels take reads whose EFFECTIVE parameters are window width 12 and distance <= 9; with a configured
    // width other than 12 or a configured distance beyond 9 only a few very short reads would qualify -- sig_proc.py:
    // 526-533 shrinks the parameters for those -- and a launch chain whose main kernel declines nearly every read
    // costs more than it saves: 1.62 against 1.99 M reads/s on the RNA002 triple (110, 15, 30))
    const bool fast_ok = f.has_ws && p.sig_norm == WDX_NORM_NONE &&   // (accept_less_cpts: the fast kernels hand over the reads it concerns)
                         p.num_events <= kFSeg - 2 && p.barcode_num_events <= p.num_events + 1 &&
                         combo != 0 && (combo == 1 || !f.prof) && cap >= 512 && !knobs.exact_path &&
                         (!f.refine || (f.refine_ws && !f.prof && p.num_events + 1 <= 128));
    if (!fast_ok) {
        // The exact kernel for the whole batch (a window width or suppression reach without a fast instantiation, a signal
        // normalisation, WDX_OPT_EXACT_PATH): large batches still get their clip bounds from the one-wave kernel first (windows
        // up to 13 312 samples; 4.5 ms per million reads against the exact kernel's ~100 for its two workgroup-wide medians)
        pl.path = FpPlan::kExact;
        const bool clip = f.has_ws && !f.prof && !knobs.no_clip_reuse && large_batch;
        if (clip) clip_ahead(max_len <= 4096 ? 4096 : (max_len <= 5120 ? 5120 : (max_len <= 6144 ? 6144 : (max_len <= 8192 ? 8192 : kClipWaveLongCap))), kEvNone);
        exact_chunks(false, clip, optimal);   // (optimal: every read leaves a record, the refine-optimal step does the rest)
        if (pl.with_huge) big(kNoList, clip, optimal);
        if (optimal) refine_optimal(clip);
        else if (pl.with_long) long_form(kNoList);
        return pl;
    }
    // A chain of launches, each handing what it cannot take to the next through device-side lists:
    //   main    one workgroup per read; the instantiation follows the longest adapter window of the batch:
    //           4096 or (large batches) 5120 samples at FIVE workgroups per CU, else 6144 at four.  A fifth
    //           resident workgroup is worth 1.16x (tools/probes/occupancy_probe.py); 89 % of RNA004 adapter
    //           windows fit 5120 samples
    //   big0    windows (and peak lists) beyond the main instantiation -> 6144-sample list kernel
    //   big1    beyond that -> 8192-sample list kernel (three workgroups per CU)
    //   retry   reads whose approximate score keys left an order decision inside the error band (about 2 in
    //           1000) -> 8192-sample list kernel with exact scores
    //   slow    everything else (NaNs, other window widths, long plateaus, ...) -> the exact general kernel
    // Small batches (live ticks) skip the approximate keys, and with them the retry launch, and go straight
    // to the 6144-sample instantiation: there a launch costs more than the arithmetic saved.
    // Peak-list capacities: local maxima of the score curve run at ~N/5.6 (>= N/5.0 observed); the capacities
    // leave headroom within the LDS budget of the instantiation's occupancy; overflows move up the chain.
    pl.path = FpPlan::kChain;
    pl.refine = f.refine;
    const int fw = p.running_stat_width;
    const bool approx = pl.approx = large_batch && !knobs.fast_exact_scores && !fast_combo_exact_only(combo);
    const int nbt = combo >= 3 ? 2 : 1;
    int capF = cap <= 4096 ? 4096 : (large_batch ? 5120 : 6144);
    if (knobs.fast_main_cap == 5120 || knobs.fast_main_cap == 6144) capF = knobs.fast_main_cap;  // experiments
    if (combo == 2) capF = large_batch ? 5120 : 6144;  // width 18: five workgroups per CU too (91 VGPRs)
    if (combo >= 3) capF = 6144;  // width 30 / reach 17 (and the round-5 widths): 115 VGPRs, four waves per SIMD either way
    // (LDS is allocated in 1280-byte granules: five workgroups per CU need <= 32 000 B each, four <= 40 960 B --
    // hipOccupancyMaxActiveBlocksPerMultiprocessor does not know and reports five at 32 640 B)
    // Large batches: the clip bounds of the MAIN kernel's reads are computed ahead of it by clip_bounds_kernel (one wave
    // per read, wdx_clip.hip) and the main kernel starts at the clip (EXT instantiation).  Small batches (live ticks:
    // every launch counts) keep the in-kernel radix selects.
    const bool ext = pl.ext = large_batch || capF == 5120;
    int capP = capF == 4096 ? 1152 : (capF == 5120 ? 980 : 1376);
    // with the threshold filter of the appends (kPeakTauLo) a read lists ~340 peaks instead of ~830: 512 entries leave the
    // 5120-sample main kernel at 26.8 KB of LDS -- six workgroups per CU (a longer list moves on to the list kernels).
    // (the width-30 instantiations, NBT = 2, are bound by their registers at four: they keep the long lists, except
    // the streaming form)
    const bool filt = pl.filt = approx && !knobs.no_peak_filter;   // (the launches on approximate keys below)
    if (ext && filt && nbt == 1 && capF <= 5120) capP = 512;
    // the NBT = 2 widths' 6144-sample main kernel at FIVE workgroups per CU: 96 VGPRs (launch bound) and the filtered
    // 512-entry list -- 31 000 B of LDS (five need <= 32 000); longer lists move on to the list kernel
    // (not width 6: its reach-3 lists are the longest -- 512 entries overflow for most reads, 23.3 -> 22.8 M reads/s)
    if (ext && filt && nbt == 2 && capF == 6144 && kWideWgPerCu == 5 && fw >= 12) capP = 512;
    if (knobs.fast_peak_cap > 0) capP = knobs.fast_peak_cap;  // experiment knob (wdx_ctx_set_option)
    const size_t flds = fast_lds_bytes(capF, capP, nbt);
    const bool chain = !(f.prof && f.stop_phase > 0);   // (ablation timing: the main kernel alone; the lists are left unprocessed)
    const bool with_big0 = chain && capF == 5120;      // windows of 5121..6144 samples, peak-list overflows
    // windows beyond 6144 samples, up to WDX_MAX_ADAPTER_SAMPLES: the streaming fast kernel (at 8 000 samples it is
    // faster than the striding 8192-sample list kernel, which then only serves list overflows and exact-score retries)
    // (odd widths are instantiated without the streaming form: their windows beyond 8192 samples take the exact kernel)
    const bool has_stream = !(fast_combo_exact_only(combo) && (fw & 1));
    const bool with_stream = pl.with_stream = chain && ext && capF >= 5120 && max_len > 6144 && has_stream;
    const bool with_big1 = chain && capF >= 5120 && cap > 6144 && !with_stream;  // windows of 6145..8192 samples
    const bool with_retry = approx && chain;
    const int main_over = with_big0 ? kCntBig0 : (with_stream ? kCntBig2 : (with_big1 ? kCntBig1 : kNoList));
    const int main_retry = approx ? kCntRetry : kNoList;
    FpKernelKey kmain{kFamFastMain};
    kmain.npt = capF / kFastBlock, kmain.prof = f.prof, kmain.fw = fw, kmain.nbt = nbt, kmain.ext = ext;
    if ((pl.refused = check_fp_main_kernel(kmain)).code) return pl;
    // The SPLIT form of the main kernel (large batches on approximate keys with the filtered 512-entry list -- the RNA004
    // triple, width 18, and the NBT = 2 widths from 12 up): the workgroup-per-read kernel ends after the tile pass and exports
    // the <= 256 peaks that can matter, one WAVE per read does the rest (fingerprint_split_tail_kernel) -- launch pairs over
    // slices of kSplitSlice reads, whose lists live in the workspace behind the read lists.  Not for the diagnostic builds
    // (the one-piece kernel serves those).
    // (not the refinement branch: measured 2.36 against 2.15 ms per 32 768 tRNA-like reads with the one-piece kernel)
    // (stop_phase == -2: the diagnostic build of the RNA004 pair, wdx_fingerprint_profile_dev's fast_path = 2)
    const bool prof_split = f.prof && f.stop_phase == -2 && combo == 1 && capF == 5120;
    FpKernelKey ktile = kmain;
    ktile.split = true;
    const bool split = fp_key_exists(ktile) && ext && approx && filt && capP == 512 && chain && (!f.prof || prof_split) && !f.refine && !knobs.no_split;
    // the list kernels
    const int64_t grid = n_reads < 1024 ? n_reads : 1024;  // striding kernels: every CU busy, nothing more
    const int capF1 = 6144, capP1 = 1376, capF2 = 8192, capP2 = 1856;
    // the same kernels behind filtered appends (the approximate-keys launches; the exact-scores retry keeps the long
    // lists): 512 entries -> five workgroups per CU at 6144 samples, four at 8192
    // (the striding 8192-sample kernel is NOT an EXT instantiation: its in-kernel medians put their 2112-word histogram
    // where the peak list will be, so its list region must hold 8448 bytes -- 768 entries, not 512)
    const int capP1f = filt && nbt == 1 ? 512 : capP1, capP2f = filt && nbt == 1 ? 768 : capP2;

    auto fast_step = [&](FpFamily fam, int cF, int cP, int in) -> FpStep & {
        FpStep &s = pl.add(fam);
        s.key.fw = fw, s.key.nbt = nbt;
        s.capF = cF, s.capP = cP, s.in = in, s.exact_scores = !approx, s.wg = kFastBlock;
        return s;
    };
    // a tile kernel's other half: one wave per read or entry of the slice (slot = workgroup of the slice)
    auto split_tail = [&](const FpStep &tile) {
        FpStep &s = fast_step(kFamSplitTail, tile.capF, tile.capP, tile.in);
        s.over = tile.over, s.retry = tile.retry, s.clip = tile.clip, s.routed = tile.routed;
        s.extent = (tile.extent + kSplitWaves - 1) / kSplitWaves, s.per_wg = kSplitWaves, s.wg = kSplitWaves * 64;
        s.rule = tile.rule, s.slice_limit = tile.slice_limit, s.ev = tile.ev;
    };
    // one workgroup per entry of a list, behind clip records
    auto list1 = [&](int cP, int in, int over, int retry, int64_t n, bool exact, bool pair) {
        FpStep &s = fast_step(kFamList1, capF1, cP, in);
        s.key.npt = kNptLarge, s.key.split = pair;
        s.lds = fast_lds_bytes(capF1, cP, nbt), s.over = over, s.retry = retry, s.clip = true, s.exact_scores = exact || !approx;
        s.extent = n, s.rule = pair ? kFullSlices : kEqualSlices, s.slice_limit = pair ? kSplitSlice : kFastSliceLimit;
        s.split_tile = pair;
        if (pair) split_tail(s);
    };
    // the striding 8192-sample kernel for the entries of a list from `start` on
    auto stride = [&](int cP, int in, int64_t start, int over, int retry, bool exact) {
        FpStep &s = fast_step(kFamListStride, capF2, cP, in);
        s.key.npt = kNptHuge;
        s.lds = fast_lds_bytes(capF2, cP, nbt), s.in_start = start, s.over = over, s.retry = retry, s.exact_scores = exact || !approx;
        s.extent = grid;
    };
    auto clip_list = [&](int capc, int in, int64_t n, bool defer) {
        FpStep &s = pl.add(kFamClipList);
        s.key.npl = clip_list_npl(capc);
        s.capF = capc, s.in = in, s.defer = defer, s.exact_scores = !approx;
        s.extent = (n + kClipWaves - 1) / kClipWaves, s.per_wg = kClipWaves, s.wg = kClipWaves * 64;
        s.rule = kFullSlices, s.slice_limit = 1ll << 22;
    };

    // A1 for the main kernel's reads (windows of 256 .. capF samples; longer ones are flagged CLIP_NONE and the main kernel
    // hands them to the lists before it would look at their record)
    bool routed = false;
    if (ext) {
        clip_ahead(capF, kEvClip);
        if (main_over != kNoList) {   // the windows beyond capF go on the main kernel's hand-over list here (one atomic per 64 reads)
            FpStep &s = pl.add(kFamRoute);
            s.capF = capF, s.over = main_over, s.exact_scores = !approx;
            s.extent = (n_reads + kRouteBlock - 1) / kRouteBlock, s.per_wg = kRouteBlock, s.wg = kRouteBlock;
            s.rule = kFullSlices, s.slice_limit = 1ll << 21, s.ev = kEvClip;
            routed = true;
        }
    }
    {
        FpStep &s = fast_step(kFamFastMain, capF, capP, kNoList);
        s.key = split ? ktile : kmain;
        s.lds = flds, s.over = main_over, s.retry = main_retry, s.clip = ext, s.routed = routed;
        s.extent = n_reads, s.rule = split ? kFullSlices : kEqualSlices, s.slice_limit = split ? kSplitSlice : kFastSliceLimit;
        s.split_tile = split, s.counted = true, s.ev = kEvMain;
        if (split) split_tail(s);
    }
    // windows of capF + 1 .. 6144 samples and the main kernel's peak-list overflows
    if (with_big0) {
        // 11 % of RNA004 adapter windows are longer than 5120 samples: a grid for a quarter of the batch, one
        // workgroup per list entry, and the striding 8192-sample kernel for whatever lies beyond it
        const int64_t g1 = fp_min(n_reads, fp_max(1024, n_reads / 4));
        clip_list(6144, kCntBig0, g1, false);
        // the same pair over the list's entries (slot = workgroup of the slice; most of the grid lies past the list's end
        // and leaves at once, in both kernels)
        FpKernelKey kl1s{kFamList1};
        kl1s.npt = kNptLarge, kl1s.fw = fw, kl1s.nbt = nbt, kl1s.split = true;
        list1(capP1f, kCntBig0, with_stream ? kCntBig2 : (with_big1 ? kCntBig1 : kNoList), main_retry, g1, false,
              split && fp_key_exists(kl1s) && capP1f == 512);
        if (g1 < n_reads) stride(capP2f, kCntBig0, g1, with_stream ? kCntBig2 : kNoList, main_retry, false);
    }
    // windows of 6145 .. 8192 samples when the streaming kernel is not in the chain
    if (with_big1) stride(capP2f, kCntBig1, 0, kNoList, main_retry, false);
    if (with_stream) {
        // windows of 6145 .. 16384 samples (RNA002: max_obs_trace + 2 * padding = 15 200): their clip bounds by one
        // workgroup per list entry (samples in LDS), then the streaming form of the fast body -- its LDS is the peak
        // list plus two tile buffers, whatever the window length: four workgroups per CU up to 12 288 samples, three
        // up to 16 384.  One workgroup per entry; the list's length is only known on the device.  With windows beyond
        // 8192 samples in the batch (RNA002-length reads: every read is on this list) the grids cover the batch; up to
        // 8192 the long windows are a tail of the batch (687 of 10 M synthetic RNA004 reads) and, for batches of more
        // than 2 M reads, the grids cover a sixteenth of it -- a workgroup past the list's end leaves at once, but 10 M of
        // them cost a millisecond per launch -- with the striding 8192-sample kernel behind them for whatever lies
        // beyond.  Doubts and refusals go to the exact kernel.
        const int scap = max_len <= 8192 ? 8192 : (max_len <= 12288 ? 12288 : 16384);
        const int capPs = filt ? (scap == 8192 ? 1024 : (scap == 12288 ? 1280 : 1536))   // (the list from kPeakTauLo up)
                               : (scap == 8192 ? 1700 : (scap == 12288 ? 2520 : 3400));
        // (WDX_OPT_MAX_LAUNCH_SLICE, the tests' switch for the multi-launch paths, also selects the bounded grids)
        const int64_t g5 = (scap == 8192 && (n_reads > (1ll << 21) || knobs.max_launch_slice > 0)) ? fp_max(1, n_reads / 16) : n_reads;
        // the one-wave clip kernel first (samples in registers, no barriers: twice the block kernel's rate per sample at
        // two workgroups of four reads per CU) for the windows its register file holds -- 8192 samples at 128 per lane,
        // 13 312 at 208; the workgroup kernel then finds a record for those and serves the rest: longer windows, and
        // the ones the wave form may not decide (negative samples it cannot clamp away)
        if (!knobs.no_wave_clip_long) clip_list(scap == 8192 ? 8192 : kClipWaveLongCap, kCntBig2, g5, true);
        {
            FpStep &s = pl.add(kFamClipBlock);
            s.capF = scap, s.lds = clip_block_lds_bytes(scap), s.in = kCntBig2, s.exact_scores = !approx;
            s.extent = g5, s.wg = kFastBlock, s.rule = kFullSlices, s.slice_limit = 1ll << 22;
        }
        // batches of long windows (beyond 8192 samples: the grids cover the batch anyway): a read with a decision inside
        // the error band, or whose cut does not clear the append filter's threshold, is redone by a second launch of the
        // same kernel on exact scores with the unfiltered list capacity -- instead of the exact general kernel, which
        // serves such a window at a twentieth of the rate.  (The 8192-sample list's slots are free: big1 is not in use
        // when the streaming kernel is.)
        const bool st_retry = approx && scap > 8192;
        auto stream = [&](int cP, int in, int retry, int64_t n, bool exact) {
            FpStep &s = fast_step(kFamStream, 16384, cP, in);
            s.lds = fast_stream_lds_bytes(cP, nbt), s.retry = retry, s.clip = true, s.exact_scores = exact || !approx;
            s.extent = n, s.rule = kEqualSlices, s.slice_limit = kFastSliceLimit;
        };
        stream(capPs, kCntBig2, st_retry ? kCntBig1 : kNoList, g5, false);
        if (st_retry) stream(scap == 12288 ? 2520 : 3400, kCntBig1, kNoList, n_reads, true);
        if (g5 < n_reads) stride(capP2f, kCntBig2, g5, kNoList, main_retry, false);
    }
    // the reads whose approximate keys left a decision in doubt, on exact scores:
    // about 2 reads in 1000: a grid for 1/64 of the batch on the 6144-sample instantiation with exact scores
    // (a window beyond 6144 samples moves on to the slow path), the striding kernel beyond
    if (with_retry) {
        const int64_t g3 = fp_min(n_reads, fp_max(1024, n_reads / 64));
        list1(capP1, kCntRetry, kNoList, kNoList, g3, true, false);
        if (g3 < n_reads) stride(capP2, kCntRetry, g3, kNoList, kNoList, true);
    }
    if (!chain) return pl;
    // the exact kernels take the clip bounds of a read that has a CLIP_OK record (every read of the batch has a record by
    // now: the main clip kernel writes one per read, the list forms fill in the longer windows) instead of redoing the
    // two workgroup-wide medians
    const bool reuse = pl.clip_reuse = ext && !knobs.no_clip_reuse;
    // the exact general kernel for the slow list (and, refinement branch, the refinement kernels behind it)
    if (optimal) {
        // the exact kernel and its big form leave a record for every read they segment; nothing comes back
        exact_list(kCntSlow, reuse, true, 2048);
        if (pl.with_huge) big(kCntSlow, reuse, true);
        refine_optimal(reuse);
        return pl;
    }
    if (f.refine) {
        // refinement branch: the exact kernel segments the adapters of the slow list's reads and leaves them, like the
        // fast kernels theirs, to the refinement kernels (reads it cannot hand over it refines in place); barcode
        // tails beyond the tail kernel's capacity come back on a list of their own for the exact kernel's full form
        exact_list(kCntSlow, reuse, true, 2048);
        FpStep &s = pl.add(kFamRefineTail);
        s.over = kCntBack, s.clip = reuse, s.exact_scores = !approx;
        s.extent = n_reads, s.wg = 64, s.rule = kFullSlices, s.slice_limit = 1 << 22;
        // (a grid-stride kernel: one workgroup per CU serves this list, which is empty unless barcodes are very long --
        // 2048 workgroups of ~100 KB that only find it empty cost 70 us)
        exact_list(kCntBack, reuse, false, 256);
    } else {
        exact_list(kCntSlow, reuse, false, 2048);
    }
    if (pl.with_huge) big(kCntSlow, reuse, false);
    if (pl.with_long) long_form(kCntSlow);
    return pl;
}

}  // namespace wdx
