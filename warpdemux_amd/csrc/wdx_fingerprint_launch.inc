// Host driver of the fingerprint stage, included by wdx_fingerprint.hip's own translation unit behind its kernels:
//   FpWorkspace        where everything lives in the caller's workspace
//   fast_kernel_set    which kernels a (window width, suppression reach) combination runs on
//   plan_fast_chain    which launches this call makes, with what capacities, LDS sizes and grids -- decides, launches nothing
//   stage_*            one function per stage of the chain: they launch what the plan says and decide nothing
//   launch_fingerprint validate, plan, run the stages in order

// ---- workspace ------------------------------------------------------------------------------------------------------
// eight counters | one ClipRec per read | six read lists (slow, big0, big1, retry, big2, back: see plan_fast_chain)
// | the split main kernel's peak lists for one launch slice (kSplitRecBytes per read, 16-byte aligned)
// | 16 diagnostic counters (WDX_OPT_DEBUG_OCCUPANCY: why reads were handed to the exact kernel) at the very end -- in the
// caller's workspace, i.e. per context and per call, ordered by the call's stream
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
static_assert(kFpCounters == kWorkCounters && sizeof(ClipRec) == kWorkClipRecBytes && kSplitRecBytes == kWorkSplitRecBytes &&
                  kSplitSlice == kWorkSplitSlice && kCntBack + 1 == kWorkLists,
              "workspace layout: wdx_work_layout.h");
constexpr int kNoList = -1;
struct FpWorkspace {
    unsigned *count;        // kFpCounters
    ClipRec *clip;          // one per read
    int32_t *slow, *big0, *big1, *retry, *big2, *back;   // n_reads entries each, counted by count[kCntSlow .. kCntBack]
    unsigned char *split;   // kSplitRecBytes x min(n_reads, kSplitSlice)
    unsigned *dbg;          // 16
    int64_t bytes;
    FpWorkspace(void *d_ws, int64_t n_reads) {   // pointers on the pieces of fp_work_layout (wdx_work_layout.h)
        const FpWorkLayout W = fp_work_layout(n_reads);
        const uintptr_t b = reinterpret_cast<uintptr_t>(d_ws);
        count = reinterpret_cast<unsigned *>(b + (uintptr_t)W.count);
        clip = reinterpret_cast<ClipRec *>(b + (uintptr_t)W.clip);
        int32_t **const lists[kWorkLists] = {&slow, &big0, &big1, &retry, &big2, &back};
        for (int i = 0; i < kWorkLists; ++i) *lists[i] = reinterpret_cast<int32_t *>(b + (uintptr_t)W.list[i]);
        split = reinterpret_cast<unsigned char *>(b + (uintptr_t)W.split);
        dbg = reinterpret_cast<unsigned *>(b + (uintptr_t)W.dbg);
        bytes = W.bytes;
    }
    int32_t *list(int c) const {
        int32_t *const l[6] = {slow, big0, big1, retry, big2, back};
        return l[c];
    }
};
int64_t fingerprint_workspace_bytes(int64_t n_reads) { return fingerprint_workspace_size(n_reads); }

// ---- kernels --------------------------------------------------------------------------------------------------------
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
static int fast_combo(const wdx_seg_params &p) {
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
static bool fast_combo_exact_only(int combo) { return combo >= 9; }

using FastKernel = void (*)(FastArgs);

// The kernels of combinations 1 .. 8 for a main capacity of capF samples (what plan_fast_chain chose); a member stays null
// where the form does not exist.  NBT = 1 (reach <= 9): main kernels of 4096 (width 12 only), 5120 and 6144 samples, the
// diagnostic (PROF) builds for width 12 only, the split pair of the 5120-sample main kernel and of the 6144-sample list
// launch.  NBT = 2: the 6144-sample main kernel, with a split pair for the widths whose EXT main kernel runs the filtered
// 512-entry list (multiples of six from 12 up).
template <int FW, int NBT>
static void fill_fast_set(int capF, bool ext, bool prof, FastKernelSet &k) {
    k = FastKernelSet{};
    k.l1 = fingerprint_fast_list1_kernel<kNptLarge, FW, NBT>;   // 6144 samples, one workgroup per entry
    k.ls = fingerprint_fast_list_kernel<kNptHuge, FW, NBT>;     // 8192 samples, striding
    k.st = fingerprint_fast_stream_kernel<FW, NBT>;
    if constexpr (NBT == 2) {
        k.main = ext ? fingerprint_fast_kernel<kNptLarge, false, FW, 2, true> : fingerprint_fast_kernel<kNptLarge, false, FW, 2, false>;
        if constexpr (FW >= 12 && FW % 6 == 0) {
            k.tile = fingerprint_fast_kernel<kNptLarge, false, FW, 2, true, true>;
            k.tail = fingerprint_split_tail_kernel<FW, 2>;
        }
    } else {
        constexpr bool kProf = FW == kFW;
        if (capF == 5120) {   // (always EXT)
            k.main = fingerprint_fast_kernel<kNptMid, false, FW, 1, true>;
            k.tile = fingerprint_fast_kernel<kNptMid, false, FW, 1, true, true>;
            k.tail = fingerprint_split_tail_kernel<FW, 1>;
            k.l1s = fingerprint_fast_list1_kernel<kNptLarge, FW, 1, true>;
            if constexpr (kProf) {
                if (prof) {   // (the tile kernel's diagnostic build: wdx_fingerprint_profile_dev's fast_path = 2)
                    k.main = fingerprint_fast_kernel<kNptMid, true, FW, 1, true>;
                    k.tile = fingerprint_fast_kernel<kNptMid, true, FW, 1, true, true>;
                }
            }
            return;
        }
        if constexpr (kProf) {
            if (capF == 4096) {
                k.main = ext ? (prof ? fingerprint_fast_kernel<kNptSmall, true, FW, 1, true> : fingerprint_fast_kernel<kNptSmall, false, FW, 1, true>)
                             : (prof ? fingerprint_fast_kernel<kNptSmall, true, FW, 1, false> : fingerprint_fast_kernel<kNptSmall, false, FW, 1, false>);
                return;
            }
            if (prof) {
                k.main = ext ? fingerprint_fast_kernel<kNptLarge, true, FW, 1, true> : fingerprint_fast_kernel<kNptLarge, true, FW, 1, false>;
                return;
            }
        }
        k.main = ext ? fingerprint_fast_kernel<kNptLarge, false, FW, 1, true> : fingerprint_fast_kernel<kNptLarge, false, FW, 1, false>;
    }
}
// false: no fast kernels for this combination (k.main stays null)
static bool fast_kernel_set(int combo, int width, int capF, bool ext, bool prof, FastKernelSet &k) {
    k = FastKernelSet{};
    switch (combo) {
        case 1: fill_fast_set<kFW, 1>(capF, ext, prof, k); return true;
        case 2: fill_fast_set<18, 1>(capF, ext, prof, k); return true;
        case 3: fill_fast_set<30, 2>(capF, ext, prof, k); return true;
        case 4: fill_fast_set<6, 2>(capF, ext, prof, k); return true;
        case 5: fill_fast_set<24, 2>(capF, ext, prof, k); return true;
        case 6: fill_fast_set<36, 2>(capF, ext, prof, k); return true;
        case 7: fill_fast_set<12, 2>(capF, ext, prof, k); return true;
        case 8: fill_fast_set<18, 2>(capF, ext, prof, k); return true;
        default:   // the exact-scores-only widths: instantiated in wdx_fingerprint_w1.hip .. _w4.hip
            return exact_only_kernels_a(width, ext, k) || exact_only_kernels_b(width, ext, k) ||
                   exact_only_kernels_c(width, ext, k) || exact_only_kernels_d(width, ext, k);
    }
}

// One LdsAttr beside each kernel of a set, static per combination: hipFuncSetAttribute once per (kernel, device, size).
// A combination has one main kernel per (capacity, EXT, PROF) and one tile kernel per PROF; its other kernels are single.
struct FastAttrSet {
    LdsAttr *main, *l1, *ls, *st, *tile, *l1s;
};
static FastAttrSet fast_attr_set(int combo, int capF, bool ext, bool prof) {
    static struct {
        LdsAttr main[3][2][2], l1, ls, st, tile[2], l1s;
    } attrs[40];
    auto &a = attrs[combo - 1];
    return {&a.main[capF == 4096 ? 0 : (capF == 5120 ? 1 : 2)][ext][prof], &a.l1, &a.ls, &a.st, &a.tile[prof], &a.l1s};
}

// ---- plan -----------------------------------------------------------------------------------------------------------
struct PlanFlags {
    bool has_ws;      // the caller gave a workspace
    bool prof;        // diagnostic build (d_prof)
    int stop_phase;
    bool has_big;     // the caller gave the buffer of fingerprint_big_bytes
    bool has_long;    // ... and the one of fingerprint_long_bytes
    bool refine;      // consensus-refinement branch
    bool refine_ws;   // ... with the fast kernels' hand-over records (RefineDev::ws)
};
struct FastPlan {
    enum Path { kProfExact, kChain, kExact } path;
    // the exact general kernel (every path ends in it)
    int cap;          // samples of its LDS carve-up
    size_t lds;
    bool small;       // 512 threads (else 1024)
    bool with_huge;   // fingerprint_big_kernel behind it
    bool with_long;   // fingerprint_long_kernel behind that (WDX_OPT_LONG_WINDOWS)
    int exact_clip_cap;   // kExact: clip_bounds_kernel ahead of it for windows up to this many samples (0 = none)
    // the chain
    int combo, nbt;
    FastKernelSet k;
    FastAttrSet attr;   // k's LdsAttr, member by member
    bool approx;      // approximate score keys first (else exact scores from the first attempt)
    bool filt;        // threshold filter of the peak appends
    bool ext;         // clip-ahead: clip_bounds_kernel runs ahead of the main kernel (EXT instantiations)
    bool chain;       // the launches behind the main kernel run
    int capF, capP;   // main kernel: samples, peak-list entries
    size_t flds;
    int main_over;    // counter / list the main kernel hands its too-long windows and list overflows to (or kNoList)
    bool split;       // main launch as (tile kernel, tail kernel) pairs
    bool with_big0, with_big1, with_stream, with_retry;
    int64_t grid;     // the striding 8192-sample kernel's
    int capF1, capP1, capP1f, capF2, capP2, capP2f;   // 6144- / 8192-sample list kernels: unfiltered and filtered lists
    size_t flds1, flds2, flds1f, flds2f;
    int64_t g1;       // big0: one workgroup per entry up to here, the striding kernel beyond
    bool big0_pair;   // big0 launch as split pairs
    int big0_over, big0_rest_over;
    int scap, capPs, capPx, wave_clip_cap;   // streaming: clip capacity, peak lists (first attempt, exact retry); 0 = no wave clip
    size_t lds_cb, lds_st, lds_x;
    int64_t g5;
    bool st_retry;
    int64_t g3;       // retry: one workgroup per entry up to here
    bool clip_reuse;  // the exact kernel behind the chain takes the reads' clip records
    bool refine;
};

static FastPlan plan_fast_chain(const wdx_seg_params &p, int64_t max_len, int64_t n_reads, const Knobs &knobs, const PlanFlags &f) {
    FastPlan pl{};
    int64_t cap64 = max_len;
    if (cap64 > kExactLdsCap) cap64 = kExactLdsCap;
    if (cap64 < 64) cap64 = 64;
    const int cap = pl.cap = (int)((cap64 + 63) / 64 * 64);
    pl.lds = fp_lds_bytes(cap);
    pl.small = pl.lds <= 80 * 1024;
    // windows of kExactLdsCap+1 .. kBigCap samples: left alone by every launch below and taken by
    // fingerprint_big_kernel at the end (needs the caller's fingerprint_big_bytes(max_len) buffer; without it they
    // are reported WDX_READ_FAIL_UNKNOWN as windows beyond WDX_MAX_ADAPTER_SAMPLES always are)
    pl.with_huge = max_len > kExactLdsCap && f.has_big && !f.prof;
    // WDX_OPT_LONG_WINDOWS (the refinement branch: WDX_OPT_LONG_REFINE_WINDOWS): windows of kBigCap+1 .. kLongCap samples are
    // left alone in the same way and taken by fingerprint_long_kernel behind that (the caller's
    // fingerprint_long_bytes(max_len) buffer), which refines in place where the call refines
    pl.with_long = knobs.long_form(f.refine) && max_len > kBigCap && f.has_long && pl.with_huge;
    if (f.prof && !f.has_ws) {
        pl.path = FastPlan::kProfExact;
        return pl;
    }
    const int64_t chain_min = knobs.fast_chain_min > 0 ? knobs.fast_chain_min : 2048;
    const bool large_batch = n_reads >= chain_min;
    const int combo = pl.combo = fast_combo(p);
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
        pl.path = FastPlan::kExact;
        if (f.has_ws && !f.prof && !knobs.no_clip_reuse && large_batch)
            pl.exact_clip_cap = max_len <= 4096 ? 4096 : (max_len <= 5120 ? 5120 : (max_len <= 6144 ? 6144 : (max_len <= 8192 ? 8192 : kClipWaveLongCap)));
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
    pl.path = FastPlan::kChain;
    pl.refine = f.refine;
    const bool approx = pl.approx = large_batch && !knobs.fast_exact_scores && !fast_combo_exact_only(combo);
    const int nbt = pl.nbt = combo >= 3 ? 2 : 1;
    int capF = cap <= 4096 ? 4096 : (large_batch ? 5120 : 6144);
    if (knobs.fast_main_cap == 5120 || knobs.fast_main_cap == 6144) capF = knobs.fast_main_cap;  // experiments
    if (combo == 2) capF = large_batch ? 5120 : 6144;  // width 18: five workgroups per CU too (91 VGPRs)
    if (combo >= 3) capF = 6144;  // width 30 / reach 17 (and the round-5 widths): 115 VGPRs, four waves per SIMD either way
    pl.capF = capF;
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
    if (ext && filt && nbt == 2 && capF == 6144 && kWideWgPerCu == 5 && p.running_stat_width >= 12) capP = 512;
    if (knobs.fast_peak_cap > 0) capP = knobs.fast_peak_cap;  // experiment knob (wdx_ctx_set_option)
    pl.capP = capP;
    pl.flds = fast_lds_bytes(capF, capP, nbt);
    const bool chain = pl.chain = !(f.prof && f.stop_phase > 0);   // (ablation timing: the main kernel alone)
    pl.with_big0 = chain && capF == 5120;                          // windows of 5121..6144 samples, peak-list overflows
    // windows beyond 6144 samples, up to WDX_MAX_ADAPTER_SAMPLES: the streaming fast kernel (at 8 000 samples it is
    // faster than the striding 8192-sample list kernel, which then only serves list overflows and exact-score retries)
    // (odd widths are instantiated without the streaming form: their windows beyond 8192 samples take the exact kernel)
    const bool has_stream = !(fast_combo_exact_only(combo) && (p.running_stat_width & 1));
    pl.with_stream = chain && ext && capF >= 5120 && max_len > 6144 && has_stream;
    pl.with_big1 = chain && capF >= 5120 && cap > 6144 && !pl.with_stream;  // windows of 6145..8192 samples
    pl.with_retry = approx && chain;
    pl.main_over = pl.with_big0 ? kCntBig0 : (pl.with_stream ? kCntBig2 : (pl.with_big1 ? kCntBig1 : kNoList));
    fast_kernel_set(combo, p.running_stat_width, capF, ext, f.prof, pl.k);
    pl.attr = fast_attr_set(combo, capF, ext, f.prof);
    // The SPLIT form of the main kernel (large batches on approximate keys with the filtered 512-entry list -- the RNA004
    // triple, width 18, and the NBT = 2 widths from 12 up): the workgroup-per-read kernel ends after the tile pass and exports
    // the <= 256 peaks that can matter, one WAVE per read does the rest (fingerprint_split_tail_kernel) -- launch pairs over
    // slices of kSplitSlice reads, whose lists live in the workspace behind the read lists.  Not for the diagnostic builds
    // (the one-piece kernel serves those).
    // (not the refinement branch: measured 2.36 against 2.15 ms per 32 768 tRNA-like reads with the one-piece kernel)
    // (stop_phase == -2: the diagnostic build of the RNA004 pair, wdx_fingerprint_profile_dev's fast_path = 2)
    const bool prof_split = f.prof && f.stop_phase == -2 && combo == 1 && capF == 5120;
    pl.split = pl.k.tile && ext && approx && filt && capP == 512 && chain && (!f.prof || prof_split) && !f.refine && !knobs.no_split;
    // the list kernels
    pl.grid = n_reads < 1024 ? n_reads : 1024;  // striding kernels: every CU busy, nothing more
    pl.capF1 = 6144, pl.capP1 = 1376, pl.capF2 = 8192, pl.capP2 = 1856;
    pl.flds1 = fast_lds_bytes(pl.capF1, pl.capP1, nbt), pl.flds2 = fast_lds_bytes(pl.capF2, pl.capP2, nbt);
    // the same kernels behind filtered appends (the approximate-keys launches; the exact-scores retry keeps the long
    // lists): 512 entries -> five workgroups per CU at 6144 samples, four at 8192
    // (the striding 8192-sample kernel is NOT an EXT instantiation: its in-kernel medians put their 2112-word histogram
    // where the peak list will be, so its list region must hold 8448 bytes -- 768 entries, not 512)
    pl.capP1f = filt && nbt == 1 ? 512 : pl.capP1, pl.capP2f = filt && nbt == 1 ? 768 : pl.capP2;
    pl.flds1f = fast_lds_bytes(pl.capF1, pl.capP1f, nbt), pl.flds2f = fast_lds_bytes(pl.capF2, pl.capP2f, nbt);
    if (pl.with_big0) {
        // 11 % of RNA004 adapter windows are longer than 5120 samples: a grid for a quarter of the batch, one
        // workgroup per list entry, and the striding 8192-sample kernel for whatever lies beyond it
        pl.g1 = std::min<int64_t>(n_reads, std::max<int64_t>(1024, n_reads / 4));
        pl.big0_over = pl.with_stream ? kCntBig2 : (pl.with_big1 ? kCntBig1 : kNoList);
        pl.big0_rest_over = pl.with_stream ? kCntBig2 : kNoList;
        // the same pair over the list's entries (slot = workgroup of the slice; most of the grid lies past the list's end
        // and leaves at once, in both kernels)
        pl.big0_pair = pl.split && pl.k.l1s && pl.capP1f == 512;
    }
    if (pl.with_stream) {
        // windows of 6145 .. 16384 samples (RNA002: max_obs_trace + 2 * padding = 15 200): their clip bounds by one
        // workgroup per list entry (samples in LDS), then the streaming form of the fast body -- its LDS is the peak
        // list plus two tile buffers, whatever the window length: four workgroups per CU up to 12 288 samples, three
        // up to 16 384.  One workgroup per entry; the list's length is only known on the device.  With windows beyond
        // 8192 samples in the batch (RNA002-length reads: every read is on this list) the grids cover the batch; up to
        // 8192 the long windows are a tail of the batch (687 of 10 M synthetic RNA004 reads) and, for batches of more
        // than 2 M reads, the grids cover a sixteenth of it -- a workgroup past the list's end leaves at once, but 10 M of
        // them cost a millisecond per launch -- with the striding 8192-sample kernel behind them for whatever lies
        // beyond.  Doubts and refusals go to the exact kernel.
        const int scap = pl.scap = max_len <= 8192 ? 8192 : (max_len <= 12288 ? 12288 : 16384);
        pl.capPs = filt ? (scap == 8192 ? 1024 : (scap == 12288 ? 1280 : 1536))   // (the list from kPeakTauLo up)
                        : (scap == 8192 ? 1700 : (scap == 12288 ? 2520 : 3400));
        pl.lds_cb = clip_block_lds_bytes(scap), pl.lds_st = fast_stream_lds_bytes(pl.capPs, nbt);
        // (WDX_OPT_MAX_LAUNCH_SLICE, the tests' switch for the multi-launch paths, also selects the bounded grids)
        pl.g5 = (scap == 8192 && (n_reads > (1ll << 21) || knobs.max_launch_slice > 0)) ? std::max<int64_t>(1, n_reads / 16) : n_reads;
        // the one-wave clip kernel first (samples in registers, no barriers: twice the block kernel's rate per sample at
        // two workgroups of four reads per CU) for the windows its register file holds -- 8192 samples at 128 per lane,
        // 13 312 at 208; the workgroup kernel then finds a record for those and serves the rest: longer windows, and
        // the ones the wave form may not decide (negative samples it cannot clamp away)
        pl.wave_clip_cap = knobs.no_wave_clip_long ? 0 : (scap == 8192 ? 8192 : kClipWaveLongCap);
        // batches of long windows (beyond 8192 samples: the grids cover the batch anyway): a read with a decision inside
        // the error band, or whose cut does not clear the append filter's threshold, is redone by a second launch of the
        // same kernel on exact scores with the unfiltered list capacity -- instead of the exact general kernel, which
        // serves such a window at a twentieth of the rate.  (The 8192-sample list's slots are free: big1 is not in use
        // when the streaming kernel is.)
        pl.st_retry = approx && scap > 8192;
        if (pl.st_retry) {
            pl.capPx = scap == 12288 ? 2520 : 3400;
            pl.lds_x = fast_stream_lds_bytes(pl.capPx, nbt);
        }
    }
    // about 2 reads in 1000: a grid for 1/64 of the batch on the 6144-sample instantiation with exact scores
    // (a window beyond 6144 samples moves on to the slow path), the striding kernel beyond
    if (pl.with_retry) pl.g3 = std::min<int64_t>(n_reads, std::max<int64_t>(1024, n_reads / 64));
    // the exact kernels take the clip bounds of a read that has a CLIP_OK record (every read of the batch has a record by
    // now: the main clip kernel writes one per read, the list forms fill in the longer windows) instead of redoing the
    // two workgroup-wide medians
    pl.clip_reuse = ext && !knobs.no_clip_reuse;
    return pl;
}

// ---- launch helpers -------------------------------------------------------------------------------------------------
// What every stage of one call sees.
struct FpRun {
    FpArgs A;
    const FastPlan &pl;
    FpWorkspace ws;
    hipStream_t stream;
    int64_t *n_launches;   // nullable
    MainEvents *ev;        // nullable
    void *d_long;          // fingerprint_long_kernel's slots (pl.with_long)
    void *d_opt;           // WDX_OPT_REFINE_OPTIMAL_CPTS: the scratch of plan_refine_optimal(n_reads, max_len, E2)
    int64_t max_len;
    // a fast kernel's arguments: the exact kernel's list, everything else null or zero
    FastArgs fast_args(int capF, int capP) const {
        FastArgs F{};
        F.a = A;
        F.capF = capF;
        F.capP = capP;
        F.slow_count = ws.count + kCntSlow;
        F.slow_list = ws.slow;
        return F;
    }
};
static void takes_from(FastArgs &F, const FpWorkspace &ws, int c, int64_t start = 0) {
    F.in_count = ws.count + c;
    F.in_list = ws.list(c);
    F.in_start = (unsigned)start;
}
static void hands_over_to(FastArgs &F, const FpWorkspace &ws, int c) {
    if (c == kNoList) return;
    F.big_count = ws.count + c;
    F.big_list = ws.list(c);
}
static void retries_on(FastArgs &F, const FpWorkspace &ws, int c) {
    F.retry_count = ws.count + c;
    F.retry_list = ws.list(c);
}

// one workgroup per read (or list entry); grid.x * block.x must stay below 2^32: EQUAL launch slices of at most
// 2^31 / FB workgroups
static void launch_sliced(FastKernel k, FastArgs fa, int64_t n_wg, size_t lds_bytes, hipStream_t stream, int64_t *n_launches) {
    const int64_t max_slice = launch_slice_limit((1ll << 31) / FB), n_slices = (n_wg + max_slice - 1) / max_slice;
    const int64_t slice = (n_wg + n_slices - 1) / n_slices;
    for (int64_t base = 0; base < n_wg; base += slice) {
        const int64_t n = n_wg - base < slice ? n_wg - base : slice;
        fa.a.block_base = base;
        hipLaunchKernelGGL(k, dim3((unsigned)n), dim3(FB), lds_bytes, stream, fa);
        if (n_launches) ++*n_launches;
    }
}
// (tile kernel, tail kernel) launch pairs over slices of kSplitSlice reads or list entries (slot = workgroup of the slice).
// ev: an event pair around each tail launch, from the context's pool.
static void launch_split_pairs(FastKernel tile, FastKernel tail, FastArgs F, int64_t n, size_t lds, hipStream_t stream,
                               int64_t *n_launches, MainEvents *ev) {
    (void)for_each_slice(n, kSplitSlice, [&](int64_t base, int64_t m) {
        F.split_base = base;
        F.split_n = m;
        F.a.block_base = base;
        hipLaunchKernelGGL(tile, dim3((unsigned)m), dim3(FB), lds, stream, F);
        if (n_launches) ++*n_launches;
        std::pair<hipEvent_t, hipEvent_t> tp{nullptr, nullptr};
        if (ev && ev->first && ev->take) tp = ev->take(ev->take_arg);
        if (tp.first) (void)hipEventRecord(tp.first, stream);
        F.a.block_base = 0;
        hipLaunchKernelGGL(tail, dim3((unsigned)((m + kSplitWaves - 1) / kSplitWaves)), dim3(kSplitWaves * 64), 0, stream, F);
        if (tp.first) {
            (void)hipEventRecord(tp.second, stream);
            ev->tail.push_back(tp);
        }
        return (int)WDX_SUCCESS;
    });
}
static int launch_exact_list(const FpRun &R, const FpArgs &A, int c, int max_grid = 2048) {
    return R.pl.small ? launch_fp_list<512>(A, R.pl.lds, R.ws.count + c, R.ws.list(c), R.stream, max_grid)
                      : launch_fp_list<1024>(A, R.pl.lds, R.ws.count + c, R.ws.list(c), R.stream, max_grid);
}

// ---- stages of the chain, in launch order ---------------------------------------------------------------------------
// A1 for the main kernel's reads (windows of 256 .. capF samples; longer ones are flagged CLIP_NONE and the main kernel
// hands them to the lists before it would look at their record)
static int stage_clip_ahead(const FpRun &R, FastArgs &F) {
    MainEvents *ev = R.ev;
    if (ev && ev->c_first) (void)hipEventRecord(ev->c_first, R.stream);
    if (int rc = launch_clip_bounds(R.A, R.ws.clip, R.pl.capF, R.stream)) return rc;
    if (F.big_list) {   // the windows beyond capF go on the main kernel's hand-over list here (one atomic per 64 reads)
        if (int rc = launch_route_long_windows(R.A, R.pl.capF, F.big_count, F.big_list, R.stream)) return rc;
        F.routed = 1;
    }
    if (ev && ev->c_first) {
        (void)hipEventRecord(ev->c_second, R.stream);
        ev->c_recorded = true;
    }
    return WDX_SUCCESS;
}
static int stage_main(const FpRun &R, FastArgs &F) {
    const FastPlan &pl = R.pl;
    MainEvents *ev = R.ev;
    if (ev && ev->first) (void)hipEventRecord(ev->first, R.stream);
    if (pl.split) {
        if (int rc = pl.attr.tile->ensure(pl.k.tile, pl.flds)) return rc;
        F.split_ws = R.ws.split;
        launch_split_pairs(pl.k.tile, pl.k.tail, F, R.A.n_reads, pl.flds, R.stream, R.n_launches, ev);
    } else {
        launch_sliced(pl.k.main, F, R.A.n_reads, pl.flds, R.stream, R.n_launches);
    }
    if (ev && ev->first) {
        (void)hipEventRecord(ev->second, R.stream);
        ev->recorded = true;
    }
    return WDX_SUCCESS;
}
// windows of capF + 1 .. 6144 samples and the main kernel's peak-list overflows
static int stage_big0(const FpRun &R, const FastArgs &Fmain) {
    const FastPlan &pl = R.pl;
    FastArgs F1 = R.fast_args(pl.capF1, pl.capP1f);
    hands_over_to(F1, R.ws, pl.big0_over);
    takes_from(F1, R.ws, kCntBig0);
    F1.retry_count = Fmain.retry_count;
    F1.retry_list = Fmain.retry_list;
    F1.clip = R.ws.clip;
    if (int rc = launch_clip_bounds_list(R.A, R.ws.clip, F1.in_count, F1.in_list, pl.g1, R.stream)) return rc;
    if (pl.big0_pair) {
        if (int rc = pl.attr.l1s->ensure(pl.k.l1s, pl.flds1f)) return rc;
        F1.split_ws = Fmain.split_ws;
        launch_split_pairs(pl.k.l1s, pl.k.tail, F1, pl.g1, pl.flds1f, R.stream, nullptr, nullptr);
    } else {
        launch_sliced(pl.k.l1, F1, pl.g1, pl.flds1f, R.stream, nullptr);
    }
    if (pl.g1 < R.A.n_reads) {
        FastArgs F1b = R.fast_args(pl.capF2, pl.capP2f);
        hands_over_to(F1b, R.ws, pl.big0_rest_over);
        takes_from(F1b, R.ws, kCntBig0, pl.g1);
        F1b.retry_count = Fmain.retry_count;
        F1b.retry_list = Fmain.retry_list;
        hipLaunchKernelGGL(pl.k.ls, dim3((unsigned)pl.grid), dim3(FB), pl.flds2f, R.stream, F1b);
    }
    return WDX_SUCCESS;
}
// windows of 6145 .. 8192 samples when the streaming kernel is not in the chain
static void stage_big1(const FpRun &R, const FastArgs &Fmain) {
    FastArgs F2 = R.fast_args(R.pl.capF2, R.pl.capP2f);
    takes_from(F2, R.ws, kCntBig1);
    F2.retry_count = Fmain.retry_count;
    F2.retry_list = Fmain.retry_list;
    hipLaunchKernelGGL(R.pl.k.ls, dim3((unsigned)R.pl.grid), dim3(FB), R.pl.flds2f, R.stream, F2);
}
// windows beyond 6144 samples: clip bounds of the list's entries, the streaming kernel, its exact-scores retry, and the
// striding kernel for the entries beyond the grids
static int stage_stream(const FpRun &R, const FastArgs &Fmain) {
    const FastPlan &pl = R.pl;
    static LdsAttr attr_cb;
    if (int rc = attr_cb.ensure(clip_bounds_block_kernel, pl.lds_cb)) return rc;
    if (int rc = pl.attr.st->ensure(pl.k.st, pl.lds_st)) return rc;
    if (pl.wave_clip_cap)
        if (int rc = launch_clip_bounds_list(R.A, R.ws.clip, R.ws.count + kCntBig2, R.ws.big2, pl.g5, R.stream, pl.wave_clip_cap, true))
            return rc;
    (void)for_each_slice(pl.g5, 1ll << 22, [&](int64_t base, int64_t m) {
        ClipBlockArgs CB{R.A, R.ws.clip, R.ws.count + kCntBig2, R.ws.big2, pl.scap};
        CB.a.block_base = base;
        hipLaunchKernelGGL(clip_bounds_block_kernel, dim3((unsigned)m), dim3(FB), pl.lds_cb, R.stream, CB);
        return (int)WDX_SUCCESS;
    });
    FastArgs F5 = R.fast_args(16384, pl.capPs);
    takes_from(F5, R.ws, kCntBig2);
    F5.clip = R.ws.clip;
    if (pl.st_retry) retries_on(F5, R.ws, kCntBig1);
    launch_sliced(pl.k.st, F5, pl.g5, pl.lds_st, R.stream, nullptr);
    if (pl.st_retry) {
        if (int rc = pl.attr.st->ensure(pl.k.st, pl.lds_x)) return rc;
        FastArgs F6 = R.fast_args(16384, pl.capPx);
        takes_from(F6, R.ws, kCntBig1);
        F6.clip = R.ws.clip;
        F6.a.exact_scores = 1;
        launch_sliced(pl.k.st, F6, R.A.n_reads, pl.lds_x, R.stream, nullptr);
    }
    if (pl.g5 < R.A.n_reads) {
        FastArgs F5b = R.fast_args(pl.capF2, pl.capP2f);
        takes_from(F5b, R.ws, kCntBig2, pl.g5);
        F5b.retry_count = Fmain.retry_count;
        F5b.retry_list = Fmain.retry_list;
        hipLaunchKernelGGL(pl.k.ls, dim3((unsigned)pl.grid), dim3(FB), pl.flds2f, R.stream, F5b);
    }
    return WDX_SUCCESS;
}
// the reads whose approximate keys left a decision in doubt, on exact scores
static void stage_retry(const FpRun &R) {
    const FastPlan &pl = R.pl;
    FastArgs F3 = R.fast_args(pl.capF1, pl.capP1);
    takes_from(F3, R.ws, kCntRetry);
    F3.clip = R.ws.clip;
    F3.a.exact_scores = 1;
    launch_sliced(pl.k.l1, F3, pl.g3, pl.flds1, R.stream, nullptr);
    if (pl.g3 < R.A.n_reads) {
        FastArgs F3b = R.fast_args(pl.capF2, pl.capP2);
        takes_from(F3b, R.ws, kCntRetry, pl.g3);
        F3b.a.exact_scores = 1;
        hipLaunchKernelGGL(pl.k.ls, dim3((unsigned)pl.grid), dim3(FB), pl.flds2, R.stream, F3b);
    }
}
// WDX_OPT_REFINE_OPTIMAL_CPTS: every read of the call has left a record by now (the fast kernels, the exact kernel and its big
// form alike); the subsequence match for all of them, then the optimal change-points of their barcode tails -- one launch
// whose workgroups stride over the reads, each with its slot of the context's scratch buffer (WDX_K_REFINE_OPTIMAL)
static int stage_refine_optimal(FpArgs A, int64_t max_len, void *d_opt, hipStream_t stream, MainEvents *ev) {
    A.refine_record = 0;
    if (int rc = for_each_slice(A.n_reads, 1 << 22, [&](int64_t base, int64_t n) {
            A.block_base = base;
            return launch_refine_match_wave(A, n, stream);
        }))
        return rc;
    std::pair<hipEvent_t, hipEvent_t> tp{nullptr, nullptr};
    if (ev && ev->take) tp = ev->take(ev->take_arg);   // (take is set whenever the context times its kernels)
    if (tp.first) (void)hipEventRecord(tp.first, stream);
    const int rc = launch_refine_optimal(A, plan_refine_optimal(A.n_reads, max_len, A.rf.E2), d_opt, stream);
    if (tp.first) {
        (void)hipEventRecord(tp.second, stream);
        ev->optimal.push_back(tp);
    }
    return rc;
}
// the exact general kernel for the slow list (and, refinement branch, the refinement kernels behind it)
static int stage_exact(FpRun &R) {
    FpArgs &A = R.A;
    if (R.pl.clip_reuse) A.clip = R.ws.clip;
    if (R.pl.refine && A.refine_optimal) {
        // the exact kernel and its big form leave a record for every read they segment; nothing comes back
        A.refine_record = 1;
        if (int rc = launch_exact_list(R, A, kCntSlow)) return rc;
        if (R.pl.with_huge)
            if (int rc = launch_fp_big(A, R.pl.cap, R.ws.count + kCntSlow, R.ws.slow, R.stream)) return rc;
        return stage_refine_optimal(A, R.max_len, R.d_opt, R.stream, R.ev);
    }
    if (R.pl.refine) {
        // refinement branch: the exact kernel segments the adapters of the slow list's reads and leaves them, like the
        // fast kernels theirs, to the refinement kernels (reads it cannot hand over it refines in place); barcode
        // tails beyond the tail kernel's capacity come back on a list of their own for the exact kernel's full form
        A.refine_record = 1;
        if (int rc = launch_exact_list(R, A, kCntSlow)) return rc;
        A.refine_record = 0;
        if (int rc = launch_refine_tail(A, R.ws.count + kCntBack, R.ws.back, R.stream)) return rc;
        // (a grid-stride kernel: one workgroup per CU serves this list, which is empty unless barcodes are very long --
        // 2048 workgroups of ~100 KB that only find it empty cost 70 us)
        if (int rc = launch_exact_list(R, A, kCntBack, 256)) return rc;
    } else if (int rc = launch_exact_list(R, A, kCntSlow)) {
        return rc;
    }
    if (R.pl.with_huge)
        if (int rc = launch_fp_big(A, R.pl.cap, R.ws.count + kCntSlow, R.ws.slow, R.stream)) return rc;
    if (R.pl.with_long)
        if (int rc = launch_fp_long(A, R.d_long, R.ws.count + kCntSlow, R.ws.slow, R.stream)) return rc;
    return WDX_SUCCESS;
}
// WDX_OPT_DEBUG_OCCUPANCY: where the reads went (synchronises)
static int print_chain_counters(const FpRun &R) {
    const FpWorkspace &ws = R.ws;
    hipStream_t stream = R.stream;
    unsigned c[kFpCounters] = {};
    WDX_HIP_TRY(hipMemcpyAsync(c, ws.count, sizeof(c), hipMemcpyDeviceToHost, stream));
    WDX_HIP_TRY(hipStreamSynchronize(stream));
    // (kCntBig1 is the 8192-sample list when the streaming kernel is not in the chain, else the streaming kernel's
    // own exact-scores retry list)
    fprintf(stderr, "[wdx] of %lld reads: %u beyond the main instantiation, %u %s, %u to the "
                    "streaming kernel, %u redone with exact scores, %u on the exact general kernel\n", (long long)R.A.n_reads,
            c[kCntBig0], c[kCntBig1], R.pl.with_stream ? "redone by the streaming kernel on exact scores" : "to the 8192-sample list kernel",
            c[kCntBig2], c[kCntRetry], c[kCntSlow]);
    unsigned h[16];
    WDX_HIP_TRY(hipMemcpyAsync(h, ws.dbg, 64, hipMemcpyDeviceToHost, stream));
    WDX_HIP_TRY(hipStreamSynchronize(stream));
    fprintf(stderr, "[wdx] handed to the exact kernel by the fast kernels, by reason (0 parameter gate / window, 1 NaN or negative, "
                    "2 sums not provably exact, 3 plateau or peak-list capacity, 4 neighbourhood, 5 kept-list capacity, 6 tie at the "
                    "top-E cut, 7 doubt without a retry list, 8 fewer peaks than events with accept_less_cpts):");
    for (int i = 0; i < 10; ++i) fprintf(stderr, " %u", h[i]);
    fprintf(stderr, "\n");
    if (R.pl.refine)
        fprintf(stderr, "[wdx] refinement: %u reads back from the tail kernel to the exact kernel (%u for a run of equal scores across a "
                        "tile's end, %u beyond the peak list)\n", c[kCntBack], c[kCntBackTie], c[kCntBackList]);
    if (R.pl.ext) {
        std::vector<ClipRec> rec((size_t)R.A.n_reads);
        WDX_HIP_TRY(hipMemcpy(rec.data(), ws.clip, sizeof(ClipRec) * rec.size(), hipMemcpyDeviceToHost));
        long long f[4] = {0, 0, 0, 0};
        for (const ClipRec &cr : rec) ++f[cr.flag & 3];
        fprintf(stderr, "[wdx] clip_bounds_kernel flags: %lld not taken, %lld ok, %lld NaN / negative, %lld sums not "
                        "provably exact\n", f[0], f[1], f[2], f[3]);
    }
    return WDX_SUCCESS;
}

static int run_fast_chain(FpRun &R, const Knobs &knobs) {
    const FastPlan &pl = R.pl;
    FpArgs &A = R.A;
    WDX_HIP_TRY(hipMemsetAsync(R.ws.count, 0, kFpCounters * 4, R.stream));
    A.exact_scores = pl.approx ? 0 : 1;
    A.peak_filter = knobs.no_peak_filter ? 0 : 1;   // (only the approximate-keys launches look at it)
    if (knobs.debug_occ) {   // (diagnostic: 16 counters at the end of this call's workspace, zeroed on its stream)
        WDX_HIP_TRY(hipMemsetAsync(R.ws.dbg, 0, 64, R.stream));
        A.dbg_reasons = R.ws.dbg;
    }
    FastArgs F = R.fast_args(pl.capF, pl.capP);
    if (pl.approx) retries_on(F, R.ws, kCntRetry);
    hands_over_to(F, R.ws, pl.main_over);
    F.clip = pl.ext ? R.ws.clip : nullptr;
    if (int rc = pl.attr.main->ensure(pl.k.main, pl.flds)) return rc;
    if (knobs.debug_occ) {
        int nb = 0;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)pl.k.main, FB, pl.flds);
        fprintf(stderr, "[wdx] fast kernel capF=%d capP=%d lds=%zu B -> %d workgroups/CU%s\n", pl.capF, pl.capP, pl.flds, nb,
                pl.approx ? ", approximate score keys" : "");
    }
    if (pl.ext)
        if (int rc = stage_clip_ahead(R, F)) return rc;
    if (int rc = stage_main(R, F)) return rc;
    if (pl.with_big0 || pl.with_retry)
        if (int rc = pl.attr.l1->ensure(pl.k.l1, pl.flds1)) return rc;
    if (pl.with_big0 || pl.with_big1 || pl.with_stream || pl.with_retry)
        if (int rc = pl.attr.ls->ensure(pl.k.ls, pl.flds2)) return rc;
    if (pl.with_big0)
        if (int rc = stage_big0(R, F)) return rc;
    if (pl.with_big1) stage_big1(R, F);
    if (pl.with_stream)
        if (int rc = stage_stream(R, F)) return rc;
    if (pl.with_retry) stage_retry(R);
    WDX_HIP_TRY(hipGetLastError());
    if (!pl.chain) return WDX_SUCCESS;  // (ablation timing of the main kernel: the lists are left unprocessed)
    if (int rc = stage_exact(R)) return rc;
    return knobs.debug_occ ? print_chain_counters(R) : WDX_SUCCESS;
}

// ---- entry ----------------------------------------------------------------------------------------------------------
static int validate_fingerprint_call(int64_t n_reads, int64_t max_len, const wdx_seg_params &p, const RefineDev *rf,
                                     const Knobs &knobs) {
    if (n_reads > 0x7fffffffLL) {
        set_error("at most 2^31-1 reads per call");
        return WDX_ERR_INVALID;
    }
    if (p.num_events < 1 || p.num_events > kMaxEvents) {
        set_error("num_events must be in [1, %d]", kMaxEvents);
        return p.num_events < 1 ? WDX_ERR_INVALID : WDX_ERR_UNSUPPORTED;
    }
    if (p.barcode_num_events < 1 || p.barcode_num_events > kSegCap) {
        set_error("barcode_num_events must be in [1, %d]", kSegCap);
        return WDX_ERR_INVALID;
    }
    if (p.running_stat_width < 0 || p.running_stat_width > kMaxW) {
        set_error("running_stat_width must be in [0, %d]", kMaxW);
        return WDX_ERR_UNSUPPORTED;
    }
    if (p.padding < 0) {
        set_error("padding must be >= 0");
        return WDX_ERR_INVALID;
    }
    if (rf) {
        if (!rf->query || rf->nq < 1 || rf->nq > kRefineMaxQuery || p.num_events + 1 > kRefineMaxSeries) {
            set_error("consensus refinement: the query must have 1..%d points and num_events + 1 <= %d", kRefineMaxQuery,
                      kRefineMaxSeries);
            return WDX_ERR_UNSUPPORTED;
        }
        if (rf->E2 < 1 || rf->E2 > kMaxEvents || rf->psi1b < 0 || rf->psi2b < 0) {
            set_error("consensus refinement: barcode_num_events[0] must be in [1, %d], psi >= 0", kMaxEvents);
            return WDX_ERR_INVALID;
        }
        if (knobs.refine_optimal) {
            if (knobs.long_refine_windows) {
                set_error("WDX_OPT_REFINE_OPTIMAL_CPTS and WDX_OPT_LONG_REFINE_WINDOWS do not go together");
                return WDX_ERR_UNSUPPORTED;
            }
            if (p.min_obs_per_base < 1) {
                set_error("optimal change-points: min_obs_per_base must be >= 1");
                return WDX_ERR_UNSUPPORTED;
            }
            if (p.sig_norm != WDX_NORM_NONE || !rf->ws) {   // (what the record path does not serve: wdx.h)
                set_error("optimal change-points: sig_extract.normalization must be \"none\"");
                return WDX_ERR_UNSUPPORTED;
            }
        }
    }
    return WDX_SUCCESS;
}

int launch_fingerprint(const FpReads &in, const wdx_seg_params &p, const FpOut &out, hipStream_t stream, void *d_ws,
                       const Knobs &knobs, int64_t *n_launches, long long *d_prof, int64_t prof_reads, int stop_phase,
                       const RefineDev *rf, MainEvents *main_ev, double *d_big, void *d_long, void *d_opt) {
    if (in.n_reads == 0) return WDX_SUCCESS;
    if (int rc = validate_fingerprint_call(in.n_reads, in.max_len, p, rf, knobs)) return rc;
    LaunchSliceScope slice_scope(knobs.max_launch_slice);
    const PlanFlags flags{d_ws != nullptr, d_prof != nullptr, stop_phase, d_big != nullptr, d_long != nullptr, rf != nullptr, rf && rf->ws};
    const FastPlan pl = plan_fast_chain(p, in.max_len, in.n_reads, knobs, flags);
    if (pl.lds > 160 * 1024) {
        set_error("fingerprint LDS carve-up (%zu B) exceeds 160 KiB", pl.lds);
        return WDX_ERR_INVALID;
    }
    if (pl.path == FastPlan::kChain && !pl.k.main) {
        set_error("no fast kernels for running_stat_width %d", (int)p.running_stat_width);
        return WDX_ERR_INVALID;
    }
    (void)hipGetLastError();  // do not inherit a stale error from an earlier failed call
    FpRun R{FpArgs{in.sig, in.row_off, in.row_len, in.stride, in.n_reads, in.a_start, in.a_end, in.ok, p, out.fpt, out.dwell, out.stats,
                   out.status, pl.cap, 0, d_prof, prof_reads, stop_phase, 1, rf ? *rf : RefineDev{}, d_big,
                   pl.with_long ? kLongCap : (pl.with_huge ? kBigCap : 0), knobs.exact_no_list ? 1 : 0},
            pl, FpWorkspace(d_ws, in.n_reads), stream, n_launches, main_ev, d_long, d_opt, in.max_len};
    const bool optimal = rf && knobs.refine_optimal;
    R.A.refine_optimal = optimal ? 1 : 0;
    const uint64_t e1 = (uint64_t)(p.num_events > 0 ? p.num_events : 1);
    R.A.e_magic1 = (unsigned)std::min<uint64_t>(((1ull << 32) + e1 - 1) / e1, 0xffffffffull);   // (E = 1: 2^32 - 1 -> q = n - 1, rounded up to n)
    R.A.e_magic2 = (unsigned)(((1ull << 32) + 2 * e1 - 1) / (2 * e1));
    switch (pl.path) {
        case FastPlan::kProfExact:
            return pl.small ? launch_fp_chunks<512, true>(R.A, pl.lds, stream, n_launches)
                            : launch_fp_chunks<1024, true>(R.A, pl.lds, stream, n_launches);
        case FastPlan::kChain:
            return run_fast_chain(R, knobs);
        case FastPlan::kExact:
            break;
    }
    if (pl.exact_clip_cap) {
        if (int rc = launch_clip_bounds(R.A, R.ws.clip, pl.exact_clip_cap, stream)) return rc;
        R.A.clip = R.ws.clip;
    }
    if (optimal) R.A.refine_record = 1;   // every read leaves a record: stage_refine_optimal does the rest
    if (int rc = pl.small ? launch_fp_chunks<512, false>(R.A, pl.lds, stream, n_launches)
                          : launch_fp_chunks<1024, false>(R.A, pl.lds, stream, n_launches))
        return rc;
    if (pl.with_huge)
        if (int rc = launch_fp_big(R.A, pl.cap, nullptr, nullptr, stream)) return rc;
    if (optimal) return stage_refine_optimal(R.A, in.max_len, d_opt, stream, main_ev);
    if (pl.with_long) return launch_fp_long(R.A, d_long, nullptr, nullptr, stream);
    return WDX_SUCCESS;
}
