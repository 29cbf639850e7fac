// Stand-alone driver of warpdemux_amd/csrc/wdx_dtw_plan.h -- which kernel a DTW dispatch takes, in which layout, over which
// grid, and what is prepared for it -- built by tests/test_dtw_plan_host.py with the system compiler and the address /
// undefined-behaviour sanitizers.
//   dtw_plan_check            reads cases from stdin, one per line: "nX nY L window want_argmin entry no_wavefront no_short_dtw
//                             wide_dtw" (entry 0: matrix entries, 1: fused device entries), and prints the case followed by its plan
//   dtw_plan_check sweep      walks every shape of sweep() below, checks what must hold of every plan (exit status = the
//                             invariant that failed) and prints "family <id> <cases>" per kernel family and "cases <n>"
#include "wdx_dtw_plan.h"

#include <stdio.h>
#include <string.h>

using namespace wdx;

struct Case {
    int64_t nX, nY, L, window;
    int argmin, entry, no_wavefront, no_short_dtw, wide_dtw;
    DtwPlan plan() const {
        return dtw_plan(nX, nY, L, window, argmin != 0, entry ? DtwEntry::kFused : DtwEntry::kMatrix,
                        DtwSwitches{no_wavefront != 0, no_short_dtw != 0, wide_dtw != 0});
    }
};

static void print_plan(const Case &c, const DtwPlan &P) {
    const wdx_dtw_launch_info &I = P.info;
    printf("%lld %lld %lld %lld %d %d %d %d %d", (long long)c.nX, (long long)c.nY, (long long)c.L, (long long)c.window, c.argmin,
           c.entry, c.no_wavefront, c.no_short_dtw, c.wide_dtw);
    printf(" %d %d %d %d %d %d %d %d %lld %lld", I.family, I.band_w, I.exact_w, I.layout, I.fused_argmin, I.launches,
           I.refs_per_block, I.window, (long long)I.grid_x, (long long)I.grid_y);
    printf(" %d %d %lld %lld %lld %d %lld %lld %lld %lld\n", (int)P.unsupported, (int)P.prep, (long long)P.ld, (long long)P.copy_bytes,
           (long long)P.flag_bytes, (int)P.argmin_after, (long long)P.lds_bytes, (long long)P.scratch_bytes, (long long)P.lanes,
           (long long)P.rows);
}

// reads / references around 1, a wave (64), the row-major threshold (8 192), the wavefront's 16 384 pairs, the scratch rows'
// 65 536 lanes per launch and the fused argmin's 2 048 and 24 576 waves; every L in 1 .. 40 plus 110, 256, 257; every window
// 0 .. L + 1; the two entries, with and without an argmin, no switch and each switch alone
template <class F>
static void sweep(F f) {
    static const int64_t NX[] = {1, 2, 3, 10, 62, 63, 64, 65, 66, 1024, 1025, 5462, 8191, 8192, 8193, 16384, 16385, 65536, 65537,
                                 131008, 131009, 131072, 131073, 1572800, 1572801, 1572864};
    static const int64_t NY[] = {1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 851, 1368, 8192, 65537, 131073};
    static const int SW[][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int64_t L = 1; L <= 257; L = L < 40 ? L + 1 : (L == 40 ? 110 : (L == 110 ? 256 : L + 1)))
        for (int64_t window = 0; window <= L + 1; ++window)
            for (int64_t nX : NX)
                for (int64_t nY : NY)
                    for (const auto &s : SW)
                        for (int entry = 0; entry < 2; ++entry)
                            for (int argmin = 0; argmin < 2; ++argmin) f(Case{nX, nY, L, window, argmin, entry, s[0], s[1], s[2]});
}

// what must hold of every plan; 0 or the number of the invariant that does not
static int check(const Case &c, const DtwPlan &P) {
    const wdx_dtw_launch_info &I = P.info;
    const int64_t w = dtw_effective_window(c.L, c.window);
    if (P.unsupported) return (c.entry == 1 && I.family == WDX_DTW_NONE && w > kMaxRegWindow) ? 0 : 1;
    // exactly one family, and only the families of the entry
    if (I.family < WDX_DTW_WAVEFRONT || I.family > WDX_DTW_WIDE || I.family == WDX_DTW_SHORT_SVM) return 2;
    if (c.entry == 1 && (I.family == WDX_DTW_WAVEFRONT || I.family == WDX_DTW_SCRATCH || I.layout == WDX_DTW_LAYOUT_REFS_AS_LANES)) return 3;
    if (I.window != w) return 4;
    const bool refs_as_lanes = I.layout == WDX_DTW_LAYOUT_REFS_AS_LANES;
    if (P.lanes != (refs_as_lanes ? c.nY : c.nX) || P.rows != (refs_as_lanes ? c.nX : c.nY)) return 5;
    if ((P.prep == DtwPrep::kPaddedReads) != refs_as_lanes) return 6;
    if ((P.prep == DtwPrep::kNone) != (I.layout == WDX_DTW_LAYOUT_ROW_MAJOR)) return 7;
    if (P.prep == DtwPrep::kReadMinor && (P.ld < c.nX || P.ld % 64 || P.ld >= c.nX + 64 || P.copy_bytes != c.L * P.ld * 8 || P.flag_bytes != P.ld)) return 8;
    if (refs_as_lanes && (P.ld != c.L + 2 * kDtwHalo || P.copy_bytes != c.nX * P.ld * 8 || P.flag_bytes < c.nX)) return 9;
    if (P.prep == DtwPrep::kNone && (P.copy_bytes || P.flag_bytes)) return 10;
    if ((P.scratch_bytes != 0) != (I.family == WDX_DTW_SCRATCH)) return 11;
    if (P.argmin_after != (c.argmin && !I.fused_argmin) || (I.fused_argmin && !c.argmin)) return 12;
    if (I.family == WDX_DTW_WAVEFRONT) {
        if (c.nX * c.nY > kWfMaxPairs || w > 16 || c.L > 256 || c.no_wavefront) return 13;
        if (I.grid_x * kWfPairsPerBlock < c.nX * c.nY || (I.grid_x - 1) * kWfPairsPerBlock >= c.nX * c.nY || I.grid_y != 1) return 14;
        if (P.lds_bytes != kWfPairsPerBlock * 2 * c.L * 8 || P.lds_bytes > 65536 || I.fused_argmin || I.launches != 1) return 15;
        return 0;
    }
    if (I.family == WDX_DTW_SCRATCH) {
        if (w <= kMaxRegWindow || wide_dtw_plan(c.L, c.window, c.wide_dtw != 0).eligible) return 16;
        if (I.launches != (P.lanes + kScratchLanes - 1) / kScratchLanes) return 17;
        const int64_t last = P.lanes - (int64_t)(I.launches - 1) * kScratchLanes;
        if (last < 1 || last > kScratchLanes || I.grid_x != (last + 63) / 64 || I.grid_y != 1 || I.fused_argmin) return 18;
        if (P.scratch_bytes != 2 * (c.L + 1) * kScratchLanes * 8 || I.layout == WDX_DTW_LAYOUT_ROW_MAJOR || I.refs_per_block != P.rows) return 19;
        return 0;
    }
    // the lane-per-pair kernels: one launch, a wave per 64 lanes, the uniform rows split over grid.y
    if (I.launches != 1 || I.grid_x != (P.lanes + 63) / 64) return 20;
    if (I.grid_y * I.refs_per_block < P.rows || (I.grid_y - 1) * I.refs_per_block >= P.rows) return 21;
    if (I.fused_argmin && (I.grid_y != 1 || refs_as_lanes)) return 22;
    const WideDtwPlan wide = wide_dtw_plan(c.L, c.window, c.wide_dtw != 0);
    if ((I.family == WDX_DTW_WIDE) != wide.eligible || P.lds_bytes != wide.lds_bytes) return 23;
    if (I.family == WDX_DTW_WIDE) return (I.band_w || I.exact_w) ? 24 : 0;
    if (w > kMaxRegWindow) return 25;
    if ((I.family == WDX_DTW_SHORT) != (c.L == 25 && w == 15 && !c.no_short_dtw)) return 26;
    if (I.band_w < w || I.exact_w != (I.band_w == 15) || (I.exact_w && w != 15)) return 27;
    if (I.band_w != 8 && I.band_w != 15 && I.band_w != 16 && I.band_w != 32) return 28;
    return 0;
}

#ifndef DTW_PLAN_CHECK_NO_MAIN
int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "sweep")) {
        long long cases = 0, family[WDX_DTW_WIDE + 1] = {}, unsupported = 0;
        int bad = 0;
        sweep([&](const Case &c) {
            const DtwPlan P = c.plan();
            const int rc = check(c, P);
            if (rc && !bad) {
                bad = rc;
                fprintf(stderr, "invariant %d: ", rc);
                print_plan(c, P);
            }
            ++cases, ++family[P.info.family], unsupported += P.unsupported;
        });
        for (int f = 0; f <= WDX_DTW_WIDE; ++f) printf("family %d %lld\n", f, family[f]);
        printf("unsupported %lld\ncases %lld\n", unsupported, cases);
        return bad;
    }
    long long nX, nY, L, window;
    Case c;
    while (scanf("%lld %lld %lld %lld %d %d %d %d %d", &nX, &nY, &L, &window, &c.argmin, &c.entry, &c.no_wavefront, &c.no_short_dtw,
                 &c.wide_dtw) == 9) {
        c.nX = nX, c.nY = nY, c.L = L, c.window = window;
        print_plan(c, c.plan());
    }
    return 0;
}
#endif
