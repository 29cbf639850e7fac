// Stand-alone driver of nearest_plan (warpdemux_amd/csrc/wdx_dtw_plan.h) -- where the nearest-reference rule of a dispatch is
// computed: in the DTW kernel's epilogue, behind it on the caller's matrix, or behind it through the block buffer -- built by
// tests/test_nearest_host.py with the system compiler and the address / undefined-behaviour sanitizers.
//   nearest_plan_check         reads cases from stdin, one per line: "nX nY L window have_dist refs_any_inf entry no_wavefront
//                              no_short_dtw wide_dtw" (entry 0: wdx_nearest_dev / wdx_dtw_nearest, 1: wdx_demux_nearest_dev), and
//                              prints the case followed by "rule(0 none, 1 fused, 2 after) buffer block_rows buffer_bytes family
//                              band_w layout fused_argmin grid_y unsupported argmin_after"
//   nearest_plan_check sweep   checks over a sweep of shapes what must hold of every such plan (exit status = the invariant that
//                              failed) and prints "rule <id> <cases>" and "cases <n>"
#include "wdx_dtw_plan.h"

#include <stdio.h>
#include <string.h>

using namespace wdx;

struct Case {
    int64_t nX, nY, L, window;
    int have_dist, any_inf, entry, no_wavefront, no_short_dtw, wide_dtw;
    DtwSwitches sw() const { return DtwSwitches{no_wavefront != 0, no_short_dtw != 0, wide_dtw != 0}; }
    DtwEntry e() const { return entry ? DtwEntry::kFused : DtwEntry::kMatrix; }
    NearestPlan plan() const { return nearest_plan(nX, nY, L, window, have_dist != 0, any_inf != 0, e(), sw()); }
};

// what must hold of every plan; 0 or the number of the invariant that does not
static int check(const Case &c, const NearestPlan &N) {
    const DtwPlan D = dtw_plan(c.nX, c.nY, c.L, c.window, true, c.e(), c.sw());
    const wdx_dtw_launch_info &I = N.dtw.info;
    // nothing to dispatch, or the fused entry's refusal: no rule, and the DTW plan's own answer
    if (D.unsupported || D.info.family == WDX_DTW_NONE)
        return (N.rule == NearestRule::kNone && N.dtw.unsupported == D.unsupported && I.family == WDX_DTW_NONE && !N.buffer) ? 0 : 1;
    if (N.rule == NearestRule::kNone) return 2;
    if (N.dtw.argmin_after) return 3;   // no argmin kernel ever follows: the rule has its own first-minimum column
    if (N.block_rows < 1 || N.block_rows > c.nX) return 4;
    if (N.rule == NearestRule::kFused) {
        // one lane walks every reference of its read, no reference holds an infinity, no buffer
        if (!I.fused_argmin || I.grid_y != 1 || I.refs_per_block != c.nY || I.layout == WDX_DTW_LAYOUT_REFS_AS_LANES) return 5;
        if (I.family != WDX_DTW_BAND && I.family != WDX_DTW_SHORT && I.family != WDX_DTW_WIDE) return 6;
        if (c.any_inf || N.buffer || N.buffer_bytes) return 7;
        if (N.block_rows == c.nX && !D.info.fused_argmin) return 8;   // (the whole call: exactly today's fused-argmin condition)
        return 0;
    }
    if (I.fused_argmin) return 9;
    if (!c.any_inf && N.block_rows == c.nX && D.info.fused_argmin) return 10;
    if (N.buffer != (c.have_dist == 0)) return 11;
    if (!N.buffer) return (N.block_rows == c.nX && N.buffer_bytes == 0) ? 0 : 12;
    if (N.buffer_bytes != N.block_rows * c.nY * 4) return 13;
    if (N.buffer_bytes > kNearestBlockBytes && N.block_rows != 1) return 14;
    // a block is the whole call or as many rows as the buffer holds (whole waves of them)
    if (N.block_rows < c.nX && (N.block_rows + 64) * c.nY * 4 <= kNearestBlockBytes) return 15;
    // the plan is the plan of one block
    const DtwPlan B = dtw_plan(N.block_rows, c.nY, c.L, c.window, true, c.e(), c.sw());
    if (B.info.family != I.family || B.info.grid_x != I.grid_x || B.info.grid_y != I.grid_y || B.info.layout != I.layout) return 16;
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "sweep")) {
        static const int64_t NX[] = {0, 1, 2, 63, 64, 65, 1000, 4096, 8191, 8192, 16385, 131008, 131009, 131072, 300000, 1572864, 3000000};
        static const int64_t NY[] = {0, 1, 2, 5, 6, 10, 12, 31, 32, 40, 200, 2601, 65537, 30000000};
        static const int64_t LW[][2] = {{25, 15}, {25, 0}, {40, 8}, {40, 15}, {40, 16}, {40, 32}, {40, 0}, {33, 15}, {110, 15}, {110, 0}, {300, 0}};
        long long cases = 0, by_rule[3] = {0, 0, 0};
        for (int64_t nX : NX)
            for (int64_t nY : NY)
                for (const auto &lw : LW)
                    for (int bits = 0; bits < 64; ++bits) {
                        const Case c{nX, nY, lw[0], lw[1], bits & 1, (bits >> 1) & 1, (bits >> 2) & 1, (bits >> 3) & 1, (bits >> 4) & 1, (bits >> 5) & 1};
                        const NearestPlan N = c.plan();
                        if (const int bad = check(c, N)) {
                            fprintf(stderr, "invariant %d: nX %lld nY %lld L %lld window %lld bits %d\n", bad, (long long)nX, (long long)nY,
                                    (long long)lw[0], (long long)lw[1], bits);
                            return bad;
                        }
                        ++cases, ++by_rule[(int)N.rule];
                    }
        for (int r = 0; r < 3; ++r) printf("rule %d %lld\n", r, by_rule[r]);
        printf("cases %lld\n", cases);
        return 0;
    }
    Case c;
    long long nX, nY, L, window;
    while (scanf("%lld %lld %lld %lld %d %d %d %d %d %d", &nX, &nY, &L, &window, &c.have_dist, &c.any_inf, &c.entry, &c.no_wavefront,
                 &c.no_short_dtw, &c.wide_dtw) == 10) {
        c.nX = nX, c.nY = nY, c.L = L, c.window = window;
        const NearestPlan N = c.plan();
        const wdx_dtw_launch_info &I = N.dtw.info;
        printf("%lld %lld %lld %lld %d %d %d %d %d %d", nX, nY, L, window, c.have_dist, c.any_inf, c.entry, c.no_wavefront, c.no_short_dtw,
               c.wide_dtw);
        printf(" %d %d %lld %lld %d %d %d %d %lld %d %d\n", (int)N.rule, (int)N.buffer, (long long)N.block_rows, (long long)N.buffer_bytes,
               I.family, I.band_w, I.layout, I.fused_argmin, (long long)I.grid_y, (int)N.dtw.unsupported, (int)N.dtw.argmin_after);
    }
    return 0;
}
