// What a device Fpt_Boost fit does with its sizes (warpdemux_amd/csrc/wdx_boost_fit_plan.h), checked without a GPU: built with the
// system compiler under the address and undefined-behaviour sanitizers and run by tests/test_boost_fit_plan_host.py.
// Over features x classes x depths x border counts x row counts it checks of every admitted plan:
//   1  the row chunks of the histogram kernel cover the n rows exactly once, none holds more than kBoostFitRows rows, and
//      rows * 2^20 < 2^31: an int32 LDS partial cannot overflow; n * 2^20 stays below 2^53 (exact in float64) for the int64 sums
//   2  every workspace piece is 256-byte aligned, the pieces are disjoint and in rising order, each named offset is a piece of the size
//      its array needs, all lie inside bytes, bytes within bytes_bound and within WDX_BOOST_FIT_MAX_WORKSPACE
//   3  per level 0 .. depth (depth: the leaf sums): the slabs cover every column exactly once, a slab's entries fit kBoostFitSlabEntries
//      and the LDS bytes the launch asks for, which stay within 160 KiB; every (feature, column, bin) of the global histogram lies
//      inside the feature's stride and the histogram piece; the grid dimensions are launchable
//   4  the launch count is 1 + n_trees (3 depth + 4)
//   5  the workspace is monotone in n
// and that each refusal carries its code and message.  Prints "checks <n>" / "failures <n>" and what the sweep met.
#include "wdx_boost_fit_plan.h"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

using namespace wdx;

static long long g_checks = 0, g_fail = 0;
#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        ++g_checks;                                                            \
        if (!(cond)) {                                                         \
            if (++g_fail <= 20) {                                              \
                fprintf(stderr, "FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); \
                fprintf(stderr, __VA_ARGS__);                                  \
                fprintf(stderr, "\n");                                         \
            }                                                                  \
        }                                                                      \
    } while (0)

static long long g_plans = 0, g_multi_slab = 0, g_short_chunk = 0, g_whole_chunks = 0, g_refusals = 0, g_inactive = 0, g_cap_refused = 0;

static wdx_boost_fit_params params(int F, int k, int T, int D, int B) {
    wdx_boost_fit_params p;
    memset(&p, 0, sizeof p);
    p.n_features = F, p.n_classes = k, p.n_trees = T, p.depth = D, p.border_count = B;
    p.learning_rate = 0.3, p.l2_leaf_reg = 3.0;
    return p;
}

// every third feature has no border, the others B, B - 1, ... (at least 1); feature 0 always has B
static std::vector<int32_t> some_borders(int F, int B, bool with_inactive) {
    std::vector<int32_t> nb((size_t)F);
    for (int f = 0; f < F; ++f) nb[(size_t)f] = with_inactive && f % 3 == 2 ? 0 : std::max(1, B - f % 5);
    nb[0] = B;
    return nb;
}

static bool is_piece(const BoostFitPlan &P, int64_t off, int64_t bytes) {
    for (int i = 0; i < P.n_pieces; ++i)
        if (P.pieces[i].off == off && P.pieces[i].bytes == bytes) return true;
    return false;
}

static int64_t check_plan(int F, int k, int D, int B, int64_t n, int T, bool with_inactive) {
    const wdx_boost_fit_params p = params(F, k, T, D, B);
    const std::vector<int32_t> nb = some_borders(F, B, with_inactive);
    const BoostFitPlan P = boost_fit_plan(n, F + 2, &p, nb.data(), true, true, true, true, true);
    if (P.rc == WDX_ERR_UNSUPPORTED && strstr(P.msg, "WDX_BOOST_FIT_MAX_WORKSPACE")) {   // the cap: the only refusal the sweep may meet
        ++g_cap_refused;
        return -1;
    }
    CHECK(P.rc == WDX_SUCCESS, "rc %d: %s", P.rc, P.msg);
    if (P.rc != WDX_SUCCESS) return -1;
    ++g_plans;
    if (with_inactive && F >= 3) ++g_inactive;
    CHECK(P.n == n && P.F == F && P.k == k && P.ch == k + 1 && P.D == D && P.T == T && P.NB == B + 1, "sizes");
    // 1: chunks and the overflow bounds
    CHECK(P.chunks == (n + kBoostFitRows - 1) / kBoostFitRows && (P.chunks - 1) * kBoostFitRows < n && P.chunks * kBoostFitRows >= n, "chunks %lld", (long long)P.chunks);
    CHECK(((int64_t)kBoostFitRows << kBoostFitGradBits) < ((int64_t)1 << 31), "the 32-bit partial bound");
    CHECK((n << kBoostFitGradBits) < ((int64_t)1 << 53), "the int64 sums are exact in float64");
    if (n % kBoostFitRows) ++g_short_chunk; else ++g_whole_chunks;
    CHECK(P.row_grid() * kBoostFitThreads >= n && (P.row_grid() - 1) * kBoostFitThreads < n, "row grid");
    CHECK(P.chunks <= 2147483647LL && P.row_grid() <= 2147483647LL && F <= 65535, "grid x, y");
    // 2: workspace
    int64_t end = 0, raw = 0;
    for (int i = 0; i < P.n_pieces; ++i) {
        CHECK(P.pieces[i].off % 256 == 0 && P.pieces[i].off >= end && P.pieces[i].bytes >= 0, "piece %d", i);
        end = P.pieces[i].off + P.pieces[i].bytes;
        raw += P.pieces[i].bytes;
    }
    CHECK(P.n_pieces == kBoostFitPieces && end <= P.bytes && P.bytes <= P.bytes_bound && P.bytes_bound == raw + 256 * (int64_t)P.n_pieces, "bytes");
    CHECK(P.bytes <= WDX_BOOST_FIT_MAX_WORKSPACE, "cap");
    const int64_t leaves = (int64_t)1 << D;
    int64_t total = 0;
    for (int f = 0; f < F; ++f) total += nb[(size_t)f];
    CHECK(P.total_borders == total && is_piece(P, P.off_borders, 4 * total) && is_piece(P, P.off_border_off, 4 * (int64_t)(F + 1)), "borders");
    CHECK(is_piece(P, P.off_bins, n * F) && is_piece(P, P.off_q, 4 * n * k) && is_piece(P, P.off_leaf, n), "rows");
    CHECK(is_piece(P, P.off_hist, P.hist_bytes) && P.hist_bytes == 8 * P.hist_feature_stride * F && is_piece(P, P.off_leafsum, 8 * leaves * (k + 1)), "hist");
    CHECK(is_piece(P, P.off_cand_score, 8 * (int64_t)F) && is_piece(P, P.off_cand_b, 4 * (int64_t)F), "candidates");
    CHECK(is_piece(P, P.off_split_f, 4 * (int64_t)T * D) && is_piece(P, P.off_split_b, 4 * (int64_t)T * D) &&
              is_piece(P, P.off_leaves, 8 * (int64_t)T * leaves * k) && is_piece(P, P.off_flags, 8), "outputs");
    // 3: slabs
    for (int l = 0; l <= D; ++l) {
        const int cols = P.cols(l), bins = P.bins_of(l), cps = P.cols_per_slab(l), slabs = P.slabs(l);
        CHECK(cols == (1 << l) * (k + 1) && bins == (l == D ? 1 : B + 1) && cps >= 1 && slabs >= 1 && slabs <= 65535, "level %d", l);
        int covered = 0;
        int64_t most = 0;
        for (int s = 0; s < slabs; ++s) {
            const int nc = P.slab_cols(l, s);
            CHECK(nc >= 1 && nc <= cps && s * cps == covered, "level %d slab %d", l, s);
            CHECK((int64_t)nc * bins <= kBoostFitSlabEntries && 4 * (int64_t)nc * bins <= P.lds_bytes(l), "level %d slab %d entries", l, s);
            most = std::max<int64_t>(most, (int64_t)nc * bins);
            covered += nc;
        }
        CHECK(covered == cols, "level %d: the slabs hold %d of %d columns", l, covered, cols);
        CHECK(P.lds_bytes(l) == 4 * most && P.lds_bytes(l) <= 160 * 1024, "level %d lds %lld", l, (long long)P.lds_bytes(l));
        if (slabs > 1) ++g_multi_slab;
        if (l < D)   // the last entry of the level's histogram of a feature lies inside the feature's stride
            CHECK((int64_t)cols * bins <= P.hist_feature_stride, "level %d stride", l);
        else
            CHECK((int64_t)cols * bins == leaves * (k + 1), "leaf sums");
    }
    CHECK(P.hist_feature_stride == (leaves / 2) * (k + 1) * (B + 1), "stride");
    // 4
    CHECK(P.launches == 1 + (int64_t)T * (3 * D + 4) && P.launches_per_tree() == 3 * D + 4, "launches");
    return P.bytes;
}

static void refused(const char *what, int64_t n, int64_t ld, const wdx_boost_fit_params *p, const int32_t *nb, bool hx, bool hy, bool hb, bool hs, bool ho,
                    int code, const char *needle) {
    const BoostFitPlan P = boost_fit_plan(n, ld, p, nb, hx, hy, hb, hs, ho);
    CHECK(P.rc == code && strstr(P.msg, needle) && P.bytes == 0 && P.n_pieces == 0, "%s: rc %d, message '%s'", what, P.rc, P.msg);
    ++g_refusals;
}

int main() {
    const int Fs[] = {1, 2, 3, 25, 120, 254}, ks[] = {2, 3, 4, 10, 16}, Ds[] = {1, 2, 3, 6, 8}, Bs[] = {1, 2, 31, 32, 63, 128, 254, 255};
    const int64_t ns[] = {1, 2, 63, 64, 65, 2046, 2047, 2048, 4094, 6146, 30000, 200000, (int64_t)1 << 24};
    for (int F : Fs)
        for (int k : ks)
            for (int D : Ds)
                for (int B : Bs) {
                    int64_t before = 0;
                    for (int64_t n : ns) {   // 5: monotone in n (rising)
                        const int64_t bytes = check_plan(F, k, D, B, n, 3, (F + k + D + B) % 2 == 0);
                        if (bytes < 0) {
                            before = WDX_BOOST_FIT_MAX_WORKSPACE;
                            continue;
                        }
                        CHECK(bytes >= before, "workspace not monotone in n at F %d k %d D %d B %d n %lld", F, k, D, B, (long long)n);
                        before = bytes;
                    }
                }
    // the issue's two extremes are admitted
    CHECK(check_plan(25, 4, 6, 128, 200000, 1000, false) > 0, "depth 6, 128 borders, 4 classes");
    CHECK(check_plan(254, 16, 8, 255, 65, 1, false) > 0, "depth 8, 255 borders, 16 classes");

    // refusals
    wdx_boost_fit_params ok = params(25, 4, 10, 6, 32), p;
    const std::vector<int32_t> nb = some_borders(254, 32, false);
    std::vector<int32_t> bad;
    const int U = WDX_ERR_UNSUPPORTED, I = WDX_ERR_INVALID;
    refused("no params", 100, 25, nullptr, nb.data(), true, true, true, true, true, I, "parameters are required");
    refused("n 0", 0, 25, &ok, nb.data(), true, true, true, true, true, I, "n must be at least 1");
    refused("n large", ((int64_t)1 << 24) + 1, 25, &ok, nb.data(), true, true, true, true, true, U, "WDX_BOOST_FIT_MAX_ROWS");
    p = ok, p.n_features = 0;
    refused("F 0", 100, 25, &p, nb.data(), true, true, true, true, true, I, "n_features");
    p = ok, p.n_features = 255;
    refused("F 255", 100, 255, &p, nb.data(), true, true, true, true, true, U, "255 features");
    p = ok, p.n_classes = 1;
    refused("k 1", 100, 25, &p, nb.data(), true, true, true, true, true, I, "at least two");
    p = ok, p.n_classes = 17;
    refused("k 17", 100, 25, &p, nb.data(), true, true, true, true, true, U, "17 classes");
    p = ok, p.depth = 0;
    refused("D 0", 100, 25, &p, nb.data(), true, true, true, true, true, I, "depth = 0");
    p = ok, p.depth = 9;
    refused("D 9", 100, 25, &p, nb.data(), true, true, true, true, true, U, "depth 9");
    p = ok, p.border_count = 0;
    refused("B 0", 100, 25, &p, nb.data(), true, true, true, true, true, I, "border_count = 0");
    p = ok, p.border_count = 256;
    refused("B 256", 100, 25, &p, nb.data(), true, true, true, true, true, U, "border_count 256");
    p = ok, p.n_trees = 0;
    refused("T 0", 100, 25, &p, nb.data(), true, true, true, true, true, I, "n_trees = 0");
    p = ok, p.n_trees = WDX_BOOST_FIT_MAX_TREES + 1;
    refused("T large", 100, 25, &p, nb.data(), true, true, true, true, true, U, "WDX_BOOST_FIT_MAX_TREES");
    p = ok, p.reserved = 1;
    refused("reserved", 100, 25, &p, nb.data(), true, true, true, true, true, I, "reserved");
    p = ok, p.l2_leaf_reg = 0.0;
    refused("lambda 0", 100, 25, &p, nb.data(), true, true, true, true, true, I, "l2_leaf_reg");
    p = ok, p.l2_leaf_reg = -1.0;
    refused("lambda < 0", 100, 25, &p, nb.data(), true, true, true, true, true, I, "l2_leaf_reg");
    p = ok, p.l2_leaf_reg = NAN;
    refused("lambda nan", 100, 25, &p, nb.data(), true, true, true, true, true, I, "l2_leaf_reg");
    p = ok, p.learning_rate = INFINITY;
    refused("lr inf", 100, 25, &p, nb.data(), true, true, true, true, true, I, "learning_rate");
    p = ok, p.learning_rate = NAN;
    refused("lr nan", 100, 25, &p, nb.data(), true, true, true, true, true, I, "learning_rate");
    refused("ld", 100, 24, &ok, nb.data(), true, true, true, true, true, I, "ld = 24");
    refused("no X", 100, 25, &ok, nb.data(), false, true, true, true, true, I, "fingerprints are required");
    refused("no y", 100, 25, &ok, nb.data(), true, false, true, true, true, I, "class indices are required");
    refused("no borders", 100, 25, &ok, nb.data(), true, true, false, true, true, I, "borders and n_borders");
    refused("no n_borders", 100, 25, &ok, nullptr, true, true, true, true, true, I, "borders and n_borders");
    refused("no scores", 100, 25, &ok, nb.data(), true, true, true, false, true, I, "scores are required");
    refused("no outputs", 100, 25, &ok, nb.data(), true, true, true, true, false, I, "split_feature, split_border and leaf_values");
    bad = nb, bad[3] = 33;
    refused("n_borders > B", 100, 25, &ok, bad.data(), true, true, true, true, true, I, "n_borders[3] = 33");
    bad = nb, bad[7] = -1;
    refused("n_borders < 0", 100, 25, &ok, bad.data(), true, true, true, true, true, I, "n_borders[7] = -1");
    bad.assign(254, 0);
    refused("no feature with a border", 100, 25, &ok, bad.data(), true, true, true, true, true, I, "no feature has a border");
    p = params(254, 16, 1, 8, 255);
    {
        const std::vector<int32_t> wide = some_borders(254, 255, false);
        refused("workspace cap", (int64_t)1 << 24, 254, &p, wide.data(), true, true, true, true, true, U, "WDX_BOOST_FIT_MAX_WORKSPACE");
    }
    p = params(4, 4, WDX_BOOST_FIT_MAX_TREES, 8, 32);
    refused("workspace cap by trees", 1000, 4, &p, nb.data(), true, true, true, true, true, U, "WDX_BOOST_FIT_MAX_WORKSPACE");

    printf("checks %lld\nfailures %lld\nplans %lld\nmulti_slab %lld\nshort_chunk %lld\nwhole_chunks %lld\ninactive %lld\ncap_refused %lld\nrefusals %lld\nrows %d\n",
           g_checks, g_fail, g_plans, g_multi_slab, g_short_chunk, g_whole_chunks, g_inactive, g_cap_refused, g_refusals, kBoostFitRows);
    return g_fail ? 1 : 0;
}
