// The device trainer of Fpt_Boost (include/wdx.h: wdx_boost_fit_device states the rule): what a fit does with its sizes, before anything
// is launched -- the one statement of it (plain C++17: no device runtime, nothing of the context, so the system compiler builds it
// alone: tests/host/boost_fit_plan_check.cpp).  wdx_boost_fit.hip launches what the plan names.
//
//   channels   ch = k + 1 per leaf: the k quantised gradients and the row count
//   columns    a level l histogram has cols(l) = 2^l * ch columns (leaf-major, channel fastest) of NB = max n_borders + 1 bins per
//              feature; the leaf sums behind the last level are the same thing with 2^depth leaves and ONE bin
//   histogram  one workgroup of 256 threads per (row chunk, feature, slab): a chunk is kBoostFitRows = 2047 rows, a slab
//              cols_per_slab(NB) = kBoostFitSlabEntries / NB whole columns, at most 8 192 int32 LDS entries (32 KiB: five workgroups
//              a CU by LDS, 20 waves).  The workgroup zeroes its slab, adds its rows with 32-bit LDS atomics, and flushes the entries
//              that are not zero to the global int64 histogram with 64-bit atomics.
//   tree       1 softmax + depth x (histogram, scan, update) + leaf histogram + leaf values + score update = 3 depth + 4 launches
//
// OVERFLOW BOUNDS (checked here and by the host program): |q| <= 2^20, so an int32 LDS entry holds at most
// kBoostFitRows * 2^20 = 2^31 - 2^20 < 2^31 in magnitude and a count of at most 2047; a global int64 entry at most n * 2^20 <= 2^44;
// (double)G is exact below 2^53 and G * G <= 2^88 is finite.
//
// WORKSPACE (context-owned, grow-only; 256 B of alignment per piece; bytes <= bytes_bound; at most WDX_BOOST_FIT_MAX_WORKSPACE):
//   borders f32 | border offsets int32[F + 1] | bins uint8 (F, n) | q int32 (k, n) | leaf uint8[n] | histogram int64 (F, 2^(depth-1) ch, NB)
//   | leaf sums int64 (2^depth, ch) | candidates: score f64[F], border int32[F] | split feature, split border int32[T depth] | leaf
//   values f64[T 2^depth k] | flags int32[2]
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/wdx.h"

namespace wdx {

constexpr int kBoostFitRows = WDX_BOOST_FIT_ROWS;       // rows per histogram workgroup
constexpr int kBoostFitThreads = 256;                   // four waves, every kernel of the trainer
constexpr int kBoostFitSlabEntries = 8192;              // int32 LDS entries of one histogram workgroup
constexpr int kBoostFitGradBits = WDX_BOOST_FIT_GRAD_BITS;
constexpr int kBoostFitMaxClasses = 16;
constexpr int kBoostFitPieces = 13;
static_assert((int64_t)kBoostFitRows << kBoostFitGradBits < ((int64_t)1 << 31), "an int32 LDS partial cannot overflow");
static_assert(kBoostFitSlabEntries / (WDX_BOOST_FIT_MAX_BORDERS + 1) >= 1, "a slab holds at least one column");

// exp_rule's constants (fdlibm's) and coefficients c_i = c_{i-1} / i
constexpr double kBoostFitLog2e = 0x1.71547652b82fep+0, kBoostFitLn2Hi = 0x1.62e42feep-1, kBoostFitLn2Lo = 0x1.a39ef35793c76p-33;
constexpr int kBoostFitExpDegree = 13;
struct BoostFitExpCoef {
    double c[kBoostFitExpDegree + 1];
    constexpr BoostFitExpCoef() : c{} {
        c[0] = 1.0;
        for (int i = 1; i <= kBoostFitExpDegree; ++i) c[i] = c[i - 1] / (double)i;
    }
};

inline int64_t boost_fit_align(int64_t b) { return (b + 255) / 256 * 256; }

struct BoostFitPiece { int64_t off, bytes; };

struct BoostFitPlan {
    int rc = WDX_SUCCESS;
    char msg[224] = {0};
    int64_t n = 0, ld = 0;
    int F = 0, k = 0, ch = 0, T = 0, D = 0, B = 0;
    int NB = 0;                       // bins per feature in the histogram: the largest n_borders + 1
    int n_active = 0;                 // features with a border
    int64_t total_borders = 0;
    int64_t chunks = 0;               // row chunks of the histogram kernel
    int64_t hist_feature_stride = 0;  // int64 entries per feature: 2^(D-1) * ch * NB
    int64_t launches = 0;             // of the whole call
    int64_t off_borders = 0, off_border_off = 0, off_bins = 0, off_q = 0, off_leaf = 0, off_hist = 0, off_leafsum = 0, off_cand_score = 0,
            off_cand_b = 0, off_split_f = 0, off_split_b = 0, off_leaves = 0, off_flags = 0;
    int64_t hist_bytes = 0, bytes = 0, bytes_bound = 0;
    int n_pieces = 0;
    BoostFitPiece pieces[kBoostFitPieces] = {};

    int cols(int level) const { return (1 << level) * ch; }            // level == D: the leaf sums
    int bins_of(int level) const { return level == D ? 1 : NB; }
    int cols_per_slab(int level) const { return kBoostFitSlabEntries / bins_of(level); }
    int slabs(int level) const { return (cols(level) + cols_per_slab(level) - 1) / cols_per_slab(level); }
    int slab_cols(int level, int slab) const {
        const int c0 = slab * cols_per_slab(level), left = cols(level) - c0;
        return left < cols_per_slab(level) ? left : cols_per_slab(level);
    }
    int64_t lds_bytes(int level) const { return 4 * (int64_t)(slabs(level) == 1 ? cols(level) : cols_per_slab(level)) * bins_of(level); }
    int64_t row_grid() const { return (n + kBoostFitThreads - 1) / kBoostFitThreads; }
    int launches_per_tree() const { return 3 * D + 4; }
};

// n_borders: the caller's host array (nullable: refused); the have_* flags: that pointer argument is there
inline BoostFitPlan boost_fit_plan(int64_t n, int64_t ld, const wdx_boost_fit_params *p, const int32_t *n_borders, bool have_X, bool have_y,
                                   bool have_borders, bool have_scores, bool have_out) {
    BoostFitPlan P;
#define WDX_BOOST_FIT_REFUSE(code, ...)                \
    do {                                               \
        P = BoostFitPlan();                            \
        snprintf(P.msg, sizeof P.msg, __VA_ARGS__);    \
        P.rc = (code);                                 \
        return P;                                      \
    } while (0)
    if (!p) WDX_BOOST_FIT_REFUSE(WDX_ERR_INVALID, "boost fit: the parameters are required (NULL given)");
    if (n < 1) WDX_BOOST_FIT_REFUSE(WDX_ERR_INVALID, "boost fit: n must be at least 1, not %lld", (long long)n);
    if (n > WDX_BOOST_FIT_MAX_ROWS)
        WDX_BOOST_FIT_REFUSE(WDX_ERR_UNSUPPORTED, "boost fit: n = %lld rows, more than WDX_BOOST_FIT_MAX_ROWS = %d", (long long)n, WDX_BOOST_FIT_MAX_ROWS);
    if (p->n_features < 1) WDX_BOOST_FIT_REFUSE(WDX_ERR_INVALID, "boost fit: n_features = %d must be at least 1", p->n_features);
    if (p->n_features > WDX_BOOST_MAX_FEATURES)
        WDX_BOOST_FIT_REFUSE(WDX_ERR_UNSUPPORTED, "boost fit: %d features (1..%d supported)", p->n_features, WDX_BOOST_MAX_FEATURES);
    if (p->n_classes < 2) WDX_BOOST_FIT_REFUSE(WDX_ERR_INVALID, "boost fit: n_classes = %d, at least two are required", p->n_classes);
    if (p->n_classes > kBoostFitMaxClasses) WDX_BOOST_FIT_REFUSE(WDX_ERR_UNSUPPORTED, "boost fit: %d classes (2..%d supported)", p->n_classes, kBoostFitMaxClasses);
    if (p->depth < 1) WDX_BOOST_FIT_REFUSE(WDX_ERR_INVALID, "boost fit: depth = %d must be at least 1", p->depth);
    if (p->depth > WDX_BOOST_FIT_MAX_DEPTH)
        WDX_BOOST_FIT_REFUSE(WDX_ERR_UNSUPPORTED, "boost fit: depth %d (1..WDX_BOOST_FIT_MAX_DEPTH = %d supported)", p->depth, WDX_BOOST_FIT_MAX_DEPTH);
    if (p->border_count < 1) WDX_BOOST_FIT_REFUSE(WDX_ERR_INVALID, "boost fit: border_count = %d must be at least 1", p->border_count);
    if (p->border_count > WDX_BOOST_FIT_MAX_BORDERS)
        WDX_BOOST_FIT_REFUSE(WDX_ERR_UNSUPPORTED, "boost fit: border_count %d (1..WDX_BOOST_FIT_MAX_BORDERS = %d supported)", p->border_count,
                             WDX_BOOST_FIT_MAX_BORDERS);
    if (p->n_trees < 1) WDX_BOOST_FIT_REFUSE(WDX_ERR_INVALID, "boost fit: n_trees = %d must be at least 1", p->n_trees);
    if (p->n_trees > WDX_BOOST_FIT_MAX_TREES)
        WDX_BOOST_FIT_REFUSE(WDX_ERR_UNSUPPORTED, "boost fit: %d trees in one call, more than WDX_BOOST_FIT_MAX_TREES = %d", p->n_trees, WDX_BOOST_FIT_MAX_TREES);
    if (p->reserved != 0) WDX_BOOST_FIT_REFUSE(WDX_ERR_INVALID, "boost fit: the reserved field must be 0, not %d", p->reserved);
    if (!(p->l2_leaf_reg > 0) || !isfinite(p->l2_leaf_reg))
        WDX_BOOST_FIT_REFUSE(WDX_ERR_INVALID, "boost fit: l2_leaf_reg must be positive and finite, not %g", p->l2_leaf_reg);
    if (!isfinite(p->learning_rate)) WDX_BOOST_FIT_REFUSE(WDX_ERR_INVALID, "boost fit: learning_rate must be finite, not %g", p->learning_rate);
    if (ld < p->n_features) WDX_BOOST_FIT_REFUSE(WDX_ERR_INVALID, "boost fit: ld = %lld is less than the %d features", (long long)ld, p->n_features);
    if (!have_X) WDX_BOOST_FIT_REFUSE(WDX_ERR_INVALID, "boost fit: the fingerprints are required (NULL given)");
    if (!have_y) WDX_BOOST_FIT_REFUSE(WDX_ERR_INVALID, "boost fit: the class indices are required (NULL given)");
    if (!have_borders || !n_borders) WDX_BOOST_FIT_REFUSE(WDX_ERR_INVALID, "boost fit: borders and n_borders are required (NULL given)");
    if (!have_scores) WDX_BOOST_FIT_REFUSE(WDX_ERR_INVALID, "boost fit: the scores are required (NULL given)");
    if (!have_out) WDX_BOOST_FIT_REFUSE(WDX_ERR_INVALID, "boost fit: split_feature, split_border and leaf_values are required (NULL given)");
    int most = 0, active = 0;
    int64_t total = 0;
    for (int f = 0; f < p->n_features; ++f) {
        if (n_borders[f] < 0 || n_borders[f] > p->border_count)
            WDX_BOOST_FIT_REFUSE(WDX_ERR_INVALID, "boost fit: n_borders[%d] = %d lies outside 0 .. border_count = %d", f, n_borders[f], p->border_count);
        most = n_borders[f] > most ? n_borders[f] : most;
        active += n_borders[f] > 0;
        total += n_borders[f];
    }
    if (!active) WDX_BOOST_FIT_REFUSE(WDX_ERR_INVALID, "boost fit: no feature has a border (every column is constant or NaN): nothing to split on");

    P.n = n, P.ld = ld, P.F = p->n_features, P.k = p->n_classes, P.ch = P.k + 1, P.T = p->n_trees, P.D = p->depth, P.B = p->border_count;
    P.NB = most + 1, P.n_active = active, P.total_borders = total;
    P.chunks = (n + kBoostFitRows - 1) / kBoostFitRows;
    P.hist_feature_stride = (int64_t)(1 << (P.D - 1)) * P.ch * P.NB;
    P.launches = 1 + (int64_t)P.T * P.launches_per_tree();

    int64_t at = 0, raw = 0;
    auto piece = [&](int64_t bytes) {
        const int64_t o = at;
        P.pieces[P.n_pieces++] = BoostFitPiece{o, bytes};
        at += boost_fit_align(bytes);
        raw += bytes;
        return o;
    };
    const int64_t leaves = (int64_t)1 << P.D;
    P.off_borders = piece(4 * total);
    P.off_border_off = piece(4 * (int64_t)(P.F + 1));
    P.off_bins = piece(n * P.F);
    P.off_q = piece(4 * n * P.k);
    P.off_leaf = piece(n);
    P.hist_bytes = 8 * P.hist_feature_stride * P.F;
    P.off_hist = piece(P.hist_bytes);
    P.off_leafsum = piece(8 * leaves * P.ch);
    P.off_cand_score = piece(8 * (int64_t)P.F);
    P.off_cand_b = piece(4 * (int64_t)P.F);
    P.off_split_f = piece(4 * (int64_t)P.T * P.D);
    P.off_split_b = piece(4 * (int64_t)P.T * P.D);
    P.off_leaves = piece(8 * (int64_t)P.T * leaves * P.k);
    P.off_flags = piece(2 * 4);
    P.bytes = at;
    P.bytes_bound = raw + 256 * (int64_t)P.n_pieces;
    if (P.bytes > WDX_BOOST_FIT_MAX_WORKSPACE) {
        const long long need = (long long)P.bytes;
        WDX_BOOST_FIT_REFUSE(WDX_ERR_UNSUPPORTED, "boost fit: this fit needs a workspace of %lld bytes, more than WDX_BOOST_FIT_MAX_WORKSPACE = %lld", need,
                             (long long)WDX_BOOST_FIT_MAX_WORKSPACE);
    }
#undef WDX_BOOST_FIT_REFUSE
    return P;
}

}  // namespace wdx
