// Leave-one-out nearest neighbours of a labelled set (include/wdx.h: wdx_self_nearest_device): what a call does with its sizes,
// before anything is launched -- the one statement of it (plain C++17: no device runtime, nothing of the context, so the system
// compiler builds it alone: tests/host/loo_plan_check.cpp).  wdx_dtw_loo.hip launches what the plan names.
//
//   rows       the n rows of the call in their own order, padded to rows_padded = 64 x chunks (padding rows are no members), as
//              in wdx_self_plan.h
//   tiles      the self matrix's: 64 x 64 tiles (I, J), J >= I, of the chunk x chunk matrix, the diagonal ones (tile k is (k, k))
//              and the strictly upper ones (medoid_upper_tile) in two lists.  Every unordered pair of rows lies in exactly one
//              tile; a tile merges its row side (rows of chunk I over the columns of chunk J) and its column side (rows of chunk J
//              over the rows of chunk I) into the keys.
//   keys       one uint64 per padded row and side {own, other}: (float32 bits of the distance << 32) | row index of the
//              candidate; all-ones = no candidate.  Distances are >= +0, so the unsigned order of a key is the rule's order
//              (+inf behind every finite value, the lowest index among equals), and the minimum over any set of tiles does not
//              depend on the order they finish in.
//   blocks     general route (effective windows beyond the register band, window 0, WDX_OPT_SELF_NEAREST_GENERAL): PADDED rows
//              [r0, r0 + rows) against all padded rows, one dispatch of dtw_plan / run_dtw_plan each into the float32 block; rows
//              is a multiple of 64 (the rows of a block are the lanes of its dispatch), as many as kLooBlockBytes holds.  A rows
//              kernel applies the rule to each row of the block and writes nn / best itself: this route has no keys.
//
// WORKSPACE BOUND (context-owned, grow-only; LooPlan::workspace_bytes, checked by the host program): O(n x L)
//   gathered rows  rows_padded x (L + Lpad) x 8 B (dense and with the zero halo), rows_padded <= n + 63
//   member flags   1 B, labels 4 B, keys 16 B per padded row
//   general route  + the float32 block, <= kLooBlockBytes = 96 MiB
//   plus 256 B of alignment per piece.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/wdx.h"
#include "wdx_medoid_plan.h"

namespace wdx {

constexpr int64_t kLooMaxRows = WDX_SELF_MATRIX_MAX_ROWS;
constexpr int64_t kLooBlockBytes = 96ll << 20;
constexpr uint64_t kLooNoKey = ~0ull;   // "no candidate"
static_assert(kLooMaxRows % kMedoidChunk == 0 && kLooBlockBytes / (kLooMaxRows * 4) >= kMedoidChunk, "64 padded rows of the cap fit a block");

// the key of candidate `row` at distance bits `fbits` (a float32 >= +0 or +inf)
inline uint64_t loo_key(uint32_t fbits, int64_t row) { return ((uint64_t)fbits << 32) | (uint64_t)(uint32_t)row; }

struct LooTile { int32_t I, J; };
struct LooBlock { int64_t r0, rows; };   // padded rows

struct LooPlan {
    int rc = WDX_SUCCESS;
    char msg[192] = {0};
    int64_t n = 0, L = 0, Lpad = 0;
    MedoidKernel kernel = MedoidKernel::kGeneral;
    bool general = false;
    int64_t chunks = 0, rows_padded = 0;
    int64_t n_diag = 0, n_off = 0;
    std::vector<LooBlock> blocks;   // general route only
    int64_t block_rows = 0, block_bytes = 0;
    // the context-owned workspace: byte offsets of its pieces, and its size
    int64_t off_member = 0, off_label = 0, off_keys = 0, off_dense = 0, off_padded = 0, off_block = 0;
    int64_t workspace_bytes = 0, workspace_bound = 0;

    int64_t tile_count() const { return n_diag + n_off; }
    // tile k of the call: the diagonal ones first
    LooTile tile(int64_t k) const {
        LooTile T{0, 0};
        if (k < n_diag) T.I = T.J = (int32_t)k;
        else medoid_upper_tile(chunks, k - n_diag, &T.I, &T.J);
        return T;
    }
};

// have_out: nn and best are both there (they may be missing when n == 0); opt_general: WDX_OPT_SELF_NEAREST_GENERAL
inline LooPlan loo_plan(int64_t n, int64_t L, int64_t window, bool have_out, bool opt_general, bool no_short_dtw) {
    LooPlan P;
    auto refuse = [&P](int rc) -> LooPlan & {
        P.rc = rc;
        return P;
    };
    if (L < 1) {
        snprintf(P.msg, sizeof P.msg, "self nearest: L must be at least 1, not %lld", (long long)L);
        return refuse(WDX_ERR_INVALID);
    }
    if (n < 0) {
        snprintf(P.msg, sizeof P.msg, "self nearest: n must not be negative (n = %lld)", (long long)n);
        return refuse(WDX_ERR_INVALID);
    }
    if (n > kLooMaxRows) {
        snprintf(P.msg, sizeof P.msg, "self nearest: n = %lld rows, more than WDX_SELF_MATRIX_MAX_ROWS = %lld: subsample them", (long long)n,
                 (long long)kLooMaxRows);
        return refuse(WDX_ERR_UNSUPPORTED);
    }
    if (n > 0 && !have_out) {
        snprintf(P.msg, sizeof P.msg, "self nearest: the outputs nn and best are required (NULL given)");
        return refuse(WDX_ERR_INVALID);
    }
    P.n = n, P.L = L, P.Lpad = dtw_padded_length(L);
    P.kernel = medoid_kernel(L, window, opt_general, no_short_dtw);
    P.general = P.kernel == MedoidKernel::kGeneral;
    P.chunks = (n + kMedoidChunk - 1) / kMedoidChunk;
    P.rows_padded = P.chunks * kMedoidChunk;
    P.n_diag = P.chunks, P.n_off = P.chunks * (P.chunks - 1) / 2;
    if (P.general && n > 0) {
        int64_t rows = kLooBlockBytes / (P.rows_padded * (int64_t)sizeof(float));
        rows -= rows % kMedoidChunk;
        if (rows > P.rows_padded) rows = P.rows_padded;
        P.block_rows = rows, P.block_bytes = rows * P.rows_padded * (int64_t)sizeof(float);
        for (int64_t r0 = 0; r0 < P.rows_padded; r0 += rows)
            P.blocks.push_back(LooBlock{r0, P.rows_padded - r0 < rows ? P.rows_padded - r0 : rows});
    }
    int64_t at = 0;
    auto piece = [&at](int64_t bytes) {
        const int64_t o = at;
        at += medoid_align(bytes);
        return o;
    };
    P.off_member = piece(P.rows_padded);
    P.off_label = piece(P.rows_padded * (int64_t)sizeof(int32_t));
    P.off_keys = piece(P.rows_padded * 2 * (int64_t)sizeof(uint64_t));
    P.off_dense = piece(P.rows_padded * L * (int64_t)sizeof(double));
    P.off_padded = piece(P.rows_padded * P.Lpad * (int64_t)sizeof(double));
    P.off_block = piece(P.block_bytes);
    P.workspace_bytes = at;
    const int64_t max_rows = n + (kMedoidChunk - 1);
    P.workspace_bound = max_rows * ((L + P.Lpad) * (int64_t)sizeof(double) + 21) + (P.general ? kLooBlockBytes : 0) + 6 * 256;
    return P;
}

}  // namespace wdx
