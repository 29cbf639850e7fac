// The symmetric DTW self-distance matrix (include/wdx.h: wdx_self_matrix_device): what a call does with its sizes, before
// anything is launched -- the one statement of it (plain C++17: no device runtime, nothing of the context, so the system compiler
// builds it alone: tests/host/self_plan_check.cpp).  wdx_dtw_self.hip launches what the plan names.
//
//   rows       the n rows of the call in their own order, padded to rows_padded = 64 x chunks (padding rows are no members)
//   tiles      64 x 64 tiles (I, J), J >= I, of the chunk x chunk matrix: the diagonal ones (tile k is (k, k)) and the strictly
//              upper ones (decoded from the block number by medoid_upper_tile) in two lists -- two kernels, they differ in LDS.
//              Every unordered pair of rows lies in exactly one tile; a tile writes both of its images into the matrix.
//   blocks     general route (effective windows beyond the register band, and WDX_OPT_SELF_MATRIX_GENERAL): the rows in blocks of
//              kSelfBlockRows, each one dispatch of dtw_plan / run_dtw_plan straight into the matrix.  A last block of fewer
//              than 64 rows is joined to the one before, so that the rows of a block are always the lanes of its dispatch.
//
// WORKSPACE BOUND (context-owned, grow-only; SelfPlan::workspace_bytes, checked by the host program):
//   gathered rows  rows_padded x (L + Lpad) x 8 B: each row once dense (the lanes' operand) and once with the zero halo (the
//                  uniform operand), rows_padded <= n + 63
//   member flags   1 B per padded row
//   plus 256 B of alignment per piece.  The matrix itself is the caller's (the host form allocates it for the call).
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/wdx.h"
#include "wdx_medoid_plan.h"

namespace wdx {

constexpr int64_t kSelfMaxRows = WDX_SELF_MATRIX_MAX_ROWS;
constexpr int64_t kSelfBlockRows = 8192;   // (from kRowMajorMinReads on a dispatch reads the rows in place)
static_assert(kSelfMaxRows % kMedoidChunk == 0 && kSelfBlockRows % kMedoidChunk == 0 && kSelfBlockRows >= kRowMajorMinReads, "whole chunks");

struct SelfTile { int32_t I, J; };
struct SelfBlock { int64_t r0, rows; };

struct SelfPlan {
    int rc = WDX_SUCCESS;
    char msg[192] = {0};
    int64_t n = 0, L = 0, Lpad = 0, ld = 0;
    MedoidKernel kernel = MedoidKernel::kGeneral;
    bool general = false;
    int64_t chunks = 0, rows_padded = 0;
    int64_t n_diag = 0, n_off = 0;
    std::vector<SelfBlock> blocks;   // general route only
    // the context-owned workspace: byte offsets of its pieces, and its size
    int64_t off_member = 0, off_dense = 0, off_padded = 0;
    int64_t workspace_bytes = 0, workspace_bound = 0;

    int64_t tile_count() const { return n_diag + n_off; }
    // tile k of the call: the diagonal ones first
    SelfTile tile(int64_t k) const {
        SelfTile T{0, 0};
        if (k < n_diag) T.I = T.J = (int32_t)k;
        else medoid_upper_tile(chunks, k - n_diag, &T.I, &T.J);
        return T;
    }
};

// have_out: the matrix is there (it may be missing when n == 0); opt_general: WDX_OPT_SELF_MATRIX_GENERAL
inline SelfPlan self_plan(int64_t n, int64_t L, int64_t ld, int64_t window, bool have_out, bool opt_general, bool no_short_dtw) {
    SelfPlan P;
    auto refuse = [&P](int rc) -> SelfPlan & {
        P.rc = rc;
        return P;
    };
    if (L < 1) {
        snprintf(P.msg, sizeof P.msg, "self matrix: L must be at least 1, not %lld", (long long)L);
        return refuse(WDX_ERR_INVALID);
    }
    if (n < 0) {
        snprintf(P.msg, sizeof P.msg, "self matrix: n must not be negative (n = %lld)", (long long)n);
        return refuse(WDX_ERR_INVALID);
    }
    if (n > kSelfMaxRows) {
        snprintf(P.msg, sizeof P.msg, "self matrix: n = %lld rows, more than WDX_SELF_MATRIX_MAX_ROWS = %lld: subsample them", (long long)n,
                 (long long)kSelfMaxRows);
        return refuse(WDX_ERR_UNSUPPORTED);
    }
    if (ld < n) {
        snprintf(P.msg, sizeof P.msg, "self matrix: ld = %lld is less than n = %lld", (long long)ld, (long long)n);
        return refuse(WDX_ERR_INVALID);
    }
    if (n > 0 && !have_out) {
        snprintf(P.msg, sizeof P.msg, "self matrix: the output matrix is required (NULL given)");
        return refuse(WDX_ERR_INVALID);
    }
    P.n = n, P.L = L, P.Lpad = dtw_padded_length(L), P.ld = ld;
    P.kernel = medoid_kernel(L, window, opt_general, no_short_dtw);
    P.general = P.kernel == MedoidKernel::kGeneral;
    P.chunks = (n + kMedoidChunk - 1) / kMedoidChunk;
    P.rows_padded = P.chunks * kMedoidChunk;
    P.n_diag = P.chunks, P.n_off = P.chunks * (P.chunks - 1) / 2;
    if (P.general)
        for (int64_t r0 = 0; r0 < n;) {
            int64_t rows = n - r0 < kSelfBlockRows ? n - r0 : kSelfBlockRows;
            if (n - (r0 + rows) < kMedoidChunk) rows = n - r0;   // (a short tail joins this block)
            P.blocks.push_back(SelfBlock{r0, rows});
            r0 += rows;
        }
    int64_t at = 0;
    auto piece = [&at](int64_t bytes) {
        const int64_t o = at;
        at += medoid_align(bytes);
        return o;
    };
    P.off_member = piece(P.rows_padded);
    P.off_dense = piece(P.rows_padded * L * (int64_t)sizeof(double));
    P.off_padded = piece(P.rows_padded * P.Lpad * (int64_t)sizeof(double));
    P.workspace_bytes = at;
    const int64_t max_rows = n + (kMedoidChunk - 1);
    P.workspace_bound = max_rows * (L + P.Lpad) * (int64_t)sizeof(double) + max_rows + 3 * 256;
    return P;
}

}  // namespace wdx
