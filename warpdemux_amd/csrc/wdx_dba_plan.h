// One barycenter step (include/wdx.h: wdx_dba_step_device): what a call does with its HOST label array, before anything is launched
// -- the one statement of it (plain C++17: no device runtime, nothing of the context, so the system compiler builds it alone:
// tests/host/dba_plan_check.cpp).  wdx_dba.hip uploads the tables the plan holds and launches what it names.
//
//   order      the padded row order of wdx_medoid_plan.h (its records and its layout): label after label, rising row order inside a
//              label, every label starting on a multiple of 64 rows.  One LANE aligns one padded row; a wave is one chunk of 64 rows
//              and so belongs to one label (chunk_label[chunk]).  A label may hold any number of rows: a step has no block that grows
//              with the square of a label, so the medoids' WDX_MEDOID_MAX_GROUP does not apply.
//   words      64-bit words of 2-bit direction codes per (row of the series, lane): the cells of row i inside the band are numbered
//              from the first one, k = j - max(0, i - (w - 1)), at most min(2w - 1, L) of them: ceil(2 min(2w - 1, L) / 64) words.
//   codes      word h of row i of lane l of a pass at [(i * words + h) * pass_rows + l]: the lanes contiguous
//   passes     consecutive chunks whose codes share the code block: at most kDbaCodeBytes, at least one wave.  A pass is one launch
//              of the align kernel.
//   partial    per chunk of the CALL: S[chunk][j] float64, K[chunk][j] int64, cost[chunk] float64, members[chunk] int64 -- written
//              once each by the chunk's wave; the reduce kernel adds them in rising chunk order after the last pass.
//
// WORKSPACE BOUND (context-owned, grow-only; DbaPlan::workspace_bytes <= workspace_bound, checked by the host program):
//   codes          <= kDbaCodeBytes = 256 MiB (64 rows at the limits L = 1024, unbanded, take 16 MiB)
//   runs           pass_rows x L x 4 B (lo | hi << 16 per column): at most half the codes
//   rolling rows   general route only: 2 x (L + 1) x pass_rows x 8 B
//   gathered rows  rows_padded x L x 8 B (the pre-pass of the medoids without its zero-haloed form: the lanes read the dense one)
//   centres        n_labels x Lpad x 8 B with the zero halo, 1 B per label of "every sample finite"
//   partial        chunks x (2 L + 2) x 8 B
//   tables         4 B per padded row, 4 B per chunk, 48 B per label
//   plus 256 B of alignment per piece.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/wdx.h"
#include "wdx_medoid_plan.h"

namespace wdx {

constexpr int64_t kDbaMaxL = WDX_DBA_MAX_L;
constexpr int64_t kDbaCodeBytes = 256ll << 20;
constexpr int kDbaSlab = 32;   // columns per hand-over through LDS

enum class DbaKernel { kGeneral, kBand8, kBand15, kBand16, kBand32 };
// the band ladder of the DTW dispatch (8, 15 exact, 16, 32); beyond it, and with WDX_OPT_DBA_GENERAL, the rolling rows
inline DbaKernel dba_kernel(int64_t L, int64_t window, bool opt_general) {
    const int64_t w = dtw_effective_window(L, window);
    if (opt_general || w > kMaxRegWindow) return DbaKernel::kGeneral;
    return w == 15 ? DbaKernel::kBand15 : (w <= 8 ? DbaKernel::kBand8 : (w <= 16 ? DbaKernel::kBand16 : DbaKernel::kBand32));
}
inline int64_t dba_band_cells(int64_t L, int64_t w) { return 2 * w - 1 < L ? 2 * w - 1 : L; }
inline int64_t dba_code_words(int64_t L, int64_t w) { return (2 * dba_band_cells(L, w) + 63) / 64; }

struct DbaPass { int64_t row0, rows; };   // padded rows [row0, row0 + rows), both multiples of 64

struct DbaPlan {
    int rc = WDX_SUCCESS;
    char msg[192] = {0};
    int64_t n = 0, n_labels = 0, L = 0, Lpad = 0, w = 0;
    DbaKernel kernel = DbaKernel::kGeneral;
    int64_t words = 0;
    int64_t rows_padded = 0, chunks = 0;
    int64_t pass_rows = 0;               // rows of a full pass (the code block is laid out for it)
    std::vector<int32_t> order;          // [rows_padded]: the caller's row at padded row p, -1 for padding
    std::vector<MedoidLabel> labels;     // [n_labels + 1]: row0, size, chunks (the device reads these records as they are)
    std::vector<int32_t> chunk_label;    // [chunks]
    std::vector<DbaPass> passes;
    int64_t off_order = 0, off_chunk_label = 0, off_labels = 0, off_member = 0, off_dense = 0, off_centres = 0,
            off_centre_ok = 0, off_codes = 0, off_runs = 0, off_rolling = 0, off_partial = 0;
    int64_t table_bytes = 0, code_bytes = 0, workspace_bytes = 0, workspace_bound = 0;
    // the partial block: float64 / int64 indices
    int64_t part_S(int64_t chunk, int64_t j) const { return chunk * L + j; }
    int64_t part_K(int64_t chunk, int64_t j) const { return chunks * L + chunk * L + j; }
    int64_t part_cost(int64_t chunk) const { return 2 * chunks * L + chunk; }
    int64_t part_members(int64_t chunk) const { return 2 * chunks * L + chunks + chunk; }
};

// The refusals of a call, alone (the host form asks before it sizes anything by the arguments): WDX_SUCCESS, or the code with the
// message in msg[192].  label: HOST int32[n] (may be null when n == 0); have_new / have_centres: the required pointers are there
inline int dba_refusal(const int32_t *label, int64_t n, int64_t n_labels, int64_t L, bool have_new, bool have_centres, char *msg) {
    constexpr size_t kMsg = 192;
    if (n_labels < 1 || n_labels > INT32_MAX) {
        snprintf(msg, kMsg, "dba: n_labels must be at least 1, not %lld", (long long)n_labels);
        return WDX_ERR_INVALID;
    }
    if (L < 1) {
        snprintf(msg, kMsg, "dba: L must be at least 1, not %lld", (long long)L);
        return WDX_ERR_INVALID;
    }
    if (n < 0 || n > INT32_MAX || (n > 0 && !label)) {
        snprintf(msg, kMsg, "dba: need 0 <= n <= 2^31 - 1 rows and their labels (n = %lld)", (long long)n);
        return WDX_ERR_INVALID;
    }
    if (!have_new || !have_centres) {
        snprintf(msg, kMsg, "dba: the centres and the new centres are required (NULL given)");
        return WDX_ERR_INVALID;
    }
    for (int64_t r = 0; r < n; ++r)
        if (label[r] < -1 || label[r] >= n_labels) {
            snprintf(msg, kMsg, "dba: the label of row %lld is %d, outside -1 .. %lld", (long long)r, (int)label[r], (long long)n_labels - 1);
            return WDX_ERR_INVALID;
        }
    if (L > kDbaMaxL) {
        snprintf(msg, kMsg, "dba: L = %lld is more than WDX_DBA_MAX_L = %lld", (long long)L, (long long)kDbaMaxL);
        return WDX_ERR_UNSUPPORTED;
    }
    return WDX_SUCCESS;
}

inline DbaPlan dba_plan(const int32_t *label, int64_t n, int64_t n_labels, int64_t L, int64_t window, bool have_new, bool have_centres,
                        bool opt_general) {
    DbaPlan P;
    if ((P.rc = dba_refusal(label, n, n_labels, L, have_new, have_centres, P.msg)) != WDX_SUCCESS) return P;
    // the padded order: the medoids' records (tile and partial fields unused) and layout
    P.labels.assign((size_t)n_labels + 1, MedoidLabel{0, 0, 0, 0, 0, 0, 0, 0});
    for (int64_t r = 0; r < n; ++r)
        if (label[r] >= 0) ++P.labels[(size_t)label[r]].size;
    int64_t row = 0;
    for (int64_t g = 0; g <= n_labels; ++g) {
        MedoidLabel &Lb = P.labels[(size_t)g];
        Lb.row0 = row, Lb.chunks = (int32_t)((Lb.size + kMedoidChunk - 1) / kMedoidChunk);
        row += kMedoidChunk * (int64_t)Lb.chunks;
    }
    P.rows_padded = row, P.chunks = row / kMedoidChunk;
    P.order.assign((size_t)P.rows_padded, -1);
    {
        std::vector<int64_t> next((size_t)n_labels);
        for (int64_t g = 0; g < n_labels; ++g) next[(size_t)g] = P.labels[(size_t)g].row0;
        for (int64_t r = 0; r < n; ++r)
            if (label[r] >= 0) P.order[(size_t)next[(size_t)label[r]]++] = (int32_t)r;
    }
    P.n = n, P.n_labels = n_labels, P.L = L, P.Lpad = dtw_padded_length(L), P.w = dtw_effective_window(L, window);
    P.kernel = dba_kernel(L, window, opt_general);
    P.words = dba_code_words(L, P.w);
    P.chunk_label.assign((size_t)P.chunks, -1);
    for (int64_t g = 0; g < n_labels; ++g) {
        const MedoidLabel &Lb = P.labels[(size_t)g];
        for (int64_t c = 0; c < Lb.chunks; ++c) P.chunk_label[(size_t)(Lb.row0 / kMedoidChunk + c)] = (int32_t)g;
    }
    // passes: as many waves as the code block holds, at least one
    const int64_t row_bytes = L * P.words * (int64_t)sizeof(uint64_t);
    int64_t rows = kDbaCodeBytes / row_bytes;
    rows -= rows % kMedoidChunk;
    if (rows < kMedoidChunk) rows = kMedoidChunk;
    if (rows > P.rows_padded) rows = P.rows_padded;
    P.pass_rows = rows;
    for (int64_t r0 = 0; r0 < P.rows_padded; r0 += rows)
        P.passes.push_back(DbaPass{r0, r0 + rows <= P.rows_padded ? rows : P.rows_padded - r0});
    P.code_bytes = rows * row_bytes;
    // the workspace
    int64_t at = 0;
    auto piece = [&at](int64_t bytes) {
        const int64_t o = at;
        at += medoid_align(bytes);
        return o;
    };
    const bool general = P.kernel == DbaKernel::kGeneral;
    P.off_order = piece(P.rows_padded * (int64_t)sizeof(int32_t));
    P.off_chunk_label = piece(P.chunks * (int64_t)sizeof(int32_t));
    P.off_labels = piece((n_labels + 1) * (int64_t)sizeof(MedoidLabel));
    P.table_bytes = at;
    P.off_member = piece(P.rows_padded);
    P.off_dense = piece(P.rows_padded * L * (int64_t)sizeof(double));
    P.off_centres = piece(n_labels * P.Lpad * (int64_t)sizeof(double));
    P.off_centre_ok = piece(n_labels);
    P.off_codes = piece(P.code_bytes);
    P.off_runs = piece(rows * L * (int64_t)sizeof(uint32_t));
    P.off_rolling = piece(general ? 2 * (L + 1) * rows * (int64_t)sizeof(double) : 0);
    P.off_partial = piece(P.chunks * (2 * L + 2) * (int64_t)sizeof(double));
    P.workspace_bytes = at;
    const int64_t max_rows = n + (kMedoidChunk - 1) * (n < n_labels ? n : n_labels);
    const int64_t max_pass = kDbaCodeBytes / row_bytes > kMedoidChunk ? kDbaCodeBytes / row_bytes : kMedoidChunk;
    P.workspace_bound = kDbaCodeBytes + kDbaCodeBytes / 2 + (general ? 2 * (L + 1) * max_pass * (int64_t)sizeof(double) : 0) +
                        max_rows * L * (int64_t)sizeof(double) + n_labels * (P.Lpad * (int64_t)sizeof(double) + 1) +
                        (max_rows / kMedoidChunk) * (2 * L + 2) * (int64_t)sizeof(double) + 5 * max_rows + max_rows / 16 +
                        (n_labels + 1) * (int64_t)sizeof(MedoidLabel) + 11 * 256;
    return P;
}

}  // namespace wdx
