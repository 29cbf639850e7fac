// Per-label DTW medoids (include/wdx.h: wdx_medoids_device): what a call does with its HOST label array, before anything is
// launched -- the one statement of it (plain C++17: no device runtime, nothing of the context, so the system compiler builds
// it alone: tests/host/medoid_plan_check.cpp).  wdx_medoid.hip uploads the tables the plan holds and launches what it names.
//
//   order      the rows of the call in a PADDED layout: label after label (stable: rising row order inside a label), every
//              label starting on a multiple of 64 rows; order[p] is the caller's row at padded row p, -1 for padding.  Rows
//              labelled -1 are not in it.
//   labels     one record per label (and a sentinel): its padded rows, its chunks of 64 rows, where its tiles start in the
//              call's two tile lists and where its partial sums start in the partial block of its pass
//   tiles      64 x 64 tiles (label, I, J), J >= I, of the label's chunk x chunk matrix: the diagonal ones (I == J) and the
//              strictly upper ones in two lists (two kernels: they differ in LDS).  Every unordered pair of rows of one label
//              lies in exactly one tile.  The kernels decode a tile's number with the functions below; no list is uploaded.
//   partial    partial[chunk c][row r] of one label, a float64 at part0 + c * (64 * chunks) + r: the sum S_c of the rule for
//              row r (r counted in the label's padded rows).  Written exactly once per (c, r): by tile (min, max) of r's chunk
//              k and c -- its row part when c > k, its column part when c < k, the diagonal tile when c == k.
//   passes     consecutive labels whose partial sums share the block at once; a pass is one launch of each tile kernel and one
//              of the reduce kernel.  A pass holds at most kMedoidPartialBytes of partial sums.
//
// WORKSPACE BOUND (context-owned, grow-only; MedoidPlan::workspace_bytes, checked by the host program):
//   partial sums   <= kMedoidPartialBytes = 512 chunks x 32 768 rows x 8 B = 128 MiB (one label at the cap fills it)
//   gathered rows  rows_padded x (L + Lpad) x 8 B: each row once dense (the lanes' operand) and once with the zero halo (the
//                  uniform operand), rows_padded <= n + 63 x min(n, n_labels)
//   tables         4 B per padded row, 1 B per padded row of member flags, 48 B per label
//   general route  + one block of the label's float32 matrix, <= kMedoidMatrixBytes (64 MiB) or 64 rows of the largest label
//   plus 256 B of alignment per piece.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/wdx.h"
#include "wdx_dtw_plan.h"

#if defined(__HIPCC__)
#define WDX_MEDOID_HD __host__ __device__
#else
#define WDX_MEDOID_HD
#endif

namespace wdx {

constexpr int64_t kMedoidChunk = 64;
constexpr int64_t kMedoidMaxGroup = WDX_MEDOID_MAX_GROUP;
constexpr int64_t kMedoidPartialBytes = (kMedoidMaxGroup / kMedoidChunk) * kMedoidMaxGroup * (int64_t)sizeof(double);
constexpr int64_t kMedoidMatrixBytes = 64ll << 20;
static_assert(kMedoidMaxGroup % kMedoidChunk == 0 && kMedoidPartialBytes == (128ll << 20), "the stated bound");

struct MedoidLabel {   // (the device reads these records as they are)
    int64_t row0;      // first padded row, a multiple of 64
    int64_t diag0;     // number of the label's first diagonal tile in the call
    int64_t off0;      // ... and of its first strictly upper tile
    int64_t part0;     // first float64 of its partial sums in the block of its pass
    int32_t size;      // rows of the label (members or not)
    int32_t chunks;    // ceil(size / 64)
    int32_t pass;
    int32_t reserved;
};
static_assert(sizeof(MedoidLabel) == 48, "MedoidLabel is uploaded as it is");

struct MedoidPass {
    int32_t g0, g1;                 // labels [g0, g1)
    int64_t diag0, diag1;           // diagonal tiles [diag0, diag1)
    int64_t off0, off1;             // strictly upper tiles [off0, off1)
    int64_t partial_doubles;        // of the pass
};
struct MedoidTile { int32_t label, I, J; };

// number of strictly upper tiles in front of row I of a c x c chunk matrix
WDX_MEDOID_HD inline int64_t medoid_upper_row_start(int64_t c, int64_t I) { return I * (c - 1) - I * (I - 1) / 2; }
// strictly upper tile t (0 <= t < c (c - 1) / 2) of a c x c chunk matrix, row by row: (I, J), J > I
WDX_MEDOID_HD inline void medoid_upper_tile(int64_t c, int64_t t, int32_t *I, int32_t *J) {
    // row I starts at s(I) = I (c - 1) - I (I - 1) / 2; largest I with s(I) <= t.  A bisection on exact integers: 10 steps at the cap.
    int64_t lo = 0, hi = c - 2;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) / 2;
        if (medoid_upper_row_start(c, mid) <= t) lo = mid;
        else hi = mid - 1;
    }
    *I = (int32_t)lo;
    *J = (int32_t)(lo + 1 + (t - medoid_upper_row_start(c, lo)));
}
// the label of tile `t` of a list (diag: the diagonal tiles, else the strictly upper ones): the last g in [g0, g1) whose first
// tile of that list is <= t
WDX_MEDOID_HD inline int32_t medoid_tile_label(const MedoidLabel *labels, bool diag, int32_t g0, int32_t g1, int64_t t) {
    int32_t lo = g0, hi = g1 - 1;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if ((diag ? labels[mid].diag0 : labels[mid].off0) <= t) lo = mid;
        else hi = mid - 1;
    }
    return lo;   // (labels without tiles share their start with the next one: the LAST such g is the one that owns t)
}

struct MedoidPlan {
    int rc = WDX_SUCCESS;
    char msg[192] = {0};
    int64_t n = 0, n_labels = 0, L = 0, Lpad = 0;
    bool general = false;
    int64_t rows_padded = 0;
    int64_t max_size = 0;                // rows of the largest label
    std::vector<int32_t> order;          // [rows_padded]
    std::vector<MedoidLabel> labels;     // [n_labels + 1]
    std::vector<MedoidPass> passes;
    int64_t n_diag = 0, n_off = 0;
    // general route: rows of the label's matrix per dispatch (a multiple of 64), its bytes
    int64_t block_rows = 0, matrix_bytes = 0;
    // the context-owned workspace: byte offsets of its pieces, and its size
    int64_t off_order = 0, off_labels = 0, off_member = 0, off_dense = 0, off_padded = 0, off_partial = 0, off_matrix = 0;
    int64_t partial_bytes = 0, workspace_bytes = 0, workspace_bound = 0;
    int64_t table_bytes = 0;             // what is uploaded: order, then labels (off_order == 0, contiguous up to off_member)

    int64_t tile_count() const { return n_diag + n_off; }
    // tile k of the call: the diagonal ones first
    MedoidTile tile(int64_t k) const {
        const bool diag = k < n_diag;
        const int64_t t = diag ? k : k - n_diag;
        const int32_t g = medoid_tile_label(labels.data(), diag, 0, (int32_t)n_labels, t);
        MedoidTile T{g, 0, 0};
        if (diag) T.I = T.J = (int32_t)(t - labels[g].diag0);
        else medoid_upper_tile(labels[g].chunks, t - labels[g].off0, &T.I, &T.J);
        return T;
    }
    // where S_c of padded row r of label g lives: a float64 index into the partial block of the label's pass
    int64_t partial_index(int32_t g, int64_t c, int64_t r) const { return labels[g].part0 + c * (kMedoidChunk * labels[g].chunks) + r; }
};

inline int64_t medoid_align(int64_t b) { return (b + 255) / 256 * 256; }

// label: HOST int32[n] (may be null when n == 0); have_medoid: the required output is there; general: WDX_OPT_MEDOID_GENERAL or a
// shape the tile kernels do not serve (the matrix block is then part of the workspace)
inline MedoidPlan medoid_plan(const int32_t *label, int64_t n, int64_t n_labels, int64_t L, bool have_medoid, bool general) {
    MedoidPlan P;
    auto refuse = [&P](int rc) -> MedoidPlan & {
        P.rc = rc;
        return P;
    };
    if (n_labels < 1 || n_labels > INT32_MAX) {
        snprintf(P.msg, sizeof P.msg, "medoids: n_labels must be at least 1, not %lld", (long long)n_labels);
        return refuse(WDX_ERR_INVALID);
    }
    if (L < 1) {
        snprintf(P.msg, sizeof P.msg, "medoids: L must be at least 1, not %lld", (long long)L);
        return refuse(WDX_ERR_INVALID);
    }
    if (n < 0 || n > INT32_MAX || (n > 0 && !label)) {
        snprintf(P.msg, sizeof P.msg, "medoids: need 0 <= n <= 2^31 - 1 rows and their labels (n = %lld)", (long long)n);
        return refuse(WDX_ERR_INVALID);
    }
    if (!have_medoid) {
        snprintf(P.msg, sizeof P.msg, "medoids: the medoid output is required (NULL given)");
        return refuse(WDX_ERR_INVALID);
    }
    P.n = n, P.n_labels = n_labels, P.L = L, P.Lpad = dtw_padded_length(L), P.general = general;
    std::vector<int64_t> size((size_t)n_labels, 0);
    for (int64_t r = 0; r < n; ++r) {
        const int32_t g = label[r];
        if (g < -1 || g >= n_labels) {
            snprintf(P.msg, sizeof P.msg, "medoids: the label of row %lld is %d, outside -1 .. %lld", (long long)r, (int)g,
                     (long long)n_labels - 1);
            return refuse(WDX_ERR_INVALID);
        }
        if (g >= 0) ++size[(size_t)g];
    }
    for (int64_t g = 0; g < n_labels; ++g)
        if (size[(size_t)g] > kMedoidMaxGroup) {
            snprintf(P.msg, sizeof P.msg, "medoids: label %lld has %lld rows, more than WDX_MEDOID_MAX_GROUP = %lld: subsample it",
                     (long long)g, (long long)size[(size_t)g], (long long)kMedoidMaxGroup);
            return refuse(WDX_ERR_UNSUPPORTED);
        }
    // labels, tiles and passes
    P.labels.resize((size_t)n_labels + 1);
    int64_t row = 0, part = 0;
    MedoidPass pass{0, 0, 0, 0, 0, 0, 0};
    for (int64_t g = 0; g <= n_labels; ++g) {
        MedoidLabel &Lb = P.labels[(size_t)g];
        const int64_t m = g < n_labels ? size[(size_t)g] : 0, c = (m + kMedoidChunk - 1) / kMedoidChunk;
        const int64_t doubles = c * c * kMedoidChunk;
        if (g == n_labels || (part + doubles) * (int64_t)sizeof(double) > kMedoidPartialBytes) {   // the pass is full (or the end)
            pass.g1 = (int32_t)g, pass.diag1 = P.n_diag, pass.off1 = P.n_off, pass.partial_doubles = part;
            if (pass.g1 > pass.g0) P.passes.push_back(pass);
            if (part * (int64_t)sizeof(double) > P.partial_bytes) P.partial_bytes = part * (int64_t)sizeof(double);
            pass = MedoidPass{(int32_t)g, (int32_t)g, P.n_diag, P.n_diag, P.n_off, P.n_off, 0};
            part = 0;
        }
        Lb = MedoidLabel{row, P.n_diag, P.n_off, part, (int32_t)m, (int32_t)c, (int32_t)P.passes.size(), 0};
        row += c * kMedoidChunk, part += doubles;
        P.n_diag += c, P.n_off += c * (c - 1) / 2;
        if (m > P.max_size) P.max_size = m;
    }
    P.rows_padded = row;
    // the stable order
    P.order.assign((size_t)P.rows_padded, -1);
    {
        std::vector<int64_t> next((size_t)n_labels);
        for (int64_t g = 0; g < n_labels; ++g) next[(size_t)g] = P.labels[(size_t)g].row0;
        for (int64_t r = 0; r < n; ++r)
            if (label[r] >= 0) P.order[(size_t)next[(size_t)label[r]]++] = (int32_t)r;
    }
    // the general route's matrix block: block_rows x (the label's padded rows) float32
    if (general && P.max_size > 0) {
        const int64_t cols = (P.max_size + kMedoidChunk - 1) / kMedoidChunk * kMedoidChunk;
        int64_t rows = kMedoidMatrixBytes / (cols * (int64_t)sizeof(float));
        rows -= rows % kMedoidChunk;
        if (rows < kMedoidChunk) rows = kMedoidChunk;
        if (rows > cols) rows = cols;
        P.block_rows = rows, P.matrix_bytes = rows * cols * (int64_t)sizeof(float);
    }
    // the workspace
    int64_t at = 0;
    auto piece = [&at](int64_t bytes) {
        const int64_t o = at;
        at += medoid_align(bytes);
        return o;
    };
    P.off_order = piece(P.rows_padded * (int64_t)sizeof(int32_t));
    P.off_labels = piece((n_labels + 1) * (int64_t)sizeof(MedoidLabel));
    P.table_bytes = at;
    P.off_member = piece(P.rows_padded);
    P.off_dense = piece(P.rows_padded * L * (int64_t)sizeof(double));
    P.off_padded = piece(P.rows_padded * P.Lpad * (int64_t)sizeof(double));
    P.off_partial = piece(P.partial_bytes);
    P.off_matrix = piece(P.matrix_bytes);
    P.workspace_bytes = at;
    const int64_t max_rows = n + (kMedoidChunk - 1) * (n < n_labels ? n : n_labels);
    const int64_t max_cols = (P.max_size + kMedoidChunk - 1) / kMedoidChunk * kMedoidChunk;
    const int64_t matrix_bound = kMedoidMatrixBytes > kMedoidChunk * max_cols * 4 ? kMedoidMatrixBytes : kMedoidChunk * max_cols * 4;
    P.workspace_bound = kMedoidPartialBytes + max_rows * (L + P.Lpad) * (int64_t)sizeof(double) + 5 * max_rows +
                        (n_labels + 1) * (int64_t)sizeof(MedoidLabel) + (general ? matrix_bound : 0) + 7 * 256;
    return P;
}

// Which route a call takes: the tile kernels serve effective windows up to kMaxRegWindow (the register-band ladder, and the
// unrolled 25-point / window-15 shape unless WDX_OPT_NO_SHORT_DTW); everything else, and every shape with WDX_OPT_MEDOID_GENERAL, goes
// block by block through dtw_plan / run_dtw_plan.
enum class MedoidKernel { kGeneral, kShort, kBand8, kBand15, kBand16, kBand32 };
inline MedoidKernel medoid_kernel(int64_t L, int64_t window, bool opt_general, bool no_short_dtw) {
    const int64_t w = dtw_effective_window(L, window);
    if (opt_general || w > kMaxRegWindow) return MedoidKernel::kGeneral;
    if (L == 25 && w == 15 && !no_short_dtw) return MedoidKernel::kShort;
    return w == 15 ? MedoidKernel::kBand15 : (w <= 8 ? MedoidKernel::kBand8 : (w <= 16 ? MedoidKernel::kBand16 : MedoidKernel::kBand32));
}

}  // namespace wdx
