// The device trainer of DTW_MLP (include/wdx.h: wdx_mlp_fit_device states the rule): what a fit does with its sizes, before anything is
// launched -- the one statement of it (plain C++17: no device runtime, nothing of the context, so the system compiler builds it alone:
// tests/host/mlp_fit_plan_check.cpp).  wdx_mlp_fit.hip launches what the plan names.
//
//   layers     weight matrix l maps sizes[l] -> sizes[l + 1] units, l = 0 .. n_layers - 1; sizes[n_layers] = n_out = the class count,
//              or 1 (one logistic unit) for two classes
//   batch      the effective batch is min(batch_size, m); an epoch takes steps = ceil(m / batch) minibatches, the last one short
//   step       2 n_layers launches on the caller's stream, in this order:
//                forward      ceil(nb / 16) workgroups of 256 threads: every layer for 16 batch rows, activations, output delta, loss
//                then for l = n_layers - 1 .. 0:
//                  delta l    (l >= 1 only) ceil(nb / 16) workgroups of 256: delta_l = (delta_{l+1} W_l^T) o act'(A_l) -- BEFORE W_l changes
//                  adam l     one WAVE per 16 x 16 tile of W_l, four waves per workgroup: gradient, moments, update; the tiles of the
//                             first tile row also own their 16 intercepts
//   slots      one float64 per forward workgroup and step (cross-entropy of its rows), one per W tile and step (its sum of squares
//              before the update): the host reads both once per epoch and adds them in slot order.  No atomics anywhere.
//
// WORKSPACE (context-owned, grow-only; 256 B of alignment per piece; MlpFitPlan::bytes <= bytes_bound, checked by the host program):
//   scaled input (m, F) f32 | per layer: W, b, and two moments of each, f32 | activations A_1 .. A_{n_layers-1} and deltas
//   delta_1 .. delta_{n_layers}, each (batch rounded up to 16, width) f32 | loss slots, L2 slots f64 | index list m int32 | flags 2 int32 | the scaler's mean and scale, F float64 each
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/wdx.h"

namespace wdx {

constexpr int kMlpFitRows = 16;            // batch rows per forward / delta workgroup
constexpr int kMlpFitThreads = 256;        // four waves
constexpr int kMlpFitWavesPerGroup = 4;    // adam: W tiles per workgroup
constexpr int64_t kMlpFitMaxBatch = WDX_MLP_FIT_MAX_BATCH;
constexpr int kMlpFitMaxPieces = 6 * WDX_MLP_MAX_LAYERS + 2 * WDX_MLP_MAX_LAYERS + 7;

inline int64_t mlp_fit_align(int64_t b) { return (b + 255) / 256 * 256; }
inline int64_t mlp_fit_tiles(int64_t v) { return (v + 15) / 16; }

struct MlpFitPiece { int64_t off, bytes; };

struct MlpFitPlan {
    int rc = WDX_SUCCESS;
    char msg[224] = {0};
    int64_t m = 0, ld = 0;
    int nl = 0, act = 0, k = 0, n_out = 0;
    int sizes[WDX_MLP_MAX_LAYERS + 1] = {0};
    int64_t batch = 0, batch_pad = 0, steps = 0, last_batch = 0;
    int64_t fwd_tiles = 0;                          // forward workgroups of a full batch = loss slots per step
    int w_tiles_i[WDX_MLP_MAX_LAYERS] = {0};        // tile rows (fan-in) and columns (fan-out) of W_l
    int w_tiles_j[WDX_MLP_MAX_LAYERS] = {0};
    int64_t w_tile0[WDX_MLP_MAX_LAYERS] = {0};      // first L2 slot of layer l within a step
    int64_t w_tiles = 0;                            // L2 slots per step
    int64_t loss_slots = 0, l2_slots = 0;
    int lds_ld = 0;                                 // row stride of the forward kernel's two LDS buffers (floats)
    int64_t lds_bytes = 0;
    // workspace pieces (byte offsets)
    int64_t off_xs = 0, off_w[WDX_MLP_MAX_LAYERS] = {0}, off_b[WDX_MLP_MAX_LAYERS] = {0};
    int64_t off_mw[WDX_MLP_MAX_LAYERS] = {0}, off_vw[WDX_MLP_MAX_LAYERS] = {0}, off_mb[WDX_MLP_MAX_LAYERS] = {0}, off_vb[WDX_MLP_MAX_LAYERS] = {0};
    int64_t off_act[WDX_MLP_MAX_LAYERS + 1] = {0};     // A_l, l = 1 .. nl - 1
    int64_t off_delta[WDX_MLP_MAX_LAYERS + 1] = {0};   // delta_l, l = 1 .. nl
    int64_t off_loss = 0, off_l2 = 0, off_idx = 0, off_flags = 0, off_mean = 0, off_scale = 0;
    int64_t bytes = 0, bytes_bound = 0;
    int n_pieces = 0;
    MlpFitPiece pieces[kMlpFitMaxPieces] = {};

    int64_t rows_of_step(int64_t s) const { return s + 1 < steps ? batch : last_batch; }
    int64_t fwd_grid(int64_t nb) const { return mlp_fit_tiles(nb); }
    int64_t delta_grid(int64_t nb) const { return mlp_fit_tiles(nb); }
    int64_t adam_grid(int l) const { return ((int64_t)w_tiles_i[l] * w_tiles_j[l] + kMlpFitWavesPerGroup - 1) / kMlpFitWavesPerGroup; }
    int launches_per_step() const { return 2 * nl; }
};

// p: the caller's parameters; the have_* flags: that pointer argument is there
inline MlpFitPlan mlp_fit_plan(int64_t m, int64_t ld, const wdx_mlp_fit_params *p, bool have_dist, bool have_y, bool have_weights, bool have_out) {
    MlpFitPlan P;
#define WDX_MLP_FIT_REFUSE(code, ...)                  \
    do {                                               \
        snprintf(P.msg, sizeof P.msg, __VA_ARGS__);    \
        P.rc = (code);                                 \
        return P;                                      \
    } while (0)
    if (!p) WDX_MLP_FIT_REFUSE(WDX_ERR_INVALID, "mlp fit: the parameters are required (NULL given)");
    if (m < 1) WDX_MLP_FIT_REFUSE(WDX_ERR_INVALID, "mlp fit: m must be at least 1, not %lld", (long long)m);
    if (p->n_layers < 2) WDX_MLP_FIT_REFUSE(WDX_ERR_INVALID, "mlp fit: n_layers = %d, at least one hidden layer is required", p->n_layers);
    if (p->n_layers > WDX_MLP_MAX_LAYERS)
        WDX_MLP_FIT_REFUSE(WDX_ERR_UNSUPPORTED, "mlp fit: n_layers = %d, more than WDX_MLP_MAX_LAYERS = %d", p->n_layers, WDX_MLP_MAX_LAYERS);
    if (p->hidden_activation < WDX_MLP_ACT_IDENTITY || p->hidden_activation > WDX_MLP_ACT_RELU)
        WDX_MLP_FIT_REFUSE(WDX_ERR_INVALID, "mlp fit: unknown hidden activation %d", p->hidden_activation);
    if (p->n_classes < 2) WDX_MLP_FIT_REFUSE(WDX_ERR_INVALID, "mlp fit: n_classes = %d, at least two are required", p->n_classes);
    if (p->n_classes > 16) WDX_MLP_FIT_REFUSE(WDX_ERR_UNSUPPORTED, "mlp fit: n_classes = %d, more than 16", p->n_classes);
    const int nl = p->n_layers;
    for (int l = 0; l <= nl; ++l)
        if (p->sizes[l] < 1) WDX_MLP_FIT_REFUSE(WDX_ERR_INVALID, "mlp fit: sizes[%d] = %d must be at least 1", l, p->sizes[l]);
    for (int l = 1; l < nl; ++l)
        if (p->sizes[l] > WDX_MLP_MAX_WIDTH)
            WDX_MLP_FIT_REFUSE(WDX_ERR_UNSUPPORTED, "mlp fit: hidden layer %d has %d units, more than WDX_MLP_MAX_WIDTH = %d", l, p->sizes[l], WDX_MLP_MAX_WIDTH);
    const int n_out = p->n_classes == 2 ? 1 : p->n_classes;
    if (p->sizes[nl] != n_out)
        WDX_MLP_FIT_REFUSE(WDX_ERR_INVALID, "mlp fit: the output layer has %d units, %d classes need %d", p->sizes[nl], p->n_classes, n_out);
    if (ld < p->sizes[0]) WDX_MLP_FIT_REFUSE(WDX_ERR_INVALID, "mlp fit: ld = %lld is less than the %d input columns", (long long)ld, p->sizes[0]);
    if (p->batch_size < 1) WDX_MLP_FIT_REFUSE(WDX_ERR_INVALID, "mlp fit: batch_size = %d must be at least 1", p->batch_size);
    if (p->batch_size > kMlpFitMaxBatch)
        WDX_MLP_FIT_REFUSE(WDX_ERR_UNSUPPORTED, "mlp fit: batch_size = %d, more than WDX_MLP_FIT_MAX_BATCH = %lld", p->batch_size, (long long)kMlpFitMaxBatch);
    if (p->max_epochs < 1) WDX_MLP_FIT_REFUSE(WDX_ERR_INVALID, "mlp fit: max_epochs = %d must be at least 1", p->max_epochs);
    if (p->n_iter_no_change < 0) WDX_MLP_FIT_REFUSE(WDX_ERR_INVALID, "mlp fit: n_iter_no_change = %d must not be negative", p->n_iter_no_change);
    if (!(p->lr > 0) || !isfinite(p->lr)) WDX_MLP_FIT_REFUSE(WDX_ERR_INVALID, "mlp fit: lr must be positive and finite, not %g", p->lr);
    if (!(p->alpha >= 0) || !isfinite(p->alpha)) WDX_MLP_FIT_REFUSE(WDX_ERR_INVALID, "mlp fit: alpha must be finite and not negative, not %g", p->alpha);
    if (!(p->beta1 >= 0 && p->beta1 < 1) || !(p->beta2 >= 0 && p->beta2 < 1))
        WDX_MLP_FIT_REFUSE(WDX_ERR_INVALID, "mlp fit: beta1 = %g and beta2 = %g must lie in [0, 1)", p->beta1, p->beta2);
    if (!(p->epsilon > 0) || !isfinite(p->epsilon)) WDX_MLP_FIT_REFUSE(WDX_ERR_INVALID, "mlp fit: epsilon must be positive and finite, not %g", p->epsilon);
    if (!isfinite(p->tol)) WDX_MLP_FIT_REFUSE(WDX_ERR_INVALID, "mlp fit: tol must be finite, not %g", p->tol);
    if (m > INT32_MAX) WDX_MLP_FIT_REFUSE(WDX_ERR_UNSUPPORTED, "mlp fit: m = %lld rows, more than an int32 index list names", (long long)m);
    if (!have_dist) WDX_MLP_FIT_REFUSE(WDX_ERR_INVALID, "mlp fit: the distance matrix is required (NULL given)");
    if (!have_y) WDX_MLP_FIT_REFUSE(WDX_ERR_INVALID, "mlp fit: the class indices are required (NULL given)");
    if (!have_weights) WDX_MLP_FIT_REFUSE(WDX_ERR_INVALID, "mlp fit: every layer's coefs and intercepts are required (NULL given)");
    if (!have_out) WDX_MLP_FIT_REFUSE(WDX_ERR_INVALID, "mlp fit: loss_curve, n_epochs and state are required (NULL given)");

    P.m = m, P.ld = ld, P.nl = nl, P.act = p->hidden_activation, P.k = p->n_classes, P.n_out = n_out;
    for (int l = 0; l <= nl; ++l) P.sizes[l] = p->sizes[l];
    P.batch = p->batch_size < m ? p->batch_size : m;
    P.batch_pad = mlp_fit_tiles(P.batch) * 16;
    P.steps = (m + P.batch - 1) / P.batch;
    P.last_batch = m - (P.steps - 1) * P.batch;
    P.fwd_tiles = mlp_fit_tiles(P.batch);
    for (int l = 0; l < nl; ++l) {
        P.w_tiles_i[l] = (int)mlp_fit_tiles(P.sizes[l]);
        P.w_tiles_j[l] = (int)mlp_fit_tiles(P.sizes[l + 1]);
        P.w_tile0[l] = P.w_tiles;
        P.w_tiles += (int64_t)P.w_tiles_i[l] * P.w_tiles_j[l];
    }
    P.loss_slots = P.steps * P.fwd_tiles;
    P.l2_slots = P.steps * P.w_tiles;
    if (P.loss_slots > INT32_MAX || P.l2_slots > INT32_MAX) {
        const long long slots = (long long)(P.loss_slots > P.l2_slots ? P.loss_slots : P.l2_slots);
        P = MlpFitPlan();
        WDX_MLP_FIT_REFUSE(WDX_ERR_UNSUPPORTED, "mlp fit: m = %lld rows at this batch size need %lld loss slots per epoch, more than an int32 index names",
                           (long long)m, slots);
    }
    int widest = 16;
    for (int l = 1; l <= nl; ++l) widest = P.sizes[l] > widest ? P.sizes[l] : widest;
    P.lds_ld = (widest + 15) / 16 * 16 + 1;   // (+1: the 16 rows of a column fall into different banks)
    P.lds_bytes = (int64_t)sizeof(float) * 2 * kMlpFitRows * P.lds_ld;

    int64_t at = 0, raw = 0;
    auto piece = [&](int64_t bytes) {
        const int64_t o = at;
        P.pieces[P.n_pieces++] = MlpFitPiece{o, bytes};
        at += mlp_fit_align(bytes);
        raw += bytes;
        return o;
    };
    P.off_xs = piece(m * (int64_t)P.sizes[0] * 4);
    for (int l = 0; l < nl; ++l) {
        const int64_t wb = (int64_t)P.sizes[l] * P.sizes[l + 1] * 4, bb = (int64_t)P.sizes[l + 1] * 4;
        P.off_w[l] = piece(wb), P.off_mw[l] = piece(wb), P.off_vw[l] = piece(wb);
        P.off_b[l] = piece(bb), P.off_mb[l] = piece(bb), P.off_vb[l] = piece(bb);
    }
    for (int l = 1; l < nl; ++l) P.off_act[l] = piece(P.batch_pad * P.sizes[l] * 4);
    for (int l = 1; l <= nl; ++l) P.off_delta[l] = piece(P.batch_pad * P.sizes[l] * 4);
    P.off_loss = piece(P.loss_slots * 8);
    P.off_l2 = piece(P.l2_slots * 8);
    P.off_idx = piece(m * 4);
    P.off_flags = piece(2 * 4);
    P.off_mean = piece((int64_t)P.sizes[0] * 8);
    P.off_scale = piece((int64_t)P.sizes[0] * 8);
    P.bytes = at;
    P.bytes_bound = raw + 256 * (int64_t)P.n_pieces;
#undef WDX_MLP_FIT_REFUSE
    return P;
}

}  // namespace wdx
