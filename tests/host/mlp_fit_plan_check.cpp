// What a device MLP fit does with its sizes (warpdemux_amd/csrc/wdx_mlp_fit_plan.h), checked without a GPU: built with the system
// compiler under the address and undefined-behaviour sanitizers and run by tests/test_mlp_fit_plan_host.py.
// Over layer shapes x batch sizes x row counts it checks of every plan:
//   1  the batch is min(batch_size, m), the steps cover the m rows exactly once in order, the last one holds the remainder
//   2  every workspace piece is 256-byte aligned, the pieces are disjoint and in rising order, each named offset is a piece of the
//      size its array needs, all lie inside bytes, and bytes within bytes_bound
//   3  grids: the forward and delta grids cover every batch row once and stay inside the padded batch; the adam grid of a layer covers
//      every 16 x 16 tile of W_l exactly once (a walk over workgroups x waves marks the tiles), every element of W_l lies in one tile
//   4  slots: every (step, forward workgroup) and every (step, layer, tile) has its own slot inside the slot arrays
//   5  the forward kernel's LDS holds two buffers of 16 rows of the widest layer and stays within 160 KiB
// and that each refusal carries its code and message.  Prints "checks <n>" / "failures <n>" and what the sweep met.
#include "wdx_mlp_fit_plan.h"

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

static long long g_plans = 0, g_short_last = 0, g_batch_clipped = 0, g_whole_tiles = 0, g_two_hidden = 0, g_one_unit = 0, g_refusals = 0, g_at_max_batch = 0;

static wdx_mlp_fit_params params(std::vector<int> sizes, int k, int batch) {
    wdx_mlp_fit_params p;
    memset(&p, 0, sizeof p);
    p.n_layers = (int)sizes.size() - 1, p.hidden_activation = WDX_MLP_ACT_RELU, p.n_classes = k, p.batch_size = batch;
    p.max_epochs = 5, p.n_iter_no_change = 10;
    for (size_t i = 0; i < sizes.size() && i < WDX_MLP_MAX_LAYERS + 1; ++i) p.sizes[i] = sizes[i];
    p.lr = 1e-3, p.alpha = 1e-4, p.beta1 = 0.9, p.beta2 = 0.999, p.epsilon = 1e-8, p.tol = 1e-4;
    return p;
}

static bool is_piece(const MlpFitPlan &P, int64_t off, int64_t bytes) {
    for (int i = 0; i < P.n_pieces; ++i)
        if (P.pieces[i].off == off && P.pieces[i].bytes == bytes) return true;
    return false;
}

static void check_plan(const std::vector<int> &sizes, int k, int batch, int64_t m) {
    const wdx_mlp_fit_params p = params(sizes, k, batch);
    const MlpFitPlan P = mlp_fit_plan(m, sizes[0] + 3, &p, true, true, true, true);
    CHECK(P.rc == WDX_SUCCESS, "rc %d: %s", P.rc, P.msg);
    if (P.rc != WDX_SUCCESS) return;
    ++g_plans;
    const int nl = P.nl;
    CHECK(nl == (int)sizes.size() - 1 && P.m == m && P.k == k && P.n_out == (k == 2 ? 1 : k), "sizes");
    // 1: batches
    CHECK(P.batch == std::min<int64_t>(batch, m) && P.batch_pad % 16 == 0 && P.batch_pad >= P.batch && P.batch_pad < P.batch + 16, "batch");
    int64_t rows = 0;
    for (int64_t s = 0; s < P.steps; ++s) {
        const int64_t nb = P.rows_of_step(s);
        CHECK(nb >= 1 && nb <= P.batch && s * P.batch == rows, "step %lld", (long long)s);
        rows += nb;
    }
    CHECK(rows == m, "the steps hold %lld of %lld rows", (long long)rows, (long long)m);
    if (P.last_batch != P.batch) ++g_short_last;
    if (batch > m) ++g_batch_clipped;
    if (batch == kMlpFitMaxBatch) ++g_at_max_batch;
    if (nl >= 3) ++g_two_hidden;
    if (P.n_out == 1) ++g_one_unit;
    bool whole = P.batch % 16 == 0 && m % P.batch == 0;
    for (int l = 0; l <= nl; ++l) whole = whole && P.sizes[l] % 16 == 0;
    if (whole) ++g_whole_tiles;
    // 2: the workspace
    CHECK(P.n_pieces <= kMlpFitMaxPieces && P.n_pieces == 1 + 6 * nl + (nl - 1) + nl + 6, "pieces %d", P.n_pieces);
    int64_t end = 0, raw = 0;
    for (int i = 0; i < P.n_pieces; ++i) {
        CHECK(P.pieces[i].off % 256 == 0 && P.pieces[i].off >= end && P.pieces[i].bytes > 0, "piece %d", i);
        end = P.pieces[i].off + P.pieces[i].bytes;
        raw += P.pieces[i].bytes;
    }
    CHECK(end <= P.bytes && P.bytes <= P.bytes_bound && P.bytes_bound == raw + 256 * (int64_t)P.n_pieces, "bytes %lld bound %lld", (long long)P.bytes,
          (long long)P.bytes_bound);
    CHECK(is_piece(P, P.off_xs, m * P.sizes[0] * 4), "xs");
    for (int l = 0; l < nl; ++l) {
        const int64_t wb = (int64_t)P.sizes[l] * P.sizes[l + 1] * 4, bb = (int64_t)P.sizes[l + 1] * 4;
        CHECK(is_piece(P, P.off_w[l], wb) && is_piece(P, P.off_mw[l], wb) && is_piece(P, P.off_vw[l], wb), "W %d", l);
        CHECK(is_piece(P, P.off_b[l], bb) && is_piece(P, P.off_mb[l], bb) && is_piece(P, P.off_vb[l], bb), "b %d", l);
    }
    for (int l = 1; l < nl; ++l) CHECK(is_piece(P, P.off_act[l], P.batch_pad * P.sizes[l] * 4), "A %d", l);
    for (int l = 1; l <= nl; ++l) CHECK(is_piece(P, P.off_delta[l], P.batch_pad * P.sizes[l] * 4), "delta %d", l);
    CHECK(is_piece(P, P.off_loss, P.loss_slots * 8) && is_piece(P, P.off_l2, P.l2_slots * 8), "slots");
    CHECK(is_piece(P, P.off_idx, m * 4) && is_piece(P, P.off_flags, 8), "idx, flags");
    CHECK(is_piece(P, P.off_mean, P.sizes[0] * 8) && is_piece(P, P.off_scale, P.sizes[0] * 8), "scaler");
    // 3: grids
    for (int64_t nb : {P.batch, P.last_batch}) {
        const int64_t g = P.fwd_grid(nb);
        CHECK(g == P.delta_grid(nb) && g * 16 >= nb && (g - 1) * 16 < nb && g * 16 <= P.batch_pad && g <= P.fwd_tiles, "row grid of %lld", (long long)nb);
    }
    for (int l = 0; l < nl; ++l) {
        const int ti = P.w_tiles_i[l], tj = P.w_tiles_j[l];
        CHECK(ti * 16 >= P.sizes[l] && (ti - 1) * 16 < P.sizes[l] && tj * 16 >= P.sizes[l + 1] && (tj - 1) * 16 < P.sizes[l + 1], "tiles of W %d", l);
        std::vector<uint8_t> seen((size_t)ti * tj, 0);
        for (int64_t g = 0; g < P.adam_grid(l); ++g)
            for (int w = 0; w < kMlpFitWavesPerGroup; ++w) {
                const int64_t tile = g * kMlpFitWavesPerGroup + w;
                if (tile < (int64_t)ti * tj) ++seen[(size_t)tile];
            }
        bool once = true;
        for (uint8_t s : seen) once = once && s == 1;
        CHECK(once, "adam grid of layer %d", l);
    }
    // 4: slots
    CHECK(P.loss_slots == P.steps * P.fwd_tiles && P.l2_slots == P.steps * P.w_tiles, "slot counts");
    int64_t t0 = 0;
    for (int l = 0; l < nl; ++l) {
        CHECK(P.w_tile0[l] == t0, "first slot of layer %d", l);
        t0 += (int64_t)P.w_tiles_i[l] * P.w_tiles_j[l];
    }
    CHECK(t0 == P.w_tiles, "tiles per step");
    const int64_t last = P.steps - 1;
    CHECK(last * P.fwd_tiles + P.fwd_grid(P.last_batch) <= P.loss_slots, "last loss slot");
    CHECK(last * P.w_tiles + P.w_tile0[nl - 1] + (int64_t)P.w_tiles_i[nl - 1] * P.w_tiles_j[nl - 1] <= P.l2_slots, "last L2 slot");
    CHECK(P.launches_per_step() == 2 * nl, "launches");
    // 5: LDS
    int widest = 0;
    for (int l = 1; l <= nl; ++l) widest = std::max(widest, P.sizes[l]);
    CHECK(P.lds_ld >= widest && P.lds_ld >= 16 && P.lds_bytes == 4 * 2 * 16 * (int64_t)P.lds_ld && P.lds_bytes <= 160 * 1024, "lds");
}

static void refused(const char *what, int64_t m, int64_t ld, const wdx_mlp_fit_params *p, int code, const char *text, bool d = true, bool y = true,
                    bool w = true, bool o = true) {
    const MlpFitPlan P = mlp_fit_plan(m, ld, p, d, y, w, o);
    ++g_refusals;
    CHECK(P.rc == code, "%s: rc %d, not %d (%s)", what, P.rc, code, P.msg);
    CHECK(strstr(P.msg, text) != nullptr && strncmp(P.msg, "mlp fit: ", 9) == 0, "%s: message '%s' lacks '%s'", what, P.msg, text);
    CHECK(P.bytes == 0 && P.n_pieces == 0 && P.steps == 0, "%s: a refused plan sizes nothing", what);
}

int main() {
    const std::vector<std::vector<int>> shapes = {
        {19, 17, 5}, {37, 24, 10, 1}, {16, 16, 3}, {16, 16, 16}, {5, 3, 16}, {2601, 100, 10}, {40, 100, 10}, {1, 1, 1}, {33, 512, 512, 512, 512, 16},
        {4, 15, 17, 2 - 1}, {64, 32, 16}, {7, 511, 9}};
    const int batches[] = {1, 2, 15, 16, 17, 64, 200, 256, 1000, 1024};
    const int64_t rows[] = {1, 2, 15, 16, 17, 70, 96, 203, 300, 530, 1024, 1025, 30000};
    for (const auto &s : shapes)
        for (int b : batches)
            for (int64_t m : rows) check_plan(s, s.back() == 1 ? 2 : s.back(), b, m);
    check_plan({40, 100, 10}, 10, 200, 100000000);   // a hundred million rows: int64 offsets

    wdx_mlp_fit_params ok = params({19, 17, 5}, 5, 64), p;
    refused("no parameters", 10, 19, nullptr, WDX_ERR_INVALID, "parameters are required");
    refused("no rows", 0, 19, &ok, WDX_ERR_INVALID, "m must be at least 1");
    p = ok, p.n_layers = 1;
    refused("no hidden layer", 10, 19, &p, WDX_ERR_INVALID, "at least one hidden layer");
    p = ok, p.n_layers = WDX_MLP_MAX_LAYERS + 1;
    refused("too many layers", 10, 19, &p, WDX_ERR_UNSUPPORTED, "WDX_MLP_MAX_LAYERS");
    p = ok, p.hidden_activation = 4;
    refused("activation", 10, 19, &p, WDX_ERR_INVALID, "unknown hidden activation");
    p = ok, p.n_classes = 1;
    refused("one class", 10, 19, &p, WDX_ERR_INVALID, "at least two");
    p = params({19, 17, 17}, 17, 64);
    refused("17 classes", 10, 19, &p, WDX_ERR_UNSUPPORTED, "more than 16");
    p = ok, p.sizes[1] = 0;
    refused("empty layer", 10, 19, &p, WDX_ERR_INVALID, "must be at least 1");
    p = ok, p.sizes[1] = WDX_MLP_MAX_WIDTH + 1;
    refused("wide layer", 10, 19, &p, WDX_ERR_UNSUPPORTED, "WDX_MLP_MAX_WIDTH");
    p = ok, p.sizes[2] = 4;
    refused("output width", 10, 19, &p, WDX_ERR_INVALID, "output layer");
    p = params({19, 17, 2}, 2, 64);
    refused("two units for two classes", 10, 19, &p, WDX_ERR_INVALID, "output layer");
    refused("ld", 10, 18, &ok, WDX_ERR_INVALID, "ld = 18");
    p = ok, p.batch_size = 0;
    refused("batch 0", 10, 19, &p, WDX_ERR_INVALID, "batch_size");
    p = ok, p.batch_size = WDX_MLP_FIT_MAX_BATCH + 1;
    refused("batch beyond the cap", 10, 19, &p, WDX_ERR_UNSUPPORTED, "WDX_MLP_FIT_MAX_BATCH");
    p = ok, p.max_epochs = 0;
    refused("epochs", 10, 19, &p, WDX_ERR_INVALID, "max_epochs");
    p = ok, p.n_iter_no_change = -1;
    refused("n_iter_no_change", 10, 19, &p, WDX_ERR_INVALID, "n_iter_no_change");
    p = ok, p.lr = 0;
    refused("lr", 10, 19, &p, WDX_ERR_INVALID, "lr must be");
    p = ok, p.alpha = -1;
    refused("alpha", 10, 19, &p, WDX_ERR_INVALID, "alpha must be");
    p = ok, p.beta1 = 1;
    refused("beta1", 10, 19, &p, WDX_ERR_INVALID, "beta1");
    p = ok, p.beta2 = -0.5;
    refused("beta2", 10, 19, &p, WDX_ERR_INVALID, "beta2");
    p = ok, p.epsilon = 0;
    refused("epsilon", 10, 19, &p, WDX_ERR_INVALID, "epsilon must be");
    p = ok, p.tol = NAN;
    refused("tol", 10, 19, &p, WDX_ERR_INVALID, "tol must be");
    refused("rows beyond int32", (int64_t)INT32_MAX + 1, 19, &ok, WDX_ERR_UNSUPPORTED, "int32 index list");
    p = params({2601, 100, 10}, 10, 1);
    refused("slots beyond int32", 2000000000, 2601, &p, WDX_ERR_UNSUPPORTED, "loss slots");
    refused("no matrix", 10, 19, &ok, WDX_ERR_INVALID, "distance matrix is required", false);
    refused("no classes", 10, 19, &ok, WDX_ERR_INVALID, "class indices are required", true, false);
    refused("no weights", 10, 19, &ok, WDX_ERR_INVALID, "coefs and intercepts are required", true, true, false);
    refused("no outputs", 10, 19, &ok, WDX_ERR_INVALID, "loss_curve, n_epochs and state are required", true, true, true, false);

    printf("checks %lld\nfailures %lld\nplans %lld\nshort_last %lld\nbatch_clipped %lld\nwhole_tiles %lld\ntwo_hidden %lld\none_unit %lld\nat_max_batch %lld\nrefusals %lld\n",
           g_checks, g_fail, g_plans, g_short_last, g_batch_clipped, g_whole_tiles, g_two_hidden, g_one_unit, g_at_max_batch, g_refusals);
    return g_fail ? 1 : 0;
}
