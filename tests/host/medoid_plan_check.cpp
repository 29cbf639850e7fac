// What a per-label medoid call does with its host labels (warpdemux_amd/csrc/wdx_medoid_plan.h), checked without a GPU:
// built with the system compiler under the address and undefined-behaviour sanitizers and run by tests/test_medoid_plan_host.py.
// Over a sweep of random label arrays (label sizes 0, 1, 2, 63, 64, 65, 128, 129, 4 097, the cap, rows labelled -1, empty labels)
// it checks of every plan:
//   1  the order is stable, holds every labelled row once, and every label starts on a multiple of 64 padded rows
//   2  every unordered pair of rows of one label lies in exactly one tile (chunk pairs (I, J), J >= I, each once; small labels
//      row pair by row pair)
//   3  every (chunk, row) partial sum is written exactly once, inside the partial block of its pass, and no two labels of a pass
//      share an entry
//   4  every piece of the workspace lies inside its stated size, a pass within kMedoidPartialBytes
//   5  the workspace is within the stated bound
//   6  every label is in exactly one pass and the passes' tile ranges tile the two lists
// and that each refusal carries its code and message.  Prints "checks <n>" / "failures <n>" and what the sweep met.
#include "wdx_medoid_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <string>
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

static long long g_plans = 0, g_tiles = 0, g_multi_pass = 0, g_at_cap = 0, g_empty_labels = 0, g_unlabelled = 0;

static void check_plan(const std::vector<int32_t> &label, int64_t G, int64_t L, bool general) {
    const int64_t n = (int64_t)label.size();
    const MedoidPlan P = medoid_plan(label.data(), n, G, L, true, general);
    CHECK(P.rc == WDX_SUCCESS, "rc %d: %s", P.rc, P.msg);
    if (P.rc != WDX_SUCCESS) return;
    ++g_plans;
    // 1: the order
    CHECK((int64_t)P.order.size() == P.rows_padded && (int64_t)P.labels.size() == G + 1, "sizes");
    std::vector<int64_t> size((size_t)G, 0);
    for (int32_t g : label)
        if (g >= 0) ++size[(size_t)g];
        else ++g_unlabelled;
    std::vector<uint8_t> seen((size_t)n, 0);
    int64_t row = 0;
    for (int64_t g = 0; g < G; ++g) {
        const MedoidLabel &Lb = P.labels[(size_t)g];
        const int64_t m = size[(size_t)g], c = (m + 63) / 64;
        if (m == 0) ++g_empty_labels;
        if (m == kMedoidMaxGroup) ++g_at_cap;
        CHECK(Lb.row0 == row && Lb.row0 % 64 == 0 && Lb.size == m && Lb.chunks == c, "label %lld: row0 %lld size %d chunks %d", (long long)g,
              (long long)Lb.row0, Lb.size, Lb.chunks);
        int32_t prev = -1;
        for (int64_t r = 0; r < 64 * c; ++r) {
            const int32_t src = P.order[(size_t)(row + r)];
            if (r < m) {
                CHECK(src > prev && src < n && label[(size_t)src] == g && !seen[(size_t)src], "label %lld padded row %lld holds %d", (long long)g,
                      (long long)r, src);
                if (src >= 0 && src < n) seen[(size_t)src] = 1;
                prev = src;
            } else {
                CHECK(src == -1, "padding row holds %d", src);
            }
        }
        row += 64 * c;
    }
    CHECK(row == P.rows_padded, "rows_padded");
    for (int64_t r = 0; r < n; ++r) CHECK((seen[(size_t)r] != 0) == (label[(size_t)r] >= 0), "row %lld", (long long)r);
    // 6: passes
    {
        int32_t g = 0;
        int64_t d = 0, o = 0;
        for (size_t q = 0; q < P.passes.size(); ++q) {
            const MedoidPass &Q = P.passes[q];
            CHECK(Q.g0 == g && Q.g1 > Q.g0 && Q.diag0 == d && Q.off0 == o && Q.diag1 >= d && Q.off1 >= o, "pass %zu", q);
            CHECK(Q.partial_doubles * 8 <= kMedoidPartialBytes && Q.partial_doubles * 8 <= P.partial_bytes, "pass %zu holds %lld doubles", q,
                  (long long)Q.partial_doubles);
            for (int32_t k = Q.g0; k < Q.g1; ++k) CHECK(P.labels[(size_t)k].pass == (int32_t)q, "label %d pass", k);
            CHECK(P.labels[(size_t)Q.g0].diag0 == Q.diag0 && P.labels[(size_t)Q.g1].diag0 == Q.diag1 && P.labels[(size_t)Q.g0].off0 == Q.off0 &&
                      P.labels[(size_t)Q.g1].off0 == Q.off1,
                  "pass %zu tiles", q);
            g = Q.g1, d = Q.diag1, o = Q.off1;
        }
        CHECK(g == G && d == P.n_diag && o == P.n_off, "the passes end at label %d", g);
        if (P.passes.size() > 1) ++g_multi_pass;
    }
    // 2 and 3: the tiles
    std::vector<std::vector<uint8_t>> chunk_pairs((size_t)G), written(P.passes.size());
    for (int64_t g = 0; g < G; ++g) chunk_pairs[(size_t)g].assign((size_t)(P.labels[(size_t)g].chunks * (int64_t)P.labels[(size_t)g].chunks), 0);
    for (size_t q = 0; q < P.passes.size(); ++q) written[q].assign((size_t)P.passes[q].partial_doubles, 0);
    std::vector<std::vector<uint8_t>> row_pairs((size_t)G);
    for (int64_t g = 0; g < G; ++g)
        if (size[(size_t)g] <= 200) row_pairs[(size_t)g].assign((size_t)(size[(size_t)g] * size[(size_t)g]), 0);
    auto write = [&](int32_t g, int64_t c, int64_t r) {
        const MedoidLabel &Lb = P.labels[(size_t)g];
        const int64_t at = P.partial_index(g, c, r);
        const bool inside = at >= 0 && at < P.passes[(size_t)Lb.pass].partial_doubles;
        CHECK(inside, "label %d partial (%lld, %lld) at %lld", g, (long long)c, (long long)r, (long long)at);
        if (!inside) return;
        CHECK(written[(size_t)Lb.pass][(size_t)at] == 0, "label %d partial (%lld, %lld) written twice", g, (long long)c, (long long)r);
        written[(size_t)Lb.pass][(size_t)at] = 1;
    };
    g_tiles += P.tile_count();
    for (int64_t k = 0; k < P.tile_count(); ++k) {
        const MedoidTile T = P.tile(k);
        const bool ok = T.label >= 0 && T.label < G && T.I >= 0 && T.J >= T.I && T.J < P.labels[(size_t)T.label].chunks && (k < P.n_diag) == (T.I == T.J);
        CHECK(ok, "tile %lld = (%d, %d, %d)", (long long)k, T.label, T.I, T.J);
        if (!ok) continue;
        const MedoidLabel &Lb = P.labels[(size_t)T.label];
        uint8_t &cp = chunk_pairs[(size_t)T.label][(size_t)(T.I * (int64_t)Lb.chunks + T.J)];
        CHECK(cp == 0, "tile (%d, %d, %d) twice", T.label, T.I, T.J);
        cp = 1;
        for (int64_t a = 0; a < 64; ++a) {   // what the kernels write: wdx_medoid.hip
            if (T.I == T.J) {
                write(T.label, T.I, 64 * T.I + a);
            } else {
                write(T.label, T.J, 64 * T.I + a);   // the row part: S_J of the rows of chunk I
                write(T.label, T.I, 64 * T.J + a);   // the column part: S_I of the rows of chunk J
            }
        }
        auto &rp = row_pairs[(size_t)T.label];
        if (!rp.empty())
            for (int64_t a = 64 * T.I; a < std::min<int64_t>(64 * T.I + 64, Lb.size); ++a)
                for (int64_t b = std::max<int64_t>(64 * T.J, T.I == T.J ? a : 0); b < std::min<int64_t>(64 * T.J + 64, Lb.size); ++b) {
                    CHECK(rp[(size_t)(a * Lb.size + b)] == 0, "pair (%lld, %lld) of label %d twice", (long long)a, (long long)b, T.label);
                    rp[(size_t)(a * Lb.size + b)] = 1;
                }
    }
    for (int64_t g = 0; g < G; ++g) {
        const int64_t c = P.labels[(size_t)g].chunks, m = size[(size_t)g];
        for (int64_t I = 0; I < c; ++I)
            for (int64_t J = 0; J < c; ++J) CHECK(chunk_pairs[(size_t)g][(size_t)(I * c + J)] == (J >= I), "label %lld chunk pair (%lld, %lld)", (long long)g, (long long)I, (long long)J);
        if (!row_pairs[(size_t)g].empty())
            for (int64_t a = 0; a < m; ++a)
                for (int64_t b = 0; b < m; ++b) CHECK(row_pairs[(size_t)g][(size_t)(a * m + b)] == (b >= a), "label %lld pair (%lld, %lld)", (long long)g, (long long)a, (long long)b);
    }
    for (size_t q = 0; q < written.size(); ++q) {
        int64_t miss = 0;
        for (uint8_t w : written[q]) miss += w == 0;
        CHECK(miss == 0, "pass %zu: %lld partial sums never written", q, (long long)miss);
    }
    // 4 and 5: the workspace
    const int64_t off[] = {P.off_order, P.off_labels, P.off_member, P.off_dense, P.off_padded, P.off_partial, P.off_matrix, P.workspace_bytes};
    const int64_t need[] = {P.rows_padded * 4, (G + 1) * (int64_t)sizeof(MedoidLabel), P.rows_padded, P.rows_padded * L * 8, P.rows_padded * P.Lpad * 8,
                            P.partial_bytes, P.matrix_bytes};
    CHECK(off[0] == 0 && P.table_bytes == P.off_member, "the tables lead the workspace");
    for (int k = 0; k < 7; ++k) CHECK(off[k] % 256 == 0 && off[k] + need[k] <= off[k + 1], "piece %d: offset %lld, %lld bytes, next %lld", k, (long long)off[k], (long long)need[k], (long long)off[k + 1]);
    CHECK(P.Lpad == L + 2 * kDtwHalo, "Lpad");
    CHECK(P.partial_bytes <= kMedoidPartialBytes, "partial block of %lld bytes", (long long)P.partial_bytes);
    CHECK(P.workspace_bytes <= P.workspace_bound, "workspace %lld beyond its bound %lld", (long long)P.workspace_bytes, (long long)P.workspace_bound);
    if (general && P.max_size > 0) {
        const int64_t cols = (P.max_size + 63) / 64 * 64;
        CHECK(P.block_rows >= 64 && P.block_rows % 64 == 0 && P.block_rows <= cols && P.matrix_bytes == P.block_rows * cols * 4 &&
                  (P.matrix_bytes <= kMedoidMatrixBytes || P.block_rows == 64),
              "matrix block: %lld rows, %lld bytes", (long long)P.block_rows, (long long)P.matrix_bytes);
    } else {
        CHECK(P.matrix_bytes == 0, "a matrix block without the general route");
    }
}

static std::vector<int32_t> labels_of(const std::vector<int64_t> &sizes, int64_t unlabelled, std::mt19937_64 &rng) {
    std::vector<int32_t> label;
    for (size_t g = 0; g < sizes.size(); ++g) label.insert(label.end(), (size_t)sizes[g], (int32_t)g);
    label.insert(label.end(), (size_t)unlabelled, -1);
    std::shuffle(label.begin(), label.end(), rng);
    return label;
}

static void refusal(const char *what, const MedoidPlan &P, int rc, const char *needle) {
    CHECK(P.rc == rc && strstr(P.msg, needle) != nullptr, "%s: rc %d, message \"%s\" (want %d, \"%s\")", what, P.rc, P.msg, rc, needle);
}

int main() {
    std::mt19937_64 rng(20240607);
    const int64_t pool[] = {0, 1, 2, 63, 64, 65, 128, 129, 4097};
    // the tile decode over every chunk count up to the cap's
    for (int64_t c = 2; c <= kMedoidMaxGroup / 64; c += (c < 20 ? 1 : 41)) {
        int64_t t = 0;
        for (int32_t I = 0; I < c; ++I)
            for (int32_t J = I + 1; J < c; ++J, ++t) {
                int32_t i, j;
                medoid_upper_tile(c, t, &i, &j);
                CHECK(i == I && j == J, "c %lld tile %lld -> (%d, %d), not (%d, %d)", (long long)c, (long long)t, i, j, I, J);
            }
        CHECK(t == c * (c - 1) / 2, "count");
    }
    // random label arrays
    for (int trial = 0; trial < 60; ++trial) {
        const int G = 1 + (int)(rng() % 12);
        std::vector<int64_t> sizes;
        for (int g = 0; g < G; ++g) sizes.push_back(pool[rng() % (trial % 3 == 0 ? 9 : 8)]);
        const std::vector<int32_t> label = labels_of(sizes, (int64_t)(rng() % 3 == 0 ? 0 : rng() % 70), rng);
        check_plan(label, G, trial % 2 ? 110 : 25, trial % 4 == 1);
    }
    // every size of the pool alone, and all of them in one call
    for (int64_t m : pool) check_plan(labels_of({m}, 3, rng), 1, 110, m % 2 == 0);
    check_plan(labels_of(std::vector<int64_t>(pool, pool + 9), 17, rng), 9, 40, false);
    check_plan({}, 4, 110, false);                 // an empty batch
    check_plan(std::vector<int32_t>(50, -1), 2, 7, true);   // nobody takes part
    // the cap: one label of 32 768 rows; two of them and small ones (several passes)
    check_plan(labels_of({kMedoidMaxGroup}, 0, rng), 1, 110, false);
    check_plan(labels_of({kMedoidMaxGroup}, 5, rng), 1, 25, true);
    check_plan(labels_of({65, kMedoidMaxGroup, 0, kMedoidMaxGroup, 129, 4097}, 9, rng), 6, 25, false);
    // refusals
    {
        const std::vector<int32_t> ok = labels_of({3, 4}, 2, rng);
        refusal("n_labels 0", medoid_plan(ok.data(), (int64_t)ok.size(), 0, 110, true, false), WDX_ERR_INVALID, "n_labels must be at least 1, not 0");
        refusal("n_labels -3", medoid_plan(ok.data(), (int64_t)ok.size(), -3, 110, true, false), WDX_ERR_INVALID, "n_labels must be at least 1, not -3");
        refusal("L 0", medoid_plan(ok.data(), (int64_t)ok.size(), 2, 0, true, false), WDX_ERR_INVALID, "L must be at least 1, not 0");
        refusal("no medoid output", medoid_plan(ok.data(), (int64_t)ok.size(), 2, 110, false, false), WDX_ERR_INVALID, "medoid output is required");
        refusal("no labels", medoid_plan(nullptr, 5, 2, 110, true, false), WDX_ERR_INVALID, "their labels");
        std::vector<int32_t> bad = ok;
        bad[3] = 2;
        refusal("label 2 of 2", medoid_plan(bad.data(), (int64_t)bad.size(), 2, 110, true, false), WDX_ERR_INVALID, "the label of row 3 is 2, outside -1 .. 1");
        bad[3] = -2;
        refusal("label -2", medoid_plan(bad.data(), (int64_t)bad.size(), 2, 110, true, false), WDX_ERR_INVALID, "the label of row 3 is -2, outside -1 .. 1");
        const std::vector<int32_t> big = labels_of({10, kMedoidMaxGroup + 1}, 4, rng);
        refusal("cap + 1", medoid_plan(big.data(), (int64_t)big.size(), 2, 110, true, false), WDX_ERR_UNSUPPORTED,
                "label 1 has 32769 rows, more than WDX_MEDOID_MAX_GROUP = 32768");
        CHECK(medoid_plan(nullptr, 0, 1, 1, true, false).rc == WDX_SUCCESS, "an empty batch without a label array");
    }
    // the route rule
    CHECK(medoid_kernel(25, 15, false, false) == MedoidKernel::kShort && medoid_kernel(25, 15, false, true) == MedoidKernel::kBand15, "short");
    CHECK(medoid_kernel(110, 15, false, false) == MedoidKernel::kBand15 && medoid_kernel(40, 3, false, false) == MedoidKernel::kBand8 &&
              medoid_kernel(110, 16, false, false) == MedoidKernel::kBand16 && medoid_kernel(110, 32, false, false) == MedoidKernel::kBand32 &&
              medoid_kernel(20, 0, false, false) == MedoidKernel::kBand32,
          "ladder");
    CHECK(medoid_kernel(110, 33, false, false) == MedoidKernel::kGeneral && medoid_kernel(110, 0, false, false) == MedoidKernel::kGeneral &&
              medoid_kernel(110, 15, true, false) == MedoidKernel::kGeneral,
          "general");
    printf("checks %lld\nfailures %lld\nplans %lld\ntiles %lld\nmulti_pass %lld\nat_cap %lld\nempty_labels %lld\nunlabelled %lld\n", g_checks, g_fail, g_plans,
           g_tiles, g_multi_pass, g_at_cap, g_empty_labels, g_unlabelled);
    return g_fail ? 1 : 0;
}
