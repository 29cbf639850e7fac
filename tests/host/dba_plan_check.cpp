// What a barycenter step does with its host labels (warpdemux_amd/csrc/wdx_dba_plan.h), checked without a GPU: built with the system
// compiler under the address and undefined-behaviour sanitizers and run by tests/test_dba_plan_host.py.  Over a sweep of (label sizes,
// L, window) -- label sizes 0, 1, 2, 63, 64, 65, 129, 4 097, the medoids' cap and beyond it, rows labelled -1, L 1 .. 1024, windows 1 .. 32, beyond, and
// unbanded -- it checks of every plan:
//   1  the word count: ceil(2 min(2w - 1, L) / 64), and that every cell of every band row has its two bits inside the row's words
//   2  the route: the band ladder up to window 32, the general route beyond it and with the option
//   3  every padded row lies in exactly one pass, every pass is whole waves, and every chunk names the label that owns its rows
//   4  no pass exceeds kDbaCodeBytes, and the largest code, run and rolling-row index of a pass lies inside its piece
//   5  the pieces of the workspace do not overlap, lie inside workspace_bytes, and workspace_bytes <= workspace_bound
//   6  the partial block's four parts are disjoint and fill it
// and that each refusal carries its code and message.  Prints "checks <n>" / "failures <n>" and what the sweep met.
#include "wdx_dba_plan.h"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <random>
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

static long long g_plans = 0, g_multi_pass = 0, g_general = 0, g_two_words = 0, g_at_max_l = 0, g_unlabelled = 0, g_empty_labels = 0, g_beyond_cap = 0;

static void check_plan(const std::vector<int32_t> &label, int64_t G, int64_t L, int64_t window, bool opt_general) {
    const int64_t n = (int64_t)label.size();
    const DbaPlan P = dba_plan(label.data(), n, G, L, window, true, true, opt_general);
    CHECK(P.rc == WDX_SUCCESS, "rc %d: %s", P.rc, P.msg);
    if (P.rc != WDX_SUCCESS) return;
    ++g_plans;
    const int64_t w = (window <= 0 || window > L) ? L : window;
    // 1: the words
    const int64_t cells = std::min<int64_t>(2 * w - 1, L);
    CHECK(P.w == w && P.words == (2 * cells + 63) / 64 && P.words >= 1, "L %lld w %lld: words %lld", (long long)L, (long long)w, (long long)P.words);
    for (int64_t i = 0; i < L; ++i) {
        const int64_t jlo = std::max<int64_t>(0, i - (w - 1)), jhi = std::min<int64_t>(L - 1, i + (w - 1));
        CHECK(jhi - jlo < cells && 2 * (jhi - jlo) + 1 < 64 * P.words, "row %lld: cells %lld .. %lld", (long long)i, (long long)jlo, (long long)jhi);
    }
    if (P.words > 1) ++g_two_words;
    if (L == kDbaMaxL) ++g_at_max_l;
    // 2: the route
    const bool general = opt_general || w > 32;
    CHECK((P.kernel == DbaKernel::kGeneral) == general, "route");
    if (!general) {
        const DbaKernel want = w == 15 ? DbaKernel::kBand15 : (w <= 8 ? DbaKernel::kBand8 : (w <= 16 ? DbaKernel::kBand16 : DbaKernel::kBand32));
        CHECK(P.kernel == want && P.words <= 2, "ladder: w %lld", (long long)w);
    } else {
        ++g_general;
    }
    // 3: rows, passes, chunks
    std::vector<int64_t> size((size_t)G, 0);
    for (int32_t g : label)
        if (g >= 0) ++size[(size_t)g];
        else ++g_unlabelled;
    int64_t rows = 0;
    for (int64_t g = 0; g < G; ++g) {
        rows += (size[(size_t)g] + 63) / 64 * 64;
        if (!size[(size_t)g]) ++g_empty_labels;
    }
    CHECK(P.rows_padded == rows && P.chunks * 64 == rows && (int64_t)P.chunk_label.size() == P.chunks, "rows %lld", (long long)P.rows_padded);
    std::vector<uint8_t> in_pass((size_t)rows, 0);
    int64_t next = 0;
    for (const DbaPass &Q : P.passes) {
        CHECK(Q.row0 == next && Q.rows > 0 && Q.rows % 64 == 0 && Q.rows <= P.pass_rows && Q.row0 + Q.rows <= rows, "pass at %lld", (long long)Q.row0);
        for (int64_t r = Q.row0; r < Q.row0 + Q.rows && r < rows; ++r) ++in_pass[(size_t)r];
        next = Q.row0 + Q.rows;
        // 4: the pass inside its pieces
        const int64_t last = Q.rows - 1;
        CHECK(Q.rows * L * P.words * 8 <= kDbaCodeBytes, "pass of %lld rows: %lld code bytes", (long long)Q.rows, (long long)(Q.rows * L * P.words * 8));
        CHECK((((L - 1) * P.words + P.words - 1) * P.pass_rows + last + 1) * 8 <= P.code_bytes, "codes");
        CHECK(((L - 1) * P.pass_rows + last + 1) * 4 <= P.off_rolling - P.off_runs, "runs");
        if (general) CHECK(((2 * (L + 1) - 1) * P.pass_rows + last + 1) * 8 <= P.off_partial - P.off_rolling, "rolling rows");
    }
    CHECK(next == rows, "passes end at %lld of %lld", (long long)next, (long long)rows);
    for (int64_t r = 0; r < rows; ++r) CHECK(in_pass[(size_t)r] == 1, "row %lld in %d passes", (long long)r, (int)in_pass[(size_t)r]);
    if (P.passes.size() > 1) ++g_multi_pass;
    CHECK(P.code_bytes <= kDbaCodeBytes && P.pass_rows % 64 == 0, "code block %lld", (long long)P.code_bytes);
    {   // the order is stable and holds every labelled row once: inside a label the rows rise and fill its first `size` places
        int64_t placed = 0;
        for (int64_t g = 0; g < G; ++g) {
            const MedoidLabel &Lb = P.labels[(size_t)g];
            CHECK(Lb.row0 % 64 == 0 && Lb.size == size[(size_t)g] && Lb.chunks == (size[(size_t)g] + 63) / 64, "label %lld", (long long)g);
            int32_t prev = -1;
            for (int64_t r = 0; r < 64 * (int64_t)Lb.chunks; ++r) {
                const int32_t src = P.order[(size_t)(Lb.row0 + r)];
                CHECK(r < Lb.size ? src > prev : src == -1, "label %lld place %lld holds %d", (long long)g, (long long)r, src);
                if (r < Lb.size) prev = src, ++placed;
            }
        }
        CHECK(placed == n -(int64_t)std::count(label.begin(), label.end(), -1), "placed %lld", (long long)placed);
    }
    for (int64_t c = 0; c < P.chunks; ++c) {
        const int32_t g = P.chunk_label[(size_t)c];
        CHECK(g >= 0 && g < G, "chunk %lld label %d", (long long)c, g);
        if (g < 0 || g >= G) continue;
        const MedoidLabel &Lb = P.labels[(size_t)g];
        CHECK(c * 64 >= Lb.row0 && c * 64 < Lb.row0 + 64 * (int64_t)Lb.chunks, "chunk %lld outside label %d", (long long)c, g);
        for (int64_t r = 0; r < 64; ++r) {
            const int32_t src = P.order[(size_t)(c * 64 + r)];
            CHECK(src == -1 || (src >= 0 && src < n && label[(size_t)src] == g), "chunk %lld row %lld holds %d", (long long)c, (long long)r, src);
        }
    }
    // 5: the workspace
    const int64_t off[] = {P.off_order, P.off_chunk_label, P.off_labels, P.off_member, P.off_dense, P.off_centres,
                           P.off_centre_ok, P.off_codes, P.off_runs, P.off_rolling, P.off_partial, P.workspace_bytes};
    const int64_t need[] = {rows * 4, P.chunks * 4, (G + 1) * (int64_t)sizeof(MedoidLabel), rows, rows * L * 8, G * P.Lpad * 8, G,
                            P.code_bytes, P.pass_rows * L * 4, general ? 2 * (L + 1) * P.pass_rows * 8 : 0, P.chunks * (2 * L + 2) * 8};
    CHECK(off[0] == 0 && P.table_bytes == P.off_member, "tables");
    for (int k = 0; k < 11; ++k)
        CHECK(off[k] % 256 == 0 && off[k] + need[k] <= off[k + 1], "piece %d: %lld + %lld > %lld", k, (long long)off[k], (long long)need[k], (long long)off[k + 1]);
    CHECK(P.workspace_bytes <= P.workspace_bound, "workspace %lld > bound %lld (n %lld G %lld L %lld w %lld)", (long long)P.workspace_bytes,
          (long long)P.workspace_bound, (long long)n, (long long)G, (long long)L, (long long)w);
    // 6: the partial block
    if (P.chunks) {
        const int64_t c = P.chunks - 1;
        CHECK(P.part_S(0, 0) == 0 && P.part_S(c, L - 1) + 1 == P.part_K(0, 0) && P.part_K(c, L - 1) + 1 == P.part_cost(0) &&
                  P.part_cost(c) + 1 == P.part_members(0) && P.part_members(c) + 1 == P.chunks * (2 * L + 2),
              "partial block");
    }
}

static void check_refusal(const char *what, const DbaPlan &P, int rc, const char *needle) {
    CHECK(P.rc == rc && strstr(P.msg, needle), "%s: rc %d msg '%s'", what, P.rc, P.msg);
    CHECK(P.passes.empty() && P.workspace_bytes == 0, "%s: a refused plan holds work", what);
}

int main() {
    std::mt19937_64 rng(20260115);
    const int64_t sizes[] = {0, 1, 2, 63, 64, 65, 129, 4097};
    const int64_t Ls[] = {1, 2, 5, 25, 33, 40, 70, 110, 257, 1024};
    const int64_t windows[] = {0, 1, 2, 8, 9, 15, 16, 17, 31, 32, 33, 40, 200, 5000};
    for (int64_t L : Ls)
        for (int64_t window : windows)
            for (int general = 0; general < 2; ++general) {
                // a random choice of label sizes, some rows labelled -1, in shuffled order
                std::vector<int32_t> label;
                const int64_t G = 2 + (int64_t)(rng() % 7);
                for (int64_t g = 0; g < G; ++g) {
                    const int64_t m = sizes[rng() % (L > 300 ? 7 : 8)];
                    label.insert(label.end(), (size_t)m, (int32_t)g);
                }
                label.insert(label.end(), (size_t)(rng() % 9), -1);
                std::shuffle(label.begin(), label.end(), rng);
                check_plan(label, G, L, window, general != 0);
            }
    // the cap of a label, several passes: 32 768 rows at L 1024 unbanded are 32 passes of 1 024 rows
    {
        std::vector<int32_t> label((size_t)kMedoidMaxGroup, 0);
        check_plan(label, 1, 1024, 0, false);
        check_plan(label, 2, 110, 15, false);
        check_plan(label, 1, 110, 15, true);
        label.resize((size_t)kMedoidMaxGroup + 4097, 0);   // beyond the medoids' cap: a step has none
        check_plan(label, 1, 25, 15, false);
        ++g_beyond_cap;
        label.resize(5000);
        check_plan(label, 1, 1024, 0, false);
        check_plan(label, 1, 1024, 32, false);
        check_plan(label, 1, 1024, 200, false);   // 13 words: 2 496 rows a pass, three passes with a short last one
    }
    check_plan({}, 3, 25, 15, false);   // an empty batch
    // the refusals
    const std::vector<int32_t> two{0, 0};
    check_refusal("n_labels 0", dba_plan(two.data(), 2, 0, 5, 0, true, true, false), WDX_ERR_INVALID, "n_labels must be at least 1, not 0");
    check_refusal("L 0", dba_plan(two.data(), 2, 1, 0, 0, true, true, false), WDX_ERR_INVALID, "L must be at least 1, not 0");
    check_refusal("n < 0", dba_plan(two.data(), -1, 1, 5, 0, true, true, false), WDX_ERR_INVALID, "0 <= n");
    check_refusal("no labels", dba_plan(nullptr, 2, 1, 5, 0, true, true, false), WDX_ERR_INVALID, "their labels");
    check_refusal("no new centres", dba_plan(two.data(), 2, 1, 5, 0, false, true, false), WDX_ERR_INVALID, "required");
    check_refusal("no centres", dba_plan(two.data(), 2, 1, 5, 0, true, false, false), WDX_ERR_INVALID, "required");
    const std::vector<int32_t> bad{0, 1}, neg{0, -2};
    check_refusal("label G", dba_plan(bad.data(), 2, 1, 5, 0, true, true, false), WDX_ERR_INVALID, "the label of row 1 is 1, outside -1 .. 0");
    check_refusal("label -2", dba_plan(neg.data(), 2, 1, 5, 0, true, true, false), WDX_ERR_INVALID, "the label of row 1 is -2");
    check_refusal("L 1025", dba_plan(two.data(), 2, 1, 1025, 0, true, true, false), WDX_ERR_UNSUPPORTED, "L = 1025 is more than WDX_DBA_MAX_L = 1024");
    printf("checks %lld\nfailures %lld\nplans %lld\nmulti_pass %lld\ngeneral %lld\ntwo_words %lld\nat_max_l %lld\nunlabelled %lld\nempty_labels %lld\nbeyond_medoid_cap %lld\n",
           g_checks, g_fail, g_plans, g_multi_pass, g_general, g_two_words, g_at_max_l, g_unlabelled, g_empty_labels, g_beyond_cap);
    return g_fail ? 1 : 0;
}
