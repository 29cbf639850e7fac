// What a self-distance-matrix call does with its sizes (warpdemux_amd/csrc/wdx_self_plan.h), checked without a GPU: built with
// the system compiler under the address and undefined-behaviour sanitizers and run by tests/test_self_plan_host.py.
// Over n in {0, 1, 63, 64, 65, 4 097, 65 536} (and 65 537, refused), both routes and several L it checks of every plan:
//   1  the padded row count is the least multiple of 64 that holds n; the two tile lists have chunks and chunks (chunks - 1) / 2
//      entries, every decoded tile is (I, J) with 0 <= I <= J < chunks, diagonal exactly in the first list, each chunk pair once
//   2  for n <= 4 097: every unordered pair of rows lies in exactly one decoded tile, and every entry (a, b), a, b < n, of the
//      matrix is written exactly once by what the kernels write of a tile (both images; the diagonal tile once)
//   3  every piece of the workspace lies inside its stated size, and the workspace is within the stated bound
//   4  the general route's row blocks tile 0 .. n in order, and each has at least 64 rows or all n of them
//   5  the route follows medoid_kernel
// and that each refusal carries its code and message.  Prints "checks <n>" / "failures <n>" and what the sweep met.
#include "wdx_self_plan.h"

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

static long long g_plans = 0, g_tiles = 0, g_at_cap = 0, g_pair_checked = 0, g_blocks = 0;

static void check_plan(int64_t n, int64_t L, int64_t ld, int64_t window, bool opt_general) {
    const SelfPlan P = self_plan(n, L, ld, window, true, opt_general, false);
    CHECK(P.rc == WDX_SUCCESS, "n %lld: rc %d: %s", (long long)n, P.rc, P.msg);
    if (P.rc != WDX_SUCCESS) return;
    ++g_plans;
    if (n == kSelfMaxRows) ++g_at_cap;
    // 5: the route
    CHECK(P.kernel == medoid_kernel(L, window, opt_general, false) && P.general == (P.kernel == MedoidKernel::kGeneral), "route");
    // 1: rows and tiles
    const int64_t c = (n + 63) / 64;
    CHECK(P.chunks == c && P.rows_padded == 64 * c && P.rows_padded >= n && P.rows_padded < n + 64, "n %lld: %lld chunks, %lld rows", (long long)n,
          (long long)P.chunks, (long long)P.rows_padded);
    CHECK(P.n_diag == c && P.n_off == c * (c - 1) / 2 && P.tile_count() == c * (c + 1) / 2, "tile counts");
    CHECK(P.n == n && P.L == L && P.ld == ld && P.Lpad == L + 2 * kDtwHalo, "sizes");
    g_tiles += P.tile_count();
    std::vector<uint8_t> chunk_pairs((size_t)(c * c), 0);
    const bool pairs = n <= 4097;
    std::vector<uint8_t> row_pairs, written;
    if (pairs) row_pairs.assign((size_t)(n * n), 0), written.assign((size_t)(n * n), 0);
    for (int64_t k = 0; k < P.tile_count(); ++k) {
        const SelfTile T = P.tile(k);
        const bool ok = T.I >= 0 && T.J >= T.I && T.J < c && (k < P.n_diag) == (T.I == T.J);
        CHECK(ok, "tile %lld = (%d, %d)", (long long)k, T.I, T.J);
        if (!ok) continue;
        uint8_t &cp = chunk_pairs[(size_t)(T.I * c + T.J)];
        CHECK(cp == 0, "tile (%d, %d) twice", T.I, T.J);
        cp = 1;
        if (!pairs) continue;
        for (int64_t a = 64 * T.I; a < std::min<int64_t>(64 * T.I + 64, n); ++a)
            for (int64_t b = std::max<int64_t>(64 * T.J, T.I == T.J ? a : 0); b < std::min<int64_t>(64 * T.J + 64, n); ++b) {
                CHECK(row_pairs[(size_t)(a * n + b)] == 0, "pair (%lld, %lld) twice", (long long)a, (long long)b);
                row_pairs[(size_t)(a * n + b)] = 1;
            }
        // what the kernels write of a tile (wdx_dtw_self.hip): rows and columns >= n are masked
        for (int64_t a = 64 * T.I; a < std::min<int64_t>(64 * T.I + 64, n); ++a)
            for (int64_t b = 64 * T.J; b < std::min<int64_t>(64 * T.J + 64, n); ++b) {
                ++written[(size_t)(a * n + b)];                    // the upper image (the whole tile when I == J)
                if (T.I != T.J) ++written[(size_t)(b * n + a)];    // the mirror image
            }
    }
    for (int64_t I = 0; I < c; ++I)
        for (int64_t J = 0; J < c; ++J) CHECK(chunk_pairs[(size_t)(I * c + J)] == (J >= I), "chunk pair (%lld, %lld)", (long long)I, (long long)J);
    if (pairs) {
        ++g_pair_checked;
        int64_t bad_pairs = 0, bad_writes = 0;
        for (int64_t a = 0; a < n; ++a)
            for (int64_t b = 0; b < n; ++b) {
                bad_pairs += row_pairs[(size_t)(a * n + b)] != (b >= a);
                bad_writes += written[(size_t)(a * n + b)] != 1;
            }
        CHECK(bad_pairs == 0, "n %lld: %lld unordered pairs not in exactly one tile", (long long)n, (long long)bad_pairs);
        CHECK(bad_writes == 0, "n %lld: %lld entries not written exactly once", (long long)n, (long long)bad_writes);
    }
    // 3: the workspace
    const int64_t off[] = {P.off_member, P.off_dense, P.off_padded, P.workspace_bytes};
    const int64_t need[] = {P.rows_padded, P.rows_padded * L * 8, P.rows_padded * P.Lpad * 8};
    CHECK(off[0] == 0, "the member flags lead the workspace");
    for (int k = 0; k < 3; ++k)
        CHECK(off[k] % 256 == 0 && off[k] + need[k] <= off[k + 1], "piece %d: offset %lld, %lld bytes, next %lld", k, (long long)off[k], (long long)need[k],
              (long long)off[k + 1]);
    CHECK(P.workspace_bytes <= P.workspace_bound, "workspace %lld beyond its bound %lld", (long long)P.workspace_bytes, (long long)P.workspace_bound);
    CHECK(P.workspace_bound == (n + 63) * (L + P.Lpad) * 8 + (n + 63) + 3 * 256, "the stated bound");
    // 4: the general route's blocks
    if (P.general) {
        int64_t r = 0;
        for (const SelfBlock &B : P.blocks) {
            CHECK(B.r0 == r && B.rows >= 1 && (B.rows >= 64 || B.rows == n) && B.rows < kSelfBlockRows + 64, "block at %lld of %lld rows", (long long)B.r0,
                  (long long)B.rows);
            r += B.rows;
            ++g_blocks;
        }
        CHECK(r == n && (n > 0 || P.blocks.empty()), "the blocks end at row %lld of %lld", (long long)r, (long long)n);
    } else {
        CHECK(P.blocks.empty(), "row blocks without the general route");
    }
}

static void refusal(const char *what, const SelfPlan &P, int rc, const char *needle) {
    CHECK(P.rc == rc && strstr(P.msg, needle) != nullptr, "%s: rc %d, message \"%s\" (want %d, \"%s\")", what, P.rc, P.msg, rc, needle);
}

int main() {
    const int64_t sizes[] = {0, 1, 63, 64, 65, 4097, 65536};
    for (int64_t n : sizes)
        for (int general = 0; general < 2; ++general) {
            check_plan(n, 110, n, 15, general != 0);
            check_plan(n, 25, n + 37, 15, general != 0);
        }
    // sizes around the general route's block edges, the unbanded route, and the rest of the ladder
    for (int64_t n : {2, 128, 129, 200, 8191, 8192, 8193, 8255, 8256, 8257, 16384, 16385, 16447, 16448}) {
        check_plan(n, 110, n, 0, false);    // unbanded: effective window 110 -> general
        check_plan(n, 40, n + 1, 3, n % 2 == 0);
    }
    check_plan(200, 110, 200, 32, false);
    check_plan(200, 110, 200, 16, false);
    // the decode at the cap's chunk count, in full
    {
        const int64_t c = kSelfMaxRows / 64;
        int64_t t = 0, bad = 0;
        for (int32_t I = 0; I < c; ++I)
            for (int32_t J = I + 1; J < c; ++J, ++t) {
                int32_t i, j;
                medoid_upper_tile(c, t, &i, &j);
                bad += !(i == I && j == J);
            }
        CHECK(bad == 0 && t == c * (c - 1) / 2, "the decode at %lld chunks: %lld wrong", (long long)c, (long long)bad);
    }
    // refusals
    refusal("cap + 1", self_plan(65537, 110, 65537, 15, true, false, false), WDX_ERR_UNSUPPORTED,
            "n = 65537 rows, more than WDX_SELF_MATRIX_MAX_ROWS = 65536");
    refusal("cap + 1, general", self_plan(65537, 25, 70000, 15, true, true, false), WDX_ERR_UNSUPPORTED, "n = 65537 rows");
    refusal("L 0", self_plan(10, 0, 10, 15, true, false, false), WDX_ERR_INVALID, "L must be at least 1, not 0");
    refusal("L -4", self_plan(10, -4, 10, 15, true, false, false), WDX_ERR_INVALID, "L must be at least 1, not -4");
    refusal("n -1", self_plan(-1, 25, 10, 15, true, false, false), WDX_ERR_INVALID, "n must not be negative (n = -1)");
    refusal("ld < n", self_plan(10, 25, 9, 15, true, false, false), WDX_ERR_INVALID, "ld = 9 is less than n = 10");
    refusal("no output", self_plan(10, 25, 10, 15, false, false, false), WDX_ERR_INVALID, "the output matrix is required");
    CHECK(self_plan(0, 25, 0, 15, false, false, false).rc == WDX_SUCCESS, "an empty call without an output");
    // the route rule, with WDX_OPT_NO_SHORT_DTW
    CHECK(self_plan(100, 25, 100, 15, true, false, false).kernel == MedoidKernel::kShort && self_plan(100, 25, 100, 15, true, false, true).kernel == MedoidKernel::kBand15 &&
              self_plan(100, 110, 100, 33, true, false, false).general && self_plan(100, 110, 100, 15, true, true, false).general,
          "routes");
    printf("checks %lld\nfailures %lld\nplans %lld\ntiles %lld\nat_cap %lld\npair_checked %lld\nblocks %lld\n", g_checks, g_fail, g_plans, g_tiles, g_at_cap,
           g_pair_checked, g_blocks);
    return g_fail ? 1 : 0;
}
