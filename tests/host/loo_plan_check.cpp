// What a leave-one-out nearest-neighbour call does with its sizes (warpdemux_amd/csrc/wdx_loo_plan.h), checked without a GPU:
// built with the system compiler under the address and undefined-behaviour sanitizers and run by tests/test_loo_plan_host.py.
// Over a sweep of (n, L, window, option) it checks of every plan:
//   1  the padded row count is the least multiple of 64 that holds n; the two tile lists have chunks and chunks (chunks - 1) / 2
//      entries, every decoded tile is (I, J) with 0 <= I <= J < chunks, diagonal exactly in the first list, and every unordered
//      chunk pair lies in exactly one tile
//   2  for n <= 4 097: what the kernels take from a tile (its row side and its column side; a diagonal tile each pair once, a == b
//      never) offers every ordered pair (a, b), a != b, a, b < n, exactly once -- every row sees every other row once
//   3  the general route's blocks cover every padded row once, in order, in multiples of 64 rows, and a block is within 96 MiB
//   4  every piece of the workspace lies inside its stated size, and the workspace is within the stated bound, which is
//      O(n L) on the tile route
//   5  the route follows medoid_kernel; the keys keep the rule's order
// and that each refusal carries its code and message.  Prints "checks <n>" / "failures <n>" and what the sweep met.
#include "wdx_loo_plan.h"

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

static long long g_plans = 0, g_tiles = 0, g_at_cap = 0, g_pair_checked = 0, g_blocks = 0, g_general = 0, g_multi_block = 0;

static void check_plan(int64_t n, int64_t L, int64_t window, bool opt_general, bool no_short = false) {
    const LooPlan P = loo_plan(n, L, window, true, opt_general, no_short);
    CHECK(P.rc == WDX_SUCCESS, "n %lld: rc %d: %s", (long long)n, P.rc, P.msg);
    if (P.rc != WDX_SUCCESS) return;
    ++g_plans;
    if (n == kLooMaxRows) ++g_at_cap;
    // 5: the route
    CHECK(P.kernel == medoid_kernel(L, window, opt_general, no_short) && P.general == (P.kernel == MedoidKernel::kGeneral), "route");
    // 1: rows and tiles
    const int64_t c = (n + 63) / 64;
    CHECK(P.chunks == c && P.rows_padded == 64 * c && P.rows_padded >= n && P.rows_padded < n + 64, "n %lld: %lld chunks, %lld rows", (long long)n,
          (long long)P.chunks, (long long)P.rows_padded);
    CHECK(P.n_diag == c && P.n_off == c * (c - 1) / 2 && P.tile_count() == c * (c + 1) / 2, "tile counts");
    CHECK(P.n == n && P.L == L && P.Lpad == L + 2 * kDtwHalo, "sizes");
    g_tiles += P.tile_count();
    std::vector<uint8_t> chunk_pairs((size_t)(c * c), 0);
    const bool pairs = n <= 4097;
    std::vector<uint8_t> offered;   // offered[a * n + b]: times row a was offered candidate b
    if (pairs) offered.assign((size_t)(n * n), 0);
    for (int64_t k = 0; k < P.tile_count(); ++k) {
        const LooTile T = P.tile(k);
        const bool ok = T.I >= 0 && T.J >= T.I && T.J < c && (k < P.n_diag) == (T.I == T.J);
        CHECK(ok, "tile %lld = (%d, %d)", (long long)k, T.I, T.J);
        if (!ok) continue;
        uint8_t &cp = chunk_pairs[(size_t)(T.I * c + T.J)];
        CHECK(cp == 0, "tile (%d, %d) twice", T.I, T.J);
        cp = 1;
        if (!pairs) continue;
        // what the kernels take of a tile (wdx_dtw_loo.hip): rows and columns >= n are padding, never members
        for (int64_t a = 64 * T.I; a < std::min<int64_t>(64 * T.I + 64, n); ++a)
            for (int64_t b = 64 * T.J; b < std::min<int64_t>(64 * T.J + 64, n); ++b) {
                if (T.I == T.J && b <= a) continue;      // a diagonal tile: pair (a, b) from lane min(a, b), a == b never
                ++offered[(size_t)(a * n + b)];          // the row side: row a, candidate b
                ++offered[(size_t)(b * n + a)];          // the column side: row b, candidate a
            }
    }
    for (int64_t I = 0; I < c; ++I)
        for (int64_t J = 0; J < c; ++J) CHECK(chunk_pairs[(size_t)(I * c + J)] == (J >= I), "chunk pair (%lld, %lld)", (long long)I, (long long)J);
    if (pairs) {
        ++g_pair_checked;
        int64_t bad = 0;
        for (int64_t a = 0; a < n; ++a)
            for (int64_t b = 0; b < n; ++b) bad += offered[(size_t)(a * n + b)] != (a != b);
        CHECK(bad == 0, "n %lld: %lld ordered pairs not offered exactly once", (long long)n, (long long)bad);
    }
    // 3: the general route's blocks
    if (P.general && n > 0) {
        ++g_general;
        int64_t r = 0;
        CHECK(P.block_rows >= 64 && P.block_rows % 64 == 0 && P.block_rows <= P.rows_padded, "block rows %lld", (long long)P.block_rows);
        CHECK(P.block_bytes == P.block_rows * P.rows_padded * 4 && P.block_bytes <= kLooBlockBytes, "block of %lld bytes", (long long)P.block_bytes);
        // as many rows as fit: another 64 would not (or there are no more rows)
        CHECK(P.block_rows == P.rows_padded || (P.block_rows + 64) * P.rows_padded * 4 > kLooBlockBytes, "the block holds fewer rows than fit");
        for (const LooBlock &B : P.blocks) {
            CHECK(B.r0 == r && B.rows >= 64 && B.rows % 64 == 0 && B.rows <= P.block_rows, "block at %lld of %lld rows", (long long)B.r0, (long long)B.rows);
            CHECK(B.rows * P.rows_padded * 4 <= P.block_bytes, "block at %lld beyond the block buffer", (long long)B.r0);
            r += B.rows;
            ++g_blocks;
        }
        CHECK(r == P.rows_padded, "the blocks end at padded row %lld of %lld", (long long)r, (long long)P.rows_padded);
        if (P.blocks.size() > 1) ++g_multi_block;
    } else {
        CHECK(P.blocks.empty() && P.block_bytes == 0 && P.block_rows == 0, "row blocks without the general route");
    }
    // 4: the workspace
    const int64_t off[] = {P.off_member, P.off_label, P.off_keys, P.off_dense, P.off_padded, P.off_block, P.workspace_bytes};
    const int64_t need[] = {P.rows_padded, P.rows_padded * 4, P.rows_padded * 16, P.rows_padded * L * 8, P.rows_padded * P.Lpad * 8, P.block_bytes};
    CHECK(off[0] == 0, "the member flags lead the workspace");
    for (int k = 0; k < 6; ++k)
        CHECK(off[k] % 256 == 0 && off[k] + need[k] <= off[k + 1], "piece %d: offset %lld, %lld bytes, next %lld", k, (long long)off[k], (long long)need[k],
              (long long)off[k + 1]);
    CHECK(P.workspace_bytes <= P.workspace_bound, "workspace %lld beyond its bound %lld", (long long)P.workspace_bytes, (long long)P.workspace_bound);
    CHECK(P.workspace_bound == (n + 63) * ((L + P.Lpad) * 8 + 21) + (P.general ? kLooBlockBytes : 0) + 6 * 256, "the stated bound");
}

static void refusal(const char *what, const LooPlan &P, int rc, const char *needle) {
    CHECK(P.rc == rc && strstr(P.msg, needle) != nullptr, "%s: rc %d, message \"%s\" (want %d, \"%s\")", what, P.rc, P.msg, rc, needle);
}

int main() {
    const int64_t sizes[] = {0, 1, 2, 63, 64, 65, 129, 200, 4097, 65536};
    for (int64_t n : sizes)
        for (int general = 0; general < 2; ++general) {
            check_plan(n, 110, 15, general != 0);
            check_plan(n, 25, 15, general != 0);
            check_plan(n, 25, 15, general != 0, true);
        }
    // sizes around the general route's block edges (96 MiB / 4 B / rows_padded), the unbanded route, and the rest of the ladder
    for (int64_t n : {128, 5016, 5017, 5056, 5057, 5120, 5121, 8192, 16384, 16385, 24576, 24577, 40000, 65535}) {
        check_plan(n, 110, 0, false);    // unbanded: effective window 110 -> general
        check_plan(n, 40, 3, n % 2 == 0);
        check_plan(n, 110, 33, false);
    }
    check_plan(200, 110, 32, false);
    check_plan(200, 110, 16, false);
    check_plan(200, 110, 8, false);
    // 5: the keys keep the rule's order: distance first (+inf behind every finite value), then the lower row; "no candidate" last
    {
        const uint32_t zero = 0u, tiny = 1u, one = 0x3f800000u, big = 0x7f7fffffu, inf = 0x7f800000u;
        CHECK(loo_key(zero, 5) < loo_key(tiny, 0) && loo_key(tiny, 65535) < loo_key(one, 0) && loo_key(one, 7) < loo_key(big, 0) &&
                  loo_key(big, 65535) < loo_key(inf, 0),
              "distance order");
        CHECK(loo_key(one, 3) < loo_key(one, 4) && loo_key(inf, 0) < loo_key(inf, 1) && loo_key(inf, 65535) < kLooNoKey, "ties and the end");
        CHECK((uint32_t)(loo_key(one, 65535) & 0xffffffffu) == 65535u && (uint32_t)(loo_key(one, 65535) >> 32) == one, "unpack");
    }
    // refusals
    refusal("cap + 1", loo_plan(65537, 110, 15, true, false, false), WDX_ERR_UNSUPPORTED, "n = 65537 rows, more than WDX_SELF_MATRIX_MAX_ROWS = 65536");
    refusal("cap + 1, general", loo_plan(65537, 25, 15, true, true, false), WDX_ERR_UNSUPPORTED, "n = 65537 rows");
    refusal("L 0", loo_plan(10, 0, 15, true, false, false), WDX_ERR_INVALID, "L must be at least 1, not 0");
    refusal("L -4", loo_plan(10, -4, 15, true, false, false), WDX_ERR_INVALID, "L must be at least 1, not -4");
    refusal("n -1", loo_plan(-1, 25, 15, true, false, false), WDX_ERR_INVALID, "n must not be negative (n = -1)");
    refusal("no output", loo_plan(10, 25, 15, false, false, false), WDX_ERR_INVALID, "the outputs nn and best are required");
    CHECK(loo_plan(0, 25, 15, false, false, false).rc == WDX_SUCCESS, "an empty call without outputs");
    // the route rule, with WDX_OPT_NO_SHORT_DTW
    CHECK(loo_plan(100, 25, 15, true, false, false).kernel == MedoidKernel::kShort && loo_plan(100, 25, 15, true, false, true).kernel == MedoidKernel::kBand15 &&
              loo_plan(100, 110, 33, true, false, false).general && loo_plan(100, 110, 15, true, true, false).general &&
              loo_plan(100, 110, 0, true, false, false).general,
          "routes");
    printf("checks %lld\nfailures %lld\nplans %lld\ntiles %lld\nat_cap %lld\npair_checked %lld\nblocks %lld\ngeneral %lld\nmulti_block %lld\n", g_checks,
           g_fail, g_plans, g_tiles, g_at_cap, g_pair_checked, g_blocks, g_general, g_multi_block);
    return g_fail ? 1 : 0;
}
