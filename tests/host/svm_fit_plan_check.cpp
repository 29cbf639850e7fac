// What a batched SMO solve does with its problems (warpdemux_amd/csrc/wdx_svm_fit_plan.h), checked without a GPU: built with the
// system compiler under the address and undefined-behaviour sanitizers and run by tests/test_svm_fit_plan_host.py.
// Over batches of 1 .. 3 000 problems of 2 .. 16 384 rows it checks of every plan:
//   1  the grid holds every problem exactly once, by falling row count and, among equal counts, rising problem number, with the
//      caller's ranges, sides and bounds
//   2  the instantiation is the smallest whose capacity holds the largest problem, and every problem fits it; the thresholds sit
//      at 256 / 257, 2 048 / 2 049 and 16 384 rows
//   3  the LDS of the instantiation is 8 B per row of capacity plus the scratch bytes, within 160 KiB; the cap is the largest capacity
//   4  the pieces of the table lie inside its stated size, and that within the stated bound
// and that each refusal carries its code and message and leaves an empty grid.  Prints "checks <n>" / "failures <n>" and what the
// sweep met.
#include "wdx_svm_fit_plan.h"

#include <stdio.h>
#include <string.h>

#include <limits>
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

static long long g_plans = 0, g_problems = 0, g_at_cap = 0, g_kernels[3] = {0, 0, 0}, g_refusals = 0;

struct Batch {
    std::vector<wdx_svm_problem> probs;
    std::vector<int32_t> rows, evals;
    int64_t m = 0;
    void add(int32_t n_pos, int32_t n_neg, int32_t n_eval, double cp = 1.0, double cn = 2.0) {
        wdx_svm_problem S;
        memset(&S, 0, sizeof S);
        S.row0 = (int64_t)rows.size(), S.eval0 = (int64_t)evals.size(), S.n_pos = n_pos, S.n_neg = n_neg, S.n_eval = n_eval, S.c_pos = cp, S.c_neg = cn;
        for (int32_t t = 0; t < n_pos + n_neg; ++t) rows.push_back((int32_t)((t * 7 + (int64_t)probs.size()) % m));
        for (int32_t e = 0; e < n_eval; ++e) evals.push_back((int32_t)((m - 1 - e) % m));
        probs.push_back(S);
    }
    SvmFitPlan plan(int64_t ld = -1, double eps = 1e-3, int64_t max_iter = 1000, bool K = true, bool out = true, bool dec = true) const {
        return svm_fit_plan(m, ld < 0 ? m : ld, probs.data(), (int64_t)probs.size(), rows.data(), (int64_t)rows.size(), evals.data(),
                            (int64_t)evals.size(), eps, max_iter, K, out, dec);
    }
};

static void check_plan(const Batch &B, int64_t ld) {
    const SvmFitPlan P = B.plan(ld);
    CHECK(P.rc == WDX_SUCCESS, "rc %d: %s", P.rc, P.msg);
    if (P.rc != WDX_SUCCESS) return;
    ++g_plans;
    const int64_t Q = (int64_t)B.probs.size();
    g_problems += Q;
    CHECK((int64_t)P.grid.size() == Q && P.n_problems == Q && P.ld == ld && P.m == B.m, "sizes");
    // 1: the grid
    std::vector<uint8_t> seen((size_t)Q, 0);
    int64_t largest = 0;
    for (int64_t b = 0; b < Q; ++b) {
        const SvmFitProb &G = P.grid[(size_t)b];
        const bool ok = G.q >= 0 && G.q < Q && !seen[(size_t)G.q];
        CHECK(ok, "workgroup %lld solves problem %d", (long long)b, G.q);
        if (!ok) continue;
        seen[(size_t)G.q] = 1;
        const wdx_svm_problem &S = B.probs[(size_t)G.q];
        CHECK(G.row0 == S.row0 && G.eval0 == S.eval0 && G.n_pos == S.n_pos && G.n_neg == S.n_neg && G.n_eval == S.n_eval && G.c_pos == S.c_pos &&
                  G.c_neg == S.c_neg,
              "workgroup %lld: not the caller's problem %d", (long long)b, G.q);
        const int64_t n = (int64_t)G.n_pos + G.n_neg;
        largest = n > largest ? n : largest;
        if (b > 0) {
            const SvmFitProb &H = P.grid[(size_t)b - 1];
            const int64_t before = (int64_t)H.n_pos + H.n_neg;
            CHECK(before > n || (before == n && H.q < G.q), "workgroups %lld, %lld: %lld rows (problem %d) then %lld rows (problem %d)", (long long)b - 1,
                  (long long)b, (long long)before, H.q, (long long)n, G.q);
        }
        CHECK(n <= P.capacity(), "workgroup %lld: %lld rows in a capacity of %lld", (long long)b, (long long)n, (long long)P.capacity());
    }
    // 2: the instantiation
    CHECK(P.largest == largest, "largest %lld, not %lld", (long long)P.largest, (long long)largest);
    CHECK(P.kernel >= 0 && P.kernel < kSvmFitKernelCount && svm_fit_capacity(P.kernel) >= largest && (P.kernel == 0 || svm_fit_capacity(P.kernel - 1) < largest),
          "instantiation %d for %lld rows", P.kernel, (long long)largest);
    ++g_kernels[P.kernel];
    if (largest == kSvmFitMaxRows) ++g_at_cap;
    CHECK(P.threads() == kSvmFitKernels[P.kernel].threads && P.threads() % 64 == 0 && P.threads() <= 1024, "threads %d", P.threads());
    // 3: LDS
    CHECK(P.lds_bytes() == 8 * P.capacity() + kSvmFitScratchBytes && P.lds_bytes() <= 160 * 1024, "LDS %lld", (long long)P.lds_bytes());
    // 4: the table
    const int64_t off[] = {P.off_probs, P.off_rows, P.off_eval, P.table_bytes};
    const int64_t need[] = {Q * 48, (int64_t)B.rows.size() * 4, (int64_t)B.evals.size() * 4};
    CHECK(off[0] == 0, "the records lead the table");
    for (int k = 0; k < 3; ++k)
        CHECK(off[k] % 256 == 0 && off[k] + need[k] <= off[k + 1], "piece %d: offset %lld, %lld bytes, next %lld", k, (long long)off[k], (long long)need[k],
              (long long)off[k + 1]);
    CHECK(P.table_bytes <= P.table_bound && P.table_bound == Q * 48 + 4 * (int64_t)(B.rows.size() + B.evals.size()) + 3 * 256, "table %lld, bound %lld",
          (long long)P.table_bytes, (long long)P.table_bound);
}

static void refusal(const char *what, const SvmFitPlan &P, int rc, const char *needle) {
    ++g_refusals;
    CHECK(P.rc == rc && strstr(P.msg, needle) != nullptr && P.grid.empty(), "%s: rc %d, message \"%s\" (want %d, \"%s\")", what, P.rc, P.msg, rc, needle);
}

int main() {
    // the constants
    CHECK(kSvmFitMaxRows == 16384 && svm_fit_capacity(0) == 256 && svm_fit_capacity(1) == 2048 && svm_fit_capacity(2) == 16384, "capacities");
    CHECK(svm_fit_lds_bytes(2) == 128 * 1024 + 1024, "the largest instantiation's LDS");
    // single problems around every threshold
    for (int32_t n : {2, 3, 63, 64, 65, 129, 255, 256, 257, 513, 1025, 2047, 2048, 2049, 4097, 16383, 16384}) {
        Batch B;
        B.m = 20000;
        B.add(n / 2, n - n / 2, n % 5);
        check_plan(B, 20000);
        check_plan(B, 20037);
        const SvmFitPlan P = B.plan();
        CHECK(P.kernel == (n <= 256 ? 0 : n <= 2048 ? 1 : 2), "%d rows on instantiation %d", n, P.kernel);
    }
    // batches: a fit's shape (pairs and folds of similar sizes), many small problems, one large among small ones, equal sizes
    {
        Batch B;
        B.m = 4096;
        for (int p = 0; p < 45; ++p) {
            B.add(400 + p, 410, 0);
            for (int f = 0; f < 5; ++f) B.add(320 + p - f, 328, 162);
        }
        check_plan(B, 4096);
    }
    {
        Batch B;
        B.m = 64;
        for (int q = 0; q < 3000; ++q) B.add(1 + q % 4, 1 + (q / 4) % 4, q % 3);
        check_plan(B, 64);
    }
    {
        Batch B;
        B.m = 16384;
        for (int q = 0; q < 10; ++q) B.add(3, 4, 1);
        B.add(8192, 8192, 7);
        for (int q = 0; q < 10; ++q) B.add(100, 100, 0);
        check_plan(B, 16384);
        const SvmFitPlan P = B.plan();
        CHECK(P.grid[0].q == 10 && P.kernel == 2 && P.grid[1].q == 11 && P.grid[11].q == 0, "the large problem leads the grid");
    }
    {
        Batch B;   // an empty batch is a plan with nothing to launch
        B.m = 10;
        const SvmFitPlan P = B.plan();
        CHECK(P.rc == WDX_SUCCESS && P.grid.empty() && P.table_bytes == 0, "an empty batch");
        CHECK(svm_fit_plan(10, 10, nullptr, 0, nullptr, 0, nullptr, 0, 1e-3, 10, false, false, false).rc == WDX_SUCCESS, "an empty batch without arrays");
    }
    // refusals
    {
        Batch G;
        G.m = 100;
        G.add(10, 12, 3);
        refusal("m 0", svm_fit_plan(0, 0, G.probs.data(), 1, G.rows.data(), 22, G.evals.data(), 3, 1e-3, 10, true, true, true), WDX_ERR_INVALID, "m must be at least 1, not 0");
        refusal("ld < m", G.plan(99), WDX_ERR_INVALID, "ld = 99 is less than m = 100");
        refusal("eps 0", G.plan(-1, 0.0), WDX_ERR_INVALID, "eps must be positive and finite");
        refusal("eps nan", G.plan(-1, std::numeric_limits<double>::quiet_NaN()), WDX_ERR_INVALID, "eps must be positive and finite");
        refusal("eps inf", G.plan(-1, std::numeric_limits<double>::infinity()), WDX_ERR_INVALID, "eps must be positive and finite");
        refusal("max_iter -1", G.plan(-1, 1e-3, -1), WDX_ERR_INVALID, "max_iter must not be negative (max_iter = -1)");
        refusal("no K", G.plan(-1, 1e-3, 10, false), WDX_ERR_INVALID, "the kernel matrix is required");
        refusal("no outputs", G.plan(-1, 1e-3, 10, true, false), WDX_ERR_INVALID, "alpha, rho, n_iter and state are required");
        refusal("no dec", G.plan(-1, 1e-3, 10, true, true, false), WDX_ERR_INVALID, "problem 0 has evaluation rows and dec is NULL");
        refusal("no table", svm_fit_plan(100, 100, nullptr, 1, G.rows.data(), 22, G.evals.data(), 3, 1e-3, 10, true, true, true), WDX_ERR_INVALID,
                "the problem table and its lists are required");
        refusal("negative count", svm_fit_plan(100, 100, G.probs.data(), -1, G.rows.data(), 22, G.evals.data(), 3, 1e-3, 10, true, true, true), WDX_ERR_INVALID,
                "negative count");
        refusal("too many problems", svm_fit_plan(100, 100, G.probs.data(), (int64_t)1 << 31, G.rows.data(), 22, G.evals.data(), 3, 1e-3, 10, true, true, true),
                WDX_ERR_UNSUPPORTED, "more than one launch takes");
        auto with = [&G](auto change) {
            Batch B = G;
            change(B);
            return B.plan();
        };
        refusal("no positive row", with([](Batch &B) { B.probs[0].n_pos = 0; }), WDX_ERR_INVALID, "problem 0 has an empty side (n_pos = 0, n_neg = 12)");
        refusal("no negative row", with([](Batch &B) { B.probs[0].n_neg = 0; }), WDX_ERR_INVALID, "has an empty side (n_pos = 10, n_neg = 0)");
        refusal("negative side", with([](Batch &B) { B.probs[0].n_neg = -3; }), WDX_ERR_INVALID, "has an empty side");
        refusal("rows beyond the list", with([](Batch &B) { B.probs[0].row0 = 1; }), WDX_ERR_INVALID, "rows 1 .. 23 lie outside the row list of 22");
        refusal("negative row0", with([](Batch &B) { B.probs[0].row0 = -1; }), WDX_ERR_INVALID, "lie outside the row list");
        refusal("evaluation rows beyond the list", with([](Batch &B) { B.probs[0].n_eval = 4; }), WDX_ERR_INVALID, "lie outside the evaluation list of 3");
        refusal("negative n_eval", with([](Batch &B) { B.probs[0].n_eval = -1; }), WDX_ERR_INVALID, "lie outside the evaluation list");
        refusal("c 0", with([](Batch &B) { B.probs[0].c_pos = 0.0; }), WDX_ERR_INVALID, "must be positive and finite");
        refusal("c negative", with([](Batch &B) { B.probs[0].c_neg = -1.0; }), WDX_ERR_INVALID, "must be positive and finite");
        refusal("c inf", with([](Batch &B) { B.probs[0].c_neg = std::numeric_limits<double>::infinity(); }), WDX_ERR_INVALID, "must be positive and finite");
        refusal("c nan", with([](Batch &B) { B.probs[0].c_pos = std::numeric_limits<double>::quiet_NaN(); }), WDX_ERR_INVALID, "must be positive and finite");
        refusal("row m", with([](Batch &B) { B.rows[21] = 100; }), WDX_ERR_INVALID, "problem 0: row 21 is K row 100, outside 0 .. 99");
        refusal("row -1", with([](Batch &B) { B.rows[0] = -1; }), WDX_ERR_INVALID, "problem 0: row 0 is K row -1");
        refusal("evaluation row m", with([](Batch &B) { B.evals[2] = 100; }), WDX_ERR_INVALID, "evaluation row 2 is K row 100, outside 0 .. 99");
        Batch Two = G;   // the second problem is the bad one: the message names it
        Two.add(5, 5, 0, 1.0, -2.0);
        refusal("second problem", Two.plan(), WDX_ERR_INVALID, "problem 1: c_pos = 1, c_neg = -2 must be positive and finite");
    }
    {
        Batch B;   // one row beyond the cap
        B.m = 20000;
        B.add(8192, 8193, 0);
        refusal("cap + 1", B.plan(), WDX_ERR_INVALID, "problem 0 has 16385 rows, more than WDX_SVM_FIT_MAX_ROWS = 16384");
        Batch Big;   // sides whose sum leaves int32
        Big.m = 10;
        Big.add(1, 1, 0);
        Big.probs[0].n_pos = 2000000000, Big.probs[0].n_neg = 2000000000;
        refusal("huge sides", Big.plan(), WDX_ERR_INVALID, "has 4000000000 rows, more than WDX_SVM_FIT_MAX_ROWS");
    }
    printf("checks %lld\nfailures %lld\nplans %lld\nproblems %lld\nat_cap %lld\nkernel0 %lld\nkernel1 %lld\nkernel2 %lld\nrefusals %lld\n", g_checks, g_fail, g_plans,
           g_problems, g_at_cap, g_kernels[0], g_kernels[1], g_kernels[2], g_refusals);
    return g_fail ? 1 : 0;
}
