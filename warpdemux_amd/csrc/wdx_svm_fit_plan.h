// The batched SMO solver of the one-vs-one C-SVC duals (include/wdx.h: wdx_svm_solve_device states the rule): what a call does
// with its problems, before anything is launched -- the one statement of it (plain C++17: no device runtime, nothing of the
// context, so the system compiler builds it alone: tests/host/svm_fit_plan_check.cpp).  wdx_svm_fit.hip launches what the plan names.
//
//   problems   one WORKGROUP per problem; the grid takes them by falling row count (equal counts: by rising problem number), so the
//              long solves start first and the short ones fill the CUs behind them
//   kernel     ONE launch, and one instantiation for all its workgroups: the smallest of kSvmFitKernels whose capacity
//              (threads x rows per thread) holds the LARGEST problem of the call
//   rows       row t of a problem belongs to thread t % threads, as that thread's slot t / threads: G_t (float64) and the two bits
//              "alpha_t is at 0 / at C_t" stay in that thread's registers for the whole solve
//   LDS        8 B per row of capacity -- the row's K index (int32) and its diagonal entry K_tt (float32) during the solve, then the
//              same bytes as one float64 per row (v_t for rho, alpha_t y_t for the decision values) -- plus kSvmFitScratchBytes for
//              the reductions and the hand-over of the pair
//
// THE CAP.  WDX_SVM_FIT_MAX_ROWS = 16 384 = 1 024 threads x 16 rows: 16 384 x 8 B = 128 KiB of the CU's 160 KiB of LDS (the
// scratch bytes on top), and 16 float64 G_t = 32 of the 128 vector registers a lane of a 1 024-thread workgroup has (with alpha_t
// beside them, 64, the kernel spilled: the compiler's report, so alpha_t's value stays in the caller's array).  A longer problem is
// refused (WDX_ERR_INVALID) before anything is launched.
//
// TABLES (context-owned device workspace, grow-only; SvmFitPlan::table_bytes, checked by the host program): the grid's records
// (SvmFitProb, 48 B each), the row lists and the evaluation lists as the caller gave them (int32), 256 B of alignment per piece:
//   table_bytes <= 48 n_problems + 4 (n_rows + n_eval) + 3 x 256
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/wdx.h"

namespace wdx {

constexpr int64_t kSvmFitMaxRows = WDX_SVM_FIT_MAX_ROWS;
constexpr int64_t kSvmFitLdsPerCu = 160 * 1024;
constexpr int64_t kSvmFitScratchBytes = 1024;   // (wdx_svm_fit.hip: SvmFitScratch, static_assert'ed there)

struct SvmFitKernel { int threads, rows_per_thread; };
constexpr int kSvmFitKernelCount = 3;
constexpr SvmFitKernel kSvmFitKernels[kSvmFitKernelCount] = {{64, 4}, {256, 8}, {1024, 16}};
constexpr int64_t svm_fit_capacity(int k) { return (int64_t)kSvmFitKernels[k].threads * kSvmFitKernels[k].rows_per_thread; }
constexpr int64_t svm_fit_lds_bytes(int k) { return 8 * svm_fit_capacity(k) + kSvmFitScratchBytes; }
static_assert(svm_fit_capacity(kSvmFitKernelCount - 1) == kSvmFitMaxRows, "the largest kernel serves the cap");
static_assert(svm_fit_lds_bytes(kSvmFitKernelCount - 1) <= kSvmFitLdsPerCu, "the largest kernel fits the CU's LDS");
static_assert(svm_fit_capacity(0) < svm_fit_capacity(1) && svm_fit_capacity(1) < svm_fit_capacity(2), "rising capacities");

// One workgroup's problem as the kernel reads it (device memory; q = the caller's problem number, where its outputs go)
struct SvmFitProb {
    int64_t row0, eval0;
    int32_t n_pos, n_neg, n_eval, q;
    double c_pos, c_neg;
};
static_assert(sizeof(SvmFitProb) == 48, "the table's record");

inline int64_t svm_fit_align(int64_t b) { return (b + 255) / 256 * 256; }

struct SvmFitPlan {
    int rc = WDX_SUCCESS;
    char msg[224] = {0};
    int64_t m = 0, ld = 0, n_problems = 0, n_rows = 0, n_eval = 0, max_iter = 0;
    double eps = 0;
    int kernel = 0;                   // index into kSvmFitKernels
    int64_t largest = 0;              // rows of the largest problem
    std::vector<SvmFitProb> grid;     // workgroup b solves grid[b]
    int64_t off_probs = 0, off_rows = 0, off_eval = 0, table_bytes = 0, table_bound = 0;

    int threads() const { return kSvmFitKernels[kernel].threads; }
    int64_t capacity() const { return svm_fit_capacity(kernel); }
    int64_t lds_bytes() const { return svm_fit_lds_bytes(kernel); }
};

// Every array is HOST memory.  have_K / have_out: the matrix and the four (with evaluation rows: five) outputs are there.
inline SvmFitPlan svm_fit_plan(int64_t m, int64_t ld, const wdx_svm_problem *problems, int64_t n_problems, const int32_t *rows, int64_t n_rows,
                               const int32_t *eval_rows, int64_t n_eval, double eps, int64_t max_iter, bool have_K, bool have_out,
                               bool have_dec) {
    SvmFitPlan P;
    auto refuse = [&P](int rc) -> SvmFitPlan & {
        P.rc = rc;
        P.grid.clear();
        return P;
    };
#define WDX_SVM_FIT_REFUSE(...)                        \
    do {                                               \
        snprintf(P.msg, sizeof P.msg, __VA_ARGS__);    \
        return refuse(WDX_ERR_INVALID);                \
    } while (0)
    if (m < 1) WDX_SVM_FIT_REFUSE("svm solve: m must be at least 1, not %lld", (long long)m);
    if (ld < m) WDX_SVM_FIT_REFUSE("svm solve: ld = %lld is less than m = %lld", (long long)ld, (long long)m);
    if (n_problems < 0 || n_rows < 0 || n_eval < 0)
        WDX_SVM_FIT_REFUSE("svm solve: negative count (n_problems = %lld, n_rows = %lld, n_eval = %lld)", (long long)n_problems, (long long)n_rows,
                           (long long)n_eval);
    if (!(eps > 0) || !isfinite(eps)) WDX_SVM_FIT_REFUSE("svm solve: eps must be positive and finite, not %g", eps);
    if (max_iter < 0) WDX_SVM_FIT_REFUSE("svm solve: max_iter must not be negative (max_iter = %lld)", (long long)max_iter);
    if (n_problems > INT32_MAX) {
        snprintf(P.msg, sizeof P.msg, "svm solve: %lld problems, more than one launch takes", (long long)n_problems);
        return refuse(WDX_ERR_UNSUPPORTED);
    }
    P.m = m, P.ld = ld, P.n_problems = n_problems, P.n_rows = n_rows, P.n_eval = n_eval, P.eps = eps, P.max_iter = max_iter;
    if (n_problems == 0) return P;
    if (!problems || (n_rows > 0 && !rows) || (n_eval > 0 && !eval_rows)) WDX_SVM_FIT_REFUSE("svm solve: the problem table and its lists are required (NULL given)");
    if (!have_K) WDX_SVM_FIT_REFUSE("svm solve: the kernel matrix is required (NULL given)");
    if (!have_out) WDX_SVM_FIT_REFUSE("svm solve: alpha, rho, n_iter and state are required (NULL given)");
    P.grid.reserve((size_t)n_problems);
    for (int64_t q = 0; q < n_problems; ++q) {
        const wdx_svm_problem &S = problems[q];
        if (S.n_pos < 1 || S.n_neg < 1)
            WDX_SVM_FIT_REFUSE("svm solve: problem %lld has an empty side (n_pos = %d, n_neg = %d)", (long long)q, S.n_pos, S.n_neg);
        const int64_t n = (int64_t)S.n_pos + S.n_neg;
        if (n > kSvmFitMaxRows)
            WDX_SVM_FIT_REFUSE("svm solve: problem %lld has %lld rows, more than WDX_SVM_FIT_MAX_ROWS = %lld", (long long)q, (long long)n,
                               (long long)kSvmFitMaxRows);
        if (S.row0 < 0 || S.row0 > n_rows - n)
            WDX_SVM_FIT_REFUSE("svm solve: problem %lld: rows %lld .. %lld lie outside the row list of %lld", (long long)q, (long long)S.row0,
                               (long long)(S.row0 + n), (long long)n_rows);
        if (S.n_eval < 0 || S.eval0 < 0 || S.eval0 > n_eval - S.n_eval)
            WDX_SVM_FIT_REFUSE("svm solve: problem %lld: evaluation rows %lld .. %lld lie outside the evaluation list of %lld", (long long)q,
                               (long long)S.eval0, (long long)(S.eval0 + S.n_eval), (long long)n_eval);
        if (S.n_eval > 0 && !have_dec) WDX_SVM_FIT_REFUSE("svm solve: problem %lld has evaluation rows and dec is NULL", (long long)q);
        if (!(S.c_pos > 0) || !isfinite(S.c_pos) || !(S.c_neg > 0) || !isfinite(S.c_neg))
            WDX_SVM_FIT_REFUSE("svm solve: problem %lld: c_pos = %g, c_neg = %g must be positive and finite", (long long)q, S.c_pos, S.c_neg);
        for (int64_t t = 0; t < n; ++t)
            if (rows[S.row0 + t] < 0 || rows[S.row0 + t] >= m)
                WDX_SVM_FIT_REFUSE("svm solve: problem %lld: row %lld is K row %d, outside 0 .. %lld", (long long)q, (long long)t, rows[S.row0 + t],
                                   (long long)(m - 1));
        for (int64_t e = 0; e < S.n_eval; ++e)
            if (eval_rows[S.eval0 + e] < 0 || eval_rows[S.eval0 + e] >= m)
                WDX_SVM_FIT_REFUSE("svm solve: problem %lld: evaluation row %lld is K row %d, outside 0 .. %lld", (long long)q, (long long)e,
                                   eval_rows[S.eval0 + e], (long long)(m - 1));
        P.largest = std::max(P.largest, n);
        P.grid.push_back(SvmFitProb{S.row0, S.eval0, S.n_pos, S.n_neg, S.n_eval, (int32_t)q, S.c_pos, S.c_neg});
    }
#undef WDX_SVM_FIT_REFUSE
    std::stable_sort(P.grid.begin(), P.grid.end(),
                     [](const SvmFitProb &a, const SvmFitProb &b) { return (int64_t)a.n_pos + a.n_neg > (int64_t)b.n_pos + b.n_neg; });
    while (svm_fit_capacity(P.kernel) < P.largest) ++P.kernel;
    int64_t at = 0;
    auto piece = [&at](int64_t bytes) {
        const int64_t o = at;
        at += svm_fit_align(bytes);
        return o;
    };
    P.off_probs = piece(n_problems * (int64_t)sizeof(SvmFitProb));
    P.off_rows = piece(n_rows * (int64_t)sizeof(int32_t));
    P.off_eval = piece(n_eval * (int64_t)sizeof(int32_t));
    P.table_bytes = at;
    P.table_bound = n_problems * (int64_t)sizeof(SvmFitProb) + 4 * (n_rows + n_eval) + 3 * 256;
    return P;
}

}  // namespace wdx
