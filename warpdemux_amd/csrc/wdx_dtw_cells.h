// The cell machinery of the lane-per-pair DTW kernels (wdx_dtw.hip: dtw_band_kernel, dtw_short_kernel, dtw_short_svm_kernel;
// wdx_dtw_tile.h for the one-wave-per-tile kernels of wdx_medoid.hip and wdx_dtw_self.hip): the band row, the unrolled short
// rows, the fused cell and the settle decision.  Device code only; every unit that includes it is compiled with
// -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <utility>

namespace wdx {

#define WDX_INF __builtin_huge_val()

// v_min_f64 without the canonicalising v_max_f64 x,x that fmin() costs per call in IEEE mode when
// the compiler cannot prove an operand quiet (the loop-carried band registers).  The operands here
// are always results of float64 adds, +0.0 or +inf -- never signalling NaNs; NaN inputs are
// handled by the per-series flags, not by the recurrence.
__device__ __forceinline__ double min_f64(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// FMA: the cell as ONE v_fma_f64, (x - y)^2 + t with a single rounding -- five float64 operations per cell instead of
// six.  Not the reference's bits cell by cell: see dtw_unsettled() for how the kernels return the reference's float32.
template <bool FMA>
__device__ __forceinline__ double dtw_cell(double d, double t) {
    if constexpr (FMA) return __builtin_fma(d, d, t);
    else return d * d + t;
}

template <int W, bool MASKED, bool FMA = false>
__device__ __forceinline__ void dtw_row(double (&r)[2 * W - 1], double x,
                                        const double *__restrict__ yi, double p2, int jbase,
                                        int jlo, int jhi) {
    constexpr int B = 2 * W - 1;
    double left = WDX_INF;
#pragma unroll
    for (int c = 0; c < B; ++c) {
        const double d = x - yi[c];
        double up = (c + 1 < B) ? r[c + 1] : WDX_INF;
        double t = (c == 0 ? up : min_f64(up, left)) + p2;  // left of the first band cell is +inf
        t = min_f64(t, r[c]);
        double v = dtw_cell<FMA>(d, t);
        if (MASKED) {
            int j = jbase + c;
            v = (j < jlo || j > jhi) ? WDX_INF : v;
        }
        r[c] = v;
        left = v;
    }
}

// dtw_row with a compile-time range [CLO, CHI] of band cells that lie inside the matrix: the head and tail
// rows of the band without masks, and without touching the cells outside (head: they stay +inf; tail:
// they go stale but are never read again).
template <int W, int CLO, int CHI, bool FMA = false>
__device__ __forceinline__ void dtw_row_ct(double (&r)[2 * W - 1], double x, const double *__restrict__ yi,
                                           double p2) {
    constexpr int B = 2 * W - 1;
    double left = WDX_INF;
#pragma unroll
    for (int c = CLO; c <= CHI; ++c) {
        const double d = x - yi[c];
        const double up = (c + 1 < B) ? r[c + 1 < B ? c + 1 : 0] : WDX_INF;
        double t = (c == CLO ? up : min_f64(up, left)) + p2;
        t = min_f64(t, r[c]);
        const double v = dtw_cell<FMA>(d, t);
        r[c] = v;
        left = v;
    }
}
// head rows i = 0 .. W-2 (band cells c >= W-1-i), tail rows i = L-W+1+t, t = 0 .. W-2 (c <= 2W-3-t)
template <int W, bool FMA, int... Is>
__device__ __forceinline__ void dtw_head_rows(double (&r)[2 * W - 1], const double *__restrict__ xp, int64_t ldA,
                                              const double *__restrict__ y, double p2,
                                              std::integer_sequence<int, Is...>) {
    (dtw_row_ct<W, W - 1 - Is, 2 * W - 2, FMA>(r, xp[(int64_t)Is * ldA], y + Is, p2), ...);
}
template <int W, bool FMA, int... Ts>
__device__ __forceinline__ void dtw_tail_rows(double (&r)[2 * W - 1], const double *__restrict__ xp, int64_t ldA,
                                              const double *__restrict__ y, double p2, int i0,
                                              std::integer_sequence<int, Ts...>) {
    (dtw_row_ct<W, 0, 2 * W - 3 - Ts, FMA>(r, xp[(int64_t)(i0 + Ts) * ldA], y + i0 + Ts, p2), ...);
}

// The fused cell and the reference's float32 (dtw_band_kernel, dtw_short_kernel, dtw_short_svm_kernel).
// Every kernel first runs the pair on fused cells (FMA = true).  With u = 2^-53: the reference's cell is
// fl(fl(d^2) + t), the fused one fl(d^2 + t'), d the same number in both; all values are non-negative, min and the
// rounding are monotone, so if the three predecessor cells agree within a relative e the sums min(..) + p2 agree within
// e + 2u and the cells within e + 5u (first order) -- a cell's predecessors lie one step of i + j earlier, hence the final
// cells agree within (2 L - 1) 5u (1 + o(1)), and their correctly rounded square roots within half of that + 2u.  The
// kernels take delta = 32 (L + 1) u (more than three times that): when [res (1 - delta), res (1 + delta)] rounds to one
// float32, the reference's distance is that float32 (float conversion is monotone).  Otherwise -- a float32 rounding
// boundary inside the interval: about one pair in 10^5 at L = 110 -- or when the sum left [1e-280, 1e280] (underflow
// makes errors absolute; zero is exact: a zero fused sum means every term on its path was below 2^-1074 in both forms),
// the WAVE runs the pair again on the reference's six operations and the flagged lanes take that result.  Returns the
// lanes to settle.
__device__ __forceinline__ bool dtw_unsettled(double Dv, double res, float f, double delta) {
    const bool same = (float)(res * (1.0 - delta)) == f && (float)(res * (1.0 + delta)) == f;
    const bool mid = Dv == 0.0 || (Dv > 1e-280 && Dv < 1e280);
    return !(same && mid);
}
__device__ __forceinline__ double dtw_delta(int L) { return 32.0 * (double)(L + 1) * 0x1p-53; }
// WDX_OPT_DTW_UNFUSED (the kernels' `unfused` argument): 0 as above | 1 the reference's six operations only | 2 fused, and
// every pair is run again (tests: the second pass and the selection) | 3 fused, never run again (diagnostic: how often the
// fused float32 differs -- NOT the reference's results)
__device__ __forceinline__ bool dtw_redo(int mode, bool unsettled) {
    if (mode == 2) return true;
    if (mode == 3) return false;
    return __ballot(unsettled) != 0ull;
}

// Short series, fully unrolled (the shipped DTW_SVM models: 25-point fingerprints, window 15, penalty 0.1
// -- every model under warpdemux/models/model_files/).  One lane per query series, the DP column
// vector D[L] and the query x[L] in registers, the reference uniform across the wave (scalar loads);
// rows and columns are compile-time, so the band limits cost nothing and only cells inside the band
// are computed (515 of the 725 that the rolling-band kernel evaluates for L = 25, all of them with
// masks there).  Same float64 operations per cell as dtw_row -> identical bits.
// row I of the short-series DP; everything about the band is a compile-time constant
template <int L, int W, int I, bool FMA>
__device__ __forceinline__ void dtw_short_row(double (&D)[L], const double xi, const double *__restrict__ y,
                                              const double p2) {
    constexpr int jlo = I - (W - 1) > 0 ? I - (W - 1) : 0;
    constexpr int jhi = I + (W - 1) < L - 1 ? I + (W - 1) : L - 1;
    double left = WDX_INF;
    double diag = jlo == 0 ? (I == 0 ? 0.0 : WDX_INF) : D[jlo > 0 ? jlo - 1 : 0];
#pragma unroll
    for (int j = jlo; j <= jhi; ++j) {
        const double up = D[j];
        const double d = xi - y[j];
        // min(min(up, left) + p2, diag) == min(min(up + p2, diag), left + p2) (rounding is monotone): the part that
        // does not depend on the cell to the left is off the row's dependency chain (3 dependent ops per cell, not 4)
        double t = __builtin_fmin(up + p2, diag);
        if (j != jlo) t = __builtin_fmin(t, left + p2);
        const double v = dtw_cell<FMA>(d, t);
        diag = up;
        D[j] = v;
        left = v;
    }
}
template <int L, int W, bool FMA, int... Is>
__device__ __forceinline__ void dtw_short_rows(double (&D)[L], const double (&x)[L], const double *__restrict__ y,
                                               const double p2, std::integer_sequence<int, Is...>) {
    (dtw_short_row<L, W, Is, FMA>(D, x[Is], y, p2), ...);
}
// the pair's distance as float64, the reference's float32 after conversion (see dtw_unsettled)
template <int L, int W>
__device__ __forceinline__ double dtw_short_pair(const double (&x)[L], const double *__restrict__ y, const double p2,
                                                 const bool pnan, const double delta, const int unfused) {
    double res;
    bool redo = unfused == 1;   // (uniform)
    if (!redo) {
        double D[L];
#pragma unroll
        for (int j = 0; j < L; ++j) D[j] = WDX_INF;
        dtw_short_rows<L, W, true>(D, x, y, p2, std::make_integer_sequence<int, L>{});
        res = sqrt(D[L - 1]);
        redo = dtw_redo(unfused, !pnan && dtw_unsettled(D[L - 1], res, (float)res, delta));
    }
    if (redo) {
        double D[L];
#pragma unroll
        for (int j = 0; j < L; ++j) D[j] = WDX_INF;
        dtw_short_rows<L, W, false>(D, x, y, p2, std::make_integer_sequence<int, L>{});
        res = sqrt(D[L - 1]);
    }
    return pnan ? __builtin_nan("") : res;
}

}  // namespace wdx
