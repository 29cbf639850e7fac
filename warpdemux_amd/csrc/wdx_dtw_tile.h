// What the one-wave-per-tile kernels share (wdx_medoid.hip: medoid_tile_kernel; wdx_dtw_self.hip: self_tile_kernel): the pre-pass
// that gathers rows into the padded layout, and one pair of (lane's row, uniform column) on the register-band machinery of
// wdx_dtw_cells.h.  Device code only; every unit that includes it is compiled with -ffp-contract=off.
#pragma once
#include "wdx_dtw_cells.h"

namespace wdx {

// ---- pre-pass: gather into the padded layout, member flags ----------------------------------------------------------------
// One wave per padded row p: X[order[p]] -> dense[p] (L samples) and padded[p] (Lpad samples, zero halo); a padding row
// (order -1) is zeros.  member[p] = a caller's row, status 0 (if given), all L samples finite.
// IDENTITY: no order array -- padded row p is the caller's row p while p < n, padding behind.
// PADDED false: the dense form alone (`padded` is not written: wdx_dba.hip, whose uniform operand is the centre, not a row).
template <bool IDENTITY, bool PADDED = true>
__global__ __launch_bounds__(256) void tile_gather_kernel(const double *__restrict__ X, const int32_t *__restrict__ status,
                                                          const int32_t *__restrict__ order, int64_t n, int64_t rows, int L,
                                                          int64_t Lpad, int halo, double *__restrict__ dense,
                                                          double *__restrict__ padded, uint8_t *__restrict__ member) {
    const int64_t p = (int64_t)blockIdx.x * 4 + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (p >= rows) return;
    const int64_t src = IDENTITY ? (p < n ? p : -1) : (int64_t)order[p];
    bool bad = false;
    for (int64_t c = lane; c < Lpad; c += 64) {
        const int64_t s = c - halo;
        const bool in = s >= 0 && s < L;
        const double v = (in && src >= 0) ? X[src * L + s] : 0.0;
        if (PADDED) padded[p * Lpad + c] = v;
        if (in) {
            dense[p * L + s] = v;
            bad |= !(v - v == 0.0);   // NaN or an infinity
        }
    }
    const unsigned long long any_bad = __ballot(bad);
    if (lane == 0) member[p] = (src >= 0 && !any_bad && (!status || status[src] == 0)) ? 1 : 0;
}

// dtw_band_kernel's pair (row-major lanes): the accumulated cost D[L][L] on fused or on the reference's cells
template <int W, bool EXACT_W, bool FMA>
__device__ __forceinline__ double medoid_band_cost(const double *__restrict__ xp, const double *__restrict__ y, const int L,
                                                   const int w, const double p2) {
    constexpr int B = 2 * W - 1;
    double r[B];
#pragma unroll
    for (int c = 0; c < B; ++c) r[c] = WDX_INF;
    r[W - 1] = 0.0;
    double xn = xp[0];
    int i = 0;
    if (EXACT_W && L >= 2 * (W - 1)) {
        dtw_head_rows<W, FMA>(r, xp, 1, y, p2, std::make_integer_sequence<int, W - 1>{});
        i = W - 1;
        constexpr int CH = 8;
        const int body_end = L - W + 1;
        if (i + CH <= body_end) {
            double xc[CH];
#pragma unroll
            for (int k = 0; k < CH; ++k) xc[k] = xp[i + k];
            for (; i + CH <= body_end; i += CH) {
                double xq[CH];
                const bool more = i + 2 * CH <= body_end;  // wave-uniform
                if (more) {
#pragma unroll
                    for (int k = 0; k < CH; ++k) xq[k] = xp[i + CH + k];
                }
#pragma unroll
                for (int k = 0; k < CH; ++k) dtw_row<W, false, FMA>(r, xc[k], y + i + k, p2, 0, 0, 0);
                if (more) {
#pragma unroll
                    for (int k = 0; k < CH; ++k) xc[k] = xq[k];
                }
            }
        }
        if (i < body_end) xn = xp[i];
        for (; i < body_end; ++i) {
            const double x = xn;
            xn = xp[i + 1];  // i + 1 <= L - W + 1 < L
            dtw_row<W, false, FMA>(r, x, y + i, p2, 0, 0, 0);
        }
        dtw_tail_rows<W, FMA>(r, xp, 1, y, p2, L - W + 1, std::make_integer_sequence<int, W - 1>{});
    } else if (EXACT_W) {
        const int head_end = min(W - 1, L);
        const int body_end = max(head_end, L - W + 1);
        for (; i < head_end; ++i) {
            const double x = xn;
            if (i + 1 < L) xn = xp[i + 1];
            dtw_row<W, true, FMA>(r, x, y + i, p2, i - (W - 1), 0, L - 1);
        }
        for (; i < body_end; ++i) {
            const double x = xn;
            if (i + 1 < L) xn = xp[i + 1];
            dtw_row<W, false, FMA>(r, x, y + i, p2, 0, 0, 0);
        }
        for (; i < L; ++i) {
            const double x = xn;
            if (i + 1 < L) xn = xp[i + 1];
            dtw_row<W, true, FMA>(r, x, y + i, p2, i - (W - 1), 0, L - 1);
        }
    } else {
        for (; i < L; ++i) {
            const double x = xn;
            if (i + 1 < L) xn = xp[i + 1];
            dtw_row<W, true, FMA>(r, x, y + i, p2, i - (W - 1), max(0, i - (w - 1)), min(L - 1, i + (w - 1)));
        }
    }
    return r[W - 1];
}

// One pair as the band kernels settle it; `use`: the lane's value will be read (only those lanes ask for the second pass)
template <int W, bool EXACT_W>
__device__ __forceinline__ float medoid_band_pair(const double *__restrict__ xp, const double *__restrict__ y, const int L, const int w,
                                                  const double p2, const bool use, const double delta, const int unfused) {
    double res = 0.0;
    bool redo = unfused == 1;   // (uniform)
    if (!redo) {
        const double Dv = medoid_band_cost<W, EXACT_W, true>(xp, y, L, w, p2);
        res = sqrt(Dv);
        redo = dtw_redo(unfused, use && dtw_unsettled(Dv, res, (float)res, delta));
    }
    if (redo) res = sqrt(medoid_band_cost<W, EXACT_W, false>(xp, y, L, w, p2));
    return (float)res;
}

// The workgroup IS one wave: its LDS operations execute in program order, so a lane reads what another lane wrote by an earlier
// instruction without a barrier.  What is needed is that the compiler keeps that order (it does: the addresses may alias) and
// schedules nothing across.
__device__ __forceinline__ void medoid_wave_sync() { __builtin_amdgcn_wave_barrier(); }

}  // namespace wdx
