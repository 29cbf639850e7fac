// Banded DTW distance matrix for gfx950 -- stage B of the hot path.
//
// Replaces dtaidistance.dtw.distance_matrix as called from
// /root/reference/warpdemux/parallel_distances.py:34-43 and :59-67 (SURVEY.md §8 rows B1-B3,
// recurrence in App. A):  D[i+1][j+1] = (a_i-b_j)^2 + min(D[i][j], D[i][j+1]+p2, D[i+1][j]+p2),
// band |i-j| <= w-1, result sqrt(D[L][L]), float64 arithmetic, float32 output.
//
// Mapping (DESIGN.md "DTW kernels"): one LANE per (series-a, series-b) pair.  Lanes of a wave run
// over different a-series (read-minor layout AT[L][ldA] -> every row load is one coalesced 512-B
// wave access); the b-series is UNIFORM across the wave, so its samples arrive through the scalar
// data path (s_load) and cost no vector issue slots.  The Sakoe-Chiba band of the previous DP row
// lives in 2W-1 float64 registers per lane and is updated in place, left to right; there is no
// cross-lane traffic and no LDS.  All float64 ops are issued un-fused (-ffp-contract=off) in the
// oracle's order, except min(up+p2, left+p2) == min(up,left)+p2, which is exact because rounding
// is monotone.  No MFMA: this is a min-plus recurrence.
#include "wdx_common.h"
#include "wdx_dtw_plan.h"
#include "wdx_dtw_cells.h"

#include <math.h>
#include <stdlib.h>
#include <type_traits>
#include <utility>

namespace wdx {

// np.argmin running update on float32 values (first minimum; first NaN wins outright)
struct ArgminAcc {
    float best = __builtin_huge_valf();
    int idx = 0;
    bool nan = false;
    bool any = false;
    __device__ __forceinline__ void push(float v, int i) {
        if (nan) return;
        if (v != v) {
            nan = true;
            idx = i;
        } else if (!any || v < best) {
            best = v;
            idx = i;
        }
        any = true;
    }
};

// ---- the nearest-reference rule (include/wdx.h: wdx_nearest_dev) -----------------------------------------------------
// Running state over the columns a lane has seen, in rising column order: b1 = their minimum, at column idx (np.argmin's first
// index; ArgminAcc's NaN latch), l1 = that column's label, b2 = the minimum over the columns of every OTHER label.  Update
// on (v, l):  l == l1: b1 = min(b1, v);  v < b1: the old b1 becomes b2 (everything of a label other than l that was seen is
// >= b1, and b1 itself is of another label) and (v, l) the new minimum;  else b2 = min(b2, v).  b1 <= b2 throughout, so the
// label of the second-best group never has to be kept.  l1 = -1 until a value below +inf arrives: a row of +inf alone ends
// with idx 0 and b1 = b2 = +inf, which is what the rule says of it.
struct NearestAcc {
    float b1 = __builtin_huge_valf(), b2 = __builtin_huge_valf();
    int l1 = -1, idx = 0;
    bool nan = false;
    __device__ __forceinline__ void push(float v, int i, int l) {
        if (nan) return;
        if (v != v) {
            nan = true;
            idx = i;
        } else if (l == l1) {
            if (v < b1) {
                b1 = v;
                idx = i;
            }
        } else if (v < b1) {
            b2 = b1;
            b1 = v;
            l1 = l;
            idx = i;
        } else {
            b2 = v < b2 ? v : b2;
        }
    }
};
// label of reference c: the caller's, the identity without labels; anything outside 0 .. G-1 is group G
__device__ __forceinline__ int nearest_label(const NearestArgs &N, int c) {
    if (!N.label) return c;
    const int l = N.label[c];
    return (unsigned)l < (unsigned)N.n_labels ? l : N.n_labels;
}
// read a's outputs from the finished state: first-minimum column idx, d1, d2, the NaN latch
__device__ __forceinline__ void nearest_emit(const NearestArgs &N, int64_t a, int idx, float d1, float d2, bool nan) {
    const int lab = nearest_label(N, idx);
    int call = lab < N.n_labels ? lab : -1;
    if (nan) {
        d1 = d2 = __builtin_nanf("");
        call = -1;
    } else if (call >= 0) {
        const float margin = d2 - d1;   // (inf - inf: NaN, and the negated comparisons reject it)
        if (N.min_margin && !(margin >= N.min_margin[lab])) call = -1;
        if (N.max_dist && !(d1 <= N.max_dist[lab])) call = -1;
    }
    if (N.status && N.status[a] != 0) {
        d1 = d2 = __builtin_nanf("");
        call = -1;
    }
    N.call[a] = call;
    if (N.best) {
        N.best[2 * a] = d1;
        N.best[2 * a + 1] = d2;
    }
}
// What stands in the argmin's place of a lane-per-pair kernel's argument list and epilogue: the int32 argmin array (nullable)
// of the existing instantiations, or the rule's arguments of the NEAREST ones -- separate instantiations, so that the
// existing ones keep their arguments, registers and code.
template <bool NEAREST>
using DtwEpilogue = std::conditional_t<NEAREST, NearestArgs, int32_t *>;
template <bool NEAREST>
using DtwAcc = std::conditional_t<NEAREST, NearestAcc, ArgminAcc>;
// one finished pair: the distance (NEAREST: only when there is a matrix to write) and the running update
template <bool NEAREST>
__device__ __forceinline__ void dtw_pair_out(DtwAcc<NEAREST> &acc, const DtwEpilogue<NEAREST> &epi, float *__restrict__ out,
                                             int64_t off, bool active, float f, int b) {
    if constexpr (NEAREST) {
        if (active && out) out[off] = f;
        acc.push(f, b, nearest_label(epi, b));
    } else {
        if (active) out[off] = f;
        acc.push(f, b);
    }
}
template <bool NEAREST>
__device__ __forceinline__ void dtw_lane_out(const DtwAcc<NEAREST> &acc, const DtwEpilogue<NEAREST> &epi, int64_t a, bool active) {
    if constexpr (NEAREST) {
        if (active) nearest_emit(epi, a, acc.idx, acc.b1, acc.b2, acc.nan);
    } else {
        if (epi && active) epi[a] = acc.idx;
    }
}

// true when the float64 row holds a NaN: lane-private sweep of a row-major series (16-byte loads)
__device__ __forceinline__ bool row_has_nan(const double *__restrict__ row, int L) {
    bool f = false;
    int i = 0;
    // (sixteen values per trip, their loads in flight together: two at a time the sweep was 55 memory latencies in a row per
    // wave of 110-point fingerprints -- 1.1 of the DTW kernel's 47.8 ms per 10 M reads)
    for (; i + 16 <= L; i += 16) {
        double v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = row[i + k];
#pragma unroll
        for (int k = 0; k < 16; ++k) f |= v[k] != v[k];
    }
    for (; i + 2 <= L; i += 2) {
        const double a = row[i], b = row[i + 1];
        f |= (a != a) | (b != b);
    }
    if (i < L) f |= row[i] != row[i];
    return f;
}

// ROWMAJOR: the a-series arrive as they are produced -- (nA, L) row-major, a lane reads its OWN row (ldA is
// ignored).  Loads of one lane are contiguous, so the body rows are fetched eight at a time with 16-byte
// loads (one 64-byte sector per lane and chunk instead of one per row) one chunk ahead of the recurrence,
// and the NaN flag of the series is computed here when the caller has none: no transposed copy of the
// fingerprints, no separate flag kernel.
// (NEAREST, W = 15: the rule's state would cost the read-minor form its third wave per SIMD -- 170 VGPRs -- so these two are held to
// the 168 three waves allow; a bound of 0 is no bound, and the existing instantiations are compiled as before)
template <int W, bool EXACT_W, bool ROWMAJOR, bool NEAREST = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NEAREST && W == 15 ? 3 : 0))) void dtw_band_kernel(
    const double *__restrict__ AT, int64_t ldA, int64_t nA, const uint8_t *__restrict__ a_nan,
    const double *__restrict__ Bpad, int64_t Lpad, int halo, int nB,
    const uint8_t *__restrict__ b_nan, int L, int w, double p2, float *__restrict__ out,
    int64_t sA, int64_t sB, DtwEpilogue<NEAREST> epi, int refs_per_block, int unfused) {
    constexpr int B = 2 * W - 1;
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = a < nA;
    const int64_t al = active ? a : nA - 1;
    const int b0 = blockIdx.y * refs_per_block;
    const int b1 = min(nB, b0 + refs_per_block);
    if (ROWMAJOR) ldA = 1;
    const double *__restrict__ xp = ROWMAJOR ? AT + al * (int64_t)L : AT + al;
    // ROWMAJOR without flags: the NaN sweep of the lane's row is LAZY.  A NaN sample makes every cell of its row NaN, and from
    // there on no cell is finite again (a cell's three predecessors are NaN or +inf: v_min_f64 returns the operand that is not
    // NaN, +inf + p2 = +inf, d^2 + inf = inf) -- so a finite result proves a NaN-free row, and only a wave that sees a result
    // that is not finite (a failed read's NaN fingerprint, an overflow) sweeps its rows, once.  The eager sweep was 55 memory
    // latencies in a row per wave: 1.2 of the kernel's 47.8 ms per 10 M reads.
    bool anan = a_nan ? (a_nan[al] != 0) : false;
    bool swept = a_nan != nullptr || !ROWMAJOR;   // (uniform)
    const double delta = dtw_delta(L);
    DtwAcc<NEAREST> acc;

    for (int b = b0; b < b1; ++b) {
        const double *__restrict__ y = Bpad + (int64_t)b * Lpad + (halo - (W - 1));
        // the pair's accumulated cost D[L][L] on fused (FMA) or on the reference's cells
        auto pair_cost = [&](auto fma_t) -> double {
            constexpr bool FMA = decltype(fma_t)::value;
            double r[B];
#pragma unroll
            for (int c = 0; c < B; ++c) r[c] = WDX_INF;
            r[W - 1] = 0.0;
            double xn = xp[0];
            int i = 0;
            if (EXACT_W && L >= 2 * (W - 1)) {
                // head and tail rows from templates (no masks, no cells outside the matrix); loads of x are
                // independent of the recurrence and get hoisted by the compiler
                dtw_head_rows<W, FMA>(r, xp, ldA, y, p2, std::make_integer_sequence<int, W - 1>{});
                i = W - 1;
                if (ROWMAJOR) {
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
                } else {
                    xn = xp[(int64_t)(W - 1) * ldA];
                }
                for (; i < L - W + 1; ++i) {
                    const double x = xn;
                    xn = xp[(int64_t)(i + 1) * ldA];  // i + 1 <= L - W + 1 < L
                    dtw_row<W, false, FMA>(r, x, y + i, p2, 0, 0, 0);
                }
                dtw_tail_rows<W, FMA>(r, xp, ldA, y, p2, L - W + 1, std::make_integer_sequence<int, W - 1>{});
            } else if (EXACT_W) {
                const int head_end = min(W - 1, L);          // rows whose band leaves [0, L)
                const int body_end = max(head_end, L - W + 1);
                for (; i < head_end; ++i) {
                    double x = xn;
                    if (i + 1 < L) xn = xp[(int64_t)(i + 1) * ldA];
                    dtw_row<W, true, FMA>(r, x, y + i, p2, i - (W - 1), 0, L - 1);
                }
                for (; i < body_end; ++i) {
                    double x = xn;
                    if (i + 1 < L) xn = xp[(int64_t)(i + 1) * ldA];
                    dtw_row<W, false, FMA>(r, x, y + i, p2, 0, 0, 0);
                }
                for (; i < L; ++i) {
                    double x = xn;
                    if (i + 1 < L) xn = xp[(int64_t)(i + 1) * ldA];
                    dtw_row<W, true, FMA>(r, x, y + i, p2, i - (W - 1), 0, L - 1);
                }
            } else {
                for (; i < L; ++i) {
                    double x = xn;
                    if (i + 1 < L) xn = xp[(int64_t)(i + 1) * ldA];
                    dtw_row<W, true, FMA>(r, x, y + i, p2, i - (W - 1), max(0, i - (w - 1)),
                                          min(L - 1, i + (w - 1)));
                }
            }
            return r[W - 1];
        };
        auto lazy_sweep = [&](double r_) __attribute__((always_inline)) {
            if (!swept && __ballot(!(r_ < WDX_INF)) != 0ull) {   // (rare: see above)
                anan = row_has_nan(xp, L);
                swept = true;
            }
        };
        const bool bnan = b_nan && b_nan[b];
        double res;
        bool redo = unfused == 1;   // (uniform)
        if (!redo) {
            const double Dv = pair_cost(std::true_type{});
            res = sqrt(Dv);
            lazy_sweep(res);
            redo = dtw_redo(unfused, !(anan || bnan) && dtw_unsettled(Dv, res, (float)res, delta));   // (the wave's decision)
        }
        if (redo) {
            res = sqrt(pair_cost(std::false_type{}));
            lazy_sweep(res);
        }
        const bool pnan = anan || bnan;
        if (pnan) res = __builtin_nan("");
        float f = (float)res;
        dtw_pair_out<NEAREST>(acc, epi, out, a * sA + (int64_t)b * sB, active, f, b);
    }
    dtw_lane_out<NEAREST>(acc, epi, a, active);
}

// (the unrolled short rows, dtw_short_row / dtw_short_rows / dtw_short_pair: wdx_dtw_cells.h)

// (NEAREST: held to three waves per SIMD like dtw_short_svm_kernel -- left alone the rule's state takes 175 VGPRs, two waves)
template <int L, int W, bool ROWMAJOR, bool NEAREST = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NEAREST ? 3 : 0))) void dtw_short_kernel(
    const double *__restrict__ AT, int64_t ldA, int64_t nA, const uint8_t *__restrict__ a_nan,
    const double *__restrict__ Bpad, int64_t Lpad, int halo, int nB,
    const uint8_t *__restrict__ b_nan, double p2, float *__restrict__ out, int64_t sA, int64_t sB,
    DtwEpilogue<NEAREST> epi, int refs_per_block, int unfused) {
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = a < nA;
    const int64_t al = active ? a : nA - 1;
    const int b0 = blockIdx.y * refs_per_block;
    const int b1 = min(nB, b0 + refs_per_block);
    const double delta = dtw_delta(L);
    double x[L];
    bool anan = a_nan ? (a_nan[al] != 0) : false;
#pragma unroll
    for (int i = 0; i < L; ++i) x[i] = ROWMAJOR ? AT[al * (int64_t)L + i] : AT[(int64_t)i * ldA + al];
    if (ROWMAJOR && !a_nan) {
#pragma unroll
        for (int i = 0; i < L; ++i) anan |= x[i] != x[i];
    }
    DtwAcc<NEAREST> acc;
    for (int b = b0; b < b1; ++b) {
        const double *__restrict__ y = Bpad + (int64_t)b * Lpad + halo;
        const double res = dtw_short_pair<L, W>(x, y, p2, anan || (b_nan && b_nan[b]), delta, unfused);
        const float f = (float)res;
        dtw_pair_out<NEAREST>(acc, epi, out, a * sA + (int64_t)b * sB, active, f, b);
    }
    dtw_lane_out<NEAREST>(acc, epi, a, active);
}

// Any window / any length: two rolling DP rows per lane in global scratch, element (row, j) of lane
// t at scratch[(row*(L+1)+j)*nT + t] (coalesced across lanes).  Slow path; correctness first.
__global__ __launch_bounds__(64) void dtw_scratch_kernel(
    const double *__restrict__ AT, int64_t ldA, int64_t a_base, int64_t nA,
    const uint8_t *__restrict__ a_nan, const double *__restrict__ Bpad, int64_t Lpad, int halo,
    int nB, const uint8_t *__restrict__ b_nan, int L, int w, double p2, float *__restrict__ out,
    int64_t sA, int64_t sB, double *__restrict__ scratch, int64_t nT) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t a = a_base + t;
    const bool active = a < nA && t < nT;
    const int64_t al = a < nA ? a : nA - 1;
    const int64_t tl = t < nT ? t : nT - 1;
    const bool anan = a_nan ? (a_nan[al] != 0) : false;
    double *row0 = scratch + tl;
    const int64_t rs = (int64_t)(L + 1) * nT;
    for (int b = 0; b < nB; ++b) {
        const double *__restrict__ y = Bpad + (int64_t)b * Lpad + halo;
        double *prev = row0, *cur = row0 + rs;
        for (int j = 0; j <= L; ++j) prev[(int64_t)j * nT] = WDX_INF;
        prev[0] = 0.0;
        for (int i = 0; i < L; ++i) {
            const double x = AT[(int64_t)i * ldA + al];
            const int j0 = max(0, i - (w - 1));
            const int j1 = min(L, i + w);
            cur[(int64_t)j0 * nT] = WDX_INF;
            if (j1 + 1 <= L) cur[(int64_t)(j1 + 1) * nT] = WDX_INF;
            double left = WDX_INF;
            double diag = prev[(int64_t)j0 * nT];
            for (int j = j0; j < j1; ++j) {
                double d = x - y[j];
                d = d * d;
                double up = prev[(int64_t)(j + 1) * nT];
                double tt = min_f64(up, left) + p2;
                tt = min_f64(tt, diag);
                double v = d + tt;
                cur[(int64_t)(j + 1) * nT] = v;
                left = v;
                diag = up;
            }
            double *sw = prev;
            prev = cur;
            cur = sw;
        }
        double res = sqrt(prev[(int64_t)L * nT]);
        if (anan || (b_nan && b_nan[b])) res = __builtin_nan("");
        if (active) out[a * sA + (int64_t)b * sB] = (float)res;
    }
}

// ---- wide windows: effective window 33 .. L at L <= WDX_DTW_WIDE_MAX_L (WDX_OPT_WIDE_DTW; wdx_dtw_wide.h) ----------
// Lane = pair like the band kernels (same operands, layouts, grid and argmin), but the band no longer fits the registers, so
// the DP matrix is walked in vertical strips of S = 32 columns [j0, j0 + S).  A strip keeps its segment of the previous DP
// row in S float64 registers and updates it in place, row by row; what the next strip needs of it -- its right-edge column
// D[i][j0 + S - 1] -- goes through LDS, edge[i * 64 + lane] (conflict-free b64 accesses), overwritten in place: a row reads
// the old value (the cell to its left) before it writes its own, and keeps the one it read as the next row's diagonal.  Per
// row and strip: one LDS read, one LDS write, one load of x, S cells; the reference's samples of a strip are uniform and the
// same for all its rows.  No global scratch.  The cell is dtw_scratch_kernel's, operation for operation (the reference's
// six, un-fused): the two kernels give the same bits, non-finite samples included.
// The band |i - j| <= w - 1 limits a strip to rows [j0 - (w-1), j0 + S-1 + (w-1)]; inside them the rows [j0 + S-1 - (w-1),
// j0 + (w-1)] see the whole strip inside the band and run without masks (every row when w = L), the up to S-1 rows above
// and below mask the cells outside it to +inf.  Columns >= L of the last strip are computed on the references' zero halo
// (kWideDtwHalo = S - 1 samples, within the halo run_dtw_plan demands) and never read: values only travel right and down.
constexpr int kWideS = kWideDtwStrip;
// (run_dtw_plan checks halo >= kMaxRegWindow - 1 for every kernel: that is the halo the last strip reads)
static_assert(kWideDtwHalo <= kMaxRegWindow - 1, "the last strip of dtw_wide_kernel reads beyond the references' halo");
static_assert(kWideDtwMinWindow == kMaxRegWindow + 1, "the wide kernel starts where the register-band kernels end");

template <bool MASKED>
__device__ __forceinline__ void dtw_wide_row(double (&r)[kWideS], const double x, const double *__restrict__ ys, const double p2,
                                             double left, double diag, const int clo, const int chi) {
#pragma unroll
    for (int c = 0; c < kWideS; ++c) {
        double d = x - ys[c];
        d = d * d;
        const double up = r[c];
        double t = min_f64(up, left) + p2;
        t = min_f64(t, diag);
        double v = d + t;
        if (MASKED) v = (c < clo || c > chi) ? WDX_INF : v;
        r[c] = v;
        left = v;
        diag = up;
    }
}

// rows [i, iend) of the strip at j0; xn = x[i] on entry and x[iend] on return (when iend <= ihi)
template <bool MASKED>
__device__ __forceinline__ void dtw_wide_rows(double (&r)[kWideS], int &i, const int iend, const int ihi, double &xn,
                                              const double *__restrict__ xp, const int64_t ldA, const double *__restrict__ ys,
                                              const double p2, double *__restrict__ edge, double &diag, const bool first,
                                              const bool last, const int j0, const int w) {
    for (; i < iend; ++i) {
        const double x = xn;
        if (i < ihi) xn = xp[(int64_t)(i + 1) * ldA];   // (uniform)
        const double left = first ? WDX_INF : edge[i * 64];
        dtw_wide_row<MASKED>(r, x, ys, p2, left, diag, i - (w - 1) - j0, i + (w - 1) - j0);
        diag = left;
        if (!last) edge[i * 64] = r[kWideS - 1];
    }
}

template <bool ROWMAJOR, bool NEAREST = false>
__global__ __launch_bounds__(64) void dtw_wide_kernel(
    const double *__restrict__ AT, int64_t ldA, int64_t nA, const uint8_t *__restrict__ a_nan,
    const double *__restrict__ Bpad, int64_t Lpad, int halo, int nB,
    const uint8_t *__restrict__ b_nan, int L, int w, double p2, float *__restrict__ out,
    int64_t sA, int64_t sB, DtwEpilogue<NEAREST> epi, int refs_per_block) {
    extern __shared__ double wide_lds[];   // L rows x 64 lanes
    constexpr int S = kWideS;
    double *__restrict__ edge = wide_lds + threadIdx.x;
    const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = a < nA;
    const int64_t al = active ? a : nA - 1;
    const int b0 = blockIdx.y * refs_per_block;
    const int b1 = min(nB, b0 + refs_per_block);
    if (ROWMAJOR) ldA = 1;
    const double *__restrict__ xp = ROWMAJOR ? AT + al * (int64_t)L : AT + al;
    // (ROWMAJOR without flags: the lazy NaN sweep of dtw_band_kernel -- a finite result proves a NaN-free row)
    bool anan = a_nan ? (a_nan[al] != 0) : false;
    bool swept = a_nan != nullptr || !ROWMAJOR;   // (uniform)
    DtwAcc<NEAREST> acc;

    for (int b = b0; b < b1; ++b) {
        const double *__restrict__ y = Bpad + (int64_t)b * Lpad + halo;
        double r[S];
        for (int j0 = 0; j0 < L; j0 += S) {
            const bool first = j0 == 0, last = j0 + S >= L;
            const int ilo = max(0, j0 - (w - 1)), ihi = min(L - 1, j0 + S - 1 + (w - 1));
            // (the strip's last column INSIDE the matrix decides where the unmasked rows begin: w = L masks nothing)
            const int m0 = max(ilo, min(j0 + S - 1, L - 1) - (w - 1)), m1 = min(ihi, j0 + (w - 1));   // ilo <= m0 <= j0 <= m1 <= ihi
#pragma unroll
            for (int c = 0; c < S; ++c) r[c] = WDX_INF;   // row ilo - 1 of the strip: outside the band, or row -1
            // D[ilo - 1][j0 - 1]: the virtual D[-1][-1] = 0 of the first strip, the band's lower edge of a later one
            double diag = first ? 0.0 : (ilo > 0 ? edge[(ilo - 1) * 64] : WDX_INF);
            double xn = xp[(int64_t)ilo * ldA];
            int i = ilo;
            dtw_wide_rows<true>(r, i, m0, ihi, xn, xp, ldA, y + j0, p2, edge, diag, first, last, j0, w);
            dtw_wide_rows<false>(r, i, m1 + 1, ihi, xn, xp, ldA, y + j0, p2, edge, diag, first, last, j0, w);
            dtw_wide_rows<true>(r, i, ihi + 1, ihi, xn, xp, ldA, y + j0, p2, edge, diag, first, last, j0, w);
            if (!last) {
                // rows of the next strip below this one's: the cell to their left is outside the band
                const int ihn = min(L - 1, j0 + 2 * S - 1 + (w - 1));
                for (; i <= ihn; ++i) edge[i * 64] = WDX_INF;
            }
        }
        // D[L-1][L-1] sits in the last strip at column (L - 1) mod S
        const int cl = (L - 1) & (S - 1);
        double Dv = r[0];
#pragma unroll
        for (int c = 1; c < S; ++c) Dv = (c == cl) ? r[c] : Dv;
        double res = sqrt(Dv);
        if (!swept && __ballot(!(res < WDX_INF)) != 0ull) {   // (rare)
            anan = row_has_nan(xp, L);
            swept = true;
        }
        if (anan || (b_nan && b_nan[b])) res = __builtin_nan("");
        const float f = (float)res;
        dtw_pair_out<NEAREST>(acc, epi, out, a * sA + (int64_t)b * sB, active, f, b);
    }
    dtw_lane_out<NEAREST>(acc, epi, a, active);
}

// ---- anti-diagonal wavefront kernel (latency path: few pairs, e.g. the live 100 ms ticks) ----------
// One 16-lane DPP row per (read, reference) pair, four pairs per wave.  Front k = i + j is evaluated
// by all lanes at once: lane l holds band offset o = j - i = 2l - 14 on even fronts and 2l - 15 on odd
// ones, so  up   (i-1, j) = previous front, lane l+1 (even k) / lane l   (odd k)
//           left (i, j-1) = previous front, lane l   (even k) / lane l-1 (odd k)
//           diag (i-1,j-1) = front k-2, same lane
// i.e. one row_shl:1 or row_shr:1 DPP move per front and no LDS traffic for the band; the two series
// of a pair are staged in LDS once.  2L-1 dependent fronts instead of L*(2w-1) dependent cells: ~15x
// shorter critical path than the lane-per-pair kernel, at ~1.6x its instruction count per pair, hence
// only used when the whole problem fits the machine at once.  Same float64 operations per cell.
__device__ __forceinline__ double dpp_row_shift(double v, double fill, bool left) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    const int flo = __double2loint(fill), fhi = __double2hiint(fill);
    if (left) {  // lane l <- lane l+1
        lo = __builtin_amdgcn_update_dpp(flo, lo, 0x101, 0xf, 0xf, false);
        hi = __builtin_amdgcn_update_dpp(fhi, hi, 0x101, 0xf, 0xf, false);
    } else {     // lane l <- lane l-1
        lo = __builtin_amdgcn_update_dpp(flo, lo, 0x111, 0xf, 0xf, false);
        hi = __builtin_amdgcn_update_dpp(fhi, hi, 0x111, 0xf, 0xf, false);
    }
    return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(256) void dtw_wavefront_kernel(
    const double *__restrict__ X, int64_t nX, const double *__restrict__ Ypad, int64_t Lpad, int halo,
    int nY, int L, int w, double p2, float *__restrict__ out) {
    extern __shared__ double wf_lds[];  // per pair: x[L], y[L]
    __shared__ int nanflag[kWfPairsPerBlock];
    const int tid = threadIdx.x;
    const int row = tid >> 4, l = tid & 15;
    const int64_t npairs = nX * (int64_t)nY;
    const int64_t q = (int64_t)blockIdx.x * kWfPairsPerBlock + row;
    const bool active = q < npairs;
    const int64_t qq = active ? q : npairs - 1;
    const int64_t r = qq / nY;
    const int c = (int)(qq % nY);
    double *xs = wf_lds + (size_t)row * 2 * L, *ys = xs + L;
    if (l == 0) nanflag[row] = 0;
    __syncthreads();
    {
        const double *xg = X + r * L, *yg = Ypad + (int64_t)c * Lpad + halo;
        int bad = 0;
        for (int t = l; t < L; t += 16) {
            const double xv = xg[t], yv = yg[t];
            bad |= (xv != xv) | (yv != yv);
            xs[t] = xv;
            ys[t] = yv;
        }
        if (bad) atomicOr(&nanflag[row], 1);
    }
    __syncthreads();
    double prev2 = (l == 7) ? 0.0 : WDX_INF;  // front k-2 (holds the virtual D[0][0] = 0 for cell (0,0))
    double prev1 = WDX_INF;                     // front k-1
    double cur = WDX_INF;
    const int nfront = 2 * L - 1;
    for (int k = 0; k < nfront; ++k) {
        const bool odd = k & 1;
        const int o = 2 * l - (odd ? 15 : 14);
        const int i = (k - o) >> 1, j = (k + o) >> 1;  // k - o is even by construction
        const bool valid = (odd || l < 15) && i >= 0 && j >= 0 && i < L && j < L && o <= w - 1 && -o <= w - 1;
        const double up = odd ? prev1 : dpp_row_shift(prev1, WDX_INF, true);
        const double left = odd ? dpp_row_shift(prev1, WDX_INF, false) : prev1;
        const double xv = xs[min(max(i, 0), L - 1)], yv = ys[min(max(j, 0), L - 1)];
        double d = xv - yv;
        d = d * d;
        double t = min_f64(up, left) + p2;
        t = min_f64(t, prev2);
        const double v = valid ? d + t : WDX_INF;
        prev2 = prev1;
        prev1 = v;
        cur = v;
    }
    // cell (L-1, L-1): last front (even), o = 0 -> lane 7
    if (active && l == 7) {
        double res = sqrt(cur);
        if (nanflag[row]) res = __builtin_nan("");
        out[q] = (float)res;
    }
}

// see wdx_common.h: launch_dtw_equal_inf
__global__ __launch_bounds__(256) void dtw_equal_inf_kernel(const double *__restrict__ X, int64_t nX, const double *__restrict__ Ypad,
                                                            int64_t Lpad, int halo, int64_t nY, int L, float *__restrict__ out) {
    const int64_t npairs = nX * nY;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npairs; q += (int64_t)gridDim.x * blockDim.x) {
        if (out[q] != __builtin_huge_valf()) continue;   // (finite, NaN already, or -- never -- negative)
        const double *__restrict__ x = X + (q / nY) * L;
        const double *__restrict__ y = Ypad + (q % nY) * Lpad + halo;
        bool hit = false;
        for (int k = 0; k < L; ++k) hit |= x[k] == y[k] && (x[k] == WDX_INF || x[k] == -WDX_INF);
        if (hit) out[q] = __builtin_nanf("");
    }
}

int launch_dtw_equal_inf(const double *X, int64_t nX, const double *Ypad, int64_t Lpad, int halo, int64_t nY, int64_t L,
                         float *out, hipStream_t stream) {
    const int64_t npairs = nX * nY;
    if (npairs == 0) return WDX_SUCCESS;
    int64_t blocks = (npairs + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(dtw_equal_inf_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, X, nX, Ypad, Lpad, halo, nY, (int)L, out);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

// The band ladder's instantiations (plan.info.band_w: 8 / 16 / 32 masked per cell, 15 exact) in both lane layouts
using BandKernel = decltype(&dtw_band_kernel<8, false, false>);
static BandKernel band_kernel(int band_w, bool rowmajor) {
    if (band_w == 8) return rowmajor ? dtw_band_kernel<8, false, true> : dtw_band_kernel<8, false, false>;
    if (band_w == 15) return rowmajor ? dtw_band_kernel<15, true, true> : dtw_band_kernel<15, true, false>;
    if (band_w == 16) return rowmajor ? dtw_band_kernel<16, false, true> : dtw_band_kernel<16, false, false>;
    return rowmajor ? dtw_band_kernel<32, false, true> : dtw_band_kernel<32, false, false>;
}
// ... and their twins with the nearest-reference rule in the epilogue
using BandNearestKernel = decltype(&dtw_band_kernel<8, false, false, true>);
static BandNearestKernel band_nearest_kernel(int band_w, bool rowmajor) {
    if (band_w == 8) return rowmajor ? dtw_band_kernel<8, false, true, true> : dtw_band_kernel<8, false, false, true>;
    if (band_w == 15) return rowmajor ? dtw_band_kernel<15, true, true, true> : dtw_band_kernel<15, true, false, true>;
    if (band_w == 16) return rowmajor ? dtw_band_kernel<16, false, true, true> : dtw_band_kernel<16, false, false, true>;
    return rowmajor ? dtw_band_kernel<32, false, true, true> : dtw_band_kernel<32, false, false, true>;
}

// see wdx_common.h.  Every decision is the plan's (wdx_dtw_plan.h); here are the launches and what guards them against a
// caller whose operands are not the plan's.
int run_dtw_plan(const DtwPlan &P, const DtwOperands &op, wdx_dtw_launch_info *record) {
    const wdx_dtw_launch_info &I = P.info;
    if (I.family == WDX_DTW_NONE) return WDX_SUCCESS;
    if (op.halo < kDtwHalo) {
        set_error("reference rows need a halo of %d samples", kDtwHalo);
        return WDX_ERR_INVALID;
    }
    if (op.argmin && (op.sA != op.nB || op.sB != 1)) {
        set_error("argmin needs the row-major (nA, nB) output layout");
        return WDX_ERR_INVALID;
    }
    if (P.scratch_bytes && (op.scratch_bytes < P.scratch_bytes || !op.scratch)) {
        set_error("DTW scratch too small for window %d", I.window);
        return WDX_ERR_INVALID;
    }
    const NearestArgs *const nz = op.nearest;
    if (nz && (!I.fused_argmin || (I.family != WDX_DTW_WIDE && I.family != WDX_DTW_SHORT && I.family != WDX_DTW_BAND) ||
               I.layout == WDX_DTW_LAYOUT_REFS_AS_LANES || op.sA != op.nB || op.sB != 1 || I.grid_y != 1 || I.refs_per_block < op.nB)) {
        set_error("the nearest-reference rule is fused only where one lane walks every reference of a read");
        return WDX_ERR_INVALID;
    }
    if (record) *record = I;
    const bool rowmajor = I.layout == WDX_DTW_LAYOUT_ROW_MAJOR;
    const int L = (int)P.L, w = I.window, nB = (int)op.nB, rpb = I.refs_per_block;
    const double p2 = op.penalty * op.penalty;
    int32_t *const fused_argmin = I.fused_argmin ? op.argmin : nullptr;
    const dim3 grid((unsigned)I.grid_x, (unsigned)I.grid_y);
    switch (I.family) {
    case WDX_DTW_WAVEFRONT:  // row-major reads against padded refs; out (nA, nB) row-major
        hipLaunchKernelGGL(dtw_wavefront_kernel, grid, dim3(256), (size_t)P.lds_bytes, op.stream, op.A, op.nA, op.Bpad, op.Lpad, op.halo,
                           nB, L, w, p2, op.out);
        break;
    case WDX_DTW_SCRATCH:
        for (int64_t a_base = 0; a_base < op.nA; a_base += kScratchLanes) {
            const int64_t n = op.nA - a_base < kScratchLanes ? op.nA - a_base : kScratchLanes;
            hipLaunchKernelGGL(dtw_scratch_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, op.stream, op.A, op.ldA, a_base, op.nA,
                               op.a_nan, op.Bpad, op.Lpad, op.halo, nB, op.b_nan, L, w, p2, op.out, op.sA, op.sB,
                               (double *)op.scratch, kScratchLanes);
        }
        break;
    case WDX_DTW_WIDE: {
        const auto kern = rowmajor ? dtw_wide_kernel<true> : dtw_wide_kernel<false>;
        static LdsAttr attr[4];   // (more than 64 KiB of dynamic LDS from L = 129 on)
        if (nz) {
            const auto kern_nz = rowmajor ? dtw_wide_kernel<true, true> : dtw_wide_kernel<false, true>;
            if (int rc = attr[2 + rowmajor].ensure(kern_nz, (size_t)P.lds_bytes)) return rc;
            hipLaunchKernelGGL(kern_nz, grid, dim3(64), (size_t)P.lds_bytes, op.stream, op.A, op.ldA, op.nA, op.a_nan, op.Bpad, op.Lpad,
                               op.halo, nB, op.b_nan, L, w, p2, op.out, op.sA, op.sB, *nz, rpb);
            break;
        }
        if (int rc = attr[rowmajor].ensure(kern, (size_t)P.lds_bytes)) return rc;
        hipLaunchKernelGGL(kern, grid, dim3(64), (size_t)P.lds_bytes, op.stream, op.A, op.ldA, op.nA, op.a_nan, op.Bpad, op.Lpad, op.halo,
                           nB, op.b_nan, L, w, p2, op.out, op.sA, op.sB, fused_argmin, rpb);
        break;
    }
    case WDX_DTW_SHORT:
        if (nz) {
            hipLaunchKernelGGL((rowmajor ? dtw_short_kernel<25, 15, true, true> : dtw_short_kernel<25, 15, false, true>), grid, dim3(64), 0,
                               op.stream, op.A, op.ldA, op.nA, op.a_nan, op.Bpad, op.Lpad, op.halo, nB, op.b_nan, p2, op.out, op.sA, op.sB,
                               *nz, rpb, op.unfused);
            break;
        }
        hipLaunchKernelGGL((rowmajor ? dtw_short_kernel<25, 15, true> : dtw_short_kernel<25, 15, false>), grid, dim3(64), 0, op.stream,
                           op.A, op.ldA, op.nA, op.a_nan, op.Bpad, op.Lpad, op.halo, nB, op.b_nan, p2, op.out, op.sA, op.sB,
                           fused_argmin, rpb, op.unfused);
        break;
    case WDX_DTW_BAND:
        if (nz) {
            hipLaunchKernelGGL(band_nearest_kernel(I.band_w, rowmajor), grid, dim3(64), 0, op.stream, op.A, op.ldA, op.nA, op.a_nan, op.Bpad,
                               op.Lpad, op.halo, nB, op.b_nan, L, w, p2, op.out, op.sA, op.sB, *nz, rpb, op.unfused);
            break;
        }
        hipLaunchKernelGGL(band_kernel(I.band_w, rowmajor), grid, dim3(64), 0, op.stream, op.A, op.ldA, op.nA, op.a_nan, op.Bpad, op.Lpad,
                           op.halo, nB, op.b_nan, L, w, p2, op.out, op.sA, op.sB, fused_argmin, rpb, op.unfused);
        break;
    }
    WDX_HIP_TRY(hipGetLastError());
    if (P.argmin_after && op.argmin) return launch_argmin(op.out, op.nA, op.nB, op.argmin, op.stream);
    return WDX_SUCCESS;
}

// ---- the shipped models' DTW with the SVM decision sums in its epilogue (wdx_demux_svm_dev; round 4) --------------
// dtw_short_kernel's body over references in libsvm's SUPPORT-VECTOR order (grouped by class), one block (= one wave)
// per 64 reads and CHUNK of one class's vectors.  Instead of writing the distance, the lane turns it into the kernel
// value k = expf(-gamma d^p) (float32 like the reference, models/dtw_svm.py:21-22) and adds coef[q][s] * k to its k - 1
// decision sums of that class -- P[q][c] = sum over the class's vectors -- kept in LDS (lane-private slots [q][lane]: the
// DTW body uses no LDS and sits at 166 of the 168 VGPRs three waves per SIMD allow, so the sums cannot live in
// registers).  A chunk's sums go to P[slot][q][read] (slot = class * halves + half); svm_finish sums the halves, adds
// -rho and runs the sigmoids / coupling.  The (n, nY) distance matrix does not exist.  Summation order: the class's
// vectors in order -- deterministic, no atomics.
struct DtwSvmArgs {
    const double *X;            // (nA, L) row-major fingerprints
    int64_t nA;
    const double *Ypad;         // references in support-vector order, padded rows
    int64_t Lpad;
    int halo;
    const uint8_t *y_nan;       // per reference (support-vector order)
    double p2;
    const double *coefT;        // [n_sv][k - 1]: dual coefficients, vector-major
    const int32_t *chunk_ref0;  // [n_chunks + 1] first vector of each chunk (chunks never straddle a class)
    const int32_t *chunk_slot;  // [n_chunks] class * halves + half
    int km1, pwr;
    float ngamma;
    double *P;                  // [n_slots][k - 1][nA]
    int unfused;                // 1: the reference's six operations per cell only (WDX_OPT_DTW_UNFUSED)
};
template <int L, int W>
__global__ __launch_bounds__(64, 3) void dtw_short_svm_kernel(DtwSvmArgs G) {
    __shared__ double sums[16][64];
    const int lane = threadIdx.x;
    const int64_t a = (int64_t)blockIdx.x * 64 + lane;
    const bool active = a < G.nA;
    const int64_t al = active ? a : G.nA - 1;
    const int b0 = G.chunk_ref0[blockIdx.y], b1 = G.chunk_ref0[blockIdx.y + 1];
    const int km1 = G.km1;
    const double delta = dtw_delta(L);
    double x[L];
    bool anan = false;
#pragma unroll
    for (int i = 0; i < L; ++i) {
        x[i] = G.X[al * (int64_t)L + i];
        anan |= x[i] != x[i];
    }
    for (int q = 0; q < km1; ++q) sums[q][lane] = 0.0;
    for (int b = b0; b < b1; ++b) {
        const double *__restrict__ y = G.Ypad + (int64_t)b * G.Lpad + G.halo;
        const double res = dtw_short_pair<L, W>(x, y, G.p2, anan || (G.y_nan && G.y_nan[b]), delta, G.unfused);
        const float d = (float)res;   // the float32 distance distance_matrix_to returns (parallel_distances.py:59-67)
        const float t = G.pwr == 1 ? d : (G.pwr == 2 ? d * d : powf(d, (float)G.pwr));
        const double kv = (double)expf(G.ngamma * t);
        const double *__restrict__ cf = G.coefT + (int64_t)b * km1;   // uniform: scalar loads
        for (int q = 0; q < km1; ++q) sums[q][lane] += cf[q] * kv;
    }
    if (active) {
        double *__restrict__ Pq = G.P + ((int64_t)G.chunk_slot[blockIdx.y] * km1) * G.nA + a;
        for (int q = 0; q < km1; ++q) Pq[(int64_t)q * G.nA] = sums[q][lane];
    }
}

int launch_dtw_svm_partial(const double *X, int64_t nA, const double *Ypad_sv, int64_t Lpad, int halo, const uint8_t *y_nan_sv,
                           int64_t L, int window, double penalty, const double *coefT, const int32_t *chunk_ref0,
                           const int32_t *chunk_slot, int n_chunks, int km1, int pwr, float ngamma, double *P,
                           hipStream_t stream, int unfused, wdx_dtw_launch_info *info) {
    if (nA == 0 || n_chunks == 0) return WDX_SUCCESS;
    if (L != 25 || window != 15 || km1 < 1 || km1 > 15) {
        set_error("the fused DTW + SVM path serves the shipped shape (25-point fingerprints, window 15, <= 16 classes)");
        return WDX_ERR_UNSUPPORTED;
    }
    DtwSvmArgs G{X, nA, Ypad_sv, Lpad, halo, y_nan_sv, penalty * penalty, coefT, chunk_ref0, chunk_slot, km1, pwr, ngamma, P, unfused};
    dim3 grid((unsigned)((nA + 63) / 64), (unsigned)n_chunks);
    if (info) *info = {WDX_DTW_SHORT_SVM, 15, 1, WDX_DTW_LAYOUT_ROW_MAJOR, 0, 1, 0, 15, grid.x, grid.y};
    hipLaunchKernelGGL((dtw_short_svm_kernel<25, 15>), grid, dim3(64), 0, stream, G);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

// rows of `src` (n_src, ld) gathered by index into `dst` (n, ld), plus their byte flags: the resident references in
// support-vector order
__global__ void gather_rows_kernel(const double *__restrict__ src, const uint8_t *__restrict__ sflag, const int32_t *__restrict__ idx,
                                   int64_t n, int64_t ld, double *__restrict__ dst, uint8_t *__restrict__ dflag) {
    const int64_t r = blockIdx.x;
    const int64_t s = idx[r];
    for (int64_t i = threadIdx.x; i < ld; i += blockDim.x) dst[r * ld + i] = src[s * ld + i];
    if (threadIdx.x == 0 && dflag) dflag[r] = sflag ? sflag[s] : 0;
}
int launch_gather_rows(const double *src, const uint8_t *sflag, const int32_t *d_idx, int64_t n, int64_t ld, double *dst,
                       uint8_t *dflag, hipStream_t stream) {
    if (n == 0) return WDX_SUCCESS;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)n), dim3(64), 0, stream, src, sflag, d_idx, n, ld, dst, dflag);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

// ---- layout helpers ----------------------------------------------------------------------------

__global__ void transpose_kernel(const double *__restrict__ src, int64_t n, int64_t L,
                                 double *__restrict__ dst, int64_t ld) {
    __shared__ double tile[32][33];
    const int64_t r0 = (int64_t)blockIdx.x * 32;  // series
    const int64_t c0 = (int64_t)blockIdx.y * 32;  // sample
    for (int k = threadIdx.y; k < 32; k += blockDim.y) {
        int64_t r = r0 + k, c = c0 + threadIdx.x;
        if (r < n && c < L) tile[k][threadIdx.x] = src[r * L + c];
    }
    __syncthreads();
    for (int k = threadIdx.y; k < 32; k += blockDim.y) {
        int64_t c = c0 + k, r = r0 + threadIdx.x;
        if (r < n && c < L) dst[c * ld + r] = tile[threadIdx.x][k];
    }
}

__global__ void nan_flags_T_kernel(const double *__restrict__ T, int64_t ld, int64_t n, int64_t L,
                                   uint8_t *__restrict__ flags) {
    int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n) return;
    bool f = false;
    for (int64_t i = 0; i < L; ++i) {
        double v = T[i * ld + a];
        f |= (v != v);
    }
    flags[a] = f ? 1 : 0;
}

int launch_transpose(const double *src, int64_t n, int64_t L, double *dstT, int64_t ld,
                     uint8_t *has_nan, hipStream_t stream) {
    if (n == 0) return WDX_SUCCESS;
    dim3 grid((unsigned)((n + 31) / 32), (unsigned)((L + 31) / 32));
    hipLaunchKernelGGL(transpose_kernel, grid, dim3(32, 8), 0, stream, src, n, L, dstT, ld);
    if (has_nan)
        hipLaunchKernelGGL(nan_flags_T_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                           stream, dstT, ld, n, L, has_nan);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

int launch_nan_flags_T(const double *T, int64_t ld, int64_t n, int64_t L, uint8_t *flags,
                       hipStream_t stream) {
    if (n == 0) return WDX_SUCCESS;
    hipLaunchKernelGGL(nan_flags_T_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       T, ld, n, L, flags);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

__global__ void pad_rows_kernel(const double *__restrict__ src, int64_t n, int64_t L,
                                double *__restrict__ dst, int64_t Lpad, int halo,
                                uint8_t *__restrict__ has_nan) {
    // one wave per series
    const int64_t r = (int64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (r >= n) return;
    bool f = false;
    for (int64_t c = lane; c < Lpad; c += 64) {
        int64_t s = c - halo;
        double v = (s >= 0 && s < L) ? src[r * L + s] : 0.0;
        f |= (v != v);
        dst[r * Lpad + c] = v;
    }
    unsigned long long m = __ballot(f);
    if (has_nan && lane == 0) has_nan[r] = m ? 1 : 0;
}

int launch_pad_rows(const double *src, int64_t n, int64_t L, double *dst, int64_t Lpad, int halo,
                    uint8_t *has_nan, hipStream_t stream) {
    if (n == 0) return WDX_SUCCESS;
    hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, src, n,
                       L, dst, Lpad, halo, has_nan);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

// ---- B3: argmin + call histogram -----------------------------------------------------------------

__global__ void argmin_rows_kernel(const float *__restrict__ D, int64_t n, int64_t m,
                                   int32_t *__restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (r >= n) return;
    // key: (is_nan desc, value asc, index asc) -- np.argmin
    float bv = __builtin_huge_valf();
    int bi = 0x7fffffff;
    bool bn = false;
    for (int64_t c = lane; c < m; c += 64) {
        float v = D[r * m + c];
        bool isn = v != v;
        bool better = bn ? false : (isn ? true : (bi == 0x7fffffff || v < bv));
        if (better) {
            bv = v;
            bi = (int)c;
            bn = isn;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        float ov = __shfl_down(bv, off);
        int oi = __shfl_down(bi, off);
        int on = __shfl_down((int)bn, off);
        bool take;
        if (oi == 0x7fffffff) take = false;
        else if (bi == 0x7fffffff) take = true;
        else if (on != (int)bn) take = on != 0;
        else if (bn) take = oi < bi;
        else take = (ov < bv) || (ov == bv && oi < bi);
        if (take) {
            bv = ov;
            bi = oi;
            bn = on != 0;
        }
    }
    if (lane == 0) out[r] = bi == 0x7fffffff ? 0 : bi;
}

int launch_argmin(const float *D, int64_t n, int64_t m, int32_t *out, hipStream_t stream) {
    if (n == 0) return WDX_SUCCESS;
    hipLaunchKernelGGL(argmin_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, D,
                       n, m, out);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

// The nearest-reference rule on a finished matrix: one wave per row, a lane keeps NearestAcc over its columns lane, lane + 64,
// ..., then the lanes' states are merged.  Merge of two states over disjoint column sets: the smaller b1 wins, on equal values
// the smaller column (so ties between labels resolve to the first column, as the sequential rule does); the merged b2 is the
// winner's b2 against what the loser holds of another label -- its b1 when its label differs from the winner's, else its b2.
// A lane without a finite value (l1 = -1) carries b1 = b2 = +inf and column INT_MAX: it never wins against one that has.  The
// first NaN column of the row is the minimum of the lanes' NaN columns (a lane stops at its first).
__global__ __launch_bounds__(256) void nearest_rows_kernel(const float *__restrict__ D, int64_t n, int64_t m, NearestArgs N) {
    const int64_t r = (int64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (r >= n) return;
    NearestAcc acc;
    for (int64_t c = lane; c < m; c += 64) acc.push(D[r * m + c], (int)c, nearest_label(N, (int)c));
    int nan_col = acc.nan ? acc.idx : 0x7fffffff;
    float b1 = acc.b1, b2 = acc.b2;
    int l1 = acc.l1, idx = (acc.nan || acc.l1 < 0) ? 0x7fffffff : acc.idx;
    for (int off = 32; off > 0; off >>= 1) {
        const float ob1 = __shfl_xor(b1, off), ob2 = __shfl_xor(b2, off);
        const int ol1 = __shfl_xor(l1, off), oidx = __shfl_xor(idx, off), onan = __shfl_xor(nan_col, off);
        nan_col = onan < nan_col ? onan : nan_col;
        const bool take = ob1 < b1 || (ob1 == b1 && oidx < idx);
        const float wb2 = take ? ob2 : b2;                                // the winner's second value
        const float lo = take ? (l1 != ol1 ? b1 : b2) : (ol1 != l1 ? ob1 : ob2);   // the loser's best of another label
        b2 = lo < wb2 ? lo : wb2;
        if (take) {
            b1 = ob1;
            l1 = ol1;
            idx = oidx;
        }
    }
    if (lane != 0) return;
    const bool nan = nan_col != 0x7fffffff;
    nearest_emit(N, r, nan ? nan_col : (l1 < 0 ? 0 : idx), b1, b2, nan);
}

int launch_nearest_rows(const float *D, int64_t n, int64_t m, const NearestArgs &N, hipStream_t stream) {
    if (n == 0) return WDX_SUCCESS;
    hipLaunchKernelGGL(nearest_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, D, n, m, N);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

__global__ void count_calls_kernel(int32_t *__restrict__ call, const int32_t *__restrict__ status,
                                   int64_t n, int m, unsigned long long *__restrict__ counts) {
    extern __shared__ unsigned int hist[];
    const bool use_lds = m + 1 <= 4096;
    if (use_lds) {
        for (int k = threadIdx.x; k <= m; k += blockDim.x) hist[k] = 0;
        __syncthreads();
    }
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n;
         r += (int64_t)gridDim.x * blockDim.x) {
        int c = call[r];
        if (status && status[r] != 0) {
            c = -1;
            call[r] = -1;
        }
        int bin = (c < 0 || c >= m) ? m : c;
        if (counts) {
            if (use_lds) atomicAdd(&hist[bin], 1u);
            else atomicAdd(&counts[bin], 1ull);
        }
    }
    if (use_lds && counts) {
        __syncthreads();
        for (int k = threadIdx.x; k <= m; k += blockDim.x)
            if (hist[k]) atomicAdd(&counts[k], (unsigned long long)hist[k]);
    }
}

int launch_count_calls(int32_t *call, const int32_t *status, int64_t n, int64_t m, int64_t *counts,
                       hipStream_t stream) {
    if (n == 0) return WDX_SUCCESS;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    size_t lds = (m + 1 <= 4096) ? (size_t)(m + 1) * sizeof(unsigned int) : 0;
    hipLaunchKernelGGL(count_calls_kernel, dim3((unsigned)blocks), dim3(256), lds, stream, call,
                       status, n, (int)m, (unsigned long long *)counts);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

}  // namespace wdx
