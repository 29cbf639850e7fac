// The device trainer of Fpt_Boost for gfx950: gradient boosting of oblivious trees on integer histograms (include/wdx.h:
// wdx_boost_fit_device states the rule; wdx_boost_fit_plan.h what a fit does with its sizes, the workspace and the overflow bounds).
//
// Once per call: boost_fit_binarise_kernel (the uint8 bins, feature-major, and the class-index check).  Per tree, 3 depth + 4
// stream-ordered plain launches with no host synchronisation between them:
//   boost_fit_gradient_kernel   one lane per row: softmax of the scores through exp_rule, q = rint(g 2^20), class-major int32
//   per level:
//     boost_fit_hist_kernel     THE HOT PATH.  One workgroup per (chunk of 2 047 rows, feature, slab of whole leaf x channel columns):
//                               int32 LDS partials by ds_add, then the entries that are not zero go to the global int64 histogram by
//                               64-bit vector atomics.  Integer sums: any arrival order gives the same bits.  No float atomics.
//     boost_fit_scan_kernel     one workgroup per feature, one thread per border: per leaf the k + 1 channels are prefix-summed over
//                               the bins in LDS (a wave per channel), the thread adds its border's terms in leaf, class order; then
//                               the feature's first maximum over its borders.  It zeroes what it read: the histogram is clean for
//                               the next level.
//     boost_fit_update_kernel   every workgroup reads the features' candidates from device memory, takes the first maximum in feature
//                               order, and sets bit `level` of its rows' leaf index; workgroup 0 records the split
//   boost_fit_hist_kernel       once more, on the final leaves with one bin: the leaves' gradient sums and row counts
//   boost_fit_leaf_kernel       the leaf values
//   boost_fit_score_kernel      S += V[leaf]; zeroes the leaf sums
#include "wdx_ctx.h"
#include "wdx_boost_fit_plan.h"
#include "wdx_exp_rule.h"

#include <math.h>

#include <algorithm>
#include <vector>

namespace wdx {

namespace {

static_assert(kBoostFitThreads == 256 && WDX_BOOST_FIT_MAX_BORDERS + 1 <= kBoostFitThreads && WDX_BOOST_MAX_FEATURES <= kBoostFitThreads,
              "one thread per border, one per feature");
constexpr int kCh = kBoostFitMaxClasses + 1;

// grid (ceil(n / 256), F).  flags[1] |= 1 when a class index lies outside 0 .. k-1
__global__ __launch_bounds__(kBoostFitThreads) void boost_fit_binarise_kernel(const double *X, int64_t n, int64_t ld, const float *borders,
                                                                              const int32_t *border_off, const int32_t *y, int k,
                                                                              uint8_t *bins, int32_t *flags) {
    __shared__ float bd[WDX_BOOST_FIT_MAX_BORDERS + 1];
    const int f = blockIdx.y, tid = threadIdx.x;
    const int b0 = border_off[f], nb = min(border_off[f + 1] - b0, WDX_BOOST_FIT_MAX_BORDERS);
    if (tid < nb) bd[tid] = borders[b0 + tid];
    __syncthreads();
    const int64_t row = (int64_t)blockIdx.x * kBoostFitThreads + tid;
    if (row >= n) return;
    if (f == 0 && (y[row] < 0 || y[row] >= k)) atomicOr(&flags[1], 1);
    const float x = (float)X[row * ld + f];
    int bin = 0;
    for (int j = 0; j < nb; ++j) bin += x > bd[j] ? 1 : 0;   // (a NaN is greater than nothing: bin 0)
    bins[(int64_t)f * n + row] = (uint8_t)bin;
}

// grid ceil(n / 256): q (k, n) int32
__global__ __launch_bounds__(kBoostFitThreads) void boost_fit_gradient_kernel(const double *S, const int32_t *y, int64_t n, int k, int32_t *q) {
    const int64_t row = (int64_t)blockIdx.x * kBoostFitThreads + threadIdx.x;
    if (row >= n) return;
    const double *s = S + row * k;
    double z[kBoostFitMaxClasses];
    double mx = s[0];
#pragma unroll
    for (int c = 0; c < kBoostFitMaxClasses; ++c)
        if (c < k) {
            z[c] = s[c];
            mx = z[c] > mx ? z[c] : mx;
        }
    double sum = 0.0;
#pragma unroll
    for (int c = 0; c < kBoostFitMaxClasses; ++c)
        if (c < k) {
            z[c] = exp_rule(z[c] - mx);
            sum = sum + z[c];
        }
    const int yc = y[row];
    constexpr double kScale = (double)(1 << kBoostFitGradBits);
#pragma unroll
    for (int c = 0; c < kBoostFitMaxClasses; ++c)
        if (c < k) {
            const double g = (c == yc ? 1.0 : 0.0) - z[c] / sum;
            q[(int64_t)c * n + row] = (int32_t)rint(g * kScale);
        }
}

// grid (chunks, features, slabs); dynamic LDS: 4 * min(cols, cps) * NB bytes.  bins == nullptr: every row is in bin 0 (the leaf sums);
// level0: every row is in leaf 0 (the leaf indices of the tree before are stale).  hist + f * fstride: (cols, NB) int64.
__global__ __launch_bounds__(kBoostFitThreads) void boost_fit_hist_kernel(const uint8_t *bins, const int32_t *border_off, const int32_t *q,
                                                                          const uint8_t *leaf, int64_t n, int k, int NB, int cols, int cps,
                                                                          int level0, int64_t fstride, long long *hist) {
    extern __shared__ int32_t part[];
    const int f = blockIdx.y, tid = threadIdx.x;
    if (border_off && border_off[f + 1] == border_off[f]) return;   // a feature without borders is never split on
    const int col0 = (int)blockIdx.z * cps;
    const int ncol = min(cps, cols - col0);
    if (ncol <= 0) return;
    const int entries = ncol * NB;   // <= kBoostFitSlabEntries
    for (int e = tid; e < entries; e += kBoostFitThreads) part[e] = 0;
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * kBoostFitRows, r1 = min(n, r0 + kBoostFitRows);
    const uint8_t *bf = bins ? bins + (int64_t)f * n : nullptr;
    const int ch = k + 1;
    for (int64_t r = r0 + tid; r < r1; r += kBoostFitThreads) {
        const int bin = bf ? min((int)bf[r], NB - 1) : 0;
        const int base = (level0 ? 0 : (int)leaf[r]) * ch - col0;
        for (int c = 0; c < ch; ++c) {
            const int col = base + c;
            if ((unsigned)col < (unsigned)ncol) {
                const int32_t v = c < k ? q[(int64_t)c * n + r] : 1;
                if (v) atomicAdd(&part[col * NB + bin], v);
            }
        }
    }
    __syncthreads();
    unsigned long long *dst = (unsigned long long *)(hist + (int64_t)f * fstride + (int64_t)col0 * NB);
    for (int e = tid; e < entries; e += kBoostFitThreads) {
        const int32_t v = part[e];
        if (v) atomicAdd(&dst[e], (unsigned long long)(long long)v);
    }
}

__device__ __forceinline__ long long wave_inclusive_scan(long long v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// grid F.  cand_b[f] = the feature's best border index (-1: no borders), cand_score[f] its score
__global__ __launch_bounds__(kBoostFitThreads) void boost_fit_scan_kernel(long long *hist, int64_t fstride, const int32_t *border_off,
                                                                          int leaves, int k, int NB, double lambda, double *cand_score,
                                                                          int32_t *cand_b) {
    __shared__ long long pre[kCh][kBoostFitThreads];
    __shared__ double sc[kBoostFitThreads];
    __shared__ int sb[kBoostFitThreads];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = min(border_off[f + 1] - border_off[f], NB - 1);
    if (nb <= 0) {
        if (tid == 0) cand_b[f] = -1, cand_score[f] = 0.0;
        return;
    }
    const int ch = k + 1;
    long long *H = hist + (int64_t)f * fstride;
    double acc = 0.0;
    for (int leaf = 0; leaf < leaves; ++leaf) {
        long long *Hl = H + (int64_t)leaf * ch * NB;
        for (int e = tid; e < ch * NB; e += kBoostFitThreads) {
            pre[e / NB][e % NB] = Hl[e];
            Hl[e] = 0;
        }
        __syncthreads();
        for (int c = wave; c < ch; c += kBoostFitThreads / 64) {
            long long carry = 0;
            for (int b0 = 0; b0 < NB; b0 += 64) {
                const int b = b0 + lane;
                const long long s = wave_inclusive_scan(b < NB ? pre[c][b] : 0, lane) + carry;
                if (b < NB) pre[c][b] = s;
                carry = __shfl(s, 63);
            }
        }
        __syncthreads();
        if (tid < nb) {
            const long long NL = pre[k][tid], NR = pre[k][NB - 1] - NL;
            const double dl = (double)NL + lambda, dr = (double)NR + lambda;
            for (int c = 0; c < k; ++c) {
                const long long GL = pre[c][tid], GR = pre[c][NB - 1] - GL;
                const double a = (double)GL, b = (double)GR;
                acc = acc + a * a / dl;
                acc = acc + b * b / dr;
            }
        }
        __syncthreads();
    }
    // the first maximum over the borders: the greatest score, the lowest index among equals
    sc[tid] = acc, sb[tid] = tid < nb ? tid : -1;
    __syncthreads();
    for (int s = kBoostFitThreads / 2; s >= 1; s >>= 1) {
        if (tid < s) {
            const int ob = sb[tid + s];
            const double os = sc[tid + s];
            if (ob >= 0 && (sb[tid] < 0 || os > sc[tid] || (os == sc[tid] && ob < sb[tid]))) sc[tid] = os, sb[tid] = ob;
        }
        __syncthreads();
    }
    if (tid == 0) cand_b[f] = sb[0], cand_score[f] = sc[0];
}

// grid ceil(n / 256).  out_f / out_b: this level's slot of the tree's splits
__global__ __launch_bounds__(kBoostFitThreads) void boost_fit_update_kernel(const double *cand_score, const int32_t *cand_b, int F,
                                                                            const uint8_t *bins, int64_t n, int level, uint8_t *leaf,
                                                                            int32_t *out_f, int32_t *out_b) {
    __shared__ double sc[kBoostFitThreads];
    __shared__ int sf[kBoostFitThreads], sb[kBoostFitThreads];
    const int tid = threadIdx.x;
    const int b_own = tid < F ? cand_b[tid] : -1;
    sc[tid] = b_own >= 0 ? cand_score[tid] : 0.0, sb[tid] = b_own, sf[tid] = tid;
    __syncthreads();
    for (int s = kBoostFitThreads / 2; s >= 1; s >>= 1) {   // the first maximum in feature order
        if (tid < s) {
            const int ob = sb[tid + s], of = sf[tid + s];
            const double os = sc[tid + s];
            if (ob >= 0 && (sb[tid] < 0 || os > sc[tid] || (os == sc[tid] && of < sf[tid]))) sc[tid] = os, sb[tid] = ob, sf[tid] = of;
        }
        __syncthreads();
    }
    const int f = sf[0], b = sb[0];   // (b >= 0: the plan refuses a fit without a feature that has borders)
    if (blockIdx.x == 0 && tid == 0) *out_f = f, *out_b = b;
    const int64_t row = (int64_t)blockIdx.x * kBoostFitThreads + tid;
    if (row >= n || b < 0) return;
    const int bit = (int)bins[(int64_t)f * n + row] > b ? 1 : 0;
    leaf[row] = (uint8_t)(level ? (int)leaf[row] | (bit << level) : bit);
}

// grid ceil(2^depth * k / 256): V[leaf][c] = lr * ((G * 2^-20) / (N + lambda))
__global__ __launch_bounds__(kBoostFitThreads) void boost_fit_leaf_kernel(const long long *leafsum, int leaves, int k, double lr, double lambda,
                                                                          double *V) {
    const int i = blockIdx.x * kBoostFitThreads + threadIdx.x;
    if (i >= leaves * k) return;
    const int leaf = i / k, c = i % k;
    const double G = (double)leafsum[leaf * (k + 1) + c], N = (double)leafsum[leaf * (k + 1) + k];
    constexpr double kInv = 1.0 / (double)(1 << kBoostFitGradBits);
    V[i] = lr * ((G * kInv) / (N + lambda));
}

// grid ceil(n / 256); workgroup 0 zeroes the leaf sums for the next tree (boost_fit_leaf_kernel has read them)
__global__ __launch_bounds__(kBoostFitThreads) void boost_fit_score_kernel(const double *V, const uint8_t *leaf, int64_t n, int k, double *S,
                                                                           long long *leafsum, int n_leafsum) {
    if (blockIdx.x == 0)
        for (int e = threadIdx.x; e < n_leafsum; e += kBoostFitThreads) leafsum[e] = 0;
    const int64_t row = (int64_t)blockIdx.x * kBoostFitThreads + threadIdx.x;
    if (row >= n) return;
    const double *v = V + (int64_t)leaf[row] * k;
    double *s = S + row * k;
    for (int c = 0; c < k; ++c) s[c] = s[c] + v[c];
}

int boost_fit_refusal(const BoostFitPlan &P) {
    if (P.rc != WDX_SUCCESS) set_error("%s", P.msg);
    return P.rc;
}

// With the context's mutex held.  d_X, d_y and d_scores are device memory, everything else the caller's host memory.
int boost_fit_locked(wdx_ctx *ctx, const BoostFitPlan &P, const double *d_X, const int32_t *d_y, const float *borders, const int32_t *n_borders,
                     const wdx_boost_fit_params &p, double *d_scores, int32_t *split_feature, int32_t *split_border, double *leaf_values,
                     hipStream_t s) {
    int rc;
    if ((rc = use_stream(ctx, s))) return rc;
    if ((rc = ctx->boost_fit_ws.ensure((size_t)P.bytes))) return rc;
    uint8_t *const ws = (uint8_t *)ctx->boost_fit_ws.p;
    const int F = P.F, k = P.k, D = P.D, NB = P.NB, leaves = 1 << D;
    const int64_t n = P.n;
    float *const d_borders = (float *)(ws + P.off_borders);
    int32_t *const d_off = (int32_t *)(ws + P.off_border_off);
    uint8_t *const d_bins = ws + P.off_bins;
    int32_t *const d_q = (int32_t *)(ws + P.off_q);
    uint8_t *const d_leaf = ws + P.off_leaf;
    long long *const d_hist = (long long *)(ws + P.off_hist);
    long long *const d_leafsum = (long long *)(ws + P.off_leafsum);
    double *const d_cand_score = (double *)(ws + P.off_cand_score);
    int32_t *const d_cand_b = (int32_t *)(ws + P.off_cand_b);
    int32_t *const d_split_f = (int32_t *)(ws + P.off_split_f), *const d_split_b = (int32_t *)(ws + P.off_split_b);
    double *const d_leaves = (double *)(ws + P.off_leaves);
    int32_t *const d_flags = (int32_t *)(ws + P.off_flags);

    std::vector<int32_t> off((size_t)F + 1, 0);
    for (int f = 0; f < F; ++f) off[(size_t)f + 1] = off[(size_t)f] + n_borders[f];

    StreamDrain drain(s);   // every exit leaves no copy from or to the caller's memory in flight
    // the histogram and the leaf sums start at zero (the kernels leave them so); then the borders
    WDX_HIP_TRY(hipMemsetAsync(d_hist, 0, (size_t)P.hist_bytes, s));
    WDX_HIP_TRY(hipMemsetAsync(d_leafsum, 0, sizeof(long long) * (size_t)leaves * P.ch, s));
    WDX_HIP_TRY(hipMemsetAsync(d_flags, 0, 2 * sizeof(int32_t), s));
    WDX_HIP_TRY(hipMemcpyAsync(d_borders, borders, sizeof(float) * (size_t)P.total_borders, hipMemcpyHostToDevice, s));
    WDX_HIP_TRY(hipMemcpyAsync(d_off, off.data(), sizeof(int32_t) * off.size(), hipMemcpyHostToDevice, s));
    const dim3 block(kBoostFitThreads);
    const unsigned row_grid = (unsigned)P.row_grid();
    {
        Timed timed(ctx, WDX_K_BOOST_FIT, s);
        timed.n_launches = 1;   // counted as they are issued: a call refused for its class indices has launched this one kernel
        hipLaunchKernelGGL(boost_fit_binarise_kernel, dim3(row_grid, (unsigned)F), block, 0, s, d_X, n, P.ld, d_borders, d_off, d_y, k, d_bins,
                           d_flags);
        WDX_HIP_TRY(hipGetLastError());
        int32_t flags[2] = {0, 0};
        WDX_HIP_TRY(hipMemcpyAsync(flags, d_flags, sizeof flags, hipMemcpyDeviceToHost, s));
        WDX_HIP_TRY(hipStreamSynchronize(s));
        if (flags[1]) {
            set_error("boost fit: a class index lies outside 0 .. %d", k - 1);
            return WDX_ERR_INVALID;
        }
        for (int t = 0; t < P.T; ++t) {
            hipLaunchKernelGGL(boost_fit_gradient_kernel, dim3(row_grid), block, 0, s, d_scores, d_y, n, k, d_q);
            for (int l = 0; l < D; ++l) {
                hipLaunchKernelGGL(boost_fit_hist_kernel, dim3((unsigned)P.chunks, (unsigned)F, (unsigned)P.slabs(l)), block, (size_t)P.lds_bytes(l),
                                   s, d_bins, d_off, d_q, d_leaf, n, k, NB, P.cols(l), P.cols_per_slab(l), l == 0 ? 1 : 0, P.hist_feature_stride, d_hist);
                hipLaunchKernelGGL(boost_fit_scan_kernel, dim3((unsigned)F), block, 0, s, d_hist, P.hist_feature_stride, d_off, 1 << l, k, NB,
                                   p.l2_leaf_reg, d_cand_score, d_cand_b);
                hipLaunchKernelGGL(boost_fit_update_kernel, dim3(row_grid), block, 0, s, d_cand_score, d_cand_b, F, d_bins, n, l, d_leaf,
                                   d_split_f + (int64_t)t * D + l, d_split_b + (int64_t)t * D + l);
            }
            double *const V = d_leaves + (int64_t)t * leaves * k;
            hipLaunchKernelGGL(boost_fit_hist_kernel, dim3((unsigned)P.chunks, 1, (unsigned)P.slabs(D)), block, (size_t)P.lds_bytes(D), s,
                               (const uint8_t *)nullptr, (const int32_t *)nullptr, d_q, d_leaf, n, k, 1, P.cols(D), P.cols_per_slab(D), 0, (int64_t)0,
                               d_leafsum);
            hipLaunchKernelGGL(boost_fit_leaf_kernel, dim3((unsigned)((leaves * k + kBoostFitThreads - 1) / kBoostFitThreads)), block, 0, s, d_leafsum,
                               leaves, k, p.learning_rate, p.l2_leaf_reg, V);
            hipLaunchKernelGGL(boost_fit_score_kernel, dim3(row_grid), block, 0, s, V, d_leaf, n, k, d_scores, d_leafsum, leaves * P.ch);
            timed.n_launches += P.launches_per_tree();
            WDX_HIP_TRY(hipGetLastError());
        }
    }
    WDX_HIP_TRY(hipMemcpyAsync(split_feature, d_split_f, sizeof(int32_t) * (size_t)P.T * D, hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipMemcpyAsync(split_border, d_split_b, sizeof(int32_t) * (size_t)P.T * D, hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipMemcpyAsync(leaf_values, d_leaves, sizeof(double) * (size_t)P.T * leaves * k, hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipStreamSynchronize(s));
    drain.done();
    return WDX_SUCCESS;
}

}  // namespace

}  // namespace wdx

using namespace wdx;

extern "C" {

int wdx_boost_fit_device(wdx_ctx *ctx, const double *d_X, int64_t n, int64_t ld, const int32_t *d_y, const float *borders,
                         const int32_t *n_borders, const wdx_boost_fit_params *p, double *d_scores, int32_t *split_feature,
                         int32_t *split_border, double *leaf_values, void *stream) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    const BoostFitPlan P = boost_fit_plan(n, ld, p, n_borders, d_X != nullptr, d_y != nullptr, borders != nullptr, d_scores != nullptr,
                                          split_feature && split_border && leaf_values);
    if ((rc = boost_fit_refusal(P))) return rc;
    return boost_fit_locked(ctx, P, d_X, d_y, borders, n_borders, *p, d_scores, split_feature, split_border, leaf_values, (hipStream_t)stream);
}

int wdx_boost_fit(wdx_ctx *ctx, const double *X, int64_t n, int64_t ld, const int32_t *y, const float *borders, const int32_t *n_borders,
                  const wdx_boost_fit_params *p, double *scores, int32_t *split_feature, int32_t *split_border, double *leaf_values) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    BoostFitPlan P = boost_fit_plan(n, ld, p, n_borders, X != nullptr, y != nullptr, borders != nullptr, scores != nullptr,
                                    split_feature && split_border && leaf_values);
    if ((rc = boost_fit_refusal(P))) return rc;
    hipStream_t s = ctx->stream;
    // the fingerprints, the class indices and the scores live on the device for this call only
    struct Block {
        void *p = nullptr;
        ~Block() {
            if (p) (void)hipFree(p);
        }
    } Dx, Dy, Ds;
    const size_t F = (size_t)P.F, k = (size_t)P.k;
    WDX_HIP_TRY(hipMalloc(&Dx.p, (size_t)n * F * sizeof(double)));
    WDX_HIP_TRY(hipMalloc(&Dy.p, (size_t)n * sizeof(int32_t)));
    WDX_HIP_TRY(hipMalloc(&Ds.p, (size_t)n * k * sizeof(double)));
    {
        StreamDrain drain(s);
        WDX_HIP_TRY(hipMemcpy2DAsync(Dx.p, F * sizeof(double), X, (size_t)ld * sizeof(double), F * sizeof(double), (size_t)n, hipMemcpyHostToDevice, s));
        WDX_HIP_TRY(hipMemcpyAsync(Dy.p, y, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
        WDX_HIP_TRY(hipMemcpyAsync(Ds.p, scores, (size_t)n * k * sizeof(double), hipMemcpyHostToDevice, s));
        P.ld = (int64_t)F;
        rc = boost_fit_locked(ctx, P, (const double *)Dx.p, (const int32_t *)Dy.p, borders, n_borders, *p, (double *)Ds.p, split_feature, split_border,
                              leaf_values, s);
        if (rc == WDX_SUCCESS) {
            WDX_HIP_TRY(hipMemcpyAsync(scores, Ds.p, (size_t)n * k * sizeof(double), hipMemcpyDeviceToHost, s));
            WDX_HIP_TRY(hipStreamSynchronize(s));
            drain.done();
        }
    }   // (drained: nothing reads the three blocks when they are freed)
    return rc;
}

}  // extern "C"
