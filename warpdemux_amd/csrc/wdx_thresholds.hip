// Accuracy thresholds from probabilities and labels for gfx950 (include/wdx.h: wdx_accuracy_thresholds_device states the rule;
// wdx_thresholds_plan.h what a call does with its sizes).
//
//   thresholds_hist_kernel    one lane per row: the first maximum, top1 - top2, the bin of the margin on the grid i / R; uint32 LDS
//                             counters per (predicted class of the workgroup's group, rows | hits, bin) by LDS integer adds, then
//                             the counters that are not zero to the global int64 histograms by 64-bit vector atomics.  Integer
//                             sums: any arrival order gives the same bits.  No float atomics.
//   thresholds_select_kernel  one wave per class: suffix sums from the top bin down, 64 bins a step, written over the histograms;
//                             per target the smallest bin j >= 1 with kept_j > 0 and 1000 hit_j >= a kept_j (int64, exact).
#include "wdx_ctx.h"
#include "wdx_thresholds_plan.h"

#include <math.h>

namespace wdx {

namespace {

struct ThrArgs {
    const double *prob;   // (n, k)
    const int32_t *y;     // [n]
    int64_t n;
    int k, R, cpg, T;
    unsigned long long *kept, *hit, *skipped;   // (k, R + 1), (k, R + 1), [1]
    double *thr;          // (T, k)
    ThrTargets targets;
};

// grid (chunks, groups); dynamic LDS: 4 * min(cpg, k) * 2 * (R + 1) bytes
__global__ __launch_bounds__(kThrThreads) void thresholds_hist_kernel(const ThrArgs A) {
    extern __shared__ uint32_t cnt[];   // [class of the group][rows, hits][bin]
    __shared__ uint32_t n_skipped;
    const int tid = threadIdx.x, k = A.k, R = A.R, bins = R + 1;
    const int c_lo = (int)blockIdx.y * A.cpg, nc = min(A.cpg, k - c_lo);
    const int entries = nc * 2 * bins;   // <= kThrLdsEntries
    for (int e = tid; e < entries; e += kThrThreads) cnt[e] = 0;
    if (tid == 0) n_skipped = 0;
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * kThrRows, r1 = min(A.n, r0 + kThrRows);
    const double Rd = (double)R;
    for (int64_t r = r0 + tid; r < r1; r += kThrThreads) {
        const double *p = A.prob + r * k;
        const int y = A.y[r];
        double v[WDX_THRESHOLDS_MAX_CLASSES];
        bool used = y >= 0;
        double top1 = p[0];
        int arg = 0;
#pragma unroll
        for (int c = 0; c < WDX_THRESHOLDS_MAX_CLASSES; ++c)
            if (c < k) {
                v[c] = p[c];
                used = used && fabs(v[c]) <= 1.7976931348623157e308;
                if (v[c] > top1) top1 = v[c], arg = c;   // the first maximum
            }
        if (!used) {
            if (blockIdx.y == 0) atomicAdd(&n_skipped, 1u);
            continue;
        }
        double top2 = -INFINITY;
#pragma unroll
        for (int c = 0; c < WDX_THRESHOLDS_MAX_CLASSES; ++c)
            if (c < k && c != arg && v[c] > top2) top2 = v[c];
        const double conf = top1 - top2;   // >= 0
        // the largest i with i / R <= conf
        const double f = floor(conf * Rd);
        int i = f >= Rd ? R : (int)f;
        if ((double)i / Rd > conf) --i;
        if (i < R && (double)(i + 1) / Rd <= conf) ++i;
        i = max(i, 0);   // (conf >= 0 = 0 / R: never below)
        const int lc = arg - c_lo;
        if ((unsigned)lc < (unsigned)nc) {
            atomicAdd(&cnt[(lc * 2) * bins + i], 1u);
            if (arg == y) atomicAdd(&cnt[(lc * 2 + 1) * bins + i], 1u);
        }
    }
    __syncthreads();
    for (int e = tid; e < entries; e += kThrThreads) {
        const uint32_t c = cnt[e];
        if (c) {
            const int col = e / bins, b = e - col * bins;
            unsigned long long *dst = (col & 1 ? A.hit : A.kept) + (int64_t)(c_lo + (col >> 1)) * bins + b;
            atomicAdd(dst, (unsigned long long)c);
        }
    }
    if (tid == 0 && n_skipped) atomicAdd(A.skipped, (unsigned long long)n_skipped);
}

__device__ __forceinline__ long long thr_inclusive_scan(long long v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// grid k, one wave.  Lane l of a step has bin top - l: the scan over the lanes runs down the bins.
__global__ __launch_bounds__(64) void thresholds_select_kernel(const ThrArgs A) {
    const int c = blockIdx.x, lane = threadIdx.x, R = A.R, bins = R + 1;
    long long *kept = (long long *)A.kept + (int64_t)c * bins, *hit = (long long *)A.hit + (int64_t)c * bins;
    long long carry_k = 0, carry_h = 0;
    int mine = 0;   // lane t: the smallest qualifying bin of target t so far (0: none)
    for (int top = R; top >= 0; top -= 64) {
        const int j = top - lane;
        const long long nk = thr_inclusive_scan(j >= 0 ? kept[j] : 0, lane) + carry_k;
        const long long nh = thr_inclusive_scan(j >= 0 ? hit[j] : 0, lane) + carry_h;
        if (j >= 0) kept[j] = nk, hit[j] = nh;
        carry_k = __shfl(nk, 63), carry_h = __shfl(nh, 63);
#pragma unroll
        for (int t = 0; t < WDX_THRESHOLDS_MAX_TARGETS; ++t) {
            if (t >= A.T) break;   // (uniform)
            const bool ok = j >= 1 && nk > 0 && 1000ll * nh >= (long long)A.targets.pm[t] * nk;
            const unsigned long long mask = __ballot(ok);
            if (mask && lane == t) mine = top - (63 - __clzll((long long)mask));   // the highest lane: the lowest bin
        }
    }
    if (lane < A.T) A.thr[(int64_t)lane * A.k + c] = mine ? (double)mine / (double)R : INFINITY;
}

int thresholds_refusal(const ThrPlan &P) {
    if (P.rc != WDX_SUCCESS) set_error("%s", P.msg);
    return P.rc;
}

// With the context's mutex held.  Every pointer but the plan is device memory; d_kept, d_hit and d_skipped are nullable.
int thresholds_locked(wdx_ctx *ctx, const ThrPlan &P, const double *d_prob, const int32_t *d_y, double *d_thr, int64_t *d_kept, int64_t *d_hit,
                      int64_t *d_skipped, hipStream_t s) {
    int rc;
    if ((rc = use_stream(ctx, s))) return rc;
    if (!d_kept || !d_hit || !d_skipped) {
        if ((rc = ctx->thr_ws.ensure((size_t)P.ws_bytes))) return rc;
        uint8_t *const ws = (uint8_t *)ctx->thr_ws.p;
        if (!d_kept) d_kept = (int64_t *)(ws + P.off_kept);
        if (!d_hit) d_hit = (int64_t *)(ws + P.off_hit);
        if (!d_skipped) d_skipped = (int64_t *)(ws + P.off_skipped);
    }
    WDX_HIP_TRY(hipMemsetAsync(d_kept, 0, 8 * (size_t)P.hist_entries, s));
    WDX_HIP_TRY(hipMemsetAsync(d_hit, 0, 8 * (size_t)P.hist_entries, s));
    WDX_HIP_TRY(hipMemsetAsync(d_skipped, 0, 8, s));
    const ThrArgs A{d_prob, d_y, P.n, P.k, P.R, P.classes_per_group, P.T, (unsigned long long *)d_kept, (unsigned long long *)d_hit,
                    (unsigned long long *)d_skipped, d_thr, P.targets};
    Timed timed(ctx, WDX_K_THRESHOLDS, s);
    timed.n_launches = 1;
    if (P.chunks > 0) {
        hipLaunchKernelGGL(thresholds_hist_kernel, dim3((unsigned)P.chunks, (unsigned)P.groups), dim3(kThrThreads), (size_t)P.lds_bytes, s, A);
        timed.n_launches = 2;
    }
    hipLaunchKernelGGL(thresholds_select_kernel, dim3((unsigned)P.k), dim3(64), 0, s, A);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

}  // namespace

}  // namespace wdx

using namespace wdx;

extern "C" {

int wdx_accuracy_thresholds_device(wdx_ctx *ctx, const double *d_prob, int64_t n, int32_t k, const int32_t *d_y_idx, int32_t resolution,
                                const int32_t *targets_pm, int32_t n_targets, double *d_thr, int64_t *d_kept, int64_t *d_hit,
                                int64_t *d_skipped, void *stream) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    const ThrPlan P = thresholds_plan(n, k, resolution, targets_pm, n_targets, d_prob != nullptr, d_y_idx != nullptr, d_thr != nullptr);
    if ((rc = thresholds_refusal(P))) return rc;
    return thresholds_locked(ctx, P, d_prob, d_y_idx, d_thr, d_kept, d_hit, d_skipped, (hipStream_t)stream);
}

int wdx_accuracy_thresholds(wdx_ctx *ctx, const double *prob, int64_t n, int32_t k, const int32_t *y_idx, int32_t resolution,
                            const int32_t *targets_pm, int32_t n_targets, double *thr, int64_t *kept, int64_t *hit, int64_t *skipped) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    const ThrPlan P = thresholds_plan(n, k, resolution, targets_pm, n_targets, prob != nullptr, y_idx != nullptr, thr != nullptr);
    if ((rc = thresholds_refusal(P))) return rc;
    hipStream_t s = ctx->stream;
    // the probabilities, the class indices and the results live on the device for this call only
    struct Block {
        void *p = nullptr;
        ~Block() {
            if (p) (void)hipFree(p);
        }
    } Dp, Dy, Do;
    const size_t pb = (size_t)n * (size_t)k * sizeof(double), yb = (size_t)n * sizeof(int32_t);
    const size_t hb = 8 * (size_t)P.hist_entries, tb = sizeof(double) * (size_t)P.T * (size_t)k;
    if (n > 0) {
        WDX_HIP_TRY(hipMalloc(&Dp.p, pb));
        WDX_HIP_TRY(hipMalloc(&Dy.p, yb));
    }
    WDX_HIP_TRY(hipMalloc(&Do.p, 2 * hb + 8 + tb));
    uint8_t *const o = (uint8_t *)Do.p;
    int64_t *const d_kept = (int64_t *)o, *const d_hit = (int64_t *)(o + hb), *const d_skipped = (int64_t *)(o + 2 * hb);
    double *const d_thr = (double *)(o + 2 * hb + 8);
    {
        StreamDrain drain(s);   // (declared behind the blocks: the stream is drained before they are freed)
        if (n > 0) {
            WDX_HIP_TRY(hipMemcpyAsync(Dp.p, prob, pb, hipMemcpyHostToDevice, s));
            WDX_HIP_TRY(hipMemcpyAsync(Dy.p, y_idx, yb, hipMemcpyHostToDevice, s));
        }
        if ((rc = thresholds_locked(ctx, P, (const double *)Dp.p, (const int32_t *)Dy.p, d_thr, d_kept, d_hit, d_skipped, s))) return rc;
        WDX_HIP_TRY(hipMemcpyAsync(thr, d_thr, tb, hipMemcpyDeviceToHost, s));
        if (kept) WDX_HIP_TRY(hipMemcpyAsync(kept, d_kept, hb, hipMemcpyDeviceToHost, s));
        if (hit) WDX_HIP_TRY(hipMemcpyAsync(hit, d_hit, hb, hipMemcpyDeviceToHost, s));
        if (skipped) WDX_HIP_TRY(hipMemcpyAsync(skipped, d_skipped, 8, hipMemcpyDeviceToHost, s));
        WDX_HIP_TRY(hipStreamSynchronize(s));
        drain.done();
    }
    return WDX_SUCCESS;
}

}  // extern "C"
