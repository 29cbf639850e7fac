// The kernel matrix of a DTW kernel machine from its self-distance matrix, on the device (include/wdx.h: wdx_svm_kernel_device states
// the rule): K_ij = exp_rule(-(gamma * D_ij^p)) rounded to float32, one read and one write per entry -- a bandwidth kernel.
//
// One thread per four consecutive entries of a row: a 16-byte load and a 16-byte store when both matrices keep every row 16-byte
// aligned (base pointers aligned, ld and ldk multiples of four); the ragged end of a row, and every entry otherwise, one by one.
// A thread reads its entries before it writes them and no other thread touches them: d_K == d_D with ldk == ld works in place.
#include "wdx_ctx.h"
#include "wdx_exp_rule.h"

#include <math.h>

namespace wdx {

namespace {

constexpr int kSvmKernelThreads = 256;
constexpr int kSvmKernelPerThread = 4;

__device__ __forceinline__ float svm_kernel_entry(float d, double gamma, int pwr) {
    const double t = (double)d;
    double pw = t;
    for (int e = 1; e < pwr; ++e) pw = pw * t;
    const double x = -(gamma * pw);
    if (x != x) return (float)x;   // (a NaN never reaches exp_rule's integer conversion)
    return (float)exp_rule(x);
}

// grid m * cpr: workgroup b has row b / cpr and the b % cpr-th run of 1 024 columns
__global__ __launch_bounds__(kSvmKernelThreads) void svm_kernel_matrix_kernel(const float *D, int64_t m, int64_t ld, double gamma, int pwr,
                                                                              float *K, int64_t ldk, int vec, int64_t cpr) {
    const int64_t row = (int64_t)blockIdx.x / cpr, chunk = (int64_t)blockIdx.x % cpr;
    const int64_t c0 = (chunk * kSvmKernelThreads + threadIdx.x) * kSvmKernelPerThread;
    if (c0 >= m) return;
    const float *src = D + row * ld;
    float *dst = K + row * ldk;
    if (vec && c0 + kSvmKernelPerThread <= m) {
        const float4 v = *reinterpret_cast<const float4 *>(src + c0);
        float4 o;
        o.x = svm_kernel_entry(v.x, gamma, pwr);
        o.y = svm_kernel_entry(v.y, gamma, pwr);
        o.z = svm_kernel_entry(v.z, gamma, pwr);
        o.w = svm_kernel_entry(v.w, gamma, pwr);
        *reinterpret_cast<float4 *>(dst + c0) = o;
    } else {
        const int64_t c1 = c0 + kSvmKernelPerThread < m ? c0 + kSvmKernelPerThread : m;
        for (int64_t c = c0; c < c1; ++c) dst[c] = svm_kernel_entry(src[c], gamma, pwr);
    }
}

}  // namespace

}  // namespace wdx

using namespace wdx;

extern "C" {

int wdx_svm_kernel_device(wdx_ctx *ctx, const float *d_D, int64_t m, int64_t ld, double gamma, int32_t pwr_dist, float *d_K, int64_t ldk,
                       void *stream) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    if (m < 1 || ld < m || ldk < m) {
        set_error("svm kernel: m = %lld must be at least 1, ld = %lld and ldk = %lld at least m", (long long)m, (long long)ld, (long long)ldk);
        return WDX_ERR_INVALID;
    }
    if (m > WDX_SVM_KERNEL_MAX_ROWS) {
        set_error("svm kernel: m = %lld rows, more than WDX_SVM_KERNEL_MAX_ROWS = %d", (long long)m, WDX_SVM_KERNEL_MAX_ROWS);
        return WDX_ERR_UNSUPPORTED;
    }
    if (pwr_dist < 1) {
        set_error("svm kernel: pwr_dist = %d must be at least 1", pwr_dist);
        return WDX_ERR_INVALID;
    }
    if (pwr_dist > WDX_SVM_KERNEL_MAX_POWER) {
        set_error("svm kernel: pwr_dist = %d (1..WDX_SVM_KERNEL_MAX_POWER = %d supported)", pwr_dist, WDX_SVM_KERNEL_MAX_POWER);
        return WDX_ERR_UNSUPPORTED;
    }
    if (!(gamma > 0.0) || !isfinite(gamma)) {
        set_error("svm kernel: gamma must be positive and finite, not %g", gamma);
        return WDX_ERR_INVALID;
    }
    if (!d_D || !d_K) {
        set_error("svm kernel: the distance matrix and the output are required (NULL given)");
        return WDX_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    if ((rc = use_stream(ctx, s))) return rc;
    const int vec = ((uintptr_t)d_D % 16 == 0 && (uintptr_t)d_K % 16 == 0 && ld % 4 == 0 && ldk % 4 == 0) ? 1 : 0;
    constexpr int64_t kCols = (int64_t)kSvmKernelThreads * kSvmKernelPerThread;
    const int64_t cpr = (m + kCols - 1) / kCols;
    Timed t(ctx, WDX_K_SVM_KERNEL, s);
    hipLaunchKernelGGL(svm_kernel_matrix_kernel, dim3((unsigned)(m * cpr)), dim3(kSvmKernelThreads), 0, s, d_D, m, ld, gamma, (int)pwr_dist, d_K,
                       ldk, vec, cpr);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

}  // extern "C"
