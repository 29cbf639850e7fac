// The device trainer of DTW_MLP for gfx950: scikit-learn's MLPClassifier(solver="adam") in float32 on a resident distance matrix
// (include/wdx.h: wdx_mlp_fit_device states the rule; wdx_mlp_fit_plan.h what a fit does with its sizes and lays out the workspace).
//
// One Adam step is 2 n_layers stream-ordered launches (plain launches: no graph, no grid-wide barrier, no atomics):
//   mlp_fit_forward_kernel   the row layout of mlp_forward_kernel<float> (wdx_mlp.hip): 256 threads per 16 batch rows, every layer
//                            through v_mfma_f32_16x16x4_f32, rows gathered through the epoch's index list from the scaled input;
//                            hidden activations to LDS and to the workspace, the output delta p - onehot, one float64 loss slot
//   mlp_fit_delta_kernel     delta_l = (delta_{l+1} W_l^T) o act'(A_l), the same row layout, enqueued before W_l is updated
//   mlp_fit_adam_kernel      one wave per 16 x 16 tile of W_l: A_l^T delta_{l+1} as an MFMA chain over the batch rows in row order, then
//                            the gradient, both moments and the update on the tile the wave owns; the first tile row owns the intercepts
// Remainders -- fan-in % 4 and % 16, fan-out % 16, a batch that is no multiple of 16 or of 4 -- are zero operands, never branches
// around an MFMA.  The host computes lr_t per step and, once per epoch, reads the loss slots, applies the stop rule and uploads
// the next epoch's index list.
#include "wdx_ctx.h"
#include "wdx_mlp_fit_plan.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace wdx {

namespace {

constexpr int kL = WDX_MLP_MAX_LAYERS;
constexpr int kMaxTilesPerWave = WDX_MLP_MAX_WIDTH / 16 / 4;
static_assert(kMlpFitThreads == 256 && kMlpFitRows == 16 && kMlpFitWavesPerGroup == 4, "the kernels' layout");

typedef float f32x4 __attribute__((ext_vector_type(4)));
// v_mfma_f32_16x16x4_f32: lane holds A[row lane & 15][k lane >> 4] and B[k lane >> 4][column lane & 15]; C/D: row (lane >> 4) * 4 + reg,
// column lane & 15
__device__ __forceinline__ f32x4 mma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

struct MlpFitDev {
    int nl, act, k, n_out, lds_ld;
    int sizes[kL + 1];
    const float *xs;
    const int32_t *idx, *y;
    float *W[kL], *B[kL], *mW[kL], *vW[kL], *mB[kL], *vB[kL];
    float *A[kL + 1];   // 1 .. nl - 1
    float *D[kL + 1];   // 1 .. nl
    double *loss, *l2;
};

struct AdamArgs {
    float alpha, beta1, om_beta1, beta2, om_beta2, epsilon;
    double lr_t;
};

__device__ __forceinline__ float activate(float v, int act) {
    switch (act) {
        case WDX_MLP_ACT_LOGISTIC: return (float)(1.0 / (1.0 + exp(-(double)v)));
        case WDX_MLP_ACT_TANH: return (float)tanh((double)v);
        case WDX_MLP_ACT_RELU: return v > 0.0f ? v : (v == v ? 0.0f : v);
        default: return v;
    }
}

// the scaled input, once per fit; flags[0]: a value that is not finite, flags[1]: a class index outside 0 .. k-1 (plain stores of 1)
__global__ __launch_bounds__(256) void mlp_fit_scale_kernel(const float *__restrict__ dist, int64_t m, int64_t ld, int F,
                                                            const double *__restrict__ mean, const double *__restrict__ scale,
                                                            float *__restrict__ xs, const int32_t *__restrict__ y, int k,
                                                            int32_t *__restrict__ flags) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = t0; i < m * F; i += stride) {
        const int64_t r = i / F;
        const int f = (int)(i - r * F);
        float x = dist[r * ld + f];
        if (mean) x = (float)((double)x - mean[f]);
        if (scale) x = (float)((double)x / scale[f]);
        xs[i] = x;
        if (!isfinite(x)) flags[0] = 1;
    }
    for (int64_t r = t0; r < m; r += stride)
        if (y[r] < 0 || y[r] >= k) flags[1] = 1;
}

__global__ __launch_bounds__(kMlpFitThreads) void mlp_fit_forward_kernel(const MlpFitDev M, int64_t b0, int nb, int64_t slot0) {
    extern __shared__ __align__(16) float fit_lds[];
    __shared__ float rowloss[kMlpFitRows];
    const int ld = M.lds_ld, nl = M.nl;
    float *src = fit_lds, *dst = fit_lds + kMlpFitRows * ld;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ar = lane & 15, kk = lane >> 4;
    const int r0 = blockIdx.x * kMlpFitRows;
    const bool row_ok = r0 + ar < nb;
    const float *__restrict__ xrow = row_ok ? M.xs + (int64_t)M.idx[b0 + r0 + ar] * M.sizes[0] : nullptr;

    for (int l = 0; l < nl; ++l) {
        const int K = M.sizes[l], H = M.sizes[l + 1];
        const int ntiles = (H + 15) / 16;
        const float *__restrict__ W = M.W[l];
        f32x4 acc[kMaxTilesPerWave];
#pragma unroll
        for (int t = 0; t < kMaxTilesPerWave; ++t) acc[t] = f32x4{0, 0, 0, 0};
#pragma unroll 2
        for (int k0 = 0; k0 < K; k0 += 4) {
            const int k = k0 + kk;
            float a = 0.0f;
            if (k < K) a = l == 0 ? (row_ok ? xrow[k] : 0.0f) : src[ar * ld + k];
#pragma unroll
            for (int t = 0; t < kMaxTilesPerWave; ++t) {
                const int tile = wave + 4 * t;
                if (tile < ntiles) {   // wave-uniform
                    const int j = tile * 16 + ar;
                    const float b = (k < K && j < H) ? W[(int64_t)k * H + j] : 0.0f;
                    acc[t] = mma(a, b, acc[t]);
                }
            }
        }
        const bool hidden = l < nl - 1;
        float *__restrict__ Aout = hidden ? M.A[l + 1] : nullptr;
#pragma unroll
        for (int t = 0; t < kMaxTilesPerWave; ++t) {
            const int tile = wave + 4 * t;
            if (tile < ntiles) {
                const int j = tile * 16 + ar;
                if (j < H) {
                    const float bj = M.B[l][j];
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int row = kk * 4 + reg;
                        float v = acc[t][reg] + bj;
                        if (hidden) v = activate(v, M.act);
                        dst[row * ld + j] = v;
                        // rows beyond the batch are zero rows of the workspace (r0 + row < the padded batch: the plan's batch_pad)
                        if (hidden) Aout[(int64_t)(r0 + row) * H + j] = r0 + row < nb ? v : 0.0f;
                    }
                }
            }
        }
        __syncthreads();
        float *t = src;
        src = dst;
        dst = t;
    }

    // output activation, delta and loss: one lane per row
    const int t = threadIdx.x;
    if (t < kMlpFitRows) {
        const int row = r0 + t;
        const bool valid = row < nb;
        const int n_out = M.n_out;
        const float *z = src + t * ld;
        float *__restrict__ Dn = M.D[nl] + (int64_t)row * n_out;
        const float eps = 1.1920928955078125e-07f, hi = 1.0f - eps;
        float loss = 0.0f;
        int yy = valid ? M.y[M.idx[b0 + row]] : 0;
        if (n_out == 1) {
            const float p = (float)(1.0 / (1.0 + exp(-(double)z[0])));
            const float pc = fminf(fmaxf(p, eps), hi);
            loss = yy == 1 ? (float)-log((double)pc) : (float)-log((double)(1.0f - pc));
            if (p != p) loss = p;
            Dn[0] = valid ? p - (yy == 1 ? 1.0f : 0.0f) : 0.0f;
        } else {
            float zmax = z[0];
            for (int c = 1; c < n_out; ++c) zmax = z[c] > zmax ? z[c] : zmax;
            float e[16], s = 0.0f;
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                e[c] = c < n_out ? (float)exp((double)(z[c] - zmax)) : 0.0f;
                if (c < n_out) s = s + e[c];
            }
            float py = 0.0f;
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                if (c < n_out) {
                    const float p = e[c] / s;
                    if (c == yy) py = p;
                    Dn[c] = valid ? p - (c == yy ? 1.0f : 0.0f) : 0.0f;
                }
            }
            const float pc = fminf(fmaxf(py, eps), hi);
            loss = (float)-log((double)pc);
            if (py != py) loss = py;   // (fminf / fmaxf drop a NaN: the loss keeps it)
        }
        rowloss[t] = valid ? loss : 0.0f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int r = 0; r < kMlpFitRows; ++r) s = s + (double)rowloss[r];
        M.loss[slot0 + blockIdx.x] = s;
    }
}

// delta_l for 16 batch rows: sum over j of delta_{l+1}[r][j] W_l[i][j], times the derivative taken from the stored activation
__global__ __launch_bounds__(kMlpFitThreads) void mlp_fit_delta_kernel(const MlpFitDev M, int l, int nb) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ar = lane & 15, kk = lane >> 4;
    const int r0 = blockIdx.x * kMlpFitRows;
    const int K = M.sizes[l + 1], H = M.sizes[l];
    const int ntiles = (H + 15) / 16;
    const float *__restrict__ W = M.W[l];
    const float *__restrict__ Din = M.D[l + 1] + (int64_t)(r0 + ar) * K;   // (a row of the padded batch: zero beyond nb)
    f32x4 acc[kMaxTilesPerWave];
#pragma unroll
    for (int t = 0; t < kMaxTilesPerWave; ++t) acc[t] = f32x4{0, 0, 0, 0};
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int k = k0 + kk;
        const float a = k < K ? Din[k] : 0.0f;
#pragma unroll
        for (int t = 0; t < kMaxTilesPerWave; ++t) {
            const int tile = wave + 4 * t;
            if (tile < ntiles) {
                const int i = tile * 16 + ar;
                const float b = (k < K && i < H) ? W[(int64_t)i * K + k] : 0.0f;
                acc[t] = mma(a, b, acc[t]);
            }
        }
    }
    const float *__restrict__ Al = M.A[l];
    float *__restrict__ Dout = M.D[l];
#pragma unroll
    for (int t = 0; t < kMaxTilesPerWave; ++t) {
        const int tile = wave + 4 * t;
        if (tile < ntiles) {
            const int i = tile * 16 + ar;
            if (i < H) {
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int row = r0 + kk * 4 + reg;
                    const float a = Al[(int64_t)row * H + i];
                    float d = acc[t][reg];
                    switch (M.act) {
                        case WDX_MLP_ACT_RELU: d = a == 0.0f ? 0.0f : d; break;
                        case WDX_MLP_ACT_TANH: d = d * (1.0f - a * a); break;
                        case WDX_MLP_ACT_LOGISTIC: d = (d * a) * (1.0f - a); break;
                        default: break;
                    }
                    Dout[(int64_t)row * H + i] = row < nb ? d : 0.0f;
                }
            }
        }
    }
}

__device__ __forceinline__ float adam_update(float w, float g, float *__restrict__ mp, float *__restrict__ vp, const AdamArgs &a) {
    const float mo = a.beta1 * *mp + a.om_beta1 * g;
    const float vo = a.beta2 * *vp + a.om_beta2 * (g * g);
    *mp = mo;
    *vp = vo;
    return (float)((double)w + (-a.lr_t * (double)mo) / (double)(sqrtf(vo) + a.epsilon));
}

// one wave per 16 x 16 tile of W_l
__global__ __launch_bounds__(kMlpFitThreads) void mlp_fit_adam_kernel(const MlpFitDev M, int l, int64_t b0, int nb, int tiles_j, int n_tiles,
                                                                      int64_t l2_slot0, const AdamArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = blockIdx.x * kMlpFitWavesPerGroup + wave;
    if (tile >= n_tiles) return;   // wave-uniform; the kernel has no barrier
    const int ar = lane & 15, kk = lane >> 4;
    const int K = M.sizes[l], H = M.sizes[l + 1];
    const int i0 = (tile / tiles_j) * 16, j0 = (tile % tiles_j) * 16;
    const float *__restrict__ D = M.D[l + 1];
    const float *__restrict__ Al = l == 0 ? M.xs : M.A[l];
    const int ia = i0 + ar, jb = j0 + ar;
    f32x4 acc = f32x4{0, 0, 0, 0};
    // (unrolled: the gathers of four steps are in flight together; the MFMA chain keeps its row order)
#pragma unroll 4
    for (int r0 = 0; r0 < nb; r0 += 4) {
        const int r = r0 + kk;
        float av = 0.0f, bv = 0.0f;
        if (r < nb) {
            const int64_t arow = l == 0 ? (int64_t)M.idx[b0 + r] : (int64_t)r;
            if (ia < K) av = Al[arow * K + ia];
            if (jb < H) bv = D[(int64_t)r * H + jb];
        }
        acc = mma(av, bv, acc);
    }
    const float nbf = (float)nb;
    float *__restrict__ W = M.W[l];
    double sq = 0.0;
    if (jb < H) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int i = i0 + kk * 4 + reg;
            if (i < K) {
                const int64_t at = (int64_t)i * H + jb;
                const float w = W[at];
                sq = sq + (double)w * (double)w;
                const float g = (acc[reg] + a.alpha * w) / nbf;
                W[at] = adam_update(w, g, M.mW[l] + at, M.vW[l] + at, a);
            }
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) sq = sq + __shfl_xor(sq, s);
    if (lane == 0) M.l2[l2_slot0 + tile] = sq;
    if (i0 == 0 && lane < 16 && jb < H) {   // the intercepts of these 16 columns: the column sum of delta in row order
        float s = 0.0f;
#pragma unroll 8
        for (int r = 0; r < nb; ++r) s = s + D[(int64_t)r * H + jb];
        const float g = s / nbf;
        M.B[l][jb] = adam_update(M.B[l][jb], g, M.mB[l] + jb, M.vB[l] + jb, a);
    }
}

int mlp_fit_refusal(const MlpFitPlan &P) {
    if (P.rc != WDX_SUCCESS) set_error("%s", P.msg);
    return P.rc;
}

// With the context's mutex held.  d_dist and d_y are device memory, everything else the caller's host memory.
int mlp_fit_locked(wdx_ctx *ctx, const MlpFitPlan &P, const float *d_dist, const int32_t *d_y, const wdx_mlp_fit_params &p,
                   const double *mean, const double *scale, float *const *coefs, float *const *intercepts, const int32_t *order,
                   double *loss_curve, int32_t *n_epochs, int32_t *state, hipStream_t s) {
    int rc;
    *n_epochs = 0;
    *state = WDX_MLP_FIT_MAX_EPOCHS;
    if ((rc = use_stream(ctx, s))) return rc;
    if ((rc = ctx->mlp_fit_ws.ensure((size_t)P.bytes))) return rc;
    uint8_t *const ws = (uint8_t *)ctx->mlp_fit_ws.p;
    const int nl = P.nl, F = P.sizes[0];
    const int64_t m = P.m;

    MlpFitDev M{};
    M.nl = nl, M.act = P.act, M.k = P.k, M.n_out = P.n_out, M.lds_ld = P.lds_ld;
    for (int l = 0; l <= nl; ++l) M.sizes[l] = P.sizes[l];
    M.xs = (const float *)(ws + P.off_xs);
    M.idx = (const int32_t *)(ws + P.off_idx);
    M.y = d_y;
    for (int l = 0; l < nl; ++l) {
        M.W[l] = (float *)(ws + P.off_w[l]), M.mW[l] = (float *)(ws + P.off_mw[l]), M.vW[l] = (float *)(ws + P.off_vw[l]);
        M.B[l] = (float *)(ws + P.off_b[l]), M.mB[l] = (float *)(ws + P.off_mb[l]), M.vB[l] = (float *)(ws + P.off_vb[l]);
    }
    for (int l = 1; l < nl; ++l) M.A[l] = (float *)(ws + P.off_act[l]);
    for (int l = 1; l <= nl; ++l) M.D[l] = (float *)(ws + P.off_delta[l]);
    M.loss = (double *)(ws + P.off_loss);
    M.l2 = (double *)(ws + P.off_l2);
    int32_t *const d_flags = (int32_t *)(ws + P.off_flags);
    double *const d_mean = (double *)(ws + P.off_mean), *const d_scale = (double *)(ws + P.off_scale);

    static LdsAttr attr;
    if ((rc = attr.ensure(mlp_fit_forward_kernel, (size_t)P.lds_bytes))) return rc;

    std::vector<double> h_loss((size_t)P.loss_slots), h_l2((size_t)P.l2_slots);
    std::vector<int32_t> iota;
    StreamDrain drain(s);   // every exit leaves no copy from or to the caller's memory in flight
    // moments, activations, deltas and slots start at zero; then the parameters and the scaler
    WDX_HIP_TRY(hipMemsetAsync(ws, 0, (size_t)P.bytes, s));
    for (int l = 0; l < nl; ++l) {
        WDX_HIP_TRY(hipMemcpyAsync(M.W[l], coefs[l], sizeof(float) * (size_t)P.sizes[l] * P.sizes[l + 1], hipMemcpyHostToDevice, s));
        WDX_HIP_TRY(hipMemcpyAsync(M.B[l], intercepts[l], sizeof(float) * (size_t)P.sizes[l + 1], hipMemcpyHostToDevice, s));
    }
    if (mean) WDX_HIP_TRY(hipMemcpyAsync(d_mean, mean, sizeof(double) * (size_t)F, hipMemcpyHostToDevice, s));
    if (scale) WDX_HIP_TRY(hipMemcpyAsync(d_scale, scale, sizeof(double) * (size_t)F, hipMemcpyHostToDevice, s));
    {
        const int64_t work = m * F;
        const unsigned grid = (unsigned)std::min<int64_t>((work + 255) / 256, 4096);
        hipLaunchKernelGGL(mlp_fit_scale_kernel, dim3(grid), dim3(256), 0, s, d_dist, m, P.ld, F, mean ? d_mean : nullptr,
                           scale ? d_scale : nullptr, (float *)(ws + P.off_xs), d_y, P.k, d_flags);
        WDX_HIP_TRY(hipGetLastError());
    }
    int32_t flags[2] = {0, 0};
    WDX_HIP_TRY(hipMemcpyAsync(flags, d_flags, sizeof flags, hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipStreamSynchronize(s));
    if (flags[1]) {
        set_error("mlp fit: a class index lies outside 0 .. %d", P.k - 1);
        return WDX_ERR_INVALID;
    }
    if (flags[0]) {
        *state = WDX_MLP_FIT_NONFINITE_INPUT;
        drain.done();
        return WDX_SUCCESS;
    }
    if (!order) {
        iota.resize((size_t)m);
        for (int64_t i = 0; i < m; ++i) iota[(size_t)i] = (int32_t)i;
        WDX_HIP_TRY(hipMemcpyAsync((void *)M.idx, iota.data(), sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, s));
    }

    AdamArgs a{};
    a.alpha = (float)p.alpha, a.beta1 = (float)p.beta1, a.om_beta1 = (float)(1.0 - p.beta1), a.beta2 = (float)p.beta2;
    a.om_beta2 = (float)(1.0 - p.beta2), a.epsilon = (float)p.epsilon;
    double best = INFINITY;
    int count = 0;
    int64_t t = 0;
    for (int e = 0; e < p.max_epochs; ++e) {
        if (order) {
            const int32_t *row = order + (int64_t)e * m;
            for (int64_t i = 0; i < m; ++i)
                if (row[i] < 0 || row[i] >= m) {
                    set_error("mlp fit: order[%d][%lld] = %d lies outside 0 .. %lld", e, (long long)i, row[i], (long long)(m - 1));
                    return WDX_ERR_INVALID;
                }
            WDX_HIP_TRY(hipMemcpyAsync((void *)M.idx, row, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, s));
        }
        {
            Timed timed(ctx, WDX_K_MLP_FIT, s);
            timed.n_launches = P.steps * P.launches_per_step();
            for (int64_t st = 0; st < P.steps; ++st) {
                const int nb = (int)P.rows_of_step(st);
                const int64_t b0 = st * P.batch;
                ++t;
                a.lr_t = p.lr * sqrt(1.0 - pow(p.beta2, (double)t)) / (1.0 - pow(p.beta1, (double)t));
                hipLaunchKernelGGL(mlp_fit_forward_kernel, dim3((unsigned)P.fwd_grid(nb)), dim3(kMlpFitThreads), (size_t)P.lds_bytes, s, M, b0,
                                   nb, st * P.fwd_tiles);
                for (int l = nl - 1; l >= 0; --l) {
                    if (l >= 1)
                        hipLaunchKernelGGL(mlp_fit_delta_kernel, dim3((unsigned)P.delta_grid(nb)), dim3(kMlpFitThreads), 0, s, M, l, nb);
                    hipLaunchKernelGGL(mlp_fit_adam_kernel, dim3((unsigned)P.adam_grid(l)), dim3(kMlpFitThreads), 0, s, M, l, b0, nb,
                                       P.w_tiles_j[l], P.w_tiles_i[l] * P.w_tiles_j[l], st * P.w_tiles + P.w_tile0[l], a);
                }
                WDX_HIP_TRY(hipGetLastError());
            }
        }
        WDX_HIP_TRY(hipMemcpyAsync(h_loss.data(), M.loss, sizeof(double) * h_loss.size(), hipMemcpyDeviceToHost, s));
        WDX_HIP_TRY(hipMemcpyAsync(h_l2.data(), M.l2, sizeof(double) * h_l2.size(), hipMemcpyDeviceToHost, s));
        WDX_HIP_TRY(hipStreamSynchronize(s));
        double total = 0.0;
        for (int64_t st = 0; st < P.steps; ++st) {
            double ce = 0.0, values = 0.0;
            const int64_t nt = P.fwd_grid(P.rows_of_step(st));
            for (int64_t b = 0; b < nt; ++b) ce += h_loss[(size_t)(st * P.fwd_tiles + b)];
            for (int64_t w = 0; w < P.w_tiles; ++w) values += h_l2[(size_t)(st * P.w_tiles + w)];
            total += ce + 0.5 * p.alpha * values;
        }
        const double loss = total / (double)m;
        loss_curve[e] = loss;
        *n_epochs = e + 1;
        if (!isfinite(loss)) {
            *state = WDX_MLP_FIT_NONFINITE_LOSS;
            break;
        }
        count = loss > best - p.tol ? count + 1 : 0;
        if (loss < best) best = loss;
        if (count > p.n_iter_no_change) {
            *state = WDX_MLP_FIT_TOL;
            break;
        }
    }
    for (int l = 0; l < nl; ++l) {
        WDX_HIP_TRY(hipMemcpyAsync(coefs[l], M.W[l], sizeof(float) * (size_t)P.sizes[l] * P.sizes[l + 1], hipMemcpyDeviceToHost, s));
        WDX_HIP_TRY(hipMemcpyAsync(intercepts[l], M.B[l], sizeof(float) * (size_t)P.sizes[l + 1], hipMemcpyDeviceToHost, s));
    }
    WDX_HIP_TRY(hipStreamSynchronize(s));
    drain.done();
    return WDX_SUCCESS;
}

bool have_weights(const wdx_mlp_fit_params *p, float *const *coefs, float *const *intercepts) {
    if (!p || !coefs || !intercepts || p->n_layers < 1 || p->n_layers > WDX_MLP_MAX_LAYERS) return coefs && intercepts;
    for (int l = 0; l < p->n_layers; ++l)
        if (!coefs[l] || !intercepts[l]) return false;
    return true;
}

}  // namespace

}  // namespace wdx

using namespace wdx;

extern "C" {

int wdx_mlp_fit_device(wdx_ctx *ctx, const float *d_dist, int64_t m, int64_t ld, const int32_t *d_y, const wdx_mlp_fit_params *p,
                       const double *mean, const double *scale, float *const *coefs, float *const *intercepts, const int32_t *order,
                       double *loss_curve, int32_t *n_epochs, int32_t *state, void *stream) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    const MlpFitPlan P = mlp_fit_plan(m, ld, p, d_dist != nullptr, d_y != nullptr, have_weights(p, coefs, intercepts),
                                      loss_curve && n_epochs && state);
    if ((rc = mlp_fit_refusal(P))) return rc;
    return mlp_fit_locked(ctx, P, d_dist, d_y, *p, mean, scale, coefs, intercepts, order, loss_curve, n_epochs, state, (hipStream_t)stream);
}

int wdx_mlp_fit(wdx_ctx *ctx, const float *dist, int64_t m, int64_t ld, const int32_t *y, const wdx_mlp_fit_params *p, const double *mean,
                const double *scale, float *const *coefs, float *const *intercepts, const int32_t *order, double *loss_curve,
                int32_t *n_epochs, int32_t *state) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    MlpFitPlan P = mlp_fit_plan(m, ld, p, dist != nullptr, y != nullptr, have_weights(p, coefs, intercepts), loss_curve && n_epochs && state);
    if ((rc = mlp_fit_refusal(P))) return rc;
    hipStream_t s = ctx->stream;
    // the matrix and the class indices live for this call only
    struct Block {
        void *p = nullptr;
        ~Block() {
            if (p) (void)hipFree(p);
        }
    } Dm, Dy;
    const size_t F = (size_t)P.sizes[0];
    WDX_HIP_TRY(hipMalloc(&Dm.p, (size_t)m * F * sizeof(float)));
    WDX_HIP_TRY(hipMalloc(&Dy.p, (size_t)m * sizeof(int32_t)));
    {
        StreamDrain drain(s);
        WDX_HIP_TRY(hipMemcpy2DAsync(Dm.p, F * sizeof(float), dist, (size_t)ld * sizeof(float), F * sizeof(float), (size_t)m, hipMemcpyHostToDevice, s));
        WDX_HIP_TRY(hipMemcpyAsync(Dy.p, y, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, s));
        P.ld = (int64_t)F;
        rc = mlp_fit_locked(ctx, P, (const float *)Dm.p, (const int32_t *)Dy.p, *p, mean, scale, coefs, intercepts, order, loss_curve, n_epochs,
                            state, s);
    }   // (drained: nothing reads the two blocks when they are freed)
    return rc;
}

}  // extern "C"
