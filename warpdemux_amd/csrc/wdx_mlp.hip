// Classifier tail of DTW_MLP.predict on the device --
//   [StandardScaler.transform]*  MLPClassifier.predict_proba (_forward_pass_fast)   models/dtw_mlp.py:85
//   process_probs                                                                  models/utils.py:45-61
// on the (n, len(_X)) float32 distance rows, so that the matrix never has to leave HBM.
//
// One 256-thread workgroup per tile of 16 rows, every layer in the same launch:
//   - layer 1 streams the distance rows (scaled on the fly, bit for bit as scikit-learn: x - mean_ and / scale_ in float64,
//     each rounded to float32) against W1 through the matrix cores: v_mfma_f32_16x16x4_f32 for float32 models (an exact
//     f32 fmaf chain), v_mfma_f64_16x16x4_f64 for float64 models (distances widened exactly);
//   - the activations of a hidden layer stay in LDS (working dtype, so a float32 model rounds them like scikit-learn) and
//     are the A operand of the next layer;
//   - the epilogue adds the bias, applies the activation, and the output layer's softmax / logistic, argmax, label map,
//     top1 - top2 margin and thresholds are done per row by one lane.
// Column tiles of 16 units go round-robin to the four waves (<= 8 per wave: 512 units); a wave keeps all of its tiles'
// accumulators in registers so that each A element is loaded once per wave.  K remainders (fan-in % 4) and width
// remainders (fan-out % 16) are zero-padded operands; rows beyond n are zero rows whose results are dropped.
#include "wdx_common.h"

#include <math.h>

namespace wdx {

namespace {

constexpr int kTile = 16;       // rows per workgroup
constexpr int kThreads = 256;   // four waves
constexpr int kMaxTilesPerWave = kMaxMlpWidth / 16 / 4;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

template <typename T>
struct Mma;
template <>
struct Mma<float> {
    typedef f32x4 acc_t;
    static __device__ __forceinline__ acc_t step(float a, float b, acc_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    // C/D map of the f32 16x16x4 form: row (lane >> 4) * 4 + reg, column lane & 15
    static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) * 4 + reg; }
};
template <>
struct Mma<double> {
    typedef f64x4 acc_t;
    static __device__ __forceinline__ acc_t step(double a, double b, acc_t c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    // the f64 form has its own map: row (lane >> 4) + 4 * reg, column lane & 15
    static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) + 4 * reg; }
};

// hidden activations (sklearn ACTIVATIONS); the transcendental ones are evaluated in float64 and rounded once
template <typename T>
__device__ __forceinline__ T activate(T v, int act) {
    switch (act) {
        case WDX_MLP_ACT_LOGISTIC: return (T)(1.0 / (1.0 + exp(-(double)v)));
        case WDX_MLP_ACT_TANH: return (T)tanh((double)v);
        case WDX_MLP_ACT_RELU: return v > (T)0 ? v : (v == v ? (T)0 : v);  // np.maximum(x, 0) keeps NaN
        default: return v;
    }
}

// scaled first-layer input: each StandardScaler step on float32 input (x - mean_ and x / scale_ in float64, each rounded)
__device__ __forceinline__ float scale_input(const MlpDev &M, int64_t col, float x) {
    for (int s = 0; s < M.n_scalers; ++s) {
        if (M.mean[s]) x = (float)((double)x - M.mean[s][col]);
        if (M.scale[s]) x = (float)((double)x / M.scale[s][col]);
    }
    return x;
}

// One dense layer for the workgroup's 16 rows: out[r][j] = act(sum_k in[r][k] W[k][j] + b[j]).  FIRST: `in` is the
// distance tile in global memory (scaled on the fly, non-finite inputs flagged per row in `bad`), else LDS.
template <typename T, bool FIRST>
__device__ void dense_layer(const MlpDev &M, int layer, const float *__restrict__ dist, int64_t r0, int64_t n,
                            const T *lin, int ld_in, T *lout, int ld_out, int act, int *bad) {
    typedef typename Mma<T>::acc_t acc_t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = M.sizes[layer], H = M.sizes[layer + 1];
    const int ntiles = (H + 15) / 16;
    const T *__restrict__ W = (const T *)M.coef[layer];
    const T *__restrict__ B = (const T *)M.bias[layer];
    const int ar = lane & 15, kk = lane >> 4;
    acc_t acc[kMaxTilesPerWave];
#pragma unroll
    for (int t = 0; t < kMaxTilesPerWave; ++t) acc[t] = acc_t{0, 0, 0, 0};
    const int64_t row = r0 + ar;
    const bool row_ok = row < n;
    const float *drow = FIRST && row_ok ? dist + row * (int64_t)K : nullptr;
    bool nonfinite = false;
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int k = k0 + kk;
        T a = (T)0;
        if (FIRST) {
            if (row_ok && k < K) {
                const float x = scale_input(M, k, drow[k]);
                nonfinite |= !isfinite(x);
                a = (T)x;
            }
        } else {
            if (k < K) a = lin[ar * ld_in + k];
        }
#pragma unroll
        for (int t = 0; t < kMaxTilesPerWave; ++t) {
            const int tile = wave + 4 * t;
            if (tile < ntiles) {  // wave-uniform
                const int j = tile * 16 + ar;
                const T b = (k < K && j < H) ? W[(int64_t)k * H + j] : (T)0;
                acc[t] = Mma<T>::step(a, b, acc[t]);
            }
        }
    }
    if (FIRST && wave == 0) {  // every wave saw the whole tile; wave 0 reports its rows
        int f = nonfinite;
        f |= __shfl_xor(f, 16);
        f |= __shfl_xor(f, 32);
        if (lane < 16) bad[lane] = f;
    }
#pragma unroll
    for (int t = 0; t < kMaxTilesPerWave; ++t) {
        const int tile = wave + 4 * t;
        if (tile < ntiles) {
            const int j = tile * 16 + ar;
            if (j < H) {
                const T bj = B[j];
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const T v = acc[t][reg] + bj;  // a @ W, then += b: two roundings as in _forward_pass_fast
                    lout[Mma<T>::row(lane, reg) * ld_out + j] = activate<T>(v, act);
                }
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void mlp_forward_kernel(MlpDev M, const float *__restrict__ dist, int64_t n,
                                                               const int32_t *__restrict__ status,
                                                               double *__restrict__ prob, int32_t *__restrict__ pred,
                                                               double *__restrict__ conf,
                                                               unsigned long long *__restrict__ n_nonfinite) {
    extern __shared__ __align__(16) unsigned char mlp_lds[];
    __shared__ int bad[kTile];
    const int ld = M.ld;
    T *buf0 = (T *)mlp_lds;
    T *buf1 = buf0 + kTile * ld;
    const int64_t r0 = (int64_t)blockIdx.x * kTile;
    const int nl = M.n_layers;

    dense_layer<T, true>(M, 0, dist, r0, n, nullptr, 0, buf0, ld, nl == 1 ? WDX_MLP_ACT_IDENTITY : M.hidden_act, bad);
    __syncthreads();
    T *src = buf0, *dst = buf1;
    for (int l = 1; l < nl; ++l) {
        dense_layer<T, false>(M, l, nullptr, r0, n, src, ld, dst, ld,
                              l == nl - 1 ? WDX_MLP_ACT_IDENTITY : M.hidden_act, bad);
        __syncthreads();
        T *t = src;
        src = dst;
        dst = t;
    }

    // output activation + process_probs: one lane per row
    const int t = threadIdx.x;
    int counted = 0;
    if (t < kTile && r0 + t < n) {
        const int64_t r = r0 + t;
        const int k = M.k, nout = M.sizes[nl];
        const T *z = src + t * ld;
        const bool failed = status && status[r] != WDX_READ_OK;
        if (failed || bad[t]) {
            // failed fingerprint (never shown to the model) or non-finite input (scikit-learn refuses the call)
            counted = !failed;
            if (pred) pred[r] = -1;
            if (conf) conf[r] = __builtin_nan("");
            if (prob)
                for (int c = 0; c < k; ++c) prob[r * k + c] = __builtin_nan("");
        } else {
            T p[16];
            if (nout == 1) {
                // logistic output: predict_proba returns [1 - p, p], 1 - p in the working dtype
                const T q = (T)(1.0 / (1.0 + exp(-(double)z[0])));
                p[0] = (T)1 - q;
                p[1] = q;
            } else {
                // softmax: z - max in the working dtype (as scikit-learn), exp / sum in float64, one rounding
                T zmax = z[0];
                for (int c = 1; c < nout; ++c) zmax = z[c] > zmax ? z[c] : zmax;
                double e[16], s = 0.0;
                for (int c = 0; c < nout; ++c) {
                    e[c] = exp((double)(T)(z[c] - zmax));
                    s += e[c];
                }
                for (int c = 0; c < nout; ++c) p[c] = (T)(e[c] / s);
            }
            // np.argmax (first maximum), margin = top1 - top2 in the working dtype, threshold compared in float64
            int best = 0;
            T b1 = p[0], b2 = -INFINITY;
            for (int c = 1; c < k; ++c) {
                const T v = p[c];
                if (v > b1) {
                    b2 = b1;
                    b1 = v;
                    best = c;
                } else if (v > b2) {
                    b2 = v;
                }
            }
            const T margin = b1 - b2;
            int label = M.label_map ? M.label_map[best] : best;
            if (M.thresholds && (double)margin < M.thresholds[best]) label = -1;
            if (pred) pred[r] = label;
            if (conf) conf[r] = (double)margin;
            if (prob)
                for (int c = 0; c < k; ++c) prob[r * k + c] = (double)p[c];
        }
    }
    if (n_nonfinite && threadIdx.x < 64) {
        const unsigned long long m = __ballot(counted);
        if (threadIdx.x == 0 && m) atomicAdd(n_nonfinite, (unsigned long long)__popcll(m));
    }
}

template <typename T>
size_t mlp_lds_bytes(const MlpDev &M) {
    return sizeof(T) * 2 * kTile * (size_t)M.ld;
}

}  // namespace

int launch_mlp_predict(const MlpDev &M, const float *d_dist, int64_t n, const int32_t *d_status, double *d_prob,
                       int32_t *d_pred, double *d_conf, int64_t *d_n_nonfinite, hipStream_t stream) {
    if (n == 0) return WDX_SUCCESS;
    const int64_t tiles = (n + kTile - 1) / kTile;
    if (tiles > 0x7fffffff) {
        set_error("mlp_predict: too many rows for one launch");
        return WDX_ERR_UNSUPPORTED;
    }
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(d_n_nonfinite);
    if (M.dtype_bytes == 4) {
        const size_t lds = mlp_lds_bytes<float>(M);
        static LdsAttr attr;
        if (int rc = attr.ensure(mlp_forward_kernel<float>, lds)) return rc;
        hipLaunchKernelGGL(mlp_forward_kernel<float>, dim3((unsigned)tiles), dim3(kThreads), lds, stream, M, d_dist, n,
                           d_status, d_prob, d_pred, d_conf, cnt);
    } else {
        const size_t lds = mlp_lds_bytes<double>(M);
        static LdsAttr attr;
        if (int rc = attr.ensure(mlp_forward_kernel<double>, lds)) return rc;
        hipLaunchKernelGGL(mlp_forward_kernel<double>, dim3((unsigned)tiles), dim3(kThreads), lds, stream, M, d_dist, n,
                           d_status, d_prob, d_pred, d_conf, cnt);
    }
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

}  // namespace wdx
