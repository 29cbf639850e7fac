// Classifier tail of Fpt_Boost.predict on the device --
//   predict_proba of an ensemble of oblivious (symmetric) trees over float features    models/fpt_boost.py:45
//   process_probs                                                                      models/utils.py:45-61
// on the (n, n_features) float64 fingerprint rows, so that they never have to leave HBM.  The contract is the
// NumPy restatement in tests/helpers/boost_ref.py; parity with CatBoost itself is not pinned.
//
// One lane per read, one wave per workgroup:
//   - the wave's 64 rows are read coalesced, rounded to float32 once and kept in LDS as [feature][lane] (rows of 65 floats:
//     the per-feature reads are conflict-free, the transposing writes low-conflict -- 2-way where 64 consecutive elements
//     cross a row boundary, i.e. for every n_features < 64);
//   - the tree headers and the (feature, border) pairs are the same for every lane: wave-uniform loads; a level costs one
//     LDS read, one compare and one bit of the leaf index in a VGPR;
//   - the `dim` leaf doubles of a tree are gathered from global memory (the leaf table of a default-sized model is a few MB:
//     L2 / memory-side cache) and added in tree order, one float64 add per tree and class, never reassociated;
//   - raw = scale * sum + bias (float64 multiply, then add: not fused), softmax / sigmoid in float64, and the process_probs
//     tail of the MLP kernel's epilogue, all by the read's own lane.
#include "wdx_common.h"

#include <math.h>

namespace wdx {

namespace {

constexpr int kLanes = 64;
constexpr int kLd = kLanes + 1;  // floats per feature row in LDS

// DMAX: compile-time capacity of the per-lane accumulators (dim <= DMAX); k <= (DMAX == 1 ? 2 : DMAX)
template <int DMAX>
__global__ __launch_bounds__(kLanes) void boost_predict_kernel(BoostDev M, const double *__restrict__ fpt,
                                                               const int32_t *__restrict__ status, int64_t n,
                                                               double *__restrict__ raw, double *__restrict__ prob,
                                                               int32_t *__restrict__ pred, double *__restrict__ conf) {
    extern __shared__ __align__(16) float boost_x[];  // [n_features][kLd]
    constexpr int KMAX = DMAX == 1 ? 2 : DMAX;
    const int lane = threadIdx.x;
    const int F = M.n_features, dim = M.dim, k = M.k;
    const int64_t r0 = (int64_t)blockIdx.x * kLanes;
    const int rows = (int)(n - r0 < kLanes ? n - r0 : kLanes);

    // the wave's rows are one contiguous block of rows * F doubles
    const double *__restrict__ src = fpt + r0 * F;
    const int total = rows * F;
    for (int i = lane; i < total; i += kLanes) {
        const int row = i / F, col = i - row * F;
        boost_x[col * kLd + row] = (float)src[i];
    }
    if (lane >= rows)  // lanes without a read walk the trees on zeros; nothing of theirs is stored
        for (int col = 0; col < F; ++col) boost_x[col * kLd + lane] = 0.0f;
    __syncthreads();

    double acc[DMAX];
#pragma unroll
    for (int c = 0; c < DMAX; ++c) acc[c] = 0.0;
    const BoostTree *__restrict__ trees = M.trees;
    const BoostSplit *__restrict__ splits = M.splits;
    const double *__restrict__ leaves = M.leaves;
    for (int t = 0; t < M.n_trees; ++t) {
        const BoostTree T = trees[t];
        const BoostSplit *__restrict__ sp = splits + T.split0;
        unsigned leaf = 0;
        for (int i = 0; i < T.depth; ++i) {
            const BoostSplit s = sp[i];
            const float x = boost_x[(s.feat & 0xffu) * kLd + lane];
            // x > border in float32: false on equality and for a NaN, which follows the split's rule instead
            const bool bit = (x > s.border) | ((x != x) & ((s.feat >> 8) != 0u));
            leaf |= (unsigned)bit << i;
        }
        const double *__restrict__ lv = leaves + T.leaf0 + (int64_t)leaf * dim;
#pragma unroll
        for (int c = 0; c < DMAX; ++c)
            if (c < dim) acc[c] = __dadd_rn(acc[c], lv[c]);
    }

    if (lane >= rows) return;
    const int64_t r = r0 + lane;
    const double nan = __builtin_nan("");
    if (status && status[r] != WDX_READ_OK) {  // failed fingerprint: never shown to the model
        if (raw)
            for (int c = 0; c < dim; ++c) raw[r * dim + c] = nan;
        if (prob)
            for (int c = 0; c < k; ++c) prob[r * k + c] = nan;
        if (pred) pred[r] = -1;
        if (conf) conf[r] = nan;
        return;
    }
    double z[DMAX];
#pragma unroll
    for (int c = 0; c < DMAX; ++c) {
        z[c] = c < dim ? __dadd_rn(__dmul_rn(M.scale, acc[c]), M.bias[c]) : 0.0;
        if (raw && c < dim) raw[r * dim + c] = z[c];
    }
    double p[KMAX];
    if (DMAX == 1) {
        // Logloss: one raw value, p = [1 - sigmoid, sigmoid]
        const double q = 1.0 / (1.0 + exp(-z[0]));
        p[0] = 1.0 - q;
        p[1] = q;
    } else {
        // MultiClass: softmax with the row maximum subtracted, exp and sum in float64
        double zmax = z[0];
#pragma unroll
        for (int c = 1; c < DMAX; ++c)
            if (c < dim) zmax = z[c] > zmax ? z[c] : zmax;
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < DMAX; ++c)
            if (c < dim) {
                p[c] = exp(z[c] - zmax);
                s += p[c];
            }
#pragma unroll
        for (int c = 0; c < DMAX; ++c)
            if (c < dim) p[c] = p[c] / s;
    }
    // np.argmax (first maximum), margin = top1 - top2, threshold of the winning class
    int best = 0;
    double b1 = p[0], b2 = -INFINITY;
#pragma unroll
    for (int c = 1; c < KMAX; ++c)
        if (c < k) {
            const double v = p[c];
            if (v > b1) {
                b2 = b1;
                b1 = v;
                best = c;
            } else if (v > b2) {
                b2 = v;
            }
        }
    const double margin = b1 - b2;
    int label = M.label_map ? M.label_map[best] : best;
    if (M.thresholds && margin < M.thresholds[best]) label = -1;
    if (pred) pred[r] = label;
    if (conf) conf[r] = margin;
    if (prob) {
#pragma unroll
        for (int c = 0; c < KMAX; ++c)
            if (c < k) prob[r * k + c] = p[c];
    }
}

template <int DMAX>
int launch(const BoostDev &M, const double *d_fpt, const int32_t *d_status, int64_t n, double *d_raw, double *d_prob,
           int32_t *d_pred, double *d_conf, unsigned blocks, size_t lds, hipStream_t stream) {
    static LdsAttr attr;
    if (int rc = attr.ensure(boost_predict_kernel<DMAX>, lds)) return rc;
    hipLaunchKernelGGL(boost_predict_kernel<DMAX>, dim3(blocks), dim3(kLanes), lds, stream, M, d_fpt, d_status, n, d_raw,
                       d_prob, d_pred, d_conf);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

}  // namespace

int launch_boost_predict(const BoostDev &M, const double *d_fpt, const int32_t *d_status, int64_t n, double *d_raw,
                         double *d_prob, int32_t *d_pred, double *d_conf, hipStream_t stream) {
    if (n == 0) return WDX_SUCCESS;
    const int64_t blocks = (n + kLanes - 1) / kLanes;
    if (blocks > 0x7fffffff) {
        set_error("boost_predict: too many rows for one launch");
        return WDX_ERR_UNSUPPORTED;
    }
    if (M.n_features < 1 || M.n_features > kMaxBoostFeatures || M.dim < 1 || M.dim > 16 || M.k < 2 || M.k > 16 ||
        !(M.dim == M.k || (M.dim == 1 && M.k == 2))) {  // (wdx_boost_set_model has refused such a model already)
        set_error("boost_predict: model outside the kernel's limits");
        return WDX_ERR_UNSUPPORTED;
    }
    const size_t lds = (size_t)M.n_features * kLd * sizeof(float);
    const unsigned b = (unsigned)blocks;
    if (M.dim == 1) return launch<1>(M, d_fpt, d_status, n, d_raw, d_prob, d_pred, d_conf, b, lds, stream);
    if (M.dim <= 4) return launch<4>(M, d_fpt, d_status, n, d_raw, d_prob, d_pred, d_conf, b, lds, stream);
    if (M.dim <= 8) return launch<8>(M, d_fpt, d_status, n, d_raw, d_prob, d_pred, d_conf, b, lds, stream);
    return launch<16>(M, d_fpt, d_status, n, d_raw, d_prob, d_pred, d_conf, b, lds, stream);
}

}  // namespace wdx
