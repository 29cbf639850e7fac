// The three resident classifier models as the host sees them, stated once: the records the kernels take, what a setter
// refuses (check_*), the one host image of a model (pack_*) and the records' pointers put on a block that holds that image
// (bind_*).  Plain host C++17: no HIP, nothing of the context, so the system compiler builds it alone and a stand-alone
// program binds an image against its own bytes and reads every value back (tests/host/model_image_check.cpp).
// wdx_classify.hip adds what needs a device: the wait, the fresh block, the copy and the swap (install).
//
// IMAGE: one block per model, its pieces in the order below, 8-byte items first and int32 items last.  Every piece starts on
// a multiple of its element size relative to the block's base (a device block is 256-byte aligned); an absent piece takes no
// bytes and binds to a null pointer.
//   SVM    f64: dual_coef (k-1, n_sv) | rho | probA | probB [k(k-1)/2 each] | thresholds [k]? | coefT (n_sv, k-1)
//          i32: n_support [k] | start [k] | support [n_sv] | label_map [k]? | chunk_ref0 [2k + 1] | chunk_slot [2k]
//          (coefT and the chunk tables serve the fused DTW + SVM route: coefficients vector-major, two chunks per class)
//   MLP    f64: per scaler step mean [n_in]? | scale [n_in]? ; thresholds [k]?
//          working dtype (4 or 8 bytes): per layer W_i (sizes[i], sizes[i+1]) | b_i [sizes[i+1]]
//          i32 (on a multiple of 8): label_map [k]?
//   boost  f64: leaves | bias [dim] | thresholds [k]?
//          BoostTree [n_trees] (16 bytes, 8-byte aligned) | BoostSplit [sum(depth)]? (8 bytes, 4-byte aligned)
//          i32: label_map [k]?
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <vector>

#include "../../include/wdx.h"

namespace wdx {

// ---- SVM tail (wdx_svm.hip) -----------------------------------------------------------------------
struct SvmDev {  // device-resident SVC(kernel="precomputed", probability=True) + label map / thresholds
    const int32_t *n_support, *support, *start, *label_map;
    const double *dual_coef, *rho, *probA, *probB, *thresholds;  // label_map / thresholds nullable
    int k, n_sv, n_train, pwr;
    float ngamma;  // -gamma rounded to float32 (NumPy: python float * float32 array -> float32)
};
struct SvmFused {  // fused DTW + SVM route (wdx_dtw.hip: dtw_short_svm_kernel): its tables in the model's block
    const double *coefT;        // [n_sv][k - 1]: dual coefficients, vector-major
    const int32_t *chunk_ref0;  // [chunks + 1] first vector of each chunk (chunks never straddle a class)
    const int32_t *chunk_slot;  // [chunks] class * halves + half
    int chunks, halves;
};
struct SvmBound {
    SvmDev dev;
    SvmFused fused;
};

// ---- MLP tail (wdx_mlp.hip) -----------------------------------------------------------------------
struct MlpDev {  // device-resident [StandardScaler]* + MLPClassifier + label map / thresholds
    const void *coef[WDX_MLP_MAX_LAYERS], *bias[WDX_MLP_MAX_LAYERS];  // working dtype
    const double *mean[WDX_MLP_MAX_SCALERS], *scale[WDX_MLP_MAX_SCALERS];  // nullable per step
    const int32_t *label_map;  // nullable
    const double *thresholds;  // nullable
    int sizes[WDX_MLP_MAX_LAYERS + 1];
    int n_layers, n_scalers, dtype_bytes, hidden_act, k;
    int ld;  // row stride (elements) of the two LDS activation buffers
};

// ---- boost tail (wdx_boost.hip) --------------------------------------------------------------------
struct BoostTree {   // 16 bytes, read through wave-uniform loads
    int32_t split0;  // first split of the tree in `splits`
    int32_t depth;
    int64_t leaf0;   // first leaf value of the tree in `leaves`
};
struct BoostSplit {  // 8 bytes
    uint32_t feat;   // bits 0..7 the feature, bit 8 the NaN rule (1: a NaN feature sets the bit)
    float border;
};
struct BoostDev {  // device-resident oblivious-tree ensemble + label map / thresholds
    const BoostTree *trees;
    const BoostSplit *splits;
    const double *leaves, *bias;
    const int32_t *label_map;  // nullable
    const double *thresholds;  // nullable
    double scale;
    int n_trees, n_features, dim, k;
};

// ---- what a setter answers ---------------------------------------------------------------------------
struct ModelCheck {  // code != WDX_SUCCESS: refused, and msg is the setter's wdx_last_error()
    int code = WDX_SUCCESS;
    char msg[192] = "";
    explicit operator bool() const { return code != WDX_SUCCESS; }
};
__attribute__((format(printf, 2, 3))) inline ModelCheck refuse(int code, const char *fmt, ...) {
    ModelCheck r;
    r.code = code;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(r.msg, sizeof r.msg, fmt, ap);
    va_end(ap);
    return r;
}

// ---- the host image ------------------------------------------------------------------------------------
struct Piece {  // bytes == 0: absent
    size_t off = 0, bytes = 0, align = 1;
    const void *src = nullptr;  // the caller's array, copied by allocate(); null: pack_* computes the piece
};
enum { kSvmDualCoef, kSvmRho, kSvmProbA, kSvmProbB, kSvmThresholds, kSvmCoefT, kSvmNSupport, kSvmStart, kSvmSupport,
       kSvmLabelMap, kSvmChunkRef0, kSvmChunkSlot, kSvmPieces };
// (mean of step s, scale of step s) at kMlpScaler + 2 s, + 1; (W_i, b_i) at kMlpLayer + 2 i, + 1
enum { kMlpScaler = 0, kMlpThresholds = 2 * WDX_MLP_MAX_SCALERS, kMlpLayer, kMlpLabelMap = kMlpLayer + 2 * WDX_MLP_MAX_LAYERS,
       kMlpPieces };
enum { kBoostLeaves, kBoostBias, kBoostThresholds, kBoostTrees, kBoostSplits, kBoostLabelMap, kBoostPieces };
constexpr int kMaxPieces = kMlpPieces;

// Dev: the kind's record; `head` holds its scalars (for the SVM: SvmBound), every pointer null until bind_* gives a base
template <class Dev>
struct ModelImage {
    std::vector<unsigned char> bytes;
    Piece piece[kMaxPieces];
    size_t size = 0;  // of the pieces laid out so far; bytes.size() once packed
    Dev head{};

    // the next piece: `count` elements of `elem` bytes from `src` on a multiple of `align` (0: of elem); count 0: absent
    void add(int id, const void *src, size_t count, size_t elem, size_t align = 0) {
        align = align ? align : elem;
        const size_t at = (size + align - 1) / align * align;
        piece[id] = Piece{at, count * elem, align, src};
        if (count) size = at + count * elem;
    }
    // the bytes, with every piece the caller supplied; false: the host refused the staging copy
    bool allocate() {
        try {
            bytes.assign(size, 0);
        } catch (const std::bad_alloc &) {
            return false;
        }
        for (const Piece &p : piece)
            if (p.bytes && p.src) memcpy(bytes.data() + p.off, p.src, p.bytes);
        return true;
    }
    template <class T>
    T *host(int id) { return reinterpret_cast<T *>(bytes.data() + piece[id].off); }
    template <class T>
    const T *at(int id, const void *base) const {
        return piece[id].bytes ? reinterpret_cast<const T *>(static_cast<const unsigned char *>(base) + piece[id].off) : nullptr;
    }
};
using SvmImage = ModelImage<SvmBound>;
using MlpImage = ModelImage<MlpDev>;
using BoostImage = ModelImage<BoostDev>;

// ---- SVM ---------------------------------------------------------------------------------------------------
inline ModelCheck check_svm(const wdx_svm_model *m) {
    if (!m || m->n_classes < 2 || m->n_classes > 16 || m->n_sv < 1 || m->n_train < 1 || !m->n_support || !m->support ||
        !m->dual_coef || !m->rho || !m->probA || !m->probB || m->pwr_dist < 1)
        return refuse(WDX_ERR_INVALID, "svm_set_model: need 2..16 classes, support vectors, coefficients and Platt parameters");
    int64_t tot = 0;
    for (int c = 0; c < m->n_classes; ++c) {
        if (m->n_support[c] < 0) return refuse(WDX_ERR_INVALID, "svm_set_model: negative n_support");
        tot += m->n_support[c];
    }
    if (tot != m->n_sv) return refuse(WDX_ERR_INVALID, "svm_set_model: sum(n_support) != n_sv");
    for (int s = 0; s < m->n_sv; ++s)
        if (m->support[s] < 0 || m->support[s] >= m->n_train)
            return refuse(WDX_ERR_INVALID, "svm_set_model: support index out of range");
    return {};
}

// a model check_svm has accepted
inline ModelCheck pack_svm(const wdx_svm_model *m, SvmImage *img) {
    const int k = m->n_classes, nsv = m->n_sv, H = 2, nch = k * H;
    const size_t np = (size_t)k * (k - 1) / 2, nc = (size_t)(k - 1) * nsv;
    SvmImage &I = *img = SvmImage{};
    I.add(kSvmDualCoef, m->dual_coef, nc, 8), I.add(kSvmRho, m->rho, np, 8);
    I.add(kSvmProbA, m->probA, np, 8), I.add(kSvmProbB, m->probB, np, 8);
    I.add(kSvmThresholds, m->thresholds, m->thresholds ? k : 0, 8), I.add(kSvmCoefT, nullptr, nc, 8);
    I.add(kSvmNSupport, m->n_support, k, 4), I.add(kSvmStart, nullptr, k, 4), I.add(kSvmSupport, m->support, nsv, 4);
    I.add(kSvmLabelMap, m->label_map, m->label_map ? k : 0, 4);
    I.add(kSvmChunkRef0, nullptr, nch + 1, 4), I.add(kSvmChunkSlot, nullptr, nch, 4);
    if (!I.allocate()) return refuse(WDX_ERR_UNSUPPORTED, "svm_set_model: no host memory for a staging copy of %zu bytes", I.size);
    double *ct = I.host<double>(kSvmCoefT);
    for (int s = 0; s < nsv; ++s)
        for (int q = 0; q < k - 1; ++q) ct[(size_t)s * (k - 1) + q] = m->dual_coef[(size_t)q * nsv + s];
    int32_t *start = I.host<int32_t>(kSvmStart), *ref0 = I.host<int32_t>(kSvmChunkRef0), *slot = I.host<int32_t>(kSvmChunkSlot);
    int32_t tot = 0;
    for (int c = 0; c < k; ++c) {
        start[c] = ref0[2 * c] = tot;
        ref0[2 * c + 1] = tot + (m->n_support[c] + 1) / 2;
        slot[2 * c] = 2 * c, slot[2 * c + 1] = 2 * c + 1;
        tot += m->n_support[c];
    }
    ref0[nch] = nsv;
    SvmDev &S = I.head.dev;
    S.k = k, S.n_sv = nsv, S.n_train = m->n_train, S.pwr = m->pwr_dist;
    S.ngamma = (float)(-m->gamma);
    I.head.fused.chunks = nch, I.head.fused.halves = H;
    return {};
}

inline SvmBound bind_svm(const SvmImage &I, const void *base) {
    SvmBound B = I.head;
    SvmDev &S = B.dev;
    S.dual_coef = I.at<double>(kSvmDualCoef, base), S.rho = I.at<double>(kSvmRho, base);
    S.probA = I.at<double>(kSvmProbA, base), S.probB = I.at<double>(kSvmProbB, base);
    S.thresholds = I.at<double>(kSvmThresholds, base), B.fused.coefT = I.at<double>(kSvmCoefT, base);
    S.n_support = I.at<int32_t>(kSvmNSupport, base), S.start = I.at<int32_t>(kSvmStart, base);
    S.support = I.at<int32_t>(kSvmSupport, base), S.label_map = I.at<int32_t>(kSvmLabelMap, base);
    B.fused.chunk_ref0 = I.at<int32_t>(kSvmChunkRef0, base), B.fused.chunk_slot = I.at<int32_t>(kSvmChunkSlot, base);
    return B;
}

// ---- MLP ---------------------------------------------------------------------------------------------------
inline ModelCheck check_mlp(const wdx_mlp_model *m) {
    if (!m || (m->dtype_bytes != 4 && m->dtype_bytes != 8) || m->n_classes < 2 || m->n_layers < 1 || m->n_scalers < 0 ||
        m->hidden_activation < WDX_MLP_ACT_IDENTITY || m->hidden_activation > WDX_MLP_ACT_RELU)
        return refuse(WDX_ERR_INVALID,
                      "mlp_set_model: need a float32 / float64 model with >= 2 classes, layers and a known activation");
    const int nl = m->n_layers, k = m->n_classes;
    if (nl < 2 || nl > WDX_MLP_MAX_LAYERS)
        return refuse(WDX_ERR_UNSUPPORTED, "mlp_set_model: %d hidden layers (1..%d supported)", nl - 1, WDX_MLP_MAX_LAYERS - 1);
    if (k > 16) return refuse(WDX_ERR_UNSUPPORTED, "mlp_set_model: %d classes (2..16 supported)", k);
    if (m->n_scalers > WDX_MLP_MAX_SCALERS)
        return refuse(WDX_ERR_UNSUPPORTED, "mlp_set_model: %d scaler steps (at most %d supported)", m->n_scalers,
                      WDX_MLP_MAX_SCALERS);
    for (int i = 0; i <= nl; ++i)
        if (m->sizes[i] < 1) return refuse(WDX_ERR_INVALID, "mlp_set_model: layer size %d of entry %d", m->sizes[i], i);
    for (int i = 0; i < nl; ++i)
        if (!m->coefs[i] || !m->intercepts[i])
            return refuse(WDX_ERR_INVALID, "mlp_set_model: layer %d has no coefficients / intercepts", i);
    const int nout = m->sizes[nl];
    if (nout != k && !(nout == 1 && k == 2))
        return refuse(WDX_ERR_INVALID, "mlp_set_model: %d output units for %d classes", nout, k);
    for (int i = 1; i < nl; ++i)
        if (m->sizes[i] > WDX_MLP_MAX_WIDTH)
            return refuse(WDX_ERR_UNSUPPORTED, "mlp_set_model: hidden layer of %d units (at most %d supported)", m->sizes[i],
                          WDX_MLP_MAX_WIDTH);
    return {};
}

// a model check_mlp has accepted
inline ModelCheck pack_mlp(const wdx_mlp_model *m, MlpImage *img) {
    const int nl = m->n_layers, k = m->n_classes;
    const size_t n_in = (size_t)m->sizes[0], T = (size_t)m->dtype_bytes;
    MlpImage &I = *img = MlpImage{};
    MlpDev &M = I.head;
    for (int s = 0; s < m->n_scalers; ++s) {
        I.add(kMlpScaler + 2 * s, m->scaler_mean[s], m->scaler_mean[s] ? n_in : 0, 8);
        I.add(kMlpScaler + 2 * s + 1, m->scaler_scale[s], m->scaler_scale[s] ? n_in : 0, 8);
    }
    I.add(kMlpThresholds, m->thresholds, m->thresholds ? k : 0, 8);
    int widest = 16;
    for (int i = 0; i < nl; ++i) {
        I.add(kMlpLayer + 2 * i, m->coefs[i], (size_t)m->sizes[i] * m->sizes[i + 1], T);
        I.add(kMlpLayer + 2 * i + 1, m->intercepts[i], (size_t)m->sizes[i + 1], T);
        if (i > 0 && m->sizes[i] > widest) widest = m->sizes[i];
    }
    I.add(kMlpLabelMap, m->label_map, m->label_map ? k : 0, 4, 8);
    if (!I.allocate()) return refuse(WDX_ERR_UNSUPPORTED, "mlp_set_model: no host memory for a staging copy of %zu bytes", I.size);
    for (int i = 0; i <= nl; ++i) M.sizes[i] = m->sizes[i];
    M.n_layers = nl, M.n_scalers = m->n_scalers, M.dtype_bytes = m->dtype_bytes, M.hidden_act = m->hidden_activation, M.k = k;
    M.ld = (widest + 15) / 16 * 16 + 1;
    return {};
}

inline MlpDev bind_mlp(const MlpImage &I, const void *base) {
    MlpDev M = I.head;
    for (int s = 0; s < M.n_scalers; ++s)
        M.mean[s] = I.at<double>(kMlpScaler + 2 * s, base), M.scale[s] = I.at<double>(kMlpScaler + 2 * s + 1, base);
    for (int i = 0; i < M.n_layers; ++i)
        M.coef[i] = I.at<unsigned char>(kMlpLayer + 2 * i, base), M.bias[i] = I.at<unsigned char>(kMlpLayer + 2 * i + 1, base);
    M.thresholds = I.at<double>(kMlpThresholds, base), M.label_map = I.at<int32_t>(kMlpLabelMap, base);
    return M;
}

// ---- boost -------------------------------------------------------------------------------------------------
inline ModelCheck check_boost(const wdx_boost_model *m) {
    if (!m || m->n_trees < 1 || m->n_features < 1 || m->dim < 1 || m->n_classes < 2 || !m->depth || !m->leaf_values || !m->bias)
        return refuse(WDX_ERR_INVALID,
                      "boost_set_model: need >= 1 tree, >= 1 feature, >= 2 classes, depths, leaf values and a bias");
    const int nt = m->n_trees, F = m->n_features, dim = m->dim, k = m->n_classes;
    if (F > WDX_BOOST_MAX_FEATURES)
        return refuse(WDX_ERR_UNSUPPORTED, "boost_set_model: %d features (1..%d supported)", F, WDX_BOOST_MAX_FEATURES);
    if (dim > 16 || k > 16)
        return refuse(WDX_ERR_UNSUPPORTED, "boost_set_model: %d values per leaf for %d classes (1..16 and 2..16 supported)", dim, k);
    if (dim != k && !(dim == 1 && k == 2))
        return refuse(WDX_ERR_INVALID, "boost_set_model: %d values per leaf for %d classes", dim, k);
    size_t n_splits = 0;
    for (int t = 0; t < nt; ++t) {
        const int d = m->depth[t];
        if (d < 0) return refuse(WDX_ERR_INVALID, "boost_set_model: tree %d has depth %d", t, d);
        if (d > WDX_BOOST_MAX_DEPTH)
            return refuse(WDX_ERR_UNSUPPORTED, "boost_set_model: tree %d has depth %d (0..%d supported)", t, d, WDX_BOOST_MAX_DEPTH);
        n_splits += (size_t)d;
    }
    if (n_splits > 0x7fffffff) return refuse(WDX_ERR_UNSUPPORTED, "boost_set_model: too many splits");
    if (n_splits && (!m->split_feature || !m->split_border))
        return refuse(WDX_ERR_INVALID, "boost_set_model: splits without features / borders");
    for (size_t i = 0; i < n_splits; ++i)
        if (m->split_feature[i] < 0 || m->split_feature[i] >= F)
            return refuse(WDX_ERR_INVALID, "boost_set_model: split %lld tests feature %d of %d", (long long)i, m->split_feature[i], F);
    return {};
}

// a model check_boost has accepted (any number of trees is: the staging copy can be refused by the host)
inline ModelCheck pack_boost(const wdx_boost_model *m, BoostImage *img) {
    const int nt = m->n_trees, dim = m->dim, k = m->n_classes;
    size_t n_splits = 0, n_leaves = 0;
    for (int t = 0; t < nt; ++t) n_splits += (size_t)m->depth[t], n_leaves += (size_t)1 << m->depth[t];
    BoostImage &I = *img = BoostImage{};
    I.add(kBoostLeaves, m->leaf_values, n_leaves * dim, 8), I.add(kBoostBias, m->bias, dim, 8);
    I.add(kBoostThresholds, m->thresholds, m->thresholds ? k : 0, 8);
    I.add(kBoostTrees, nullptr, nt, sizeof(BoostTree), 8), I.add(kBoostSplits, nullptr, n_splits, sizeof(BoostSplit), 4);
    I.add(kBoostLabelMap, m->label_map, m->label_map ? k : 0, 4);
    if (!I.allocate()) return refuse(WDX_ERR_UNSUPPORTED, "boost_set_model: no host memory for a staging copy of %zu bytes", I.size);
    BoostTree *ht = I.host<BoostTree>(kBoostTrees);
    size_t s0 = 0, l0 = 0;
    for (int t = 0; t < nt; ++t) {
        ht[t] = BoostTree{(int32_t)s0, m->depth[t], (int64_t)l0};
        s0 += (size_t)m->depth[t];
        l0 += ((size_t)1 << m->depth[t]) * dim;
    }
    BoostSplit *hs = I.host<BoostSplit>(kBoostSplits);
    for (size_t i = 0; i < n_splits; ++i)
        hs[i] = BoostSplit{(uint32_t)m->split_feature[i] | ((m->split_nan_true && m->split_nan_true[i]) ? 0x100u : 0u),
                           m->split_border[i]};
    BoostDev &M = I.head;
    M.scale = m->scale, M.n_trees = nt, M.n_features = m->n_features, M.dim = dim, M.k = k;
    return {};
}

inline BoostDev bind_boost(const BoostImage &I, const void *base) {
    BoostDev M = I.head;
    M.leaves = I.at<double>(kBoostLeaves, base), M.bias = I.at<double>(kBoostBias, base);
    M.thresholds = I.at<double>(kBoostThresholds, base), M.label_map = I.at<int32_t>(kBoostLabelMap, base);
    M.trees = I.at<BoostTree>(kBoostTrees, base), M.splits = I.at<BoostSplit>(kBoostSplits, base);
    return M;
}

}  // namespace wdx
