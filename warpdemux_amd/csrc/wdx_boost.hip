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
//     tail of the MLP kernel's epilogue, all by the read's own lane (boost_epilogue).
//
// A second kernel for minibatch-sized batches (boost_small_kernel; WDX_OPT_BOOST_KERNEL).  A 1000-read
// minibatch is 16 one-wave workgroups of the kernel above, each a dependent chain per tree.  Here one workgroup of 256
// threads serves WDX_BOOST_SMALL_READS reads and walks the trees in chunks of WDX_BOOST_TREE_CHUNK:
//   - phase A, lanes = trees: a thread loads its trees' headers and splits itself and computes the leaf index of every read
//     of the group (same float32 compare, same NaN rule); the indices go to LDS as uint16 [read][tree];
//   - phase B, lanes = (read, class): each walks the chunk's trees IN TREE ORDER, acc = acc + leaf value, one float64 add
//     per tree as above -- the gathers do not depend on acc, so sixteen are in flight while the adds stay in order;
//   - after the last chunk scale * acc + bias goes to LDS and one lane per read runs boost_epilogue.
// Only work that does not reorder a float64 sum is spread over lanes: raw, prob, pred and conf are those of the kernel
// above bit for bit.
#include "wdx_common.h"

#include <stdio.h>

#include <math.h>

namespace wdx {

namespace {

constexpr int kLanes = 64;
constexpr int kLd = kLanes + 1;  // floats per feature row in LDS

// What one lane does with the raw scores z[c] = scale * sum + bias of its read r: softmax / sigmoid in float64, np.argmax
// (first maximum), label map, top1 - top2 margin, threshold of the winning class; a read whose fingerprint failed gets
// pred -1 and NaN.  Both kernels end here, so their outputs are the same by construction.
template <int DMAX>
__device__ __forceinline__ void boost_epilogue(const BoostDev &M, const double (&z)[DMAX], int64_t r,
                                               const int32_t *__restrict__ status, double *__restrict__ raw,
                                               double *__restrict__ prob, int32_t *__restrict__ pred,
                                               double *__restrict__ conf) {
    constexpr int KMAX = DMAX == 1 ? 2 : DMAX;
    const int dim = M.dim, k = M.k;
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
    if (raw) {
#pragma unroll
        for (int c = 0; c < DMAX; ++c)
            if (c < dim) raw[r * dim + c] = z[c];
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

// DMAX: compile-time capacity of the per-lane accumulators (dim <= DMAX); k <= (DMAX == 1 ? 2 : DMAX)
template <int DMAX>
__global__ __launch_bounds__(kLanes) void boost_predict_kernel(BoostDev M, const double *__restrict__ fpt,
                                                               const int32_t *__restrict__ status, int64_t n,
                                                               double *__restrict__ raw, double *__restrict__ prob,
                                                               int32_t *__restrict__ pred, double *__restrict__ conf) {
    extern __shared__ __align__(16) float boost_x[];  // [n_features][kLd]
    const int lane = threadIdx.x;
    const int F = M.n_features, dim = M.dim;
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
    double z[DMAX];
#pragma unroll
    for (int c = 0; c < DMAX; ++c) z[c] = c < dim ? __dadd_rn(__dmul_rn(M.scale, acc[c]), M.bias[c]) : 0.0;
    boost_epilogue<DMAX>(M, z, r0 + lane, status, raw, prob, pred, conf);
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

// ---- the tree-parallel kernel for small batches ---------------------------------------------------------------------
constexpr int kSmallThreads = 256;
constexpr int kSmallReads = WDX_BOOST_SMALL_READS;  // reads of one workgroup
constexpr int kTreeChunk = WDX_BOOST_TREE_CHUNK;    // trees per pass of phase A + phase B
constexpr int kGather = 16;                         // leaf gathers of one (read, class) lane in flight
static_assert(kSmallReads * 16 <= kSmallThreads, "phase B: one lane per (read, class), dim <= 16");
static_assert(kSmallReads <= 64 && kTreeChunk % kGather == 0 && WDX_BOOST_MAX_DEPTH <= 16, "uint16 leaf indices, whole gather groups");
// dynamic LDS: [leaf index uint16 [read][tree of the chunk]][raw scores double [read][16]][rows float [read][feature]]
constexpr size_t kSmallLeafBytes = (size_t)kSmallReads * kTreeChunk * sizeof(uint16_t);
constexpr size_t kSmallRawBytes = (size_t)kSmallReads * 16 * sizeof(double);
static_assert(kSmallLeafBytes % 16 == 0, "the doubles behind the indices stay aligned");

template <int DMAX>
__global__ __launch_bounds__(kSmallThreads) void boost_small_kernel(BoostDev M, const double *__restrict__ fpt,
                                                                    const int32_t *__restrict__ status, int64_t n,
                                                                    double *__restrict__ raw, double *__restrict__ prob,
                                                                    int32_t *__restrict__ pred, double *__restrict__ conf) {
    extern __shared__ __align__(16) unsigned char boost_small_lds[];
    uint16_t *leaf_of = reinterpret_cast<uint16_t *>(boost_small_lds);                      // [kSmallReads][kTreeChunk]
    double *z_of = reinterpret_cast<double *>(boost_small_lds + kSmallLeafBytes);           // [kSmallReads][16]
    float *x_of = reinterpret_cast<float *>(boost_small_lds + kSmallLeafBytes + kSmallRawBytes);  // [kSmallReads][F]
    const int tid = threadIdx.x;
    const int F = M.n_features, dim = M.dim;
    const int64_t r0 = (int64_t)blockIdx.x * kSmallReads;
    const int rows = (int)(n - r0 < kSmallReads ? n - r0 : kSmallReads);

    // the group's rows are one contiguous block of rows * F doubles: [read][feature] as they lie; reads past the last: zeros
    const double *__restrict__ src = fpt + r0 * F;
    const int total = rows * F;
    for (int i = tid; i < kSmallReads * F; i += kSmallThreads) x_of[i] = i < total ? (float)src[i] : 0.0f;
    __syncthreads();

    const BoostTree *__restrict__ trees = M.trees;
    const BoostSplit *__restrict__ splits = M.splits;
    const double *__restrict__ leaves = M.leaves;
    const bool adds = tid < kSmallReads * dim;   // phase B lane (read br, class bc)
    const int br = adds ? tid / dim : 0, bc = adds ? tid - br * dim : 0;
    const uint16_t *lf = leaf_of + br * kTreeChunk;
    double acc = 0.0;   // lives across the chunks
    for (int c0 = 0; c0 < M.n_trees; c0 += kTreeChunk) {
        const int nt = M.n_trees - c0 < kTreeChunk ? M.n_trees - c0 : kTreeChunk;
        // phase A, lanes = trees
        for (int j = tid; j < nt; j += kSmallThreads) {
            const BoostTree T = trees[c0 + j];
            const BoostSplit *__restrict__ sp = splits + T.split0;
            unsigned leaf[kSmallReads];
#pragma unroll
            for (int r = 0; r < kSmallReads; ++r) leaf[r] = 0;
            for (int i = 0; i < T.depth; ++i) {
                const BoostSplit s = sp[i];
                const int f = (int)(s.feat & 0xffu);
                const bool nan_true = (s.feat >> 8) != 0u;
#pragma unroll
                for (int r = 0; r < kSmallReads; ++r) {
                    const float x = x_of[r * F + f];
                    // x > border in float32: false on equality and for a NaN, which follows the split's rule instead
                    const bool bit = (x > s.border) | ((x != x) & nan_true);
                    leaf[r] |= (unsigned)bit << i;
                }
            }
#pragma unroll
            for (int r = 0; r < kSmallReads; ++r) leaf_of[r * kTreeChunk + j] = (uint16_t)leaf[r];
        }
        __syncthreads();
        // phase B, lanes = (read, class): the chunk's trees in tree order, one float64 add per tree
        if (adds) {
            int j = 0;
            for (; j + kGather <= nt; j += kGather) {
                double v[kGather];
#pragma unroll
                for (int g = 0; g < kGather; ++g)
                    v[g] = leaves[trees[c0 + j + g].leaf0 + (int64_t)lf[j + g] * dim + bc];
#pragma unroll
                for (int g = 0; g < kGather; ++g) acc = __dadd_rn(acc, v[g]);
            }
            for (; j < nt; ++j) acc = __dadd_rn(acc, leaves[trees[c0 + j].leaf0 + (int64_t)lf[j] * dim + bc]);
        }
        __syncthreads();   // (the next chunk's phase A writes the indices this one read)
    }
    if (adds) z_of[br * 16 + bc] = __dadd_rn(__dmul_rn(M.scale, acc), M.bias[bc]);
    __syncthreads();
    if (tid >= rows) return;
    double z[DMAX];
#pragma unroll
    for (int c = 0; c < DMAX; ++c) z[c] = c < dim ? z_of[tid * 16 + c] : 0.0;
    boost_epilogue<DMAX>(M, z, r0 + tid, status, raw, prob, pred, conf);
}

template <int DMAX>
int launch_small(const BoostDev &M, const double *d_fpt, const int32_t *d_status, int64_t n, double *d_raw, double *d_prob,
                 int32_t *d_pred, double *d_conf, unsigned blocks, size_t lds, hipStream_t stream) {
    static LdsAttr attr;
    if (int rc = attr.ensure(boost_small_kernel<DMAX>, lds)) return rc;
    hipLaunchKernelGGL(boost_small_kernel<DMAX>, dim3(blocks), dim3(kSmallThreads), lds, stream, M, d_fpt, d_status, n, d_raw,
                       d_prob, d_pred, d_conf);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

}  // namespace

int launch_boost_predict(const BoostDev &M, const double *d_fpt, const int32_t *d_status, int64_t n, double *d_raw,
                         double *d_prob, int32_t *d_pred, double *d_conf, hipStream_t stream, const Knobs &knobs) {
    if (n == 0) return WDX_SUCCESS;
    // WDX_OPT_BOOST_KERNEL: 1 / 2 name the kernel; 0 takes the tree-parallel one up to WDX_BOOST_SMALL_MAX_READS reads
    const bool small = knobs.boost_kernel == 2 || (knobs.boost_kernel == 0 && n <= WDX_BOOST_SMALL_MAX_READS);
    const int per_block = small ? kSmallReads : kLanes;
    const int64_t blocks = (n + per_block - 1) / per_block;
    if (blocks > 0x7fffffff) {
        set_error("boost_predict: too many rows for one launch");
        return WDX_ERR_UNSUPPORTED;
    }
    if (M.n_features < 1 || M.n_features > kMaxBoostFeatures || M.dim < 1 || M.dim > 16 || M.k < 2 || M.k > 16 ||
        !(M.dim == M.k || (M.dim == 1 && M.k == 2))) {  // (wdx_boost_set_model has refused such a model already)
        set_error("boost_predict: model outside the kernel's limits");
        return WDX_ERR_UNSUPPORTED;
    }
    const unsigned b = (unsigned)blocks;
    if (knobs.debug_occ)
        fprintf(stderr, "wdx boost: %s kernel, %lld reads, %u workgroups\n", small ? "tree-parallel" : "lane-per-read", (long long)n, b);
    if (small) {
        const size_t lds = kSmallLeafBytes + kSmallRawBytes + (size_t)kSmallReads * M.n_features * sizeof(float);
        if (M.dim == 1) return launch_small<1>(M, d_fpt, d_status, n, d_raw, d_prob, d_pred, d_conf, b, lds, stream);
        if (M.dim <= 4) return launch_small<4>(M, d_fpt, d_status, n, d_raw, d_prob, d_pred, d_conf, b, lds, stream);
        if (M.dim <= 8) return launch_small<8>(M, d_fpt, d_status, n, d_raw, d_prob, d_pred, d_conf, b, lds, stream);
        return launch_small<16>(M, d_fpt, d_status, n, d_raw, d_prob, d_pred, d_conf, b, lds, stream);
    }
    const size_t lds = (size_t)M.n_features * kLd * sizeof(float);
    if (M.dim == 1) return launch<1>(M, d_fpt, d_status, n, d_raw, d_prob, d_pred, d_conf, b, lds, stream);
    if (M.dim <= 4) return launch<4>(M, d_fpt, d_status, n, d_raw, d_prob, d_pred, d_conf, b, lds, stream);
    if (M.dim <= 8) return launch<8>(M, d_fpt, d_status, n, d_raw, d_prob, d_pred, d_conf, b, lds, stream);
    return launch<16>(M, d_fpt, d_status, n, d_raw, d_prob, d_pred, d_conf, b, lds, stream);
}

}  // namespace wdx
