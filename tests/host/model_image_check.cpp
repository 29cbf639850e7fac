// Stand-alone sweep of warpdemux_amd/csrc/wdx_model_image.h -- what the three classifier setters refuse, the one host image
// of a model and the kernels' records bound to it -- built by tests/test_model_image_host.py with the system compiler and the
// address / undefined-behaviour sanitizers.  For every synthetic model of the sweep: check_* accepts it, pack_* lays it out,
// bind_* puts the record on the image's OWN bytes (base = image.bytes.data()), and every value is read back through the
// record's pointers and compared with the caller's arrays; every piece is aligned to its element type, lies inside the image
// and overlaps no other; a piece the caller left out is a null pointer.  The image is bound a second time on a copy of its
// bytes, and every pointer must lie as far behind that base as behind the first.
//   SVM    k = 2..16; per class n_support of 0, 1, an odd and an even value in four rotations; thresholds / label_map each
//          present and absent
//   MLP    float32 and float64; 1 .. WDX_MLP_MAX_LAYERS - 1 hidden layers of 1, 16, 17, WDX_MLP_MAX_WIDTH units (every
//          width in every position for up to two hidden layers, rotated beyond); 0 .. WDX_MLP_MAX_SCALERS scaler steps
//          with mean only, scale only, both and neither; the 1-output 2-class form and k outputs for k = 2, 3, 16
//   boost  depths 0 and WDX_BOOST_MAX_DEPTH and mixed; depth-0 trees only (no splits: null split pointers in and out);
//          dim 1 with k 2, dim = k = 2, 5, 16; n_features 1 and WDX_BOOST_MAX_FEATURES; the NaN rule absent, 0 and 1
// Then every refusal of the three setters once, with its code and the message word for word.
// Exit status 0 and "<models> models <refusals> refusals" on stderr; a failure is named on stderr and ends the run.
#include "wdx_model_image.h"

#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

using namespace wdx;

static long long models = 0, refusals = 0;

#define REQUIRE(cond, ...)                                       \
    do {                                                         \
        if (!(cond)) {                                           \
            fprintf(stderr, "FAILED: %s -- ", #cond);            \
            fprintf(stderr, __VA_ARGS__);                        \
            fprintf(stderr, " (%s:%d)\n", __FILE__, __LINE__);   \
            exit(1);                                             \
        }                                                        \
    } while (0)

// a value no two positions of one model share
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t next_u64() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return rng_state >> 11;
}
static double next_f64() { return (double)(next_u64() % 2000001) / 1000.0 - 1000.0; }
static std::vector<double> doubles(size_t n) {
    std::vector<double> v(n);
    for (double &x : v) x = next_f64();
    return v;
}
static std::vector<int32_t> ints(size_t n, int32_t below) {
    std::vector<int32_t> v(n);
    for (int32_t &x : v) x = (int32_t)(next_u64() % (uint64_t)below);
    return v;
}

// every piece inside the image, aligned to `align` and to its element, and no two pieces overlapping
template <class Image>
static void check_pieces(const Image &I, const char *kind) {
    REQUIRE(I.bytes.size() == I.size, "%s: %zu bytes packed, %zu laid out", kind, I.bytes.size(), I.size);
    for (int a = 0; a < kMaxPieces; ++a) {
        const Piece &p = I.piece[a];
        if (!p.bytes) continue;
        REQUIRE(p.off % p.align == 0, "%s: piece %d at %zu is not on a multiple of %zu", kind, a, p.off, p.align);
        REQUIRE(p.off + p.bytes <= I.bytes.size(), "%s: piece %d ends at %zu of %zu", kind, a, p.off + p.bytes, I.bytes.size());
        for (int b = 0; b < a; ++b) {
            const Piece &q = I.piece[b];
            REQUIRE(!q.bytes || q.off + q.bytes <= p.off || p.off + p.bytes <= q.off, "%s: pieces %d and %d overlap", kind, b, a);
        }
    }
}
template <class T>
static void aligned(const T *p, const void *base, const char *what) {
    if (p) REQUIRE(((const unsigned char *)p - (const unsigned char *)base) % alignof(T) == 0 && (uintptr_t)p % alignof(T) == 0,
                   "%s is misaligned for its element type", what);
}
static void aligned_to(const void *p, size_t a, const char *what) {
    if (p) REQUIRE((uintptr_t)p % a == 0, "%s is misaligned for its element type", what);
}
// the same piece bound on two bases: both null, or as far behind the one base as behind the other
static void moved(const void *p0, const void *p1, const void *b0, const void *b1, const char *what) {
    REQUIRE((!p0 && !p1) || (p0 && p1 && (uintptr_t)p1 - (uintptr_t)b1 == (uintptr_t)p0 - (uintptr_t)b0),
            "%s does not follow the base", what);
}
static bool same(const void *a, const void *b, size_t bytes) { return bytes == 0 || memcmp(a, b, bytes) == 0; }

// ---- SVM -----------------------------------------------------------------------------------------------------

struct SvmCase {
    wdx_svm_model m{};
    std::vector<int32_t> n_support, support, label_map;
    std::vector<double> dual_coef, rho, probA, probB, thresholds;
};
static void make_svm(SvmCase &c, int k, int rot, bool thr, bool lab) {
    static const int counts[4] = {0, 1, 5, 8};
    c.n_support.resize(k);
    int nsv = 0;
    for (int i = 0; i < k; ++i) nsv += c.n_support[i] = counts[(i + rot) % 4];
    // (two neighbours of the cycle are never both 0: n_sv >= 1)
    const int n_train = nsv + 7, np = k * (k - 1) / 2;
    c.support = ints(nsv, n_train);
    c.dual_coef = doubles((size_t)(k - 1) * nsv);
    c.rho = doubles(np), c.probA = doubles(np), c.probB = doubles(np);
    c.thresholds = doubles(k);
    c.label_map = ints(k, 100);
    c.m = wdx_svm_model{k, nsv, n_train, 1 + rot % 3, 0.25 * (rot + 1), c.n_support.data(), c.support.data(), c.dual_coef.data(),
                        c.rho.data(), c.probA.data(), c.probB.data(), lab ? c.label_map.data() : nullptr,
                        thr ? c.thresholds.data() : nullptr};
}
static void check_svm_model(const SvmCase &c) {
    const wdx_svm_model &m = c.m;
    const int k = m.n_classes, nsv = m.n_sv, np = k * (k - 1) / 2;
    ModelCheck r = check_svm(&m);
    REQUIRE(!r, "svm k=%d refused: %s", k, r.msg);
    SvmImage I;
    r = pack_svm(&m, &I);
    REQUIRE(!r, "svm k=%d not packed: %s", k, r.msg);
    check_pieces(I, "svm");
    const unsigned char *base = I.bytes.data();
    const SvmBound B = bind_svm(I, base);
    const SvmDev &S = B.dev;
    REQUIRE(S.k == k && S.n_sv == nsv && S.n_train == m.n_train && S.pwr == m.pwr_dist && S.ngamma == (float)(-m.gamma), "svm scalars");
    REQUIRE(B.fused.chunks == 2 * k && B.fused.halves == 2, "svm chunk counts");
    aligned(S.dual_coef, base, "dual_coef"), aligned(S.rho, base, "rho"), aligned(S.probA, base, "probA");
    aligned(S.probB, base, "probB"), aligned(S.thresholds, base, "thresholds"), aligned(B.fused.coefT, base, "coefT");
    aligned(S.n_support, base, "n_support"), aligned(S.start, base, "start"), aligned(S.support, base, "support");
    aligned(S.label_map, base, "label_map"), aligned(B.fused.chunk_ref0, base, "chunk_ref0"), aligned(B.fused.chunk_slot, base, "chunk_slot");
    REQUIRE(same(S.dual_coef, m.dual_coef, (size_t)(k - 1) * nsv * 8), "dual_coef");
    REQUIRE(same(S.rho, m.rho, np * 8) && same(S.probA, m.probA, np * 8) && same(S.probB, m.probB, np * 8), "rho / probA / probB");
    REQUIRE(same(S.n_support, m.n_support, k * 4) && same(S.support, m.support, nsv * 4), "n_support / support");
    REQUIRE(m.thresholds ? S.thresholds && same(S.thresholds, m.thresholds, k * 8) : !S.thresholds, "thresholds");
    REQUIRE(m.label_map ? S.label_map && same(S.label_map, m.label_map, k * 4) : !S.label_map, "label_map");
    int32_t tot = 0;
    for (int cl = 0; cl < k; ++cl) {
        REQUIRE(S.start[cl] == tot, "start[%d] = %d, want %d", cl, S.start[cl], tot);
        REQUIRE(B.fused.chunk_ref0[2 * cl] == tot && B.fused.chunk_ref0[2 * cl + 1] == tot + (m.n_support[cl] + 1) / 2,
                "chunk_ref0 of class %d", cl);
        REQUIRE(B.fused.chunk_slot[2 * cl] == 2 * cl && B.fused.chunk_slot[2 * cl + 1] == 2 * cl + 1, "chunk_slot of class %d", cl);
        tot += m.n_support[cl];
    }
    REQUIRE(B.fused.chunk_ref0[2 * k] == nsv, "chunk_ref0 ends at n_sv");
    for (int s = 0; s < nsv; ++s)
        for (int q = 0; q < k - 1; ++q)
            REQUIRE(same(&B.fused.coefT[(size_t)s * (k - 1) + q], &m.dual_coef[(size_t)q * nsv + s], 8), "coefT[%d][%d]", s, q);
    // another base (a copy of the image): every pointer moves with it
    const std::vector<unsigned char> copy(I.bytes);
    const unsigned char *far = copy.data();
    const SvmBound F = bind_svm(I, far);
    moved(S.dual_coef, F.dev.dual_coef, base, far, "dual_coef"), moved(S.rho, F.dev.rho, base, far, "rho");
    moved(S.probA, F.dev.probA, base, far, "probA"), moved(S.probB, F.dev.probB, base, far, "probB");
    moved(S.thresholds, F.dev.thresholds, base, far, "thresholds"), moved(S.n_support, F.dev.n_support, base, far, "n_support");
    moved(S.start, F.dev.start, base, far, "start"), moved(S.support, F.dev.support, base, far, "support");
    moved(S.label_map, F.dev.label_map, base, far, "label_map"), moved(B.fused.coefT, F.fused.coefT, base, far, "coefT");
    moved(B.fused.chunk_ref0, F.fused.chunk_ref0, base, far, "chunk_ref0");
    moved(B.fused.chunk_slot, F.fused.chunk_slot, base, far, "chunk_slot");
    ++models;
}
static void sweep_svm() {
    for (int k = 2; k <= 16; ++k)
        for (int rot = 0; rot < 4; ++rot)
            for (int opt = 0; opt < 4; ++opt) {
                SvmCase c;
                make_svm(c, k, rot, opt & 1, opt & 2);
                check_svm_model(c);
            }
}

// ---- MLP -----------------------------------------------------------------------------------------------------

struct MlpCase {
    wdx_mlp_model m{};
    std::vector<std::vector<unsigned char>> coefs, intercepts;
    std::vector<std::vector<double>> mean, scale;
    std::vector<int32_t> label_map;
    std::vector<double> thresholds;
};
static std::vector<unsigned char> working(size_t n, int T) {
    std::vector<unsigned char> v(n * T);
    for (size_t i = 0; i < n; ++i) {
        const double d = next_f64();
        const float f = (float)d;
        memcpy(v.data() + i * T, T == 4 ? (const void *)&f : (const void *)&d, T);
    }
    return v;
}
// scalers[s]: 0 neither, 1 mean only, 2 scale only, 3 both
static void make_mlp(MlpCase &c, int T, const std::vector<int> &hidden, int n_in, int k, int nout, const std::vector<int> &scalers,
                     bool thr, bool lab) {
    wdx_mlp_model &m = c.m;
    m.n_layers = (int)hidden.size() + 1;
    m.dtype_bytes = T;
    m.hidden_activation = WDX_MLP_ACT_IDENTITY + (int)(hidden.size() % 4);
    m.n_classes = k;
    m.n_scalers = (int)scalers.size();
    m.sizes[0] = n_in;
    for (size_t i = 0; i < hidden.size(); ++i) m.sizes[i + 1] = hidden[i];
    m.sizes[m.n_layers] = nout;
    c.coefs.resize(m.n_layers), c.intercepts.resize(m.n_layers);
    for (int i = 0; i < m.n_layers; ++i) {
        c.coefs[i] = working((size_t)m.sizes[i] * m.sizes[i + 1], T);
        c.intercepts[i] = working(m.sizes[i + 1], T);
        m.coefs[i] = c.coefs[i].data(), m.intercepts[i] = c.intercepts[i].data();
    }
    c.mean.resize(scalers.size()), c.scale.resize(scalers.size());
    for (size_t s = 0; s < scalers.size(); ++s) {
        c.mean[s] = doubles(n_in), c.scale[s] = doubles(n_in);
        m.scaler_mean[s] = (scalers[s] & 1) ? c.mean[s].data() : nullptr;
        m.scaler_scale[s] = (scalers[s] & 2) ? c.scale[s].data() : nullptr;
    }
    c.thresholds = doubles(k), c.label_map = ints(k, 100);
    m.thresholds = thr ? c.thresholds.data() : nullptr;
    m.label_map = lab ? c.label_map.data() : nullptr;
}
static void check_mlp_model(const MlpCase &c) {
    const wdx_mlp_model &m = c.m;
    const int nl = m.n_layers, k = m.n_classes, T = m.dtype_bytes, n_in = m.sizes[0];
    ModelCheck r = check_mlp(&m);
    REQUIRE(!r, "mlp refused: %s", r.msg);
    MlpImage I;
    r = pack_mlp(&m, &I);
    REQUIRE(!r, "mlp not packed: %s", r.msg);
    check_pieces(I, "mlp");
    const std::vector<unsigned char> copy(I.bytes);
    const unsigned char *base = I.bytes.data(), *far = copy.data();
    const MlpDev M = bind_mlp(I, base), F = bind_mlp(I, far);
    int widest = 16;
    for (int i = 1; i < nl; ++i) widest = m.sizes[i] > widest ? m.sizes[i] : widest;
    REQUIRE(M.ld == (widest + 15) / 16 * 16 + 1, "ld = %d for a widest hidden layer of %d", M.ld, widest);
    REQUIRE(M.n_layers == nl && M.n_scalers == m.n_scalers && M.dtype_bytes == T && M.hidden_act == m.hidden_activation && M.k == k,
            "mlp scalars");
    for (int i = 0; i <= nl; ++i) REQUIRE(M.sizes[i] == m.sizes[i], "sizes[%d]", i);
    for (int i = 0; i < WDX_MLP_MAX_LAYERS; ++i) {
        if (i >= nl) {
            REQUIRE(!M.coef[i] && !M.bias[i], "layer %d of %d is bound", i, nl);
            continue;
        }
        aligned_to(M.coef[i], T, "coef"), aligned_to(M.bias[i], T, "bias");
        REQUIRE(M.coef[i] && same(M.coef[i], m.coefs[i], (size_t)m.sizes[i] * m.sizes[i + 1] * T), "coefs[%d]", i);
        REQUIRE(M.bias[i] && same(M.bias[i], m.intercepts[i], (size_t)m.sizes[i + 1] * T), "intercepts[%d]", i);
        moved(M.coef[i], F.coef[i], base, far, "coef"), moved(M.bias[i], F.bias[i], base, far, "bias");
    }
    for (int s = 0; s < WDX_MLP_MAX_SCALERS; ++s) {
        const double *mean = s < m.n_scalers ? m.scaler_mean[s] : nullptr, *scale = s < m.n_scalers ? m.scaler_scale[s] : nullptr;
        aligned(M.mean[s], base, "mean"), aligned(M.scale[s], base, "scale");
        REQUIRE(mean ? M.mean[s] && same(M.mean[s], mean, (size_t)n_in * 8) : !M.mean[s], "mean of step %d", s);
        REQUIRE(scale ? M.scale[s] && same(M.scale[s], scale, (size_t)n_in * 8) : !M.scale[s], "scale of step %d", s);
        moved(M.mean[s], F.mean[s], base, far, "mean"), moved(M.scale[s], F.scale[s], base, far, "scale");
    }
    aligned(M.thresholds, base, "thresholds"), aligned(M.label_map, base, "label_map");
    REQUIRE(m.thresholds ? M.thresholds && same(M.thresholds, m.thresholds, k * 8) : !M.thresholds, "thresholds");
    REQUIRE(m.label_map ? M.label_map && same(M.label_map, m.label_map, k * 4) : !M.label_map, "label_map");
    moved(M.thresholds, F.thresholds, base, far, "thresholds"), moved(M.label_map, F.label_map, base, far, "label_map");
    ++models;
}
static void sweep_mlp() {
    static const int widths[4] = {1, 16, 17, WDX_MLP_MAX_WIDTH};
    static const int outs[4][2] = {{2, 1}, {2, 2}, {3, 3}, {16, 16}};   // (k, output units)
    int turn = 0;
    for (int T : {4, 8})
        for (int nh = 1; nh <= WDX_MLP_MAX_LAYERS - 1; ++nh)
            for (int w0 = 0; w0 < 4; ++w0)
                for (int w1 = 0; w1 < (nh > 1 ? 4 : 1); ++w1)
                    for (int ns = 0; ns <= WDX_MLP_MAX_SCALERS; ++ns)
                        for (int kind = 0; kind < (ns ? 4 : 1); ++kind, ++turn) {
                            std::vector<int> hidden(nh), scalers(ns);
                            for (int i = 0; i < nh; ++i) hidden[i] = widths[i == 0 ? w0 : i == 1 ? w1 : (w0 + w1 + i + turn) % 4];
                            // step 0 takes the kind of this turn, the later ones rotate through all four
                            for (int s = 0; s < ns; ++s) scalers[s] = (kind + s * (1 + turn % 3)) % 4;
                            MlpCase c;
                            make_mlp(c, T, hidden, widths[turn % 4] + turn % 3, outs[turn % 4][0], outs[turn % 4][1], scalers,
                                     turn & 1, turn & 2);
                            check_mlp_model(c);
                        }
}

// ---- boost ---------------------------------------------------------------------------------------------------

struct BoostCase {
    wdx_boost_model m{};
    std::vector<int32_t> depth, split_feature, label_map;
    std::vector<float> split_border;
    std::vector<uint8_t> nan_true;
    std::vector<double> leaves, bias, thresholds;
};
// nan: 0 no array, 1 an array of 0 / 1
static void make_boost(BoostCase &c, const std::vector<int> &depths, int dim, int k, int F, int nan, bool thr, bool lab) {
    c.depth.assign(depths.begin(), depths.end());
    size_t ns = 0, nleaf = 0;
    for (int d : depths) ns += d, nleaf += (size_t)1 << d;
    c.split_feature = ints(ns, F);
    if (ns) c.split_feature[ns - 1] = F - 1;   // the largest feature a split may test
    c.split_border.resize(ns);
    for (float &b : c.split_border) b = (float)next_f64();
    c.nan_true.resize(ns);
    for (uint8_t &b : c.nan_true) b = (uint8_t)(next_u64() & 1);
    c.leaves = doubles(nleaf * dim), c.bias = doubles(dim), c.thresholds = doubles(k), c.label_map = ints(k, 100);
    c.m = wdx_boost_model{(int32_t)depths.size(), F, dim, k, c.depth.data(), ns ? c.split_feature.data() : nullptr,
                          ns ? c.split_border.data() : nullptr, (ns && nan) ? c.nan_true.data() : nullptr, c.leaves.data(), 0.37,
                          c.bias.data(), lab ? c.label_map.data() : nullptr, thr ? c.thresholds.data() : nullptr};
}
static void check_boost_model(const BoostCase &c) {
    const wdx_boost_model &m = c.m;
    const int nt = m.n_trees, dim = m.dim, k = m.n_classes;
    ModelCheck r = check_boost(&m);
    REQUIRE(!r, "boost refused: %s", r.msg);
    BoostImage I;
    r = pack_boost(&m, &I);
    REQUIRE(!r, "boost not packed: %s", r.msg);
    check_pieces(I, "boost");
    const std::vector<unsigned char> copy(I.bytes);
    const unsigned char *base = I.bytes.data(), *far = copy.data();
    const BoostDev M = bind_boost(I, base), F = bind_boost(I, far);
    REQUIRE(M.n_trees == nt && M.n_features == m.n_features && M.dim == dim && M.k == k && M.scale == m.scale, "boost scalars");
    aligned(M.leaves, base, "leaves"), aligned(M.bias, base, "bias"), aligned(M.thresholds, base, "thresholds");
    aligned(M.trees, base, "trees"), aligned(M.splits, base, "splits"), aligned(M.label_map, base, "label_map");
    size_t s0 = 0, l0 = 0;
    for (int t = 0; t < nt; ++t) {
        REQUIRE(M.trees[t].split0 == (int32_t)s0 && M.trees[t].depth == m.depth[t] && M.trees[t].leaf0 == (int64_t)l0, "tree %d", t);
        s0 += m.depth[t];
        l0 += ((size_t)1 << m.depth[t]) * dim;
    }
    REQUIRE(same(M.leaves, m.leaf_values, l0 * 8) && same(M.bias, m.bias, dim * 8), "leaves / bias");
    REQUIRE(s0 ? M.splits != nullptr : !M.splits && !m.split_feature && !m.split_border, "splits of a model with %zu", s0);
    for (size_t i = 0; i < s0; ++i) {
        const uint32_t want = (uint32_t)m.split_feature[i] | ((m.split_nan_true && m.split_nan_true[i]) ? 0x100u : 0u);
        REQUIRE(M.splits[i].feat == want && same(&M.splits[i].border, &m.split_border[i], 4), "split %zu", i);
    }
    REQUIRE(m.thresholds ? M.thresholds && same(M.thresholds, m.thresholds, k * 8) : !M.thresholds, "thresholds");
    REQUIRE(m.label_map ? M.label_map && same(M.label_map, m.label_map, k * 4) : !M.label_map, "label_map");
    moved(M.leaves, F.leaves, base, far, "leaves"), moved(M.bias, F.bias, base, far, "bias");
    moved(M.thresholds, F.thresholds, base, far, "thresholds"), moved(M.trees, F.trees, base, far, "trees");
    moved(M.splits, F.splits, base, far, "splits"), moved(M.label_map, F.label_map, base, far, "label_map");
    ++models;
}
static void sweep_boost() {
    const int D = WDX_BOOST_MAX_DEPTH;
    const std::vector<std::vector<int>> forests = {{0}, {0, 0, 0}, {D}, {0, D}, {D, 0, 3}, {1, 2, 3, 4, 5, 0, 7}, {6, 6, 6, 6}};
    static const int dims[4][2] = {{1, 2}, {2, 2}, {5, 5}, {16, 16}};   // (dim, k)
    for (const std::vector<int> &depths : forests)
        for (const auto &dk : dims)
            for (int F : {1, 25, WDX_BOOST_MAX_FEATURES})
                for (int nan = 0; nan < 2; ++nan)
                    for (int opt = 0; opt < 4; ++opt) {
                        BoostCase c;
                        make_boost(c, depths, dk[0], dk[1], F, nan, opt & 1, opt & 2);
                        check_boost_model(c);
                    }
}

// ---- refusals ------------------------------------------------------------------------------------------------

static void refused(const ModelCheck &r, int code, const std::string &msg, const char *what) {
    REQUIRE(r.code == code, "%s: code %d, want %d (%s)", what, r.code, code, r.msg);
    REQUIRE(msg == r.msg, "%s: message \"%s\", want \"%s\"", what, r.msg, msg.c_str());
    ++refusals;
}

static void refusals_svm() {
    const std::string need = "svm_set_model: need 2..16 classes, support vectors, coefficients and Platt parameters";
    refused(check_svm(nullptr), WDX_ERR_INVALID, need, "no model");
    auto with = [](auto change) {
        SvmCase c;
        make_svm(c, 5, 1, true, true);
        change(c);
        return check_svm(&c.m);
    };
    refused(with([](SvmCase &c) { c.m.n_classes = 1; }), WDX_ERR_INVALID, need, "k=1");
    refused(with([](SvmCase &c) {
                c.n_support.assign(17, 1);
                c.m.n_classes = 17, c.m.n_sv = 17, c.m.n_support = c.n_support.data();
            }),
            WDX_ERR_INVALID, need, "k=17");
    refused(with([](SvmCase &c) { c.m.n_sv = 0; }), WDX_ERR_INVALID, need, "n_sv=0");
    refused(with([](SvmCase &c) { c.m.n_train = 0; }), WDX_ERR_INVALID, need, "n_train=0");
    refused(with([](SvmCase &c) { c.m.pwr_dist = 0; }), WDX_ERR_INVALID, need, "pwr_dist=0");
    refused(with([](SvmCase &c) { c.m.n_support = nullptr; }), WDX_ERR_INVALID, need, "no n_support");
    refused(with([](SvmCase &c) { c.m.support = nullptr; }), WDX_ERR_INVALID, need, "no support");
    refused(with([](SvmCase &c) { c.m.dual_coef = nullptr; }), WDX_ERR_INVALID, need, "no dual_coef");
    refused(with([](SvmCase &c) { c.m.rho = nullptr; }), WDX_ERR_INVALID, need, "no rho");
    refused(with([](SvmCase &c) { c.m.probA = nullptr; }), WDX_ERR_INVALID, need, "no probA");
    refused(with([](SvmCase &c) { c.m.probB = nullptr; }), WDX_ERR_INVALID, need, "no probB");
    refused(with([](SvmCase &c) { c.n_support[1] = -c.n_support[1]; }), WDX_ERR_INVALID, "svm_set_model: negative n_support",
            "negative n_support");
    refused(with([](SvmCase &c) { c.n_support[0] += 1; }), WDX_ERR_INVALID, "svm_set_model: sum(n_support) != n_sv",
            "sum(n_support) != n_sv");
    refused(with([](SvmCase &c) { c.support.back() = c.m.n_train; }), WDX_ERR_INVALID, "svm_set_model: support index out of range",
            "support >= n_train");
    refused(with([](SvmCase &c) { c.support[3] = -1; }), WDX_ERR_INVALID, "svm_set_model: support index out of range", "support < 0");
}

static void refusals_mlp() {
    const std::string need = "mlp_set_model: need a float32 / float64 model with >= 2 classes, layers and a known activation";
    refused(check_mlp(nullptr), WDX_ERR_INVALID, need, "no model");
    auto with = [](auto change) {
        MlpCase c;
        make_mlp(c, 4, {17, 16}, 12, 3, 3, {3}, true, true);
        change(c);
        return check_mlp(&c.m);
    };
    refused(with([](MlpCase &c) { c.m.dtype_bytes = 2; }), WDX_ERR_INVALID, need, "float16");
    refused(with([](MlpCase &c) { c.m.n_classes = 1; }), WDX_ERR_INVALID, need, "k=1");
    refused(with([](MlpCase &c) { c.m.n_layers = 0; }), WDX_ERR_INVALID, need, "n_layers=0");
    refused(with([](MlpCase &c) { c.m.n_scalers = -1; }), WDX_ERR_INVALID, need, "n_scalers=-1");
    refused(with([](MlpCase &c) { c.m.hidden_activation = WDX_MLP_ACT_RELU + 1; }), WDX_ERR_INVALID, need, "activation 4");
    refused(with([](MlpCase &c) { c.m.hidden_activation = -1; }), WDX_ERR_INVALID, need, "activation -1");
    refused(with([](MlpCase &c) { c.m.n_layers = 1; }), WDX_ERR_UNSUPPORTED, "mlp_set_model: 0 hidden layers (1..4 supported)",
            "no hidden layer");
    refused(with([](MlpCase &c) { c.m.n_layers = WDX_MLP_MAX_LAYERS + 1; }), WDX_ERR_UNSUPPORTED,
            "mlp_set_model: 5 hidden layers (1..4 supported)", "five hidden layers");
    refused(with([](MlpCase &c) { c.m.n_classes = 17; }), WDX_ERR_UNSUPPORTED, "mlp_set_model: 17 classes (2..16 supported)", "k=17");
    refused(with([](MlpCase &c) { c.m.n_scalers = WDX_MLP_MAX_SCALERS + 1; }), WDX_ERR_UNSUPPORTED,
            "mlp_set_model: 5 scaler steps (at most 4 supported)", "five scaler steps");
    refused(with([](MlpCase &c) { c.m.sizes[1] = 0; }), WDX_ERR_INVALID, "mlp_set_model: layer size 0 of entry 1", "layer size 0");
    refused(with([](MlpCase &c) { c.m.sizes[0] = -3; }), WDX_ERR_INVALID, "mlp_set_model: layer size -3 of entry 0", "n_in < 0");
    refused(with([](MlpCase &c) { c.m.coefs[1] = nullptr; }), WDX_ERR_INVALID,
            "mlp_set_model: layer 1 has no coefficients / intercepts", "no coefs[1]");
    refused(with([](MlpCase &c) { c.m.intercepts[2] = nullptr; }), WDX_ERR_INVALID,
            "mlp_set_model: layer 2 has no coefficients / intercepts", "no intercepts[2]");
    refused(with([](MlpCase &c) { c.m.sizes[3] = 2; }), WDX_ERR_INVALID, "mlp_set_model: 2 output units for 3 classes", "2 outputs, k=3");
    refused(with([](MlpCase &c) { c.m.sizes[3] = 1; }), WDX_ERR_INVALID, "mlp_set_model: 1 output units for 3 classes", "1 output, k=3");
    refused(with([](MlpCase &c) { c.m.sizes[2] = WDX_MLP_MAX_WIDTH + 1; }), WDX_ERR_UNSUPPORTED,
            "mlp_set_model: hidden layer of 513 units (at most 512 supported)", "513 units");
}

static void refusals_boost() {
    const std::string need = "boost_set_model: need >= 1 tree, >= 1 feature, >= 2 classes, depths, leaf values and a bias";
    refused(check_boost(nullptr), WDX_ERR_INVALID, need, "no model");
    auto with = [](auto change) {
        BoostCase c;
        make_boost(c, {2, 0, 3}, 4, 4, 25, 1, true, true);
        change(c);
        return check_boost(&c.m);
    };
    refused(with([](BoostCase &c) { c.m.n_trees = 0; }), WDX_ERR_INVALID, need, "no tree");
    refused(with([](BoostCase &c) { c.m.n_features = 0; }), WDX_ERR_INVALID, need, "no feature");
    refused(with([](BoostCase &c) { c.m.dim = 0; }), WDX_ERR_INVALID, need, "dim=0");
    refused(with([](BoostCase &c) { c.m.n_classes = 1; }), WDX_ERR_INVALID, need, "k=1");
    refused(with([](BoostCase &c) { c.m.depth = nullptr; }), WDX_ERR_INVALID, need, "no depths");
    refused(with([](BoostCase &c) { c.m.leaf_values = nullptr; }), WDX_ERR_INVALID, need, "no leaves");
    refused(with([](BoostCase &c) { c.m.bias = nullptr; }), WDX_ERR_INVALID, need, "no bias");
    refused(with([](BoostCase &c) { c.m.n_features = WDX_BOOST_MAX_FEATURES + 1; }), WDX_ERR_UNSUPPORTED,
            "boost_set_model: 255 features (1..254 supported)", "255 features");
    refused(with([](BoostCase &c) { c.m.dim = 17, c.m.n_classes = 17; }), WDX_ERR_UNSUPPORTED,
            "boost_set_model: 17 values per leaf for 17 classes (1..16 and 2..16 supported)", "dim = k = 17");
    refused(with([](BoostCase &c) { c.m.dim = 1, c.m.n_classes = 17; }), WDX_ERR_UNSUPPORTED,
            "boost_set_model: 1 values per leaf for 17 classes (1..16 and 2..16 supported)", "k=17");
    refused(with([](BoostCase &c) { c.m.dim = 3; }), WDX_ERR_INVALID, "boost_set_model: 3 values per leaf for 4 classes", "dim 3, k 4");
    refused(with([](BoostCase &c) { c.m.dim = 1; }), WDX_ERR_INVALID, "boost_set_model: 1 values per leaf for 4 classes", "dim 1, k 4");
    refused(with([](BoostCase &c) { c.depth[1] = -1; }), WDX_ERR_INVALID, "boost_set_model: tree 1 has depth -1", "negative depth");
    refused(with([](BoostCase &c) { c.depth[2] = WDX_BOOST_MAX_DEPTH + 1; }), WDX_ERR_UNSUPPORTED,
            "boost_set_model: tree 2 has depth 17 (0..16 supported)", "depth 17");
    refused(with([](BoostCase &c) { c.m.split_border = nullptr; }), WDX_ERR_INVALID, "boost_set_model: splits without features / borders",
            "no borders");
    refused(with([](BoostCase &c) { c.m.split_feature = nullptr; }), WDX_ERR_INVALID,
            "boost_set_model: splits without features / borders", "no split features");
    refused(with([](BoostCase &c) { c.split_feature[4] = 25; }), WDX_ERR_INVALID, "boost_set_model: split 4 tests feature 25 of 25",
            "feature = n_features");
    refused(with([](BoostCase &c) { c.split_feature[0] = -1; }), WDX_ERR_INVALID, "boost_set_model: split 0 tests feature -1 of 25",
            "feature < 0");
    {   // 2^27 trees of depth 16: 2^31 splits (512 MiB of depths; the check stops before it reads a split)
        BoostCase c;
        make_boost(c, {1}, 4, 4, 25, 0, false, false);
        c.depth.assign((size_t)1 << 27, WDX_BOOST_MAX_DEPTH);
        c.m.n_trees = 1 << 27, c.m.depth = c.depth.data();
        refused(check_boost(&c.m), WDX_ERR_UNSUPPORTED, "boost_set_model: too many splits", "2^31 splits");
    }
}

int main() {
    sweep_svm();
    sweep_mlp();
    sweep_boost();
    refusals_svm();
    refusals_mlp();
    refusals_boost();
    fprintf(stderr, "%lld models %lld refusals\n", models, refusals);
    return 0;
}
