// Out-of-fold probabilities of a cross-validated DTW kernel machine for gfx950 (include/wdx.h: wdx_svm_cv_couple_device): from the
// decision values the batched SMO solve left for every fold's held-out rows (wdx_svm_fit.hip: the evaluation rows of the folds' full
// problems) and the folds' probA / probB to probabilities, class index and margin per held-out row -- what the resident tail does
// BEHIND its decision values, by the same device code (wdx_svm_couple.h).
//
// One 16-lane group per held-out row, four rows a wave, ceil(rows / 4) one-wave workgroups.  A group gathers its row's k (k - 1) / 2
// decision values -- one per pair, each from that (fold, pair)'s evaluation block -- into LDS, then runs the coupling.
#include "wdx_ctx.h"
#include "wdx_svm_couple.h"

#include <math.h>
#include <string.h>

namespace wdx {

namespace {

struct SvmCvArgs {
    const double *dec;
    const int64_t *dec_off;    // [folds * pairs]
    const double *A, *B;       // [folds * pairs]
    const int64_t *held_off;   // [folds + 1]
    const int32_t *held;       // [total]
    int k, folds;
    int64_t total;
    double *prob;              // (m, k)
    int32_t *pred;             // [m]
    double *conf;              // [m]
};

// grid ceil(total / 4), one wave; dynamic LDS: 8 * 4 * (pairs + k * k) bytes
__global__ __launch_bounds__(64) void svm_cv_couple_kernel(const SvmCvArgs A) {
    extern __shared__ double cv_lds[];   // dec[4][pairs] | pw[4][k * k]
    const int lane = threadIdx.x, g = lane >> 4, t = lane & 15, k = A.k, npairs = k * (k - 1) / 2;
    int64_t i = (int64_t)blockIdx.x * 4 + g;
    const bool real = i < A.total;
    if (!real) i = A.total - 1;   // (a group behind the last row computes that row again and writes nothing)
    int f = 0;
    while (f + 1 < A.folds && i >= A.held_off[f + 1]) ++f;
    const int64_t e = i - A.held_off[f];
    double *dr = cv_lds + g * npairs, *pw = cv_lds + 4 * npairs + g * (k * k);
    int bad = 0;
    for (int p = t; p < npairs; p += 16) {
        const double v = A.dec[A.dec_off[(int64_t)f * npairs + p] + e];
        dr[p] = v;
        bad |= v != v;
    }
    for (int off = 8; off > 0; off >>= 1) bad |= __shfl_xor(bad, off);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const SvmCoupled c = svm_couple_group(dr, A.A + (int64_t)f * npairs, A.B + (int64_t)f * npairs, pw, k, lane);
    if (!real) return;
    const int64_t row = A.held[i];
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    if (t < k) A.prob[row * k + t] = bad ? qnan : c.pt;
    if (t == 0) {
        A.pred[row] = bad ? -1 : c.best;
        A.conf[row] = bad ? qnan : c.b1 - c.b2;
    }
}

}  // namespace

}  // namespace wdx

using namespace wdx;

extern "C" {

int wdx_svm_cv_couple_device(wdx_ctx *ctx, const double *d_dec, int64_t n_dec, int32_t k, int32_t n_folds, const int64_t *dec_off,
                          const double *probA, const double *probB, const int32_t *held, const int64_t *held_off, int64_t m, double *d_prob,
                          int32_t *d_pred_idx, double *d_conf, void *stream) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    if (k < 2 || k > WDX_SVM_CV_MAX_CLASSES || n_folds < 1 || n_folds > WDX_SVM_CV_MAX_FOLDS || m < 1 || n_dec < 0) {
        set_error("svm cv couple: k = %d (2..%d), n_folds = %d (1..%d), m = %lld (at least 1), n_dec = %lld (not negative)", k,
                  WDX_SVM_CV_MAX_CLASSES, n_folds, WDX_SVM_CV_MAX_FOLDS, (long long)m, (long long)n_dec);
        return WDX_ERR_INVALID;
    }
    if (!dec_off || !probA || !probB || !held_off || !d_prob || !d_pred_idx || !d_conf) {
        set_error("svm cv couple: the tables and the outputs are required (NULL given)");
        return WDX_ERR_INVALID;
    }
    const int64_t npairs = (int64_t)k * (k - 1) / 2, cells = npairs * n_folds;
    if (held_off[0] != 0) {
        set_error("svm cv couple: held_off[0] must be 0, not %lld", (long long)held_off[0]);
        return WDX_ERR_INVALID;
    }
    for (int f = 0; f < n_folds; ++f) {
        const int64_t nf = held_off[f + 1] - held_off[f];
        if (nf < 0) {
            set_error("svm cv couple: held_off must not decrease (fold %d)", f);
            return WDX_ERR_INVALID;
        }
        for (int64_t p = 0; p < npairs; ++p) {
            const int64_t o = dec_off[f * npairs + p];
            if (o < 0 || o > n_dec || nf > n_dec - o) {
                set_error("svm cv couple: the block of fold %d, pair %lld (%lld values from %lld) lies outside the %lld decision values", f,
                          (long long)p, (long long)nf, (long long)o, (long long)n_dec);
                return WDX_ERR_INVALID;
            }
        }
    }
    const int64_t total = held_off[n_folds];
    if (total > 0 && (!held || !d_dec)) {
        set_error("svm cv couple: the held-out rows and the decision values are required (NULL given)");
        return WDX_ERR_INVALID;
    }
    for (int64_t i = 0; i < total; ++i)
        if (held[i] < 0 || held[i] >= m) {
            set_error("svm cv couple: held[%lld] = %d lies outside 0 .. m-1 = %lld", (long long)i, held[i], (long long)m - 1);
            return WDX_ERR_INVALID;
        }
    if (total > ((int64_t)1 << 31)) {
        set_error("svm cv couple: %lld held-out rows, more than 2^31", (long long)total);
        return WDX_ERR_UNSUPPORTED;
    }
    if (total == 0) return WDX_SUCCESS;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = use_stream(ctx, s))) return rc;
    // the tables: dec_off | A | B | held_off (8-byte entries), then held -- through a page-locked block (the call returns with the copy pending)
    const size_t off_A = 8 * (size_t)cells, off_B = 16 * (size_t)cells, off_ho = 24 * (size_t)cells, off_held = off_ho + 8 * (size_t)(n_folds + 1);
    const size_t bytes = off_held + 4 * (size_t)total;
    if ((rc = ctx->svm_cv_ws.ensure(bytes))) return rc;
    uint8_t *const ws = (uint8_t *)ctx->svm_cv_ws.p;
    {
        MedoidStage *St = nullptr;
        if ((rc = medoid_stage_block(ctx, bytes, &St))) return rc;
        uint8_t *host = (uint8_t *)St->host;
        memcpy(host, dec_off, 8 * (size_t)cells);
        memcpy(host + off_A, probA, 8 * (size_t)cells);
        memcpy(host + off_B, probB, 8 * (size_t)cells);
        memcpy(host + off_ho, held_off, 8 * (size_t)(n_folds + 1));
        memcpy(host + off_held, held, 4 * (size_t)total);
        const hipError_t e1 = hipMemcpyAsync(ws, host, bytes, hipMemcpyHostToDevice, s);
        const hipError_t e2 = hipEventRecord(St->copied, s);
        WDX_HIP_TRY(e1);
        WDX_HIP_TRY(e2);
    }
    const SvmCvArgs A{d_dec, (const int64_t *)ws, (const double *)(ws + off_A), (const double *)(ws + off_B), (const int64_t *)(ws + off_ho),
                      (const int32_t *)(ws + off_held), (int)k, (int)n_folds, total, d_prob, d_pred_idx, d_conf};
    const size_t lds = 8 * 4 * (size_t)(npairs + (int64_t)k * k);
    Timed t(ctx, WDX_K_SVM_CV_COUPLE, s);
    hipLaunchKernelGGL(svm_cv_couple_kernel, dim3((unsigned)((total + 3) / 4)), dim3(64), lds, s, A);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

}  // extern "C"
