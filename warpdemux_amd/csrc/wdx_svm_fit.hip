// The batched SMO solver of the one-vs-one C-SVC duals for gfx950 (include/wdx.h: wdx_svm_solve_device states the rule;
// wdx_svm_fit_plan.h what a call does with its problems).
//
// One WORKGROUP per problem (DESIGN.md "SMO solver").  Row t of the problem belongs to thread t % THREADS as its slot t / THREADS:
// G_t and the two bits "alpha_t is at 0 / at C_t" live in that thread's registers, the row's K index and K_tt in LDS; the value
// alpha_t, which only the two rows of an iteration's pair change and only their owners read, in the caller's alpha array.
// An iteration is
//   A  every thread's best of v over I_up (lowest row first) and of -v over I_low -> one workgroup reduction: i, gmax, gmin
//   B  row i of K through the index list; every thread's best score -> one workgroup reduction: j
//   C  the owners of i and j hand alpha and G over through LDS; EVERY thread moves and clips the pair (the same float64
//      operations on the same values: uniform)
//   D  rows i and j of K (row i from the cache); G_t of the thread's own rows
// A reduction is a maximum with the lowest row among equals: it rounds nothing, so its tree does not matter.  Nothing here sums
// across lanes; rho's sum over the free rows is one thread's, in row order, and one lane owns one evaluation row.
// The Makefile's -ffp-contract=off keeps every product and sum of the update apart.
#include "wdx_ctx.h"
#include "wdx_svm_fit_plan.h"

#include <math.h>
#include <string.h>

namespace wdx {

struct SvmFitArgs {
    const float *K;              // (m, ld)
    int64_t ld;
    const SvmFitProb *probs;     // [grid]
    const int32_t *rows;         // the row lists
    const int32_t *eval_rows;    // the evaluation lists
    double eps;
    int64_t max_iter;
    double *alpha, *rho;
    int64_t *n_iter;
    int32_t *state;
    double *dec;
};

constexpr int kSvmFitMaxWaves = 16;
struct SvmFitScratch {
    // two buffers each: a reduction's partials are read by every thread after ONE barrier, and written again two barriers later
    double va[2][kSvmFitMaxWaves], vb[2][kSvmFitMaxWaves];
    int32_t ia[2][kSvmFitMaxWaves], bad[2][kSvmFitMaxWaves];
    double a_i, g_i, a_j, g_j, rho;
};
static_assert(sizeof(SvmFitScratch) <= (size_t)kSvmFitScratchBytes, "the scratch the plan reserves");

constexpr int32_t kNoRow = 0x7fffffff;

// (v, i) beats (w, k): larger, or equal and the lower row.  A NaN never wins and never loses to a NaN.
__device__ __forceinline__ bool svm_beats(double v, int32_t i, double w, int32_t k) { return v > w || (v == w && i < k); }

// Workgroup maximum of (va, ia) with the lowest row among equals, plain maximum of vb, OR of bad.  Every thread returns with the
// same three (four) values.  `buf` alternates between the calls of an iteration.
template <int WAVES>
__device__ __forceinline__ void svm_reduce(SvmFitScratch &S, int buf, double &va, int32_t &ia, double &vb, int &bad) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ova = __shfl_xor(va, off), ovb = __shfl_xor(vb, off);
        const int32_t oia = __shfl_xor(ia, off);
        bad |= __shfl_xor(bad, off);
        if (svm_beats(ova, oia, va, ia)) va = ova, ia = oia;
        if (ovb > vb) vb = ovb;
    }
    if constexpr (WAVES > 1) {
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) S.va[buf][wave] = va, S.ia[buf][wave] = ia, S.vb[buf][wave] = vb, S.bad[buf][wave] = bad;
        __syncthreads();
        va = S.va[buf][0], ia = S.ia[buf][0], vb = S.vb[buf][0], bad = S.bad[buf][0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
            const double ova = S.va[buf][w], ovb = S.vb[buf][w];
            const int32_t oia = S.ia[buf][w];
            bad |= S.bad[buf][w];
            if (svm_beats(ova, oia, va, ia)) va = ova, ia = oia;
            if (ovb > vb) vb = ovb;
        }
    }
}

template <int THREADS, int RPT>
__global__ __launch_bounds__(THREADS) void svm_fit_kernel(const SvmFitArgs A) {
    constexpr int CAP = THREADS * RPT, WAVES = THREADS / 64;
    constexpr double TAU = 1e-12;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int32_t *const idx = reinterpret_cast<int32_t *>(smem);              // [CAP] K row of row t
    float *const kd = reinterpret_cast<float *>(smem + 4 * CAP);         // [CAP] K_tt
    double *const col = reinterpret_cast<double *>(smem);                // [CAP] after the solve: v_t, then alpha_t y_t
    SvmFitScratch &S = *reinterpret_cast<SvmFitScratch *>(smem + 8 * CAP);
    const int tid = threadIdx.x;
    const SvmFitProb Pb = A.probs[blockIdx.x];
    const int n_pos = Pb.n_pos, n = Pb.n_pos + Pb.n_neg;   // (n <= CAP: the plan chose the instantiation)
    const double c_pos = Pb.c_pos, c_neg = Pb.c_neg;
    const float *__restrict__ K = A.K;
    const int64_t ld = A.ld;
    const int32_t *__restrict__ rows = A.rows + Pb.row0;

    // A row's alpha is read in every iteration only as "at 0" / "at C": those two bits per row stay in registers (bit k: slot k).
    // The value itself changes for two rows per iteration and is read by their owners alone: it stays in the caller's alpha
    // array, each entry written and read by ONE thread.
    double *__restrict__ out_alpha = A.alpha + Pb.row0;
    double G[RPT];
    uint32_t at_lower = ~0u, at_upper = 0u;   // !(alpha > 0), !(alpha < C)
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        G[k] = -1.0;
        const int t = tid + k * THREADS;
        if (t < n) {
            const int32_t r = rows[t];
            idx[t] = r;
            kd[t] = K[(int64_t)r * ld + r];
            out_alpha[t] = 0.0;
        }
    }
    __syncthreads();

    int state = 0;
    int64_t it = 0;
    double gmax = 0.0, gmin = 0.0;
    for (;;) {
        // A: i, gmax, gmin -- and whether every G is finite
        double va = -INFINITY, vb = -INFINITY;
        int32_t ia = kNoRow;
        int bad = 0;
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            if (k * THREADS >= n) break;
            const int t = tid + k * THREADS;
            if (t < n) {
                const bool pos = t < n_pos;
                const double g = G[k];
                const double v = pos ? -g : g;
                bad |= !(fabs(g) <= 1.7976931348623157e308);
                const bool lo = (at_lower >> k) & 1u, hi = (at_upper >> k) & 1u;
                const bool up = pos ? !hi : !lo, low = pos ? !lo : !hi;
                if (up && svm_beats(v, t, va, ia)) va = v, ia = t;
                if (low && -v > vb) vb = -v;
            }
        }
        svm_reduce<WAVES>(S, 0, va, ia, vb, bad);
        if (bad) {
            state = 2;
            break;
        }
        gmax = va, gmin = -vb;
        const int i = ia;
        if (gmax - gmin < A.eps) break;
        if (it >= A.max_iter) {
            state = 1;
            break;
        }
        // (an empty I_up or I_low made the gap -inf and stopped above: i is a row, and gmin's row has b >= eps > 0)
        const bool i_pos = i < n_pos;
        const double Kii = (double)kd[i];
        const int64_t row_i = (int64_t)idx[i] * ld;
        if (tid == i % THREADS) {
            double g = 0.0;
#pragma unroll
            for (int k = 0; k < RPT; ++k)
                if (k == i / THREADS) g = G[k];
            S.a_i = out_alpha[i], S.g_i = g;
        }
        // B: j
        double sb = -INFINITY, unused = -INFINITY;
        int32_t jb = kNoRow;
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            if (k * THREADS >= n) break;
            const int t = tid + k * THREADS;
            if (t < n) {
                const float f = K[row_i + idx[t]];
                const bool pos = t < n_pos;
                const double g = G[k];
                const double v = pos ? -g : g;
                const bool low = !(((pos ? at_lower : at_upper) >> k) & 1u);
                const double b = gmax - v;
                if (low && b > 0.0) {
                    double cv = (Kii + (double)kd[t]) - 2.0 * (double)f;
                    if (!(cv > 0.0)) cv = TAU;
                    const double score = (b * b) / cv;
                    if (svm_beats(score, t, sb, jb)) sb = score, jb = t;
                }
            }
        }
        int nothing = 0;
        svm_reduce<WAVES>(S, 1, sb, jb, unused, nothing);
        const int j = jb;
        if (j == kNoRow) {
            state = 2;
            break;
        }
        // C: the pair
        const bool j_pos = j < n_pos;
        if (tid == j % THREADS) {
            double g = 0.0;
#pragma unroll
            for (int k = 0; k < RPT; ++k)
                if (k == j / THREADS) g = G[k];
            S.a_j = out_alpha[j], S.g_j = g;
        }
        const int64_t row_j = (int64_t)idx[j] * ld;
        const double Kij = (double)K[row_i + idx[j]];   // (uniform: the entry row i's owner of j has just read)
        __syncthreads();
        const double Ci = i_pos ? c_pos : c_neg, Cj = j_pos ? c_pos : c_neg;
        const double old_i = S.a_i, old_j = S.a_j, Gi = S.g_i, Gj = S.g_j;
        double q = (Kii + (double)kd[j]) - 2.0 * Kij;
        if (!(q > 0.0)) q = TAU;
        double ai = old_i, aj = old_j;
        if (i_pos != j_pos) {
            const double d = (-Gi - Gj) / q, diff = ai - aj;
            ai += d, aj += d;
            if (diff > 0.0) {
                if (aj < 0.0) aj = 0.0, ai = diff;
            } else {
                if (ai < 0.0) ai = 0.0, aj = -diff;
            }
            if (diff > Ci - Cj) {
                if (ai > Ci) ai = Ci, aj = Ci - diff;
            } else {
                if (aj > Cj) aj = Cj, ai = Cj + diff;
            }
        } else {
            const double d = (Gi - Gj) / q, sum = ai + aj;
            ai -= d, aj += d;
            if (sum > Ci) {
                if (ai > Ci) ai = Ci, aj = sum - Ci;
            } else {
                if (aj < 0.0) aj = 0.0, ai = sum;
            }
            if (sum > Cj) {
                if (aj > Cj) aj = Cj, ai = sum - Cj;
            } else {
                if (ai < 0.0) ai = 0.0, aj = sum;
            }
        }
        const double da_i = ai - old_i, da_j = aj - old_j;
        // D: the two rows' alpha and bound bits, by their owners; the gradient
        if (tid == i % THREADS) {
            const uint32_t bit = 1u << (i / THREADS);
            out_alpha[i] = ai;
            at_lower = (at_lower & ~bit) | (ai > 0.0 ? 0u : bit), at_upper = (at_upper & ~bit) | (ai < Ci ? 0u : bit);
        }
        if (tid == j % THREADS) {
            const uint32_t bit = 1u << (j / THREADS);
            out_alpha[j] = aj;
            at_lower = (at_lower & ~bit) | (aj > 0.0 ? 0u : bit), at_upper = (at_upper & ~bit) | (aj < Cj ? 0u : bit);
        }
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            if (k * THREADS >= n) break;
            const int t = tid + k * THREADS;
            if (t < n) {
                const bool pos = t < n_pos;
                const double kti = (double)K[row_i + idx[t]], ktj = (double)K[row_j + idx[t]];
                const double qti = pos == i_pos ? kti : -kti, qtj = pos == j_pos ? ktj : -ktj;
                G[k] = G[k] + (qti * da_i + qtj * da_j);
            }
        }
        ++it;
    }

    // the results.  (every thread left the loop at the same place: what decides it is uniform)
    __syncthreads();   // the last reads of idx / kd are behind: their bytes become `col`
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int t = tid + k * THREADS;
        if (t < n) {
            const bool is_free = !(((at_lower | at_upper) >> k) & 1u);
            col[t] = is_free ? (t < n_pos ? -G[k] : G[k]) : INFINITY;   // v_t of a free row (finite in state 0 and 1)
        }
    }
    __syncthreads();
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    if (tid == 0) {
        double rho = qnan;
        if (state != 2) {
            double sum = 0.0;
            int64_t free = 0;
            for (int t = 0; t < n; ++t) {
                const double v = col[t];
                if (v != INFINITY) sum = sum + v, ++free;
            }
            rho = free ? -sum / (double)free : -(gmax + gmin) / 2.0;
        }
        S.rho = rho;
        A.rho[Pb.q] = rho, A.n_iter[Pb.q] = it, A.state[Pb.q] = state;
    }
    __syncthreads();
    if (Pb.n_eval == 0) return;   // (uniform)
    const double rho = S.rho;
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int t = tid + k * THREADS;
        if (t < n) {
            const double a = out_alpha[t];   // (this thread's own stores)
            col[t] = t < n_pos ? a : -a;     // alpha_t y_t
        }
    }
    __syncthreads();
    const int32_t *__restrict__ ev = A.eval_rows + Pb.eval0;
    double *__restrict__ dec = A.dec + Pb.eval0;
    for (int e = tid; e < Pb.n_eval; e += THREADS) {
        double acc = 0.0;
        if (state != 2) {
            const float *__restrict__ Ke = K + (int64_t)ev[e] * ld;
            for (int s = 0; s < n; ++s) {
                const double c = col[s];
                if (c != 0.0) acc = acc + c * (double)Ke[rows[s]];
            }
        }
        dec[e] = state != 2 ? acc - rho : qnan;
    }
}

using SvmFitKernelFn = void (*)(const SvmFitArgs);
static SvmFitKernelFn svm_fit_kernel_of(int k) {
    switch (k) {
    case 0: return svm_fit_kernel<kSvmFitKernels[0].threads, kSvmFitKernels[0].rows_per_thread>;
    case 1: return svm_fit_kernel<kSvmFitKernels[1].threads, kSvmFitKernels[1].rows_per_thread>;
    default: return svm_fit_kernel<kSvmFitKernels[2].threads, kSvmFitKernels[2].rows_per_thread>;
    }
}
static int svm_fit_lds_attr(int k, SvmFitKernelFn fn, size_t lds) {
    static LdsAttr attr[kSvmFitKernelCount];
    return attr[k].ensure(fn, lds);
}

static int svm_fit_refusal(const SvmFitPlan &P) {
    if (P.rc != WDX_SUCCESS) set_error("%s", P.msg);
    return P.rc;
}

// With the context's mutex held.  d_K and the outputs are device memory; the plan was made of the caller's HOST tables.
static int svm_solve_locked(wdx_ctx *ctx, const SvmFitPlan &P, const float *d_K, const int32_t *rows, const int32_t *eval_rows,
                            double *d_alpha, double *d_rho, int64_t *d_n_iter, int32_t *d_state, double *d_dec, hipStream_t s) {
    if (P.n_problems == 0) return WDX_SUCCESS;
    int rc;
    if ((rc = use_stream(ctx, s))) return rc;
    if ((rc = ctx->svm_fit_ws.ensure((size_t)P.table_bytes))) return rc;
    uint8_t *const ws = (uint8_t *)ctx->svm_fit_ws.p;
    {   // the tables, through a page-locked block (the call returns with the copy pending)
        MedoidStage *St = nullptr;
        if ((rc = medoid_stage_block(ctx, (size_t)P.table_bytes, &St))) return rc;
        uint8_t *host = (uint8_t *)St->host;
        memcpy(host + P.off_probs, P.grid.data(), P.grid.size() * sizeof(SvmFitProb));
        if (P.n_rows) memcpy(host + P.off_rows, rows, (size_t)P.n_rows * sizeof(int32_t));
        if (P.n_eval) memcpy(host + P.off_eval, eval_rows, (size_t)P.n_eval * sizeof(int32_t));
        const hipError_t e1 = hipMemcpyAsync(ws, host, (size_t)P.table_bytes, hipMemcpyHostToDevice, s);
        const hipError_t e2 = hipEventRecord(St->copied, s);
        WDX_HIP_TRY(e1);
        WDX_HIP_TRY(e2);
    }
    const SvmFitArgs A{d_K, P.ld, (const SvmFitProb *)(ws + P.off_probs), (const int32_t *)(ws + P.off_rows), (const int32_t *)(ws + P.off_eval),
                       P.eps, P.max_iter, d_alpha, d_rho, d_n_iter, d_state, d_dec};
    const SvmFitKernelFn fn = svm_fit_kernel_of(P.kernel);
    if ((rc = svm_fit_lds_attr(P.kernel, fn, (size_t)P.lds_bytes()))) return rc;
    Timed t(ctx, WDX_K_SVM_FIT, s);
    hipLaunchKernelGGL(fn, dim3((unsigned)P.n_problems), dim3((unsigned)P.threads()), (size_t)P.lds_bytes(), s, A);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

}  // namespace wdx

using namespace wdx;

extern "C" {

int wdx_svm_solve_device(wdx_ctx *ctx, const float *d_K, int64_t m, int64_t ld, const wdx_svm_problem *problems, int64_t n_problems,
                         const int32_t *rows, int64_t n_rows, const int32_t *eval_rows, int64_t n_eval, double eps, int64_t max_iter,
                         double *d_alpha, double *d_rho, int64_t *d_n_iter, int32_t *d_state, double *d_dec, void *stream) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    const SvmFitPlan P = svm_fit_plan(m, ld, problems, n_problems, rows, n_rows, eval_rows, n_eval, eps, max_iter, d_K != nullptr,
                                      d_alpha && d_rho && d_n_iter && d_state, d_dec != nullptr);
    if ((rc = svm_fit_refusal(P))) return rc;
    return svm_solve_locked(ctx, P, d_K, rows, eval_rows, d_alpha, d_rho, d_n_iter, d_state, d_dec, (hipStream_t)stream);
}

int wdx_svm_solve(wdx_ctx *ctx, const float *K, int64_t m, int64_t ld, const wdx_svm_problem *problems, int64_t n_problems,
                  const int32_t *rows, int64_t n_rows, const int32_t *eval_rows, int64_t n_eval, double eps, int64_t max_iter, double *alpha,
                  double *rho, int64_t *n_iter, int32_t *state, double *dec) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    const SvmFitPlan P = svm_fit_plan(m, ld, problems, n_problems, rows, n_rows, eval_rows, n_eval, eps, max_iter, K != nullptr,
                                      alpha && rho && n_iter && state, dec != nullptr);
    if ((rc = svm_fit_refusal(P))) return rc;
    if (n_problems == 0) return WDX_SUCCESS;
    for (int64_t a = 0; a < m; ++a)
        for (int64_t b = 0; b < m; ++b)
            if (!isfinite(K[a * ld + b])) {
                set_error("svm solve: K[%lld, %lld] is not finite", (long long)a, (long long)b);
                return WDX_ERR_INVALID;
            }
    hipStream_t s = ctx->stream;
    if ((rc = use_stream(ctx, s))) return rc;
    const size_t Q = (size_t)n_problems, ab = (size_t)n_rows * sizeof(double), eb = (size_t)n_eval * sizeof(double);
    if ((rc = ctx->out0.ensure(ab ? ab : 8))) return rc;
    if ((rc = ctx->out1.ensure(Q * sizeof(double)))) return rc;
    if ((rc = ctx->out2.ensure(Q * sizeof(int64_t)))) return rc;
    if ((rc = ctx->out3.ensure(Q * sizeof(int32_t)))) return rc;
    if (eb && (rc = ctx->tmp0.ensure(eb))) return rc;
    // the matrix lives for this call only (a context never keeps a gigabyte)
    struct Matrix {
        float *p = nullptr;
        ~Matrix() {
            if (p) (void)hipFree(p);
        }
    } M;
    WDX_HIP_TRY(hipMalloc((void **)&M.p, (size_t)m * (size_t)m * sizeof(float)));
    {
        StreamDrain drain(s);   // (declared behind M: the stream is drained before the matrix is freed)
        WDX_HIP_TRY(hipMemcpy2DAsync(M.p, (size_t)m * sizeof(float), K, (size_t)ld * sizeof(float), (size_t)m * sizeof(float), (size_t)m,
                                     hipMemcpyHostToDevice, s));
        // (rows no problem names keep alpha 0)
        if (ab) WDX_HIP_TRY(hipMemsetAsync(ctx->out0.p, 0, ab, s));
        if (eb) WDX_HIP_TRY(hipMemsetAsync(ctx->tmp0.p, 0, eb, s));
        SvmFitPlan Pd = P;
        Pd.ld = m;
        if ((rc = svm_solve_locked(ctx, Pd, M.p, rows, eval_rows, (double *)ctx->out0.p, (double *)ctx->out1.p, (int64_t *)ctx->out2.p,
                                   (int32_t *)ctx->out3.p, eb ? (double *)ctx->tmp0.p : nullptr, s)))
            return rc;
        if (ab) WDX_HIP_TRY(hipMemcpyAsync(alpha, ctx->out0.p, ab, hipMemcpyDeviceToHost, s));
        WDX_HIP_TRY(hipMemcpyAsync(rho, ctx->out1.p, Q * sizeof(double), hipMemcpyDeviceToHost, s));
        WDX_HIP_TRY(hipMemcpyAsync(n_iter, ctx->out2.p, Q * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        WDX_HIP_TRY(hipMemcpyAsync(state, ctx->out3.p, Q * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (eb) WDX_HIP_TRY(hipMemcpyAsync(dec, ctx->tmp0.p, eb, hipMemcpyDeviceToHost, s));
        WDX_HIP_TRY(hipStreamSynchronize(s));
        drain.done();
    }
    return WDX_SUCCESS;
}

}  // extern "C"
