// Consensus-guided barcode refinement, the OPTIMAL change-points of the barcode tail (WDX_OPT_REFINE_OPTIMAL_CPTS;
// sig_proc.py:348-354: ruptures.KernelCPD(kernel="linear", min_size=min_obs_per_base).predict(n_bkps=barcode_num_events[0])
// instead of the peaks of the score curve).  The finishing step of a matched read (RefineRec::state == 3), whichever kernel
// segmented its adapter: ONE WORKGROUP per read in flight, a grid of `slots` workgroups that stride over the reads.
//
// The rule (include/wdx.h; parity with ruptures' own bits is unpinned), float64, nothing fused:
//   x = adapter_scores[sig_barcode_start:]  (N samples; the adapter's t-scores with the ADAPTED width), m = min_obs_per_base
//   as configured, B = barcode_num_events[0]
//   P[t] = P[t-1] + x[t-1], Q[t] = Q[t-1] + x[t-1] * x[t-1]                       sequential
//   cost(s, t) = (Q[t] - Q[s]) - ((P[t] - P[s]) * (P[t] - P[s])) / (double)(t - s)
//   V_0[t] = cost(0, t), V_k[t] = min over s in [k m, t - m] of V_{k-1}[s] + cost(s, t), ties -> the smallest s
//   boundaries 0, b_1 .. b_B, N by the back-trace from (B, N): B + 1 dwell times -- and B + 2 event means, because the reference's
//   compute_base_means closes the slice with one more event over the 2 W samples behind the score curve's end.
// Infeasible ((B + 1) m > N) or a non-finite score: WDX_READ_FAIL_SEGMENT (ruptures raises there).
//
// The kernel: the tail's scores with the exact kernel's operations (window statistics once per window start, tiles of
// 256 - W positions, as fingerprint_refine_tail_kernel), the prefix sums by one lane, then B rounds in which a thread owns
// an end point t and walks its candidates s in ascending order (strict `<`: the smallest s of a tie; V, P, Q of the
// candidate are one broadcast read per wave).  Only the states that can lie on a path to (B, N) are filled:
// t in [(k + 1) m, N - (B - k) m].  The path table -- 16-bit entries, B rows of N + 1 -- lives in the workgroup's slot of a
// context-owned scratch buffer; P, Q and two rows of V live in LDS for tails of up to kOptLdsCap samples and in the slot
// beyond that, up to WDX_MAX_ADAPTER_SAMPLES.  The cap follows from the kernel's resources (profiles/optimal_cpts_resource_usage.txt):
// 4 x 2048 doubles are 64 KiB of the 75 288 B a workgroup takes, so TWO workgroups share a CU's 160 KiB -- eight waves, two
// per SIMD, which the 121 VGPRs of the kernel (four waves per SIMD, no scratch memory) admit and which is all the work can
// use: it is bound by its arithmetic, one float64 division and about thirty vector instructions per candidate (measured:
// 1.2e12 candidates per second, 58 000 tRNA-shaped reads per second).  A third workgroup per CU (1 364 samples) would serve
// fewer tails from LDS and add nothing.  What would: cost(s, t) does not depend on k, so a pass over the (s, t) pairs that
// carries several rows of V at once would pay the division once per pair instead of once per row -- not done here.
#include "wdx_fp_types.h"

namespace wdx {

namespace {

constexpr int kOB = 256;            // threads of a workgroup
constexpr int kOptSegMax = 254;     // events of the barcode: barcode_num_events[0] + 1 <= kMaxEvents + 1

struct OptLds {
    double dp[4][kOptLdsCap + 1];   // P, Q, V (two rows)
    double Mt[kOB + 64], Vt[kOB + 64];
    float sig[kOB + 2 * 64 + 8];
    double ev[kOptSegMax + 1];
    int cp[kOptSegMax + 2];
};
static_assert(sizeof(OptLds) <= 75 * 1024, "two workgroups per CU");

struct OptArrays {
    double *P, *Q, *V0, *V1;
    unsigned short *path;   // B rows of `stride` entries
    int64_t stride;
};

// the optimal partition of x[0 .. N) -- already in A.V1 -- into B + 1 pieces of at least m samples; boundaries into cp[0 .. B + 1].
// false: a non-finite sample.  Block-uniform call; N >= (B + 1) m >= 1 is the caller's business.
__device__ __forceinline__ bool optimal_cpts(const OptArrays &A, const int N, const int B, const int m, int *cp) {
    const int tid = threadIdx.x;
    int bad = 0;
    for (int i = tid; i < N; i += kOB) {
        const double v = A.V1[i];
        bad |= !(v - v == 0.0);
    }
    if (__syncthreads_or(bad)) return false;
    if (tid == 0) {
        double p = 0.0, q = 0.0;
        A.P[0] = 0.0;
        A.Q[0] = 0.0;
        for (int t = 0; t < N; ++t) {
            const double v = A.V1[t];
            p = p + v;
            q = q + v * v;
            A.P[t + 1] = p;
            A.Q[t + 1] = q;
        }
    }
    __syncthreads();
    double *Vp = A.V0, *Vn = A.V1;
    for (int t = m + tid; t <= N - B * m; t += kOB) {
        const double dP = A.P[t];
        Vp[t] = A.Q[t] - (dP * dP) / (double)t;
    }
    __syncthreads();
    for (int k = 1; k <= B; ++k) {
        const int s_lo = k * m, t_hi = N - (B - k) * m;
        unsigned short *row = A.path + (int64_t)(k - 1) * A.stride;
        for (int t = s_lo + m + tid; t <= t_hi; t += kOB) {
            const double Pt = A.P[t], Qt = A.Q[t];
            double best = __builtin_huge_val();
            int bs = s_lo;
            for (int s = s_lo; s <= t - m; ++s) {
                const double dP = Pt - A.P[s];
                const double c = Vp[s] + ((Qt - A.Q[s]) - (dP * dP) / (double)(t - s));
                if (c < best) {
                    best = c;
                    bs = s;
                }
            }
            Vn[t] = best;
            row[t] = (unsigned short)bs;
        }
        __syncthreads();
        double *sw = Vp;
        Vp = Vn;
        Vn = sw;
    }
    if (tid == 0) {
        int t = N;
        cp[B + 1] = N;
        for (int k = B; k >= 1; --k) {
            t = A.path[(int64_t)(k - 1) * A.stride + t];
            cp[k] = t;
        }
        cp[0] = 0;
    }
    __syncthreads();
    return true;
}

// where a workgroup's arrays live: LDS for tails of up to kOptLdsCap samples, its slot beyond (slot: path rows, then -- only
// when the launch was sized for such tails -- four arrays of cap + 1 doubles)
__device__ __forceinline__ OptArrays opt_arrays(OptLds &S, unsigned char *slot, const int N, const int B, const int64_t cap,
                                                const bool lds) {
    OptArrays a;
    a.stride = cap + 1;
    a.path = reinterpret_cast<unsigned short *>(slot);
    double *g = reinterpret_cast<double *>(slot + (((size_t)B * (size_t)(cap + 1) * 2 + 15) & ~(size_t)15));
    if (lds) {
        a.P = S.dp[0]; a.Q = S.dp[1]; a.V0 = S.dp[2]; a.V1 = S.dp[3];
    } else {
        a.P = g; a.Q = g + (cap + 1); a.V0 = g + 2 * (cap + 1); a.V1 = g + 3 * (cap + 1);
    }
    return a;
}

__global__ __launch_bounds__(kOB) void fingerprint_refine_optimal_kernel(FpArgs A, unsigned char *scratch, size_t slot_bytes,
                                                                         int64_t cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    OptLds &S = *reinterpret_cast<OptLds *>(smem);
    const int tid = threadIdx.x;
    const wdx_seg_params &P = A.p;
    const RefineDev &R = A.rf;
    const int K = P.barcode_num_events, B = R.E2, m = P.min_obs_per_base;
    unsigned char *slot = scratch + (size_t)blockIdx.x * slot_bytes;
    for (int64_t r = A.block_base + blockIdx.x; r < A.n_reads; r += gridDim.x) {
        __syncthreads();   // (the previous read's LDS is free)
        RefineRec *rec = reinterpret_cast<RefineRec *>(R.ws) + r;
        if (rec->state != 3) continue;   // (block-uniform)
        auto fail = [&](const int st, const bool with_stats) {   // fp_refine_finish's finish(st, with_stats), st != OK
            for (int i = tid; i < K; i += kOB) {
                if (A.fpt) A.fpt[r * K + i] = __builtin_nan("");
                if (A.dwell) A.dwell[r * K + i] = 0;
            }
            if (!with_stats) {
                if (A.stats && tid < 6) A.stats[r * 6 + tid] = __builtin_nan("");
                if (R.idx && tid < 3) R.idx[r * 3 + tid] = -1;
            }
            if (tid == 0) A.status[r] = st;
        };
        RefineMatch M;
        memcpy(&M, rec->m, sizeof(M));
        const int n = rec->n;
        const float lo = rec->lo, hi = rec->hi;
        const bool bad_bounds = (lo != lo) || (hi != hi);
        // the exact kernel's clip (fp_process_read P1): a NaN sample stays, NaN bounds make every sample NaN
        auto clip = [&](float v) {
            if (v == v) {
                if (bad_bounds) v = __builtin_nanf("");
                else {
                    if (!(v > lo)) v = lo;
                    if (!(v < hi)) v = hi;
                }
            }
            return v;
        };
        // the ADAPTED window width of the adapter pass (sig_proc.py:317-320; fp_process_read's parameter shrink)
        int W = (int)rint((double)n / (double)P.num_events);
        if (P.running_stat_width < W) W = P.running_stat_width;
        int ns = n - 2 * W;
        if (ns < 0 || (ns > 0 && W == 0)) ns = 0;   // the Cython call raises -> zeros(0)
        const int sbs = M.sbs;
        int N = ns - sbs;
        if (N < 0) N = 0;
        if ((int64_t)(B + 1) * m > N || N > cap) {   // infeasible (N > cap cannot happen: cap bounds the window)
            fail(N > cap ? WDX_READ_FAIL_UNKNOWN : WDX_READ_FAIL_SEGMENT, false);
            continue;
        }
        const bool lds = N <= kOptLdsCap;
        const OptArrays arr = opt_arrays(S, slot, N, B, cap, lds);
        const int64_t row_off = A.row_off ? A.row_off[r] : r * A.stride;
        int64_t start = (int64_t)A.a_start[r] - P.padding;
        if (start < 0) start = 0;
        const float *__restrict__ src = A.sig + row_off + start + sbs;   // the tail's samples: N + 2 W of them at least
        // ---- the tail of the score curve (fingerprint_refine_tail_kernel's tiles) -> arr.V1 ------------------------------
        {
            const int nwin = N + W;        // window starts 0 .. N + W - 1
            const int TP = kOB - W;        // W <= kMaxW = 64
            for (int t0 = 0; t0 < N; t0 += TP) {
                for (int i = tid; i < kOB + W; i += kOB) S.sig[i] = t0 + i < N + 2 * W ? clip(src[t0 + i]) : 0.f;
                __syncthreads();
                if (t0 + tid < nwin) {
                    double mm, vv;
                    if (W == 18) window_stats<18>(S.sig + tid, W, mm, vv);
                    else if (W == 12) window_stats<12>(S.sig + tid, W, mm, vv);
                    else window_stats<0>(S.sig + tid, W, mm, vv);
                    S.Mt[tid] = mm;
                    S.Vt[tid] = vv;
                }
                __syncthreads();
                const int pos = t0 + tid;
                if (tid < TP && pos < N) {
                    const double m1 = S.Mt[tid], m2 = S.Mt[tid + W];
                    const double vs = S.Vt[tid] + S.Vt[tid + W];
                    double sc;
                    if (vs == 0) sc = 0.0;
                    else if (m1 > m2) sc = (m1 - m2) / sqrt(vs);
                    else sc = (m2 - m1) / sqrt(vs);
                    arr.V1[pos] = sc;
                }
                __syncthreads();
            }
        }
        bool finite;
        if (lds) finite = optimal_cpts(opt_arrays(S, slot, N, B, cap, true), N, B, m, S.cp);
        else finite = optimal_cpts(opt_arrays(S, slot, N, B, cap, false), N, B, m, S.cp);
        if (!finite) {
            fail(WDX_READ_FAIL_SEGMENT, false);
            continue;
        }
        // ---- compute_base_means(adapter_sig[sig_barcode_start:], valid_cpts): sequential float64 sums ---------------------
        // (compute_base_means appends the slice's end when the last boundary is not there, and N is the score curve's end: one more
        // event mean over the last 2 W samples -- B + 2 means beside the B + 1 dwell times of valid_cpts, as in the reference)
        const int nseg2 = B + 1, nmean = B + 2;
        if (tid == 0) S.cp[B + 2] = N + 2 * W;
        __syncthreads();
        for (int s = tid; s < nmean; s += kOB) {
            const int b = S.cp[s], e = S.cp[s + 1];
            double sum = 0.0;
            for (int i = b; i < e; ++i) sum += (double)clip(src[i]);
            S.ev[s] = sum / (double)(e - b);
        }
        __syncthreads();
        // ---- normalize_wrt, the outlier filter, outputs (fp_refine_finish) -----------------------------------------------
        double shift, scale;
        if (P.seg_norm == WDX_NORM_MEAN) { shift = M.mean; scale = M.sd; }
        else if (P.seg_norm == WDX_NORM_MEDIAN) { shift = M.ev_med; scale = M.ev_mad; }
        else { fail(WDX_READ_FAIL_UNKNOWN, false); continue; }
        const bool outlier = M.qs > R.ub_start || M.qe < R.lb_end || M.qe > R.ub_end;
        if (!outlier && nseg2 < K) {
            fail(WDX_READ_FAIL_UNKNOWN, false);
            continue;
        }
        if (tid == 0) {
            if (A.stats) {
                double *o = A.stats + r * 6;
                o[0] = M.dt_med; o[1] = M.dt_mad; o[2] = M.mean; o[3] = M.sd; o[4] = M.ev_med; o[5] = M.ev_mad;
            }
            if (R.idx) {
                R.idx[r * 3] = M.qs; R.idx[r * 3 + 1] = M.qe; R.idx[r * 3 + 2] = sbs;
            }
        }
        if (outlier) {
            fail(WDX_READ_FAIL_CONSENSUS, true);
            continue;
        }
        for (int i = tid; i < K; i += kOB) {
            const int s = nseg2 - K + i;   // the last K dwell times, the last K of the B + 2 means
            if (A.fpt) A.fpt[r * K + i] = (S.ev[s + 1] - shift) / scale;
            if (A.dwell) A.dwell[r * K + i] = (int64_t)(S.cp[s + 1] - S.cp[s]);
        }
        if (tid == 0) A.status[r] = WDX_READ_OK;
    }
}

// the DP alone on series handed over as they are (wdx_selftest_optimal_cpts_dev): series i = x[off[i] .. off[i + 1])
__global__ __launch_bounds__(kOB) void optimal_cpts_selftest_kernel(const double *__restrict__ x, const int64_t *__restrict__ off,
                                                                    int64_t n_series, int B, int m, int32_t *cpts, int32_t *status,
                                                                    unsigned char *scratch, size_t slot_bytes, int64_t cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    OptLds &S = *reinterpret_cast<OptLds *>(smem);
    const int tid = threadIdx.x;
    unsigned char *slot = scratch + (size_t)blockIdx.x * slot_bytes;
    for (int64_t i = blockIdx.x; i < n_series; i += gridDim.x) {
        __syncthreads();
        const int64_t N64 = off[i + 1] - off[i];
        int32_t *out = cpts + i * (B + 2);
        if (N64 < 0 || N64 > cap || (int64_t)(B + 1) * m > N64) {
            for (int j = tid; j < B + 2; j += kOB) out[j] = -1;
            if (tid == 0) status[i] = N64 < 0 || N64 > cap ? WDX_READ_FAIL_UNKNOWN : WDX_READ_FAIL_SEGMENT;
            continue;
        }
        const int N = (int)N64;
        const bool lds = N <= kOptLdsCap;
        const OptArrays arr = opt_arrays(S, slot, N, B, cap, lds);
        for (int j = tid; j < N; j += kOB) arr.V1[j] = x[off[i] + j];
        __syncthreads();
        bool finite;
        if (lds) finite = optimal_cpts(opt_arrays(S, slot, N, B, cap, true), N, B, m, S.cp);
        else finite = optimal_cpts(opt_arrays(S, slot, N, B, cap, false), N, B, m, S.cp);
        for (int j = tid; j < B + 2; j += kOB) out[j] = finite ? S.cp[j] : -1;
        if (tid == 0) status[i] = finite ? WDX_READ_OK : WDX_READ_FAIL_SEGMENT;
    }
}

}  // namespace

// (the slot plan -- optimal_slot_bytes, optimal_tail_cap, plan_refine_optimal -- is wdx_refine_optimal_plan.h)
int64_t fingerprint_optimal_bytes(int64_t n_reads, int64_t max_len, int32_t barcode_segm_events) {
    return n_reads > 0 ? (int64_t)plan_refine_optimal(n_reads, max_len, barcode_segm_events).bytes : 0;
}

static int ensure_optimal_lds() {
    static LdsAttr attr_k, attr_s;
    if (int rc = attr_k.ensure(fingerprint_refine_optimal_kernel, sizeof(OptLds))) return rc;
    return attr_s.ensure(optimal_cpts_selftest_kernel, sizeof(OptLds));
}

int launch_refine_optimal(FpArgs A, const OptimalPlan &pl, void *d_scratch, hipStream_t stream) {
    if (A.n_reads == 0) return WDX_SUCCESS;
    if (!d_scratch) {
        set_error("optimal change-points: no scratch buffer");
        return WDX_ERR_INVALID;
    }
    if (int rc = ensure_optimal_lds()) return rc;
    A.block_base = 0;
    hipLaunchKernelGGL(fingerprint_refine_optimal_kernel, dim3((unsigned)pl.slots), dim3(kOB), sizeof(OptLds), stream, A,
                       reinterpret_cast<unsigned char *>(d_scratch), pl.slot_bytes, pl.cap);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

int launch_optimal_cpts_selftest(const double *d_x, const int64_t *d_off, int64_t n_series, int B, int m, int32_t *d_cpts,
                                 int32_t *d_status, const OptimalPlan &pl, void *d_scratch, hipStream_t stream) {
    if (n_series == 0) return WDX_SUCCESS;
    if (int rc = ensure_optimal_lds()) return rc;
    hipLaunchKernelGGL(optimal_cpts_selftest_kernel, dim3((unsigned)pl.slots), dim3(kOB), sizeof(OptLds), stream, d_x, d_off,
                       n_series, B, m, d_cpts, d_status, reinterpret_cast<unsigned char *>(d_scratch), pl.slot_bytes, pl.cap);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

}  // namespace wdx
