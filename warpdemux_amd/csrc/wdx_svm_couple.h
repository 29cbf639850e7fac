// What the SVM tail does BEHIND the decision values, one copy for the kernels that need it (wdx_svm.hip: phase 2 of
// svm_predict_mfma_kernel; wdx_svm_cv.hip: the out-of-fold probabilities of a cross-validation): libsvm's sigmoid_predict with the
// 1e-7 clamp, multiclass_probability, np.argmax with the first-maximum rule and top1 - top2.  Equal decision values and equal
// probA / probB give equal bits in both.
//
// One 16-lane group per read, four groups a wave.  Lane t of a group owns row t of Q in REGISTERS (Q is symmetric, so Q[u][t] of
// the update step is its own element u) together with Qp[t] and p[t]; what the sweep needs from other lanes (Qp[u], p[j]) comes by
// lane shuffle, the diagonal is replicated once per read.  No LDS round trip and no barrier inside the iteration: it is a chain of
// ~k shuffles + divisions per sweep, and with only the decision values and the pairwise table left in LDS more than twice as
// many waves fit a CU to hide it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace wdx {

struct SvmCoupled {
    double pt;       // lane t < k of the group: the probability of class t
    int best;        // every lane of the group: np.argmax (first maximum) ...
    double b1, b2;   // ... the largest and the second largest probability (the margin is b1 - b2)
};

// Called by all 64 lanes.  dr: the group's read's k (k - 1) / 2 decision values (LDS); pw: the group's k * k doubles of LDS
// scratch; 2 <= k <= 16.
__device__ __forceinline__ SvmCoupled svm_couple_group(const double *dr, const double *probA, const double *probB, double *pw, int k, int lane) {
    const int npairs = k * (k - 1) / 2;
    const int t = lane & 15, gbase = lane & 48;
    const bool on = t < k;
    for (int p = t; p < npairs; p += 16) {
        int i = 0, rem = p;
        while (rem >= k - 1 - i) {
            rem -= k - 1 - i;
            ++i;
        }
        const int j = i + 1 + rem;
        const double fApB = dr[p] * probA[p] + probB[p];
        double v = fApB >= 0 ? exp(-fApB) / (1.0 + exp(-fApB)) : 1.0 / (1.0 + exp(fApB));
        v = fmin(fmax(v, 1e-7), 1.0 - 1e-7);
        pw[i * k + j] = v;
        pw[j * k + i] = 1.0 - v;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    double qrow[16];  // (the diagonal element of the sweep step comes by shuffle: registers are what limits the wave count)
    {
        double qtt = 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const bool in = on && j < k && j != t;
            const double a = in ? pw[j * k + t] : 0.0;  // r[j][t]
            const double b = in ? pw[t * k + j] : 0.0;  // r[t][j]
            qtt += a * a;
            qrow[j] = -a * b;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) qrow[j] = (j == t) ? qtt : qrow[j];
    }
    __builtin_amdgcn_wave_barrier();  // pw is rewritten for the next read only after every lane has its row
    double pt = 1.0 / k, qp = 0.0;
    const double eps = 0.005 / k;
    const int max_iter = k > 100 ? k : 100;
    bool live = true;  // per 16-lane group; the wave keeps sweeping until every group has converged
    for (int iter = 0; iter < max_iter; ++iter) {
        // Qp[t] = sum_j Q[t][j] p[j] and pQp = sum_t p[t] Qp[t], both in libsvm's index order
        double qn = 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j < k) qn += qrow[j] * __shfl(pt, gbase + j);
        if (live) qp = qn;
        const double pq = pt * qp;
        double pQp = 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j < k) pQp += __shfl(pq, gbase + j);
        double err = on ? fabs(qp - pQp) : 0.0;
        for (int off = 8; off > 0; off >>= 1) err = fmax(err, __shfl_xor(err, off));
        if (err < eps) live = false;
        if (!__ballot(live)) break;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            if (u < k) {  // wave-uniform
                // libsvm divides three times by (1 + diff); one reciprocal here, which moves the iterates
                // by ~1e-16
                const double Qpu = __shfl(qp, gbase + u);
                const double Quu = __shfl(qrow[u], gbase + u);
                const double diff = (-Qpu + pQp) / Quu;
                const double inv = 1.0 / (1 + diff);
                double pn = pt;
                if (t == u) pn += diff;
                pn *= inv;
                const double qpn = (qp + diff * qrow[u]) * inv;
                pQp = (pQp + diff * (diff * Quu + 2 * Qpu)) * inv * inv;
                if (live) {
                    pt = pn;
                    qp = qpn;
                }
            }
        }
    }
    // process_probs: np.argmax (first maximum), margin top1 - top2
    int best = 0;
    double b1 = __shfl(pt, gbase), b2 = -1.0;
#pragma unroll
    for (int j = 1; j < 16; ++j) {
        if (j < k) {
            const double v = __shfl(pt, gbase + j);
            if (v > b1) {
                b2 = b1;
                b1 = v;
                best = j;
            } else if (v > b2) {
                b2 = v;
            }
        }
    }
    return SvmCoupled{pt, best, b1, b2};
}

}  // namespace wdx
