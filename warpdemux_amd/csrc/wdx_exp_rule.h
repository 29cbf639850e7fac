// exp_rule: the engine's stated exp(x) for x <= 0, one copy for every kernel that needs its bits to be defined (the Fpt_Boost
// trainer's softmax, wdx_boost_fit.hip; the kernel matrix of a DTW kernel machine, wdx_svm_kernel.hip).  The constants and the
// coefficients stay where the host programs read them: wdx_boost_fit_plan.h.
#pragma once
#include "wdx_boost_fit_plan.h"

#include <math.h>

namespace wdx {

// exp(x) for x <= 0 by the stated rule: every multiply and add rounded on its own (the build has -ffp-contract=off)
__device__ __forceinline__ double exp_rule(double x) {
    if (x < -700.0) return 0.0;
    constexpr BoostFitExpCoef C;
    const double kk = rint(x * kBoostFitLog2e);
    const double r = (x - kk * kBoostFitLn2Hi) - kk * kBoostFitLn2Lo;
    double P = C.c[kBoostFitExpDegree];
#pragma unroll
    for (int i = kBoostFitExpDegree - 1; i >= 0; --i) {
        P = P * r;
        P = P + C.c[i];
    }
    return ldexp(P, (int)kk);
}

}  // namespace wdx
