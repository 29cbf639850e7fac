// The refining long form of the exact kernel (WDX_OPT_LONG_REFINE_WINDOWS: adapter windows of 16 385 .. 65 536 samples on
// the consensus-refinement branch) -- a translation unit of its own because it is BUILT differently: the Makefile lifts the
// AMDGPU inliner's basic-block limit for this file, so that fingerprint_long_refine_kernel is one function.  Left as calls,
// fp_refine_tail and the block primitives take FpArgs and their lambdas by address and the kernel's arguments go to scratch
// memory (as they do in the other forms of the exact kernel, which keep their code).  The templates are wdx_fingerprint.hip's;
// nothing else of it is compiled here.
#define WDX_DEV_KERNELS_ONLY 1
#define WDX_EXTRA_TU 1
#include "wdx_fingerprint.hip"

namespace wdx {

int launch_fp_long_refine(const FpArgs &A, const unsigned *count, const int32_t *list, int64_t grid, size_t lds_bytes,
                          hipStream_t stream) {
    static LdsAttr attr;
    if (int rc = attr.ensure(fingerprint_long_refine_kernel<kLongRefineBlock>, lds_bytes)) return rc;
    hipLaunchKernelGGL((fingerprint_long_refine_kernel<kLongRefineBlock>), dim3((unsigned)grid), dim3(kLongRefineBlock), lds_bytes,
                       stream, A, count, list);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

}  // namespace wdx
