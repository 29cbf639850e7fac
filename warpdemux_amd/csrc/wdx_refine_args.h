// The refinement parameters as every entry point checks them -- the one statement of the rule (plain host C++17: no HIP,
// nothing of the context, so the system compiler builds it alone: tests/host/refine_args_check.cpp).
#pragma once
#include "../../include/wdx.h"

namespace wdx {

void set_error(const char *fmt, ...);

// which ranges of *rp a site refuses (a null p and a null rp->query are refused by every site)
enum : unsigned { kRefineQuery = 1u, kRefineKeep = 2u };

// *pv = the segmentation parameters the fingerprint stage runs with: *p, and under refinement (rp != null) K =
// rp->barcode_keep_events, which is the K of the outputs, of the DTW and of the boost tail.  Reported in this order, all
// WDX_ERR_INVALID: a null p or query ("<who>: bad arguments"), n_query < 1, barcode_keep_events < 1.
// (hidden: an inline function's symbol would otherwise join the library's exports)
__attribute__((visibility("hidden"))) inline int refine_seg_params(const char *who, const wdx_seg_params *p,
                                                                   const wdx_refine_params *rp, wdx_seg_params *pv,
                                                                   unsigned checks = kRefineQuery) {
    if (!p || (rp && !rp->query)) {
        set_error("%s: bad arguments", who);
        return WDX_ERR_INVALID;
    }
    if (rp && (checks & kRefineQuery) && rp->n_query < 1) {
        set_error("consensus refinement: empty query");
        return WDX_ERR_INVALID;
    }
    if (rp && (checks & kRefineKeep) && rp->barcode_keep_events < 1) {
        set_error("barcode_num_events must be >= 1");
        return WDX_ERR_INVALID;
    }
    *pv = *p;
    if (rp) pv->barcode_num_events = rp->barcode_keep_events;
    return WDX_SUCCESS;
}

}  // namespace wdx
