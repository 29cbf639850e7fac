// What the entry points with a classifier tail share (wdx_ctx.h): the model preconditions and the device chain "fingerprint
// stage -> DTW + call -> tail".  Host code only; nothing here computes results.
#include "wdx_ctx.h"

namespace wdx {

int tail_ready(const wdx_ctx *ctx, int tail, int64_t nY, int64_t K, bool refined, const char *who) {
    if ((tail == WDX_LIVE_TAIL_SVM || tail == WDX_LIVE_TAIL_MLP) && ctx->refs.window == 0) {
        set_error("no reference set: call wdx_set_refs first");
        return WDX_ERR_NO_REFS;
    }
    const bool set = tail == WDX_LIVE_TAIL_SVM ? ctx->svm.set : tail == WDX_LIVE_TAIL_MLP ? ctx->mlp.set
                   : tail == WDX_LIVE_TAIL_BOOST ? ctx->boost.set : true;
    if (!set) {
        set_error("%s needs wdx_%s_set_model first", who,
                  tail == WDX_LIVE_TAIL_SVM ? "svm" : tail == WDX_LIVE_TAIL_MLP ? "mlp" : "boost");
        return WDX_ERR_NO_REFS;
    }
    if (tail == WDX_LIVE_TAIL_SVM && nY != ctx->svm.dev.n_train) {
        set_error("reference set has %lld rows but the SVM was trained on %d", (long long)nY, ctx->svm.dev.n_train);
        return WDX_ERR_INVALID;
    }
    if (tail == WDX_LIVE_TAIL_MLP && nY != ctx->mlp.dev.sizes[0]) {
        set_error("reference set has %lld rows but the MLP takes %d inputs", (long long)nY, ctx->mlp.dev.sizes[0]);
        return WDX_ERR_INVALID;
    }
    if (tail == WDX_LIVE_TAIL_BOOST && K != ctx->boost.dev.n_features) {
        set_error("%s (%lld) != the boost model's features (%d)", refined ? "barcode_keep_events" : "barcode_num_events",
                  (long long)K, ctx->boost.dev.n_features);
        return WDX_ERR_INVALID;
    }
    return WDX_SUCCESS;
}

int demux_chain(wdx_ctx *B, const DtwRefs &R, const FpReads &rd, const wdx_seg_params &p, const wdx_refine_params *rp,
                int32_t *d_refine_idx, void *d_refine_ws, void *d_fp_ws, bool main_events, const ChainTail &tail,
                const ChainOut &out, hipStream_t s) {
    int rc = WDX_SUCCESS;
    const int64_t n_reads = rd.n_reads;
    RefineDev *rf = nullptr;
    RefineDevGuard rf_guard{rf};
    if (rp && (rc = refine_prepare(B, *rp, n_reads, d_refine_idx, d_refine_ws, s, &rf))) return rc;
    if ((rc = fingerprint_stage(B, rd, p, out.fp, d_fp_ws, s, rf, main_events))) return rc;
    if (R.nY > 0) {
        if ((rc = dtw_dev_locked(B, out.fp.fpt, n_reads, out.dist, out.call, s))) return rc;
        if ((rc = launch_count_calls(out.call, out.fp.status, n_reads, R.nY, out.counts, s))) return rc;
    }
    if (tail.kind == WDX_LIVE_TAIL_BOOST)
        // Fpt_Boost.predict on the fingerprint rows themselves (models/fpt_boost.py): no references, no distances; the
        // kernel gives failed reads pred -1 and NaN
        return boost_tail(B, *tail.boost, out.fp.fpt, out.fp.status, n_reads, out.raw, out.prob, out.pred, out.conf, s);
    // (a DTW tail without a single reference has nothing to read: its outputs are left alone)
    if (tail.kind == WDX_LIVE_TAIL_NONE || R.nY == 0) return WDX_SUCCESS;
    if (tail.kind == WDX_LIVE_TAIL_SVM)
        // the classifier tail on the distance rows that are on the device anyway (models/dtw_svm.py:90-93, models/utils.py:45-61);
        // failed reads: pred -1, NaN probabilities (the reference never shows them to the model)
        return svm_tail(B, *tail.svm, out.dist, n_reads, out.fp.status, out.prob, out.pred, out.conf, s);
    if (out.n_nonfinite) WDX_HIP_TRY(hipMemsetAsync(out.n_nonfinite, 0, 8, s));
    Timed t(B, WDX_K_MLP, s);
    return launch_mlp_predict(*tail.mlp, out.dist, n_reads, out.fp.status, out.prob, out.pred, out.conf, out.n_nonfinite, s);
}

}  // namespace wdx
