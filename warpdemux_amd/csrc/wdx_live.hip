// Live path (BASELINE config 5): all reads of one 100 ms chunk round in ONE call.
// Replaces the per-read loops of live_balancing/worker.py:26-96 (segmentation_worker: extract_adapter, MAD
// clip, segment_signal, normalize, keep the last K events) and :99-131 (classification_worker:
// model.predict(fpt, nproc=1)).  Ragged host rows in, results out; staged through page-locked buffers on the
// context's own stream: one host->device copy, the kernel chain, one device->host copy, one synchronisation.
//
// One tick body (live_tick) serves every combination wdx_live_tick_ex offers -- float32 or int16 rows, the plain or the
// consensus-refinement fingerprint, no tail / SVM / MLP / boost -- and wdx_live_tick, which is the float32 + plain +
// [SVM] corner of it with its own, older argument list.  The body in parts:
//   live_check_args, live_check_resident   every refusal, in the order they have always been made; a refused tick writes nothing
//   plan_tick_stage, out_plan              what is staged and what comes back (wdx_stage_plan.h: host arithmetic only)
//   fill_tick_stage                        the staging block: index columns, ok, the adapter windows
//   live_enqueue                           the copies and the kernel chain below, in stream order
//   deliver                                the output block's front into the caller's arrays
// What is enqueued:
//   H2D   the staging block: per-read index arrays + the adapter windows (float32, or int16 at 2 bytes per sample)
//   [decode_adc_kernel        int16 windows -> calibrated float32 windows, NaN tail where a window passes the read's end]
//   [refine_prepare           refinement: refine_idx = -1, the hand-over records' state words = 0]
//   fingerprint chain         plain or refinement branch; fpt, dwell, stats, status [, refine_idx] straight into the output block
//   [DTW + call               when references are resident]
//   [tail                     SVM or MLP on the distances, boost on the fingerprints]
//   D2H   the wanted pieces of the output block, which lie at its front back to back
// No new kernel: every producer writes its piece of the output block in place, so nothing has to be gathered.
#include "wdx_ctx.h"
#include "wdx_stage_plan.h"

using namespace wdx;

namespace {

// The refusals that need nothing of the context.  *pv: the parameters the chain runs with (K of the outputs, of the DTW and
// of the boost tail).  An empty tick (n_reads == 0) passes the first five and is not looked at further.
int live_check_args(const wdx_live_in *in, const wdx_seg_params *p_in, const wdx_refine_params *rp, uint32_t want,
                    const wdx_minibatch_out *out, const int32_t *refine_idx, wdx_seg_params *pv) {
    if (!in || !p_in || !out || in->n_reads < 0) {
        set_error("live_tick: bad arguments");
        return WDX_ERR_INVALID;
    }
    const int64_t n_reads = in->n_reads;
    const bool adc = in->adc_rows != nullptr;
    if (n_reads > 0 && (!in->row_len || !in->a_start || !in->a_end || !out->status)) {
        set_error("live_tick: bad arguments");
        return WDX_ERR_INVALID;
    }
    if (n_reads > 0 && (in->rows != nullptr) == adc) {
        set_error("live_tick: exactly one of rows / adc_rows must be given");
        return WDX_ERR_INVALID;
    }
    if (n_reads > 0 && adc && (!in->offset || !in->scale)) {
        set_error("live_tick: int16 rows need offset and scale of every read");
        return WDX_ERR_INVALID;
    }
    const int tail = in->tail;
    if (tail < WDX_LIVE_TAIL_NONE || tail > WDX_LIVE_TAIL_BOOST) {
        set_error("live_tick: unknown tail %d", tail);
        return WDX_ERR_INVALID;
    }
    if (want & ~(WDX_WANT_FPT | WDX_WANT_DIST | WDX_WANT_DWELL | WDX_WANT_STATS | WDX_WANT_REFINE_IDX)) {
        set_error("live_tick: `want` takes WDX_WANT_FPT / _DIST / _DWELL / _STATS / _REFINE_IDX only (the tail is wdx_live_in.tail)");
        return WDX_ERR_INVALID;
    }
    if (n_reads == 0) return WDX_SUCCESS;   // (and nothing was touched, *n_nonfinite included)
    if (int rc = refine_seg_params("live_tick", p_in, rp, pv)) return rc;
    if (rp && (tail == WDX_LIVE_TAIL_SVM || tail == WDX_LIVE_TAIL_MLP)) {
        set_error("live_tick: consensus refinement is served with no tail or the boost tail (no DTW model is trained on "
                  "refined fingerprints)");
        return WDX_ERR_INVALID;
    }
    if ((want & WDX_WANT_REFINE_IDX) && (!rp || !refine_idx)) {
        set_error("live_tick: WDX_WANT_REFINE_IDX needs refinement parameters and a refine_idx array");
        return WDX_ERR_INVALID;
    }
    if (((want & WDX_WANT_FPT) && !out->fpt) || ((want & WDX_WANT_DIST) && !out->dist) || ((want & WDX_WANT_DWELL) && !out->dwell) ||
        ((want & WDX_WANT_STATS) && !out->stats)) {
        set_error("live_tick: an output `want` asks for has no array");
        return WDX_ERR_INVALID;
    }
    if (pv->barcode_num_events < 1) {
        set_error("barcode_num_events must be >= 1");
        return WDX_ERR_INVALID;
    }
    return WDX_SUCCESS;
}

// The refusals that look at what is resident (the context's mutex is held), and the two of the arguments that have always
// come behind them.  *nY: the references the chain runs against (0: none).
int live_check_resident(const wdx_ctx *ctx, const wdx_live_in *in, const wdx_seg_params &p, bool refine, int64_t n_refs,
                        uint32_t want, bool legacy, int64_t *nY) {
    int rc = WDX_SUCCESS;
    const DtwRefs &R = ctx->refs;
    const int tail = in->tail;
    const bool resident = R.window != 0;
    if (!resident) {
        // no reference set: fingerprints [+ boost tail] only
        if (legacy || n_refs != 0 || tail == WDX_LIVE_TAIL_SVM || tail == WDX_LIVE_TAIL_MLP) {
            set_error("no reference set: call wdx_set_refs first");
            return WDX_ERR_NO_REFS;
        }
        if (want & WDX_WANT_DIST) {
            set_error("live_tick: a tick without references (n_refs = 0) has no distances");
            return WDX_ERR_INVALID;
        }
    } else {
        if ((rc = check_ref_length(R, p))) return rc;
        if (n_refs != R.nY) {
            set_error("live_tick: the caller sized `dist` for %lld references but %lld are resident", (long long)n_refs,
                      (long long)R.nY);
            return WDX_ERR_INVALID;
        }
    }
    *nY = resident ? R.nY : 0;
    if (tail == WDX_LIVE_TAIL_SVM && (!ctx->svm.set || ctx->svm.dev.n_train != *nY)) {
        set_error("live_tick: use_svm needs wdx_svm_set_model with a model trained on the resident reference set");
        return WDX_ERR_NO_REFS;
    }
    // (the SVM's two refusals above share one code here and nowhere else: kept as found)
    if (tail != WDX_LIVE_TAIL_SVM && (rc = tail_ready(ctx, tail, *nY, p.barcode_num_events, refine, "live_tick"))) return rc;
    if (p.padding < 0) {
        set_error("padding must be >= 0");
        return WDX_ERR_INVALID;
    }
    for (int64_t r = 0; r < in->n_reads; ++r) {
        const void *row = in->adc_rows ? (const void *)in->adc_rows[r] : (const void *)in->rows[r];
        if (in->row_len[r] < 0 || (in->row_len[r] > 0 && !row)) {
            set_error("live_tick: row %lld is null or has a negative length", (long long)r);
            return WDX_ERR_INVALID;
        }
    }
    return WDX_SUCCESS;
}

// The staging block (filled, in ctx->pin_in) -> the device, the kernel chain, the front of the output block -> ctx->pin_out;
// everything on s, the caller synchronises.  in0: the staging block; in1: the decoded rows of an int16 tick; out0: the block.
int live_enqueue(wdx_ctx *ctx, const TickStage &T, const OutPlan &B, int64_t n_reads, const wdx_seg_params &p,
                 const wdx_refine_params *rp, int tail, hipStream_t s) {
    int rc = WDX_SUCCESS;
    unsigned char *din = (unsigned char *)ctx->in0.p, *dout = (unsigned char *)ctx->out0.p;
    auto at = [&](OutPiece q) { return (void *)(dout + B.off[q]); };
    auto at_or_null = [&](OutPiece q) { return B.exists[q] ? at(q) : nullptr; };
    WDX_HIP_TRY(hipMemcpyAsync(din, ctx->pin_in.p, T.L.bytes, hipMemcpyHostToDevice, s));
    const uint8_t *d_ok = din + T.L.ok;
    FpReads rd;
    if (T.adc) {
        // decode_adc_kernel ahead of the unchanged chain: the windows, calibrated, and the NaN tail where one passes its read's end
        const AdcImage D(din, T.L);
        float *d_rows = (float *)ctx->in1.p;
        const AdcRows rows{(const int16_t *)(din + T.L.sig), D.src, 0, D.valid, D.offset, D.scale, d_rows, D.dst, 0, D.out};
        if ((rc = launch_adc_rows(rows, n_reads, false, s))) return rc;
        rd = FpReads{d_rows, D.dst, D.out, 0, T.max_len, n_reads, D.a_start, D.a_end, d_ok};
    } else {
        const int32_t *d_len = image_col<int32_t>(din, T.L, FT_LEN);
        rd = FpReads{(const float *)(din + T.L.sig), image_col<int64_t>(din, T.L, FT_OFF), nullptr, 0, T.max_len, n_reads,
                     image_col<int32_t>(din, T.L, FT_ZERO), d_len, d_ok};
    }
    ChainTail ct;
    ct.kind = tail;
    ct.svm = &ctx->svm.dev, ct.mlp = &ctx->mlp.dev, ct.boost = &ctx->boost.dev;
    ChainOut co{FpOut{(double *)at(P_FPT), (int64_t *)at_or_null(P_DWELL), (double *)at_or_null(P_STATS), (int32_t *)at(P_STATUS)}};
    co.dist = (float *)at(P_DIST), co.call = (int32_t *)at(P_CALL);
    co.prob = (double *)at(P_PROB), co.pred = (int32_t *)at(P_PRED), co.conf = (double *)at(P_CONF);
    co.n_nonfinite = (int64_t *)at(P_CNT);
    // main_events = false, with and without refinement: wdx_live_tick has never recorded them (wdx_ctx.h: fingerprint_stage)
    const DtwRefs R = ctx->refs.window != 0 ? ctx->refs : DtwRefs{};
    if ((rc = demux_chain(ctx, R, rd, p, rp, (int32_t *)at_or_null(P_RIDX), nullptr, ctx->fp_ws.p, false, ct, co, s))) return rc;
    // one device->host copy: the wanted pieces are the front of the block
    WDX_HIP_TRY(hipMemcpyAsync(ctx->pin_out.p, dout, B.copy_bytes, hipMemcpyDeviceToHost, s));
    return WDX_SUCCESS;
}

int live_tick(wdx_ctx *ctx, const wdx_live_in *in, const wdx_seg_params *p_in, const wdx_refine_params *rp, int64_t n_refs,
              uint32_t want, const wdx_minibatch_out *out, int32_t *refine_idx, int64_t *n_nonfinite, bool legacy) {
    WDX_ENTER(ctx);
    wdx_seg_params pv;
    if ((rc = live_check_args(in, p_in, rp, want, out, refine_idx, &pv))) return rc;
    const int64_t n_reads = in->n_reads;
    if (n_reads == 0) return WDX_SUCCESS;
    std::lock_guard<std::mutex> g(ctx->mu);
    int64_t nY = 0;
    if ((rc = live_check_resident(ctx, in, pv, rp != nullptr, n_refs, want, legacy, &nY))) return rc;
    if (n_nonfinite) *n_nonfinite = 0;   // (behind every refusal: a refused tick writes nothing)
    hipStream_t s = ctx->stream;
    if ((rc = use_stream(ctx, s))) return rc;
    // the longest window of the branch this tick runs (the context's: WDX_OPT_LONG_WINDOWS raises it for a plain tick,
    // WDX_OPT_LONG_REFINE_WINDOWS for one with refine parameters)
    const TickStage T = plan_tick_stage(*in, pv.padding, ctx->knobs.max_window(rp != nullptr) + 1);
    if ((rc = ctx->pin_in.ensure(T.L.bytes))) return rc;
    if ((rc = ctx->in0.ensure(T.L.bytes))) return rc;
    if (T.adc && (rc = ctx->in1.ensure((size_t)(T.dst_total ? T.dst_total : 1) * 4))) return rc;
    fill_tick_stage(*in, T, (unsigned char *)ctx->pin_in.p);
    const int tail = in->tail;
    const int k = tail == WDX_LIVE_TAIL_SVM ? ctx->svm.dev.k : tail == WDX_LIVE_TAIL_MLP ? ctx->mlp.dev.k
                : tail == WDX_LIVE_TAIL_BOOST ? ctx->boost.dev.k : 0;
    const OutPlan B = out_plan(n_reads, pv.barcode_num_events, nY, k, want, tail, rp != nullptr, have_of(*out));
    if ((rc = ctx->out0.ensure(B.total))) return rc;
    if ((rc = ctx->pin_out.ensure(B.copy_bytes))) return rc;
    if ((rc = ctx->fp_ws.ensure((size_t)fingerprint_workspace_bytes(n_reads)))) return rc;
    StreamDrain drain(s);
    if ((rc = live_enqueue(ctx, T, B, n_reads, pv, rp, tail, s))) return rc;
    WDX_HIP_TRY(hipStreamSynchronize(s));
    drain.done();
    deliver(B, (const unsigned char *)ctx->pin_out.p, *out, refine_idx, n_nonfinite);
    return WDX_SUCCESS;
}

}  // namespace

extern "C" {

int wdx_live_tick_ex(wdx_ctx *ctx, const wdx_live_in *in, const wdx_seg_params *p, const wdx_refine_params *rp, int64_t n_refs,
                     uint32_t want, const wdx_minibatch_out *out, int32_t *refine_idx, int64_t *n_nonfinite) {
    return live_tick(ctx, in, p, rp, n_refs, want, out, refine_idx, n_nonfinite, false);
}

// The float32 + plain branch + [SVM tail] corner of wdx_live_tick_ex under its own argument list: an output is wanted
// when its pointer is given, and a reference set is required (WDX_ERR_NO_REFS without one), as it always was.
int wdx_live_tick(wdx_ctx *ctx, const float *const *rows, const int32_t *row_len, int64_t n_reads,
                  const int32_t *a_start, const int32_t *a_end, const uint8_t *ok, const wdx_seg_params *p,
                  int64_t n_refs, int32_t use_svm, double *fpt, float *dist, int32_t *call, int32_t *status,
                  double *prob, int32_t *pred, double *conf) {
    const wdx_live_in in{rows, nullptr, nullptr, nullptr, row_len, n_reads, a_start, a_end, ok,
                         use_svm ? WDX_LIVE_TAIL_SVM : WDX_LIVE_TAIL_NONE, 0};
    const wdx_minibatch_out out{status, call, dist, fpt, nullptr, nullptr, prob, pred, conf};
    return live_tick(ctx, &in, p, nullptr, n_refs, (fpt ? WDX_WANT_FPT : 0u) | (dist ? WDX_WANT_DIST : 0u), &out, nullptr,
                     nullptr, true);
}

}  // extern "C"
