// Live path (BASELINE config 5): all reads of one 100 ms chunk round in ONE call.
// Replaces the per-read loops of live_balancing/worker.py:26-96 (segmentation_worker: extract_adapter, MAD
// clip, segment_signal, normalize, keep the last K events) and :99-131 (classification_worker:
// model.predict(fpt, nproc=1)).  Ragged host rows in, results out; staged through page-locked buffers on the
// context's own stream: one host->device copy, the kernel chain, one device->host copy, one synchronisation.
//
// One tick body (live_tick) serves every combination wdx_live_tick_ex offers -- float32 or int16 rows, the plain or the
// consensus-refinement fingerprint, no tail / SVM / MLP / boost -- and wdx_live_tick, which is the float32 + plain +
// [SVM] corner of it with its own, older argument list.  What is enqueued, in stream order:
//   H2D   the staging block: per-read index arrays + the adapter windows (float32, or int16 at 2 bytes per sample)
//   [decode_adc_kernel        int16 windows -> calibrated float32 windows, NaN tail where a window passes the read's end]
//   [refine_prepare           refinement: refine_idx = -1, the hand-over records' state words = 0]
//   fingerprint chain         plain or refinement branch; fpt, dwell, stats, status [, refine_idx] straight into the output block
//   [DTW + call               when references are resident]
//   [tail                     SVM or MLP on the distances, boost on the fingerprints]
//   D2H   the wanted pieces of the output block, which lie at its front back to back
// No new kernel: every producer writes its piece of the output block in place, so nothing has to be gathered.
#include "wdx_ctx.h"
#include "wdx_window.h"

#include <string.h>

#include <algorithm>

using namespace wdx;

namespace {

// The device / page-locked output block: the pieces the caller asked for first, back to back (they are what the one
// device->host copy moves), the pieces only the device needs (fingerprints and distances nobody asked for) behind them.
enum Piece { P_FPT, P_DWELL, P_STATS, P_PROB, P_CONF, P_CNT, P_DIST, P_RIDX, P_STATUS, P_CALL, P_PRED, P_COUNT };
struct OutBlock {
    size_t off[P_COUNT] = {}, bytes[P_COUNT] = {};
    bool want[P_COUNT] = {};
    size_t copy_bytes = 0, total = 0;
    // need: the piece exists on the device; wanted: it travels back.  8-byte pieces before 4-byte ones (enum order).
    void lay_out(const bool (&need)[P_COUNT]) {
        size_t o = 0;
        for (int pass = 0; pass < 2; ++pass) {
            for (int q = 0; q < P_COUNT; ++q) {
                if (!need[q] || want[q] != (pass == 0)) continue;
                off[q] = o;
                o += (bytes[q] + 7) / 8 * 8;
            }
            if (pass == 0) copy_bytes = o;
        }
        total = o;
    }
};

int live_tick(wdx_ctx *ctx, const wdx_live_in *in, const wdx_seg_params *p_in, const wdx_refine_params *rp, int64_t n_refs,
              uint32_t want, const wdx_minibatch_out *out, int32_t *refine_idx, int64_t *n_nonfinite, bool legacy) {
    WDX_ENTER(ctx);
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
    wdx_seg_params pv;   // K of the outputs, of the DTW and of the boost tail
    if ((rc = refine_seg_params("live_tick", p_in, rp, &pv))) return rc;
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
    const wdx_seg_params *p = &pv;
    const int64_t K = p->barcode_num_events;
    if (K < 1) {
        set_error("barcode_num_events must be >= 1");
        return WDX_ERR_INVALID;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    DtwRefs &R = ctx->refs;
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
        if ((rc = check_ref_length(R, *p))) return rc;
        if (n_refs != R.nY) {
            set_error("live_tick: the caller sized `dist` for %lld references but %lld are resident", (long long)n_refs,
                      (long long)R.nY);
            return WDX_ERR_INVALID;
        }
    }
    const int64_t nY = resident ? R.nY : 0;
    if (tail == WDX_LIVE_TAIL_SVM && (!ctx->svm.set || ctx->svm.dev.n_train != nY)) {
        set_error("live_tick: use_svm needs wdx_svm_set_model with a model trained on the resident reference set");
        return WDX_ERR_NO_REFS;
    }
    // (the SVM's two refusals above share one code here and nowhere else: kept as found)
    if (tail != WDX_LIVE_TAIL_SVM && (rc = tail_ready(ctx, tail, nY, K, rp != nullptr, "live_tick"))) return rc;
    if (p->padding < 0) {
        set_error("padding must be >= 0");
        return WDX_ERR_INVALID;
    }
    for (int64_t r = 0; r < n_reads; ++r) {
        const void *row = adc ? (const void *)in->adc_rows[r] : (const void *)in->rows[r];
        if (in->row_len[r] < 0 || (in->row_len[r] > 0 && !row)) {
            set_error("live_tick: row %lld is null or has a negative length", (long long)r);
            return WDX_ERR_INVALID;
        }
    }
    if (n_nonfinite) *n_nonfinite = 0;   // (behind every refusal: a refused tick writes nothing)
    hipStream_t s = ctx->stream;
    if ((rc = use_stream(ctx, s))) return rc;
    const int32_t *row_len = in->row_len, *a_start = in->a_start, *a_end = in->a_end;
    const uint8_t *ok = in->ok;
    const size_t n = (size_t)n_reads;

    // ---- adapter windows (extract_adapter, sig_proc.py:382-391), packed into the page-locked staging block ---------
    // float32: [int64 off[n+1]] [int32 zero[n]] [int32 len[n]] [uint8 ok[n] padded] [float samples, back to back]
    //          the packed row IS the window: a_start' = 0, a_end' = len makes [max(0, 0-pad), min(len, len+pad)) = the row
    // int16:   [int64 dst_off[n+1]] [int64 src_off[n]] [int32 zero[n]] [int32 win[n]] [int32 valid[n]] [float offset[n]]
    //          [float scale[n]] [uint8 ok[n] padded] [int16 samples, every row on a 16-byte boundary]
    //          row r stands for win[r] float32 samples, the first valid[r] of them the read's own, the rest the NaN tail
    //          of the *_adc contract (a window that runs past the read's end: wdx_minibatch_adc_in.row_win); decoded
    //          rows start on 32-byte boundaries of the float32 buffer (in1), as fingerprint_adc_rows lays them out
    // float32: the window inside the read, taken from its very first sample.  int16: a ragged row has no limit -- a window that
    // runs past the read's end keeps its NaN tail -- and a window beyond the kernels' limit keeps one sample more than the
    // limit (the context's, for the branch this tick runs: WDX_OPT_LONG_WINDOWS raises it for a plain tick,
    // WDX_OPT_LONG_REFINE_WINDOWS for one with refine parameters), which is what reports it.
    const WindowOpts wo{p->padding, 1, adc ? ctx->knobs.max_window(rp != nullptr) + 1 : 0};
    auto window = [&](int64_t r) {
        return adapter_window(a_start[r], a_end[r], adc ? kNoRowLimit : (int64_t)row_len[r], ok && !ok[r], wo, adc ? (int64_t)row_len[r] : -1);
    };
    // staged samples back to back (int16: every row on a 16-byte boundary); decoded int16 rows on 32-byte boundaries
    const int64_t src_round = adc ? 8 : 1, dst_round = 8;
    int64_t max_len = 0;
    PackedOffset fit(src_round), dfit(dst_round);   // (the sizing pass; the fill pass below counts again)
    for (int64_t r = 0; r < n_reads; ++r) {
        const Window w = window(r);
        max_len = std::max(max_len, w.win);
        fit.take(w.valid);
        dfit.take(w.row);
    }
    const int64_t total = fit.next, dst_total = dfit.next;
    size_t o_off = 0, o_src = 0, o_zero, o_len, o_valid = 0, o_cal = 0, o_ok, o_sig, in_bytes;
    if (adc) {
        o_src = (n + 1) * 8;
        o_zero = o_src + n * 8;
        o_len = o_zero + n * 4;
        o_valid = o_len + n * 4;
        o_cal = o_valid + n * 4;
        o_ok = o_cal + n * 8;
        o_sig = (o_ok + n + 15) / 16 * 16;
        in_bytes = o_sig + (size_t)total * 2;
    } else {
        o_zero = (n + 1) * 8;
        o_len = o_zero + n * 4;
        o_ok = o_len + n * 4;
        o_sig = (o_ok + n + 15) / 16 * 16;
        in_bytes = o_sig + (size_t)total * 4;
    }
    if ((rc = ctx->pin_in.ensure(in_bytes))) return rc;
    if ((rc = ctx->in0.ensure(in_bytes))) return rc;
    if (adc && (rc = ctx->in1.ensure((size_t)(dst_total ? dst_total : 1) * 4))) return rc;
    unsigned char *hin = (unsigned char *)ctx->pin_in.p;
    int64_t *h_off = (int64_t *)(hin + o_off), *h_src = (int64_t *)(hin + o_src);
    int32_t *h_zero = (int32_t *)(hin + o_zero), *h_len = (int32_t *)(hin + o_len), *h_valid = (int32_t *)(hin + o_valid);
    float *h_cal = (float *)(hin + o_cal);
    uint8_t *h_ok = hin + o_ok;
    PackedOffset pos(src_round), dpos(dst_round);
    for (int64_t r = 0; r < n_reads; ++r) {
        const Window w = window(r);
        const int64_t at = pos.take(w.valid);
        h_zero[r] = 0;
        h_len[r] = (int32_t)w.row;
        h_ok[r] = (!ok || ok[r]) ? 1 : 0;
        if (adc) {
            h_off[r] = dpos.take(w.row);
            h_src[r] = at;
            h_valid[r] = (int32_t)w.valid;
            h_cal[r] = in->offset[r];
            h_cal[n + r] = in->scale[r];
            if (w.valid > 0) memcpy((int16_t *)(hin + o_sig) + at, in->adc_rows[r] + w.first, (size_t)w.valid * 2);
        } else {
            h_off[r] = at;
            if (w.valid > 0) memcpy((float *)(hin + o_sig) + at, in->rows[r] + w.first, (size_t)w.valid * 4);
        }
    }
    h_off[n_reads] = adc ? dpos.next : pos.next;

    // ---- the output block -------------------------------------------------------------------------------------------
    const int k = tail == WDX_LIVE_TAIL_SVM ? ctx->svm.dev.k : tail == WDX_LIVE_TAIL_MLP ? ctx->mlp.dev.k
                : tail == WDX_LIVE_TAIL_BOOST ? ctx->boost.dev.k : 0;
    const bool run_dtw = nY > 0;
    // (a DTW tail without a single reference has nothing to read: as before, its outputs are left alone)
    const bool run_tail = tail == WDX_LIVE_TAIL_BOOST || (tail != WDX_LIVE_TAIL_NONE && run_dtw);
    OutBlock B;
    bool need[P_COUNT] = {};
    B.bytes[P_FPT] = n * K * 8, need[P_FPT] = true, B.want[P_FPT] = (want & WDX_WANT_FPT) != 0;
    B.bytes[P_DWELL] = n * K * 8, need[P_DWELL] = B.want[P_DWELL] = (want & WDX_WANT_DWELL) != 0;
    B.bytes[P_STATS] = n * 48, need[P_STATS] = B.want[P_STATS] = (want & WDX_WANT_STATS) != 0;
    B.bytes[P_PROB] = n * (size_t)k * 8, need[P_PROB] = run_tail, B.want[P_PROB] = run_tail && out->prob;
    B.bytes[P_CONF] = n * 8, need[P_CONF] = run_tail, B.want[P_CONF] = run_tail && out->conf;
    B.bytes[P_CNT] = 8, need[P_CNT] = B.want[P_CNT] = run_tail && tail == WDX_LIVE_TAIL_MLP;
    B.bytes[P_DIST] = n * (size_t)nY * 4, need[P_DIST] = run_dtw, B.want[P_DIST] = run_dtw && (want & WDX_WANT_DIST);
    B.bytes[P_RIDX] = n * 12, need[P_RIDX] = B.want[P_RIDX] = (want & WDX_WANT_REFINE_IDX) != 0;
    B.bytes[P_STATUS] = n * 4, need[P_STATUS] = B.want[P_STATUS] = true;
    B.bytes[P_CALL] = n * 4, need[P_CALL] = run_dtw, B.want[P_CALL] = run_dtw && out->call;
    B.bytes[P_PRED] = n * 4, need[P_PRED] = run_tail, B.want[P_PRED] = run_tail && out->pred;
    B.lay_out(need);
    if ((rc = ctx->out0.ensure(B.total))) return rc;
    if ((rc = ctx->pin_out.ensure(B.copy_bytes))) return rc;
    if ((rc = ctx->fp_ws.ensure((size_t)fingerprint_workspace_bytes(n_reads)))) return rc;
    unsigned char *din = (unsigned char *)ctx->in0.p, *dout = (unsigned char *)ctx->out0.p;
    unsigned char *hout = (unsigned char *)ctx->pin_out.p;
    double *d_fpt = (double *)(dout + B.off[P_FPT]), *d_prob = (double *)(dout + B.off[P_PROB]),
           *d_conf = (double *)(dout + B.off[P_CONF]);
    float *d_dist = (float *)(dout + B.off[P_DIST]);
    int32_t *d_status = (int32_t *)(dout + B.off[P_STATUS]), *d_call = (int32_t *)(dout + B.off[P_CALL]),
            *d_pred = (int32_t *)(dout + B.off[P_PRED]);
    int64_t *d_cnt = (int64_t *)(dout + B.off[P_CNT]);

    StreamDrain drain(s);
    WDX_HIP_TRY(hipMemcpyAsync(din, hin, in_bytes, hipMemcpyHostToDevice, s));
    const float *d_sig = (const float *)(din + o_sig);
    if (adc) {
        // decode_adc_kernel ahead of the unchanged chain: the windows, calibrated, and the NaN tail where one passes its read's end
        const float *d_cal = (const float *)(din + o_cal);
        const AdcRows rows{(const int16_t *)(din + o_sig), (const int64_t *)(din + o_src), 0, (const int32_t *)(din + o_valid),
                           d_cal, d_cal + n, (float *)ctx->in1.p, (const int64_t *)(din + o_off), 0, (const int32_t *)(din + o_len)};
        if ((rc = launch_adc_rows(rows, n_reads, false, s))) return rc;
        d_sig = (const float *)ctx->in1.p;
    }
    const FpReads rd{d_sig, (const int64_t *)(din + o_off), adc ? (const int32_t *)(din + o_len) : nullptr, 0, max_len, n_reads,
                     (const int32_t *)(din + o_zero), (const int32_t *)(din + o_len), (const uint8_t *)(din + o_ok)};
    ChainTail ct;
    ct.kind = tail;
    ct.svm = &ctx->svm.dev, ct.mlp = &ctx->mlp.dev, ct.boost = &ctx->boost.dev;
    ChainOut co{FpOut{d_fpt, need[P_DWELL] ? (int64_t *)(dout + B.off[P_DWELL]) : nullptr,
                      need[P_STATS] ? (double *)(dout + B.off[P_STATS]) : nullptr, d_status}};
    co.dist = d_dist, co.call = d_call, co.prob = d_prob, co.pred = d_pred, co.conf = d_conf, co.n_nonfinite = d_cnt;
    // main_events = false, with and without refinement: wdx_live_tick has never recorded them (wdx_ctx.h: fingerprint_stage)
    int32_t *d_ridx = need[P_RIDX] ? (int32_t *)(dout + B.off[P_RIDX]) : nullptr;
    if ((rc = demux_chain(ctx, resident ? R : DtwRefs{}, rd, *p, rp, d_ridx, nullptr, ctx->fp_ws.p, false, ct, co, s))) return rc;
    // one device->host copy: the wanted pieces are the front of the block
    WDX_HIP_TRY(hipMemcpyAsync(hout, dout, B.copy_bytes, hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipStreamSynchronize(s));
    drain.done();
    memcpy(out->status, hout + B.off[P_STATUS], B.bytes[P_STATUS]);
    if (out->call) {
        if (run_dtw) memcpy(out->call, hout + B.off[P_CALL], B.bytes[P_CALL]);
        else for (int64_t r = 0; r < n_reads; ++r) out->call[r] = -1;
    }
    if (B.want[P_DIST]) memcpy(out->dist, hout + B.off[P_DIST], B.bytes[P_DIST]);
    if (B.want[P_FPT]) memcpy(out->fpt, hout + B.off[P_FPT], B.bytes[P_FPT]);
    if (B.want[P_DWELL]) memcpy(out->dwell, hout + B.off[P_DWELL], B.bytes[P_DWELL]);
    if (B.want[P_STATS]) memcpy(out->stats, hout + B.off[P_STATS], B.bytes[P_STATS]);
    if (B.want[P_RIDX]) memcpy(refine_idx, hout + B.off[P_RIDX], B.bytes[P_RIDX]);
    if (B.want[P_PROB]) memcpy(out->prob, hout + B.off[P_PROB], B.bytes[P_PROB]);
    if (B.want[P_PRED]) memcpy(out->pred, hout + B.off[P_PRED], B.bytes[P_PRED]);
    if (B.want[P_CONF]) memcpy(out->conf, hout + B.off[P_CONF], B.bytes[P_CONF]);
    if (B.want[P_CNT] && n_nonfinite) memcpy(n_nonfinite, hout + B.off[P_CNT], 8);
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
