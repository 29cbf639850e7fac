// C ABI of libwdx_hip.so, classifier tails (include/wdx.h): the SVM and the MLP behind the DTW distances, and the boosted
// trees on the fingerprints themselves (at the end of the file; no DTW).  Host code only: the kernels are in wdx_svm.hip /
// wdx_mlp.hip / wdx_boost.hip / wdx_dtw.hip.  The two tails share one host path each for "raw rows -> fingerprints
// -> DTW row blocks -> tail" (wdx_demux_{svm,mlp}_dev) and "host rows in chunks -> DTW -> tail" (wdx_dtw_{svm,mlp}_predict);
// what differs between them -- the SVM's fused route, the MLP's counter -- is in the entry points (model checks: tail_ready).
#include "wdx_ctx.h"

#include <algorithm>

using namespace wdx;

namespace wdx {

int svm_tail(wdx_ctx *B, const SvmDev &M, const float *d_dist, int64_t n, const int32_t *d_status, double *d_prob,
             int32_t *d_pred, double *d_conf, hipStream_t s) {
    {
        Timed t(B, WDX_K_SVM, s);
        if (int rc = launch_svm_predict(M, d_dist, n, d_prob, d_pred, d_conf, s, B->knobs)) return rc;
    }
    return d_status ? launch_svm_mask_failed(d_status, n, M.k, d_prob, d_pred, d_conf, s) : WDX_SUCCESS;
}

int boost_tail(wdx_ctx *B, const BoostDev &M, const double *d_fpt, const int32_t *d_status, int64_t n, double *d_raw,
               double *d_prob, int32_t *d_pred, double *d_conf, hipStream_t s) {
    Timed t(B, WDX_K_BOOST, s);
    return launch_boost_predict(M, d_fpt, d_status, n, d_raw, d_prob, d_pred, d_conf, s, B->knobs);
}

}  // namespace wdx

// rows per block of wdx_demux_{svm,mlp}_dev when the caller names none: the (rows, nY) float32 distances of a block stay in
// the memory-side cache (<= 96 MiB)
static int64_t default_block_rows(int64_t nY) { return std::max<int64_t>(2048, (((int64_t)96 << 20) / (4 * nY)) / 64 * 64); }

// What wdx_demux_{svm,mlp}_dev do between their own checks and their tails: the fingerprints of the reads into d_fpt, or
// into the front of d_work when the caller does not want them (*fpt says where), the fingerprint workspace behind them.
static int demux_fingerprints(wdx_ctx *ctx, const FpReads &in, const wdx_seg_params &p, double *d_fpt, int32_t *d_status,
                              void *d_work, hipStream_t s, const double **fpt) {
    double *f = d_fpt ? d_fpt : (double *)d_work;
    *fpt = f;
    void *fp_ws = (unsigned char *)d_work + demux_work_layout(in.n_reads, p.barcode_num_events, false).fp_ws;
    return fingerprint_stage(ctx, in, p, FpOut{f, nullptr, nullptr, d_status}, fp_ws, s);
}

// DTW of the fingerprint rows against the resident references, `rows` at a time; every block's distances (in d_dist when the
// caller wants them, else in out0, which the caller has sized) go to tail(distances, first row, rows) while they are hot.
template <class Tail>
static int dtw_row_blocks(wdx_ctx *ctx, const double *fpt, int64_t n_reads, int64_t rows, float *d_dist, hipStream_t s,
                          Tail tail) {
    const DtwRefs &R = ctx->refs;
    for (int64_t r0 = 0; r0 < n_reads; r0 += rows) {
        const int64_t m = std::min(rows, n_reads - r0);
        float *dblk = d_dist ? d_dist + r0 * R.nY : (float *)ctx->out0.p;
        if (int rc = dtw_dev_locked(ctx, fpt + r0 * R.L, m, dblk, nullptr, s)) return rc;
        if (int rc = tail(dblk, r0, m)) return rc;
    }
    return WDX_SUCCESS;
}

// Host rows X (n, L) through DTW and a tail, `chunk` rows per pass: the (chunk, nY) float32 distance block stays <= 1 GiB and
// never leaves HBM.  Workspaces: in0 rows | out0 distances | out1 prob (chunk, k) | out2 pred | out3 conf (+ tail_bytes that
// the caller keeps behind them).
static int64_t host_chunk_rows(int64_t n, int64_t nY) {
    return std::max<int64_t>(1, std::min<int64_t>(n, ((int64_t)1 << 30) / (4 * nY)));
}
static int ensure_chunk_buffers(wdx_ctx *ctx, int64_t chunk, int k, size_t tail_bytes) {
    const DtwRefs &R = ctx->refs;
    int rc;
    if ((rc = ctx->in0.ensure((size_t)(chunk * R.L) * 8))) return rc;
    if ((rc = ctx->out0.ensure((size_t)(chunk * R.nY) * 4))) return rc;
    if ((rc = ctx->out1.ensure((size_t)chunk * k * 8))) return rc;
    if ((rc = ctx->out2.ensure((size_t)chunk * 4))) return rc;
    return ctx->out3.ensure((size_t)chunk * 8 + tail_bytes);
}
// ... enqueued on s: copy in, DTW, tail(distances, first row, rows) writing out1 / out2 / out3, copies out.  The caller
// holds the StreamDrain and synchronises.
template <class Tail>
static int dtw_predict_chunks(wdx_ctx *ctx, const double *X, int64_t n, int64_t chunk, int k, double *prob, int32_t *pred,
                              double *conf, hipStream_t s, Tail tail) {
    const DtwRefs &R = ctx->refs;
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t m = std::min(chunk, n - r0);
        WDX_HIP_TRY(hipMemcpyAsync(ctx->in0.p, X + r0 * R.L, (size_t)(m * R.L) * 8, hipMemcpyHostToDevice, s));
        if (int rc = dtw_dev_locked(ctx, (const double *)ctx->in0.p, m, (float *)ctx->out0.p, nullptr, s)) return rc;
        if (int rc = tail((const float *)ctx->out0.p, r0, m)) return rc;
        if (prob) WDX_HIP_TRY(hipMemcpyAsync(prob + r0 * k, ctx->out1.p, (size_t)m * k * 8, hipMemcpyDeviceToHost, s));
        if (pred) WDX_HIP_TRY(hipMemcpyAsync(pred + r0, ctx->out2.p, (size_t)m * 4, hipMemcpyDeviceToHost, s));
        if (conf) WDX_HIP_TRY(hipMemcpyAsync(conf + r0, ctx->out3.p, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    }
    return WDX_SUCCESS;
}

// Fused form of wdx_demux_svm_dev (the distances are not asked for, the shipped shape): dtw_short_svm_kernel over the
// references in support-vector order leaves the decision sums P[slot][q][read] -- 16 (k - 1) k bytes per read instead of 4 nY
// -- and the tail only adds them up, takes the sigmoids and runs the coupling.  No distance matrix, no row blocks.
static int svm_fused_route(wdx_ctx *ctx, const double *fpt, int64_t n_reads, double *d_prob, int32_t *d_pred, double *d_conf,
                           hipStream_t s) {
    const DtwRefs &R = ctx->refs;
    const SvmDev &M = ctx->svm.dev;
    const SvmFused &F = ctx->svm.fused;
    const int k = M.k;
    int rc;
    if (ctx->svm_refs_gen != ctx->refs_gen || ctx->svm_refs_model_gen != ctx->svm.gen) {
        const size_t rb = (size_t)M.n_sv * R.Lpad * 8;
        if ((rc = ctx->svm_refs.ensure(rb + (size_t)M.n_sv))) return rc;
        if ((rc = launch_gather_rows(R.pad, R.has_nan, M.support, M.n_sv, R.Lpad, (double *)ctx->svm_refs.p,
                                     (uint8_t *)ctx->svm_refs.p + rb, s)))
            return rc;
        ctx->svm_refs_gen = ctx->refs_gen;
        ctx->svm_refs_model_gen = ctx->svm.gen;
    }
    const size_t rb = (size_t)M.n_sv * R.Lpad * 8;
    if ((rc = ctx->out0.ensure((size_t)F.chunks * (k - 1) * (size_t)n_reads * 8))) return rc;
    {
        Timed t(ctx, WDX_K_DTW, s);
        if ((rc = launch_dtw_svm_partial(fpt, n_reads, (const double *)ctx->svm_refs.p, R.Lpad, R.halo,
                                         (const uint8_t *)ctx->svm_refs.p + rb, R.L, R.window, R.penalty, F.coefT,
                                         F.chunk_ref0, F.chunk_slot, F.chunks, k - 1, M.pwr, M.ngamma,
                                         (double *)ctx->out0.p, s, ctx->knobs.dtw_unfused, &ctx->dtw_last)))
            return rc;
    }
    {
        Timed t(ctx, WDX_K_SVM, s);
        if ((rc = launch_svm_finish(M, (const double *)ctx->out0.p, F.halves, n_reads, d_prob, d_pred, d_conf, s)))
            return rc;
    }
    return WDX_SUCCESS;
}

// ---- wdx_demux_{svm,mlp,boost}_dev and their *_adc_dev twins (int16 device shards): one body each, on the entry's DevRows ----

int wdx::demux_svm_dev_rows(wdx_ctx *ctx, const DevRows &rd, const wdx_seg_params *p, double *d_fpt, int32_t *d_status,
                            float *d_dist, double *d_prob, int32_t *d_pred, double *d_conf, void *d_work, int64_t block_rows,
                            void *stream) {
    WDX_ENTER(ctx);
    if (rd.f32.n_reads < 0 || !p || block_rows < 0 ||
        (rd.f32.n_reads > 0 && (rd.missing() || !rd.f32.a_start || !rd.f32.a_end || !d_status || !d_work))) {
        set_error("demux_svm_dev: bad arguments");
        return WDX_ERR_INVALID;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    DtwRefs &R = ctx->refs;
    if ((rc = tail_ready(ctx, WDX_LIVE_TAIL_SVM, R.nY, 0, false, "demux_svm_dev"))) return rc;
    if ((rc = check_ref_length(R, *p))) return rc;
    if (rd.f32.n_reads == 0) return WDX_SUCCESS;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = use_stream(ctx, s))) return rc;
    const int k = ctx->svm.dev.k;
    // (R.any_inf: the fused form has no distance matrix for launch_dtw_equal_inf to settle -- the row blocks do)
    const bool fused = !d_dist && R.L == 25 && R.window == 15 && !ctx->knobs.no_short_dtw && !ctx->knobs.svm_scalar && k >= 2 &&
                       k <= 16 && ctx->svm.fused.chunks > 0 && !R.any_inf;
    return for_each_slice(ctx, rd, false, p->padding, s, [&](const FpReads &in, int64_t r0) {
        int rc = WDX_SUCCESS;
        const int64_t n_reads = in.n_reads;
        // ASYMMETRY, kept: an explicit block_rows below 2048 is raised to 2048 here; wdx_demux_mlp_dev honours it
        const int64_t rows = std::min(n_reads, block_rows > 0 ? std::max<int64_t>(block_rows, 2048) : default_block_rows(R.nY));
        if (!d_dist && !fused && (rc = ctx->out0.ensure((size_t)(rows * R.nY) * 4))) return rc;
        double *prob = from_read(d_prob, r0, k), *conf = from_read(d_conf, r0);
        int32_t *pred = from_read(d_pred, r0), *status = d_status + r0;
        const double *fpt = nullptr;
        if ((rc = demux_fingerprints(ctx, in, *p, from_read(d_fpt, r0, R.L), status, d_work, s, &fpt))) return rc;
        if (fused)
            rc = svm_fused_route(ctx, fpt, n_reads, prob, pred, conf, s);
        else
            rc = dtw_row_blocks(ctx, fpt, n_reads, rows, from_read(d_dist, r0, R.nY), s, [&](const float *dblk, int64_t b0, int64_t m) {
                return svm_tail(ctx, ctx->svm.dev, dblk, m, nullptr, from_read(prob, b0, k), from_read(pred, b0), from_read(conf, b0), s);
            });
        if (rc) return rc;
        // failed reads are masked ONCE over all reads (of an int16 shard: of the slice), behind the last block
        return launch_svm_mask_failed(status, n_reads, k, prob, pred, conf, s);
    });
}

int wdx::demux_mlp_dev_rows(wdx_ctx *ctx, const DevRows &rd, const wdx_seg_params *p, double *d_fpt, int32_t *d_status,
                            float *d_dist, double *d_prob, int32_t *d_pred, double *d_conf, int64_t *d_n_nonfinite,
                            void *d_work, int64_t block_rows, void *stream) {
    WDX_ENTER(ctx);
    if (rd.f32.n_reads < 0 || !p || block_rows < 0 ||
        (rd.f32.n_reads > 0 && (rd.missing() || !rd.f32.a_start || !rd.f32.a_end || !d_status || !d_work))) {
        set_error("demux_mlp_dev: bad arguments");
        return WDX_ERR_INVALID;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    DtwRefs &R = ctx->refs;
    if ((rc = tail_ready(ctx, WDX_LIVE_TAIL_MLP, R.nY, 0, false, "demux_mlp_dev"))) return rc;
    if ((rc = check_ref_length(R, *p))) return rc;
    if (rd.f32.n_reads == 0) return WDX_SUCCESS;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = use_stream(ctx, s))) return rc;
    const int k = ctx->mlp.dev.k;
    return for_each_slice(ctx, rd, false, p->padding, s, [&](const FpReads &in, int64_t r0) {
        int rc = WDX_SUCCESS;
        const int64_t n_reads = in.n_reads;
        // ASYMMETRY, kept: an explicit block_rows is honoured as given; wdx_demux_svm_dev raises it to 2048
        const int64_t rows = std::min(n_reads, block_rows > 0 ? block_rows : default_block_rows(R.nY));
        if (!d_dist && (rc = ctx->out0.ensure((size_t)(rows * R.nY) * 4))) return rc;
        const double *fpt = nullptr;
        if ((rc = demux_fingerprints(ctx, in, *p, from_read(d_fpt, r0, R.L), d_status + r0, d_work, s, &fpt))) return rc;
        // (failed reads are masked by the kernel itself, block by block: its d_status argument)
        return dtw_row_blocks(ctx, fpt, n_reads, rows, from_read(d_dist, r0, R.nY), s, [&](const float *dblk, int64_t b0, int64_t m) {
            Timed t(ctx, WDX_K_MLP, s);
            return launch_mlp_predict(ctx->mlp.dev, dblk, m, d_status + r0 + b0, from_read(d_prob, r0 + b0, k),
                                      from_read(d_pred, r0 + b0), from_read(d_conf, r0 + b0), d_n_nonfinite, s);
        });
    });
}

int wdx::demux_boost_dev_rows(wdx_ctx *ctx, const DevRows &rd, const wdx_seg_params *p, const wdx_refine_params *rp,
                              double *d_fpt, int32_t *d_refine_idx, int32_t *d_status, double *d_raw, double *d_prob,
                              int32_t *d_pred, double *d_conf, void *d_work, void *stream) {
    WDX_ENTER(ctx);
    if (rd.f32.n_reads < 0 ||
        (rd.f32.n_reads > 0 && (rd.missing() || !rd.f32.a_start || !rd.f32.a_end || !d_status || !d_work))) {
        set_error("demux_boost_dev: bad arguments");
        return WDX_ERR_INVALID;
    }
    wdx_seg_params pv;
    if ((rc = refine_seg_params("demux_boost_dev", p, rp, &pv))) return rc;
    const int64_t K = pv.barcode_num_events;
    std::lock_guard<std::mutex> g(ctx->mu);
    if ((rc = tail_ready(ctx, WDX_LIVE_TAIL_BOOST, 0, K, rp != nullptr, "demux_boost_dev"))) return rc;
    if (rd.f32.n_reads == 0) return WDX_SUCCESS;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = use_stream(ctx, s))) return rc;
    // d_work as wdx_demux_refine_dev lays it out: [fpt][fingerprint workspace] | the refinement kernels' hand-over records
    unsigned char *w = (unsigned char *)d_work;
    const BoostDev &M = ctx->boost.dev;
    return for_each_slice(ctx, rd, rp != nullptr, pv.padding, s, [&](const FpReads &in, int64_t r0) {
        const DemuxWork W = demux_work_layout(in.n_reads, K, false);
        double *fpt = d_fpt ? d_fpt + r0 * K : (double *)w;
        ChainTail tail;
        tail.kind = WDX_LIVE_TAIL_BOOST;
        tail.boost = &M;
        ChainOut out{FpOut{fpt, nullptr, nullptr, d_status + r0}};
        out.raw = from_read(d_raw, r0, M.dim), out.prob = from_read(d_prob, r0, M.k);
        out.pred = from_read(d_pred, r0), out.conf = from_read(d_conf, r0);
        // (no DTW here, whatever is resident: an empty reference set)
        return demux_chain(ctx, DtwRefs{}, in, pv, rp, from_read(d_refine_idx, r0, 3), w + demux_refine_records_offset(W), w + W.fp_ws, !rp,
                           tail, out, s);
    });
}

// ---- the three setters: check, pack (wdx_model_image.h), install ------------------------------------------------------------

static int refused(const ModelCheck &c) {
    set_error("%s", c.msg);
    return c.code;
}

// The one way a model becomes resident (include/wdx.h, "Resident models").  The caller may have work pending on any stream of
// the device -- its own, a minibatch slot's -- that reads the previous model through pointers it took at its enqueue: the
// device is idle before anything of that model goes away.  The image goes into a block of its own, and block, record and
// flag are swapped only after the copy has succeeded: a failed allocation or copy keeps the previous model, still set.
// bind(res): res.dev (and what lies beside it) on res.block.p.
template <class R, class Image, class Bind>
static int install(wdx_ctx *ctx, R &res, const Image &img, const char *who, Bind bind) {
    std::lock_guard<std::mutex> g(ctx->mu);
    if (int rc = use_stream(ctx, ctx->stream)) return rc;
    WDX_HIP_TRY(hipStreamSynchronize(ctx->stream));
    WDX_HIP_TRY(hipDeviceSynchronize());
    const size_t bytes = img.bytes.size();
    Buffer nb;
    if (int rc = nb.ensure(bytes)) return rc;
    if (hipError_t e = hipMemcpy(nb.p, img.bytes.data(), bytes, hipMemcpyHostToDevice); e != hipSuccess) {
        set_error("%s: hipMemcpy of %zu bytes failed: %s", who, bytes, hipGetErrorString(e));
        nb.release();
        return WDX_ERR_HIP;
    }
    res.block.release();
    res.block = nb;
    bind(res);  // (every pointer of the previous model is replaced here, in one step with its block above)
    res.set = true;
    ++res.gen;
    return WDX_SUCCESS;
}

extern "C" {

int wdx_svm_set_model(wdx_ctx *ctx, const wdx_svm_model *m) {
    WDX_ENTER(ctx);
    SvmImage img;
    if (ModelCheck c = check_svm(m); c || (c = pack_svm(m, &img))) return refused(c);
    return install(ctx, ctx->svm, img, "svm_set_model", [&](ResidentSvm &R) {
        const SvmBound B = bind_svm(img, R.block.p);
        R.dev = B.dev;
        R.fused = B.fused;
    });
}

int wdx_svm_predict_dev(wdx_ctx *ctx, const float *d_dist, int64_t n, double *d_prob, int32_t *d_pred,
                        double *d_conf, void *stream) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    if (!ctx->svm.set) {
        set_error("no SVM model: call wdx_svm_set_model first");
        return WDX_ERR_NO_REFS;
    }
    if (n < 0 || (n > 0 && !d_dist)) {
        set_error("svm_predict_dev: bad arguments");
        return WDX_ERR_INVALID;
    }
    if ((rc = use_stream(ctx, (hipStream_t)stream))) return rc;
    return svm_tail(ctx, ctx->svm.dev, d_dist, n, nullptr, d_prob, d_pred, d_conf, (hipStream_t)stream);
}

int wdx_demux_svm_dev(wdx_ctx *ctx, const float *d_sig, const int64_t *d_row_off, const int32_t *d_row_len, int64_t stride,
                      int64_t max_len, int64_t n_reads, const int32_t *d_a_start, const int32_t *d_a_end,
                      const uint8_t *d_ok, const wdx_seg_params *p, double *d_fpt, int32_t *d_status, float *d_dist,
                      double *d_prob, int32_t *d_pred, double *d_conf, void *d_work, int64_t block_rows, void *stream) {
    return demux_svm_dev_rows(ctx, DevRows(d_sig, d_row_off, d_row_len, stride, max_len, n_reads, d_a_start, d_a_end, d_ok), p,
                              d_fpt, d_status, d_dist, d_prob, d_pred, d_conf, d_work, block_rows, stream);
}

int wdx_demux_svm_adc_dev(wdx_ctx *ctx, const wdx_adc_dev_in *in, int64_t max_len, int64_t n_reads, const int32_t *d_a_start,
                          const int32_t *d_a_end, const uint8_t *d_ok, const wdx_seg_params *p, double *d_fpt,
                          int32_t *d_status, float *d_dist, double *d_prob, int32_t *d_pred, double *d_conf, void *d_work,
                          int64_t block_rows, void *stream) {
    if (int e = adc_dev_in_ok("demux_svm_adc_dev", in)) return e;
    return demux_svm_dev_rows(ctx, DevRows(in, max_len, n_reads, d_a_start, d_a_end, d_ok), p, d_fpt, d_status, d_dist, d_prob,
                              d_pred, d_conf, d_work, block_rows, stream);
}

int wdx_dtw_svm_predict(wdx_ctx *ctx, const double *X, int64_t n, double *prob, int32_t *pred, double *conf) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    DtwRefs &R = ctx->refs;
    if ((rc = tail_ready(ctx, WDX_LIVE_TAIL_SVM, R.nY, 0, false, "dtw_svm_predict"))) return rc;
    if (n < 0 || (n > 0 && !X)) {
        set_error("dtw_svm_predict: bad arguments");
        return WDX_ERR_INVALID;
    }
    if (n == 0) return WDX_SUCCESS;
    hipStream_t s = ctx->stream;
    if ((rc = use_stream(ctx, s))) return rc;
    const int k = ctx->svm.dev.k;
    const int64_t chunk = host_chunk_rows(n, R.nY);
    if ((rc = ensure_chunk_buffers(ctx, chunk, k, 0))) return rc;
    StreamDrain drain(s);
    if ((rc = dtw_predict_chunks(ctx, X, n, chunk, k, prob, pred, conf, s, [&](const float *d, int64_t, int64_t m) {
            return svm_tail(ctx, ctx->svm.dev, d, m, nullptr, (double *)ctx->out1.p, (int32_t *)ctx->out2.p, (double *)ctx->out3.p, s);
        })))
        return rc;
    WDX_HIP_TRY(hipStreamSynchronize(s));
    drain.done();
    return WDX_SUCCESS;
}

int wdx_mlp_set_model(wdx_ctx *ctx, const wdx_mlp_model *m) {
    WDX_ENTER(ctx);
    MlpImage img;
    if (ModelCheck c = check_mlp(m); c || (c = pack_mlp(m, &img))) return refused(c);
    return install(ctx, ctx->mlp, img, "mlp_set_model", [&](Resident<MlpDev> &R) { R.dev = bind_mlp(img, R.block.p); });
}

int wdx_mlp_predict_dev(wdx_ctx *ctx, const float *d_dist, int64_t n, double *d_prob, int32_t *d_pred, double *d_conf,
                        int64_t *d_n_nonfinite, void *stream) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    if (!ctx->mlp.set) {
        set_error("no MLP model: call wdx_mlp_set_model first");
        return WDX_ERR_NO_REFS;
    }
    if (n < 0 || (n > 0 && !d_dist)) {
        set_error("mlp_predict_dev: bad arguments");
        return WDX_ERR_INVALID;
    }
    if ((rc = use_stream(ctx, (hipStream_t)stream))) return rc;
    Timed t(ctx, WDX_K_MLP, (hipStream_t)stream);
    return launch_mlp_predict(ctx->mlp.dev, d_dist, n, nullptr, d_prob, d_pred, d_conf, d_n_nonfinite, (hipStream_t)stream);
}

int wdx_dtw_mlp_predict(wdx_ctx *ctx, const double *X, int64_t n, double *prob, int32_t *pred, double *conf,
                        int64_t *n_nonfinite) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    DtwRefs &R = ctx->refs;
    if ((rc = tail_ready(ctx, WDX_LIVE_TAIL_MLP, R.nY, 0, false, "dtw_mlp_predict"))) return rc;
    if (n < 0 || (n > 0 && !X)) {
        set_error("dtw_mlp_predict: bad arguments");
        return WDX_ERR_INVALID;
    }
    if (n_nonfinite) *n_nonfinite = 0;
    if (n == 0) return WDX_SUCCESS;
    hipStream_t s = ctx->stream;
    if ((rc = use_stream(ctx, s))) return rc;
    const int k = ctx->mlp.dev.k;
    int64_t chunk = host_chunk_rows(n, R.nY);
    if (ctx->knobs.mlp_chunk_rows > 0) chunk = std::min<int64_t>(chunk, ctx->knobs.mlp_chunk_rows);
    if ((rc = ensure_chunk_buffers(ctx, chunk, k, 8))) return rc;   // (+ 8: the non-finite counter behind conf)
    int64_t *d_cnt = (int64_t *)((unsigned char *)ctx->out3.p + (size_t)chunk * 8);
    int64_t h_cnt = 0;
    StreamDrain drain(s);
    WDX_HIP_TRY(hipMemsetAsync(d_cnt, 0, 8, s));
    if ((rc = dtw_predict_chunks(ctx, X, n, chunk, k, prob, pred, conf, s, [&](const float *d, int64_t, int64_t m) {
            Timed t(ctx, WDX_K_MLP, s);
            return launch_mlp_predict(ctx->mlp.dev, d, m, nullptr, (double *)ctx->out1.p, (int32_t *)ctx->out2.p,
                                      (double *)ctx->out3.p, d_cnt, s);
        })))
        return rc;
    WDX_HIP_TRY(hipMemcpyAsync(&h_cnt, d_cnt, 8, hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipStreamSynchronize(s));
    drain.done();
    if (n_nonfinite) *n_nonfinite = h_cnt;
    return WDX_SUCCESS;
}

int wdx_demux_mlp_dev(wdx_ctx *ctx, const float *d_sig, const int64_t *d_row_off, const int32_t *d_row_len, int64_t stride,
                      int64_t max_len, int64_t n_reads, const int32_t *d_a_start, const int32_t *d_a_end,
                      const uint8_t *d_ok, const wdx_seg_params *p, double *d_fpt, int32_t *d_status, float *d_dist,
                      double *d_prob, int32_t *d_pred, double *d_conf, int64_t *d_n_nonfinite, void *d_work,
                      int64_t block_rows, void *stream) {
    return demux_mlp_dev_rows(ctx, DevRows(d_sig, d_row_off, d_row_len, stride, max_len, n_reads, d_a_start, d_a_end, d_ok), p,
                              d_fpt, d_status, d_dist, d_prob, d_pred, d_conf, d_n_nonfinite, d_work, block_rows, stream);
}

int wdx_demux_mlp_adc_dev(wdx_ctx *ctx, const wdx_adc_dev_in *in, int64_t max_len, int64_t n_reads, const int32_t *d_a_start,
                          const int32_t *d_a_end, const uint8_t *d_ok, const wdx_seg_params *p, double *d_fpt,
                          int32_t *d_status, float *d_dist, double *d_prob, int32_t *d_pred, double *d_conf,
                          int64_t *d_n_nonfinite, void *d_work, int64_t block_rows, void *stream) {
    if (int e = adc_dev_in_ok("demux_mlp_adc_dev", in)) return e;
    return demux_mlp_dev_rows(ctx, DevRows(in, max_len, n_reads, d_a_start, d_a_end, d_ok), p, d_fpt, d_status, d_dist, d_prob,
                              d_pred, d_conf, d_n_nonfinite, d_work, block_rows, stream);
}

// ---- Fpt_Boost: oblivious trees on the fingerprint rows (wdx_boost.hip) ----------------------------------

int wdx_boost_set_model(wdx_ctx *ctx, const wdx_boost_model *m) {
    WDX_ENTER(ctx);
    BoostImage img;
    if (ModelCheck c = check_boost(m); c || (c = pack_boost(m, &img))) return refused(c);
    return install(ctx, ctx->boost, img, "boost_set_model", [&](Resident<BoostDev> &R) { R.dev = bind_boost(img, R.block.p); });
}

int wdx_boost_predict_dev(wdx_ctx *ctx, const double *d_fpt, const int32_t *d_status, int64_t n, double *d_raw,
                          double *d_prob, int32_t *d_pred, double *d_conf, void *stream) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    if (!ctx->boost.set) {
        set_error("no boost model: call wdx_boost_set_model first");
        return WDX_ERR_NO_REFS;
    }
    if (n < 0 || (n > 0 && !d_fpt)) {
        set_error("boost_predict_dev: bad arguments");
        return WDX_ERR_INVALID;
    }
    if ((rc = use_stream(ctx, (hipStream_t)stream))) return rc;
    return boost_tail(ctx, ctx->boost.dev, d_fpt, d_status, n, d_raw, d_prob, d_pred, d_conf, (hipStream_t)stream);
}

int wdx_boost_predict(wdx_ctx *ctx, const double *X, int64_t n, double *raw, double *prob, int32_t *pred, double *conf) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    if (!ctx->boost.set) {
        set_error("no boost model: call wdx_boost_set_model first");
        return WDX_ERR_NO_REFS;
    }
    if (n < 0 || (n > 0 && !X)) {
        set_error("boost_predict: bad arguments");
        return WDX_ERR_INVALID;
    }
    if (n == 0) return WDX_SUCCESS;
    hipStream_t s = ctx->stream;
    if ((rc = use_stream(ctx, s))) return rc;
    const BoostDev &M = ctx->boost.dev;
    const int F = M.n_features, dim = M.dim, k = M.k;
    // rows per pass: the float64 rows of a chunk stay <= 1 GiB.  Workspaces: in0 rows | out0 raw | out1 prob | out2 pred | out3 conf
    int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, ((int64_t)1 << 30) / (8 * F)));
    if (ctx->knobs.boost_chunk_rows > 0) chunk = std::min<int64_t>(chunk, ctx->knobs.boost_chunk_rows);
    if ((rc = ctx->in0.ensure((size_t)(chunk * F) * 8))) return rc;
    if ((rc = ctx->out0.ensure((size_t)(chunk * dim) * 8))) return rc;
    if ((rc = ctx->out1.ensure((size_t)(chunk * k) * 8))) return rc;
    if ((rc = ctx->out2.ensure((size_t)chunk * 4))) return rc;
    if ((rc = ctx->out3.ensure((size_t)chunk * 8))) return rc;
    StreamDrain drain(s);
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t c = std::min(chunk, n - r0);
        WDX_HIP_TRY(hipMemcpyAsync(ctx->in0.p, X + r0 * F, (size_t)(c * F) * 8, hipMemcpyHostToDevice, s));
        if ((rc = boost_tail(ctx, ctx->boost.dev, (const double *)ctx->in0.p, nullptr, c, (double *)ctx->out0.p, (double *)ctx->out1.p,
                             (int32_t *)ctx->out2.p, (double *)ctx->out3.p, s)))
            return rc;
        if (raw) WDX_HIP_TRY(hipMemcpyAsync(raw + r0 * dim, ctx->out0.p, (size_t)(c * dim) * 8, hipMemcpyDeviceToHost, s));
        if (prob) WDX_HIP_TRY(hipMemcpyAsync(prob + r0 * k, ctx->out1.p, (size_t)(c * k) * 8, hipMemcpyDeviceToHost, s));
        if (pred) WDX_HIP_TRY(hipMemcpyAsync(pred + r0, ctx->out2.p, (size_t)c * 4, hipMemcpyDeviceToHost, s));
        if (conf) WDX_HIP_TRY(hipMemcpyAsync(conf + r0, ctx->out3.p, (size_t)c * 8, hipMemcpyDeviceToHost, s));
    }
    WDX_HIP_TRY(hipStreamSynchronize(s));
    drain.done();
    return WDX_SUCCESS;
}

int wdx_demux_boost_dev(wdx_ctx *ctx, const float *d_sig, const int64_t *d_row_off, const int32_t *d_row_len, int64_t stride,
                        int64_t max_len, int64_t n_reads, const int32_t *d_a_start, const int32_t *d_a_end,
                        const uint8_t *d_ok, const wdx_seg_params *p, const wdx_refine_params *rp, double *d_fpt,
                        int32_t *d_refine_idx, int32_t *d_status, double *d_raw, double *d_prob, int32_t *d_pred,
                        double *d_conf, void *d_work, void *stream) {
    return demux_boost_dev_rows(ctx, DevRows(d_sig, d_row_off, d_row_len, stride, max_len, n_reads, d_a_start, d_a_end, d_ok), p,
                                rp, d_fpt, d_refine_idx, d_status, d_raw, d_prob, d_pred, d_conf, d_work, stream);
}

int wdx_demux_boost_adc_dev(wdx_ctx *ctx, const wdx_adc_dev_in *in, int64_t max_len, int64_t n_reads,
                            const int32_t *d_a_start, const int32_t *d_a_end, const uint8_t *d_ok, const wdx_seg_params *p,
                            const wdx_refine_params *rp, double *d_fpt, int32_t *d_refine_idx, int32_t *d_status,
                            double *d_raw, double *d_prob, int32_t *d_pred, double *d_conf, void *d_work, void *stream) {
    if (int e = adc_dev_in_ok("demux_boost_adc_dev", in)) return e;
    return demux_boost_dev_rows(ctx, DevRows(in, max_len, n_reads, d_a_start, d_a_end, d_ok), p, rp, d_fpt, d_refine_idx,
                                d_status, d_raw, d_prob, d_pred, d_conf, d_work, stream);
}

}  // extern "C"
