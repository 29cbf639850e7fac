// C ABI of libwdx_hip.so, classifier tails (include/wdx.h): the SVM and the MLP behind the DTW distances, and the boosted
// trees on the fingerprints themselves (at the end of the file; no DTW).  Host code only: the kernels are in wdx_svm.hip /
// wdx_mlp.hip / wdx_boost.hip / wdx_dtw.hip.  The two tails share one host path each for "raw rows -> fingerprints
// -> DTW row blocks -> tail" (wdx_demux_{svm,mlp}_dev) and "host rows in chunks -> DTW -> tail" (wdx_dtw_{svm,mlp}_predict);
// what differs between them -- the SVM's fused route, the MLP's counter -- is in the entry points (model checks: tail_ready).
#include "wdx_ctx.h"

#include <string.h>

#include <algorithm>
#include <new>

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
    const SvmDev &M = ctx->svm;
    const int k = M.k;
    int rc;
    if (ctx->svm_refs_gen != ctx->refs_gen || ctx->svm_refs_model_gen != ctx->svm_model_gen) {
        const size_t rb = (size_t)M.n_sv * R.Lpad * 8;
        if ((rc = ctx->svm_refs.ensure(rb + (size_t)M.n_sv))) return rc;
        if ((rc = launch_gather_rows(R.pad, R.has_nan, M.support, M.n_sv, R.Lpad, (double *)ctx->svm_refs.p,
                                     (uint8_t *)ctx->svm_refs.p + rb, s)))
            return rc;
        ctx->svm_refs_gen = ctx->refs_gen;
        ctx->svm_refs_model_gen = ctx->svm_model_gen;
    }
    const size_t rb = (size_t)M.n_sv * R.Lpad * 8;
    if ((rc = ctx->out0.ensure((size_t)ctx->svm_chunks * (k - 1) * (size_t)n_reads * 8))) return rc;
    {
        Timed t(ctx, WDX_K_DTW, s);
        if ((rc = launch_dtw_svm_partial(fpt, n_reads, (const double *)ctx->svm_refs.p, R.Lpad, R.halo,
                                         (const uint8_t *)ctx->svm_refs.p + rb, R.L, R.window, R.penalty, ctx->svm_coefT,
                                         ctx->svm_chunk_ref0, ctx->svm_chunk_slot, ctx->svm_chunks, k - 1, M.pwr, M.ngamma,
                                         (double *)ctx->out0.p, s, ctx->knobs.dtw_unfused, &ctx->dtw_last)))
            return rc;
    }
    {
        Timed t(ctx, WDX_K_SVM, s);
        if ((rc = launch_svm_finish(M, (const double *)ctx->out0.p, ctx->svm_halves, n_reads, d_prob, d_pred, d_conf, s)))
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
    const int k = ctx->svm.k;
    // (R.any_inf: the fused form has no distance matrix for launch_dtw_equal_inf to settle -- the row blocks do)
    const bool fused = !d_dist && R.L == 25 && R.window == 15 && !ctx->knobs.no_short_dtw && !ctx->knobs.svm_scalar && k >= 2 &&
                       k <= 16 && ctx->svm_chunks > 0 && !R.any_inf;
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
                return svm_tail(ctx, ctx->svm, dblk, m, nullptr, from_read(prob, b0, k), from_read(pred, b0), from_read(conf, b0), s);
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
    const int k = ctx->mlp.k;
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
            return launch_mlp_predict(ctx->mlp, dblk, m, d_status + r0 + b0, from_read(d_prob, r0 + b0, k),
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
    const BoostDev &M = ctx->boost;
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

extern "C" {

int wdx_svm_set_model(wdx_ctx *ctx, const wdx_svm_model *m) {
    WDX_ENTER(ctx);
    if (!m || m->n_classes < 2 || m->n_classes > 16 || m->n_sv < 1 || m->n_train < 1 || !m->n_support ||
        !m->support || !m->dual_coef || !m->rho || !m->probA || !m->probB || m->pwr_dist < 1) {
        set_error("svm_set_model: need 2..16 classes, support vectors, coefficients and Platt parameters");
        return WDX_ERR_INVALID;
    }
    const int k = m->n_classes, nsv = m->n_sv, np = k * (k - 1) / 2;
    int64_t tot = 0;
    std::vector<int32_t> start(k);
    for (int c = 0; c < k; ++c) {
        if (m->n_support[c] < 0) {
            set_error("svm_set_model: negative n_support");
            return WDX_ERR_INVALID;
        }
        start[c] = (int32_t)tot;
        tot += m->n_support[c];
    }
    if (tot != nsv) {
        set_error("svm_set_model: sum(n_support) != n_sv");
        return WDX_ERR_INVALID;
    }
    for (int s_ = 0; s_ < nsv; ++s_)
        if (m->support[s_] < 0 || m->support[s_] >= m->n_train) {
            set_error("svm_set_model: support index out of range");
            return WDX_ERR_INVALID;
        }
    std::lock_guard<std::mutex> g(ctx->mu);
    if ((rc = use_stream(ctx, ctx->stream))) return rc;
    WDX_HIP_TRY(hipStreamSynchronize(ctx->stream));  // no kernel may still be reading the previous model
    // a pipelined minibatch (WDX_WANT_SVM) may still be reading it too: its tail's arguments point into svm_buf, which is
    // rewritten in place below, and a slot's stream is non-blocking (as wdx_set_refs drains the slots for the reference set)
    for (wdx_ctx *S : ctx->slots)
        if (S) WDX_HIP_TRY(hipStreamSynchronize(S->stream));
    // one device block: [doubles: dual_coef | rho | probA | probB | thresholds][int32: n_support | start | support | label_map]
    const size_t nd = (size_t)(k - 1) * nsv + 3 * (size_t)np + (size_t)k;
    const size_t ni = 3 * (size_t)k + (size_t)nsv;
    ctx->svm_set = false;  // not set until the upload below has succeeded
    if ((rc = ctx->svm_buf.ensure(nd * 8 + ni * 4))) return rc;
    std::vector<unsigned char> h(nd * 8 + ni * 4);
    double *hd = reinterpret_cast<double *>(h.data());
    int32_t *hi = reinterpret_cast<int32_t *>(h.data() + nd * 8);
    size_t o = 0;
    memcpy(hd + o, m->dual_coef, (size_t)(k - 1) * nsv * 8); o += (size_t)(k - 1) * nsv;
    memcpy(hd + o, m->rho, (size_t)np * 8); o += np;
    memcpy(hd + o, m->probA, (size_t)np * 8); o += np;
    memcpy(hd + o, m->probB, (size_t)np * 8); o += np;
    if (m->thresholds) memcpy(hd + o, m->thresholds, (size_t)k * 8);
    memcpy(hi, m->n_support, (size_t)k * 4);
    memcpy(hi + k, start.data(), (size_t)k * 4);
    memcpy(hi + 2 * k, m->support, (size_t)nsv * 4);
    if (m->label_map) memcpy(hi + 2 * k + nsv, m->label_map, (size_t)k * 4);
    WDX_HIP_TRY(hipMemcpy(ctx->svm_buf.p, h.data(), h.size(), hipMemcpyHostToDevice));
    const double *dd = reinterpret_cast<const double *>(ctx->svm_buf.p);
    const int32_t *di = reinterpret_cast<const int32_t *>(reinterpret_cast<const unsigned char *>(ctx->svm_buf.p) + nd * 8);
    SvmDev &S = ctx->svm;
    S.dual_coef = dd;
    S.rho = dd + (size_t)(k - 1) * nsv;
    S.probA = S.rho + np;
    S.probB = S.probA + np;
    S.thresholds = m->thresholds ? S.probB + np : nullptr;
    S.n_support = di;
    S.start = di + k;
    S.support = di + 2 * k;
    S.label_map = m->label_map ? di + 2 * k + nsv : nullptr;
    S.k = k;
    S.n_sv = nsv;
    S.n_train = m->n_train;
    S.pwr = m->pwr_dist;
    S.ngamma = (float)(-m->gamma);
    // for the fused DTW + SVM path (wdx_demux_svm_dev): coefficients vector-major, two chunks per class
    {
        const int H = 2, nch = k * H;
        const size_t cb = (size_t)nsv * (k - 1) * 8, ib = (size_t)(2 * nch + 1) * 4;
        if ((rc = ctx->svm_fused.ensure(cb + ib))) return rc;
        std::vector<unsigned char> hf(cb + ib);
        double *ct = reinterpret_cast<double *>(hf.data());
        for (int s_ = 0; s_ < nsv; ++s_)
            for (int q = 0; q < k - 1; ++q) ct[(size_t)s_ * (k - 1) + q] = m->dual_coef[(size_t)q * nsv + s_];
        int32_t *ref0 = reinterpret_cast<int32_t *>(hf.data() + cb), *slot = ref0 + nch + 1;
        for (int c = 0; c < k; ++c) {
            const int half = (m->n_support[c] + 1) / 2;
            ref0[2 * c] = start[c];
            ref0[2 * c + 1] = start[c] + half;
            slot[2 * c] = 2 * c;
            slot[2 * c + 1] = 2 * c + 1;
        }
        ref0[nch] = nsv;
        WDX_HIP_TRY(hipMemcpy(ctx->svm_fused.p, hf.data(), hf.size(), hipMemcpyHostToDevice));
        ctx->svm_coefT = reinterpret_cast<const double *>(ctx->svm_fused.p);
        ctx->svm_chunk_ref0 = reinterpret_cast<const int32_t *>(reinterpret_cast<const unsigned char *>(ctx->svm_fused.p) + cb);
        ctx->svm_chunk_slot = ctx->svm_chunk_ref0 + nch + 1;
        ctx->svm_chunks = nch;
        ctx->svm_halves = H;
        ++ctx->svm_model_gen;
    }
    ctx->svm_set = true;
    return WDX_SUCCESS;
}

int wdx_svm_predict_dev(wdx_ctx *ctx, const float *d_dist, int64_t n, double *d_prob, int32_t *d_pred,
                        double *d_conf, void *stream) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    if (!ctx->svm_set) {
        set_error("no SVM model: call wdx_svm_set_model first");
        return WDX_ERR_NO_REFS;
    }
    if (n < 0 || (n > 0 && !d_dist)) {
        set_error("svm_predict_dev: bad arguments");
        return WDX_ERR_INVALID;
    }
    if ((rc = use_stream(ctx, (hipStream_t)stream))) return rc;
    return svm_tail(ctx, ctx->svm, d_dist, n, nullptr, d_prob, d_pred, d_conf, (hipStream_t)stream);
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
    const int k = ctx->svm.k;
    const int64_t chunk = host_chunk_rows(n, R.nY);
    if ((rc = ensure_chunk_buffers(ctx, chunk, k, 0))) return rc;
    StreamDrain drain(s);
    if ((rc = dtw_predict_chunks(ctx, X, n, chunk, k, prob, pred, conf, s, [&](const float *d, int64_t, int64_t m) {
            return svm_tail(ctx, ctx->svm, d, m, nullptr, (double *)ctx->out1.p, (int32_t *)ctx->out2.p, (double *)ctx->out3.p, s);
        })))
        return rc;
    WDX_HIP_TRY(hipStreamSynchronize(s));
    drain.done();
    return WDX_SUCCESS;
}

int wdx_mlp_set_model(wdx_ctx *ctx, const wdx_mlp_model *m) {
    WDX_ENTER(ctx);
    // every check before anything of the resident model is touched: a refused model keeps the previous one
    if (!m || (m->dtype_bytes != 4 && m->dtype_bytes != 8) || m->n_classes < 2 || m->n_layers < 1 || m->n_scalers < 0 ||
        m->hidden_activation < WDX_MLP_ACT_IDENTITY || m->hidden_activation > WDX_MLP_ACT_RELU) {
        set_error("mlp_set_model: need a float32 / float64 model with >= 2 classes, layers and a known activation");
        return WDX_ERR_INVALID;
    }
    const int nl = m->n_layers, k = m->n_classes;
    if (nl < 2 || nl > WDX_MLP_MAX_LAYERS) {
        set_error("mlp_set_model: %d hidden layers (1..%d supported)", nl - 1, WDX_MLP_MAX_LAYERS - 1);
        return WDX_ERR_UNSUPPORTED;
    }
    if (k > 16) {
        set_error("mlp_set_model: %d classes (2..16 supported)", k);
        return WDX_ERR_UNSUPPORTED;
    }
    if (m->n_scalers > WDX_MLP_MAX_SCALERS) {
        set_error("mlp_set_model: %d scaler steps (at most %d supported)", m->n_scalers, WDX_MLP_MAX_SCALERS);
        return WDX_ERR_UNSUPPORTED;
    }
    for (int i = 0; i <= nl; ++i)
        if (m->sizes[i] < 1) {
            set_error("mlp_set_model: layer size %d of entry %d", m->sizes[i], i);
            return WDX_ERR_INVALID;
        }
    for (int i = 0; i < nl; ++i)
        if (!m->coefs[i] || !m->intercepts[i]) {
            set_error("mlp_set_model: layer %d has no coefficients / intercepts", i);
            return WDX_ERR_INVALID;
        }
    const int nout = m->sizes[nl];
    if (nout != k && !(nout == 1 && k == 2)) {
        set_error("mlp_set_model: %d output units for %d classes", nout, k);
        return WDX_ERR_INVALID;
    }
    int widest = 16;
    for (int i = 1; i < nl; ++i) {
        if (m->sizes[i] > WDX_MLP_MAX_WIDTH) {
            set_error("mlp_set_model: hidden layer of %d units (at most %d supported)", m->sizes[i], WDX_MLP_MAX_WIDTH);
            return WDX_ERR_UNSUPPORTED;
        }
        widest = std::max(widest, m->sizes[i]);
    }
    const int64_t n_in = m->sizes[0];
    const size_t T = (size_t)m->dtype_bytes;
    // one device block: [doubles: scaler mean / scale steps | thresholds][working dtype: W_i | b_i ...][int32: label map]
    size_t nd = (m->thresholds ? (size_t)k : 0);
    for (int s_ = 0; s_ < m->n_scalers; ++s_) nd += (m->scaler_mean[s_] ? n_in : 0) + (m->scaler_scale[s_] ? n_in : 0);
    size_t nw = 0;
    for (int i = 0; i < nl; ++i) nw += (size_t)m->sizes[i] * m->sizes[i + 1] + (size_t)m->sizes[i + 1];
    const size_t bytes = nd * 8 + round_up((int64_t)(nw * T), 8) + (m->label_map ? (size_t)k * 4 : 0);
    std::lock_guard<std::mutex> g(ctx->mu);
    if ((rc = use_stream(ctx, ctx->stream))) return rc;
    WDX_HIP_TRY(hipStreamSynchronize(ctx->stream));  // no kernel may still be reading the previous model
    WDX_HIP_TRY(hipDeviceSynchronize());  // nor one on any other stream: the model is replaced in place
    std::vector<unsigned char> h(bytes);
    ctx->mlp_set = false;  // not set until the upload below has succeeded
    if ((rc = ctx->mlp_buf.ensure(bytes))) return rc;
    MlpDev M{};
    unsigned char *dev = (unsigned char *)ctx->mlp_buf.p;
    size_t o = 0;
    for (int s_ = 0; s_ < m->n_scalers; ++s_) {
        for (int which = 0; which < 2; ++which) {
            const double *src = which ? m->scaler_scale[s_] : m->scaler_mean[s_];
            if (!src) continue;
            memcpy(h.data() + o, src, (size_t)n_in * 8);
            (which ? M.scale[s_] : M.mean[s_]) = (const double *)(dev + o);
            o += (size_t)n_in * 8;
        }
    }
    if (m->thresholds) {
        memcpy(h.data() + o, m->thresholds, (size_t)k * 8);
        M.thresholds = (const double *)(dev + o);
        o += (size_t)k * 8;
    }
    for (int i = 0; i < nl; ++i) {
        const size_t wb = (size_t)m->sizes[i] * m->sizes[i + 1] * T, bb = (size_t)m->sizes[i + 1] * T;
        memcpy(h.data() + o, m->coefs[i], wb);
        M.coef[i] = dev + o;
        o += wb;
        memcpy(h.data() + o, m->intercepts[i], bb);
        M.bias[i] = dev + o;
        o += bb;
    }
    o = (size_t)round_up((int64_t)o, 8);
    if (m->label_map) {
        memcpy(h.data() + o, m->label_map, (size_t)k * 4);
        M.label_map = (const int32_t *)(dev + o);
    }
    WDX_HIP_TRY(hipMemcpy(ctx->mlp_buf.p, h.data(), h.size(), hipMemcpyHostToDevice));
    for (int i = 0; i <= nl; ++i) M.sizes[i] = m->sizes[i];
    M.n_layers = nl;
    M.n_scalers = m->n_scalers;
    M.dtype_bytes = m->dtype_bytes;
    M.hidden_act = m->hidden_activation;
    M.k = k;
    M.ld = (int)round_up(widest, 16) + 1;
    ctx->mlp = M;
    ctx->mlp_set = true;
    return WDX_SUCCESS;
}

int wdx_mlp_predict_dev(wdx_ctx *ctx, const float *d_dist, int64_t n, double *d_prob, int32_t *d_pred, double *d_conf,
                        int64_t *d_n_nonfinite, void *stream) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    if (!ctx->mlp_set) {
        set_error("no MLP model: call wdx_mlp_set_model first");
        return WDX_ERR_NO_REFS;
    }
    if (n < 0 || (n > 0 && !d_dist)) {
        set_error("mlp_predict_dev: bad arguments");
        return WDX_ERR_INVALID;
    }
    if ((rc = use_stream(ctx, (hipStream_t)stream))) return rc;
    Timed t(ctx, WDX_K_MLP, (hipStream_t)stream);
    return launch_mlp_predict(ctx->mlp, d_dist, n, nullptr, d_prob, d_pred, d_conf, d_n_nonfinite, (hipStream_t)stream);
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
    const int k = ctx->mlp.k;
    int64_t chunk = host_chunk_rows(n, R.nY);
    if (ctx->knobs.mlp_chunk_rows > 0) chunk = std::min<int64_t>(chunk, ctx->knobs.mlp_chunk_rows);
    if ((rc = ensure_chunk_buffers(ctx, chunk, k, 8))) return rc;   // (+ 8: the non-finite counter behind conf)
    int64_t *d_cnt = (int64_t *)((unsigned char *)ctx->out3.p + (size_t)chunk * 8);
    int64_t h_cnt = 0;
    StreamDrain drain(s);
    WDX_HIP_TRY(hipMemsetAsync(d_cnt, 0, 8, s));
    if ((rc = dtw_predict_chunks(ctx, X, n, chunk, k, prob, pred, conf, s, [&](const float *d, int64_t, int64_t m) {
            Timed t(ctx, WDX_K_MLP, s);
            return launch_mlp_predict(ctx->mlp, d, m, nullptr, (double *)ctx->out1.p, (int32_t *)ctx->out2.p,
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
    // every check before anything of the resident model is touched: a refused model keeps the previous one
    if (!m || m->n_trees < 1 || m->n_features < 1 || m->dim < 1 || m->n_classes < 2 || !m->depth || !m->leaf_values ||
        !m->bias) {
        set_error("boost_set_model: need >= 1 tree, >= 1 feature, >= 2 classes, depths, leaf values and a bias");
        return WDX_ERR_INVALID;
    }
    const int nt = m->n_trees, F = m->n_features, dim = m->dim, k = m->n_classes;
    if (F > WDX_BOOST_MAX_FEATURES) {
        set_error("boost_set_model: %d features (1..%d supported)", F, WDX_BOOST_MAX_FEATURES);
        return WDX_ERR_UNSUPPORTED;
    }
    if (dim > 16 || k > 16) {
        set_error("boost_set_model: %d values per leaf for %d classes (1..16 and 2..16 supported)", dim, k);
        return WDX_ERR_UNSUPPORTED;
    }
    if (dim != k && !(dim == 1 && k == 2)) {
        set_error("boost_set_model: %d values per leaf for %d classes", dim, k);
        return WDX_ERR_INVALID;
    }
    size_t n_splits = 0, n_leaves = 0;
    for (int t = 0; t < nt; ++t) {
        const int d = m->depth[t];
        if (d < 0) {
            set_error("boost_set_model: tree %d has depth %d", t, d);
            return WDX_ERR_INVALID;
        }
        if (d > WDX_BOOST_MAX_DEPTH) {
            set_error("boost_set_model: tree %d has depth %d (0..%d supported)", t, d, WDX_BOOST_MAX_DEPTH);
            return WDX_ERR_UNSUPPORTED;
        }
        n_splits += (size_t)d;
        n_leaves += (size_t)1 << d;
    }
    if (n_splits > 0x7fffffff) {
        set_error("boost_set_model: too many splits");
        return WDX_ERR_UNSUPPORTED;
    }
    if (n_splits && (!m->split_feature || !m->split_border)) {
        set_error("boost_set_model: splits without features / borders");
        return WDX_ERR_INVALID;
    }
    for (size_t i = 0; i < n_splits; ++i)
        if (m->split_feature[i] < 0 || m->split_feature[i] >= F) {
            set_error("boost_set_model: split %lld tests feature %d of %d", (long long)i, m->split_feature[i], F);
            return WDX_ERR_INVALID;
        }
    // one device block: [doubles: leaves | bias | thresholds][trees][splits][int32: label map]
    const size_t nd = n_leaves * dim + (size_t)dim + (m->thresholds ? (size_t)k : 0);
    const size_t o_trees = nd * 8, o_splits = o_trees + (size_t)nt * sizeof(BoostTree);
    const size_t o_labels = o_splits + n_splits * sizeof(BoostSplit);
    const size_t bytes = o_labels + (m->label_map ? (size_t)k * 4 : 0);
    std::vector<unsigned char> h;
    try {
        h.resize(bytes);
    } catch (const std::bad_alloc &) {  // any number of trees is accepted: the staging copy can be refused by the host
        set_error("boost_set_model: no host memory for a staging copy of %zu bytes", bytes);
        return WDX_ERR_UNSUPPORTED;
    }
    double *hd = reinterpret_cast<double *>(h.data());
    memcpy(hd, m->leaf_values, n_leaves * dim * 8);
    memcpy(hd + n_leaves * dim, m->bias, (size_t)dim * 8);
    if (m->thresholds) memcpy(hd + n_leaves * dim + dim, m->thresholds, (size_t)k * 8);
    BoostTree *ht = reinterpret_cast<BoostTree *>(h.data() + o_trees);
    BoostSplit *hs = reinterpret_cast<BoostSplit *>(h.data() + o_splits);
    {
        size_t s0 = 0, l0 = 0;
        for (int t = 0; t < nt; ++t) {
            ht[t] = BoostTree{(int32_t)s0, m->depth[t], (int64_t)l0};
            s0 += (size_t)m->depth[t];
            l0 += ((size_t)1 << m->depth[t]) * dim;
        }
    }
    for (size_t i = 0; i < n_splits; ++i)
        hs[i] = BoostSplit{(uint32_t)m->split_feature[i] | ((m->split_nan_true && m->split_nan_true[i]) ? 0x100u : 0u),
                           m->split_border[i]};
    if (m->label_map) memcpy(h.data() + o_labels, m->label_map, (size_t)k * 4);
    std::lock_guard<std::mutex> g(ctx->mu);
    if ((rc = use_stream(ctx, ctx->stream))) return rc;
    WDX_HIP_TRY(hipStreamSynchronize(ctx->stream));
    WDX_HIP_TRY(hipDeviceSynchronize());  // no kernel on any stream may still be reading the previous model (as the MLP's)
    // upload into a block of its own and swap only after it has succeeded: a failed allocation or copy keeps the previous model
    Buffer nb;
    if ((rc = nb.ensure(bytes))) return rc;
    if (hipError_t e = hipMemcpy(nb.p, h.data(), bytes, hipMemcpyHostToDevice); e != hipSuccess) {
        set_error("boost_set_model: hipMemcpy of %zu bytes failed: %s", bytes, hipGetErrorString(e));
        nb.release();
        return WDX_ERR_HIP;
    }
    ctx->boost_buf.release();
    ctx->boost_buf = nb;
    const unsigned char *dev = (const unsigned char *)ctx->boost_buf.p;
    BoostDev M{};
    M.leaves = (const double *)dev;
    M.bias = M.leaves + n_leaves * dim;
    M.thresholds = m->thresholds ? M.bias + dim : nullptr;
    M.trees = (const BoostTree *)(dev + o_trees);
    M.splits = (const BoostSplit *)(dev + o_splits);
    M.label_map = m->label_map ? (const int32_t *)(dev + o_labels) : nullptr;
    M.scale = m->scale;
    M.n_trees = nt;
    M.n_features = F;
    M.dim = dim;
    M.k = k;
    ctx->boost = M;  // (every pointer of the previous model is replaced here, in one step with its block above)
    ctx->boost_set = true;
    return WDX_SUCCESS;
}

int wdx_boost_predict_dev(wdx_ctx *ctx, const double *d_fpt, const int32_t *d_status, int64_t n, double *d_raw,
                          double *d_prob, int32_t *d_pred, double *d_conf, void *stream) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    if (!ctx->boost_set) {
        set_error("no boost model: call wdx_boost_set_model first");
        return WDX_ERR_NO_REFS;
    }
    if (n < 0 || (n > 0 && !d_fpt)) {
        set_error("boost_predict_dev: bad arguments");
        return WDX_ERR_INVALID;
    }
    if ((rc = use_stream(ctx, (hipStream_t)stream))) return rc;
    return boost_tail(ctx, ctx->boost, d_fpt, d_status, n, d_raw, d_prob, d_pred, d_conf, (hipStream_t)stream);
}

int wdx_boost_predict(wdx_ctx *ctx, const double *X, int64_t n, double *raw, double *prob, int32_t *pred, double *conf) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    if (!ctx->boost_set) {
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
    const BoostDev &M = ctx->boost;
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
        if ((rc = boost_tail(ctx, ctx->boost, (const double *)ctx->in0.p, nullptr, c, (double *)ctx->out0.p, (double *)ctx->out1.p,
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
