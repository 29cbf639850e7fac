// The host-minibatch path behind include/wdx.h: float32 or int16 rows in host memory -> staged on the device -> the fingerprint
// stage [-> DTW -> call -> classifier tail] -> results in host memory; the blocking entries (wdx_demux_batch*,
// wdx_fingerprint_batch*) and the pipelined ones (wdx_demux_submit* / wdx_demux_wait*).  Nothing here computes results.
#include "wdx_ctx.h"
#include "wdx_window.h"

#include <string.h>

#include <algorithm>

using namespace wdx;

extern "C" {

struct MbHostOut {  // host destinations of one minibatch; null = not wanted (status always)
    int32_t *status = nullptr, *call = nullptr;
    float *dist = nullptr;
    double *fpt = nullptr;
    int64_t *dwell = nullptr;
    double *stats = nullptr, *prob = nullptr;
    int32_t *pred = nullptr;
    double *conf = nullptr;
};

// Way (i) in of float32 rows of one stride, pageable or not: the 2-D DMA copy of the columns that hold every adapter window
// of the batch into B->in0, a_start / a_end / ok into in1 / in2 / in3 (the caller sized all four); *rd = the reads as the
// fingerprint stage takes them.  The rows are NaN-padded to sig_preload_size (file_proc.py:244-260) and the kernels never
// read outside [start, stop), so nothing else has to travel.
static int fingerprint_float_columns(wdx_ctx *B, const wdx_minibatch_in &in, const WindowBatch &wb, FpReads *rd) {
    hipStream_t s = B->stream;
    const int64_t n_reads = in.n_reads, stride = in.stride;
    if (wb.col1 > wb.col0)
        WDX_HIP_TRY(hipMemcpy2DAsync((float *)B->in0.p + wb.col0, (size_t)stride * sizeof(float), in.sig + wb.col0,
                                     (size_t)stride * sizeof(float), (size_t)(wb.col1 - wb.col0) * sizeof(float),
                                     (size_t)n_reads, hipMemcpyHostToDevice, s));
    WDX_HIP_TRY(hipMemcpyAsync(B->in1.p, in.a_start, (size_t)n_reads * 4, hipMemcpyHostToDevice, s));
    WDX_HIP_TRY(hipMemcpyAsync(B->in2.p, in.a_end, (size_t)n_reads * 4, hipMemcpyHostToDevice, s));
    if (in.ok) WDX_HIP_TRY(hipMemcpyAsync(B->in3.p, in.ok, (size_t)n_reads, hipMemcpyHostToDevice, s));
    *rd = FpReads{(const float *)B->in0.p, nullptr, nullptr, stride, wb.max_len, n_reads, (const int32_t *)B->in1.p,
                  (const int32_t *)B->in2.p, in.ok ? (const uint8_t *)B->in3.p : nullptr};
    return WDX_SUCCESS;
}

// The float32 rows of one minibatch -> device (on B->stream); *rd = the reads as the fingerprint stage takes them.  (The
// refinement branch's sig_barcode_start counts from the window's first sample, which none of the three ways in moves.)
static int fingerprint_float_rows(wdx_ctx *B, const wdx_minibatch_in &in, const wdx_seg_params *p, FpReads *rd) {
    int rc = WDX_SUCCESS;
    hipStream_t s = B->stream;
    const float *sig = in.sig;
    const int64_t n_reads = in.n_reads, stride = in.stride;
    const int32_t *a_start = in.a_start, *a_end = in.a_end;
    const uint8_t *ok = in.ok;
    const bool packed_in = in.row_off != nullptr;
    WindowBatch wb(stride);
    const WindowOpts exact{p->padding, 1, 0};
    for (int64_t r = 0; r < n_reads; ++r)
        wb.add(adapter_window(a_start[r], a_end[r], packed_in ? (int64_t)in.row_len[r] : stride, ok && !ok[r], exact));
    const size_t sb = (size_t)(packed_in ? in.row_off[n_reads] : n_reads * stride) * sizeof(float);
    if ((rc = B->in0.ensure(sb ? sb : 4))) return rc;
    if ((rc = B->in1.ensure((size_t)n_reads * 4))) return rc;
    if ((rc = B->in2.ensure((size_t)n_reads * 4))) return rc;
    if ((rc = B->in3.ensure((size_t)n_reads))) return rc;
    // (Letting the FINGERPRINT kernel read a page-locked minibatch in place over the bus was measured and lost: 1.80 M
    // reads/s against 2.46 M with a DMA copy, which runs at 49 GB/s.)
    // Three ways in.  (i) The 2-D DMA copy of the column range that holds every adapter window of the batch -- all a
    // pageable array allows, and the best there is when every read's adapter starts at the same sample.  (ii) Rows that
    // carry whole reads have their adapters at different places (sig_proc.py:382-391: adapter_start varies per read) and
    // the column union is most of the row: when the minibatch is page-locked (wdx_host_alloc) and the windows are less
    // than 0.85 of the union, a copy kernel reads ONLY the windows over the bus, back to back into a packed device
    // buffer (pack_windows_kernel: pure copy, every load in flight), and the kernels run on the packed layout
    // (wdx_window.h).  (iii) Rows the CALLER packed (wdx_minibatch_in.row_off; the feeder's workers): one flat copy of
    // exactly the windows.
    const float *sig_dev = nullptr;  // the minibatch as the device sees it, when it is page-locked
    const uint8_t *d_ok = ok ? (const uint8_t *)B->in3.p : nullptr;
    if (!packed_in && wb.col1 > wb.col0 && (double)wb.win_total < 0.85 * (double)((wb.col1 - wb.col0) * n_reads)) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, sig) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer)
            sig_dev = (const float *)at.devicePointer;
        else
            (void)hipGetLastError();
    }
    if (packed_in) {
        // device images: off int64[n+1] | len int32[n] | a_start int32[n] | a_end int32[n], straight from the caller's arrays
        const size_t ib = (size_t)(n_reads + 1) * 8 + (size_t)n_reads * 12;
        if ((rc = B->pk_idx.ensure(ib))) return rc;
        int64_t *d_off = (int64_t *)B->pk_idx.p;
        int32_t *d_len = (int32_t *)(d_off + n_reads + 1), *d_as = d_len + n_reads, *d_ae = d_as + n_reads;
        if (sb) WDX_HIP_TRY(hipMemcpyAsync(B->in0.p, sig, sb, hipMemcpyHostToDevice, s));
        WDX_HIP_TRY(hipMemcpyAsync(d_off, in.row_off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, s));
        WDX_HIP_TRY(hipMemcpyAsync(d_len, in.row_len, (size_t)n_reads * 4, hipMemcpyHostToDevice, s));
        WDX_HIP_TRY(hipMemcpyAsync(d_as, a_start, (size_t)n_reads * 4, hipMemcpyHostToDevice, s));
        WDX_HIP_TRY(hipMemcpyAsync(d_ae, a_end, (size_t)n_reads * 4, hipMemcpyHostToDevice, s));
        if (ok) WDX_HIP_TRY(hipMemcpyAsync(B->in3.p, ok, (size_t)n_reads, hipMemcpyHostToDevice, s));
        *rd = FpReads{(const float *)B->in0.p, d_off, d_len, 0, wb.max_len, n_reads, d_as, d_ae, d_ok};
        return WDX_SUCCESS;
    }
    if (!sig_dev) return fingerprint_float_columns(B, in, wb, rd);
    // host images (page-locked, owned by the slot until its copy has run): off int64[n+1] | st int32[n] | len
    // int32[n] | a_start' int32[n] | a_end' int32[n]
    const size_t ib = (size_t)(n_reads + 1) * 8 + (size_t)n_reads * 16;
    if ((rc = B->pk_host.ensure(ib))) return rc;
    if ((rc = B->pk_idx.ensure(ib))) return rc;
    int64_t *h_off = (int64_t *)B->pk_host.p;
    int32_t *h_st = (int32_t *)(h_off + n_reads + 1), *h_len = h_st + n_reads, *h_as = h_len + n_reads, *h_ae = h_as + n_reads;
    const WindowOpts bus{p->padding, 4, 0};  // (up to three samples ahead of the window come along: 16-byte aligned bus reads)
    PackedOffset pos(4);                     // (rows start on 16-byte boundaries)
    for (int64_t r = 0; r < n_reads; ++r) {
        const Window w = adapter_window(a_start[r], a_end[r], stride, ok && !ok[r], bus);
        h_off[r] = pos.take(w.row);
        h_st[r] = (int32_t)w.first;
        h_len[r] = (int32_t)w.row;
        h_as[r] = w.a_start;
        h_ae[r] = w.a_end;
    }
    h_off[n_reads] = pos.next;
    if ((rc = B->in0.ensure((size_t)(pos.next ? pos.next : 1) * sizeof(float)))) return rc;
    WDX_HIP_TRY(hipMemcpyAsync(B->pk_idx.p, B->pk_host.p, ib, hipMemcpyHostToDevice, s));
    const int64_t *d_off = (const int64_t *)B->pk_idx.p;
    const int32_t *d_st = (const int32_t *)(d_off + n_reads + 1), *d_len = d_st + n_reads, *d_as = d_len + n_reads,
                  *d_ae = d_as + n_reads;
    if ((rc = launch_pack_windows(sig_dev, stride, n_reads, d_off, d_st, d_len, (float *)B->in0.p, s))) return rc;
    if (ok) WDX_HIP_TRY(hipMemcpyAsync(B->in3.p, ok, (size_t)n_reads, hipMemcpyHostToDevice, s));
    *rd = FpReads{(const float *)B->in0.p, d_off, d_len, 0, wb.max_len, n_reads, d_as, d_ae, d_ok};
    return WDX_SUCCESS;
}

// Argument checks of every *_adc entry point: host arithmetic only, so a bad descriptor is refused before (and without) a
// device.
static int adc_check_args(const char *who, const wdx_minibatch_adc_in *in) {
    if (!in) {
        set_error("%s: null minibatch", who);
        return WDX_ERR_INVALID;
    }
    const int64_t n = in->n_reads;
    if (n < 0 || (!in->row_off && (in->stride < 0 || in->stride > INT32_MAX)) ||
        (n > 0 && (!in->adc || !in->a_start || !in->a_end))) {
        set_error("%s: bad arguments", who);
        return WDX_ERR_INVALID;
    }
    if (n > 0 && !in->row_len) {
        set_error("%s: int16 rows need row_len (there is no NaN tail to find a read's end by)", who);
        return WDX_ERR_INVALID;
    }
    if (n > 0 && (!in->offset || !in->scale)) {
        set_error("%s: int16 rows need offset and scale of every read", who);
        return WDX_ERR_INVALID;
    }
    if (in->row_win && !in->row_off) {
        set_error("%s: row_win belongs to packed rows (row_off)", who);
        return WDX_ERR_INVALID;
    }
    for (int64_t r = 0; r < n; ++r) {
        const int64_t len = in->row_len[r];
        if (in->row_off) {
            const int64_t o0 = in->row_off[r], o1 = in->row_off[r + 1];
            if (o0 < 0 || (o0 & 7) || o1 < o0) {
                set_error("%s: packed row %lld: row_off must ascend in multiples of 8 (16-byte groups of int16)", who, (long long)r);
                return WDX_ERR_INVALID;
            }
            if (len < 0 || len > o1 - o0 || (in->row_win && in->row_win[r] < 0)) {
                set_error("%s: packed row %lld: row_len %lld does not fit its %lld samples", who, (long long)r, (long long)len,
                          (long long)(o1 - o0));
                return WDX_ERR_INVALID;
            }
        } else if (len < 0 || len > in->stride) {
            set_error("%s: row_len[%lld] = %lld is outside 0 .. stride (%lld)", who, (long long)r, (long long)len,
                      (long long)in->stride);
            return WDX_ERR_INVALID;
        }
    }
    return WDX_SUCCESS;
}

// The int16 ADC rows of one minibatch -> calibrated float32 windows in a PACKED device buffer (wdx_adc.hip); *rd = the reads
// as the fingerprint stage takes them.  The same three ways in as the float32 rows: (i) 2-D DMA copy of the int16 columns that hold
// the windows, then decode_adc_kernel; (ii) a page-locked minibatch: pack_windows_adc_kernel reads the windows over the
// bus; (iii) rows the caller packed: one flat copy, then decode_adc_kernel.  Row r of the packed buffer = the window of the
// float32 row the read stands for, its start rounded down to a multiple of 8 (16-byte groups of int16; wdx_window.h).
static int fingerprint_adc_rows(wdx_ctx *B, const wdx_minibatch_adc_in &A, const wdx_seg_params *p, FpReads *rd) {
    int rc = WDX_SUCCESS;
    hipStream_t s = B->stream;
    const int64_t n = A.n_reads, stride = A.stride;
    const bool packed_in = A.row_off != nullptr;
    // host images (page-locked, owned by the slot until its copy has run):
    // dst_off int64[n+1] | src_off int64[n] | n_out int32[n] | n_valid int32[n] | a_start' int32[n] | a_end' int32[n] |
    // offset float[n] | scale float[n]
    const size_t ib = (size_t)(n + 1) * 8 + (size_t)n * 8 + (size_t)n * 24;
    if ((rc = B->pk_host.ensure(ib))) return rc;
    if ((rc = B->pk_idx.ensure(ib))) return rc;
    if ((rc = B->in3.ensure((size_t)n))) return rc;
    int64_t *h_dst = (int64_t *)B->pk_host.p, *h_src = h_dst + n + 1;
    int32_t *h_out = (int32_t *)(h_src + n), *h_valid = h_out + n, *h_as = h_valid + n, *h_ae = h_as + n;
    float *h_cal = (float *)(h_ae + n);
    WindowBatch wb(stride);
    PackedOffset pos(8);   // (rows start on 32-byte boundaries)
    const WindowOpts exact{p->padding, 1, 0}, groups{p->padding, 8, 0};
    for (int64_t r = 0; r < n; ++r) {
        const bool dead = A.ok && !A.ok[r];
        Window w;
        if (packed_in) {
            // the caller's row as it stands; its window only bounds max_len
            w.row = A.row_win ? (int64_t)A.row_win[r] : (int64_t)A.row_len[r];
            w.valid = std::min<int64_t>(A.row_len[r], w.row);
            w.a_start = A.a_start[r];
            w.a_end = A.a_end[r];
            wb.max_len = std::max(wb.max_len, adapter_window(w.a_start, w.a_end, w.row, dead, exact).win);
            h_src[r] = A.row_off[r];
        } else {
            w = adapter_window(A.a_start[r], A.a_end[r], stride, dead, groups, A.row_len[r]);
            wb.add(w);
            h_src[r] = r * stride + w.first;
        }
        h_dst[r] = pos.take(w.row);
        h_out[r] = (int32_t)w.row;
        h_valid[r] = (int32_t)w.valid;
        h_as[r] = w.a_start;
        h_ae[r] = w.a_end;
        h_cal[r] = A.offset[r];
        h_cal[n + r] = A.scale[r];
    }
    h_dst[n] = pos.next;
    const int64_t col0 = wb.col0, col1 = wb.col1;
    if ((rc = B->in0.ensure((size_t)(pos.next ? pos.next : 1) * sizeof(float)))) return rc;
    WDX_HIP_TRY(hipMemcpyAsync(B->pk_idx.p, B->pk_host.p, ib, hipMemcpyHostToDevice, s));
    const int64_t *d_dst = (const int64_t *)B->pk_idx.p, *d_src = d_dst + n + 1;
    const int32_t *d_out = (const int32_t *)(d_src + n), *d_valid = d_out + n, *d_as = d_valid + n, *d_ae = d_as + n;
    const float *d_cal = (const float *)(d_ae + n);
    AdcRows rows{nullptr, d_src, 0, d_valid, d_cal, d_cal + n, (float *)B->in0.p, d_dst, 0, d_out};
    const int16_t *adc_dev = nullptr;  // the minibatch as the device sees it, when it is page-locked
    if (!packed_in && col1 > col0 && (double)wb.win_total < 0.85 * (double)((col1 - col0) * n)) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, A.adc) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer)
            adc_dev = (const int16_t *)at.devicePointer;
        else
            (void)hipGetLastError();
    }
    if (adc_dev) {
        rows.src = adc_dev;
    } else {
        const size_t sb = (size_t)(packed_in ? A.row_off[n] : n * stride) * sizeof(int16_t);
        if ((rc = B->in_adc.ensure(sb ? sb : 2))) return rc;
        if (packed_in) {
            if (sb) WDX_HIP_TRY(hipMemcpyAsync(B->in_adc.p, A.adc, sb, hipMemcpyHostToDevice, s));
        } else if (col1 > col0) {
            WDX_HIP_TRY(hipMemcpy2DAsync((int16_t *)B->in_adc.p + col0, (size_t)stride * sizeof(int16_t), A.adc + col0,
                                         (size_t)stride * sizeof(int16_t), (size_t)(col1 - col0) * sizeof(int16_t), (size_t)n,
                                         hipMemcpyHostToDevice, s));
        }
        rows.src = (const int16_t *)B->in_adc.p;
    }
    if ((rc = launch_adc_rows(rows, n, adc_dev != nullptr, s))) return rc;
    if (A.ok) WDX_HIP_TRY(hipMemcpyAsync(B->in3.p, A.ok, (size_t)n, hipMemcpyHostToDevice, s));
    *rd = FpReads{(const float *)B->in0.p, d_dst, d_out, 0, wb.max_len, n, d_as, d_ae, A.ok ? (const uint8_t *)B->in3.p : nullptr};
    return WDX_SUCCESS;
}

// wdx_fingerprint_batch / wdx_fingerprint_refine_batch: float32 rows of one stride through way (i) on the context's own
// stream, every fingerprint output back, one synchronisation.  (The batch call never takes the page-locked way in.)
static int fingerprint_batch_impl(wdx_ctx *ctx, const float *sig, int64_t n_reads, int64_t stride,
                                  const int32_t *a_start, const int32_t *a_end, const uint8_t *ok,
                                  const wdx_seg_params *p_in, const wdx_refine_params *rp, double *fpt, int64_t *dwell,
                                  double *stats, int32_t *refine_idx, int32_t *status) {
    WDX_ENTER(ctx);
    if ((rp && !refine_idx) || n_reads < 0 || stride < 0 ||
        (n_reads > 0 && (!sig || !a_start || !a_end || !fpt || !dwell || !stats || !status))) {
        set_error("fingerprint_batch: bad arguments");
        return WDX_ERR_INVALID;
    }
    wdx_seg_params pv;   // (an empty batch succeeds whatever the query's length, as it always has)
    if ((rc = refine_seg_params("fingerprint_batch", p_in, rp, &pv, n_reads > 0 ? kRefineQuery : 0u))) return rc;
    if (n_reads == 0) return WDX_SUCCESS;
    std::lock_guard<std::mutex> g(ctx->mu);
    hipStream_t s = ctx->stream;
    if ((rc = use_stream(ctx, s))) return rc;
    const int64_t K = pv.barcode_num_events;
    if (K < 1) {
        set_error("barcode_num_events must be >= 1");
        return WDX_ERR_INVALID;
    }
    WindowBatch wb(stride);
    const WindowOpts exact{pv.padding, 1, 0};
    for (int64_t r = 0; r < n_reads; ++r) wb.add(adapter_window(a_start[r], a_end[r], stride, ok && !ok[r], exact));
    const size_t sb = (size_t)(n_reads * stride) * sizeof(float);
    if ((rc = ctx->in0.ensure(sb ? sb : 4))) return rc;
    if ((rc = ctx->in1.ensure((size_t)n_reads * 4))) return rc;
    if ((rc = ctx->in2.ensure((size_t)n_reads * 4))) return rc;
    if ((rc = ctx->in3.ensure((size_t)n_reads))) return rc;
    if ((rc = ctx->out0.ensure((size_t)(n_reads * K) * 8))) return rc;
    if ((rc = ctx->out1.ensure((size_t)(n_reads * K) * 8))) return rc;
    if ((rc = ctx->out2.ensure((size_t)n_reads * 6 * 8))) return rc;
    if ((rc = ctx->out3.ensure((size_t)n_reads * 4))) return rc;
    if ((rc = ctx->fp_ws.ensure((size_t)fingerprint_workspace_bytes(n_reads)))) return rc;
    if (rp && (rc = ctx->mb_ridx.ensure((size_t)n_reads * 12))) return rc;
    StreamDrain drain(s);
    const wdx_minibatch_in in{sig, n_reads, stride, nullptr, nullptr, a_start, a_end, ok};
    FpReads rd;
    if ((rc = fingerprint_float_columns(ctx, in, wb, &rd))) return rc;
    const ChainOut out{FpOut{(double *)ctx->out0.p, (int64_t *)ctx->out1.p, (double *)ctx->out2.p, (int32_t *)ctx->out3.p}};
    int32_t *d_ridx = (int32_t *)ctx->mb_ridx.p;
    if ((rc = demux_chain(ctx, DtwRefs{}, rd, pv, rp, d_ridx, nullptr, ctx->fp_ws.p, false, ChainTail{}, out, s))) return rc;
    WDX_HIP_TRY(hipMemcpyAsync(fpt, ctx->out0.p, (size_t)(n_reads * K) * 8, hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipMemcpyAsync(dwell, ctx->out1.p, (size_t)(n_reads * K) * 8, hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipMemcpyAsync(stats, ctx->out2.p, (size_t)n_reads * 48, hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipMemcpyAsync(status, ctx->out3.p, (size_t)n_reads * 4, hipMemcpyDeviceToHost, s));
    if (rp) WDX_HIP_TRY(hipMemcpyAsync(refine_idx, ctx->mb_ridx.p, (size_t)n_reads * 12, hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipStreamSynchronize(s));
    drain.done();
    return WDX_SUCCESS;
}

int wdx_fingerprint_batch(wdx_ctx *ctx, const float *sig, int64_t n_reads, int64_t stride,
                          const int32_t *a_start, const int32_t *a_end, const uint8_t *ok,
                          const wdx_seg_params *p, double *fpt, int64_t *dwell, double *stats,
                          int32_t *status) {
    return fingerprint_batch_impl(ctx, sig, n_reads, stride, a_start, a_end, ok, p, nullptr, fpt, dwell, stats, nullptr,
                                  status);
}

int wdx_fingerprint_refine_batch(wdx_ctx *ctx, const float *sig, int64_t n_reads, int64_t stride,
                                 const int32_t *a_start, const int32_t *a_end, const uint8_t *ok,
                                 const wdx_seg_params *p, const wdx_refine_params *rp, double *fpt, int64_t *dwell,
                                 double *stats, int32_t *refine_idx, int32_t *status) {
    if (!rp) {
        set_error("fingerprint_refine_batch: null refinement parameters");
        return WDX_ERR_INVALID;
    }
    return fingerprint_batch_impl(ctx, sig, n_reads, stride, a_start, a_end, ok, p, rp, fpt, dwell, stats, refine_idx,
                                  status);
}

// One minibatch as demux_batch_enqueue takes it: float32 rows or int16 ADC rows (exactly one is set).
struct MbIn {
    const wdx_minibatch_in *f = nullptr;
    const wdx_minibatch_adc_in *adc = nullptr;
    int64_t n_reads() const { return adc ? adc->n_reads : f->n_reads; }
};
// The refinement branch of one minibatch: p->barcode_num_events is rp->barcode_keep_events already; h_idx = the host
// destination of refine_idx (null: not wanted)
struct MbRefine {
    const wdx_refine_params *rp = nullptr;
    int32_t *h_idx = nullptr;
};

// Body of the fused host-buffer call.  `B` owns the stream and every workspace that is touched (the context itself
// for wdx_demux_batch; one of its pipeline slots for wdx_demux_submit[_ex]), `R` is the resident reference set
// (read-only device memory of the parent context), `svm` the parent's resident model when the SVM tail is asked for.
// Everything is ENQUEUED on B->stream -- copies in, the kernel chain, copies out to the host destinations (caller arrays
// or the slot's page-locked block); the caller synchronises.
static int demux_batch_enqueue(wdx_ctx *B, const DtwRefs &R, const MbIn &in, const wdx_seg_params *p,
                               const MbHostOut &H, const ChainTail &tail = ChainTail{}, const MbRefine *rfn = nullptr) {
    int rc = WDX_SUCCESS;
    hipStream_t s = B->stream;
    const int64_t n_reads = in.n_reads();
    const int64_t K = p->barcode_num_events;
    const size_t db = (size_t)(n_reads * (R.nY > 0 ? R.nY : 1)) * sizeof(float);
    if ((rc = B->out0.ensure((size_t)(n_reads * K) * 8))) return rc;
    if ((rc = B->out1.ensure(db))) return rc;
    if ((rc = B->out2.ensure((size_t)n_reads * 4))) return rc;
    if ((rc = B->out3.ensure((size_t)n_reads * 4))) return rc;
    if (H.dwell && (rc = B->mb_dwell.ensure((size_t)(n_reads * K) * 8))) return rc;
    if (H.stats && (rc = B->mb_stats.ensure((size_t)n_reads * 48))) return rc;
    const size_t pb = (size_t)n_reads * (tail.svm ? tail.svm->k : tail.boost ? tail.boost->k : 0) * 8;   // (never both)
    if (pb) {
        if ((rc = B->mb_prob.ensure(pb))) return rc;
        if ((rc = B->mb_pred.ensure((size_t)n_reads * 4))) return rc;
        if ((rc = B->mb_conf.ensure((size_t)n_reads * 8))) return rc;
    }
    if ((rc = B->fp_ws.ensure((size_t)fingerprint_workspace_bytes(n_reads)))) return rc;
    int64_t *d_dwell = H.dwell ? (int64_t *)B->mb_dwell.p : nullptr;
    double *d_stats = H.stats ? (double *)B->mb_stats.p : nullptr;
    if (rfn && (rc = B->mb_ridx.ensure((size_t)n_reads * 12))) return rc;
    FpReads rd;
    if ((rc = in.adc ? fingerprint_adc_rows(B, *in.adc, p, &rd) : fingerprint_float_rows(B, *in.f, p, &rd))) return rc;
    ChainOut out{FpOut{(double *)B->out0.p, d_dwell, d_stats, (int32_t *)B->out3.p}};
    out.dist = (float *)B->out1.p, out.call = (int32_t *)B->out2.p;
    out.prob = (double *)B->mb_prob.p, out.pred = (int32_t *)B->mb_pred.p, out.conf = (double *)B->mb_conf.p;
    const wdx_refine_params *rp = rfn ? rfn->rp : nullptr;
    if ((rc = demux_chain(B, R, rd, *p, rp, (int32_t *)B->mb_ridx.p, nullptr, B->fp_ws.p, !rp, tail, out, s))) return rc;
    if (R.nY > 0) {
        if (H.call) WDX_HIP_TRY(hipMemcpyAsync(H.call, B->out2.p, (size_t)n_reads * 4, hipMemcpyDeviceToHost, s));
        if (H.dist) WDX_HIP_TRY(hipMemcpyAsync(H.dist, B->out1.p, db, hipMemcpyDeviceToHost, s));
    }
    if (pb && (tail.boost || R.nY > 0)) {
        if (H.prob) WDX_HIP_TRY(hipMemcpyAsync(H.prob, B->mb_prob.p, pb, hipMemcpyDeviceToHost, s));
        if (H.pred) WDX_HIP_TRY(hipMemcpyAsync(H.pred, B->mb_pred.p, (size_t)n_reads * 4, hipMemcpyDeviceToHost, s));
        if (H.conf) WDX_HIP_TRY(hipMemcpyAsync(H.conf, B->mb_conf.p, (size_t)n_reads * 8, hipMemcpyDeviceToHost, s));
    }
    WDX_HIP_TRY(hipMemcpyAsync(H.status, B->out3.p, (size_t)n_reads * 4, hipMemcpyDeviceToHost, s));
    if (H.fpt) WDX_HIP_TRY(hipMemcpyAsync(H.fpt, B->out0.p, (size_t)(n_reads * K) * 8, hipMemcpyDeviceToHost, s));
    if (H.dwell) WDX_HIP_TRY(hipMemcpyAsync(H.dwell, d_dwell, (size_t)(n_reads * K) * 8, hipMemcpyDeviceToHost, s));
    if (H.stats) WDX_HIP_TRY(hipMemcpyAsync(H.stats, d_stats, (size_t)n_reads * 48, hipMemcpyDeviceToHost, s));
    if (rfn && rfn->h_idx) WDX_HIP_TRY(hipMemcpyAsync(rfn->h_idx, B->mb_ridx.p, (size_t)n_reads * 12, hipMemcpyDeviceToHost, s));
    return WDX_SUCCESS;
}

// need_refs = false: a fingerprint-only refine minibatch (n_refs == 0), which reads no reference set
static int demux_check_args(wdx_ctx *ctx, const char *who, int64_t n_reads, int64_t stride, const void *sig,
                            const int32_t *a_start, const int32_t *a_end, const wdx_seg_params *p, int64_t n_refs,
                            bool need_refs = true) {
    if (n_reads < 0 || stride < 0 || !p || (n_reads > 0 && (!sig || !a_start || !a_end))) {
        set_error("%s: bad arguments", who);
        return WDX_ERR_INVALID;
    }
    if (!need_refs) return WDX_SUCCESS;
    DtwRefs &R = ctx->refs;
    if (R.window == 0) {
        set_error("no reference set: call wdx_set_refs first");
        return WDX_ERR_NO_REFS;
    }
    if (int rc = check_ref_length(R, *p)) return rc;
    if (n_refs != R.nY) {
        set_error("%s: the caller sized `dist` for %lld references but %lld are resident", who, (long long)n_refs,
                  (long long)R.nY);
        return WDX_ERR_INVALID;
    }
    return WDX_SUCCESS;
}

// wdx_demux_batch / wdx_demux_batch_adc: one minibatch on the context's own stream, one synchronisation
static int demux_batch_blocking(wdx_ctx *ctx, const char *who, const MbIn &in, const void *rows, int64_t stride,
                                const int32_t *a_start, const int32_t *a_end, const wdx_seg_params *p, int64_t n_refs,
                                double *fpt, float *dist, int32_t *call, int32_t *status) {
    WDX_ENTER(ctx);
    const int64_t n_reads = in.n_reads();
    if (n_reads > 0 && (!call || !status)) {
        set_error("%s: bad arguments", who);
        return WDX_ERR_INVALID;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    if ((rc = demux_check_args(ctx, who, n_reads, stride, rows, a_start, a_end, p, n_refs))) return rc;
    if (n_reads == 0) return WDX_SUCCESS;
    hipStream_t s = ctx->stream;
    if ((rc = use_stream(ctx, s))) return rc;
    StreamDrain drain(s);
    MbHostOut H;
    H.status = status;
    H.call = call;
    H.dist = dist;
    H.fpt = fpt;
    if ((rc = demux_batch_enqueue(ctx, ctx->refs, in, p, H))) return rc;
    WDX_HIP_TRY(hipStreamSynchronize(s));
    drain.done();
    if (ctx->refs.nY == 0)
        for (int64_t r = 0; r < n_reads; ++r) call[r] = -1;
    return WDX_SUCCESS;
}

int wdx_demux_batch(wdx_ctx *ctx, const float *sig, int64_t n_reads, int64_t stride,
                    const int32_t *a_start, const int32_t *a_end, const uint8_t *ok,
                    const wdx_seg_params *p, int64_t n_refs, double *fpt, float *dist, int32_t *call,
                    int32_t *status) {
    const wdx_minibatch_in in{sig, n_reads, stride, nullptr, nullptr, a_start, a_end, ok};
    MbIn mb;
    mb.f = &in;
    return demux_batch_blocking(ctx, "demux_batch", mb, sig, stride, a_start, a_end, p, n_refs, fpt, dist, call, status);
}

int wdx_demux_batch_adc(wdx_ctx *ctx, const wdx_minibatch_adc_in *in, const wdx_seg_params *p, int64_t n_refs, double *fpt,
                        float *dist, int32_t *call, int32_t *status) {
    if (int e = adc_check_args("demux_batch_adc", in)) return e;
    MbIn mb;
    mb.adc = in;
    return demux_batch_blocking(ctx, "demux_batch_adc", mb, in->adc, in->row_off ? 0 : in->stride, in->a_start, in->a_end, p,
                                n_refs, fpt, dist, call, status);
}

// wdx_fingerprint_batch for int16 rows: the minibatch path above with no reference set (nothing behind the fingerprint
// stage runs), so that the int16 rows have ONE way in
int wdx_fingerprint_batch_adc(wdx_ctx *ctx, const wdx_minibatch_adc_in *in, const wdx_seg_params *p, double *fpt,
                              int64_t *dwell, double *stats, int32_t *status) {
    if (int e = adc_check_args("fingerprint_batch_adc", in)) return e;
    WDX_ENTER(ctx);
    const int64_t n_reads = in->n_reads;
    if (!p || (n_reads > 0 && (!fpt || !dwell || !stats || !status))) {
        set_error("fingerprint_batch_adc: bad arguments");
        return WDX_ERR_INVALID;
    }
    if (p->barcode_num_events < 1) {
        set_error("barcode_num_events must be >= 1");
        return WDX_ERR_INVALID;
    }
    if (n_reads == 0) return WDX_SUCCESS;
    std::lock_guard<std::mutex> g(ctx->mu);
    hipStream_t s = ctx->stream;
    if ((rc = use_stream(ctx, s))) return rc;
    StreamDrain drain(s);
    MbIn mb;
    mb.adc = in;
    MbHostOut H;
    H.status = status;
    H.fpt = fpt;
    H.dwell = dwell;
    H.stats = stats;
    if ((rc = demux_batch_enqueue(ctx, DtwRefs{}, mb, p, H))) return rc;
    WDX_HIP_TRY(hipStreamSynchronize(s));
    drain.done();
    return WDX_SUCCESS;
}

// ---- pipelined minibatches: two slots per context, submit / wait -------------------------------------------------
// The reference's workers (file_proc.py:380-454, 1197-1243) alternate "fill the next minibatch" with "process this
// one".  A slot is a child context (its own non-blocking stream and workspaces) that shares the parent's resident
// reference set: minibatch k+1's host->device copy runs while minibatch k's kernels and device->host copy are still
// in flight, and the caller's thread is free to fill the next buffer in between.
static int slot_get(wdx_ctx *ctx, int32_t slot, wdx_ctx **out) {
    if (slot < 0 || slot >= WDX_MAX_SLOTS) {
        set_error("slot must be in [0, %d)", WDX_MAX_SLOTS);
        return WDX_ERR_INVALID;
    }
    if (!ctx->slots[slot]) {
        wdx_ctx *c = nullptr;
        if (int rc = wdx_ctx_create(ctx->device, &c)) return rc;
        ctx->slots[slot] = c;
    }
    *out = ctx->slots[slot];
    return WDX_SUCCESS;
}

// wdx_demux_submit_ex / wdx_demux_submit_adc behind their own argument checks (the context's mutex is held)
// rp: the refinement branch (p->barcode_num_events = rp->barcode_keep_events already); no_refs: fingerprint only
static int demux_submit_locked(wdx_ctx *ctx, int32_t slot, const MbIn &in, const wdx_seg_params *p, uint32_t want,
                               const wdx_refine_params *rp = nullptr, bool no_refs = false);

// wdx_demux_submit_ex / _adc with n_refs == 0: legal when, and only when, WDX_WANT_BOOST is set (the boost tail reads the
// fingerprints, not a reference set); there are no distances then
static bool boost_without_refs(int64_t n_refs, uint32_t want) { return n_refs == 0 && (want & WDX_WANT_BOOST) != 0; }
static int boost_without_refs_check(const char *who, uint32_t want) {
    if (want & WDX_WANT_DIST) {
        set_error("%s: a minibatch without references (n_refs = 0) has no distances", who);
        return WDX_ERR_INVALID;
    }
    return WDX_SUCCESS;
}

// packed float32 rows: offsets ascending on 16-byte boundaries, every row inside its slice
static int packed_rows_check(const wdx_minibatch_in *in) {
    const int64_t n_reads = in->n_reads;
    if (n_reads > 0 && !in->row_len) {
        set_error("demux_submit: packed rows need row_len");
        return WDX_ERR_INVALID;
    }
    for (int64_t r = 0; r < n_reads; ++r) {
        const int64_t o0 = in->row_off[r], o1 = in->row_off[r + 1];
        if (o0 < 0 || (o0 & 3) || o1 < o0 || in->row_len[r] < 0 || (int64_t)in->row_len[r] > o1 - o0) {
            set_error("demux_submit: packed row %lld: offsets must ascend in multiples of 4 and hold row_len samples", (long long)r);
            return WDX_ERR_INVALID;
        }
    }
    return WDX_SUCCESS;
}

int wdx_demux_submit_ex(wdx_ctx *ctx, int32_t slot, const wdx_minibatch_in *in, const wdx_seg_params *p, int64_t n_refs,
                        uint32_t want) {
    WDX_ENTER(ctx);
    if (!in) {
        set_error("demux_submit: null minibatch");
        return WDX_ERR_INVALID;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    const int64_t n_reads = in->n_reads;
    const bool no_refs = boost_without_refs(n_refs, want);
    if (no_refs && (rc = boost_without_refs_check("demux_submit", want))) return rc;
    if ((rc = demux_check_args(ctx, "demux_submit", n_reads, in->row_off ? 0 : in->stride, in->sig, in->a_start, in->a_end, p,
                               n_refs, !no_refs)))
        return rc;
    if (in->row_off && (rc = packed_rows_check(in))) return rc;
    MbIn mb;
    mb.f = in;
    return demux_submit_locked(ctx, slot, mb, p, want, nullptr, no_refs);
}

int wdx_demux_submit_refine(wdx_ctx *ctx, int32_t slot, const wdx_minibatch_in *in, const wdx_minibatch_adc_in *in_adc,
                            const wdx_seg_params *p, const wdx_refine_params *rp, int64_t n_refs, uint32_t want) {
    if ((in != nullptr) == (in_adc != nullptr)) {
        set_error("demux_submit_refine: exactly one of in / in_adc must be given");
        return WDX_ERR_INVALID;
    }
    if (in_adc)
        if (int e = adc_check_args("demux_submit_refine", in_adc)) return e;
    WDX_ENTER(ctx);
    if (!rp || n_refs < 0) {
        set_error("demux_submit_refine: bad arguments");
        return WDX_ERR_INVALID;
    }
    wdx_seg_params pv;   // K of the outputs and of the DTW
    if ((rc = refine_seg_params("demux_submit_refine", p, rp, &pv, kRefineQuery | kRefineKeep))) return rc;
    if (n_refs == 0 && (want & (WDX_WANT_DIST | WDX_WANT_SVM))) {
        set_error("demux_submit_refine: a fingerprint-only minibatch (n_refs = 0) has no distances and no SVM tail");
        return WDX_ERR_INVALID;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    MbIn mb;
    mb.f = in;
    mb.adc = in_adc;
    const bool packed = in ? in->row_off != nullptr : in_adc->row_off != nullptr;
    if ((rc = demux_check_args(ctx, "demux_submit_refine", mb.n_reads(), packed ? 0 : (in ? in->stride : in_adc->stride),
                               in ? (const void *)in->sig : (const void *)in_adc->adc, in ? in->a_start : in_adc->a_start,
                               in ? in->a_end : in_adc->a_end, &pv, n_refs, n_refs > 0)))
        return rc;
    if (in && in->row_off && (rc = packed_rows_check(in))) return rc;
    return demux_submit_locked(ctx, slot, mb, &pv, want, rp, n_refs == 0);
}

int wdx_demux_submit_adc(wdx_ctx *ctx, int32_t slot, const wdx_minibatch_adc_in *in, const wdx_seg_params *p, int64_t n_refs,
                         uint32_t want) {
    if (int e = adc_check_args("demux_submit_adc", in)) return e;
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    const bool no_refs = boost_without_refs(n_refs, want);
    if (no_refs && (rc = boost_without_refs_check("demux_submit_adc", want))) return rc;
    if ((rc = demux_check_args(ctx, "demux_submit_adc", in->n_reads, in->row_off ? 0 : in->stride, in->adc, in->a_start,
                               in->a_end, p, n_refs, !no_refs)))
        return rc;
    MbIn mb;
    mb.adc = in;
    return demux_submit_locked(ctx, slot, mb, p, want, nullptr, no_refs);
}

static int demux_submit_locked(wdx_ctx *ctx, int32_t slot, const MbIn &in, const wdx_seg_params *p, uint32_t want,
                               const wdx_refine_params *rp, bool no_refs) {
    int rc = WDX_SUCCESS;
    const int64_t n_reads = in.n_reads();
    const bool want_svm = (want & WDX_WANT_SVM) != 0, want_boost = (want & WDX_WANT_BOOST) != 0;
    if (want_svm && want_boost) {
        set_error("demux_submit: WDX_WANT_SVM and WDX_WANT_BOOST share prob / pred / conf: ask for one of them");
        return WDX_ERR_INVALID;
    }
    const BoostDev boost = ctx->boost.dev;   // (by value: the kernel's arguments are this model, whatever is set later)
    ChainTail tail;
    tail.kind = want_svm ? WDX_LIVE_TAIL_SVM : want_boost ? WDX_LIVE_TAIL_BOOST : WDX_LIVE_TAIL_NONE;
    tail.svm = want_svm ? &ctx->svm.dev : nullptr;
    tail.boost = want_boost ? &boost : nullptr;
    if ((rc = tail_ready(ctx, tail.kind, ctx->refs.nY, p->barcode_num_events, rp != nullptr, "demux_submit"))) return rc;
    wdx_ctx *S = nullptr;
    if ((rc = slot_get(ctx, slot, &S))) return rc;
    if (S->slot_busy) {
        set_error("demux_submit: slot %d still holds a minibatch (wdx_demux_wait it first)", (int)slot);
        return WDX_ERR_INVALID;
    }
    // the parent's own stream may still be building the reference set this slot is about to read
    if ((rc = use_stream(ctx, ctx->stream))) return rc;
    WDX_HIP_TRY(hipStreamSynchronize(ctx->stream));
    S->knobs = ctx->knobs;
    S->timing = ctx->timing;  // (timed like the parent's own launches; wdx_kernel_time sums the slots' events)
    const DtwRefs none{};
    const DtwRefs &R = no_refs ? none : ctx->refs;
    S->refs = R;  // device pointers of the parent's resident set (read-only; wdx_set_refs drains the slots)
    const int64_t K = p->barcode_num_events;
    const int64_t k = want_svm ? ctx->svm.dev.k : (want_boost ? ctx->boost.dev.k : 0);
    const bool want_tail = want_svm || want_boost;
    // page-locked output block of the slot, 8-byte aligned pieces:
    // [fpt f64 n*K][dwell i64 n*K][stats f64 n*6][prob f64 n*k][conf f64 n][dist f32 n*nY][call i32 n][status i32 n][pred i32 n]
    const size_t n = (size_t)n_reads;
    const size_t bytes[9] = {(want & WDX_WANT_FPT) ? n * K * 8 : 0,
                             (want & WDX_WANT_DWELL) ? n * K * 8 : 0,
                             (want & WDX_WANT_STATS) ? n * 48 : 0,
                             want_tail ? n * (size_t)k * 8 : 0,
                             want_tail ? n * 8 : 0,
                             ((want & WDX_WANT_DIST) && R.nY > 0) ? n * (size_t)R.nY * 4 : 0,
                             n * 4,
                             n * 4,
                             want_tail ? n * 4 : 0};
    size_t off = 0;
    for (int q = 0; q < 9; ++q) {
        S->slot_off[q] = off;
        off += (bytes[q] + 7) / 8 * 8;
    }
    S->slot_want_ridx = rp && (want & WDX_WANT_REFINE_IDX);
    S->slot_off_ridx = off;   // [refine_idx i32 n*3] behind the nine
    if (S->slot_want_ridx) off += (n * 12 + 7) / 8 * 8;
    if ((rc = S->pin_out.ensure(off + 8))) return rc;
    unsigned char *ho = (unsigned char *)S->pin_out.p;
    S->slot_n = n_reads;
    S->slot_K = K;
    S->slot_nY = R.nY;
    S->slot_k = k;
    S->slot_want = want & ~(bytes[5] ? 0u : WDX_WANT_DIST);
    if (n_reads == 0) {
        S->slot_busy = true;
        return WDX_SUCCESS;
    }
    MbHostOut H;
    H.fpt = bytes[0] ? (double *)(ho + S->slot_off[0]) : nullptr;
    H.dwell = bytes[1] ? (int64_t *)(ho + S->slot_off[1]) : nullptr;
    H.stats = bytes[2] ? (double *)(ho + S->slot_off[2]) : nullptr;
    H.prob = bytes[3] ? (double *)(ho + S->slot_off[3]) : nullptr;
    H.conf = bytes[4] ? (double *)(ho + S->slot_off[4]) : nullptr;
    H.dist = bytes[5] ? (float *)(ho + S->slot_off[5]) : nullptr;
    H.call = (int32_t *)(ho + S->slot_off[6]);
    H.status = (int32_t *)(ho + S->slot_off[7]);
    H.pred = bytes[8] ? (int32_t *)(ho + S->slot_off[8]) : nullptr;
    StreamDrain drain(S->stream);
    S->dtw_last.family = WDX_DTW_NONE;   // (a submit that dispatches no DTW leaves the parent's record as it was)
    MbRefine rfn;
    rfn.rp = rp;
    rfn.h_idx = S->slot_want_ridx ? (int32_t *)(ho + S->slot_off_ridx) : nullptr;
    if ((rc = demux_batch_enqueue(S, R, in, p, H, tail, rp ? &rfn : nullptr))) return rc;
    drain.done();  // in flight on purpose: wdx_demux_wait synchronises
    if (S->dtw_last.family != WDX_DTW_NONE) ctx->dtw_last = S->dtw_last;
    S->slot_busy = true;
    return WDX_SUCCESS;
}

int wdx_demux_submit(wdx_ctx *ctx, int32_t slot, const float *sig, int64_t n_reads, int64_t stride,
                     const int32_t *a_start, const int32_t *a_end, const uint8_t *ok, const wdx_seg_params *p,
                     int64_t n_refs, int32_t want_fpt, int32_t want_dist) {
    const wdx_minibatch_in in{sig, n_reads, stride, nullptr, nullptr, a_start, a_end, ok};
    return wdx_demux_submit_ex(ctx, slot, &in, p, n_refs, (want_fpt ? WDX_WANT_FPT : 0u) | (want_dist ? WDX_WANT_DIST : 0u));
}

// wdx_demux_wait_ex / wdx_demux_wait_refine: refine_idx must be given exactly when the slot asked for it
static int demux_wait_body(wdx_ctx *ctx, int32_t slot, const wdx_minibatch_out *out, int32_t *refine_idx) {
    WDX_ENTER(ctx);
    if (!out) {
        set_error("demux_wait: null output block");
        return WDX_ERR_INVALID;
    }
    wdx_ctx *S = nullptr;
    {
        std::lock_guard<std::mutex> g(ctx->mu);
        if (slot < 0 || slot >= WDX_MAX_SLOTS || !ctx->slots[slot] || !ctx->slots[slot]->slot_busy) {
            set_error("demux_wait: nothing was submitted on slot %d", (int)slot);
            return WDX_ERR_INVALID;
        }
        S = ctx->slots[slot];
        // argument errors are reported BEFORE the wait and leave the minibatch in the slot: the caller can wait again
        // with the right arguments; a second thread waiting on the same slot is refused
        if (S->slot_waiting) {
            set_error("demux_wait: another thread is waiting on slot %d", (int)slot);
            return WDX_ERR_INVALID;
        }
        if (S->slot_n > 0 && (!out->call || !out->status)) {
            set_error("demux_wait: call and status are required");
            return WDX_ERR_INVALID;
        }
        const uint32_t w = S->slot_want;
        if (S->slot_n > 0 && ((out->fpt && !(w & WDX_WANT_FPT)) || (out->dist && !(w & WDX_WANT_DIST) && S->slot_nY > 0) ||
                              (out->dwell && !(w & WDX_WANT_DWELL)) || (out->stats && !(w & WDX_WANT_STATS)) ||
                              ((out->prob || out->pred || out->conf) && !(w & (WDX_WANT_SVM | WDX_WANT_BOOST))))) {
            set_error("demux_wait: an output that was not requested at wdx_demux_submit");
            return WDX_ERR_INVALID;
        }
        if (S->slot_n > 0 && refine_idx && !S->slot_want_ridx) {
            set_error("demux_wait: refine_idx was not requested at wdx_demux_submit_refine");
            return WDX_ERR_INVALID;
        }
        if (S->slot_n > 0 && !refine_idx && S->slot_want_ridx) {
            set_error("demux_wait: the slot holds a refine_idx (WDX_WANT_REFINE_IDX): wdx_demux_wait_refine takes it");
            return WDX_ERR_INVALID;
        }
        S->slot_waiting = true;
    }
    // (the wait itself runs outside the parent's mutex: the other slots can be submitted meanwhile)
    hipError_t e = S->slot_n > 0 ? hipStreamSynchronize(S->stream) : hipSuccess;
    std::lock_guard<std::mutex> g(ctx->mu);
    S->slot_waiting = false;
    S->slot_busy = false;
    if (e != hipSuccess) {
        set_error("demux_wait: hipStreamSynchronize failed: %s", hipGetErrorString(e));
        return WDX_ERR_HIP;
    }
    const int64_t n = S->slot_n;
    if (n == 0) return WDX_SUCCESS;
    const unsigned char *ho = (const unsigned char *)S->pin_out.p;
    const size_t nn = (size_t)n;
    memcpy(out->status, ho + S->slot_off[7], nn * 4);
    if (S->slot_nY > 0) memcpy(out->call, ho + S->slot_off[6], nn * 4);
    else for (int64_t r = 0; r < n; ++r) out->call[r] = -1;
    if (out->fpt) memcpy(out->fpt, ho + S->slot_off[0], nn * S->slot_K * 8);
    if (out->dwell) memcpy(out->dwell, ho + S->slot_off[1], nn * S->slot_K * 8);
    if (out->stats) memcpy(out->stats, ho + S->slot_off[2], nn * 48);
    if (out->prob) memcpy(out->prob, ho + S->slot_off[3], nn * (size_t)S->slot_k * 8);
    if (out->conf) memcpy(out->conf, ho + S->slot_off[4], nn * 8);
    if (out->dist && S->slot_nY > 0) memcpy(out->dist, ho + S->slot_off[5], nn * S->slot_nY * 4);
    if (out->pred) memcpy(out->pred, ho + S->slot_off[8], nn * 4);
    if (refine_idx) memcpy(refine_idx, ho + S->slot_off_ridx, nn * 12);
    return WDX_SUCCESS;
}

int wdx_demux_wait_ex(wdx_ctx *ctx, int32_t slot, const wdx_minibatch_out *out) {
    return demux_wait_body(ctx, slot, out, nullptr);
}

int wdx_demux_wait_refine(wdx_ctx *ctx, int32_t slot, const wdx_minibatch_out *out, int32_t *refine_idx) {
    return demux_wait_body(ctx, slot, out, refine_idx);
}

int wdx_demux_wait(wdx_ctx *ctx, int32_t slot, double *fpt, float *dist, int32_t *call, int32_t *status) {
    wdx_minibatch_out out{};
    out.status = status;
    out.call = call;
    out.dist = dist;
    out.fpt = fpt;
    return wdx_demux_wait_ex(ctx, slot, &out);
}

}  // extern "C"
