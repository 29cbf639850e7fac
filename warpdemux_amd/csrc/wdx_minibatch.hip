// The host-minibatch path behind include/wdx.h: float32 or int16 rows in host memory -> staged on the device -> the fingerprint
// stage [-> DTW -> call -> classifier tail] -> results in host memory; the blocking entries (wdx_demux_batch*,
// wdx_fingerprint_batch*) and the pipelined ones (wdx_demux_submit* / wdx_demux_wait*).  Nothing here computes results.
#include "wdx_ctx.h"
#include "wdx_window.h"

#include <string.h>

#include <algorithm>

using namespace wdx;

extern "C" {

// Host destinations of one minibatch, piece by piece of its plan (wdx_stage_plan.h): the caller's arrays, or the pieces of a
// slot's page-locked block; null = the piece stays on the device
struct MbHost {
    void *to[P_COUNT];
};
static MbHost host_arrays(const wdx_minibatch_out &out) {
    MbHost H{};
    for (int q = 0; q < P_COUNT; ++q) H.to[q] = destination(q, out, nullptr, nullptr);
    return H;
}
static MbHost host_block(const OutPlan &pl, unsigned char *block) {
    MbHost H{};
    for (int q = 0; q < P_COUNT; ++q) H.to[q] = pl.travels[q] ? block + pl.off[q] : nullptr;
    return H;
}
// Which device buffer of `B` backs which piece of a minibatch (the MLP tail's count is the live tick's alone)
static Buffer *piece_buffer(wdx_ctx *B, int q) {
    Buffer *const of[P_COUNT] = {&B->out0, &B->mb_dwell, &B->mb_stats, &B->mb_prob, &B->mb_conf, nullptr,
                                 &B->out1, &B->mb_ridx, &B->out3,     &B->out2,    &B->mb_pred};
    return of[q];
}

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
        // the device image (kPackedRowsImage), column by column straight from the caller's arrays
        const ImageLayout L = image_layout(kPackedRowsImage, (size_t)n_reads);
        if ((rc = B->pk_idx.ensure(L.bytes))) return rc;
        int64_t *d_off = image_col<int64_t>(B->pk_idx.p, L, PK_OFF);
        int32_t *d_len = image_col<int32_t>(B->pk_idx.p, L, PK_LEN), *d_as = image_col<int32_t>(B->pk_idx.p, L, PK_A_START),
                *d_ae = image_col<int32_t>(B->pk_idx.p, L, PK_A_END);
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
    // the bus-pack image (kBusPackImage; page-locked, owned by the slot until its copy has run) and its device copy
    const ImageLayout L = image_layout(kBusPackImage, (size_t)n_reads);
    if ((rc = B->pk_host.ensure(L.bytes))) return rc;
    if ((rc = B->pk_idx.ensure(L.bytes))) return rc;
    const int64_t packed = fill_bus_pack_image((unsigned char *)B->pk_host.p, L, n_reads, stride, a_start, a_end, ok, p->padding);
    if ((rc = B->in0.ensure((size_t)(packed ? packed : 1) * sizeof(float)))) return rc;
    WDX_HIP_TRY(hipMemcpyAsync(B->pk_idx.p, B->pk_host.p, L.bytes, hipMemcpyHostToDevice, s));
    const int64_t *d_off = image_col<int64_t>(B->pk_idx.p, L, BP_OFF);
    const int32_t *d_len = image_col<int32_t>(B->pk_idx.p, L, BP_LEN), *d_as = image_col<int32_t>(B->pk_idx.p, L, BP_A_START),
                  *d_ae = image_col<int32_t>(B->pk_idx.p, L, BP_A_END);
    if ((rc = launch_pack_windows(sig_dev, stride, n_reads, d_off, image_col<int32_t>(B->pk_idx.p, L, BP_FIRST), d_len,
                                  (float *)B->in0.p, s)))
        return rc;
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
    // the int16 image (kAdcImage; page-locked, owned by the slot until its copy has run) and its device copy
    const ImageLayout L = image_layout(kAdcImage, (size_t)n);
    if ((rc = B->pk_host.ensure(L.bytes))) return rc;
    if ((rc = B->pk_idx.ensure(L.bytes))) return rc;
    if ((rc = B->in3.ensure((size_t)n))) return rc;
    const AdcImage H(B->pk_host.p, L), D(B->pk_idx.p, L);
    WindowBatch wb(stride);
    PackedOffset pos(kDecodedRowRound);
    const WindowOpts exact{p->padding, 1, 0}, groups{p->padding, 8, 0};
    for (int64_t r = 0; r < n; ++r) {
        const bool dead = A.ok && !A.ok[r];
        Window w;
        int64_t src;
        if (packed_in) {
            // the caller's row as it stands; its window only bounds max_len
            w.row = A.row_win ? (int64_t)A.row_win[r] : (int64_t)A.row_len[r];
            w.valid = std::min<int64_t>(A.row_len[r], w.row);
            w.a_start = A.a_start[r];
            w.a_end = A.a_end[r];
            wb.max_len = std::max(wb.max_len, adapter_window(w.a_start, w.a_end, w.row, dead, exact).win);
            src = A.row_off[r];
        } else {
            w = adapter_window(A.a_start[r], A.a_end[r], stride, dead, groups, A.row_len[r]);
            wb.add(w);
            src = r * stride + w.first;
        }
        adc_image_row(H, r, w, src, pos, A.offset[r], A.scale[r]);
    }
    H.dst[n] = pos.next;
    const int64_t col0 = wb.col0, col1 = wb.col1;
    if ((rc = B->in0.ensure((size_t)(pos.next ? pos.next : 1) * sizeof(float)))) return rc;
    WDX_HIP_TRY(hipMemcpyAsync(B->pk_idx.p, B->pk_host.p, L.bytes, hipMemcpyHostToDevice, s));
    AdcRows rows{nullptr, D.src, 0, D.valid, D.offset, D.scale, (float *)B->in0.p, D.dst, 0, D.out};
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
    *rd = FpReads{(const float *)B->in0.p, D.dst, D.out, 0, wb.max_len, n, D.a_start, D.a_end, A.ok ? (const uint8_t *)B->in3.p : nullptr};
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
    // every fingerprint output, each in a buffer of its own: fpt out0, dwell out1, stats out2, status out3, refine_idx mb_ridx
    const OutPlan pl = out_plan(n_reads, K, 0, 0, WDX_WANT_FPT | WDX_WANT_DWELL | WDX_WANT_STATS | WDX_WANT_REFINE_IDX,
                                WDX_LIVE_TAIL_NONE, rp != nullptr, 0);
    if ((rc = ctx->out0.ensure(pl.bytes[P_FPT]))) return rc;
    if ((rc = ctx->out1.ensure(pl.bytes[P_DWELL]))) return rc;
    if ((rc = ctx->out2.ensure(pl.bytes[P_STATS]))) return rc;
    if ((rc = ctx->out3.ensure(pl.bytes[P_STATUS]))) return rc;
    if ((rc = ctx->fp_ws.ensure((size_t)fingerprint_workspace_bytes(n_reads)))) return rc;
    if (rp && (rc = ctx->mb_ridx.ensure(pl.bytes[P_RIDX]))) return rc;
    StreamDrain drain(s);
    const wdx_minibatch_in in{sig, n_reads, stride, nullptr, nullptr, a_start, a_end, ok};
    FpReads rd;
    if ((rc = fingerprint_float_columns(ctx, in, wb, &rd))) return rc;
    const ChainOut out{FpOut{(double *)ctx->out0.p, (int64_t *)ctx->out1.p, (double *)ctx->out2.p, (int32_t *)ctx->out3.p}};
    int32_t *d_ridx = (int32_t *)ctx->mb_ridx.p;
    if ((rc = demux_chain(ctx, DtwRefs{}, rd, pv, rp, d_ridx, nullptr, ctx->fp_ws.p, false, ChainTail{}, out, s))) return rc;
    WDX_HIP_TRY(hipMemcpyAsync(fpt, ctx->out0.p, pl.bytes[P_FPT], hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipMemcpyAsync(dwell, ctx->out1.p, pl.bytes[P_DWELL], hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipMemcpyAsync(stats, ctx->out2.p, pl.bytes[P_STATS], hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipMemcpyAsync(status, ctx->out3.p, pl.bytes[P_STATUS], hipMemcpyDeviceToHost, s));
    if (rp) WDX_HIP_TRY(hipMemcpyAsync(refine_idx, ctx->mb_ridx.p, pl.bytes[P_RIDX], hipMemcpyDeviceToHost, s));
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
// Body of the fused host-buffer call.  `B` owns the stream and every workspace that is touched (the context itself
// for wdx_demux_batch; one of its pipeline slots for wdx_demux_submit[_ex]), `R` is the resident reference set
// (read-only device memory of the parent context), `tail` names the parent's resident model when a tail is asked for, `pl` is
// the plan of what comes back (for n_reads, p->barcode_num_events, R.nY and the tail) and `H` where its pieces go.  rp: the
// refinement branch (p->barcode_num_events is rp->barcode_keep_events already).
// Everything is ENQUEUED on B->stream -- copies in, the kernel chain, one copy out per travelling piece to its host
// destination (caller arrays or the slot's page-locked block); the caller synchronises.
static int demux_batch_enqueue(wdx_ctx *B, const DtwRefs &R, const MbIn &in, const wdx_seg_params *p, const OutPlan &pl,
                               const MbHost &H, const ChainTail &tail = ChainTail{}, const wdx_refine_params *rp = nullptr) {
    int rc = WDX_SUCCESS;
    hipStream_t s = B->stream;
    // (a refine minibatch records refine_idx on the device whether or not it travels: kept as found)
    for (int q = 0; q < P_COUNT; ++q)
        if ((pl.exists[q] || (q == P_RIDX && rp)) && (rc = piece_buffer(B, q)->ensure(pl.bytes[q]))) return rc;
    if ((rc = B->fp_ws.ensure((size_t)fingerprint_workspace_bytes(pl.n)))) return rc;
    auto dev = [&](OutPiece q) { return pl.exists[q] ? piece_buffer(B, q)->p : nullptr; };
    FpReads rd;
    if ((rc = in.adc ? fingerprint_adc_rows(B, *in.adc, p, &rd) : fingerprint_float_rows(B, *in.f, p, &rd))) return rc;
    ChainOut out{FpOut{(double *)dev(P_FPT), (int64_t *)dev(P_DWELL), (double *)dev(P_STATS), (int32_t *)dev(P_STATUS)}};
    out.dist = (float *)dev(P_DIST), out.call = (int32_t *)dev(P_CALL);
    out.prob = (double *)dev(P_PROB), out.pred = (int32_t *)dev(P_PRED), out.conf = (double *)dev(P_CONF);
    if ((rc = demux_chain(B, R, rd, *p, rp, (int32_t *)B->mb_ridx.p, nullptr, B->fp_ws.p, !rp, tail, out, s))) return rc;
    // (the small pieces first, the order these copies have always been enqueued in)
    constexpr OutPiece kCopyOrder[] = {P_CALL, P_DIST, P_PROB, P_PRED, P_CONF, P_STATUS, P_FPT, P_DWELL, P_STATS, P_RIDX};
    for (OutPiece q : kCopyOrder)
        if (pl.travels[q] && H.to[q])
            WDX_HIP_TRY(hipMemcpyAsync(H.to[q], piece_buffer(B, q)->p, pl.bytes[q], hipMemcpyDeviceToHost, s));
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
    wdx_minibatch_out out{};   // (an output is wanted when its array is given)
    out.status = status, out.call = call, out.dist = dist, out.fpt = fpt;
    const OutPlan pl = out_plan(n_reads, p->barcode_num_events, ctx->refs.nY, 0, (fpt ? WDX_WANT_FPT : 0u) | (dist ? WDX_WANT_DIST : 0u),
                                WDX_LIVE_TAIL_NONE, false, kHaveCall);
    if ((rc = demux_batch_enqueue(ctx, ctx->refs, in, p, pl, host_arrays(out)))) return rc;
    WDX_HIP_TRY(hipStreamSynchronize(s));
    drain.done();
    fill_no_call(pl, call);
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
    wdx_minibatch_out out{};
    out.status = status, out.fpt = fpt, out.dwell = dwell, out.stats = stats;
    const OutPlan pl = out_plan(n_reads, p->barcode_num_events, 0, 0, WDX_WANT_FPT | WDX_WANT_DWELL | WDX_WANT_STATS,
                                WDX_LIVE_TAIL_NONE, false, 0);
    if ((rc = demux_batch_enqueue(ctx, DtwRefs{}, mb, p, pl, host_arrays(out)))) return rc;
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
    const int64_t k = want_svm ? ctx->svm.dev.k : (want_boost ? ctx->boost.dev.k : 0);
    // the slot's page-locked block holds every piece that travels (wdx_stage_plan.h); wdx_demux_wait delivers from it by the
    // plan kept here
    const OutPlan pl = out_plan(n_reads, p->barcode_num_events, R.nY, k, want, tail.kind, rp != nullptr, kHaveAll);
    if ((rc = S->pin_out.ensure(pl.copy_bytes + 8))) return rc;
    S->slot_plan = pl;
    S->slot_want = want;
    if (n_reads == 0) {
        S->slot_busy = true;
        return WDX_SUCCESS;
    }
    StreamDrain drain(S->stream);
    S->dtw_last.family = WDX_DTW_NONE;   // (a submit that dispatches no DTW leaves the parent's record as it was)
    if ((rc = demux_batch_enqueue(S, R, in, p, pl, host_block(pl, (unsigned char *)S->pin_out.p), tail, rp))) return rc;
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
        const OutPlan &pl = S->slot_plan;
        if (pl.n > 0 && (!out->call || !out->status)) {
            set_error("demux_wait: call and status are required");
            return WDX_ERR_INVALID;
        }
        const uint32_t w = S->slot_want;
        if (pl.n > 0 && ((out->fpt && !(w & WDX_WANT_FPT)) || (out->dist && !(w & WDX_WANT_DIST) && pl.nY > 0) ||
                         (out->dwell && !(w & WDX_WANT_DWELL)) || (out->stats && !(w & WDX_WANT_STATS)) ||
                         ((out->prob || out->pred || out->conf) && !(w & (WDX_WANT_SVM | WDX_WANT_BOOST))))) {
            set_error("demux_wait: an output that was not requested at wdx_demux_submit");
            return WDX_ERR_INVALID;
        }
        if (pl.n > 0 && refine_idx && !pl.travels[P_RIDX]) {
            set_error("demux_wait: refine_idx was not requested at wdx_demux_submit_refine");
            return WDX_ERR_INVALID;
        }
        if (pl.n > 0 && !refine_idx && pl.travels[P_RIDX]) {
            set_error("demux_wait: the slot holds a refine_idx (WDX_WANT_REFINE_IDX): wdx_demux_wait_refine takes it");
            return WDX_ERR_INVALID;
        }
        S->slot_waiting = true;
    }
    // (the wait itself runs outside the parent's mutex: the other slots can be submitted meanwhile)
    hipError_t e = S->slot_plan.n > 0 ? hipStreamSynchronize(S->stream) : hipSuccess;
    std::lock_guard<std::mutex> g(ctx->mu);
    S->slot_waiting = false;
    S->slot_busy = false;
    if (e != hipSuccess) {
        set_error("demux_wait: hipStreamSynchronize failed: %s", hipGetErrorString(e));
        return WDX_ERR_HIP;
    }
    // the pieces the caller gave an array for (every one of them was asked for: the refusals above); an empty minibatch
    // writes nothing
    if (S->slot_plan.n > 0) deliver(S->slot_plan, (const unsigned char *)S->pin_out.p, *out, refine_idx, nullptr);
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
