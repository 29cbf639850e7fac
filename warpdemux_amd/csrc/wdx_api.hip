// C ABI of libwdx_hip.so (include/wdx.h): context, buffers, timing, the reference set, the DTW route, the device-resident entries,
// host allocation, the self-test hooks (host minibatches: wdx_minibatch.hip).  Nothing here computes results.
#include "wdx_ctx.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

namespace wdx {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static thread_local int64_t g_slice_cap = 0;   // WDX_OPT_MAX_LAUNCH_SLICE of the call running on this thread (0 = none)

int64_t launch_slice_limit(int64_t builtin) { return fp_slice_limit(builtin, g_slice_cap); }
LaunchSliceScope::LaunchSliceScope(int64_t cap) : saved(g_slice_cap) { g_slice_cap = cap; }
LaunchSliceScope::~LaunchSliceScope() { g_slice_cap = saved; }

// content hash of the reference set (cache key): 64-bit words, multiply-xorshift mixing
static uint64_t fnv1a(const void *data, size_t n, uint64_t h = 0xcbf29ce484222325ull) {
    const unsigned char *p = (const unsigned char *)data;
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t w;
        memcpy(&w, p + i, 8);
        h = (h ^ w) * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29;
    }
    for (; i < n; ++i) {
        h ^= p[i];
        h *= 0x100000001b3ull;
    }
    return h;
}

int Buffer::ensure(size_t need, bool exact) {
    if (need <= bytes) return WDX_SUCCESS;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    size_t want = exact ? need : need + need / 4;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess && !exact) {
        e = hipMalloc(&p, need);
        want = need;
    }
    if (e != hipSuccess) {
        set_error("hipMalloc(%zu) failed: %s", need, hipGetErrorString(e));
        p = nullptr;
        return WDX_ERR_HIP;
    }
    bytes = want;
    return WDX_SUCCESS;
}

void Buffer::release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
}

int PinnedBuffer::ensure(size_t need) {
    if (need <= bytes) return WDX_SUCCESS;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
    const size_t want = need + need / 4;
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e != hipSuccess) {
        set_error("hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        p = nullptr;
        return WDX_ERR_HIP;
    }
    bytes = want;
    return WDX_SUCCESS;
}

void PinnedBuffer::release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
}

DeviceGuard::DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device) {
        hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) {
            set_error("hipSetDevice(%d) failed: %s", device, hipGetErrorString(e));
            rc = WDX_ERR_HIP;
            prev = -1;
        }
    } else {
        prev = -1;  // nothing to restore
    }
}

DeviceGuard::~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
}

// one event pair from the context's pool, or two fresh events -- both or neither (a failed second create must not leak
// the first)
static std::pair<hipEvent_t, hipEvent_t> take_event_pair(wdx_ctx *c) {
    std::pair<hipEvent_t, hipEvent_t> q{nullptr, nullptr};
    if (!c->pool.empty()) {
        q = c->pool.back();
        c->pool.pop_back();
        return q;
    }
    if (hipEventCreate(&q.first) != hipSuccess) return {nullptr, nullptr};
    if (hipEventCreate(&q.second) != hipSuccess) {
        (void)hipEventDestroy(q.first);
        return {nullptr, nullptr};
    }
    return q;
}

Timed::Timed(wdx_ctx *c_, int id_, hipStream_t s_) : c(c_), id(id_), s(s_) {
    if (!c->timing) return;
    ev = take_event_pair(c);
    if (!ev.first) return;
    (void)hipEventRecord(ev.first, s);
    if (id == WDX_K_FINGERPRINT) {  // a second pair for the main fast-kernel launches (recorded by launch_fingerprint)
        const auto m = take_event_pair(c);
        main.first = m.first;
        main.second = m.second;
        const auto q = take_event_pair(c);   // ... and a third around clip_bounds_kernel
        main.c_first = q.first;
        main.c_second = q.second;
        // (the split main kernel asks for one more pair per tail-kernel launch)
        main.take = [](void *arg) { return take_event_pair(static_cast<wdx_ctx *>(arg)); };
        main.take_arg = c;
    }
}

Timed::~Timed() {
    if (!ev.first) return;
    (void)hipEventRecord(ev.second, s);
    c->pending[id].push_back(ev);
    c->pending_launches[id].push_back(n_launches > 0 ? n_launches : 1);
    if (main.first) {
        if (main.recorded) {
            c->pending[WDX_K_FINGERPRINT_MAIN].push_back({main.first, main.second});
            c->pending_launches[WDX_K_FINGERPRINT_MAIN].push_back(n_launches > 0 ? n_launches : 1);
        } else {
            c->pool.push_back({main.first, main.second});
        }
    }
    for (const auto &tp : main.tail) {
        c->pending[WDX_K_FINGERPRINT_TAIL].push_back(tp);
        c->pending_launches[WDX_K_FINGERPRINT_TAIL].push_back(1);
    }
    for (const auto &tp : main.optimal) {
        c->pending[WDX_K_REFINE_OPTIMAL].push_back(tp);
        c->pending_launches[WDX_K_REFINE_OPTIMAL].push_back(1);
    }
    if (main.c_first) {
        if (main.c_recorded) {
            c->pending[WDX_K_FINGERPRINT_CLIP].push_back({main.c_first, main.c_second});
            c->pending_launches[WDX_K_FINGERPRINT_CLIP].push_back(1);
        } else {
            c->pool.push_back({main.c_first, main.c_second});
        }
    }
}

int check_ctx(wdx_ctx *ctx) {
    if (!ctx) {
        set_error("null context");
        return WDX_ERR_INVALID;
    }
    return WDX_SUCCESS;
}

int use_stream(wdx_ctx *ctx, hipStream_t s) {
    if (ctx->last_stream_valid && ctx->last_stream != s) WDX_HIP_TRY(hipStreamSynchronize(ctx->last_stream));
    ctx->last_stream = s;
    ctx->last_stream_valid = true;
    return WDX_SUCCESS;
}

int fingerprint_stage(wdx_ctx *B, const FpReads &in, const wdx_seg_params &p, const FpOut &out, void *d_ws,
                      hipStream_t s, const RefineDev *rf, bool main_events) {
    if (int rc = B->fp_big.ensure((size_t)fingerprint_big_bytes(in.max_len))) return rc;
    const bool with_long = B->knobs.long_form(rf != nullptr) && fingerprint_long_bytes(in.max_len) > 0;
    if (with_long)
        if (int rc = B->fp_long.ensure((size_t)fingerprint_long_bytes(in.max_len))) return rc;
    // WDX_OPT_REFINE_OPTIMAL_CPTS: the scratch of the optimal change-points (path tables of the reads in flight), allocated by
    // the first refining call with the option on and never otherwise
    const bool optimal = rf != nullptr && B->knobs.refine_optimal;
    if (optimal)
        if (int rc = B->fp_opt.ensure((size_t)fingerprint_optimal_bytes(in.n_reads, in.max_len, refine_segm_events(rf)))) return rc;
    Timed t(B, WDX_K_FINGERPRINT, s);
    MainEvents only_optimal;   // (a caller that asked for no main-kernel events still gets the optimal kernel's pair)
    MainEvents *ev = main_events ? &t.main : nullptr;
    if (!ev && optimal && t.main.take) {
        only_optimal.take = t.main.take;
        only_optimal.take_arg = t.main.take_arg;
        ev = &only_optimal;
    }
    const int rc = launch_fingerprint(in, p, out, s, d_ws, B->knobs, &t.n_launches, nullptr, 0, 0, rf, ev, (double *)B->fp_big.p,
                                      with_long ? B->fp_long.p : nullptr, optimal ? B->fp_opt.p : nullptr);
    for (const auto &tp : only_optimal.optimal) t.main.optimal.push_back(tp);
    return rc;
}

int check_ref_length(const DtwRefs &R, const wdx_seg_params &p) {
    if (p.barcode_num_events == R.L) return WDX_SUCCESS;
    set_error("barcode_num_events (%lld) != reference length (%lld)", (long long)p.barcode_num_events, (long long)R.L);
    return WDX_ERR_INVALID;
}

// The refinement branch's device state for n_reads reads on stream s, everything but the rows themselves:
//   * the consensus comes from the host (84 doubles) and is kept resident in B->ref_buf: uploaded only when its content
//     changes, and then synchronously after the stream has drained (no reliance on how the runtime stages pageable copies;
//     ADVICE r3) -- so rp->query is free again when this returns;
//   * d_idx (nullable) starts as -1 (reads that fail before the match);
//   * the hand-over records of the fast kernels in d_ws (null: B->ref_ws) start untouched: only the state word of every
//     record is cleared, 4 of its 1632 bytes.
int refine_prepare(wdx_ctx *B, const wdx_refine_params &rp, int64_t n_reads, int32_t *d_idx, void *d_ws, hipStream_t s,
                   RefineDev **rf) {
    int rc = WDX_SUCCESS;
    const size_t qb = ((size_t)rp.n_query * 8 + 15) / 16 * 16;
    {
        const void *before = B->ref_buf.p;
        if ((rc = B->ref_buf.ensure(qb))) return rc;
        if (B->ref_buf.p != before) B->ref_query_host.clear();  // (a new block: nothing is resident in it)
    }
    if (!d_ws) {
        const size_t wb = (size_t)fingerprint_refine_ws_bytes(n_reads);
        if ((rc = B->ref_ws.ensure(wb ? wb : 8))) return rc;
        d_ws = B->ref_ws.p;
    }
    if (B->ref_query_host.size() != (size_t)rp.n_query ||
        memcmp(B->ref_query_host.data(), rp.query, (size_t)rp.n_query * 8) != 0) {
        WDX_HIP_TRY(hipStreamSynchronize(s));
        WDX_HIP_TRY(hipMemcpy(B->ref_buf.p, rp.query, (size_t)rp.n_query * 8, hipMemcpyHostToDevice));
        B->ref_query_host.assign(rp.query, rp.query + rp.n_query);
    }
    if (d_idx) WDX_HIP_TRY(hipMemsetAsync(d_idx, 0xff, (size_t)n_reads * 12, s));
    WDX_HIP_TRY(hipMemset2DAsync(d_ws, (size_t)fingerprint_refine_ws_bytes(1), 0, 4, (size_t)n_reads, s));
    if ((rc = fill_refine_dev(rp, (const double *)B->ref_buf.p, d_idx, rf))) return rc;
    set_refine_ws(*rf, d_ws);
    return WDX_SUCCESS;
}

}  // namespace wdx

using namespace wdx;

namespace wdx {

// (re)build the resident reference set from a HOST array
int set_refs_locked(wdx_ctx *ctx, const double *Y, int64_t nY, int64_t L, int32_t window,
                    double penalty, hipStream_t stream) {
    if (nY < 0 || L <= 0 || (nY > 0 && !Y)) {
        set_error("set_refs: need nY >= 0, L > 0 and a non-null Y");
        return WDX_ERR_INVALID;
    }
    if (penalty != penalty) {
        set_error("set_refs: penalty is NaN");
        return WDX_ERR_INVALID;
    }
    const int w_eff = (int)dtw_effective_window(L, window);
    uint64_t h = fnv1a(Y, (size_t)(nY * L) * sizeof(double));
    h = fnv1a(&nY, sizeof(nY), h);
    h = fnv1a(&L, sizeof(L), h);
    DtwRefs &R = ctx->refs;
    if (R.window != 0 && R.content_hash == h && R.nY == nY && R.L == L) {
        if (R.window != w_eff || R.penalty != penalty) ++ctx->refs_gen;
        R.window = w_eff;  // same samples: only the scalars may have changed
        R.penalty = penalty;
        return WDX_SUCCESS;
    }
    ++ctx->refs_gen;
    // a pipelined minibatch (wdx_demux_submit) may still be reading the set that is about to be rebuilt
    for (wdx_ctx *S : ctx->slots)
        if (S) WDX_HIP_TRY(hipStreamSynchronize(S->stream));
    // not set until every buffer below is rebuilt: a failure in the middle must not leave a stale hash over
    // freed or half-written buffers (a later call then reports WDX_ERR_NO_REFS instead of reading them)
    R.window = 0;
    R.content_hash = 0;
    const int halo = kDtwHalo;
    const int64_t Lpad = dtw_padded_length(L);
    const int64_t ldT = round_up(nY > 0 ? nY : 1, 64);
    int rc;
    if ((rc = ctx->refs_pad.ensure((size_t)(nY > 0 ? nY : 1) * Lpad * sizeof(double)))) return rc;
    if ((rc = ctx->refs_T.ensure((size_t)L * ldT * sizeof(double)))) return rc;
    if ((rc = ctx->refs_nan.ensure((size_t)ldT))) return rc;
    if ((rc = ctx->tmp0.ensure((size_t)(nY > 0 ? nY : 1) * L * sizeof(double)))) return rc;
    if (nY > 0) {
        WDX_HIP_TRY(hipMemcpyAsync(ctx->tmp0.p, Y, (size_t)(nY * L) * sizeof(double),
                                   hipMemcpyHostToDevice, stream));
        WDX_HIP_TRY(hipMemsetAsync(ctx->refs_T.p, 0, (size_t)L * ldT * sizeof(double), stream));
        if ((rc = launch_pad_rows((const double *)ctx->tmp0.p, nY, L, (double *)ctx->refs_pad.p,
                                  Lpad, halo, (uint8_t *)ctx->refs_nan.p, stream)))
            return rc;
        if ((rc = launch_transpose((const double *)ctx->tmp0.p, nY, L, (double *)ctx->refs_T.p, ldT,
                                   nullptr, stream)))
            return rc;
        WDX_HIP_TRY(hipStreamSynchronize(stream));  // tmp0 is reused by later calls
    }
    R.pad = (double *)ctx->refs_pad.p;
    R.T = (double *)ctx->refs_T.p;
    R.has_nan = (uint8_t *)ctx->refs_nan.p;
    R.nY = nY;
    R.L = L;
    R.Lpad = Lpad;
    R.ldT = ldT;
    R.halo = halo;
    R.window = w_eff;
    R.penalty = penalty;
    R.content_hash = h;
    R.any_inf = false;
    for (int64_t i = 0; i < nY * L && !R.any_inf; ++i) R.any_inf = Y[i] - Y[i] != 0.0 && Y[i] == Y[i];   // (+-inf, not NaN)
    return WDX_SUCCESS;
}

// Where the copy a plan names lives (plan.copy_bytes, plan.flag_bytes), and the scratch rows' block (plan.scratch_bytes)
struct DtwWork {
    double *copy;
    uint8_t *flags;
    void *scratch;
    int64_t scratch_bytes;
};

// Device rows dX (nX, L) against the resident refs -> d_out (nX, nY) [+ argmin] as the plan (wdx_dtw_plan.h) says: the copy it
// names into W (WDX_K_TRANSPOSE), then its launches (WDX_K_DTW).  dtw_settle_inf is the caller's.
static int dtw_rows_vs_refs(wdx_ctx *ctx, const DtwPlan &P, const double *dX, const DtwWork &W, float *d_out, int32_t *d_argmin,
                            hipStream_t stream, const NearestArgs *nearest = nullptr) {
    const DtwRefs &R = ctx->refs;
    if (P.info.family == WDX_DTW_NONE) return WDX_SUCCESS;   // (no reads or no references)
    const int64_t nX = P.prep == DtwPrep::kPaddedReads ? P.rows : P.lanes;
    // lanes = reads, each reading its own row-major row in place, against the resident padded refs
    DtwOperands op{dX, 1, P.lanes, nullptr, R.pad, R.Lpad, R.halo, P.rows, R.has_nan, R.penalty, d_out, R.nY, 1,
                   d_argmin, W.scratch, W.scratch_bytes, ctx->knobs.dtw_unfused, stream};
    op.nearest = nearest;   // (the rule in the kernel's epilogue: plans of nearest_plan with rule kFused)
    if (P.prep == DtwPrep::kReadMinor) {
        Timed t(ctx, WDX_K_TRANSPOSE, stream);
        if (int rc = launch_transpose(dX, nX, P.L, W.copy, P.ld, W.flags, stream)) return rc;
        op.A = W.copy, op.ldA = P.ld, op.a_nan = W.flags;
    } else if (P.prep == DtwPrep::kPaddedReads) {
        // lanes = refs (the resident transposed set), the padded reads are the uniform operand
        Timed t(ctx, WDX_K_TRANSPOSE, stream);
        if (int rc = launch_pad_rows(dX, nX, P.L, W.copy, P.ld, kDtwHalo, W.flags, stream)) return rc;
        op.A = R.T, op.ldA = R.ldT, op.a_nan = R.has_nan;
        op.Bpad = W.copy, op.Lpad = P.ld, op.halo = kDtwHalo, op.b_nan = W.flags;
        op.sA = 1, op.sB = R.nY;
    }
    // the wavefront and the refs-as-lanes routes take their argmin behind the WDX_K_DTW scope, the others inside it
    const bool late_argmin = P.info.family == WDX_DTW_WAVEFRONT || P.prep == DtwPrep::kPaddedReads;
    if (late_argmin) op.argmin = nullptr;
    {
        Timed t(ctx, WDX_K_DTW, stream);
        if (int rc = run_dtw_plan(P, op, &ctx->dtw_last)) return rc;
    }
    if (late_argmin && P.argmin_after && d_argmin) return launch_argmin(d_out, nX, R.nY, d_argmin, stream);
    return WDX_SUCCESS;
}

// DTW of device rows dX (nX, L) against the resident refs -> d_out (nX, nY) [+ argmin]
int dtw_dev_locked(wdx_ctx *ctx, const double *dX, int64_t nX, float *d_out, int32_t *d_argmin,
                   hipStream_t stream) {
    const DtwRefs &R = ctx->refs;
    if (R.window == 0) {
        set_error("no reference set: call wdx_set_refs first");
        return WDX_ERR_NO_REFS;
    }
    const DtwPlan P = dtw_plan(nX, R.nY, R.L, R.window, d_argmin != nullptr, DtwEntry::kMatrix, ctx->knobs.dtw_switches());
    int rc;
    if (P.scratch_bytes && (rc = ctx->scratch.ensure((size_t)P.scratch_bytes))) return rc;
    if (P.copy_bytes && (rc = ctx->tmp1.ensure((size_t)P.copy_bytes))) return rc;
    if (P.flag_bytes && (rc = ctx->tmp2.ensure((size_t)P.flag_bytes))) return rc;
    const DtwWork W{(double *)ctx->tmp1.p, (uint8_t *)ctx->tmp2.p, ctx->scratch.p, (int64_t)ctx->scratch.bytes};
    if ((rc = dtw_rows_vs_refs(ctx, P, dX, W, d_out, d_argmin, stream))) return rc;
    return dtw_settle_inf(R, dX, nX, d_out, d_argmin, stream);
}

// a reference with an infinite sample (never a fingerprint)
int dtw_settle_inf(const DtwRefs &R, const double *dX, int64_t nX, float *d_out, int32_t *d_argmin, hipStream_t stream) {
    if (!R.any_inf || nX == 0 || R.nY == 0) return WDX_SUCCESS;
    if (int rc = launch_dtw_equal_inf(dX, nX, R.pad, R.Lpad, R.halo, R.nY, R.L, d_out, stream)) return rc;
    if (d_argmin) return launch_argmin(d_out, nX, R.nY, d_argmin, stream);
    return WDX_SUCCESS;
}

// What every nearest-reference entry refuses before it looks at its reads (include/wdx.h: wdx_nearest_dev)
static int nearest_args_ok(const char *who, const DtwRefs &R, bool have_labels, int64_t n_labels) {
    if (R.window == 0) {
        set_error("no reference set: call wdx_set_refs first");
        return WDX_ERR_NO_REFS;
    }
    if (n_labels < 1 || n_labels > INT32_MAX) {
        set_error("%s: n_labels must be at least 1, not %lld", who, (long long)n_labels);
        return WDX_ERR_INVALID;
    }
    if (R.nY < 1 || R.nY > INT32_MAX) {
        set_error("%s: the resident reference set holds %lld references", who, (long long)R.nY);
        return WDX_ERR_INVALID;
    }
    if (!have_labels && n_labels != R.nY) {
        set_error("%s: without reference labels n_labels (%lld) must be the number of resident references (%lld)", who,
                  (long long)n_labels, (long long)R.nY);
        return WDX_ERR_INVALID;
    }
    return WDX_SUCCESS;
}

// Device rows dX (nX, L) against the resident refs, then the nearest-reference rule, as nearest_plan says: row block by row
// block, each with the rule in its DTW kernel's epilogue or behind it on the block's matrix (d_dist, or the context's block
// buffer when the caller wants no distances).  The copies a plan names live in the context's tmp1 / tmp2, the scratch rows in
// its scratch block.  d_counts (nullable) is incremented by the calls.  With the mutex held, after use_stream.
static int nearest_rows_vs_refs(wdx_ctx *ctx, const double *dX, int64_t nX, DtwEntry entry, const NearestArgs &N, float *d_dist,
                                int64_t *d_counts, hipStream_t stream) {
    const DtwRefs &R = ctx->refs;
    const DtwSwitches sw = ctx->knobs.dtw_switches();
    const int64_t step = nearest_plan(nX, R.nY, R.L, R.window, d_dist != nullptr, R.any_inf, entry, sw).block_rows;
    for (int64_t r0 = 0; r0 < nX && step > 0; r0 += step) {
        const int64_t m = std::min(step, nX - r0);
        const NearestPlan NP = nearest_plan(m, R.nY, R.L, R.window, d_dist != nullptr, R.any_inf, entry, sw);
        const DtwPlan &P = NP.dtw;
        int rc;
        if (P.scratch_bytes && (rc = ctx->scratch.ensure((size_t)P.scratch_bytes))) return rc;
        if (P.copy_bytes && (rc = ctx->tmp1.ensure((size_t)P.copy_bytes))) return rc;
        if (P.flag_bytes && (rc = ctx->tmp2.ensure((size_t)P.flag_bytes))) return rc;
        if (NP.buffer && (rc = ctx->nearest_buf.ensure((size_t)NP.buffer_bytes))) return rc;
        const DtwWork W{(double *)ctx->tmp1.p, (uint8_t *)ctx->tmp2.p, ctx->scratch.p, (int64_t)ctx->scratch.bytes};
        const double *X = dX + r0 * R.L;
        float *out = d_dist ? d_dist + r0 * R.nY : (NP.buffer ? (float *)ctx->nearest_buf.p : nullptr);
        const NearestArgs Nb = N.from(r0);
        if (NP.rule == NearestRule::kFused) {
            if ((rc = dtw_rows_vs_refs(ctx, P, X, W, out, nullptr, stream, &Nb))) return rc;
        } else {
            if ((rc = dtw_rows_vs_refs(ctx, P, X, W, out, nullptr, stream))) return rc;
            if ((rc = dtw_settle_inf(R, X, m, out, nullptr, stream))) return rc;
            Timed t(ctx, WDX_K_COUNT, stream);
            if ((rc = launch_nearest_rows(out, m, R.nY, Nb, stream))) return rc;
        }
    }
    if (!d_counts) return WDX_SUCCESS;
    Timed t(ctx, WDX_K_COUNT, stream);
    return launch_count_calls(N.call, nullptr, nX, N.n_labels, d_counts, stream);
}

}  // namespace wdx

namespace wdx {

AdcDevPlan adc_dev_plan_for(const wdx_ctx *ctx, int64_t n_reads, int64_t max_len, bool refine) {
    return adc_dev_plan(n_reads, adc_dev_max_len(max_len, ctx->knobs.max_window(refine)), ctx->knobs.adc_dev_slice_reads);
}

int adc_dev_stage(wdx_ctx *B, const DevRows &rows, const AdcDevPlan &plan, bool refine, int64_t padding, int64_t r0, int64_t m,
                  hipStream_t s, FpReads *rd) {
    const wdx_adc_dev_in &A = *rows.adc;
    float *stage = (float *)B->adc_stage.p;
    // the three int32 arrays behind the rows of the LARGEST slice the block was planned for: every slice finds them there
    int32_t *idx = (int32_t *)(stage + std::min(rows.f32.n_reads, plan.slice_reads) * plan.pitch);
    AdcDevWindows W{};
    W.adc = A.adc, W.row_off = A.row_off, W.stride = A.stride, W.row_len = A.row_len, W.row_win = A.row_off ? A.row_win : nullptr;
    W.offset = A.offset, W.scale = A.scale, W.a_start = rows.f32.a_start, W.a_end = rows.f32.a_end, W.ok = rows.f32.ok;
    W.padding = padding, W.max_len = adc_dev_max_len(rows.f32.max_len, B->knobs.max_window(refine));
    W.r0 = r0, W.n = m, W.dst = stage, W.pitch = plan.pitch;
    W.a_start_out = idx, W.a_end_out = idx + m, W.row_len_out = idx + 2 * m;
    {
        Timed t(B, WDX_K_ADC_DEV_WINDOWS, s);
        if (int rc = launch_adc_dev_windows(W, s)) return rc;
    }
    *rd = FpReads{stage, nullptr, W.row_len_out, plan.pitch, rows.f32.max_len, m, W.a_start_out, W.a_end_out,
                  from_read(rows.f32.ok, r0)};
    return WDX_SUCCESS;
}

// the shard descriptor itself (a HOST struct of device pointers); its arrays are looked at by DevRows::missing when there
// are reads
int adc_dev_in_ok(const char *who, const wdx_adc_dev_in *in) {
    if (in && (in->row_off || (in->stride >= 0 && in->stride <= INT32_MAX))) return WDX_SUCCESS;
    set_error("%s: bad arguments", who);
    return WDX_ERR_INVALID;
}

int fingerprint_dev_rows(wdx_ctx *ctx, const DevRows &rows, const wdx_seg_params *p, double *d_fpt, int64_t *d_dwell,
                         double *d_stats, int32_t *d_status, void *stream) {
    WDX_ENTER(ctx);
    const int64_t n_reads = rows.f32.n_reads;
    if (n_reads < 0 || !p || (n_reads > 0 && (rows.missing() || !rows.f32.a_start || !rows.f32.a_end || !d_status))) {
        set_error("fingerprint_dev: bad arguments");
        return WDX_ERR_INVALID;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = use_stream(ctx, s))) return rc;
    const int64_t K = p->barcode_num_events;
    return for_each_slice(ctx, rows, false, p->padding, s, [&](const FpReads &in, int64_t r0) {
        if (int e = ctx->fp_ws.ensure((size_t)fingerprint_workspace_bytes(in.n_reads))) return e;
        return fingerprint_stage(ctx, in, *p, FpOut{from_read(d_fpt, r0, K), from_read(d_dwell, r0, K), from_read(d_stats, r0, 6),
                                                   from_read(d_status, r0)}, ctx->fp_ws.p, s);
    });
}

int fingerprint_refine_dev_rows(wdx_ctx *ctx, const DevRows &rows, const wdx_seg_params *p_in, const wdx_refine_params *rp,
                                double *d_fpt, int64_t *d_dwell, double *d_stats, int32_t *d_refine_idx, int32_t *d_status,
                                void *stream) {
    WDX_ENTER(ctx);
    const int64_t n_reads = rows.f32.n_reads;
    if (n_reads < 0 || !rp ||
        (n_reads > 0 && (rows.missing() || !rows.f32.a_start || !rows.f32.a_end || !d_status || !d_refine_idx))) {
        set_error("fingerprint_refine_dev: bad arguments");
        return WDX_ERR_INVALID;
    }
    wdx_seg_params pv;
    if ((rc = refine_seg_params("fingerprint_refine_dev", p_in, rp, &pv))) return rc;
    if (n_reads == 0) return WDX_SUCCESS;
    std::lock_guard<std::mutex> g(ctx->mu);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = use_stream(ctx, s))) return rc;
    const int64_t K = pv.barcode_num_events;
    return for_each_slice(ctx, rows, true, pv.padding, s, [&](const FpReads &in, int64_t r0) {
        if (int e = ctx->fp_ws.ensure((size_t)fingerprint_workspace_bytes(in.n_reads))) return e;
        return demux_chain(ctx, DtwRefs{}, in, pv, rp, from_read(d_refine_idx, r0, 3), nullptr, ctx->fp_ws.p, false, ChainTail{},
                           ChainOut{FpOut{from_read(d_fpt, r0, K), from_read(d_dwell, r0, K), from_read(d_stats, r0, 6),
                                          from_read(d_status, r0)}}, s);
    });
}

}  // namespace wdx

extern "C" {

int wdx_abi_version(void) { return WDX_ABI_VERSION; }

const char *wdx_last_error(void) { return g_err; }

int wdx_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        set_error("hipGetDeviceCount failed: %s", hipGetErrorString(e));
        return WDX_ERR_NO_DEVICE;
    }
    return n;
}

int wdx_ctx_create(int device, wdx_ctx **out) {
    if (!out) {
        set_error("null out pointer");
        return WDX_ERR_INVALID;
    }
    *out = nullptr;
    int n = wdx_device_count();
    if (n < 0) return n;
    if (n == 0) {
        set_error("no HIP device visible");
        return WDX_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) {
        set_error("device %d out of range (0..%d)", device, n - 1);
        return WDX_ERR_INVALID;
    }
    DeviceGuard guard(device);
    if (guard.rc) return guard.rc;
    hipDeviceProp_t prop;
    WDX_HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s; this library is built for gfx950 only", device,
                  prop.gcnArchName);
        return WDX_ERR_NO_DEVICE;
    }
    wdx_ctx *c = new wdx_ctx();
    c->device = device;
    // the context's own stream: host-buffer calls of different contexts (one per thread)
    // overlap instead of queueing on the NULL stream
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        set_error("hipStreamCreateWithFlags failed: %s", hipGetErrorString(e));
        delete c;
        return WDX_ERR_HIP;
    }
    *out = c;
    return WDX_SUCCESS;
}

void wdx_ctx_destroy(wdx_ctx *ctx) {
    if (!ctx) return;
    DeviceGuard guard(ctx->device);
    (void)hipDeviceSynchronize();
    for (wdx_ctx *&S : ctx->slots) {
        if (S) {
            S->refs = wdx::DtwRefs{};  // (borrowed pointers)
            wdx_ctx_destroy(S);
        }
        S = nullptr;
    }
    comm_destroy(ctx);
    medoid_release_staged(ctx, true);
    for (Buffer *b : {&ctx->refs_pad, &ctx->refs_T, &ctx->refs_nan, &ctx->in0, &ctx->in1, &ctx->in2,
                      &ctx->in3, &ctx->out0, &ctx->out1, &ctx->out2, &ctx->out3, &ctx->tmp0,
                      &ctx->tmp1, &ctx->tmp2, &ctx->scratch, &ctx->fp_ws, &ctx->svm.block, &ctx->ref_buf, &ctx->fp_big, &ctx->fp_long, &ctx->fp_opt, &ctx->ref_ws, &ctx->pk_idx, &ctx->in_adc, &ctx->adc_stage, &ctx->nearest_buf, &ctx->medoid_ws, &ctx->self_ws, &ctx->loo_ws, &ctx->dba_ws, &ctx->svm_fit_ws, &ctx->mlp_fit_ws, &ctx->boost_fit_ws, &ctx->thr_ws, &ctx->svm_cv_ws, &ctx->svm_refs, &ctx->mlp.block, &ctx->boost.block,
                      &ctx->mb_dwell, &ctx->mb_stats, &ctx->mb_prob, &ctx->mb_pred, &ctx->mb_conf, &ctx->mb_ridx})
        b->release();
    ctx->pin_in.release();
    ctx->pin_out.release();
    ctx->pk_host.release();
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    for (int k = 0; k < kNumTimed; ++k)
        for (auto &e : ctx->pending[k]) {
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
    for (auto &e : ctx->pool) {
        (void)hipEventDestroy(e.first);
        (void)hipEventDestroy(e.second);
    }
    delete ctx;
}

int wdx_ctx_set_option(wdx_ctx *ctx, int32_t option, int64_t value) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    switch (option) {
        case WDX_OPT_EXACT_PATH: ctx->knobs.exact_path = value != 0; break;
        case WDX_OPT_NO_WAVEFRONT_DTW: ctx->knobs.no_wavefront = value != 0; break;
        case WDX_OPT_NO_SHORT_DTW: ctx->knobs.no_short_dtw = value != 0; break;
        case WDX_OPT_SVM_SCALAR: ctx->knobs.svm_scalar = value != 0; break;
        case WDX_OPT_DEBUG_OCCUPANCY: ctx->knobs.debug_occ = value != 0; break;
        case WDX_OPT_FAST_PEAK_CAP: ctx->knobs.fast_peak_cap = (int)value; break;
        case WDX_OPT_FAST_EXACT_SCORES: ctx->knobs.fast_exact_scores = value != 0; break;
        case WDX_OPT_FAST_MAIN_CAP: ctx->knobs.fast_main_cap = (int)value; break;
        case WDX_OPT_FAST_CHAIN_MIN_READS: ctx->knobs.fast_chain_min = (int)value; break;
        case WDX_OPT_EXACT_NO_PEAK_LIST: ctx->knobs.exact_no_list = value != 0; break;
        case WDX_OPT_NO_PEAK_FILTER: ctx->knobs.no_peak_filter = value != 0; break;
        case WDX_OPT_NO_WAVE_CLIP_LONG: ctx->knobs.no_wave_clip_long = value != 0; break;
        case WDX_OPT_NO_CLIP_REUSE: ctx->knobs.no_clip_reuse = value != 0; break;
        case WDX_OPT_NO_SPLIT_TAIL: ctx->knobs.no_split = value != 0; break;
        case WDX_OPT_DTW_UNFUSED: ctx->knobs.dtw_unfused = (value >= 0 && value <= 3) ? (int)value : 0; break;
        case WDX_OPT_MAX_LAUNCH_SLICE: ctx->knobs.max_launch_slice = value > 0 ? value : 0; break;
        case WDX_OPT_MLP_CHUNK_ROWS: ctx->knobs.mlp_chunk_rows = value > 0 ? value : 0; break;
        case WDX_OPT_BOOST_CHUNK_ROWS: ctx->knobs.boost_chunk_rows = value > 0 ? value : 0; break;
        case WDX_OPT_BOOST_KERNEL: ctx->knobs.boost_kernel = (value >= 0 && value <= 2) ? (int)value : 0; break;
        case WDX_OPT_LONG_WINDOWS:
            if (value != 0 && value != 1) {
                set_error("WDX_OPT_LONG_WINDOWS is 0 or 1, not %lld", (long long)value);
                return WDX_ERR_INVALID;
            }
            ctx->knobs.long_windows = value == 1;
            break;
        case WDX_OPT_LONG_REFINE_WINDOWS:
            if (value != 0 && value != 1) {
                set_error("WDX_OPT_LONG_REFINE_WINDOWS is 0 or 1, not %lld", (long long)value);
                return WDX_ERR_INVALID;
            }
            ctx->knobs.long_refine_windows = value == 1;
            break;
        case WDX_OPT_REFINE_OPTIMAL_CPTS:
            if (value != 0 && value != 1) {
                set_error("WDX_OPT_REFINE_OPTIMAL_CPTS is 0 or 1, not %lld", (long long)value);
                return WDX_ERR_INVALID;
            }
            ctx->knobs.refine_optimal = value == 1;
            break;
        case WDX_OPT_WIDE_DTW:
            if (value != 0 && value != 1) {
                set_error("WDX_OPT_WIDE_DTW is 0 or 1, not %lld", (long long)value);
                return WDX_ERR_INVALID;
            }
            ctx->knobs.wide_dtw = value == 1;
            break;
        case WDX_OPT_MEDOID_GENERAL:
            if (value != 0 && value != 1) {
                set_error("WDX_OPT_MEDOID_GENERAL is 0 or 1, not %lld", (long long)value);
                return WDX_ERR_INVALID;
            }
            ctx->knobs.medoid_general = value == 1;
            break;
        case WDX_OPT_SELF_MATRIX_GENERAL:
            if (value != 0 && value != 1) {
                set_error("WDX_OPT_SELF_MATRIX_GENERAL is 0 or 1, not %lld", (long long)value);
                return WDX_ERR_INVALID;
            }
            ctx->knobs.self_matrix_general = value == 1;
            break;
        case WDX_OPT_DBA_GENERAL:
            if (value != 0 && value != 1) {
                set_error("WDX_OPT_DBA_GENERAL is 0 or 1, not %lld", (long long)value);
                return WDX_ERR_INVALID;
            }
            ctx->knobs.dba_general = value == 1;
            break;
        case WDX_OPT_SELF_NEAREST_GENERAL:
            if (value != 0 && value != 1) {
                set_error("WDX_OPT_SELF_NEAREST_GENERAL is 0 or 1, not %lld", (long long)value);
                return WDX_ERR_INVALID;
            }
            ctx->knobs.self_nearest_general = value == 1;
            break;
        case WDX_OPT_ADC_DEV_SLICE_READS:
            if (value < 0) {
                set_error("WDX_OPT_ADC_DEV_SLICE_READS is 0 (built-in) or a number of reads, not %lld", (long long)value);
                return WDX_ERR_INVALID;
            }
            ctx->knobs.adc_dev_slice_reads = value;
            break;
        default:
            set_error("unknown option %d", (int)option);
            return WDX_ERR_INVALID;
    }
    return WDX_SUCCESS;
}

int wdx_ctx_stream(wdx_ctx *ctx, void **stream) {
    WDX_ENTER(ctx);
    if (!stream) {
        set_error("ctx_stream: null output");
        return WDX_ERR_INVALID;
    }
    *stream = (void *)ctx->stream;
    return WDX_SUCCESS;
}

int wdx_ctx_synchronize(wdx_ctx *ctx, void *stream) {
    WDX_ENTER(ctx);
    // NULL names the legacy NULL stream, as in every *_dev entry point (engine.py hands over torch's default
    // stream, whose handle is 0).  The context's own non-blocking stream -- the one the host-buffer calls run
    // on -- is waited for as well: those calls synchronise before they return, so this costs nothing and a
    // caller who only knows the context cannot be handed a half-finished result.
    if (stream) {
        WDX_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    } else {
        WDX_HIP_TRY(hipStreamSynchronize(nullptr));
        WDX_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return WDX_SUCCESS;
}

int wdx_refs_generation(wdx_ctx *ctx, int64_t *generation) {
    WDX_ENTER(ctx);
    if (!generation) {
        set_error("refs_generation: null output");
        return WDX_ERR_INVALID;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    *generation = ctx->refs_gen;
    return WDX_SUCCESS;
}

int wdx_set_refs(wdx_ctx *ctx, const double *Y, int64_t nY, int64_t L, int32_t window,
                 double penalty) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    if ((rc = use_stream(ctx, ctx->stream))) return rc;
    for (wdx_ctx *S : ctx->slots)   // (also when only window / penalty change: a slot copied them at its submit)
        if (S) WDX_HIP_TRY(hipStreamSynchronize(S->stream));
    return set_refs_locked(ctx, Y, nY, L, window, penalty, ctx->stream);
}

int wdx_dtw_matrix_dev(wdx_ctx *ctx, const double *dX, int64_t nX, float *d_out, int32_t *d_argmin,
                       void *stream) {
    WDX_ENTER(ctx);
    if (nX < 0 || (nX > 0 && (!dX || !d_out))) {
        set_error("dtw_matrix_dev: bad arguments");
        return WDX_ERR_INVALID;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    if ((rc = use_stream(ctx, (hipStream_t)stream))) return rc;
    return dtw_dev_locked(ctx, dX, nX, d_out, d_argmin, (hipStream_t)stream);
}

int wdx_dtw_matrix(wdx_ctx *ctx, const double *X, int64_t nX, const double *Y, int64_t nY,
                   int64_t L, int32_t window, double penalty, float *out, int32_t *argmin) {
    WDX_ENTER(ctx);
    if (nX < 0 || nY < 0 || L <= 0 || (nX > 0 && !X) || (nY > 0 && !Y) ||
        (nX > 0 && nY > 0 && !out)) {
        set_error("dtw_matrix: need nX,nY >= 0, L > 0 and non-null buffers");
        return WDX_ERR_INVALID;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    hipStream_t s = ctx->stream;
    if ((rc = use_stream(ctx, s))) return rc;
    if ((rc = set_refs_locked(ctx, Y, nY, L, window, penalty, s))) return rc;
    if (nX == 0 || nY == 0) {
        if (argmin)
            for (int64_t i = 0; i < nX; ++i) argmin[i] = 0;
        return WDX_SUCCESS;
    }
    const size_t xb = (size_t)(nX * L) * sizeof(double), ob = (size_t)(nX * nY) * sizeof(float);
    if ((rc = ctx->in0.ensure(xb))) return rc;
    if ((rc = ctx->out0.ensure(ob))) return rc;
    if (argmin && (rc = ctx->out1.ensure((size_t)nX * sizeof(int32_t)))) return rc;
    StreamDrain drain(s);
    WDX_HIP_TRY(hipMemcpyAsync(ctx->in0.p, X, xb, hipMemcpyHostToDevice, s));
    if ((rc = dtw_dev_locked(ctx, (const double *)ctx->in0.p, nX, (float *)ctx->out0.p,
                             argmin ? (int32_t *)ctx->out1.p : nullptr, s)))
        return rc;
    WDX_HIP_TRY(hipMemcpyAsync(out, ctx->out0.p, ob, hipMemcpyDeviceToHost, s));
    if (argmin)
        WDX_HIP_TRY(hipMemcpyAsync(argmin, ctx->out1.p, (size_t)nX * sizeof(int32_t),
                                   hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipStreamSynchronize(s));
    drain.done();
    return WDX_SUCCESS;
}

int wdx_fingerprint_dev(wdx_ctx *ctx, const float *d_sig, const int64_t *d_row_off,
                        const int32_t *d_row_len, int64_t stride, int64_t max_len, int64_t n_reads,
                        const int32_t *d_a_start, const int32_t *d_a_end, const uint8_t *d_ok,
                        const wdx_seg_params *p, double *d_fpt, int64_t *d_dwell, double *d_stats,
                        int32_t *d_status, void *stream) {
    return fingerprint_dev_rows(ctx, DevRows(d_sig, d_row_off, d_row_len, stride, max_len, n_reads, d_a_start, d_a_end, d_ok), p,
                                d_fpt, d_dwell, d_stats, d_status, stream);
}

int wdx_fingerprint_adc_dev(wdx_ctx *ctx, const wdx_adc_dev_in *in, int64_t max_len, int64_t n_reads,
                            const int32_t *d_a_start, const int32_t *d_a_end, const uint8_t *d_ok, const wdx_seg_params *p,
                            double *d_fpt, int64_t *d_dwell, double *d_stats, int32_t *d_status, void *stream) {
    if (int e = adc_dev_in_ok("fingerprint_adc_dev", in)) return e;
    return fingerprint_dev_rows(ctx, DevRows(in, max_len, n_reads, d_a_start, d_a_end, d_ok), p, d_fpt, d_dwell, d_stats,
                                d_status, stream);
}

int wdx_fingerprint_refine_dev(wdx_ctx *ctx, const float *d_sig, const int64_t *d_row_off,
                               const int32_t *d_row_len, int64_t stride, int64_t max_len, int64_t n_reads,
                               const int32_t *d_a_start, const int32_t *d_a_end, const uint8_t *d_ok,
                               const wdx_seg_params *p_in, const wdx_refine_params *rp, double *d_fpt,
                               int64_t *d_dwell, double *d_stats, int32_t *d_refine_idx, int32_t *d_status,
                               void *stream) {
    return fingerprint_refine_dev_rows(ctx, DevRows(d_sig, d_row_off, d_row_len, stride, max_len, n_reads, d_a_start, d_a_end, d_ok),
                                       p_in, rp, d_fpt, d_dwell, d_stats, d_refine_idx, d_status, stream);
}

int wdx_fingerprint_refine_adc_dev(wdx_ctx *ctx, const wdx_adc_dev_in *in, int64_t max_len, int64_t n_reads,
                                   const int32_t *d_a_start, const int32_t *d_a_end, const uint8_t *d_ok,
                                   const wdx_seg_params *p, const wdx_refine_params *rp, double *d_fpt, int64_t *d_dwell,
                                   double *d_stats, int32_t *d_refine_idx, int32_t *d_status, void *stream) {
    if (int e = adc_dev_in_ok("fingerprint_refine_adc_dev", in)) return e;
    return fingerprint_refine_dev_rows(ctx, DevRows(in, max_len, n_reads, d_a_start, d_a_end, d_ok), p, rp, d_fpt, d_dwell,
                                       d_stats, d_refine_idx, d_status, stream);
}

int wdx_fingerprint_profile_dev(wdx_ctx *ctx, const float *d_sig, const int64_t *d_row_off,
                                int64_t stride, int64_t max_len, int64_t n_reads,
                                const int32_t *d_a_start, const int32_t *d_a_end,
                                const wdx_seg_params *p, int32_t *d_status, long long *d_prof,
                                int64_t prof_reads, int32_t fast_path, int32_t stop_phase, void *stream) {
    WDX_ENTER(ctx);
    if (!p || !d_prof || !d_status) {
        set_error("fingerprint_profile_dev: bad arguments");
        return WDX_ERR_INVALID;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    if ((rc = use_stream(ctx, (hipStream_t)stream))) return rc;
    if ((rc = ctx->fp_ws.ensure((size_t)fingerprint_workspace_bytes(n_reads)))) return rc;
    const FpReads in{d_sig, d_row_off, nullptr, stride, max_len, n_reads, d_a_start, d_a_end, nullptr};
    rc = launch_fingerprint(in, *p, FpOut{nullptr, nullptr, nullptr, d_status}, (hipStream_t)stream,
                            fast_path ? ctx->fp_ws.p : nullptr, ctx->knobs, nullptr, d_prof, prof_reads,
                            fast_path == 2 ? -2 : stop_phase);   // (-2: the split pair's diagnostic build)
    if (rc == WDX_SUCCESS && fast_path && prof_reads > 0 && stop_phase == 0) {
        // slot 15 of read 0 <- number of reads the fast kernel handed to the slow path
        WDX_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        unsigned cnt = 0;
        WDX_HIP_TRY(hipMemcpy(&cnt, ctx->fp_ws.p, 4, hipMemcpyDeviceToHost));
        long long v = cnt;
        WDX_HIP_TRY(hipMemcpy(d_prof + 15, &v, 8, hipMemcpyHostToDevice));  // row 0, slot 15 of 32
    }
    return rc;
}

}  // extern "C"

extern "C" {

int64_t wdx_demux_workspace_bytes(int64_t n_reads, int32_t K) {
    return demux_workspace_size(n_reads, K);   // (wdx_work_layout.h)
}

int64_t wdx_demux_refine_workspace_bytes(int64_t n_reads, int32_t K) {
    return demux_refine_workspace_size(n_reads, K);
}

// the largest d_work any slice of an int16 shard asks its float32 twin's layout for: a full slice, or the last, shorter one
// (which may be the one below kRowMajorMinReads that holds the read-minor copy)
static int64_t adc_workspace_bytes(wdx_ctx *ctx, int64_t n_reads, int64_t max_len, int32_t K, bool refine) {
    if (!ctx || n_reads < 0 || K < 1) return 0;
    const AdcDevPlan P = adc_dev_plan_for(ctx, n_reads, max_len, refine);
    return demux_shard_workspace_size(n_reads, P.slice_reads, P.last_reads, K, refine);
}

int64_t wdx_demux_adc_workspace_bytes(wdx_ctx *ctx, int64_t n_reads, int64_t max_len, int32_t K) {
    return adc_workspace_bytes(ctx, n_reads, max_len, K, false);
}

int64_t wdx_demux_refine_adc_workspace_bytes(wdx_ctx *ctx, int64_t n_reads, int64_t max_len, int32_t K) {
    return adc_workspace_bytes(ctx, n_reads, max_len, K, true);
}

int64_t wdx_adc_dev_staging_bytes(wdx_ctx *ctx, int64_t n_reads, int64_t max_len, int32_t refine) {
    return ctx ? adc_dev_plan_for(ctx, n_reads, max_len, refine != 0).staging_bytes : 0;
}

}  // extern "C"

// wdx_demux_dev; with rp the fingerprint stage takes the refinement branch (wdx_demux_refine_dev: `p` carries
// K = rp->barcode_keep_events already, the hand-over records live behind the plain call's pieces of d_work)
int wdx::demux_dev_rows(wdx_ctx *ctx, const DevRows &rows, const wdx_seg_params *p, const wdx_refine_params *rp, double *d_fpt,
                        int64_t *d_dwell, double *d_stats, int32_t *d_refine_idx, int32_t *d_status, float *d_dist,
                        int32_t *d_call, int64_t *d_counts, void *d_work, void *stream) {
    WDX_ENTER(ctx);
    if (rows.f32.n_reads < 0 || !p ||
        (rows.f32.n_reads > 0 &&
         (rows.missing() || !rows.f32.a_start || !rows.f32.a_end || !d_status || !d_dist || !d_call || !d_work))) {
        set_error("demux_dev: bad arguments");
        return WDX_ERR_INVALID;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    DtwRefs &R = ctx->refs;
    if (R.window == 0) {
        set_error("no reference set: call wdx_set_refs first");
        return WDX_ERR_NO_REFS;
    }
    const int64_t K = p->barcode_num_events;
    if ((rc = check_ref_length(R, *p))) return rc;
    const DtwSwitches sw = ctx->knobs.dtw_switches();
    if (dtw_plan(rows.f32.n_reads, R.nY, R.L, R.window, true, DtwEntry::kFused, sw).unsupported) {
        set_error("demux_dev needs window <= %d", kMaxRegWindow);
        return WDX_ERR_UNSUPPORTED;
    }
    if (rows.f32.n_reads == 0) return WDX_SUCCESS;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = use_stream(ctx, s))) return rc;
    unsigned char *w = (unsigned char *)d_work;
    return for_each_slice(ctx, rows, rp != nullptr, p->padding, s, [&](const FpReads &in, int64_t r0) {
        int rc = WDX_SUCCESS;
        const int64_t n_reads = in.n_reads;
        double *fpt = d_fpt ? d_fpt + r0 * K : (double *)w;
        int32_t *status = d_status + r0, *call = d_call + r0;
        float *dist = d_dist + r0 * R.nY;
        // (failed reads carry NaN fingerprints: the row-major kernels flag them themselves, the read-minor copy has flags)
        const DtwPlan P = dtw_plan(n_reads, R.nY, R.L, R.window, true, DtwEntry::kFused, sw);
        const DemuxWork W = demux_work_layout(n_reads, K, P.prep == DtwPrep::kReadMinor);
        RefineDev *rf = nullptr;
        RefineDevGuard rf_guard{rf};
        if (rp && (rc = refine_prepare(ctx, *rp, n_reads, from_read(d_refine_idx, r0, 3), w + demux_refine_records_offset(W), s, &rf)))
            return rc;
        if ((rc = fingerprint_stage(ctx, in, *p, FpOut{fpt, from_read(d_dwell, r0, K), from_read(d_stats, r0, 6), status},
                                    w + W.fp_ws, s, rf, rf == nullptr)))
            return rc;
        if ((rc = dtw_rows_vs_refs(ctx, P, fpt, DtwWork{(double *)(w + W.fptT), w + W.flags, nullptr, 0}, dist, call, s))) return rc;
        if ((rc = dtw_settle_inf(R, fpt, n_reads, dist, call, s))) return rc;
        Timed t(ctx, WDX_K_COUNT, s);
        return launch_count_calls(call, status, n_reads, R.nY, d_counts, s);
    });
}

extern "C" {

int wdx_demux_dev(wdx_ctx *ctx, const float *d_sig, const int64_t *d_row_off,
                  const int32_t *d_row_len, int64_t stride, int64_t max_len, int64_t n_reads,
                  const int32_t *d_a_start, const int32_t *d_a_end, const uint8_t *d_ok,
                  const wdx_seg_params *p, double *d_fpt, int64_t *d_dwell, double *d_stats,
                  int32_t *d_status, float *d_dist, int32_t *d_call, int64_t *d_counts, void *d_work,
                  void *stream) {
    return demux_dev_rows(ctx, DevRows(d_sig, d_row_off, d_row_len, stride, max_len, n_reads, d_a_start, d_a_end, d_ok), p,
                          nullptr, d_fpt, d_dwell, d_stats, nullptr, d_status, d_dist, d_call, d_counts, d_work, stream);
}

int wdx_demux_adc_dev(wdx_ctx *ctx, const wdx_adc_dev_in *in, int64_t max_len, int64_t n_reads, const int32_t *d_a_start,
                      const int32_t *d_a_end, const uint8_t *d_ok, const wdx_seg_params *p, double *d_fpt, int64_t *d_dwell,
                      double *d_stats, int32_t *d_status, float *d_dist, int32_t *d_call, int64_t *d_counts, void *d_work,
                      void *stream) {
    if (int e = adc_dev_in_ok("demux_adc_dev", in)) return e;
    return demux_dev_rows(ctx, DevRows(in, max_len, n_reads, d_a_start, d_a_end, d_ok), p, nullptr, d_fpt, d_dwell, d_stats,
                          nullptr, d_status, d_dist, d_call, d_counts, d_work, stream);
}

int wdx_demux_refine_dev(wdx_ctx *ctx, const float *d_sig, const int64_t *d_row_off, const int32_t *d_row_len,
                         int64_t stride, int64_t max_len, int64_t n_reads, const int32_t *d_a_start,
                         const int32_t *d_a_end, const uint8_t *d_ok, const wdx_seg_params *p,
                         const wdx_refine_params *rp, double *d_fpt, int64_t *d_dwell, double *d_stats,
                         int32_t *d_refine_idx, int32_t *d_status, float *d_dist, int32_t *d_call, int64_t *d_counts,
                         void *d_work, void *stream) {
    if (!rp) {
        set_error("demux_refine_dev: bad arguments");
        return WDX_ERR_INVALID;
    }
    wdx_seg_params pv;
    if (int e = refine_seg_params("demux_refine_dev", p, rp, &pv)) return e;
    return demux_dev_rows(ctx, DevRows(d_sig, d_row_off, d_row_len, stride, max_len, n_reads, d_a_start, d_a_end, d_ok), &pv, rp,
                          d_fpt, d_dwell, d_stats, d_refine_idx, d_status, d_dist, d_call, d_counts, d_work, stream);
}

int wdx_demux_refine_adc_dev(wdx_ctx *ctx, const wdx_adc_dev_in *in, int64_t max_len, int64_t n_reads,
                             const int32_t *d_a_start, const int32_t *d_a_end, const uint8_t *d_ok, const wdx_seg_params *p,
                             const wdx_refine_params *rp, double *d_fpt, int64_t *d_dwell, double *d_stats,
                             int32_t *d_refine_idx, int32_t *d_status, float *d_dist, int32_t *d_call, int64_t *d_counts,
                             void *d_work, void *stream) {
    if (!rp) {
        set_error("demux_refine_adc_dev: bad arguments");
        return WDX_ERR_INVALID;
    }
    if (int e = adc_dev_in_ok("demux_refine_adc_dev", in)) return e;
    wdx_seg_params pv;
    if (int e = refine_seg_params("demux_refine_adc_dev", p, rp, &pv)) return e;
    return demux_dev_rows(ctx, DevRows(in, max_len, n_reads, d_a_start, d_a_end, d_ok), &pv, rp, d_fpt, d_dwell, d_stats,
                          d_refine_idx, d_status, d_dist, d_call, d_counts, d_work, stream);
}

int wdx_calibrate_adc_dev(wdx_ctx *ctx, const int16_t *d_adc, const int64_t *d_row_off, const int32_t *d_row_len,
                          int64_t stride, int64_t n_reads, const float *d_offset, const float *d_scale, float *d_out,
                          void *stream) {
    if (n_reads < 0 || stride < 0 || stride > INT32_MAX || (n_reads > 0 && stride > 0 && (!d_adc || !d_out))) {
        set_error("calibrate_adc_dev: bad arguments");
        return WDX_ERR_INVALID;
    }
    if (n_reads > 0 && !d_row_len) {
        set_error("calibrate_adc_dev: int16 rows need row_len (there is no NaN tail to find a read's end by)");
        return WDX_ERR_INVALID;
    }
    if (n_reads > 0 && (!d_offset || !d_scale)) {
        set_error("calibrate_adc_dev: int16 rows need offset and scale of every read");
        return WDX_ERR_INVALID;
    }
    WDX_ENTER(ctx);
    if (n_reads == 0 || stride == 0) return WDX_SUCCESS;
    const AdcRows rows{d_adc, d_row_off, stride, d_row_len, d_offset, d_scale, d_out, nullptr, stride, nullptr};
    return launch_adc_rows(rows, n_reads, false, (hipStream_t)stream);
}

int wdx_host_alloc_on(int device, size_t bytes, void **out) {
    DeviceGuard guard(device);   // page-lock under the device that will read the buffer: no stray context on device 0
    if (guard.rc) return guard.rc;
    return wdx_host_alloc(bytes, out);
}

int wdx_host_alloc(size_t bytes, void **out) {
    if (!out) {
        set_error("host_alloc: null output");
        return WDX_ERR_INVALID;
    }
    *out = nullptr;
    hipError_t e = hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocPortable);
    if (e != hipSuccess) {
        set_error("hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        *out = nullptr;
        return e == hipErrorNoDevice ? WDX_ERR_NO_DEVICE : WDX_ERR_HIP;
    }
    return WDX_SUCCESS;
}

int wdx_host_register(void *p, size_t bytes) {
    if (!p || bytes == 0) {
        set_error("host_register: bad arguments");
        return WDX_ERR_INVALID;
    }
    WDX_HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterMapped | hipHostRegisterPortable));
    return WDX_SUCCESS;
}

int wdx_host_unregister(void *p) {
    if (!p) return WDX_SUCCESS;
    WDX_HIP_TRY(hipHostUnregister(p));
    return WDX_SUCCESS;
}

int wdx_host_free(void *p) {
    if (p) WDX_HIP_TRY(hipHostFree(p));
    return WDX_SUCCESS;
}

int wdx_dtw_last_launch(wdx_ctx *ctx, wdx_dtw_launch_info *info) {
    if (int e = check_ctx(ctx)) return e;
    if (!info) {
        set_error("dtw_last_launch: null output");
        return WDX_ERR_INVALID;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    *info = ctx->dtw_last;
    return WDX_SUCCESS;
}

int wdx_kernel_timing(wdx_ctx *ctx, int enable) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    ctx->timing = enable != 0;
    for (wdx_ctx *S : ctx->slots)   // pipelined minibatches are timed on their slot's events
        if (S) S->timing = ctx->timing;
    return WDX_SUCCESS;
}

int wdx_kernel_time(wdx_ctx *ctx, int kernel_id, double *total_ms, int64_t *launches) {
    WDX_ENTER(ctx);
    if (kernel_id < 0 || kernel_id >= kNumTimed) {
        set_error("kernel id out of range");
        return WDX_ERR_INVALID;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    double tot = 0.0;
    int64_t nl = 0;
    // the context's own launches and those of its pipeline slots (wdx_demux_submit enqueues on a slot's stream)
    wdx_ctx *all[1 + WDX_MAX_SLOTS] = {ctx};
    for (int k = 0; k < WDX_MAX_SLOTS; ++k) all[1 + k] = ctx->slots[k];
    for (wdx_ctx *c : all) {
        if (!c) continue;
        for (size_t i = 0; i < c->pending[kernel_id].size(); ++i) {
            auto &e = c->pending[kernel_id][i];
            WDX_HIP_TRY(hipEventSynchronize(e.second));
            float ms = 0;
            WDX_HIP_TRY(hipEventElapsedTime(&ms, e.first, e.second));
            c->acc_ms[kernel_id] += ms;
            c->launches[kernel_id] += c->pending_launches[kernel_id][i];
            c->pool.push_back(e);
        }
        c->pending[kernel_id].clear();
        c->pending_launches[kernel_id].clear();
        tot += c->acc_ms[kernel_id];
        nl += c->launches[kernel_id];
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = nl;
    return WDX_SUCCESS;
}

int wdx_kernel_time_reset(wdx_ctx *ctx) {
    WDX_ENTER(ctx);
    std::lock_guard<std::mutex> g(ctx->mu);
    wdx_ctx *all[1 + WDX_MAX_SLOTS] = {ctx};
    for (int k = 0; k < WDX_MAX_SLOTS; ++k) all[1 + k] = ctx->slots[k];
    for (wdx_ctx *c : all) {
        if (!c) continue;
        for (int k = 0; k < kNumTimed; ++k) {
            for (auto &e : c->pending[k]) {
                (void)hipEventSynchronize(e.second);
                c->pool.push_back(e);
            }
            c->pending[k].clear();
            c->pending_launches[k].clear();
            c->acc_ms[k] = 0;
            c->launches[k] = 0;
        }
    }
    return WDX_SUCCESS;
}

int wdx_selftest_score_dev(wdx_ctx *ctx, const double *d_dm, const double *d_vs, int64_t n, double *d_fast,
                           double *d_ref, void *stream) {
    WDX_ENTER(ctx);
    if (n < 0 || (n > 0 && (!d_dm || !d_vs || !d_fast || !d_ref))) {
        set_error("selftest_score_dev: bad arguments");
        return WDX_ERR_INVALID;
    }
    return launch_score_selftest(d_dm, d_vs, n, d_fast, d_ref, (hipStream_t)stream);
}

int wdx_selftest_optimal_cpts_dev(wdx_ctx *ctx, const double *d_x, const int64_t *d_off, int64_t n_series, int32_t n_bkps,
                                  int32_t min_size, int64_t max_len, int32_t max_slots, int32_t *d_cpts, int32_t *d_status,
                                  void *stream) {
    WDX_ENTER(ctx);
    if (n_series < 0 || n_bkps < 1 || n_bkps > 253 || max_len < 0 || max_len > WDX_MAX_ADAPTER_SAMPLES || max_slots < 0 ||
        (n_series > 0 && (!d_x || !d_off || !d_cpts || !d_status))) {
        set_error("selftest_optimal_cpts_dev: bad arguments");
        return WDX_ERR_INVALID;
    }
    if (min_size < 1) {
        set_error("optimal change-points: min_size must be >= 1");
        return WDX_ERR_UNSUPPORTED;
    }
    if (n_series == 0) return WDX_SUCCESS;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (int rc = use_stream(ctx, (hipStream_t)stream)) return rc;
    const OptimalPlan pl = plan_refine_optimal(n_series, max_len, n_bkps, max_slots);
    if (int rc = ctx->fp_opt.ensure(pl.bytes)) return rc;
    return launch_optimal_cpts_selftest(d_x, d_off, n_series, n_bkps, min_size, d_cpts, d_status, pl, ctx->fp_opt.p,
                                        (hipStream_t)stream);
}

int wdx_selftest_clip_dev(wdx_ctx *ctx, const float *d_sig, const int64_t *d_row_off, int64_t stride, int64_t n_reads,
                          const int32_t *d_a_start, const int32_t *d_a_end, const wdx_seg_params *p, int32_t cap,
                          void *d_rec, void *stream) {
    WDX_ENTER(ctx);
    if (n_reads < 0 || !p || (n_reads > 0 && (!d_sig || !d_a_start || !d_a_end || !d_rec)) ||
        (cap != 4096 && cap != 5120 && cap != 6144 && cap != 8192 && cap != 13312)) {
        set_error("selftest_clip_dev: bad arguments");
        return WDX_ERR_INVALID;
    }
    if (n_reads == 0) return WDX_SUCCESS;
    return launch_clip_bounds_selftest(d_sig, d_row_off, stride, n_reads, d_a_start, d_a_end, *p, cap, d_rec,
                                       (hipStream_t)stream);
}

int wdx_calib_read_dev(wdx_ctx *ctx, const float *d_p, int64_t n, float *d_out, void *stream) {
    WDX_ENTER(ctx);
    return launch_calib_read(d_p, n, d_out, (hipStream_t)stream);
}

int wdx_synth_lengths_dev(wdx_ctx *ctx, uint64_t seed, int64_t first_read, int64_t n_reads,
                          int32_t n_barcodes, const int32_t *d_dwell_table, int64_t *d_len,
                          void *stream) {
    WDX_ENTER(ctx);
    return launch_synth_lengths(seed, first_read, n_reads, n_barcodes, d_dwell_table, d_len,
                                (hipStream_t)stream);
}

int wdx_synth_fill_dev(wdx_ctx *ctx, uint64_t seed, int64_t first_read, int64_t n_reads,
                       int32_t n_barcodes, int32_t n_bc_events, float noise_scale, int32_t spikes,
                       const int32_t *d_dwell_table, const float *d_lead, const float *d_bc,
                       const int64_t *d_off, float *d_sig, int32_t *d_barcode, void *stream) {
    WDX_ENTER(ctx);
    return launch_synth_fill(seed, first_read, n_reads, n_barcodes, n_bc_events, noise_scale, spikes,
                             d_dwell_table, d_lead, d_bc, d_off, d_sig, d_barcode,
                             (hipStream_t)stream);
}

}  // extern "C"

// ---- nearest-reference calls with reference labels, margin and rejection (include/wdx.h) ------------------------------

int wdx::demux_nearest_dev_rows(wdx_ctx *ctx, const DevRows &rows, const wdx_seg_params *p, double *d_fpt, int64_t *d_dwell,
                                double *d_stats, int32_t *d_status, const NearestArgs &N, float *d_dist, int64_t *d_counts,
                                void *d_work, void *stream) {
    WDX_ENTER(ctx);
    if (rows.f32.n_reads < 0 || !p ||
        (rows.f32.n_reads > 0 && (rows.missing() || !rows.f32.a_start || !rows.f32.a_end || !d_status || !N.call || !d_work))) {
        set_error("demux_nearest_dev: bad arguments");
        return WDX_ERR_INVALID;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    DtwRefs &R = ctx->refs;
    if ((rc = nearest_args_ok("demux_nearest_dev", R, N.label != nullptr, N.n_labels))) return rc;
    const int64_t K = p->barcode_num_events;
    if ((rc = check_ref_length(R, *p))) return rc;
    if (dtw_plan(rows.f32.n_reads, R.nY, R.L, R.window, true, DtwEntry::kFused, ctx->knobs.dtw_switches()).unsupported) {
        set_error("demux_nearest_dev needs window <= %d", kMaxRegWindow);
        return WDX_ERR_UNSUPPORTED;
    }
    if (rows.f32.n_reads == 0) return WDX_SUCCESS;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = use_stream(ctx, s))) return rc;
    unsigned char *w = (unsigned char *)d_work;
    return for_each_slice(ctx, rows, false, p->padding, s, [&](const FpReads &in, int64_t r0) {
        const int64_t n_reads = in.n_reads;
        double *fpt = d_fpt ? d_fpt + r0 * K : (double *)w;
        // (the read-minor copy of a small slice lives in the context's own blocks here: d_work holds the fingerprints and the
        // fingerprint workspace, which wdx_demux_workspace_bytes covers for every n_reads)
        const DemuxWork W = demux_work_layout(n_reads, K, false);
        if (int e = fingerprint_stage(ctx, in, *p, FpOut{fpt, from_read(d_dwell, r0, K), from_read(d_stats, r0, 6), d_status + r0},
                                      w + W.fp_ws, s))
            return e;
        NearestArgs Ns = N.from(r0);
        Ns.status = d_status + r0;
        return nearest_rows_vs_refs(ctx, fpt, n_reads, DtwEntry::kFused, Ns, from_read(d_dist, r0, R.nY), d_counts, s);
    });
}

extern "C" {

int wdx_nearest_dev(wdx_ctx *ctx, const double *dX, int64_t nX, const int32_t *d_status, const int32_t *d_ref_label,
                    int64_t n_labels, const float *d_min_margin, const float *d_max_dist, float *d_dist, int32_t *d_call,
                    float *d_best, int64_t *d_counts, void *stream) {
    WDX_ENTER(ctx);
    if (nX < 0 || (nX > 0 && (!dX || !d_call))) {
        set_error("nearest_dev: bad arguments");
        return WDX_ERR_INVALID;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    if ((rc = nearest_args_ok("nearest_dev", ctx->refs, d_ref_label != nullptr, n_labels))) return rc;
    if (nX == 0) return WDX_SUCCESS;
    if ((rc = use_stream(ctx, (hipStream_t)stream))) return rc;
    const NearestArgs N{d_ref_label, (int32_t)n_labels, d_min_margin, d_max_dist, d_status, d_call, d_best};
    return nearest_rows_vs_refs(ctx, dX, nX, DtwEntry::kMatrix, N, d_dist, d_counts, (hipStream_t)stream);
}

int wdx_demux_nearest_dev(wdx_ctx *ctx, const float *d_sig, const int64_t *d_row_off, const int32_t *d_row_len, int64_t stride,
                          int64_t max_len, int64_t n_reads, const int32_t *d_a_start, const int32_t *d_a_end, const uint8_t *d_ok,
                          const wdx_seg_params *p, double *d_fpt, int64_t *d_dwell, double *d_stats, int32_t *d_status,
                          const int32_t *d_ref_label, int64_t n_labels, const float *d_min_margin, const float *d_max_dist,
                          float *d_dist, int32_t *d_call, float *d_best, int64_t *d_counts, void *d_work, void *stream) {
    const NearestArgs N{d_ref_label, (int32_t)(n_labels >= 1 && n_labels <= INT32_MAX ? n_labels : 0), d_min_margin, d_max_dist, nullptr,
                        d_call, d_best};
    return demux_nearest_dev_rows(ctx, DevRows(d_sig, d_row_off, d_row_len, stride, max_len, n_reads, d_a_start, d_a_end, d_ok), p,
                                  d_fpt, d_dwell, d_stats, d_status, N, d_dist, d_counts, d_work, stream);
}

int wdx_dtw_nearest(wdx_ctx *ctx, const double *X, int64_t nX, const int32_t *ref_label, int64_t n_labels, const float *min_margin,
                    const float *max_dist, float *dist, int32_t *call, float *best) {
    WDX_ENTER(ctx);
    if (nX < 0 || (nX > 0 && (!X || !call || !best))) {
        set_error("dtw_nearest: bad arguments");
        return WDX_ERR_INVALID;
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    const DtwRefs &R = ctx->refs;
    if ((rc = nearest_args_ok("dtw_nearest", R, ref_label != nullptr, n_labels))) return rc;
    if (ref_label)
        for (int64_t c = 0; c < R.nY; ++c)
            if (ref_label[c] < 0 || ref_label[c] >= n_labels) {
                set_error("dtw_nearest: the label of reference %lld is %d, outside 0 .. %lld", (long long)c, (int)ref_label[c],
                          (long long)n_labels - 1);
                return WDX_ERR_INVALID;
            }
    if (nX == 0) return WDX_SUCCESS;
    hipStream_t s = ctx->stream;
    if ((rc = use_stream(ctx, s))) return rc;
    const size_t xb = (size_t)(nX * R.L) * sizeof(double), ob = (size_t)(nX * R.nY) * sizeof(float);
    const size_t lb = (size_t)R.nY * sizeof(int32_t), tb = (size_t)n_labels * sizeof(float);
    if ((rc = ctx->in0.ensure(xb))) return rc;
    if (ref_label && (rc = ctx->in1.ensure(lb))) return rc;
    if (min_margin && (rc = ctx->in2.ensure(tb))) return rc;
    if (max_dist && (rc = ctx->in3.ensure(tb))) return rc;
    if (dist && (rc = ctx->out0.ensure(ob))) return rc;
    if ((rc = ctx->out1.ensure((size_t)nX * sizeof(int32_t)))) return rc;
    if ((rc = ctx->out2.ensure((size_t)nX * 2 * sizeof(float)))) return rc;
    StreamDrain drain(s);
    WDX_HIP_TRY(hipMemcpyAsync(ctx->in0.p, X, xb, hipMemcpyHostToDevice, s));
    if (ref_label) WDX_HIP_TRY(hipMemcpyAsync(ctx->in1.p, ref_label, lb, hipMemcpyHostToDevice, s));
    if (min_margin) WDX_HIP_TRY(hipMemcpyAsync(ctx->in2.p, min_margin, tb, hipMemcpyHostToDevice, s));
    if (max_dist) WDX_HIP_TRY(hipMemcpyAsync(ctx->in3.p, max_dist, tb, hipMemcpyHostToDevice, s));
    const NearestArgs N{ref_label ? (const int32_t *)ctx->in1.p : nullptr, (int32_t)n_labels,
                        min_margin ? (const float *)ctx->in2.p : nullptr, max_dist ? (const float *)ctx->in3.p : nullptr, nullptr,
                        (int32_t *)ctx->out1.p, (float *)ctx->out2.p};
    if ((rc = nearest_rows_vs_refs(ctx, (const double *)ctx->in0.p, nX, DtwEntry::kMatrix, N, dist ? (float *)ctx->out0.p : nullptr,
                                   nullptr, s)))
        return rc;
    if (dist) WDX_HIP_TRY(hipMemcpyAsync(dist, ctx->out0.p, ob, hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipMemcpyAsync(call, ctx->out1.p, (size_t)nX * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipMemcpyAsync(best, ctx->out2.p, (size_t)nX * 2 * sizeof(float), hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipStreamSynchronize(s));
    drain.done();
    return WDX_SUCCESS;
}

}  // extern "C"
