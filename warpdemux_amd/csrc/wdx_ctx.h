// The opaque context behind include/wdx.h's wdx_ctx (internal; shared by wdx_api.hip, wdx_minibatch.hip,
// wdx_chain.hip, wdx_classify.hip, wdx_comm.hip and wdx_live.hip).  Nothing here computes results.
#pragma once
#include "wdx_common.h"
#include "wdx_refine_args.h"
#include "wdx_stage_plan.h"

#include <mutex>
#include <utility>
#include <vector>

// kept out of the library's dynamic symbol table
#define WDX_INTERNAL __attribute__((visibility("hidden")))

namespace wdx {

struct Buffer {  // grow-only device workspace
    void *p = nullptr;
    size_t bytes = 0;
    // exact: allocate `need` bytes and no head-room (a block whose size is a stated bound: the int16 shards' staging)
    int ensure(size_t need, bool exact = false);
    void release();
};

// A classifier model resident on the device (wdx_classify.hip: install): ONE block that holds its image
// (wdx_model_image.h) and the kernels' record bound to that block.  Block, record and flag change together, with the device
// idle; gen counts the changes.
template <class Dev>
struct Resident {
    Buffer block;
    Dev dev{};
    bool set = false;
    int64_t gen = 0;
};
struct ResidentSvm : Resident<SvmDev> {
    SvmFused fused{};  // the fused route's tables, in the same block
};

struct PinnedBuffer {  // grow-only page-locked host staging area
    void *p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need);
    void release();
};

constexpr int kNumTimed = 22;

struct MedoidStage {   // a page-locked block and the event behind the latest copy out of it
    void *host = nullptr;
    size_t bytes = 0;
    hipEvent_t copied = nullptr;
};

// RAII: make the context's device current for the duration of one entry point and put the caller's
// device back afterwards (a host thread that also drives torch must not find its device switched).
struct DeviceGuard {
    int prev = -1;
    int rc = WDX_SUCCESS;
    explicit DeviceGuard(int device);
    ~DeviceGuard();
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

struct Comm;  // wdx_comm.hip: RCCL communicator + the dlopen'ed entry points

}  // namespace wdx

struct wdx_ctx {
    int device = 0;
    std::mutex mu;
    hipStream_t stream = nullptr;  // the context's own non-blocking stream: every host-buffer call runs on it
    hipStream_t last_stream = nullptr;  // stream of the latest enqueue that used the shared workspaces
    bool last_stream_valid = false;
    wdx::Knobs knobs;
    wdx::DtwRefs refs;
    wdx_dtw_launch_info dtw_last{};  // what the latest DTW dispatch launched (wdx_dtw_last_launch)
    wdx::Buffer refs_pad, refs_T, refs_nan;
    // host-buffer call workspaces
    wdx::Buffer in0, in1, in2, in3, out0, out1, out2, out3, tmp0, tmp1, tmp2, scratch, fp_ws, ref_buf;
    wdx::Buffer ref_ws;  // refinement branch: the fast kernels' hand-over records (fingerprint_refine_ws_bytes)
    wdx::Buffer fp_big;  // score curves of adapter windows beyond the exact kernel's LDS capacity (fingerprint_big_bytes)
    // WDX_OPT_LONG_WINDOWS: slots of the long form (fingerprint_long_bytes: 12 MB), allocated by the first call that meets a
    // window beyond WDX_MAX_ADAPTER_SAMPLES with the option on -- never otherwise.  A pipeline slot owns its own: 96 MB for 8
    wdx::Buffer fp_long;
    // WDX_OPT_REFINE_OPTIMAL_CPTS: scratch of fingerprint_refine_optimal_kernel (fingerprint_optimal_bytes: at most 256 MiB),
    // allocated by the first refining call with the option on -- never otherwise
    wdx::Buffer fp_opt;
    wdx::PinnedBuffer pin_in, pin_out;  // staging of small (live-tick sized) host-buffer calls
    std::vector<double> ref_query_host;  // the consensus query resident in ref_buf (refine_prepare uploads on change)
    wdx::Buffer pk_idx;       // packed staging of a page-locked minibatch: window offsets / first columns / shifted bounds
    wdx::PinnedBuffer pk_host;  // ... and their host images (kept until the slot's copy has run)
    wdx::Buffer in_adc;       // int16 ADC rows as they arrived by DMA copy, ahead of decode_adc_kernel (wdx_adc.hip)
    // float32 staging of an int16 DEVICE shard, one slice at a time (wdx_adc_dev.h: rows, then the slice's shifted bounds and
    // packed lengths); reused in stream order by every slice and every *_adc_dev call
    wdx::Buffer adc_stage;
    // distances of one row block of a nearest-reference call that asked for no `dist` and whose rule runs behind the DTW
    // kernels (wdx_dtw_plan.h: nearest_plan, at most kNearestBlockBytes); allocated by the first such call
    wdx::Buffer nearest_buf;
    // per-label medoids (wdx_medoid.hip): the workspace wdx_medoid_plan.h lays out, allocated by the first such call; and the
    // page-locked images of the tables a call uploads.  A call returns with its copy pending, so the next call takes a block
    // whose copy has run (its event has fired) or allocates another; blocks are freed only when a larger one is needed and at
    // the context's end -- hipHostMalloc / hipHostFree wait for the device, and a call in the steady state must not
    wdx::Buffer medoid_ws;
    // the self-distance matrix (wdx_dtw_self.hip): the workspace wdx_self_plan.h lays out, allocated by the first such call
    wdx::Buffer self_ws;
    // leave-one-out nearest neighbours (wdx_dtw_loo.hip): the workspace wdx_loo_plan.h lays out, allocated by the first such call
    wdx::Buffer loo_ws;
    // barycenter steps (wdx_dba.hip): the workspace wdx_dba_plan.h lays out (its tables go through the medoid calls' staged blocks)
    wdx::Buffer dba_ws;
    // the batched SMO solve (wdx_svm_fit.hip): the tables wdx_svm_fit_plan.h lays out (uploaded through the medoid calls' staged blocks)
    wdx::Buffer svm_fit_ws;
    // the MLP trainer (wdx_mlp_fit.hip): the workspace wdx_mlp_fit_plan.h lays out, allocated by the first fit
    wdx::Buffer mlp_fit_ws;
    // the Fpt_Boost trainer (wdx_boost_fit.hip): the workspace wdx_boost_fit_plan.h lays out, allocated by the first fit
    wdx::Buffer boost_fit_ws;
    // accuracy thresholds (wdx_thresholds.hip): the histograms and the skipped count a caller did not ask for (wdx_thresholds_plan.h)
    wdx::Buffer thr_ws;
    // out-of-fold probabilities (wdx_svm_cv.hip): the tables of a call (uploaded through the medoid calls' staged blocks)
    wdx::Buffer svm_cv_ws;
    std::vector<wdx::MedoidStage> medoid_staged;
    int64_t refs_gen = 0;  // bumped whenever the resident reference set (samples or window/penalty) changes
    // the classifier tails (wdx_svm_set_model, wdx_mlp_set_model, wdx_boost_set_model): a slot each, independent of one another
    wdx::ResidentSvm svm;
    wdx::Resident<wdx::MlpDev> mlp;
    wdx::Resident<wdx::BoostDev> boost;
    // fused DTW + SVM path of wdx_demux_svm_dev: the resident references gathered into support-vector order (rebuilt when
    // the reference set or the model changes: refs_gen, svm.gen)
    wdx::Buffer svm_refs;
    int64_t svm_refs_gen = -1, svm_refs_model_gen = -1;
    wdx::Comm *comm = nullptr;
    // pipelined minibatches (wdx_demux_submit / wdx_demux_wait): up to WDX_MAX_SLOTS child contexts, each with its own stream and
    // workspaces, sharing this context's resident reference set; the fields below describe a child's batch in flight
    wdx_ctx *slots[WDX_MAX_SLOTS] = {};
    bool slot_busy = false, slot_waiting = false;
    uint32_t slot_want = 0;   // WDX_WANT_* of the batch in flight
    wdx::OutPlan slot_plan;   // ... and what it hands back: the pieces of the slot's page-locked block (wdx_stage_plan.h)
    wdx::Buffer mb_dwell, mb_stats, mb_prob, mb_pred, mb_conf;  // device side of the optional minibatch outputs
    // a refine minibatch (wdx_demux_submit_refine; wdx_fingerprint_refine_batch on the context itself): its refine_idx on the
    // device; the consensus query lives in its own ref_buf / ref_query_host, the records in ref_ws
    wdx::Buffer mb_ridx;
    // timing
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending[wdx::kNumTimed];
    std::vector<int64_t> pending_launches[wdx::kNumTimed];
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    double acc_ms[wdx::kNumTimed] = {};
    int64_t launches[wdx::kNumTimed] = {};
};

namespace wdx {

struct Timed {  // RAII: hipEvents around one kernel launch when timing is on
    wdx_ctx *c;
    int id;
    hipStream_t s;
    std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
    int64_t n_launches = 0;  // kernel launches bracketed by this event pair (0 -> counted as 1)
    MainEvents main;         // WDX_K_FINGERPRINT only: a second pair around the main fast-kernel launches alone
    Timed(wdx_ctx *c_, int id_, hipStream_t s_);
    ~Timed();
};

// Entry-point prologue: null check.  (The device is made current by a DeviceGuard in the caller.)
int check_ctx(wdx_ctx *ctx);
// The shared workspaces of a context are ordered by stream order only.  Call with the mutex held before
// enqueueing on `s`: when the previous user enqueued on a different stream, wait for that stream first.
int use_stream(wdx_ctx *ctx, hipStream_t s);
void comm_destroy(wdx_ctx *ctx);
// (wdx_api.hip) with the context's mutex held:
// (re)build the resident reference set from a HOST array (content-hashed: uploads only on change)
int set_refs_locked(wdx_ctx *ctx, const double *Y, int64_t nY, int64_t L, int32_t window, double penalty,
                    hipStream_t stream);
// DTW of device rows dX (nX, L) against the resident refs -> d_out (nX, nY) [+ argmin]
int dtw_dev_locked(wdx_ctx *ctx, const double *dX, int64_t nX, float *d_out, int32_t *d_argmin,
                   hipStream_t stream);
// (wdx_medoid.hip) frees the page-locked table blocks whose copies have run (all: waits for each; wdx_ctx_destroy calls that)
void medoid_release_staged(wdx_ctx *ctx, bool all);
// (wdx_medoid.hip) a page-locked block of `bytes` whose previous copy has run; the caller fills it, enqueues its copy and records
// `copied` behind it (wdx_dba.hip uploads its tables the same way)
int medoid_stage_block(wdx_ctx *ctx, size_t bytes, MedoidStage **out);
// (wdx_api.hip) behind a DTW launch when a resident reference holds an infinite sample (R.any_inf): pairs with the same
// infinity at one index are NaN in the reference and +inf out of the kernels -- settled here, then the argmin again (a NaN
// wins its row)
WDX_INTERNAL int dtw_settle_inf(const DtwRefs &R, const double *dX, int64_t nX, float *d_out, int32_t *d_argmin,
                                hipStream_t stream);

// (wdx_api.hip) The fingerprint stage as every entry point but the profiling one runs it: `B` (the context, or the
// pipeline slot that owns the stream) supplies fp_big (and fp_long) for max_len, the knobs and the WDX_K_FINGERPRINT event scope.
// main_events = false leaves the main / clip / tail kernel pairs unrecorded (they go back to the pool):
// wdx_fingerprint_refine_dev, the host-batch call (wdx_minibatch.hip: fingerprint_batch_impl) and wdx_live_tick have never
// recorded them.  Kept as found: neither DESIGN.md nor DESIGN_HISTORY.md gives a reason.
int fingerprint_stage(wdx_ctx *B, const FpReads &in, const wdx_seg_params &p, const FpOut &out, void *d_ws,
                      hipStream_t s, const RefineDev *rf = nullptr, bool main_events = true);
// (wdx_api.hip) The refinement branch's device state for n_reads reads on stream s (see its definition); *rf is freed by
// the caller's RefineDevGuard
struct RefineDevGuard {   // frees what fill_refine_dev made (launch_fingerprint copies it into the kernels' arguments)
    RefineDev *&r;
    ~RefineDevGuard() { free_refine_dev(r); }
};
int refine_prepare(wdx_ctx *B, const wdx_refine_params &rp, int64_t n_reads, int32_t *d_idx, void *d_ws, hipStream_t s,
                   RefineDev **rf);
// (wdx_api.hip) "barcode_num_events != reference length" check of every entry that fingerprints and then runs the DTW
int check_ref_length(const DtwRefs &R, const wdx_seg_params &p);
// (wdx_work_layout.h) demux_work_layout: byte offsets of the pieces of a caller's d_work, and its size
// (wdx_classify.hip) SVM tail on a device distance block (n, n_train) under WDX_K_SVM; with d_status (nullable) the
// failed reads are masked right behind it: pred -1, NaN probabilities (the reference never shows them to the model)
int svm_tail(wdx_ctx *B, const SvmDev &M, const float *d_dist, int64_t n, const int32_t *d_status, double *d_prob,
             int32_t *d_pred, double *d_conf, hipStream_t s);
// (wdx_classify.hip) boost tail on device fingerprint rows (n, M.n_features) under WDX_K_BOOST, with B's knobs; the kernel
// masks the reads whose d_status (nullable) is not 0 itself
int boost_tail(wdx_ctx *B, const BoostDev &M, const double *d_fpt, const int32_t *d_status, int64_t n, double *d_raw,
               double *d_prob, int32_t *d_pred, double *d_conf, hipStream_t s);

// (wdx_chain.hip) "Is this model usable here": a DTW tail has its reference set and the tail's model is resident
// (WDX_ERR_NO_REFS otherwise), and the model fits -- the SVM was trained on nY references, the MLP takes nY inputs, the boost
// model K features (WDX_ERR_INVALID otherwise; refined: K is rp->barcode_keep_events and is named so).  tail: WDX_LIVE_TAIL_*.
WDX_INTERNAL int tail_ready(const wdx_ctx *ctx, int tail, int64_t nY, int64_t K, bool refined, const char *who);

// (wdx_chain.hip) The device chain of the host minibatches, the live tick and wdx_demux_boost_dev, enqueued on s:
//   [refine_prepare]  with rp: d_refine_idx (nullable) = -1, the hand-over records in d_refine_ws (null: B->ref_ws) reset
//   fingerprint stage on rd into out.fp, workspace d_fp_ws
//   [DTW + call]      when R.nY > 0: out.dist (n, nY), out.call, out.counts (nullable)
//   [tail]            SVM / MLP on out.dist (without a reference, R.nY == 0, their outputs are left alone), boost on out.fp.fpt;
//                     failed reads: pred -1, NaN prob / conf
// It sizes no buffer and copies nothing to the host.  `B` owns the stream's workspaces, the knobs and the event scopes.
struct ChainTail {
    int kind = WDX_LIVE_TAIL_NONE;   // WDX_LIVE_TAIL_*, and the model of that kind
    const SvmDev *svm = nullptr; const MlpDev *mlp = nullptr; const BoostDev *boost = nullptr;
};
struct ChainOut {
    FpOut fp;
    float *dist = nullptr; int32_t *call = nullptr; int64_t *counts = nullptr;   // dist / call: null when no DTW runs
    double *raw = nullptr, *prob = nullptr, *conf = nullptr; int32_t *pred = nullptr;
    int64_t *n_nonfinite = nullptr;   // MLP tail: zeroed, then counted into
};
WDX_INTERNAL int demux_chain(wdx_ctx *B, const DtwRefs &R, const FpReads &rd, const wdx_seg_params &p, const wdx_refine_params *rp,
                int32_t *d_refine_idx, void *d_refine_ws, void *d_fp_ws, bool main_events, const ChainTail &tail,
                const ChainOut &out, hipStream_t s);

// The rows of a device-resident entry as it got them -- what the float32 entries and their *_adc_dev twins hand to ONE body:
// float32 rows (`f32` whole), or an int16 shard (`adc` non-null; of f32 only max_len, n_reads, a_start, a_end and ok are
// read).  for_each_slice gives the body the reads as the chain takes them and the number of the first one: the float32
// rows in one piece, the shard slice by slice from the context's staging block (wdx_adc_dev.h).
struct DevRows {
    FpReads f32;
    const wdx_adc_dev_in *adc = nullptr;
    DevRows(const float *d_sig, const int64_t *d_row_off, const int32_t *d_row_len, int64_t stride, int64_t max_len,
            int64_t n_reads, const int32_t *d_a_start, const int32_t *d_a_end, const uint8_t *d_ok)
        : f32{d_sig, d_row_off, d_row_len, stride, max_len, n_reads, d_a_start, d_a_end, d_ok} {}
    DevRows(const wdx_adc_dev_in *in, int64_t max_len, int64_t n_reads, const int32_t *d_a_start, const int32_t *d_a_end,
            const uint8_t *d_ok)
        : f32{nullptr, nullptr, nullptr, 0, max_len, n_reads, d_a_start, d_a_end, d_ok}, adc(in) {}
    // n_reads > 0 and no samples to read: the entry's "bad arguments"
    bool missing() const { return adc ? !adc->adc || !adc->row_len || !adc->offset || !adc->scale : !f32.sig; }
};
// (wdx_api.hip) the shard descriptor of an *_adc_dev entry is there and names a layout ("<who>: bad arguments" otherwise)
int adc_dev_in_ok(const char *who, const wdx_adc_dev_in *in);
// (wdx_api.hip) the slices of a call on this context (its slice option, the longest window of its branch) ...
AdcDevPlan adc_dev_plan_for(const wdx_ctx *ctx, int64_t n_reads, int64_t max_len, bool refine);
// ... and reads r0 .. r0 + m - 1 of the shard decoded into B->adc_stage (already sized) on s; *rd = the slice for the chain
int adc_dev_stage(wdx_ctx *B, const DevRows &rows, const AdcDevPlan &plan, bool refine, int64_t padding, int64_t r0, int64_t m,
                  hipStream_t s, FpReads *rd);
// With the context's mutex held, after use_stream(B, s).  body(const FpReads &, int64_t r0) -> int.
template <class Body>
int for_each_slice(wdx_ctx *B, const DevRows &rows, bool refine, int64_t padding, hipStream_t s, Body body) {
    if (!rows.adc) return body(rows.f32, (int64_t)0);
    const AdcDevPlan plan = adc_dev_plan_for(B, rows.f32.n_reads, rows.f32.max_len, refine);
    if (plan.n_slices == 0) return WDX_SUCCESS;
    if (int rc = B->adc_stage.ensure((size_t)plan.staging_bytes, true)) return rc;   // never beyond the budget
    for (int64_t k = 0; k < plan.n_slices; ++k) {
        FpReads rd;
        const int64_t r0 = k * plan.slice_reads, m = k + 1 < plan.n_slices ? plan.slice_reads : plan.last_reads;
        if (int rc = adc_dev_stage(B, rows, plan, refine, padding, r0, m, s, &rd)) return rc;
        if (int rc = body(rd, r0)) return rc;
    }
    return WDX_SUCCESS;
}
// an output of `cols` values per read, from read r0 on (null stays null)
template <class T>
inline T *from_read(T *p, int64_t r0, int64_t cols = 1) { return p ? p + r0 * cols : nullptr; }

// (wdx_api.hip / wdx_classify.hip) The device-resident entries behind their argument lists: the float32 entry and its
// *_adc_dev twin call the same function with their DevRows.
int fingerprint_dev_rows(wdx_ctx *ctx, const DevRows &rows, const wdx_seg_params *p, double *d_fpt, int64_t *d_dwell,
                         double *d_stats, int32_t *d_status, void *stream);
int fingerprint_refine_dev_rows(wdx_ctx *ctx, const DevRows &rows, const wdx_seg_params *p_in, const wdx_refine_params *rp,
                                double *d_fpt, int64_t *d_dwell, double *d_stats, int32_t *d_refine_idx, int32_t *d_status,
                                void *stream);
int demux_dev_rows(wdx_ctx *ctx, const DevRows &rows, const wdx_seg_params *p, const wdx_refine_params *rp, double *d_fpt,
                   int64_t *d_dwell, double *d_stats, int32_t *d_refine_idx, int32_t *d_status, float *d_dist, int32_t *d_call,
                   int64_t *d_counts, void *d_work, void *stream);
// (wdx_api.hip) wdx_demux_nearest_dev: demux_dev_rows without the refinement branch, the nearest-reference rule in the argmin's place
int demux_nearest_dev_rows(wdx_ctx *ctx, const DevRows &rows, const wdx_seg_params *p, double *d_fpt, int64_t *d_dwell,
                           double *d_stats, int32_t *d_status, const NearestArgs &N, float *d_dist, int64_t *d_counts, void *d_work,
                           void *stream);
int demux_svm_dev_rows(wdx_ctx *ctx, const DevRows &rows, const wdx_seg_params *p, double *d_fpt, int32_t *d_status,
                       float *d_dist, double *d_prob, int32_t *d_pred, double *d_conf, void *d_work, int64_t block_rows,
                       void *stream);
int demux_mlp_dev_rows(wdx_ctx *ctx, const DevRows &rows, const wdx_seg_params *p, double *d_fpt, int32_t *d_status,
                       float *d_dist, double *d_prob, int32_t *d_pred, double *d_conf, int64_t *d_n_nonfinite, void *d_work,
                       int64_t block_rows, void *stream);
int demux_boost_dev_rows(wdx_ctx *ctx, const DevRows &rows, const wdx_seg_params *p, const wdx_refine_params *rp,
                         double *d_fpt, int32_t *d_refine_idx, int32_t *d_status, double *d_raw, double *d_prob,
                         int32_t *d_pred, double *d_conf, void *d_work, void *stream);

}  // namespace wdx

// Host-buffer entry points enqueue copies from/to the CALLER's (or the context's page-locked) memory and
// synchronise once at the end.  A failure half way must not return while such a copy may still be in flight
// (the caller frees or rewrites its buffers; PinnedBuffer::ensure may hipHostFree the staging block on the next
// call): every exit of the enqueue region drains the stream unless the normal final synchronisation already ran.
struct StreamDrain {
    hipStream_t s;
    bool armed = true;
    explicit StreamDrain(hipStream_t s_) : s(s_) {}
    void done() { armed = false; }
    ~StreamDrain() {
        if (armed) (void)hipStreamSynchronize(s);  // best effort: the error already recorded is the one reported
    }
};

#define WDX_ENTER(ctx)                                  \
    if (int _e = ::wdx::check_ctx(ctx)) return _e;      \
    ::wdx::DeviceGuard _guard((ctx)->device);           \
    if (_guard.rc) return _guard.rc;                    \
    int rc = WDX_SUCCESS;                               \
    (void)rc
