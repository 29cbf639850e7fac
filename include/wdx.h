/*
 * wdx.h -- C ABI of libwdx_hip.so, the MI355X (gfx950) engine for the WarpDemuX
 *          sig_proc / parallel_distances hot path.
 *
 * Plain pointers and sizes only; no torch / numpy / HIP types.  Paths below are relative to the
 * reference tree (KleistLab/WarpDemuX v1.0.0).
 *
 * Two families of entry points:
 *   - HOST-BUFFER calls  (wdx_dtw_matrix, wdx_fingerprint_batch, ...): the caller owns every
 *     buffer (NumPy arrays); the library copies in/out and keeps nothing but the opaque context.
 *     These are what a ctypes binding inside warpdemux.parallel_distances / warpdemux.sig_proc
 *     would call.
 *   - DEVICE-RESIDENT calls (*_dev): every data pointer is a HIP device pointer on the context's
 *     device, `stream` is a hipStream_t passed as void* (NULL = default stream).  They enqueue
 *     work and return without synchronising.  Used by the fused pipeline and by bench.py.
 *
 * All functions return WDX_SUCCESS (0) or a negative WDX_ERR_* code; wdx_last_error() gives the
 * message for the calling thread.  Per-read soft failures are reported in status[] exactly like
 * the reference's ReadResult.success / fail_reason (sig_proc.py:26-62) and never fail the call.
 *
 * Threading: a context may be used from several threads (entry points serialise on it); create
 * one context per thread/stream for concurrency (live_balancing/session.py:162-169 runs thread pools):
 * every context owns a non-blocking HIP stream on which all of its host-buffer calls run, so calls
 * through different contexts overlap on the device.  The workspaces of a context are ordered by stream
 * order; when consecutive calls on one context name different streams the library waits for the earlier
 * stream first.  Streams, as tests/test_gpu_streams.py holds them:
 *   - A context may be used from any stream of its device -- the NULL stream, the context's own, a caller's non-blocking
 *     ones -- one call at a time; a *_dev call reads its inputs and writes its outputs in the order of the stream it was
 *     given and returns without waiting for it (test_late_inputs_on_one_side_stream).
 *   - When a call names another stream than the call before it on the same context, everything enqueued on the earlier
 *     stream has finished before the new call's work touches the context's workspaces
 *     (test_two_streams_share_one_context).
 *   - A setter (wdx_set_refs, wdx_svm_set_model, wdx_mlp_set_model, wdx_boost_set_model) may be called with work pending,
 *     on a caller's stream or in a minibatch slot: that work finishes with the state it was enqueued with, later calls
 *     see the new one (test_resident_state_replaced_behind_pending_work,
 *     test_minibatch_in_flight_keeps_what_it_was_submitted_with).
 * Resident models -- the ONE rule of wdx_svm_set_model, wdx_mlp_set_model and wdx_boost_set_model:
 *   - The setter copies every array of the model at set time, and may be called with work pending on any stream of the
 *     device.  It waits for the device.
 *   - A refused model (WDX_ERR_INVALID, WDX_ERR_UNSUPPORTED), or a host or device allocation or a copy that fails, keeps
 *     the previous model resident and usable.
 *   - A minibatch in flight (WDX_WANT_SVM, WDX_WANT_BOOST) hands over the answers of the model it was submitted with; every
 *     later submit reads the new one.  The class count a slot's prob is sized by is fixed at its submit.
 *   Each model lives in its own slot of the context: setting one kind leaves the other two untouched.
 * HIP is initialised lazily inside wdx_ctx_create, so a process may fork
 * (file_proc.py:1197-1243, ProcessPoolExecutor workers) before creating its context; a context must not
 * be used in a child forked after its creation.  The caller's current HIP device is left unchanged by
 * every entry point.  Nothing in the library reads the environment.
 */
#ifndef WDX_H
#define WDX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WDX_ABI_VERSION 4

/* ---- call status ------------------------------------------------------------------------- */
#define WDX_SUCCESS 0
#define WDX_ERR_INVALID (-1)     /* bad argument (maps to ValueError in the Python shim)        */
#define WDX_ERR_NO_DEVICE (-2)   /* no usable HIP device / runtime                              */
#define WDX_ERR_HIP (-3)         /* a HIP call failed                                           */
#define WDX_ERR_UNSUPPORTED (-4) /* legal in the reference, outside this engine's limits        */
#define WDX_ERR_NO_REFS (-5)     /* a call that needs wdx_set_refs() came before it             */

/* ---- per-read status (fingerprint stage); 0 == ReadResult.success ------------------------ */
#define WDX_READ_OK 0
#define WDX_READ_FAIL_DETECT 1  /* detect_results.success False   sig_proc.py:400-407           */
#define WDX_READ_FAIL_SIGNORM 2 /* "signal normalization failed"  sig_proc.py:433-446           */
#define WDX_READ_FAIL_SEGMENT 3 /* "event segmentation failed"    sig_proc.py:537-544           */
#define WDX_READ_FAIL_SEGNORM 4 /* "segment normalization failed" sig_proc.py:546-560           */
#define WDX_READ_FAIL_UNKNOWN 5 /* exception -> "unknown"         file_proc.py:209-224          */
#define WDX_READ_FAIL_CONSENSUS 6 /* "consensus query outlier"    sig_proc.py:497-512 (refinement) */

/* normalisation selectors (sig_proc.py:114-136) */
#define WDX_NORM_NONE 0
#define WDX_NORM_MEAN 1
#define WDX_NORM_MEDIAN 2

/* The hot-path knobs of SigProcConfig (config/sig_proc.py:16-70 + ADAPTed core.*), by value.
 * Limits, checked once per call before any launch (wdx_fingerprint.hip, launch_fingerprint):
 *   num_events          1 .. 253   0 or less -> WDX_ERR_INVALID, 254 or more -> WDX_ERR_UNSUPPORTED
 *   barcode_num_events  1 .. 254   outside   -> WDX_ERR_INVALID (beyond num_events + 1 every read fails, as in
 *                                               the reference)
 *   running_stat_width  0 .. 64    outside   -> WDX_ERR_UNSUPPORTED (0 is accepted: no t-scores, so every read
 *                                               fails, WDX_READ_FAIL_SEGMENT or with accept_less_cpts
 *                                               WDX_READ_FAIL_UNKNOWN, as in the reference)
 *   padding             >= 0       negative  -> WDX_ERR_INVALID
 *   min_obs_per_base    any        below 1 every read fails with WDX_READ_FAIL_UNKNOWN (scipy refuses distance 0)
 * Adapter windows (padding included) longer than WDX_MAX_ADAPTER_SAMPLES come back WDX_READ_FAIL_UNKNOWN -- on a context
 * with WDX_OPT_LONG_WINDOWS = 1 (plain branch) / WDX_OPT_LONG_REFINE_WINDOWS = 1 (consensus-refinement branch), longer
 * than WDX_MAX_LONG_ADAPTER_SAMPLES. */
typedef struct wdx_seg_params {
    int32_t padding;            /* sig_extract.padding                                          */
    int32_t sig_norm;           /* sig_extract.normalization   (WDX_NORM_*)                     */
    float outlier_thresh;       /* core.sig_norm_outlier_thresh                                 */
    int32_t min_obs_per_base;   /* segmentation.min_obs_per_base                                */
    int32_t running_stat_width; /* segmentation.running_stat_width                              */
    int32_t num_events;         /* segmentation.num_events                                      */
    int32_t accept_less_cpts;   /* segmentation.accept_less_cpts                                */
    int32_t seg_norm;           /* segmentation.normalization  (WDX_NORM_*)                     */
    int32_t barcode_num_events; /* segmentation.barcode_num_events (int form)                   */
    /* How the clip bounds `med -/+ thresh*mad` (sig_proc.py:426-431) are evaluated -- the one place on the
     * path where the reference's result depends on its NumPy: 0 = in float32 from outlier_thresh (NumPy >= 2
     * promotion: float32 scalar x Python float stays float32); 1 = in float64 from outlier_thresh_f64 and
     * rounded to float32 once (NumPy 1.x value-based promotion -- the reference pins numpy 1.26.4,
     * environment.yml -- or an np.float64 threshold under NumPy 2).  The Python shim picks the rule of the
     * NumPy it runs under, so the drop-in returns what the reference would have returned in that process. */
    int32_t clip_bounds_f64;
    double outlier_thresh_f64;  /* core.sig_norm_outlier_thresh as a double (used when clip_bounds_f64 != 0) */
} wdx_seg_params;

typedef struct wdx_ctx wdx_ctx;

/* ---- context ----------------------------------------------------------------------------- */
int wdx_abi_version(void);
/* Message of the last failing call on this thread ("" if none). Never NULL. */
const char *wdx_last_error(void);
/* Number of visible HIP devices, or a negative WDX_ERR_*. Does not create a context. */
int wdx_device_count(void);
/* Create a context on HIP device `device`.  First HIP use in the process happens here. */
int wdx_ctx_create(int device, wdx_ctx **out);
void wdx_ctx_destroy(wdx_ctx *ctx);
/* Block until all work enqueued on `stream` has finished.  stream == NULL names the legacy NULL stream,
 * exactly as in the *_dev entry points, AND the context's own stream (wdx_ctx_stream) is waited for too --
 * so `wdx_demux_dev(..., NULL); wdx_ctx_synchronize(ctx, NULL);` is complete when it returns (ABI 2 briefly
 * waited for the context stream only: fixed in ABI 3). */
int wdx_ctx_synchronize(wdx_ctx *ctx, void *stream);
/* The context's own stream (hipStream_t as void*): the one its host-buffer calls run on. */
int wdx_ctx_stream(wdx_ctx *ctx, void **stream);

/* Diagnostic switches (all 0 by default = the product path); used by tests and profiling tools only. */
#define WDX_OPT_EXACT_PATH 1        /* fingerprint every read on the exact general kernel               */
#define WDX_OPT_NO_WAVEFRONT_DTW 2  /* never dispatch the anti-diagonal DTW kernel                       */
#define WDX_OPT_NO_SHORT_DTW 3      /* never dispatch the unrolled 25-point DTW kernel                   */
#define WDX_OPT_SVM_SCALAR 4        /* scalar SVM tail kernel instead of the matrix-core one             */
#define WDX_OPT_DEBUG_OCCUPANCY 5   /* print the fast fingerprint kernel's workgroups per CU to stderr   */
#define WDX_OPT_FAST_PEAK_CAP 6     /* peak-list capacity of the fast fingerprint kernel (0 = built-in)  */
#define WDX_OPT_FAST_EXACT_SCORES 7 /* fast fingerprint kernel: exact t-scores, no approximate keys       */
#define WDX_OPT_FAST_MAIN_CAP 8     /* main fast instantiation: 5120 or 6144 samples (0 = chosen by batch)  */
#define WDX_OPT_FAST_CHAIN_MIN_READS 9 /* smallest batch that takes the approximate-keys launch chain (0 = 2048) */
#define WDX_OPT_EXACT_NO_PEAK_LIST 10  /* exact kernel: suppression / top-E over positions, never over the peak list */
#define WDX_OPT_MAX_LAUNCH_SLICE 11    /* fingerprint chain: at most this many workgroups per launch slice (0 = built-in) */
#define WDX_OPT_NO_PEAK_FILTER 12      /* fast fingerprint kernels: no threshold filter of the peak list (every local maximum) */
#define WDX_OPT_NO_WAVE_CLIP_LONG 13    /* windows beyond 6144 samples: clip bounds by the workgroup kernel alone (A/B, tests) */
#define WDX_OPT_NO_CLIP_REUSE 14        /* exact kernel behind the launch chain: recompute the clip bounds (A/B, tests) */
#define WDX_OPT_NO_SPLIT_TAIL 15        /* main fast fingerprint kernel in one piece: no tile kernel + tail kernel split (A/B, tests) */
#define WDX_OPT_DTW_UNFUSED 16          /* DTW cells: 0 (default) one v_fma_f64 per cell, pairs whose float32 could differ from the
                                         * reference's are run again on its six operations (wdx_dtw.hip: dtw_unsettled) | 1 the six
                                         * operations only (A/B) | 2 fused and every pair run again (tests) | 3 fused, never run again
                                         * (diagnostic: NOT the reference's results) */
#define WDX_OPT_MLP_CHUNK_ROWS 17       /* wdx_dtw_mlp_predict: rows per DTW + MLP pass (0 = built-in; tests walk several chunks) */
#define WDX_OPT_BOOST_CHUNK_ROWS 18     /* wdx_boost_predict: rows per pass (0 = built-in; tests walk several chunks) */
#define WDX_OPT_BOOST_KERNEL 19         /* boost tail: 0 (default) the kernel is chosen by batch size (WDX_BOOST_SMALL_MAX_READS) |
                                         * 1 the lane-per-read kernel only | 2 the tree-parallel kernel only (A/B, tests); both
                                         * give the same bits */
/* A product option, not a diagnostic one.  0 (default): adapter windows beyond WDX_MAX_ADAPTER_SAMPLES are reported
 * WDX_READ_FAIL_UNKNOWN.  1: windows up to WDX_MAX_LONG_ADAPTER_SAMPLES are fingerprinted (the reference has no limit:
 * `--export core.max_obs_trace=...`), bit for bit like the shorter ones, by one more storage form of the exact kernel
 * (samples and score curve in HBM: a rare-read path); longer ones are reported WDX_READ_FAIL_UNKNOWN.  Any other value:
 * WDX_ERR_INVALID.  Every entry that fingerprints on this context honours it -- wdx_fingerprint_batch[_adc],
 * wdx_fingerprint_dev, wdx_demux_batch[_adc], wdx_demux_dev, wdx_demux_svm_dev / _mlp_dev / _boost_dev,
 * wdx_demux_submit[_ex|_adc] (a pipeline slot copies the options at every submit), a feeder served by this
 * context, wdx_live_tick[_ex] -- with two exceptions: the consensus-refinement branch (wdx_*_refine*, rp != NULL) does not
 * look at this option but at WDX_OPT_LONG_REFINE_WINDOWS, and wdx_fingerprint_profile_dev keeps the limit of
 * WDX_MAX_ADAPTER_SAMPLES.  Cost: 12 MiB of device memory per context
 * (16 slots of 768 KiB), allocated by the first call that meets such a window with the option on (a synchronising
 * hipMalloc on that one call) and never otherwise; each pipeline slot that meets one owns its own (96 MiB for 8). */
#define WDX_OPT_LONG_WINDOWS 20
/* The same product option for the consensus-refinement branch (the flow of the tRNA models), independent of the one above:
 * a call with rp != NULL looks at this option only, a plain call at WDX_OPT_LONG_WINDOWS only.  0 (default): a refined
 * adapter window beyond WDX_MAX_ADAPTER_SAMPLES is reported WDX_READ_FAIL_UNKNOWN.  1: windows up to
 * WDX_MAX_LONG_ADAPTER_SAMPLES are segmented, matched against the consensus and their barcode tail -- of any length inside
 * the window -- segmented again, in place, by the long form of the exact kernel, bit for bit like the shorter ones; longer
 * ones are reported WDX_READ_FAIL_UNKNOWN.  Any other value: WDX_ERR_INVALID.  Honoured by wdx_fingerprint_refine_batch,
 * wdx_fingerprint_refine_dev, wdx_demux_refine_dev, wdx_demux_boost_dev with rp, wdx_demux_submit_refine (float32 and int16
 * descriptors; a pipeline slot copies the options at every submit), a refine feeder ring served by this context and
 * wdx_live_tick_ex with rp (an int16 tick's staging cuts at the cap of the branch the tick runs, plus one).  The slots are
 * the ones of WDX_OPT_LONG_WINDOWS (12 MiB per context or pipeline slot, allocated by the first call that meets such a
 * window with the option of its branch on, never otherwise). */
#define WDX_OPT_LONG_REFINE_WINDOWS 21
/* Reads per slice of the *_adc_dev entries (int16 device shards, below): 0 (default) = as many as the 1 GiB staging budget
 * holds; a positive value is used as given wherever it stays inside that budget (tests walk several slices at small n);
 * negative: WDX_ERR_INVALID.  It changes which reads share a launch, never a result. */
#define WDX_OPT_ADC_DEV_SLICE_READS 22
/* A product option of the consensus-refinement branch: segmentation.refinement_optimal_cpts (sig_proc.py:348-354).  0 (default): the
 * barcode tail of the score curve is cut at its strongest peaks.  1: it is cut at the least-squares OPTIMAL change-points, what the
 * reference asks ruptures.KernelCPD(kernel="linear", min_size=min_obs_per_base).predict(n_bkps=barcode_num_events[0]) for; everything up
 * to and including the subsequence match (stats, refine_idx, the outlier filter) is unchanged.  Any other value: WDX_ERR_INVALID.
 * THE RULE, in float64 with no operation fused -- parity with ruptures' own bits is NOT pinned (the library is absent where this was
 * built):
 *   x = adapter_scores[sig_barcode_start:], the adapter's t-scores with the ADAPTED window width w_eff: N = max(0, n - 2 w_eff -
 *   sig_barcode_start) samples; m = min_obs_per_base as configured; B = barcode_segm_events
 *   P[0] = Q[0] = 0, P[t] = P[t-1] + x[t-1], Q[t] = Q[t-1] + x[t-1] * x[t-1]               (sequential)
 *   cost(s, t) = (Q[t] - Q[s]) - ((P[t] - P[s]) * (P[t] - P[s])) / (double)(t - s)
 *   V_0[t] = cost(0, t) for t >= m;  V_k[t] = min over s in [k m, t - m] of V_{k-1}[s] + cost(s, t), ties to the smallest s
 *   valid_cpts = [0, b_1 .. b_B, N] by the back-trace from t = N, k = B; like the reference this branch adds no
 *   running_stat_width to the boundaries and ends at N, not at the signal's end.  Dwell times = diff(valid_cpts): B + 1 of them.
 *   Event means = the reference's compute_base_means(adapter_sig[sig_barcode_start:], valid_cpts), which closes the slice with one
 *   more event when the last boundary is not its end: B + 2 means, the last over the 2 w_eff samples behind the score curve.  fpt =
 *   the last barcode_keep_events of the normalize_wrt'ed means, dwell = the last barcode_keep_events dwell times -- as the
 *   reference returns them, one event apart.  barcode_keep_events > B + 1 (the reference would return fewer dwell times than
 *   fingerprint entries, or raise): WDX_READ_FAIL_UNKNOWN.
 * Deviation: an infeasible tail ((B + 1) m > N) or a non-finite score in it is WDX_READ_FAIL_SEGMENT with NaN stats and refine_idx
 * -1 (ruptures raises there and the reference's call dies).
 * Honoured by every entry that takes rp: wdx_fingerprint_refine_batch, wdx_fingerprint_refine_dev / _adc_dev, wdx_demux_refine_dev /
 * _adc_dev, wdx_demux_boost_dev / _adc_dev with rp, wdx_demux_submit_refine (a pipeline slot copies the options at every submit), a
 * refine feeder ring served by this context, wdx_live_tick_ex with rp.  With the option on a call with rp returns
 * WDX_ERR_UNSUPPORTED when WDX_OPT_LONG_REFINE_WINDOWS is 1 as well, when min_obs_per_base < 1, or when sig_extract.normalization is
 * not WDX_NORM_NONE (no shipped configuration normalises the signal on this branch).  Cost: a per-read dynamic programme of B N^2 / 2
 * candidates (fingerprint_refine_optimal_kernel, WDX_K_REFINE_OPTIMAL) and a context-owned scratch buffer of at most 256 MiB for the
 * path tables of the reads in flight, allocated by the first refining call with the option on and never otherwise (each pipeline
 * slot that meets one owns its own); workspaces and every allocation of the default path are unchanged. */
#define WDX_OPT_REFINE_OPTIMAL_CPTS 23
/* A product option of the DTW seam, not a diagnostic one.  0 (default): effective windows beyond 32 -- the reference's default
 * window=None (unbanded) on series longer than 32 points included -- run on the scratch-row kernel (WDX_DTW_SCRATCH: two DP rows per
 * lane in a context-owned global block, one launch per 65 536 lanes), and the fused device-resident entries (wdx_demux_dev,
 * wdx_demux_refine_dev and their _adc_dev twins) return WDX_ERR_UNSUPPORTED for such a reference set.  1: effective windows
 * 33 .. L at series lengths L <= WDX_DTW_WIDE_MAX_L run on the wide-window kernel (WDX_DTW_WIDE) wherever a DTW is dispatched on this
 * context: wdx_dtw_matrix[_dev], wdx_demux_batch[_adc], wdx_demux_dev / _refine_dev / _adc_dev / _refine_adc_dev (which then accept
 * such a set), wdx_demux_submit* (a pipeline slot copies the options at every submit), a feeder served by this context,
 * wdx_live_tick[_ex], wdx_dtw_svm_predict, wdx_dtw_mlp_predict, wdx_demux_svm_dev, wdx_demux_mlp_dev.  Any other value:
 * WDX_ERR_INVALID.  Same float32 distances and argmin as the scratch rows, bit for bit (the reference's six float64 operations per
 * cell; WDX_OPT_DTW_UNFUSED changes nothing here); all three operand layouts, the reference split over grid.y and the fused
 * argmin follow the rules of the register-band kernels; one launch per dispatch.  Cost: none in memory -- no scratch block, nothing
 * added to wdx_demux_workspace_bytes; the DP state is 32 float64 registers per lane plus 512 L bytes of LDS per wave (so 2 waves
 * per CU at L = 110, 1 from L = 161 on).
 * Limits: L > WDX_DTW_WIDE_MAX_L stays on the scratch rows with the option on, and the fused device-resident entries still return
 * WDX_ERR_UNSUPPORTED ("demux_dev needs window <= 32") there, as they do for every window beyond 32 with the option off.
 * Measured against the scratch rows (profiles/wide_dtw.json): see there for the figures of every shape class. */
#define WDX_OPT_WIDE_DTW 24
#define WDX_DTW_WIDE_MAX_L 256 /* longest series of the wide-window kernel: every fingerprint length (K <= 254) fits */
/* Diagnostic: 1 sends every wdx_medoids_device / wdx_dtw_medoids call through the general route (the label's matrix block by block
 * through the DTW dispatch, then chunk sums) instead of the tile kernels.  Same bits.  Any other value than 0 or 1: WDX_ERR_INVALID. */
#define WDX_OPT_MEDOID_GENERAL 25
/* Diagnostic: 1 sends every wdx_self_matrix_device / wdx_dtw_self_matrix call through the general route (row blocks through the
 * DTW dispatch straight into the matrix, then a mask kernel for the non-members) instead of the tile kernels.  Same bits.  Any
 * other value than 0 or 1: WDX_ERR_INVALID. */
#define WDX_OPT_SELF_MATRIX_GENERAL 26
/* Diagnostic: 1 sends every wdx_dba_step_device / wdx_dtw_dba_step call through the general route (two rolling rows per lane in
 * global memory) instead of the register band.  Same bits.  Any other value than 0 or 1: WDX_ERR_INVALID. */
#define WDX_OPT_DBA_GENERAL 27
/* Diagnostic: 1 sends every wdx_self_nearest_device / wdx_dtw_self_nearest call through the general route (blocks of rows through
 * the DTW dispatch into a float32 block, then a rows kernel) instead of the tile kernels.  Same bits.  Any other value than 0 or 1:
 * WDX_ERR_INVALID. */
#define WDX_OPT_SELF_NEAREST_GENERAL 28
int wdx_ctx_set_option(wdx_ctx *ctx, int32_t option, int64_t value);

/* ---- seam 1: batched DTW  (replaces parallel_distances.py:48-67 `distance_matrix_to`,
 *      i.e. dtaidistance.dtw.distance_matrix(vstack[X,Y], block=((0,nX),(nX,nX+nY)),
 *      window, penalty, use_c=True)[:nX, nX:].astype(float32) ) ------------------------------ */

/* X: (nX,L) float64 row-major host; Y: (nY,L) float64 row-major host; out: (nX,nY) float32 host.
 * window <= 0 means unbanded (reference: None/0); penalty is the un-squared dtaidistance penalty
 * (0 = none).  argmin (nullable): int32[nX] = np.argmin(out, axis=1).  Both nX and nY may be 0. */
int wdx_dtw_matrix(wdx_ctx *ctx, const double *X, int64_t nX, const double *Y, int64_t nY,
                   int64_t L, int32_t window, double penalty, float *out, int32_t *argmin);

/* Upload the reference set once (model._X, models/dtw_base.py:14-17) and keep it resident.
 * Y is a HOST pointer; it is re-uploaded only if its content/params differ from the cached set. */
int wdx_set_refs(wdx_ctx *ctx, const double *Y, int64_t nY, int64_t L, int32_t window,
                 double penalty);
/* Counter that changes whenever the resident reference set changes (samples, window or penalty) -- by
 * wdx_set_refs or by wdx_dtw_matrix, which installs its Y.  A caller that keeps "its" references resident
 * across calls (the live tick loop, worker.py:26-131) compares it with the value it saw after its own
 * wdx_set_refs to learn that another user of the context has replaced them. */
int wdx_refs_generation(wdx_ctx *ctx, int64_t *generation);

/* Device-resident DTW against the resident reference set.
 * dX: (nX,L) float64 row-major DEVICE; d_out: (nX,nY) float32 DEVICE;
 * d_argmin (nullable): int32[nX] DEVICE. */
int wdx_dtw_matrix_dev(wdx_ctx *ctx, const double *dX, int64_t nX, float *d_out,
                       int32_t *d_argmin, void *stream);

/* ---- seam 2: batched fingerprinting (replaces the per-read loop file_proc.py:418-428 over
 *      sig_proc.py:394-605 `detect_results_to_fpt`, non-refinement branch) ------------------- */

/* sig: (n_reads, stride) float32 host minibatch, NaN tail (file_proc.py:244-260);
 * a_start/a_end: DetectResults.adapter_start/end; ok (nullable): DetectResults.success.
 * Outputs (host): fpt (n_reads,K) float64, dwell (n_reads,K) int64, stats (n_reads,6) float64 =
 * {adapter_dt_med, adapter_dt_mad, adapter_event_mean, adapter_event_std, adapter_event_med,
 * adapter_event_mad}, status int32[n_reads] (WDX_READ_*).  Rows of failed reads hold NaN / 0.
 * K = p->barcode_num_events.  The input rows are NOT clipped in place (the reference's
 * in-place clip, sig_proc.py:426-431, is never read again: file_proc.py:430). */
int wdx_fingerprint_batch(wdx_ctx *ctx, const float *sig, int64_t n_reads, int64_t stride,
                          const int32_t *a_start, const int32_t *a_end, const uint8_t *ok,
                          const wdx_seg_params *p, double *fpt, int64_t *dwell, double *stats,
                          int32_t *status);

/* Device-resident form.  Read r occupies d_sig[row_off[r] .. row_off[r] + row_len[r]) where
 *   d_row_off == NULL  -> row_off[r] = r*stride        (minibatch layout)
 *   d_row_len == NULL  -> row_len[r] = d_row_off ? d_row_off[r+1]-d_row_off[r] : stride
 * (so a packed batch passes int64 offsets[n_reads+1] and NULL lengths).  max_len bounds the
 * adapter window of every read (it sizes the LDS carve-up); windows longer than max_len or than
 * WDX_MAX_ADAPTER_SAMPLES (WDX_OPT_LONG_WINDOWS / WDX_OPT_LONG_REFINE_WINDOWS = 1: than WDX_MAX_LONG_ADAPTER_SAMPLES, see there) are reported
 * WDX_READ_FAIL_UNKNOWN.  (The largest window the reference admits is
 * max_obs_trace + 2*padding = 15 200 samples, DEPRECATED/config_files/rna002_70bps@v0.4.4.toml:2; up to 11 200
 * samples a read's score curve lives in LDS, beyond that in a context-owned HBM block of 32 MiB that is
 * allocated on first need -- a synchronising hipMalloc on that one call.)
 * Any output pointer except d_status may be NULL. */
int wdx_fingerprint_dev(wdx_ctx *ctx, const float *d_sig, const int64_t *d_row_off,
                        const int32_t *d_row_len, int64_t stride, int64_t max_len,
                        int64_t n_reads, const int32_t *d_a_start, const int32_t *d_a_end,
                        const uint8_t *d_ok, const wdx_seg_params *p, double *d_fpt,
                        int64_t *d_dwell, double *d_stats, int32_t *d_status, void *stream);

#define WDX_MAX_ADAPTER_SAMPLES 16384
#define WDX_MAX_LONG_ADAPTER_SAMPLES 65536 /* with WDX_OPT_LONG_WINDOWS = 1 (refinement: WDX_OPT_LONG_REFINE_WINDOWS = 1) */

/* ---- N3: consensus-guided barcode refinement (tRNA models) -- detect_results_to_fpt with
 *      segmentation.consensus_refinement = True (sig_proc.py:257-378, 452-521): segment the adapter, find the
 *      constant adapter part by subsequence DTW of a consensus signal against the normalised event means
 *      (dtaidistance warping_paths_fast + SubsequenceAlignment.best_match in the reference), re-segment the score
 *      curve behind it into barcode events, normalise them with the ADAPTER's mean/std (normalize_wrt). */
typedef struct wdx_refine_params {
    const double *query;          /* consensus signal (warpdemux/_consensus.py ALL[consensus_model]); HOST pointer   */
    int32_t n_query;              /* 1..96                                                                         */
    int32_t subseq_norm;          /* segmentation.consensus_subseq_match_normalization (WDX_NORM_*)                 */
    double penalty;               /* segmentation.consensus_subseq_match_penalty (un-squared)                      */
    int32_t psi[4];               /* segmentation.consensus_subseq_match_psi: relaxation at the begin / end of the
                                     query and the begin / end of the series (the two end values do not enter the
                                     matching function the reference reads)                                        */
    int32_t ub_start, lb_end, ub_end; /* consensus_subseq_match_ub_start / lb_end / ub_end (outlier filter)         */
    int32_t barcode_segm_events;  /* barcode_num_events[0]: events detected in the barcode tail                     */
    int32_t barcode_keep_events;  /* barcode_num_events[1]: events kept = K of fpt / dwell                          */
} wdx_refine_params;
/* As wdx_fingerprint_batch; K = rp->barcode_keep_events (p->barcode_num_events is ignored); stats are the ADAPTER's;
 * refine_idx (n_reads, 3) int32 = {seg_cons_query_start, seg_cons_query_end, sig_barcode_start} (-1 when the read
 * failed earlier).  Status WDX_READ_FAIL_CONSENSUS still reports stats and refine_idx, like the reference's
 * ReadResult.  Limits: num_events <= 127; refinement_optimal_cpts (ruptures KernelCPD): WDX_OPT_REFINE_OPTIMAL_CPTS = 1 on the
 * context (off by default; the rule and its limits are stated there). */
int wdx_fingerprint_refine_batch(wdx_ctx *ctx, const float *sig, int64_t n_reads, int64_t stride,
                                 const int32_t *a_start, const int32_t *a_end, const uint8_t *ok,
                                 const wdx_seg_params *p, const wdx_refine_params *rp, double *fpt, int64_t *dwell,
                                 double *stats, int32_t *refine_idx, int32_t *status);

/* Device-resident form of the refinement branch: inputs and outputs as in wdx_fingerprint_dev (d_fpt / d_dwell have
 * K = rp->barcode_keep_events columns), d_refine_idx (n_reads, 3) int32 on the device; rp and its query are HOST
 * memory (copied before the call returns).  Enqueued on `stream`; no synchronisation. */
int wdx_fingerprint_refine_dev(wdx_ctx *ctx, const float *d_sig, const int64_t *d_row_off,
                               const int32_t *d_row_len, int64_t stride, int64_t max_len, int64_t n_reads,
                               const int32_t *d_a_start, const int32_t *d_a_end, const uint8_t *d_ok,
                               const wdx_seg_params *p, const wdx_refine_params *rp, double *d_fpt,
                               int64_t *d_dwell, double *d_stats, int32_t *d_refine_idx, int32_t *d_status,
                               void *stream);

/* ---- fused path: raw adapter rows -> fingerprint -> DTW to the resident refs -> call ------ */

/* As wdx_fingerprint_dev, then DTW of every successful read against the resident refs.
 * d_dist: (n_reads,nY) float32; d_call: int32[n_reads] = argmin column or -1 for failed reads;
 * d_counts (nullable): int64[nY+1], INCREMENTED by the per-column call histogram, slot nY =
 * failed reads.  d_fpt/d_dwell/d_stats are optional as above.  d_work: DEVICE scratch of at
 * least wdx_demux_workspace_bytes(n_reads, K) bytes (fingerprints, the chain's hand-over lists and clip records -- 40 bytes per
 * read -- and the split main kernel's peak lists for one launch slice: 4 624 bytes per read of min(n_reads, 524 288)).
 * ALIGNMENT, of this and of every other *_dev entry: d_work must be a multiple of 16 bytes (its pieces lie at multiples of 8, the clip
 * and peak-list records at multiples of 16 and are read 16 bytes at a time: warpdemux_amd/csrc/wdx_work_layout.h); every output array
 * needs the alignment of its element type and no more -- 8 bytes for float64 / int64, 4 for float32 / int32. */
int64_t wdx_demux_workspace_bytes(int64_t n_reads, int32_t barcode_num_events);
int wdx_demux_dev(wdx_ctx *ctx, const float *d_sig, const int64_t *d_row_off,
                  const int32_t *d_row_len, int64_t stride, int64_t max_len, int64_t n_reads,
                  const int32_t *d_a_start, const int32_t *d_a_end, const uint8_t *d_ok,
                  const wdx_seg_params *p, double *d_fpt, int64_t *d_dwell, double *d_stats,
                  int32_t *d_status, float *d_dist, int32_t *d_call, int64_t *d_counts,
                  void *d_work, void *stream);

/* Host-buffer form of the fused path (one call per minibatch or per live tick, one synchronisation):
 * fingerprint the (n_reads, stride) float32 minibatch, DTW every successful read against the resident
 * reference set (wdx_set_refs; K = p->barcode_num_events must equal its length), nearest-reference call.
 * n_refs = the number of references the caller sized `dist` for; it must equal the resident nY
 * (WDX_ERR_INVALID otherwise: another user of the context may have replaced the set).
 * Host outputs: status int32[n_reads]; call int32[n_reads] (argmin column, -1 for failed reads);
 * dist (n_reads, n_refs) float32 (nullable; NaN rows for failed reads); fpt (n_reads, K) float64 (nullable). */
int wdx_demux_batch(wdx_ctx *ctx, const float *sig, int64_t n_reads, int64_t stride,
                    const int32_t *a_start, const int32_t *a_end, const uint8_t *ok,
                    const wdx_seg_params *p, int64_t n_refs, double *fpt, float *dist, int32_t *call,
                    int32_t *status);

/* ---- nearest-reference calls with reference labels, margin and rejection ------------------------------------------
 * The `process_probs` of the distance path (models/utils.py:45-61 ends every classifier of the reference that way: argmax,
 * label map, top1 - top2 margin, per-class thresholds -> -1), computed where the distances are produced.  The reference has
 * no such function for distances: the rule below is this engine's own, on the float32 distances wdx_dtw_matrix[_dev] returns.
 * Reference c of the resident set carries the label ref_label[c] in 0 .. n_labels-1 (several references may share one: a
 * few consensus signals per barcode, a model's training rows as a 1-nearest-neighbour classifier); a NULL label array is
 * the identity and n_labels must then be nY.  For the distance row d of a read (float32 throughout):
 *   c1 = np.argmin(d) (first minimum; a first NaN wins outright), lab = ref_label[c1], d1 = d[c1]
 *   d2 = min(d[c] for c with ref_label[c] != lab): +inf when no reference has another label, NaN when the row holds a NaN
 *   margin = d2 - d1 (inf - inf is NaN)
 *   call = lab, but -1 when d1 is NaN, when min_margin is given and !(margin >= min_margin[lab]), or when max_dist is given
 *          and !(d1 <= max_dist[lab]) -- a NaN rejects
 *   a read whose status (nullable) is not 0: call = -1, d1 = d2 = NaN
 *   counts int64[n_labels + 1] (nullable) is INCREMENTED: bin lab by the accepted reads, bin n_labels by every call of -1.
 * With identity labels and no thresholds, call is the argmin wdx_dtw_matrix_dev / wdx_demux_dev return wherever the row has
 * no NaN.  Outputs: call int32[n]; best (n, 2) float32 = {d1, d2} (NaN as 0x7fc00000); dist (n, nY) float32, NULLABLE --
 * without it the (n, nY) matrix is never written where one lane of the DTW kernel walks all references of a read
 * (wdx_dtw_last_launch: fused_argmin = 1 reports that the rule ran in the kernel's epilogue), and goes through a
 * context-owned block of at most 96 MiB, row block by row block, on every other route (fused_argmin = 0: the rule ran on the
 * block's matrix, nearest_rows_kernel).  Every DTW option (WDX_OPT_WIDE_DTW included) applies as in wdx_dtw_matrix_dev /
 * wdx_demux_dev.  Label and threshold arrays are read during the call only: no context state, no lifetime rule.
 * WDX_ERR_NO_REFS without a resident reference set; WDX_ERR_INVALID: n_labels < 1, a NULL label array with n_labels != nY, an
 * empty reference set.  The context stays usable after a refusal.
 *
 * wdx_nearest_dev: dX (nX, L) float64 DEVICE fingerprints against the resident set; every array DEVICE memory; d_status,
 * d_ref_label, d_min_margin, d_max_dist, d_dist, d_best, d_counts nullable.  Enqueued on `stream`; no synchronisation.
 * PRECONDITION: device labels lie in 0 .. n_labels-1.  One that does not is read as a group of its own whose reads get call
 * -1 (bin n_labels); it indexes nothing. */
int wdx_nearest_dev(wdx_ctx *ctx, const double *dX, int64_t nX, const int32_t *d_status, const int32_t *d_ref_label,
                    int64_t n_labels, const float *d_min_margin, const float *d_max_dist, float *d_dist, int32_t *d_call,
                    float *d_best, int64_t *d_counts, void *stream);
/* wdx_demux_dev (same inputs, same d_work of wdx_demux_workspace_bytes(n_reads, K) bytes, float32 rows) with the rule in the
 * argmin's place: d_call, d_best and d_counts int64[n_labels + 1] follow it, with the reads' own d_status; d_dist is
 * nullable. */
int wdx_demux_nearest_dev(wdx_ctx *ctx, const float *d_sig, const int64_t *d_row_off, const int32_t *d_row_len, int64_t stride,
                          int64_t max_len, int64_t n_reads, const int32_t *d_a_start, const int32_t *d_a_end, const uint8_t *d_ok,
                          const wdx_seg_params *p, double *d_fpt, int64_t *d_dwell, double *d_stats, int32_t *d_status,
                          const int32_t *d_ref_label, int64_t n_labels, const float *d_min_margin, const float *d_max_dist,
                          float *d_dist, int32_t *d_call, float *d_best, int64_t *d_counts, void *d_work, void *stream);
/* Host form: X (nX, L) float64, the label and threshold arrays, dist (nullable), call and best are HOST memory; runs against
 * the RESIDENT set (wdx_set_refs), so that the labels' length is the resident nY.  A label outside 0 .. n_labels-1 is
 * WDX_ERR_INVALID.  One synchronisation. */
int wdx_dtw_nearest(wdx_ctx *ctx, const double *X, int64_t nX, const int32_t *ref_label, int64_t n_labels, const float *min_margin,
                    const float *max_dist, float *dist, int32_t *call, float *best);

/* ---- reference signals from labelled fingerprints: per-label DTW medoids -----------------------------------------------
 * The engine classifies against reference signals (wdx_set_refs, wdx_nearest_dev); this picks them.  The medoid of a label is
 * the training fingerprint whose summed DTW distance to the fingerprints of its label is smallest -- the usual start of
 * barycenter averaging, and a usable reference set as it is.  The reference has no such function: the rule below is this
 * engine's own, exact arithmetic on the float32 distances wdx_dtw_matrix returns.
 * Inputs: X (n, L) float64; label int32[n], one per row, in 0 .. n_labels-1, or -1 for "takes no part"; status int32[n]
 * (nullable); window and penalty as for wdx_dtw_matrix (no resident reference set is read or written).  Every DTW option of the
 * context (WDX_OPT_WIDE_DTW, WDX_OPT_DTW_UNFUSED, WDX_OPT_NO_SHORT_DTW, ...) applies as it does there.
 *   A row is a MEMBER of label g when its label is g, its status (if given) is 0 and all L samples are finite.
 *   f(a, b) is the float32 distance wdx_dtw_matrix returns for (X[a], X[b]).
 *   The rows of label g in rising row order, members or not, are q_0 < q_1 < ... < q_{m-1}; chunk c holds q_{64c} .. q_{64c+63}.
 *   cost[r] of a member r of g: a float64 total that starts at 0.0 and adds the chunk sums S_0, S_1, ... in rising c; S_c is a
 *           float64 sum that starts at 0.0 and adds (double)f(r, q_j) over the MEMBERS of chunk c in rising j (non-members are
 *           skipped, f(r, r) is included, an infinite sum is legal).  cost of a non-member: NaN.
 *   medoid[g] int64: the member of g with the smallest cost, the first in row order among equal costs; -1 without a member
 *   count[g] int64: the number of members;  medoid_cost[g] float64: cost[medoid[g]], or NaN
 *   refs (n_labels, L) float64: row g is X[medoid[g]] bit for bit, or a row of NaN
 * The summation order is part of the rule, so that the result does not depend on how the work is cut up: each unordered pair is
 * computed once (f(a, b) == f(b, a) bit for bit: DESIGN.md), in 64 x 64 tiles, one wave each.
 * Limit: a label of more than WDX_MEDOID_MAX_GROUP rows is WDX_ERR_UNSUPPORTED (the message names the label and its size; the
 * caller subsamples).  WDX_ERR_INVALID: n_labels < 1, a label outside -1 .. n_labels-1, L < 1, a NULL medoid output.  An empty
 * batch is success: every medoid -1, counts 0, NaN rows.  The context stays usable after a refusal, and nothing resident is
 * touched: references, models and wdx_refs_generation stay as they are.  Workspace: context-owned and bounded, see
 * warpdemux_amd/csrc/wdx_medoid_plan.h.
 *
 * wdx_medoids_device: dX, d_status and every output are DEVICE memory; d_status, d_medoid_cost, d_count, d_cost (float64[n]) and
 * d_refs are nullable; `label` is HOST memory, read during the call only.  Enqueued on `stream`; no synchronisation -- the
 * contract of the *_dev entries.  The entries whose names end in _device are the training entries; they have a closed table of
 * their own (tests/helpers/device_entries.py: one row per entry with its arguments by role and their exact sizes), which
 * tests/test_gpu_device_entries.py holds to exact buffers, workspace states and the stream contract, as
 * tests/test_gpu_buffer_bounds.py and tests/test_gpu_streams.py hold the table of the *_dev names. */
#define WDX_MEDOID_MAX_GROUP 32768
int wdx_medoids_device(wdx_ctx *ctx, const double *dX, int64_t n, int64_t L, const int32_t *label /* HOST */, int64_t n_labels,
                       const int32_t *d_status, int32_t window, double penalty, int64_t *d_medoid, double *d_medoid_cost,
                       int64_t *d_count, double *d_cost, double *d_refs, void *stream);
/* Host form: every array HOST memory; one synchronisation. */
int wdx_dtw_medoids(wdx_ctx *ctx, const double *X, int64_t n, int64_t L, const int32_t *label, int64_t n_labels,
                    const int32_t *status, int32_t window, double penalty, int64_t *medoid, double *medoid_cost, int64_t *count,
                    double *cost, double *refs);

/* ---- training matrix of a DTW kernel machine: the symmetric DTW self-distance matrix --------------------------------------
 * The (n, n) matrix of the rows of X against themselves, which a DTW_SVM is fitted on (the reference computes it with
 * distance_matrix_to(X, X), every unordered pair twice).  Each unordered pair is computed once, in 64 x 64 tiles of one wave
 * each, and written to both of its places: f(a, b) == f(b, a) bit for bit.
 * Inputs are those of the medoid entries: X (n, L) float64; status int32[n] (nullable); window and penalty as for
 * wdx_dtw_matrix.
 *   A row is a MEMBER when its status (if given) is 0 and all L samples are finite.
 *   out[a * ld + b] is float32, 0 <= a, b < n, ld >= n.
 *   Where a and b are both members it is f(a, b), the float32 wdx_dtw_matrix returns for (X[a], X[b]).
 *   Otherwise it is the quiet NaN 0x7fc00000.
 *   Columns n .. ld-1 of every row are not written.
 * Every DTW option of the context applies as it does to wdx_dtw_matrix (WDX_OPT_WIDE_DTW, WDX_OPT_DTW_UNFUSED,
 * WDX_OPT_NO_SHORT_DTW).  No resident reference set, no model and no wdx_refs_generation is read or changed.
 * Limit: n > WDX_SELF_MATRIX_MAX_ROWS (1 024 chunks of 64 rows, a 16 GiB matrix) is WDX_ERR_UNSUPPORTED (the message names n).
 * WDX_ERR_INVALID: L < 1, n < 0, ld < n, a NULL out with n > 0.  n == 0 is success and writes nothing.  After a refusal the
 * context stays usable and nothing has been written.  Workspace: context-owned, grow-only and bounded, see
 * warpdemux_amd/csrc/wdx_self_plan.h.
 *
 * wdx_self_matrix_device: dX, d_status and d_out are DEVICE memory.  Enqueued on `stream`; no synchronisation -- the contract of
 * the *_dev entries (a row of the table of the _device entries: wdx_medoids_device says where it is held). */
#define WDX_SELF_MATRIX_MAX_ROWS 65536
int wdx_self_matrix_device(wdx_ctx *ctx, const double *dX, int64_t n, int64_t L, const int32_t *d_status, int32_t window,
                           double penalty, float *d_out, int64_t ld, void *stream);
/* Host form: every array HOST memory; one synchronisation.  The device matrix is allocated for the call and freed before it
 * returns (a context never keeps 16 GiB). */
int wdx_dtw_self_matrix(wdx_ctx *ctx, const double *X, int64_t n, int64_t L, const int32_t *status, int32_t window,
                        double penalty, float *out, int64_t ld);

/* ---- is a labelled set any good: leave-one-out nearest neighbours ----------------------------------------------------------
 * Per row of a labelled set, the nearest other row of its own label and the nearest row of any other label: what the choice of
 * window and penalty, the screening of labels before a fit, and the leave-one-out 1-nearest-neighbour error all come from
 * (parallel_distances.loo_summary, loo_grid).  The self matrix's tile walk with this reduction in the place of the matrix: each
 * unordered pair is computed once, nothing of size n x n is written, the workspace is O(n x L).
 * Inputs: X (n, L) float64; label int32[n]: -1 means "takes no part", any value >= 0 is a label, NULL means every row has label
 * 0; status int32[n] (nullable); window and penalty as for wdx_dtw_matrix.  Every DTW option of the context applies as it does
 * to wdx_self_matrix_device (WDX_OPT_WIDE_DTW, WDX_OPT_DTW_UNFUSED, WDX_OPT_NO_SHORT_DTW).  Only equality of labels is used.
 *   A row is a MEMBER when its label is >= 0, its status (if given) is 0 and all L samples are finite.
 *   f(a, b) is the float32 wdx_dtw_matrix returns for (X[a], X[b]).  Between members it is never NaN: finite or +inf (the medoid
 *   rule's note); +inf is ordered after every finite value.
 *   For a member a, the OWN candidates are the members b != a with label[b] == label[a], the OTHER candidates the members with
 *   label[b] != label[a].  On each side nn is the candidate with the smallest f(a, b) and best is that f; among equal distances
 *   the lowest row index wins (also when every candidate is at +inf).  A side without a candidate has nn = -1, best = +inf.
 *   For a non-member both sides have nn = -1 and best = the quiet NaN 0x7fc00000.
 * Outputs: nn int32 (n, 2) = {own, other}; best float32 (n, 2).
 * Nothing resident is read or changed: references, models and wdx_refs_generation stay as they are.
 * Limit: n > WDX_SELF_MATRIX_MAX_ROWS is WDX_ERR_UNSUPPORTED (the message names n).  WDX_ERR_INVALID: L < 1, n < 0, a NULL nn or
 * best with n > 0.  n == 0 is success and writes nothing.  Refusals happen before anything is launched or written, and the context
 * stays usable.  Routes: the cases the self matrix's tile kernels serve run on tiles whose partial results are merged as 64-bit
 * keys (float32 bits << 32 | row) by an atomic minimum, so the result does not depend on the order the tiles finish in; wider
 * windows, window 0 and WDX_OPT_SELF_NEAREST_GENERAL = 1 go through the DTW dispatch in row blocks of at most 96 MiB; same bits.
 * Workspace: context-owned, grow-only and bounded, see warpdemux_amd/csrc/wdx_loo_plan.h.
 *
 * wdx_self_nearest_device: every array is DEVICE memory (d_label and d_status nullable).  Enqueued on `stream`; no
 * synchronisation -- the contract of the *_dev entries (a row of the table of the _device entries: wdx_medoids_device says where it
 * is held). */
int wdx_self_nearest_device(wdx_ctx *ctx, const double *dX, int64_t n, int64_t L, const int32_t *d_label, const int32_t *d_status,
                            int32_t window, double penalty, int32_t *d_nn, float *d_best, void *stream);
/* Host form: every array HOST memory; one synchronisation. */
int wdx_dtw_self_nearest(wdx_ctx *ctx, const double *X, int64_t n, int64_t L, const int32_t *label, const int32_t *status,
                         int32_t window, double penalty, int32_t *nn, float *best);

/* ---- barycenter reference signals: one step of DTW alignment and averaging ------------------------------------------------
 * The medoid of a label is one noisy read; a barycenter averages the noise of the whole label away.  One call aligns every
 * member of a label to the label's current centre and returns, per centre point, the mean of the samples matched to it; the
 * iteration is a short host loop over this step (parallel_distances.label_barycenters).  The rule below is this engine's own,
 * stated bit for bit as the medoid rule is: parity with dtaidistance's dtw_barycenter is NOT claimed.
 * Inputs: X (n, L) float64; label int32[n] on the HOST, -1 .. n_labels-1; status int32[n] (nullable); C (n_labels, L) float64,
 * the current centres; window and penalty as for wdx_dtw_matrix, w the effective window, p2 = penalty * penalty.
 *   MEMBERS are those of the medoid rule: label g, status 0 (if given), all L samples finite.  A label whose centre row holds a
 *   sample that is not finite, or which has no member, is IDLE.
 *   Cost matrix of member x (rows i) against its centre c (columns j), on the reference's six operations (never the fused cell):
 *     D[0][0] = 0, +inf elsewhere; for the cells inside the band (|i - j| < w)
 *     t = fl(min(D[i][j+1], D[i+1][j]) + p2);  D[i+1][j+1] = fl(fl(d*d) + min(t, D[i][j])),  d = fl(x[i] - c[j]);
 *     cost = D[L][L], a float64 that is not rooted.
 *   Direction of cell (i, j), with diag = D[i][j], up = D[i][j+1], left = D[i+1][j]:  diag if diag <= t;  otherwise up if
 *     up <= left (the raw values);  otherwise left.  Whatever the values, at i == 0 the step is left and at j == 0 it is up.
 *     (The recurrence's own argmin with ties in that order: in exact arithmetic a step cannot raise the summed cost.)
 *   Path: from (L-1, L-1) by the directions to (0, 0).  The rows matched to column j form one run lo[j] .. hi[j];
 *     lo[0] = 0, hi[L-1] = L-1, hi[j] <= lo[j+1] <= hi[j] + 1.
 *   Sums (float64, strictly sequential, starting at 0.0):  s_r[j] = x[lo[j]] + ... + x[hi[j]] in rising i;
 *     k_r[j] = hi[j] - lo[j] + 1.  The rows of label g in rising row order, members or not, form chunks of 64 as in the medoid
 *     rule;  S_c[j] adds s_r[j] over the MEMBERS of chunk c in rising order;  T[j] adds S_0[j], S_1[j], ...;  K[j] is the int64
 *     sum of k_r[j];  inertia[g] is the same two-level sum of cost.
 * Outputs: new_centres (n_labels, L) float64 = T[j] / (double)K[j], an idle label's row the quiet NaN;  count int64[n_labels], the
 *   members (idle: 0);  inertia float64[n_labels] (idle: NaN);  cost float64[n] (nullable; the quiet NaN for a non-member and for a
 *   member of an idle label);  runs int32 (n, L, 2) = lo, hi (nullable; -1 for those rows).
 *   (float)sqrt(cost[r]) is the float32 wdx_dtw_matrix returns for (X[r], C[label[r]]).
 * Nothing resident is read or changed: references, models and wdx_refs_generation stay as they are.
 * Routes: effective windows up to 32 run on the register band (dba_align_kernel), wider ones and window 0 (unbanded) on two
 * rolling rows per lane in global memory (dba_align_general_kernel); same bits.  WDX_OPT_DBA_GENERAL = 1 sends every call the
 * second way.
 * WDX_ERR_INVALID: n_labels < 1, a label outside -1 .. n_labels-1, L < 1, n < 0, a NULL d_new or d_centres.
 * WDX_ERR_UNSUPPORTED: L > WDX_DBA_MAX_L (the message names L).  A label may hold any number of rows (the medoids' cap does not
 * apply: a step has no block that grows with the square of a label).  n == 0 is success
 * with every label idle.  Refusals happen before anything is launched or written, and the context stays usable.  Workspace:
 * context-owned, grow-only and bounded, see warpdemux_amd/csrc/wdx_dba_plan.h.
 *
 * wdx_dba_step_device: dX, d_status, d_centres and every output are DEVICE memory; d_status, d_count, d_inertia, d_cost and d_runs
 * are nullable; d_new must not overlap d_centres; `label` is HOST memory, read during the call only.  Enqueued on `stream`; no
 * synchronisation -- the contract of the *_dev entries (a row of the table of the _device entries: wdx_medoids_device says where it
 * is held). */
#define WDX_DBA_MAX_L 1024
int wdx_dba_step_device(wdx_ctx *ctx, const double *dX, int64_t n, int64_t L, const int32_t *label /* HOST */, int64_t n_labels,
                        const int32_t *d_status, const double *d_centres, int32_t window, double penalty, double *d_new,
                        int64_t *d_count, double *d_inertia, double *d_cost, int32_t *d_runs, void *stream);
/* Host form: every array HOST memory; one synchronisation. */
int wdx_dtw_dba_step(wdx_ctx *ctx, const double *X, int64_t n, int64_t L, const int32_t *label, int64_t n_labels,
                     const int32_t *status, const double *centres, int32_t window, double penalty, double *new_centres,
                     int64_t *count, double *inertia, double *cost, int32_t *runs);

/* ---- fitting a DTW kernel machine: a batch of binary C-SVC duals by SMO ------------------------------------------------------
 * What a fit does behind the self-distance matrix: the k (k - 1) / 2 one-vs-one problems of a precomputed-kernel SVC, and the
 * five fold problems of each that libsvm's Platt scaling cross-validates, are independent -- one call solves all of them, one
 * workgroup per problem (models.DTW_SVM.fit(solver="device")).  Each problem is
 *     min 1/2 a'Qa - e'a,   0 <= a_s <= C_s,   y'a = 0,   Q_st = y_s y_t K_st
 * on rows of ONE kernel matrix K (m, m) float32 with leading dimension ld, every entry read as float64 (exactly).
 * A problem (wdx_svm_problem) names n_pos + n_neg entries of the row list from row0 on -- K-row indices; the first n_pos carry
 * y = +1 and C = c_pos, the next n_neg y = -1 and C = c_neg; "row t" below is the t-th of them, K_st = K[rows[s] * ld + rows[t]]
 * -- and n_eval entries of the evaluation list from eval0 on: K-row indices e whose decision value is wanted (a fold's held-out
 * rows).  alpha[row0 + t] belongs to row t, dec[eval0 + e] to evaluation row e, rho / n_iter / state [q] to problem q.
 *
 * THE RULE is libsvm's second-order working-set selection (Fan, Chen, Lin 2005) without shrinking, restated so that the result
 * is defined bit for bit.  All arithmetic is float64; every product, sum and quotient is rounded on its own (nothing is
 * contracted into a fused multiply-add); a maximum or minimum over rows rounds nothing.  TAU = 1e-12.
 *   1. a = 0, G = -1 for every row; it = 0.
 *   2. If any G_t is not finite: state 2, stop.   v_t = -y_t G_t.
 *   3. I_up = {t: (y_t = +1 and a_t < C_t) or (y_t = -1 and a_t > 0)};  I_low = {t: (y_t = +1 and a_t > 0) or (y_t = -1 and a_t < C_t)}.
 *   4. gmax = max of v over I_up and i the lowest row that attains it (-inf and no row when I_up is empty); gmin = min of v over
 *      I_low (+inf when empty).  If gmax - gmin < eps: state 0, stop.  Otherwise, if it == max_iter: state 1, stop.
 *   5. For t in I_low with b = gmax - v_t > 0:  c = (K_ii + K_tt) - 2 K_it, replaced by TAU unless c > 0;  score_t = (b b) / c.
 *      j = the lowest row that attains the largest score.  No such row (every score NaN): state 2, stop.
 *   6. The pair, exactly as libsvm's Solver::Solve moves and clips it.  q = (K_ii + K_jj) - 2 K_ij, replaced by TAU unless q > 0.
 *      y_i != y_j:  d = (-G_i - G_j) / q;  diff = a_i - a_j;  a_i += d;  a_j += d;
 *                   diff > 0:  if a_j < 0 then a_j = 0, a_i = diff;          else:  if a_i < 0 then a_i = 0, a_j = -diff;
 *                   diff > C_i - C_j:  if a_i > C_i then a_i = C_i, a_j = C_i - diff;
 *                   else:              if a_j > C_j then a_j = C_j, a_i = C_j + diff.
 *      y_i == y_j:  d = (G_i - G_j) / q;  sum = a_i + a_j;  a_i -= d;  a_j += d;
 *                   sum > C_i:  if a_i > C_i then a_i = C_i, a_j = sum - C_i;   else:  if a_j < 0 then a_j = 0, a_i = sum;
 *                   sum > C_j:  if a_j > C_j then a_j = C_j, a_i = sum - C_j;   else:  if a_i < 0 then a_i = 0, a_j = sum.
 *   7. With da_i, da_j the changes of the two:  G_t = G_t + ((y_t y_i K_it) da_i + (y_t y_j K_jt) da_j) for every t (rows i and j
 *      of K are the ones read);  it = it + 1;  back to 2.
 *   8. n_iter = it.  State 0 or 1:  rho = -(the sum of v_t over the free rows, 0 < a_t < C_t, added one by one in rising t from
 *      0.0) / their count, or -(gmax + gmin) / 2 of the last step 4 when no row is free;
 *      dec_e = (the sum over the rows s with a_s > 0, in rising s from 0.0, of (a_s y_s) K[e * ld + rows[s]]) - rho.
 *      State 2:  rho and every dec_e are the quiet NaN 0x7ff8000000000000; alpha is what the solve had reached.
 * A NaN in K therefore ends a solve (its gradient stops being finite), and every loop is bounded by max_iter.
 *
 * Refused before anything is launched or written (WDX_ERR_INVALID; the context stays usable): m < 1, ld < m, a negative count,
 * eps not positive and finite, max_iter < 0, a NULL K, table or output, a problem with an empty side, with more than
 * WDX_SVM_FIT_MAX_ROWS rows (warpdemux_amd/csrc/wdx_svm_fit_plan.h derives the cap), with a c that is not positive and finite,
 * with a list range outside its list, or with a row or evaluation row outside 0 .. m-1.  n_problems == 0 is success.
 *
 * wdx_svm_solve_device: d_K and the five outputs are DEVICE memory; the problem table and the two lists are HOST memory, read
 * during the call only (a row index is checked before it can reach a kernel; the call uploads them through a page-locked block
 * of the context, as wdx_medoids_device does its labels).  Enqueued on `stream`; no synchronisation -- the contract of the *_dev
 * entries (a row of the table of the _device entries: wdx_medoids_device says where it is held).  Only K[r * ld + c] with r and c
 * among the rows and evaluation rows named is read: columns m .. ld-1 of K are never read, and K ends on element (m-1) ld + m - 1.
 * Outputs of different problems must not overlap;
 * d_alpha is the solve's working storage too (what it held before the call is ignored, and it must not be read before the call's
 * work on the stream has run).  Timed as WDX_K_SVM_FIT. */
#define WDX_SVM_FIT_MAX_ROWS 16384
typedef struct wdx_svm_problem {
    int64_t row0;    /* first of the problem's n_pos + n_neg entries of the row list, and of its alpha values */
    int64_t eval0;   /* first of its n_eval entries of the evaluation list, and of its dec values              */
    int32_t n_pos, n_neg, n_eval, reserved_;
    double c_pos, c_neg;
} wdx_svm_problem;
int wdx_svm_solve_device(wdx_ctx *ctx, const float *d_K, int64_t m, int64_t ld, const wdx_svm_problem *problems /* HOST */,
                         int64_t n_problems, const int32_t *rows /* HOST */, int64_t n_rows, const int32_t *eval_rows /* HOST */,
                         int64_t n_eval, double eps, int64_t max_iter, double *d_alpha, double *d_rho, int64_t *d_n_iter,
                         int32_t *d_state, double *d_dec, void *stream);
/* Host form: every array HOST memory; one synchronisation.  A K with an entry (of its m x m part) that is not finite is
 * WDX_ERR_INVALID.  The device copy of K lives for the call only. */
int wdx_svm_solve(wdx_ctx *ctx, const float *K, int64_t m, int64_t ld, const wdx_svm_problem *problems, int64_t n_problems,
                  const int32_t *rows, int64_t n_rows, const int32_t *eval_rows, int64_t n_eval, double eps, int64_t max_iter,
                  double *alpha, double *rho, int64_t *n_iter, int32_t *state, double *dec);

/* ---- the kernel matrix of a DTW kernel machine, on the device ------------------------------------------------------------------
 * K = exp(-gamma D^p) of the float32 self-distance matrix D (m, m) with leading dimension ld (wdx_self_matrix_device leaves it on
 * the device), so that a fit, a cross-validation or a sweep over gamma never moves a matrix over the bus.
 *
 * THE RULE, per entry, in float64 with every operation rounded on its own (nothing is contracted into a fused multiply-add):
 *     t = (double)D_ij;   w = t, then pwr_dist - 1 times w = w * t;   x = -(gamma * w);
 *     K_ij = (float)exp_rule(x)   (round to nearest even);   x NaN: K_ij = (float)x, a NaN.
 * exp_rule is the engine's stated exponential (the one wdx_boost_fit_device's softmax uses):  0 for x < -700;  otherwise
 *     kk = rint(x * LOG2E);   r = (x - kk * LN2_HI) - kk * LN2_LO;   P = c_13, then for i = 12 .. 0: P = P * r, P = P + c_i;
 *     exp_rule(x) = ldexp(P, (int)kk)
 * with LOG2E = 0x1.71547652b82fep+0, LN2_HI = 0x1.62e42feep-1, LN2_LO = 0x1.a39ef35793c76p-33, c_0 = 1 and c_i = c_{i-1} / i.
 * A distance of +inf therefore gives 0 and a NaN (a row that is no member) gives NaN.  It is NOT numpy.exp: the host route of
 * models.DTW_SVM.fit computes K with NumPy from a float32 product, and an entry of the two matrices may differ by a few float32
 * ulps (profiles/svm_cv.json holds the measured distance).
 *
 * d_D and d_K are DEVICE memory.  d_K == d_D with ldk == ld is allowed (in place: 65 536 rows need one matrix, not two); any other
 * overlap of the two is not.  Columns from m on of either matrix are neither read nor written.  Refused before anything is
 * launched (the context stays usable): m < 1, ld < m, ldk < m, pwr_dist < 1, a gamma that is not positive and finite, a NULL
 * matrix (WDX_ERR_INVALID); m > WDX_SVM_KERNEL_MAX_ROWS or pwr_dist > WDX_SVM_KERNEL_MAX_POWER (WDX_ERR_UNSUPPORTED).  Enqueued
 * on `stream`; no synchronisation -- the contract of the *_dev entries (a row of the table of the _device entries: wdx_medoids_device
 * says where it is held).  Rows are read and written with 16-byte accesses when
 * both base pointers are 16-byte aligned and ld and ldk are multiples of four, entry by entry otherwise and at the ragged end of a
 * row: the same bits either way.  Timed as WDX_K_SVM_KERNEL. */
#define WDX_SVM_KERNEL_MAX_ROWS 1048576
#define WDX_SVM_KERNEL_MAX_POWER 16
int wdx_svm_kernel_device(wdx_ctx *ctx, const float *d_D, int64_t m, int64_t ld, double gamma, int32_t pwr_dist, float *d_K, int64_t ldk,
                       void *stream);

/* ---- cross-validated probabilities of a DTW kernel machine: behind the decision values ------------------------------------------
 * A cross-validation on one resident kernel matrix is ONE wdx_svm_solve_device launch (warpdemux_amd/_svm_cv.py states the plan):
 * every fold's one-vs-one problems and their Platt folds, each pair's full problem naming the fold's held-out rows H_f as its
 * evaluation rows.  Behind it the host fits probA / probB per (fold, pair) and this entry does, per held-out row, what the resident
 * tail (wdx_svm_predict_dev) does behind ITS decision values, with the same device code, so that equal decision values and equal
 * probA / probB give equal bits:  libsvm's sigmoid_predict per pair, clamped to [1e-7, 1 - 1e-7];  libsvm's
 * multiclass_probability;  pred_idx = np.argmax (the first maximum);  conf = top1 - top2.
 *
 * Row i of fold f (the i-th entry of its held-out list, held[held_off[f] + i]) takes pair p's decision value from
 * d_dec[dec_off[f * pairs + p] + i], pairs = k (k - 1) / 2 in libsvm's order (0, 1), (0, 2), ..; probA / probB [f * pairs + p].
 * Outputs in MEMBER-ROW order: d_prob (m, k) float64, d_pred_idx int32[m] (the class INDEX: no label map, no threshold),
 * d_conf float64[m]; a row no fold holds out is not written, a row named twice gets one of its results.  A row with a NaN
 * decision value (a problem that ended in state 2) gets NaN probabilities, pred_idx -1 and a NaN margin.
 *
 * d_dec and the outputs are DEVICE memory; the five tables are HOST memory, read during the call only (checked before anything is
 * launched, uploaded through a page-locked block of the context).  Refused (WDX_ERR_INVALID; the context stays usable): k outside
 * 2 .. WDX_SVM_CV_MAX_CLASSES, n_folds outside 1 .. WDX_SVM_CV_MAX_FOLDS, m < 1, a NULL table or output, held_off that does not
 * start at 0 or decreases, a block outside the n_dec decision values, a held-out row outside 0 .. m-1.  No held-out rows: success.
 * Enqueued on `stream`; no synchronisation -- the contract of the *_dev entries.  Timed as WDX_K_SVM_CV_COUPLE. */
#define WDX_SVM_CV_MAX_CLASSES 16
#define WDX_SVM_CV_MAX_FOLDS 16
int wdx_svm_cv_couple_device(wdx_ctx *ctx, const double *d_dec, int64_t n_dec, int32_t k, int32_t n_folds, const int64_t *dec_off /* HOST */,
                          const double *probA /* HOST */, const double *probB /* HOST */, const int32_t *held /* HOST */,
                          const int64_t *held_off /* HOST */, int64_t m, double *d_prob, int32_t *d_pred_idx, double *d_conf, void *stream);

/* ---- accuracy thresholds from probabilities and labels ---------------------------------------------------------------------------
 * What a shipped model carries and a fitted one lacked: per predicted class the confidence margin below which a read is left
 * uncalled (process_probs: `-1` when top1 - top2 < thresholds[pred_idx]), chosen so that the calls that remain reach a target
 * accuracy on labelled probabilities -- held-out ones, or a whole labelled shard that wdx_demux_svm_dev / wdx_demux_mlp_dev /
 * wdx_demux_boost_dev left in device memory.  The reference ships such tables (target_accuracy_thresholds/) but not the procedure
 * that made them: THE RULE below is this engine's own, and it is integer and order-free.
 *   Rows.        prob (n, k) float64, contiguous; y_idx int32[n].  A row is USED when y_idx >= 0 and each of its k probabilities is
 *                finite; the others are counted in `skipped`.  (A y_idx >= k is used, and no prediction hits it.)
 *   Prediction.  p = the first maximum of the row; conf = top1 - top2 in float64, top2 the largest of the other k - 1 entries.
 *   Grid.        g_i = (double)i / (double)R for i = 0 .. R, one IEEE division each.  bin = the largest i with g_i <= conf (conf
 *                >= 0 = g_0; a conf beyond 1 lands in bin R).
 *   Histograms.  N[p][bin] += 1;  H[p][bin] += (p == y_idx).
 *   Suffix sums. kept[c][j] = the sum of N[c][b] over b >= j;  hit[c][j] = the same of H: the rows called c whose margin is at
 *                least g_j, and those of them that are right.
 *   Threshold.   thr[t][c] = g_j for the SMALLEST j in 1 .. R with kept[c][j] > 0 and 1000 * hit[c][j] >= targets_pm[t] *
 *                kept[c][j] (int64: exact); +inf when no j qualifies -- every read called c is then left uncalled.  j >= 1: the
 *                reference's tables bottom out at 0.01.
 * Limits (WDX_ERR_INVALID outside them, before anything is launched; the context stays usable): 0 <= n, 2 <= k <=
 * WDX_THRESHOLDS_MAX_CLASSES, 1 <= resolution R <= WDX_THRESHOLDS_MAX_RESOLUTION, 1 <= n_targets <= WDX_THRESHOLDS_MAX_TARGETS,
 * 0 <= targets_pm[t] <= 1000 (per mille); n > WDX_THRESHOLDS_MAX_ROWS is WDX_ERR_UNSUPPORTED.
 *
 * wdx_accuracy_thresholds_device: d_prob, d_y_idx and the outputs are DEVICE memory; targets_pm is HOST memory, read during the call
 * only.  d_thr (n_targets, k) float64 is required; d_kept and d_hit, (k, R + 1) int64 each, and d_skipped, one int64, are
 * nullable (the context keeps what the caller does not want).  Enqueued on `stream`; no synchronisation -- the contract of the
 * *_dev entries.  All sums are integers added by integer atomics: two runs give the same bits.  Timed as WDX_K_THRESHOLDS. */
#define WDX_THRESHOLDS_MAX_CLASSES 16
#define WDX_THRESHOLDS_MAX_RESOLUTION 4096
#define WDX_THRESHOLDS_MAX_TARGETS 16
#define WDX_THRESHOLDS_MAX_ROWS 1099511627776
int wdx_accuracy_thresholds_device(wdx_ctx *ctx, const double *d_prob, int64_t n, int32_t k, const int32_t *d_y_idx, int32_t resolution,
                                const int32_t *targets_pm /* HOST */, int32_t n_targets, double *d_thr, int64_t *d_kept, int64_t *d_hit,
                                int64_t *d_skipped, void *stream);
/* Host form: every array HOST memory (kept, hit and skipped nullable); one synchronisation.  The device copies live for the call
 * only. */
int wdx_accuracy_thresholds(wdx_ctx *ctx, const double *prob, int64_t n, int32_t k, const int32_t *y_idx, int32_t resolution,
                            const int32_t *targets_pm, int32_t n_targets, double *thr, int64_t *kept, int64_t *hit, int64_t *skipped);

/* Pipelined form of wdx_demux_batch for the reference's worker loop (file_proc.py:380-454: fill minibatch k+1
 * while minibatch k is processed; 1197-1243: several such workers share one GPU).  A context has WDX_MAX_SLOTS slots (the
 * worker loop uses two; a feeder that serves many producers keeps more minibatches in flight), each with its own stream
 * and device workspaces:
 *   wdx_demux_submit(ctx, slot, ...)  enqueues copy-in, fingerprint, DTW, call and copy-out of one minibatch on the
 *                                     slot's stream and returns; WDX_ERR_INVALID if the slot still holds a batch.
 *                                     The input arrays must stay untouched until the matching wait returns (rows in
 *                                     page-locked memory -- wdx_host_alloc -- are copied by DMA at the bus rate and the
 *                                     call returns at once; pageable rows are staged by the runtime first).
 *   wdx_demux_wait(ctx, slot, ...)    blocks until that minibatch is done and hands the results over (same outputs
 *                                     and meanings as wdx_demux_batch; fpt / dist only if requested at submit).
 * Submitting slot 1 while slot 0 is in flight overlaps its host->device copy with slot 0's kernels.  Results are
 * bit-identical to wdx_demux_batch.  wdx_set_refs waits for every slot before it changes the resident set. */
#define WDX_MAX_SLOTS 8
int wdx_demux_submit(wdx_ctx *ctx, int32_t slot, const float *sig, int64_t n_reads, int64_t stride,
                     const int32_t *a_start, const int32_t *a_end, const uint8_t *ok, const wdx_seg_params *p,
                     int64_t n_refs, int32_t want_fpt, int32_t want_dist);
int wdx_demux_wait(wdx_ctx *ctx, int32_t slot, double *fpt, float *dist, int32_t *call, int32_t *status);
/* The same pipeline with everything the reference's worker needs from a minibatch (file_proc.py:380-454: the
 * ReadResults -- fingerprint, dwell times, six statistics, sig_proc.py:562-605 -- AND model.predict of the stacked
 * fingerprints, models/dtw_svm.py:54-98) produced by ONE pass over the rows:
 *   wdx_demux_submit_ex(ctx, slot, in, p, n_refs, want)   `want` = WDX_WANT_* bits; status and call always come back.
 *                                                         in->row_off != NULL: the rows are PACKED -- row r holds only the
 *                                                         samples the kernels read, sig[row_off[r] .. + row_len[r]), and
 *                                                         a_start / a_end are relative to it (what a worker that copies
 *                                                         [a_start - padding, a_end + padding) of each read hands over:
 *                                                         half the bytes of the NaN-padded rows); row_off[r] % 4 == 0.
 *                                                         WDX_WANT_SVM needs wdx_svm_set_model (a model trained on the
 *                                                         resident references); reads whose fingerprint failed get
 *                                                         pred -1 and NaN prob / conf, like wdx_demux_svm_dev.
 *   wdx_demux_wait_ex(ctx, slot, out)                     out->X may be NULL for anything; an output that was not asked
 *                                                         for at submit is WDX_ERR_INVALID and leaves the slot busy.
 * Bit-identical to wdx_fingerprint_batch / wdx_demux_batch / wdx_dtw_svm_predict on the same rows. */
#define WDX_WANT_FPT 0x01u   /* fpt   (n, K) float64                                      */
#define WDX_WANT_DIST 0x02u  /* dist  (n, n_refs) float32                                 */
#define WDX_WANT_DWELL 0x04u /* dwell (n, K) int64                                        */
#define WDX_WANT_STATS 0x08u /* stats (n, 6) float64 (order: wdx_fingerprint_batch)       */
#define WDX_WANT_SVM 0x10u   /* prob (n, k) float64, pred int32[n], conf float64[n]       */
/* WDX_WANT_BOOST (0x40, below WDX_WANT_REFINE_IDX): prob / pred / conf of the resident BOOST model (wdx_boost_set_model) on
 * the fingerprints this minibatch produced -- the tRNA models' classifier; wdx_demux_submit_ex, _adc and _refine take it.
 *   - never together with WDX_WANT_SVM (WDX_ERR_INVALID); without a resident boost model WDX_ERR_NO_REFS; K (refine:
 *     rp->barcode_keep_events) must equal the model's n_features (WDX_ERR_INVALID); a refused submit leaves the slot free
 *   - n_refs == 0 is legal on wdx_demux_submit_ex / _adc when, and only when, this bit is set: no reference set is needed,
 *     call is -1 for every read, WDX_WANT_DIST is WDX_ERR_INVALID.  With resident references and n_refs = nY the DTW, call
 *     and dist run as before, beside the boost tail
 *   - a read whose status is not 0 gets pred -1 and NaN prob / conf
 *   - wdx_demux_wait_ex / _refine hand prob / pred / conf over when the slot asked for either tail
 * Bit-identical to wdx_fingerprint[_refine]_batch followed by wdx_boost_predict on those fingerprints. */
typedef struct wdx_minibatch_in {
    const float *sig;          /* (n_reads, stride) rows, or the packed rows when row_off != NULL             */
    int64_t n_reads, stride;   /* stride is ignored for packed rows                                          */
    const int64_t *row_off;    /* packed: int64[n_reads + 1], multiples of 4; NULL = minibatch layout        */
    const int32_t *row_len;    /* packed: samples of row r (<= row_off[r+1] - row_off[r])                    */
    const int32_t *a_start, *a_end;
    const uint8_t *ok;         /* nullable                                                                    */
} wdx_minibatch_in;
typedef struct wdx_minibatch_out {
    int32_t *status, *call;
    float *dist;
    double *fpt;
    int64_t *dwell;
    double *stats, *prob;
    int32_t *pred;
    double *conf;
} wdx_minibatch_out;
int wdx_demux_submit_ex(wdx_ctx *ctx, int32_t slot, const wdx_minibatch_in *in, const wdx_seg_params *p, int64_t n_refs,
                        uint32_t want);
int wdx_demux_wait_ex(wdx_ctx *ctx, int32_t slot, const wdx_minibatch_out *out);
/* ---- raw int16 ADC minibatches, calibrated on the device -------------------------------------------------------
 * The reference's reader makes its float32 rows from int16 ADC samples (file_proc.py:258, read_record.signal_pa); a
 * caller that hands over the int16 samples and the two calibration numbers of every read moves 2 bytes per sample
 * over the bus instead of 4.  THE CONTRACT: read r with row_len[r] samples adc, offset[r], scale[r] stands for the
 * float32 row
 *     pa[i] = scale[r] * ((float)adc[i] + offset[r])    i < row_len[r]     float32 add, THEN float32 multiply: two
 *                                                                          roundings, never one fused operation
 *     pa[i] = NaN                                       row_len[r] <= i < stride
 * (the calibrated samples, then the NaN tail of file_proc.py:255-260; NumPy form: warpdemux_amd.sig_proc.calibrate_adc),
 * and every *_adc entry point returns, bit for bit, what its float32 counterpart returns on those rows -- status,
 * fingerprints, dwell times, statistics, distances, call, prob / pred / conf, failed reads and windows that run into
 * the NaN tail included.  A caller whose reader calibrates by another formula must not use this path.
 * Two copy kernels do the work ahead of the unchanged fingerprint chain (wdx_adc.hip): pack_windows_adc_kernel reads
 * the adapter windows of a page-locked minibatch over the bus, decode_adc_kernel decodes rows that arrived by a DMA
 * copy (pageable minibatches, rows the caller packed). */
typedef struct wdx_minibatch_adc_in {
    const int16_t *adc;        /* (n_reads, stride) int16 rows, or the packed rows when row_off != NULL                */
    int64_t n_reads, stride;   /* stride = samples of the float32 row (NaN tail included); ignored for packed rows     */
    const int32_t *row_len;    /* REQUIRED: ADC samples of read r, 0 .. stride (there is no NaN tail to find the end by) */
    const float *offset, *scale; /* REQUIRED: float32[n_reads] calibration of every read                               */
    const int64_t *row_off;    /* packed: int64[n_reads + 1], multiples of 8, row r holds its row_len[r] samples at
                                  adc[row_off[r] ..); a_start / a_end are relative to the row; NULL = minibatch layout */
    const int32_t *row_win;    /* packed only, nullable: samples of the float32 row r stands for, row_win[r] - row_len[r]
                                  of them the NaN tail (a worker that copies a window which runs past the read's end);
                                  NULL = row_len                                                                        */
    const int32_t *a_start, *a_end;
    const uint8_t *ok;         /* nullable                                                                              */
} wdx_minibatch_adc_in;
/* wdx_demux_submit_ex for int16 rows (pair it with wdx_demux_wait_ex): the same three ways in -- 2-D copy of the column
 * range, window pack over the bus for a page-locked minibatch, rows the caller packed.  WDX_ERR_INVALID: row_len /
 * offset / scale NULL, row_len[r] outside 0 .. stride (packed: beyond the row's slice), row_off not ascending in
 * multiples of 8. */
int wdx_demux_submit_adc(wdx_ctx *ctx, int32_t slot, const wdx_minibatch_adc_in *in, const wdx_seg_params *p, int64_t n_refs,
                         uint32_t want);
/* Blocking forms on the context's own stream: wdx_fingerprint_batch / wdx_demux_batch for int16 rows (outputs as there). */
int wdx_fingerprint_batch_adc(wdx_ctx *ctx, const wdx_minibatch_adc_in *in, const wdx_seg_params *p, double *fpt,
                              int64_t *dwell, double *stats, int32_t *status);
int wdx_demux_batch_adc(wdx_ctx *ctx, const wdx_minibatch_adc_in *in, const wdx_seg_params *p, int64_t n_refs, double *fpt,
                        float *dist, int32_t *call, int32_t *status);
/* The decode alone, on DEVICE buffers: d_out (n_reads, stride) float32 = the rows of the contract above.  d_adc:
 * (n_reads, stride) int16, or packed rows at d_row_off int64[n_reads] (multiples of 8; NULL = r * stride); d_row_len
 * int32[n_reads] (clamped to 0 .. stride); d_offset / d_scale float32[n_reads].  Enqueued on `stream`; no
 * synchronisation. */
int wdx_calibrate_adc_dev(wdx_ctx *ctx, const int16_t *d_adc, const int64_t *d_row_off, const int32_t *d_row_len,
                          int64_t stride, int64_t n_reads, const float *d_offset, const float *d_scale, float *d_out,
                          void *stream);
/* ---- int16 ADC shards that STAY on the device: the *_adc_dev twins of the device-resident entries ------------------
 * A caller who holds what a pod5 file holds keeps its shard int16 in HBM -- 2 bytes per sample instead of the 4 of a float32
 * copy -- and float32 exists only for the reads in flight.  An int16 device shard (all pointers DEVICE memory):
 *   adc                      the samples, in one of two layouts:
 *                              strided   row_off == NULL: (n_reads, stride) int16 rows
 *                              packed    row_off int64[n_reads + 1], every entry a multiple of 8 (A PRECONDITION: these are
 *                                        device arrays, nothing is checked synchronously; as for wdx_calibrate_adc_dev);
 *                                        read r holds its samples at adc[row_off[r] ..)
 *   row_len  int32[n_reads]  REQUIRED: ADC samples of read r; clamped to the row (0 .. stride; packed: 0 .. row_off[r+1] -
 *                            row_off[r]), as wdx_calibrate_adc_dev clamps it
 *   offset, scale            REQUIRED: float32[n_reads]
 *   row_win  int32[n_reads]  nullable, packed only: as wdx_minibatch_adc_in.row_win -- samples of the float32 row read r
 *                            stands for, row_win[r] - row_len[r] of them the NaN tail; NULL (or less than row_len) = row_len
 * THE CONTRACT is the one above: read r stands for the float32 row pa[i] = scale[r] * ((float)adc[i] + offset[r]) for
 * i < row_len[r] (float32 add, THEN float32 multiply: two roundings, never fused), NaN from there to `stride` (strided) or
 * row_win[r] (packed); a_start / a_end are relative to the row.  Every *_adc_dev entry returns, bit for bit, what its
 * float32 twin returns on those rows -- status, fpt, dwell, stats, refine_idx, dist, call, the INCREMENTED counts, prob /
 * pred / conf / n_nonfinite; failed detections, empty and inverted windows, windows that run into the NaN tail and whatever
 * WDX_OPT_LONG_WINDOWS / WDX_OPT_LONG_REFINE_WINDOWS select on the context included.  A caller whose reader calibrates by
 * another formula must not use this path.
 * How: the reads are walked in slices.  adc_dev_windows_kernel (wdx_adc.hip) decodes the adapter window of every read of a
 * slice -- the window rule of the host ways in, start rounded down to a multiple of 8 samples -- into a context-owned
 * float32 staging block of at most 1 GiB, the float32 twin's own body runs on that block and writes its outputs at the
 * slice's read offset, the next slice reuses the block in stream order: no host synchronisation, and the staging never
 * depends on the size of the shard.  Arguments other than `in` are those of the float32 twin (max_len bounds the adapter
 * windows as there; a window beyond it is reported WDX_READ_FAIL_UNKNOWN as there).  d_work: the *_adc_workspace_bytes of
 * the same context, n_reads, max_len and K (they depend on the context's WDX_OPT_ADC_DEV_SLICE_READS and long-window options:
 * ask after setting those).  n_reads == 0 returns what the twin returns. */
typedef struct wdx_adc_dev_in {
    const int16_t *adc;
    const int64_t *row_off;      /* packed: int64[n_reads + 1], multiples of 8; NULL = strided              */
    int64_t stride;              /* strided: samples of a row (= of the float32 row); ignored when packed   */
    const int32_t *row_len;      /* REQUIRED                                                                */
    const float *offset, *scale; /* REQUIRED                                                                */
    const int32_t *row_win;      /* packed only, nullable                                                   */
} wdx_adc_dev_in;
int wdx_fingerprint_adc_dev(wdx_ctx *ctx, const wdx_adc_dev_in *in, int64_t max_len, int64_t n_reads,
                            const int32_t *d_a_start, const int32_t *d_a_end, const uint8_t *d_ok, const wdx_seg_params *p,
                            double *d_fpt, int64_t *d_dwell, double *d_stats, int32_t *d_status, void *stream);
int wdx_fingerprint_refine_adc_dev(wdx_ctx *ctx, const wdx_adc_dev_in *in, int64_t max_len, int64_t n_reads,
                                   const int32_t *d_a_start, const int32_t *d_a_end, const uint8_t *d_ok,
                                   const wdx_seg_params *p, const wdx_refine_params *rp, double *d_fpt, int64_t *d_dwell,
                                   double *d_stats, int32_t *d_refine_idx, int32_t *d_status, void *stream);
/* d_work of wdx_demux_adc_dev / _svm_adc_dev / _mlp_adc_dev and of wdx_demux_boost_adc_dev without rp: the float32 twin's
 * workspace for the largest slice; ..._refine_...: of wdx_demux_refine_adc_dev and wdx_demux_boost_adc_dev with rp.  0 on
 * bad arguments.  Neither holds the staging block: the context owns it. */
int64_t wdx_demux_adc_workspace_bytes(wdx_ctx *ctx, int64_t n_reads, int64_t max_len, int32_t barcode_num_events);
int64_t wdx_demux_refine_adc_workspace_bytes(wdx_ctx *ctx, int64_t n_reads, int64_t max_len, int32_t barcode_keep_events);
/* Device bytes of the staging block a call with these arguments needs (the context keeps the largest so far; at most
 * 1 GiB); refine != 0: for the consensus-refinement entries. */
int64_t wdx_adc_dev_staging_bytes(wdx_ctx *ctx, int64_t n_reads, int64_t max_len, int32_t refine);
int wdx_demux_adc_dev(wdx_ctx *ctx, const wdx_adc_dev_in *in, int64_t max_len, int64_t n_reads, const int32_t *d_a_start,
                      const int32_t *d_a_end, const uint8_t *d_ok, const wdx_seg_params *p, double *d_fpt, int64_t *d_dwell,
                      double *d_stats, int32_t *d_status, float *d_dist, int32_t *d_call, int64_t *d_counts, void *d_work,
                      void *stream);
int wdx_demux_refine_adc_dev(wdx_ctx *ctx, const wdx_adc_dev_in *in, int64_t max_len, int64_t n_reads,
                             const int32_t *d_a_start, const int32_t *d_a_end, const uint8_t *d_ok, const wdx_seg_params *p,
                             const wdx_refine_params *rp, double *d_fpt, int64_t *d_dwell, double *d_stats,
                             int32_t *d_refine_idx, int32_t *d_status, float *d_dist, int32_t *d_call, int64_t *d_counts,
                             void *d_work, void *stream);
int wdx_demux_svm_adc_dev(wdx_ctx *ctx, const wdx_adc_dev_in *in, int64_t max_len, int64_t n_reads, const int32_t *d_a_start,
                          const int32_t *d_a_end, const uint8_t *d_ok, const wdx_seg_params *p, double *d_fpt,
                          int32_t *d_status, float *d_dist, double *d_prob, int32_t *d_pred, double *d_conf, void *d_work,
                          int64_t block_rows, void *stream);
int wdx_demux_mlp_adc_dev(wdx_ctx *ctx, const wdx_adc_dev_in *in, int64_t max_len, int64_t n_reads, const int32_t *d_a_start,
                          const int32_t *d_a_end, const uint8_t *d_ok, const wdx_seg_params *p, double *d_fpt,
                          int32_t *d_status, float *d_dist, double *d_prob, int32_t *d_pred, double *d_conf,
                          int64_t *d_n_nonfinite, void *d_work, int64_t block_rows, void *stream);
int wdx_demux_boost_adc_dev(wdx_ctx *ctx, const wdx_adc_dev_in *in, int64_t max_len, int64_t n_reads,
                            const int32_t *d_a_start, const int32_t *d_a_end, const uint8_t *d_ok, const wdx_seg_params *p,
                            const wdx_refine_params *rp, double *d_fpt, int32_t *d_refine_idx, int32_t *d_status,
                            double *d_raw, double *d_prob, int32_t *d_pred, double *d_conf, void *d_work, void *stream);
/* ---- consensus refinement (wdx_refine_params) through the pipelined minibatches ----------------------------------
 * The tRNA models' branch on the same slots, for float32 rows (`in`) or int16 ADC rows (`in_adc`): exactly one of the
 * two is non-NULL, and all three ways in of either format work as above.  K = rp->barcode_keep_events for fpt, dwell and
 * the DTW (p->barcode_num_events is ignored, as in wdx_fingerprint_refine_batch); rp and its query are HOST memory and
 * are copied before the call returns, so slots in flight may carry different rp.
 *   n_refs > 0    DTW against the resident references: K must equal their length and n_refs the resident nY
 *                 (WDX_ERR_INVALID otherwise); WDX_WANT_SVM as in wdx_demux_submit_ex -- a read whose status is not 0,
 *                 WDX_READ_FAIL_CONSENSUS included, gets pred -1 and NaN prob / conf
 *   n_refs == 0   fingerprint only: no resident references are needed, nothing behind the fingerprint stage runs, call
 *                 is -1 for every read; WDX_WANT_DIST / WDX_WANT_SVM are WDX_ERR_INVALID (WDX_WANT_BOOST is served: the boost
 *                 tail needs no references)
 * Limits and their codes are those of wdx_fingerprint_refine_batch (n_query 1..96, num_events <= 127).
 * WDX_WANT_REFINE_IDX asks for refine_idx (n, 3) int32 -- the numbers wdx_fingerprint_refine_batch returns for the same
 * reads, whichever way the rows came in: sig_barcode_start counts from the first sample of the read's adapter window
 * (max(0, a_start - padding) of ITS row), which no packing, cropping or decoding moves.
 * wdx_demux_wait_refine is wdx_demux_wait_ex plus refine_idx: required when the slot asked for it, WDX_ERR_INVALID (the
 * slot stays busy) when it did not; wdx_demux_wait_ex completes a refine slot that did not ask for refine_idx and refuses
 * one that did.  Bit-identical to wdx_fingerprint_refine_batch [+ wdx_dtw_matrix + wdx_dtw_svm_predict] on the same rows. */
#define WDX_WANT_REFINE_IDX 0x20u /* refine_idx (n, 3) int32, as wdx_fingerprint_refine_batch */
#define WDX_WANT_BOOST 0x40u      /* prob (n, k) float64, pred int32[n], conf float64[n] of the resident boost model */
int wdx_demux_submit_refine(wdx_ctx *ctx, int32_t slot, const wdx_minibatch_in *in, const wdx_minibatch_adc_in *in_adc,
                            const wdx_seg_params *p, const wdx_refine_params *rp, int64_t n_refs, uint32_t want);
int wdx_demux_wait_refine(wdx_ctx *ctx, int32_t slot, const wdx_minibatch_out *out, int32_t *refine_idx);
/* wdx_demux_dev with the refinement branch in front: refine fingerprint (K = rp->barcode_keep_events = the reference
 * length) -> DTW -> argmin -> histogram, enqueued on `stream`; d_counts slot nY counts every read whose status is not 0.
 * d_refine_idx (n_reads, 3) int32 DEVICE, nullable.  rp and its query are HOST memory (copied before the call returns).
 * d_work: wdx_demux_refine_workspace_bytes(n_reads, K) bytes = wdx_demux_workspace_bytes plus the refinement kernels'
 * hand-over records (1 632 bytes per read). */
int64_t wdx_demux_refine_workspace_bytes(int64_t n_reads, int32_t barcode_keep_events);
int wdx_demux_refine_dev(wdx_ctx *ctx, const float *d_sig, const int64_t *d_row_off, const int32_t *d_row_len,
                         int64_t stride, int64_t max_len, int64_t n_reads, const int32_t *d_a_start,
                         const int32_t *d_a_end, const uint8_t *d_ok, const wdx_seg_params *p,
                         const wdx_refine_params *rp, double *d_fpt, int64_t *d_dwell, double *d_stats,
                         int32_t *d_refine_idx, int32_t *d_status, float *d_dist, int32_t *d_call, int64_t *d_counts,
                         void *d_work, void *stream);
/* Page-locked host memory for minibatch buffers the caller fills (what file_proc.py:244-260 allocates with
 * np.full): the GPU reads it directly.  Needs no context; free with wdx_host_free. */
int wdx_host_alloc(size_t bytes, void **out);
/* the same with `device` made current for the allocation (a multi-GPU worker whose context lives on device N: the
 * plain call initialises HIP on the process's current device) */
int wdx_host_alloc_on(int device, size_t bytes, void **out);
int wdx_host_free(void *p);
/* Page-lock memory the caller already owns -- e.g. a shared-memory ring that producer PROCESSES fill while one feeder
 * process owns the context and submits (tools/host_workers.py --mode feeder) -- so that it is read like wdx_host_alloc
 * memory.  Undo with wdx_host_unregister before the memory is unmapped. */
int wdx_host_register(void *p, size_t bytes);
int wdx_host_unregister(void *p);

/* ---- many worker processes, ONE GPU-facing process (replaces the reference's per-worker GPU use in its `-j 8..16`
 *      forked workers, file_proc.py:1197-1243, 380-454).  Sixteen HIP processes on one device run at 40 % of the rate of
 *      four; one process that owns the context and keeps up to WDX_MAX_SLOTS minibatches in flight for everybody does not
 *      have that problem.  The ring lives in shared memory the caller maps in every process (parent: create + init BEFORE
 *      the fork; Python: warpdemux_amd.feeder.Feeder):
 *        wdx_feeder_ring_bytes / _init   size and lay out the ring: n_slots (<= WDX_FEEDER_MAX_RING_SLOTS) minibatches of at
 *                                        most max_reads x max_stride float32 samples, distances to n_refs references,
 *                                        n_events > 0: room for fingerprints / dwell times / statistics (K = n_events =
 *                                        p->barcode_num_events), n_classes > 0: room for the DTW_SVM outputs.  `p` = the
 *                                        parameters every minibatch is fingerprinted with (kept in the ring: the workers
 *                                        pack their rows with its `padding`).
 *                                        (A worker holds its ring slot while it copies its windows in and the results out;
 *                                        the feeder keeps at most WDX_MAX_SLOTS of the READY ones in flight on the device.)
 *        wdx_feeder_serve(ctx, ring)     the GPU-facing process: page-locks the ring and serves it until wdx_feeder_stop --
 *                                        every READY slot goes through wdx_demux_submit_ex, the oldest in flight through
 *                                        wdx_demux_wait_ex; the context's resident references (wdx_set_refs) classify, its
 *                                        resident model (wdx_svm_set_model) serves WDX_WANT_SVM and wdx_feeder_predict
 *        wdx_feeder_run(ring, job)       a worker: one minibatch, `job->want` = WDX_WANT_* bits -- what the reference's
 *                                        worker needs from it (file_proc.py:380-454): status + fpt + dwell + stats (the
 *                                        ReadResults, = wdx_fingerprint_batch), call + dist (= wdx_demux_batch), prob +
 *                                        pred + conf (= model.predict of the stacked fingerprints, models/dtw_svm.py:54-98;
 *                                        failed reads: pred -1, NaN) -- from ONE pass, bit-identical to those calls.  No
 *                                        context and NO HIP call: only samples [a_start - padding, a_end + padding) of each
 *                                        row are copied into a free slot (packed rows), the worker sleeps on the slot
 *                                        (futex) until the results are there.  WDX_ERR_NO_DEVICE when the feeder has
 *                                        stopped or died (a dead feeder is noticed even while it is an unreaped zombie)
 *        wdx_feeder_run_adc(ring, job)   the same for a ring whose slots hold int16 ADC samples (geometry.sample_format =
 *                                        WDX_FEEDER_SAMPLES_INT16): the worker copies the int16 windows and the reads'
 *                                        offset / scale, the server submits through wdx_demux_submit_adc -- half the bytes
 *                                        in the worker's memcpy, in the ring and over the bus; results bit-identical to
 *                                        wdx_feeder_run on the calibrated rows.  A float32 job on an int16 ring, and the
 *                                        reverse, is WDX_ERR_INVALID
 *        wdx_feeder_demux(ring, ...)     wdx_demux_batch's arguments through wdx_feeder_run (status, call, dist)
 *        wdx_feeder_predict(ring, X, ..) DTW_SVM.predict on (n, n_events) float64 fingerprints the worker holds
 *        wdx_feeder_predict_boost(..)    Fpt_Boost.predict on them: the server calls wdx_boost_predict
 *      WDX_WANT_BOOST in a job's `want` (plain and refine rings, rings with n_refs == 0 included; the ring needs n_classes > 0
 *      and n_events > 0; never together with WDX_WANT_SVM): prob / pred / conf of the serving context's boost model
 *      (wdx_boost_set_model).  Checked per minibatch: a model whose k is not the ring's n_classes, or whose n_features is not
 *      n_events, answers that minibatch WDX_ERR_INVALID and the ring keeps serving.  A plain ring with n_refs == 0 serves
 *      minibatches with WDX_WANT_BOOST only.
 *        wdx_feeder_stop(ring)           ends wdx_feeder_serve: minibatches in flight are finished and handed over, READY
 *                                        ones that were never submitted are answered WDX_ERR_NO_DEVICE, new claims are
 *                                        refused
 *      A worker that dies while it holds a slot does not leak it: the slot's owner pid is part of its state word, and the
 *      serve loop (and any claimant that finds the ring full) gives slots of dead owners back to the ring. */
#define WDX_FEEDER_MAX_RING_SLOTS 32
#define WDX_FEEDER_SAMPLES_FLOAT32 0 /* wdx_feeder_run / wdx_feeder_demux                                    */
#define WDX_FEEDER_SAMPLES_INT16 1   /* wdx_feeder_run_adc: 2 bytes per sample + offset / scale per read     */
typedef struct wdx_feeder_geometry {
    int32_t n_slots;
    int32_t n_events;    /* K of fpt / dwell (0: no room for WDX_WANT_FPT / _DWELL / _STATS)      */
    int32_t n_classes;   /* k of prob (0: no room for WDX_WANT_SVM / WDX_WANT_BOOST / wdx_feeder_predict[_boost]), <= 16 */
    int32_t sample_format; /* WDX_FEEDER_SAMPLES_*: what a slot's sample region holds (0 = float32)  */
    int64_t max_reads, max_stride, n_refs;
} wdx_feeder_geometry;
typedef struct wdx_feeder_job {
    const float *sig;          /* (n_reads, stride) float32 rows, NaN tail (file_proc.py:244-260)               */
    int64_t n_reads, stride;
    const int32_t *a_start, *a_end;
    const uint8_t *ok;         /* nullable                                                                       */
    uint32_t want, pad_;       /* WDX_WANT_* bits                                                                */
    /* outputs: caller-owned host arrays; status is required, call nullable, the others where their bit is set   */
    int32_t *status, *call;
    float *dist;               /* (n_reads, n_refs)                                                              */
    double *fpt;               /* (n_reads, n_events)                                                            */
    int64_t *dwell;            /* (n_reads, n_events)                                                            */
    double *stats;             /* (n_reads, 6)                                                                   */
    double *prob;              /* (n_reads, n_classes)                                                           */
    int32_t *pred;
    double *conf;
} wdx_feeder_job;
/* wdx_feeder_job for int16 rows: the minibatch as wdx_minibatch_adc_in's minibatch layout describes it */
typedef struct wdx_feeder_job_adc {
    const int16_t *adc;        /* (n_reads, stride) int16 rows                                                   */
    int64_t n_reads, stride;
    const int32_t *row_len;    /* ADC samples of read r, 0 .. stride                                             */
    const float *offset, *scale;
    const int32_t *a_start, *a_end;
    const uint8_t *ok;         /* nullable                                                                       */
    uint32_t want, pad_;
    int32_t *status, *call;    /* outputs as in wdx_feeder_job                                                   */
    float *dist;
    double *fpt;
    int64_t *dwell;
    double *stats;
    double *prob;
    int32_t *pred;
    double *conf;
} wdx_feeder_job_adc;
size_t wdx_feeder_ring_bytes(const wdx_feeder_geometry *g);
int wdx_feeder_ring_init(void *mem, size_t bytes, const wdx_feeder_geometry *g, const wdx_seg_params *p);
int wdx_feeder_serve(wdx_ctx *ctx, void *ring);
int wdx_feeder_run(void *ring, const wdx_feeder_job *job);
int wdx_feeder_run_adc(void *ring, const wdx_feeder_job_adc *job);
/* A ring whose minibatches take the consensus-refinement branch (tRNA models).  wdx_feeder_ring_bytes_refine /
 * wdx_feeder_ring_init_refine size and lay it out: the layout of wdx_feeder_ring_init, rp and its query (<= 96 doubles)
 * kept behind the ring header, and a refine_idx region per slot; n_events, when not 0, must equal
 * rp->barcode_keep_events; g->n_refs == 0 makes a fingerprint-only ring (the serving context needs no references; only
 * WDX_WANT_FPT / _DWELL / _STATS / _REFINE_IDX are served).  A bad rp is refused with the codes of
 * wdx_fingerprint_refine_batch.  A ring made by wdx_feeder_ring_init keeps its byte layout and behaviour.
 * wdx_feeder_serve, wdx_feeder_run and wdx_feeder_run_adc see the ring's kind and do the rest; wdx_feeder_run_refine is
 * either of the two run calls (exactly one job is non-NULL) plus refine_idx (n_reads, 3) int32, which
 * WDX_WANT_REFINE_IDX in the job's `want` asks for -- on a refine ring only, WDX_ERR_INVALID on another. */
size_t wdx_feeder_ring_bytes_refine(const wdx_feeder_geometry *g);
int wdx_feeder_ring_init_refine(void *mem, size_t bytes, const wdx_feeder_geometry *g, const wdx_seg_params *p,
                                const wdx_refine_params *rp);
int wdx_feeder_run_refine(void *ring, const wdx_feeder_job *job, const wdx_feeder_job_adc *job_adc, int32_t *refine_idx);
int wdx_feeder_demux(void *ring, const float *sig, int64_t n_reads, int64_t stride, const int32_t *a_start,
                     const int32_t *a_end, const uint8_t *ok, int64_t n_refs, float *dist, int32_t *call, int32_t *status);
int wdx_feeder_predict(void *ring, const double *X, int64_t n, double *prob, int32_t *pred, double *conf);
int wdx_feeder_predict_boost(void *ring, const double *X, int64_t n, double *prob, int32_t *pred, double *conf);
int wdx_feeder_stop(void *ring);
int wdx_feeder_served(void *ring, int64_t *minibatches);   /* minibatches handed back so far */
/* served minibatches, slots taken back from dead workers, slots FREE right now (outputs nullable) */
int wdx_feeder_stats(void *ring, int64_t *served, int64_t *reclaimed, int32_t *free_slots);
/* Test hooks (no GPU): 1 = claim a slot for the calling process and leave it FILLING (returns its index), 2 = pose as the
 * serving feeder without serving.  Never on the product path. */
int wdx_feeder_selftest(void *ring, int32_t what);
int wdx_feeder_alive(void *ring);   /* 1 while a feeder process serves the ring, 0 once it has stopped or died (< 0: error) */

/* Live path (BASELINE config 5; N4): every read of one 100 ms chunk round in one call -- the batched form of
 * live_balancing/worker.py:26-96 (segmentation_worker) + :99-131 (classification_worker).  rows[r] points at
 * read r's float32 samples (row_len[r] of them; ragged, caller-owned, only the adapter window
 * [max(0, a_start-padding), min(row_len, a_end+padding)) is read -- the live caller passes a_start = 0 and
 * a_end = polya_start, worker.py:39-44).  The windows are packed into a page-locked staging block, copied
 * once, run through fingerprint -> DTW against the resident references [-> SVM tail when use_svm != 0 and a
 * model trained on those references is resident] on the context's own stream, and the requested outputs
 * come back in one copy; one synchronisation per call.  Outputs are HOST pointers: status int32[n] is
 * required; call int32[n], dist (n, n_refs) float32, fpt (n, K) float64, prob (n, k) float64,
 * pred int32[n] (barcode label or -1 = outlier, worker.py:125), conf float64[n] are nullable.  A read whose
 * fingerprint failed has pred -1 and NaN prob / conf, like wdx_demux_svm_dev. */
int wdx_live_tick(wdx_ctx *ctx, const float *const *rows, const int32_t *row_len, int64_t n_reads,
                  const int32_t *a_start, const int32_t *a_end, const uint8_t *ok, const wdx_seg_params *p,
                  int64_t n_refs, int32_t use_svm, double *fpt, float *dist, int32_t *call, int32_t *status,
                  double *prob, int32_t *pred, double *conf);

/* The live tick for every shipped model kind (file_proc.load_model: DTW_SVM, DTW_MLP, Fpt_Boost) and for int16 chunks:
 * wdx_live_tick is the float32 + plain fingerprint + [SVM] corner of this call, and both run the same tick body.
 *   in->rows / in->adc_rows  exactly one is non-NULL: one pointer per read to its float32 samples, or to its int16 ADC
 *                            samples with in->offset / in->scale float32[n].  int16 rows follow the *_adc contract above
 *                            word for word -- pa = scale * ((float)adc + offset), add then multiply, two roundings, and NaN
 *                            behind the read's last sample: only the adapter windows are packed into the staging block, as
 *                            int16 (2 bytes per sample over the bus), and decode_adc_kernel calibrates them on the device.
 *                            A window that runs past its read's end therefore reads the NaN tail, exactly as on an int16
 *                            minibatch whose stride holds the whole window (wdx_minibatch_adc_in.row_win); the float32 rows
 *                            are ragged and end with the read, so there the window is cut at row_len, as in wdx_live_tick
 *   in->tail                 WDX_LIVE_TAIL_*: which classifier runs behind the fingerprints.  prob (n, k) / pred / conf come
 *                            back when tail != NONE (each nullable); a read whose status is not 0 gets pred -1 and NaN
 *                              _SVM    needs resident references and wdx_svm_set_model (WDX_ERR_NO_REFS otherwise)
 *                              _MLP    needs resident references and wdx_mlp_set_model (WDX_ERR_NO_REFS otherwise); rows
 *                                      with a non-finite scaled input get pred -1 and NaN, as in wdx_demux_mlp_dev, and are
 *                                      counted in *n_nonfinite (nullable; failed reads are not counted)
 *                              _BOOST  needs wdx_boost_set_model (WDX_ERR_NO_REFS otherwise); K must equal the model's
 *                                      n_features (WDX_ERR_INVALID)
 *   rp                       NULL = the plain branch; else the consensus-refinement branch as in wdx_demux_submit_refine
 *                            (K = rp->barcode_keep_events, p->barcode_num_events is ignored).  Refinement is served with
 *                            tail NONE or BOOST; with the SVM or the MLP tail it is WDX_ERR_INVALID
 *   n_refs                   with a resident reference set: its nY (WDX_ERR_INVALID otherwise), and K must equal its length;
 *                            DTW, call and dist run beside whatever tail is asked for.  Without one, n_refs must be 0 and
 *                            the tail NONE or BOOST: call is -1 for every read, WDX_WANT_DIST is WDX_ERR_INVALID
 *   want                     WDX_WANT_FPT | _DIST | _DWELL | _STATS | _REFINE_IDX (the last with rp only); any other bit --
 *                            WDX_WANT_SVM and WDX_WANT_BOOST included: `tail` selects the tail -- is WDX_ERR_INVALID.  A
 *                            wanted output needs its array in `out` / `refine_idx`.  status (required) and call (nullable)
 *                            always come back
 * One host->device copy of the staging block, the kernel chain on the context's own stream, one device->host copy of the
 * wanted outputs (every kernel writes its piece of one output block in place), one synchronisation.  n_reads == 0 returns
 * WDX_SUCCESS and touches nothing.  A refused call leaves the context as it was.  Bit-identical to wdx_fingerprint_batch[_adc] /
 * wdx_fingerprint_refine_batch / wdx_demux_batch / wdx_dtw_svm_predict / wdx_dtw_mlp_predict / wdx_boost_predict on the same
 * windows. */
#define WDX_LIVE_TAIL_NONE 0
#define WDX_LIVE_TAIL_SVM 1
#define WDX_LIVE_TAIL_MLP 2
#define WDX_LIVE_TAIL_BOOST 3
typedef struct wdx_live_in {
    const float *const *rows;        /* float32 rows: rows[r] -> row_len[r] samples; NULL when adc_rows is given      */
    const int16_t *const *adc_rows;  /* int16 rows: adc_rows[r] -> row_len[r] ADC samples; NULL when rows is given    */
    const float *offset, *scale;     /* int16 rows: float32[n_reads] calibration of every read                        */
    const int32_t *row_len;
    int64_t n_reads;
    const int32_t *a_start, *a_end;
    const uint8_t *ok;               /* nullable                                                                      */
    int32_t tail;                    /* WDX_LIVE_TAIL_*                                                               */
    int32_t pad_;
} wdx_live_in;
int wdx_live_tick_ex(wdx_ctx *ctx, const wdx_live_in *in, const wdx_seg_params *p, const wdx_refine_params *rp, int64_t n_refs,
                     uint32_t want, const wdx_minibatch_out *out, int32_t *refine_idx, int64_t *n_nonfinite);

/* ---- N1: classifier tail of DTW_SVM.predict (models/dtw_svm.py:90-93 + models/utils.py:45-61):
 *      K = exp(-gamma * d^pwr_dist) -> SVC.predict_proba(K) (libsvm, precomputed kernel) -> argmax,
 *      label map, top1-top2 margin, per-class thresholds.  Arrays are HOST pointers, copied at set time. */
typedef struct wdx_svm_model {
    int32_t n_classes;         /* k = len(svc.classes_) (barcodes + noise class), 2..16              */
    int32_t n_sv;              /* total support vectors                                              */
    int32_t n_train;           /* columns of the distance matrix = len(model._X)                     */
    int32_t pwr_dist;          /* DTW_SVM.pwr_dist                                                   */
    double gamma;              /* DTW_SVM.gamma                                                      */
    const int32_t *n_support;  /* [k]    svc._n_support                                              */
    const int32_t *support;    /* [n_sv] svc.support_ (column index of every support vector)         */
    const double *dual_coef;   /* [(k-1) x n_sv] svc._dual_coef_ (libsvm sign convention)            */
    const double *rho;         /* [k(k-1)/2]  = -svc._intercept_                                     */
    const double *probA;       /* [k(k-1)/2]  svc._probA                                             */
    const double *probB;       /* [k(k-1)/2]  svc._probB                                             */
    const int32_t *label_map;  /* [k] class index -> barcode label (model.label_mapper); nullable     */
    const double *thresholds;  /* [k] model.thresholds; nullable = no thresholding                    */
} wdx_svm_model;
/* The rule of every model setter: "Resident models" at the top of this file. */
int wdx_svm_set_model(wdx_ctx *ctx, const wdx_svm_model *m);
/* d_dist: (n, n_train) float32 DEVICE distances (wdx_dtw_matrix_dev output); outputs DEVICE, nullable:
 * d_prob (n,k) float64 = y_prob, d_pred int32[n] = predicted barcode or -1, d_conf float64[n] = margin. */
int wdx_svm_predict_dev(wdx_ctx *ctx, const float *d_dist, int64_t n, double *d_prob, int32_t *d_pred,
                        double *d_conf, void *stream);

/* The shipped models' whole path in ONE device-resident call (file_proc.py:418-450 + models/dtw_svm.py:54-98 +
 * models/utils.py:19-61): raw adapter rows -> fingerprint (K = the reference length) -> DTW against the resident
 * training set -> exp(-gamma d^p) -> one-vs-one decision values -> Platt sigmoids + coupling -> process_probs.
 * Inputs as wdx_demux_dev; needs wdx_set_refs and wdx_svm_set_model (a model trained on the resident set).
 * The distance matrix is produced and consumed in row blocks of `block_rows` reads (0 = chosen so that a block is
 * <= 96 MiB, i.e. stays in the 256 MB memory-side cache between the DTW kernel that writes it and the SVM tail that
 * reads it) in a context-owned buffer; it is only written out in full when d_dist (n, nY) is given.
 * Outputs DEVICE: d_status int32[n]; d_prob (n,k) float64, d_pred int32[n] (barcode label or -1), d_conf float64[n],
 * each nullable; reads whose fingerprint failed get pred -1 and NaN probabilities / margin.  d_fpt (n,K) nullable.
 * d_work: wdx_demux_workspace_bytes(n_reads, K) bytes.  Enqueued on `stream`; no synchronisation. */
int wdx_demux_svm_dev(wdx_ctx *ctx, const float *d_sig, const int64_t *d_row_off, const int32_t *d_row_len, int64_t stride,
                      int64_t max_len, int64_t n_reads, const int32_t *d_a_start, const int32_t *d_a_end,
                      const uint8_t *d_ok, const wdx_seg_params *p, double *d_fpt, int32_t *d_status, float *d_dist,
                      double *d_prob, int32_t *d_pred, double *d_conf, void *d_work, int64_t block_rows, void *stream);
/* DTW_SVM.predict on host buffers: X (n, L) float64 fingerprints -> DTW against the resident reference
 * set (wdx_set_refs with model._X, window, penalty) -> SVM tail.  Outputs host, nullable. */
int wdx_dtw_svm_predict(wdx_ctx *ctx, const double *X, int64_t n, double *prob, int32_t *pred, double *conf);

/* ---- classifier tail of DTW_MLP.predict (models/dtw_mlp.py:74-93 + models/utils.py:45-61): the float32 distance
 *      rows -> zero or more StandardScaler steps -> MLPClassifier.predict_proba -> argmax, label map, top1-top2 margin,
 *      per-class thresholds.  The model lives in its own slot of the context: a resident SVM is untouched.
 *      Working dtype = result_type(float32, coefs_ dtype): a float32 model runs every layer in float32 (matrix cores:
 *      v_mfma_f32_16x16x4_f32), a float64 model in float64 (v_mfma_f64_16x16x4_f64).  Probabilities and margins cross
 *      the ABI as float64; for a float32 model each is the float32 result widened exactly.
 *      Limits: 1..WDX_MLP_MAX_LAYERS-1 hidden layers of 1..WDX_MLP_MAX_WIDTH units, k = 2..16 classes (softmax over k
 *      output units, or one logistic output unit for k = 2), at most WDX_MLP_MAX_SCALERS scaler steps; beyond them
 *      WDX_ERR_UNSUPPORTED, a malformed model WDX_ERR_INVALID.
 *      A row whose (scaled) input holds a NaN or an infinity -- scikit-learn refuses the whole call -- gets pred -1 and
 *      NaN probabilities / margin and is counted. */
#define WDX_MLP_MAX_LAYERS 5   /* weight matrices: hidden layers + the output layer */
#define WDX_MLP_MAX_WIDTH 512
#define WDX_MLP_MAX_SCALERS 4
#define WDX_MLP_ACT_IDENTITY 0
#define WDX_MLP_ACT_LOGISTIC 1
#define WDX_MLP_ACT_TANH 2
#define WDX_MLP_ACT_RELU 3
typedef struct wdx_mlp_model {
    int32_t n_layers;          /* weight matrices = len(coefs_), 2..WDX_MLP_MAX_LAYERS                               */
    int32_t dtype_bytes;       /* working dtype: 4 = float32, 8 = float64                                            */
    int32_t hidden_activation; /* WDX_MLP_ACT_* of the hidden layers (MLPClassifier.activation)                      */
    int32_t n_classes;         /* k = len(classes_); output units: k (softmax) or 1 (logistic, k == 2)               */
    int32_t n_scalers;         /* StandardScaler steps ahead of the MLP, 0..WDX_MLP_MAX_SCALERS                     */
    int32_t pad_;
    int32_t sizes[WDX_MLP_MAX_LAYERS + 1]; /* sizes[0] = n_in = len(model._X), sizes[i + 1] = fan-out of layer i       */
    const void *coefs[WDX_MLP_MAX_LAYERS];      /* layer i: (sizes[i], sizes[i + 1]) row-major, working dtype          */
    const void *intercepts[WDX_MLP_MAX_LAYERS]; /* layer i: sizes[i + 1], working dtype                                 */
    const double *scaler_mean[WDX_MLP_MAX_SCALERS];  /* step s: mean_ [n_in] float64, NULL = with_mean False            */
    const double *scaler_scale[WDX_MLP_MAX_SCALERS]; /* step s: scale_ [n_in] float64, NULL = with_std False            */
    const int32_t *label_map;  /* [k] class index -> barcode label (model.label_mapper); nullable                     */
    const double *thresholds;  /* [k] model.thresholds; nullable = no thresholding                                    */
} wdx_mlp_model;
/* The rule of every model setter: "Resident models" at the top of this file. */
int wdx_mlp_set_model(wdx_ctx *ctx, const wdx_mlp_model *m);
/* d_dist: (n, n_in) float32 DEVICE rows; outputs DEVICE, nullable: d_prob (n,k) float64, d_pred int32[n], d_conf
 * float64[n]; d_n_nonfinite: nullable DEVICE int64, INCREMENTED by the rows with a non-finite input.  Enqueued on
 * `stream`; no synchronisation.  WDX_ERR_NO_REFS without a model. */
int wdx_mlp_predict_dev(wdx_ctx *ctx, const float *d_dist, int64_t n, double *d_prob, int32_t *d_pred, double *d_conf,
                        int64_t *d_n_nonfinite, void *stream);
/* DTW_MLP.predict on host buffers: X (n, L) float64 fingerprints -> DTW against the resident reference set (wdx_set_refs
 * with model._X, window, penalty; its nY must equal n_in) -> MLP tail, in row chunks whose distances stay on the device.
 * Outputs host, nullable; n_nonfinite (nullable, host) receives the count of rows with a non-finite distance. */
int wdx_dtw_mlp_predict(wdx_ctx *ctx, const double *X, int64_t n, double *prob, int32_t *pred, double *conf,
                        int64_t *n_nonfinite);
/* wdx_demux_svm_dev's row-block path with the MLP tail: raw adapter rows -> fingerprint -> DTW row blocks of `block_rows`
 * reads (0 = blocks of <= 96 MiB of distances) -> MLP tail.  Reads whose fingerprint failed get pred -1 and NaN and are
 * not counted in d_n_nonfinite (nullable DEVICE int64, incremented).  d_work: wdx_demux_workspace_bytes(n_reads, K). */
int wdx_demux_mlp_dev(wdx_ctx *ctx, const float *d_sig, const int64_t *d_row_off, const int32_t *d_row_len, int64_t stride,
                      int64_t max_len, int64_t n_reads, const int32_t *d_a_start, const int32_t *d_a_end,
                      const uint8_t *d_ok, const wdx_seg_params *p, double *d_fpt, int32_t *d_status, float *d_dist,
                      double *d_prob, int32_t *d_pred, double *d_conf, int64_t *d_n_nonfinite, void *d_work,
                      int64_t block_rows, void *stream);

/* ---- training a DTW_MLP on the device: scikit-learn's MLPClassifier(solver="adam") on a float32 distance matrix, in float32, with the
 *      random draws (initial weights, the epochs' row orders) made by the caller (warpdemux_amd/_mlp_fit.py makes scikit-learn's).
 *      Layer l = 0 .. n_layers-1 maps sizes[l] -> sizes[l+1] units; sizes[n_layers] = n_classes, or 1 (one logistic unit) for two classes.
 *
 *      THE RULE, bit for bit.  Every operation is float32 and rounded on its own (nothing is fused) unless float64 is named.
 *        input     xs[i][f] = x[i][f]; with mean: xs = (float)((double)xs - mean[f]); with scale: xs = (float)((double)xs / scale[f]).
 *                  A value of xs that is not finite ends the fit before the first step: state WDX_MLP_FIT_NONFINITE_INPUT.
 *        epoch e   takes the rows in the order order[e][0 .. m-1] (NULL: 0 .. m-1) in batches of B = min(batch_size, m) rows, the last
 *                  one of m - (steps-1) B rows; nb = the rows of the batch, step t = 1, 2, ... counts the batches of the whole fit.
 *        forward   z = sum over k = 0, 1, ... (rising, one chain: a fused multiply-add per term, starting at +0) of a[k] W[k][j]; then
 *                  z + b[j]; hidden units: relu max(z, 0), tanh (float)tanh((double)z), logistic (float)(1 / (1 + exp(-(double)z))).
 *        output    softmax: zmax over the columns; e_c = (float)exp((double)(z_c - zmax)); s = e_0 + e_1 + ... in column order;
 *                  p_c = e_c / s.  One logistic unit: p = (float)(1 / (1 + exp(-(double)z))).
 *        loss      pc = min(max(p, eps), 1 - eps) with eps = 2^-23 and 1 - eps in float32; a row's loss = (float)-log((double)pc[y]) (one
 *                  unit: pc for class 1, 1 - pc for class 0).  A workgroup adds the losses of its 16 rows in row order in float64;
 *                  the host adds the workgroups' sums in batch-row order in float64: ce.
 *        L2        per step and 16 x 16 tile of every W, BEFORE the update: the float64 sum of w * w (float64 products; the lane sums
 *                  over its 4 rows, then lanes are added by halving strides 32, 16, ..., 1); the host adds the tiles in layer, tile-row,
 *                  tile-column order: values.  The step's loss is ce + 0.5 alpha values, the epoch's loss their float64 sum over the
 *                  steps in order, divided by m.
 *        delta     output: p_c - (c == y) (one unit: p - y).  Hidden layer l: d = sum over j rising (one chain) of delta_{l+1}[j] W_l[i][j],
 *                  then relu: 0 where A_l[i] == 0; tanh: d * (1 - A_l[i] * A_l[i]); logistic: (d * A_l[i]) * (1 - A_l[i]).
 *        gradient  g = sum over the batch rows in row order (one chain) of A_l[r][i] delta_{l+1}[r][j]; g = (g + (float)alpha * w) / (float)nb.
 *                  Intercepts: g = (delta[0][j] + delta[1][j] + ... in row order) / (float)nb.
 *        Adam      m = (float)beta1 * m + (float)(1 - beta1) * g;  v = (float)beta2 * v + (float)(1 - beta2) * (g * g);
 *                  lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t) in float64 on the host;
 *                  w = (float)((double)w + (-lr_t * (double)m) / (double)(sqrtf(v) + (float)epsilon)).
 *        stop      after each epoch, on the float64 loss: count = loss > best - tol ? count + 1 : 0; best = min(best, loss); the fit ends
 *                  with state WDX_MLP_FIT_TOL when count > n_iter_no_change, with WDX_MLP_FIT_MAX_EPOCHS after max_epochs epochs, and
 *                  with WDX_MLP_FIT_NONFINITE_LOSS (the weights of that epoch's end are returned) when the epoch's loss is not finite.
 *      Two fits of the same inputs return the same bits: there is no atomic operation and no order that depends on timing.
 *
 *      Limits (WDX_ERR_UNSUPPORTED beyond them; warpdemux_amd/csrc/wdx_mlp_fit_plan.h states every refusal and lays out the workspace):
 *      n_layers <= WDX_MLP_MAX_LAYERS, hidden widths <= WDX_MLP_MAX_WIDTH, 2 .. 16 classes, batch_size 1 .. WDX_MLP_FIT_MAX_BATCH, m and
 *      the loss slots of one epoch within int32.  WDX_ERR_INVALID: a malformed argument, or a class index outside 0 .. n_classes-1
 *      (found on the device before the first step).  After a refusal or a stated state the context stays usable.
 *
 *      wdx_mlp_fit_device BLOCKS: it enqueues 2 n_layers launches per step on `stream` and synchronises it once per epoch (the loss
 *      slots come back, the stop rule runs, the next order goes up).  d_dist (m, ld) float32 and d_y int32[m] are DEVICE memory
 *      (columns sizes[0] .. ld-1 of d_dist are never read: it ends on element (m-1) ld + sizes[0] - 1); all
 *      else is HOST memory: mean / scale float64[sizes[0]] (nullable), coefs[l] (sizes[l], sizes[l+1]) and intercepts[l] float32 --
 *      the initial values in, the trained ones out --, order (max_epochs, m) int32 (nullable; every entry within 0 .. m-1,
 *      checked on the host before it is uploaded: WDX_ERR_INVALID), loss_curve float64[max_epochs], *n_epochs the epochs run, *state WDX_MLP_FIT_*.  Nothing reads the
 *      environment.  Timed as WDX_K_MLP_FIT (one event pair per epoch).  wdx_mlp_fit: the same on a HOST matrix and HOST class indices,
 *      uploaded for the call, on the context's own stream. */
#define WDX_MLP_FIT_MAX_BATCH 1024
#define WDX_MLP_FIT_MAX_EPOCHS 0
#define WDX_MLP_FIT_TOL 1
#define WDX_MLP_FIT_NONFINITE_INPUT 2
#define WDX_MLP_FIT_NONFINITE_LOSS 3
typedef struct wdx_mlp_fit_params {
    int32_t n_layers;          /* weight matrices, 2..WDX_MLP_MAX_LAYERS                     */
    int32_t hidden_activation; /* WDX_MLP_ACT_*                                              */
    int32_t n_classes;         /* 2..16                                                      */
    int32_t batch_size;        /* 1..WDX_MLP_FIT_MAX_BATCH; beyond m: m                      */
    int32_t max_epochs;        /* >= 1                                                       */
    int32_t n_iter_no_change;  /* >= 0                                                       */
    int32_t sizes[WDX_MLP_MAX_LAYERS + 1];
    double lr, alpha, beta1, beta2, epsilon, tol;
} wdx_mlp_fit_params;
int wdx_mlp_fit_device(wdx_ctx *ctx, const float *d_dist, int64_t m, int64_t ld, const int32_t *d_y, const wdx_mlp_fit_params *p,
                       const double *mean, const double *scale, float *const *coefs, float *const *intercepts, const int32_t *order,
                       double *loss_curve, int32_t *n_epochs, int32_t *state, void *stream);
int wdx_mlp_fit(wdx_ctx *ctx, const float *dist, int64_t m, int64_t ld, const int32_t *y, const wdx_mlp_fit_params *p,
                const double *mean, const double *scale, float *const *coefs, float *const *intercepts, const int32_t *order,
                double *loss_curve, int32_t *n_epochs, int32_t *state);

/* ---- classifier tail of Fpt_Boost.predict (models/fpt_boost.py + models/utils.py:45-61): the float64 fingerprint rows
 *      themselves (no DTW, no reference set) -> an ensemble of oblivious (symmetric) trees over float features ->
 *      scale * sum + bias -> softmax (dim == k) or sigmoid (dim == 1, k == 2) -> argmax, label map, top1-top2 margin,
 *      per-class thresholds.  The model lives in its own slot of the context: a resident SVM or MLP is untouched.
 *      The contract is the NumPy restatement in tests/helpers/boost_ref.py; parity with CatBoost itself is
 *      NOT pinned.  Layout, explicit so that a loader fixes conventions and the kernel does not:
 *        tree t has depth[t] splits, stored at split_*[sum(depth[:t]) + i]; split i sets BIT i of the leaf index when
 *        (float)x[split_feature] > split_border (float32 compare; equality false; a NaN feature gives split_nan_true);
 *        its 2^depth[t] * dim leaf values follow those of the trees before it, leaf-major, class fastest:
 *        leaf_values[leaf_base(t) + leaf * dim + c].
 *      raw_c = scale * (sum over trees, tree 0 first, one float64 add per tree) + bias[c]: float64 multiply, then add.
 *      Limits: 1..254 features, depth 0..16, dim 1..16, k 2..16, >= 1 tree; beyond them WDX_ERR_UNSUPPORTED, a malformed
 *      model WDX_ERR_INVALID. */
#define WDX_BOOST_MAX_FEATURES 254
#define WDX_BOOST_MAX_DEPTH 16
/* Two kernels serve the tail (wdx_boost.hip), with the same bits in every output: one lane per read (large batches), and
 * a tree-parallel one for minibatch-sized batches -- a workgroup per WDX_BOOST_SMALL_READS reads, the trees in chunks of
 * WDX_BOOST_TREE_CHUNK.  By default a call of at most WDX_BOOST_SMALL_MAX_READS rows takes the tree-parallel kernel (the
 * largest batch of the sweep in DESIGN.md 4.8, at every point of which it was the faster one; nothing beyond it has been
 * measured, so larger calls stay on the lane-per-read kernel). */
#define WDX_BOOST_SMALL_READS 16
#define WDX_BOOST_TREE_CHUNK 1024
#define WDX_BOOST_SMALL_MAX_READS 65536
typedef struct wdx_boost_model {
    int32_t n_trees;
    int32_t n_features;            /* columns of a fingerprint row                                                     */
    int32_t dim;                   /* values per leaf: n_classes (MultiClass) or 1 (Logloss, n_classes == 2)           */
    int32_t n_classes;             /* k                                                                                */
    const int32_t *depth;          /* [n_trees]                                                                        */
    const int32_t *split_feature;  /* [sum(depth)] column index, 0..n_features-1                                       */
    const float *split_border;     /* [sum(depth)]                                                                     */
    const uint8_t *split_nan_true; /* [sum(depth)] 1: a NaN feature takes the "greater" branch (AsTrue), 0: it does not;
                                      nullable = all 0                                                                 */
    const double *leaf_values;     /* [sum(2^depth[t]) * dim]                                                          */
    double scale;
    const double *bias;            /* [dim]                                                                            */
    const int32_t *label_map;      /* [k] class index -> barcode label; nullable                                       */
    const double *thresholds;      /* [k]; nullable = no thresholding                                                  */
} wdx_boost_model;
/* The rule of every model setter: "Resident models" at the top of this file. */
int wdx_boost_set_model(wdx_ctx *ctx, const wdx_boost_model *m);
/* d_fpt: (n, n_features) float64 DEVICE rows; d_status: nullable DEVICE int32[n], rows with status != WDX_READ_OK get
 * pred -1 and NaN raw / probabilities / margin.  Outputs DEVICE, nullable: d_raw (n, dim) float64, d_prob (n, k) float64,
 * d_pred int32[n], d_conf float64[n].  Enqueued on `stream`; no synchronisation.  WDX_ERR_NO_REFS without a model. */
int wdx_boost_predict_dev(wdx_ctx *ctx, const double *d_fpt, const int32_t *d_status, int64_t n, double *d_raw,
                          double *d_prob, int32_t *d_pred, double *d_conf, void *stream);
/* Fpt_Boost.predict on host buffers: X (n, n_features) float64, in row chunks; outputs host, nullable. */
int wdx_boost_predict(wdx_ctx *ctx, const double *X, int64_t n, double *raw, double *prob, int32_t *pred, double *conf);
/* The tRNA flow in one call: raw adapter rows -> fingerprint stage (with rp: the consensus-refinement branch, K =
 * rp->barcode_keep_events; rp NULL: the plain fingerprint, K = p->barcode_num_events) -> boost tail.  K must equal the
 * model's n_features (WDX_ERR_INVALID).  Needs no reference set.  Everything DEVICE, enqueued on `stream`, no
 * synchronisation: d_status int32[n]; d_refine_idx int32 (n, 3), nullable (written with rp only); d_fpt (n, K), d_raw
 * (n, dim), d_prob (n, k), d_pred, d_conf nullable.  Reads whose fingerprint failed get pred -1 and NaN.
 * d_work: wdx_demux_refine_workspace_bytes(n_reads, K) bytes (without rp wdx_demux_workspace_bytes(n_reads, K) is enough). */
int wdx_demux_boost_dev(wdx_ctx *ctx, const float *d_sig, const int64_t *d_row_off, const int32_t *d_row_len, int64_t stride,
                        int64_t max_len, int64_t n_reads, const int32_t *d_a_start, const int32_t *d_a_end,
                        const uint8_t *d_ok, const wdx_seg_params *p, const wdx_refine_params *rp, double *d_fpt,
                        int32_t *d_refine_idx, int32_t *d_status, double *d_raw, double *d_prob, int32_t *d_pred,
                        double *d_conf, void *d_work, void *stream);

/* ---- training an Fpt_Boost on the device: gradient boosting of oblivious trees on the raw fingerprint, MultiClass with dim == k
 *      (also for k = 2), emitting exactly the arrays the tail above reads.  The rule is this engine's own (parity with CatBoost's
 *      trainer is NOT a goal: no ordered boosting, random strength or bootstrap) and is written so that NumPy restates the whole fit
 *      bit for bit (tests/helpers/boost_fit_rule.py): gradients are quantised to integers, histograms are integer sums (any arrival
 *      order of the atomics gives the same bits), exp is the stated polynomial, every float64 expression has one operation order and
 *      nothing is fused.
 *
 *      THE RULE.  x = (float)X[row][f], rounded once.  Borders come from the caller (warpdemux_amd/_boost_fit.py: borders makes them
 *      from the data): per feature n_borders[f] ascending float32 values, 0 .. border_count of them.
 *        bins      bin[f][row] = the number of the feature's borders with x > border (float32 compare; NaN: 0), uint8.
 *        per tree, from the scores S (n, k) float64:
 *        softmax   z_c = S_c - max_c S_c;  e_c = exp_rule(z_c);  sum = e_0 + e_1 + ... in class order;  p_c = e_c / sum.
 *        exp_rule  (x <= 0)  0 for x < -700; else kk = rint(x * LOG2E), r = (x - kk * LN2_HI) - kk * LN2_LO with fdlibm's
 *                  LOG2E = 0x1.71547652b82fep+0, LN2_HI = 0x1.62e42feep-1, LN2_LO = 0x1.a39ef35793c76p-33;
 *                  P = c_13; P = P * r + c_i for i = 12 .. 0 (a multiply, then an add), c_0 = 1, c_i = c_{i-1} / i;  ldexp(P, kk).
 *        gradient  g_c = (y == c) - p_c;  q_c = (int32)rint(g_c * 2^20), ties to even.
 *        levels    l = 0 .. depth-1, every row starting in leaf 0.  For every feature f with borders and every border index b, per
 *                  current leaf: GL_c, NL = the sums of q_c and the row count over the rows with bin <= b, GR_c, NR over bin > b
 *                  (int64).  score(f, b): acc = 0; for leaf ascending, for class ascending: acc += GL*GL / (NL + lambda), then
 *                  acc += GR*GR / (NR + lambda), with G and N converted to float64.  The level's split is the first maximum in
 *                  (f, b) order (ties: the lowest f, then the lowest b).  Then leaf |= (bin[f] > b) << l.
 *        leaves    V[leaf][c] = lr * (((double)G_c * 2^-20) / ((double)N + lambda)) over the rows of the leaf; an empty leaf gives 0.
 *        update    S[row][c] = S[row][c] + V[leaf(row)][c].
 *      The model is scale = 1, bias = 0 and per tree (split_feature, the float32 border borders[f][split_border], nan_true = 0,
 *      leaves): d_scores after the call is, bit for bit, what the tail's raw scores are on the training rows.
 *
 *      Limits (WDX_ERR_UNSUPPORTED beyond them; warpdemux_amd/csrc/wdx_boost_fit_plan.h states every refusal, the workspace and the
 *      overflow bounds): 1 .. WDX_BOOST_MAX_FEATURES features, 2 .. 16 classes, depth 1 .. WDX_BOOST_FIT_MAX_DEPTH, border_count
 *      1 .. 255, n 1 .. 2^24, n_trees 1 .. WDX_BOOST_FIT_MAX_TREES, a workspace of at most WDX_BOOST_FIT_MAX_WORKSPACE bytes.
 *      WDX_ERR_INVALID: lambda <= 0 or not finite, lr not finite, ld < n_features, an n_borders[f] outside 0 .. border_count, no
 *      feature with a border, a NULL argument, a class index outside 0 .. k-1 (found on the device before the first tree; nothing
 *      is written then).  After a refusal the context and its resident models stay usable.
 *
 *      wdx_boost_fit_device BLOCKS, but synchronises `stream` only before the first tree (the class-index check) and after the last:
 *      3 * depth + 4 launches per tree, splits and leaves staying on the device in between.  Columns n_features .. ld-1 of d_X are
 *      never read (it ends on element (n-1) ld + n_features - 1).  d_X (n, ld) float64, d_y int32[n] and
 *      d_scores (n, k) float64 are DEVICE memory; d_scores is IN/OUT -- zero it for a fresh fit; a further call continues the fit
 *      with n_trees more trees.  HOST memory: borders (the features' borders one after another), n_borders int32[n_features], and
 *      the outputs split_feature / split_border int32[n_trees * depth] (split l of tree t at t * depth + l; split_border is the
 *      INDEX into the feature's borders) and leaf_values float64[n_trees * 2^depth * k] (leaf-major, class fastest).  Timed as
 *      WDX_K_BOOST_FIT.  wdx_boost_fit: the same on HOST X, y and scores, uploaded for the call, on the context's own stream. */
#define WDX_BOOST_FIT_MAX_DEPTH 8
#define WDX_BOOST_FIT_MAX_BORDERS 255
#define WDX_BOOST_FIT_MAX_ROWS (1 << 24)
#define WDX_BOOST_FIT_MAX_TREES (1 << 20)
#define WDX_BOOST_FIT_MAX_WORKSPACE ((int64_t)4 << 30)
#define WDX_BOOST_FIT_GRAD_BITS 20   /* q = rint(g * 2^20) */
#define WDX_BOOST_FIT_ROWS 2047      /* rows per workgroup pass of the histogram kernel: 2047 * 2^20 < 2^31 (int32 LDS partials) */
typedef struct wdx_boost_fit_params {
    int32_t n_features;   /* columns of X read, 1..WDX_BOOST_MAX_FEATURES          */
    int32_t n_classes;    /* k, 2..16                                              */
    int32_t n_trees;      /* trees added by this call                              */
    int32_t depth;        /* 1..WDX_BOOST_FIT_MAX_DEPTH                            */
    int32_t border_count; /* 1..255: no feature has more borders                   */
    int32_t reserved;     /* 0                                                     */
    double learning_rate, l2_leaf_reg;
} wdx_boost_fit_params;
int wdx_boost_fit_device(wdx_ctx *ctx, const double *d_X, int64_t n, int64_t ld, const int32_t *d_y, const float *borders,
                         const int32_t *n_borders, const wdx_boost_fit_params *p, double *d_scores, int32_t *split_feature,
                         int32_t *split_border, double *leaf_values, void *stream);
int wdx_boost_fit(wdx_ctx *ctx, const double *X, int64_t n, int64_t ld, const int32_t *y, const float *borders, const int32_t *n_borders,
                  const wdx_boost_fit_params *p, double *scores, int32_t *split_feature, int32_t *split_border, double *leaf_values);

/* ---- adapter boundary detection: a_start / a_end / ok of every entry above, found on the device --------------------------------
 * In the reference these come from ADAPTed (combined_detect_llr2 / _cnn / _start_peak, file_proc.py:395-413; the live session's
 * mean_var_shift_polyA_detect), whose source is not part of the reference tree.  THE RULE below is
 * the engine's own rule; parity with ADAPTed unpinned; accuracy on real reads unmeasured.
 * Every quantity is an exact integer except the one float64 expression of step 3, whose operations are single IEEE operations in a
 * stated order: any summation order gives the same bits.  NumPy
 * restatement: tests/helpers/detect_rule.py; the kernel (wdx_detect.hip) is held to it with array_equal.
 *
 * Thresholds, converted once on the host (float32 products, float32 clamps; a clamp never changes a comparison below, because
 * q lies in -32768 .. 32767):
 *   thr1    = (int32)fminf(fmaxf(rintf(open_pore_pa * quant_per_pa), -32768.f), 32768.f)
 *   shift_q = (int32)fminf(fmaxf(rintf(min_shift_pa * quant_per_pa), -65536.f), 65536.f)
 *   var_q   = (int64)fmin(fmax(floor(((double)max_polya_var * (double)quant_per_pa) * (double)quant_per_pa), -1.0), 2147483648.0)
 * Trace of read r:
 *   n     the number of leading non-NaN samples of the row, capped by the row's length and by max_obs_trace
 *   v     = x[i] * quant_per_pa                       one float32 multiply
 *   q[i]  = 32767 if v >= 32767, -32768 if v <= -32768, else (int)rintf(v)      (round half to even)
 *   P[t]  = sum of q[i], i < t;  P2[t] = sum of q[i]^2, i < t                   (int64, exact)
 * With sw = start_win, pw = polya_win, tw = step_win:
 *   1  n < sw + min_obs_adapter + pw: WDX_DETECT_SHORT.
 *   2  find_start == 0: s = 0.  Otherwise s = the smallest i in 0 .. min(max_start, n - sw) with q[i] < thr1 and
 *      P[i + sw] - P[i] < thr1 * sw; none: WDX_DETECT_NO_START.
 *   3  lo = s + min_obs_adapter, hi = min(n - pw, s + max_obs_adapter); lo > hi: WDX_DETECT_NO_ROOM.  For i in lo .. hi, in
 *      float64 with nothing fused, L = P[i] - P[s], R = P[n] - P[i]:
 *          g(i) = ((double)L * (double)L) / (double)(i - s) + ((double)R * (double)R) / (double)(n - i)
 *      c = the i with the largest g, ties to the smallest i.
 *   4  For j in max(lo, c - refine) .. min(hi, c + refine): S1 = P[j + pw] - P[j], S2 = P2[j + pw] - P2[j], A1 = P[j] - P[s],
 *      la = j - s.  j qualifies when  pw * S2 - S1 * S1 <= var_q * pw * pw  and  S1 * la - A1 * pw >= shift_q * pw * la.
 *      e = the qualifying j with the largest D(j) = (P[j + tw] - P[j]) - (P[j] - P[j - tw]), ties to the smallest j; none:
 *      WDX_DETECT_NO_POLYA.
 * Outputs per read (all nullable except code):
 *   a_start int32  s once step 2 has it (NO_ROOM, NO_POLYA, OK), else -1   a_end int32  e on WDX_DETECT_OK, else -1
 *   ok uint8       1 on WDX_DETECT_OK, else 0                             code int32   WDX_DETECT_*
 *   info (n_reads, 4) int32 = {n, c, P[e] - P[s], P[e + pw] - P[e]}, -1 where a value is not reached
 *   gain float64   g(c); where c is not reached the NaN with the bits 0x7FF8000000000000
 * Domain (WDX_ERR_INVALID outside it, nothing launched or written): 1 <= max_obs_trace <= WDX_DETECT_MAX_TRACE; quant_per_pa > 0;
 * find_start 0 or 1; 1 <= step_win <= polya_win <= 1024; step_win <= min_obs_adapter <= max_obs_adapter; 1 <= start_win <= 256;
 * 0 <= refine <= 4096; max_start >= 0; every float finite. */
#define WDX_DETECT_MAX_TRACE 16384
#define WDX_DETECT_OK 0
#define WDX_DETECT_SHORT 1
#define WDX_DETECT_NO_START 2
#define WDX_DETECT_NO_ROOM 3
#define WDX_DETECT_NO_POLYA 4
typedef struct wdx_detect_params {
    int32_t max_obs_trace;    /* samples of a row the rule looks at, 1 .. WDX_DETECT_MAX_TRACE                            */
    float quant_per_pa;       /* integer steps per pA (> 0; 8: steps of 0.125 pA, +-4 096 pA before the clamp)           */
    int32_t find_start;       /* 0: s = 0; 1: step 2                                                                     */
    float open_pore_pa;       /* step 2: the adapter starts where the signal has left the open-pore level                */
    int32_t start_win;        /* step 2: samples of the mean that must lie below open_pore_pa too                        */
    int32_t max_start;        /* step 2: the last sample the start is looked for at                                      */
    int32_t min_obs_adapter;  /* step 3: the fewest and the most samples between the start and the adapter's end         */
    int32_t max_obs_adapter;
    int32_t polya_win;        /* steps 3 and 4: samples behind the adapter's end that must look like the polyA tail      */
    int32_t step_win;         /* step 4: samples on either side of the step D(j)                                         */
    int32_t refine;           /* step 4: candidates on either side of c                                                  */
    float min_shift_pa;       /* step 4: mean of the polyA window minus mean of the adapter, at least                    */
    float max_polya_var;      /* step 4: variance of the polyA window (pA^2), at most                                    */
} wdx_detect_params;
/* Device-resident float32 rows, in the layouts of wdx_fingerprint_dev (strided; strided with d_row_len, clamped to 0 .. stride;
 * packed int64 d_row_off[n_reads + 1] with or without d_row_len, clamped to the row's slice).  Nothing beyond
 * min(row length, max_obs_trace) samples of a row is read.  Outputs DEVICE arrays as stated above.  detect_kernel, one wave per
 * read: the row quantised once into 2 * max_obs_trace bytes of LDS, every step on it.  Enqueued on `stream`; no synchronisation,
 * no allocation.  n_reads == 0 is success and writes nothing.  Timed as WDX_K_DETECT. */
int wdx_detect_rows(wdx_ctx *ctx, const float *d_sig, const int64_t *d_row_off, const int32_t *d_row_len, int64_t stride,
                    int64_t n_reads, const wdx_detect_params *params, int32_t *d_a_start, int32_t *d_a_end, uint8_t *d_ok,
                    int32_t *d_code, int32_t *d_info, double *d_gain, void *stream);
/* The same on an int16 shard that stays in device memory (wdx_adc_dev_in and its contract, above; row_win plays no part: the rule
 * ends at the first NaN).  Bit-identical to wdx_detect_rows on the calibrated rows.  There is no float32 staging block: the kernel
 * calibrates and quantises as it loads. */
int wdx_detect_rows_adc(wdx_ctx *ctx, const wdx_adc_dev_in *in, int64_t n_reads, const wdx_detect_params *params,
                        int32_t *d_a_start, int32_t *d_a_end, uint8_t *d_ok, int32_t *d_code, int32_t *d_info, double *d_gain,
                        void *stream);
/* Blocking host-buffer forms on the context's own stream: sig (n_reads, stride) float32 with a NaN tail and row_len (nullable)
 * int32[n_reads]; adc (n_reads, stride) int16 with row_len, offset, scale [n_reads] REQUIRED.  The rows are copied up, the call
 * above is made, the outputs (HOST arrays, nullable as above) are copied down.  One synchronisation. */
int wdx_detect_batch(wdx_ctx *ctx, const float *sig, int64_t n_reads, int64_t stride, const int32_t *row_len,
                     const wdx_detect_params *params, int32_t *a_start, int32_t *a_end, uint8_t *ok, int32_t *code, int32_t *info,
                     double *gain);
int wdx_detect_batch_adc(wdx_ctx *ctx, const int16_t *adc, int64_t n_reads, int64_t stride, const int32_t *row_len,
                         const float *offset, const float *scale, const wdx_detect_params *params, int32_t *a_start,
                         int32_t *a_end, uint8_t *ok, int32_t *code, int32_t *info, double *gain);

/* ---- multi-GPU: the only exchange on the path ---------------------------------------
 * Reads shard over one process per GPU with no data-path collective; after the last batch the per-barcode
 * call histogram -- the engine's form of the reference's shared run counters `ridx_dict`
 * (file_proc.py:1059-1066) -- is summed over ranks by ONE RCCL all-reduce (xGMI within a node).
 * librccl is dlopen'ed on first use (the copy already loaded in the process, e.g. PyTorch's, is
 * preferred), so a single-GPU user never needs it. */
#define WDX_COMM_ID_BYTES 128 /* == NCCL_UNIQUE_ID_BYTES */
/* WDX_SUCCESS when librccl could be bound in this process, WDX_ERR_NO_DEVICE (and the reason in
 * wdx_last_error) when it could not.  Local and cheap: every rank asks BEFORE anyone enters the collective
 * wdx_comm_init, so that all ranks take the same road.  Needs no context. */
int wdx_comm_available(void);
/* Rank 0 creates the rendezvous id and hands the 128 bytes to the other ranks by any means (the
 * launcher's store, a file, MPI ...).  Needs no context. */
int wdx_comm_unique_id(void *id_out /* WDX_COMM_ID_BYTES */);
/* Collective over all `world` ranks: bind the context to rank `rank` of the communicator `id`. */
int wdx_comm_init(wdx_ctx *ctx, const void *id, int32_t rank, int32_t world);
int wdx_comm_destroy(wdx_ctx *ctx);
/* What the context is bound to: rank/world as given to wdx_comm_init (0 / 1 without a communicator) and
 * rccl_count = the rank count RCCL itself reports for the communicator (ncclCommCount; 0 without a
 * communicator, -1 if this librccl lacks the query).  Outputs nullable. */
int wdx_comm_info(wdx_ctx *ctx, int32_t *rank, int32_t *world, int32_t *rccl_count);
/* In-place SUM all-reduce of d_counts int64[n] (DEVICE pointer, e.g. wdx_demux_dev's d_counts) over the
 * communicator, enqueued on `stream`; no synchronisation.  Without a communicator (single process) it is
 * a no-op that returns WDX_SUCCESS. */
int wdx_reduce_counts(wdx_ctx *ctx, int64_t *d_counts, int32_t n, void *stream);
/* Host-buffer form: counts int64[n] on the host, reduced in place; synchronises. */
int wdx_reduce_counts_host(wdx_ctx *ctx, int64_t *counts, int32_t n);

/* ---- measurement helpers ------------------------------------------------------------------ */

/* Kernel ids for wdx_kernel_time */
#define WDX_K_FINGERPRINT 0
#define WDX_K_DTW 1
#define WDX_K_TRANSPOSE 2
#define WDX_K_COUNT 3
#define WDX_K_SVM 4
#define WDX_K_REDUCE 5
#define WDX_K_FINGERPRINT_MAIN 6 /* the main fast fingerprint kernel alone (WDX_K_FINGERPRINT = the whole chain) */
#define WDX_K_FINGERPRINT_CLIP 7 /* clip_bounds_kernel alone (median / MAD / clip bounds ahead of the main kernel) */
#define WDX_K_FINGERPRINT_TAIL 8 /* fingerprint_split_tail_kernel alone (the split main kernel's second half; its time is part of
                                    WDX_K_FINGERPRINT_MAIN, which brackets the tile-kernel / tail-kernel launch pairs) */
#define WDX_K_MLP 9              /* the MLP tail kernel (wdx_mlp_predict_dev, wdx_dtw_mlp_predict, wdx_demux_mlp_dev) */
#define WDX_K_BOOST 10           /* the boost tail, whichever of its two kernels ran (wdx_boost_predict_dev, wdx_boost_predict,
                                    wdx_demux_boost_dev, WDX_WANT_BOOST minibatches) */
#define WDX_K_ADC_DEV_WINDOWS 11 /* adc_dev_windows_kernel: the window decode ahead of every slice of an *_adc_dev call */
#define WDX_K_REFINE_OPTIMAL 12   /* fingerprint_refine_optimal_kernel alone (WDX_OPT_REFINE_OPTIMAL_CPTS; part of WDX_K_FINGERPRINT) */
#define WDX_K_MEDOID 13           /* per-label medoids: the pre-pass, the tile kernels (or the general route's chunk sums) and the reduce kernel */
#define WDX_K_SELF_NEAREST 14     /* leave-one-out nearest neighbours: the pre-pass, the tile kernels and the finish kernel (or the general
                                    route's dispatches and rows kernel) */
#define WDX_K_SVM_FIT 15          /* the batched SMO solve (wdx_svm_solve_device, wdx_svm_solve): its one launch */
#define WDX_K_MLP_FIT 16          /* the trainer of wdx_mlp_fit_device / wdx_mlp_fit: one event pair per epoch around its 2 n_layers launches per step */
#define WDX_K_BOOST_FIT 17        /* the trainer of wdx_boost_fit_device / wdx_boost_fit: one event pair per call around 1 + n_trees (3 depth + 4) launches, counted as issued (refused for a class index: 1) */
#define WDX_K_SVM_KERNEL 18       /* the kernel matrix of wdx_svm_kernel_device: its one launch */
#define WDX_K_SVM_CV_COUPLE 20    /* the out-of-fold probabilities of wdx_svm_cv_couple_device: its one launch */
#define WDX_K_THRESHOLDS 19       /* wdx_accuracy_thresholds_device / wdx_accuracy_thresholds: one event pair around the histogram pass and the selection (n == 0: the selection alone) */
#define WDX_K_DETECT 21           /* detect_kernel (wdx_detect_rows, wdx_detect_rows_adc and the host-buffer forms): its one launch */
/* When enabled, every kernel launch through this context is bracketed by hipEvents on its
 * stream; wdx_kernel_time() synchronises them and returns accumulated ms and launch count. */
int wdx_kernel_timing(wdx_ctx *ctx, int enable);
int wdx_kernel_time(wdx_ctx *ctx, int kernel_id, double *total_ms, int64_t *launches);
int wdx_kernel_time_reset(wdx_ctx *ctx);
/* Which DTW kernel the latest dispatch through this context took (wdx_dtw_matrix[_dev], wdx_demux_*, wdx_nearest_dev, wdx_dtw_nearest, wdx_live_tick,
 * wdx_dtw_svm_predict, wdx_demux_svm_dev; a pipelined minibatch reports at its wdx_demux_submit[_ex]).  Host-side
 * bookkeeping of the launcher: nothing on the device changes.  The thresholds between the paths are tuning constants;
 * tests that mean "band<8>, row-major" ask here instead of restating them.  A call that dispatched nothing (no reads, no
 * references) leaves the record as it was; family is WDX_DTW_NONE until the first dispatch. */
#define WDX_DTW_NONE 0
#define WDX_DTW_WAVEFRONT 1 /* anti-diagonal kernel, one 16-lane row per pair                                  */
#define WDX_DTW_SHORT 2     /* unrolled 25-point / window-15 kernel                                           */
#define WDX_DTW_BAND 3      /* rolling register band: band_w = 8, 15, 16 or 32                                */
#define WDX_DTW_SCRATCH 4   /* two DP rows per lane in global scratch (windows beyond 32)                     */
#define WDX_DTW_SHORT_SVM 5 /* the 25-point kernel with the SVM decision sums in its epilogue                 */
#define WDX_DTW_WIDE 6      /* strips of 32 columns in registers, edge column in LDS (WDX_OPT_WIDE_DTW: windows 33 .. L)  */
#define WDX_DTW_LAYOUT_ROW_MAJOR 0     /* lanes = reads, each lane reads its own (n, L) row in place                      */
#define WDX_DTW_LAYOUT_READ_MINOR 1    /* lanes = reads, transposed copy (L, ld): one coalesced load per sample           */
#define WDX_DTW_LAYOUT_REFS_AS_LANES 2 /* lanes = references (resident transposed set), the reads are the uniform operand */
typedef struct wdx_dtw_launch_info {
    int32_t family;         /* WDX_DTW_*                                                                             */
    int32_t band_w;         /* template window of the instantiation (band: 8 / 15 / 16 / 32, short: 15), else 0      */
    int32_t exact_w;        /* 1: the instantiation serves exactly window band_w (no per-cell window mask)           */
    int32_t layout;         /* WDX_DTW_LAYOUT_* (wavefront and short+svm read row-major rows)                        */
    int32_t fused_argmin;   /* 1: the DTW kernel wrote the argmin itself, 0: separate kernel or none asked for; after a
                               nearest-reference call: 1 the rule ran in the DTW kernel's epilogue, 0 behind it on the matrix */
    int32_t launches;       /* DTW kernel launches of the dispatch (the scratch-row loop: one per 65 536 lanes)      */
    int32_t refs_per_block; /* uniform-operand series one block walks (wavefront: 1)                                 */
    int32_t window;         /* effective window, 1..L                                                                */
    int64_t grid_x, grid_y; /* of the (last) DTW launch                                                              */
} wdx_dtw_launch_info;
int wdx_dtw_last_launch(wdx_ctx *ctx, wdx_dtw_launch_info *info);
/* Diagnostic build of the fingerprint kernel with s_memtime stamps between its phases:
 * d_prof receives 32 int64 per read for the first prof_reads reads (slots 0..9 = shader-clock
 * stamps at the phase boundaries P0..P7, 10 = suppression iterations, 11 = adapter samples,
 * 12 = score positions / peaks).  fast_path selects the 256-thread fast kernel (+ slow-path list;
 * slot 15 of read 0 then holds the number of reads it declined) or the one-kernel exact path.
 * fast_path == 2: the split pair of the RNA004 main kernel (tile kernel: slots 0, 3, 4 = start, samples clipped in LDS, tile pass
 * done, 5 = export done; tail kernel: 6 entries loaded, 7 boundaries written, 8 event means + mean / sd, 9 end; 12 = exported peaks).
 * stop_phase k > 0 makes the fast kernel return after phase k (ablation timing; results are garbage).
 * Outputs other than d_status are discarded.  Never on the product path. */
int wdx_fingerprint_profile_dev(wdx_ctx *ctx, const float *d_sig, const int64_t *d_row_off,
                                int64_t stride, int64_t max_len, int64_t n_reads,
                                const int32_t *d_a_start, const int32_t *d_a_end,
                                const wdx_seg_params *p, int32_t *d_status, long long *d_prof,
                                int64_t prof_reads, int32_t fast_path, int32_t stop_phase, void *stream);

/* Self-test: d_fast[i] = the fast fingerprint kernel's unscaled quotient/sqrt sequence for dm[i] / sqrt(vs[i]),
 * d_ref[i] = the compiler's general float64 expansions of the same expression.  The two must agree bit for bit
 * on the kernel's value range (variance sums in [2^-402, 2^261], mean differences in {0} U [2^-201, 2^129]). */
int wdx_selftest_score_dev(wdx_ctx *ctx, const double *d_dm, const double *d_vs, int64_t n, double *d_fast,
                           double *d_ref, void *stream);

/* Self-test: the dynamic programme of WDX_OPT_REFINE_OPTIMAL_CPTS alone.  Series i = d_x[d_off[i] .. d_off[i + 1]) (float64, DEVICE;
 * d_off int64[n_series + 1]), at most max_len <= WDX_MAX_ADAPTER_SAMPLES samples each; n_bkps (1..253) change-points, pieces of at
 * least min_size samples (< 1: WDX_ERR_UNSUPPORTED).  d_cpts (n_series, n_bkps + 2) int32 = [0, b_1 .. b_B, N]; d_status[i] =
 * WDX_READ_OK, or WDX_READ_FAIL_SEGMENT (infeasible, or a non-finite sample) / WDX_READ_FAIL_UNKNOWN (longer than max_len) with a
 * row of -1.  max_slots > 0 bounds the workgroups (= slices of the context's scratch buffer) the series are walked by. */
int wdx_selftest_optimal_cpts_dev(wdx_ctx *ctx, const double *d_x, const int64_t *d_off, int64_t n_series, int32_t n_bkps,
                                  int32_t min_size, int64_t max_len, int32_t max_slots, int32_t *d_cpts, int32_t *d_status,
                                  void *stream);

/* Self-test of clip_bounds_kernel (A1 ahead of the fast fingerprint kernels: one wave per read): packed
 * reads (d_row_off int64[n_reads+1]) or rows of `stride` samples; cap = 4096, 5120 or 6144 selects the instantiation
 * (windows of 256..cap samples are taken).  d_rec: n_reads records of 16 bytes {float lo, hi, cmax; int32 flag}
 * (flag 0 not taken, 1 bounds valid + sums provably exact, 2 NaN / infinity / no non-negative sample, 3 exactness gate
 * fails or the negative-sample shortcut does not apply).  Must equal sig_proc.py:421-431's med -/+ thresh * mad bit for bit. */
int wdx_selftest_clip_dev(wdx_ctx *ctx, const float *d_sig, const int64_t *d_row_off, int64_t stride, int64_t n_reads,
                          const int32_t *d_a_start, const int32_t *d_a_end, const wdx_seg_params *p, int32_t cap,
                          void *d_rec, void *stream);

/* Diagnostic: stream n floats with coalesced dword loads (known byte count) to calibrate the
 * FETCH_SIZE PMC counter for the fingerprint kernel's access pattern. */
int wdx_calib_read_dev(wdx_ctx *ctx, const float *d_p, int64_t n, float *d_out, void *stream);

/* ---- synthetic input generator (bench / tests; spec "wdx-synth v1", warpdemux_amd/synth.py) */

/* Lengths (incl. both 100-sample pads) of reads first_read .. first_read+n-1 -> d_len int64[n] */
int wdx_synth_lengths_dev(wdx_ctx *ctx, uint64_t seed, int64_t first_read, int64_t n_reads,
                          int32_t n_barcodes, const int32_t *d_dwell_table /*1024*/,
                          int64_t *d_len, void *stream);
/* Fill d_sig (packed, offsets d_off int64[n+1]) and d_barcode int32[n] (nullable). */
int wdx_synth_fill_dev(wdx_ctx *ctx, uint64_t seed, int64_t first_read, int64_t n_reads,
                       int32_t n_barcodes, int32_t n_bc_events, float noise_scale, int32_t spikes,
                       const int32_t *d_dwell_table, const float *d_lead /*160*/,
                       const float *d_bc /*n_barcodes x 64*/, const int64_t *d_off, float *d_sig,
                       int32_t *d_barcode, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* WDX_H */
