// Shared declarations of the libwdx_hip translation units (internal; the public ABI is include/wdx.h).
#pragma once
#include <utility>
#include <vector>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wdx.h"
#include "wdx_window.h"
#include "wdx_adc_dev.h"
#include "wdx_dtw_plan.h"
#include "wdx_refine_optimal_plan.h"
#include "wdx_work_layout.h"
#include "wdx_model_image.h"
#include "wdx_fp_plan.h"

namespace wdx {

// Thread-local error message backing wdx_last_error().
void set_error(const char *fmt, ...);

#define WDX_HIP_TRY(expr)                                                                 \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess) {                                                           \
            ::wdx::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),       \
                             __FILE__, __LINE__);                                         \
            return WDX_ERR_HIP;                                                           \
        }                                                                                 \
    } while (0)

// Diagnostic switches of one context (wdx_ctx_set_option).  All off on the product path; nothing in the
// library reads the environment.
struct Knobs {
    bool exact_path = false;    // WDX_OPT_EXACT_PATH: fingerprint every read on the exact general kernel
    bool no_wavefront = false;  // WDX_OPT_NO_WAVEFRONT_DTW
    bool no_short_dtw = false;  // WDX_OPT_NO_SHORT_DTW
    bool svm_scalar = false;    // WDX_OPT_SVM_SCALAR
    bool debug_occ = false;     // WDX_OPT_DEBUG_OCCUPANCY
    int fast_peak_cap = 0;      // WDX_OPT_FAST_PEAK_CAP (0 = built-in capacity)
    int fast_chain_min = 0;     // WDX_OPT_FAST_CHAIN_MIN_READS: batch size from which the launch chain is used (0 = 2048)
    int fast_main_cap = 0;      // WDX_OPT_FAST_MAIN_CAP: 5120 / 6144 forces the main fast instantiation (0 = by batch)
    bool fast_exact_scores = false;  // WDX_OPT_FAST_EXACT_SCORES: fast fingerprint kernel without the approximate first attempt
    bool exact_no_list = false;      // WDX_OPT_EXACT_NO_PEAK_LIST: exact kernel's suppression / top-E in position space only
    bool no_clip_reuse = false;      // WDX_OPT_NO_CLIP_REUSE: the exact kernel behind the chain recomputes its clip bounds
    bool no_wave_clip_long = false;  // WDX_OPT_NO_WAVE_CLIP_LONG: long windows' clip bounds by clip_bounds_block_kernel alone
    bool no_peak_filter = false;     // WDX_OPT_NO_PEAK_FILTER: fast kernels append every local maximum (no threshold filter)
    int64_t max_launch_slice = 0;    // WDX_OPT_MAX_LAUNCH_SLICE: upper bound of one launch slice of the fingerprint chain (0 = built-in)
    bool no_split = false;           // WDX_OPT_NO_SPLIT_TAIL: the main fast kernel in one piece (A/B, tests)
    int dtw_unfused = 0;             // WDX_OPT_DTW_UNFUSED: 0 fused cells + settle | 1 six operations only | 2 / 3 tests, diagnostics
    int64_t mlp_chunk_rows = 0;      // WDX_OPT_MLP_CHUNK_ROWS: rows per pass of wdx_dtw_mlp_predict (0 = built-in)
    int64_t boost_chunk_rows = 0;    // WDX_OPT_BOOST_CHUNK_ROWS: rows per pass of wdx_boost_predict (0 = built-in)
    int boost_kernel = 0;            // WDX_OPT_BOOST_KERNEL: 0 by batch size | 1 lane-per-read | 2 tree-parallel
    bool long_windows = false;       // WDX_OPT_LONG_WINDOWS: adapter windows up to WDX_MAX_LONG_ADAPTER_SAMPLES (product option)
    bool long_refine_windows = false;   // WDX_OPT_LONG_REFINE_WINDOWS: the same for the consensus-refinement branch (product option)
    bool refine_optimal = false;        // WDX_OPT_REFINE_OPTIMAL_CPTS: barcode tails cut at their optimal change-points (product option)
    int64_t adc_dev_slice_reads = 0;    // WDX_OPT_ADC_DEV_SLICE_READS: reads per slice of an int16 device shard (0 = built-in)
    bool wide_dtw = false;              // WDX_OPT_WIDE_DTW: effective windows 33 .. L at L <= WDX_DTW_WIDE_MAX_L on dtw_wide_kernel (product option)
    bool medoid_general = false;        // WDX_OPT_MEDOID_GENERAL: per-label medoids through the DTW dispatch + chunk sums (diagnostic)
    bool self_matrix_general = false;   // WDX_OPT_SELF_MATRIX_GENERAL: the self-distance matrix through the DTW dispatch + mask kernel (diagnostic)
    bool dba_general = false;           // WDX_OPT_DBA_GENERAL: barycenter steps on the rolling rows in global memory (diagnostic)
    bool self_nearest_general = false;  // WDX_OPT_SELF_NEAREST_GENERAL: leave-one-out neighbours through the DTW dispatch + rows kernel (diagnostic)
    // the long form of the exact kernel serves this call (wdx_window.h: the refinement branch has its own option)
    bool long_form(bool refine) const { return long_form_on(refine, long_windows, long_refine_windows); }
    // the longest adapter window a call of this branch fingerprints (the host loops cut one sample beyond it: that reports it)
    int64_t max_window(bool refine) const { return max_adapter_window(refine, long_windows, long_refine_windows); }
    // what the DTW dispatch rule reads of them (wdx_dtw_plan.h)
    DtwSwitches dtw_switches() const { return {no_wavefront, no_short_dtw, wide_dtw}; }
    // ... and the fingerprint plan (wdx_fp_plan.h)
    FpSwitches fp_switches() const {
        FpSwitches s;
        s.exact_path = exact_path, s.fast_peak_cap = fast_peak_cap, s.fast_main_cap = fast_main_cap, s.fast_chain_min = fast_chain_min;
        s.fast_exact_scores = fast_exact_scores, s.no_clip_reuse = no_clip_reuse, s.no_wave_clip_long = no_wave_clip_long;
        s.no_peak_filter = no_peak_filter, s.no_split = no_split, s.max_launch_slice = max_launch_slice;
        s.long_windows = long_windows, s.long_refine_windows = long_refine_windows, s.refine_optimal = refine_optimal;
        return s;
    }
};

// A launch over more workgroups than grid.x admits is cut into slices (block_base != 0 from the second on).  The built-in
// slice sizes are millions of workgroups; WDX_OPT_MAX_LAUNCH_SLICE lowers them for the calling thread while one
// launch_fingerprint runs, so that the tests walk the multi-slice paths on batches the oracle finishes in seconds.
int64_t launch_slice_limit(int64_t builtin);   // fp_slice_limit (wdx_fp_plan.h) of the calling thread's WDX_OPT_MAX_LAUNCH_SLICE
struct LaunchSliceScope {
    explicit LaunchSliceScope(int64_t cap);
    ~LaunchSliceScope();
    int64_t saved;
};

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device, size): a launch on the live
// path is ~0.1 ms, the attribute call must not be paid on each of them.  One static LdsAttr per kernel.
struct LdsAttr {
    int set[16] = {};
    template <class K>
    int ensure(K kern, size_t lds) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = -1;
        if (dev >= 0 && __atomic_load_n(&set[dev], __ATOMIC_RELAXED) >= (int)lds) return WDX_SUCCESS;
        WDX_HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        if (dev >= 0) __atomic_store_n(&set[dev], (int)lds, __ATOMIC_RELAXED);
        return WDX_SUCCESS;
    }
};
template <auto K>   // the one LdsAttr of kernel K
inline LdsAttr &lds_attr_of() {
    static LdsAttr attr;
    return attr;
}

// ---- DTW (wdx_dtw.hip) -----------------------------------------------------------------------
struct DtwRefs {  // resident reference set, both layouts (see DESIGN.md "DTW data layout")
    double *pad = nullptr;   // (nY, Lpad) row-major, Lpad = L + 2*halo, series starts at +halo
    double *T = nullptr;     // (L, ldT) read-minor (series along columns)
    uint8_t *has_nan = nullptr;  // nY flags
    int64_t nY = 0, L = 0, Lpad = 0, ldT = 0;
    int halo = 0;
    int window = 0;  // effective window (1..L), 0 = not set
    double penalty = 0;
    uint64_t content_hash = 0;
    bool any_inf = false;  // a reference holds an infinite sample: dtw_dev_locked runs launch_dtw_equal_inf behind the DTW kernel
};

// The operands of one DTW dispatch (run_dtw_plan).  Lanes run over the columns of A (L, ldA) [nA series] -- or, in the plan's
// row-major layout, over the rows of an (nA, L) row-major array (ldA ignored; a_nan may be null: the kernel flags NaN series
// itself; the wavefront kernel reads such rows too); the uniform operand is Bpad (nB rows of Lpad samples, each series at +halo).
// out[a*sA + b*sB] = (float)dtw(a, b).  argmin (nullable) is only legal when the lanes are the reads (sA == nB, sB == 1): int32[nA].
// The nearest-reference rule of one dispatch (include/wdx.h: wdx_nearest_dev), every pointer DEVICE memory and already at the
// dispatch's first read.  label[c] in 0 .. n_labels-1 is the label of reference c (null: the identity); a label outside that
// range is read as n_labels, a group of its own whose call is -1 -- it never indexes a threshold or a histogram bin.
struct NearestArgs {
    const int32_t *label;     // [nY], nullable
    int32_t n_labels;
    const float *min_margin;  // [n_labels], nullable
    const float *max_dist;    // [n_labels], nullable
    const int32_t *status;    // [n], nullable: a read whose status is not 0 gets call -1 and best NaN
    int32_t *call;            // [n]
    float *best;              // (n, 2): d1, d2; nullable
    NearestArgs from(int64_t r0) const {
        return {label, n_labels, min_margin, max_dist, status ? status + r0 : nullptr, call + r0, best ? best + 2 * r0 : nullptr};
    }
};

struct DtwOperands {
    const double *A;
    int64_t ldA, nA;
    const uint8_t *a_nan;  // nullable
    const double *Bpad;
    int64_t Lpad;
    int halo;
    int64_t nB;
    const uint8_t *b_nan;
    double penalty;
    float *out;
    int64_t sA, sB;
    int32_t *argmin;
    void *scratch;  // the scratch rows' block (plan.scratch_bytes bytes at least), else unused
    int64_t scratch_bytes;
    int unfused;  // Knobs::dtw_unfused
    hipStream_t stream;
    // The nearest-reference rule in the kernel's epilogue (a plan of nearest_plan with rule kFused only: the lanes are the reads
    // and one lane walks every reference).  `out` may then be null: no distance is written.  `argmin` is not used.
    const NearestArgs *nearest = nullptr;
};
// Launches what the plan names -- one kernel family, the scratch rows' launch loop included -- then launch_argmin where the plan
// asks for one and `argmin` is given, and stores plan.info as the record of the dispatch (wdx_dtw_last_launch).
int run_dtw_plan(const DtwPlan &plan, const DtwOperands &op, wdx_dtw_launch_info *record);
// The shipped models' DTW (25 points, window 15) over references in support-vector order with the SVM decision sums in
// its epilogue: P[slot][q][read] (wdx_dtw.hip: dtw_short_svm_kernel); gather of the resident references into that order.
int launch_dtw_svm_partial(const double *X, int64_t nA, const double *Ypad_sv, int64_t Lpad, int halo, const uint8_t *y_nan_sv,
                           int64_t L, int window, double penalty, const double *coefT, const int32_t *chunk_ref0,
                           const int32_t *chunk_slot, int n_chunks, int km1, int pwr, float ngamma, double *P,
                           hipStream_t stream, int unfused, wdx_dtw_launch_info *info = nullptr);
int launch_gather_rows(const double *src, const uint8_t *sflag, const int32_t *d_idx, int64_t n, int64_t ld, double *dst,
                       uint8_t *dflag, hipStream_t stream);
// Equal infinities in a read and a reference at ONE index k: x[k] - y[k] is NaN without a NaN sample.  The reference's
// `if (t < minv)` keeps a NaN diagonal predecessor, so cell (k, k) poisons the main diagonal and the distance is NaN; v_min_f64
// drops the NaN and the DTW kernels return +inf (row k holds nothing finite).  This pass turns exactly those +inf entries of
// out (nX, nY) row-major into NaN.  Run only when a reference holds an infinity (DtwRefs::any_inf): never on the product path.
int launch_dtw_equal_inf(const double *X, int64_t nX, const double *Ypad, int64_t Lpad, int halo, int64_t nY, int64_t L,
                         float *out, hipStream_t stream);

// (n, L) row-major -> (L, ld) read-minor, plus per-series NaN flag (nullable)
int launch_transpose(const double *src, int64_t n, int64_t L, double *dstT, int64_t ld,
                     uint8_t *has_nan, hipStream_t stream);
int launch_nan_flags_T(const double *T, int64_t ld, int64_t n, int64_t L, uint8_t *flags,
                       hipStream_t stream);
// (n, L) row-major -> (n, Lpad) with `halo` zero entries either side, plus NaN flags
int launch_pad_rows(const double *src, int64_t n, int64_t L, double *dst, int64_t Lpad, int halo,
                    uint8_t *has_nan, hipStream_t stream);
// per-row argmin of a float32 (n, m) matrix with np.argmin semantics
int launch_argmin(const float *D, int64_t n, int64_t m, int32_t *out, hipStream_t stream);
// The nearest-reference rule on the rows of a float32 (n, m) matrix (one wave per row): call, best as NearestArgs says
int launch_nearest_rows(const float *D, int64_t n, int64_t m, const NearestArgs &N, hipStream_t stream);
// call[r] = status[r] ? -1 : call[r]; counts[call or m] += 1
int launch_count_calls(int32_t *call, const int32_t *status /*nullable*/, int64_t n, int64_t m,
                       int64_t *counts /*nullable*/, hipStream_t stream);

struct RefineDev;  // wdx_fingerprint.hip: device-side view of wdx_refine_params
int fill_refine_dev(const wdx_refine_params &rp, const double *d_query, int32_t *d_idx, struct RefineDev **out);
void free_refine_dev(struct RefineDev *rf);
int refine_segm_events(const struct RefineDev *rf);   // barcode_num_events[0]

// ---- fingerprint (wdx_fingerprint.hip) ---------------------------------------------------------
// Optional event pair recorded around the launches of the MAIN fast kernel only (WDX_K_FINGERPRINT_MAIN): the
// fingerprint stage is a chain of launches, and the roofline is quoted on its dominant kernel.
struct MainEvents {
    hipEvent_t first = nullptr, second = nullptr;
    bool recorded = false;
    // a third pair around clip_bounds_kernel (WDX_K_FINGERPRINT_CLIP): the launch ahead of the main kernel
    hipEvent_t c_first = nullptr, c_second = nullptr;
    bool c_recorded = false;
    // ... and one around fingerprint_refine_optimal_kernel (WDX_K_REFINE_OPTIMAL), from the pool through `take`
    std::vector<std::pair<hipEvent_t, hipEvent_t>> optimal;
    // SPLIT main kernel: first / second bracket the whole sequence of (tile kernel, tail kernel) launch pairs; one more
    // pair per slice around the tail kernel alone (WDX_K_FINGERPRINT_TAIL), taken from the context's pool through `take`
    std::vector<std::pair<hipEvent_t, hipEvent_t>> tail;
    std::pair<hipEvent_t, hipEvent_t> (*take)(void *) = nullptr;
    void *take_arg = nullptr;
};
// The reads of one fingerprint call and where its results go (device pointers; named members, because d_a_start, d_a_end
// and d_row_len are three adjacent const int32_t * and a transposed positional argument compiles).
struct FpReads {
    const float *sig;
    const int64_t *row_off;  // packed rows: int64[n_reads + 1] (then stride is ignored); null = (n_reads, stride) rows
    const int32_t *row_len;  // nullable
    int64_t stride, max_len, n_reads;
    const int32_t *a_start, *a_end;
    const uint8_t *ok;  // nullable
};
struct FpOut {
    double *fpt;
    int64_t *dwell;  // nullable
    double *stats;   // nullable
    int32_t *status;
};
int launch_fingerprint(const FpReads &in, const wdx_seg_params &p, const FpOut &out, hipStream_t stream,
                       void *d_ws /* fingerprint_workspace_bytes(n) or null */, const Knobs &knobs,
                       int64_t *n_launches = nullptr, long long *d_prof = nullptr, int64_t prof_reads = 0,
                       int stop_phase = 0, const struct RefineDev *rf = nullptr, MainEvents *main_ev = nullptr,
                       double *d_big = nullptr /* fingerprint_big_bytes(max_len) bytes, or null */,
                       void *d_long = nullptr /* fingerprint_long_bytes(max_len) bytes, or null: WDX_OPT_LONG_WINDOWS */,
                       void *d_opt = nullptr /* fingerprint_optimal_bytes(n_reads, max_len, E2) bytes: WDX_OPT_REFINE_OPTIMAL_CPTS */);
// device bytes of the optimal change-points' scratch for a refining call (at most 256 MiB: the reads are taken in slices)
int64_t fingerprint_optimal_bytes(int64_t n_reads, int64_t max_len, int32_t barcode_segm_events);
int64_t fingerprint_workspace_bytes(int64_t n_reads);
// device bytes of the fast kernels' hand-over records for the refinement branch (RefineDev::ws), zero-initialised
int64_t fingerprint_refine_ws_bytes(int64_t n_reads);
void set_refine_ws(struct RefineDev *rf, void *d_ws);
// device bytes the exact kernel needs for the score curves of windows beyond its LDS capacity (0 when max_len fits)
int64_t fingerprint_big_bytes(int64_t max_len);
// ... and, with WDX_OPT_LONG_WINDOWS, for the score curves and samples of windows beyond WDX_MAX_ADAPTER_SAMPLES: 16 slots
// of 768 KB = 12 MB (0 when max_len <= WDX_MAX_ADAPTER_SAMPLES)
int64_t fingerprint_long_bytes(int64_t max_len);
// WDX_OPT_REFINE_OPTIMAL_CPTS: the optimal change-points of the barcode tail for the matched reads (RefineRec::state == 3) of
// A, whichever kernel segmented the adapter (wdx_refine_optimal.hip).  A grid of `slots` workgroups strides over the reads;
// each owns `slot_bytes` of the context's scratch buffer (the path table of the read in flight and, for tails beyond
// kOptLdsCap samples, its prefix sums and two rows of the value table).  OptimalPlan, plan_refine_optimal and their constants:
// wdx_refine_optimal_plan.h.
int launch_optimal_cpts_selftest(const double *d_x, const int64_t *d_off, int64_t n_series, int B, int m, int32_t *d_cpts,
                                 int32_t *d_status, const OptimalPlan &pl, void *d_scratch, hipStream_t stream);
int launch_clip_bounds_selftest(const float *d_sig, const int64_t *d_row_off, int64_t stride, int64_t n_reads,
                                const int32_t *d_a_start, const int32_t *d_a_end, const wdx_seg_params &p, int cap,
                                void *d_rec, hipStream_t stream);
int launch_score_selftest(const double *dm, const double *vs, int64_t n, double *fast, double *ref, hipStream_t stream);

// ---- synthetic generator (wdx_synth.hip) -------------------------------------------------------
int launch_synth_lengths(uint64_t seed, int64_t first_read, int64_t n, int32_t n_barcodes,
                         const int32_t *dwell_table, int64_t *d_len, hipStream_t stream);
int launch_synth_fill(uint64_t seed, int64_t first_read, int64_t n, int32_t n_barcodes,
                      int32_t n_bc_events, float noise_scale, int32_t spikes,
                      const int32_t *dwell_table, const float *lead, const float *bc,
                      const int64_t *off, float *sig, int32_t *barcode, hipStream_t stream);

// ---- SVM tail (wdx_svm.hip; SvmDev, MlpDev, BoostDev and what they point to: wdx_model_image.h) ---
int launch_svm_predict(const SvmDev &M, const float *d_dist, int64_t n, double *d_prob, int32_t *d_pred,
                       double *d_conf, hipStream_t stream, const Knobs &knobs);

int launch_svm_finish(const SvmDev &M, const double *d_P, int halves, int64_t n, double *d_prob, int32_t *d_pred,
                      double *d_conf, hipStream_t stream);
int launch_svm_mask_failed(const int32_t *d_status, int64_t n, int k, double *d_prob, int32_t *d_pred, double *d_conf,
                           hipStream_t stream);

// ---- MLP tail (wdx_mlp.hip) -----------------------------------------------------------------------
constexpr int kMaxMlpWidth = 512;  // widest hidden layer (WDX_MLP_MAX_WIDTH)
// d_status (nullable): rows with status != WDX_READ_OK get pred -1 and NaN, uncounted; d_n_nonfinite (nullable) is
// INCREMENTED by the rows whose (scaled) input holds a NaN or an infinity
int launch_mlp_predict(const MlpDev &M, const float *d_dist, int64_t n, const int32_t *d_status, double *d_prob,
                       int32_t *d_pred, double *d_conf, int64_t *d_n_nonfinite, hipStream_t stream);

// ---- boost tail (wdx_boost.hip) --------------------------------------------------------------------
constexpr int kMaxBoostFeatures = WDX_BOOST_MAX_FEATURES;  // (the widest fingerprint the kernels write: kSegCap)
// d_status (nullable): rows with status != WDX_READ_OK get pred -1 and NaN raw / prob / conf
int launch_boost_predict(const BoostDev &M, const double *d_fpt, const int32_t *d_status, int64_t n, double *d_raw,
                         double *d_prob, int32_t *d_pred, double *d_conf, hipStream_t stream, const Knobs &knobs);

// row r of a page-locked (n, stride) host minibatch, samples [st[r], st[r] + len[r]) -> dst + off[r] (device), read over
// the bus by a copy kernel
int launch_pack_windows(const float *src_dev, int64_t stride, int64_t n_reads, const int64_t *d_off, const int32_t *d_st,
                        const int32_t *d_len, float *dst, hipStream_t stream);
int launch_calib_read(const float *p, int64_t n, float *out, hipStream_t stream);

// ---- int16 ADC rows -> calibrated float32 rows (wdx_adc.hip) --------------------------------------
// Where read r's samples are and where they go (all arrays DEVICE memory; `src` itself may be a mapped host pointer):
//   source       src + (src_off ? src_off[r] : r * src_stride), n_valid[r] samples (clamped to 0 .. the row's n)
//   destination  dst + (dst_off ? dst_off[r] : r * dst_stride), n = n_out ? n_out[r] : dst_stride samples:
//                scale[r] * ((float)adc + offset[r]) for the first n_valid[r], NaN behind them
struct AdcRows {
    const int16_t *src;
    const int64_t *src_off;
    int64_t src_stride;
    const int32_t *n_valid;
    const float *offset, *scale;
    float *dst;
    const int64_t *dst_off;
    int64_t dst_stride;
    const int32_t *n_out;
};
// over_the_bus: pack_windows_adc_kernel (src = a page-locked host minibatch), else decode_adc_kernel
int launch_adc_rows(const AdcRows &A, int64_t n_reads, bool over_the_bus, hipStream_t stream);

// One slice of an int16 DEVICE shard (wdx_adc_dev_in; wdx_adc_dev.h) -> the staged float32 windows of reads r0 .. r0 + n - 1
// and what the chain needs to read them: staged read i = dst + i * pitch, a_start_out / a_end_out / row_len_out int32[n].
// The shard's arrays are indexed by the read's number in the shard (r0 + i), the outputs by i.
struct AdcDevWindows {
    const int16_t *adc;
    const int64_t *row_off;   // packed: int64[n_reads + 1], multiples of 8; null = (n_reads, stride) rows
    int64_t stride;
    const int32_t *row_len, *row_win;   // row_win nullable (packed only)
    const float *offset, *scale;
    const int32_t *a_start, *a_end;
    const uint8_t *ok;        // nullable
    int64_t padding, max_len; // wdx_seg_params.padding; adc_dev_max_len's answer
    int64_t r0, n;
    float *dst;
    int64_t pitch;
    int32_t *a_start_out, *a_end_out, *row_len_out;
};
int launch_adc_dev_windows(const AdcDevWindows &A, hipStream_t stream);

}  // namespace wdx
