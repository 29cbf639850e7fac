// What the host-fed paths stage ahead of the kernels and what they hand back -- the one statement of that arithmetic (plain
// host C++17: no HIP, nothing of the context, so the system compiler builds it alone: tests/host/stage_plan_check.cpp):
//   out_plan / deliver     the pieces a minibatch returns: size, whether a piece exists on the device, whether it travels back,
//                          its offset in an output block, and the copies into the caller's arrays (wdx_live.hip: the tick's
//                          device and page-locked block; wdx_minibatch.hip: a slot's page-locked block, the device->host copies)
//   image_layout           an index image: columns of n or n + 1 elements [+ ok bytes] [+ samples on a 16-byte boundary];
//                          the five images below are instances of it
//   adc_image_row, fill_*  what goes into the columns, from the rule of wdx_window.h; plain pointers in, plain pointers out
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "wdx_window.h"

namespace wdx {

// ---- the output plan ---------------------------------------------------------------------------------------------------
// 8-byte pieces before 4-byte ones.  P_CNT: the MLP tail's count of non-finite inputs (one int64).
enum OutPiece { P_FPT, P_DWELL, P_STATS, P_PROB, P_CONF, P_CNT, P_DIST, P_RIDX, P_STATUS, P_CALL, P_PRED, P_COUNT };
// the optional destinations without a `want` bit: a piece the caller gave no array for does not travel
enum : uint32_t { kHaveCall = 1, kHaveProb = 2, kHavePred = 4, kHaveConf = 8, kHaveAll = 15 };

struct OutPlan {
    int64_t n = 0, nY = 0;
    size_t bytes[P_COUNT] = {}, off[P_COUNT] = {};
    bool exists[P_COUNT] = {};    // the piece is produced on the device
    bool travels[P_COUNT] = {};   // ... and comes back to the host (travels implies exists)
    size_t copy_bytes = 0;        // the travelling pieces: the front of the block
    size_t total = 0;
};

inline uint32_t have_of(const wdx_minibatch_out &o) {
    return (o.call ? kHaveCall : 0u) | (o.prob ? kHaveProb : 0u) | (o.pred ? kHavePred : 0u) | (o.conf ? kHaveConf : 0u);
}

// want: WDX_WANT_FPT / _DIST / _DWELL / _STATS / _REFINE_IDX (other bits are not looked at: `tail`, WDX_LIVE_TAIL_*, names the
// tail and k its classes); refine: the refinement branch runs (without it there is no refine_idx to ask for).
// The block: the travelling pieces first, every piece rounded up to 8 bytes, then the pieces only the device needs.
// A DTW tail without a single reference has nothing to read: its pieces do not exist.
inline OutPlan out_plan(int64_t n_reads, int64_t K, int64_t nY, int64_t k, uint32_t want, int tail, bool refine, uint32_t have) {
    OutPlan P;
    P.n = n_reads, P.nY = nY;
    const size_t n = (size_t)n_reads;
    const bool run_dtw = nY > 0;
    const bool run_tail = tail == WDX_LIVE_TAIL_BOOST || (tail != WDX_LIVE_TAIL_NONE && run_dtw);
    auto piece = [&](OutPiece q, size_t bytes, bool exists, bool travels) {
        P.bytes[q] = bytes, P.exists[q] = exists, P.travels[q] = exists && travels;
    };
    piece(P_FPT, n * (size_t)K * 8, true, (want & WDX_WANT_FPT) != 0);
    piece(P_DWELL, n * (size_t)K * 8, (want & WDX_WANT_DWELL) != 0, true);
    piece(P_STATS, n * 6 * 8, (want & WDX_WANT_STATS) != 0, true);
    piece(P_PROB, n * (size_t)k * 8, run_tail, (have & kHaveProb) != 0);
    piece(P_CONF, n * 8, run_tail, (have & kHaveConf) != 0);
    piece(P_CNT, 8, run_tail && tail == WDX_LIVE_TAIL_MLP, true);
    piece(P_DIST, n * (size_t)nY * 4, run_dtw, (want & WDX_WANT_DIST) != 0);
    piece(P_RIDX, n * 3 * 4, refine && (want & WDX_WANT_REFINE_IDX) != 0, true);
    piece(P_STATUS, n * 4, true, true);
    piece(P_CALL, n * 4, run_dtw, (have & kHaveCall) != 0);
    piece(P_PRED, n * 4, run_tail, (have & kHavePred) != 0);
    size_t o = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int q = 0; q < P_COUNT; ++q) {
            if (!P.exists[q] || P.travels[q] != (pass == 0)) continue;
            P.off[q] = o;
            o += (P.bytes[q] + 7) / 8 * 8;
        }
        if (pass == 0) P.copy_bytes = o;
    }
    P.total = o;
    return P;
}

// where piece q of the plan goes in the caller's arrays (null: nowhere)
inline void *destination(int q, const wdx_minibatch_out &out, int32_t *refine_idx, int64_t *n_nonfinite) {
    void *const to[P_COUNT] = {out.fpt, out.dwell, out.stats, out.prob, out.conf, n_nonfinite, out.dist, refine_idx,
                               out.status, out.call, out.pred};
    return to[q];
}

// `call` of a batch no DTW ran on: -1 for every read
inline void fill_no_call(const OutPlan &P, int32_t *call) {
    if (call && !P.exists[P_CALL])
        for (int64_t r = 0; r < P.n; ++r) call[r] = -1;
}

// The front of a block laid out by `P` -> the caller's arrays: every travelling piece that has a destination, and the `call`
// of a batch without a DTW.  Nothing else is written.
inline void deliver(const OutPlan &P, const unsigned char *block, const wdx_minibatch_out &out, int32_t *refine_idx,
                    int64_t *n_nonfinite) {
    for (int q = 0; q < P_COUNT; ++q) {
        void *to = destination(q, out, refine_idx, n_nonfinite);
        if (to && P.travels[q]) memcpy(to, block + P.off[q], P.bytes[q]);
    }
    fill_no_call(P, out.call);
}

// ---- index images ------------------------------------------------------------------------------------------------------
// The arrays a kernel chain indexes the staged reads by, in one block: columns of n (or n + 1) elements back to back, the
// 8-byte ones before the 4-byte ones, so that every column starts on a multiple of its element size; behind them, when the
// image has them, one `ok` byte per read and the samples, which start on a 16-byte boundary.
constexpr int kImageMaxCols = 8;
struct ImageCol {
    uint8_t elem, plus;   // n + plus elements of elem bytes
};
struct ImageDesc {
    int n_cols;
    ImageCol col[kImageMaxCols];
    bool ok;           // uint8 ok[n] behind the columns
    int sample_elem;   // > 0: a sample area of elements this wide behind everything
};
struct ImageLayout {
    size_t col[kImageMaxCols] = {}, ok = 0, sig = 0;
    size_t bytes = 0;   // the whole image; without samples, the columns [+ ok]
};
inline ImageLayout image_layout(const ImageDesc &D, size_t n, size_t samples = 0) {
    ImageLayout L;
    size_t o = 0;
    for (int c = 0; c < D.n_cols; ++c) {
        L.col[c] = o;
        o += (n + D.col[c].plus) * D.col[c].elem;
    }
    L.ok = o;
    if (D.ok) o += n;
    if (D.sample_elem > 0) {
        o = (o + 15) / 16 * 16;
        L.sig = o;
        o += samples * (size_t)D.sample_elem;
    }
    L.bytes = o;
    return L;
}
template <class T>
inline T *image_col(void *base, const ImageLayout &L, int c) {
    return (T *)((unsigned char *)base + L.col[c]);
}

// rows the caller packed (wdx_minibatch_in.row_off): the device image of its own arrays
enum { PK_OFF, PK_LEN, PK_A_START, PK_A_END };
constexpr ImageDesc kPackedRowsImage = {4, {{8, 1}, {4, 0}, {4, 0}, {4, 0}}, false, 0};
// a page-locked float32 minibatch read over the bus (pack_windows_kernel): where row r goes, its first column, its samples
enum { BP_OFF, BP_FIRST, BP_LEN, BP_A_START, BP_A_END };
constexpr ImageDesc kBusPackImage = {5, {{8, 1}, {4, 0}, {4, 0}, {4, 0}, {4, 0}}, false, 0};
// int16 rows ahead of decode_adc_kernel / pack_windows_adc_kernel (AdcRows) and of the fingerprint stage (FpReads): a
// minibatch's image ends behind `scale`; a tick's carries ok and the int16 samples, every row on a 16-byte boundary
enum { AD_DST, AD_SRC, AD_OUT, AD_VALID, AD_A_START, AD_A_END, AD_OFFSET, AD_SCALE };
constexpr ImageDesc kAdcImage = {8, {{8, 1}, {8, 0}, {4, 0}, {4, 0}, {4, 0}, {4, 0}, {4, 0}, {4, 0}}, false, 0};
constexpr ImageDesc kAdcTickImage = {8, {{8, 1}, {8, 0}, {4, 0}, {4, 0}, {4, 0}, {4, 0}, {4, 0}, {4, 0}}, true, 2};
// a float32 tick: the packed row IS the window -- a_start' = 0 (the zero column), a_end' = len makes
// [max(0, 0 - pad), min(len, len + pad)) the row -- and the samples lie back to back
enum { FT_OFF, FT_ZERO, FT_LEN };
constexpr ImageDesc kFloatTickImage = {3, {{8, 1}, {4, 0}, {4, 0}}, true, 4};

// The int16 image's columns on a block, and THE fill of one row of it: row r stands for w.row float32 samples, the first
// w.valid of them the read's own (at sample `src` of the int16 source), the rest the NaN tail of the *_adc contract; the
// decoded rows start on 32-byte boundaries (`dst`: PackedOffset(8)).
struct AdcImage {
    int64_t *dst, *src;
    int32_t *out, *valid, *a_start, *a_end;
    float *offset, *scale;
    AdcImage(void *base, const ImageLayout &L)   // (host block, or its device copy)
        : dst(image_col<int64_t>(base, L, AD_DST)), src(image_col<int64_t>(base, L, AD_SRC)),
          out(image_col<int32_t>(base, L, AD_OUT)), valid(image_col<int32_t>(base, L, AD_VALID)),
          a_start(image_col<int32_t>(base, L, AD_A_START)), a_end(image_col<int32_t>(base, L, AD_A_END)),
          offset(image_col<float>(base, L, AD_OFFSET)), scale(image_col<float>(base, L, AD_SCALE)) {}
};
constexpr int64_t kDecodedRowRound = 8;   // float32 samples: 32 bytes
inline void adc_image_row(const AdcImage &I, int64_t r, const Window &w, int64_t src, PackedOffset &dst, float offset, float scale) {
    I.dst[r] = dst.take(w.row);
    I.src[r] = src;
    I.out[r] = (int32_t)w.row;
    I.valid[r] = (int32_t)w.valid;
    I.a_start[r] = w.a_start;
    I.a_end[r] = w.a_end;
    I.offset[r] = offset;
    I.scale[r] = scale;
}

// The bus-pack image of (n, stride) float32 rows: up to three samples ahead of a window come along (16-byte aligned bus
// reads) and the packed rows start on 16-byte boundaries.  Returns the packed total, which is off[n].
inline int64_t fill_bus_pack_image(unsigned char *base, const ImageLayout &L, int64_t n, int64_t stride, const int32_t *a_start,
                                   const int32_t *a_end, const uint8_t *ok, int64_t padding) {
    int64_t *off = image_col<int64_t>(base, L, BP_OFF);
    int32_t *first = image_col<int32_t>(base, L, BP_FIRST), *len = image_col<int32_t>(base, L, BP_LEN);
    int32_t *as = image_col<int32_t>(base, L, BP_A_START), *ae = image_col<int32_t>(base, L, BP_A_END);
    const WindowOpts bus{padding, 4, 0};
    PackedOffset pos(4);
    for (int64_t r = 0; r < n; ++r) {
        const Window w = adapter_window(a_start[r], a_end[r], stride, ok && !ok[r], bus);
        off[r] = pos.take(w.row);
        first[r] = (int32_t)w.first;
        len[r] = (int32_t)w.row;
        as[r] = w.a_start;
        ae[r] = w.a_end;
    }
    return off[n] = pos.next;
}

// ---- the staging block of a live tick ----------------------------------------------------------------------------------
// float32: the window inside the read, taken from its very first sample.  int16: a ragged row has no limit -- a window that
// runs past the read's end keeps its NaN tail (wdx_minibatch_adc_in.row_win) -- and a window beyond the kernels' limit keeps
// one sample more than the limit (max_win), which is what reports it.
struct TickStage {
    bool adc = false;
    WindowOpts wo;
    ImageLayout L;
    int64_t max_len = 0;     // FpReads::max_len
    int64_t dst_total = 0;   // int16: float32 samples of the decoded rows
};
inline Window tick_window(const wdx_live_in &in, const TickStage &T, int64_t r) {
    return adapter_window(in.a_start[r], in.a_end[r], T.adc ? kNoRowLimit : (int64_t)in.row_len[r], in.ok && !in.ok[r], T.wo,
                          T.adc ? (int64_t)in.row_len[r] : -1);
}
// the sizing pass; max_win: the longest window of the branch this tick runs, plus one (int16 rows only)
inline TickStage plan_tick_stage(const wdx_live_in &in, int64_t padding, int64_t max_win) {
    TickStage T;
    T.adc = in.adc_rows != nullptr;
    T.wo = WindowOpts{padding, 1, T.adc ? max_win : 0};
    PackedOffset fit(T.adc ? 8 : 1), dfit(kDecodedRowRound);   // (staged int16 rows start on 16-byte boundaries)
    for (int64_t r = 0; r < in.n_reads; ++r) {
        const Window w = tick_window(in, T, r);
        T.max_len = std::max(T.max_len, w.win);
        fit.take(w.valid);
        dfit.take(w.row);
    }
    T.dst_total = dfit.next;
    T.L = image_layout(T.adc ? kAdcTickImage : kFloatTickImage, (size_t)in.n_reads, (size_t)fit.next);
    return T;
}
// the fill pass, into T.L.bytes bytes at `base`
inline void fill_tick_stage(const wdx_live_in &in, const TickStage &T, unsigned char *base) {
    const int64_t n = in.n_reads;
    uint8_t *ok = base + T.L.ok;
    for (int64_t r = 0; r < n; ++r) ok[r] = (!in.ok || in.ok[r]) ? 1 : 0;
    if (T.adc) {
        const AdcImage I(base, T.L);
        int16_t *sig = (int16_t *)(base + T.L.sig);
        PackedOffset pos(8), dpos(kDecodedRowRound);
        for (int64_t r = 0; r < n; ++r) {
            const Window w = tick_window(in, T, r);
            const int64_t at = pos.take(w.valid);
            adc_image_row(I, r, w, at, dpos, in.offset[r], in.scale[r]);
            if (w.valid > 0) memcpy(sig + at, in.adc_rows[r] + w.first, (size_t)w.valid * 2);
        }
        I.dst[n] = dpos.next;
        return;
    }
    int64_t *off = image_col<int64_t>(base, T.L, FT_OFF);
    int32_t *zero = image_col<int32_t>(base, T.L, FT_ZERO), *len = image_col<int32_t>(base, T.L, FT_LEN);
    float *sig = (float *)(base + T.L.sig);
    PackedOffset pos(1);
    for (int64_t r = 0; r < n; ++r) {
        const Window w = tick_window(in, T, r);
        off[r] = pos.take(w.valid);
        zero[r] = 0;
        len[r] = (int32_t)w.row;
        if (w.valid > 0) memcpy(sig + off[r], in.rows[r] + w.first, (size_t)w.valid * 4);
    }
    off[n] = pos.next;
}

}  // namespace wdx
