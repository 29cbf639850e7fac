// Where everything lives in a caller's d_work, and how large it is told to be -- the one statement of the arithmetic (plain
// host C++17: no HIP, nothing of the context, so the system compiler builds it alone: tests/host/work_layout_check.cpp):
//   fp_work_layout       the fingerprint stage's workspace (wdx_fingerprint_launch.inc: FpWorkspace puts pointers on it)
//   demux_work_layout    [fpt (n,K) f64][with_T only: fptT (K,ld) f64 | nan flags ld][fingerprint workspace], pieces on
//                        256-byte boundaries, and behind it, with refinement, one hand-over record per read
//   demux_*_bytes        what wdx_demux_workspace_bytes / wdx_demux_refine_workspace_bytes / the two *_adc_workspace_bytes return
// The record sizes are the constants below; the translation units that own the records static_assert them against these.
// ALIGNMENT: every offset here is a multiple of 8 and the split records' a multiple of 16, so on a d_work whose base is a
// multiple of 16 every float64 piece is 8-byte aligned and every split record (float64 at +8, 4 624 bytes each) 16-byte
// aligned; the kernels' widest access to d_work is 16 bytes (ClipRec, the split records' header).
#pragma once
#include <stdint.h>

#include "wdx_dtw_plan.h"

namespace wdx {

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

constexpr int kWorkCounters = 8;                 // FpCounter: unsigned each, at the very front
constexpr int kWorkLists = 6;                    // slow, big0, big1, retry, big2, back: int32 per read each
constexpr int64_t kWorkClipRecBytes = 16;        // sizeof(ClipRec)
constexpr int64_t kWorkSplitRecBytes = 4624;     // kSplitRecBytes: SplitHdr + 256 x (key f64, P f64, pos u16)
constexpr int64_t kWorkSplitSlice = 524288;      // kSplitSlice: reads whose split records exist at one time
constexpr int64_t kWorkDbgBytes = 64;            // 16 diagnostic counters at the very end
constexpr int64_t kWorkRefineRecBytes = 1632;    // sizeof(RefineRec)
constexpr int64_t kWorkWidestAccess = 16;        // bytes: what the base of d_work must be a multiple of

// byte offsets of the fingerprint workspace's pieces (relative to its own base) and its size:
// eight counters | one ClipRec per read | six read lists | (16-byte aligned) split records of one launch slice | dbg
struct FpWorkLayout {
    int64_t count, clip, list[kWorkLists], split, dbg, bytes;
};
inline FpWorkLayout fp_work_layout(int64_t n_reads) {
    const int64_t n = n_reads > 0 ? n_reads : 0;
    FpWorkLayout W{};
    int64_t off = 0;
    auto carve = [&](int64_t size) {
        const int64_t at = off;
        off += size;
        return at;
    };
    W.count = carve(kWorkCounters * 4);
    W.clip = carve(kWorkClipRecBytes * n);
    for (int64_t &l : W.list) l = carve(4 * n);
    off = (off + 15) / 16 * 16;
    // (the lists of one slice for every batch size: 4.6 KB per read -- the launch chain is for batches of 2048 reads and
    // more by default, but WDX_OPT_FAST_CHAIN_MIN_READS sends smaller ones through it: the randomised parameter tests)
    W.split = carve(kWorkSplitRecBytes * (n < kWorkSplitSlice ? n : kWorkSplitSlice));
    W.dbg = carve(kWorkDbgBytes);
    W.bytes = off;
    return W;
}
inline int64_t fingerprint_workspace_size(int64_t n_reads) { return fp_work_layout(n_reads).bytes; }

// Byte offsets of the pieces of a caller's d_work, and its size (wdx_demux_workspace_bytes).
// with_T: the read-minor copy wdx_demux_dev makes of a small batch; the classifier entries pass false.
struct DemuxWork {
    int64_t ld, fptT, flags, fp_ws, bytes;
};
inline DemuxWork demux_work_layout(int64_t n_reads, int64_t K, bool with_T) {
    DemuxWork W;
    W.ld = round_up(n_reads > 0 ? n_reads : 1, 64);
    W.fptT = round_up(n_reads * K * 8, 256);
    W.flags = W.fptT + (with_T ? K * W.ld * 8 : 0);
    W.fp_ws = W.flags + (with_T ? round_up(W.ld, 256) : 0);
    // (the unrounded pieces plus 512 for the two roundings: what callers have always been told to allocate)
    W.bytes = n_reads * K * 8 + (with_T ? K * W.ld * 8 + W.ld : 0) + 512 + fingerprint_workspace_size(n_reads);
    return W;
}
// the refinement kernels' hand-over records (kWorkRefineRecBytes per read) behind the pieces of this slice's layout
inline int64_t demux_refine_records_offset(const DemuxWork &W) { return round_up(W.bytes, 256); }

inline int64_t demux_workspace_size(int64_t n_reads, int64_t K) {
    if (n_reads < 0 || K < 1) return 0;
    return demux_work_layout(n_reads, K, n_reads < kRowMajorMinReads).bytes;   // (small batches: wdx_demux_dev transposes)
}
inline int64_t demux_refine_workspace_size(int64_t n_reads, int64_t K) {
    const int64_t base = demux_workspace_size(n_reads, K);
    return base ? round_up(base, 256) + kWorkRefineRecBytes * (n_reads > 0 ? n_reads : 0) : 0;
}
// the largest d_work any slice of an int16 shard asks its float32 twin's layout for: a full slice, or the last, shorter one
// (which may be the one below kRowMajorMinReads that holds the read-minor copy)
inline int64_t demux_shard_workspace_size(int64_t n_reads, int64_t slice_reads, int64_t last_reads, int64_t K, bool refine) {
    if (n_reads < 0 || K < 1) return 0;
    int64_t (*bytes)(int64_t, int64_t) = refine ? demux_refine_workspace_size : demux_workspace_size;
    const int64_t full = bytes((n_reads > 1 ? n_reads : 1) < slice_reads ? (n_reads > 1 ? n_reads : 1) : slice_reads, K);
    const int64_t last = bytes(last_reads > 1 ? last_reads : 1, K);
    return full > last ? full : last;
}

}  // namespace wdx
