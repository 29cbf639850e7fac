// Stand-alone sweep of warpdemux_amd/csrc/wdx_work_layout.h -- where the pieces of a caller's d_work lie and what the four
// *_workspace_bytes functions promise -- built by tests/test_work_layout_host.py with the system compiler and the address /
// undefined-behaviour sanitizers.  n from 0 to 20 000 (every value to 300, then every 7th, and both neighbours of every
// multiple of 64, 256 and 8 192 on the way), K from 1 to 128, both with_T, refinement on and off; shards of 1 to 4 slices
// with every last-slice length.  For every point: each piece starts at or after the end of the piece before it and ends inside
// the stated size; every float64 piece is 8-byte and the split records 16-byte aligned relative to a 16-byte-aligned base; the
// layout a slice takes never needs more than the size function promised for the whole call.  Exit status 0 and the number of
// points on stderr; a failing point is named on stderr and ends the sweep.
// With arguments "n K" it prints one line for the Python restatement (tests/helpers/framed.py: work_pieces):
//   "fp_ws count clip list0 .. list5 split dbg fp_bytes plain_bytes refine_off refine_bytes" of the layout wdx_demux_dev takes.
#include "wdx_work_layout.h"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

using namespace wdx;

struct Piece {
    const char *name;
    int64_t at, size, align;
};

static long long points = 0;

static bool fail(const char *what, const char *piece, int64_t n, int64_t K, int with_T, int refine) {
    fprintf(stderr, "FAILED: %s (%s) at n=%lld K=%lld with_T=%d refine=%d\n", what, piece, (long long)n, (long long)K, with_T, refine);
    return false;
}

// one slice of n reads laid out inside a d_work of `promised` bytes
static bool check_slice(int64_t n, int64_t K, bool with_T, bool refine, int64_t promised) {
    const DemuxWork W = demux_work_layout(n, K, with_T);
    const FpWorkLayout F = fp_work_layout(n);
    const int64_t m = n < kWorkSplitSlice ? n : kWorkSplitSlice;
    Piece p[16];
    int np = 0;
    p[np++] = Piece{"fpt", 0, n * K * 8, 8};
    if (with_T) {
        p[np++] = Piece{"fptT", W.fptT, K * W.ld * 8, 8};
        p[np++] = Piece{"flags", W.flags, W.ld, 1};
    }
    p[np++] = Piece{"count", W.fp_ws + F.count, kWorkCounters * 4, 4};
    p[np++] = Piece{"clip", W.fp_ws + F.clip, kWorkClipRecBytes * n, 16};
    for (int i = 0; i < kWorkLists; ++i) p[np++] = Piece{"list", W.fp_ws + F.list[i], 4 * n, 4};
    p[np++] = Piece{"split", W.fp_ws + F.split, kWorkSplitRecBytes * m, 16};
    p[np++] = Piece{"dbg", W.fp_ws + F.dbg, kWorkDbgBytes, 4};
    if (refine) p[np++] = Piece{"records", demux_refine_records_offset(W), kWorkRefineRecBytes * n, 16};
    int64_t end = 0;
    for (int i = 0; i < np; ++i) {
        const Piece &q = p[i];
        if (q.at < end) return fail("a piece starts inside the one before it", q.name, n, K, with_T, refine);
        if (q.at % q.align) return fail("a piece is misaligned", q.name, n, K, with_T, refine);
        end = q.at + q.size;
        if (end > promised) return fail("a piece ends beyond the promised size", q.name, n, K, with_T, refine);
    }
    if (W.fp_ws + F.bytes > W.bytes) return fail("the layout's own size is too small", "bytes", n, K, with_T, refine);
    if (kWorkSplitRecBytes % 16 || kWorkRefineRecBytes % 16 || kWorkClipRecBytes % 16)
        return fail("a record's size breaks the alignment of the next", "records", n, K, with_T, refine);
    ++points;
    return true;
}

static bool check_call(int64_t n, int64_t K) {
    // the float32 entries: wdx_demux_dev and its kin transpose below kRowMajorMinReads; the classifier entries never do
    const bool call_T = n < kRowMajorMinReads;
    for (int refine = 0; refine < 2; ++refine) {
        const int64_t promised = refine ? demux_refine_workspace_size(n, K) : demux_workspace_size(n, K);
        if (!check_slice(n, K, call_T, refine, promised) || !check_slice(n, K, false, refine, promised)) return false;
        // (with_T = true beyond the threshold is no call's layout; it must still be consistent with its own size)
        const DemuxWork W = demux_work_layout(n, K, true);
        if (!check_slice(n, K, true, refine, refine ? demux_refine_records_offset(W) + kWorkRefineRecBytes * n : W.bytes)) return false;
    }
    // wdx_demux_boost_dev without rp: wdx_demux_workspace_bytes is enough
    return check_slice(n, K, false, false, demux_workspace_size(n, K));
}

static bool check_shards(int64_t slice_reads, int64_t K) {
    for (int64_t slices = 1; slices <= 4; ++slices)
        for (int64_t last = 1; last <= slice_reads; last += (slice_reads > 600 && last > 300 && last + 7 < slice_reads ? 7 : 1)) {
            const int64_t n = (slices - 1) * slice_reads + last;
            for (int refine = 0; refine < 2; ++refine) {
                const int64_t promised = demux_shard_workspace_size(n, slice_reads, last, K, refine);
                if (slices > 1 && !check_slice(slice_reads, K, slice_reads < kRowMajorMinReads, refine, promised)) return false;
                if (!check_slice(last, K, last < kRowMajorMinReads, refine, promised)) return false;
                if (!check_slice(last, K, false, refine, promised)) return false;   // the classifier entries' slices
            }
        }
    return true;
}

int main(int argc, char **argv) {
    if (argc == 3) {
        const int64_t n = atoll(argv[1]), K = atoll(argv[2]);
        const DemuxWork W = demux_work_layout(n, K, n < kRowMajorMinReads);
        const FpWorkLayout F = fp_work_layout(n);
        printf("%lld %lld %lld", (long long)W.fp_ws, (long long)F.count, (long long)F.clip);
        for (int i = 0; i < kWorkLists; ++i) printf(" %lld", (long long)F.list[i]);
        printf(" %lld %lld %lld %lld %lld %lld\n", (long long)F.split, (long long)F.dbg, (long long)F.bytes,
               (long long)demux_workspace_size(n, K), (long long)demux_refine_records_offset(W),
               (long long)demux_refine_workspace_size(n, K));
        return 0;
    }
    std::vector<int64_t> ns;
    for (int64_t n = 0; n <= 20000; ++n) {
        bool edge = false;
        for (int64_t m : {64, 256, 8192})
            if (n % m <= 1 || n % m == m - 1) edge = true;
        if (n <= 300 || n % 7 == 0 || edge) ns.push_back(n);
    }
    for (int64_t n : ns)
        for (int64_t K = 1; K <= 128; ++K)
            if (!check_call(n, K)) return 1;
    if (demux_workspace_size(-1, 25) || demux_workspace_size(5, 0) || demux_refine_workspace_size(-1, 25)) return 2;
    // shards: slices on both sides of kRowMajorMinReads, and small ones
    for (int64_t slice_reads : {1, 2, 63, 64, 65, 300, 8191, 8192, 8193, 9000})
        for (int64_t K : {1, 13, 25, 128})
            if (!check_shards(slice_reads, K)) return 3;
    fprintf(stderr, "%lld points\n", points);
    return 0;
}
