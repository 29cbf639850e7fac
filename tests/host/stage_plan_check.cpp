// Stand-alone check of warpdemux_amd/csrc/wdx_stage_plan.h (tests/test_stage_plan_host.py builds it with the system compiler
// and the address / undefined-behaviour sanitizers; every block below is malloc'ed to exactly the size the header states, so
// an overrun of a fill or of a delivery is the sanitizer's to report).  Three parts:
//   the output plan   swept over its domain: no overlap, alignment, the travelling pieces are the front, and -- for the live
//                     tick's use of it -- total, copy_bytes and every offset equal to the arithmetic live_tick did by hand
//                     before the plan existed, transcribed below as plain formulas (parent_block)
//   the delivery      a block with a pattern per piece into arrays with another: wanted arrays hold their piece, nothing
//                     else is written, call is -1 without references
//   the images        seeded batches through the fills: offsets, row alignment, totals, the staged samples, the columns
//                     against adapter_window, the tick's int16 image against a minibatch's of the same rows
// stderr, last line: "<count> points".
#include "wdx_stage_plan.h"

#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

using namespace wdx;

static long long g_points = 0;
#define CHECK(cond, ...)                                          \
    do {                                                          \
        ++g_points;                                               \
        if (!(cond)) {                                            \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                         \
            fprintf(stderr, "\n");                                \
            exit(1);                                              \
        }                                                         \
    } while (0)

static size_t r8(size_t v) { return (v + 7) / 8 * 8; }

// ---- the output plan -----------------------------------------------------------------------------------------------------
// What live_tick computed before wdx_stage_plan.h: the sizes, `need` and `want` of its eleven pieces in its enum's order
// (fpt dwell stats prob conf cnt dist ridx status call pred), then OutBlock::lay_out.  `want` is a mask the tick accepts:
// without refinement parameters it refuses WDX_WANT_REFINE_IDX, so the caller clears that bit.
struct ParentBlock {
    size_t off[11], bytes[11], copy_bytes, total;
    bool need[11], want[11];
};
static ParentBlock parent_block(size_t n, size_t K, size_t nY, size_t k, uint32_t want, int tail, bool out_call, bool out_prob,
                                bool out_pred, bool out_conf) {
    ParentBlock B{};
    const bool run_dtw = nY > 0;
    const bool run_tail = tail == 3 || (tail != 0 && run_dtw);
    B.bytes[0] = n * K * 8, B.need[0] = true, B.want[0] = (want & 0x01u) != 0;
    B.bytes[1] = n * K * 8, B.need[1] = B.want[1] = (want & 0x04u) != 0;
    B.bytes[2] = n * 48, B.need[2] = B.want[2] = (want & 0x08u) != 0;
    B.bytes[3] = n * k * 8, B.need[3] = run_tail, B.want[3] = run_tail && out_prob;
    B.bytes[4] = n * 8, B.need[4] = run_tail, B.want[4] = run_tail && out_conf;
    B.bytes[5] = 8, B.need[5] = B.want[5] = run_tail && tail == 2;
    B.bytes[6] = n * nY * 4, B.need[6] = run_dtw, B.want[6] = run_dtw && (want & 0x02u);
    B.bytes[7] = n * 12, B.need[7] = B.want[7] = (want & 0x20u) != 0;
    B.bytes[8] = n * 4, B.need[8] = B.want[8] = true;
    B.bytes[9] = n * 4, B.need[9] = run_dtw, B.want[9] = run_dtw && out_call;
    B.bytes[10] = n * 4, B.need[10] = run_tail, B.want[10] = run_tail && out_pred;
    size_t o = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int q = 0; q < 11; ++q) {
            if (!B.need[q] || B.want[q] != (pass == 0)) continue;
            B.off[q] = o;
            o += (B.bytes[q] + 7) / 8 * 8;
        }
        if (pass == 0) B.copy_bytes = o;
    }
    B.total = o;
    return B;
}

static void check_invariants(const OutPlan &P, const char *who) {
    size_t front = 0;
    for (int q = 0; q < P_COUNT; ++q) {
        CHECK(!P.travels[q] || P.exists[q], "%s piece %d", who, q);
        if (!P.exists[q]) continue;
        CHECK(P.off[q] % 8 == 0, "%s piece %d", who, q);
        CHECK(P.off[q] + P.bytes[q] <= P.total, "%s piece %d", who, q);
        if (P.travels[q]) {
            CHECK(P.off[q] + r8(P.bytes[q]) <= P.copy_bytes, "%s piece %d travels but is not in the front", who, q);
            front += r8(P.bytes[q]);
        } else {
            CHECK(P.off[q] >= P.copy_bytes, "%s piece %d stays but is in the front", who, q);
        }
        for (int t = q + 1; t < P_COUNT; ++t)
            if (P.exists[t])
                CHECK(P.off[q] + P.bytes[q] <= P.off[t] || P.off[t] + P.bytes[t] <= P.off[q], "%s pieces %d and %d overlap", who, q, t);
    }
    CHECK(front == P.copy_bytes && P.copy_bytes <= P.total, "%s: the front is the travelling pieces", who);
}

static const int64_t kN[] = {0, 1, 2, 63, 64, 65, 513}, kK[] = {1, 13, 25, 110}, kNY[] = {0, 1, 4, 96}, kCls[] = {0, 2, 4, 13};
static const uint32_t kLiveBits[5] = {WDX_WANT_FPT, WDX_WANT_DIST, WDX_WANT_DWELL, WDX_WANT_STATS, WDX_WANT_REFINE_IDX};

static void sweep_plan() {
    static_assert(P_COUNT == 11 && P_FPT == 0 && P_DWELL == 1 && P_STATS == 2 && P_PROB == 3 && P_CONF == 4 && P_CNT == 5 &&
                      P_DIST == 6 && P_RIDX == 7 && P_STATUS == 8 && P_CALL == 9 && P_PRED == 10,
                  "the transcription is in the enum's order");
    for (int64_t n : kN) for (int64_t K : kK) for (int64_t nY : kNY) for (int64_t k : kCls)
        for (int refine = 0; refine < 2; ++refine) {
            // the live tick: the 32 masks of its five bits, the four tails, every set of optional destinations
            for (int m = 0; m < 32; ++m) for (int tail = WDX_LIVE_TAIL_NONE; tail <= WDX_LIVE_TAIL_BOOST; ++tail)
                for (uint32_t have : {0u, (uint32_t)kHaveCall, (uint32_t)kHaveProb, (uint32_t)kHavePred, (uint32_t)kHaveConf, (uint32_t)kHaveAll}) {
                    uint32_t want = 0;
                    for (int b = 0; b < 5; ++b) if (m >> b & 1) want |= kLiveBits[b];
                    const OutPlan P = out_plan(n, K, nY, k, want, tail, refine != 0, have);
                    check_invariants(P, "tick");
                    // (refine_idx without refinement is refused by the tick and ignored by a slot: no such piece)
                    const uint32_t accepted = refine ? want : want & ~WDX_WANT_REFINE_IDX;
                    const ParentBlock B = parent_block((size_t)n, (size_t)K, (size_t)nY, (size_t)k, accepted, tail, have & kHaveCall,
                                                       have & kHaveProb, have & kHavePred, have & kHaveConf);
                    CHECK(P.total == B.total && P.copy_bytes == B.copy_bytes, "n %lld K %lld nY %lld k %lld want %x tail %d have %x",
                          (long long)n, (long long)K, (long long)nY, (long long)k, want, tail, have);
                    for (int q = 0; q < P_COUNT; ++q)
                        CHECK(P.exists[q] == B.need[q] && P.travels[q] == B.want[q] && P.bytes[q] == B.bytes[q] &&
                                  (!B.need[q] || P.off[q] == B.off[q]),
                              "piece %d: n %lld K %lld nY %lld k %lld want %x tail %d have %x", q, (long long)n, (long long)K,
                              (long long)nY, (long long)k, want, tail, have);
                }
            // a pipeline slot: every WDX_WANT_* mask wdx_demux_submit* accepts (never both tails), every destination in the block
            for (uint32_t want = 0; want < 0x80u; ++want) {
                if ((want & WDX_WANT_SVM) && (want & WDX_WANT_BOOST)) continue;
                const int tail = (want & WDX_WANT_SVM) ? WDX_LIVE_TAIL_SVM : (want & WDX_WANT_BOOST) ? WDX_LIVE_TAIL_BOOST : WDX_LIVE_TAIL_NONE;
                const OutPlan P = out_plan(n, K, nY, k, want, tail, refine != 0, kHaveAll);
                check_invariants(P, "slot");
                CHECK(P.travels[P_STATUS] && P.travels[P_CALL] == (nY > 0), "slot: status always, call with references");
                CHECK(P.travels[P_RIDX] == (refine && (want & WDX_WANT_REFINE_IDX)), "slot: refine_idx");
            }
        }
}

// ---- the delivery --------------------------------------------------------------------------------------------------------
static unsigned char pattern(int q, size_t i) { return (unsigned char)(1 + q * 23 + i * 7); }
constexpr unsigned char kUntouched = 0xEE;

static void check_delivery(int64_t n, int64_t K, int64_t nY, int64_t k, uint32_t want, int tail, bool refine, uint32_t have,
                           bool spare_arrays) {
    const OutPlan P = out_plan(n, K, nY, k, want, tail, refine, have);
    unsigned char *block = (unsigned char *)malloc(P.copy_bytes ? P.copy_bytes : 1);   // the front, as both callers hold it
    for (int q = 0; q < P_COUNT; ++q)
        if (P.travels[q])
            for (size_t i = 0; i < P.bytes[q]; ++i) block[P.off[q] + i] = pattern(q, i);
    // the caller's arrays: one for every piece it may name (spare_arrays: also for pieces it did not ask for)
    const uint32_t bit[P_COUNT] = {WDX_WANT_FPT, WDX_WANT_DWELL, WDX_WANT_STATS, 0, 0, 0, WDX_WANT_DIST, WDX_WANT_REFINE_IDX, 0, 0, 0};
    const uint32_t opt[P_COUNT] = {0, 0, 0, kHaveProb, kHaveConf, 0, 0, 0, 0, kHaveCall, kHavePred};
    std::vector<unsigned char> arr[P_COUNT];
    void *to[P_COUNT] = {};
    for (int q = 0; q < P_COUNT; ++q) {
        const bool given = q == P_STATUS || q == P_CNT || (bit[q] && ((want & bit[q]) || spare_arrays)) || (opt[q] && (have & opt[q]));
        if (!given) continue;
        arr[q].assign(P.bytes[q] ? P.bytes[q] : 1, kUntouched);
        to[q] = arr[q].data();
    }
    wdx_minibatch_out out{};
    out.fpt = (double *)to[P_FPT], out.dwell = (int64_t *)to[P_DWELL], out.stats = (double *)to[P_STATS];
    out.prob = (double *)to[P_PROB], out.conf = (double *)to[P_CONF], out.dist = (float *)to[P_DIST];
    out.status = (int32_t *)to[P_STATUS], out.call = (int32_t *)to[P_CALL], out.pred = (int32_t *)to[P_PRED];
    for (int q = 0; q < P_COUNT; ++q) CHECK(destination(q, out, (int32_t *)to[P_RIDX], (int64_t *)to[P_CNT]) == to[q], "piece %d", q);
    deliver(P, block, out, (int32_t *)to[P_RIDX], (int64_t *)to[P_CNT]);
    for (int q = 0; q < P_COUNT; ++q) {
        if (!to[q]) continue;
        bool good = true;
        if (P.travels[q]) {
            for (size_t i = 0; i < P.bytes[q]; ++i) good = good && arr[q][i] == pattern(q, i);
        } else if (q == P_CALL && nY == 0) {
            for (int64_t r = 0; r < n; ++r) good = good && ((int32_t *)to[q])[r] == -1;
        } else {
            for (unsigned char c : arr[q]) good = good && c == kUntouched;
        }
        CHECK(good, "piece %d: n %lld K %lld nY %lld k %lld want %x tail %d refine %d have %x", q, (long long)n, (long long)K,
              (long long)nY, (long long)k, want, tail, (int)refine, have);
    }
    free(block);
}

static void sweep_delivery() {
    for (int64_t n : {1, 2, 65}) for (int64_t K : {1, 13}) for (int64_t nY : {0, 4}) for (int64_t k : {0, 4})
        for (int m = 0; m < 32; ++m) for (int tail = WDX_LIVE_TAIL_NONE; tail <= WDX_LIVE_TAIL_BOOST; ++tail)
            for (int refine = 0; refine < 2; ++refine) for (uint32_t have : {0u, 1u, 2u, 4u, 8u, 7u, 14u, 15u}) {
                uint32_t want = 0;
                for (int b = 0; b < 5; ++b) if (m >> b & 1) want |= kLiveBits[b];
                check_delivery(n, K, nY, k, want, tail, refine != 0, have, (m + have) % 2 != 0);
            }
}

// ---- the images ----------------------------------------------------------------------------------------------------------
static void check_desc(const ImageDesc &D, const char *name) {
    for (int c = 0; c + 1 < D.n_cols; ++c) CHECK(D.col[c].elem >= D.col[c + 1].elem, "%s: 8-byte columns before 4-byte ones", name);
    for (size_t n : {(size_t)0, (size_t)1, (size_t)5, (size_t)64, (size_t)200}) {
        const ImageLayout L = image_layout(D, n, 3 * n);
        size_t end = 0;
        for (int c = 0; c < D.n_cols; ++c) {
            CHECK(L.col[c] % D.col[c].elem == 0 && L.col[c] == end, "%s column %d", name, c);
            end = L.col[c] + (n + D.col[c].plus) * D.col[c].elem;
        }
        CHECK(L.ok == end, "%s: ok", name);
        if (D.ok) end += n;
        if (D.sample_elem) {
            CHECK(L.sig % 16 == 0 && L.sig >= end && L.sig < end + 16, "%s: samples", name);
            end = L.sig + 3 * n * D.sample_elem;
        }
        CHECK(L.bytes == end, "%s: total", name);
    }
}

// One seeded batch of ragged reads: windows that are empty, dead, start beyond the row, end beyond the read, exceed max_win.
struct Batch {
    int64_t n;
    std::vector<std::vector<float>> f32;      // every row exactly row_len long: a read beyond it is the sanitizer's
    std::vector<std::vector<int16_t>> i16;
    std::vector<const float *> f32_rows;
    std::vector<const int16_t *> i16_rows;
    std::vector<int32_t> row_len, a_start, a_end;
    std::vector<uint8_t> ok;
    std::vector<float> offset, scale;
};
constexpr int64_t kMaxWin = 300;
static Batch make_batch(int64_t n, unsigned seed) {
    Batch B;
    B.n = n;
    std::mt19937 g(seed);
    auto u = [&](int lo, int hi) { return (int32_t)(lo + (int)(g() % (unsigned)(hi - lo + 1))); };
    for (int64_t r = 0; r < n; ++r) {
        const int kind = n >= 5 ? (int)(r % 8) : (int)(g() % 8);
        int32_t len = u(40, 400), as = u(0, len / 2), ae = as + u(8, len / 2);
        uint8_t ok = 1;
        if (kind == 1) ae = as;                                   // empty
        if (kind == 2) ok = 0;                                    // dead
        if (kind == 3) as = len + u(1, 50), ae = as + u(1, 60);   // starts beyond the row
        if (kind == 4) ae = len + u(1, 80);                       // ends beyond the read (int16: the NaN tail)
        if (kind == 5) len = u(500, 900), as = u(0, 50), ae = as + kMaxWin + u(1, 150);   // longer than max_win
        if (kind == 6) len = 0;                                   // a read without samples
        B.row_len.push_back(len), B.a_start.push_back(as), B.a_end.push_back(ae), B.ok.push_back(ok);
        B.offset.push_back((float)u(-20, 20)), B.scale.push_back(0.125f * (float)u(1, 16));
        B.f32.emplace_back((size_t)len), B.i16.emplace_back((size_t)len);
        for (int32_t i = 0; i < len; ++i) B.f32.back()[i] = (float)(r * 1000 + i), B.i16.back()[i] = (int16_t)(r * 131 + i);
    }
    for (int64_t r = 0; r < n; ++r) B.f32_rows.push_back(B.f32[r].data()), B.i16_rows.push_back(B.i16[r].data());
    return B;
}

static void check_tick(const Batch &B, bool adc, int64_t padding, bool with_ok, int64_t max_win) {
    wdx_live_in in{};
    in.rows = adc ? nullptr : B.f32_rows.data(), in.adc_rows = adc ? B.i16_rows.data() : nullptr;
    in.offset = adc ? B.offset.data() : nullptr, in.scale = adc ? B.scale.data() : nullptr;
    in.row_len = B.row_len.data(), in.n_reads = B.n, in.a_start = B.a_start.data(), in.a_end = B.a_end.data();
    in.ok = with_ok ? B.ok.data() : nullptr;
    const TickStage T = plan_tick_stage(in, padding, max_win);
    const ImageDesc &D = adc ? kAdcTickImage : kFloatTickImage;
    for (int c = 0; c < D.n_cols; ++c) CHECK(T.L.col[c] % D.col[c].elem == 0, "column %d", c);
    CHECK(T.L.sig % 16 == 0, "samples on a 16-byte boundary");
    unsigned char *base = (unsigned char *)malloc(T.L.bytes);   // exactly in_bytes
    fill_tick_stage(in, T, base);
    const WindowOpts wo{padding, 1, adc ? max_win : 0};
    int64_t at = 0, dst = 0, max_len = 0;
    const AdcImage I(base, T.L);
    for (int64_t r = 0; r < B.n; ++r) {
        const bool dead = with_ok && !B.ok[r];
        const Window w = adapter_window(B.a_start[r], B.a_end[r], adc ? kNoRowLimit : (int64_t)B.row_len[r], dead, wo,
                                        adc ? (int64_t)B.row_len[r] : -1);
        max_len = std::max(max_len, w.win);
        CHECK(base[T.L.ok + r] == (dead ? 0 : 1), "ok of read %lld", (long long)r);
        CHECK(w.first + w.valid <= B.row_len[r] || w.valid == 0, "read %lld: the copy stays inside the row", (long long)r);
        if (adc) {
            CHECK(I.dst[r] == dst && I.src[r] == at && I.out[r] == w.row && I.valid[r] == w.valid && I.a_start[r] == w.a_start &&
                      I.a_end[r] == w.a_end && I.offset[r] == B.offset[r] && I.scale[r] == B.scale[r],
                  "int16 columns of read %lld", (long long)r);
            CHECK((T.L.sig + (size_t)at * 2) % 16 == 0 && ((size_t)dst * 4) % 32 == 0, "read %lld: row alignment", (long long)r);
            CHECK(w.row <= max_win && w.valid <= w.row, "read %lld: at most max_win samples", (long long)r);
            CHECK(w.valid == 0 || !memcmp(base + T.L.sig + at * 2, B.i16_rows[r] + w.first, (size_t)w.valid * 2), "samples of read %lld", (long long)r);
            at += (w.valid + 7) / 8 * 8, dst += (w.row + 7) / 8 * 8;
        } else {
            const int64_t *off = image_col<int64_t>(base, T.L, FT_OFF);
            CHECK(off[r] == at && image_col<int32_t>(base, T.L, FT_ZERO)[r] == 0 && image_col<int32_t>(base, T.L, FT_LEN)[r] == w.row &&
                      w.valid == w.row,
                  "float32 columns of read %lld", (long long)r);
            CHECK(w.valid == 0 || !memcmp(base + T.L.sig + at * 4, B.f32_rows[r] + w.first, (size_t)w.valid * 4), "samples of read %lld", (long long)r);
            at += w.valid;
        }
    }
    CHECK(T.max_len == max_len, "max_len");
    CHECK(T.L.bytes == T.L.sig + (size_t)at * (adc ? 2 : 4), "the image ends behind the last staged sample");
    if (adc) CHECK(I.dst[B.n] == dst && T.dst_total == dst, "dst[n] is the decoded total");
    else CHECK(image_col<int64_t>(base, T.L, FT_OFF)[B.n] == at, "off[n] is the packed total");
    free(base);
}

// (n, stride) copies of the batch's rows, as a caller-unpacked minibatch carries them
static void check_minibatch_images(const Batch &B, int64_t padding, bool with_ok) {
    const int64_t n = B.n;
    int64_t stride = 8;
    for (int64_t r = 0; r < n; ++r) stride = std::max({stride, (int64_t)B.row_len[r], (int64_t)B.a_end[r] + padding});
    const uint8_t *ok = with_ok ? B.ok.data() : nullptr;
    // the bus-pack image of float32 rows
    {
        const ImageLayout L = image_layout(kBusPackImage, (size_t)n);
        unsigned char *base = (unsigned char *)malloc(L.bytes);
        const int64_t total = fill_bus_pack_image(base, L, n, stride, B.a_start.data(), B.a_end.data(), ok, padding);
        int64_t at = 0;
        for (int64_t r = 0; r < n; ++r) {
            const Window w = adapter_window(B.a_start[r], B.a_end[r], stride, ok && !ok[r], WindowOpts{padding, 4, 0});
            CHECK(image_col<int64_t>(base, L, BP_OFF)[r] == at && image_col<int32_t>(base, L, BP_FIRST)[r] == w.first &&
                      image_col<int32_t>(base, L, BP_LEN)[r] == w.row && image_col<int32_t>(base, L, BP_A_START)[r] == w.a_start &&
                      image_col<int32_t>(base, L, BP_A_END)[r] == w.a_end,
                  "bus-pack columns of read %lld", (long long)r);
            CHECK((at * 4) % 16 == 0 && (w.first * 4) % 16 == 0 && w.first + w.row <= stride, "bus-pack row %lld", (long long)r);
            at += (w.row + 3) / 4 * 4;
        }
        CHECK(total == at && image_col<int64_t>(base, L, BP_OFF)[n] == at, "off[n] is the packed total");
        free(base);
    }
    // the int16 image of a minibatch (fingerprint_adc_rows' loop over rows of one stride), at its own alignment (8) and at the
    // tick's (1); the latter against the tick's image of the same rows, column for column -- but `src`, which says where the
    // samples are: inside the (n, stride) array there, in the tick's own sample area here; each is held against its rule
    for (int64_t align : {8, 1}) {
        const ImageLayout L = image_layout(kAdcImage, (size_t)n);
        unsigned char *base = (unsigned char *)malloc(L.bytes);
        const AdcImage M(base, L);
        PackedOffset pos(kDecodedRowRound);
        for (int64_t r = 0; r < n; ++r) {
            const Window w = adapter_window(B.a_start[r], B.a_end[r], stride, ok && !ok[r], WindowOpts{padding, align, 0}, B.row_len[r]);
            adc_image_row(M, r, w, r * stride + w.first, pos, B.offset[r], B.scale[r]);
            CHECK(M.src[r] == r * stride + w.first && w.first % align == 0, "src of read %lld", (long long)r);
            CHECK((M.dst[r] * 4) % 32 == 0 && M.out[r] == w.row && M.valid[r] == w.valid, "read %lld", (long long)r);
        }
        M.dst[n] = pos.next;
        if (align == 1) {
            wdx_live_in in{};
            in.adc_rows = B.i16_rows.data(), in.offset = B.offset.data(), in.scale = B.scale.data(), in.row_len = B.row_len.data();
            in.n_reads = n, in.a_start = B.a_start.data(), in.a_end = B.a_end.data(), in.ok = ok;
            const TickStage T = plan_tick_stage(in, padding, (int64_t)1 << 20);   // (no window is cut: a minibatch has no max_win)
            unsigned char *tb = (unsigned char *)malloc(T.L.bytes);
            fill_tick_stage(in, T, tb);
            const AdcImage I(tb, T.L);
            for (int c = 0; c < kAdcImage.n_cols; ++c) {
                CHECK(T.L.col[c] == L.col[c], "column %d lies where the minibatch's does", c);
                if (c != AD_SRC)
                    CHECK(!memcmp(tb + T.L.col[c], base + L.col[c], ((size_t)n + kAdcImage.col[c].plus) * kAdcImage.col[c].elem),
                          "column %d of the tick's image is the minibatch's (n %lld padding %lld)", c, (long long)n, (long long)padding);
            }
            int64_t at = 0;
            for (int64_t r = 0; r < n; ++r) {
                CHECK(I.src[r] == at, "tick src of read %lld", (long long)r);
                at += (I.valid[r] + 7) / 8 * 8;
            }
            free(tb);
        }
        free(base);
    }
}

int main() {
    sweep_plan();
    sweep_delivery();
    for (const ImageDesc *D : {&kPackedRowsImage, &kBusPackImage, &kAdcImage, &kAdcTickImage, &kFloatTickImage}) check_desc(*D, "image");
    unsigned seed = 1;
    for (int64_t n : {1, 5, 64, 200})
        for (int64_t padding : {0, 7})
            for (int with_ok = 0; with_ok < 2; ++with_ok)
                for (int rep = 0; rep < (n == 1 ? 16 : 2); ++rep) {   // (one read at a time: every kind of window comes up)
                    const Batch B = make_batch(n, seed++);
                    check_tick(B, false, padding, with_ok != 0, 0);
                    check_tick(B, true, padding, with_ok != 0, kMaxWin);
                    check_minibatch_images(B, padding, with_ok != 0);
                }
    fprintf(stderr, "%lld points\n", g_points);
    return 0;
}
