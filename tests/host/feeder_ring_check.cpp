// Stand-alone check of warpdemux_amd/csrc/wdx_feeder_ring.h (tests/test_feeder_ring_host.py builds it with the system
// compiler: parts `layout` and `script` under the address / undefined-behaviour sanitizers, part `stress` under the thread
// sanitizer).  No process, no futex and no device: threads with ids of their own play the server and the workers.
//   layout   stdin: one geometry per line, "n_slots max_reads max_stride n_refs n_events n_classes sample_format refine";
//            stdout: "ring_bytes header_bytes off[16] stride[16]" of each.  Every geometry is held against the claims of the
//            header: the regions ascend, page-aligned and disjoint, and end at R->bytes == ring_bytes(g); a ring small enough
//            is allocated at exactly ring_bytes and every piece of every slot is written through its SlotView pointer.
//   script   the transitions one after the other in one thread, the contested ones in both orders.
//   stress   one server and six workers on a 2-slot ring; every worker must get its own answers.
#include "wdx_feeder_ring.h"

#include <sched.h>
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <thread>
#include <vector>

using namespace wdx;

#define CHECK(cond)                                                       \
    if (!(cond)) {                                                        \
        fprintf(stderr, "%s:%d (%s): %s\n", __FILE__, __LINE__, what, #cond); \
        return 1;                                                         \
    }

static wdx_seg_params seg_params(int K) {
    wdx_seg_params p;
    memset(&p, 0, sizeof(p));
    p.barcode_num_events = K;
    return p;
}

struct Ring {
    void *mem = nullptr;
    FeederRing *R = nullptr;
    Ring(const wdx_feeder_geometry &g, bool refine) {
        static const double query[3] = {0.5, -1.0, 2.0};
        wdx_refine_params rp;
        memset(&rp, 0, sizeof(rp));
        rp.query = query;
        rp.n_query = 3;
        const wdx_seg_params p = seg_params(g.n_events);
        mem = aligned_alloc(4096, ring_bytes(&g, refine));   // exactly: one byte beyond it is the sanitizer's
        R = ring_write(mem, &g, &p, refine ? &rp : nullptr);
    }
    ~Ring() { free(mem); }
    Ring(const Ring &) = delete;
    SlotView view(uint32_t s) const { return slot_view(R, mem, s); }
};

// every region pointer of a view, in the table's order
static void view_pointers(const SlotView &V, unsigned char *p[kRegions]) {
    unsigned char *const q[kRegions] = {V.sig, (unsigned char *)V.row_off, (unsigned char *)V.row_len, (unsigned char *)V.a_start,
                                        (unsigned char *)V.a_end, V.ok, (unsigned char *)V.dist, (unsigned char *)V.call,
                                        (unsigned char *)V.status, (unsigned char *)V.fpt, (unsigned char *)V.dwell,
                                        (unsigned char *)V.stats, (unsigned char *)V.prob, (unsigned char *)V.pred,
                                        (unsigned char *)V.conf, (unsigned char *)V.ridx};
    memcpy(p, q, sizeof(q));
}
static bool all_bytes(const unsigned char *p, size_t n, unsigned char tag) {
    return n == 0 || (p[0] == tag && memcmp(p, p + 1, n - 1) == 0);
}
static unsigned char tag_of(uint32_t s, int r) { return (unsigned char)((s * kRegions + (uint32_t)r) % 251u + 1u); }

static int layout() {
    const char *what = "layout";
    constexpr size_t kAllocLimit = 8u << 20;
    long long n_cases = 0, n_written = 0;
    long long in[8];
    while (scanf("%lld %lld %lld %lld %lld %lld %lld %lld", &in[0], &in[1], &in[2], &in[3], &in[4], &in[5], &in[6], &in[7]) == 8) {
        wdx_feeder_geometry g;
        memset(&g, 0, sizeof(g));
        g.n_slots = (int32_t)in[0];
        g.max_reads = in[1];
        g.max_stride = in[2];
        g.n_refs = in[3];
        g.n_events = (int32_t)in[4];
        g.n_classes = (int32_t)in[5];
        g.sample_format = (int32_t)in[6];
        const bool refine = in[7] != 0;
        RingGeo G;
        CHECK(geometry(&g, refine, G));
        const RingLayout L = ring_layout(G);
        const size_t bytes = ring_bytes(&g, refine), header = ring_header_bytes(refine);
        printf("%zu %zu", bytes, header);
        for (int r = 0; r < kRegions; ++r) printf(" %llu", (unsigned long long)L.off[r]);
        for (int r = 0; r < kRegions; ++r) printf(" %zu", region_stride(G, r));
        printf("\n");
        // ascending, page-aligned, disjoint, nothing between them, the last one ends the ring
        size_t o = header;
        CHECK(header % 4096 == 0 && header >= sizeof(FeederRing));
        for (int r = 0; r < kRegions; ++r) {
            CHECK(L.off[r] == o && o % 4096 == 0 && region_stride(G, r) % 4096 == 0);
            CHECK(region_stride(G, r) >= region_table()[r].bytes(G));
            o += G.n_slots * region_stride(G, r);
        }
        CHECK(o == bytes && L.bytes == bytes);
        // what the sample region must hold: the rows, packed; the predict path's fingerprints
        CHECK(G.sig_floats * 4 >= G.mr * G.K * 8);
        CHECK(G.sig_floats * (G.int16 ? 2 : 1) >= G.mr * (size_t)g.max_stride);
        ++n_cases;
        if (bytes > kAllocLimit) continue;
        const Ring ring(g, refine);
        FeederRing *R = ring.R;
        CHECK(R->magic == kFeederMagic && R->bytes == bytes && R->sig_floats == G.sig_floats);
        CHECK(R->sig_slot_bytes == region_stride(G, kSig) && (R->kind == kRingRefine) == refine);
        for (int r = 0; r < kRingRegions; ++r) CHECK(R->off[r] == L.off[r]);
        static FeederRing record;
        record = *R;
        if (refine) CHECK(refine_ext(R)->off_ridx == L.off[kRidx] && refine_ext_offset() + sizeof(FeederRefine) <= header);
        // every piece of every slot, at its whole stride, through the view: the pieces tile [header, bytes) exactly, so a
        // tag that survives everywhere says they are where the table puts them and disjoint
        for (uint32_t s = 0; s < R->n_slots; ++s) {
            unsigned char *p[kRegions];
            view_pointers(ring.view(s), p);
            for (int r = 0; r < kRegions; ++r) {
                const size_t stride = region_stride(G, r);
                CHECK((p[r] == nullptr) == (stride == 0));
                if (p[r]) CHECK(p[r] == (unsigned char *)ring.mem + L.off[r] + s * stride);
                if (p[r]) memset(p[r], tag_of(s, r), stride);
            }
        }
        for (uint32_t s = 0; s < R->n_slots; ++s) {
            const SlotView V = ring.view(s);
            unsigned char *p[kRegions];
            view_pointers(V, p);
            for (int r = 0; r < kRegions; ++r) CHECK(all_bytes(p[r], region_stride(G, r), tag_of(s, r)));
            CHECK((V.offset != nullptr) == G.int16 && (V.scale != nullptr) == G.int16 && (V.row_win != nullptr) == G.int16);
            if (G.int16) {
                // the calibration lies behind the samples, inside the piece
                for (size_t i = 0; i < G.mr; ++i) V.offset[i] = 1.0f, V.scale[i] = 2.0f, V.row_win[i] = 3;
                CHECK((unsigned char *)V.offset == V.sig + G.sig_floats * 4 && V.scale == V.offset + G.mr);
                CHECK((unsigned char *)(V.row_win + G.mr) <= V.sig + region_stride(G, kSig));
                CHECK(all_bytes(V.sig, G.sig_floats * 4, tag_of(s, kSig)));
                for (size_t i = 0; i < G.mr; ++i) CHECK(V.offset[i] == 1.0f && V.scale[i] == 2.0f && V.row_win[i] == 3);
            }
            // the predict path: max_reads x n_events doubles in the sample region; the rows' last index, row_off[max_reads]
            double *X = (double *)V.sig;
            for (size_t i = 0; i < G.mr * G.K; ++i) X[i] = 0.25;
            V.row_off[G.mr] = 7;
        }
        CHECK(memcmp(R, &record, sizeof(FeederRing)) == 0);   // (and the record in front of them is as it was)
        ++n_written;
    }
    fprintf(stderr, "%lld geometries, %lld written\n", n_cases, n_written);
    return 0;
}

static wdx_feeder_geometry small_geometry(int n_slots) {
    wdx_feeder_geometry g;
    memset(&g, 0, sizeof(g));
    g.n_slots = n_slots;
    g.max_reads = 4;
    g.max_stride = 16;
    g.n_refs = 2;
    g.n_events = 5;
    g.n_classes = 3;
    return g;
}

static int script() {
    const char *what = "";
    const auto nobody_gone = [](int32_t) { return false; };
    const int32_t A = 11, B = 12, C = 13;
    for (const uint32_t mode : {(uint32_t)kModeRows, (uint32_t)kModePredict}) {
        what = mode == kModeRows ? "life cycle, rows" : "life cycle, predict";
        const Ring ring(small_geometry(3), false);
        FeederRing *R = ring.R;
        const int s = ring_try_claim(R, A);
        CHECK(s == A % 3 && ld(&R->slot[s].state) == word_of(A, kFilling));
        const SlotView V = ring.view((uint32_t)s);
        V.S->mode = mode;
        V.S->n_reads = 4;
        if (mode == kModePredict)
            for (int i = 0; i < 4 * 5; ++i) ((double *)V.sig)[i] = i;
        else
            for (int i = 0; i < 4; ++i) V.row_len[i] = i;
        const uint32_t gen = slot_publish(*V.S, A);
        CHECK(gen == 1 && ld(&V.S->state) == word_of(A, kReady));
        CHECK(ring_reclaim(R, nobody_gone) == 0);
        uint32_t taken = 0;
        CHECK(slot_take(*V.S, ld(&V.S->state), taken) && taken == gen && ld(&V.S->state) == word_of(A, kInflight));
        for (int i = 0; i < 4; ++i) V.pred[i] = mode == kModePredict ? (int32_t)((double *)V.sig)[i * 5] : V.row_len[i];
        V.S->rc = WDX_SUCCESS;
        slot_hand_over(*V.S, taken);
        CHECK(ld(&V.S->state) == word_of(A, kDone) && V.S->gen_done == gen);
        for (int i = 0; i < 4; ++i) CHECK(V.pred[i] == (mode == kModePredict ? 5 * i : i));
        slot_release(*V.S);
        CHECK(ld(&V.S->state) == kFree);
        // the next turn with the slot is another generation
        CHECK(slot_try_claim(*V.S, B) && slot_publish(*V.S, B) == 2 && V.S->gen_done == 1);
    }
    {
        what = "take, then give up: the server wins and the owner sees it";
        const Ring ring(small_geometry(1), false);
        FeederSlot &S = ring.R->slot[0];
        CHECK(ring_try_claim(ring.R, A) == 0);
        slot_publish(S, A);
        uint32_t gen = 0;
        CHECK(slot_take(S, ld(&S.state), gen));
        CHECK(slot_give_up(S, A) == kDisowned && ld(&S.state) == word_of(0, kInflight));
        CHECK(ring_try_claim(ring.R, B) < 0);
    }
    {
        what = "give up, then take: the owner wins and the server sees it";
        const Ring ring(small_geometry(1), false);
        FeederSlot &S = ring.R->slot[0];
        CHECK(ring_try_claim(ring.R, A) == 0);
        slot_publish(S, A);
        const uint32_t seen = ld(&S.state);   // the server looked ...
        CHECK(slot_give_up(S, A) == kGaveBack && ld(&S.state) == kFree);
        uint32_t gen = 77;
        CHECK(!slot_take(S, seen, gen) && gen == 77 && ld(&S.state) == kFree);   // ... and took too late
        // the same with the slot already in other hands, and with another owner's READY in its place
        CHECK(ring_try_claim(ring.R, C) == 0);
        CHECK(!slot_take(S, seen, gen) && ld(&S.state) == word_of(C, kFilling));
        slot_publish(S, C);
        CHECK(!slot_take(S, seen, gen) && ld(&S.state) == word_of(C, kReady));
    }
    {
        what = "a server believed dead resumes (ADVICE.md item 1)";
        const Ring ring(small_geometry(1), false);
        FeederRing *R = ring.R;
        FeederSlot &S = R->slot[0];
        CHECK(ring_try_claim(R, A) == 0);
        const uint32_t gen_a = slot_publish(S, A);                       // 1. A publishes
        uint32_t taken = 0;
        CHECK(slot_take(S, ld(&S.state), taken) && taken == gen_a);      // 2. the server takes the slot
        CHECK(slot_give_up(S, A) == kDisowned);                          // 3. A gives up
        // 4. the slot reaches nobody while the server holds it: no reclaim returns it, B cannot claim it
        CHECK(ring_reclaim(R, [](int32_t) { return true; }) == 0 && ring_try_claim(R, B) < 0);
        CHECK(phase_of(ld(&S.state)) == kInflight);
        S.rc = WDX_SUCCESS;
        slot_hand_over(S, taken);                                        // 5. the resumed server hands A's minibatch over
        CHECK(ld(&S.state) == word_of(0, kDone) && S.gen_done == gen_a);
        // an abandoned in-flight slot is back in the ring after the hand-over plus one reclaim, whoever is alive
        CHECK(ring_try_claim(R, B) < 0 && ring_reclaim(R, nobody_gone) == 1 && ld(&S.state) == kFree);
        CHECK(ring_try_claim(R, B) == 0);
        const uint32_t gen_b = slot_publish(S, B);
        // B's generation is the next one: what the server handed over for A is not an answer for B
        CHECK(gen_b == gen_a + 1 && S.gen_done != gen_b && ld(&S.state) == word_of(B, kReady));
    }
    {
        what = "give up on an answered slot; put a taken slot back";
        const Ring ring(small_geometry(1), false);
        FeederSlot &S = ring.R->slot[0];
        CHECK(ring_try_claim(ring.R, A) == 0);
        const uint32_t gen_a = slot_publish(S, A);
        uint32_t gen = 0;
        CHECK(slot_take(S, ld(&S.state), gen) && slot_untake(S) && ld(&S.state) == word_of(A, kReady));
        CHECK(slot_take(S, ld(&S.state), gen) && gen == gen_a);
        slot_hand_over(S, gen);
        CHECK(slot_give_up(S, A) == kAnswered && ld(&S.state) == word_of(A, kDone));
        slot_release(S);
        CHECK(ring_try_claim(ring.R, B) == 0);
        slot_publish(S, B);
        CHECK(slot_take(S, ld(&S.state), gen) && slot_give_up(S, B) == kDisowned && !slot_untake(S));
        CHECK(ld(&S.state) == word_of(0, kInflight));
    }
    {
        what = "reclaim: FILLING / DONE slots of gone owners and nothing else";
        const Ring ring(small_geometry(9), false);
        FeederRing *R = ring.R;
        const int32_t gone_id = 100, live_id = 5;
        const uint32_t before[9] = {word_of(gone_id, kFilling), word_of(live_id, kFilling), word_of(gone_id, kReady),
                                    word_of(gone_id, kInflight), word_of(gone_id, kDone),   word_of(live_id, kDone),
                                    kFree,                       word_of(0, kInflight),     word_of(0, kDone)};
        for (int s = 0; s < 9; ++s) st(&R->slot[s].state, before[s]);
        CHECK(ring_reclaim(R, [&](int32_t id) { return id == gone_id; }) == 3);
        for (int s = 0; s < 9; ++s) CHECK(ld(&R->slot[s].state) == ((s == 0 || s == 4 || s == 8) ? (uint32_t)kFree : before[s]));
        CHECK(ring_reclaim(R, [&](int32_t id) { return id == gone_id; }) == 0);
    }
    fprintf(stderr, "script ok\n");
    return 0;
}

// The answer the server owes a job: a function of the payload, which names the worker and the job.
static int32_t answer_of(int32_t worker, int32_t job, int i) { return worker * 1000003 + job * 7 + i; }

static int stress(int jobs_per_worker) {
    const char *what = "stress";
    constexpr int kWorkers = 6;
    const Ring ring(small_geometry(2), false);
    FeederRing *R = ring.R;
    const int mr = (int)R->max_reads;
    std::atomic<bool> stop{false};
    std::atomic<long long> served{0}, reclaimed{0}, wrong{0}, gave_back{0}, disowned{0};
    std::thread server([&]() {
        while (!stop.load(std::memory_order_acquire)) {
            bool any = false;
            for (uint32_t s = 0; s < R->n_slots; ++s) {
                const uint32_t v = ld(&R->slot[s].state);
                uint32_t gen;
                if (phase_of(v) != kReady || !slot_take(R->slot[s], v, gen)) continue;
                const SlotView V = slot_view(R, ring.mem, s);
                if (gen % 2) sched_yield();   // (the device at work: time for the owner to lose patience with a slot in flight)
                for (int i = 0; i < mr; ++i) V.status[i] = answer_of(V.a_start[i], V.a_end[i], i);
                V.S->rc = (int32_t)V.S->n_reads;
                slot_hand_over(*V.S, gen);
                served.fetch_add(1);
                any = true;
            }
            reclaimed.fetch_add(ring_reclaim(R, [](int32_t) { return false; }));   // (what the workers disowned)
            if (!any) sched_yield();
        }
    });
    std::vector<std::thread> workers;
    for (int w = 1; w <= kWorkers; ++w)
        workers.emplace_back([&, w]() {
            for (int job = 0; job < jobs_per_worker; ++job) {
                bool impatient = job % 4 == 1;   // every 4th job its worker loses patience, once, at once or a yield or two
                                                 // later: the contest with the server's take, live, won by either side
                for (bool answered = false; !answered;) {
                    int s;
                    while ((s = ring_try_claim(R, w)) < 0) sched_yield();
                    const SlotView V = slot_view(R, ring.mem, (uint32_t)s);
                    for (int i = 0; i < mr; ++i) V.a_start[i] = w, V.a_end[i] = job;
                    V.S->n_reads = job;
                    const uint32_t gen = slot_publish(*V.S, w);
                    if (impatient) {
                        impatient = false;
                        for (int y = 0; y < job / 4 % 3; ++y) sched_yield();
                        const GiveUp g = slot_give_up(*V.S, w);
                        if (g == kGaveBack) gave_back.fetch_add(1);
                        if (g == kDisowned) disowned.fetch_add(1);
                        if (g != kAnswered) continue;   // (the slot is not this worker's any more: once more from the start)
                    }
                    while (phase_of(ld(&V.S->state)) != kDone) sched_yield();
                    bool ok = V.S->gen_done == gen && owner_of(ld(&V.S->state)) == w && V.S->rc == job;
                    for (int i = 0; i < mr; ++i) ok = ok && V.status[i] == answer_of(w, job, i);
                    if (!ok) wrong.fetch_add(1);
                    slot_release(*V.S);
                    answered = true;
                }
            }
        });
    for (std::thread &t : workers) t.join();
    // what was disowned last comes back once the server has answered it
    for (int spin = 0; spin < 1000000 && reclaimed.load() < disowned.load(); ++spin) sched_yield();
    stop.store(true, std::memory_order_release);
    server.join();
    fprintf(stderr, "stress: %d workers x %d jobs, served %lld, given back %lld, disowned %lld, reclaimed %lld, wrong %lld\n",
            kWorkers, jobs_per_worker, served.load(), gave_back.load(), disowned.load(), reclaimed.load(), wrong.load());
    CHECK(wrong.load() == 0);
    CHECK(served.load() == (long long)kWorkers * jobs_per_worker + disowned.load());
    CHECK(reclaimed.load() == disowned.load());
    for (uint32_t s = 0; s < R->n_slots; ++s) CHECK(ld(&R->slot[s].state) == kFree);
    return 0;
}

int main(int argc, char **argv) {
    const char *part = argc > 1 ? argv[1] : "";
    if (!strcmp(part, "layout")) return layout();
    if (!strcmp(part, "script")) return script();
    if (!strcmp(part, "stress")) return stress(argc > 2 ? atoi(argv[2]) : 8000);
    fprintf(stderr, "usage: feeder_ring_check layout|script|stress [jobs]\n");
    return 2;
}
