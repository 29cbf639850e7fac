// The feeder's ring in shared memory, stated once: its records, the layout of a slot's data regions and the transitions
// of a slot's state word (plain host C++17: no HIP, nothing of the context, no futex and no /proc, so the system compiler
// builds it alone and threads of one process can play server and workers: tests/host/feeder_ring_check.cpp).
// wdx_feeder.hip adds what needs a process around it: futex sleeping, the liveness of pids, the heartbeat, the device.
//
// Slot life cycle.  One word per slot, (owner id << 8) | phase:
//   FREE -> FILLING(me)            slot_try_claim / ring_try_claim   compare-and-swap, the owner in the same atomic
//   FILLING(me) -> READY(me)       slot_publish                      a new generation of the slot
//   READY(o) -> INFLIGHT(o)        slot_take                         compare-and-swap on the full word   } the two sides
//   READY(me) -> FREE              slot_give_up                      compare-and-swap on the full word   } of one contest
//   INFLIGHT(o) -> DONE(o)         slot_hand_over                    gen_done = the generation recorded by slot_take
//   DONE(me) -> FREE               slot_release
//   FILLING / DONE(gone) -> FREE   ring_reclaim                      compare-and-swap; owner 0 counts as gone
// A worker that gives up on a slot the server holds disowns it (INFLIGHT(me) -> INFLIGHT(0)): the hand-over then makes it
// DONE(0), which the next reclaim returns to the ring -- the slot reaches nobody else while the server may write to it.
// The plain fields of a slot and its data regions belong to whoever the word names: the owner while FILLING / DONE, the
// server while INFLIGHT, nobody while READY.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/wdx.h"

namespace wdx {

constexpr uint32_t kFeederMagic = 0x57444633u;  // "WDF3"
// Ring slots and in-flight slots are different things: a ring slot is held by its worker while the worker COPIES its
// minibatch in (milliseconds) and again while it copies the results out, the context keeps at most WDX_MAX_SLOTS of
// them in flight on the device.  With as many ring slots as in-flight slots the ring is what sixteen workers queue for.
constexpr int kMaxRingSlots = WDX_FEEDER_MAX_RING_SLOTS;
enum : uint32_t { kFree = 0, kFilling = 1, kReady = 2, kInflight = 3, kDone = 4 };
enum : uint32_t { kModeRows = 0, kModePredict = 1 };

inline uint32_t phase_of(uint32_t v) { return v & 0xffu; }
inline int32_t owner_of(uint32_t v) { return (int32_t)(v >> 8); }
inline uint32_t word_of(int32_t id, uint32_t phase) { return ((uint32_t)id << 8) | phase; }

struct FeederSlot {
    uint32_t state;    // futex word: (owner pid << 8) | phase
    int32_t rc;        // WDX_* of the slot's last minibatch
    int64_t n_reads;
    uint32_t has_ok, want, mode, gen, gen_done, pad_;
    char err[224];     // wdx_last_error() of the feeder for rc != 0
};
static_assert(sizeof(FeederSlot) == 264, "slot record");

// The data regions, in the order they lie in the ring; each holds n_slots consecutive per-slot pieces.
enum Region { kSig, kRowOff, kRowLen, kAStart, kAEnd, kOk, kDist, kCall, kStatus, kFpt, kDwell, kStats, kProb, kPred, kConf,
              kRidx, kRegions };
constexpr int kRingRegions = kRidx;   // those whose offset the FeederRing record keeps; kRidx's is FeederRefine's

struct FeederRing {
    uint32_t magic, n_slots;
    int64_t max_reads, max_stride, n_refs;
    int32_t n_events, n_classes;
    int32_t sample_format, kind;   // WDX_FEEDER_SAMPLES_*: what the sample region of a slot holds; kRingPlain / kRingRefine
    wdx_seg_params params;   // what every minibatch is fingerprinted with (workers read `padding` to pack their rows)
    uint64_t off[kRingRegions];   // byte offsets of the data regions kSig .. kConf
    uint64_t bytes;
    uint64_t sig_floats;     // per-slot capacity of the sample region, in 4-byte units
    // bytes from one slot's sample region to the next; int16 rings keep the reads' calibration behind the samples:
    // offset float32[max_reads] | scale float32[max_reads] | row_win int32[max_reads] at byte sig_floats * 4
    uint64_t sig_slot_bytes;
    uint32_t seq;        // futex: bumped by a worker that made a slot READY
    uint32_t free_seq;   // futex: bumped by whoever made a slot FREE
    uint32_t stop;       // 1: wdx_feeder_stop was called (or the server is leaving)
    int32_t server_pid;  // the feeder process while it serves, else 0
    uint64_t served;     // minibatches handed back (statistics)
    uint64_t reclaimed;  // slots taken back from dead workers (statistics)
    int64_t heartbeat_ns;  // CLOCK_MONOTONIC of the server's latest sign of life
    FeederSlot slot[kMaxRingSlots];
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// A refine ring (wdx_feeder_ring_init_refine) keeps this behind the FeederRing record, inside the header area; a plain
// ring (kind 0, the word wdx_feeder_ring_init has always left zero) has nothing there and keeps its layout byte for byte.
enum : int32_t { kRingPlain = 0, kRingRefine = 1 };
constexpr int kRingMaxQuery = 96;    // wdx_refine_params.n_query's limit
constexpr int kRingMaxSeries = 128;  // ... and that of num_events + 1
struct FeederRefine {
    wdx_refine_params rp;   // (rp.query is a pointer of the process that made the ring: every user points it at `query`)
    double query[kRingMaxQuery];
    uint64_t off_ridx;      // per-slot refine_idx regions, max_reads * 3 int32 each
};
inline size_t refine_ext_offset() { return align_up(sizeof(FeederRing), 16); }
inline size_t ring_header_bytes(bool refine) {
    return align_up(refine ? refine_ext_offset() + sizeof(FeederRefine) : sizeof(FeederRing), 4096);
}
inline FeederRefine *refine_ext(FeederRing *R) {
    return R->kind == kRingRefine ? (FeederRefine *)((unsigned char *)R + refine_ext_offset()) : nullptr;
}

// ---- the layout -------------------------------------------------------------------------------------------------------
// What the sizes of a slot's pieces depend on: from wdx_feeder_geometry when a ring is sized and laid out, from the ring's
// own record when a slot is looked at.
struct RingGeo {
    size_t n_slots, mr, nY, K, kc;   // max_reads, n_refs, n_events, n_classes
    size_t sig_floats;
    bool int16, refine;
};

inline bool geometry(const wdx_feeder_geometry *g, bool refine, RingGeo &G) {
    if (!g || g->n_slots < 1 || g->n_slots > kMaxRingSlots || g->max_reads < 1 || g->max_stride < 1 || g->n_refs < 0 ||
        g->n_events < 0 || g->n_classes < 0 || g->n_classes > 16 ||
        (g->sample_format != WDX_FEEDER_SAMPLES_FLOAT32 && g->sample_format != WDX_FEEDER_SAMPLES_INT16))
        return false;
    G = RingGeo{(size_t)g->n_slots, (size_t)g->max_reads, (size_t)g->n_refs, (size_t)g->n_events, (size_t)g->n_classes, 0,
                g->sample_format == WDX_FEEDER_SAMPLES_INT16, refine};
    // a packed row starts on a 16-byte boundary: up to 3 + 3 floats of slack per row; fingerprints for
    // wdx_feeder_predict (max_reads x n_events doubles) use the same region
    G.sig_floats = G.mr * (size_t)((g->max_stride + 3) / 4 * 4 + 4);
    // int16 samples: rows start on 16-byte boundaries = 8 samples, 7 + 7 of slack per row, two samples per 4-byte unit
    if (G.int16) G.sig_floats = G.mr * (size_t)((g->max_stride + 7) / 8 * 8 + 8) / 2;
    if (G.K * 2 * G.mr > G.sig_floats) G.sig_floats = G.K * 2 * G.mr;
    return true;
}
inline RingGeo geometry_of(const FeederRing *R) {
    return RingGeo{R->n_slots, (size_t)R->max_reads, (size_t)R->n_refs, (size_t)R->n_events, (size_t)R->n_classes,
                   (size_t)R->sig_floats, R->sample_format == WDX_FEEDER_SAMPLES_INT16, R->kind == kRingRefine};
}

// THE table: a region's name and the bytes one slot's piece of it holds -- 0 where the geometry has no such region (no
// fingerprints without n_events, no classifier outputs without n_classes, refine_idx on a refine ring only).  A piece
// occupies its bytes rounded up to a page (region_stride).
struct RegionDef {
    const char *name;
    size_t (*bytes)(const RingGeo &);
};
inline const RegionDef *region_table() {
    static const RegionDef T[kRegions] = {
        {"sig", [](const RingGeo &g) { return g.sig_floats * 4 + (g.int16 ? g.mr * 12 : 0); }},
        {"row_off", [](const RingGeo &g) { return (g.mr + 1) * 8; }},
        {"row_len", [](const RingGeo &g) { return g.mr * 4; }},
        {"a_start", [](const RingGeo &g) { return g.mr * 4; }},
        {"a_end", [](const RingGeo &g) { return g.mr * 4; }},
        {"ok", [](const RingGeo &g) { return g.mr; }},
        {"dist", [](const RingGeo &g) { return g.mr * (g.nY ? g.nY : 1) * 4; }},
        {"call", [](const RingGeo &g) { return g.mr * 4; }},
        {"status", [](const RingGeo &g) { return g.mr * 4; }},
        {"fpt", [](const RingGeo &g) { return g.mr * g.K * 8; }},
        {"dwell", [](const RingGeo &g) { return g.mr * g.K * 8; }},
        {"stats", [](const RingGeo &g) { return g.K ? g.mr * 48 : 0; }},
        {"prob", [](const RingGeo &g) { return g.mr * g.kc * 8; }},
        {"pred", [](const RingGeo &g) { return g.kc ? g.mr * 4 : 0; }},
        {"conf", [](const RingGeo &g) { return g.kc ? g.mr * 8 : 0; }},
        {"ridx", [](const RingGeo &g) { return g.refine ? g.mr * 12 : 0; }},
    };
    return T;
}
inline size_t region_stride(const RingGeo &G, int r) { return align_up(region_table()[r].bytes(G), 4096); }

// Offsets of the regions behind the header, and the ring's size.  An absent region keeps the offset of its successor.
struct RingLayout {
    uint64_t off[kRegions], bytes;
};
inline RingLayout ring_layout(const RingGeo &G) {
    RingLayout L;
    size_t o = ring_header_bytes(G.refine);
    for (int r = 0; r < kRegions; ++r) {
        L.off[r] = o;
        o += G.n_slots * region_stride(G, r);
    }
    L.bytes = o;
    return L;
}
inline size_t ring_bytes(const wdx_feeder_geometry *g, bool refine) {
    RingGeo G;
    return geometry(g, refine, G) ? (size_t)ring_layout(G).bytes : 0;
}

// Writes the record of a ring of geometry `g` (checked by the caller: geometry()) at `mem`, ring_bytes(g) bytes; rp: a
// refine ring.  The magic goes in last.
inline FeederRing *ring_write(void *mem, const wdx_feeder_geometry *g, const wdx_seg_params *p, const wdx_refine_params *rp) {
    RingGeo G;
    (void)geometry(g, rp != nullptr, G);
    const RingLayout L = ring_layout(G);
    FeederRing *R = (FeederRing *)mem;
    memset(R, 0, sizeof(FeederRing));
    R->n_slots = (uint32_t)g->n_slots;
    R->max_reads = g->max_reads;
    R->max_stride = g->max_stride;
    R->n_refs = g->n_refs;
    R->n_events = g->n_events;
    R->n_classes = g->n_classes;
    R->sample_format = g->sample_format;
    R->params = *p;
    R->sig_floats = G.sig_floats;
    R->sig_slot_bytes = region_stride(G, kSig);
    memcpy(R->off, L.off, sizeof(R->off));
    if (rp) {
        R->kind = kRingRefine;
        FeederRefine *X = refine_ext(R);
        memset(X, 0, sizeof(FeederRefine));
        X->rp = *rp;
        X->rp.query = nullptr;
        memcpy(X->query, rp->query, (size_t)rp->n_query * 8);
        X->off_ridx = L.off[kRidx];
    }
    R->bytes = L.bytes;
    __atomic_store_n(&R->magic, kFeederMagic, __ATOMIC_RELEASE);
    return R;
}

// Every pointer of slot `s`, computed once; a region the ring does not have is null.
struct SlotView {
    FeederSlot *S;
    unsigned char *sig;   // float32 or int16 samples, packed rows; wdx_feeder_predict's (n, n_events) doubles
    float *offset, *scale;   // int16 rings: the calibration behind the samples, max_reads each
    int32_t *row_win;        // ...
    int64_t *row_off;
    int32_t *row_len, *a_start, *a_end;
    uint8_t *ok;
    float *dist;
    int32_t *call, *status;
    double *fpt;
    int64_t *dwell;
    double *stats, *prob;
    int32_t *pred;
    double *conf;
    int32_t *ridx;
};
inline SlotView slot_view(FeederRing *R, void *base, uint32_t s) {
    const RingGeo G = geometry_of(R);
    const FeederRefine *X = refine_ext(R);
    unsigned char *p[kRegions];
    for (int r = 0; r < kRegions; ++r) {
        const size_t stride = region_stride(G, r);
        const uint64_t off = r < kRingRegions ? R->off[r] : X ? X->off_ridx : 0;
        p[r] = stride ? (unsigned char *)base + off + (size_t)s * stride : nullptr;
    }
    float *cal = G.int16 ? (float *)(p[kSig] + G.sig_floats * 4) : nullptr;
    return SlotView{&R->slot[s], p[kSig], cal, cal ? cal + G.mr : nullptr, cal ? (int32_t *)(cal + 2 * G.mr) : nullptr,
                    (int64_t *)p[kRowOff], (int32_t *)p[kRowLen], (int32_t *)p[kAStart], (int32_t *)p[kAEnd], p[kOk],
                    (float *)p[kDist], (int32_t *)p[kCall], (int32_t *)p[kStatus], (double *)p[kFpt], (int64_t *)p[kDwell],
                    (double *)p[kStats], (double *)p[kProb], (int32_t *)p[kPred], (double *)p[kConf], (int32_t *)p[kRidx]};
}

// ---- the transitions ----------------------------------------------------------------------------------------------------
inline uint32_t ld(const uint32_t *p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }
inline void st(uint32_t *p, uint32_t v) { __atomic_store_n(p, v, __ATOMIC_RELEASE); }
inline bool cas(uint32_t *p, uint32_t &expect, uint32_t v) {   // (a failure leaves the word's value in `expect`)
    return __atomic_compare_exchange_n(p, &expect, v, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE);
}

inline bool slot_try_claim(FeederSlot &S, int32_t me) {
    uint32_t expect = kFree;
    return cas(&S.state, expect, word_of(me, kFilling));
}
// a FREE slot for `me`, looked for from a slot of its own so that the claimants do not all contend for slot 0; -1: none
inline int ring_try_claim(FeederRing *R, int32_t me) {
    const uint32_t first = (uint32_t)me % R->n_slots;
    for (uint32_t k = 0; k < R->n_slots; ++k) {
        const uint32_t c = (first + k) % R->n_slots;
        if (slot_try_claim(R->slot[c], me)) return (int)c;
    }
    return -1;
}

// the owner has filled the slot: the generation its answer must carry
inline uint32_t slot_publish(FeederSlot &S, int32_t me) {
    const uint32_t gen = ++S.gen;
    st(&S.state, word_of(me, kReady));
    return gen;
}

// The server takes a slot it saw READY as `seen`.  False: the owner gave up first (the slot may be anybody's by now) -- skip
// it.  True: the slot is the server's until slot_hand_over, and `gen` is the generation to hand over.
inline bool slot_take(FeederSlot &S, uint32_t seen, uint32_t &gen) {
    if (!cas(&S.state, seen, word_of(owner_of(seen), kInflight))) return false;
    gen = S.gen;
    return true;
}
// ... and puts it back untouched (it cannot submit now).  False: the owner disowned the slot meanwhile -- hand it over.
inline bool slot_untake(FeederSlot &S) {
    uint32_t v = ld(&S.state);
    return owner_of(v) != 0 && cas(&S.state, v, word_of(owner_of(v), kReady));
}
// (the slot's rc / err and its result regions are written before this; the owner may disown the slot at any time)
inline void slot_hand_over(FeederSlot &S, uint32_t gen) {
    S.gen_done = gen;
    uint32_t v = ld(&S.state);
    while (!cas(&S.state, v, word_of(owner_of(v), kDone))) {}
}

inline void slot_release(FeederSlot &S) { st(&S.state, (uint32_t)kFree); }

// The owner of a published slot stops waiting for it (the server is believed gone).  kGaveBack: the slot was never taken
// and is FREE again; kDisowned: the server holds it, and whatever it hands over goes to nobody (DONE(0), then ring_reclaim);
// kAnswered: the server has handed it over after all -- the slot is DONE and the owner's as usual.
enum GiveUp { kGaveBack, kDisowned, kAnswered };
inline GiveUp slot_give_up(FeederSlot &S, int32_t me) {
    for (;;) {
        uint32_t ready = word_of(me, kReady), held = word_of(me, kInflight);
        if (cas(&S.state, ready, (uint32_t)kFree)) return kGaveBack;
        if (cas(&S.state, held, word_of(0, kInflight))) return kDisowned;
        if (phase_of(held) != kReady) return kAnswered;   // (READY again: the server put the slot back in between)
    }
}

// Slots a gone owner left in FILLING / DONE go back to the ring (READY / INFLIGHT ones pass through the server first).
// gone(id): is this owner gone?  Owner 0, a disowned slot, always is.  Returns the number of slots freed.
template <class Gone>
inline int ring_reclaim(FeederRing *R, Gone gone) {
    int n = 0;
    for (uint32_t s = 0; s < R->n_slots; ++s) {
        uint32_t v = ld(&R->slot[s].state);
        const uint32_t ph = phase_of(v);
        if ((ph == kFilling || ph == kDone) && (owner_of(v) == 0 || gone(owner_of(v))) && cas(&R->slot[s].state, v, (uint32_t)kFree))
            ++n;
    }
    return n;
}

}  // namespace wdx
