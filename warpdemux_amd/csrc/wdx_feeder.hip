// Many worker processes, one GPU-facing process: the shared-memory minibatch ring behind include/wdx.h's wdx_feeder_*.
//
// The reference runs `-j 8..16` forked workers (file_proc.py:1197-1243), each of which would drive the GPU from its own
// process.  Sixteen HIP processes on one device collapse (0.86 M reads/s where four reach 2.17 M; a cross-process gate that
// lets only four of them work at a time made it worse -- the device time-slices the processes' queues whether they have
// work or not).  The cure is ONE process that owns the context and keeps up to eight minibatches in flight
// (wdx_demux_submit_ex / wdx_demux_wait_ex) for everybody: the workers copy their minibatch into a slot of a ring in
// shared memory, which the feeder has page-locked, and sleep on the slot until the results are there.  Nothing on the
// workers' side touches HIP -- a worker needs no context and initialises no runtime.
//
// What a worker gets back is what the reference's worker needs from its minibatch (file_proc.py:380-454): the
// ReadResults' arrays (fingerprint, dwell times, six statistics, status: WDX_WANT_FPT / _DWELL / _STATS), the
// nearest-reference call and distance rows, and the DTW_SVM prediction (WDX_WANT_SVM: prob / pred / conf) -- one pass
// over the rows for all of it.  wdx_feeder_predict is model.predict() on fingerprints the worker already holds.
// WDX_WANT_BOOST / wdx_feeder_predict_boost are the same two for the tRNA models' class (Fpt_Boost, wdx_boost_set_model):
// the trees run on the fingerprints themselves, so such a ring needs no references (n_refs == 0, plain or refine).
//
// A worker copies only what the kernels read: samples [a_start - padding, a_end + padding) of each row, back to back
// (PACKED rows, wdx_minibatch_in.row_off) -- 18.7 MB instead of 40 MB per 1000-read minibatch on both of the worker's
// copies' sides (its own memcpy and the feeder's DMA).  A ring laid out for int16 samples (wdx_feeder_geometry.sample_format
// = WDX_FEEDER_SAMPLES_INT16, wdx_feeder_run_adc) halves that again: the worker copies the raw ADC windows and each read's
// offset / scale, the server submits through wdx_demux_submit_adc and the device calibrates (wdx_adc.hip).
//
// The ring itself -- its records, the one table a slot's data regions are laid out and addressed by (slot_view), and the
// transitions of a slot's state word, FREE -> FILLING -> READY -> INFLIGHT -> DONE -> FREE -- is wdx_feeder_ring.h, which
// needs no process and no device around it.  This file is what does: the sleeping, who is alive, and the GPU.
// Workers sleep on `free_seq` when no slot is FREE and on their slot's word until it is DONE; the feeder sleeps on `seq`
// when nothing is READY or in flight.  Shared futexes (no FUTEX_PRIVATE_FLAG): the words live in memory mapped by several
// processes.
//   * a worker that dies while it holds a slot (OOM kill, pool.terminate()): the feeder's idle loop and every claimant
//     that finds the ring full give FILLING / DONE slots whose owner is gone back to the ring;
//   * a feeder that dies without saying so (SIGKILL, an abort inside the runtime) is noticed although it stays a zombie
//     until its parent reaps it: its heartbeat (a thread beside the serve loop stamps CLOCK_MONOTONIC every 20 ms) goes
//     stale, /proc/<pid>/stat says 'Z', or kill(pid, 0) says ESRCH -- whichever a worker sees first;
//   * a feeder that only LOOKED dead (stopped for seconds, then resumed) meets compare-and-swap on both sides: a READY slot
//     goes to the server or back to the ring, never both, and a slot the server holds is disowned, not freed -- its late
//     answer, stamped with the generation the server took, reaches nobody and the slot returns through the reclaim;
//   * wdx_feeder_stop drains: INFLIGHT slots are finished and handed over, READY slots that were never submitted are
//     answered WDX_ERR_NO_DEVICE, and only then does the server leave (server_pid = 0).  A waiting worker gives up on
//     "server gone", never on `stop` alone, and never frees a slot the server may still write to; new claims are
//     refused from `stop` on.
#include "wdx_ctx.h"
#include "wdx_feeder_ring.h"
#include "wdx_window.h"

#include <errno.h>
#include <fcntl.h>
#include <linux/futex.h>
#include <signal.h>
#include <string.h>
#include <sys/syscall.h>
#include <time.h>
#include <unistd.h>

#include <atomic>
#include <thread>

namespace wdx {

constexpr long long kHeartbeatStaleNs = 3000000000ll;   // a serving feeder stamps every 20 ms

static long futex(uint32_t *addr, int op, uint32_t val, const struct timespec *to) {
    return syscall(SYS_futex, addr, op, val, to, nullptr, 0);
}
static void futex_wait_ms(uint32_t *addr, uint32_t val, long ms) {
    struct timespec ts{ms / 1000, (ms % 1000) * 1000000L};
    (void)futex(addr, FUTEX_WAIT, val, &ts);   // (EAGAIN: the word changed already; EINTR / ETIMEDOUT: the caller loops)
}
static void futex_wake_all(uint32_t *addr) { (void)futex(addr, FUTEX_WAKE, 0x7fffffff, nullptr); }
// `seq` / `free_seq`: something changed for whoever sleeps on the word
static void bump_and_wake(uint32_t *seq) {
    __atomic_fetch_add(seq, 1u, __ATOMIC_ACQ_REL);
    futex_wake_all(seq);
}

static long long now_ns() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (long long)ts.tv_sec * 1000000000ll + ts.tv_nsec;
}

// Is process `pid` gone -- exited, or dead and only waiting to be reaped?  kill(pid, 0) keeps answering 0 for a zombie
// (a parent blocked in pool.map never reaps the feeder), so /proc/<pid>/stat's state letter is read as well.
static bool pid_gone(int32_t pid) {
    if (pid <= 0) return true;
    if (kill(pid, 0) != 0 && errno == ESRCH) return true;
    char path[48], buf[256];
    snprintf(path, sizeof(path), "/proc/%d/stat", (int)pid);
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return false;   // (no /proc here, or reaped this instant: kill() says so on the next poll; the heartbeat covers the server)
    const ssize_t n = read(fd, buf, sizeof(buf) - 1);
    close(fd);
    if (n <= 0) return false;
    buf[n] = 0;
    const char *q = strrchr(buf, ')');   // "pid (comm) S ..." -- comm may contain anything, the last ')' ends it
    return q && q[1] == ' ' && (q[2] == 'Z' || q[2] == 'X');
}

static int ring_check(const FeederRing *R) {
    if (!R || R->magic != kFeederMagic || R->n_slots < 1 || R->n_slots > (uint32_t)kMaxRingSlots) {
        set_error("feeder: not an initialised ring (wdx_feeder_ring_init)");
        return WDX_ERR_INVALID;
    }
    return WDX_SUCCESS;
}

// the server is serving (or about to); false once it has left after a stop, or died
static bool server_up(const FeederRing *R) {
    const int32_t pid = __atomic_load_n(&R->server_pid, __ATOMIC_ACQUIRE);
    if (pid <= 0) return false;
    if (pid_gone(pid)) return false;
    const long long hb = __atomic_load_n(&R->heartbeat_ns, __ATOMIC_ACQUIRE);
    return now_ns() - hb < kHeartbeatStaleNs;
}

static int reclaim_dead_owners(FeederRing *R) {
    const int n = ring_reclaim(R, pid_gone);
    if (n) {
        __atomic_fetch_add(&R->reclaimed, (uint64_t)n, __ATOMIC_ACQ_REL);
        bump_and_wake(&R->free_seq);
    }
    return n;
}

// claim a FREE slot for this process; WDX_ERR_NO_DEVICE once the feeder has stopped or died
static int claim_slot(FeederRing *R, int &slot) {
    const int32_t me = (int32_t)getpid();
    int rounds = 0;
    for (;;) {
        if (ld(&R->stop)) {
            set_error("feeder: the feeder has stopped");
            return WDX_ERR_NO_DEVICE;
        }
        const uint32_t seen = ld(&R->free_seq);
        if ((slot = ring_try_claim(R, me)) >= 0) return WDX_SUCCESS;
        // (a server that has not come up yet -- server_pid still 0, no stop -- is waited for: the parent starts it first)
        if (__atomic_load_n(&R->server_pid, __ATOMIC_ACQUIRE) != 0 && !server_up(R)) {
            set_error("feeder: the feeder process died");
            return WDX_ERR_NO_DEVICE;
        }
        if ((++rounds & 3) == 0) (void)reclaim_dead_owners(R);   // the ring is full: is a dead worker sitting on a slot?
        futex_wait_ms(&R->free_seq, seen, 50);
    }
}

static void release_slot(FeederRing *R, int s) {
    slot_release(R->slot[s]);
    bump_and_wake(&R->free_seq);
}

// The serve loop's state: the ring, and the ring slots in flight, oldest first, each on one of the context's
// WDX_MAX_SLOTS submit / wait slots.
struct Server {
    wdx_ctx *ctx;
    FeederRing *R;
    void *ring;
    FeederRefine *X;        // a refine ring: every minibatch goes through wdx_demux_submit_refine / _wait_refine with its rp
    wdx_refine_params rp{};
    struct Fly { uint32_t ring, gen; int cslot; } fifo[WDX_MAX_SLOTS];   // gen: the slot's generation when it was taken
    int head = 0, count = 0;
    bool cbusy[WDX_MAX_SLOTS] = {};

    Server(wdx_ctx *ctx_, void *ring_) : ctx(ctx_), R((FeederRing *)ring_), ring(ring_), X(refine_ext(R)) {
        if (X) {
            rp = X->rp;
            rp.query = X->query;
        }
    }

    // INFLIGHT -> DONE with the minibatch's code (and the message behind it): the owner wakes up
    void hand_over(uint32_t s, uint32_t gen, int rc) {
        FeederSlot &S = R->slot[s];
        S.rc = rc;
        if (rc != WDX_SUCCESS) {
            strncpy(S.err, wdx_last_error(), sizeof(S.err) - 1);
            S.err[sizeof(S.err) - 1] = 0;
        }
        __atomic_fetch_add(&R->served, 1ull, __ATOMIC_ACQ_REL);
        slot_hand_over(S, gen);
        futex_wake_all(&S.state);
    }

    // The classifier tail a minibatch asks for, checked per minibatch: the slot's prob region holds n_classes doubles per
    // read and the fingerprints have n_events columns, so a resident model of another shape must not be run into it.  No
    // model set: the call itself answers WDX_ERR_NO_REFS.
    bool tail_fits(uint32_t want) {
        if (!(want & (WDX_WANT_BOOST | WDX_WANT_SVM))) return true;
        const int kc = R->n_classes, K = R->n_events;
        std::lock_guard<std::mutex> g(ctx->mu);
        if ((want & WDX_WANT_BOOST) && ctx->boost.set && (ctx->boost.dev.k != kc || ctx->boost.dev.n_features != K)) {
            set_error("feeder: the boost model has %d classes and %d features, the ring was laid out for %d and %d", ctx->boost.dev.k,
                      ctx->boost.dev.n_features, kc, K);
            return false;
        }
        // (the SVM's fingerprints are as long as the resident references; a ring without fingerprint regions has no length)
        if ((want & WDX_WANT_SVM) && ctx->svm.set && (ctx->svm.dev.k != kc || (K && ctx->refs.L && ctx->refs.L != K))) {
            set_error("feeder: the SVM model has %d classes and %d-event fingerprints, the ring was laid out for %d and %d",
                      ctx->svm.dev.k, (int)ctx->refs.L, kc, K);
            return false;
        }
        return true;
    }

    // One slot seen READY as `seen`: answered at once (predict mode, a refused minibatch) or put in flight.  False: every
    // context slot is lost to refused waits -- nothing can be submitted.
    bool submit(uint32_t s, uint32_t seen) {
        const SlotView V = slot_view(R, ring, s);
        FeederSlot &S = *V.S;
        uint32_t gen;
        if (!slot_take(S, seen, gen)) return true;   // (its owner gave up first)
        if (!tail_fits(S.want)) {
            hand_over(s, gen, WDX_ERR_INVALID);
            return true;
        }
        if (S.mode == kModePredict) {
            // model.predict on fingerprints the worker holds (models/dtw_svm.py:54-98; Fpt_Boost.predict, models/fpt_boost.py:
            // no DTW, no references): a synchronous call on the context's own stream -- milliseconds, beside the slots in flight
            const double *Xf = (const double *)V.sig;
            hand_over(s, gen, (S.want & WDX_WANT_BOOST) ? wdx_boost_predict(ctx, Xf, S.n_reads, nullptr, V.prob, V.pred, V.conf)
                                                        : wdx_dtw_svm_predict(ctx, Xf, S.n_reads, V.prob, V.pred, V.conf));
            return true;
        }
        int cs = 0;
        while (cs < WDX_MAX_SLOTS && cbusy[cs]) ++cs;
        if (cs == WDX_MAX_SLOTS) {
            if (!slot_untake(S)) hand_over(s, gen, WDX_ERR_NO_DEVICE);   // (disowned meanwhile: nobody reads the answer)
            return false;
        }
        const int64_t nY = R->n_refs;
        const bool int16 = R->sample_format == WDX_FEEDER_SAMPLES_INT16;
        wdx_minibatch_in in{};
        wdx_minibatch_adc_in adc{};
        auto rows = [&](auto &mb) {   // the packed rows, as either kind of minibatch names them
            mb.n_reads = S.n_reads;
            mb.row_off = V.row_off;
            mb.row_len = V.row_len;
            mb.a_start = V.a_start;
            mb.a_end = V.a_end;
            mb.ok = S.has_ok ? V.ok : nullptr;
        };
        if (int16) {
            rows(adc);
            adc.adc = (const int16_t *)V.sig;
            adc.offset = V.offset;
            adc.scale = V.scale;
            adc.row_win = V.row_win;
        } else {
            rows(in);
            in.sig = (const float *)V.sig;
        }
        const int rc = X       ? wdx_demux_submit_refine(ctx, cs, int16 ? nullptr : &in, int16 ? &adc : nullptr, &R->params, &rp, nY, S.want)
                       : int16 ? wdx_demux_submit_adc(ctx, cs, &adc, &R->params, nY, S.want)
                               : wdx_demux_submit_ex(ctx, cs, &in, &R->params, nY, S.want);
        if (rc == WDX_SUCCESS) {
            cbusy[cs] = true;
            fifo[(head + count++) % WDX_MAX_SLOTS] = Fly{s, gen, cs};
        } else {   // (an argument error of this minibatch: its worker gets the code and the message)
            hand_over(s, gen, rc);
        }
        return true;
    }

    int finish_oldest() {
        const Fly f = fifo[head];
        head = (head + 1) % WDX_MAX_SLOTS;
        --count;
        const SlotView V = slot_view(R, ring, f.ring);
        const uint32_t want = V.S->want;
        wdx_minibatch_out out{};
        out.status = V.status;
        out.call = V.call;
        if ((want & WDX_WANT_DIST) && R->n_refs) out.dist = V.dist;
        if (want & WDX_WANT_FPT) out.fpt = V.fpt;
        if (want & WDX_WANT_DWELL) out.dwell = V.dwell;
        if (want & WDX_WANT_STATS) out.stats = V.stats;
        if (want & (WDX_WANT_SVM | WDX_WANT_BOOST)) {
            out.prob = V.prob;
            out.pred = V.pred;
            out.conf = V.conf;
        }
        int32_t *const ridx = (want & WDX_WANT_REFINE_IDX) ? V.ridx : nullptr;
        int rc = wdx_demux_wait_refine(ctx, f.cslot, &out, ridx);
        if (rc == WDX_ERR_INVALID) {
            // by contract the context slot still holds the minibatch: take it out with the two outputs every batch has,
            // and keep the slot marked busy if even that is refused (it is lost to this serve loop, not reused)
            char keep[224];
            strncpy(keep, wdx_last_error(), sizeof(keep) - 1);
            keep[sizeof(keep) - 1] = 0;
            wdx_minibatch_out two{};
            two.status = out.status;
            two.call = out.call;
            if (wdx_demux_wait_refine(ctx, f.cslot, &two, ridx) != WDX_ERR_INVALID) cbusy[f.cslot] = false;
            set_error("%s", keep);
        } else {
            cbusy[f.cslot] = false;
        }
        hand_over(f.ring, f.gen, rc);
        return rc;
    }

    // What is in flight is finished and handed over; what was READY but never submitted is answered, so that no worker
    // sleeps on a slot that will never change.
    void drain() {
        while (count > 0) (void)finish_oldest();
        for (uint32_t s = 0; s < R->n_slots; ++s) {
            const uint32_t v = ld(&R->slot[s].state);
            uint32_t gen;
            if (phase_of(v) == kReady && slot_take(R->slot[s], v, gen)) {
                set_error("feeder: stopped before this minibatch was submitted");
                hand_over(s, gen, WDX_ERR_NO_DEVICE);
            }
        }
    }
};

}  // namespace wdx

using namespace wdx;

extern "C" {

size_t wdx_feeder_ring_bytes(const wdx_feeder_geometry *g) { return ring_bytes(g, false); }
size_t wdx_feeder_ring_bytes_refine(const wdx_feeder_geometry *g) { return ring_bytes(g, true); }

// rp == nullptr: the plain ring, exactly the bytes wdx_feeder_ring_init has always written
static int ring_init(void *mem, size_t bytes, const wdx_feeder_geometry *g, const wdx_seg_params *p, const wdx_refine_params *rp) {
    const size_t need = ring_bytes(g, rp != nullptr);
    if (!mem || !p || need == 0 || bytes < need || ((uintptr_t)mem & 4095u)) {
        set_error("feeder_ring_init: need parameters and a page-aligned block of %zu bytes for this geometry", need);
        return WDX_ERR_INVALID;
    }
    if (g->n_events && g->n_events != p->barcode_num_events) {
        set_error("feeder_ring_init: n_events (%d) must equal barcode_num_events (%d)", (int)g->n_events, (int)p->barcode_num_events);
        return WDX_ERR_INVALID;
    }
    (void)ring_write(mem, g, p, rp);
    return WDX_SUCCESS;
}

int wdx_feeder_ring_init(void *mem, size_t bytes, const wdx_feeder_geometry *g, const wdx_seg_params *p) {
    return ring_init(mem, bytes, g, p, nullptr);
}

int wdx_feeder_ring_init_refine(void *mem, size_t bytes, const wdx_feeder_geometry *g, const wdx_seg_params *p,
                                const wdx_refine_params *rp) {
    if (!rp) {
        set_error("feeder_ring_init_refine: null refinement parameters");
        return WDX_ERR_INVALID;
    }
    // the limits of wdx_fingerprint_refine_batch, with its codes: a ring no minibatch could be served from is refused here
    // (reported behind a null or empty query and ahead of barcode_keep_events, as they always were)
    if (rp->query && rp->n_query >= 1 && (rp->n_query > kRingMaxQuery || (p && p->num_events + 1 > kRingMaxSeries))) {
        set_error("consensus refinement: the query must have 1..%d points and num_events + 1 <= %d", kRingMaxQuery, kRingMaxSeries);
        return WDX_ERR_UNSUPPORTED;
    }
    wdx_seg_params pv;   // K of every minibatch of a refine ring
    if (int e = refine_seg_params("feeder_ring_init_refine", p, rp, &pv, kRefineQuery | kRefineKeep)) return e;
    return ring_init(mem, bytes, g, &pv, rp);
}

int wdx_feeder_stop(void *ring) {
    FeederRing *R = (FeederRing *)ring;
    if (int rc = ring_check(R)) return rc;
    st(&R->stop, 1u);
    bump_and_wake(&R->seq);
    bump_and_wake(&R->free_seq);
    // (workers asleep on their slot keep sleeping: the server hands their minibatch over, or answers it, before it leaves)
    return WDX_SUCCESS;
}

int wdx_feeder_alive(void *ring) {
    FeederRing *R = (FeederRing *)ring;
    if (int rc = ring_check(R)) return rc;
    return (!ld(&R->stop) && server_up(R)) ? 1 : 0;
}

int wdx_feeder_served(void *ring, int64_t *minibatches) { return wdx_feeder_stats(ring, minibatches, nullptr, nullptr); }

int wdx_feeder_stats(void *ring, int64_t *served, int64_t *reclaimed, int32_t *free_slots) {
    FeederRing *R = (FeederRing *)ring;
    if (int rc = ring_check(R)) return rc;
    if (served) *served = (int64_t)__atomic_load_n(&R->served, __ATOMIC_ACQUIRE);
    if (reclaimed) *reclaimed = (int64_t)__atomic_load_n(&R->reclaimed, __ATOMIC_ACQUIRE);
    if (free_slots) {
        int32_t n = 0;
        for (uint32_t s = 0; s < R->n_slots; ++s) n += phase_of(ld(&R->slot[s].state)) == kFree;
        *free_slots = n;
    }
    return WDX_SUCCESS;
}

// Test hooks (no GPU, no context): what == 1 claims a ring slot for the calling process and leaves it FILLING (returns the
// slot index) -- a worker that then dies is what the reclaim logic exists for; what == 2 makes the calling process pose as
// the serving feeder (server_pid + one heartbeat stamp) without serving -- when it dies unreaped, wdx_feeder_alive and the
// workers must notice.  Never on the product path.
int wdx_feeder_selftest(void *ring, int32_t what) {
    FeederRing *R = (FeederRing *)ring;
    if (int rc = ring_check(R)) return rc;
    if (what == 1) {
        int s = -1;
        if (int rc = claim_slot(R, s)) return rc;
        return s;
    }
    if (what == 2) {
        __atomic_store_n(&R->heartbeat_ns, (int64_t)now_ns(), __ATOMIC_RELEASE);
        __atomic_store_n(&R->server_pid, (int32_t)getpid(), __ATOMIC_RELEASE);
        return WDX_SUCCESS;
    }
    set_error("feeder_selftest: unknown hook");
    return WDX_ERR_INVALID;
}

// The GPU-facing process: serves the ring until wdx_feeder_stop.  The resident reference set of `ctx` (wdx_set_refs) is
// what every minibatch is classified against; a resident SVM (wdx_svm_set_model) serves WDX_WANT_SVM / wdx_feeder_predict.
int wdx_feeder_serve(wdx_ctx *ctx, void *ring) {
    FeederRing *R = (FeederRing *)ring;
    if (int rc = check_ctx(ctx)) return rc;
    if (int rc = ring_check(R)) return rc;
    {
        DeviceGuard guard(ctx->device);
        if (guard.rc) return guard.rc;
        // page-lock the data regions: a minibatch is then copied by DMA at the bus rate and wdx_demux_submit returns at once
        hipError_t e = hipHostRegister(ring, (size_t)R->bytes, hipHostRegisterMapped | hipHostRegisterPortable);
        if (e != hipSuccess) {
            set_error("feeder_serve: hipHostRegister of the ring failed: %s", hipGetErrorString(e));
            return WDX_ERR_HIP;
        }
    }
    // sign of life for the workers: independent of the serve loop, which may sit in a stream synchronisation
    std::atomic<bool> beat_on{true};
    __atomic_store_n(&R->heartbeat_ns, (int64_t)now_ns(), __ATOMIC_RELEASE);
    std::thread beat([&]() {
        while (beat_on.load(std::memory_order_acquire)) {
            __atomic_store_n(&R->heartbeat_ns, (int64_t)now_ns(), __ATOMIC_RELEASE);
            struct timespec ts{0, 20000000L};
            nanosleep(&ts, nullptr);
        }
    });
    __atomic_store_n(&R->server_pid, (int32_t)getpid(), __ATOMIC_RELEASE);
    const pid_t parent = getppid();   // (the process that created the ring: when it is gone, nobody will stop us)
    Server sv(ctx, ring);
    int rc_fatal = WDX_SUCCESS;
    uint32_t scan_from = 0;   // (READY slots are taken round-robin: no worker is starved by the slots in front of its own)
    int idle_rounds = 0;
    while (!ld(&R->stop)) {
        if (getppid() != parent) break;   // orphaned: the parent died without wdx_feeder_stop
        const uint32_t seen = ld(&R->seq);
        bool progressed = false;
        for (uint32_t q = 0; q < R->n_slots && sv.count < WDX_MAX_SLOTS; ++q) {
            const uint32_t s = (scan_from + q) % R->n_slots;
            const uint32_t v = ld(&R->slot[s].state);
            if (phase_of(v) != kReady) continue;
            progressed = true;
            scan_from = (s + 1) % R->n_slots;
            if (!sv.submit(s, v)) break;
        }
        if (sv.count > 0) {
            progressed = true;
            if (sv.finish_oldest() == WDX_ERR_HIP) {   // the device is gone: nothing more can be served
                rc_fatal = WDX_ERR_HIP;
                break;
            }
        }
        if (!progressed) {
            if (++idle_rounds >= 25) {   // ~50 ms of idling: look for slots whose worker died
                idle_rounds = 0;
                (void)reclaim_dead_owners(R);
            }
            futex_wait_ms(&R->seq, seen, 2);
        } else if (++idle_rounds >= 2000) {
            idle_rounds = 0;
            (void)reclaim_dead_owners(R);
        }
    }
    // From here on no new claims are accepted.  Drain, then leave (server_pid = 0), which is what the waiting workers
    // give up on.
    st(&R->stop, 1u);
    sv.drain();
    __atomic_store_n(&R->server_pid, 0, __ATOMIC_RELEASE);
    beat_on.store(false, std::memory_order_release);
    beat.join();
    for (uint32_t s = 0; s < R->n_slots; ++s) futex_wake_all(&R->slot[s].state);
    bump_and_wake(&R->free_seq);
    {
        DeviceGuard guard(ctx->device);
        (void)hipHostUnregister(ring);
    }
    if (rc_fatal) set_error("feeder_serve: the device failed while a minibatch was in flight");
    return rc_fatal;
}

}  // extern "C"

namespace wdx {

// A worker's turn with one slot -- no context, NO HIP call: claim, fill(view) and the slot's header, publish, sleep until
// DONE, then take(view) or the server's error, and release.  Gives up when the server is really gone: it has left after a
// stop (its drain answers every slot first), or it died.  A slot the server may still be writing to is never freed here.
template <class Fill, class Take>
static int slot_turn(FeederRing *R, void *ring, uint32_t mode, int64_t n_reads, bool has_ok, uint32_t want, Fill fill, Take take) {
    int s = -1;
    if (int rc = claim_slot(R, s)) return rc;
    const SlotView V = slot_view(R, ring, (uint32_t)s);
    FeederSlot &S = *V.S;
    fill(V);
    S.n_reads = n_reads;
    S.has_ok = has_ok ? 1u : 0u;
    S.want = want;
    S.mode = mode;
    S.rc = WDX_SUCCESS;
    const int32_t me = (int32_t)getpid();
    const uint32_t my_gen = slot_publish(S, me);
    bump_and_wake(&R->seq);
    for (;;) {
        const uint32_t v = ld(&S.state);
        if (phase_of(v) == kDone) break;
        const int32_t pid = __atomic_load_n(&R->server_pid, __ATOMIC_ACQUIRE);
        const bool left = pid == 0 && ld(&R->stop);           // the drain is over and did not answer this slot
        const bool died = pid != 0 && !server_up(R);
        if (left || died) {
            // READY was never picked up: the slot is ours to give back.  One the server holds is disowned -- should the
            // server be alive after all, its answer reaches nobody and the slot returns through the reclaim.
            const GiveUp g = slot_give_up(S, me);
            if (g == kAnswered) break;
            set_error(died ? "feeder: the feeder process died while the minibatch was in its hands"
                           : "feeder: the feeder stopped before the minibatch was served");
            if (g == kGaveBack) bump_and_wake(&R->free_seq);
            return WDX_ERR_NO_DEVICE;
        }
        futex_wait_ms(&S.state, v, 100);
    }
    int rc = S.rc;
    if (S.gen_done != my_gen) {   // (cannot happen while a slot the server holds reaches nobody else; a stale hand-over is not a result)
        set_error("feeder: slot %d was handed over for generation %u, not %u", s, S.gen_done, my_gen);
        rc = WDX_ERR_INVALID;
    } else if (rc == WDX_SUCCESS) {
        take(V);
    } else {
        set_error("feeder: %s", S.err);
    }
    release_slot(R, s);
    return rc;
}

// One minibatch as a worker hands it over: wdx_feeder_job's float32 rows or wdx_feeder_job_adc's int16 rows (is_adc:
// row_len / offset / scale are set); the outputs are the job's.
struct WorkerRows {
    bool is_adc = false;
    const void *samples = nullptr;
    int64_t n_reads = 0, stride = 0;
    const int32_t *row_len = nullptr;
    const float *offset = nullptr, *scale = nullptr;
    const int32_t *a_start = nullptr, *a_end = nullptr;
    const uint8_t *ok = nullptr;
    uint32_t want = 0;
    wdx_minibatch_out out{};
    int32_t *refine_idx = nullptr;   // WDX_WANT_REFINE_IDX (a refine ring)
};

// A worker process: one minibatch through the feeder.  Blocks until the results are there.
static int feeder_run_rows(FeederRing *R, void *ring, const char *who, const WorkerRows &job) {
    const bool is_adc = job.is_adc;
    const int64_t n_reads = job.n_reads, stride = job.stride;
    const uint32_t want = job.want;
    const wdx_minibatch_out &O = job.out;
    if (n_reads < 0 || stride < 0 || (n_reads > 0 && (!job.samples || !job.a_start || !job.a_end || !O.status))) {
        set_error("%s: bad arguments", who);
        return WDX_ERR_INVALID;
    }
    if (is_adc != (R->sample_format == WDX_FEEDER_SAMPLES_INT16)) {
        set_error("%s: %s rows on a ring laid out for %s samples (wdx_feeder_geometry.sample_format)", who,
                  is_adc ? "int16" : "float32", is_adc ? "float32" : "int16");
        return WDX_ERR_INVALID;
    }
    if (is_adc && n_reads > 0) {
        if (!job.row_len) {
            set_error("%s: int16 rows need row_len (there is no NaN tail to find a read's end by)", who);
            return WDX_ERR_INVALID;
        }
        if (!job.offset || !job.scale) {
            set_error("%s: int16 rows need offset and scale of every read", who);
            return WDX_ERR_INVALID;
        }
        for (int64_t r = 0; r < n_reads; ++r)
            if (job.row_len[r] < 0 || (int64_t)job.row_len[r] > stride) {
                set_error("%s: row_len[%lld] = %d is outside 0 .. stride (%lld)", who, (long long)r, (int)job.row_len[r],
                          (long long)stride);
                return WDX_ERR_INVALID;
            }
    }
    if (n_reads > R->max_reads) {
        set_error("%s: %lld reads do not fit the ring's %lld-read slots", who, (long long)n_reads, (long long)R->max_reads);
        return WDX_ERR_INVALID;
    }
    if ((want & WDX_WANT_REFINE_IDX) && R->kind != kRingRefine) {
        set_error("%s: WDX_WANT_REFINE_IDX on a ring without refinement (wdx_feeder_ring_init_refine)", who);
        return WDX_ERR_INVALID;
    }
    if ((want & WDX_WANT_SVM) && (want & WDX_WANT_BOOST)) {
        set_error("%s: WDX_WANT_SVM and WDX_WANT_BOOST share prob / pred / conf: ask for one of them", who);
        return WDX_ERR_INVALID;
    }
    if (R->kind == kRingRefine && R->n_refs == 0 && (want & (WDX_WANT_DIST | WDX_WANT_SVM))) {
        set_error("%s: a fingerprint-only ring (n_refs = 0) serves no distances and no SVM tail", who);
        return WDX_ERR_INVALID;
    }
    constexpr uint32_t kTails = WDX_WANT_SVM | WDX_WANT_BOOST;
    if ((want & ~(WDX_WANT_FPT | WDX_WANT_DIST | WDX_WANT_DWELL | WDX_WANT_STATS | kTails | WDX_WANT_REFINE_IDX)) ||
        ((want & (WDX_WANT_FPT | WDX_WANT_DWELL | WDX_WANT_STATS | WDX_WANT_BOOST)) && R->n_events == 0) ||
        ((want & kTails) && R->n_classes == 0)) {
        set_error("%s: the ring was laid out without room for an output that is asked for (n_events %d, n_classes %d)", who,
                  (int)R->n_events, (int)R->n_classes);
        return WDX_ERR_INVALID;
    }
    if (n_reads > 0 && (((want & WDX_WANT_FPT) && !O.fpt) || ((want & WDX_WANT_DWELL) && !O.dwell) ||
                        ((want & WDX_WANT_STATS) && !O.stats) || ((want & WDX_WANT_DIST) && R->n_refs > 0 && !O.dist) ||
                        ((want & kTails) && (!O.prob || !O.pred || !O.conf)) ||
                        ((want & WDX_WANT_REFINE_IDX) && !job.refine_idx))) {
        set_error("%s: an output that is asked for has no destination", who);
        return WDX_ERR_INVALID;
    }
    if (n_reads == 0) return WDX_SUCCESS;
    // the windows, packed (wdx_window.h): float32 rows from a multiple of 4 samples, int16 rows from a multiple of 8, so
    // that every row starts on a 16-byte boundary; of an int16 row the `valid` samples below the read's row_len are copied
    // -- the rest is the NaN tail the device writes.
    const WindowOpts wo{R->params.padding, is_adc ? 8 : 4, 0};
    auto window = [&](int64_t r) {
        return adapter_window(job.a_start[r], job.a_end[r], stride, job.ok && !job.ok[r], wo, is_adc ? (int64_t)job.row_len[r] : -1);
    };
    PackedOffset fit(wo.align);
    for (int64_t r = 0; r < n_reads; ++r) fit.take(window(r).valid);
    const int64_t need = fit.next;
    if ((uint64_t)need > R->sig_floats * (is_adc ? 2u : 1u)) {
        set_error("%s: the minibatch's adapter windows (%lld samples) do not fit a ring slot (%llu)", who, (long long)need,
                  (unsigned long long)(R->sig_floats * (is_adc ? 2u : 1u)));
        return WDX_ERR_INVALID;
    }
    const size_t n = (size_t)n_reads, nY = (size_t)R->n_refs, K = (size_t)R->n_events, kc = (size_t)R->n_classes;
    auto fill = [&](const SlotView &V) {
        const size_t esz = is_adc ? 2 : 4;
        const unsigned char *src = (const unsigned char *)job.samples;
        PackedOffset pos(wo.align);
        for (int64_t r = 0; r < n_reads; ++r) {
            const Window w = window(r);
            V.row_off[r] = pos.take(w.valid);
            V.row_len[r] = (int32_t)w.valid;
            if (is_adc) V.row_win[r] = (int32_t)w.row;
            V.a_start[r] = w.a_start;
            V.a_end[r] = w.a_end;
            if (w.valid > 0) memcpy(V.sig + (size_t)V.row_off[r] * esz, src + (size_t)(r * stride + w.first) * esz, (size_t)w.valid * esz);
        }
        V.row_off[n_reads] = pos.next;
        if (is_adc) {
            memcpy(V.offset, job.offset, n * 4);
            memcpy(V.scale, job.scale, n * 4);
        }
        if (job.ok) memcpy(V.ok, job.ok, n);
    };
    auto take = [&](const SlotView &V) {
        memcpy(O.status, V.status, n * 4);
        if (O.call) memcpy(O.call, V.call, n * 4);
        if ((want & WDX_WANT_DIST) && nY) memcpy(O.dist, V.dist, n * nY * 4);
        if (want & WDX_WANT_FPT) memcpy(O.fpt, V.fpt, n * K * 8);
        if (want & WDX_WANT_DWELL) memcpy(O.dwell, V.dwell, n * K * 8);
        if (want & WDX_WANT_STATS) memcpy(O.stats, V.stats, n * 48);
        if (want & kTails) {
            memcpy(O.prob, V.prob, n * kc * 8);
            memcpy(O.pred, V.pred, n * 4);
            memcpy(O.conf, V.conf, n * 8);
        }
        if (want & WDX_WANT_REFINE_IDX) memcpy(job.refine_idx, V.ridx, n * 12);
    };
    return slot_turn(R, ring, kModeRows, n_reads, job.ok != nullptr, want, fill, take);
}

// what the two kinds of job differ in; everything behind the samples they share, name for name
static void job_samples(WorkerRows &w, const wdx_feeder_job &job) { w.samples = job.sig; }
static void job_samples(WorkerRows &w, const wdx_feeder_job_adc &job) {
    w.is_adc = true;
    w.samples = job.adc;
    w.row_len = job.row_len;
    w.offset = job.offset;
    w.scale = job.scale;
}
template <class Job>
static int feeder_run_job(void *ring, const char *who, const Job *job, int32_t *refine_idx) {
    FeederRing *R = (FeederRing *)ring;
    if (int rc = ring_check(R)) return rc;
    if (!job) {
        set_error("%s: null job", who);
        return WDX_ERR_INVALID;
    }
    WorkerRows w;
    job_samples(w, *job);
    w.n_reads = job->n_reads;
    w.stride = job->stride;
    w.a_start = job->a_start;
    w.a_end = job->a_end;
    w.ok = job->ok;
    w.want = job->want;
    w.out = wdx_minibatch_out{job->status, job->call, job->dist, job->fpt, job->dwell, job->stats, job->prob, job->pred, job->conf};
    w.refine_idx = refine_idx;
    return feeder_run_rows(R, ring, who, w);
}

}  // namespace wdx

extern "C" {

int wdx_feeder_run(void *ring, const wdx_feeder_job *job) { return feeder_run_job(ring, "feeder_run", job, nullptr); }

// The same for a ring of int16 samples: the raw ADC windows and the reads' offset / scale go into the slot
int wdx_feeder_run_adc(void *ring, const wdx_feeder_job_adc *job) { return feeder_run_job(ring, "feeder_run_adc", job, nullptr); }

// either run call plus the destination of refine_idx (wdx_feeder_job has no room for the pointer)
int wdx_feeder_run_refine(void *ring, const wdx_feeder_job *job, const wdx_feeder_job_adc *job_adc, int32_t *refine_idx) {
    if ((job != nullptr) == (job_adc != nullptr)) {
        set_error("feeder_run_refine: exactly one of job / job_adc must be given");
        return WDX_ERR_INVALID;
    }
    return job ? feeder_run_job(ring, "feeder_run", job, refine_idx) : feeder_run_job(ring, "feeder_run_adc", job_adc, refine_idx);
}

// wdx_demux_batch's arguments and outputs (bit-identical results) through the feeder
int wdx_feeder_demux(void *ring, const float *sig, int64_t n_reads, int64_t stride, const int32_t *a_start,
                     const int32_t *a_end, const uint8_t *ok, int64_t n_refs, float *dist, int32_t *call, int32_t *status) {
    FeederRing *R = (FeederRing *)ring;
    if (int rc = ring_check(R)) return rc;
    if (n_refs != R->n_refs) {
        set_error("feeder_demux: the caller sized `dist` for %lld references but the ring serves %lld", (long long)n_refs,
                  (long long)R->n_refs);
        return WDX_ERR_INVALID;
    }
    if (n_reads > 0 && !call) {
        set_error("feeder_demux: bad arguments");
        return WDX_ERR_INVALID;
    }
    wdx_feeder_job job{};
    job.sig = sig;
    job.n_reads = n_reads;
    job.stride = stride;
    job.a_start = a_start;
    job.a_end = a_end;
    job.ok = ok;
    job.want = dist ? WDX_WANT_DIST : 0u;
    job.status = status;
    job.call = call;
    job.dist = dist;
    return wdx_feeder_run(ring, &job);
}

// model.predict on fingerprints the worker holds: X (n, n_events) float64 -> prob / pred / conf.  tail = WDX_WANT_SVM:
// DTW_SVM.predict (models/dtw_svm.py:54-98); WDX_WANT_BOOST: Fpt_Boost.predict (models/fpt_boost.py)
static int feeder_predict_rows(void *ring, const char *who, uint32_t tail, const double *X, int64_t n, double *prob,
                               int32_t *pred, double *conf) {
    FeederRing *R = (FeederRing *)ring;
    if (int rc = ring_check(R)) return rc;
    if (n < 0 || (n > 0 && (!X || !prob || !pred || !conf))) {
        set_error("%s: bad arguments", who);
        return WDX_ERR_INVALID;
    }
    if (R->n_classes == 0 || R->n_events == 0) {
        set_error("%s: the ring was laid out without a model (n_classes / n_events)", who);
        return WDX_ERR_INVALID;
    }
    const size_t K = (size_t)R->n_events, kc = (size_t)R->n_classes;
    for (int64_t r0 = 0; r0 < n; r0 += R->max_reads) {   // (model.predict takes any number of rows: slot-sized pieces)
        const size_t m = (size_t)(n - r0 < R->max_reads ? n - r0 : R->max_reads);
        auto fill = [&](const SlotView &V) { memcpy(V.sig, X + r0 * (int64_t)K, m * K * 8); };
        auto take = [&](const SlotView &V) {
            memcpy(prob + r0 * (int64_t)kc, V.prob, m * kc * 8);
            memcpy(pred + r0, V.pred, m * 4);
            memcpy(conf + r0, V.conf, m * 8);
        };
        if (int rc = slot_turn(R, ring, kModePredict, (int64_t)m, false, tail, fill, take)) return rc;
    }
    return WDX_SUCCESS;
}

int wdx_feeder_predict(void *ring, const double *X, int64_t n, double *prob, int32_t *pred, double *conf) {
    return feeder_predict_rows(ring, "feeder_predict", WDX_WANT_SVM, X, n, prob, pred, conf);
}

int wdx_feeder_predict_boost(void *ring, const double *X, int64_t n, double *prob, int32_t *pred, double *conf) {
    return feeder_predict_rows(ring, "feeder_predict_boost", WDX_WANT_BOOST, X, n, prob, pred, conf);
}

}  // extern "C"
