// Host driver of the fingerprint stage, included by wdx_fingerprint.hip's own translation unit behind its kernels.  What a call
// launches is decided in wdx_fp_plan.h (plan_fingerprint: host-only, replayed and swept without a GPU); this file holds
//   FpWorkspace        where everything lives in the caller's workspace
//   resolve_fast       from a kernel key of the fast families to its kernel and LdsAttr
//   run_fp_plan        the one loop over the plan's steps: resolve the key, ensure the LDS attribute, build the arguments from
//                      the step's fields, record the step's events, launch slice by slice -- it decides nothing
//   launch_fingerprint validate, plan, run

// ---- workspace ------------------------------------------------------------------------------------------------------
// eight counters | one ClipRec per read | six read lists (slow, big0, big1, retry, big2, back: FpCounter, wdx_fp_plan.h)
// | the split main kernel's peak lists for one launch slice (kSplitRecBytes per read, 16-byte aligned)
// | 16 diagnostic counters (WDX_OPT_DEBUG_OCCUPANCY: why reads were handed to the exact kernel) at the very end -- in the
// caller's workspace, i.e. per context and per call, ordered by the call's stream
static_assert(sizeof(ClipRec) == kWorkClipRecBytes && kSplitRecBytes == kWorkSplitRecBytes, "workspace layout: wdx_work_layout.h");
struct FpWorkspace {
    unsigned *count;        // kFpCounters
    ClipRec *clip;          // one per read
    int32_t *slow, *big0, *big1, *retry, *big2, *back;   // n_reads entries each, counted by count[kCntSlow .. kCntBack]
    unsigned char *split;   // kSplitRecBytes x min(n_reads, kSplitSlice)
    unsigned *dbg;          // 16
    int64_t bytes;
    FpWorkspace(void *d_ws, int64_t n_reads) {   // pointers on the pieces of fp_work_layout (wdx_work_layout.h)
        const FpWorkLayout W = fp_work_layout(n_reads);
        const uintptr_t b = reinterpret_cast<uintptr_t>(d_ws);
        count = reinterpret_cast<unsigned *>(b + (uintptr_t)W.count);
        clip = reinterpret_cast<ClipRec *>(b + (uintptr_t)W.clip);
        int32_t **const lists[kWorkLists] = {&slow, &big0, &big1, &retry, &big2, &back};
        for (int i = 0; i < kWorkLists; ++i) *lists[i] = reinterpret_cast<int32_t *>(b + (uintptr_t)W.list[i]);
        split = reinterpret_cast<unsigned char *>(b + (uintptr_t)W.split);
        dbg = reinterpret_cast<unsigned *>(b + (uintptr_t)W.dbg);
        bytes = W.bytes;
    }
    int32_t *list(int c) const {   // (kNoList: null)
        int32_t *const l[6] = {slow, big0, big1, retry, big2, back};
        return c == kNoList ? nullptr : l[c];
    }
    unsigned *counter(int c) const { return c == kNoList ? nullptr : count + c; }
};
int64_t fingerprint_workspace_bytes(int64_t n_reads) { return fingerprint_workspace_size(n_reads); }

// ---- kernels --------------------------------------------------------------------------------------------------------
// (which (width, NBT) pairs exist and what each has: fp_width_class, fp_key_exists)
static FpKernel resolve_fast(const FpKernelKey &k) {
    if (k.nbt == 1) return k.fw == kFW ? resolve_fast_width<kFW, 1>(k) : resolve_fast_width<18, 1>(k);
    switch (k.fw) {
        case 30: return resolve_fast_width<30, 2>(k);
        case 6: return resolve_fast_width<6, 2>(k);
        case 24: return resolve_fast_width<24, 2>(k);
        case 36: return resolve_fast_width<36, 2>(k);
        case 12: return resolve_fast_width<12, 2>(k);
        case 18: return resolve_fast_width<18, 2>(k);
        default: break;   // the exact-scores-only widths: instantiated in wdx_fingerprint_w1.hip .. _w4.hip
    }
    for (FpKernel (*unit)(const FpKernelKey &) : {resolve_fast_w1, resolve_fast_w2, resolve_fast_w3, resolve_fast_w4})
        if (const FpKernel kern = unit(k); kern.fn) return kern;
    return {};
}

template <int BLOCK>
static int launch_exact_list(const FpStep &s, const FpArgs &A, hipStream_t stream, const unsigned *count, const int32_t *list) {
    return launch_exact<fingerprint_list_kernel<BLOCK>>(s, A, 0, stream, nullptr, count, list);   // (a fixed grid: one launch)
}
template <int BLOCK, bool PROF>
static int launch_exact_chunks(const FpStep &s, const FpArgs &A, int64_t max_launch_slice, hipStream_t stream, int64_t *n_launches) {
    return launch_exact<fingerprint_kernel<BLOCK, PROF>>(s, A, max_launch_slice, stream, n_launches);
}
// count / list: the read list the step takes (null: every read of the call); d_long: fingerprint_long_kernel's slots
static int launch_exact_step(const FpStep &s, FpArgs A, const unsigned *count, const int32_t *list, void *d_long, int64_t max_launch_slice,
                             hipStream_t stream, int64_t *n_launches) {
    const bool small = s.key.block == 512;
    switch (s.key.family) {
        case kFamLong: case kFamBig:
            return launch_big_long_step(s, A, count, list, d_long, stream);
        case kFamExactList:
            return small ? launch_exact_list<512>(s, A, stream, count, list) : launch_exact_list<1024>(s, A, stream, count, list);
        case kFamExactChunks:
            if (s.key.prof) return small ? launch_exact_chunks<512, true>(s, A, max_launch_slice, stream, n_launches) : launch_exact_chunks<1024, true>(s, A, max_launch_slice, stream, n_launches);
            return small ? launch_exact_chunks<512, false>(s, A, max_launch_slice, stream, n_launches) : launch_exact_chunks<1024, false>(s, A, max_launch_slice, stream, n_launches);
        default:
            set_error("launch_exact_step: not an exact family");
            return WDX_ERR_INVALID;
    }
}

// ---- run ------------------------------------------------------------------------------------------------------------
// What every step of one call sees.
struct FpRun {
    FpArgs A;
    const FpPlan &pl;
    FpWorkspace ws;
    hipStream_t stream;
    int64_t *n_launches;   // nullable
    MainEvents *ev;        // nullable
    void *d_long;          // fingerprint_long_kernel's slots (pl.with_long)
    void *d_opt;           // WDX_OPT_REFINE_OPTIMAL_CPTS: the scratch of plan_refine_optimal(n_reads, max_len, E2)
    int64_t max_len, max_launch_slice;
};
// a pair from the context's pool (take is set whenever the context times its kernels); first == null: none
static std::pair<hipEvent_t, hipEvent_t> take_event_pair(MainEvents *ev, bool wanted) {
    if (wanted && ev && ev->take) return ev->take(ev->take_arg);
    return {nullptr, nullptr};
}
// A step of the fast families: the arguments from the step's fields.  A tile step launches its tail (the next step) behind
// each of its slices: slot = workgroup of the slice.
static int run_fast_step(const FpRun &R, const FpStep &s, const FpStep *tail) {
    const FpKernel kern = resolve_fast(s.key), ktail = tail ? resolve_fast(tail->key) : FpKernel{};
    if (!kern.fn || (tail && !ktail.fn)) {
        set_error("no fast kernels for running_stat_width %d", s.key.fw);
        return WDX_ERR_INVALID;
    }
    if (int rc = kern.attr->ensure(kern.fn, s.lds)) return rc;
    FastArgs F{};
    F.a = R.A;
    F.a.exact_scores = s.exact_scores ? 1 : 0;
    F.capF = s.capF;
    F.capP = s.capP;
    F.slow_count = R.ws.count + kCntSlow;
    F.slow_list = R.ws.slow;
    F.in_count = R.ws.counter(s.in), F.in_list = R.ws.list(s.in), F.in_start = (unsigned)s.in_start;
    F.big_count = R.ws.counter(s.over), F.big_list = R.ws.list(s.over);
    F.retry_count = R.ws.counter(s.retry), F.retry_list = R.ws.list(s.retry);
    F.clip = s.clip ? R.ws.clip : nullptr;
    F.routed = s.routed ? 1 : 0;
    if (tail) F.split_ws = R.ws.split;
    const FpSlices S = fp_slices(s.extent, s.rule, s.slice_limit, R.max_launch_slice);
    for (int64_t i = 0; i < S.count; ++i) {
        const int64_t base = S.base(i) * s.per_wg, n = S.n(i);
        F.a.block_base = base;
        if (tail) F.split_base = base, F.split_n = n;
        hipLaunchKernelGGL(kern.fn, dim3((unsigned)n), dim3(s.wg), s.lds, R.stream, F);
        if (s.counted && R.n_launches) ++*R.n_launches;
        if (!tail) continue;
        // (an event pair around each tail launch of the main pair, from the context's pool)
        const std::pair<hipEvent_t, hipEvent_t> tp = take_event_pair(R.ev, tail->ev == kEvMain && R.ev && R.ev->first);
        if (tp.first) (void)hipEventRecord(tp.first, R.stream);
        F.a.block_base = 0;
        hipLaunchKernelGGL(ktail.fn, dim3((unsigned)((n + tail->per_wg - 1) / tail->per_wg)), dim3(tail->wg), tail->lds, R.stream, F);
        if (tp.first) {
            (void)hipEventRecord(tp.second, R.stream);
            R.ev->tail.push_back(tp);
        }
    }
    return WDX_SUCCESS;
}
static int run_clip_block_step(const FpRun &R, const FpStep &s) {
    if (int rc = lds_attr_of<clip_bounds_block_kernel>().ensure(clip_bounds_block_kernel, s.lds)) return rc;
    ClipBlockArgs CB{R.A, R.ws.clip, R.ws.counter(s.in), R.ws.list(s.in), s.capF};
    CB.a.exact_scores = s.exact_scores ? 1 : 0;
    const FpSlices S = fp_slices(s.extent, s.rule, s.slice_limit, R.max_launch_slice);
    for (int64_t i = 0; i < S.count; ++i) {
        CB.a.block_base = S.base(i);
        hipLaunchKernelGGL(clip_bounds_block_kernel, dim3((unsigned)S.n(i)), dim3(s.wg), s.lds, R.stream, CB);
    }
    return WDX_SUCCESS;
}
// every read of the call has left a record: the subsequence match for all of them, slice by slice, then the optimal change-points
static int run_refine_optimal_step(const FpRun &R, const FpStep &s, FpArgs A) {
    const FpSlices S = fp_slices(s.extent, s.rule, s.slice_limit, R.max_launch_slice);
    for (int64_t i = 0; i < S.count; ++i) {
        A.block_base = S.base(i);
        if (int rc = launch_refine_match_wave(A, S.n(i), R.stream)) return rc;
    }
    const std::pair<hipEvent_t, hipEvent_t> tp = take_event_pair(R.ev, s.ev == kEvOptimal);
    if (tp.first) (void)hipEventRecord(tp.first, R.stream);
    const int rc = launch_refine_optimal(A, plan_refine_optimal(A.n_reads, R.max_len, A.rf.E2), R.d_opt, R.stream);
    if (tp.first) {
        (void)hipEventRecord(tp.second, R.stream);
        R.ev->optimal.push_back(tp);
    }
    return rc;
}
// the first / second events of MainEvents that bracket the steps of a slot
static void record_slot_event(const FpRun &R, FpEventSlot slot, bool closing) {
    MainEvents *ev = R.ev;
    if (!ev) return;
    if (slot == kEvClip && ev->c_first) {
        (void)hipEventRecord(closing ? ev->c_second : ev->c_first, R.stream);
        if (closing) ev->c_recorded = true;
    }
    if (slot == kEvMain && ev->first) {
        (void)hipEventRecord(closing ? ev->second : ev->first, R.stream);
        if (closing) ev->recorded = true;
    }
}

// WDX_OPT_DEBUG_OCCUPANCY: where the reads went (synchronises)
static int print_chain_counters(const FpRun &R) {
    const FpWorkspace &ws = R.ws;
    hipStream_t stream = R.stream;
    unsigned c[kFpCounters] = {};
    WDX_HIP_TRY(hipMemcpyAsync(c, ws.count, sizeof(c), hipMemcpyDeviceToHost, stream));
    WDX_HIP_TRY(hipStreamSynchronize(stream));
    // (kCntBig1 is the 8192-sample list when the streaming kernel is not in the chain, else the streaming kernel's
    // own exact-scores retry list)
    fprintf(stderr, "[wdx] of %lld reads: %u beyond the main instantiation, %u %s, %u to the "
                    "streaming kernel, %u redone with exact scores, %u on the exact general kernel\n", (long long)R.A.n_reads,
            c[kCntBig0], c[kCntBig1], R.pl.with_stream ? "redone by the streaming kernel on exact scores" : "to the 8192-sample list kernel",
            c[kCntBig2], c[kCntRetry], c[kCntSlow]);
    unsigned h[16];
    WDX_HIP_TRY(hipMemcpyAsync(h, ws.dbg, 64, hipMemcpyDeviceToHost, stream));
    WDX_HIP_TRY(hipStreamSynchronize(stream));
    fprintf(stderr, "[wdx] handed to the exact kernel by the fast kernels, by reason (0 parameter gate / window, 1 NaN or negative, "
                    "2 sums not provably exact, 3 plateau or peak-list capacity, 4 neighbourhood, 5 kept-list capacity, 6 tie at the "
                    "top-E cut, 7 doubt without a retry list, 8 fewer peaks than events with accept_less_cpts):");
    for (int i = 0; i < 10; ++i) fprintf(stderr, " %u", h[i]);
    fprintf(stderr, "\n");
    if (R.pl.refine)
        fprintf(stderr, "[wdx] refinement: %u reads back from the tail kernel to the exact kernel (%u for a run of equal scores across a "
                        "tile's end, %u beyond the peak list)\n", c[kCntBack], c[kCntBackTie], c[kCntBackList]);
    if (R.pl.ext) {
        std::vector<ClipRec> rec((size_t)R.A.n_reads);
        WDX_HIP_TRY(hipMemcpy(rec.data(), ws.clip, sizeof(ClipRec) * rec.size(), hipMemcpyDeviceToHost));
        long long f[4] = {0, 0, 0, 0};
        for (const ClipRec &cr : rec) ++f[cr.flag & 3];
        fprintf(stderr, "[wdx] clip_bounds_kernel flags: %lld not taken, %lld ok, %lld NaN / negative, %lld sums not "
                        "provably exact\n", f[0], f[1], f[2], f[3]);
    }
    return WDX_SUCCESS;
}

static int run_fp_plan(FpRun &R, const Knobs &knobs) {
    const FpPlan &pl = R.pl;
    if (pl.path == FpPlan::kChain) {
        WDX_HIP_TRY(hipMemsetAsync(R.ws.count, 0, kFpCounters * 4, R.stream));
        R.A.peak_filter = knobs.no_peak_filter ? 0 : 1;   // (only the approximate-keys launches look at it)
        if (knobs.debug_occ) {   // (diagnostic: 16 counters at the end of this call's workspace, zeroed on its stream)
            WDX_HIP_TRY(hipMemsetAsync(R.ws.dbg, 0, 64, R.stream));
            R.A.dbg_reasons = R.ws.dbg;
        }
    }
    FpEventSlot open = kEvNone;
    bool fast_done = false;   // (the fast families' launches are checked once, behind the last of them)
    for (int i = 0; i < pl.n_steps; ++i) {
        const FpStep &s = pl.steps[i];
        const FpEventSlot slot = s.ev == kEvOptimal ? kEvNone : s.ev;
        if (slot != open) {
            record_slot_event(R, open, true);
            record_slot_event(R, slot, false);
            open = slot;
        }
        FpArgs A = R.A;   // what the clip, exact and refinement families take (the fast ones: run_fast_step)
        A.exact_scores = s.exact_scores ? 1 : 0;
        A.clip = s.clip ? R.ws.clip : nullptr;
        A.refine_record = s.refine_record ? 1 : 0;
        int rc = WDX_SUCCESS;
        switch (s.key.family) {
            case kFamFastMain:
                if (knobs.debug_occ) {   // (the one-piece kernel's occupancy, whichever form runs)
                    FpKernelKey whole = s.key;
                    whole.split = false;
                    const FpKernel km = resolve_fast(whole);
                    int nb = 0;
                    if (km.fn && km.attr->ensure(km.fn, s.lds) == WDX_SUCCESS)
                        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)km.fn, FB, s.lds);
                    fprintf(stderr, "[wdx] fast kernel capF=%d capP=%d lds=%zu B -> %d workgroups/CU%s\n", s.capF, s.capP, s.lds, nb,
                            pl.approx ? ", approximate score keys" : "");
                }
                [[fallthrough]];
            case kFamList1:
                rc = run_fast_step(R, s, s.split_tile ? &pl.steps[i + 1] : nullptr);
                if (s.split_tile) ++i;
                break;
            case kFamListStride: case kFamStream:
                rc = run_fast_step(R, s, nullptr);
                break;
            case kFamSplitTail:
                set_error("fingerprint plan: a tail step without its tile");
                return WDX_ERR_INVALID;
            case kFamClip: case kFamClipList:
                rc = launch_clip_step(s, A, R.ws.clip, R.ws.counter(s.in), R.ws.list(s.in), R.max_launch_slice, R.stream);
                break;
            case kFamRoute:
                rc = launch_clip_step(s, A, R.ws.clip, R.ws.counter(s.over), R.ws.list(s.over), R.max_launch_slice, R.stream);
                break;
            case kFamClipBlock:
                rc = run_clip_block_step(R, s);
                break;
            default:   // the exact and refinement families: behind the fast ones
                if (pl.path == FpPlan::kChain && !fast_done) {
                    WDX_HIP_TRY(hipGetLastError());
                    fast_done = true;
                }
                if (s.key.family == kFamRefineTail)
                    rc = launch_refine_tail(A, R.ws.counter(s.over), R.ws.list(s.over), R.stream);
                else if (s.key.family == kFamRefineOptimal)
                    rc = run_refine_optimal_step(R, s, A);
                else
                    rc = launch_exact_step(s, A, R.ws.counter(s.in), R.ws.list(s.in), R.d_long, R.max_launch_slice, R.stream, R.n_launches);
        }
        if (rc) return rc;
    }
    record_slot_event(R, open, true);
    if (pl.path != FpPlan::kChain) return WDX_SUCCESS;
    if (!fast_done) {   // (ablation timing of the main kernel: no step behind it, the lists are left unprocessed)
        WDX_HIP_TRY(hipGetLastError());
        return WDX_SUCCESS;
    }
    return knobs.debug_occ ? print_chain_counters(R) : WDX_SUCCESS;
}

// ---- entry ----------------------------------------------------------------------------------------------------------
int launch_fingerprint(const FpReads &in, const wdx_seg_params &p, const FpOut &out, hipStream_t stream, void *d_ws,
                       const Knobs &knobs, int64_t *n_launches, long long *d_prof, int64_t prof_reads, int stop_phase,
                       const RefineDev *rf, MainEvents *main_ev, double *d_big, void *d_long, void *d_opt) {
    if (in.n_reads == 0) return WDX_SUCCESS;
    const FpSwitches sw = knobs.fp_switches();
    const PlanFlags flags{d_ws != nullptr, d_prof != nullptr, stop_phase, d_big != nullptr, d_long != nullptr, rf != nullptr, rf && rf->ws};
    const FpRefineView view{rf && rf->query, rf ? rf->nq : 0, rf ? rf->E2 : 0, rf ? rf->psi1b : 0, rf ? rf->psi2b : 0};
    FpCheck ok = check_fingerprint_call(in.n_reads, p, rf ? &view : nullptr, flags, sw);
    if (ok.code == WDX_SUCCESS) {
        LaunchSliceScope slice_scope(knobs.max_launch_slice);
        const FpPlan pl = plan_fingerprint(p, in.max_len, in.n_reads, sw, flags);
        if (pl.refused.code == WDX_SUCCESS) {
            (void)hipGetLastError();  // do not inherit a stale error from an earlier failed call
            FpRun R{FpArgs{in.sig, in.row_off, in.row_len, in.stride, in.n_reads, in.a_start, in.a_end, in.ok, p, out.fpt, out.dwell, out.stats,
                           out.status, pl.cap, 0, d_prof, prof_reads, stop_phase, 1, rf ? *rf : RefineDev{}, d_big,
                           pl.with_long ? kLongCap : (pl.with_huge ? kBigCap : 0), knobs.exact_no_list ? 1 : 0},
                    pl, FpWorkspace(d_ws, in.n_reads), stream, n_launches, main_ev, d_long, d_opt, in.max_len, knobs.max_launch_slice};
            R.A.refine_optimal = rf && knobs.refine_optimal ? 1 : 0;
            const uint64_t e1 = (uint64_t)(p.num_events > 0 ? p.num_events : 1);
            R.A.e_magic1 = (unsigned)std::min<uint64_t>(((1ull << 32) + e1 - 1) / e1, 0xffffffffull);   // (E = 1: 2^32 - 1 -> q = n - 1, rounded up to n)
            R.A.e_magic2 = (unsigned)(((1ull << 32) + 2 * e1 - 1) / (2 * e1));
            return run_fp_plan(R, knobs);
        }
        ok = pl.refused;
    }
    set_error("%s", ok.msg);
    return ok.code;
}
