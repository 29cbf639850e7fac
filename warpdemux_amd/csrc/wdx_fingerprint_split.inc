// ---- the tail of the SPLIT main kernel -----------------------------------------------------------------------------
// fingerprint_split_tail_kernel: one WAVE per read, everything that follows the tile pass of the fast body -- greedy
// distance suppression (find_peaks' distance rule, sig_proc.py:176-198 -> scipy.signal.find_peaks), the E highest kept
// peaks, the boundaries, the event means (_c_segmentation.pyx:41-53), normalisation and the last K events
// (sig_proc.py:546-589) -- from the <= 256 peaks the main kernel exported (SplitHdr, wdx_fingerprint_fast.inc).
//
// In the one-kernel form these stages are one wave's work while the workgroup's other three waves wait at a barrier and
// its 26.8 KB of LDS hold a read that no longer needs them (16 k of a workgroup's 42 k cycles: the kernel ran at six reads
// per CU x 42 k cycles, VALU-busy 0.68).  Here a wave needs 4.4 KB of LDS and no barrier at all: one read per (one-wave) workgroup,
// as many workgroups per CU as the registers allow, and no sample is read -- an event's sum is the difference of two of
// the exported prefix sums (every partial sum of the clipped samples is exactly representable: the clip record's gate).
//
// Same decisions, same arithmetic as fast_body's one-wave P3b..P5 + P6 + P7 (the code below is that code: a lane owns four
// consecutive list entries, the neighbours' four come by DPP wave shifts instead of an LDS gather):
//   outcome 0 fingerprint written | 1 an order decision inside the error band, or a cut that does not clear kPeakTauLo ->
//   the exact-scores launch | 2 fewer than E kept peaks -> status 3 (or the exact kernel under accept_less_cpts) | 3 -- |
//   4 the cut does not lie certainly above kPeakTauHi -> the 6144-sample list kernel (its workgroup-wide form on the whole
//   list)
// (one wave per workgroup: a finished wave's slot and LDS go to the next read at once -- with four reads per workgroup they
// waited for the slowest of the four: main pair 96.2 -> 95.4 ms per 10 M reads)
// (kSplitWaves = 1: wdx_fp_plan.h, where the plan sizes the tail kernel's grid by it)
struct alignas(8) SplitWaveLds {
    int cpts[kFSeg + 4];
    double pb[kFSeg + 2];   // P at the boundaries
    double ev[kFSeg];
    double tmp[kFSeg];
    unsigned wl[64];
    unsigned long long wlist[64];
};

template <int FW, int NBT = 1>
__global__ __launch_bounds__(kSplitWaves * 64) void fingerprint_split_tail_kernel(FastArgs F) {
    __shared__ SplitWaveLds lds_all[kSplitWaves];
    // NBT = neighbour LANES per side the suppression looks at (a lane owns 4 peaks, peaks are >= 2 apart: 4 NBT neighbours
    // per side cover d_eff <= 8 NBT + 1), as in fast_body
    static_assert(NBT == 1 || NBT == 2, "suppression reach");
    constexpr int kPad = 4 * NBT, kNBW = 4 * NBT, WNs = 4 + 2 * kPad;
    const FpArgs &A = F.a;
    const wdx_seg_params &P = A.p;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t q = A.block_base + (int64_t)blockIdx.x * kSplitWaves + wave;
    if (q >= F.split_n) return;
    // main kernel's slice: read = split_base + q; list kernel's slice: entry split_base + q of the list (if it exists)
    if (F.in_list && F.split_base + q >= (int64_t)*F.in_count) return;
    const int64_t r = F.in_list ? (int64_t)F.in_list[F.split_base + q] : F.split_base + q;
    const unsigned char *rec = F.split_ws + (size_t)q * kSplitRecBytes;
    // the lane's four entries are requested before the header is looked at (one memory latency, not two; the addresses are
    // inside the record whatever it holds)
    const int k0 = 4 * lane;
    const double *gk = reinterpret_cast<const double *>(rec + 16);
    const double *gp = reinterpret_cast<const double *>(rec + 16 + 8 * kSplitMax);
    const unsigned short *gpos = reinterpret_cast<const unsigned short *>(rec + 16 + 16 * kSplitMax);
    const double2 ka = reinterpret_cast<const double2 *>(gk + k0)[0], kb = reinterpret_cast<const double2 *>(gk + k0)[1];
    const double2 pa = reinterpret_cast<const double2 *>(gp + k0)[0], pb = reinterpret_cast<const double2 *>(gp + k0)[1];
    const uint2 p4 = *reinterpret_cast<const uint2 *>(gpos + k0);
    const SplitHdr hdr = *reinterpret_cast<const SplitHdr *>(rec);
    if (hdr.m < 0) return;   // (wave-uniform) nothing exported: the read failed or is on one of the lists
    SplitWaveLds &L = lds_all[wave];
    // diagnostic runs (wdx_fingerprint_profile_dev, fast_path = 2): shader-clock stamps in slots 6 .. 9 of the read's row
    // (6 entries loaded, 7 boundaries written, 8 event means + mean / sd, 9 end); the tile kernel owns slots 0 .. 5
    long long *pp = (A.prof && r < A.prof_reads) ? A.prof + r * 32 : nullptr;
    auto stamp = [&](int k) __attribute__((always_inline)) {
        if (pp) {
            const long long t = (long long)__builtin_amdgcn_s_memtime();
            if (lane == 0) pp[k] = t;
        }
    };
    const int M = hdr.m & 0xffff, n = hdr.n;
    const bool cut_hi = (hdr.m & kSplitCutHi) != 0;
    const int K = P.barcode_num_events, E = P.num_events;
    int d_eff = rdiv_half_even((unsigned)n, 2u * (unsigned)E, A.e_magic2);   // (int)rint((double)n / (double)E / 2.0)
    if (P.min_obs_per_base < d_eff) d_eff = P.min_obs_per_base;
    auto wfence = []() __attribute__((always_inline)) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    auto karg = [&]() {
        return (const volatile FastArgs __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr();
    };
    auto push = [&](unsigned *cnt, int32_t *lst) {
        if (lane == 0) lst[atomicAdd(cnt, 1u)] = (int32_t)r;
    };
    auto to_slow = [&](int reason) {
        push(karg()->slow_count, karg()->slow_list);
        if (lane == 0)
            if (unsigned *h = karg()->a.dbg_reasons) atomicAdd(h + (reason & 15), 1u);
    };
    auto to_retry = [&]() {
        if (karg()->retry_list) push(karg()->retry_count, karg()->retry_list);
        else to_slow(7);
    };
    auto to_big = [&]() {
        if (karg()->big_list) push(karg()->big_count, karg()->big_list);
        else to_retry();
    };
    auto fail = [&](int st) {
        for (int i = lane; i < K; i += 64) {
            if (A.fpt) A.fpt[r * K + i] = __builtin_nan("");
            if (A.dwell) A.dwell[r * K + i] = 0;
        }
        if (A.stats && lane < 6) A.stats[r * 6 + lane] = __builtin_nan("");
        if (lane == 0) A.status[r] = st;
    };

    // the lane's four entries, and the four on either side from the lanes next door
    double ws[WNs], pq[4];
    int wp[WNs];
    {
        const double kown[4] = {ka.x, ka.y, kb.x, kb.y};
        const int pown[4] = {(int)(p4.x & 0xffffu), (int)(p4.x >> 16), (int)(p4.y & 0xffffu), (int)(p4.y >> 16)};
        pq[0] = pa.x; pq[1] = pa.y; pq[2] = pb.x; pq[3] = pb.y;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = k0 + j < M;
            ws[kPad + j] = in ? kown[j] : -__builtin_inf();   // (never outranks, never inside a band)
            wp[kPad + j] = in ? pown[j] : 0;
        }
        auto from_below = [](unsigned x) __attribute__((always_inline)) {   // wave_shr:1 -- lane l reads lane l - 1, lane 0 reads zero
            return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x138, 0xf, 0xf, true);
        };
        auto from_above = [](unsigned x) __attribute__((always_inline)) {   // wave_shl:1 -- lane l reads lane l + 1, lane 63 reads zero
            return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x130, 0xf, 0xf, true);
        };
        // lanes at distance 2 (NBT = 2): by ds_bpermute -- LDS-pipe instructions, this kernel is bound by its VALU count
        const int a_dn2 = (lane >= 2 ? lane - 2 : lane) << 2, a_up2 = (lane < 62 ? lane + 2 : lane) << 2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned long long b = (unsigned long long)__double_as_longlong(ws[kPad + j]);
            const unsigned long long lft = ((unsigned long long)from_below((unsigned)(b >> 32)) << 32) | from_below((unsigned)b);
            const unsigned long long rgt = ((unsigned long long)from_above((unsigned)(b >> 32)) << 32) | from_above((unsigned)b);
            // (the wave's ends: no entry there -- the one-kernel form's index test `f >= 0 && f < M`)
            ws[kPad - 4 + j] = lane > 0 ? __longlong_as_double((long long)lft) : -__builtin_inf();
            ws[kPad + 4 + j] = lane < 63 ? __longlong_as_double((long long)rgt) : -__builtin_inf();
            wp[kPad - 4 + j] = (int)from_below((unsigned)wp[kPad + j]);
            wp[kPad + 4 + j] = (int)from_above((unsigned)wp[kPad + j]);
            if constexpr (NBT == 2) {
                const unsigned long long l2 = ((unsigned long long)(unsigned)__builtin_amdgcn_ds_bpermute(a_dn2, (int)(unsigned)(b >> 32)) << 32) |
                                              (unsigned)__builtin_amdgcn_ds_bpermute(a_dn2, (int)(unsigned)b);
                const unsigned long long r2 = ((unsigned long long)(unsigned)__builtin_amdgcn_ds_bpermute(a_up2, (int)(unsigned)(b >> 32)) << 32) |
                                              (unsigned)__builtin_amdgcn_ds_bpermute(a_up2, (int)(unsigned)b);
                const int pl2 = __builtin_amdgcn_ds_bpermute(a_dn2, wp[kPad + j]), pr2 = __builtin_amdgcn_ds_bpermute(a_up2, wp[kPad + j]);
                ws[j] = lane > 1 ? __longlong_as_double((long long)l2) : -__builtin_inf();
                ws[kPad + 8 + j] = lane < 62 ? __longlong_as_double((long long)r2) : -__builtin_inf();
                wp[j] = lane > 1 ? pl2 : 0;
                wp[kPad + 8 + j] = lane < 62 ? pr2 : 0;
            }
        }
    }
    stamp(6);
    const double tau_v = cut_hi ? kPeakTauHi : kPeakTauLo;   // the cut the selection must clear
    const double tau_vhi = __builtin_fma(tau_v, kBandHi, kBandAbs);
    const unsigned not_clear = cut_hi ? 4u : 1u;              // ... and where a read goes that does not
    unsigned outcome = 0;
    const int nb = min(kNBW, (d_eff - 1) / 2);
    bool dbt = false;
    unsigned mk[4] = {0, 0, 0, 0};
    unsigned und = 0, kept0 = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (k0 + j < M) {
            const int pk = wp[kPad + j];
            const double sk = ws[kPad + j];
            const double sk_hi = __builtin_fma(sk, kBandHi, kBandAbs);
            const double sk_lo = (sk - kBandAbs) * kBandLo;
#pragma unroll
            for (int o = 1; o <= kNBW; ++o) {
                if (o > nb) break;  // wave-uniform
                const bool inl = pk - wp[kPad + j - o] < d_eff;
                const bool inr = wp[kPad + j + o] - pk < d_eff;
                const bool outl = ws[kPad + j - o] > sk_hi, outr = ws[kPad + j + o] >= sk_hi;
                if (inl && outl) mk[j] |= 1u << (kPad + j - o);
                if (inr && outr) mk[j] |= 1u << (kPad + j + o);
                dbt |= inl && !outl && ws[kPad + j - o] >= sk_lo;
                dbt |= inr && !outr && ws[kPad + j + o] >= sk_lo;
            }
            if (mk[j] == 0u) kept0 |= 1u << j;
            else und |= 1u << j;
        }
    }
    // the relaxation (monotone: any schedule reaches the same fixed point), neighbours' bytes by DPP wave shifts
    unsigned bC = kept0 | (und << 4);
    for (;;) {
        unsigned keptW = (bC & 15u) << kPad, undW = (bC >> 4) << kPad;
#pragma unroll
        for (int q = 1; q <= NBT; ++q) {
            // (DPP wave shifts, one per lane of distance; a lane without a source reads zero -- exactly the edge rule)
            unsigned bL = bC, bR = bC;
#pragma unroll
            for (int z = 0; z < q; ++z) {
                bL = (unsigned)__builtin_amdgcn_update_dpp(0, (int)bL, 0x138, 0xf, 0xf, true);   // wave_shr:1: from lane - 1
                bR = (unsigned)__builtin_amdgcn_update_dpp(0, (int)bR, 0x130, 0xf, 0xf, true);   // wave_shl:1: from lane + 1
            }
            keptW |= ((bL & 15u) << (kPad - 4 * q)) | ((bR & 15u) << (kPad + 4 * q));
            undW |= ((bL >> 4) << (kPad - 4 * q)) | ((bR >> 4) << (kPad + 4 * q));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned own = undW & (1u << (kPad + j));
            const unsigned keepb = ((keptW | undW) & mk[j]) == 0u ? own : 0u;
            const unsigned dropb = (keptW & mk[j]) != 0u ? own : 0u;
            undW &= ~(keepb | dropb);
            keptW |= keepb;
        }
        bC = ((keptW >> kPad) & 15u) | (((undW >> kPad) & 15u) << 4);
        if (!__ballot((bC >> 4) != 0u)) break;
    }
    const unsigned keep = bC & 15u;
    const bool doubt_any = __ballot(dbt) != 0ull;
    const unsigned incl_k = wave_incl_scan_u32((unsigned)__popc(keep));
    const int nkw = (int)__builtin_amdgcn_readlane((int)incl_k, 63);
    unsigned long long key[4];
    bool val[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        key[j] = (unsigned long long)__double_as_longlong(ws[kPad + j]);
        val[j] = (keep >> j) & 1u;
    }
    unsigned long long Tw = 0ull;
    if (nkw <= E) {
        // the cut list does not hold E + 1 kept peaks: the peaks below the threshold could belong to the E (or, with the
        // whole unfiltered... -- the list is always filtered on this path)
        outcome = not_clear;
    } else {
        // the E-th largest kept key: MSD radix select from the top, six bits a level, lane l counts digit 63 - l
        unsigned hmn = 0xffffffffu, hmx = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned hw = (unsigned)(key[j] >> 32);
            hmn = min(hmn, val[j] ? hw : 0xffffffffu);
            hmx = max(hmx, val[j] ? hw : 0u);
        }
        hmn = wave_min_u32(hmn);
        hmx = wave_max_u32(hmx);
        const unsigned long long gmin = (unsigned long long)hmn << 32, gmax = ((unsigned long long)hmx << 32) | 0xffffffffull;
        int shift = 63 - __clzll((long long)(gmin ^ gmax)) - 5;   // (>= 26: the low words differ by construction)
        int width = 6;
        unsigned long long pfx = gmin >> (shift + 6);              // bits above the digit, common to every key
        unsigned rnk = (unsigned)E - 1u;                           // rank from the top, 0-based
        for (;;) {
            L.wl[lane] = 0u;
            wfence();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool mbr = val[j] && (key[j] >> (shift + width)) == pfx;
                if (mbr) atomicAdd(&L.wl[63u - (unsigned)((key[j] >> shift) & ((1ull << width) - 1ull))], 1u);
            }
            wfence();
            const unsigned c = L.wl[lane];
            const unsigned incl = wave_incl_scan_u32(c);
            const int fl = (int)__builtin_ctzll(__ballot(incl > rnk));   // (the members number more than rnk)
            const unsigned cb = (unsigned)__builtin_amdgcn_readlane((int)c, fl);
            rnk -= (unsigned)__builtin_amdgcn_readlane((int)(incl - c), fl);
            pfx = (pfx << width) | (unsigned long long)(63 - fl);
            if (shift == 0) {   // every bit decided: the members are copies of one key
                Tw = pfx;
                break;
            }
            if (cb <= 64u) {
                unsigned wc = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool mbr = val[j] && (key[j] >> shift) == pfx;
                    const unsigned long long mask = __ballot(mbr);
                    const unsigned at = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                    if (mbr) L.wlist[wc + at] = key[j];
                    wc += (unsigned)__popcll(mask);
                }
                wfence();
                const unsigned long long mine = (unsigned)lane < cb ? L.wlist[lane] : 0ull;
                unsigned rank = 0;
                for (unsigned i = 0; i < cb; ++i) {
                    const unsigned long long o =
                        ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(mine >> 32), (int)i) << 32) |
                        (unsigned)__builtin_amdgcn_readlane((int)(unsigned)mine, (int)i);
                    rank += (o > mine || (o == mine && i < (unsigned)lane)) ? 1u : 0u;
                }
                const int tl = (int)__builtin_ctzll(__ballot((unsigned)lane < cb && rank == rnk));
                Tw = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(mine >> 32), tl) << 32) |
                     (unsigned)__builtin_amdgcn_readlane((int)(unsigned)mine, tl);
                break;
            }
            const int ns_ = shift >= 6 ? shift - 6 : 0;
            width = shift - ns_;
            shift = ns_;
        }
        // the cut is certain when no other key reaches the lower end of T's band, and it must lie certainly above the
        // threshold the peaks were picked with
        const double Td = __longlong_as_double((long long)Tw);
        const unsigned long long Tlo = (unsigned long long)__double_as_longlong(fmax((Td - kBandAbs) * kBandLo, 0.0));
        unsigned gelo = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) gelo += (unsigned)__popcll(__ballot(val[j] && key[j] >= Tlo));
        if (doubt_any || gelo != (unsigned)E) outcome = 1;
        else if (!(Td >= tau_vhi)) outcome = not_clear;
    }
    if (outcome == 1u) {
        to_retry();
        return;
    }
    if (outcome == 4u) {
        to_big();
        return;
    }
    // (outcome 2 of the one-kernel form -- fewer than E kept peaks in an UNfiltered list -- cannot arise here: the list is
    // always threshold-filtered on this path, so a short list is "not clear" and is redone without the filter)

    // boundaries 0, selected peaks + FW (ascending: the list is position-ordered), n -- with P at each of them
    {
        unsigned sel = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) sel |= (val[j] && key[j] >= Tw) ? 1u << j : 0u;
        const unsigned cnt = (unsigned)__popc(sel);
        unsigned o = wave_incl_scan_u32(cnt) - cnt;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (sel & (1u << j)) {
                L.cpts[1 + o] = wp[kPad + j] + FW;
                L.pb[1 + o] = pq[j];
            }
            o += (sel >> j) & 1u;
        }
        if (lane == 0) {
            L.cpts[0] = 0;
            L.pb[0] = 0.0;
            L.cpts[E + 1] = n;
            L.pb[E + 1] = hdr.ptot;
        }
    }
    wfence();
    stamp(7);
    const int nseg = E + 1;
    // event means: sum = P(end) - P(start) (exact), one division each
    for (int s = lane; s < nseg; s += 64) L.ev[s] = (L.pb[s + 1] - L.pb[s]) / (double)(L.cpts[s + 1] - L.cpts[s]);
    wfence();
    // Refinement branch (tRNA models): the adapter's segmentation and the clip bounds go to the refinement kernels
    // (fast_body's hand-over record, written from here)
    if (A.rf.ws) {
        RefineRec *rr = reinterpret_cast<RefineRec *>(A.rf.ws) + r;
        for (int s = lane; s < nseg; s += 64) rr->ev[s] = L.ev[s];
        for (int s = lane; s <= nseg; s += 64) rr->cpts[s] = L.cpts[s];
        if (lane == 0) {
            const ClipRec cr = F.clip[r];
            rr->n = n;
            rr->lo = cr.lo;
            rr->hi = cr.hi;
            rr->state = 1;
        }
        return;
    }
    // mean and population sd in numpy's summation order (fast_mean_sd's wave-0 body, without its workgroup barriers)
    double mean, sd;
    {
        const double *ev = L.ev;
        double *tmp = L.tmp;
        const int nn = nseg;
        auto pw = [&](const double *a) -> double {
            double res;
            if (nn < 8) {
                res = 0.0;
                for (int i = 0; i < nn; ++i) res += a[i];
                return res;
            }
            const int nmain = nn - (nn % 8), J = nmain / 8;  // J <= 16
            double v[16], tl[7];
            // (lanes 0 .. 7 carry numpy's eight accumulators; the other lanes read the same slots: one address, sixteen
            // loads at immediate offsets, all inside the kFSeg-entry arrays -- entries from nmain on are never added)
            const double *al = a + (lane & 7);
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = al[8 * j];
#pragma unroll
            for (int j = 0; j < 7; ++j) tl[j] = a[min(nmain + j, nn - 1)];
            double rr = v[0];
#pragma unroll
            for (int j = 1; j < 16; ++j)
                if (j < J) rr += v[j];
            auto rl = [&](int l) __attribute__((always_inline)) -> double {
                const long long b = __double_as_longlong(rr);
                const unsigned lo_ = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l);
                const unsigned hi_ = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l);
                return __longlong_as_double((long long)(((unsigned long long)hi_ << 32) | lo_));
            };
            const double r0 = rl(0), r1 = rl(1), r2 = rl(2), r3 = rl(3);
            const double r4 = rl(4), r5 = rl(5), r6 = rl(6), r7 = rl(7);
            res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
#pragma unroll
            for (int j = 0; j < 7; ++j)
                if (nmain + j < nn) res += tl[j];
            return res;
        };
        mean = pw(ev) / (double)nn;
        for (int s = lane; s < nn; s += 64) {
            const double df = ev[s] - mean;
            tmp[s] = df * df;
        }
        wfence();
        sd = sqrt(pw(tmp) / (double)nn);
    }
    stamp(8);
    double zc = 0.0, zs = 1.0;  // z = (ev - zc) / zs
    // medians (np.median of <= 128 values, no NaN: a bitonic sort of two values per lane in registers, wdx_wave.h) -- only for
    // the median normalisation and the six statistics (adapter_dt_med/mad, adapter_event_mean/std/med/mad, sig_proc.py:562-567)
    const bool in0 = lane < nseg, in1 = lane + 64 < nseg;
    const double inf = __builtin_inf();
    double ev_med = 0.0, ev_mad = 0.0;
    if (P.seg_norm == WDX_NORM_MEDIAN || A.stats) {   // (wave-uniform)
        const double e0 = in0 ? L.ev[lane] : inf, e1 = in1 ? L.ev[lane + 64] : inf;
        ev_med = wave_median(e0, e1, nseg, lane);
        ev_mad = wave_median(in0 ? fabs(e0 - ev_med) : inf, in1 ? fabs(e1 - ev_med) : inf, nseg, lane);
    }
    if (P.seg_norm == WDX_NORM_MEAN) {
        zc = mean;
        zs = sd;
    } else if (P.seg_norm == WDX_NORM_MEDIAN) {
        zc = ev_med;
        zs = ev_mad;
    }
    if (nseg < K) {
        fail(WDX_READ_FAIL_UNKNOWN);
        return;
    }
    for (int i = lane; i < K; i += 64) {
        const int s = nseg - K + i;
        if (A.fpt) A.fpt[r * K + i] = P.seg_norm == WDX_NORM_NONE ? L.ev[s] : (L.ev[s] - zc) / zs;
        if (A.dwell) A.dwell[r * K + i] = (int64_t)(L.cpts[s + 1] - L.cpts[s]);
    }
    if (A.stats) {
        const double d0 = in0 ? (double)(L.cpts[lane + 1] - L.cpts[lane]) : inf;
        const double d1 = in1 ? (double)(L.cpts[lane + 65] - L.cpts[lane + 64]) : inf;
        const double dt_med = wave_median(d0, d1, nseg, lane);
        const double dt_mad = wave_median(in0 ? fabs(d0 - dt_med) : inf, in1 ? fabs(d1 - dt_med) : inf, nseg, lane);
        if (lane == 0) {
            double *o = A.stats + r * 6;
            o[0] = dt_med; o[1] = dt_mad; o[2] = mean; o[3] = sd; o[4] = ev_med; o[5] = ev_mad;
        }
    }
    if (lane == 0) A.status[r] = WDX_READ_OK;
    if (pp && lane == 0) {
        pp[9] = (long long)__builtin_amdgcn_s_memtime();
        pp[12] = M;
        pp[14] = 1;
    }
}

// ---- from a key to its kernel ------------------------------------------------------------------------------------------
// A kernel of the fast families and the LdsAttr that belongs to it: one static per instantiation.
using FastKernel = void (*)(FastArgs);
struct FpKernel {
    FastKernel fn = nullptr;   // null: not built (fp_key_exists says which are)
    LdsAttr *attr = nullptr;
};
template <auto K>
inline FpKernel fp_kernel() {
    return {K, &lds_attr_of<K>()};
}
// The kernels of one (width, NBT) pair, as fp_key_exists (wdx_fp_plan.h) lists them: what a pair has follows from its class
// there, and nothing is instantiated here that the table does not name.  The exact-scores-only widths (kWide, kWideOdd) are
// resolved in translation units of their own (wdx_fingerprint_w1.hip .. _w4.hip: the build compiles them side by side -- one
// unit with every width took seven minutes).
template <int FW, int NBT>
inline FpKernel resolve_fast_width(const FpKernelKey &k) {
    constexpr FpWidthClass WC = fp_width_class(FW, NBT);
    static_assert(WC != kNoWidth, "fp_width_class: wdx_fp_plan.h");
    if (k.fw != FW || k.nbt != NBT || !fp_key_exists(k)) return {};
    const bool main = k.family == kFamFastMain;
    if constexpr (WC != kFull) {
        // (exact-scores-only widths: no retry launch and capF = 6144, so the one-workgroup-per-entry list kernel is never launched
        // for them; odd widths do without the streaming form too -- windows beyond 8192 samples take the exact kernel)
        if (main) return k.ext ? fp_kernel<fingerprint_fast_kernel<kNptLarge, false, FW, 2, true>>() : fp_kernel<fingerprint_fast_kernel<kNptLarge, false, FW, 2, false>>();
        if (k.family == kFamListStride) return fp_kernel<fingerprint_fast_list_kernel<kNptHuge, FW, 2>>();
        if constexpr (WC == kWide) {
            if (k.family == kFamStream) return fp_kernel<fingerprint_fast_stream_kernel<FW, 2>>();
        }
        return {};
    } else {
        if (k.family == kFamList1 && !k.split) return fp_kernel<fingerprint_fast_list1_kernel<kNptLarge, FW, NBT>>();   // 6144 samples, one workgroup per entry
        if (k.family == kFamListStride) return fp_kernel<fingerprint_fast_list_kernel<kNptHuge, FW, NBT>>();       // 8192 samples, striding
        if (k.family == kFamStream) return fp_kernel<fingerprint_fast_stream_kernel<FW, NBT>>();
        if constexpr (NBT == 2) {
            if (main && !k.split) return k.ext ? fp_kernel<fingerprint_fast_kernel<kNptLarge, false, FW, 2, true>>() : fp_kernel<fingerprint_fast_kernel<kNptLarge, false, FW, 2, false>>();
            if constexpr (fp_has_split(FW, 2)) {
                if (main) return fp_kernel<fingerprint_fast_kernel<kNptLarge, false, FW, 2, true, true>>();
                if (k.family == kFamSplitTail) return fp_kernel<fingerprint_split_tail_kernel<FW, 2>>();
            }
        } else {
            if (main && k.npt == kNptMid && !k.prof)   // (always EXT)
                return !k.split ? fp_kernel<fingerprint_fast_kernel<kNptMid, false, FW, 1, true>>() : fp_kernel<fingerprint_fast_kernel<kNptMid, false, FW, 1, true, true>>();
            if (k.family == kFamSplitTail) return fp_kernel<fingerprint_split_tail_kernel<FW, 1>>();
            if (k.family == kFamList1) return fp_kernel<fingerprint_fast_list1_kernel<kNptLarge, FW, 1, true>>();
            if constexpr (fp_has_prof(FW, 1)) {
                if (main && k.npt == kNptMid)   // (the tile kernel's diagnostic build: wdx_fingerprint_profile_dev's fast_path = 2)
                    return !k.split ? fp_kernel<fingerprint_fast_kernel<kNptMid, true, FW, 1, true>>() : fp_kernel<fingerprint_fast_kernel<kNptMid, true, FW, 1, true, true>>();
                if (main && k.npt == kNptSmall)
                    return k.ext ? (k.prof ? fp_kernel<fingerprint_fast_kernel<kNptSmall, true, FW, 1, true>>() : fp_kernel<fingerprint_fast_kernel<kNptSmall, false, FW, 1, true>>())
                                 : (k.prof ? fp_kernel<fingerprint_fast_kernel<kNptSmall, true, FW, 1, false>>() : fp_kernel<fingerprint_fast_kernel<kNptSmall, false, FW, 1, false>>());
                if (main && k.prof) return k.ext ? fp_kernel<fingerprint_fast_kernel<kNptLarge, true, FW, 1, true>>() : fp_kernel<fingerprint_fast_kernel<kNptLarge, true, FW, 1, false>>();
            }
            if (main) return k.ext ? fp_kernel<fingerprint_fast_kernel<kNptLarge, false, FW, 1, true>>() : fp_kernel<fingerprint_fast_kernel<kNptLarge, false, FW, 1, false>>();
        }
        return {};
    }
}
FpKernel resolve_fast_w1(const FpKernelKey &k);   // widths 8, 10, 14, 16, 20      (wdx_fingerprint_w1.hip)
FpKernel resolve_fast_w2(const FpKernelKey &k);   // widths 22, 26, 28, 32, 34     (wdx_fingerprint_w2.hip)
FpKernel resolve_fast_w3(const FpKernelKey &k);   // odd widths 7 .. 19            (wdx_fingerprint_w3.hip)
FpKernel resolve_fast_w4(const FpKernelKey &k);   // odd widths 21 .. 35           (wdx_fingerprint_w4.hip)
