// ---- fast path -------------------------------------------------------------------------------------
// fingerprint_fast_kernel / _list1_kernel / _list_kernel: one 256-thread workgroup per read, the read's samples in
// LDS (five workgroups per CU up to 5120 samples, four at 6144, three at 8192).  They take the common case and hand
// everything else on through device-side lists (launch_fingerprint chains the launches, DESIGN.md 4.1):
//   a window or peak list beyond this instantiation's capacity        -> the next larger instantiation
//   an order decision inside the error band of the approximate keys   -> the same code with exact scores
//   NaN in the window, window > 8192 samples, effective window width != 12, a plateau beyond the walk's reach,
//   an exact score tie at the top-E cut, sums that are not provably exact, fewer than E peaks under accept_less_cpts, signal
//   normalisation options                                             -> the exact general path (fp_process_read)
// Everything they do produce is bit-identical to that path:
//   * medians: 11-bit-digit MSD radix select + small-list finish (exact order statistics)
//   * scores: only their ORDER reaches the output.  Approximate keys (S1 - S1')^2 / (V + V') from sliding sums, every
//     comparison taken only beyond an error band (kBandHi / kBandAbs), and the reference's exact operations
//     (left-to-right float64 sums, un-fused; x/12 as q=x*c, r=fma(-12,q,x), fma(r,c,q) -- the correctly rounded
//     quotient; the compiler's sqrt / division iterations without their range scaling) wherever a decision falls
//     inside the band.  A lane handles kR consecutive window starts; the statistics of window pos+12 come from
//     lane + kShift by wave shuffle; halo lanes make a wave independent of its neighbours
//   * strict local maxima (incl. in-wave plateaus) go straight into a position-ordered compact peak list;
//     suppression / top-E / boundaries operate on that list (~N/5.6 entries)
//   * event means: when every partial sum of the float32 samples is exactly representable in float64
//     (checked from the clip bounds) summation order is irrelevant -> chunked partial sums + LDS atomics

// Workgroup shape, capacities and the LDS carve-up's formulae (FB, kFW, kFSeg, kNpt*, kCapPMax, fast_sh_offset, ...): wdx_fp_plan.h,
// where the host's plan reads the same ones.
constexpr int FB = kFastBlock;   // threads per workgroup
#ifndef WDX_WIDE_WG
#define WDX_WIDE_WG 5
#endif
static_assert(kWideWgPerCu == WDX_WIDE_WG, "the plan's capacities assume this budget: wdx_fp_plan.h");
constexpr int kWaves = FB / 64;
constexpr int kR = 6;             // consecutive score positions per lane in the t-score tile
constexpr int kMaxPk = kR / 2;   // strict local maxima a lane can hold (they are >= 2 apart)
// (per instantiation, in fast_body: kShiftW = FW / kR lanes between a window and the one FW samples further, kOwnW =
// 63 - 2 kShiftW owned lanes per wave, kTSW = kWaves * kOwnW * kR score positions per tile)
constexpr int kRounds = kCapPMax / (4 * FB) > 0 ? kCapPMax / (4 * FB) : 1;  // 4-peak ownership rounds
constexpr int kNB = 4;           // neighbours per side inspected by the suppression, per neighbour thread (x NBT)
static_assert(kFW % kR == 0 && kR == 6, "tile geometry");

constexpr int kReach = 2;        // lanes ahead whose scores a plateau walk holds in registers (further ones: by shuffle)
// Banded decisions on approximate score keys (first attempt of P2..P4, see fast_body): key ~ (S1 - S1')^2 / (V + V')
// = 144 t^2 within a relative 2^-27 (+ 2^-43); a comparison "a outranks b" is taken only when
// a > b * kBandHi + kBandAbs, which implies the same strict order between the reference's rounded scores
// (error budget in DESIGN.md 4.1); anything closer is a doubt and the read is redone with exact scores.
constexpr double kBandHi = 1.0 + 0x1p-20;
constexpr double kBandLo = 1.0 - 0x1p-20;
constexpr double kBandAbs = 0x1p-50;
// variance sums below kVarFloorC(FW) * max|x|^2 are not trusted.  Error of a window's variance from the fused sliding
// sums, in units of u * B with B = FW * max|x|^2: 6 roundings per six-sample block sum and FW / 6 blocks in the
// first window, FW / 6 - 1 additions of block sums, two fused updates per slide (<= 5 slides), the S1 * (1/FW)
// product with its rounded constant and the final fma -> c(FW) = FW + FW/6 - 1 + 10 + 3.1 = 26.1 / 33.1 / 47.1 for
// FW = 12 / 18 / 30; the floor 2 c(FW) * 2^27 * u * B (rounded up: 53 / 67 / 95) keeps V + V' good to 2^-27 relative.
// (general width: 2 c(FW) rounded up = 2 FW + FW / 3 + 25 -- 39 / 53 / 67 / 81 / 95 / 109 for FW = 6 ... 36)
__host__ __device__ constexpr double kVarFloorC(int fw) {
    return (double)(2 * fw + fw / 3 + 25) * (double)fw * 0x1p-26;
}
static_assert(2 * 12 + 12 / 3 + 25 == 53 && 2 * 18 + 18 / 3 + 25 == 67 && 2 * 30 + 30 / 3 + 25 == 95, "the shipped widths' floors");
// Threshold filters of the peak list (fast_body).  Of the ~830 strict local maxima of a read only the ~E + 12 that reach
// the score of the E-th selected peak matter: greedy suppression is decided from the top down (a peak is dropped only by a
// HIGHER kept peak within d_eff), so the fate of every peak above a threshold tau does not depend on the peaks below it,
// and the E highest kept peaks of the list cut at tau are the E highest kept peaks of the whole list as soon as the E-th
// of them lies certainly above tau.  That condition is checked wherever a cut was applied; a read that fails it takes the
// next, less filtered form -- so the thresholds decide speed, never results.
// They are constants of the statistic, not of the data: key = FW^2 t^2 is scale-free, and over windows of pure noise
// (two windows of FW samples, variance sigma^2) key ~ z^2 with z standard normal, whatever sigma and FW, while a change
// of level by delta gives key ~ FW (delta / sigma)^2 / 2.
//   kPeakTauLo (|z| = 1.58) at the APPEND: ~340 entries per RNA004 read instead of ~830, never more than ~430 -- the list
//     fits 512 entries (26.8 KB of LDS: six workgroups per CU).  Where the E-th selected peak is itself a noise maximum
//     (fewer than E real level changes in the window) the cut at the E-th score falls below it: that read is redone by
//     the exact-scores launch, which never filters.
//   kPeakTauHi (|z| = 2.45) when the one-wave form of P3b..P5 picks its <= 256 peaks out of that list (~195 on RNA004
//     reads): a read whose E-th selected peak does not lie certainly above it (a third of the reads when the RNA002 triple
//     meets RNA004-length windows) runs the workgroup-wide form on the whole list instead.
constexpr double kPeakTauLo = 2.5, kPeakTauHi = 6.0;
constexpr int kTopBits = 9;       // radix digit of the top-E select over the kept peaks' float64 scores
constexpr int kTopKHistBytes = ((1 << kTopBits) + 64) * 4;  // its histogram (+ one trash bin per lane)
struct FastArgs {
    FpArgs a;
    int capF;              // adapter samples the LDS carve-up holds (multiple of 64)
    int capP;              // peak-list capacity
    unsigned *slow_count;  // list of reads for the slow path
    int32_t *slow_list;
    unsigned *big_count;   // list of reads that only exceed THIS instantiation's capacities (adapter
    int32_t *big_list;     // window > capF, peak lists): retried by the 8192-sample one; may be null
    const unsigned *in_count;  // list kernels: the reads to process
    const int32_t *in_list;
    unsigned in_start;         // striding list kernel: first list entry it takes
    unsigned *retry_count;     // reads whose approximate score keys left a decision inside the error band: redone by
    int32_t *retry_list;       // an exact-scores launch (a.exact_scores = 1); null -> slow path
    const ClipRec *clip;       // EXT main kernel: its reads' clip bounds (clip_bounds_kernel ran ahead of it); else null
    int routed;                // 1: windows beyond capF are on big_list already (route_long_windows_kernel): not listed here
    // SPLIT kernels (fingerprint_fast_kernel / _list1_kernel<..., SPLIT> + fingerprint_split_tail_kernel): the peak lists of
    // one launch slice, kSplitRecBytes each (see SplitHdr), slot = workgroup index of the slice -- reads split_base ..
    // split_base + split_n - 1 (main kernel) or entries split_base .. of in_list (list kernel: in_list / in_count set)
    unsigned char *split_ws;
    int64_t split_base, split_n;
};

// What the SPLIT main kernel leaves per read for fingerprint_split_tail_kernel (one wave per read): the peaks that can
// matter -- the list's entries from kPeakTauHi up when it has more than 256, else the whole (kPeakTauLo-filtered) list --
// in position order, each with its key and with P = the sum of the window's clipped samples before the boundary the peak
// would become (position + FW).  The tail kernel needs no sample: an event's sum is the difference of two P.
//   [0, 16)        SplitHdr
//   [16, 2064)     key[256]  float64
//   [2064, 4112)   P[256]    float64
//   [4112, 4624)   pos[256]  uint16
struct SplitHdr {
    int32_t m;       // < 0: nothing exported (the read failed, or went to one of the lists); else entries | kSplitCutHi
    int32_t n;       // adapter window length
    double ptot;     // sum of all n clipped samples = P(n)
};
constexpr int kSplitMax = 256;
constexpr int kSplitCutHi = 1 << 16;   // the entries were cut at kPeakTauHi (else: the whole list, cut at kPeakTauLo)
constexpr size_t kSplitRecBytes = 16 + (size_t)kSplitMax * 18;

struct alignas(8) FastShared {
    // cross-wave exchange slots, double-buffered by call parity so that every block-wide
    // reduction / scan / vote needs ONE barrier (see BlockEx)
    unsigned slot_a[2][kWaves], slot_b[2][kWaves], slot_c[2][kWaves];
    unsigned long long w64[kWaves];
    unsigned sel_bin, sel_k, sel_cnt, pad0_;
    unsigned long long sel_key, sel_key2;  // rank k and (when it sits in the same small list) rank k+1
    unsigned sel_has2, pad_;
    unsigned rk[64];       // partial ranks of the <= 64 members of a select's final bin
    double mean, sd;
    double stat[6];
};
static_assert(sizeof(FastShared) == kFastSharedBytes, "the LDS formulae: wdx_fp_plan.h");

// Block-wide exchange with one barrier per call: calls alternate between two slot sets, so a wave
// that races ahead into call k+2 cannot overwrite what a slower wave still reads in call k
// (call k+1's barrier sits in between).
struct BlockEx {
    FastShared &sh;
    int par;
    __device__ __forceinline__ BlockEx(FastShared &s) : sh(s), par(0) {}

    // exclusive scan of one unsigned per thread; total = block sum
    // (the wave index as a scalar: the prefix over the waves' totals is then SALU work)
    __device__ __forceinline__ unsigned scan(unsigned v, unsigned &total) {
        const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        const unsigned incl = wave_incl_scan_u32(v);
        if (lane == 63) sh.slot_a[par][wave] = incl;
        __syncthreads();
        unsigned base = 0;
        total = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) {
            const unsigned w = sh.slot_a[par][k];
            base += k < wave ? w : 0u;
            total += w;
        }
        par ^= 1;
        return base + incl - v;
    }
    // (min, max, sum) over the block
    __device__ __forceinline__ void minmaxsum(unsigned mn, unsigned mx, unsigned sm, unsigned &omn,
                                              unsigned &omx, unsigned &osm) {
        const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        mn = wave_min_u32(mn);
        mx = wave_max_u32(mx);
        sm = wave_sum_u32(sm);
        if (lane == 0) {
            sh.slot_a[par][wave] = mn;
            sh.slot_b[par][wave] = mx;
            sh.slot_c[par][wave] = sm;
        }
        __syncthreads();
        omn = 0xffffffffu;
        omx = 0;
        osm = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) {
            omn = min(omn, sh.slot_a[par][k]);
            omx = max(omx, sh.slot_b[par][k]);
            osm += sh.slot_c[par][k];
        }
        par ^= 1;
    }
    __device__ __forceinline__ unsigned sum(unsigned v) {
        const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        v = wave_sum_u32(v);
        if (lane == 0) sh.slot_a[par][wave] = v;
        __syncthreads();
        unsigned r = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) r += sh.slot_a[par][k];
        par ^= 1;
        return r;
    }
    // block-wide OR of a predicate (replaces __syncthreads_or, which costs several barriers)
    __device__ __forceinline__ bool any(bool pred) {
        const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        const unsigned long long b = __ballot(pred);
        if (lane == 0) sh.slot_a[par][wave] = b != 0;
        __syncthreads();
        unsigned r = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) r |= sh.slot_a[par][k];
        par ^= 1;
        return r != 0;
    }
};

__device__ __forceinline__ void fast_minmax64(unsigned long long mn, unsigned long long mx,
                                              FastShared &sh, unsigned long long &omn,
                                              unsigned long long &omx) {
    for (int off = 32; off > 0; off >>= 1) {
        unsigned long long a = __shfl_xor(mn, off), b = __shfl_xor(mx, off);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh.w64[wave] = mn;
    __syncthreads();
    omn = sh.w64[0];
    for (int k = 1; k < kWaves; ++k) omn = sh.w64[k] < omn ? sh.w64[k] : omn;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh.w64[wave] = mx;
    __syncthreads();
    omx = sh.w64[0];
    for (int k = 1; k < kWaves; ++k) omx = sh.w64[k] > omx ? sh.w64[k] : omx;
}

// (fast_sqrt_mid, fast_div_mid, max0_f64: wdx_fp_types.h -- shared with the refinement tail kernel)

template <class K>
__device__ __forceinline__ int key_bits(K v) {
    if (sizeof(K) == 8) return v ? 64 - __clzll((long long)v) : 0;
    return v ? 32 - __clz((int)v) : 0;
}

// k-th smallest key (0-based) among this workgroup's items.  `each(f)` calls f(key, valid) for EVERY
// slot of the calling thread (fully unrolled, branch-free consumers): invalid slots are steered to a
// trash bin / identity value instead of being branched around.  MSD digits of HBITS bits; as soon as
// the bin holding rank k has <= 64 members they are gathered and ranked by one wave.
// hist must hold (1 << HBITS) + 64 words (one trash bin per lane).  kmin/kmax: exact extremes of the valid keys.
#define WDX_SSTAMP(slot)                                                              \
    do {                                                                             \
        if (pp) {                                                                    \
            __syncthreads();                                                         \
            if (threadIdx.x == 0) pp[slot] = (long long)__builtin_amdgcn_s_memtime(); \
        }                                                                            \
    } while (0)

// FULLRANGE: kmax - kmin may need all bits of K (only the signed float32 keys can)
template <class K, int HBITS, bool FULLRANGE, class Each>
__device__ K fast_select(Each each, unsigned k, K kmin, K kmax, unsigned *hist, BlockEx &bx,
                         long long *pp = nullptr, int stop_sub = 0, float lin_scale = 0.0f) {
    FastShared &sh = bx.sh;
    constexpr int KB = sizeof(K) * 8;
    constexpr int HB = 1 << HBITS;
    constexpr int BPT = HB / FB;  // bins per thread: 2, 4, 8 or 16
    static_assert(BPT == 2 || BPT % 4 == 0, "bins per thread must be 2 or a multiple of 4");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int rb = key_bits<K>(kmax - kmin);
    K prefix = 0;
    bool first = true;
    // lin_scale > 0 (32-bit keys that are bit patterns of non-negative floats starting at 0, i.e. the
    // |x - median| keys): the first level bins the VALUE linearly, bin = floor(value * lin_scale) < HB,
    // instead of taking the top bits of the pattern, which are exponent-aligned and far too coarse
    // around the median when outliers stretch the range.  The bin function is monotone in the key, so
    // the members of a bin are a contiguous key range; it is re-evaluated wherever membership is needed
    // until the members' key range [kmin, kmax] has been narrowed to exactly that bin.
    bool lin = lin_scale > 0.0f && sizeof(K) == 4;
    unsigned lin_bin = 0;
    bool restricted = false;  // kmin/kmax were narrowed to a sub-range: keys outside it are not members
    // (no clamp: every key is <= kmax = dmax, lin_scale = RN((HB - 1) / dmax), so the product is at most
    // (HB - 1)(1 + 3 * 2^-24) < HB)
    auto linbin = [&](K key) -> unsigned { return (unsigned)(__uint_as_float((unsigned)key) * lin_scale); };
    while (rb > 0) {
        const int b = rb < HBITS ? rb : HBITS;
        const int shift = rb - b;
        uint4 *h4 = reinterpret_cast<uint4 *>(hist);
        uint2 *h2 = reinterpret_cast<uint2 *>(hist);
        if (BPT == 2) {
            h2[tid] = make_uint2(0, 0);
        } else {
#pragma unroll
            for (int j = 0; j < BPT / 4; ++j) h4[tid * (BPT / 4) + j] = make_uint4(0, 0, 0, 0);
        }
        __syncthreads();
        const unsigned dmask = (1u << b) - 1u;
        const bool top = FULLRANGE && rb >= KB;
        if (first && lin) {
            each([&](K key, bool valid) {
                const unsigned bin = valid ? linbin(key) : (unsigned)(HB + lane);
                atomicAdd(&hist[bin], 1u);
            });
        } else if (first) {
            // first level: every key shares the (empty) prefix and d >> shift < 2^b by construction
            each([&](K key, bool valid) {
                const K d = key - kmin;
                const unsigned bin = valid ? (unsigned)(d >> shift) : (unsigned)(HB + lane);
                atomicAdd(&hist[bin], 1u);
            });
        } else {
            if (restricted) {
                each([&](K key, bool valid) {
                    const K d = key - kmin;
                    const bool in = key >= kmin && key <= kmax;
                    const unsigned bin = (valid && in && (d >> rb) == prefix) ? ((unsigned)(d >> shift) & dmask)
                                                                              : (unsigned)(HB + lane);
                    atomicAdd(&hist[bin], 1u);
                });
            } else {
                each([&](K key, bool valid) {
                    const K d = key - kmin;
                    const K hi = top ? (K)0 : (d >> rb);
                    const unsigned bin =
                        (valid && hi == prefix) ? ((unsigned)(d >> shift) & dmask) : (unsigned)(HB + lane);
                    atomicAdd(&hist[bin], 1u);
                });
            }
        }
        const bool lin_level = first && lin;
        first = false;
        if (stop_sub == 1) return kmin;  // ablation timing only
        __syncthreads();
        WDX_SSTAMP(1);
        unsigned c[BPT];
        if (BPT == 2) {
            const uint2 v = h2[tid];
            c[0] = v.x;
            c[BPT - 1] = v.y;
        } else {
#pragma unroll
            for (int j = 0; j < BPT / 4; ++j) {
                const uint4 v = h4[tid * (BPT / 4) + j];
                c[4 * j] = v.x; c[4 * j + 1] = v.y; c[4 * j + 2] = v.z; c[4 * j + 3] = v.w;
            }
        }
        unsigned s = 0;
#pragma unroll
        for (int j = 0; j < BPT; ++j) s += c[j];
        unsigned total;
        const unsigned e = bx.scan(s, total);
        if (k >= e && k < e + s) {
            unsigned kk = k - e;
            int bin = 0;
#pragma unroll
            for (int j = 0; j < BPT; ++j) {
                if (bin == j && kk >= c[j]) {
                    kk -= c[j];
                    bin = j + 1;
                }
            }
            unsigned cb = 0;
#pragma unroll
            for (int j = 0; j < BPT; ++j)
                if (j == bin) cb = c[j];
            sh.sel_bin = (unsigned)(tid * BPT + bin);
            sh.sel_k = kk;
            sh.sel_cnt = cb;
        }
        __syncthreads();
        if (lin_level) {
            lin_bin = sh.sel_bin;  // membership = linbin(key) == lin_bin until the range is narrowed
        } else {
            prefix = (prefix << b) | (K)sh.sel_bin;
            rb = shift;
        }
        k = sh.sel_k;
        const unsigned cnt = sh.sel_cnt;
        WDX_SSTAMP(2);
        if (stop_sub == 2) return kmin;
        // membership tests of the selected bin; the choice between them is made OUTSIDE the data sweeps
        // (block-uniform), so a sweep carries only the arithmetic of its own variant
        auto member_lin = [&](K key, bool valid) -> bool { return valid && linbin(key) == lin_bin; };
        // (the members of a digit bin are a key range: one subtraction + one unsigned compare)
        const K dig_lo = kmin + (rb < KB ? (K)(prefix << rb) : (K)0);
        const K dig_span = rb < KB ? (K)((((K)1) << rb) - 1) : (K)~(K)0;
        auto member_dig = [&](K key, bool valid) -> bool { return valid && (K)(key - dig_lo) <= dig_span; };
        auto member_res = [&](K key, bool valid) -> bool {
            const K d = key - kmin;
            return valid && key >= kmin && key <= kmax && (d >> rb) == prefix;
        };
        if ((rb > 0 || lin_level) && cnt <= 64) {
            // Gather the <= 64 members of the bin without returning atomics or divergent branches: a
            // wave appends to its own list (the histogram is dead by now) at ballot-derived offsets,
            // skipping whole element slots without a member on a scalar branch.
            static_assert(kWaves * 64 * sizeof(K) <= (HB + 64) * sizeof(unsigned), "per-wave lists fit the histogram");
            K *wl = reinterpret_cast<K *>(hist);
            unsigned wcnt = 0;  // wave-uniform
            auto take = [&](auto &&memb) {
                each([&](K key, bool valid) {
                    const bool m = memb(key, valid);
                    const unsigned long long mask = __ballot(m);
                    if (mask) {
                        const unsigned at = __builtin_amdgcn_mbcnt_hi(
                            (unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                        if (m) wl[wave * 64 + wcnt + at] = key;
                        wcnt += (unsigned)__popcll(mask);
                    }
                });
            };
            if (lin_level) take(member_lin);
            else if (restricted) take(member_res);
            else take(member_dig);
            if (lane == 0) sh.slot_a[bx.par][wave] = wcnt;
            if (wave == 0) sh.rk[lane] = 0;
            __syncthreads();
            WDX_SSTAMP(3);
            if (stop_sub == 3) return kmin;
            {
                // lane l takes the l-th member over the concatenated wave lists; every wave ranks it against its
                // quarter of the members, reading their keys with v_readlane (no LDS round trip per comparison);
                // the partial ranks meet in LDS
                const unsigned ucnt = (unsigned)__builtin_amdgcn_readfirstlane((int)cnt);
                unsigned b = 0, src = 0;
#pragma unroll
                for (int w = 0; w < kWaves; ++w) {
                    const unsigned cw = sh.slot_a[bx.par][w];
                    if ((unsigned)lane >= b && (unsigned)lane < b + cw) src = w * 64 + (unsigned)lane - b;
                    b += cw;
                }
                const K mine = wl[src];  // lanes >= cnt read slot 0 and are ignored below
                const unsigned per = (ucnt + kWaves - 1) / kWaves;
                const unsigned j0 = (unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned)wave * per));
                const unsigned j1 = min(ucnt, j0 + per);
                unsigned rank = 0;
                for (unsigned j = j0; j < j1; ++j) {
                    K u;
                    if (sizeof(K) == 8) {
                        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)mine, (int)j);
                        const unsigned hi2 = (unsigned)__builtin_amdgcn_readlane(
                            (int)(unsigned)((unsigned long long)mine >> 32), (int)j);
                        u = (K)(((unsigned long long)hi2 << 32) | lo);
                    } else {
                        u = (K)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)mine, (int)j);
                    }
                    rank += (u < mine) || (u == mine && j < (unsigned)lane);
                }
                if (j0 < j1 && (unsigned)lane < ucnt) atomicAdd(&sh.rk[lane], rank);
                __syncthreads();
                if (wave == 0) {
                    const unsigned rk = sh.rk[lane];
                    if (lane == 0) sh.sel_has2 = (k + 1 < ucnt) ? 1u : 0u;
                    if ((unsigned)lane < ucnt && rk == k) sh.sel_key = (unsigned long long)mine;
                    if ((unsigned)lane < ucnt && rk == k + 1) sh.sel_key2 = (unsigned long long)mine;
                }
            }
            bx.par ^= 1;
            __syncthreads();
            WDX_SSTAMP(4);
            if (pp && threadIdx.x == 0) pp[6] = cnt;
            return (K)sh.sel_key;
        }
        if (lin_level) {
            // More than 64 members in a bin narrower than the sample quantum: usually copies of ONE value
            // (quantised samples repeat a lot) -- which no digit could split, and none has to.  Otherwise
            // the bit-pattern digits take over on the members' exact key range.
            unsigned mmn = 0xffffffffu, mmx = 0u;
            each([&](K key, bool valid) {
                const bool m = member_lin(key, valid);
                mmn = min(mmn, m ? (unsigned)key : 0xffffffffu);
                mmx = max(mmx, m ? (unsigned)key : 0u);
            });
            unsigned gmn, gmx, dmy;
            bx.minmaxsum(mmn, mmx, 0u, gmn, gmx, dmy);
            if (gmn == gmx) {
                if (tid == 0) {
                    sh.sel_has2 = (k + 1 < cnt) ? 1u : 0u;
                    sh.sel_key2 = (unsigned long long)gmn;
                }
                return (K)gmn;
            }
            kmin = (K)gmn;
            kmax = (K)gmx;
            restricted = true;
            lin = false;
            prefix = 0;
            rb = key_bits<K>(kmax - kmin);
        }
    }
    (void)wave;
    if (tid == 0) sh.sel_has2 = 0;  // (made visible by the caller's next barrier)
    return kmin + prefix;
}

// Exact np.median (float32) of sig[0..n) (mode 0) or of |sig[i] - center| (mode 1); no NaNs.
// kmin/kmax: any lower/upper bound of the keys (the caller knows the data extremes from the load).
// Inlined: each key kind (KM) has exactly one call site, so inlining duplicates nothing, and the call itself cost
// ~60 VALU instructions per wave plus a callee-saved register spilled to scratch (HBM writes) per call -- 2 % of the
// kernel.  Samples are re-read from LDS per pass, 4 consecutive per lane
// (ds_read_b128), only the ceil(n/1024) groups that hold data.  Passes: histogram, gather (+ a
// count pass only when the two middle elements of an even n fall into different histogram bins).
struct MedRet {
    float v;
    int par;
};
// KM: 0 = median of non-negative samples (keys are the raw bit patterns), 1 = median of |x - center|, 2 = median of
// samples that may be negative (order-preserving key transform).  One instantiation per key kind: the
// per-element key arithmetic is the bulk of every sweep.
template <int KM>
__device__ __forceinline__ MedRet fast_median_lds(unsigned sig_off, int n, float center, int mode,
                                               unsigned kmin, unsigned kmax, unsigned hist_off,
                                               unsigned sh_off, int par, long long *pp, int stop_sub = 0,
                                               bool final_barrier = true) {
    // LDS regions arrive as byte offsets into the workgroup's dynamic LDS block and every argument goes through
    // v_readfirstlane (kept from the time this body was a non-inlined function, whose arguments arrive in VGPRs and
    // whose pointer parameters would have been generic): all of them are workgroup-uniform, and pinning them to
    // SGPRs keeps every loop and branch below scalar control flow
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    sig_off = (unsigned)__builtin_amdgcn_readfirstlane((int)sig_off);
    hist_off = (unsigned)__builtin_amdgcn_readfirstlane((int)hist_off);
    sh_off = (unsigned)__builtin_amdgcn_readfirstlane((int)sh_off);
    n = __builtin_amdgcn_readfirstlane(n);
    kmin = (unsigned)__builtin_amdgcn_readfirstlane((int)kmin);
    kmax = (unsigned)__builtin_amdgcn_readfirstlane((int)kmax);
    par = __builtin_amdgcn_readfirstlane(par);
    stop_sub = __builtin_amdgcn_readfirstlane(stop_sub);
    center = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(center)));
    const float *sig = reinterpret_cast<const float *>(smem + sig_off);
    unsigned *hist = reinterpret_cast<unsigned *>(smem + hist_off);
    FastShared *shp = reinterpret_cast<FastShared *>(smem + sh_off);
    (void)mode;  // (kept in the signature for the diagnostic builds; the key kind is the template parameter)
    BlockEx bx(*shp);
    bx.par = par;
    FastShared &sh = *shp;
    const int tid = threadIdx.x;
    const float4 *sig4 = reinterpret_cast<const float4 *>(sig);
    const int NG = (n + 4 * FB - 1) / (4 * FB);
    // Keys are the raw float32 bit patterns whenever every value is non-negative (|x - center| always
    // is; the samples themselves almost always are), for which the bit pattern orders like the value;
    // the SIGNED instantiation applies the usual order-preserving transform instead.  Every group
    // but the last is full, so only the last one carries validity tests.
    constexpr bool SIGNED = KM == 2;
    auto K = [&](float v) -> unsigned {
        return KM == 2 ? f32_key(v) : (KM == 1 ? __float_as_uint(fabsf(v - center)) : __float_as_uint(v));
    };
    auto each = [&](auto &&f) {
        // the next group's ds_read_b128 is issued before the current group is consumed, so the LDS
        // latency overlaps the (atomic-issuing) consumer instead of preceding it
        float4 v = sig4[tid];
#pragma unroll 2
        for (int j = 0; j < NG - 1; ++j) {
            const float4 nx = sig4[(j + 1) * FB + tid];
            f(K(v.x), true);
            f(K(v.y), true);
            f(K(v.z), true);
            f(K(v.w), true);
            v = nx;
        }
        {
            const int i = ((NG - 1) * FB + tid) * 4;
            f(K(v.x), i < n);
            f(K(v.y), i + 1 < n);
            f(K(v.z), i + 2 < n);
            f(K(v.w), i + 3 < n);
        }
    };
    WDX_SSTAMP(0);
    const unsigned h = (unsigned)n / 2;
    const bool odd = n & 1;
    // |x - center| keys (mode 1; kmin == 0, kmax == bits(dmax)): linear first level over [0, dmax]
    float lin_scale = 0.0f;
    if (KM == 1) {
        const float dmaxf = __uint_as_float(kmax);
        if (dmaxf > 0.0f && dmaxf < 3.0e38f) lin_scale = (float)(kHB - 1) / dmaxf;
        if (!(lin_scale > 0.0f && lin_scale < 3.0e38f)) lin_scale = 0.0f;
    }
    const unsigned klo = fast_select<unsigned, kHBits, SIGNED>(each, odd ? h : h - 1, kmin, kmax, hist, bx, pp,
                                                               stop_sub, lin_scale);
    if (stop_sub) return MedRet{0.0f, bx.par};
    float res;
    if (odd) {
        res = SIGNED ? key_f32(klo) : __uint_as_float(klo);
    } else {
        __syncthreads();  // sel_has2 / sel_key2 of the exhausted-digits path
        unsigned khi;
        if (sh.sel_has2) {  // block-uniform
            khi = (unsigned)sh.sel_key2;
        } else {
            unsigned nxt = 0xffffffffu, le = 0;
            each([&](unsigned key, bool valid) {
                le += (valid && key <= klo) ? 1u : 0u;
                nxt = min(nxt, (valid && key > klo) ? key : 0xffffffffu);
            });
            unsigned gnxt, gle, dummy;
            bx.minmaxsum(nxt, 0u, le, gnxt, dummy, gle);
            khi = gle > h ? klo : gnxt;
        }
        WDX_SSTAMP(5);
        const float s = SIGNED ? key_f32(klo) + key_f32(khi) : __uint_as_float(klo) + __uint_as_float(khi);
        res = s / 2.0f;
    }
    if (final_barrier) __syncthreads();  // sh.sel_* may be rewritten by the next call
    return MedRet{res, bx.par};
}

// np.median of n <= 128 float64 values in LDS by rank counting spread over all 256 threads:
// thread t ranks element (t & 127) against half of the others; two elements may hit klo/khi.
__device__ double fast_small_median(const double *a, int n, unsigned *rankbuf, FastShared &sh) {
    const int tid = threadIdx.x;
    constexpr int kParts = FB / 128;  // each element is ranked against 128/kParts others per thread
    const int i = tid & 127, part = tid >> 7;
    __syncthreads();
    if (tid < 128) rankbuf[tid] = 0;
    __syncthreads();
    if (i < n) {
        const double v = a[i];
        const int j0 = part * (128 / kParts), j1 = min(n, j0 + 128 / kParts);
        unsigned rank = 0;
        for (int j = j0; j < j1; ++j) {
            const double u = a[j];
            rank += (u < v) || (u == v && j < i);
        }
        atomicAdd(&rankbuf[i], rank);
    }
    __syncthreads();
    const int klo = (n - 1) / 2, khi = n / 2;
    if (tid < n) {
        const unsigned rk = rankbuf[tid];
        if ((int)rk == klo) sh.w64[0] = (unsigned long long)__double_as_longlong(a[tid]);
        if ((int)rk == khi) sh.w64[1] = (unsigned long long)__double_as_longlong(a[tid]);
    }
    __syncthreads();
    const double lo = __longlong_as_double((long long)sh.w64[0]);
    const double hi = __longlong_as_double((long long)sh.w64[1]);
    return (n & 1) ? hi : (lo + hi) / 2.0;
}

// mean and population sd of n <= 128 event means in numpy's summation order, by wave 0 alone: the
// strided operands are fetched up front (one LDS latency), the squared deviations go through LDS inside
// the wave, and the workgroup meets at two barriers in total.
__device__ void fast_mean_sd(const double *ev, double *tmp, int n, FastShared &sh, double &mean, double &sd) {
    __syncthreads();
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        auto pw = [&](const double *a) -> double {
            double res;
            if (n < 8) {
                res = 0.0;
                for (int i = 0; i < n; ++i) res += a[i];
                return res;
            }
            const int nmain = n - (n % 8), J = nmain / 8;  // J <= 16
            double v[16], tl[7];
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = a[min(lane + 8 * j, n - 1) * (lane < 8 ? 1 : 0)];
#pragma unroll
            for (int j = 0; j < 7; ++j) tl[j] = a[min(nmain + j, n - 1)];
            double r = v[0];
#pragma unroll
            for (int j = 1; j < 16; ++j)
                if (j < J) r += v[j];
            // (lanes 0 .. 7 by v_readlane: scalar operands of the adds, no LDS round trip)
            auto rl = [&](int l) __attribute__((always_inline)) -> double {
                const long long b = __double_as_longlong(r);
                const unsigned lo_ = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l);
                const unsigned hi_ = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l);
                return __longlong_as_double((long long)(((unsigned long long)hi_ << 32) | lo_));
            };
            const double r0 = rl(0), r1 = rl(1), r2 = rl(2), r3 = rl(3);
            const double r4 = rl(4), r5 = rl(5), r6 = rl(6), r7 = rl(7);
            res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
#pragma unroll
            for (int j = 0; j < 7; ++j)
                if (nmain + j < n) res += tl[j];
            return res;
        };
        const double m = pw(ev) / (double)n;
        for (int s = lane; s < n; s += 64) {
            const double df = ev[s] - m;
            tmp[s] = df * df;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const double sdv = sqrt(pw(tmp) / (double)n);
        if (lane == 0) {
            sh.mean = m;
            sh.sd = sdv;
        }
    }
    __syncthreads();
    mean = sh.mean;
    sd = sh.sd;
}

#define WDX_FSTAMP(k)                                                                       \
    do {                                                                                    \
        if (PROF) {                                                                         \
            if ((k) > 0 && A.stop_phase == (k)) return; /* ablation: cost of phases <= k */ \
            if (r < A.prof_reads) {                                                         \
                __syncthreads();                                                            \
                if (tid == 0) A.prof[r * 32 + (k)] = (long long)__builtin_amdgcn_s_memtime(); \
            }                                                                               \
        }                                                                                   \
    } while (0)

// NPT = samples per thread in the load phase (capF = NPT * FB); a multiple of 4
// FW = the (effective) window width the instantiation takes: 12 (RNA004), 18 (tRNA triple), 30 (RNA002 triple).
// NBT = neighbour threads per side in the suppression: a thread owns 4 peaks, peaks are >= 2 apart, so 4 * NBT
// neighbours per side cover d_eff <= 8 * NBT + 1 (1: the RNA004 / tRNA distances 6 and 9; 2: RNA002's 15).
// EXT: the clip bounds come from clip_bounds_kernel (F.clip; large batches) -- the body starts at the clip and holds no
// median code; else (small batches: one launch, latency-bound) the two radix selects run here.
// STREAM (implies EXT; windows up to NPT * FB = 16384 samples): the samples are never resident -- the tiles stream
// them through two 1536-sample LDS buffers (tile t + 1 is requested from HBM before tile t is scored and lands in the
// other buffer behind it), the event means read them once more from HBM / L2 -- so the workgroup's LDS is the peak list
// plus 12 KB whatever the window length: three to four workgroups per CU for the 8193 .. 16384-sample windows of the
// RNA002 config instead of the exact kernel's one.
// SPLIT: 0 = the one-piece body; 1 = end after the tile pass and export the peaks for fingerprint_split_tail_kernel, a read with
// more than 256 peaks above the cut goes to the next launch (the main kernel: stays lean); 2 = the same, but such a read is
// finished in place by the one-piece code below (the 6144-sample list kernel: the last stop before the exact-scores launch)
#ifndef WDX_TILE_PRIO
#define WDX_TILE_PRIO 2
#endif
template <int NPT, bool PROF, int FW = kFW, int NBT = 1, bool EXT = false, bool STREAM = false, int SPLIT = 0>
__device__ __forceinline__ void fast_body(const FastArgs &F, const int64_t r) {
    static_assert(!STREAM || EXT, "the streaming form needs the clip bounds from clip_bounds_block_kernel");
    static_assert(!SPLIT || (EXT && !STREAM), "the split form is the large batches' main kernel");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const FpArgs &A = F.a;
    const wdx_seg_params &P = A.p;
    // (the wave index as a scalar: everything derived from it -- a wave's first position, whether it has work in a tile,
    // the prefix over the waves' counts -- is SALU work and scalar branches, and wave masks merged across such a branch
    // stay in scalar registers)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K = P.barcode_num_events, E = P.num_events;
    constexpr int capF = NPT * FB;
    static_assert(FW >= 6 && (NBT == 1 || NBT == 2), "tile / suppression geometry");
    // Widths that are not multiples of the tile's six positions per lane (round 6: every other width from 7 to 35) run on EXACT scores
    // only: the approximate pass builds a lane's first window from whole six-sample blocks of its neighbours, the exact pass
    // loads the lane's own kR + FW samples and needs the neighbours only for the partner window's statistics -- window
    // (pos + FW) of slot rr lives (rr + FW) / kR lanes further at slot (rr + FW) % kR.
    constexpr bool kExactOnly = FW % kR != 0;
    // window (pos + FW) lives kShiftW lanes further; lanes 1 .. kOwnW of a wave own score positions (lane 0 and
    // kOwnW + 1: halos).  The halo's score needs the window statistics of lane kOwnW + 1 + kShiftW, whose first window
    // is the sum of the blocks of kShiftW consecutive lanes: the last of them must exist -> kOwnW = 63 - 2 kShiftW
    constexpr int kShiftW = (FW + kR - 1) / kR, kOwnW = 63 - 2 * kShiftW, kTSW = kWaves * kOwnW * kR;   // (exact-only widths: rounded up)
    constexpr int kNBW = 4 * NBT, kPad = 4 * NBT;
    constexpr int kRounds = STREAM ? 4 : wdx::kRounds;  // 4-peak ownership rounds: peak lists up to 1024 * kRounds
    constexpr int kTB = kStreamBuf;                     // STREAM: samples per tile buffer
    static_assert(kTSW + FW + 2 * kR <= kTB, "a tile's samples fit the stream buffer");

    // LDS carve-up (sized for five workgroups per CU at capF = 5120, four at 6144): the samples, the peak list, the
    // exchange block.  Everything else aliases the peak-list region R while that part of it is dead:
    //   medians   hist   2048+64 words                      at R            (peak list not yet in use)
    //   top-E     hist   512+64 words                       at the end of pk_score (kept_key: the first nk <= kept_cap slots)
    //   P5..P7    cpts, rankbuf, ev, zz, tmp (4112 B)       at R            (kept lists are read before P5's barrier)
    float *sig = reinterpret_cast<float *>(smem);  // capF + 32 (STREAM: two tile buffers)
    double *pk_score = reinterpret_cast<double *>(sig + (STREAM ? 2 * kTB : capF + 32)) + kPad;        // pad | capP | pad
    unsigned short *pk_pos = reinterpret_cast<unsigned short *>(pk_score + F.capP + kPad) + kPad;     // pad | capP | pad
    unsigned char *pk_state = reinterpret_cast<unsigned char *>(pk_pos + F.capP + kPad) + kPad;       // pad | capP | pad
    FastShared &sh = *reinterpret_cast<FastShared *>(smem + (STREAM ? fast_stream_sh_offset(F.capP, NBT)
                                                                    : fast_sh_offset(capF, F.capP, NBT)));
    unsigned char *R = reinterpret_cast<unsigned char *>(pk_score - kPad);
    unsigned *hist = reinterpret_cast<unsigned *>(R);
    // kept peaks (after suppression) that leave room for hist_topk
    const int kept_cap = F.capP + kPad - kTopKHistBytes / 8;
    unsigned *hist_topk = reinterpret_cast<unsigned *>(pk_score + kept_cap);  // ends with pk_score's tail pad
    int *cpts = reinterpret_cast<int *>(R);                                    // kFSeg + 4
    unsigned *rankbuf = reinterpret_cast<unsigned *>(cpts + kFSeg + 4);        // 128
    double *ev = reinterpret_cast<double *>(rankbuf + 128);                    // kFSeg
    double *zz = ev + kFSeg;                                                   // kFSeg
    double *tmp = zz + kFSeg;                                                  // kFSeg
    unsigned long long *kept_key = reinterpret_cast<unsigned long long *>(pk_score);  // after suppression
    unsigned short *kept_pos = pk_pos;
    BlockEx bx(sh);

    // The hand-over lists are touched by a handful of reads per million: their pointers are re-read from the kernel
    // argument segment at the point of use (volatile: not hoisted) instead of occupying four SGPR pairs for the
    // whole kernel -- which the register allocator answered with scratch stores at every workgroup's entry
    // (4 KB of HBM writes per read).  Both kernels that inline this body take FastArgs as their only argument.
    auto karg = [&]() {
        return (const volatile FastArgs __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr();
    };
    auto to_slow = [&](int reason) {
        if (tid == 0) {
            unsigned *cnt = karg()->slow_count;
            int32_t *lst = karg()->slow_list;
            lst[atomicAdd(cnt, 1u)] = (int32_t)r;
            if (unsigned *h = karg()->a.dbg_reasons) atomicAdd(h + (reason & 15), 1u);   // (diagnostic runs only)
            if (PROF && r < A.prof_reads) A.prof[r * 32 + 13] = reason;
        }
    };
    auto to_retry_or = [&](int reason) {  // the exact-scores list kernel (unfiltered peak list, its largest capacity), else slow path
        int32_t *lst = karg()->retry_list;
        if (!lst) {
            to_slow(reason);
        } else if (tid == 0) {
            unsigned *cnt = karg()->retry_count;
            lst[atomicAdd(cnt, 1u)] = (int32_t)r;
            if (PROF && r < A.prof_reads) A.prof[r * 32 + 13] = 7;
        }
    };
    // a decision inside the error band: again with exact scores
    auto to_retry = [&]() { to_retry_or(7); };
    // capacity only: the next larger instantiation takes it; the last one of the chain hands a peak list that outgrew the
    // threshold-filtered capacity to the exact-scores launch (three times the entries) before the exact general kernel
    auto to_big = [&](int reason) {
        int32_t *lst = karg()->big_list;
        if (!lst) {
            to_retry_or(reason);
        } else if (tid == 0) {
            unsigned *cnt = karg()->big_count;
            lst[atomicAdd(cnt, 1u)] = (int32_t)r;
        }
    };
    auto fail = [&](int st) {
        for (int i = tid; i < K; i += FB) {
            if (A.fpt) A.fpt[r * K + i] = __builtin_nan("");
            if (A.dwell) A.dwell[r * K + i] = 0;
        }
        if (A.stats && tid < 6) A.stats[r * 6 + tid] = __builtin_nan("");
        if (tid == 0) A.status[r] = st;
    };

    // (the latency-bound ends of the workgroup -- the loads and medians of P0 / P1, the export, the one-wave stages of the
    // one-piece form -- issue ahead of the other workgroups' tile passes; the VALU-bound tile pass runs at the default priority)
    __builtin_amdgcn_s_setprio(WDX_TILE_PRIO);
    if constexpr (SPLIT) {
        // nothing exported yet: whatever way this workgroup leaves, the tail kernel must not take the slot's previous read
        if (tid == 0) reinterpret_cast<SplitHdr *>(F.split_ws + (size_t)blockIdx.x * kSplitRecBytes)->m = -1;   // (slot = workgroup of the slice)
    }
    // (the read's clip record is requested with the rest of its metadata -- one memory latency ahead of the samples' loads, not two:
    // behind the parameter checks below the compiler may not hoist the load, and P0 waited for it before it issued the samples')
    ClipRec cr_early{};
    if constexpr (EXT) cr_early = F.clip[r];
    if (A.ok && !A.ok[r]) {
        fail(WDX_READ_FAIL_DETECT);
        return;
    }
    // A0 extract_adapter
    const int64_t row_off = A.row_off ? A.row_off[r] : r * A.stride;
    const int64_t row_len = A.row_len ? (int64_t)A.row_len[r]
                                      : (A.row_off ? A.row_off[r + 1] - A.row_off[r] : A.stride);
    int64_t start = (int64_t)A.a_start[r] - P.padding;
    if (start < 0) start = 0;
    int64_t stop = (int64_t)A.a_end[r] + P.padding;
    if (stop > row_len) stop = row_len;
    const int64_t n64 = stop - start;
    // parameter shrink (sig_proc.py:526-533) -- the fast path only takes the un-shrunk common case
    bool fast = n64 >= 256 && n64 <= capF;
    const int n = (int)(fast ? n64 : 0);
    // (EXT, window resident: the samples' loads are issued HERE, ahead of the parameter checks' float64 divisions -- ~70 VALU
    // operations that every lane executes and the loads used to wait behind; a window the checks decline wastes its loads)
    struct __attribute__((packed, aligned(4))) F4Upre { float x, y, z, w; };
    F4Upre xpre[(EXT && !STREAM) ? NPT / 4 : 1];
    if constexpr (EXT && !STREAM) {
        if (fast) {   // block-uniform
            const float *__restrict__ srcp = A.sig + row_off + start;
            const unsigned last4p = (unsigned)(n - 4);
#pragma unroll
            for (int j = 0; j < NPT / 4; ++j) {
                const unsigned i = (unsigned)(j * FB + tid) * 4u;
                xpre[j] = *reinterpret_cast<const F4Upre *>(srcp + min(i, last4p));
            }
        }
    }
    int d_eff = 0;
    if (fast) {
        d_eff = rdiv_half_even((unsigned)n, 2u * (unsigned)E, A.e_magic2);   // (int)rint((double)n / (double)E / 2.0)
        if (P.min_obs_per_base < d_eff) d_eff = P.min_obs_per_base;
        int W = rdiv_half_even((unsigned)n, (unsigned)E, A.e_magic1);        // (int)rint((double)n / (double)E)
        if (P.running_stat_width < W) W = P.running_stat_width;
        fast = (W == FW) && d_eff >= 1 && d_eff <= 2 * kNBW + 1;
    }
    if (!fast) {
        if (n64 > capF) {
            if (!F.routed) to_big(0);   // (routed: listed ahead of this launch, sixty-four reads per atomic)
        } else {
            to_slow(0);
        }
        return;
    }
    const int ns = n - 2 * FW;
    WDX_FSTAMP(0);

    float lo, hi;
    double var_floor;  // approximate scores: smallest variance sum whose rounding error stays below 2^-27 relative
    if constexpr (EXT) {
        // P0 + clip: the bounds were computed by clip_bounds_kernel (one wave per read) ahead of this launch.  HBM ->
        // registers -> v_med3_f32 -> LDS: every thread writes its own four positions with their final values -- clipped
        // samples inside the window, zeros from n on (the event means add whole four-sample groups) -- so ONE barrier
        // ends the phase.  Loads are dword-aligned 16-byte loads clamped to the last whole group; a wave whose group
        // reaches past the window (one per read, and the groups beyond) shifts the clamped lanes' samples into place.
        const ClipRec cr = cr_early;
        if (cr.flag != CLIP_OK) {  // block-uniform
            to_slow(cr.flag == CLIP_NAN_NEG ? 1 : 2);
            return;
        }
        lo = cr.lo;
        hi = cr.hi;
        var_floor = kVarFloorC(FW) * (double)cr.cmax * (double)cr.cmax;
      if constexpr (STREAM) {
        // (the first tile's samples are loaded by the tile loop's prologue below)
      } else {
        const unsigned last4 = (unsigned)(n - 4);  // n >= 256
        const F4Upre (&x)[NPT / 4] = xpre;   // (requested ahead of the parameter checks, above)
        float4 *sig4w = reinterpret_cast<float4 *>(sig);
        const int wave_u = __builtin_amdgcn_readfirstlane(wave);
#pragma unroll
        for (int j = 0; j < NPT / 4; ++j) {
            const unsigned i = (unsigned)(j * FB + tid) * 4u;
            float e0 = __builtin_amdgcn_fmed3f(x[j].x, lo, hi), e1 = __builtin_amdgcn_fmed3f(x[j].y, lo, hi);
            float e2 = __builtin_amdgcn_fmed3f(x[j].z, lo, hi), e3 = __builtin_amdgcn_fmed3f(x[j].w, lo, hi);
            if ((unsigned)(j * FB + wave_u * 64 + 63) * 4u + 3u >= (unsigned)n) {  // wave-uniform, rare
                const int sft = (int)i - (int)last4;  // > 0: the load was clamped and holds samples n - 4 .. n - 1
                if (sft > 0) {
                    e0 = sft == 1 ? e1 : sft == 2 ? e2 : sft == 3 ? e3 : 0.0f;
                    e1 = sft == 1 ? e2 : sft == 2 ? e3 : 0.0f;
                    e2 = sft == 1 ? e3 : 0.0f;
                    e3 = 0.0f;
                }
            }
            sig4w[j * FB + tid] = make_float4(e0, e1, e2, e3);
        }
        if (tid < 32) {
            sig[capF + tid] = 0.0f;
            sh.rk[tid] = 0u;   // (the tile loop's hand-over words, below: nothing else uses rk before the loop has ended)
        }
        __syncthreads();
      }
        WDX_FSTAMP(1);
        WDX_FSTAMP(2);
    } else {
    // (the medians' histogram aliases the peak-list region: a launch whose list is too short for it is a host error --
    // the read goes to the exact kernel rather than through a histogram that overruns the exchange block)
    if ((size_t)(F.capP + 2 * kPad) * 11 < (size_t)(kHB + 64) * 4) {
        to_slow(0);
        return;
    }
    // P0: HBM -> LDS, four consecutive samples per lane and load (dword-aligned 16-byte global loads,
    // ds_write_b128), every load of the thread in flight together.  A group that is not entirely inside
    // the window is loaded from the last whole group instead (in bounds; duplicates cannot move the
    // extremes); the <= 3 samples of a ragged tail are patched in by three lanes.
    // NaN check and the key extremes of the samples (bounds for the radix selects) ride along.
    unsigned xkmin, xkmax;
    {
        struct __attribute__((packed, aligned(4))) F4U { float x, y, z, w; };
        const float *__restrict__ src = A.sig + row_off + start;
        const unsigned last4 = (unsigned)(n - 4);  // n >= 256
        F4U x[NPT / 4];
#pragma unroll
        for (int j = 0; j < NPT / 4; ++j) {
            const unsigned i = (unsigned)(j * FB + tid) * 4u;
            x[j] = *reinterpret_cast<const F4U *>(src + min(i, last4));
        }
        const int tail_i = (n & ~3) + tid;  // ragged tail (lanes 0..2 of wave 0)
        const bool tail = tid < 3 && tail_i < n;
        const float xt = tail ? src[tail_i] : 0.0f;
        // Extremes of the raw bit patterns as unsigned integers (v_min3_u32 / v_max3_u32: one VALU op per
        // sample): for non-negative samples the pattern orders like the value and its key is pattern | 2^31;
        // any negative sample (or a NaN of either sign) shows up as a maximum beyond +inf's pattern.
        unsigned umn = 0xffffffffu, umx = 0;
        float4 *sig4w = reinterpret_cast<float4 *>(sig);
#pragma unroll
        for (int j = 0; j < NPT / 4; ++j) {
            const unsigned i = (unsigned)(j * FB + tid) * 4u;
            const float e[4] = {x[j].x, x[j].y, x[j].z, x[j].w};
            const unsigned u0 = __float_as_uint(e[0]), u1 = __float_as_uint(e[1]), u2 = __float_as_uint(e[2]),
                           u3 = __float_as_uint(e[3]);
            umn = min(min(umn, u0), u1);
            umn = min(min(umn, u2), u3);
            umx = max(max(umx, u0), u1);
            umx = max(max(umx, u2), u3);
            // (stored as loaded: a group beyond the last whole one holds that group's samples again -- every consumer
            // tests indices against n, the ragged tail is patched below, the event means get their zeros after the clip)
            sig4w[j * FB + tid] = make_float4(e[0], e[1], e[2], e[3]);
            (void)i;
        }
        if (tid < 32) sig[capF + tid] = 0.0f;
        if (tail) {
            umn = min(umn, __float_as_uint(xt));
            umx = max(umx, __float_as_uint(xt));
        }
        unsigned unused, gumn, gumx;
        bx.minmaxsum(umn, umx, 0u, gumn, gumx, unused);
        if (gumx > 0x7f800000u) {  // block-uniform, rare: a negative sample or a NaN -> extremes in key order
            unsigned kmn = 0xffffffffu, kmx = 0;
#pragma unroll
            for (int j = 0; j < NPT / 4; ++j) {
                const float e[4] = {x[j].x, x[j].y, x[j].z, x[j].w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const unsigned key = f32_key(e[q]);
                    kmn = min(kmn, key);
                    kmx = max(kmx, key);
                }
            }
            if (tail) {
                const unsigned key = f32_key(xt);
                kmn = min(kmn, key);
                kmx = max(kmx, key);
            }
            bx.minmaxsum(kmn, kmx, 0u, xkmin, xkmax, unused);
        } else {
            xkmin = gumn | 0x80000000u;
            xkmax = gumx | 0x80000000u;
        }
        // the tail patch lands in a group another lane has zeroed: after the barrier above, and before
        // the one that precedes the first pass over the samples (fast_select's histogram reset)
        if (tail) sig[tail_i] = xt;
        // NaNs sort outside the infinities in key order: key(+NaN) > key(+inf), key(-NaN) < key(-inf)
        if (xkmax > f32_key(__builtin_inff()) || xkmin < f32_key(-__builtin_inff())) {
            to_slow(1);
            return;
        }
    }
    WDX_FSTAMP(1);

    // P1: MAD clip bounds (float32).  Every pass re-reads the thread's samples from LDS with
    // ds_read_b128 (a thread owns 4 consecutive samples per group), so a pass costs one LDS latency.
    {
        // xkmin/xkmax are order-preserving keys; a key below 0x80000000 is a negative sample (or -0.0)
        const bool neg = xkmin < 0x80000000u;  // block-uniform
        long long *pp = (PROF && r < A.prof_reads) ? A.prof + r * 32 + 16 : nullptr;
        const unsigned sig_off = (unsigned)(reinterpret_cast<unsigned char *>(sig) - smem);
        const unsigned hist_off = (unsigned)(reinterpret_cast<unsigned char *>(hist) - smem);
        const unsigned sh_off = (unsigned)(reinterpret_cast<unsigned char *>(&sh) - smem);
        const int stop_sub = (PROF && A.stop_phase > 20) ? A.stop_phase - 20 : 0;
        MedRet mr = neg ? fast_median_lds<2>(sig_off, n, 0.0f, 0, xkmin, xkmax, hist_off, sh_off, bx.par, pp,
                                                stop_sub)
                        : fast_median_lds<0>(sig_off, n, 0.0f, 0, xkmin & 0x7fffffffu,
                                                 xkmax & 0x7fffffffu, hist_off, sh_off, bx.par, pp, stop_sub);
        if (stop_sub) return;
        bx.par = mr.par;
        const float med = mr.v;
        WDX_FSTAMP(2);
        // |x - med| is monotone in x on either side of med, and rounding is monotone, so its largest
        // value is attained at one of the data extremes; 0 bounds it from below
        const float dmax = fmaxf(fabsf(key_f32(xkmin) - med), fabsf(key_f32(xkmax) - med));
        // (no closing barrier: the one after the clip pass below also separates this select from the next)
        mr = fast_median_lds<1>(sig_off, n, med, 1, 0u, __float_as_uint(dmax), hist_off, sh_off, bx.par, nullptr, 0,
                                false);
        bx.par = mr.par;
        const float mad = mr.v;
        clip_bounds(P, med, mad, lo, hi);
        // Event-mean sums are order-independent iff every partial sum of <= n samples is exactly
        // representable in float64: all clipped samples are multiples of ulp32(min |x|) and any partial
        // sum is below n * 2^(exp(max|x|)+1).  The clipped extremes follow from the data extremes; a
        // clipped range that reaches zero or below gives no lower bound on |x| -> slow path.
        const float cmin = __builtin_amdgcn_fmed3f(key_f32(xkmin), lo, hi);
        const float cmax = __builtin_amdgcn_fmed3f(key_f32(xkmax), lo, hi);
        bool exact = (lo == lo) && (hi == hi) && lo <= hi && cmin > 0.0f && cmax < 3.0e38f;
        if (exact) {
            int fa = (int)(__float_as_uint(cmin) >> 23), fb = (int)(__float_as_uint(cmax) >> 23);
            if (fa == 0) fa = 1;
            exact = (fb - fa) + (32 - __clz(n)) <= 28;
        }
        if (!exact) {  // block-uniform
            to_slow(2);
            return;
        }
        var_floor = kVarFloorC(FW) * (double)cmax * (double)cmax;
        // The clip as ONE in-place pass (np.clip == v_med3_f32 for lo <= hi and no NaN): the tile's lanes read every
        // sample three times and the event means once more -- four clips per sample on the fly against one here, and
        // the pass's barrier stands in for the one the select above would have ended with.
        {
            float4 *s4 = reinterpret_cast<float4 *>(sig);
#pragma unroll
            for (int j = 0; j < NPT / 4; ++j) {
                float4 v = s4[j * FB + tid];
                v.x = __builtin_amdgcn_fmed3f(v.x, lo, hi);
                v.y = __builtin_amdgcn_fmed3f(v.y, lo, hi);
                v.z = __builtin_amdgcn_fmed3f(v.z, lo, hi);
                v.w = __builtin_amdgcn_fmed3f(v.w, lo, hi);
                s4[j * FB + tid] = v;
            }
        }
        __syncthreads();
        // (zeros behind the data: the event means add whole four-sample groups; made visible by the barriers of the
        // tile loop, long before P6)
        if (tid < 24) sig[n + tid] = 0.0f;
        // hist (aliasing the peak list) is dead from here on (the median routine ends with a barrier)
    }
    }
    __builtin_amdgcn_s_setprio(0);
    WDX_FSTAMP(3);

    // P2 + P3a: t-scores tile by tile; strict local maxima are appended in position order.
    // A wave covers 64 lanes x kR consecutive window starts; scores exist for lanes 0 .. 63 - kShift (the
    // statistics of window pos + 12 come from lane + kShift).  Lanes 1 .. kOwn own their positions; lane 0
    // and lane kOwn + 1 are halos whose scores only serve as the neighbours' left / right values, so a wave
    // never needs another wave's scores: ONE barrier per tile (the ordered append) -- and none where the list length in front of
    // a wave comes from the wave before it (kChain, below).
    // P2..P4 run on approximate score keys (a third of the exact statistics' float64 operations) with every order
    // decision taken only outside an error band.  A wave whose tile has neighbouring positions inside the band
    // (ties, plateaus, flat windows) falls back to exact scores for that tile; a read with a suppression or top-E
    // decision inside the band (about two per thousand) is listed and redone by a launch with a.exact_scores set,
    // which runs the same code on the reference's exact scores.  (Repeating P2..P4 in place was tried first: the
    // loop's back edge kept ~40 more registers live and cost the fifth resident workgroup per CU.)
    unsigned nk;
    unsigned long long T = 0;
    int np, nms_iters = 0;
    // byte addresses of the tile's three lane shuffles (ds_bpermute; __shfl_* semantics: the own lane past the wave's
    // end), computed once: inside the tile loop the compiler re-derived them every iteration
    const int a_dnS = (lane + kShiftW < 64 ? lane + kShiftW : lane) << 2;
    int a_dnB[kShiftW];  // lanes + 1 .. + kShiftW - 1: the other blocks of a lane's first window ([0] unused)
#pragma unroll
    for (int b = 0; b < kShiftW; ++b) a_dnB[b] = (lane + b < 64 ? lane + b : lane) << 2;
    auto dpp_shift = [](double x, auto ctrl) __attribute__((always_inline)) -> double {
        const long long b = __double_as_longlong(x);
        // (bound_ctrl: the lane without a source reads zero -- no `old` operand to set up)
        const unsigned lo_ = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, decltype(ctrl)::value, 0xf, 0xf, true);
        const unsigned hi_ = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), decltype(ctrl)::value, 0xf, 0xf, true);
        return __longlong_as_double((long long)(((unsigned long long)hi_ << 32) | lo_));
    };
    auto dpp_from_lane_below = [&](double x) __attribute__((always_inline)) { return dpp_shift(x, std::integral_constant<int, 0x138>{}); };  // wave_shr:1
    auto dpp_from_lane_above = [&](double x) __attribute__((always_inline)) { return dpp_shift(x, std::integral_constant<int, 0x130>{}); };  // wave_shl:1
    auto bperm = [](int addr, double x) -> double {
        const long long b = __double_as_longlong(x);
        const unsigned lo = (unsigned)__builtin_amdgcn_ds_bpermute(addr, (int)(unsigned)b);
        const unsigned hi = (unsigned)__builtin_amdgcn_ds_bpermute(addr, (int)(unsigned)(b >> 32));
        return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    };
    const bool exact_sc = kExactOnly || A.exact_scores != 0;
    // the partner window's lane for the exact-only widths: FW / kR or FW / kR + 1 lanes further (a_dnS is the latter)
    const int a_dnS0 = (lane + FW / kR < 64 ? lane + FW / kR : lane) << 2;
    np = 0;
    // the threshold filter of the appends (kPeakTauLo): approximate keys only -- the exact-scores launch is the unfiltered one
    const bool pre_ok = !exact_sc && A.peak_filter != 0;
    {
        const double c12 = 1.0 / (double)FW;  // (named for the width it was first written for)
        int slow = 0;
        // STREAM: thread tid owns samples [6 tid, 6 tid + 6) of a tile buffer, which holds the window's samples
        // [t0 - kR, t0 - kR + kTB) -- clipped, zero outside the window.  Three 8-byte loads (dword-aligned), clamped into
        // the window; requested one tile ahead.
        struct __attribute__((packed, aligned(4))) F2U { float x, y; };
        const float *__restrict__ ssrc = A.sig + row_off + start;
        auto stream_load = [&](int tb0, F2U (&v)[3]) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int i = tb0 + 6 * tid + 2 * q;
                v[q] = *reinterpret_cast<const F2U *>(ssrc + max(0, min(i, n - 2)));
            }
        };
        auto stream_store = [&](int tb0, const F2U (&v)[3], float *buf) {
            float2 *b2 = reinterpret_cast<float2 *>(buf + 6 * tid);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int i = tb0 + 6 * tid + 2 * q;  // (even: both elements clamp together unless i == n - 1 / i == -1)
                const int ic = max(0, min(i, n - 2));
                float e0 = __builtin_amdgcn_fmed3f(v[q].x, lo, hi), e1 = __builtin_amdgcn_fmed3f(v[q].y, lo, hi);
                if (ic != i) {  // clamped: the pair holds samples ic, ic + 1
                    e0 = (i == ic + 1 && i < n) ? e1 : 0.0f;   // i = n - 1: the pair loaded is (n - 2, n - 1)
                    e1 = (i + 1 == ic && i + 1 >= 0) ? __builtin_amdgcn_fmed3f(v[q].x, lo, hi) : 0.0f;  // i = -1: (0, 1)
                }
                b2[q] = make_float2(e0, e1);
            }
        };
        if constexpr (STREAM) {
            F2U v0[3];
            stream_load(-kR, v0);
            stream_store(-kR, v0, sig);
            __syncthreads();
        }
        int tix = 0;
        constexpr bool kChain = EXT && !STREAM;   // (see the ordered append below)
        static_assert(!kChain || (capF + kTSW - 1) / kTSW <= 32 / kWaves, "one hand-over word per wave and tile in sh.rk");
        unsigned chain_end = 0;
        // the band's constants in two vector pairs for the whole loop (opaque to the compiler, which otherwise rebuilds the
        // addend with two v_mov_b32 in front of each v_fmac_f64: 16 of a wave tile's 224 VALU instructions) -- where the
        // registers allow it: the width-18 kernel at six workgroups per CU has none to spare
        constexpr bool kBandRegs = !(FW == 18 && NBT == 1);
        double band_hi_s = kBandHi, band_abs_v = kBandAbs;
        if constexpr (kBandRegs) {
            asm volatile("" : "+v"(band_hi_s));
            asm volatile("" : "+v"(band_abs_v));
        }
        for (int t0 = 0; t0 < ns; t0 += kTSW, ++tix) {
            const int ub = wave * (kR * kOwnW) + (lane - 1) * kR;  // first tile-local position of this lane (halo: -kR)
            const int q0 = t0 + ub;
            // STREAM: this tile's buffer, addressed by the sample's index in the window; the next tile's samples are
            // requested now and written to the other buffer once this tile has been scored (before its barrier)
            const float *sigt = STREAM ? sig + (tix & 1) * kTB - (t0 - kR) : sig;
            F2U vnx[3];
            const bool more = STREAM && t0 + kTSW < ns;  // block-uniform
            if constexpr (STREAM) {
                if (more) stream_load(t0 + kTSW - kR, vnx);
            }
            // a wave whose positions all lie past the end of the scores (last tile) skips the arithmetic
            const bool wave_active = t0 + wave * (kR * kOwnW) < ns;
            unsigned mine = 0;
            // plateau peaks: 4-bit position offsets per rr (zero otherwise; at most 11 from the walk in registers); 15 = the one
            // plateau per lane that ran on beyond the following kReach lanes: its offset (<= 189) sits in the top byte
            unsigned padj = 0;
            // pkm[rr]: the lanes whose slot rr is a peak, as WAVE masks (scalar registers): a v_cmp writes one, their
            // combination is scalar work, and the appends below use them as execution masks directly -- as a per-lane
            // bit mask the peaks cost a v_cndmask + v_or per slot to build and a v_and + v_cmp per slot to test again
            unsigned long long pkm[kR];
#pragma unroll
            for (int rr = 0; rr < kR; ++rr) pkm[rr] = 0ull;
            double sc[kR];
            bool wave_plateau = false;
            if (wave_active) {
                const bool lane_own = lane >= 1 && lane <= kOwnW;
                constexpr unsigned long long own_mask = ((1ull << kOwnW) - 1ull) << 1;  // lanes 1 .. kOwnW
                const int lim_lo = lane_own ? 1 - q0 : kR;        // rr >= lim_lo  <=>  pos >= 1
                const int lim_hi = lane_own ? ns - 2 - q0 : -1;    // rr <= lim_hi  <=>  pos <= ns - 2
                // every owned position of this wave inside [1, ns - 2] (all but the first and last tiles'
                // edge waves): the per-slot position tests reduce to lane ownership (wave-uniform choice)
                const int w_first = t0 + wave * (kR * kOwnW);
                const bool interior = w_first >= 1 && w_first + kR * kOwnW - 1 <= ns - 2;
                double left, right;
                // One pass over the wave's positions: window statistics, scores (EX: the reference's operations;
                // else approximate keys), strict local maxima as lane predicates (the compiler keeps them as wave
                // masks in SGPRs).  Returns the lanes with a rising edge into equal scores (EX: a plateau,
                // resolved below) / with a neighbour pair of an owned position inside the band (keys: a doubt).
                auto pass = [&](auto ex_t) -> unsigned long long {
                    constexpr bool EX = decltype(ex_t)::value;
                    // the lane's kR + 11 (+1 pad) samples, loaded by the pass itself (a fall-back pass reads them
                    // again) so that they are dead once the window statistics exist.  Unconditional, index-clamped
                    // loads (halo lanes before the first sample and lanes past the data only feed unused positions):
                    // all of them in flight, one wait
                    // (STREAM: every lane's kR + FW samples lie inside the tile buffer: no clamp)
                    // (odd widths load one sample more than they use: the pairs are eight-byte loads)
                    constexpr int kLd = (kR + FW + 1) / 2 * 2;
                    const int qc = STREAM ? q0 : max(0, min(q0, capF + 32 - kLd));  // the sample array ends at capF + 32
                    const float2 *s2p = reinterpret_cast<const float2 *>(sigt + qc);
                    double xx[EX ? kLd : 2 * kR];
                    double M[kR], V[kR];
                    unsigned long long pz[kR];  // approximate pass: lanes whose slot rr has an untrusted variance sum
                    if constexpr (!EX) {
                        // approximate keys: exact sliding sums S1 (see below), fused sliding sums of squares S2
                        // (<= 24 roundings of <= u * 12 max|x|^2), V = S2 - S1^2 / 12, key = (S1 - S1')^2 / (V + V')
                        // by v_rcp_f64 + one Newton step (2^-48); a variance sum below var_floor is untrusted (wave mask
                        // pz: a doubt at every owned position whose own or neighbouring key it is).
                        // A lane loads its own six samples and the six that slide in (they are lane + 2's own); the
                        // first window is the lane's block plus lane + 1's, whose block sums come by shuffle -- 12
                        // conversions and 13 additions where the 18-sample window took 18 and 23.  (A lane whose
                        // loads were clamped feeds no position that is used, nor does its neighbour's use of it.)
                        // (general FW: the first window is the sum of the blocks of kShiftW consecutive lanes, the
                        // samples that slide in are lane + kShiftW's own)
#pragma unroll
                        for (int j = 0; j < kR / 2; ++j) {
                            const float2 v = s2p[j], w = s2p[FW / 2 + j];  // samples q0 + 2j.., q0 + FW + 2j..
                            xx[2 * j] = (double)v.x;  // (clipped in place after P1)
                            xx[2 * j + 1] = (double)v.y;
                            xx[kR + 2 * j] = (double)w.x;
                            xx[kR + 2 * j + 1] = (double)w.y;
                        }
                        double b1 = xx[0], b2 = xx[0] * xx[0];
#pragma unroll
                        for (int k = 1; k < kR; ++k) {
                            b1 += xx[k];
                            b2 = __builtin_fma(xx[k], xx[k], b2);
                        }
                        double s1 = b1, s2 = b2;
#pragma unroll
                        for (int b = 1; b < kShiftW; ++b) {  // (FW = 12: one neighbour, by a DPP wave shift)
                            s1 += b == 1 ? dpp_from_lane_above(b1) : bperm(a_dnB[b], b1);
                            s2 += b == 1 ? dpp_from_lane_above(b2) : bperm(a_dnB[b], b2);
                        }
#pragma unroll
                        for (int rr = 0; rr < kR; ++rr) {
                            if (rr > 0) {
                                s1 = (s1 - xx[rr - 1]) + xx[kR + rr - 1];
                                s2 = __builtin_fma(xx[kR + rr - 1], xx[kR + rr - 1],
                                                   __builtin_fma(-xx[rr - 1], xx[rr - 1], s2));
                            }
                            M[rr] = s1;
                            V[rr] = __builtin_fma(-(s1 * c12), s1, s2);
                        }
#pragma unroll
                        for (int rr = 0; rr < kR; ++rr) {
                            const double m2 = bperm(a_dnS, M[rr]);
                            const double v2 = bperm(a_dnS, V[rr]);
                            const double vs = V[rr] + v2;
                            const double dm = M[rr] - m2;
                            const double rc = __builtin_amdgcn_rcp(vs);   // (2^29 ulp: inside the band without a Newton step)
                            sc[rr] = (dm * dm) * rc;
                            pz[rr] = __ballot(!(vs >= var_floor));  // untrusted (also a NaN): a doubt wherever it is used
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < kLd / 2; ++j) {
                            const float2 v = s2p[j];
                            xx[2 * j] = (double)v.x;  // (clipped in place after P1)
                            xx[2 * j + 1] = (double)v.y;
                        }
                        // Window sums: the fast path has established that every partial sum of the clipped samples
                        // is exactly representable in float64 (see P1), so the first sum in the reference's order
                        // and the next ones by sliding (S - x[out] + x[in]) are the same numbers.
                        double wsum = 0.0;
#pragma unroll
                        for (int k = 0; k < FW; ++k) wsum += xx[k];
#pragma unroll
                        for (int rr = 0; rr < kR; ++rr) {
                            if (rr > 0) wsum = (wsum - xx[rr - 1]) + xx[rr + FW - 1];
                            const double s = wsum;
                            double m;
                            if constexpr (FW == 12) {
                                const double q = s * c12;
                                const double rem = __builtin_fma(-12.0, q, s);
                                m = __builtin_fma(rem, c12, q);  // == s / 12.0, correctly rounded
                            } else {
                                m = fast_div_mid(s, (double)FW);  // the compiler's correctly rounded quotient (unscaled form)
                            }
                            double v = 0.0;
#pragma unroll
                            for (int k = 0; k < FW; ++k) {
                                const double df = xx[rr + k] - m;
                                v += df * df;
                            }
                            M[rr] = m;
                            V[rr] = v;
                        }
                        // exact scores |dm| / sqrt(vs) (the reference's operations) for the lane's positions
#pragma unroll
                        for (int rr = 0; rr < kR; ++rr) {
                            // the statistics of window (pos + FW): slot rs of the lane la lanes further (multiples of six: the
                            // same slot, kShiftW lanes further)
                            const int rs = (rr + FW) % kR;
                            const bool far = (rr + FW) / kR > FW / kR;   // (compile-time after unrolling)
                            const int addr = kExactOnly ? (far ? a_dnS : a_dnS0) : a_dnS;
                            const double m2 = bperm(addr, M[kExactOnly ? rs : rr]);
                            const double v2 = bperm(addr, V[kExactOnly ? rs : rr]);
                            const double vs = V[rr] + v2;
                            const double dm = fabs(M[rr] - m2);
                            // vs == 0 (two flat windows): the reference's score is 0; the unscaled sequences give
                            // rsq(0) = inf -> 0 * inf = NaN -> NaN all the way, and v_max_f64(NaN, 0) = 0 (IEEE
                            // maxNum), while every regular quotient is >= 0 and passes unchanged: one instruction
                            sc[rr] = max0_f64(fast_div_mid(dm, fast_sqrt_mid(vs)));
                        }
                    }
                    // neighbours' scores by lane shuffles only (halo lanes)
                    // (the lanes next door by DPP wave shifts -- VALU moves, no LDS round trip; lane 0's left and lane 63's
                    // right read zero: halo lanes, whose results are not used)
                    left = dpp_from_lane_below(sc[kR - 1]);
                    right = dpp_from_lane_above(sc[0]);
                    // One lt / gt pair per adjacent pair of scores (7 pairs) serves both neighbours; the position
                    // tests collapse into one compare per slot against a per-lane window [lim_lo, lim_hi] of
                    // admissible rr (empty for the halo lanes).
                    // The compares as wave masks (a v_cmp writes one): their combination is scalar ALU work, and each slot's
                    // result stays a wave mask (pkm[rr]) all the way to the appends
                    unsigned long long lt[kR + 1], gt[kR + 1];  // pair j: (e[j-1], e[j]) with e[-1] = left, e[kR] = right
                    if constexpr (EX) {
#pragma unroll
                        for (int j = 0; j <= kR; ++j) {
                            const double a = j ? sc[j - 1] : left;
                            const double b = j < kR ? sc[j] : right;
                            lt[j] = __ballot(a < b);
                            gt[j] = __ballot(a > b);
                        }
                    } else {  // certainly lower / certainly higher; neither = doubt
                        double hb[kR + 2];
                        // (the band's constants from registers: one v_fma_f64 per product)
                        hb[0] = __builtin_fma(left, band_hi_s, band_abs_v);
#pragma unroll
                        for (int j = 0; j < kR; ++j) hb[j + 1] = __builtin_fma(sc[j], band_hi_s, band_abs_v);
                        hb[kR + 1] = __builtin_fma(right, band_hi_s, band_abs_v);
#pragma unroll
                        for (int j = 0; j <= kR; ++j) {
                            const double a = j ? sc[j - 1] : left;
                            const double b = j < kR ? sc[j] : right;
                            lt[j] = __ballot(hb[j] < b);
                            gt[j] = __ballot(a > hb[j + 1]);
                        }
                    }
                    unsigned long long flag = 0;
                    auto detect = [&](auto inner) {
#pragma unroll
                        for (int rr = 0; rr < kR; ++rr) {
                            const unsigned long long inr =
                                decltype(inner)::value ? own_mask : __ballot(rr >= lim_lo && rr <= lim_hi);
                            const unsigned long long rising = inr & lt[rr];
                            pkm[rr] = rising & gt[rr + 1];
                            if constexpr (EX) {
                                flag |= rising & ~(lt[rr + 1] | gt[rr + 1]);
                            } else {  // (a neighbouring lane's mask is one shift away)
                                const unsigned long long bad = pz[rr] | (rr ? pz[rr - 1] : pz[kR - 1] << 1) |
                                                               (rr < kR - 1 ? pz[rr + 1] : pz[0] >> 1);
                                flag |= inr & (bad | ~((lt[rr] | gt[rr]) & (lt[rr + 1] | gt[rr + 1])));
                            }
                        }
                    };
                    if (__builtin_amdgcn_readfirstlane((int)interior)) detect(std::true_type{});
                    else detect(std::false_type{});
                    return flag;
                };
                // Approximate keys first; a wave with a doubt among its own positions (ties and plateaus of flat,
                // clipped stretches mostly) classifies its tile again from exact scores and appends their keys
                // 144 t^2 (two roundings: inside every band)
                bool wave_exact = exact_sc;
                if constexpr (!kExactOnly) {
                    if (!wave_exact) wave_exact = pass(std::false_type{}) != 0;  // wave-uniform
                }
                if (PROF && wave_exact && !exact_sc && lane == 0 && r < A.prof_reads)
                    atomicAdd(reinterpret_cast<unsigned long long *>(A.prof + r * 32 + 25), 1ull);
                bool plateau = false;
                if (wave_exact) {
                    const unsigned long long pl = pass(std::true_type{});
                    wave_plateau = pl != 0;
                    plateau = __builtin_amdgcn_inverse_ballot_w64(pl);
                }
                if (wave_plateau) {
                    // Rare (wave-uniform branch): scipy's _local_maxima_1d plateau rule -- walk to the first
                    // different score; a peak iff that one is lower, at the plateau's midpoint.  The walk
                    // sees the lane's own scores and those of the following kReach lanes in registers; a plateau that
                    // runs on (2 W equal scores around one unclipped sample inside a long clipped stretch, say) is followed
                    // lane by lane through shuffles below; one that leaves this wave's scores goes to the slow path.
                    double nx[kReach * kR];
                    int avail = kReach * kR;  // following scores this lane knows
#pragma unroll
                    for (int h = 1; h <= kReach; ++h) {
#pragma unroll
                        for (int q = 0; q < kR; ++q) nx[(h - 1) * kR + q] = __shfl_down(sc[q], h);
                        if (lane + h > 63 - kShiftW && avail > (h - 1) * kR) avail = (h - 1) * kR;  // no scores there
                    }
                    unsigned pm = 0;  // (this rare path works on the lane's own bits: bit rr = slot rr is a peak)
#pragma unroll
                    for (int rr = 0; rr < kR; ++rr) pm |= __builtin_amdgcn_inverse_ballot_w64(pkm[rr]) ? 1u << rr : 0u;
                    // (the slot whose walk ran through every score in registers waits in padj's top byte, 0x80 | slot -- no
                    // register of its own in this loop; such a walk has seen every position up to q0 + (kReach + 1) kR - 1)
                    if (plateau) {
                        int covered = -0x7fffffff;  // positions up to here belong to a resolved plateau
#pragma unroll
                        for (int rr = 0; rr < kR; ++rr) {
                            const int pos = q0 + rr;
                            pm &= ~(1u << rr);
                            if (lane_own && pos >= 1 && pos <= ns - 2 && pos > covered) {
                                const double a = rr ? sc[rr - 1] : left;
                                const double c = rr < kR - 1 ? sc[rr + 1] : right;
                                const double b = sc[rr];
                                if (a < b && c <= b) {
                                    int ia = pos + 1;
                                    double val = c;
                                    bool stop = !(c == b), known = true;
                                    // (dynamic index into [sc | nx] through a select chain: this branch is
                                    // rare and must stay small in the instruction cache)
#pragma unroll 1
                                    for (int idx = rr + 1; idx < (kReach + 1) * kR && !stop; ++idx) {
                                        known = idx < kR + avail;
                                        double v = sc[0];
#pragma unroll
                                        for (int j = 1; j < kR; ++j) v = idx == j ? sc[j] : v;
#pragma unroll
                                        for (int j = 0; j < kReach * kR; ++j) v = idx == kR + j ? nx[j] : v;
                                        if (known && ia < ns - 1 && v == b) {
                                            ++ia;
                                        } else {
                                            stop = true;
                                            val = v;
                                        }
                                    }
                                    if (!stop && known) {   // equal all the way: the lanes further on decide (below)
                                        padj |= (0x80u | (unsigned)rr) << 24;
                                    } else if (!stop || !known) {
                                        slow |= 1;
                                    } else if (val < b) {
                                        pm |= 1u << rr;   // recorded at the plateau's midpoint
                                        padj |= (unsigned)(((pos + ia - 1) / 2) - pos) << (4 * rr);
                                    }
                                    covered = (padj >> 31) ? 0x7ffffff0 : ia - 1;   // (a pending plateau holds the lane's later slots)
                                }
                            }
                        }
                    }
                    if (__ballot((padj >> 31) != 0u)) {  // (wave-uniform, rarer still)
                        // no register of its own here either (the tile loop's state stays live across this block): bit 31 of
                        // padj = still walking, bits 30:29 = how it ended (1 on a lower score: a peak, 2 not a peak, 3 left the
                        // wave's scores), bits 26:24 = the slot; the positions walked beyond the registers count up in pm >> 8
#pragma unroll 1
                        for (int h = kReach + 1; h < 64 && __ballot((padj >> 31) != 0u); ++h) {
                            const bool have = lane + h <= 63 - kShiftW;  // that lane has scores
#pragma unroll 1
                            for (int q = 0; q < kR; ++q) {  // (one slot at a time, picked through a select chain)
                                double own = sc[0];
#pragma unroll
                                for (int j = 1; j < kR; ++j) own = q == j ? sc[j] : own;
                                const double nq = __shfl_down(own, h);
                                const int pend = (int)((padj >> 24) & 7u);
                                double b = sc[0];   // (the plateau's score, picked again: not held across the shuffle)
#pragma unroll
                                for (int j = 1; j < kR; ++j) b = pend == j ? sc[j] : b;
                                if (padj >> 31) {
                                    const int ia = q0 + (kReach + 1) * kR + (int)(pm >> 8);   // the position nq belongs to
                                    if (!have) padj = (padj & 0x7fffffffu) | (3u << 29);
                                    else if (ia < ns - 1 && nq == b) pm += 1u << 8;
                                    else padj = (padj & 0x7fffffffu) | ((nq < b ? 1u : 2u) << 29);
                                }
                            }
                        }
                        const unsigned endst = (padj >> 29) & 7u;   // 4..7: still walking at the wave's last lane
                        if (endst >= 3u) {
                            slow |= 1;
                        } else if (endst == 1u) {
                            const int pend = (int)((padj >> 24) & 7u);
                            const int ia = q0 + (kReach + 1) * kR + (int)(pm >> 8);
                            padj = (padj & 0x00ffffffu) | (15u << (4 * pend)) | ((unsigned)(((q0 + pend + ia - 1) / 2) - (q0 + pend)) << 24);
                            pm |= 1u << pend;
                        }
                        if (endst != 1u) padj &= 0x00ffffffu;
                        pm &= 0xffu;
                    }
#pragma unroll
                    for (int rr = 0; rr < kR; ++rr) pkm[rr] = __ballot((pm >> rr) & 1u);
                }
                if (wave_exact && !exact_sc) {  // (wave-uniform) exact scores into the key domain
#pragma unroll
                    for (int rr = 0; rr < kR; ++rr) sc[rr] = (sc[rr] * sc[rr]) * (double)(FW * FW);
                }
                if (pre_ok) {  // (block-uniform) the threshold filter: one compare per slot, folded into the wave masks
#pragma unroll
                    for (int rr = 0; rr < kR; ++rr) pkm[rr] &= __ballot(sc[rr] >= kPeakTauLo);
                }
#pragma unroll
                for (int rr = 0; rr < kR; ++rr) mine += __builtin_amdgcn_inverse_ballot_w64(pkm[rr]) ? 1u : 0u;
            }
            if constexpr (STREAM) {
                if (more) stream_store(t0 + kTSW - kR, vnx, sig + ((tix + 1) & 1) * kTB);
            }
            // (a wave that has scored its tile goes first: the others of its workgroup wait for it at the scan's barrier)
            // The ordered append needs the number of peaks in front of this wave's -- nothing else of the other waves.
            // kChain (window resident, bounds from the clip record: the large batches' kernels): NO barrier per tile.  A wave
            // takes the list length in front of it from the hand-over word of the wave before it in position order (wave w - 1 of
            // this tile, the last wave of the tile before for wave 0), adds its own count and hands that on; it waits only if
            // that ONE wave has not scored its tile yet, and runs ahead into its next tile otherwise (a word holds length + 1,
            // zero = not yet; every wave of the workgroup is resident and the wait chain ends at wave 0 of tile 0: no deadlock).
            // Measured with per-wave list segments as the barrier-free bound: 4.38 -> 4.08 ms per 524 288 reads.
            unsigned o_first;
            bool room;
            if constexpr (kChain) {
                const unsigned incl = wave_incl_scan_u32(mine);
                const unsigned tw = (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
                unsigned base = 0;
                if (tix != 0 || wave != 0) {
                    unsigned *src = &sh.rk[wave ? tix * kWaves + wave - 1 : (tix - 1) * kWaves + kWaves - 1];
                    unsigned v;
                    while ((v = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) == 0u) {}
                    base = (unsigned)__builtin_amdgcn_readfirstlane((int)v) - 1u;
                }
                if (lane == 0) __hip_atomic_store(&sh.rk[tix * kWaves + wave], base + tw + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                room = base + tw <= (unsigned)F.capP;   // (wave-uniform; the list lengths grow from wave to wave: voted on below)
                o_first = base + incl - mine;
                chain_end = base + tw;
            } else {
                __builtin_amdgcn_s_setprio(1);
                unsigned total;
                const unsigned off = bx.scan(mine, total);
                room = np + (int)total <= F.capP;   // capacity, not a property of the read (np and total are block-uniform)
                o_first = (unsigned)np + off;
                np += (int)total;
            }
            if (!room) {
                slow |= 2;
            } else if (wave_active) {
                // predicated appends: slot = running count of this lane's earlier peaks; the wave masks are the execution
                // masks.  (The plateau path's position offsets live in a body of their own: wave-uniform, rare.)
                unsigned o = o_first;
                if (!wave_plateau) {
#pragma unroll
                    for (int rr = 0; rr < kR; ++rr) {
                        const bool pk = __builtin_amdgcn_inverse_ballot_w64(pkm[rr]);
                        if (pk) {
                            pk_pos[o] = (unsigned short)(q0 + rr);
                            pk_score[o] = sc[rr];
                        }
                        o += pk ? 1u : 0u;
                    }
                } else {
#pragma unroll
                    for (int rr = 0; rr < kR; ++rr) {
                        const bool pk = __builtin_amdgcn_inverse_ballot_w64(pkm[rr]);
                        if (pk) {
                            const unsigned f4 = (padj >> (4 * rr)) & 15u;
                            pk_pos[o] = (unsigned short)(q0 + rr + (int)(f4 == 15u ? padj >> 24 : f4));
                            pk_score[o] = sc[rr];
                        }
                        o += pk ? 1u : 0u;
                    }
                }
            }
            if constexpr (!kChain) __builtin_amdgcn_s_setprio(0);
        }
        // sentinels around the list (-inf: never outranks, never inside a band) stand in for the index-range tests of
        // the suppression's neighbour windows
        if constexpr (kChain) {
            // (the last wave of the last tile knows the list's length: it writes the sentinels, ahead of the vote's barrier)
            if (wave == kWaves - 1 && !(slow & 2) && lane < 2 * kPad)
                pk_score[lane < kPad ? lane - kPad : (int)chain_end + lane - kPad] = -__builtin_inf();
            // (this vote's barrier is also what orders the appends before the reads of the list; capacity is a wave's finding here)
            unsigned d0_, any1, any2;
            bx.minmaxsum(0u, (unsigned)(slow & 1), (unsigned)(slow & 2), d0_, any1, any2);
            np = (int)(__hip_atomic_load(&sh.rk[(tix - 1) * kWaves + kWaves - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) - 1u);
            slow = (any1 ? 1 : 0) | (any2 ? 2 : 0);
            if (slow & 1) {
                to_slow(3);
                return;
            }
        } else {
        if (tid < 2 * kPad && !(slow & 2)) pk_score[tid < kPad ? tid - kPad : np + tid - kPad] = -__builtin_inf();  // (np <= capP)
        // (this vote's barrier is also what orders the last tile's appends before the suppression's reads of the list)
        if (bx.any((slow & 1) != 0)) {
            to_slow(3);
            return;
        }
        }
        if (slow & 2) {
            to_big(3);
            return;
        }
    }
    // > 0: the appends were filtered; every dropped peak's key lies below kPeakTauLo, tau_hi = the band above it
    const double tau_hi = pre_ok ? __builtin_fma(kPeakTauLo, kBandHi, kBandAbs) : 0.0;
    WDX_FSTAMP(4);

    __builtin_amdgcn_s_setprio(WDX_TILE_PRIO);
    if constexpr (SPLIT) {
        // The workgroup ends here.  What follows the tile pass -- suppression, top-E, boundaries, event means, normalisation --
        // is one wave's work with three waves waiting (16 k of this workgroup's 42 k cycles, during which its 26.8 KB of LDS
        // hold one read that no longer needs them): fingerprint_split_tail_kernel does it, one wave per read at ten times the
        // occupancy, from what is exported here: the <= 256 peaks that can matter, each with the prefix sum of the clipped
        // samples at the boundary it would become (P6's chunk sums and scan, evaluated at the peaks instead of at the
        // boundaries -- every partial sum is exact, so an event's sum is the difference of two of them).
        unsigned char *rec = F.split_ws + (size_t)blockIdx.x * kSplitRecBytes;
        const bool cut_hi = np > kSplitMax;                  // as the one-wave form: the whole list when it is short enough
        const double tau_s = cut_hi ? kPeakTauHi : 0.0;
        const int i0 = 2 * tid;                              // (capP == 512: two list entries per thread)
        const double2 kk = *reinterpret_cast<const double2 *>(pk_score + i0);
        const unsigned pp2 = *reinterpret_cast<const unsigned *>(pk_pos + i0);
        const bool t0 = i0 < np && kk.x >= tau_s, t1 = i0 + 1 < np && kk.y >= tau_s;
        unsigned total;
        const unsigned off = bx.scan((unsigned)t0 + (unsigned)t1, total);   // (its barrier: every thread has read its entries)
        // More than 256 peaks above the cut (block-uniform; reads with many strong level changes -- clip-heavy tRNA-like
        // signals).  The main kernel hands the read to the list launch (falling through here costs it two registers and 0.6 %
        // on C3); the list kernel finishes it in place: nothing has been written yet and the list is intact, so the
        // workgroup goes on into the one-piece form below, whose workgroup-wide suppression takes any list.  The slot stays
        // marked "nothing exported".
        if (SPLIT == 1 && total > (unsigned)kSplitMax) {
            to_big(3);
            return;
        }
        if (total <= (unsigned)kSplitMax) {
        // LDS from here on (the list is dead: every thread holds its two entries in registers): 2 FB half-chunk prefixes over
        // the score array, the exported positions densely over the position array
        double *scanbuf = reinterpret_cast<double *>(R);                                        // 2 FB x 8 B <= capP x 8 B
        unsigned short *cpos = reinterpret_cast<unsigned short *>(pk_pos - kPad);               // kSplitMax x 2 B
        {
            // the keys go out from the threads that hold them (neighbouring threads, neighbouring slots)
            double *gkey = reinterpret_cast<double *>(rec + 16);
            unsigned o = off;
            if (t0) {
                gkey[o] = kk.x;
                cpos[o] = (unsigned short)(pp2 & 0xffffu);
                ++o;
            }
            if (t1) {
                gkey[o] = kk.y;
                cpos[o] = (unsigned short)(pp2 >> 16);
            }
        }
        // prefix sums of the clipped samples at HALF-chunk granularity (a thread's consecutive 4 c4 samples in two halves
        // of 2 c4): the boundary's thread then adds at most 2 c4 - 1 <= 9 samples instead of 19
        const int c4 = (n + 4 * FB - 1) / (4 * FB);  // groups of four samples per thread: <= NPT / 4
        const int chunk = 4 * c4, half = 2 * c4;
        {
            const int ic = tid * chunk;
            float4 v4[NPT / 4];
#pragma unroll
            for (int g = 0; g < NPT / 4; ++g) v4[g] = reinterpret_cast<const float4 *>(sig + min(ic + 4 * g, capF + 16))[0];
            // (samples [n, capF + 32) are zero: whole groups are added; chunks beyond n are masked below)
            double lo_half = 0.0, acc = 0.0;
#pragma unroll
            for (int g = 0; g < NPT / 4; ++g) {
                if (g < c4) {  // workgroup-uniform
                    const double e0 = (double)v4[g].x, e1 = (double)v4[g].y, e2 = (double)v4[g].z, e3 = (double)v4[g].w;
                    // the first half ends after sample 2 c4 - 1: inside group c4 / 2 when c4 is odd, at its start when even
                    if (2 * g + 2 <= c4) lo_half += (e0 + e1) + (e2 + e3);
                    else if (2 * g < c4) lo_half += e0 + e1;
                    acc += (e0 + e1) + (e2 + e3);
                }
            }
            if (ic >= n) {
                acc = 0.0;
                lo_half = 0.0;
            }
            double incl = acc;
            auto shifted = [&](double x, auto ctrl, auto rmask) -> double {
                const long long b = __double_as_longlong(x);
                const unsigned lo_ = WDX_DPP(0u, (unsigned)b, decltype(ctrl)::value, decltype(rmask)::value);
                const unsigned hi_ = WDX_DPP(0u, (unsigned)(b >> 32), decltype(ctrl)::value, decltype(rmask)::value);
                return __longlong_as_double((long long)(((unsigned long long)hi_ << 32) | lo_));
            };
            incl += shifted(incl, std::integral_constant<int, 0x111>{}, std::integral_constant<int, 0xf>{});
            incl += shifted(incl, std::integral_constant<int, 0x112>{}, std::integral_constant<int, 0xf>{});
            incl += shifted(incl, std::integral_constant<int, 0x114>{}, std::integral_constant<int, 0xf>{});
            incl += shifted(incl, std::integral_constant<int, 0x118>{}, std::integral_constant<int, 0xf>{});
            incl += shifted(incl, std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xa>{});
            incl += shifted(incl, std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xc>{});
            const double excl = incl - acc;
            *reinterpret_cast<double2 *>(scanbuf + 2 * tid) = make_double2(excl, excl + lo_half);
            if (lane == 63) sh.stat[wave] = incl;
        }
        __syncthreads();
        if (tid < (int)total) {   // one exported peak per thread: coalesced stores
            const int pos = cpos[tid];
            const int b = pos + FW;                           // the boundary this peak would become: FW <= b < n
            int hc = (int)((float)(b >> 1) / (float)c4);      // half-chunk of sample b: exact quotient of small integers
            if (hc > 2 * FB - 1) hc = 2 * FB - 1;
            const int h0 = hc * half;                         // its first sample (even)
            const int cnt = b - h0;                           // samples of the half-chunk before the boundary: 0 .. 2 c4 - 1
            double base = scanbuf[hc];
            const int tw = hc >> 7;
            base += tw > 0 ? sh.stat[0] : 0.0;
            base += tw > 1 ? sh.stat[1] : 0.0;
            base += tw > 2 ? sh.stat[2] : 0.0;
            const float2 *hp = reinterpret_cast<const float2 *>(sig + h0);
            float2 w2[NPT / 4];
#pragma unroll
            for (int g = 0; g < NPT / 4; ++g) w2[g] = hp[g < c4 ? g : 0];
            double part = 0.0;
#pragma unroll
            for (int g = 0; g < NPT / 4; ++g) {
                if (g < c4) {
                    const float f0 = 2 * g < cnt ? w2[g].x : 0.0f, f1 = 2 * g + 1 < cnt ? w2[g].y : 0.0f;
                    part += (double)f0 + (double)f1;
                }
            }
            reinterpret_cast<double *>(rec + 16 + 8 * kSplitMax)[tid] = base + part;
            reinterpret_cast<unsigned short *>(rec + 16 + 16 * kSplitMax)[tid] = (unsigned short)pos;
        }
        WDX_FSTAMP(5);   // (diagnostic build: the end of the export; slots 6 .. 9 are the tail kernel's)
        if (tid == 0) {
            SplitHdr h;
            h.m = (int32_t)total | (cut_hi ? kSplitCutHi : 0);
            h.n = n;
            h.ptot = ((sh.stat[0] + sh.stat[1]) + sh.stat[2]) + sh.stat[3];   // (exact: any order)
            *reinterpret_cast<SplitHdr *>(rec) = h;
        }
        return;
        }   // (total <= kSplitMax)
    }

    // P3b..P5 by ONE wave: at most 256 peaks, four per lane of wave 0 -- the whole list when it is that short, else its
    // entries from kPeakTauHi up (picked through an index array: the list itself stays as it is).  Suppression sweeps
    // exchange their state bytes by lane shuffles alone, the kept peaks never leave the registers, the E-th largest kept
    // key comes from a wave-local radix select (64 bins = 64 lanes, members of the last bin ranked through v_readlane) and
    // the boundaries are written straight from the lanes: no barrier between the last tile and the event means but one,
    // no compaction, no workgroup-wide scan -- the other three waves wait.  Same decisions as the workgroup-wide form
    // below, which takes what this one declines (more than 256 picked peaks, a cut not certainly above kPeakTauHi).
    // NBT = 2 (suppression reach up to 17): the lane's window is its four peaks and eight on either side, the neighbours'
    // state bytes come from the lanes +-1 and +-2.
    bool solo_done = false;
    {
        constexpr int WNs = 4 + 2 * kPad;   // window entries: own 4 + kPad = 4 NBT on either side
        // (block-uniform) capP: the wave's index array / member list live in the suppression's state bytes
        // (a list of more than 512 entries -- long windows -- rarely leaves 256 or fewer above kPeakTauHi: not attempted)
        if (F.capP >= 512 && (np <= 4 * 64 || (pre_ok && np <= 512))) {
            if (wave == 0) {
                auto wfence = []() __attribute__((always_inline)) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                };
                // 0 boundaries written, 1 retry with exact scores, 2 too few peaks, 3 exact tie at the cut, 4 the workgroup-wide
                // form on the whole list
                unsigned outcome = 0;
                const int nb = min(kNBW, (d_eff - 1) / 2);
                const int k0 = 4 * lane;
                int wp[WNs];
                double ws[WNs];
                // the picked entries' list indices, in list (= position) order
                unsigned short *pidx = reinterpret_cast<unsigned short *>(
                    (reinterpret_cast<uintptr_t>(pk_pos + F.capP + kPad) + 7u) & ~(uintptr_t)7);   // 256 entries
                const double tau_s = np > 4 * 64 ? kPeakTauHi : 0.0;        // this form's own cut (0: the whole list)
                const double tau_v = tau_s > 0.0 ? tau_s : (pre_ok ? kPeakTauLo : 0.0);   // the cut the selection must clear
                const double tau_vhi = tau_v > 0.0 ? __builtin_fma(tau_v, kBandHi, kBandAbs) : 0.0;
                const unsigned not_clear = tau_s > 0.0 ? 4u : 1u;   // ... and where a read goes that does not
                int M = 0;
                auto pick = [&](int i, double sc_i) __attribute__((always_inline)) {
                    const bool take = i < np && sc_i >= tau_s;
                    const unsigned long long mask = __ballot(take);
                    const unsigned at = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                    if (take && M + (int)at < 4 * 64) pidx[M + (int)at] = (unsigned short)i;
                    M += (int)__popcll(mask);
                };
                {   // (np <= 512: eight rounds, their scores in flight together -- one LDS latency)
                    double sc8[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) sc8[q] = pk_score[min(64 * q + lane, np - 1)];
#pragma unroll
                    for (int q = 0; q < 8; ++q)
                        if (64 * q < np) pick(64 * q + lane, sc8[q]);
                }
                wfence();
                if (M > 4 * 64) {
                    outcome = 4;
                    M = 0;   // (nothing below looks at the list)
                }
#pragma unroll
                for (int q = 0; q < WNs; ++q) {
                    const int f = k0 - kPad + q;
                    const bool in = f >= 0 && f < M;
                    const int o = in ? (int)pidx[f] : 0;
                    const int pq = pk_pos[o];
                    const double sq = pk_score[o];
                    wp[q] = in ? pq : 0;
                    ws[q] = in ? sq : -__builtin_inf();   // (never outranks, never inside a band)
                }
                wfence();   // (the index array is dead: the select's member list reuses its bytes)
                bool dbt = false;
                unsigned mk[4] = {0, 0, 0, 0};
                unsigned und = 0, kept0 = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (k0 + j < M) {
                        const int pk = wp[kPad + j];
                        const double sk = ws[kPad + j];
                        const double sk_hi = exact_sc ? sk : __builtin_fma(sk, kBandHi, kBandAbs);
                        const double sk_lo = (sk - kBandAbs) * kBandLo;
#pragma unroll
                        for (int o = 1; o <= kNBW; ++o) {
                            if (o > nb) break;  // block-uniform
                            const bool inl = pk - wp[kPad + j - o] < d_eff;
                            const bool inr = wp[kPad + j + o] - pk < d_eff;
                            const bool outl = ws[kPad + j - o] > sk_hi, outr = ws[kPad + j + o] >= sk_hi;
                            if (inl && outl) mk[j] |= 1u << (kPad + j - o);
                            if (inr && outr) mk[j] |= 1u << (kPad + j + o);
                            if (!exact_sc) {
                                dbt |= inl && !outl && ws[kPad + j - o] >= sk_lo;
                                dbt |= inr && !outr && ws[kPad + j + o] >= sk_lo;
                            }
                        }
                        if (mk[j] == 0u) kept0 |= 1u << j;
                        else und |= 1u << j;
                    }
                }
                // the relaxation (monotone: any schedule reaches the same fixed point), neighbours' bytes by shuffle
                unsigned bC = kept0 | (und << 4);
                for (;;) {
                    // the window's kept / undecided bits: the state bytes of the lanes -NBT .. +NBT, four bits each
                    unsigned keptW = (bC & 15u) << kPad, undW = (bC >> 4) << kPad;
#pragma unroll
                    for (int q = 1; q <= NBT; ++q) {
                        // (DPP wave shifts, one per lane of distance: VALU moves instead of LDS round trips on this one wave's
                        // critical path; a lane without a source reads zero -- exactly the edge rule)
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
                    ++nms_iters;
                    if (!__ballot((bC >> 4) != 0u)) break;
                }
                const unsigned keep = bC & 15u;
                const bool doubt_any = !exact_sc && __ballot(dbt) != 0ull;
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
                if (outcome != 0) {
                    // (more than 256 picked peaks)
                } else if (tau_v > 0.0 && nkw <= E) {
                    outcome = not_clear;   // the cut list does not hold E + 1 kept peaks
                } else if (nkw < E) {
                    outcome = doubt_any ? 1u : 2u;
                } else if (nkw > E) {
                    // the E-th largest kept key: MSD radix select from the top, six bits a level, lane l counts digit 63 - l
                    // (scratch: 64 counters in the exchange block's rank slots, 64 members in the suppression's state bytes --
                    // neither is in use here: this wave's suppression lives in registers)
                    unsigned *wl = sh.rk;
                    unsigned long long *wlist = reinterpret_cast<unsigned long long *>(
                        (reinterpret_cast<uintptr_t>(pk_pos + F.capP + kPad) + 7u) & ~(uintptr_t)7);
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
                        wl[lane] = 0u;
                        wfence();
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const bool mbr = val[j] && (key[j] >> (shift + width)) == pfx;
                            if (mbr) atomicAdd(&wl[63u - (unsigned)((key[j] >> shift) & ((1ull << width) - 1ull))], 1u);
                        }
                        wfence();
                        const unsigned c = wl[lane];
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
                                const unsigned at = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32),
                                                                              __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                                if (mbr) wlist[wc + at] = key[j];
                                wc += (unsigned)__popcll(mask);
                            }
                            wfence();
                            const unsigned long long mine = (unsigned)lane < cb ? wlist[lane] : 0ull;
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
                    // approximate keys: the cut is certain when no other key reaches the lower end of T's band, and it must
                    // lie certainly above the append filter's threshold
                    const double Td = __longlong_as_double((long long)Tw);
                    const unsigned long long Tlo =
                        exact_sc ? Tw : (unsigned long long)__double_as_longlong(fmax((Td - kBandAbs) * kBandLo, 0.0));
                    unsigned ge = 0, gelo = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        ge += (unsigned)__popcll(__ballot(val[j] && key[j] >= Tw));
                        gelo += (unsigned)__popcll(__ballot(val[j] && key[j] >= Tlo));
                    }
                    if (exact_sc) {
                        if (ge != (unsigned)E) outcome = 3;   // exact score tie across the cut
                    } else if (doubt_any || gelo != (unsigned)E) {
                        outcome = 1;
                    } else if (tau_vhi > 0.0 && !(Td >= tau_vhi)) {
                        outcome = not_clear;   // the cut does not lie certainly above the threshold the peaks were picked with
                    }
                } else if (doubt_any) {   // nkw == E (unfiltered): every kept peak is selected
                    outcome = 1;
                }
                if (outcome == 0) {
                    // boundaries 0, selected peaks + FW (ascending: the list is position-ordered), n -- all the lanes' list
                    // entries were read into registers above, so the boundaries may overwrite the head of the score array
                    unsigned sel = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) sel |= (val[j] && key[j] >= Tw) ? 1u << j : 0u;
                    const unsigned cnt = (unsigned)__popc(sel);
                    unsigned o = wave_incl_scan_u32(cnt) - cnt;
                    wfence();
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (sel & (1u << j)) cpts[1 + o] = wp[kPad + j] + FW;
                        o += (sel >> j) & 1u;
                    }
                    if (lane == 0) {
                        cpts[0] = 0;
                        cpts[E + 1] = n;
                    }
                }
                if (lane == 0) {
                    sh.sel_bin = outcome;
                    sh.sel_cnt = (unsigned)nkw;
                }
            }
            __syncthreads();
            const unsigned oc = sh.sel_bin;
            nk = sh.sel_cnt;
            if (oc == 1u) {
                to_retry();
                return;
            }
            if (oc == 2u) {
                // fewer than E kept peaks: the reference gives up -- or, with accept_less_cpts, segments into fewer events
                // (sig_proc.py:185-188), which is the exact kernel's business (a handful of reads)
                if (P.accept_less_cpts) to_slow(8);
                else fail(WDX_READ_FAIL_SEGMENT);
                return;
            }
            if (oc == 3u) {
                to_slow(6);
                return;
            }
            if (oc == 0u) {
                solo_done = true;
                WDX_FSTAMP(5);
                WDX_FSTAMP(6);
                WDX_FSTAMP(7);
            }
        }
    }
    if (!solo_done) {

    // P3b: greedy distance suppression on the compact list (fixed point, see fp_process_read).
    // A thread owns 4 consecutive peaks per round of 1024.  Its state is ONE byte (kept nibble |
    // undecided nibble << 4); with the bytes of the threads before and after it sees a 12-peak window
    // (d_eff <= 9 and peaks are >= 2 apart: at most 4 neighbours per side can be in range), and each
    // owned peak has a 12-bit mask of the window members that outrank it within d_eff.  A sweep is then
    // two ANDs per peak: dropped if a masked neighbour is kept, kept if none is undecided.
    nms_iters = 0;
    bool doubt = false;  // approximate keys: a pair within d_eff whose order is inside the band
    const int R4 = (np + 4 * FB - 1) / (4 * FB);  // <= kRounds (capP <= kCapPMax)
    unsigned keepn[kRounds];                       // kept nibble at the fixed point
    if constexpr (NBT == 1) {
        // (the 12-peak window form, kept literally as it was tuned for the RNA004 kernel: the general form below
        // compiles to a slightly slower kernel at NBT = 1 -- 236.8 against 232.3 ms per 10 M reads)
        const int nb = min(kNB, (d_eff - 1) / 2);      // neighbours per side that can lie within d_eff
        unsigned hmA[kRounds], hmB[kRounds];           // window masks of peaks 0,1 | 2,3 (16 bits each)
        unsigned char *st8 = pk_state;                 // [-1] pad | kRounds * FB thread bytes | pad
    #pragma unroll
        for (int m = 0; m < kRounds; ++m) hmA[m] = hmB[m] = keepn[m] = 0u;
        {
    #pragma unroll
            for (int m = 0; m < kRounds; ++m) {
                const int k0 = m * 4 * FB + 4 * tid;
                if (m < R4) {
                    unsigned und = 0, kept0 = 0;
                    if (k0 < np) {
                        int wp[12];
                        double ws[12];
                        const uint2 *pp2 = reinterpret_cast<const uint2 *>(pk_pos + k0 - 4);
                        const double2 *sp2 = reinterpret_cast<const double2 *>(pk_score + k0 - 4);
    #pragma unroll
                        for (int q = 0; q < 3; ++q) {
                            const uint2 v = pp2[q];
                            wp[4 * q] = v.x & 0xffff; wp[4 * q + 1] = v.x >> 16;
                            wp[4 * q + 2] = v.y & 0xffff; wp[4 * q + 3] = v.y >> 16;
                        }
    #pragma unroll
                        for (int q = 0; q < 6; ++q) {
                            const double2 v = sp2[q];
                            ws[2 * q] = v.x;
                            ws[2 * q + 1] = v.y;
                        }
                        unsigned mk[4] = {0, 0, 0, 0};
    #pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int k = k0 + j;
                            if (k < np) {
                                const int pk = wp[4 + j];
                                const double sk = ws[4 + j];
                                // exact scores: an earlier peak outranks with >, a later one with >= (the greedy
                                // order's tie rule); approximate keys: outranked only beyond the band, and a
                                // neighbour between the band's ends is a doubt
                                const double sk_hi = exact_sc ? sk : __builtin_fma(sk, kBandHi, kBandAbs);
                                const double sk_lo = (sk - kBandAbs) * kBandLo;
    #pragma unroll
                                for (int o = 1; o <= kNB; ++o) {
                                    if (o > nb) break;  // block-uniform: peaks are >= 2 apart
                                    // (entries outside the list carry -inf keys: no index tests)
                                    const bool inl = pk - wp[4 + j - o] < d_eff;
                                    const bool inr = wp[4 + j + o] - pk < d_eff;
                                    const bool outl = ws[4 + j - o] > sk_hi, outr = ws[4 + j + o] >= sk_hi;
                                    if (inl && outl) mk[j] |= 1u << (4 + j - o);
                                    if (inr && outr) mk[j] |= 1u << (4 + j + o);
                                    if (!exact_sc) {  // (keys are never NaN here: a poisoned key cannot be a maximum)
                                        doubt |= inl && !outl && ws[4 + j - o] >= sk_lo;
                                        doubt |= inr && !outr && ws[4 + j + o] >= sk_lo;
                                    }
                                }
                                // a peak nothing outranks within d_eff is kept before the first sweep
                                if (mk[j] == 0u) kept0 |= 1u << j;
                                else und |= 1u << j;
                            }
                        }
                        hmA[m] = mk[0] | (mk[1] << 16);
                        hmB[m] = mk[2] | (mk[3] << 16);
                    }
                    st8[m * FB + tid] = (unsigned char)(kept0 | (und << 4));
                }
            }
            if (tid == 0) {
                st8[-1] = 0;
                st8[R4 * FB] = 0;
            }
            __syncthreads();
            // The relaxation is monotone (states only move UNDECIDED -> KEPT/DROPPED, and a stale UNDECIDED
            // neighbour only delays a decision), so any schedule reaches the same fixed point.  Between two
            // workgroup-wide exchanges (LDS + barrier) a wave therefore runs kSub sweeps on its own 256
            // consecutive peaks with the neighbouring lanes' state bytes taken by lane shuffles.
            constexpr int kSub = 3;
            for (;;) {
                int pending = 0;
    #pragma unroll
                for (int m = 0; m < kRounds; ++m) {
                    // (block-uniform round test; a wave whose 256 peaks of the round all lie past the list's end -- three
                    // of the four once the pre-filter has cut the list -- has nothing to sweep)
                    if (m < R4 && m * 4 * FB + 256 * wave < np) {
                        const int slot = m * FB + tid;
                        unsigned bL = st8[slot - 1], bC = st8[slot], bR = st8[slot + 1];
                        const unsigned orig = bC;
                        int pend = 0;
                        const unsigned mk4[4] = {hmA[m] & 0xffffu, hmA[m] >> 16, hmB[m] & 0xffffu, hmB[m] >> 16};
    #pragma unroll 1
                        for (int sub = 0; sub < kSub; ++sub) {
                            unsigned kept12 = (bL & 15u) | ((bC & 15u) << 4) | ((bR & 15u) << 8);
                            unsigned und12 = (bL >> 4) | ((bC >> 4) << 4) | ((bR >> 4) << 8);
    #pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                // dropped if a masked neighbour is kept, kept if no masked neighbour is kept or undecided;
                                // the peak's own (undecided) bit is selected in place, so nothing is normalised or shifted
                                const unsigned own = und12 & (1u << (4 + j));
                                const unsigned keepb = ((kept12 | und12) & mk4[j]) == 0u ? own : 0u;
                                const unsigned dropb = (kept12 & mk4[j]) != 0u ? own : 0u;
                                und12 &= ~(keepb | dropb);
                                kept12 |= keepb;
                            }
                            bC = ((kept12 >> 4) & 15u) | (((und12 >> 4) & 15u) << 4);
                            pend = (bC >> 4) != 0;
                            if (sub + 1 < kSub) {
                                if (!__ballot(pend)) break;  // wave-uniform: nothing left to decide here
                                const unsigned fromL = (unsigned)__shfl_up((int)bC, 1);
                                const unsigned fromR = (unsigned)__shfl_down((int)bC, 1);
                                if (lane > 0) bL = fromL;
                                if (lane < 63) bR = fromR;
                            }
                        }
                        pending |= pend;
                        if (bC != orig) st8[slot] = (unsigned char)bC;
                        keepn[m] = bC & 15u;
                    }
                }
                ++nms_iters;
                if (!bx.any(pending != 0)) break;
            }
        }
    } else {
        const int nb = min(kNBW, (d_eff - 1) / 2);     // neighbours per side that can lie within d_eff
        // A thread's window: its 4 peaks and the 4 * NBT on either side (WN = 12 or 20 list entries); each owned peak has a
        // WN-bit mask of the window members that outrank it within d_eff.  NBT = 1 packs two 12-bit masks per register
        // (hm[m][0..1]); NBT = 2 keeps one 20-bit mask per register (hm[m][0..3]).
        constexpr int WN = 4 + 8 * NBT, kHM = NBT == 1 ? 2 : 4;
        unsigned hm[kRounds][kHM];
        unsigned char *st8 = pk_state;                 // [-NBT .. -1] pad | kRounds * FB thread bytes | pad
    #pragma unroll
        for (int m = 0; m < kRounds; ++m) {
    #pragma unroll
            for (int q = 0; q < kHM; ++q) hm[m][q] = 0u;
            keepn[m] = 0u;
        }
        {
    #pragma unroll
            for (int m = 0; m < kRounds; ++m) {
                const int k0 = m * 4 * FB + 4 * tid;
                if (m < R4) {
                    unsigned und = 0, kept0 = 0;
                    if (k0 < np) {
                        int wp[WN];
                        double ws[WN];
                        const uint2 *pp2 = reinterpret_cast<const uint2 *>(pk_pos + k0 - kPad);
                        const double2 *sp2 = reinterpret_cast<const double2 *>(pk_score + k0 - kPad);
    #pragma unroll
                        for (int q = 0; q < WN / 4; ++q) {
                            const uint2 v = pp2[q];
                            wp[4 * q] = v.x & 0xffff; wp[4 * q + 1] = v.x >> 16;
                            wp[4 * q + 2] = v.y & 0xffff; wp[4 * q + 3] = v.y >> 16;
                        }
    #pragma unroll
                        for (int q = 0; q < WN / 2; ++q) {
                            const double2 v = sp2[q];
                            ws[2 * q] = v.x;
                            ws[2 * q + 1] = v.y;
                        }
                        unsigned mk[4] = {0, 0, 0, 0};
    #pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int k = k0 + j;
                            if (k < np) {
                                const int pk = wp[kPad + j];
                                const double sk = ws[kPad + j];
                                // exact scores: an earlier peak outranks with >, a later one with >= (the greedy
                                // order's tie rule); approximate keys: outranked only beyond the band, and a
                                // neighbour between the band's ends is a doubt
                                const double sk_hi = exact_sc ? sk : __builtin_fma(sk, kBandHi, kBandAbs);
                                const double sk_lo = (sk - kBandAbs) * kBandLo;
    #pragma unroll
                                for (int o = 1; o <= kNBW; ++o) {
                                    if (o > nb) break;  // block-uniform: peaks are >= 2 apart
                                    // (entries outside the list carry -inf keys: no index tests)
                                    const bool inl = pk - wp[kPad + j - o] < d_eff;
                                    const bool inr = wp[kPad + j + o] - pk < d_eff;
                                    const bool outl = ws[kPad + j - o] > sk_hi, outr = ws[kPad + j + o] >= sk_hi;
                                    if (inl && outl) mk[j] |= 1u << (kPad + j - o);
                                    if (inr && outr) mk[j] |= 1u << (kPad + j + o);
                                    if (!exact_sc) {  // (keys are never NaN here: a poisoned key cannot be a maximum)
                                        doubt |= inl && !outl && ws[kPad + j - o] >= sk_lo;
                                        doubt |= inr && !outr && ws[kPad + j + o] >= sk_lo;
                                    }
                                }
                                // a peak nothing outranks within d_eff is kept before the first sweep
                                if (mk[j] == 0u) kept0 |= 1u << j;
                                else und |= 1u << j;
                            }
                        }
                        if constexpr (NBT == 1) {
                            hm[m][0] = mk[0] | (mk[1] << 16);
                            hm[m][1] = mk[2] | (mk[3] << 16);
                        } else {
    #pragma unroll
                            for (int j = 0; j < 4; ++j) hm[m][j] = mk[j];
                        }
                    }
                    st8[m * FB + tid] = (unsigned char)(kept0 | (und << 4));
                }
            }
            if (tid < NBT) {
                st8[-1 - tid] = 0;
                st8[R4 * FB + tid] = 0;
            }
            __syncthreads();
            // The relaxation is monotone (states only move UNDECIDED -> KEPT/DROPPED, and a stale UNDECIDED
            // neighbour only delays a decision), so any schedule reaches the same fixed point.  Between two
            // workgroup-wide exchanges (LDS + barrier) a wave therefore runs kSub sweeps on its own 256
            // consecutive peaks with the neighbouring lanes' state bytes taken by lane shuffles.
            constexpr int kSub = 3;
            for (;;) {
                int pending = 0;
    #pragma unroll
                for (int m = 0; m < kRounds; ++m) {
                    // (block-uniform round test; a wave whose 256 peaks of the round all lie past the list's end -- three
                    // of the four once the pre-filter has cut the list -- has nothing to sweep)
                    if (m < R4 && m * 4 * FB + 256 * wave < np) {
                        const int slot = m * FB + tid;
                        // state bytes of the threads slot - NBT .. slot + NBT (index NBT = this thread)
                        unsigned bN[2 * NBT + 1];
    #pragma unroll
                        for (int q = 0; q < 2 * NBT + 1; ++q) bN[q] = st8[slot - NBT + q];
                        const unsigned orig = bN[NBT];
                        int pend = 0;
                        unsigned mk4[4];
                        if constexpr (NBT == 1) {
                            mk4[0] = hm[m][0] & 0xffffu; mk4[1] = hm[m][0] >> 16;
                            mk4[2] = hm[m][1] & 0xffffu; mk4[3] = hm[m][1] >> 16;
                        } else {
    #pragma unroll
                            for (int j = 0; j < 4; ++j) mk4[j] = hm[m][j];
                        }
    #pragma unroll 1
                        for (int sub = 0; sub < kSub; ++sub) {
                            unsigned keptW = 0, undW = 0;
    #pragma unroll
                            for (int q = 0; q < 2 * NBT + 1; ++q) {
                                keptW |= (bN[q] & 15u) << (4 * q);
                                undW |= (bN[q] >> 4) << (4 * q);
                            }
    #pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                // dropped if a masked neighbour is kept, kept if no masked neighbour is kept or undecided;
                                // the peak's own (undecided) bit is selected in place, so nothing is normalised or shifted
                                const unsigned own = undW & (1u << (kPad + j));
                                const unsigned keepb = ((keptW | undW) & mk4[j]) == 0u ? own : 0u;
                                const unsigned dropb = (keptW & mk4[j]) != 0u ? own : 0u;
                                undW &= ~(keepb | dropb);
                                keptW |= keepb;
                            }
                            bN[NBT] = ((keptW >> kPad) & 15u) | (((undW >> kPad) & 15u) << 4);
                            pend = (bN[NBT] >> 4) != 0;
                            if (sub + 1 < kSub) {
                                if (!__ballot(pend)) break;  // wave-uniform: nothing left to decide here
    #pragma unroll
                                for (int q = 1; q <= NBT; ++q) {
                                    const unsigned fromL = (unsigned)__shfl_up((int)bN[NBT], q);
                                    const unsigned fromR = (unsigned)__shfl_down((int)bN[NBT], q);
                                    if (lane >= q) bN[NBT - q] = fromL;
                                    if (lane < 64 - q) bN[NBT + q] = fromR;
                                }
                            }
                        }
                        pending |= pend;
                        if (bN[NBT] != orig) st8[slot] = (unsigned char)bN[NBT];
                        keepn[m] = bN[NBT] & 15u;
                    }
                }
                ++nms_iters;
                if (!bx.any(pending != 0)) break;
            }
        }
    }
    WDX_FSTAMP(5);

    // P4: compact the kept peaks (position order), then keep the E highest
    T = 0;
    {
        unsigned keep[kRounds];
        uint2 kp2[kRounds];
        double2 ks2[kRounds][2];
#pragma unroll
        for (int m = 0; m < kRounds; ++m) {
            const int k0 = m * 4 * FB + 4 * tid;
            keep[m] = 0u;
            kp2[m] = make_uint2(0, 0);
            ks2[m][0] = ks2[m][1] = make_double2(0, 0);
            if (m < R4 && k0 < np) {
                kp2[m] = *reinterpret_cast<const uint2 *>(pk_pos + k0);
                ks2[m][0] = reinterpret_cast<const double2 *>(pk_score + k0)[0];
                ks2[m][1] = reinterpret_cast<const double2 *>(pk_score + k0)[1];
                keep[m] = keepn[m];
            }
        }
        unsigned offs[kRounds];
        nk = 0;
#pragma unroll
        for (int m = 0; m < kRounds; ++m) {
            offs[m] = 0;
            if (m < R4) {  // block-uniform; the first scan's barrier fences every read above
                unsigned tot;
                offs[m] = nk + bx.scan((unsigned)__popc(keep[m]), tot);
                nk += tot;
            }
        }
        if (tau_hi > 0.0 && (int)nk <= E) {   // (block-uniform) the cut list does not hold E + 1 kept peaks: redone unfiltered
            to_retry();
            return;
        }
        if ((int)nk < E) {
            if (!exact_sc && bx.any(doubt)) {
                to_retry();
                return;
            }
            if (P.accept_less_cpts) to_slow(8);   // (fewer events than configured: the exact kernel's business)
            else fail(WDX_READ_FAIL_SEGMENT);
            return;
        }
        if (nk > 4 * FB || (int)nk > kept_cap) {
            to_big(5);
            return;
        }
#pragma unroll
        for (int m = 0; m < kRounds; ++m) {
            unsigned off = offs[m];
            const unsigned short pj[4] = {(unsigned short)(kp2[m].x & 0xffff), (unsigned short)(kp2[m].x >> 16),
                                          (unsigned short)(kp2[m].y & 0xffff), (unsigned short)(kp2[m].y >> 16)};
            const double sj[4] = {ks2[m][0].x, ks2[m][0].y, ks2[m][1].x, ks2[m][1].y};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (keep[m] & (1u << j)) {
                    kept_pos[off] = pj[j];
                    kept_key[off] = (unsigned long long)__double_as_longlong(sj[j]);
                    ++off;
                }
            }
        }
        __syncthreads();
        if ((int)nk > E) {
            // kept keys, NS per thread: two slots cover the usual ~400 kept peaks (every sweep of the select costs per
            // slot), four the capacity
            auto top_e = [&](auto ns_t) -> bool {
                constexpr int NS = decltype(ns_t)::value;
                unsigned long long key[NS];
#pragma unroll
                for (int m = 0; m < NS; ++m) key[m] = kept_key[min(tid + m * FB, (int)nk - 1)];
                auto each_k = [&](auto &&f) {
#pragma unroll
                    for (int m = 0; m < NS; ++m) f(key[m], tid + m * FB < (int)nk);
                };
                // bounds from the high words only (one DPP reduction): [hmin << 32, (hmax << 32) | ~0u]
                unsigned hmin = 0xffffffffu, hmax = 0;
                each_k([&](unsigned long long k_, bool valid) {
                    const unsigned hw = (unsigned)(k_ >> 32);
                    hmin = min(hmin, valid ? hw : 0xffffffffu);
                    hmax = max(hmax, valid ? hw : 0u);
                });
                unsigned ghmin, ghmax, dmy;
                bx.minmaxsum(hmin, hmax, 0u, ghmin, ghmax, dmy);
                const unsigned long long gmin = (unsigned long long)ghmin << 32;
                const unsigned long long gmax = ((unsigned long long)ghmax << 32) | 0xffffffffull;
                // kTopBits-bit digits: the histogram sits behind the kept keys in the score array
                T = fast_select<unsigned long long, kTopBits, false>(each_k, nk - (unsigned)E, gmin, gmax, hist_topk, bx);
                // approximate keys: the cut is certain when no other key reaches the lower end of T's band
                const double Td = __longlong_as_double((long long)T);
                const unsigned long long Tlo =
                    exact_sc ? T : (unsigned long long)__double_as_longlong(fmax((Td - kBandAbs) * kBandLo, 0.0));
                unsigned ge = 0;
                each_k([&](unsigned long long k_, bool valid) {
                    ge += (valid && k_ >= T) ? 1u : 0u;
                    ge += (valid && k_ >= Tlo) ? 1u << 11 : 0u;
                });
                ge += doubt ? 1u << 22 : 0u;  // (nk <= 1024: 11 + 11 + 9 bits)
                const unsigned gge = bx.sum(ge);
                // block-uniform from here: a suppression doubt, or a key inside the band below the cut -- or a cut that does
                // not lie certainly above the pre-filter's threshold (the peaks it dropped could then belong to the E)
                doubt = (gge >> 22) != 0 || ((gge >> 11) & 0x7ffu) != (unsigned)E || (tau_hi > 0.0 && !(Td >= tau_hi));
                return exact_sc && (gge & 0x7ffu) != (unsigned)E;  // exact score tie across the cut
            };
            const bool tie = (int)nk <= FB ? top_e(std::integral_constant<int, 1>{})
                             : ((int)nk <= 2 * FB ? top_e(std::integral_constant<int, 2>{})
                                                  : top_e(std::integral_constant<int, 4>{}));
            if (tie) {  // block-uniform -> slow path
                to_slow(6);
                return;
            }
        } else {
            doubt = !exact_sc && bx.any(doubt);
        }
    }
    if (!exact_sc && doubt) {  // block-uniform
        to_retry();
        return;
    }
    WDX_FSTAMP(6);

    // P5: boundaries 0, selected peaks + 12 (ascending), n
    {
        unsigned sel = 0;
        int ppos4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx = tid * 4 + j;
            const int ic = idx < (int)nk ? idx : 0;
            ppos4[j] = kept_pos[ic];
            if (idx < (int)nk && kept_key[ic] >= T) sel |= 1u << j;
        }
        unsigned total;
        unsigned o = bx.scan((unsigned)__popc(sel), total);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (sel & (1u << j)) cpts[1 + o++] = ppos4[j] + FW;
        if (tid == 0) {
            cpts[0] = 0;
            cpts[E + 1] = n;
        }
        __syncthreads();
    }
    WDX_FSTAMP(7);
    }  // (!solo_done)
    const int nseg = E + 1;

    // P6: event means.  Every partial sum of the clipped samples is exactly representable (checked in P1), so any
    // grouping gives the reference's left-to-right sums: a thread sums its chunk of consecutive samples, a scan turns
    // the chunk sums into prefix sums, and the thread of boundary s adds the few samples between its chunk's start and
    // the boundary -- P(cpts[s]); an event's sum is the difference of two of those.  No search for the first segment
    // of a chunk, no boundary test per sample, no atomics.
    {
        const int c4 = (n + 4 * FB - 1) / (4 * FB);  // groups of four samples per thread: <= NPT / 4
        const int chunk = 4 * c4;
        const int i0 = tid * chunk;
        double *scanbuf = zz;  // FB wave-local exclusive prefix sums (zz | tmp), then dead
        double acc = 0.0;
        // STREAM: the samples are not resident -- the clipped samples come from HBM / L2 again (16-byte loads clamped to
        // the last whole group of the window, v_med3_f32 with the recorded bounds, zeros from n on: the values the
        // resident form's P0 writes to LDS)
        struct __attribute__((packed, aligned(4))) F4G { float x, y, z, w; };
        const float *__restrict__ gsrc = A.sig + row_off + start;
        auto ld4 = [&](int idx) -> float4 {
            const unsigned last4g = (unsigned)(n - 4);
            const F4G v = *reinterpret_cast<const F4G *>(gsrc + min((unsigned)idx, last4g));
            float e0 = __builtin_amdgcn_fmed3f(v.x, lo, hi), e1 = __builtin_amdgcn_fmed3f(v.y, lo, hi);
            float e2 = __builtin_amdgcn_fmed3f(v.z, lo, hi), e3 = __builtin_amdgcn_fmed3f(v.w, lo, hi);
            const int sft = idx - (int)last4g;  // > 0: the load was clamped and holds samples n - 4 .. n - 1
            if (__builtin_amdgcn_ballot_w64(sft > 0)) {  // wave-uniform: only the wave at the window's end
                if (sft > 0) {
                    e0 = sft == 1 ? e1 : sft == 2 ? e2 : sft == 3 ? e3 : 0.0f;
                    e1 = sft == 1 ? e2 : sft == 2 ? e3 : 0.0f;
                    e2 = sft == 1 ? e3 : 0.0f;
                    e3 = 0.0f;
                }
            }
            return make_float4(e0, e1, e2, e3);
        };
        if constexpr (STREAM) {
            // up to 64 samples per thread: four 16-byte loads in flight at a time
            for (int g0 = 0; g0 < c4; g0 += 4) {
                float4 v4[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) v4[g] = ld4(i0 + 4 * (g0 + g));  // (beyond the chunk: the next thread's, masked)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (g0 + g < c4) {
                        acc += (double)v4[g].x;
                        acc += (double)v4[g].y;
                        acc += (double)v4[g].z;
                        acc += (double)v4[g].w;
                    }
                }
            }
            if (i0 >= n) acc = 0.0;
        } else {
            float4 v4[NPT / 4];
#pragma unroll
            for (int g = 0; g < NPT / 4; ++g) {
                v4[g] = reinterpret_cast<const float4 *>(sig + min(i0 + 4 * g, capF + 16))[0];
            }
#pragma unroll
            for (int g = 0; g < NPT / 4; ++g) {
                if (g < c4) {  // workgroup-uniform; samples [n, n + 24) are zero, whole chunks beyond n are masked below
                    acc += (double)v4[g].x;
                    acc += (double)v4[g].y;
                    acc += (double)v4[g].z;
                    acc += (double)v4[g].w;
                }
            }
            if (i0 >= n) acc = 0.0;
        }
        // inclusive scan over the wave (DPP moves on the two halves), exclusive prefix and wave total to LDS
        double incl = acc;
        {
            auto shifted = [&](double x, auto ctrl, auto rmask) -> double {
                const long long b = __double_as_longlong(x);
                const unsigned lo_ = WDX_DPP(0u, (unsigned)b, decltype(ctrl)::value, decltype(rmask)::value);
                const unsigned hi_ = WDX_DPP(0u, (unsigned)(b >> 32), decltype(ctrl)::value, decltype(rmask)::value);
                return __longlong_as_double((long long)(((unsigned long long)hi_ << 32) | lo_));
            };
            incl += shifted(incl, std::integral_constant<int, 0x111>{}, std::integral_constant<int, 0xf>{});
            incl += shifted(incl, std::integral_constant<int, 0x112>{}, std::integral_constant<int, 0xf>{});
            incl += shifted(incl, std::integral_constant<int, 0x114>{}, std::integral_constant<int, 0xf>{});
            incl += shifted(incl, std::integral_constant<int, 0x118>{}, std::integral_constant<int, 0xf>{});
            incl += shifted(incl, std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xa>{});
            incl += shifted(incl, std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xc>{});
        }
        scanbuf[tid] = incl - acc;
        if (lane == 63) sh.stat[wave] = incl;  // (stat[] is free until the optional statistics of P7)
        __syncthreads();
        if (tid <= nseg) {
            const int b = cpts[tid];                          // 0 <= b <= n
            int t = (int)((float)(b >> 2) / (float)c4);       // owner of sample b: exact quotient of small integers
            if (t > FB - 1) t = FB - 1;                       // (b == n == FB * chunk)
            const int cnt = b - t * chunk;                    // samples of t's chunk before the boundary: 0 .. chunk
            double base = scanbuf[t];
            const int tw = t >> 6;
            base += tw > 0 ? sh.stat[0] : 0.0;
            base += tw > 1 ? sh.stat[1] : 0.0;
            base += tw > 2 ? sh.stat[2] : 0.0;
            double part = 0.0;
            if constexpr (STREAM) {
                for (int g0 = 0; g0 < c4; g0 += 4) {
                    if (4 * g0 >= cnt) break;  // (per thread: the boundary threads' chunk prefixes differ in length)
                    float4 w4[4];
#pragma unroll
                    for (int g = 0; g < 4; ++g) w4[g] = ld4(t * chunk + 4 * (g0 + g));
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int k = 4 * (g0 + g);
                        part += k < cnt ? (double)w4[g].x : 0.0;
                        part += k + 1 < cnt ? (double)w4[g].y : 0.0;
                        part += k + 2 < cnt ? (double)w4[g].z : 0.0;
                        part += k + 3 < cnt ? (double)w4[g].w : 0.0;
                    }
                }
            } else {
                const float4 *c4p = reinterpret_cast<const float4 *>(sig + t * chunk);
                float4 w4[NPT / 4];
#pragma unroll
                for (int g = 0; g < NPT / 4; ++g) {
                    w4[g] = c4p[g < c4 ? g : 0];
                }
#pragma unroll
                for (int g = 0; g < NPT / 4; ++g) {
                    if (g < c4) {
                        const int k = 4 * g;
                        part += k < cnt ? (double)w4[g].x : 0.0;
                        part += k + 1 < cnt ? (double)w4[g].y : 0.0;
                        part += k + 2 < cnt ? (double)w4[g].z : 0.0;
                        part += k + 3 < cnt ? (double)w4[g].w : 0.0;
                    }
                }
            }
            ev[tid] = base + part;                            // P(cpts[tid])
        }
        __syncthreads();
        // (the means land in zz, which takes over the name ev: ev held the prefix values its neighbours still read)
        for (int s2 = tid; s2 < nseg; s2 += FB) zz[s2] = (ev[s2 + 1] - ev[s2]) / (double)(cpts[s2 + 1] - cpts[s2]);
        double *t_ = ev;
        ev = zz;
        zz = t_;
    }
    WDX_FSTAMP(8);

    // Refinement branch (tRNA models): the adapter's segmentation and the clip bounds go to
    // fingerprint_refine_tail_kernel, which does the rest (statistics, subsequence match, the barcode's segmentation)
    if (A.rf.ws) {
        RefineRec *rec = reinterpret_cast<RefineRec *>(A.rf.ws) + r;
        for (int s = tid; s < nseg; s += FB) rec->ev[s] = ev[s];
        for (int s = tid; s <= nseg; s += FB) rec->cpts[s] = cpts[s];
        if (tid == 0) {
            rec->n = n;
            rec->lo = lo;
            rec->hi = hi;
            rec->state = 1;
        }
        return;
    }

    // P7: normalise, (optional) stats, tail
    {
        double mean, sd;
        fast_mean_sd(ev, tmp, nseg, sh, mean, sd);
        double zc = 0.0, zs = 1.0;  // z = (ev - zc) / zs
        if (P.seg_norm == WDX_NORM_MEAN) {
            zc = mean;
            zs = sd;
        } else if (P.seg_norm == WDX_NORM_MEDIAN) {
            zc = fast_small_median(ev, nseg, rankbuf, sh);
            for (int s = tid; s < nseg; s += FB) tmp[s] = fabs(ev[s] - zc);
            zs = fast_small_median(tmp, nseg, rankbuf, sh);
        }
        if (nseg < K) {
            fail(WDX_READ_FAIL_UNKNOWN);
            return;
        }
        for (int i = tid; i < K; i += FB) {
            const int s = nseg - K + i;
            if (A.fpt) A.fpt[r * K + i] = P.seg_norm == WDX_NORM_NONE ? ev[s] : (ev[s] - zc) / zs;
            if (A.dwell) A.dwell[r * K + i] = (int64_t)(cpts[s + 1] - cpts[s]);
        }
        if (A.stats) {  // adapter_dt_med/mad, adapter_event_mean/std/med/mad (sig_proc.py:562-567)
            for (int s = tid; s < nseg; s += FB) tmp[s] = (double)(cpts[s + 1] - cpts[s]);
            const double dt_med = fast_small_median(tmp, nseg, rankbuf, sh);
            for (int s = tid; s < nseg; s += FB) tmp[s] = fabs(tmp[s] - dt_med);
            const double dt_mad = fast_small_median(tmp, nseg, rankbuf, sh);
            const double ev_med = fast_small_median(ev, nseg, rankbuf, sh);
            for (int s = tid; s < nseg; s += FB) tmp[s] = fabs(ev[s] - ev_med);
            const double ev_mad = fast_small_median(tmp, nseg, rankbuf, sh);
            if (tid == 0) {
                double *o = A.stats + r * 6;
                o[0] = dt_med; o[1] = dt_mad; o[2] = mean; o[3] = sd; o[4] = ev_med; o[5] = ev_mad;
            }
        }
        if (tid == 0) A.status[r] = WDX_READ_OK;
    }
    WDX_FSTAMP(9);
    if (PROF && tid == 0 && r < A.prof_reads) {
        A.prof[r * 32 + 10] = nms_iters;
        A.prof[r * 32 + 11] = n;
        A.prof[r * 32 + 12] = np;
        A.prof[r * 32 + 14] = exact_sc ? 2 : 1;
    }
}

template <int NPT, bool PROF, int FW = kFW, int NBT = 1, bool EXT = false, bool SPLIT = false>
// (SPLIT: the tile kernel of the split pair, hand-on mode; PROF + SPLIT: wdx_fingerprint_profile_dev's fast_path = 2)
// (EXT up to 5120 samples with the filtered peak list: 26.8 KB of LDS and 80 VGPRs -> SIX workgroups per CU)
__global__ __launch_bounds__(FB, (NPT <= kNptMid ? (EXT && NBT == 1 ? 6 : 5) : (EXT && NBT == 2 && NPT == kNptLarge && FW >= 12 && FW % 6 == 0 ? kWideWgPerCu : 4)) * FB / 256)
void fingerprint_fast_kernel(FastArgs F) {
    fast_body<NPT, PROF, FW, NBT, EXT, false, SPLIT ? 1 : 0>(F, F.a.block_base + blockIdx.x);
}

// the reads of a device-side list, a fixed grid striding over it
template <int NPT, int FW = kFW, int NBT = 1>
__global__ __launch_bounds__(FB, (NPT <= 24 ? 4 : 3) * FB / 256) void fingerprint_fast_list_kernel(FastArgs F) {
    const unsigned n = *F.in_count;
    for (unsigned k = F.in_start + blockIdx.x; k < n; k += gridDim.x) {
        __syncthreads();  // the previous read's LDS is dead only once every wave has left it
        fast_body<NPT, false, FW, NBT>(F, (int64_t)F.in_list[k]);
    }
}

// The first `grid` reads of a device-side list, one workgroup each; workgroups past the end of the list leave at once
// (0.2 us per thousand of them).  The striding kernel above pays for its loop with registers: loop-invariant code
// motion stretches dozens of live ranges over the whole body (128 VGPRs and spills at 6144 samples instead of 97),
// so the lists that carry a real share of the reads go through this one with a grid sized for the expected share,
// and the striding kernel only takes what lies beyond that grid.
// (always behind a main kernel of a large batch: EXT -- clip_bounds_list_kernel runs over the same list entries first;
// a read without a record, flag CLIP_NONE, is handed to the exact kernel)
template <int NPT, int FW = kFW, int NBT = 1, bool SPLIT = false>
__global__ __launch_bounds__(FB, (NPT <= kNptMid ? 5 : 4) * FB / 256) void fingerprint_fast_list1_kernel(FastArgs F) {
    const int64_t k = F.a.block_base + blockIdx.x;
    if (k >= (int64_t)*F.in_count) return;   // (SPLIT: the tail kernel makes the same test before it looks at this slot)
    fast_body<NPT, false, FW, NBT, true, false, SPLIT ? 2 : 0>(F, (int64_t)F.in_list[k]);
}

// Windows of 8193 .. 16384 samples (the reference's RNA002 config admits 15 200): the streaming form of the body, one
// workgroup per entry of a device-side list (entries beyond the list's end leave at once).  Ahead of it
// clip_bounds_block_kernel (below) writes the list entries' clip records.
template <int FW = kFW, int NBT = 1>
__global__ __launch_bounds__(FB, 4 * FB / 256) void fingerprint_fast_stream_kernel(FastArgs F) {
    const int64_t k = F.a.block_base + blockIdx.x;
    if (k >= (int64_t)*F.in_count) return;
    fast_body<kNptStream, false, FW, NBT, true, true>(F, (int64_t)F.in_list[k]);
}

// (from a kernel key to these instantiations: resolve_fast_width, behind the split tail kernel in wdx_fingerprint_split.inc)

// A1 for long windows (up to 16384 samples), one WORKGROUP per list entry with the samples in LDS: the radix selects of
// the non-EXT fast kernels (fast_median_lds) as a kernel of their own -- clip_bounds_kernel's one-wave form would need
// 256 registers per lane for the samples alone.  Writes the same ClipRec.
struct ClipBlockArgs {
    FpArgs a;
    ClipRec *rec;
    const unsigned *in_count;
    const int32_t *in_list;
    int cap;  // samples the LDS carve-up holds (multiple of 1024)
};
#ifndef WDX_EXTRA_TU   // (a non-template kernel: defined by wdx_fingerprint.hip's own translation unit only)
__global__ __launch_bounds__(FB) void clip_bounds_block_kernel(ClipBlockArgs C) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const FpArgs &A = C.a;
    const wdx_seg_params &P = A.p;
    const int tid = threadIdx.x;
    const int64_t k = A.block_base + blockIdx.x;
    if (k >= (int64_t)*C.in_count) return;
    const int64_t r = C.in_list[k];
    ClipRec out{0.0f, 0.0f, 0.0f, CLIP_NONE};
    if (C.rec[r].flag != CLIP_NONE) return;  // (block-uniform: the record exists already)
    const int64_t row_off = A.row_off ? A.row_off[r] : r * A.stride;
    const int64_t row_len = A.row_len ? (int64_t)A.row_len[r] : (A.row_off ? A.row_off[r + 1] - A.row_off[r] : A.stride);
    int64_t start = (int64_t)A.a_start[r] - P.padding;
    if (start < 0) start = 0;
    int64_t stop = (int64_t)A.a_end[r] + P.padding;
    if (stop > row_len) stop = row_len;
    const int64_t n64 = stop - start;
    if ((A.ok && !A.ok[r]) || n64 < 256 || n64 > (int64_t)C.cap) return;  // (the record stays CLIP_NONE)
    const int n = (int)n64;
    float *sig = reinterpret_cast<float *>(smem);                                   // cap + 32
    unsigned *hist = reinterpret_cast<unsigned *>(sig + C.cap + 32);                // kHB + 64
    FastShared &sh = *reinterpret_cast<FastShared *>(hist + kHB + 64);
    BlockEx bx(sh);
    // HBM -> LDS with the extremes of the order-preserving keys (any sign: this kernel serves a minority of the reads)
    const float *__restrict__ src = A.sig + row_off + start;
    unsigned kmn = 0xffffffffu, kmx = 0u;
    {
        // sixteen-byte loads (dword-aligned), four in flight per thread; the <= 3 samples of a ragged tail one by one
        struct __attribute__((packed, aligned(4))) F4U { float x, y, z, w; };
        const int n4 = n & ~3;
#pragma unroll 4
        for (int i = 4 * tid; i < n4; i += 4 * FB) {
            const F4U v = *reinterpret_cast<const F4U *>(src + i);
            *reinterpret_cast<float4 *>(sig + i) = make_float4(v.x, v.y, v.z, v.w);
            const unsigned k0 = f32_key(v.x), k1 = f32_key(v.y), k2 = f32_key(v.z), k3 = f32_key(v.w);
            kmn = min(min(kmn, k0), min(k1, min(k2, k3)));
            kmx = max(max(kmx, k0), max(k1, max(k2, k3)));
        }
        if (n4 + tid < n) {
            const float v = src[n4 + tid];
            sig[n4 + tid] = v;
            const unsigned key = f32_key(v);
            kmn = min(kmn, key);
            kmx = max(kmx, key);
        }
    }
    for (int i = n + tid; i < ((n + 4 * FB - 1) / (4 * FB)) * (4 * FB); i += FB) sig[i] = 0.0f;  // (the selects read whole groups)
    unsigned xkmin, xkmax, unused;
    bx.minmaxsum(kmn, kmx, 0u, xkmin, xkmax, unused);
    // an infinity or a NaN (NaNs sort outside the infinities in key order) -> the exact general kernel
    if (xkmax >= f32_key(__builtin_inff()) || xkmin <= f32_key(-__builtin_inff())) {
        out.flag = CLIP_NAN_NEG;
        if (tid == 0) C.rec[r] = out;
        return;
    }
    const bool neg = xkmin < 0x80000000u;  // block-uniform
    const unsigned sig_off = 0u;
    const unsigned hist_off = (unsigned)(reinterpret_cast<unsigned char *>(hist) - smem);
    const unsigned sh_off = (unsigned)(reinterpret_cast<unsigned char *>(&sh) - smem);
    MedRet mr = neg ? fast_median_lds<2>(sig_off, n, 0.0f, 0, xkmin, xkmax, hist_off, sh_off, bx.par, nullptr)
                    : fast_median_lds<0>(sig_off, n, 0.0f, 0, xkmin & 0x7fffffffu, xkmax & 0x7fffffffu, hist_off, sh_off,
                                         bx.par, nullptr);
    bx.par = mr.par;
    const float med = mr.v;
    const float dmax = fmaxf(fabsf(key_f32(xkmin) - med), fabsf(key_f32(xkmax) - med));
    mr = fast_median_lds<1>(sig_off, n, med, 1, 0u, __float_as_uint(dmax), hist_off, sh_off, bx.par, nullptr);
    const float mad = mr.v;
    float lo, hi;
    clip_bounds(P, med, mad, lo, hi);
    const float cmin = __builtin_amdgcn_fmed3f(key_f32(xkmin), lo, hi);
    const float cmax = __builtin_amdgcn_fmed3f(key_f32(xkmax), lo, hi);
    bool exact = (lo == lo) && (hi == hi) && lo <= hi && cmin > 0.0f && cmax < 3.0e38f;
    if (exact) {
        int fa = (int)(__float_as_uint(cmin) >> 23), fb = (int)(__float_as_uint(cmax) >> 23);
        if (fa == 0) fa = 1;
        exact = (fb - fa) + (32 - __clz(n)) <= 28;
    }
    out.lo = lo;
    out.hi = hi;
    out.cmax = cmax;
    out.flag = exact ? CLIP_OK : CLIP_INEXACT;
    if (tid == 0) C.rec[r] = out;
}
#endif  // WDX_EXTRA_TU
