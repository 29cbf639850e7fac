// Per-read adapter fingerprinting for gfx950 -- stage A of the hot path.
//
// Replaces the per-read Python loop /root/reference/warpdemux/file_proc.py:418-428 over
// sig_proc.py:394-605 `detect_results_to_fpt` (non-refinement branch) and the Cython primitives
// segmentation/_c_segmentation.pyx:41-53 (c_new_means) and :124-161 (c_windowed_t_test), plus the
// scipy.signal.find_peaks(distance=) call at sig_proc.py:183.
//
// Mapping (DESIGN.md "Fingerprint kernel"): ONE WORKGROUP PER READ.  The adapter samples are read
// from HBM exactly once (coalesced), and everything else -- the clipped float32 signal, the
// float64 t-score curve, the peak state bytes, change-points and event means -- lives in LDS until
// the K-point fingerprint is written.  All float64 arithmetic is issued un-fused and in the
// reference's operation order, so t-scores, change-points and fingerprints are bit-identical to
// the CPU path.  Phases:
//   P0 load            HBM -> LDS (float32)
//   P1 MAD clip        two exact medians by range-adaptive radix select over LDS (A1)
//   P2 t-score         window mean/variance M[q],V[q] once per window start (m2(pos) == m1(pos+W)
//                      operation for operation), tiled through LDS, float64 (A3)
//   P3 peaks           local maxima incl. plateaus; greedy minimum-distance suppression as a
//                      fixed-point iteration over the position-space state bytes (A4, App. B)
//   P4 top-E           radix select on the float64 score bits (A4)
//   P5 boundaries      ordered compaction -> change-points
//   P6 event means     sequential float64 sums per segment (A5)
//   P7 normalise+stats numpy pairwise mean/std, medians by rank counting, tail-K extract (A6)
#include "wdx_common.h"
#include "wdx_fp_types.h"
#include "wdx_wave.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

namespace wdx {

// kMaxW, kMaxEvents, kSegCap, the exact kernel's capacities (kExactLdsCap, kBigCap, kLongCap), their slot counts and the LDS
// formulae (fp_lds_bytes, ...): wdx_fp_plan.h, where the host's plan reads the same ones.
constexpr int kTile = 512;       // t-score tile, positions
static_assert(kTile == kExactTile, "the LDS formulae: wdx_fp_plan.h");
constexpr size_t kLongSlotBytes = (size_t)kLongCap * (8 + 4);
// positions fit 16 bits (the peak list's uint16 entries hold positions < ns < kLongCap); one thread's chunk of the state
// bytes fits a 64-bit mask at 1024 threads
static_assert(kLongCap % 64 == 0 && kLongCap <= 65536 && kLongCap > kBigCap && kLongCap <= 64 * 1024, "long form of the exact kernel");

enum : unsigned char { ST_NONE = 0, ST_UNDECIDED = 1, ST_KEPT = 2, ST_DROPPED = 3, ST_SELECTED = 4 };

struct alignas(8) FpShared {
    unsigned long long red64[16];
    unsigned red_a[16], red_b[16], red_c[16];
    unsigned sel_bin, sel_k;
    unsigned long long sel_key64;
    int flag;
    int count;
    float med, mad;
    double mean, sd;
    double stat[6];
};
static_assert(sizeof(FpShared) == kFpSharedBytes, "the LDS formulae: wdx_fp_plan.h");

// ---- block primitives ----------------------------------------------------------------------------

template <int BLOCK>
__device__ __forceinline__ void block_minmax_count(unsigned kmin, unsigned kmax, unsigned cnt,
                                                   FpShared &sh, unsigned &omin, unsigned &omax,
                                                   unsigned &ocnt) {
    for (int off = 32; off > 0; off >>= 1) {
        kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, off));
        kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, off));
        cnt += (unsigned)__shfl_xor((int)cnt, off);
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        sh.red_a[wave] = kmin;
        sh.red_b[wave] = kmax;
        sh.red_c[wave] = cnt;
    }
    __syncthreads();
    omin = 0xffffffffu;
    omax = 0;
    ocnt = 0;
#pragma unroll
    for (int k = 0; k < BLOCK / 64; ++k) {
        omin = min(omin, sh.red_a[k]);
        omax = max(omax, sh.red_b[k]);
        ocnt += sh.red_c[k];
    }
}

template <int BLOCK>
__device__ __forceinline__ void block_minmax64_count(unsigned long long kmin,
                                                     unsigned long long kmax, unsigned cnt,
                                                     FpShared &sh, unsigned long long &omin,
                                                     unsigned long long &omax, unsigned &ocnt) {
    for (int off = 32; off > 0; off >>= 1) {
        unsigned long long a = __shfl_xor(kmin, off), b = __shfl_xor(kmax, off);
        kmin = a < kmin ? a : kmin;
        kmax = b > kmax ? b : kmax;
        cnt += (unsigned)__shfl_xor((int)cnt, off);
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        sh.red64[wave] = kmin;
        sh.red_c[wave] = cnt;
    }
    __syncthreads();
    omin = ~0ull;
    ocnt = 0;
#pragma unroll
    for (int k = 0; k < BLOCK / 64; ++k) {
        omin = sh.red64[k] < omin ? sh.red64[k] : omin;
        ocnt += sh.red_c[k];
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh.red64[wave] = kmax;
    __syncthreads();
    omax = 0;
#pragma unroll
    for (int k = 0; k < BLOCK / 64; ++k) omax = sh.red64[k] > omax ? sh.red64[k] : omax;
}

// After the histogram of one digit is complete: wave 0 finds the bin holding rank k.
__device__ __forceinline__ void select_scan_bins(unsigned *hist, unsigned k, FpShared &sh) {
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        unsigned c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2],
                 c3 = hist[4 * lane + 3];
        unsigned s = c0 + c1 + c2 + c3, incl = s;
        for (int off = 1; off < 64; off <<= 1) {
            unsigned t = (unsigned)__shfl_up((int)incl, off);
            if (lane >= off) incl += t;
        }
        unsigned e = incl - s;
        if (k >= e && k < e + s) {
            unsigned bin = 4 * lane, kk = k - e;
            if (kk >= c0) { kk -= c0; bin++;
                if (kk >= c1) { kk -= c1; bin++;
                    if (kk >= c2) { kk -= c2; bin++; } } }
            sh.sel_bin = bin;
            sh.sel_k = kk;
        }
    }
}

// k-th smallest (0-based) 32-bit key among the valid items; keyfn(i, key) -> valid.
// All threads must call; 0 <= k < n_valid; kmin/kmax are the exact extremes of the valid keys.
template <int BLOCK, class KeyFn>
__device__ unsigned block_select_u32(KeyFn keyfn, int n, unsigned k, unsigned kmin, unsigned kmax,
                                     unsigned *hist, FpShared &sh) {
    const unsigned range = kmax - kmin;
    int rb = range ? 32 - __clz((int)range) : 0;
    unsigned prefix = 0;
    while (rb > 0) {
        const int b = rb < 8 ? rb : 8;
        const int shift = rb - b;
        for (int t = threadIdx.x; t < 256; t += BLOCK) hist[t] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += BLOCK) {
            unsigned key;
            if (keyfn(i, key)) {
                unsigned d = key - kmin;
                unsigned hi = rb >= 32 ? 0u : (d >> rb);
                if (hi == prefix) atomicAdd(&hist[(d >> shift) & ((1u << b) - 1u)], 1u);
            }
        }
        __syncthreads();
        select_scan_bins(hist, k, sh);
        __syncthreads();
        prefix = (prefix << b) | sh.sel_bin;
        k = sh.sel_k;
        rb = shift;
    }
    return kmin + prefix;
}

template <int BLOCK, class KeyFn>
__device__ unsigned long long block_select_u64(KeyFn keyfn, int n, unsigned k,
                                               unsigned long long kmin, unsigned long long kmax,
                                               unsigned *hist, FpShared &sh) {
    const unsigned long long range = kmax - kmin;
    int rb = range ? 64 - __clzll((long long)range) : 0;
    unsigned long long prefix = 0;
    while (rb > 0) {
        const int b = rb < 8 ? rb : 8;
        const int shift = rb - b;
        for (int t = threadIdx.x; t < 256; t += BLOCK) hist[t] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += BLOCK) {
            unsigned long long key;
            if (keyfn(i, key)) {
                unsigned long long d = key - kmin;
                unsigned long long hi = rb >= 64 ? 0ull : (d >> rb);
                if (hi == prefix) atomicAdd(&hist[(unsigned)(d >> shift) & ((1u << b) - 1u)], 1u);
            }
        }
        __syncthreads();
        select_scan_bins(hist, k, sh);
        __syncthreads();
        prefix = (prefix << b) | sh.sel_bin;
        k = sh.sel_k;
        rb = shift;
    }
    return kmin + prefix;
}

// np.nanmedian over the float32 values val(i) (NaN = invalid): exact, float32 result.
template <int BLOCK, class ValFn>
__device__ float block_nanmedian_f32(ValFn val, int n, unsigned *hist, FpShared &sh) {
    unsigned kmin = 0xffffffffu, kmax = 0, cnt = 0;
    for (int i = threadIdx.x; i < n; i += BLOCK) {
        float v = val(i);
        if (v == v) {
            unsigned k = f32_key(v);
            kmin = min(kmin, k);
            kmax = max(kmax, k);
            cnt++;
        }
    }
    unsigned gmin, gmax, m;
    block_minmax_count<BLOCK>(kmin, kmax, cnt, sh, gmin, gmax, m);
    if (m == 0) return __builtin_nanf("");
    auto keyfn = [&](int i, unsigned &key) {
        float v = val(i);
        key = f32_key(v);
        return v == v;
    };
    const unsigned h = m / 2;
    if (m & 1) return key_f32(block_select_u32<BLOCK>(keyfn, n, h, gmin, gmax, hist, sh));
    // even: ranks h-1 and h.  khi = klo if more than h keys are <= klo, else the next larger key.
    const unsigned klo = block_select_u32<BLOCK>(keyfn, n, h - 1, gmin, gmax, hist, sh);
    unsigned nxt = 0xffffffffu, dummy = 0, le = 0;
    for (int i = threadIdx.x; i < n; i += BLOCK) {
        unsigned key;
        if (keyfn(i, key)) {
            if (key <= klo) le++;
            else nxt = min(nxt, key);
        }
    }
    unsigned gnxt, gdummy, gle;
    block_minmax_count<BLOCK>(nxt, dummy, le, sh, gnxt, gdummy, gle);
    const unsigned khi = gle > h ? klo : gnxt;
    const float s = key_f32(klo) + key_f32(khi);
    return s / 2.0f;
}

// numpy pairwise float64 summation (loops_utils.h.src::pairwise_sum), single thread.
__device__ __forceinline__ double np_pairwise_leaf(const double *p, int n) {  // n <= 128
    double res;
    if (n < 8) {
        res = 0.0;
        for (int i = 0; i < n; ++i) res += p[i];
    } else {
        double r0 = p[0], r1 = p[1], r2 = p[2], r3 = p[3], r4 = p[4], r5 = p[5], r6 = p[6],
               r7 = p[7];
        int i;
        for (i = 8; i < n - (n % 8); i += 8) {
            r0 += p[i]; r1 += p[i + 1]; r2 += p[i + 2]; r3 += p[i + 3];
            r4 += p[i + 4]; r5 += p[i + 5]; r6 += p[i + 6]; r7 += p[i + 7];
        }
        res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
        for (; i < n; ++i) res += p[i];
    }
    return res;
}
template <int kDepth>
__device__ double np_pairwise_tree(const double *a, int n) {
    if constexpr (kDepth == 0) {
        return np_pairwise_leaf(a, n);
    } else {
        if (n <= 128) return np_pairwise_leaf(a, n);
        int n2 = n / 2;
        n2 -= n2 % 8;
        return np_pairwise_tree<kDepth - 1>(a, n2) + np_pairwise_tree<kDepth - 1>(a + n2, n - n2);
    }
}
// n <= kSegCap + 1 = 255: two levels of the recursion.  The split point is rounded DOWN to a multiple of 8, so the right
// half of n = 249 .. 255 still holds 129 .. 135 values and is split once more (120 + 134 -> 120 + (64 + 70) for 254)
__device__ double np_pairwise_sum_dev(const double *a, int n) { return np_pairwise_tree<2>(a, n); }

// np.add.reduce over the float32 values val(0..n): NumPy's exact association -- the ufunc hands the inner loop at
// most 8192 elements (np.getbufsize()) at a time, each chunk is summed by the pairwise routine (leaves of <= 128
// elements with 8 accumulators, halves split at multiples of 8), chunk sums accumulate left to right.  The leaves
// are independent: thread 0 lists them, one thread sums each, thread 0 folds them back up the same tree.
// lstart: >= 258 unsigned, lsum: >= 257 floats, stk: >= 48 ints (all LDS).  Result to every thread.
template <int BLOCK, class ValFn>
__device__ float block_np_add_reduce_f32(ValFn val, int n, unsigned *lstart, float *lsum, int *stk, FpShared &sh) {
    constexpr int kBuf = 8192;
    __syncthreads();
    if (threadIdx.x == 0) {
        int nl = 0;
        for (int c = 0; c < n || c == 0; c += kBuf) {
            const int m = min(kBuf, n - c);
            // depth-first, left before right: leaves come out in increasing start order
            int sp = 0;
            stk[0] = c;
            stk[1] = m;
            sp = 1;
            while (sp > 0) {
                --sp;
                const int lo = stk[2 * sp], len = stk[2 * sp + 1];
                if (len <= 128) {
                    lstart[nl++] = (unsigned)lo;
                } else {
                    int n2 = len / 2;
                    n2 -= n2 % 8;
                    stk[2 * sp] = lo + n2;       // right half: popped second
                    stk[2 * sp + 1] = len - n2;
                    ++sp;
                    stk[2 * sp] = lo;            // left half: popped first
                    stk[2 * sp + 1] = n2;
                    ++sp;
                }
            }
            if (n == 0) break;
        }
        lstart[nl] = (unsigned)n;
        sh.count = nl;
    }
    __syncthreads();
    const int nl = sh.count;
    for (int l = threadIdx.x; l < nl; l += BLOCK) {
        const int lo = (int)lstart[l];
        // a leaf ends at the next leaf's start, and never crosses an 8192-element chunk
        const int hi = min((int)lstart[l + 1], (lo / kBuf + 1) * kBuf);
        const int len = hi - lo;
        float res;
        if (len < 8) {
            res = 0.0f;
            for (int i = 0; i < len; ++i) res += val(lo + i);
        } else {
            float r0 = val(lo), r1 = val(lo + 1), r2 = val(lo + 2), r3 = val(lo + 3), r4 = val(lo + 4),
                  r5 = val(lo + 5), r6 = val(lo + 6), r7 = val(lo + 7);
            int i;
            for (i = 8; i < len - (len % 8); i += 8) {
                r0 += val(lo + i); r1 += val(lo + i + 1); r2 += val(lo + i + 2); r3 += val(lo + i + 3);
                r4 += val(lo + i + 4); r5 += val(lo + i + 5); r6 += val(lo + i + 6); r7 += val(lo + i + 7);
            }
            res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
            for (; i < len; ++i) res += val(lo + i);
        }
        lsum[l] = res;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float total = 0.0f;
        int li = 0;
        for (int c = 0; c < n || c == 0; c += kBuf) {
            const int m = min(kBuf, n - c);
            // post-order fold: frame = (len, phase), value stack alongside (float bits in the int array)
            float ret = 0.0f;
            int sp = 0;
            stk[0] = m;
            stk[1] = 0;
            sp = 1;
            while (sp > 0) {
                int &len = stk[3 * (sp - 1)], &phase = stk[3 * (sp - 1) + 1], &left = stk[3 * (sp - 1) + 2];
                if (phase == 0) {
                    if (len <= 128) {
                        ret = lsum[li++];
                        --sp;
                    } else {
                        int n2 = len / 2;
                        n2 -= n2 % 8;
                        phase = 1;
                        stk[3 * sp] = n2;
                        stk[3 * sp + 1] = 0;
                        ++sp;
                    }
                } else if (phase == 1) {
                    left = __float_as_int(ret);
                    phase = 2;
                    int n2 = len / 2;
                    n2 -= n2 % 8;
                    stk[3 * sp] = len - n2;
                    stk[3 * sp + 1] = 0;
                    ++sp;
                } else {
                    ret = __int_as_float(left) + ret;
                    --sp;
                }
            }
            total = (c == 0) ? ret : total + ret;
            if (n == 0) break;
        }
        sh.med = total;
    }
    __syncthreads();
    const float out = sh.med;
    __syncthreads();
    return out;
}

// np.median of n <= kSegCap float64 values in LDS (no NaN) by rank counting; result via sh.stat[slot]
template <int BLOCK>
__device__ void block_small_median(const double *a, int n, FpShared &sh, int slot) {
    const int klo = (n - 1) / 2, khi = n / 2;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += BLOCK) {
        const double v = a[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const double u = a[j];
            rank += (u < v) || (u == v && j < i);
        }
        if (rank == klo) sh.red64[0] = (unsigned long long)__double_as_longlong(v);
        if (rank == khi) sh.red64[1] = (unsigned long long)__double_as_longlong(v);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double lo = __longlong_as_double((long long)sh.red64[0]);
        double hi = __longlong_as_double((long long)sh.red64[1]);
        sh.stat[slot] = (n & 1) ? hi : (lo + hi) / 2.0;
    }
    __syncthreads();
}

// find_peaks(scores[0..ns), distance=d_eff) -> the E highest -> boundaries 0, peaks + W, n_end
// -> event means over sig (sig_proc.py:176-198, segmentation.py:48-74).  Used for the adapter and, in the
// consensus-refinement branch, once more for the barcode tail of the same score curve.  All threads call;
// returns a block-uniform WDX_READ_* status; on success cpts[0..nseg] and ev[0..nseg).
// block-wide exclusive scan of one int per thread (chunk counts); total = block sum.  Two barriers.
template <int BLOCK>
__device__ __forceinline__ int block_excl_scan(int v, FpShared &sh, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    __syncthreads();  // sh.red_a may still be read by the previous user
    if (lane == 63) sh.red_a[wave] = (unsigned)incl;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < BLOCK / 64; ++k) {
        const int w = (int)sh.red_a[k];
        base += k < wave ? w : 0;
        total += w;
    }
    return base + incl - v;
}

// WIDE (the long form, ns up to kLongCap): a thread's chunk of the state bytes is up to 64 positions -- a 64-bit mask
template <int BLOCK, bool WIDE = false>
__device__ int fp_segment(const double *scores, unsigned char *state, const int ns, const int d_eff, const int W,
                          const int E, const bool accept_less, const float *sig, const int n_end, int *cpts, double *ev,
                          unsigned *hist, FpShared &sh, int &nseg, int &nms_iters, const bool no_list = false,
                          const bool exact_sums = false) {
    const int tid = threadIdx.x;
    // ---- P3: find_peaks(scores, distance=d_eff) ----------------------------------
    for (int i = tid; i < ns; i += BLOCK) state[i] = ST_NONE;
    __syncthreads();
    for (int i = 1 + tid; i < ns - 1; i += BLOCK) {
        const double s = scores[i];
        if (scores[i - 1] < s) {
            int ia = i + 1;
            while (ia < ns - 1 && scores[ia] == s) ++ia;
            if (scores[ia] < s) state[(i + ia - 1) / 2] = ST_UNDECIDED;
        }
    }
    __syncthreads();
    // The local maxima (about ns / 5.6 of the positions) are compacted into a position-ordered LIST that overwrites
    // the state bytes in place -- uint16 positions, then one state byte per peak: 3 bytes per peak against one byte per
    // position, so it fits whenever np <= ns / 3 (else, and with WDX_OPT_EXACT_NO_PEAK_LIST, the position-space
    // code below runs; same decisions, same results).  Suppression, the top-E cut and the boundaries then walk
    // ~ns / 5.6 entries instead of ns positions: the suppression's neighbourhood scan is a few list entries instead
    // of 2 (d - 1) state bytes, and every pass of the select is 5.6x shorter.
    int nsel;
    bool use_list;
    int np = 0, lbase = 0;
    // (WIDE at 512 threads -- the refining long kernel -- : up to 128 positions, two 64-bit words)
    constexpr int kLBits = WIDE ? (BLOCK >= 1024 ? 64 : 128) : 32;
    using LBits = typename std::conditional<!WIDE, unsigned,
                                            typename std::conditional<kLBits == 64, unsigned long long, unsigned __int128>::type>::type;
    LBits lbits = 0;
    const int lchunk = (ns + BLOCK - 1) / BLOCK;  // <= 32: cap <= 16 384, BLOCK >= 512 (WIDE: <= 64 at 1024 threads, <= 128 at 512; cap <= 65 536)
    const int lc0 = tid * lchunk;
    {
        const int lc1 = min(ns, lc0 + lchunk);
        for (int i = lc0; i < lc1; ++i) lbits |= (LBits)(state[i] == ST_UNDECIDED ? 1u : 0u) << (i - lc0);
        int lcount;
        if constexpr (kLBits == 128) lcount = __popcll((unsigned long long)lbits) + __popcll((unsigned long long)(lbits >> 64));
        else if constexpr (WIDE) lcount = __popcll(lbits);
        else lcount = __popc(lbits);
        lbase = block_excl_scan<BLOCK>(lcount, sh, np);  // (its barriers: every state byte has been read)
        use_list = !no_list && lchunk <= kLBits && 3 * np + 8 <= ns;
    }
    if (use_list) {
        unsigned short *lpos = reinterpret_cast<unsigned short *>(state);
        unsigned char *lst = state + ((2 * np + 3) & ~3);
        {
            int o = lbase;
            LBits b = lbits;
            while (b) {
                int j;
                if constexpr (kLBits == 128) {
                    const unsigned long long b_lo = (unsigned long long)b;
                    j = b_lo ? __ffsll(b_lo) - 1 : 63 + __ffsll((unsigned long long)(b >> 64));
                } else if constexpr (WIDE) j = __ffsll((unsigned long long)b) - 1;
                else j = __ffs((int)b) - 1;
                b &= b - 1;
                lpos[o] = (unsigned short)(lc0 + j);
                lst[o] = ST_UNDECIDED;
                ++o;
            }
        }
        __syncthreads();
        // greedy suppression by priority (see the position-space form below for the rule): a peak's rivals are the list
        // neighbours closer than d_eff; ties -> the LATER peak outranks.  Only the rivals that OUTRANK a peak decide
        // about it (a lower-ranked rival stays undecided for as long as this peak is), and which those are never
        // changes: each thread finds them once -- a 16-bit mask over the up to eight list neighbours on either side
        // (local maxima are at least two positions apart, d_eff <= 17) -- and the rounds only re-read their state bytes.
        constexpr int kNmsPer = 4;   // list entries per thread held in registers
        if (d_eff <= 17 && np <= kNmsPer * BLOCK) {
            unsigned hp[kNmsPer];
            bool und[kNmsPer];
#pragma unroll
            for (int m = 0; m < kNmsPer; ++m) {
                const int k = tid + m * BLOCK;
                hp[m] = 0;
                und[m] = k < np;
                if (k < np) {
                    const int p = lpos[k];
                    const double s = scores[p];
                    for (int q = k - 1; q >= 0 && p - (int)lpos[q] < d_eff; --q)
                        if (scores[lpos[q]] > s) hp[m] |= 1u << (q - k + 8);
                    for (int q = k + 1; q < np && (int)lpos[q] - p < d_eff; ++q) {
                        const double sq = scores[lpos[q]];
                        if (sq > s || sq == s) hp[m] |= 1u << (q - k + 7);
                    }
                }
            }
            for (;;) {
                int pending = 0;
#pragma unroll
                for (int m = 0; m < kNmsPer; ++m) {
                    if (!und[m]) continue;
                    const int k = tid + m * BLOCK;
                    bool kept_near = false, wait = false;
                    unsigned mask = hp[m];
                    while (mask) {
                        const int b = __ffs((int)mask) - 1;
                        mask &= mask - 1;
                        const unsigned char st = lst[k + (b < 8 ? b - 8 : b - 7)];
                        kept_near |= st == ST_KEPT;
                        wait |= st == ST_UNDECIDED;
                    }
                    if (kept_near) { lst[k] = ST_DROPPED; und[m] = false; }
                    else if (!wait) { lst[k] = ST_KEPT; und[m] = false; }
                    else pending = 1;
                }
                ++nms_iters;
                if (!__syncthreads_or(pending)) break;
            }
        } else
        for (;;) {
            int pending = 0;
            for (int k = tid; k < np; k += BLOCK) {
                if (lst[k] != ST_UNDECIDED) continue;
                const int p = lpos[k];
                const double s = scores[p];
                bool kept_near = false, wait = false;
                for (int q = k - 1; q >= 0 && p - (int)lpos[q] < d_eff; --q) {
                    const unsigned char st = lst[q];
                    if (st == ST_KEPT) kept_near = true;
                    else if (st == ST_UNDECIDED && scores[lpos[q]] > s) wait = true;
                }
                for (int q = k + 1; q < np && (int)lpos[q] - p < d_eff; ++q) {
                    const unsigned char st = lst[q];
                    if (st == ST_KEPT) kept_near = true;
                    else if (st == ST_UNDECIDED) {
                        const double sq = scores[lpos[q]];
                        if (sq > s || sq == s) wait = true;
                    }
                }
                if (kept_near) lst[k] = ST_DROPPED;
                else if (!wait) lst[k] = ST_KEPT;
                else pending = 1;
            }
            ++nms_iters;
            if (!__syncthreads_or(pending)) break;
        }
        // ---- P4 on the list: keep the E highest peaks (sig_proc.py:185-188) --------------------------
        unsigned long long kmin = ~0ull, kmax = 0;
        unsigned cnt = 0;
        for (int k = tid; k < np; k += BLOCK) {
            if (lst[k] == ST_KEPT) {
                const unsigned long long key = (unsigned long long)__double_as_longlong(scores[lpos[k]]);
                kmin = key < kmin ? key : kmin;
                kmax = key > kmax ? key : kmax;
                cnt++;
            }
        }
        unsigned long long gmin, gmax;
        unsigned nk;
        block_minmax64_count<BLOCK>(kmin, kmax, cnt, sh, gmin, gmax, nk);
        if ((int)nk < E && !accept_less) return WDX_READ_FAIL_SEGMENT;
        if (nk == 0) return WDX_READ_FAIL_UNKNOWN;  // valid_cpts[0] on an empty array
        if ((int)nk <= E) {
            nsel = (int)nk;
            __syncthreads();
            for (int k = tid; k < np; k += BLOCK)
                if (lst[k] == ST_KEPT) lst[k] = ST_SELECTED;
        } else if ((int)nk <= kSegCap) {
            // few survivors (a barcode tail: ~100): their keys go, in list order, to a dense array and every survivor
            // counts the ones that outrank it (larger score; equal score and later) -- one pass instead of the seven
            // digit passes of the radix select below
            nsel = E;
            unsigned long long *dk = reinterpret_cast<unsigned long long *>(ev);   // (free until P6)
            unsigned short *dmap = reinterpret_cast<unsigned short *>(hist);
            const int c2 = (np + BLOCK - 1) / BLOCK;
            const int k0 = tid * c2, k1 = min(np, k0 + c2);
            int local = 0;
            for (int k = k0; k < k1; ++k) local += lst[k] == ST_KEPT;
            int tot;
            int o = block_excl_scan<BLOCK>(local, sh, tot);
            for (int k = k0; k < k1; ++k)
                if (lst[k] == ST_KEPT) {
                    dk[o] = (unsigned long long)__double_as_longlong(scores[lpos[k]]);
                    dmap[o] = (unsigned short)k;
                    ++o;
                }
            __syncthreads();
            for (int t = tid; t < (int)nk; t += BLOCK) {
                const unsigned long long key = dk[t];
                int rank = 0;
                for (int j = 0; j < (int)nk; ++j) {
                    const unsigned long long kj = dk[j];
                    rank += (kj > key) || (kj == key && j > t);
                }
                if (rank < E) lst[dmap[t]] = ST_SELECTED;
            }
        } else {
            nsel = E;
            auto keyfn = [&](int k, unsigned long long &key) {
                key = (unsigned long long)__double_as_longlong(scores[lpos[k]]);
                return lst[k] == ST_KEPT;
            };
            const unsigned long long T = block_select_u64<BLOCK>(keyfn, np, nk - (unsigned)E, gmin, gmax, hist, sh);
            unsigned gt = 0, eq = 0, z0 = 0xffffffffu;
            for (int k = tid; k < np; k += BLOCK) {
                if (lst[k] == ST_KEPT) {
                    const unsigned long long key = (unsigned long long)__double_as_longlong(scores[lpos[k]]);
                    gt += key > T;
                    eq += key == T;
                }
            }
            unsigned ggt, geq, dmy;
            block_minmax_count<BLOCK>(z0, gt, eq, sh, dmy, dmy, geq);  // geq = sum(eq)
            block_minmax_count<BLOCK>(z0, 0u, gt, sh, dmy, dmy, ggt);  // ggt = sum(gt)
            const unsigned need = (unsigned)E - ggt;  // 1 <= need <= geq
            __syncthreads();
            for (int k = tid; k < np; k += BLOCK) {
                if (lst[k] == ST_KEPT) {
                    const unsigned long long key = (unsigned long long)__double_as_longlong(scores[lpos[k]]);
                    if (key > T || (key == T && need == geq)) lst[k] = ST_SELECTED;
                }
            }
            __syncthreads();
            if (need != geq && tid == 0) {
                // exact score ties at the cut: the stable order keeps the LAST `need` of them
                unsigned left = need;
                for (int k = np - 1; k >= 0 && left; --k) {
                    if (lst[k] == ST_KEPT && (unsigned long long)__double_as_longlong(scores[lpos[k]]) == T) {
                        lst[k] = ST_SELECTED;
                        --left;
                    }
                }
            }
        }
        __syncthreads();
        // ---- P5 on the list: boundaries 0, peaks+W (ascending), n  (sig_proc.py:188-196) ---------------
        {
            const int c2 = (np + BLOCK - 1) / BLOCK;
            const int k0 = tid * c2, k1 = min(np, k0 + c2);
            int local = 0;
            for (int k = k0; k < k1; ++k) local += lst[k] == ST_SELECTED;
            int tot;
            int o = block_excl_scan<BLOCK>(local, sh, tot);
            for (int k = k0; k < k1; ++k)
                if (lst[k] == ST_SELECTED) cpts[1 + o++] = (int)lpos[k] + W;
            if (tid == 0) {
                cpts[0] = 0;
                cpts[nsel + 1] = n_end;
            }
            __syncthreads();
        }
    } else {
    {
        // greedy suppression by priority == fixed point of: a peak is KEPT once every higher-priority
        // peak closer than d_eff is DROPPED, and DROPPED as soon as one of them is KEPT.
        // priority order: score, ties -> larger position first (stable argsort read from the end).
        const int D1 = d_eff - 1;
        for (;;) {
            int pending = 0;
            for (int i = tid; i < ns; i += BLOCK) {
                if (state[i] != ST_UNDECIDED) continue;
                const double s = scores[i];
                bool kept_near = false, wait = false;
                const int lo = max(0, i - D1), hi = min(ns - 1, i + D1);
                for (int q = lo; q <= hi; ++q) {
                    if (q == i) continue;
                    const unsigned char st = state[q];
                    if (st == ST_KEPT) kept_near = true;
                    else if (st == ST_UNDECIDED) {
                        const double sq = scores[q];
                        if (sq > s || (sq == s && q > i)) wait = true;
                    }
                }
                if (kept_near) state[i] = ST_DROPPED;
                else if (!wait) state[i] = ST_KEPT;
                else pending = 1;
            }
            ++nms_iters;
            if (!__syncthreads_or(pending)) break;
        }
    }

    // ---- P4: keep the E highest peaks (sig_proc.py:185-188) -----------------------------------------
    {
        unsigned long long kmin = ~0ull, kmax = 0;
        unsigned cnt = 0;
        for (int i = tid; i < ns; i += BLOCK) {
            if (state[i] == ST_KEPT) {
                unsigned long long k = (unsigned long long)__double_as_longlong(scores[i]);
                kmin = k < kmin ? k : kmin;
                kmax = k > kmax ? k : kmax;
                cnt++;
            }
        }
        unsigned long long gmin, gmax;
        unsigned nk;
        block_minmax64_count<BLOCK>(kmin, kmax, cnt, sh, gmin, gmax, nk);
        if ((int)nk < E && !accept_less) return WDX_READ_FAIL_SEGMENT;
        if (nk == 0) return WDX_READ_FAIL_UNKNOWN;  // valid_cpts[0] on an empty array
        if ((int)nk <= E) {
            nsel = (int)nk;
            __syncthreads();
            for (int i = tid; i < ns; i += BLOCK)
                if (state[i] == ST_KEPT) state[i] = ST_SELECTED;
        } else {
            nsel = E;
            auto keyfn = [&](int i, unsigned long long &key) {
                key = (unsigned long long)__double_as_longlong(scores[i]);
                return state[i] == ST_KEPT;
            };
            const unsigned long long T =
                block_select_u64<BLOCK>(keyfn, ns, nk - (unsigned)E, gmin, gmax, hist, sh);
            unsigned gt = 0, eq = 0, z0 = 0xffffffffu;
            for (int i = tid; i < ns; i += BLOCK) {
                if (state[i] == ST_KEPT) {
                    unsigned long long k = (unsigned long long)__double_as_longlong(scores[i]);
                    gt += k > T;
                    eq += k == T;
                }
            }
            unsigned ggt, geq, dmy;
            block_minmax_count<BLOCK>(z0, gt, eq, sh, dmy, dmy, geq);  // geq = sum(eq)
            block_minmax_count<BLOCK>(z0, 0u, gt, sh, dmy, dmy, ggt);  // ggt = sum(gt)
            const unsigned need = (unsigned)E - ggt;  // 1 <= need <= geq
            __syncthreads();
            for (int i = tid; i < ns; i += BLOCK) {
                if (state[i] == ST_KEPT) {
                    unsigned long long k = (unsigned long long)__double_as_longlong(scores[i]);
                    if (k > T || (k == T && need == geq)) state[i] = ST_SELECTED;
                }
            }
            __syncthreads();
            if (need != geq && tid == 0) {
                // exact score ties at the cut: the stable order keeps the LAST `need` of them
                unsigned left = need;
                for (int i = ns - 1; i >= 0 && left; --i) {
                    if (state[i] == ST_KEPT &&
                        (unsigned long long)__double_as_longlong(scores[i]) == T) {
                        state[i] = ST_SELECTED;
                        --left;
                    }
                }
            }
        }
        __syncthreads();
    }

    // ---- P5: boundaries 0, peaks+W (ascending), n  (sig_proc.py:188-196) -----------------------------
    {
        const int chunk = (ns + BLOCK - 1) / BLOCK;
        const int c0 = tid * chunk, c1 = min(ns, c0 + chunk);
        int local = 0;
        for (int i = c0; i < c1; ++i) local += state[i] == ST_SELECTED;
        // block exclusive scan of `local`
        int incl = local;
        const int lane = tid & 63, wave = tid >> 6;
        for (int off = 1; off < 64; off <<= 1) {
            int t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        if (lane == 63) sh.red_a[wave] = (unsigned)incl;
        __syncthreads();
        int base = 0;
        for (int k = 0; k < wave; ++k) base += (int)sh.red_a[k];
        int o = base + incl - local;
        for (int i = c0; i < c1; ++i)
            if (state[i] == ST_SELECTED) cpts[1 + o++] = i + W;
        if (tid == 0) {
            cpts[0] = 0;
            cpts[nsel + 1] = n_end;
        }
        __syncthreads();
    }
    }
    nseg = nsel + 1;

    // ---- P6: event means (_c_segmentation.pyx:41-53), sequential float64 sums ------------------------
    // exact_sums (the caller's promise: every partial sum of the samples is exactly representable in float64 -- positive
    // float32 samples within a factor 2^16 of each other): the sum does not depend on its order, eight lanes share a segment
    if (exact_sums) {
        const int j = tid & 7;
        for (int s0 = 0; s0 < nseg; s0 += BLOCK / 8) {   // block-uniform trip count: the shuffles see whole waves
            const int s = s0 + (tid >> 3);
            double sum = 0.0;
            int b = 0, e = 1;
            if (s < nseg) {
                b = cpts[s];
                e = cpts[s + 1];
                for (int i = b + j; i < e; i += 8) sum += (double)sig[i];
            }
            sum += __shfl_xor(sum, 4);
            sum += __shfl_xor(sum, 2);
            sum += __shfl_xor(sum, 1);
            if (s < nseg && j == 0) ev[s] = sum / (double)(e - b);
        }
    } else
    for (int s = tid; s < nseg; s += BLOCK) {
        const int b = cpts[s], e = cpts[s + 1];
        double sum = 0.0;
        for (int i = b; i < e; ++i) sum += (double)sig[i];
        ev[s] = sum / (double)(e - b);
    }
    __syncthreads();

    return WDX_READ_OK;
}

// Consensus-guided barcode refinement, everything after the adapter's segmentation (sig_proc.py:287-378,
// 452-521; oracle: fingerprint_refine_one_impl).  The subsequence match (dtaidistance warping_paths_fast +
// SubsequenceAlignment.best_match, restated -- parity unpinned) is an anti-diagonal wavefront:
// thread i owns query row i, front k holds the cells (i, k - i); a cell needs the two previous fronts only, so
// three fronts of (cost, sqrt(cost)) pairs rotate through LDS, and what the back-trace needs -- argmin of the
// three predecessors' sqrt'ed costs per cell, first minimum -- is kept as 2-bit codes, 16 per word, one row of
// words per thread.  scratch: >= 3*(nq+1)*16 + nq*ceil(nseries/16)*4 bytes of LDS (the t-score tile buffers).
// `prep(sbs, ns2, scores_tail, sig_tail)` is called (block-uniform) once the barcode's first sample `sbs` is known and
// hands back the score curve and the clipped samples FROM `sbs` ON: the exact kernel has both in LDS already
// (scores + sbs, sig + sbs); fingerprint_refine_tail_kernel -- the refinement behind the fast kernels -- loads and
// scores only that tail.  Returning false leaves the read untouched (the caller hands it on).
// The branch comes in two halves so that the kernel behind the fast kernels can run them as two launches with very
// different LDS needs (the match is pure latency and wants many resident workgroups; the barcode's segmentation
// needs the tail's samples and scores): fp_refine_match -- adapter statistics, subsequence match, back-trace ->
// RefineMatch (false: the read has been reported, nothing more to do) -- and fp_refine_finish.
template <int BLOCK>
__device__ bool fp_refine_match(const FpArgs &A, const int64_t r, const int *cpts, double *ev, double *zz, double *tmp,
                                unsigned char *scratch, FpShared &sh, const int nseg, RefineMatch &M) {
    const int tid = threadIdx.x;
    const wdx_seg_params &P = A.p;
    const RefineDev &R = A.rf;
    const int K = P.barcode_num_events;  // = barcode_num_events[1], set by the host
    auto finish = [&](int st, bool with_stats) {
        if (st != WDX_READ_OK) {
            for (int i = tid; i < K; i += BLOCK) {
                if (A.fpt) A.fpt[r * K + i] = __builtin_nan("");
                if (A.dwell) A.dwell[r * K + i] = 0;
            }
            if (!with_stats) {
                if (A.stats && tid < 6) A.stats[r * 6 + tid] = __builtin_nan("");
                if (R.idx && tid < 3) R.idx[r * 3 + tid] = -1;
            }
        }
        if (tid == 0) A.status[r] = st;
    };
    // normalize(series, method, accept_nan=False) inside _get_subseq_match raises on NaN -> "unknown"
    {
        int has_nan = 0;
        for (int s = tid; s < nseg; s += BLOCK) has_nan |= (ev[s] != ev[s]);
        if (__syncthreads_or(has_nan)) {
            finish(WDX_READ_FAIL_UNKNOWN, false);
            return false;
        }
    }
    // adapter statistics (sig_proc.py:486-494) and the shift / scale of both normalisations
    if (tid == 0) sh.mean = np_pairwise_sum_dev(ev, nseg) / (double)nseg;
    __syncthreads();
    const double mean = sh.mean;
    for (int s = tid; s < nseg; s += BLOCK) {
        const double df = ev[s] - mean;
        tmp[s] = df * df;
    }
    __syncthreads();
    if (tid == 0) sh.sd = sqrt(np_pairwise_sum_dev(tmp, nseg) / (double)nseg);
    __syncthreads();
    const double sd = sh.sd;
    for (int s = tid; s < nseg; s += BLOCK) tmp[s] = (double)(cpts[s + 1] - cpts[s]);
    block_small_median<BLOCK>(tmp, nseg, sh, 0);
    const double dt_med = sh.stat[0];
    for (int s = tid; s < nseg; s += BLOCK) tmp[s] = fabs(tmp[s] - dt_med);
    block_small_median<BLOCK>(tmp, nseg, sh, 1);
    block_small_median<BLOCK>(ev, nseg, sh, 4);
    const double ev_med = sh.stat[4];
    for (int s = tid; s < nseg; s += BLOCK) tmp[s] = fabs(ev[s] - ev_med);
    block_small_median<BLOCK>(tmp, nseg, sh, 5);
    const double ev_mad = sh.stat[5];
    const double dt_mad = sh.stat[1];
    // series of the match: normalize(adapter_event_means, consensus_subseq_match_normalization)
    {
        double c0 = 0.0, c1 = 1.0;
        if (R.norm == WDX_NORM_MEAN) { c0 = mean; c1 = sd; }
        else if (R.norm == WDX_NORM_MEDIAN) { c0 = ev_med; c1 = ev_mad; }
        else if (R.norm != WDX_NORM_NONE) { finish(WDX_READ_FAIL_UNKNOWN, false); return false; }
        int bad = 0;
        for (int s = tid; s < nseg; s += BLOCK) {
            const double v = R.norm == WDX_NORM_NONE ? ev[s] : (ev[s] - c0) / c1;
            zz[s] = v;
            bad |= (v != v);
        }
        if (__syncthreads_or(bad)) {  // a constant series (0/0): the library's behaviour on NaN is not restated
            finish(WDX_READ_FAIL_UNKNOWN, false);
            return false;
        }
    }
    // ---- subsequence DTW of the consensus query against the normalised event means ------------------------
    const int nq = R.nq, c = nseg, WPR = (c + 15) >> 4;
    struct DS { double D, S; };
    DS *F = reinterpret_cast<DS *>(scratch);
    unsigned *dirw = reinterpret_cast<unsigned *>(F + 3 * (nq + 1));
    double *lastS = tmp;
    {
        const double p2 = R.pen * R.pen, inf = __builtin_huge_val();
        const double qi = (tid >= 1 && tid <= nq) ? R.query[tid - 1] : 0.0;
        unsigned acc = 0;
        for (int k = 0; k <= nq + c; ++k) {
            if (tid <= nq) {
                const int i = tid, j = k - i;
                if (j >= 0 && j <= c) {
                    DS out;
                    if (i == 0) {
                        out.D = j <= R.psi2b ? 0.0 : inf;
                        out.S = out.D;
                    } else if (j == 0) {
                        out.D = i <= R.psi1b ? 0.0 : inf;
                        out.S = out.D;
                    } else {
                        const DS dg = F[((k - 2) % 3) * (nq + 1) + i - 1], up = F[((k - 1) % 3) * (nq + 1) + i - 1],
                                 lf = F[((k - 1) % 3) * (nq + 1) + i];
                        double d = qi - zz[j - 1];
                        d = d * d;
                        double m = dg.D, t = up.D + p2;
                        if (t < m) m = t;
                        t = lf.D + p2;
                        if (t < m) m = t;
                        out.D = d + m;
                        out.S = sqrt(out.D);
                        unsigned code = 0;
                        double mv = dg.S;
                        if (up.S < mv) { mv = up.S; code = 1; }
                        if (lf.S < mv) code = 2;
                        acc |= code << (2 * ((j - 1) & 15));
                        if (((j - 1) & 15) == 15 || j == c) {
                            dirw[(i - 1) * WPR + ((j - 1) >> 4)] = acc;
                            acc = 0;
                        }
                        if (i == nq) lastS[j - 1] = out.S;
                    }
                    F[(k % 3) * (nq + 1) + i] = out;
                }
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        int best = 0;
        double bv = lastS[0] / (double)nq;
        for (int j = 1; j < c; ++j) {
            const double v = lastS[j] / (double)nq;
            if (v < bv) { bv = v; best = j; }
        }
        int i = nq, j = best + 1, sj = j;
        while (i > 0 && j > 0) {
            sj = j;
            const unsigned code = (dirw[(i - 1) * WPR + ((j - 1) >> 4)] >> (2 * ((j - 1) & 15))) & 3u;
            if (code == 0) { --i; --j; }
            else if (code == 1) --i;
            else --j;
        }
        sh.flag = sj - 1;   // seg_cons_query_start
        sh.count = best;    // seg_cons_query_end
    }
    __syncthreads();
    const int qs = sh.flag, qe = sh.count;
    const int sbs = cpts[qe];   // int(np.sum(adapter_dwell_times[:seg_query_end]))
    __syncthreads();            // cpts is rewritten below
    M = RefineMatch{mean, sd, ev_med, ev_mad, dt_med, dt_mad, qs, qe, sbs, 0};
    return true;
}

// WIDE: the long form -- the barcode tail can exceed 16 384 positions, so fp_segment takes its 64-bit chunk masks
template <int BLOCK, bool WIDE = false, class Prep>
__device__ void fp_refine_finish(const FpArgs &A, const int64_t r, const RefineMatch &M, unsigned char *state, const int ns,
                                 const int n, int *cpts, double *zz, unsigned *hist, FpShared &sh, Prep prep,
                                 const bool exact_sums = false) {
    const int tid = threadIdx.x;
    const wdx_seg_params &P = A.p;
    const RefineDev &R = A.rf;
    const int K = P.barcode_num_events;
    auto finish = [&](int st, bool with_stats) {
        if (st != WDX_READ_OK) {
            for (int i = tid; i < K; i += BLOCK) {
                if (A.fpt) A.fpt[r * K + i] = __builtin_nan("");
                if (A.dwell) A.dwell[r * K + i] = 0;
            }
            if (!with_stats) {
                if (A.stats && tid < 6) A.stats[r * 6 + tid] = __builtin_nan("");
                if (R.idx && tid < 3) R.idx[r * 3 + tid] = -1;
            }
        }
        if (tid == 0) A.status[r] = st;
    };
    const double mean = M.mean, sd = M.sd, ev_med = M.ev_med, ev_mad = M.ev_mad, dt_med = M.dt_med, dt_mad = M.dt_mad;
    const int qs = M.qs, qe = M.qe, sbs = M.sbs;
    // ---- the barcode tail: discrepenacy_curve_to_cpts(adapter_scores[sbs:], E2, config d, config W, False) -----
    int ns2 = ns - sbs;
    if (ns2 < 0) ns2 = 0;
    if (P.min_obs_per_base < 1) {  // scipy: `distance` must be >= 1
        finish(WDX_READ_FAIL_UNKNOWN, false);
        return;
    }
    int nseg2 = 0, it2 = 0;
    const int n_end2 = ns2 + 2 * P.running_stat_width;
    const double *sc_t = nullptr;
    const float *sg_t = nullptr;
    if (!prep(sbs, ns2, sc_t, sg_t)) return;
    {
        // a last boundary beyond the slice (window width shrunk below the configured one): the Cython loop of
        // compute_base_means indexes out of bounds -> exception -> "unknown"; checked BEFORE the means are summed
        if (n_end2 != n - sbs) {
            // still "event segmentation failed" when the tail has too few peaks (that return comes first)
            const int st0 = fp_segment<BLOCK, WIDE>(sc_t, state, ns2, P.min_obs_per_base, P.running_stat_width, R.E2,
                                              false, sg_t, min(n_end2, n - sbs), cpts, zz, hist, sh, nseg2, it2, A.no_list != 0);
            finish(st0 == WDX_READ_FAIL_SEGMENT ? WDX_READ_FAIL_SEGMENT : WDX_READ_FAIL_UNKNOWN, false);
            return;
        }
        const int st = fp_segment<BLOCK, WIDE>(sc_t, state, ns2, P.min_obs_per_base, P.running_stat_width, R.E2, false,
                                         sg_t, n_end2, cpts, zz, hist, sh, nseg2, it2, A.no_list != 0, exact_sums);
        if (st != WDX_READ_OK) {
            finish(st, false);
            return;
        }
    }
    // normalize_wrt(barcode_event_means, adapter_event_means, segmentation.normalization) (sig_proc.py:139-168)
    double shift, scale;
    if (P.seg_norm == WDX_NORM_MEAN) { shift = mean; scale = sd; }
    else if (P.seg_norm == WDX_NORM_MEDIAN) { shift = ev_med; scale = ev_mad; }
    else { finish(WDX_READ_FAIL_UNKNOWN, false); return; }  // "none" is not a normalize_wrt method: ValueError
    // The final status is decided first and stats / indices are written ONCE: "consensus query outlier" and
    // success report them, the nseg2 < K "unknown" path (the np.pad call subtracts an int from a tuple ->
    // TypeError) reports NaN / -1 -- no second write to the same addresses by other lanes.
    const bool outlier = qs > R.ub_start || qe < R.lb_end || qe > R.ub_end;
    if (!outlier && nseg2 < K) {
        finish(WDX_READ_FAIL_UNKNOWN, false);
        return;
    }
    if (tid == 0) {
        if (A.stats) {
            double *o = A.stats + r * 6;
            o[0] = dt_med; o[1] = dt_mad; o[2] = mean; o[3] = sd; o[4] = ev_med; o[5] = ev_mad;
        }
        if (R.idx) {
            R.idx[r * 3] = qs; R.idx[r * 3 + 1] = qe; R.idx[r * 3 + 2] = sbs;
        }
    }
    if (outlier) {
        finish(WDX_READ_FAIL_CONSENSUS, true);  // "consensus query outlier": stats and indices are reported
        return;
    }
    for (int i = tid; i < K; i += BLOCK) {
        const int s = nseg2 - K + i;
        if (A.fpt) A.fpt[r * K + i] = (zz[s] - shift) / scale;
        if (A.dwell) A.dwell[r * K + i] = (int64_t)(cpts[s + 1] - cpts[s]);
    }
    finish(WDX_READ_OK, true);
}


template <int BLOCK, bool WIDE = false, class Prep>
__device__ void fp_refine_tail(const FpArgs &A, const int64_t r, unsigned char *state,
                               const int ns, const int W, const int n, int *cpts, double *ev,
                               double *zz, double *tmp, unsigned char *scratch, unsigned *hist, FpShared &sh,
                               const int nseg, Prep prep) {
    (void)W;
    RefineMatch M;
    if (!fp_refine_match<BLOCK>(A, r, cpts, ev, zz, tmp, scratch, sh, nseg, M)) return;
    fp_refine_finish<BLOCK, WIDE>(A, r, M, state, ns, n, cpts, zz, hist, sh, prep);
}

// ---- the kernel -----------------------------------------------------------------------------------

// PROF = diagnostic instantiation with s_memtime stamps between phases (never used by the product
// entry points; see wdx_fingerprint_profile_dev).
#define WDX_STAMP(k)                                                                        \
    do {                                                                                    \
        if (PROF) {                                                                         \
            __syncthreads();                                                                \
            if (tid == 0 && r < A.prof_reads)                                               \
                A.prof[r * 32 + (k)] = (long long)__builtin_amdgcn_s_memtime();             \
        }                                                                                   \
    } while (0)

// LONG_REFINE: the long form that also refines in place (fingerprint_long_refine_kernel; the plain long kernel is never
// sent a refining call and is compiled without that code: its registers are the plain branch's)
template <int BLOCK, bool PROF, bool BIG = false, bool LONG = false, bool LONG_REFINE = false>
__device__ void fp_process_read(const FpArgs &A, const int64_t r, unsigned char *smem) {
    static_assert(!LONG || (BIG && !PROF), "the long form is the big form with the samples in the slot as well");
    static_assert(!LONG_REFINE || LONG, "the refining long form is a long form");
    const int tid = threadIdx.x;
    const wdx_seg_params &P = A.p;
    const int K = P.barcode_num_events;
    const int E = P.num_events;

    // LDS carve-up (every region starts 8-byte aligned; cap is a multiple of 64).  BIG: the score curve lives in
    // this workgroup's HBM slot instead (same code, global loads/stores: the address space follows the
    // instantiation), everything else stays in LDS.  LONG: the slot (A.big_scores: kLongSlotBytes each) holds the score
    // curve and, behind it, the clipped samples; LDS keeps the fixed tables and the dedicated peak-state bytes.
    double *scores = LONG ? A.big_scores + (size_t)blockIdx.x * (kLongSlotBytes / 8)
                          : (BIG ? A.big_scores + (size_t)blockIdx.x * kBigCap : reinterpret_cast<double *>(smem));  // cap
    double *Mt = BIG ? reinterpret_cast<double *>(smem) : scores + A.cap;  // kTile + kMaxW
    double *Vt = Mt + (kTile + kMaxW);                                    // kTile + kMaxW
    double *ev = Vt + (kTile + kMaxW);                                    // kSegCap
    double *zz = ev + kSegCap;                                            // kSegCap
    double *tmp = zz + kSegCap;                                           // kSegCap
    FpShared &sh = *reinterpret_cast<FpShared *>(tmp + kSegCap);
    float *sig = LONG ? reinterpret_cast<float *>(scores + kLongCap) : reinterpret_cast<float *>(&sh + 1);   // cap
    unsigned *hist = LONG ? reinterpret_cast<unsigned *>(&sh + 1) : reinterpret_cast<unsigned *>(sig + A.cap);   // 256
    int *cpts = reinterpret_cast<int *>(hist + 256);                      // kSegCap + 1
    // the peak-state bytes are live only after the last t-score tile: they reuse the tile buffers
    // whenever they fit, else a dedicated tail region
    unsigned char *state = (A.cap <= (int)((kTile + kMaxW) * 16))
                               ? reinterpret_cast<unsigned char *>(Mt)
                               : reinterpret_cast<unsigned char *>(cpts + kSegCap + 1);

    int status = WDX_READ_OK;

    auto finish = [&](int st) {
        // failed reads: NaN fingerprint / stats, zero dwell (block-uniform call)
        if (st != WDX_READ_OK) {
            for (int i = tid; i < K; i += BLOCK) {
                if (A.fpt) A.fpt[r * K + i] = __builtin_nan("");
                if (A.dwell) A.dwell[r * K + i] = 0;
            }
            if (A.stats && tid < 6) A.stats[r * 6 + tid] = __builtin_nan("");
        }
        if (tid == 0) A.status[r] = st;
    };

    if (A.ok && !A.ok[r]) {
        finish(WDX_READ_FAIL_DETECT);
        return;
    }

    WDX_STAMP(0);
    // ---- A0 extract_adapter (sig_proc.py:382-391) --------------------------------------------------
    const int64_t row_off = A.row_off ? A.row_off[r] : r * A.stride;
    const int64_t row_len = A.row_len ? (int64_t)A.row_len[r]
                                      : (A.row_off ? A.row_off[r + 1] - A.row_off[r] : A.stride);
    int64_t start = (int64_t)A.a_start[r] - P.padding;
    if (start < 0) start = 0;
    int64_t stop = (int64_t)A.a_end[r] + P.padding;
    if (stop > row_len) stop = row_len;
    int64_t n64 = stop - start;
    if (n64 < 0) n64 = 0;
    if (n64 > A.cap) {
        if (!BIG && n64 <= A.defer_big) return;  // fingerprint_big_kernel (fingerprint_long_kernel) takes it
        finish(WDX_READ_FAIL_UNKNOWN);
        return;
    }
    const int n = (int)n64;

    // ---- P0: HBM -> LDS ----------------------------------------------------------------------------
    {
        const float *__restrict__ src = A.sig + row_off + start;
        for (int i = tid; i < n; i += BLOCK) sig[i] = src[i];
    }
    __syncthreads();

    WDX_STAMP(1);
    // ---- P1: MAD outlier clip (sig_proc.py:421-431), float32 ---------------------------------------
    int any_nan = 0;          // (this thread saw a NaN sample / the bounds are NaN: only the refinement hand-over asks)
    float clip_lo = 0.f, clip_hi = 0.f;
    {
        float lo, hi;
        // behind the launch chain the bounds exist already (clip_bounds_kernel: the same float32 numbers; CLIP_OK also
        // says that the window holds no NaN and lo <= hi) -- the two workgroup-wide selects are a quarter of this kernel
        const ClipRec *crp = LONG ? nullptr : A.clip;   // (no clip kernel takes a long window: its own two medians)
        int cflag = CLIP_NONE;
        if (crp) {
            const ClipRec cr = crp[r];   // (block-uniform)
            cflag = cr.flag;
            lo = cr.lo;
            hi = cr.hi;
        }
        if (cflag != CLIP_OK) {
            const float med = block_nanmedian_f32<BLOCK>([&](int i) { return sig[i]; }, n, hist, sh);
            const float mad =
                block_nanmedian_f32<BLOCK>([&](int i) { return fabsf(sig[i] - med); }, n, hist, sh);
            clip_bounds(P, med, mad, lo, hi);
        }
        const bool bad = (lo != lo) || (hi != hi);
        __syncthreads();
        for (int i = tid; i < n; i += BLOCK) {
            float v = sig[i];
            if (v == v) {
                if (bad) v = __builtin_nanf("");
                else {
                    if (!(v > lo)) v = lo;
                    if (!(v < hi)) v = hi;
                }
                sig[i] = v;
            } else {
                any_nan = 1;
            }
        }
        __syncthreads();
        clip_lo = lo;
        clip_hi = hi;
        if (bad) any_nan = 1;
    }

    WDX_STAMP(2);
    // ---- A2: optional signal normalisation (sig_proc.py:433-446); "none" in every shipped config ----
    if (n > 0 && P.sig_norm == WDX_NORM_MEDIAN) {
        const float shift = block_nanmedian_f32<BLOCK>([&](int i) { return sig[i]; }, n, hist, sh);
        const float scale =
            block_nanmedian_f32<BLOCK>([&](int i) { return fabsf(sig[i] - shift); }, n, hist, sh);
        __syncthreads();
        for (int i = tid; i < n; i += BLOCK) sig[i] = (sig[i] - shift) / scale;
        __syncthreads();
    } else if (n > 0 && P.sig_norm == WDX_NORM_MEAN) {
        // mean_normalize on the float32 signal (sig_proc.py:99-111, accept_nan=True): np.mean / np.std, or
        // np.nanmean / np.nanstd when the window holds a NaN -- float32 sums in NumPy's association
        // (oracle: mean_normalize_f32).  LDS scratch: the score curve and the event arrays are still unused.
        // LONG: up to 7 x 64 + 130 leaves (seven full 8192-element chunks and a partial one) -- more than hist and ev
        // hold: the leaf tables take the tile buffers instead (2 x 4 KB of their 9 KB, the stack behind them)
        float *sq = reinterpret_cast<float *>(scores);   // n floats
        unsigned *lstart = LONG ? reinterpret_cast<unsigned *>(Mt) : hist;                         // leaf starts
        float *lsum = LONG ? reinterpret_cast<float *>(Mt) + 1024 : reinterpret_cast<float *>(ev); // leaf sums
        int *stk = LONG ? reinterpret_cast<int *>(Mt) + 2048 : reinterpret_cast<int *>(zz);        // traversal stack
        unsigned vcnt = 0;
        for (int i = tid; i < n; i += BLOCK) vcnt += (sig[i] == sig[i]);
        unsigned gmin_, gmax_, cnt;
        block_minmax_count<BLOCK>(0u, 0u, vcnt, sh, gmin_, gmax_, cnt);
        const bool has_nan = cnt != (unsigned)n;
        float shift, scale;
        if (!has_nan) {
            shift = block_np_add_reduce_f32<BLOCK>([&](int i) { return sig[i]; }, n, lstart, lsum, stk, sh) / (float)n;
            for (int i = tid; i < n; i += BLOCK) {
                const float d = sig[i] - shift;
                sq[i] = d * d;
            }
            scale = sqrtf(block_np_add_reduce_f32<BLOCK>([&](int i) { return sq[i]; }, n, lstart, lsum, stk, sh) / (float)n);
        } else {
            // _replace_nan(a, 0); sums in float32; _divide_by_count forms the quotient in float64 (float32 / intp)
            const float tot = block_np_add_reduce_f32<BLOCK>(
                [&](int i) { const float v = sig[i]; return v == v ? v : 0.0f; }, n, lstart, lsum, stk, sh);
            shift = (float)((double)tot / (double)cnt);
            for (int i = tid; i < n; i += BLOCK) {
                const float v = sig[i];
                const float d = (v == v) ? v - shift : 0.0f;
                sq[i] = d * d;
            }
            const float var = (float)((double)block_np_add_reduce_f32<BLOCK>([&](int i) { return sq[i]; }, n, lstart,
                                                                             lsum, stk, sh) / (double)cnt);
            scale = sqrtf(var);
        }
        __syncthreads();
        for (int i = tid; i < n; i += BLOCK) sig[i] = (sig[i] - shift) / scale;
        __syncthreads();
    } else if (n > 0 && P.sig_norm != WDX_NORM_NONE) {
        finish(WDX_READ_FAIL_SIGNORM);  // unknown codes fail here
        return;
    }

    // ---- parameter shrink (sig_proc.py:526-533), Python round() == rint() ---------------------------
    int d_eff = (int)rint((double)n / (double)E / 2.0);
    if (P.min_obs_per_base < d_eff) d_eff = P.min_obs_per_base;
    int W = (int)rint((double)n / (double)E);
    if (P.running_stat_width < W) W = P.running_stat_width;

    // ---- P2: windowed t-statistic (_c_segmentation.pyx:124-161) -------------------------------------
    int ns = n - 2 * W;
    if (ns < 0 || (ns > 0 && W == 0)) ns = 0;  // the Cython call raises -> zeros(0)
    if (d_eff < 1) {                            // scipy: `distance` must be >= 1 -> "unknown"
        finish(WDX_READ_FAIL_UNKNOWN);
        return;
    }
    {
        const double Wd = (double)W;
        const int nq = n - W + 1;  // window starts
        for (int t0 = 0; t0 < ns; t0 += kTile) {
            const int qend = min(t0 + kTile + W, nq);
            for (int q = t0 + tid; q < qend; q += BLOCK) {
                double m = 0.0;
                for (int k = 0; k < W; ++k) m += (double)sig[q + k];
                m /= Wd;
                double v = 0.0;
                for (int k = 0; k < W; ++k) {
                    const double df = (double)sig[q + k] - m;
                    v += df * df;
                }
                Mt[q - t0] = m;
                Vt[q - t0] = v;
            }
            __syncthreads();
            const int pend = min(t0 + kTile, ns);
            for (int pos = t0 + tid; pos < pend; pos += BLOCK) {
                const double m1 = Mt[pos - t0], m2 = Mt[pos - t0 + W];
                const double vs = Vt[pos - t0] + Vt[pos - t0 + W];
                double s;
                if (vs == 0) s = 0.0;
                else if (m1 > m2) s = (m1 - m2) / sqrt(vs);
                else s = (m2 - m1) / sqrt(vs);
                scores[pos] = s;
            }
            __syncthreads();
        }
    }

    WDX_STAMP(3);
    // ---- P3-P6: find_peaks + top-E + boundaries + event means (fp_segment) ----------------------------
    int nms_iters = 0, nseg = 0;
    {
        const int st = fp_segment<BLOCK, LONG>(scores, state, ns, d_eff, W, E, P.accept_less_cpts != 0, sig, n, cpts, ev,
                                         hist, sh, nseg, nms_iters, A.no_list != 0);
        if (st != WDX_READ_OK) {
            finish(st);
            return;
        }
    }
    WDX_STAMP(7);
    if constexpr (!LONG || LONG_REFINE)
    if (A.rf.query) {
        // The refinement kernels behind the fast kernels (one wave per three reads for the match, a quarter of this
        // workgroup for the barcode's segmentation) take this read too when they can reproduce its clipped samples from
        // the recorded bounds: no NaN in the window, samples as loaded, the configured window width.
        // (LONG never hands over: no clip record exists for its windows and the tail kernels hold kTailCap samples.  It
        // refines in place like the BIG form, the tail's score curve and samples at `sbs` inside the slot.  The match's
        // scratch and ev / zz / tmp / hist / cpts depend on num_events and the query alone; the tail's state bytes and the
        // peak list's uint16 positions, relative to sbs, are bounded by ns2 <= ns < kLongCap like the adapter pass's.)
        // (WDX_OPT_REFINE_OPTIMAL_CPTS: its kernel re-creates the adapted width and the exact clip itself -- every read)
        if (!LONG && A.refine_record && A.rf.ws && P.sig_norm == WDX_NORM_NONE && nseg <= 128 &&
            (A.refine_optimal || (W == P.running_stat_width && !__syncthreads_or(any_nan)))) {
            RefineRec *rec = reinterpret_cast<RefineRec *>(A.rf.ws) + r;
            for (int s = tid; s < nseg; s += BLOCK) rec->ev[s] = ev[s];
            for (int s = tid; s <= nseg; s += BLOCK) rec->cpts[s] = cpts[s];
            if (tid == 0) {
                rec->n = n;
                rec->lo = clip_lo;
                rec->hi = clip_hi;
                rec->state = 1;
            }
            return;
        }
        fp_refine_tail<BLOCK, LONG>(A, r, state, ns, W, n, cpts, ev, zz, tmp, reinterpret_cast<unsigned char *>(Mt), hist, sh, nseg,
                              [&](int sbs, int, const double *&sc_t, const float *&sg_t) {
                                  sc_t = scores + sbs;   // the adapter pass's score curve and clipped samples are still here
                                  sg_t = sig + sbs;
                                  return true;
                              });
        return;
    }

    WDX_STAMP(8);
    // ---- P7: normalise, stats, tail (sig_proc.py:546-605) --------------------------------------------
    {
        int has_nan = 0;
        for (int s = tid; s < nseg; s += BLOCK) has_nan |= (ev[s] != ev[s]);
        if (__syncthreads_or(has_nan)) {
            finish(WDX_READ_FAIL_SEGNORM);  // normalize(..., accept_nan=False) raises
            return;
        }
        // np.mean / np.std of the event means (also adapter_event_mean / adapter_event_std)
        if (tid == 0) sh.mean = np_pairwise_sum_dev(ev, nseg) / (double)nseg;
        __syncthreads();
        const double mean = sh.mean;
        for (int s = tid; s < nseg; s += BLOCK) {
            const double df = ev[s] - mean;
            tmp[s] = df * df;
        }
        __syncthreads();
        if (tid == 0) sh.sd = sqrt(np_pairwise_sum_dev(tmp, nseg) / (double)nseg);
        __syncthreads();
        const double sd = sh.sd;

        if (P.seg_norm == WDX_NORM_MEAN) {
            for (int s = tid; s < nseg; s += BLOCK) zz[s] = (ev[s] - mean) / sd;
        } else if (P.seg_norm == WDX_NORM_MEDIAN) {
            block_small_median<BLOCK>(ev, nseg, sh, 4);
            const double m = sh.stat[4];
            for (int s = tid; s < nseg; s += BLOCK) tmp[s] = fabs(ev[s] - m);
            block_small_median<BLOCK>(tmp, nseg, sh, 5);
            const double sc = sh.stat[5];
            for (int s = tid; s < nseg; s += BLOCK) zz[s] = (ev[s] - m) / sc;
        } else if (P.seg_norm == WDX_NORM_NONE) {
            for (int s = tid; s < nseg; s += BLOCK) zz[s] = ev[s];
        } else {
            finish(WDX_READ_FAIL_SEGNORM);
            return;
        }
        __syncthreads();

        // stats (sig_proc.py:562-567) -- only when the caller takes them (four medians by rank counting)
        if (A.stats) {
            for (int s = tid; s < nseg; s += BLOCK) tmp[s] = (double)(cpts[s + 1] - cpts[s]);
            block_small_median<BLOCK>(tmp, nseg, sh, 0);
            const double dt_med = sh.stat[0];
            for (int s = tid; s < nseg; s += BLOCK) tmp[s] = fabs(tmp[s] - dt_med);
            block_small_median<BLOCK>(tmp, nseg, sh, 1);
            block_small_median<BLOCK>(ev, nseg, sh, 4);
            const double ev_med = sh.stat[4];
            for (int s = tid; s < nseg; s += BLOCK) tmp[s] = fabs(ev[s] - ev_med);
            block_small_median<BLOCK>(tmp, nseg, sh, 5);
        }

        if (nseg < K) {
            finish(WDX_READ_FAIL_UNKNOWN);  // np.pad(int64 dwell, NaN) raises in the reference
            return;
        }
        for (int i = tid; i < K; i += BLOCK) {
            const int s = nseg - K + i;
            if (A.fpt) A.fpt[r * K + i] = zz[s];
            if (A.dwell) A.dwell[r * K + i] = (int64_t)(cpts[s + 1] - cpts[s]);
        }
        if (A.stats && tid == 0) {
            double *o = A.stats + r * 6;
            o[0] = sh.stat[0];
            o[1] = sh.stat[1];
            o[2] = mean;
            o[3] = sd;
            o[4] = sh.stat[4];
            o[5] = sh.stat[5];
        }
    }
    WDX_STAMP(9);
    if (PROF && tid == 0 && r < A.prof_reads) {
        A.prof[r * 32 + 10] = nms_iters;
        A.prof[r * 32 + 11] = n;
        A.prof[r * 32 + 12] = ns;
    }
    finish(status);
}

// one workgroup per read
template <int BLOCK, bool PROF>
__global__ __launch_bounds__(BLOCK) void fingerprint_kernel(FpArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    fp_process_read<BLOCK, PROF>(A, A.block_base + blockIdx.x, smem);
}

// exact slow path: the reads the fast kernel declined (list built with atomics), grid-stride
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void fingerprint_list_kernel(FpArgs A, const unsigned *count,
                                                                 const int32_t *list) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const unsigned n = *count;
    for (unsigned k = blockIdx.x; k < n; k += gridDim.x) {
        __syncthreads();
        fp_process_read<BLOCK, false>(A, (int64_t)list[k], smem);
    }
}

// windows beyond the LDS capacity of the exact kernel (kExactLdsCap < n <= kBigCap): a fixed grid of <= kBigSlots
// workgroups strides over the slow list (or over all reads when there is none) and takes only those
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void fingerprint_big_kernel(FpArgs A, const unsigned *count, const int32_t *list,
                                                                int small_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int64_t n = count ? (int64_t)*count : A.n_reads;
    for (int64_t k = blockIdx.x; k < n; k += gridDim.x) {
        const int64_t r = list ? (int64_t)list[k] : k;
        if (A.ok && !A.ok[r]) continue;  // the regular kernel reported it
        const int64_t row_len = A.row_len ? (int64_t)A.row_len[r]
                                          : (A.row_off ? A.row_off[r + 1] - A.row_off[r] : A.stride);
        int64_t start = (int64_t)A.a_start[r] - A.p.padding;
        if (start < 0) start = 0;
        int64_t stop = (int64_t)A.a_end[r] + A.p.padding;
        if (stop > row_len) stop = row_len;
        if (stop - start <= small_cap || stop - start > kBigCap) continue;
        __syncthreads();
        fp_process_read<BLOCK, false, true>(A, r, smem);
    }
}

// WDX_OPT_LONG_WINDOWS: windows of kBigCap+1 .. kLongCap samples, left alone by every launch before this one: a fixed grid
// of <= kLongSlots workgroups strides over the slow list (or over all reads) and takes only those
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void fingerprint_long_kernel(FpArgs A, const unsigned *count, const int32_t *list) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int64_t n = count ? (int64_t)*count : A.n_reads;
    for (int64_t k = blockIdx.x; k < n; k += gridDim.x) {
        const int64_t r = list ? (int64_t)list[k] : k;
        if (A.ok && !A.ok[r]) continue;  // the regular kernel reported it
        const int64_t row_len = A.row_len ? (int64_t)A.row_len[r]
                                          : (A.row_off ? A.row_off[r + 1] - A.row_off[r] : A.stride);
        int64_t start = (int64_t)A.a_start[r] - A.p.padding;
        if (start < 0) start = 0;
        int64_t stop = (int64_t)A.a_end[r] + A.p.padding;
        if (stop > row_len) stop = row_len;
        if (stop - start <= kBigCap || stop - start > kLongCap) continue;
        __syncthreads();
        fp_process_read<BLOCK, false, true, true>(A, r, smem);
    }
}

// WDX_OPT_LONG_REFINE_WINDOWS: the same windows on the consensus-refinement branch -- the long form with fp_refine_tail in
// place, the barcode tail's score curve and samples at sig_barcode_start inside the slot.  A kernel of its own, of
// kLongRefineBlock = 512 threads, in a translation unit of its own (wdx_fingerprint_long.hip: built with every call
// inlined): adapter pass and refinement in one function need 169 VGPRs, and as calls they take FpArgs and the lambdas by
// address, which puts them into scratch memory -- at 1024 threads (128 VGPRs) it spills; the plain long kernel above keeps
// its registers and its code.
[[maybe_unused]] constexpr int kLongRefineBlock = 512;
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void fingerprint_long_refine_kernel(FpArgs A, const unsigned *count, const int32_t *list) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int64_t n = count ? (int64_t)*count : A.n_reads;
    for (int64_t k = blockIdx.x; k < n; k += gridDim.x) {
        const int64_t r = list ? (int64_t)list[k] : k;
        if (A.ok && !A.ok[r]) continue;  // the regular kernel reported it
        const int64_t row_len = A.row_len ? (int64_t)A.row_len[r]
                                          : (A.row_off ? A.row_off[r + 1] - A.row_off[r] : A.stride);
        int64_t start = (int64_t)A.a_start[r] - A.p.padding;
        if (start < 0) start = 0;
        int64_t stop = (int64_t)A.a_end[r] + A.p.padding;
        if (stop > row_len) stop = row_len;
        if (stop - start <= kBigCap || stop - start > kLongCap) continue;
        __syncthreads();
        fp_process_read<BLOCK, false, true, true, true>(A, r, smem);
    }
}

// The refinement branch behind the FAST kernels (round 3; the match as a kernel of wave-sized workgroups and the exact
// kernel's hand-over since round 4): a fast kernel -- or the exact kernel, for a read of the slow list it can hand over --
// segments the adapter and leaves a RefineRec; two kernels do everything after it, bit for bit what fp_refine_match /
// fp_refine_finish (the exact kernel's own code) do:
//   fingerprint_refine_match_wave_kernel  (wdx_refine_match.hip) adapter statistics, subsequence DP, back-trace: one
//                                    wave per three reads;
//   fingerprint_refine_tail_kernel   the barcode's own segmentation: loads ONLY the samples from sig_barcode_start on,
//                                    re-clips them with the recorded bounds (the same v_med3_f32 on the same values),
//                                    computes their t-scores with the exact kernel's operations (every window's
//                                    statistics once, tiles of 256 window starts) and segments them (fp_segment).
// A barcode tail beyond kTailCap samples goes back to the exact kernel, which then refines the read in place.
// LDS of fingerprint_refine_tail_kernel<256>: FpShared | cpts | U | scores | samples, where U holds the event means, the
// select's histogram and the peak-state bytes of the segmentation and, before it, the window statistics of one t-score tile
constexpr int kTailBlock = 256;
constexpr size_t kTailU = ((size_t)kSegCap * 8 + 256 * 4 + kTailCap) > (size_t)kTailBlock * 16
                              ? ((size_t)kSegCap * 8 + 256 * 4 + kTailCap) : (size_t)kTailBlock * 16;
static_assert(kTailU % 16 == 0 && (kSegCap * 8) % 16 == 0, "alignment of the regions inside U");
static size_t refine_tail_lds_bytes() {
    size_t b = sizeof(FpShared) + (size_t)(kSegCap + 1) * 4;
    b = (b + 15) & ~(size_t)15;
    b += kTailU + (size_t)kTailCap * 8 + (size_t)(kTailCap + 64) * 4;
    return (b + 15) & ~(size_t)15;
}
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void fingerprint_refine_tail_kernel(FpArgs A, unsigned *slow_count, int32_t *slow_list) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int64_t r = A.block_base + blockIdx.x;
    if (r >= A.n_reads) return;
    RefineRec *rec = reinterpret_cast<RefineRec *>(A.rf.ws) + r;
    if (rec->state != 3) return;
    const wdx_seg_params &P = A.p;
    static_assert(BLOCK == kTailBlock, "refine_tail_lds_bytes");
    FpShared &sh = *reinterpret_cast<FpShared *>(smem);
    int *cpts = reinterpret_cast<int *>(&sh + 1);
    unsigned char *U = reinterpret_cast<unsigned char *>((reinterpret_cast<uintptr_t>(cpts + kSegCap + 1) + 15) & ~(uintptr_t)15);
    double *zz = reinterpret_cast<double *>(U);                                  // kSegCap
    unsigned *hist = reinterpret_cast<unsigned *>(zz + kSegCap);                 // 256
    unsigned char *state = reinterpret_cast<unsigned char *>(hist + 256);        // kTailCap
    double *Mt = reinterpret_cast<double *>(U), *Vt = Mt + BLOCK;                // one tile's window statistics (before these)
    double *t_scores = reinterpret_cast<double *>(U + kTailU);                   // kTailCap
    float *t_sig = reinterpret_cast<float *>(t_scores + kTailCap);               // kTailCap + 64
    RefineMatch M;
    memcpy(&M, rec->m, sizeof(M));
    const int n = rec->n, W = P.running_stat_width;
    const float lo = rec->lo, hi = rec->hi;
    const int64_t row_off = A.row_off ? A.row_off[r] : r * A.stride;
    int64_t start = (int64_t)A.a_start[r] - P.padding;
    if (start < 0) start = 0;
    const float *__restrict__ src = A.sig + row_off + start;
    const int ns = n - 2 * W;
    fp_refine_finish<BLOCK>(A, r, M, state, ns, n, cpts, zz, hist, sh,
                            [&](int sbs, int ns2, const double *&sc_t, const float *&sg_t) -> bool {
        const int nt = n - sbs;  // samples of the barcode tail
        if (nt > kTailCap || nt < 0) {  // block-uniform: hand the whole read to the exact kernel
            if (tid == 0) {
                rec->state = 2;
                slow_list[atomicAdd(slow_count, 1u)] = (int32_t)r;
            }
            return false;
        }
        for (int i = tid; i < nt; i += BLOCK) t_sig[i] = __builtin_amdgcn_fmed3f(src[sbs + i], lo, hi);
        __syncthreads();
        // windowed t-statistic of the tail (_c_segmentation.pyx:124-161; fp_process_read's operations): tiles of BLOCK
        // window starts -- every window's mean and squared deviations once, one thread each -- then the scores of the
        // BLOCK - W positions whose two windows the tile holds
        const int nwin = ns2 > 0 ? ns2 + W : 0;   // window starts 0 .. ns2 + W - 1 (the last one ends at sample nt - 1)
        const int TP = BLOCK - W;                 // W <= kMaxW = 64 < BLOCK
        for (int t0 = 0; t0 < ns2; t0 += TP) {
            const int q = t0 + tid;
            if (q < nwin) {
                double m, v;
                if (W == 18) window_stats<18>(t_sig + q, W, m, v);
                else if (W == 12) window_stats<12>(t_sig + q, W, m, v);
                else window_stats<0>(t_sig + q, W, m, v);
                Mt[tid] = m;
                Vt[tid] = v;
            }
            __syncthreads();
            const int pos = t0 + tid;
            if (tid < TP && pos < ns2) {
                const double m1 = Mt[tid], m2 = Mt[tid + W];
                const double vs = Vt[tid] + Vt[tid + W];
                double sc;
                if (vs == 0) sc = 0.0;
                else if (m1 > m2) sc = (m1 - m2) / sqrt(vs);
                else sc = (m2 - m1) / sqrt(vs);
                t_scores[pos] = sc;
            }
            __syncthreads();
        }
        sc_t = t_scores;
        sg_t = t_sig;
        return true;
    }, lo > 0.f && hi <= lo * 65536.f);   // (clipped samples in [lo, hi], at most kTailCap of them: their float64 sums are exact)
}

#ifndef WDX_DEV_KERNELS_ONLY  // (development: a TU that instantiates single kernels includes this file with the macro set)
// fn(base, n) over n_items in slices of at most launch_slice_limit(builtin), full slices and a remainder (fp_slices' kFullSlices:
// wdx_fp_plan.h); stops at fn's first error
template <class Fn>
static int for_each_slice(int64_t n_items, int64_t builtin, Fn fn) {
    const int64_t slice = launch_slice_limit(builtin);
    for (int64_t base = 0; base < n_items; base += slice)
        if (int rc = fn(base, std::min(slice, n_items - base))) return rc;
    return WDX_SUCCESS;
}

static int launch_refine_tail(FpArgs A, unsigned *slow_count, int32_t *slow_list, hipStream_t stream) {
    static LdsAttr attr_t;
    const size_t lds_t = refine_tail_lds_bytes();
    if (int rc = attr_t.ensure(fingerprint_refine_tail_kernel<256>, lds_t)) return rc;
    if (int rc = for_each_slice(A.n_reads, 1 << 22, [&](int64_t base, int64_t n) {
            A.block_base = base;
            if (int rc = launch_refine_match_wave(A, n, stream)) return rc;
            if (refine_tail_wave_takes(A)) return launch_refine_tail_wave(A, n, slow_count, slow_list, stream);
            hipLaunchKernelGGL((fingerprint_refine_tail_kernel<256>), dim3((unsigned)n), dim3(256), lds_t, stream, A, slow_count,
                               slow_list);
            return (int)WDX_SUCCESS;
        }))
        return rc;
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}
int64_t fingerprint_refine_ws_bytes(int64_t n_reads) { return (int64_t)sizeof(RefineRec) * (n_reads > 0 ? n_reads : 0); }

#endif  // WDX_DEV_KERNELS_ONLY
#include "wdx_fingerprint_fast.inc"
#include "wdx_fingerprint_split.inc"
#ifndef WDX_DEV_KERNELS_ONLY

int64_t fingerprint_big_bytes(int64_t max_len) {
    return max_len > kExactLdsCap ? (int64_t)kBigSlots * kBigCap * 8 : 0;
}
int64_t fingerprint_long_bytes(int64_t max_len) { return max_len > kBigCap ? (int64_t)(kLongSlots * kLongSlotBytes) : 0; }

// One step of the exact families (fingerprint_kernel, _list_kernel, _big_kernel, _long_kernel): the plan's grid, workgroup, LDS
// bytes and slices; `extra` is what the kernel takes behind its FpArgs.
template <auto K, class... Extra>
static int launch_exact(const FpStep &s, FpArgs A, int64_t max_launch_slice, hipStream_t stream, int64_t *n_launches, Extra... extra) {
    if (int rc = lds_attr_of<K>().ensure(K, s.lds)) return rc;
    const FpSlices S = fp_slices(s.extent, s.rule, s.slice_limit, max_launch_slice);
    for (int64_t i = 0; i < S.count; ++i) {
        A.block_base = S.base(i);
        hipLaunchKernelGGL(K, dim3((unsigned)S.n(i)), dim3(s.wg), s.lds, stream, A, extra...);
        if (s.counted && n_launches) ++*n_launches;
    }
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}
// the big and long forms of the exact kernel: a fixed grid of slots strides over the list (or over all reads)
static int launch_big_long_step(const FpStep &s, FpArgs A, const unsigned *count, const int32_t *list, void *d_long, hipStream_t stream) {
    switch (s.key.family) {
        case kFamLong:
            A.cap = kLongCap;
            A.defer_big = 0;
            A.big_scores = reinterpret_cast<double *>(d_long);
            A.clip = nullptr;
            A.refine_record = 0;
            if (A.rf.query) return launch_fp_long_refine(A, count, list, s.extent, s.lds, stream);   // (wdx_fingerprint_long.hip)
            return launch_exact<fingerprint_long_kernel<1024>>(s, A, 0, stream, nullptr, count, list);
        case kFamBig: {
            const int small_cap = A.cap;   // (the windows the launches before this one took)
            A.cap = kBigCap;
            A.defer_big = 0;
            return launch_exact<fingerprint_big_kernel<1024>>(s, A, 0, stream, nullptr, count, list, small_cap);
        }
        default:
            set_error("launch_big_long_step: not the big or the long form");
            return WDX_ERR_INVALID;
    }
}

int fill_refine_dev(const wdx_refine_params &rp, const double *d_query, int32_t *d_idx, RefineDev **out) {
    if (rp.subseq_norm != WDX_NORM_NONE && rp.subseq_norm != WDX_NORM_MEAN && rp.subseq_norm != WDX_NORM_MEDIAN) {
        set_error("Normalization method %d not recognized.", (int)rp.subseq_norm);
        return WDX_ERR_INVALID;
    }
    if (rp.penalty != rp.penalty || rp.penalty < 0) {
        set_error("consensus refinement: penalty must be >= 0");
        return WDX_ERR_INVALID;
    }
    RefineDev *r = new RefineDev{d_query, rp.n_query, rp.subseq_norm, rp.penalty, rp.psi[0], rp.psi[2],
                                 rp.ub_start, rp.lb_end, rp.ub_end, rp.barcode_segm_events, d_idx, nullptr};
    *out = r;
    return WDX_SUCCESS;
}
void free_refine_dev(RefineDev *rf) { delete rf; }
int refine_segm_events(const RefineDev *rf) { return rf->E2; }
void set_refine_ws(RefineDev *rf, void *d_ws) { rf->ws = reinterpret_cast<unsigned char *>(d_ws); }

// Self-test of the t-score's unscaled sqrt / quotient sequences (fast_sqrt_mid, fast_div_mid) against the
// compiler's general float64 sqrt() and '/': same bits on the documented value range is what the fast path's
// bit-identity rests on; a toolchain whose expansions change shows up here (tests/test_gpu_parity.py).
__global__ void score_selftest_kernel(const double *__restrict__ dm, const double *__restrict__ vs, int64_t n,
                                      double *__restrict__ fast, double *__restrict__ ref) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fast[i] = fast_div_mid(dm[i], fast_sqrt_mid(vs[i]));
    ref[i] = dm[i] / sqrt(vs[i]);
}
int launch_score_selftest(const double *dm, const double *vs, int64_t n, double *fast, double *ref, hipStream_t stream) {
    if (n <= 0) return WDX_SUCCESS;
    hipLaunchKernelGGL(score_selftest_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, dm, vs, n, fast, ref);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

#include "wdx_fingerprint_launch.inc"
#endif  // WDX_DEV_KERNELS_ONLY

}  // namespace wdx
