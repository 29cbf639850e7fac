// Adapter boundary detection for gfx950 (include/wdx.h: wdx_detect_rows states the rule, bit for bit; wdx_detect_plan.h the
// domain of the parameters and the integer thresholds).
//
//   detect_kernel<ADC>   one wave per read, one-wave workgroups.  The row is loaded once, coalesced (eight loads in flight per
//                        lane; the int16 form calibrates as it loads, two samples per lane and load where the row starts on
//                        a 4-byte boundary), quantised to int16 and kept in LDS: 2 bytes per sample of max_obs_trace,
//                        nothing else.
//                        Every partial sum of q fits int32 (16 384 samples of at most 2^15), so the prefix sums the rule
//                        names are running int32 sums; only the sums of squares and the products of step 4 are int64.
//                        A step that walks candidates hands every lane a run of `seg` consecutive candidates, seg / 2 odd: the
//                        lanes' LDS addresses then fall on 64 different banks at every step of the walk.  The prefix at the head
//                        of a lane's run is the wave scan of the runs' sums.
//                          step 2   64 candidates a round, a lane sums its window only behind q[i] < thr1; first hit by ballot
//                          step 3   two float64 divisions per candidate, argmax over (g, smallest i) by lane exchange
//                          step 4   a lane sums its first window, then slides: four LDS reads per candidate
//                        No atomics, no scratch memory, no global memory but the row and the six outputs.
#include "wdx_ctx.h"
#include "wdx_detect_plan.h"
#include "wdx_wave.h"

#include <limits.h>

namespace wdx {

namespace {

struct DetectArgs {
    const float *sig;        // float32 rows, or
    const int16_t *adc;      // an int16 shard with
    const float *offset, *scale;
    const int64_t *row_off;  // packed: [n_reads + 1]; null: r * stride
    const int32_t *row_len;  // nullable for float32 rows
    int64_t stride;
    int32_t *a_start, *a_end;
    uint8_t *ok;
    int32_t *code, *info;
    double *gain;
    DetectQ q;
};

__device__ __forceinline__ int wave_sum_i32(int v) { return (int)wave_sum_u32((unsigned)v); }
__device__ __forceinline__ int wave_excl_scan_i32(int v) { return (int)wave_incl_scan_u32((unsigned)v) - v; }

// sum of q[a .. b), the wave together
__device__ __forceinline__ int range_sum(const int16_t *qs, int a, int b, int lane) {
    int acc = 0;
    for (int i = a + lane; i < b; i += 64) acc += qs[i];
    return wave_sum_i32(acc);
}

// candidates per lane when `count` of them are spread over the wave: the smallest t >= ceil(count / 64) with t / 2 odd
__device__ __forceinline__ int run_length(int count) {
    const int t = (count + 63) >> 6;
    return t + ((2 - t) & 3);
}

__device__ __forceinline__ void detect_write(const DetectArgs &A, int64_t r, int lane, int code, int s, int e, int n, int c, int i2,
                                             int i3, double gain) {
    if (lane != 0) return;
    if (A.a_start) A.a_start[r] = s;
    if (A.a_end) A.a_end[r] = e;
    if (A.ok) A.ok[r] = code == WDX_DETECT_OK ? 1 : 0;
    A.code[r] = code;
    if (A.info) {
        int32_t *o = A.info + 4 * r;
        o[0] = n, o[1] = c, o[2] = i2, o[3] = i3;
    }
    if (A.gain) A.gain[r] = gain;
}

template <bool ADC>
__global__ __launch_bounds__(64) void detect_kernel(const DetectArgs A) {
    extern __shared__ int16_t qs[];   // q[0 .. n)
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    const DetectQ &Q = A.q;
    const double nan_out = __longlong_as_double(0x7FF8000000000000ll);

    // ---- the row: where it lies, how much of it counts ----
    int64_t base, len;
    if (A.row_off) {
        base = A.row_off[r];
        len = A.row_off[r + 1] - base;
    } else {
        base = r * A.stride;
        len = A.stride;
    }
    if (A.row_len) {
        const int64_t l = A.row_len[r];
        len = l < len ? l : len;
    }
    len = len < 0 ? 0 : len;
    const int cap = (int)(len < (int64_t)Q.max_trace ? len : (int64_t)Q.max_trace);

    // ---- load, quantise, find n ----
    constexpr int U = 8;
    const float nanv = __builtin_nanf("");
    float off = 0.f, sc = 0.f;
    if constexpr (ADC) off = A.offset[r], sc = A.scale[r];
    int n = cap, acc = 0;
    bool ended = false;
    // an int16 row that starts on a 4-byte boundary: two samples per lane and load (samples 2 l, 2 l + 1 of every 128), half the
    // load instructions of the one-sample form below; nothing at or behind sample `cap` is read
    bool pairs = false;
    if constexpr (ADC) pairs = (((uintptr_t)(A.adc + base)) & 3) == 0;
    if (pairs) {
        const int16_t *__restrict__ ap = A.adc + base;
        for (int b0 = 0; b0 < cap && !ended; b0 += 128 * U) {
            float v0[U], v1[U];
#pragma unroll
            for (int k = 0; k < U; ++k) {
                const int i = b0 + 128 * k + 2 * lane;
                int x0 = 0, x1 = 0;
                if (i + 1 < cap) {
                    const int w = *reinterpret_cast<const int *>(ap + i);
                    x0 = (int)(short)(w & 0xffff), x1 = w >> 16;
                } else if (i < cap) {
                    x0 = ap[i];
                }
                v0[k] = i < cap ? __fmul_rn(sc, __fadd_rn((float)x0, off)) : nanv;
                v1[k] = i + 1 < cap ? __fmul_rn(sc, __fadd_rn((float)x1, off)) : nanv;
            }
#pragma unroll
            for (int k = 0; k < U; ++k) {
                if (ended) continue;   // (wave-uniform)
                const unsigned long long m0 = __ballot(v0[k] != v0[k]), m1 = __ballot(v1[k] != v1[k]);
                const int f0 = m0 ? 2 * __builtin_ctzll(m0) : 128, f1 = m1 ? 2 * __builtin_ctzll(m1) + 1 : 128;
                const int first = f0 < f1 ? f0 : f1;   // among the 128 samples of this step
                const int i = b0 + 128 * k + 2 * lane;
                if (2 * lane < first) {
                    const float w = __fmul_rn(v0[k], Q.qpp);
                    const int q = w >= 32767.f ? 32767 : (w <= -32768.f ? -32768 : (int)rintf(w));
                    qs[i] = (int16_t)q;
                    acc += q;
                }
                if (2 * lane + 1 < first) {
                    const float w = __fmul_rn(v1[k], Q.qpp);
                    const int q = w >= 32767.f ? 32767 : (w <= -32768.f ? -32768 : (int)rintf(w));
                    qs[i + 1] = (int16_t)q;
                    acc += q;
                }
                if (first < 128) n = b0 + 128 * k + first, ended = true;
            }
        }
        ended = true;   // (the one-sample loop below is skipped)
    }
    for (int b0 = 0; b0 < cap && !ended; b0 += 64 * U) {
        float v[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int i = b0 + 64 * k + lane;
            if constexpr (ADC)
                v[k] = i < cap ? __fmul_rn(sc, __fadd_rn((float)A.adc[base + i], off)) : nanv;
            else
                v[k] = i < cap ? A.sig[base + i] : nanv;
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            if (ended) continue;   // (wave-uniform)
            // a sample behind the cap counts as NaN: the row ends there at the latest
            const unsigned long long m = __ballot(v[k] != v[k]);
            const int first = m ? __builtin_ctzll(m) : 64;
            if (lane < first) {
                const float w = __fmul_rn(v[k], Q.qpp);
                const int q = w >= 32767.f ? 32767 : (w <= -32768.f ? -32768 : (int)rintf(w));
                qs[b0 + 64 * k + lane] = (int16_t)q;
                acc += q;
            }
            if (m) n = b0 + 64 * k + first, ended = true;
        }
    }
    const int Pn = wave_sum_i32(acc);   // P[n]
    __syncthreads();

    // ---- 1: length ----
    if ((int64_t)n < (int64_t)Q.start_win + Q.min_ad + Q.polya_win) {
        detect_write(A, r, lane, WDX_DETECT_SHORT, -1, -1, n, -1, -1, -1, nan_out);
        return;
    }
    const int sw = Q.start_win, pw = Q.polya_win, tw = Q.step_win;

    // ---- 2: start ----
    int s = 0;
    if (Q.find_start) {
        const int m = min(Q.max_start, n - sw);
        const int lim = Q.thr1 * sw;   // |thr1| <= 2^15, sw <= 2^8
        s = -1;
        for (int b0 = 0; b0 <= m; b0 += 64) {
            const int i = b0 + lane;
            bool hit = false;
            if (i <= m && (int)qs[i] < Q.thr1) {
                int w = 0;
                for (int t = 0; t < sw; ++t) w += qs[i + t];   // i + t <= m + sw - 1 < n
                hit = w < lim;
            }
            const unsigned long long mk = __ballot(hit);
            if (mk) {
                s = b0 + __builtin_ctzll(mk);
                break;
            }
        }
        if (s < 0) {
            detect_write(A, r, lane, WDX_DETECT_NO_START, -1, -1, n, -1, -1, -1, nan_out);
            return;
        }
    }

    // ---- 3: coarse adapter end ----
    const int lo = s + Q.min_ad;   // (min_ad < n here)
    const int64_t hi64 = (int64_t)s + Q.max_ad;
    const int hi = (int)(hi64 < (int64_t)(n - pw) ? hi64 : (int64_t)(n - pw));
    if (lo > hi) {
        detect_write(A, r, lane, WDX_DETECT_NO_ROOM, s, -1, n, -1, -1, -1, nan_out);
        return;
    }
    const int Ps = range_sum(qs, 0, s, lane);
    const int Rs = Pn - Ps;   // P[n] - P[s]
    int c;
    double gain;
    {
        const int seg = run_length(hi - lo + 1);
        const int i0 = lo + lane * seg, i1 = min(i0 + seg, hi + 1);
        int run = 0;
        for (int i = i0; i < i1; ++i) run += qs[i];
        int L = range_sum(qs, s, lo, lane) + wave_excl_scan_i32(run);   // P[i0] - P[s]
        double best = -1.0;   // (g >= 0)
        int bi = INT_MAX;
        for (int i = i0; i < i1; ++i) {
            const double dl = (double)L, dr = (double)(Rs - L);
            const double g = __dadd_rn(__ddiv_rn(__dmul_rn(dl, dl), (double)(i - s)), __ddiv_rn(__dmul_rn(dr, dr), (double)(n - i)));
            if (g > best) best = g, bi = i;
            L += qs[i];
        }
#pragma unroll
        for (int d = 32; d; d >>= 1) {
            const double og = __shfl_xor(best, d);
            const int oi = __shfl_xor(bi, d);
            if (og > best || (og == best && oi < bi)) best = og, bi = oi;
        }
        c = bi, gain = best;
    }

    // ---- 4: refinement ----
    const int jlo = max(lo, c - Q.refine), jhi = min(hi, c + Q.refine);
    const int seg = run_length(jhi - jlo + 1);
    const int j0 = jlo + lane * seg, j1 = min(j0 + seg, jhi + 1);
    int run = 0;
    for (int j = j0; j < j1; ++j) run += qs[j];
    int A1 = range_sum(qs, s, jlo, lane) + wave_excl_scan_i32(run);   // P[j0] - P[s]
    int bD = 0, bj = INT_MAX, bA1 = -1, bS1 = -1;
    if (j0 < j1) {
        int S1 = 0, D = 0;
        long long S2 = 0;
        for (int t = 0; t < pw; ++t) {
            const int x = qs[j0 + t];
            S1 += x;
            S2 += x * x;   // (at most 2^30)
        }
        for (int t = 0; t < tw; ++t) D += (int)qs[j0 + t] - (int)qs[j0 - tw + t];   // j0 - tw >= lo - tw >= s
        const long long var_lim = Q.var_q * pw * pw, shift_pw = (long long)Q.shift_q * pw;
        for (int j = j0; j < j1; ++j) {
            const long long la = j - s;
            const bool flat = (long long)pw * S2 - (long long)S1 * S1 <= var_lim;
            const bool up = (long long)S1 * la - (long long)A1 * pw >= shift_pw * la;
            if (flat && up && (bj == INT_MAX || D > bD)) bD = D, bj = j, bA1 = A1, bS1 = S1;
            if (j + 1 < j1) {   // (j + pw <= jhi - 1 + pw < n)
                const int x = qs[j], xp = qs[j + pw];
                S1 += xp - x;
                S2 += (long long)(xp * xp) - (long long)(x * x);
                D += (int)qs[j + tw] - 2 * x + (int)qs[j - tw];
                A1 += x;
            }
        }
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const int oD = __shfl_xor(bD, d), oj = __shfl_xor(bj, d), oA = __shfl_xor(bA1, d), oS = __shfl_xor(bS1, d);
        if (oj != INT_MAX && (bj == INT_MAX || oD > bD || (oD == bD && oj < bj))) bD = oD, bj = oj, bA1 = oA, bS1 = oS;
    }
    if (bj == INT_MAX) {
        detect_write(A, r, lane, WDX_DETECT_NO_POLYA, s, -1, n, c, -1, -1, gain);
        return;
    }
    detect_write(A, r, lane, WDX_DETECT_OK, s, bj, n, c, bA1, bS1, gain);
}

// With the context's mutex held.  No workspace of the context is used: nothing waits for another stream.
int detect_launch(wdx_ctx *ctx, const DetectPlan &P, DetectArgs A, int64_t n_reads, hipStream_t s) {
    if (n_reads == 0) return WDX_SUCCESS;
    if (n_reads > INT32_MAX) {
        set_error("detect: %lld reads are too many for one launch", (long long)n_reads);
        return WDX_ERR_UNSUPPORTED;
    }
    A.q = P.q;
    Timed timed(ctx, WDX_K_DETECT, s);
    if (A.adc)
        hipLaunchKernelGGL(detect_kernel<true>, dim3((unsigned)n_reads), dim3(64), (size_t)P.lds_bytes, s, A);
    else
        hipLaunchKernelGGL(detect_kernel<false>, dim3((unsigned)n_reads), dim3(64), (size_t)P.lds_bytes, s, A);
    WDX_HIP_TRY(hipGetLastError());
    return WDX_SUCCESS;
}

int detect_refusal(const DetectPlan &P) {
    if (P.rc != WDX_SUCCESS) set_error("%s", P.msg);
    return P.rc;
}

struct DetectBlock {   // device memory of one host-buffer call
    void *p = nullptr;
    ~DetectBlock() {
        if (p) (void)hipFree(p);
    }
};

// the outputs of a host-buffer call in one device block: where each lies
struct DetectOutLayout {
    size_t gain, info, a_start, a_end, code, ok, bytes;
    explicit DetectOutLayout(size_t n) {
        gain = 0, info = gain + 8 * n, a_start = info + 16 * n, a_end = a_start + 4 * n, code = a_end + 4 * n, ok = code + 4 * n;
        bytes = ok + n;
    }
};

// Host-buffer forms: `A` holds the DEVICE inputs; the outputs go through one device block.  With the mutex held.
int detect_host(wdx_ctx *ctx, const DetectPlan &P, DetectArgs A, int64_t n_reads, int32_t *a_start, int32_t *a_end, uint8_t *ok,
                int32_t *code, int32_t *info, double *gain, hipStream_t s) {
    const size_t n = (size_t)n_reads;
    const DetectOutLayout lay(n);
    DetectBlock out;
    WDX_HIP_TRY(hipMalloc(&out.p, lay.bytes));
    uint8_t *const o = (uint8_t *)out.p;
    A.gain = gain ? (double *)(o + lay.gain) : nullptr, A.info = info ? (int32_t *)(o + lay.info) : nullptr;
    A.a_start = a_start ? (int32_t *)(o + lay.a_start) : nullptr, A.a_end = a_end ? (int32_t *)(o + lay.a_end) : nullptr;
    A.code = (int32_t *)(o + lay.code), A.ok = ok ? o + lay.ok : nullptr;
    StreamDrain drain(s);
    if (int rc = detect_launch(ctx, P, A, n_reads, s)) return rc;
    if (gain) WDX_HIP_TRY(hipMemcpyAsync(gain, A.gain, 8 * n, hipMemcpyDeviceToHost, s));
    if (info) WDX_HIP_TRY(hipMemcpyAsync(info, A.info, 16 * n, hipMemcpyDeviceToHost, s));
    if (a_start) WDX_HIP_TRY(hipMemcpyAsync(a_start, A.a_start, 4 * n, hipMemcpyDeviceToHost, s));
    if (a_end) WDX_HIP_TRY(hipMemcpyAsync(a_end, A.a_end, 4 * n, hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipMemcpyAsync(code, A.code, 4 * n, hipMemcpyDeviceToHost, s));
    if (ok) WDX_HIP_TRY(hipMemcpyAsync(ok, A.ok, n, hipMemcpyDeviceToHost, s));
    WDX_HIP_TRY(hipStreamSynchronize(s));
    drain.done();
    return WDX_SUCCESS;
}

int detect_bad_arguments(const char *who) {
    set_error("%s: bad arguments", who);
    return WDX_ERR_INVALID;
}

}  // namespace

}  // namespace wdx

using namespace wdx;

extern "C" {

int wdx_detect_rows(wdx_ctx *ctx, const float *d_sig, const int64_t *d_row_off, const int32_t *d_row_len, int64_t stride,
                    int64_t n_reads, const wdx_detect_params *params, int32_t *d_a_start, int32_t *d_a_end, uint8_t *d_ok,
                    int32_t *d_code, int32_t *d_info, double *d_gain, void *stream) {
    WDX_ENTER(ctx);
    const DetectPlan P = detect_plan(params);
    if ((rc = detect_refusal(P))) return rc;
    if (n_reads < 0 || (!d_row_off && stride < 0) || (n_reads > 0 && (!d_sig || !d_code))) return detect_bad_arguments("detect_rows");
    std::lock_guard<std::mutex> g(ctx->mu);
    DetectArgs A{};
    A.sig = d_sig, A.row_off = d_row_off, A.row_len = d_row_len, A.stride = stride;
    A.a_start = d_a_start, A.a_end = d_a_end, A.ok = d_ok, A.code = d_code, A.info = d_info, A.gain = d_gain;
    return detect_launch(ctx, P, A, n_reads, (hipStream_t)stream);
}

int wdx_detect_rows_adc(wdx_ctx *ctx, const wdx_adc_dev_in *in, int64_t n_reads, const wdx_detect_params *params,
                        int32_t *d_a_start, int32_t *d_a_end, uint8_t *d_ok, int32_t *d_code, int32_t *d_info, double *d_gain,
                        void *stream) {
    WDX_ENTER(ctx);
    const DetectPlan P = detect_plan(params);
    if ((rc = detect_refusal(P))) return rc;
    if ((rc = adc_dev_in_ok("detect_rows_adc", in))) return rc;
    if (n_reads < 0 || (n_reads > 0 && (!in->adc || !in->row_len || !in->offset || !in->scale || !d_code)))
        return detect_bad_arguments("detect_rows_adc");
    std::lock_guard<std::mutex> g(ctx->mu);
    DetectArgs A{};
    A.adc = in->adc, A.offset = in->offset, A.scale = in->scale, A.row_off = in->row_off, A.row_len = in->row_len, A.stride = in->stride;
    A.a_start = d_a_start, A.a_end = d_a_end, A.ok = d_ok, A.code = d_code, A.info = d_info, A.gain = d_gain;
    return detect_launch(ctx, P, A, n_reads, (hipStream_t)stream);
}

int wdx_detect_batch(wdx_ctx *ctx, const float *sig, int64_t n_reads, int64_t stride, const int32_t *row_len,
                     const wdx_detect_params *params, int32_t *a_start, int32_t *a_end, uint8_t *ok, int32_t *code, int32_t *info,
                     double *gain) {
    WDX_ENTER(ctx);
    const DetectPlan P = detect_plan(params);
    if ((rc = detect_refusal(P))) return rc;
    if (n_reads < 0 || stride < 0 || (n_reads > 0 && (!code || (stride > 0 && !sig)))) return detect_bad_arguments("detect_batch");
    if (n_reads == 0) return WDX_SUCCESS;
    std::lock_guard<std::mutex> g(ctx->mu);
    hipStream_t s = ctx->stream;
    DetectBlock Ds, Dl;
    const size_t sb = sizeof(float) * (size_t)n_reads * (size_t)stride, lb = sizeof(int32_t) * (size_t)n_reads;
    WDX_HIP_TRY(hipMalloc(&Ds.p, sb ? sb : 4));
    if (row_len) WDX_HIP_TRY(hipMalloc(&Dl.p, lb));
    StreamDrain drain(s);   // (declared behind the blocks: the stream is drained before they are freed)
    if (sb) WDX_HIP_TRY(hipMemcpyAsync(Ds.p, sig, sb, hipMemcpyHostToDevice, s));
    if (row_len) WDX_HIP_TRY(hipMemcpyAsync(Dl.p, row_len, lb, hipMemcpyHostToDevice, s));
    DetectArgs A{};
    A.sig = (const float *)Ds.p, A.row_len = (const int32_t *)Dl.p, A.stride = stride;
    rc = detect_host(ctx, P, A, n_reads, a_start, a_end, ok, code, info, gain, s);
    if (rc == WDX_SUCCESS) drain.done();
    return rc;
}

int wdx_detect_batch_adc(wdx_ctx *ctx, const int16_t *adc, int64_t n_reads, int64_t stride, const int32_t *row_len,
                         const float *offset, const float *scale, const wdx_detect_params *params, int32_t *a_start,
                         int32_t *a_end, uint8_t *ok, int32_t *code, int32_t *info, double *gain) {
    WDX_ENTER(ctx);
    const DetectPlan P = detect_plan(params);
    if ((rc = detect_refusal(P))) return rc;
    if (n_reads < 0 || stride < 0 || (n_reads > 0 && (!code || !row_len || !offset || !scale || (stride > 0 && !adc))))
        return detect_bad_arguments("detect_batch_adc");
    if (n_reads == 0) return WDX_SUCCESS;
    std::lock_guard<std::mutex> g(ctx->mu);
    hipStream_t s = ctx->stream;
    DetectBlock Ds, Dt;   // the samples; row_len | offset | scale
    const size_t sb = sizeof(int16_t) * (size_t)n_reads * (size_t)stride, tb = 4 * (size_t)n_reads;
    WDX_HIP_TRY(hipMalloc(&Ds.p, sb ? sb : 4));
    WDX_HIP_TRY(hipMalloc(&Dt.p, 3 * tb));
    uint8_t *const t = (uint8_t *)Dt.p;
    StreamDrain drain(s);
    if (sb) WDX_HIP_TRY(hipMemcpyAsync(Ds.p, adc, sb, hipMemcpyHostToDevice, s));
    WDX_HIP_TRY(hipMemcpyAsync(t, row_len, tb, hipMemcpyHostToDevice, s));
    WDX_HIP_TRY(hipMemcpyAsync(t + tb, offset, tb, hipMemcpyHostToDevice, s));
    WDX_HIP_TRY(hipMemcpyAsync(t + 2 * tb, scale, tb, hipMemcpyHostToDevice, s));
    DetectArgs A{};
    A.adc = (const int16_t *)Ds.p, A.row_len = (const int32_t *)t, A.offset = (const float *)(t + tb), A.scale = (const float *)(t + 2 * tb);
    A.stride = stride;
    rc = detect_host(ctx, P, A, n_reads, a_start, a_end, ok, code, info, gain, s);
    if (rc == WDX_SUCCESS) drain.done();
    return rc;
}

}  // extern "C"
